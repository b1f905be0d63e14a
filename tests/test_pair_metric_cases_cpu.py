"""The paired image metrics without a GPU: that the restatements of tests/pair_metric_cases.py are right (two independent forms agree,
known identities hold, numpy / sklearn agree where they apply), that every float budget the GPU test will use is tight, and the host
side of la_pair_metrics_f32 / la_joint_hist_f32 (exported symbols, the workspace query, refusals before any launch).

Measured on the CPU before the bound below was written: over every case of the GPU test the worst float32 restatement error is
printed by test_budgets_are_tight; no budget may exceed 1e-5."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_metric_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in pc.all_float_cases() if c[0] * c[1] <= 80 * 80]


def _lib_loaded():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


@pytest.mark.parametrize('case', SMALL, ids=pc.case_id)
def test_separable_equals_dense_in_float64(case):
    H, W, levels, win, Cn, P, kind = case
    x, y = pc.case_reference(case)[:2]
    a = pc.pair_restate(x, y, win, levels, form='separable')
    b = pc.pair_restate(x, y, win, levels, form='dense')
    for k in ('ssim', 'cs', 'ms'):
        assert a[k].shape == b[k].shape == ((P, Cn, levels) if k != 'ms' else (P, Cn))
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-12)


def test_window_and_weights():
    g = pc.window(11)
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and (g == g[::-1]).all() and g.argmax() == 5
    assert g[5] / g[4] == pytest.approx(np.exp(1 / 4.5), rel=1e-14)
    assert pc.window(1).tolist() == [1.0]
    assert pc.weights_for(5).tolist() == np.float32(pc.MS_WEIGHTS).tolist()
    assert float(pc.weights_for(3).astype(np.float64).sum()) == pytest.approx(1.0, abs=1e-7)
    assert pc.weights_for(1).tolist() == [1.0]
    from latentaugment_amd import metrics
    for win in (1, 3, 5, 7, 9, 11):
        assert (metrics.gaussian_window(win, 1.5) == pc.window(win)).all()
    for lv in range(1, 6):
        assert (metrics.msssim_weights(lv) == pc.weights_for(lv)).all()
    assert (metrics.msssim_weights(2, [0.25, 0.75]) == np.float32([0.25, 0.75])).all()
    for bad in (0, 2, 13):
        with pytest.raises(ValueError):
            metrics.gaussian_window(bad)
    for lv, w in ((0, None), (6, None), (2, [1.0]), (2, [0.5, -0.5])):
        with pytest.raises(ValueError):
            metrics.msssim_weights(lv, w)


def test_identities():
    x, y = pc.images('texture', 2, 2, 40, 48, seed=1)
    same = pc.pair_restate(x, x, 11, 2)
    np.testing.assert_allclose(same['ssim'], 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(same['ms'], 1.0, rtol=0, atol=1e-12)
    a, b = pc.pair_restate(x, y, 11, 2), pc.pair_restate(y, x, 11, 2)
    for k in ('ssim', 'cs', 'ms'):
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-14)
    assert (a['ssim'] < 0.99).all() and (a['ssim'] <= a['cs'] + 1e-12).all()
    # y = x + d on a grid where the float32 difference is exact: mse = d^2, mae = d
    xq = np.round(x * 64) / 64 * 0.5
    e = pc.error_sums(xq, (xq + 0.25).astype(np.float32))
    assert (e[..., 0] == 0.0625 * 40 * 48).all() and (e[..., 1] == 0.25 * 40 * 48).all()
    # a negative contrast term gives exactly 0, never NaN
    neg = pc.pair_restate(x, -x, 11, 2)
    assert (neg['cs'][..., 0] < 0).all() and (neg['ms'] == 0.0).all()
    # levels = 1 is plain SSIM
    one = pc.pair_restate(x, y, 11, 1)
    np.testing.assert_allclose(one['ms'], one['ssim'][..., 0], rtol=1e-15)
    # the pyramid is the 2 x 2 mean
    assert pc.pool2(np.arange(16, dtype=np.float64).reshape(4, 4)).tolist() == [[2.5, 4.5], [10.5, 12.5]]


@pytest.mark.parametrize('case', pc.all_float_cases(), ids=pc.case_id)
def test_budgets_are_tight(case):
    """the yardstick of the GPU test, per case: the larger of the two float32 orders; none may exceed 1e-5"""
    x, y, r64, bud, (sep, den) = pc.case_reference(case)
    for k in ('ssim', 'cs', 'ms'):
        es, ed = float(np.abs(sep[k] - r64[k]).max()), float(np.abs(den[k] - r64[k]).max())
        print(f'{pc.case_id(case)} {k}: float32 error separable {es:.3e} dense {ed:.3e} budget {bud[k]:.3e}')
        assert bud[k] == 4.0 * max(es, ed) + 2.0 ** -23
        assert bud[k] <= 1e-5
        assert np.isfinite(r64[k]).all()


@pytest.mark.parametrize('bins', pc.HIST_BINS)
def test_histogram_restatement_equals_numpy_off_the_edges(bins):
    a, b = pc.hist_values('off_edges', 3, 5000, bins, seed=bins)
    got = pc.joint_hist_restate(a, b, bins)
    for p in range(3):
        want, _, _ = np.histogram2d(a[p].astype(np.float64), b[p].astype(np.float64), bins=bins, range=[[-1, 1], [-1, 1]])
        assert (got[p] == want.astype(np.int64)).all()
    assert got.sum() == 3 * 5000


def test_bin_rule_on_the_edges_op_by_op():
    for bins in pc.HIST_BINS:
        s = pc.hist_scale(bins, -1.0, 1.0)
        assert s.dtype == np.float32 and float(s) == bins / 2.0
        a, _ = pc.hist_values('edges', 1, 4000, bins, seed=3)
        got = pc.bin_rule(a[0], -1.0, s, bins)
        for v, k in zip(a[0][:500], got[:500]):
            t = np.float32(np.float32(v) - np.float32(-1.0)) * s          # one float32 subtraction, one float32 product
            want = bins - 1 if t >= bins else (0 if t < 0 else int(np.floor(t)))
            assert k == want, (bins, v, k, want)
        assert got.min() == 0 and got.max() == bins - 1
    # an edge belongs to the bin it opens; hi itself and everything beyond falls in the last bin, everything below lo in the first
    assert pc.bin_rule(np.float32([-1.0, 0.0, 1.0, 7.0, -7.0]), -1.0, pc.hist_scale(16, -1, 1), 16).tolist() == [0, 8, 15, 15, 0]


def test_mutual_information_restatement():
    from latentaugment_amd import metrics
    rs = np.random.RandomState(0)
    tables = [rs.randint(0, 50, [8, 8]), np.diag(rs.randint(1, 9, [6])), np.outer([1, 2, 3], [4, 5, 6, 7])[:3, :3], np.eye(64, dtype=int),
              np.pad(np.array([[7]]), (0, 3))]
    for t in tables:
        mi, nmi = pc.mi_restate(t)
        c = np.asarray(t, np.float64)
        p, pa, pb = c / c.sum(), c.sum(1) / c.sum(), c.sum(0) / c.sum()
        ent = lambda q: float(-(q[q > 0] * np.log(q[q > 0])).sum())      # noqa: E731
        assert mi == pytest.approx(ent(pa) + ent(pb) - ent(p), abs=1e-12)          # MI = H_a + H_b - H_ab
        gm, gn = metrics.mi_from_counts(t)
        assert float(gm) == pytest.approx(mi, abs=1e-12) and float(gn) == pytest.approx(nmi, abs=1e-12)
        try:
            from sklearn.metrics import mutual_info_score
        except ImportError:
            continue
        assert mi == pytest.approx(mutual_info_score(None, None, contingency=np.asarray(t)), abs=1e-12)
    assert pc.mi_restate(np.diag([3, 3]))[1] == pytest.approx(2.0)          # identical images: NMI = 2
    assert pc.mi_restate(tables[-1]) == (0.0, 2.0)                          # one bin: H_ab = 0
    assert pc.mi_restate(np.outer([1, 2], [3, 4]))[0] == pytest.approx(0.0, abs=1e-15)      # independent
    mi, nmi = metrics.mi_from_counts(np.stack([np.diag([3, 3]), np.pad(np.array([[7]]), (0, 1))]))
    assert mi.shape == nmi.shape == (2,) and mi[1] == 0.0 and nmi[1] == 2.0 and nmi[0] == pytest.approx(2.0)


def test_diversity_pairs_rule():
    from latentaugment_amd import metrics
    for n, m, seed in ((2, 1000, 0), (5, 10, 0), (5, 9, 3), (40, 100, 1), (1000, 64, 7)):
        ix, iy = metrics.msssim_diversity_pairs(n, m, seed)
        want = pc.diversity_pairs(n, m, seed)
        assert ix.dtype == iy.dtype == np.int32 and len(ix) == min(m, n * (n - 1) // 2)
        assert list(zip(ix.tolist(), iy.tolist())) == want
        assert (ix < iy).all() and iy.max() < n and len(set(want)) == len(want)
    assert metrics.msssim_diversity_pairs(40, 100, 1)[0].tolist() != metrics.msssim_diversity_pairs(40, 100, 2)[0].tolist()
    with pytest.raises(ValueError):
        metrics.msssim_diversity_pairs(1, 10, 0)


def test_cpu_and_wrong_inputs_are_refused():
    from latentaugment_amd import _lib, metrics
    x = torch.zeros([2, 2, 16, 16])
    for call in (lambda: metrics.compute_pair_metrics(x, x, levels=1), lambda: metrics.compute_msssim_diversity(x, levels=1),
                 lambda: metrics.compute_modality_mi(x), lambda: metrics.compute_pair_mi(x, x),
                 lambda: metrics.compute_pair_metrics(x.numpy(), x.numpy(), levels=1)):
        with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
            call()
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_pair_metrics_for_aug_dataset('/nonexistent', device='cpu')


def test_symbols_declared_and_exported():
    _lib, lib = _lib_loaded()
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    for name in ('la_pair_metrics_workspace_bytes', 'la_pair_metrics_f32', 'la_joint_hist_f32'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in include/latentaug_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by the library'
    P, I, L, F = C.c_void_p, C.c_int, C.c_long, C.c_float
    assert _lib.SIGNATURES['la_pair_metrics_workspace_bytes'] == (C.c_size_t, [L, I, I, I, I, I])
    assert _lib.SIGNATURES['la_pair_metrics_f32'] == (I, [P, P, P, P, L, I, I, I, P, I, I, P, F, F, P, P, P, P, P, C.c_size_t, P])
    assert _lib.SIGNATURES['la_joint_hist_f32'] == (I, [P, L, P, L, L, L, I, F, F, P, P])
    assert lib.la_abi_version() == 1


REFUSED_SHAPES = [(0, 1, 16, 16, 11, 1), (1, 0, 16, 16, 11, 1), (1, 1, 0, 16, 1, 1), (1, 1, 16, 16, 0, 1), (1, 1, 16, 16, 2, 1),
                  (1, 1, 16, 16, 13, 1), (1, 1, 16, 16, -1, 1), (1, 1, 16, 16, 3, 0), (1, 1, 16, 16, 3, 6), (1, 1, 10, 16, 11, 1),
                  (1, 1, 16, 10, 11, 1), (1, 1, 18, 16, 3, 3), (1, 1, 16, 18, 3, 3), (1, 1, 16, 16, 11, 2), (1, 1, 160, 160, 11, 5),
                  (1, 1, 65536, 65536, 11, 1), (1 << 31, 2, 16, 16, 3, 1)]


def test_workspace_query():
    _, lib = _lib_loaded()
    ws = lib.la_pair_metrics_workspace_bytes
    for shape in REFUSED_SHAPES:
        assert ws(*shape) == 0, shape
    for shape in ((1, 1, 11, 11, 11, 1), (1, 3, 8, 8, 1, 1), (2, 2, 176, 176, 11, 5), (1, 1, 16, 16, 3, 3)):
        assert ws(*shape) > 0, shape
    prev = 0
    for P in (1, 2, 3, 8, 100, 70000):
        cur = ws(P, 2, 256, 256, 11, 5)
        assert cur > prev
        prev = cur
    sizes = [ws(P, 1, 11, 11, 11, 1) for P in range(1, 40)]          # small shapes: buffers are rounded up to 64 bytes, never shrinking
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # tile partials and the pyramid (1/4 + 1/16 + .. of both images): well under the images themselves
    assert ws(8, 2, 256, 256, 11, 5) < 8 * 2 * 256 * 256 * 4 * 2 * 0.4


def test_refusals_come_before_any_launch():
    """Pure host code (so this runs without a device: nothing reaches the HIP runtime): each refused call returns its code and sets
    la_last_error."""
    _, lib = _lib_loaded()
    p = 4096          # a non-null, aligned address: every call below is refused before it is looked at
    taps = (C.c_float * 11)(*pc.window(11).astype(np.float32))
    wts = (C.c_float * 5)(*pc.weights_for(5))
    ok = dict(x=p, y=p, ix=None, iy=None, P=1, C=1, H=176, W=176, taps=taps, win=11, levels=5, w=wts, err=p, ssim=p, cs=p, ms=p, ws=p,
              ws_bytes=1 << 30)

    def call(**change):
        a = dict(ok, **change)
        return lib.la_pair_metrics_f32(a['x'], a['y'], a['ix'], a['iy'], a['P'], a['C'], a['H'], a['W'], a['taps'], a['win'], a['levels'],
                                       a['w'], 0.0004, 0.0036, a['err'], a['ssim'], a['cs'], a['ms'], a['ws'], a['ws_bytes'], None)
    need = lib.la_pair_metrics_workspace_bytes(1, 1, 176, 176, 11, 5)
    for change, code, word in ((dict(x=None), -1, 'null'), (dict(ms=None), -1, 'null'), (dict(ws=None), -1, 'null'), (dict(taps=None), -1, 'null'),
                               (dict(win=2), -1, 'win'), (dict(win=13), -1, 'win'), (dict(win=0), -1, 'win'), (dict(levels=0), -1, 'levels'),
                               (dict(levels=6), -1, 'levels'), (dict(P=0), -1, 'positive'), (dict(C=0), -1, 'positive'),
                               (dict(H=168), -1, 'multiples'), (dict(W=184), -1, 'multiples'), (dict(H=160), -1, 'smaller than the window'),
                               (dict(W=16, levels=2), -1, 'smaller than the window'), (dict(ws_bytes=need - 1), -3, 'workspace'),
                               (dict(ws_bytes=0), -3, 'workspace'), (dict(ws=p + 4), -1, 'aligned'), (dict(x=p + 2), -1, 'aligned'),
                               (dict(w=(C.c_float * 5)(0.2, -0.1, 0.3, 0.3, 0.3)), -1, 'non-negative')):
        rc = call(**change)
        assert rc == code, (change, rc)
        assert word in lib.la_last_error().decode(), (change, lib.la_last_error())
    okh = dict(a=p, sa=64, b=p, sb=64, planes=2, npix=64, bins=16, lo=-1.0, scale=8.0, hist=p)
    for change, word in ((dict(a=None), 'null'), (dict(hist=None), 'null'), (dict(bins=0), 'bins'), (dict(bins=65), 'bins'),
                         (dict(planes=0), 'positive'), (dict(npix=0), 'positive'), (dict(sa=-1), 'stride'), (dict(scale=0.0), 'scale'),
                         (dict(scale=float('nan')), 'scale'), (dict(b=p + 1), 'aligned'), (dict(npix=1 << 33), 'uint32')):
        a = dict(okh, **change)
        rc = lib.la_joint_hist_f32(a['a'], a['sa'], a['b'], a['sb'], a['planes'], a['npix'], a['bins'], a['lo'], a['scale'], a['hist'], None)
        assert rc == -1, (change, rc)
        assert word in lib.la_last_error().decode(), (change, lib.la_last_error())
