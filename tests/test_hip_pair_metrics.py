"""Paired image metrics on the GPU: la_pair_metrics_f32 and la_joint_hist_f32 through the C ABI, and their Python layer
(metrics.compute_pair_metrics, compute_msssim_diversity, compute_modality_mi, compute_pair_mi, compute_pair_metrics_for_aug_dataset),
against the float64 restatements of tests/pair_metric_cases.py.

Float outputs (ssim, cs per level, ms): |HIP - float64| <= 4 x the error of the restatement run in float32 on the CPU (the larger of
the separable and the dense order) + 2^-23, per case; test_pair_metric_cases_cpu.py shows that no such budget exceeds 1e-5.
Error sums: exact on integer inputs, within n 2^-53 sum|terms| on float inputs (n = H W float64 additions at most).
Histogram counts: equal.  Outputs are pre-filled with garbage before every C-ABI call.  Every case prints its error / budget ratio.

Largest measured ratio on an MI355X: 0.25 (64 x 96, 3 levels, background with a disc); the budgets run from 1.2e-7 to 8.9e-6 and
the whole file takes under 4 seconds."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_metric_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _dev_array(a, dev, offset=0):
    """device copy of a numpy array; offset > 0: the data start `offset` elements into a larger allocation (an unaligned base)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(dev)
    flat = torch.empty([t.numel() + offset], dtype=t.dtype, device=dev)
    flat[offset:] = t.flatten().to(dev)
    return flat[offset:].view(t.shape)


def run_abi(dev, x, y, win, levels, ix=None, iy=None, weights=None, offset=0, ws_bytes=None, sigma=1.5):
    """one la_pair_metrics_f32 call on numpy inputs -> (rc, {'err', 'ssim', 'cs', 'ms'} numpy, workspace tensor)"""
    from latentaugment_amd import _lib
    lib = _lib.load()
    Cn, H, W = x.shape[1:]
    P = x.shape[0] if ix is None else len(ix)
    xd, yd = _dev_array(x, dev, offset), _dev_array(y, dev, offset)
    ixd = None if ix is None else _dev_array(np.asarray(ix, np.int32), dev)
    iyd = None if iy is None else _dev_array(np.asarray(iy, np.int32), dev)
    taps = pc.window(win, sigma).astype(np.float32) if win in (1, 3, 5, 7, 9, 11) else np.zeros([11], np.float32)
    w = pc.weights_for(max(1, min(levels, 5)), weights)
    c1, c2 = pc.constants()
    need = lib.la_pair_metrics_workspace_bytes(P, Cn, H, W, win, levels)
    ws = torch.full([max(need, 8) // 8], -7.0, dtype=torch.float64, device=dev)
    lv = max(levels, 1)
    err = torch.full([P, Cn, 2], -7.0, dtype=torch.float64, device=dev)
    ssim, cs = (torch.full([P, Cn, lv], -7.0, dtype=torch.float32, device=dev) for _ in range(2))
    ms = torch.full([P, Cn], -7.0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.la_pair_metrics_f32(_lib.ptr(xd), _lib.ptr(yd), _lib.ptr(ixd), _lib.ptr(iyd), P, Cn, H, W, taps.ctypes.data, win, levels,
                                     w.ctypes.data, float(c1), float(c2), _lib.ptr(err), _lib.ptr(ssim), _lib.ptr(cs), _lib.ptr(ms),
                                     _lib.ptr(ws), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dict(err=err.cpu().numpy(), ssim=ssim.cpu().numpy(), cs=cs.cpu().numpy(), ms=ms.cpu().numpy()), ws


def check_floats(name, got, r64, bud):
    worst = 0.0
    for k in ('ssim', 'cs', 'ms'):
        assert got[k].dtype == np.float32 and got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert np.isfinite(got[k]).all()
        e = float(np.abs(got[k].astype(np.float64) - r64[k]).max())
        print(f'pair {name} {k}: err {e:.3e} / budget {bud[k]:.3e}  ratio {e / bud[k]:.3f}')
        worst = max(worst, e / bud[k])
    for k in ('ssim', 'cs', 'ms'):
        e = float(np.abs(got[k].astype(np.float64) - r64[k]).max())
        assert e <= bud[k], f'{name}: {k} off by {e:.3e} > budget {bud[k]:.3e}'
    return worst


def check_errors(name, got, x, y):
    want = pc.error_sums(x, y)
    n = x.shape[-1] * x.shape[-2]
    tol = n * 2.0 ** -53 * want          # the terms are non-negative: sum|terms| is the sum
    e = np.abs(got['err'] - want)
    print(f'pair {name} error sums: worst relative {float((e / np.maximum(want, 1e-300)).max()):.3e} (tolerance {n * 2.0 ** -53:.3e})')
    assert (e <= tol).all(), f'{name}: error sums off by {float(e.max()):.3e}'


def check_case(dev, case, **kw):
    H, W, levels, win, Cn, P, kind = case
    x, y, r64, bud, _ = pc.case_reference(case)
    rc, got, _ = run_abi(dev, x, y, win, levels, **kw)
    assert rc == 0
    check_floats(pc.case_id(case), got, r64, bud)
    check_errors(pc.case_id(case), got, x, y)
    return got


@pytest.mark.parametrize('case', [(H, W, 1, win, Cn, P, kind) for H, W, win, Cn, P, kind in pc.SINGLE], ids=pc.case_id)
def test_single_level(dev, case):
    got = check_case(dev, case)
    assert (got['ms'] == np.maximum(got['ssim'][..., 0], 0)).all()          # levels = 1 is plain SSIM


@pytest.mark.parametrize('case', pc.MULTI, ids=pc.case_id)
def test_multi_level(dev, case):
    got = check_case(dev, case)
    x, y = pc.case_reference(case)[:2]
    _, again, _ = run_abi(dev, x, y, case[3], case[2])
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), f'{k}: two calls differ'


@pytest.mark.parametrize('case', pc.SPECIAL, ids=pc.case_id)
def test_special_inputs(dev, case):
    got = check_case(dev, case)
    kind = case[-1]
    if kind == 'negated':
        assert (got['cs'][..., 0] < 0).all()
        assert (got['ms'] == 0.0).all() and np.isfinite(got['ms']).all()          # exactly 0, never NaN
    if kind == 'identical':
        assert (got['err'] == 0.0).all()
        np.testing.assert_allclose(got['ssim'], 1.0, rtol=0, atol=2.0 ** -23)
    if kind == 'constant':
        assert (got['err'][..., 0] == 0.375 ** 2 * 64 * 96).all() and (got['err'][..., 1] == 0.375 * 64 * 96).all()


def test_base_pointer_offset_by_one_float(dev):
    case = (43, 42, 1, 11, 2, 1, 'background')
    x, y, r64, bud, _ = pc.case_reference(case)
    _, aligned, _ = run_abi(dev, x, y, 11, 1)
    rc, shifted, _ = run_abi(dev, x, y, 11, 1, offset=1)
    assert rc == 0
    check_floats('offset 1', shifted, r64, bud)
    for k in aligned:
        assert aligned[k].tobytes() == shifted[k].tobytes(), k
    case = (48, 80, 3, 3, 1, 3, 'texture')
    x, y, r64, bud, _ = pc.case_reference(case)
    rc, shifted, _ = run_abi(dev, x, y, 3, 3, offset=1)
    assert rc == 0
    check_floats('offset 1, 3 levels', shifted, r64, bud)
    check_errors('offset 1, 3 levels', shifted, x, y)


@pytest.mark.parametrize('levels,win,H,W', [(1, 7, 33, 34), (3, 3, 48, 80)])
def test_gathered_pairs_equal_the_contiguous_call(dev, levels, win, H, W):
    x, y = pc.images('texture', 5, 2, H, W, seed=9)
    for ix, iy in (([3, 0, 4, 1, 2], [1, 2, 0, 4, 3]), ([2, 2, 0, 2, 4, 4, 1], [0, 3, 3, 3, 0, 1, 1])):
        rc, got, _ = run_abi(dev, x, y, win, levels, ix=ix, iy=iy)
        assert rc == 0
        _, want, _ = run_abi(dev, x[ix], y[iy], win, levels)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
        rc, half, _ = run_abi(dev, x, y[iy], win, levels, ix=ix)          # one side gathered, the other in place
        assert rc == 0 and all(half[k].tobytes() == want[k].tobytes() for k in want)
    r64, bud, _ = pc.pair_budgets(x[ix], y[iy], win, levels)
    check_floats(f'gathered {levels} levels', got, r64, bud)


def test_more_planes_than_a_grid_axis(dev):
    P = 65600
    x, y = pc.images('texture', P, 1, 11, 11, seed=4)
    r64, bud, _ = pc.pair_budgets(x, y, 11, 1)
    rc, got, _ = run_abi(dev, x, y, 11, 1)
    assert rc == 0
    check_floats(f'{P} planes', got, r64, bud)
    check_errors(f'{P} planes', got, x, y)


def test_integer_inputs_give_the_exact_error_sums(dev):
    x, y = pc.integer_images(3, 2, 74, 75, seed=2)
    rc, got, _ = run_abi(dev, x, y, 11, 1)
    assert rc == 0
    d = x.astype(np.float64) - y.astype(np.float64)
    assert (got['err'][..., 0] == (d * d).sum(axis=(-2, -1))).all() and (got['err'][..., 1] == np.abs(d).sum(axis=(-2, -1))).all()
    x, y = pc.integer_images(1, 1, 192, 176, seed=3)
    rc, got, _ = run_abi(dev, x, y, 11, 5)
    d = x.astype(np.float64) - y.astype(np.float64)
    assert rc == 0 and got['err'][0, 0].tolist() == [float((d * d).sum()), float(np.abs(d).sum())]


def test_refusals_launch_nothing_and_the_next_call_is_right(dev):
    from latentaugment_amd import _lib
    lib = _lib.load()
    case = (32, 32, 2, 11, 3, 1, 'texture')
    x, y, r64, bud, _ = pc.case_reference(case)
    need = lib.la_pair_metrics_workspace_bytes(1, 3, 32, 32, 11, 2)
    assert need > 0
    for kw, code in ((dict(win=2), -1), (dict(win=13), -1), (dict(levels=0), -1), (dict(levels=6), -1), (dict(levels=3), -1),
                     (dict(ws_bytes=need - 1), -3), (dict(ws_bytes=0), -3)):
        a = dict(dict(win=11, levels=2), **kw)
        rc, got, ws = run_abi(dev, x, y, a['win'], a['levels'], ws_bytes=a.get('ws_bytes', 1 << 20))
        assert rc == code and lib.la_last_error(), (kw, rc)
        assert all((v == -7.0).all() for v in got.values()) and (ws == -7.0).all(), f'{kw}: a refused call wrote'
    # H = 30: the last level is 15 x 16, which is allowed (nothing is halved again); H = 31 cannot be halved
    rc, got, _ = run_abi(dev, x[:, :, :30], y[:, :, :30], 11, 2)
    assert rc == 0 and la_ok(got)
    rc, got, _ = run_abi(dev, x[:, :, :31], y[:, :, :31], 11, 2)
    assert rc == -1 and all((v == -7.0).all() for v in got.values())
    rc, got, _ = run_abi(dev, x, y, 11, 2)
    assert rc == 0
    check_floats('after refusals', got, r64, bud)


def la_ok(got):
    return all(np.isfinite(v).all() and (v != -7.0).all() for v in got.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# joint histogram

def run_hist(dev, a, b, bins, lo=-1.0, hi=1.0, a_t=None, b_t=None, stride_a=None, stride_b=None):
    """a, b numpy [planes, npix] (uploaded contiguously) or device views a_t, b_t with plane strides -> counts int64"""
    from latentaugment_amd import _lib
    lib = _lib.load()
    planes, npix = a.shape
    if a_t is None:
        a_t, b_t, stride_a, stride_b = _dev_array(a, dev), _dev_array(b, dev), npix, npix
    hist = torch.full([planes, bins, bins], -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.la_joint_hist_f32(_lib.ptr(a_t), stride_a, _lib.ptr(b_t), stride_b, planes, npix, bins, lo, float(pc.hist_scale(bins, lo, hi)),
                                   _lib.ptr(hist), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return hist.cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize('npix', pc.HIST_NPIX)
@pytest.mark.parametrize('bins', pc.HIST_BINS)
def test_histogram_counts(dev, bins, npix):
    for kind in ('off_edges', 'edges', 'slice', 'constant'):
        a, b = pc.hist_values(kind, 3, npix, bins, seed=bins + npix)
        want = pc.joint_hist_restate(a, b, bins)
        got = run_hist(dev, a, b, bins)
        assert got.sum() == 3 * npix and (got == want).all(), f'{kind}: {int((got != want).sum())} cells differ'
        if kind == 'constant':
            assert (got[:, 0, 0] == npix).all()          # all of npix in one bin
        if kind == 'slice':
            assert (run_hist(dev, a, b, bins) == got).all()


def test_histogram_of_another_range(dev):
    a, b = pc.hist_values('off_edges', 2, 3000, 16, seed=1, lo=0.0, hi=255.0)
    assert (run_hist(dev, a, b, 16, lo=0.0, hi=255.0) == pc.joint_hist_restate(a, b, 16, lo=0.0, hi=255.0)).all()


@pytest.mark.parametrize('H,W', [(16, 16), (15, 15), (33, 62), (10, 10)])
def test_histogram_reads_channels_in_place(dev, H, W):
    """the two channels of one [N][2][H][W] tensor through the plane strides; at 15 x 15 no plane but the first is 16-byte aligned; at
    10 x 10 all are and the last thread holds a partial run"""
    N = 3
    a, b = pc.hist_values('slice', N, H * W, 64, seed=H)
    img = _dev_array(np.stack([a.reshape(N, H, W), b.reshape(N, H, W)], axis=1), dev)
    got = run_hist(dev, a, b, 64, a_t=img[:, 0], b_t=img[:, 1], stride_a=2 * H * W, stride_b=2 * H * W)
    assert (got == pc.joint_hist_restate(a, b, 64)).all()
    swapped = run_hist(dev, b, a, 64, a_t=img[:, 1], b_t=img[:, 0], stride_a=2 * H * W, stride_b=2 * H * W)
    assert (swapped == got.transpose(0, 2, 1)).all()


def test_histogram_more_planes_than_a_grid_axis(dev):
    a, b = pc.hist_values('edges', 70000, 4, 2, seed=5)
    got = run_hist(dev, a, b, 2)
    assert (got == pc.joint_hist_restate(a, b, 2)).all() and got.sum() == 70000 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python layer

def _check_python_pairs(name, out, x, y, win, levels, data_range=2.0, **kw):
    r64, bud, _ = pc.pair_budgets(x, y, win, levels, data_range=data_range, **kw)
    P, Cn = x.shape[:2]
    n = x.shape[-1] * x.shape[-2]
    e = pc.error_sums(x, y)
    for k, v in out.items():
        assert v.dtype == torch.float64 and v.device.type == 'cpu', k
    assert out['ssim_per_channel'].shape == out['ms_ssim_per_channel'].shape == out['mse_per_channel'].shape == (P, Cn)
    assert out['ssim'].shape == out['ms_ssim'].shape == out['mse'].shape == out['mae'].shape == out['psnr'].shape == (P,)
    assert out['ssim_levels'].shape == out['cs_levels'].shape == (P, Cn, levels)
    for k, ref, b in (('ssim_per_channel', r64['ssim'][..., 0], bud['ssim']), ('ms_ssim_per_channel', r64['ms'], bud['ms']),
                      ('ssim_levels', r64['ssim'], bud['ssim']), ('cs_levels', r64['cs'], bud['cs'])):
        err = float(np.abs(out[k].numpy() - ref).max())
        print(f'python {name} {k}: err {err:.3e} / budget {b:.3e}')
        assert err <= b, (k, err, b)
    assert np.abs(out['ssim'].numpy() - r64['ssim'][..., 0].mean(1)).max() <= bud['ssim'] + 1e-15
    assert np.abs(out['ms_ssim'].numpy() - r64['ms'].mean(1)).max() <= bud['ms'] + 1e-15
    tol = 2.0 ** -53 * (n + 4)
    np.testing.assert_allclose(out['mse_per_channel'].numpy(), e[..., 0] / n, rtol=tol, atol=0)
    np.testing.assert_allclose(out['mae_per_channel'].numpy(), e[..., 1] / n, rtol=tol, atol=0)
    np.testing.assert_allclose(out['mse'].numpy(), (e[..., 0] / n).mean(1), rtol=tol, atol=0)
    np.testing.assert_allclose(out['mae'].numpy(), (e[..., 1] / n).mean(1), rtol=tol, atol=0)
    with np.errstate(divide='ignore'):
        np.testing.assert_allclose(out['psnr'].numpy(), 10 * np.log10(data_range ** 2 / (e[..., 0] / n).mean(1)), rtol=1e-12)
        np.testing.assert_allclose(out['psnr_per_channel'].numpy(), 10 * np.log10(data_range ** 2 / (e[..., 0] / n)), rtol=1e-12)


def test_compute_pair_metrics(dev, monkeypatch):
    from latentaugment_amd import _lib, metrics
    x, y = pc.images('background', 5, 2, 64, 96, seed=21)
    y[3] = x[3]                                               # one identical pair: mse 0, psnr inf
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    out = metrics.compute_pair_metrics(xd, yd, levels=3)
    _check_python_pairs('defaults, 3 levels', out, x, y, 11, 3)
    assert out['psnr'][3] == float('inf') and out['mse'][3] == 0 and torch.isfinite(out['psnr'][:3]).all()
    # the pairs are chunked by the workspace bound: the same bits whatever the chunk
    monkeypatch.setattr(metrics, '_PAIR_WORKSPACE_BYTES', 2 * _lib.load().la_pair_metrics_workspace_bytes(1, 2, 64, 96, 11, 3))
    chunked = metrics.compute_pair_metrics(xd, yd, levels=3)
    assert all(torch.equal(out[k], chunked[k]) for k in out)
    ix, iy = np.array([4, 0, 0, 2, 1], np.int32), np.array([1, 1, 3, 0, 4], np.int32)
    g = metrics.compute_pair_metrics(xd, yd, pairs=(ix, iy), levels=3)
    monkeypatch.undo()
    g2 = metrics.compute_pair_metrics(xd[torch.from_numpy(ix).long().to(dev)], yd[torch.from_numpy(iy).long().to(dev)], levels=3)
    assert all(torch.equal(g[k], g2[k]) for k in g)
    # other parameters: window, sigma, weights, data range; a strided view is taken by value
    out = metrics.compute_pair_metrics(xd[:, :, ::2, 8:72], yd[:, :, ::2, 8:72], data_range=1.5, win_size=5, win_sigma=1.0, levels=2,
                                       weights=[0.3, 0.7])
    _check_python_pairs('win 5 sigma 1 range 1.5', out, x[:, :, ::2, 8:72], y[:, :, ::2, 8:72], 5, 2, data_range=1.5, sigma=1.0,
                        weights=[0.3, 0.7])
    for bad in (lambda: metrics.compute_pair_metrics(xd.double(), yd.double(), levels=1),
                lambda: metrics.compute_pair_metrics(xd.half(), yd.half(), levels=1), lambda: metrics.compute_pair_metrics(xd, y, levels=1)):
        with pytest.raises(_lib.LatentAugHipError):
            bad()
    with pytest.raises(ValueError, match='multiples'):
        metrics.compute_pair_metrics(xd, yd, levels=5)          # 64 x 96 at 5 levels ends at 4 x 6
    with pytest.raises(ValueError, match='outside'):
        metrics.compute_pair_metrics(xd, yd, pairs=([0, 5], [0, 1]), levels=1)


def test_msssim_diversity(dev):
    from latentaugment_amd import metrics
    x, _ = pc.images('smooth', 12, 2, 32, 48, seed=8)
    xd = torch.from_numpy(x).to(dev)
    out = metrics.compute_msssim_diversity(xd, num_pairs=20, seed=3, levels=2)
    pairs = pc.diversity_pairs(12, 20, 3)
    assert list(zip(out['ix'].tolist(), out['iy'].tolist())) == pairs and len(set(pairs)) == 20 and all(i != j for i, j in pairs)
    ix, iy = np.array(pairs).T
    r64, bud, _ = pc.pair_budgets(x[ix], x[iy], 11, 2)
    assert out['ms_ssim'].shape == (20,) and out['ms_ssim'].dtype == torch.float64
    assert np.abs(out['ms_ssim'].numpy() - r64['ms'].mean(1)).max() <= bud['ms'] + 1e-15
    assert out['mean'] == pytest.approx(float(r64['ms'].mean()), abs=bud['ms'] + 1e-15)
    assert metrics.compute_msssim_diversity(xd, num_pairs=20, seed=3, levels=2)['mean'] == out['mean']
    assert metrics.compute_msssim_diversity(xd, num_pairs=20, seed=4, levels=2)['ix'].tolist() != out['ix'].tolist()
    # a collapsed set: every pair identical
    same = metrics.compute_msssim_diversity(xd[:1].expand(6, -1, -1, -1), num_pairs=1000, levels=2)
    assert len(same['ix']) == 15 and same['mean'] == pytest.approx(1.0, abs=2.0 ** -23)
    assert same['mean'] > out['mean']


def test_modality_and_pair_mi(dev):
    from latentaugment_amd import metrics
    N, H, W = 4, 24, 40
    a, b = pc.hist_values('slice', N, H * W, 64, seed=12)
    b[3] = a[3]                                   # identical planes: NMI = 2
    a[2], b[2] = -1.0, -1.0                       # one bin: MI = 0 and NMI = 2 by definition
    img = np.stack([a.reshape(N, H, W), np.zeros([N, H, W], np.float32), b.reshape(N, H, W)], axis=1)
    imgd = torch.from_numpy(img).to(dev)
    for bins in (64, 16):
        out = metrics.compute_modality_mi(imgd, channels=(0, 2), bins=bins)
        want = pc.joint_hist_restate(a, b, bins)
        assert out['counts'].dtype == np.int64 and (out['counts'] == want).all()
        ref = np.array([pc.mi_restate(t) for t in want])
        np.testing.assert_allclose(out['mi'], ref[:, 0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(out['nmi'], ref[:, 1], rtol=0, atol=1e-12)
        assert out['nmi'][3] == pytest.approx(2.0, abs=1e-12) and out['mi'][2] == 0.0 and out['nmi'][2] == 2.0
        assert out['mi'][0] > 0.1
    other = np.ascontiguousarray(img[:, ::-1])
    out = metrics.compute_pair_mi(imgd, torch.from_numpy(other).to(dev), channel=0, bins=32, value_range=(-1.0, 1.0))
    assert (out['counts'] == pc.joint_hist_restate(a, b, 32)).all()
    np.testing.assert_allclose(out['mi'], [pc.mi_restate(t)[0] for t in out['counts']], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        metrics.compute_modality_mi(imgd, channels=(0, 3))
    with pytest.raises(ValueError):
        metrics.compute_modality_mi(imgd, bins=65)


class _Callable:
    def __reduce__(self):
        return (os.getcwd, ())


def test_aug_dataset_reader(dev, tmp_path):
    from latentaugment_amd import metrics
    run = tmp_path / 'run'
    os.makedirs(run / 'img')
    os.makedirs(run / 'img_aug')
    xs, ys = [], []
    for i, n in enumerate((2, 3)):          # as the reference's driver writes them: one dict of batches per file
        x, y = pc.images('background', n, 2, 32, 48, seed=30 + i)
        xs.append(x)
        ys.append(y)
        with open(run / 'img' / f'img_{i}', 'wb') as f:
            pickle.dump({'A': torch.from_numpy(x[:, :1].copy()), 'B': torch.from_numpy(x[:, 1:].copy()), 'A_paths': ['p'] * n}, f)
        with open(run / 'img_aug' / f'img_aug_{i}', 'wb') as f:
            pickle.dump({'A': y[:, :1].copy(), 'B': y[:, 1:].copy()}, f, protocol=pickle.HIGHEST_PROTOCOL)
    out = metrics.compute_pair_metrics_for_aug_dataset(str(run), levels=2)
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert out['num_items'] == 5
    means = {k: out.pop(k) for k in list(out) if k.endswith('_mean')}
    out.pop('num_items')
    _check_python_pairs('aug dataset', out, x, y, 11, 2)
    assert set(means) == {'mse_mean', 'mae_mean', 'psnr_mean', 'ssim_mean', 'ms_ssim_mean'}
    for k, v in means.items():
        assert isinstance(v, float) and v == float(out[k[:-5]].mean())
    with pytest.raises(FileNotFoundError):
        metrics.compute_pair_metrics_for_aug_dataset(str(tmp_path / 'nowhere'))
    os.makedirs(tmp_path / 'bad' / 'img')
    os.makedirs(tmp_path / 'bad' / 'img_aug')
    for sub, name in (('img', 'img_0'), ('img_aug', 'img_aug_0')):
        with open(tmp_path / 'bad' / sub / name, 'wb') as f:
            pickle.dump({'A': xs[0][:, :1], 'B': _Callable()}, f)
    with pytest.raises(pickle.UnpicklingError, match='allow-list'):
        metrics.compute_pair_metrics_for_aug_dataset(str(tmp_path / 'bad'), levels=2)
