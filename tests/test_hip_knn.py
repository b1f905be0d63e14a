"""The per-sample neighbour queries on the GPU: la_knn_f32 / la_realism_f32 at the C ABI and metrics.knn_from_features,
compute_realism_from_features, compute_authenticity_from_features, against the restatements of tests/knn_cases.py.

EXACT: integer inputs in -3 .. 3 (every sum exact in any order): dist2 and idx equal the restatement bit for bit -- full of exact ties,
so this is the test of the (d2, index) order; position independence; two runs; a captured graph.
BOUNDED: float inputs: every dist2 within B(q, x) = (2 D + 4) 2^-53 (|q|^2 + |x|^2) of the restatement (derived in knn_cases.py, not
measured) and EVERY index equal -- test_knn_cases_cpu.py shows the compared neighbours are more than 1000 x 2B apart.  The realism
quotient radius2 / d2: relative error at most b / (1 - b) with b = B / d2, and one rounding of the quotient.
Every bounded case prints its figures.  Nothing here is larger than 5000 rows; the file takes a few seconds.

Largest measured on an MI355X: d2 error 0.17 of B (127 x 200, D = 4), realism quotient 0.16 of its bound (same case), no index or
arg differing in any case; a float copy of a bank row at d2 = 0 exactly.  Wall time of the file: 4 s for 117 tests.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as kc  # noqa: E402
import helpers_script_detector as hsd  # noqa: E402
from guarded_alloc import Guarded, guarded_tensor  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _p(t):
    from latentaugment_amd import _lib
    return _lib.ptr(t)


def _s():
    from latentaugment_amd import _lib
    return _lib.stream_ptr()


def _dev32(a, dev, offset=False):
    """a float32 device copy; offset: it starts one float past the start of its allocation"""
    a = np.array(a, np.float32)          # (a copy: the shared inputs are read-only)
    if not offset:
        return torch.from_numpy(a).to(dev)
    buf = torch.empty([a.size + 1], dtype=torch.float32, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def _knn(lib, dev, q, x, k, exclude_self=False, offset=False):
    """la_knn_f32 -> (dist2 [nq][k] float64, idx [nq][k] int64) as numpy; outputs and scratch between guard bands"""
    qd, xd = _dev32(q, dev, offset), _dev32(x, dev, offset)
    nq, nx, D = qd.shape[0], xd.shape[0], qd.shape[1]
    nbytes = lib.la_knn_scratch_bytes(nq, nx, D, k)
    assert nbytes > 0
    g = Guarded('ones')
    ws = g.alloc(nbytes, dev, torch.float64)
    dist2 = g.tensor([nq, k], torch.float64, dev, -7.0)
    idx = g.tensor([nq, k], torch.int32, dev, -7)
    with torch.cuda.device(dev):
        rc = lib.la_knn_f32(_p(qd), nq, _p(xd), nx, D, k, int(exclude_self), _p(dist2), _p(idx), _p(ws), nbytes, _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    return dist2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _realism(lib, dev, q, x, radius2):
    qd, xd = _dev32(q, dev), _dev32(x, dev)
    nq, nx, D = qd.shape[0], xd.shape[0], qd.shape[1]
    nbytes = lib.la_knn_scratch_bytes(nq, nx, D, 1)
    g = Guarded('ones')
    ws = g.alloc(nbytes, dev, torch.float64)
    score2 = g.tensor([nq], torch.float64, dev, -7.0)
    arg = g.tensor([nq], torch.int32, dev, -7)
    r2 = torch.from_numpy(np.array(radius2, np.float64)).to(dev)          # (a copy: the shared radii are read-only)
    with torch.cuda.device(dev):
        rc = lib.la_realism_f32(_p(qd), nq, _p(xd), nx, D, _p(r2), _p(score2), _p(arg), _p(ws), nbytes, _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    return score2.cpu().numpy(), arg.cpu().numpy().astype(np.int64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# integer inputs: bit for bit

@pytest.mark.parametrize('nq,nx,D,k', kc.exact_cases())
def test_knn_is_exact_on_integers(lib, dev, nq, nx, D, k):
    q, x = kc.exact_inputs(nq, nx, D)
    dist2, idx = _knn(lib, dev, q, x, k)
    want_d, want_i = kc.knn_restate(q, x, k)
    assert _same_bits(dist2, want_d) and (idx == want_i).all()
    if k > nx:
        assert (idx[:, nx:] == -1).all() and np.isposinf(dist2[:, nx:]).all()


@pytest.mark.parametrize('n,D,k', [(5, 3, 5), (32, 4, 32), (33, 17, 32), (65, 1, 3), (129, 33, 5), (2, 130, 1), (1, 4, 3)])
def test_knn_exclude_self_on_integers(lib, dev, n, D, k):
    """n == k leaves one empty slot per row; n == 1 leaves nothing but empty slots"""
    q, _ = kc.exact_inputs(n, n, D)
    dist2, idx = _knn(lib, dev, q, q, k, exclude_self=True)
    want_d, want_i = kc.knn_restate(q, q, k, exclude_self=True)
    assert _same_bits(dist2, want_d) and (idx == want_i).all()
    assert not (idx == np.arange(n)[:, None]).any()
    if k >= n:
        assert (idx[:, n - 1:] == -1).all() and np.isposinf(dist2[:, n - 1:]).all()


def test_knn_merges_more_than_one_column_split_on_integers(lib, dev):
    nq, nx, D, k = kc.SPLIT_CASE
    assert lib.la_knn_col_splits(nq, nx) > 1
    q, x = kc.exact_inputs(nq, nx, D)
    dist2, idx = _knn(lib, dev, q, x, k)
    want_d, want_i = kc.knn_restate(q, x, k)
    assert _same_bits(dist2, want_d) and (idx == want_i).all()
    assert (np.diff(dist2, axis=1) == 0).any()          # ties across the chunks: the merge orders them by index


def test_duplicate_bank_rows_and_a_query_that_is_a_bank_row(lib, dev):
    q, x = (a.copy() for a in kc.exact_inputs(65, 129, 17))
    x[100] = x[3]
    x[64] = x[3]
    q[10] = x[3]
    dist2, idx = _knn(lib, dev, q, x, 5)
    want_d, want_i = kc.knn_restate(q, x, 5)
    assert _same_bits(dist2, want_d) and (idx == want_i).all()
    assert dist2[10, :3].tolist() == [0.0, 0.0, 0.0] and idx[10, :3].tolist() == [3, 64, 100]
    # float rows: the copies still have equal d2 bits (equal rows, equal norms, one k order), the lower index first
    i = 1
    fq, fx = (a.copy() for a in kc.float_inputs(i))
    fx[90] = fx[7]
    fx[64] = fx[7]
    fq[10] = fx[7]
    fq[128] = fx[126]
    d2, ix = _knn(lib, dev, fq, fx, 32)
    # a query that is a bank row: the norms are the diagonal of the same product, so d2 is 0 to the bit on float rows too
    assert d2[10, :3].tolist() == [0.0, 0.0, 0.0] and ix[10, :3].tolist() == [7, 64, 90] and d2[10, 3] > 0
    assert d2[128, 0] == 0.0 and ix[128, 0] == 126 and d2[128, 1] > 0
    for r in range(fq.shape[0]):
        at = [int(np.nonzero(ix[r] == c)[0][0]) for c in (7, 64, 90) if (ix[r] == c).any()]
        assert at == sorted(at) and len({d2[r, a].tobytes() for a in at}) <= 1
        assert len(at) in (0, 3) or at[-1] == 31          # all three or none, unless the list ends among them
        assert at == list(range(at[0], at[0] + len(at))) if at else True          # next to one another


def test_base_pointers_offset_by_one_float(lib, dev):
    for nq, nx, D, k in [(33, 65, 17, 5), (64, 63, 3, 3)]:
        q, x = kc.exact_inputs(nq, nx, D)
        dist2, idx = _knn(lib, dev, q, x, k, offset=True)
        want_d, want_i = kc.knn_restate(q, x, k)
        assert _same_bits(dist2, want_d) and (idx == want_i).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# float inputs: within B, every index equal

@pytest.mark.parametrize('i', range(len(kc.FLOAT_CASES)))
def test_knn_float_cases_within_the_bound(lib, dev, i):
    nq, nx, D, k = kc.FLOAT_CASES[i]
    q, x = kc.float_inputs(i)
    dist2, idx = _knn(lib, dev, q, x, k)
    want_d, want_i = kc.knn_restate(q, x, k)
    kk = min(k, nx)
    B = np.take_along_axis(kc.bound(q, x), want_i[:, :kk], axis=1)
    err = np.abs(dist2[:, :kk] - want_d[:, :kk])
    print(f'knn float case {i} {kc.FLOAT_CASES[i]} ({lib.la_knn_col_splits(nq, nx)} splits): worst |d2 - ref| {err.max():.2e}, '
          f'worst err / B {float((err / B).max()):.4f}, indices differing {int((idx != want_i).sum())} (cap 0)')
    assert (idx == want_i).all()
    assert (err <= B).all()
    assert (idx[:, kk:] == -1).all() and np.isposinf(dist2[:, kk:]).all()


def test_exclude_self_float(lib, dev):
    q, _ = kc.float_inputs(6)
    dist2, idx = _knn(lib, dev, q, q, 5, exclude_self=True)
    want_d, want_i = kc.knn_restate(q, q, 5, exclude_self=True)
    B = np.take_along_axis(kc.bound(q, q), want_i, axis=1)
    assert (idx == want_i).all() and (np.abs(dist2 - want_d) <= B).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# position independence

def test_rows_of_a_batch_do_not_depend_on_the_batch(lib, dev):
    q, x = kc.float_inputs(0)          # 200 x 300: the slices below start in other tiles, rows and splits than the whole has
    dist2, idx = _knn(lib, dev, q, x, 5)
    for a, b in [(0, 1), (3, 70), (64, 129), (190, 200)]:
        d, i = _knn(lib, dev, q[a:b], x, 5)
        assert _same_bits(d, dist2[a:b]) and (i == idx[a:b]).all(), (a, b)
        assert lib.la_knn_col_splits(b - a, 300) >= lib.la_knn_col_splits(200, 300)


def test_appending_farther_bank_rows_changes_nothing(lib, dev):
    q, x = kc.float_inputs(5)          # 127 x 200, D = 4
    dist2, idx = _knn(lib, dev, q, x, 5)
    far = (x[:150] + np.float32(50.0)).astype(np.float32)          # every appended row is farther than any current 5th neighbour
    assert kc.dist2(q, far).min() > dist2.max() * 4
    d, i = _knn(lib, dev, q, np.concatenate([x, far]), 5)
    assert lib.la_knn_col_splits(127, 350) != lib.la_knn_col_splits(127, 200)          # (other chunks too)
    assert _same_bits(d, dist2) and (i == idx).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the realism entry

@pytest.mark.parametrize('i', range(len(kc.FLOAT_CASES)))
def test_realism_entry_float_cases(lib, dev, i):
    nq, nx, D, _ = kc.FLOAT_CASES[i]
    q, x = kc.float_inputs(i)
    radius2 = kc.realism_radii(i)          # every third sphere dropped
    score2, arg = _realism(lib, dev, q, x, radius2)
    want_s, want_a = kc.realism_entry_restate(q, x, radius2)
    d2 = kc.dist2(q, x)[np.arange(nq), want_a]
    b = kc.bound(q, x)[np.arange(nq), want_a] / d2
    rel = (1.0 + b / (1.0 - b)) * (1.0 + 2.0 ** -53) - 1.0
    err = np.abs(score2 - want_s) / want_s
    print(f'realism float case {i} ({lib.la_knn_col_splits(nq, nx)} splits): worst relative error {err.max():.2e}, '
          f'worst err / bound {float((err / rel).max()):.4f}, args differing {int((arg != want_a).sum())} (cap 0)')
    assert (arg == want_a).all() and (radius2[arg] >= 0).all()
    assert (err <= rel).all()
    if kc.FLOAT_CASES[i] == kc.SPLIT_CASE:
        assert lib.la_knn_col_splits(nq, nx) > 1


def test_realism_entry_on_integers_zero_distance_and_no_sphere(lib, dev):
    q, x = (a.copy() for a in kc.exact_inputs(33, 129, 3))
    q[5] = x[77]
    radius2 = np.arange(1, 130, dtype=np.float64)
    radius2[::4] = -1.0
    radius2[77] = 2.0
    score2, arg = _realism(lib, dev, q, x, radius2)
    want_s, want_a = kc.realism_entry_restate(q, x, radius2)
    assert _same_bits(score2, want_s) and (arg == want_a).all()
    dup = int(np.nonzero((x == x[77]).all(axis=1) & (radius2 >= 0))[0][0])          # the lowest kept copy of that row
    assert np.isposinf(score2[5]) and arg[5] == dup
    # a dropped sphere at distance 0 is ignored
    radius2[(x == x[77]).all(axis=1)] = -1.0
    score2, arg = _realism(lib, dev, q, x, radius2)
    want_s, want_a = kc.realism_entry_restate(q, x, radius2)
    assert np.isfinite(score2[5]) and _same_bits(score2, want_s) and (arg == want_a).all()
    # no kept sphere at all
    score2, arg = _realism(lib, dev, q, x, np.full([129], -1.0))
    assert not score2.any() and (arg == -1).all()
    # more than one column split, exact
    nq, nx, D, _ = kc.SPLIT_CASE
    q, x = kc.exact_inputs(nq, nx, D)
    radius2 = np.where(np.arange(nx) % 5 == 0, -1.0, 1.0 + (np.arange(nx) % 7))
    score2, arg = _realism(lib, dev, q, x, radius2)
    want_s, want_a = kc.realism_entry_restate(q, x, radius2)
    assert lib.la_knn_col_splits(nq, nx) > 1 and _same_bits(score2, want_s) and (arg == want_a).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python level

def test_python_functions_agree_with_the_restatement(dev):
    from latentaugment_amd import metrics
    real, gen = kc.two_blobs()
    dist, idx = metrics.knn_from_features(gen, real, 5, device=dev)
    want_d, want_i = kc.knn_restate(gen, real, 5)
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (90, 5)
    B = np.take_along_axis(kc.bound(gen, real), want_i, axis=1)
    assert (idx == want_i).all() and (np.abs(dist * dist - want_d) <= B + 4 * np.spacing(want_d)).all()
    d2, i2 = metrics.knn_from_features(torch.from_numpy(real).double(), real, 3, exclude_self=True, device=dev)
    assert (i2 == kc.knn_restate(real, real, 3, exclude_self=True)[1]).all()
    for keep in (0.5, 1.0):
        realism, det = metrics.compute_realism_from_features(real, gen, nhood_size=3, keep_fraction=keep, device=dev, return_details=True)
        want, bnd = kc.realism_restate(real, gen, 3, keep), kc.realism_rel_bounds(real, gen, 3, keep)
        rel = np.abs(realism / want['realism'] - 1.0)
        rrel = np.abs(det['radii'] / want['radii'] - 1.0)
        print(f'realism keep {keep}: worst relative error {rel.max():.2e} = {float((rel / bnd["realism"]).max()):.4f} of its bound, radii '
              f'{rrel.max():.2e} = {float((rrel / bnd["radii"]).max()):.4f}; {int((realism >= 1).sum())} of {len(realism)} at or above 1')
        assert realism.dtype == np.float64 and realism.shape == (90,)
        assert (det['kept'] == want['kept']).all() and (det['arg'] == want['arg']).all()
        assert (rrel <= bnd['radii']).all() and (rel <= bnd['realism']).all()
        assert (metrics.compute_realism_from_features(real, gen, 3, keep, device=dev) == realism).all()
    assert ((realism >= 1.0) == kc.membership64(real, gen, 3)).all() and 0 < (realism >= 1).sum() < 90
    auth, det = metrics.compute_authenticity_from_features(real, gen, device=dev, return_details=True)
    want = kc.authenticity_restate(real, gen)
    assert auth == want['authenticity'] and (det['authentic'] == want['authentic']).all() and (det['nearest'] == want['nearest']).all()
    near_real = kc.knn_restate(real, real, 1, exclude_self=True)[1][:, 0]
    assert (np.abs(det['d_gen'] / want['d_gen'] - 1.0) <= kc.dist_rel_bound(gen, real, want['nearest'])).all()
    assert (np.abs(det['d_real'] / want['d_real'] - 1.0) <= kc.dist_rel_bound(real, real, near_real)[want['nearest']]).all()
    assert 0.0 < auth < 1.0


def test_copies_are_not_authentic_and_far_samples_are_not_real(dev):
    from latentaugment_amd import metrics
    real, _ = kc.two_blobs()
    copies = real[10:60].copy()
    assert metrics.compute_authenticity_from_features(real, copies, device=dev) == 0.0
    # realism of a copy: inf where its source's sphere is kept; keep_fraction = 1 keeps all
    assert np.isposinf(metrics.compute_realism_from_features(real, copies, keep_fraction=1.0, device=dev)).all()
    far = real + np.float32(100.0)
    realism = metrics.compute_realism_from_features(real, far, keep_fraction=1.0, device=dev)
    assert (realism < 1.0).all() and (realism > 0.0).all()
    assert metrics.compute_authenticity_from_features(real, far, device=dev) == 1.0


def test_python_misuse_raises(dev):
    from latentaugment_amd import _lib, metrics
    real, gen = kc.two_blobs()
    with pytest.raises(ValueError, match='k must'):
        metrics.knn_from_features(gen, real, 33, device=dev)
    with pytest.raises(ValueError, match='exclude_self'):
        metrics.knn_from_features(gen, real, 3, exclude_self=True, device=dev)
    with pytest.raises(ValueError, match='one D'):
        metrics.knn_from_features(gen[:, :5], real, 3, device=dev)
    with pytest.raises(ValueError, match='nhood_size'):
        metrics.compute_realism_from_features(real[:3], gen, nhood_size=3, device=dev)
    with pytest.raises(ValueError, match='keep_fraction'):
        metrics.compute_realism_from_features(real, gen, keep_fraction=0.0, device=dev)
    with pytest.raises(ValueError, match='at least 2'):
        metrics.compute_authenticity_from_features(real[:1], gen, device=dev)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.knn_from_features(gen, real, 3, device='cpu')


def test_metrics_from_images_take_the_two_keys_on_request(dev, tmp_path):
    from latentaugment_amd import metrics
    from latentaugment_amd.synthesis import DetectorEngine
    path = tmp_path / 'det.pt'
    hsd.save_scripted_detector(path)          # the small scripted detector of the detector tests
    det = DetectorEngine.from_torchscript(str(path), dev, max_batch=4)
    g = torch.Generator().manual_seed(31)
    real = [torch.rand([4, 1, 40, 40], generator=g) * 2 - 1 for _ in range(3)]
    gen = [torch.rand([4, 1, 40, 40], generator=g) * 1.6 - 0.8 for _ in range(2)]
    plain = metrics.compute_metrics_from_images(real, gen, det, nhood_size=3)
    assert set(plain) == {'precision', 'recall', 'density', 'coverage', 'kid'}
    one = metrics.compute_metrics_from_images(real, gen, det, nhood_size=3, realism=True)
    assert set(one) == set(plain) | {'realism'} and all(one[k] == plain[k] for k in plain)
    out = metrics.compute_metrics_from_images(real, gen, det, nhood_size=3, realism=True, authenticity=True)
    assert set(out) == set(plain) | {'realism', 'authenticity'} and all(out[k] == plain[k] for k in plain)
    fr = metrics.compute_feature_stats_for_images(real, det, capture_all=True).get_all()
    fg = metrics.compute_feature_stats_for_images(gen, det, capture_all=True).get_all()
    assert out['realism'] == float(metrics.compute_realism_from_features(fr, fg, nhood_size=3, device=dev).mean()) == one['realism']
    assert out['authenticity'] == metrics.compute_authenticity_from_features(fr, fg, device=dev)
    assert 0.0 <= out['authenticity'] <= 1.0 and out['realism'] >= 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism, scratch, capture

def test_two_runs_give_the_same_bits(lib, dev):
    q, x = kc.float_inputs(3)          # 40 column splits
    a, b = _knn(lib, dev, q, x, 32), _knn(lib, dev, q, x, 32)
    assert _same_bits(a[0], b[0]) and (a[1] == b[1]).all()
    r = kc.realism_radii(3)
    a, b = _realism(lib, dev, q, x, r), _realism(lib, dev, q, x, r)
    assert _same_bits(a[0], b[0]) and (a[1] == b[1]).all()


def test_package_scratch_is_guarded_and_its_contents_are_not_read(dev, monkeypatch):
    from latentaugment_amd import _lib, metrics
    real, gen = kc.two_blobs()
    res = {}
    for pattern in ('zeros', 'ones', 'bytes'):
        g = Guarded(pattern)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'workspace', g.alloc)
            dist, idx = metrics.knn_from_features(gen, real, 5, device=dev)
            realism, rd = metrics.compute_realism_from_features(real, gen, device=dev, return_details=True)
            auth, ad = metrics.compute_authenticity_from_features(real, gen, device=dev, return_details=True)
            torch.cuda.synchronize()
        g.check()
        assert len(g.records) == 1 + 2 + 2          # every scratch buffer of the three functions came through _lib.workspace
        res[pattern] = [dist, idx, realism, rd['radii'], rd['arg'], ad['d_gen'], ad['d_real'], np.float64(auth)]
    for pattern in ('ones', 'bytes'):
        assert all(_same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(res['zeros'], res[pattern])), pattern


def test_short_scratch_is_refused_and_outputs_keep_their_fill(lib, dev):
    q, x = kc.exact_inputs(33, 65, 17)
    qd, xd = _dev32(q, dev), _dev32(x, dev)
    need = lib.la_knn_scratch_bytes(33, 65, 17, 5)
    ws = torch.full([need // 8], -7.0, dtype=torch.float64, device=dev)
    dist2 = guarded_tensor([33, 5], torch.float64, dev, -7.0)
    idx = guarded_tensor([33, 5], torch.int32, dev, -7)
    with torch.cuda.device(dev):
        rc = lib.la_knn_f32(_p(qd), 33, _p(xd), 65, 17, 5, 0, _p(dist2), _p(idx), _p(ws), need - 8, _s())
        rc2 = lib.la_knn_f32(_p(qd), 33, _p(xd), 65, 17, 5, 1, _p(dist2), _p(idx), _p(ws), need, _s())
    torch.cuda.synchronize()
    assert rc == LA_ERR_WORKSPACE and rc2 == LA_ERR_ARG
    assert (ws == -7.0).all() and (dist2 == -7.0).all() and (idx == -7).all()


def test_one_captured_graph_replay_equals_eager(lib, dev):
    nq, nx, D, k = 65, 300, 17, 5
    q, x = kc.float_inputs(0)
    q, x = q[:nq, :D], x[:nx, :D]
    eager_d, eager_i = _knn(lib, dev, q, x, k)
    qd, xd = _dev32(q, dev), _dev32(x, dev)
    nbytes = lib.la_knn_scratch_bytes(nq, nx, D, k)
    ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
    dist2 = torch.full([nq, k], -7.0, dtype=torch.float64, device=dev)
    idx = torch.full([nq, k], -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.la_knn_f32(_p(qd), nq, _p(xd), nx, D, k, 0, _p(dist2), _p(idx), _p(ws), nbytes, _s())
    assert rc == 0, lib.la_last_error()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(dist2.cpu().numpy(), eager_d) and (idx.cpu().numpy() == eager_i).all()
