"""The Frechet distance on the GPU: la_fd_gram_f32 / la_fd_jacobi_sweep_f64 / la_fd_finish_f64 at the C ABI and
metrics.compute_fd_from_features, against the float64 restatements of tests/fd_cases.py and the reference's golden FID.

EXACT: the cross-Gram matrix and the three scalar terms on integer-valued features with zero column means (every sum is exact in
float64, so any order gives numpy's bits); two runs of anything.
BOUNDED: |FD_hip - FD_ref| <= 1e-10 x (mean_term + trace_gen + trace_real).  FD is a difference of those terms, so the bound is stated
against their size; float64 arithmetic in another order is about m x eps x sweeps of it, near 1e-12 at these sizes.  Singular values:
1e-12 of the largest.  The scale comes from the restatement, never from the code under test.  Every case prints its figures.

Largest measured on an MI355X: FD error 9.6e-12 = 0.0006 of its bound (golden b, 513 x 700, 23 sweeps), singular values 7.4e-14 of the
largest (same case), Gram centring error 0, sweeps 3 .. 23; every comparable rotation count equal to the restatement's.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_cases as fc  # noqa: E402
import helpers_script_detector as hsd  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz'))
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3
FD_TOL = 1e-10
CASES = fc.fd_cases()


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


def _offset_by_one_float(a, dev):
    """a device copy that starts one float past the start of its allocation"""
    buf = torch.empty([a.size + 1], dtype=torch.float32, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def _gram(lib, dev, x, y):
    """la_fd_gram_f32 on device tensors x [nx][D], y [ny][D] -> (vectors [n'][m] float64, terms [3] float64) as numpy"""
    nx, ny, D = x.shape[0], y.shape[0], x.shape[1]
    n, m = min(nx, ny), max(nx, ny)
    ws_bytes = lib.la_fd_workspace_bytes(nx, ny, D)
    assert ws_bytes >= (n + (n & 1)) * m * 8
    ws = torch.full([ws_bytes // 8], -7.0, dtype=torch.float64, device=dev)
    terms = torch.full([4], -7.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.la_fd_gram_f32(_p(x), nx, _p(y), ny, D, _p(terms), _p(ws), ws_bytes, _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return ws[:(n + (n & 1)) * m].reshape(-1, m).cpu().numpy(), terms[:3].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# cross-Gram matrix and scalar terms

@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('nx,ny,D', fc.GRAM_EXACT_SIZES)
def test_gram_and_terms_are_exact_on_integers(lib, dev, nx, ny, D, offset):
    x, y = fc.gram_exact_inputs(nx, ny, D, seed=nx + D)
    assert not x.mean(0).any() and not y.mean(0).any()
    xd = _offset_by_one_float(x, dev) if offset else torch.from_numpy(x).to(dev)
    V, terms = _gram(lib, dev, xd, torch.from_numpy(y).to(dev))
    want = fc.vectors_of(x.astype(np.float64) @ y.astype(np.float64).T)
    bad = np.argwhere(V != want)
    assert V.shape == want.shape and bad.size == 0, f'{len(bad)} of {want.size} entries differ, first at {bad[0].tolist()}'
    want_terms = np.array([0.0, np.square(x.astype(np.float64)).sum(), np.square(y.astype(np.float64)).sum()])
    assert (terms == want_terms).all(), (terms, want_terms)


def test_gram_is_centred_in_float64(lib, dev):
    """features of mean 1000 and spread 1: a centred float32 copy would lose about 1e-4 of |C|_max"""
    rs = np.random.RandomState(21)
    x = (1000.0 + rs.randn(40, 96)).astype(np.float32)
    y = (1000.0 + rs.randn(48, 96)).astype(np.float32)
    V, terms = _gram(lib, dev, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    a, b = x.astype(np.float64), y.astype(np.float64)
    a, b = a - a.mean(0), b - b.mean(0)
    want = a @ b.T
    err = float(np.abs(V - want).max()) / float(np.abs(want).max())
    want_terms = np.array([np.square(x.astype(np.float64).mean(0) - y.astype(np.float64).mean(0)).sum(), np.square(a).sum(), np.square(b).sum()])
    terr = float(np.abs(terms / want_terms - 1).max())
    print(f'gram centring 40 x 48 x 96: worst |C - ref| / |C|max {err:.2e} (bound 1e-12), terms rel {terr:.2e}')
    assert err <= 1e-12 and terr <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# one sweep at the C ABI

@pytest.mark.parametrize('name', fc.SWEEP_CASES)
def test_sweeps_follow_the_restatement(lib, dev, name):
    """7 x 5: odd n, the padding vector takes part in every round; 300 x 9: m above one workgroup's width; 2048 .. 8193: the last and the
    first m of the round kernel's forms with 8, 16 and 32 elements a thread in registers and of the streaming one.  After every sweep the Gram
    matrix of the vectors equals the restatement's.  The rotation counts are compared in the sweeps whose decisions are all clear of
    the threshold by a factor 8 in the restatement (the first always is: tests/test_fd_cases_cpu.py); next to the threshold the two
    summation orders may decide differently, by a rotation of an angle near eps."""
    Cm = fc.jacobi_cases()[name]
    ref = fc.vectors_of(Cm)
    n, m = min(Cm.shape), max(Cm.shape)
    tol = fc.jacobi_tol(m)
    v = torch.from_numpy(ref.copy()).to(dev)
    rot = torch.full([1], -5, dtype=torch.int32, device=dev)
    compared = 0
    for sweep in range(1, 16):
        margin = []
        want = fc.jacobi_sweep(ref, tol, margin)
        with torch.cuda.device(dev):
            rc = lib.la_fd_jacobi_sweep_f64(_p(v), n, m, _p(rot), _s())
        assert rc == 0, lib.la_last_error()
        got = int(rot.item())
        V = v.cpu().numpy()
        g_got, g_want = V @ V.T, ref @ ref.T
        err = float(np.abs(g_got - g_want).max()) / float(np.abs(g_want).max())
        decisive = all(x > 8.0 or x < 0.125 for x in margin)
        print(f'sweep {name} #{sweep}: rotations {got} (restatement {want}, decisive {decisive}), Gram err {err:.2e} of the largest entry')
        assert err <= 1e-12
        if decisive:
            assert got == want
            compared += 1
        if n & 1:
            assert not V[n].any()          # the padding vector stays zero
        if want == 0:
            break
    assert want == 0 and compared >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole function

def _check(name, real, gen, dev, ref=None):
    from latentaugment_amd import metrics
    fd, det = metrics.compute_fd_from_features(real, gen, device=dev, return_details=True)
    mean, tg, tr, nuc, sv = fc.fd_terms64(real, gen)
    scale = mean + tg + tr
    want = (mean + tg + tr - 2.0 * nuc) if ref is None else ref
    err = abs(fd - want)
    sv_err = float(np.abs(np.sort(det['singular_values'])[::-1] - sv).max()) / float(sv[0])
    print(f'FD {name}: {fd:.12e} ref {want:.12e} err {err:.2e} / bound {FD_TOL * scale:.2e} = {err / (FD_TOL * scale):.4f}; '
          f'sweeps {det["sweeps"]}; singular values err {sv_err:.2e} of the largest')
    assert isinstance(fd, float) and det['singular_values'].shape == (min(real.shape[0], gen.shape[0]),)
    assert err <= FD_TOL * scale
    assert sv_err <= 1e-12
    assert det['sweeps'] <= 30
    assert det['mean_term'] == pytest.approx(mean, rel=1e-12, abs=1e-300) and det['trace_gen'] == pytest.approx(tg, rel=1e-12)
    assert det['trace_real'] == pytest.approx(tr, rel=1e-12) and det['nuclear'] == pytest.approx(nuc, rel=1e-12)
    assert fd == det['mean_term'] + det['trace_gen'] + det['trace_real'] - 2.0 * det['nuclear']
    return fd, det


@pytest.mark.parametrize('name', list(CASES))
def test_fd_against_the_float64_restatement(dev, name):
    real, gen = CASES[name]
    # gen = real: the exact value is 0, which needs no reference
    _check(name, real, gen, dev, ref=0.0 if name.startswith('gen = real') else None)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_fd_vs_reference_golden(dev, case):
    """the number the reference's compute_fid produced, at the tolerance the scipy-route test holds; b is 513 x 700: n odd"""
    real, gen = GOLD[f'{case}_real'], GOLD[f'{case}_gen']
    fd, det = _check(f'golden {case}', real, gen, dev)
    assert fd == pytest.approx(float(GOLD[f'{case}_fid']), rel=1e-8)


@pytest.mark.parametrize('name', ['rank-deficient 40/48 x 96', 'rank-deficient 33/17 x 256'])
def test_fd_is_symmetric_in_its_arguments(dev, name):
    """exchanging the sets exchanges which side supplies the vectors: both storage orientations of each case"""
    from latentaugment_amd import metrics
    real, gen = CASES[name]
    a = metrics.compute_fd_from_features(real, gen, device=dev)
    b = metrics.compute_fd_from_features(gen, real, device=dev)
    bound = FD_TOL * fc.fd_scale(real, gen)
    print(f'FD symmetry {name}: {a:.15e} / {b:.15e}, differ by {abs(a - b):.2e} (bound {bound:.2e})')
    assert abs(a - b) <= bound


def test_fd_two_runs_give_the_same_bits(dev):
    from latentaugment_amd import metrics
    real, gen = CASES['rank-deficient 33/17 x 256']
    f1, d1 = metrics.compute_fd_from_features(real, gen, device=dev, return_details=True)
    f2, d2 = metrics.compute_fd_from_features(torch.from_numpy(real).to(dev), torch.from_numpy(gen).to(dev).double(), device=dev,
                                              return_details=True)
    assert f1 == f2 and d1['sweeps'] == d2['sweeps']
    assert (d1['terms'] == d2['terms']).all() and (d1['singular_values'] == d2['singular_values']).all()


def test_fd_misuse_raises_and_leaves_the_path_usable(lib, dev):
    from latentaugment_amd import _lib, metrics
    real, gen = CASES['n = 2']
    want = fc.fd_ref64(real, gen)
    bound = FD_TOL * fc.fd_scale(real, gen)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_fd_from_features(torch.from_numpy(real), torch.from_numpy(gen).to(dev), device=dev)          # a CPU tensor
    with pytest.raises(_lib.LatentAugHipError, match='at least 2 samples'):
        metrics.compute_fd_from_features(real, gen[:1], device=dev)
    with pytest.raises(_lib.LatentAugHipError, match='one D'):
        metrics.compute_fd_from_features(real, gen[:, :8], device=dev)
    with pytest.raises(_lib.LatentAugHipError, match='max_sweeps'):
        metrics.compute_fd_from_features(*CASES['rank-deficient 40/48 x 96'], device=dev, max_sweeps=1)
    # a short workspace at the C ABI: refused before anything is launched
    x, y = torch.from_numpy(gen).to(dev), torch.from_numpy(real).to(dev)
    need = lib.la_fd_workspace_bytes(x.shape[0], y.shape[0], x.shape[1])
    ws = torch.full([need // 8], -7.0, dtype=torch.float64, device=dev)
    terms = torch.full([4], -7.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.la_fd_gram_f32(_p(x), x.shape[0], _p(y), y.shape[0], x.shape[1], _p(terms), _p(ws), need - 1, _s())
        rc2 = lib.la_fd_finish_f64(_p(ws), need - 1, x.shape[0], y.shape[0], x.shape[1], None, _p(terms), _s())
    torch.cuda.synchronize()
    assert rc == LA_ERR_WORKSPACE and rc2 == LA_ERR_WORKSPACE and b'workspace' in lib.la_last_error()
    assert (ws == -7.0).all() and (terms == -7.0).all()
    assert abs(metrics.compute_fd_from_features(real, gen, device=dev) - want) <= bound


# ---------------------------------------------------------------------------------------------------------------------------------
# from images

def test_metrics_from_images_take_the_frechet_key_on_request(dev, tmp_path):
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
    out = metrics.compute_metrics_from_images(real, gen, det, nhood_size=3, frechet=True)
    assert set(out) == set(plain) | {'fd'} and all(out[k] == plain[k] for k in plain)
    fr = metrics.compute_feature_stats_for_images(real, det, capture_all=True).get_all()
    fg = metrics.compute_feature_stats_for_images(gen, det, capture_all=True).get_all()
    assert out['fd'] == metrics.compute_fd_from_features(fr, fg, device=dev)
    assert abs(out['fd'] - fc.fd_ref64(fr, fg)) <= FD_TOL * fc.fd_scale(fr, fg)
