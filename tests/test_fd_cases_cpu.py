"""CPU side of the Frechet distance (la_frechet.hip, metrics.compute_fd_from_features): the float64 restatements of tests/fd_cases.py
against the reference's golden FID and numpy's SVD, the pairing of the Jacobi rounds (la_fd_round_pair, a pure host entry), the
workspace query and the host argument checks.  No GPU: everything here is refused or answered before any launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_cases as fc  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz'))
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('case', ['a', 'b'])
def test_restatement_reproduces_the_reference_golden_fid(case):
    """the nuclear-norm form against the number the reference's compute_fid produced (scipy sqrtm of full-rank covariances)"""
    fd = fc.fd_ref64(GOLD[f'{case}_real'], GOLD[f'{case}_gen'])
    want = float(GOLD[f'{case}_fid'])
    print(f'fd_ref64 {case}: {fd:.15e} golden {want:.15e} rel {abs(fd - want) / abs(want):.2e}')
    assert fd == pytest.approx(want, rel=1e-11)


@pytest.mark.parametrize('n', [2, 3, 4, 7, 8, 33, 514])
def test_round_pair_is_a_round_robin_and_the_library_agrees(lib, n):
    n2 = n + (n & 1)
    p, q = C.c_int(-1), C.c_int(-1)
    seen = set()
    for r in range(n2 - 1):
        used = set()
        for k in range(n2 // 2):
            want = fc.round_pair(n, r, k)
            assert lib.la_fd_round_pair(n, r, k, C.byref(p), C.byref(q)) == 0
            assert (p.value, q.value) == want and 0 <= want[0] < want[1] < n2
            assert not (used & set(want)), f'round {r}: a vector appears twice'
            used |= set(want)
            if want[1] < n:          # a pair of real vectors (index n of an odd n is the padding vector)
                assert want not in seen, f'pair {want} visited twice in a sweep'
                seen.add(want)
        assert used == set(range(n2))
    assert len(seen) == n * (n - 1) // 2          # every unordered pair of real vectors exactly once
    for bad in ((n, -1, 0), (n, n2 - 1, 0), (n, 0, n2 // 2), (n, 0, -1), (1, 0, 0), (8193, 0, 0)):
        assert lib.la_fd_round_pair(*bad, C.byref(p), C.byref(q)) == LA_ERR_ARG, bad
    assert lib.la_fd_round_pair(n, 0, 0, None, C.byref(q)) == LA_ERR_ARG and b'null' in lib.la_last_error()


@pytest.mark.parametrize('name', list(fc.jacobi_cases()))
def test_jacobi_restatement_meets_numpy_svd(name):
    Cm = fc.jacobi_cases()[name]
    sv, sweeps = fc.jacobi_ref(Cm)
    want = np.linalg.svd(Cm, compute_uv=False)
    err = float(np.abs(np.sort(sv)[::-1] - want).max()) / float(want[0])
    zeros = int((want < 1e-10 * want[0]).sum())
    # A matrix with SEVERAL zero singular values (D < min(Ng, Nr), or duplicated rows) converges twice: the vectors that end as rounding
    # noise span a subspace of their own, and they start to settle among themselves only when the others have, up to ten sweeps later.
    # One zero singular value (what centring alone leaves) has no such second phase.  So: 15 sweeps with at most one zero singular
    # value, and the bound compute_fd_from_features has (max_sweeps = 30) otherwise.  Measured: 21 sweeps for '200/150 x 64' (86
    # zeros), 17 for the duplicated rows (11 zeros), 7 to 12 for the rest.
    bound = 15 if zeros <= 1 else 30
    print(f'jacobi_ref {name}: {sweeps} sweeps (bound {bound}, {zeros} zero singular values), worst singular value error {err:.2e} of '
          f'the largest, nuclear rel {abs(sv.sum() - want.sum()) / want.sum():.2e}')
    assert err <= 1e-12 and sweeps <= bound


def test_first_sweeps_of_the_sweep_cases_are_decisive():
    """test_hip_fd compares the rotation COUNT of the kernel's sweep with jacobi_sweep's.  A count can only be compared where no
    pair's |gamma| lies near the threshold (the two sides add in different orders); this pins that the sweeps compared there are
    such sweeps, so that test cannot become vacuous."""
    for name in fc.SWEEP_CASES:
        V = fc.vectors_of(fc.jacobi_cases()[name])
        margin = []
        rot = fc.jacobi_sweep(V, fc.jacobi_tol(V.shape[1]), margin)
        assert rot > 0 and all(x > 8.0 or x < 0.125 for x in margin), (name, min(margin))


def test_workspace_query(lib):
    f = lib.la_fd_workspace_bytes
    assert f(2, 2, 1) > 0
    # at least the n' x m doubles and both means
    assert f(1572, 1572, 4096) >= (1572 * 1572 + 2 * 4096) * 8 and f(1572, 1572, 4096) < 2 * 1572 * 1572 * 8
    assert f(33, 17, 130) >= (18 * 33 + 2 * 130) * 8
    for nx, ny, D in ((2, 2, 1), (17, 33, 130), (40, 48, 96), (375, 375, 4096), (513, 700, 96), (8191, 9000, 8)):
        base = f(nx, ny, D)
        assert base > 0 and base % 8 == 0
        assert f(nx + 1, ny, D) >= base and f(nx, ny + 1, D) >= base and f(nx, ny, D + 1) >= base, (nx, ny, D)
        assert f(ny, nx, D) == base
    for bad in ((1, 5, 4), (5, 1, 4), (0, 0, 4), (5, 5, 0), (8193, 8193, 4), (9000, 8193, 4)):
        assert f(*bad) == 0, bad
    assert f(8192, 100000, 4) > 0 and f(100000, 8192, 4) > 0          # only the SMALLER side is limited


def test_host_argument_checks(lib):
    """every refusal comes before any launch, so this runs without a device: nothing reaches the HIP runtime"""
    p = 4096          # a non-null, aligned address: every call below is refused before it is looked at
    ok = dict(x=p, nx=10, y=p, ny=12, D=4, terms=p, ws=p, ws_bytes=1 << 20)
    for change, code, word in ((dict(x=None), LA_ERR_ARG, 'null'), (dict(y=None), LA_ERR_ARG, 'null'), (dict(terms=None), LA_ERR_ARG, 'null'),
                               (dict(ws=None), LA_ERR_ARG, 'null'), (dict(nx=1), LA_ERR_ARG, 'at least 2'), (dict(ny=1), LA_ERR_ARG, 'at least 2'),
                               (dict(D=0), LA_ERR_ARG, 'positive'), (dict(nx=8193, ny=8193), LA_ERR_ARG, 'compute_fid_from_stats'),
                               (dict(ws_bytes=lib.la_fd_workspace_bytes(10, 12, 4) - 1), LA_ERR_WORKSPACE, 'workspace'),
                               (dict(ws_bytes=0), LA_ERR_WORKSPACE, 'workspace')):
        a = dict(ok, **change)
        rc = lib.la_fd_gram_f32(a['x'], a['nx'], a['y'], a['ny'], a['D'], a['terms'], a['ws'], a['ws_bytes'], None)
        assert rc == code and word in lib.la_last_error().decode(), (change, rc, lib.la_last_error())
        if 'x' in change or 'y' in change:
            continue
        rc = lib.la_fd_finish_f64(a['ws'], a['ws_bytes'], a['nx'], a['ny'], a['D'], None, a['terms'], None)
        assert rc == code and word in lib.la_last_error().decode(), (change, rc, lib.la_last_error())
    for args, word in (((None, 4, 8, p), 'null'), ((p, 4, 8, None), 'null'), ((p, 1, 8, p), '2 .. 8192'), ((p, 8193, 9000, p), '2 .. 8192'),
                       ((p, 4, 0, p), 'length')):
        assert lib.la_fd_jacobi_sweep_f64(*args, None) == LA_ERR_ARG and word in lib.la_last_error().decode(), args


def test_signatures_come_from_the_header():
    from latentaugment_amd import _lib
    P, I, L, Z = C.c_void_p, C.c_int, C.c_long, C.c_size_t
    assert _lib.SIGNATURES['la_fd_workspace_bytes'] == (Z, [L, L, I])
    assert _lib.SIGNATURES['la_fd_round_pair'] == (I, [I, I, I, P, P])
    assert _lib.SIGNATURES['la_fd_gram_f32'] == (I, [P, L, P, L, I, P, P, Z, P])
    assert _lib.SIGNATURES['la_fd_jacobi_sweep_f64'] == (I, [P, L, L, P, P])
    assert _lib.SIGNATURES['la_fd_finish_f64'] == (I, [P, Z, L, L, I, P, P, P])


def test_python_misuse_is_refused_without_a_device():
    from latentaugment_amd import _lib, metrics
    a, b = fc.features(8, 4, 0), fc.features(9, 4, 1)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_fd_from_features(a, b, device='cpu')
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_fd_from_features(torch.from_numpy(a), torch.from_numpy(b))          # CPU tensors
    with pytest.raises(_lib.LatentAugHipError, match='at least 2 samples'):
        metrics.compute_fd_from_features(a[:1], b)
    with pytest.raises(_lib.LatentAugHipError, match='one D'):
        metrics.compute_fd_from_features(a, fc.features(9, 5, 1))
    big = np.zeros([8193, 1], np.float32)
    with pytest.raises(_lib.LatentAugHipError, match='compute_fid_from_stats'):
        metrics.compute_fd_from_features(big, big)
    import inspect
    assert inspect.signature(metrics.compute_metrics_from_images).parameters['frechet'].default is False
