"""Kernel Inception Distance without a GPU: the properties of the float64 restatement (tests/kid_cpu.py) that the GPU test leans on,
and the host side of metrics.compute_kid_from_features / la_kid_poly3_f32 (argument errors, the header, the exported symbols).

The seeded inputs below were run on the CPU before their margins were written down:
  null: 3000 pairs of standard-normal sets (n = 48 per side, D = 16, full-set estimator), seeds 2p, 2p + 1 from the bases 0, 10000
        and 20000: mean 3.5e-6, standard error 9.0e-4.  The three bases of 1000 pairs alone sit at +1.08, -0.71 and -0.38 of their
        own standard errors (1.6e-3), i.e. "within one standard error" is a 68 % event per base; the pooled run is what is asserted.
        The biased estimator has mean 0.316 on the same draws.
        (Detector-like features with their rare large coordinates have so heavy a tail at D = 16 that 1000 pairs give a standard
        error of 2.7e-2 and means of -1.4 .. +1.5 standard errors: the Gaussian draw is used for this property.)
  mean shift of 0.25 on every coordinate (detector-like, n = 64, D = 16): mmd2 = 0.771, the unshifted pair gives -0.048
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_cpu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full(real, gen):
    return kid_cpu.kid(real, gen, num_subsets=1, max_subset_size=None)


def test_unbiased_under_the_null():
    """Two independent draws from one distribution: the mean of the estimator over many seeds is within its own standard error of 0
    (the biased estimator, with the diagonals kept, sits many standard errors above 0 on the same draws)."""
    draw = lambda seed: np.random.RandomState(seed).standard_normal([48, 16]).astype(np.float32)      # noqa: E731
    kd = lambda f: float((((f.astype(np.float64) ** 2).sum(1) / 16 + 1) ** 3).sum())                  # noqa: E731  the i == j terms
    m = 48
    vals, biased = [], []
    for base in (0, 10000, 20000):
        for pair in range(1000):
            a, b = draw(base + 2 * pair), draw(base + 2 * pair + 1)
            r = _full(a, b)
            vals.append(float(r['kid']))
            biased.append((r['sums'][0, 0] + kd(b)) / m ** 2 + (r['sums'][0, 1] + kd(a)) / m ** 2 - 2 * r['sums'][0, 2] / m ** 2)
    vals, biased = np.asarray(vals), np.asarray(biased)
    se = vals.std(ddof=1) / np.sqrt(len(vals))
    print(f'null: mean {vals.mean():.3e}  standard error {se:.3e}  biased mean {biased.mean():.3e}')
    assert abs(vals.mean()) <= se
    assert biased.mean() > 5 * se


def test_mean_shift_is_positive():
    a, b = kid_cpu.detector_like_features(64, 16, 100), kid_cpu.detector_like_features(64, 16, 101)
    null = float(_full(a, b)['kid'])
    shifted = float(_full(a, b + np.float32(0.25))['kid'])
    print(f'null {null:.3e}  shifted {shifted:.3e}')
    assert shifted > 0.3 and shifted > 10 * abs(null)


def test_sums_do_not_depend_on_row_order_within_a_subset():
    real, gen = kid_cpu.detector_like_features(90, 24, 5), kid_cpu.detector_like_features(70, 24, 6, scale=1.1)
    ix, iy = kid_cpu.subset_indices(90, 70, num_subsets=4, max_subset_size=40, seed=3)
    rs = np.random.RandomState(9)
    ix2 = np.stack([rs.permutation(r) for r in ix])
    iy2 = np.stack([rs.permutation(r) for r in iy])
    r1, r2 = kid_cpu.kid_from_indices(real, gen, ix, iy), kid_cpu.kid_from_indices(real, gen, ix2, iy2)
    # the same 40 * 39, 40 * 39 and 40 * 40 float64 terms in another order
    np.testing.assert_allclose(r2['sums'], r1['sums'], rtol=1e-13, atol=0)
    np.testing.assert_allclose(r2['mmd2'], r1['mmd2'], rtol=0, atol=1e-13 * float(r1['nsums'].max()))


def test_full_set_form_equals_the_closed_formula():
    real, gen = kid_cpu.detector_like_features(7, 5, 1).astype(np.float64), kid_cpu.detector_like_features(5, 5, 2).astype(np.float64)
    k = lambda a, b: (float(np.dot(a, b)) / 5 + 1) ** 3      # noqa: E731
    mx, my = 5, 7
    sxx = sum(k(gen[i], gen[j]) for i in range(mx) for j in range(mx) if i != j)
    syy = sum(k(real[i], real[j]) for i in range(my) for j in range(my) if i != j)
    sxy = sum(k(gen[i], real[j]) for i in range(mx) for j in range(my))
    want = sxx / (mx * (mx - 1)) + syy / (my * (my - 1)) - 2 * sxy / (mx * my)
    r = _full(real, gen)
    assert r['mmd2'].shape == (1,) and r['sums'].shape == (1, 3)
    np.testing.assert_allclose(r['sums'][0], [sxx, syy, sxy], rtol=1e-13)
    assert float(r['kid']) == pytest.approx(want, rel=1e-11, abs=1e-13)


def test_index_draw_matches_the_restatement():
    """metrics.kid_subset_indices is the rule of the restatement: RandomState(seed), generated side first, then the real side."""
    from latentaugment_amd import metrics
    for nr, ng, S, msz, seed in ((50, 40, 3, 16, 0), (1572, 1572, 2, 1000, 7), (12, 30, 5, 1000, 1)):
        ix, iy = metrics.kid_subset_indices(nr, ng, S, msz, seed)
        jx, jy = kid_cpu.subset_indices(nr, ng, S, msz, seed)
        assert ix.dtype == iy.dtype == np.int32 and ix.shape == iy.shape == (S, min(nr, ng, msz))
        assert (ix == jx).all() and (iy == jy).all()
        assert ix.max() < ng and iy.max() < nr and all(len(set(r)) == len(r) for r in ix)
    rs = np.random.RandomState(0)
    first_gen = rs.choice(40, 16, replace=False)
    assert (metrics.kid_subset_indices(50, 40, 3, 16, 0)[0][0] == first_gen).all()
    ix, iy = metrics.kid_subset_indices(9, 5, num_subsets=1, max_subset_size=None)
    assert (ix == np.arange(5)).all() and (iy == np.arange(9)).all() and ix.shape == (1, 5) and iy.shape == (1, 9)


def test_cpu_call_is_refused():
    from latentaugment_amd import _lib, metrics
    a, b = kid_cpu.detector_like_features(8, 4, 0), kid_cpu.detector_like_features(8, 4, 1)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_kid_from_features(a, b, device='cpu')
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_kid_from_features(torch.from_numpy(a), torch.from_numpy(b), device=torch.device('cpu'))


def test_fewer_than_two_rows_is_an_error():
    from latentaugment_amd import metrics
    a = kid_cpu.detector_like_features(8, 4, 0)
    for real, gen, kw in ((a[:1], a, {}), (a, a[:1], {}), (a, a, dict(max_subset_size=1)), (a, a[:1], dict(num_subsets=1, max_subset_size=None))):
        with pytest.raises(ValueError, match='at least 2 rows'):
            metrics.compute_kid_from_features(real, gen, **kw)
    with pytest.raises(ValueError, match='num_subsets=1'):
        metrics.compute_kid_from_features(a, a, num_subsets=2, max_subset_size=None)


def test_symbols_declared_and_exported():
    from latentaugment_amd import _lib
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for name in ('la_kid_poly3_f32', 'la_kid_workspace_bytes'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in include/latentaug_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by the library'
    P, I, L = C.c_void_p, C.c_int, C.c_long
    assert _lib.SIGNATURES['la_kid_workspace_bytes'] == (C.c_size_t, [L, L, L])
    assert _lib.SIGNATURES['la_kid_poly3_f32'] == (I, [P, L, P, L, I, P, P, L, L, L, P, P, P, P, C.c_size_t, P])


def test_workspace_query_and_host_argument_checks():
    """Pure host code: the workspace stays far below one float32 Gram matrix, and bad arguments are refused before any launch (so this
    runs without a device: nothing reaches the HIP runtime)."""
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.la_kid_workspace_bytes(100, 1000, 1000) == 100 * (36 + 36 + 64) * 8 < 4_000_000
    assert lib.la_kid_workspace_bytes(1, 2, 2) == 3 * 8
    assert lib.la_kid_workspace_bytes(1, 129, 128) == (3 + 1 + 2) * 8
    assert lib.la_kid_workspace_bytes(1, 1, 5) == 0 and lib.la_kid_workspace_bytes(0, 5, 5) == 0
    p = 4096          # a non-null, aligned address: every call below is refused before it is looked at
    ok = dict(x=p, nx=10, y=p, ny=10, D=4, ix=p, iy=p, S=1, mx=5, my=5, sums=p, mmd2=p, kid=p, ws=p, ws_bytes=1 << 20)
    for change, code, word in ((dict(x=None), -1, 'null'), (dict(iy=None), -1, 'null'), (dict(kid=None), -1, 'null'), (dict(ws=None), -1, 'null'),
                               (dict(mx=1), -1, 'at least 2'), (dict(my=0), -1, 'at least 2'), (dict(D=0), -1, 'positive'),
                               (dict(S=0), -1, 'positive'), (dict(ws_bytes=23), -3, 'workspace'), (dict(ws_bytes=0), -3, 'workspace')):
        a = dict(ok, **change)
        rc = lib.la_kid_poly3_f32(a['x'], a['nx'], a['y'], a['ny'], a['D'], a['ix'], a['iy'], a['S'], a['mx'], a['my'], a['sums'],
                                  a['mmd2'], a['kid'], a['ws'], a['ws_bytes'], None)
        assert rc == code, (change, rc)
        assert word in lib.la_last_error().decode(), (change, lib.la_last_error())
