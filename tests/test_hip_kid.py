"""Kernel Inception Distance on the GPU: metrics.compute_kid_from_features (la_kid_poly3_f32) against the float64 restatement
(tests/kid_cpu.py) on the same indices.

Error budget, per case, for every per-subset mmd2 and for the mean: the HIP error against float64 must be at most 4x the error of the
SAME restatement run in float32 on the CPU (worst subset of the case), plus a floor of 2e-6 x the largest of the case's three
normalised sums (float64).  The float32 CPU run is the yardstick; the code under test never sets its own budget.  Every case prints
its error / budget ratio.

Largest measured ratio on an MI355X: 0.090 (D=2048 m=2 S=3: mmd2 err 6.262e-07 against a budget of 6.980e-06); the largest at D=7 is
0.064.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_cpu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _features(nr, ng, d, seed):
    """real and generated sets that differ a little (5 % in scale): mmd2 is a small difference of sums of order 1..10"""
    return kid_cpu.detector_like_features(nr, d, seed), kid_cpu.detector_like_features(ng, d, seed + 1000, scale=1.05)


def _check(name, real, gen, dev, **kw):
    from latentaugment_amd import metrics
    kid, det = metrics.compute_kid_from_features(real, gen, device=dev, return_details=True, **kw)
    ix, iy = det['ix'], det['iy']
    jx, jy = kid_cpu.subset_indices(real.shape[0], gen.shape[0], kw['num_subsets'], kw['max_subset_size'], kw.get('seed', 0))
    assert (ix == jx).all() and (iy == jy).all()
    r64 = kid_cpu.kid_from_indices(real, gen, ix, iy, np.float64)
    r32 = kid_cpu.kid_from_indices(real, gen, ix, iy, np.float32)
    assert det['mmd2'].dtype == np.float64 and det['mmd2'].shape == r64['mmd2'].shape and isinstance(kid, float)
    scale = float(r64['nsums'].max())
    floor = 2e-6 * scale
    budget = 4.0 * float(np.abs(r32['mmd2'].astype(np.float64) - r64['mmd2']).max()) + floor
    err = float(np.abs(det['mmd2'] - r64['mmd2']).max())
    budget_mean = 4.0 * abs(float(r32['kid']) - float(r64['kid'])) + floor
    err_mean = abs(kid - float(r64['kid']))
    counts = np.array([ix.shape[1] * (ix.shape[1] - 1), iy.shape[1] * (iy.shape[1] - 1), ix.shape[1] * iy.shape[1]], np.float64)
    err_sums = float(np.abs(det['sums'] / counts - r64['nsums']).max())
    ratio = max(err / budget, err_mean / budget_mean)
    print(f'KID {name}: kid {kid:.6e} scale {scale:.3e}  mmd2 err {err:.3e} / budget {budget:.3e}  mean err {err_mean:.3e} / budget '
          f'{budget_mean:.3e}  worst ratio {ratio:.3f}  (normalised sums err {err_sums:.3e}, floor {floor:.3e})')
    assert err <= budget, f'{name}: per-subset mmd2 off by {err:.3e} > budget {budget:.3e}'
    assert err_mean <= budget_mean, f'{name}: KID off by {err_mean:.3e} > budget {budget_mean:.3e}'
    assert kid == pytest.approx(float(det['mmd2'].mean()), rel=1e-12, abs=1e-15)
    return ratio


@pytest.mark.parametrize('m', [2, 31, 32, 33, 257, 1000])
@pytest.mark.parametrize('D', [7, 64, 2048, 2049])
def test_accuracy_three_subsets(dev, D, m):
    real, gen = _features(1100, 1050, D, seed=D + m)          # Nr != Ng
    _check(f'D={D} m={m} S=3', real, gen, dev, num_subsets=3, max_subset_size=m, seed=m)


@pytest.mark.parametrize('D,m,S,nr,ng', [(64, 33, 1, 90, 70), (2049, 257, 1, 300, 400), (7, 2, 100, 40, 50), (64, 31, 100, 200, 180),
                                         (2048, 1000, 100, 1572, 1500)])
def test_accuracy_one_and_hundred_subsets(dev, D, m, S, nr, ng):
    real, gen = _features(nr, ng, D, seed=S + D)
    _check(f'D={D} m={m} S={S}', real, gen, dev, num_subsets=S, max_subset_size=m, seed=1)


@pytest.mark.parametrize('D,nr,ng', [(7, 2, 131), (2049, 300, 257), (64, 129, 128), (2048, 1000, 33)])
def test_accuracy_full_set_form(dev, D, nr, ng):
    """num_subsets=1, max_subset_size=None: every row once, mx = Ng and my = Nr differ"""
    real, gen = _features(nr, ng, D, seed=nr)
    _check(f'full set D={D} mx={ng} my={nr}', real, gen, dev, num_subsets=1, max_subset_size=None)


def test_subset_axis_beyond_65535(dev):
    real, gen = _features(12, 9, 7, seed=5)
    _check('D=7 m=2 S=66000', real, gen, dev, num_subsets=66000, max_subset_size=2, seed=2)


def test_bit_identical_runs_and_permutations(dev):
    from latentaugment_amd import metrics
    real, gen = _features(700, 650, 2048, seed=77)
    ix, iy = kid_cpu.subset_indices(700, 650, 4, 300, seed=6)
    run = lambda r, g, i, j: metrics.compute_kid_from_features(r, g, device=dev, return_details=True, indices=(i, j))      # noqa: E731
    k1, d1 = run(real, gen, ix, iy)
    k2, d2 = run(real, gen, ix, iy)
    assert k1 == k2 and (d1['mmd2'] == d2['mmd2']).all() and (d1['sums'] == d2['sums']).all()
    # (a) the rows of R shuffled in memory and iy renumbered to match: every subset position holds the same feature row as before, and
    #     the order of every sum depends on positions only -> the same bits, tolerance 0.
    perm = np.random.RandomState(0).permutation(700)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(700)
    k3, d3 = run(real[perm], gen, ix, inv[iy].astype(np.int32))
    assert (real[perm][inv[iy[0]]] == real[iy[0]]).all()
    assert k3 == k1 and (d3['sums'] == d1['sums']).all() and (d3['mmd2'] == d1['mmd2']).all()
    # (b) the rows shuffled WITHIN each subset (positions change).  Every fp32 kernel value is unchanged: a dot product is one
    #     k-ordered chain whichever tile it falls in, a_k * b_k commutes, and the factor 2 of a mirrored tile is exact.  Only the
    #     float64 order changes: all terms are positive and every term passes through at most 64 (lane) + 8 (workgroup tree) +
    #     1 (tile partials, at most 256 per sum here) + 8 (tree) = 81 float64 additions, so each run is within 81 * 2^-53 of the exact
    #     sum of its terms, relatively, and two runs within twice that.
    rs = np.random.RandomState(1)
    ix4, iy4 = np.stack([rs.permutation(r) for r in ix]), np.stack([rs.permutation(r) for r in iy])
    k4, d4 = run(real, gen, ix4, iy4)
    tol = 2 * 81 * 2.0 ** -53
    rel = np.abs(d4['sums'] - d1['sums']) / d1['sums']
    print(f'KID row order within a subset: sums differ by at most {rel.max():.3e} relative (tolerance {tol:.3e})')
    assert rel.max() <= tol


def test_workspace_is_small_and_a_short_one_is_refused(dev):
    from latentaugment_amd import _lib
    lib = _lib.load()
    S, m, D = 2, 40, 16
    need = lib.la_kid_workspace_bytes(S, m, m)
    assert lib.la_kid_workspace_bytes(100, 1000, 1000) < 4_000_000 and need == S * 3 * 8
    real, gen = _features(64, 64, D, seed=3)
    x, y = torch.from_numpy(gen).to(dev), torch.from_numpy(real).to(dev)
    ix, iy = (torch.from_numpy(i).to(dev) for i in kid_cpu.subset_indices(64, 64, S, m, seed=0))
    out = torch.full([S * 4 + 1], -7.0, dtype=torch.float64, device=dev)
    ws = torch.full([need // 8], -7.0, dtype=torch.float64, device=dev)

    def call(ws_bytes):
        with torch.cuda.device(dev):
            rc = lib.la_kid_poly3_f32(_lib.ptr(x), 64, _lib.ptr(y), 64, D, _lib.ptr(ix), _lib.ptr(iy), S, m, m, _lib.ptr(out),
                                      _lib.ptr(out[S * 3:]), _lib.ptr(out[S * 4:]), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    assert call(need - 1) == -3 and b'workspace' in lib.la_last_error()          # LA_ERR_WORKSPACE
    assert (out == -7.0).all() and (ws == -7.0).all()                            # nothing was launched
    assert call(need) == 0
    ref = kid_cpu.kid(real, gen, S, m, seed=0)
    np.testing.assert_allclose(out[S * 3:S * 4].cpu().numpy(), ref['mmd2'], rtol=0, atol=1e-5 * float(ref['nsums'].max()))
    assert (ws != -7.0).all()


def test_through_feature_stats(dev):
    """FeatureStats(capture_all=True) filled by append_torch -> get_all() -> compute_kid_from_features; any float dtype is taken from
    its float32 values; the indices come back and are those of the seed."""
    from latentaugment_amd import metrics
    real, gen = _features(500, 420, 96, seed=11)
    sr, sg = metrics.FeatureStats(capture_all=True), metrics.FeatureStats(capture_all=True)
    for i in range(0, 500, 128):
        sr.append_torch(torch.from_numpy(real[i:i + 128]).to(dev))
    for i in range(0, 420, 100):
        sg.append_torch(torch.from_numpy(gen[i:i + 100]).to(dev))
    kid, det = metrics.compute_kid_from_features(sr.get_all(), sg.get_all(), num_subsets=5, max_subset_size=100, seed=4, device=dev,
                                                 return_details=True)
    assert isinstance(kid, float) and det['mmd2'].shape == (5,) and det['mmd2'].dtype == np.float64 and det['sums'].shape == (5, 3)
    assert det['ix'].shape == det['iy'].shape == (5, 100) and det['ix'].dtype == np.int32
    jx, jy = metrics.kid_subset_indices(500, 420, 5, 100, seed=4)
    assert (det['ix'] == jx).all() and (det['iy'] == jy).all() and det['ix'].max() < 420
    ref = kid_cpu.kid(real, gen, 5, 100, seed=4)
    np.testing.assert_allclose(det['mmd2'], ref['mmd2'], rtol=0, atol=1e-5 * float(ref['nsums'].max()))
    assert metrics.compute_kid_from_features(sr.get_all(), sg.get_all(), num_subsets=5, max_subset_size=100, seed=4) == kid
    assert metrics.compute_kid_from_features(real.astype(np.float64), torch.from_numpy(gen).to(dev), 5, 100, 4) == kid
    assert metrics.compute_kid_from_features(sr.get_all(), sg.get_all(), num_subsets=5, max_subset_size=100, seed=5) != kid
    h = metrics.compute_kid_from_features(torch.from_numpy(real).half(), torch.from_numpy(gen).half(), 5, 100, 4)
    assert h == pytest.approx(float(kid_cpu.kid(real.astype(np.float16), gen.astype(np.float16), 5, 100, seed=4)['kid']), abs=1e-4)
    assert kid > 0          # the generated set is the real distribution scaled by 1.05
