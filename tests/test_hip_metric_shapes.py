"""The precision / recall kernels and the feature moments on the GPU (la_pr_kth_f16, la_pr_member_f16, la_cdist_f16,
la_feature_moments_f64) at the C ABI and through metrics.py, against the float64 restatements of tests/criteria_cases.py.

EXACT inputs: float16 features in -2..2, so every squared distance is an integer that float32 holds exactly whatever the summation
order.  A distance must then equal float32(sqrt(float64(d^2))) to within 1 float32 ulp -- that one ulp is the whole allowance, for the
square root alone -- and a k-th radius likewise.  A squared distance of exactly 0 is clamped at 1e-30 before the root, so the expected
distance is sqrt(1e-30) rounded to float32 (about 1e-15), not 0.  Membership is tested with radii the test supplies, sqrt(q + 1/2) with
integer q: no squared distance lies on a boundary and every membership bit must be equal.  Moments on integer-valued inputs are exact in
float64: equality.
FLOAT inputs: cdist against float64 with the budget rule of test_hip_kid.py (4x the float32 CPU restatement's worst error + one float32
rounding of the largest term, carried through the root); moments with 16 x 2^-53 x sum |terms| per entry (the depth of a 50-row chain in
tiles of 16 plus the final add, with slack; products of two float32 values are exact in float64, only the order differs).
Every float case prints its err / budget ratio.

Largest measured ratio on an MI355X: moments 0.105 (D15 n50); cdist 0.194 (D48-r32-c32: err 7.856e-07 against a budget of 3.773e-06 ..
4.278e-06).  On the exact inputs every distance and every k-th radius came out as the correctly rounded root: 0 values differed in each
of the 196 printed one-ulp checks (the rule stays at 1 ulp, which is what sqrtf promises), and every membership bit was equal.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criteria_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG = -1
PR_CASES = [(D, nr, nc) for D in cc.PR_D for nr, nc in cc.PR_SHAPES]
PR_IDS = [cc.pr_case_id(*c) for c in PR_CASES]


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


def _h(x, dev):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    assert t.dtype == torch.float16 and t.data_ptr() % 16 == 0
    return t


def _ws(lib, nr, nc, dev):
    return torch.full([lib.la_pr_workspace_floats(nr, nc)], float('nan'), dtype=torch.float32, device=dev)


def _kth(lib, dev, rows, cols, k):
    nr, nc, D = rows.shape[0], cols.shape[0], rows.shape[1]
    out = torch.full([nr], float('nan'), dtype=torch.float32, device=dev)
    r, c, ws = _h(rows, dev), _h(cols, dev), _ws(lib, nr, nc, dev)          # held until the kernels have run
    rc = lib.la_pr_kth_f16(_p(r), nr, _p(c), nc, D, k, _p(out), _p(ws), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return out.cpu().numpy()


def _member(lib, dev, rows, cols, radius):
    nr, nc, D = rows.shape[0], cols.shape[0], rows.shape[1]
    out = torch.full([nr], 7, dtype=torch.uint8, device=dev)
    rad = torch.from_numpy(np.asarray(radius, np.float32)).to(dev)
    r, c, ws = _h(rows, dev), _h(cols, dev), _ws(lib, nr, nc, dev)
    rc = lib.la_pr_member_f16(_p(r), nr, _p(c), nc, D, _p(rad), _p(out), _p(ws), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    return got.astype(bool)


def _cdist(lib, dev, rows, cols):
    nr, nc, D = rows.shape[0], cols.shape[0], rows.shape[1]
    out = torch.full([nr, nc], float('nan'), dtype=torch.float32, device=dev)
    r, c, ws = _h(rows, dev), _h(cols, dev), _ws(lib, nr, nc, dev)
    rc = lib.la_cdist_f16(_p(r), nr, _p(c), nc, D, _p(out), _p(ws), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return out.cpu().numpy()


def _assert_one_ulp(name, got, want32):
    ok = cc.within_one_ulp(got, want32)
    off = int((np.asarray(got, np.float32) != want32).sum())
    print(f'{name}: {off} of {want32.size} values differ from the correctly rounded root (each by at most 1 ulp: {bool(ok.all())})')
    bad = np.argwhere(~ok)
    assert bad.size == 0, f'{name}: {len(bad)} values off by more than 1 ulp, first at {bad[0]}: {np.asarray(got)[tuple(bad[0])]} != {want32[tuple(bad[0])]}'


@pytest.mark.parametrize('D,nr,nc', PR_CASES, ids=PR_IDS)
def test_cdist_exact_and_float(lib, dev, D, nr, nc):
    name = cc.pr_case_id(D, nr, nc)
    rows, cols = cc.pr_features(nr, D, 2), cc.pr_features(nc, D, 1)
    rows[nr - 1] = cols[nc - 1]          # one exact zero, in the last row and the last column: the clamp
    want = cc.sqrt_expect32(cc.pr_dist2(rows, cols))
    assert want[nr - 1, nc - 1] == cc.sqrt_expect32(0.0) > 0
    _assert_one_ulp(f'cdist {name} exact', _cdist(lib, dev, rows, cols), want)
    rows, cols = cc.pr_features(nr, D, 4, 'float'), cc.pr_features(nc, D, 3, 'float')
    d64, d32 = cc.pr_dist(rows, cols), cc.pr_dist(rows, cols, np.float32)
    a, b = rows.astype(np.float64), cols.astype(np.float64)
    top = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    # one float32 rounding of the largest term of d^2 moves d by 2^-23 (|a|^2 + |b|^2) / (2 d); one more for the root itself
    floor = cc.EPS32 * (top / (2 * d64) + d64)
    bud = 4.0 * float(np.abs(d32 - d64).max()) + floor
    err = np.abs(_cdist(lib, dev, rows, cols) - d64)
    r = float((err / bud).max())
    print(f'cdist {name} float: err {err.max():.3e} / budget {bud.min():.3e}..{bud.max():.3e} = ratio {r:.3f}')
    assert (err <= bud).all()


@pytest.mark.parametrize('D,nr,nc', PR_CASES, ids=PR_IDS)
def test_kth_exact(lib, dev, D, nr, nc):
    """the manifold (nc points) against itself for every nhood_size it can hold, and nr other rows against it (nr != nc)"""
    name = cc.pr_case_id(D, nr, nc)
    cols, rows = cc.pr_features(nc, D, 1), cc.pr_features(nr, D, 2)
    d2_self, d2_rows = np.sort(cc.pr_dist2(cols, cols), axis=1), np.sort(cc.pr_dist2(rows, cols), axis=1)
    assert (d2_self[:, 0] == 0).all()
    for k in cc.PR_NHOOD:
        assert k + 1 <= nc
        _assert_one_ulp(f'kth {name} self k{k}' + ('-KMAX' if k + 1 == cc.PR_KMAX else ''), _kth(lib, dev, cols, cols, k), cc.sqrt_expect32(d2_self[:, k]))
        _assert_one_ulp(f'kth {name} rows k{k}', _kth(lib, dev, rows, cols, k), cc.sqrt_expect32(d2_rows[:, k]))
    want0 = np.full([nc], cc.sqrt_expect32(0.0))          # nhood_size 0: every point's own (clamped) zero
    assert (cc.sqrt_expect32(d2_self[:, 0]) == want0).all()


@pytest.mark.parametrize('D', cc.PR_D)
def test_kth_of_a_duplicated_set_is_the_clamp(lib, dev, D):
    """Every point twice: the 2nd smallest squared distance (nhood_size 1) is exactly 0.  The kernels clamp d^2 at 1e-30 before the
    root, so the radius is sqrt(1e-30) rounded to float32 -- not 0 -- and the 3rd smallest (nhood_size 2) is an ordinary distance."""
    x = cc.pr_features(65, D, 9)
    xx = np.concatenate([x, x])
    d2 = np.sort(cc.pr_dist2(xx, xx), axis=1)
    assert (d2[:, 1] == 0).all()
    clamp = cc.sqrt_expect32(0.0)
    assert 0 < clamp < 1.1e-15
    _assert_one_ulp(f'kth D{D} duplicated k1', _kth(lib, dev, xx, xx, 1), np.full([130], clamp))
    _assert_one_ulp(f'kth D{D} duplicated k2', _kth(lib, dev, xx, xx, 2), cc.sqrt_expect32(d2[:, 2]))


@pytest.mark.parametrize('D,nr,nc', PR_CASES, ids=PR_IDS)
def test_membership_every_bit(lib, dev, D, nr, nc):
    name = cc.pr_case_id(D, nr, nc)
    cols, rows = cc.pr_features(nc, D, 1), cc.pr_features(nr, D, 2)
    # (a) hand-set radii with the member fraction in [0.2, 0.8] (asserted in test_criteria_cases_cpu.py)
    for pat, rad, want in cc.member_pattern_a(rows, cols, seed=D + nr):
        got = _member(lib, dev, rows, cols, rad)
        assert (got == want).all(), f'{name} (a/{pat}): probes {np.flatnonzero(got != want)} differ; member fraction {want.mean():.2f}'
    # (b) planted copies of columns 0, 31, 32, 127, 128 and nc - 1; every radius sqrt(1/2)
    probes, planted = cc.member_pattern_b(nr, cols, seed=D + nc)
    got = _member(lib, dev, probes, cols, np.full([nc], np.sqrt(0.5), np.float32))
    assert (np.flatnonzero(got) == np.array(sorted(planted))).all(), f'{name} (b): members {np.flatnonzero(got)}, planted {planted}'
    # (c) only the last column admits anything
    rad = cc.member_pattern_c(nc)
    assert _member(lib, dev, rows, cols, rad).all(), f'{name} (c): the last column was not looked at for every probe'
    rad[nc - 1] = 0.0
    assert not _member(lib, dev, rows, cols, rad).any()


def test_pr_refusals(lib, dev):
    x = _h(cc.pr_features(40, 48, 1), dev)
    ws, kth = _ws(lib, 40, 40, dev), torch.full([40], -7.0, device=dev)
    mem, rad = torch.full([40], 7, dtype=torch.uint8, device=dev), torch.ones([40], device=dev)
    dist = torch.full([40, 40], -7.0, device=dev)

    def kth_rc(rows, nr, cols, nc, D, k):
        return lib.la_pr_kth_f16(rows, nr, cols, nc, D, k, _p(kth), _p(ws), _s())
    assert kth_rc(_p(x), 40, _p(x), 40, 48, 8) == LA_ERR_ARG and b'nhood_size' in lib.la_last_error()          # PR_KMAX
    assert kth_rc(_p(x), 40, _p(x), 40, 48, -1) == LA_ERR_ARG
    assert kth_rc(_p(x), 40, _p(x), 4, 48, 4) == LA_ERR_ARG and b'nhood_size' in lib.la_last_error()           # nhood_size + 1 > nc
    assert kth_rc(_p(x), 40, _p(x), 40, 24, 3) == LA_ERR_ARG and b'multiple of 16' in lib.la_last_error()      # D = 24 (the rows hold 48)
    assert kth_rc(_p(x), 40, _p(x), 40, 0, 3) == LA_ERR_ARG
    off = x.view(-1)[1:1 + 39 * 48]          # a base pointer 2 bytes off alignment
    assert off.data_ptr() % 16 == 2
    assert kth_rc(_p(off), 39, _p(x), 40, 48, 3) == LA_ERR_ARG and b'aligned' in lib.la_last_error()
    assert kth_rc(_p(x), 40, _p(off), 39, 48, 3) == LA_ERR_ARG and b'aligned' in lib.la_last_error()
    assert kth_rc(None, 40, _p(x), 40, 48, 3) == LA_ERR_ARG and kth_rc(_p(x), 0, _p(x), 40, 48, 3) == LA_ERR_ARG
    assert lib.la_pr_member_f16(_p(x), 40, _p(x), 40, 48, None, _p(mem), _p(ws), _s()) == LA_ERR_ARG
    assert lib.la_pr_member_f16(_p(x), 40, _p(x), 40, 40, _p(rad), _p(mem), _p(ws), _s()) == LA_ERR_ARG
    assert lib.la_pr_member_f16(_p(off), 39, _p(x), 40, 48, _p(rad), _p(mem), _p(ws), _s()) == LA_ERR_ARG
    assert lib.la_cdist_f16(_p(x), 40, _p(x), 40, 48, None, _p(ws), _s()) == LA_ERR_ARG
    assert lib.la_cdist_f16(_p(x), 40, _p(off), 39, 48, _p(dist), _p(ws), _s()) == LA_ERR_ARG
    assert lib.la_cdist_f16(_p(x), 40, _p(x), 40, 48, _p(dist), None, _s()) == LA_ERR_ARG
    torch.cuda.synchronize()
    assert (kth == -7.0).all() and (mem == 7).all() and (dist == -7.0).all()          # nothing was launched


def test_through_metrics_with_host_padding(dev):
    """D = 100 is padded to 112 on the host.  compute_distances: the 1-ulp rule.  compute_pr_from_features end to end on exact inputs:
    the radii pass through float16 there, so the float64 restatement rounds them the same way; no distance of this case is within
    80 float32 ulps of a radius it does not equal (test_criteria_cases_cpu.py), so radii, membership bits and both numbers are equal."""
    from latentaugment_amd import _lib, metrics
    real, gen = cc.pr_features(161, cc.PR_D_PADDED, 11), cc.pr_features(130, cc.PR_D_PADDED, 12)
    d = metrics.compute_distances(real, gen, device=dev).numpy()
    _assert_one_ulp('compute_distances D100', d, cc.sqrt_expect32(cc.pr_dist2(real, gen)))
    p, r, det = metrics.compute_pr_from_features(real, gen, nhood_size=3, device=dev, return_details=True)
    want = cc.pr_from_features(real, gen, 3)
    for name in ('precision', 'recall'):
        assert (det[name + '_kth'] == want[name + '_kth']).all()
        assert (det[name + '_pred'] == want[name + '_pred']).all()
    assert p == pytest.approx(want['precision'], abs=1e-6) and r == pytest.approx(want['recall'], abs=1e-6)      # a float32 mean of bits
    with pytest.raises(_lib.LatentAugHipError):
        metrics.compute_pr_from_features(real[:5], gen, nhood_size=5, device=dev)          # nc < k + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# feature moments

def _moments(lib, dev, x, mean0, cov0):
    n, D = x.shape
    mean, cov = torch.from_numpy(mean0.copy()).to(dev), torch.from_numpy(cov0.copy()).to(dev)
    xd = torch.from_numpy(x).to(dev) if n else torch.zeros([1, D], device=dev)
    rc = lib.la_feature_moments_f64(_p(xd), n, D, _p(mean), _p(cov), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize('D', cc.MOM_D)
def test_moments_add_to_preset_accumulators(lib, dev, D):
    worst = 0.0
    rs = np.random.RandomState(D)
    mean0, cov0 = rs.randint(-99, 100, size=[D]).astype(np.float64), rs.randint(-99, 100, size=[D, D]).astype(np.float64)
    for n in cc.MOM_N:
        x = cc.mom_inputs(n, D, 'exact')
        want_m, want_c, _, _ = cc.mom_restate(x, mean0, cov0)
        got_m, got_c = _moments(lib, dev, x, mean0, cov0)
        assert (got_m == want_m).all() and (got_c == want_c).all(), f'moments D{D} n{n} exact'
        x = cc.mom_inputs(n, D, 'float')
        want_m, want_c, am, ac = cc.mom_restate(x, mean0, cov0)
        got_m, got_c = _moments(lib, dev, x, mean0, cov0)
        bud_m, bud_c = 16 * 2.0 ** -53 * (am + np.abs(mean0)), 16 * 2.0 ** -53 * (ac + np.abs(cov0))
        r = max(float((np.abs(got_m - want_m) / bud_m).max()), float((np.abs(got_c - want_c) / bud_c).max()))
        print(f'moments D{D} n{n} float: mean err {np.abs(got_m - want_m).max():.3e} cov err {np.abs(got_c - want_c).max():.3e} ratio {r:.3f}')
        worst = max(worst, r)
        assert (np.abs(got_m - want_m) <= bud_m).all() and (np.abs(got_c - want_c) <= bud_c).all()
    got_m, got_c = _moments(lib, dev, np.zeros([0, D], np.float32), mean0, cov0)          # n = 0: both untouched
    assert (got_m == mean0).all() and (got_c == cov0).all()
    print(f'moments D{D}: worst ratio {worst:.3f}')


def test_moments_refusals(lib, dev):
    x, m, c = torch.zeros([4, 3], device=dev), torch.full([3], -7.0, dtype=torch.float64, device=dev), torch.full([3, 3], -7.0, dtype=torch.float64, device=dev)
    assert lib.la_feature_moments_f64(_p(x), -1, 3, _p(m), _p(c), _s()) == LA_ERR_ARG and b'feature_moments' in lib.la_last_error()
    assert lib.la_feature_moments_f64(_p(x), 4, 0, _p(m), _p(c), _s()) == LA_ERR_ARG
    assert lib.la_feature_moments_f64(_p(x), 4, 3, None, _p(c), _s()) == LA_ERR_ARG
    torch.cuda.synchronize()
    assert (m == -7.0).all() and (c == -7.0).all()


@pytest.mark.parametrize('D', [17, 33])
def test_feature_stats_appends_max_items_and_round_trip(dev, tmp_path, D):
    from latentaugment_amd import metrics
    x = cc.mom_inputs(50, D, 'exact', seed=3)
    want_m, want_c, _, _ = cc.mom_restate(x)
    one, three = metrics.FeatureStats(capture_mean_cov=True, device=dev), metrics.FeatureStats(capture_mean_cov=True, capture_all=True, device=dev)
    one.append(x)
    three.append(x[:1])
    three.append_torch(torch.from_numpy(x[1:18]).to(dev))
    three.append(x[18:])
    for st in (one, three):          # three appends of unequal size = one append of the concatenation, exactly
        assert st.num_items == 50 and (st.raw_mean == want_m).all() and (st.raw_cov == want_c).all()
    assert (three.get_all() == x).all()
    cut = metrics.FeatureStats(capture_mean_cov=True, capture_all=True, max_items=23, device=dev)
    for i in range(0, 50, 16):          # the second batch (16..31) is cut in the middle, the rest is dropped
        cut.append(x[i:i + 16])
    cm, cv, _, _ = cc.mom_restate(x[:23])
    assert cut.num_items == 23 and cut.is_full() and (cut.raw_mean == cm).all() and (cut.raw_cov == cv).all() and (cut.get_all() == x[:23]).all()
    path = str(tmp_path / 'stats.pkl')
    cut.save(path)
    back = metrics.FeatureStats.load(path, device=dev)
    assert back.num_items == 23 and back.num_features == D and back.max_items == 23 and back.is_full()
    assert (back.raw_mean == cm).all() and (back.raw_cov == cv).all() and (back.get_all() == x[:23]).all()
    mu, sig = back.get_mean_cov()
    assert np.abs(mu - x[:23].astype(np.float64).mean(0)).max() <= 1e-14 * 9
    half = metrics.FeatureStats(capture_mean_cov=True, device=dev)
    half.append(x[:20])
    half.save(path)
    more = metrics.FeatureStats.load(path, device=dev)          # the loaded accumulators are live: the kernel adds to them
    more.append(x[20:])
    assert more.num_items == 50 and (more.raw_mean == want_m).all() and (more.raw_cov == want_c).all()
