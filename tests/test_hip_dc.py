"""Density and coverage on the GPU: la_dc_count_f16 at the C ABI and metrics.compute_dc_from_features / compute_prdc_from_features,
against the float64 restatements of tests/dc_cases.py.

EXACT inputs (float16 integers in -2..2): every squared distance is an integer that float32 holds exactly whatever the summation order,
so every count and every covered bit must be EQUAL to the restatement's -- with hand-set radii sqrt(q + 1/2) (no distance on a boundary)
and with the radii la_pr_kth_f16 returns (exact ties present: the radius is the float32 root of the same integer, and d <= r holds at
the tie).  nearest must equal float32(sqrt(float64(min d^2))) to within 1 float32 ulp: that ulp is the allowance for the root alone.
FLOAT inputs (one detector-like draw, split): a float32 kernel may differ from float64 only inside the derived bracket of
dc_cases.dc_brackets: lower <= count <= upper per generated row, covered forced where the bracket is closed (at least 95 % of the rows
and of the real samples, test_dc_cases_cpu.py).  Every float case prints how many rows and samples were forced.
Output buffers are pre-filled with garbage before every C ABI call, so a missing initialisation shows.

Measured on an MI355X (188 tests, 4.2 s): every exact case equal; every nearest distance EQUAL to the correctly rounded root (0 of
all values differ, so the 1-ulp allowance was not used); float cases: the radius error is at most 0.08 of its delta; the least forced
shares are 688 of 700 generated rows (D112, 300 x 700, k 5) and 129 of 130 real samples (D112, 130 x 161, k 1).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criteria_cases as cc  # noqa: E402
import dc_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_WORKSPACE = -3
CASES = [(D, nr, ng) for D in dc.DC_D for nr, ng in dc.DC_SHAPES] + [(dc.DC_SPLIT_D, nr, ng) for nr, ng in dc.DC_SPLIT_SHAPES]
IDS = [dc.dc_case_id(*c) for c in CASES]
FLOAT_CASES = [(D, nr, ng) for D in dc.DC_D for nr, ng in dc.DC_SHAPES]
FLOAT_IDS = [dc.dc_case_id(*c) for c in FLOAT_CASES]


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
    t = torch.tensor(np.asarray(x)).to(dev)          # a copy: the shared case inputs stay as they are
    assert t.dtype == torch.float16 and t.data_ptr() % 16 == 0
    return t


class _Call:
    """device buffers of one la_dc_count_f16 call; count, nearest and ws start as garbage"""

    def __init__(self, lib, dev, real, gen, radius):
        self.lib, self.nr, self.ng, self.D = lib, real.shape[0], gen.shape[0], real.shape[1]
        self.real, self.gen = _h(real, dev), _h(gen, dev)
        self.radius = torch.tensor(np.asarray(radius, np.float32)).to(dev)
        self.count = torch.full([self.ng], -777, dtype=torch.int32, device=dev)
        self.nearest = torch.full([self.nr], -3.0, dtype=torch.float32, device=dev)
        self.ws_bytes = lib.la_dc_workspace_bytes(self.ng, self.nr)
        self.ws = torch.full([self.ws_bytes // 4], float('nan'), dtype=torch.float32, device=dev)

    def launch(self, ws_bytes=None):
        return self.lib.la_dc_count_f16(_p(self.gen), self.ng, _p(self.real), self.nr, self.D, _p(self.radius), _p(self.count),
                                        _p(self.nearest), _p(self.ws), self.ws_bytes if ws_bytes is None else ws_bytes, _s())

    def run(self):
        rc = self.launch()
        torch.cuda.synchronize()
        assert rc == 0, self.lib.la_last_error()
        return self.count.cpu().numpy(), self.nearest.cpu().numpy()


def _dc(lib, dev, real, gen, radius):
    return _Call(lib, dev, real, gen, radius).run()


def _kth(lib, dev, real, k):
    nr, D = real.shape
    out = torch.full([nr], float('nan'), dtype=torch.float32, device=dev)
    x = _h(real, dev)
    ws = torch.full([lib.la_pr_workspace_floats(nr, nr)], float('nan'), dtype=torch.float32, device=dev)
    rc = lib.la_pr_kth_f16(_p(x), nr, _p(x), nr, D, k, _p(out), _p(ws), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return out.cpu().numpy()


def _member(lib, dev, probes, cols, radius):
    n, nc, D = probes.shape[0], cols.shape[0], cols.shape[1]
    out = torch.full([n], 7, dtype=torch.uint8, device=dev)
    rad = torch.tensor(np.asarray(radius, np.float32)).to(dev)
    r, c = _h(probes, dev), _h(cols, dev)
    ws = torch.full([lib.la_pr_workspace_floats(n, nc)], float('nan'), dtype=torch.float32, device=dev)
    rc = lib.la_pr_member_f16(_p(r), n, _p(c), nc, D, _p(rad), _p(out), _p(ws), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    return out.cpu().numpy().astype(bool)


def _assert_equal(name, count, nearest, radius, want):
    assert count.dtype == np.int32 and nearest.dtype == np.float32
    bad = np.flatnonzero(count != want['count'])
    assert bad.size == 0, f'{name}: {bad.size} counts differ, first row {bad[0]}: {count[bad[0]]} != {want["count"][bad[0]]}'
    covered = nearest <= np.asarray(radius, np.float32)
    bad = np.flatnonzero(covered != want['covered'])
    assert bad.size == 0, f'{name}: {bad.size} covered bits differ, first real {bad[0]}: nearest {nearest[bad[0]]} radius {radius[bad[0]]}'


@pytest.mark.parametrize('D,nr,ng', CASES, ids=IDS)
def test_exact_hand_set_radii(lib, dev, D, nr, ng):
    name = dc.dc_case_id(D, nr, ng)
    assert lib.la_dc_col_splits(ng, nr) == dc.dc_col_splits(ng, nr)
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    rad = dc.dc_radii_pattern(real, gen, seed=D + nr)
    want = dc.dc_from_radii(real, gen, rad)
    count, nearest = _dc(lib, dev, real, gen, rad)
    _assert_equal(name, count, nearest, rad, want)
    want32 = cc.sqrt_expect32(want['nearest_d2'])
    ok = cc.within_one_ulp(nearest, want32)
    print(f'{name}: {int((nearest != want32).sum())} of {nr} nearest distances differ from the correctly rounded root; covered '
          f'{want["covered"].mean():.2f}, mean count {want["count"].mean():.2f}')
    assert ok.all(), f'{name}: nearest off by more than 1 ulp at {np.flatnonzero(~ok)[:5]}'


@pytest.mark.parametrize('k', dc.DC_K)
@pytest.mark.parametrize('D,nr,ng', CASES, ids=IDS)
def test_exact_radii_from_the_kth_kernel(lib, dev, D, nr, ng, k):
    """ties present: every count and covered bit is equal, and count > 0 is the membership bit of la_pr_member_f16 with the same radii"""
    name = dc.dc_case_id(D, nr, ng) + f'-k{k}'
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    want = dc.dc_restate_case(nr, ng, D, 'exact', k)
    rad = _kth(lib, dev, real, k)
    assert cc.within_one_ulp(rad, want['radii'].astype(np.float32)).all()
    count, nearest = _dc(lib, dev, real, gen, rad)
    print(f'{name}: {want["ties"]} ties, density {want["density"]:.3f}, coverage {want["coverage"]:.3f}')
    _assert_equal(name, count, nearest, rad, want)
    assert ((count > 0) == _member(lib, dev, gen, real, rad)).all()


@pytest.mark.parametrize('D,nr,ng', [c for c in CASES if c[0] == 16], ids=[i for c, i in zip(CASES, IDS) if c[0] == 16])
def test_planted(lib, dev, D, nr, ng):
    name = dc.dc_case_id(D, nr, ng)
    real, gen0 = dc.dc_inputs(nr, ng, D, 'exact')
    # only the last real column admits anything, and it admits every row
    rad = dc.dc_last_column_only(nr)
    count, nearest = _dc(lib, dev, real, gen0, rad)
    assert (count == 1).all(), f'{name}: the last column was not looked at for rows {np.flatnonzero(count != 1)[:8]}'
    assert (np.flatnonzero(nearest <= rad) == [nr - 1]).all()
    rad[nr - 1] = 0.0
    count, nearest = _dc(lib, dev, real, gen0, rad)
    assert not count.any() and not (nearest <= rad).any()
    # copies of real columns on both sides of every seam are the only members, each of its own column's ball only
    gen, planted = dc.dc_planted(real, ng, seed=D + nr)
    rad = np.full([nr], np.sqrt(0.5), np.float32)
    count, nearest = _dc(lib, dev, real, gen, rad)
    assert planted[ng - 1] == nr - 1
    assert (np.flatnonzero(count) == np.array(sorted(planted))).all() and count.max() == 1, f'{name}: members {np.flatnonzero(count)}, planted {planted}'
    assert (np.flatnonzero(nearest <= rad) == np.array(sorted(planted.values()))).all()
    assert (nearest[sorted(planted.values())] == cc.sqrt_expect32(0.0)).all()          # an exact zero, clamped at 1e-30 before the root


@pytest.mark.parametrize('k', dc.DC_K)
@pytest.mark.parametrize('D,nr,ng', FLOAT_CASES, ids=FLOAT_IDS)
def test_python_entry_float_inside_the_brackets(dev, D, nr, ng, k):
    from latentaugment_amd import metrics
    name = dc.dc_case_id(D, nr, ng) + f'-k{k}'
    real, gen = dc.dc_inputs(nr, ng, D, 'float')
    b = dc.dc_brackets_case(nr, ng, D, k)
    density, coverage, det = metrics.compute_dc_from_features(real.copy(), gen.copy(), nhood_size=k, device=dev, return_details=True)
    _check_float(name, b, density, coverage, det, nr, ng, k)


def _check_float(name, b, density, coverage, det, nr, ng, k):
    assert det['radii'].dtype == np.float32 and det['count'].dtype == np.int32 and det['nearest'].dtype == np.float32
    assert det['covered'].dtype == bool and det['radii'].shape == det['nearest'].shape == det['covered'].shape == (nr,) and det['count'].shape == (ng,)
    rad_err = np.abs(det['radii'].astype(np.float64) - b['radii'])
    forced_g, forced_r = b['lower'] == b['upper'], b['cov_lower'] == b['cov_upper']
    print(f'{name}: {int(forced_g.sum())} of {ng} generated rows and {int(forced_r.sum())} of {nr} real samples forced; density {density:.4f} in '
          f'[{b["lower"].sum() / (k * ng):.4f}, {b["upper"].sum() / (k * ng):.4f}], coverage {coverage:.4f}; radius err / delta at most '
          f'{float((rad_err / b["rad_delta"]).max()):.3f}')
    assert (rad_err <= b['rad_delta']).all()
    assert (b['lower'] <= det['count']).all() and (det['count'] <= b['upper']).all()
    assert (det['covered'][forced_r] == b['cov_lower'][forced_r]).all()
    assert (b['cov_lower'] <= det['covered']).all() and (det['covered'] <= b['cov_upper']).all()
    assert (det['covered'] == (det['nearest'] <= det['radii'])).all()
    assert isinstance(density, float) and isinstance(coverage, float)
    assert density == int(det['count'].astype(np.int64).sum()) / (k * ng) and coverage == int(det['covered'].sum()) / nr
    assert int(b['lower'].sum()) / (k * ng) <= density <= int(b['upper'].sum()) / (k * ng)
    assert b['cov_lower'].mean() <= coverage <= b['cov_upper'].mean()


def test_python_entry_with_host_padding(dev):
    """D = 100 is padded to 112 on the host: zero columns change no distance; float inputs inside the brackets of the padded sum, exact
    inputs equal to the restatement as Python floats, and compute_prdc_from_features equal to the separate calls."""
    from latentaugment_amd import metrics
    nr, ng, D, k = 161, 130, dc.DC_D_PADDED, 5
    real, gen = dc.dc_inputs(nr, ng, D, 'float')
    density, coverage, det = metrics.compute_dc_from_features(real.copy(), gen.copy(), nhood_size=k, device=dev, return_details=True)
    _check_float(f'D{D}-padded', dc.dc_brackets(real, gen, k, D=112), density, coverage, det, nr, ng, k)
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    want = dc.dc_restate_case(nr, ng, D, 'exact', 3)
    got = metrics.compute_dc_from_features(torch.tensor(real).float(), torch.tensor(gen).to(dev), nhood_size=3, device=dev)
    assert got == (want['density'], want['coverage']) and want['ties'] > 0
    p, r = metrics.compute_pr_from_features(real.copy(), gen.copy(), nhood_size=3, device=dev)
    assert metrics.compute_prdc_from_features(real.copy(), gen.copy(), 3, device=dev) == dict(precision=p, recall=r, density=got[0], coverage=got[1])


@pytest.mark.parametrize('k', dc.DC_K)
@pytest.mark.parametrize('D,nr,ng', FLOAT_CASES, ids=FLOAT_IDS)
def test_python_entry_exact_equals_the_restatement(dev, D, nr, ng, k):
    from latentaugment_amd import metrics
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    want = dc.dc_restate_case(nr, ng, D, 'exact', k)
    density, coverage, det = metrics.compute_dc_from_features(real.copy(), gen.copy(), nhood_size=k, device=dev, return_details=True)
    assert (det['count'] == want['count']).all() and (det['covered'] == want['covered']).all()
    assert density == want['density'] and coverage == want['coverage']


def test_bit_identical_runs_and_row_permutations(lib, dev):
    """integer adds and minima: the same bits on every run, and after the rows of either side are shuffled in memory (un-permuted)"""
    nr, ng, D, k = 300, 700, 48, 5
    real, gen = dc.dc_inputs(nr, ng, D, 'float')
    rad = _kth(lib, dev, real, k)
    c1, n1 = _dc(lib, dev, real, gen, rad)
    c2, n2 = _dc(lib, dev, real, gen, rad)
    assert (c1 == c2).all() and (n1.view(np.uint32) == n2.view(np.uint32)).all() and c1.sum() > 0
    pr, pg = np.random.RandomState(0).permutation(nr), np.random.RandomState(1).permutation(ng)
    c3, n3 = _dc(lib, dev, real[pr], gen[pg], rad[pr])
    # a distance is one k-ordered fp32 chain of its two rows wherever the pair falls in the grid, and a_k * b_k commutes
    assert (c3 == c1[pg]).all() and (n3.view(np.uint32) == n1[pr].view(np.uint32)).all()


def test_graph_capture_and_replay(lib, dev):
    """la_dc_count_f16 captured on one stream (its initialisation is stream work), replayed after the inputs changed: the eager bits"""
    nr, ng, D = 257, 130, 48
    real, gen = dc.dc_inputs(nr, ng, D, 'float')
    real2, gen2 = dc.dc_inputs(nr, ng, D, 'exact')
    rad, rad2 = _kth(lib, dev, real, 5), _kth(lib, dev, real2, 5)
    want1, want2 = _dc(lib, dev, real, gen, rad), _dc(lib, dev, real2, gen2, rad2)
    call = _Call(lib, dev, real, gen, rad)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call.launch()
    assert rc == 0, lib.la_last_error()
    torch.cuda.synchronize()
    for want, (r, g, ra) in ((want1, (real, gen, rad)), (want2, (real2, gen2, rad2)), (want1, (real, gen, rad))):
        call.real.copy_(torch.tensor(r))
        call.gen.copy_(torch.tensor(g))
        call.radius.copy_(torch.tensor(ra))
        call.count.fill_(-777)
        call.nearest.fill_(-3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert (call.count.cpu().numpy() == want[0]).all()
        assert (call.nearest.cpu().numpy().view(np.uint32) == want[1].view(np.uint32)).all()
    assert (want1[0] != want2[0]).any()


def test_a_short_workspace_is_refused_and_the_next_call_succeeds(lib, dev):
    nr, ng, D = 130, 161, 16
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    rad = dc.dc_radii_pattern(real, gen, seed=D + nr)
    call = _Call(lib, dev, real, gen, rad)
    assert call.ws_bytes == (nr + ng) * 4
    rc = call.launch(call.ws_bytes - 1)
    torch.cuda.synchronize()
    assert rc == LA_ERR_WORKSPACE and b'workspace' in lib.la_last_error()
    assert (call.count == -777).all() and (call.nearest == -3.0).all() and torch.isnan(call.ws).all()          # nothing was launched
    count, nearest = call.run()
    _assert_equal('after the refusal', count, nearest, rad, dc.dc_from_radii(real, gen, rad))
