"""The yardsticks of the style / content distance on the host: the float64 restatement of tests/nst_cases.py against the reference's
recorded values (tests/golden/nst.npz), the proofs behind the case table of the direct entry, and the pure-host queries
(la_gram_pair_scratch_bytes, la_gram_pair_slices).  Nothing here needs a GPU.

Measured here: the D / S restatement against the reference's float64 run, 1.4e-13 relative at worst over both sizes; a float32 numpy run
of the restatement uses at most 0.08 of the analytic style bound (C = 4, HW = 1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nst_cases as nc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'nst.npz'))


@pytest.mark.parametrize('R', [32, 48])
def test_restatement_reproduces_the_reference_float64(fx, R):
    """The D / S form, E = D S^T + S D^T, gives the reference's float64 style and content of every pair, modality and tap to 1e-12
    relative, and so does the reference's own expression restated: the fixture holds what the docstring of nst_cases says it holds."""
    x, y = fx[f'nst{R}_x'], fx[f'nst{R}_y']
    style64, content64 = fx[f'nst{R}_style64'], fx[f'nst{R}_content64']
    assert style64.shape == content64.shape == (3, 2, 5)
    worst = 0.0
    for p in range(3):
        for mode in range(2):
            tx, ty = nc.fixture_taps(fx, x[p], mode), nc.fixture_taps(fx, y[p], mode)
            assert [t.shape[1] for t in tx] == [R * R, (R // 2) ** 2, (R // 4) ** 2, (R // 8) ** 2, (R // 16) ** 2]
            for t in range(5):
                assert float(tx[t].min()) == 0.0          # the tapped tensors are post-ReLU
                s, c = nc.restate_pair64(tx[t].numpy(), ty[t].numpy())
                s_ref, c_ref = nc.reference_form(tx[t].numpy(), ty[t].numpy())
                for got, want in ((s, style64[p, mode, t]), (c, content64[p, mode, t]), (s_ref, style64[p, mode, t]), (c_ref, content64[p, mode, t])):
                    worst = max(worst, abs(got - want) / abs(want))
    print(f'R {R}: restatement vs the reference float64, worst relative {worst:.2e}')
    assert worst <= 1e-12


def test_fixture_inputs_are_what_the_tests_need(fx):
    for R in (32, 48):
        x, y = fx[f'nst{R}_x'], fx[f'nst{R}_y']
        assert x.shape == y.shape == (3, 2, R, R) and x.dtype == np.float32
        assert np.abs(x).max() <= 1.0 and np.abs(y).max() <= 1.0
        assert (x > 127 / 127.5).sum() + (y > 127 / 127.5).sum() > 0          # the clamp acts
        assert np.abs(y[0] - x[0]).max() <= 0.0201 and np.abs(y[1] - x[1]).max() > 0.5          # pair 0 is close
    assert nc.CONV_IDS[-1] == 28 and (32 // 16) ** 2 == 4 and (48 // 16) ** 2 == 9          # HW = 4 and HW = 9 at the last tap


@pytest.mark.parametrize('C,HW', nc.CASES)
def test_integer_cases_are_exact_by_construction(C, HW):
    """|E| <= 32 HW < 2^24 (every float32 partial sum an exact integer) and C^2 (32 HW)^2 < 2^53 (the float64 sum of squares exact)."""
    assert 32 * HW < 2 ** 24 and C * C * (32 * HW) ** 2 < 2 ** 53
    f = nc.int_inputs(C, HW, 3)
    D, S = nc.split(f)
    assert np.abs(D).max() <= 4 and np.abs(S).max() <= 4 and np.abs(nc.gram_diff(D, S, np.float64)).max() <= 32 * HW
    s32, c32 = nc.restate(f, np.float32)          # exact in float32 too (the sums stay below 2^24 only for the small cases: compare those)
    s64, c64 = nc.restate(f)
    if C * C * (32 * HW) ** 2 < 2 ** 24:
        assert s32.tobytes() == s64.tobytes() and c32.tobytes() == c64.tobytes()


@pytest.mark.parametrize('C,HW', nc.CASES)
def test_float32_restatement_lies_inside_the_analytic_bound(C, HW):
    f = nc.float_inputs(C, HW)
    s64, c64 = nc.restate(f)
    D, S = nc.split(f)
    E32 = nc.gram_diff(D, S, np.float32).astype(np.float64)          # float32 products and sums, then the float64 finish of the kernel
    s32 = (E32 * E32).sum(axis=(1, 2)) / (4.0 * HW * HW * C * C)
    sb, cb = nc.bounds(f)
    assert s64[2] == 0.0 and c64[2] == 0.0 and sb[2] == 0.0 and s32[2] == 0.0          # the identical pair
    assert (sb[:2] > 0).all() and (np.abs(s32 - s64) <= sb).all()
    print(f'C {C} HW {HW}: float32 style error / bound {np.max(np.abs(s32 - s64)[:2] / sb[:2]):.3f}; bound / style {np.max(sb[:2] / s64[:2]):.2e}')


def test_case_table_reaches_every_path(lib):
    """The shapes are chosen with the kernel's own tile edges and slice rule: a ragged single tile, exactly one (of either edge, and
    the first C past the small edge), one plus 4 (two tile rows), three tile rows; HW below a K chunk, odd, and one with >= 3 slices whose last is shorter; the mirror of the slice rule in
    nst_cases is the library's."""
    T, TS = nc.TILE, nc.TILE_SMALL
    assert {C for C in nc.CHANNELS if C < TS} >= {4, 12} and T in nc.CHANNELS and T + 4 in nc.CHANNELS and max(nc.CHANNELS) > 2 * T
    assert TS in nc.CHANNELS and TS + 1 in nc.CHANNELS          # both sides of the threshold between the two tile edges
    assert {1, 4, 9, 33} <= set(nc.PIXELS) and min(nc.PIXELS) < nc.KC
    for C in nc.CHANNELS:
        ks, per, nchunk = nc.slices(C, nc.HW_SPLIT)
        assert ks >= 3 and nchunk - (ks - 1) * per < per and nc.HW_SPLIT % nc.KC != 0
    for C in list(nc.CHANNELS) + [64, 256, 512, 2048]:
        for HW in list(nc.PIXELS) + [256, 1024, 4096, 16384, 65536]:
            assert lib.la_gram_pair_slices(C, HW) == nc.slices(C, HW)[0], (C, HW)
    assert lib.la_gram_pair_slices(64, 65536) > 1          # a single tile per pair: split-K fills the chip


def test_pure_host_queries(lib):
    """Refusals return 0; the scratch is non-decreasing in P; the slices do not depend on P (the entry has no P to depend on, and the
    scratch grows linearly: the same per-pair layout at every P)."""
    for bad in ((0, 8, 16), (-1, 8, 16), (1, 0, 16), (1, 8, 0), (1, -4, 16), (1, 8, -1), (65536, 8, 16), (1, 8193, 16), (1, 8, (1 << 26) + 1)):
        assert lib.la_gram_pair_scratch_bytes(*bad) == 0, bad
    assert lib.la_gram_pair_slices(0, 16) == 0 and lib.la_gram_pair_slices(8, 0) == 0 and lib.la_gram_pair_slices(8193, 4) == 0
    for C, HW in nc.CASES + [(64, 65536), (512, 256)]:
        sizes = [lib.la_gram_pair_scratch_bytes(P, C, HW) for P in range(1, 40)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), (C, HW)
        ks = lib.la_gram_pair_slices(C, HW)
        edge = nc.TILE_SMALL if C <= nc.TILE_SMALL else nc.TILE
        tw = min(C, edge)
        T = -(-C // edge)
        assert sizes[7] >= 8 * ks * (T * (T + 1) // 2) * tw * tw * 4          # P = 8: at least the float32 slice partials
