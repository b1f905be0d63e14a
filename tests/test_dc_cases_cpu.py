"""Density and coverage without a GPU: the properties of the float64 restatement (tests/dc_cases.py) that test_hip_dc.py leans on, proof
that the case tables reach what they claim, and the host side of la_dc_count_f16 / metrics.compute_dc_from_features (the header, the
exported symbols, the workspace and chunk queries, every argument error).

Figures of the cases as they stand (printed by the tests; seeds in dc_cases.py):
  exact cases: density 0.60 .. 1.58, coverage 0.11 .. 1.0 over every shape x D x k; ties in 44 of the 52 cases, e.g. 106 pairs at
        (nr, ng) = (130, 161), D 16, k 5
  float cases (one draw, seed 21, split): share of generated rows / of real samples whose bracket is closed (lower == upper):
        at least 98.3 % / 99.2 % over every listed shape x D x k; the condition asserted is 95 % of each.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criteria_cases as cc  # noqa: E402
import dc_cases as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(D, nr, ng) for D in dc.DC_D for nr, ng in dc.DC_SHAPES] + [(dc.DC_SPLIT_D, nr, ng) for nr, ng in dc.DC_SPLIT_SHAPES]
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


def _lib_built():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement

def _dyadic_features(n, D, seed):
    """detector-like float16 rows rounded to multiples of 2^-8 below 4: every product and every sum of pr_dist2 is exact in float64, so
    the distance matrix of a set with itself is symmetric to the bit on any machine"""
    x = np.round(cc.pr_features(n, D, seed, 'float').astype(np.float64) * 256) / 256
    assert np.abs(x).max() < 4
    x16 = x.astype(np.float16)
    assert (x16.astype(np.float64) == x).all()
    return x16


def test_identical_sets_are_covered_and_dense():
    """gen == real: every real sample holds itself (coverage 1) and every ball holds at least its k + 1 defining points; where no two
    distances of a row are equal every ball holds exactly k + 1 and density is (k + 1) / k."""
    for k in dc.DC_K:
        x = cc.pr_features(90, 48, 5, 'exact')
        r = dc.dc_restate(x, x, k)
        assert r['coverage'] == 1.0 and int(r['count'].sum()) >= 90 * (k + 1)
        x = _dyadic_features(40, 112, 5)
        d = cc.pr_dist(x, x)
        assert (d == d.T).all() and (np.diff(np.sort(d, axis=1), axis=1) > 0).all()
        r = dc.dc_restate(x, x, k)
        assert r['coverage'] == 1.0 and int(r['count'].sum()) == 40 * (k + 1) and r['density'] == (k + 1) / k
        assert r['ties'] == 40          # each ball's own k-th neighbour lies on its boundary, and nothing else does


def test_far_away_generated_points_give_zero():
    real = cc.pr_features(70, 48, 5, 'float')
    gen = (cc.pr_features(50, 48, 6, 'float').astype(np.float32) + 100).astype(np.float16)
    r = dc.dc_restate(real, gen, 5)
    assert r['density'] == 0.0 and r['coverage'] == 0.0 and not r['count'].any() and not r['covered'].any()


def test_positive_counts_are_the_precision_bits():
    for kind in ('exact', 'float'):
        real, gen = dc.dc_inputs(130, 161, 48, kind)
        r = dc.dc_restate(real, gen, 5)
        assert ((r['count'] > 0) == cc.pr_member(gen, real, r['radii'])).all()
        assert 0 < (r['count'] > 0).mean() < 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the case tables

def test_exact_cases_are_inside_the_open_range_and_some_have_ties():
    ties, dens, cov = {}, [], []
    for D, nr, ng in CASES:
        for k in dc.DC_K:
            r = dc.dc_restate_case(nr, ng, D, 'exact', k)
            assert 0 < r['density'] < 2 and 0 < r['coverage'] <= 1, (D, nr, ng, k, r['density'], r['coverage'])
            ties[(D, nr, ng, k)] = r['ties']
            dens.append(r['density'])
            cov.append(r['coverage'])
    print(f'exact cases: density {min(dens):.2f} .. {max(dens):.2f}  coverage {min(cov):.2f} .. {max(cov):.2f}')
    print('exact cases with ties:', {key: v for key, v in ties.items() if v})
    assert sum(1 for v in ties.values() if v) >= 1
    # at a tie <= and prdc's < give different counts: the restatement with < is a different answer
    D, nr, ng, k = max(ties, key=ties.get)
    real, gen = dc.dc_inputs(nr, ng, D, 'exact')
    r = dc.dc_restate_case(nr, ng, D, 'exact', k)
    strict = (cc.pr_dist(gen, real) < r['radii'][None, :]).sum(axis=1)
    assert int(r['count'].sum()) - int(strict.sum()) == r['ties'] > 0


def test_float_cases_close_their_brackets():
    """95 % of the generated rows and 95 % of the real samples of every float case have lower == upper: the float32 kernel is pinned
    there, and the case is not degenerate (something is inside a ball, something is not)."""
    worst_g, worst_r = 1.0, 1.0
    for D in dc.DC_D:
        for nr, ng in dc.DC_SHAPES:
            for k in dc.DC_K:
                b = dc.dc_brackets_case(nr, ng, D, k)
                r = dc.dc_restate_case(nr, ng, D, 'float', k)
                assert (b['lower'] <= r['count']).all() and (r['count'] <= b['upper']).all()
                assert (b['cov_lower'] <= r['covered']).all() and (r['covered'] <= b['cov_upper']).all()
                sg, sr = float((b['lower'] == b['upper']).mean()), float((b['cov_lower'] == b['cov_upper']).mean())
                worst_g, worst_r = min(worst_g, sg), min(worst_r, sr)
                assert sg >= 0.95 and sr >= 0.95, (D, nr, ng, k, sg, sr)
                if ng > 1:          # a single generated row may lie in no ball
                    assert 0 < r['density'] and 0 < r['coverage'], (D, nr, ng, k)
    print(f'float cases: closed brackets on at least {100 * worst_g:.1f} % of the generated rows and {100 * worst_r:.1f} % of the real samples')


def test_hand_set_radii_split_the_real_samples():
    for D, nr, ng in CASES:
        real, gen = dc.dc_inputs(nr, ng, D, 'exact')
        r = dc.dc_from_radii(real, gen, dc.dc_radii_pattern(real, gen, seed=D + nr))
        assert r['ties'] == 0 and 0 < r['covered'].mean() < 1 and r['count'].sum() > 0, (D, nr, ng)


def test_planted_cases_hold_exactly_the_planted_pairs():
    for D, nr, ng in CASES:
        real, _ = dc.dc_inputs(nr, ng, D, 'exact')
        gen, planted = dc.dc_planted(real, ng, seed=D + nr)
        assert planted[ng - 1] == nr - 1 and len(set(planted.values())) == len(planted)
        r = dc.dc_from_radii(real, gen, np.full([nr], np.sqrt(0.5), np.float32))
        assert (np.flatnonzero(r['count']) == np.array(sorted(planted))).all() and r['count'].max() == 1
        assert (np.flatnonzero(r['covered']) == np.array(sorted(planted.values()))).all()
        if ng > 128 and nr > 128:
            assert {0, 31, 32, 127, 128} <= set(planted) and {0, 31, 32, 127, 128} <= set(planted.values())
        r = dc.dc_from_radii(real, gen, dc.dc_last_column_only(nr))
        assert (r['count'] == 1).all() and (np.flatnonzero(r['covered']) == [nr - 1]).all()


def test_shapes_sit_on_both_sides_of_the_chunk_rule():
    """one chunk and more than one; a chunk of one and of several 128-column steps; a short last chunk; agreement with the library"""
    lib = _lib_built()
    seen = set()
    for D, nr, ng in CASES:
        s, chunk = dc.dc_col_splits(ng, nr), dc.dc_chunk_cols(ng, nr)
        assert lib.la_dc_col_splits(ng, nr) == s, (nr, ng)
        assert chunk % 128 == 0 and (s - 1) * chunk < nr <= s * chunk
        seen.add(('one' if s == 1 else 'many', 'step1' if min(chunk, nr) <= 128 else 'steps', 'short' if s > 1 and nr % chunk else 'even'))
    print(sorted(seen))
    assert {('one', 'step1', 'even'), ('one', 'steps', 'even'), ('many', 'step1', 'short'), ('many', 'steps', 'short')} <= seen
    assert lib.la_dc_col_splits(1572, 1572) == dc.dc_col_splits(1572, 1572) == 13          # 13 x 13 = 169 workgroups, not 13
    assert lib.la_dc_col_splits(10000, 10000) == dc.dc_col_splits(10000, 10000) == 7         # 79 x 7 = 553, the last chunk 7 of 12 steps
    assert lib.la_dc_col_splits(0, 5) == 0 and lib.la_dc_col_splits(5, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side

def test_symbols_declared_and_exported():
    from latentaugment_amd import _lib
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    lib = _lib_built()
    for name in ('la_dc_count_f16', 'la_dc_workspace_bytes', 'la_dc_col_splits'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), f'{name} is not declared in include/latentaug_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by the library'
    P, I, L = C.c_void_p, C.c_int, C.c_long
    assert _lib.SIGNATURES['la_dc_workspace_bytes'] == (C.c_size_t, [L, L])
    assert _lib.SIGNATURES['la_dc_col_splits'] == (I, [L, L])
    assert _lib.SIGNATURES['la_dc_count_f16'] == (I, [P, L, P, L, I, P, P, P, P, C.c_size_t, P])


def test_workspace_query_and_host_argument_checks():
    """Pure host code: the workspace stays far below one float32 ng x nr matrix, and bad arguments are refused before any launch (so this
    runs without a device: nothing reaches the HIP runtime)."""
    lib = _lib_built()
    assert lib.la_dc_workspace_bytes(10000, 10000) == 80000 < 10000 * 10000 * 4 // 1000
    assert lib.la_dc_workspace_bytes(1, 9) == 40
    assert lib.la_dc_workspace_bytes(0, 9) == 0 and lib.la_dc_workspace_bytes(9, 0) == 0
    p = 4096          # a non-null, aligned address: every call below is refused before it is looked at
    ok = dict(gen=p, ng=10, real=p, nr=10, D=16, radius=p, count=p, nearest=p, ws=p, ws_bytes=1 << 20)
    for change, code, word in ((dict(gen=None), LA_ERR_ARG, 'null'), (dict(real=None), LA_ERR_ARG, 'null'), (dict(radius=None), LA_ERR_ARG, 'null'),
                               (dict(count=None), LA_ERR_ARG, 'null'), (dict(nearest=None), LA_ERR_ARG, 'null'), (dict(ws=None), LA_ERR_ARG, 'null'),
                               (dict(ng=0), LA_ERR_ARG, 'at least one row'), (dict(nr=0), LA_ERR_ARG, 'at least one row'),
                               (dict(nr=-3), LA_ERR_ARG, 'at least one row'),
                               (dict(D=0), LA_ERR_ARG, 'multiple of 16'), (dict(D=24), LA_ERR_ARG, 'multiple of 16'),
                               (dict(gen=p + 2), LA_ERR_ARG, '16-byte aligned'), (dict(real=p + 8), LA_ERR_ARG, '16-byte aligned'),
                               (dict(radius=p + 2), LA_ERR_ARG, '4-byte aligned'), (dict(ws=p + 1), LA_ERR_ARG, '4-byte aligned'),
                               (dict(ws_bytes=79), LA_ERR_WORKSPACE, 'workspace'), (dict(ws_bytes=0), LA_ERR_WORKSPACE, 'workspace')):
        a = dict(ok, **change)
        rc = lib.la_dc_count_f16(a['gen'], a['ng'], a['real'], a['nr'], a['D'], a['radius'], a['count'], a['nearest'], a['ws'], a['ws_bytes'],
                                 None)
        assert rc == code, (change, rc)
        assert word in lib.la_last_error().decode(), (change, lib.la_last_error())


def test_cpu_device_and_nhood_range_are_refused():
    from latentaugment_amd import _lib, metrics
    real, gen = dc.dc_inputs(33, 31, 16, 'float')
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_dc_from_features(real, gen, device='cpu')
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        metrics.compute_dc_from_features(torch.tensor(real), torch.tensor(gen), nhood_size=3, device=torch.device('cpu'))
    for real_n, k in ((33, 0), (33, 8), (33, -1), (5, 5), (2, 2), (1, 1), (33, 2.5)):
        with pytest.raises(ValueError, match='nhood_size'):
            metrics.compute_dc_from_features(real[:real_n], gen, nhood_size=k)
    with pytest.raises(ValueError, match='one D'):
        metrics.compute_dc_from_features(real, gen[:, :8])
    assert callable(metrics.compute_prdc_from_features)
