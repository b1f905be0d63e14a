"""What test_hip_knn.py relies on, shown without a GPU: the float64 restatement of tests/knn_cases.py is right, its float cases keep
the neighbours that get compared well apart, and the host entries of la_knn.hip (split rule, scratch size, argument checks) behave as
the header says.  The library loads without a GPU and every call here returns before any launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as kc  # noqa: E402

LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert 'la_knn_f32' in _lib.SIGNATURES and 'la_realism_f32' in _lib.SIGNATURES
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement

@pytest.mark.parametrize('nq,nx,D,k', kc.SMALL_CASES)
@pytest.mark.parametrize('kind', ['float', 'exact'])
def test_restatement_agrees_with_brute_force(nq, nx, D, k, kind):
    if kind == 'exact':
        q, x = kc.exact_inputs(nq, nx, D)
    else:
        both = np.random.default_rng(nq + 10 * nx).standard_normal((nq + nx, D)).astype(np.float32)
        q, x = both[:nq], both[nq:]
    d2 = kc.dist2(q, x)
    want = np.array(kc.brute_d2(q, x))
    # math.fsum is the exact sum rounded once; the wide sum then rounds twice: at most one unit in the last place apart
    assert (np.abs(d2 - want) <= np.spacing(want)).all()
    if kind == 'exact':
        assert (d2 == want).all()
    for excl in ([False, True] if nq == nx else [False]):
        dist, idx = kc.knn_from_d2(want, k, excl)
        bdist, bidx = kc.brute_knn(q, x, k, excl)
        assert (dist == bdist).all() and (idx == bidx).all()
        assert (idx[:, min(k, nx - excl):] == -1).all() and np.isinf(dist[:, min(k, nx - excl):]).all()
    radius2 = np.abs(np.random.default_rng(3).standard_normal(nx)) + 0.1
    radius2[::3] = -1.0
    s, a = kc.realism_entry_restate(q, x, radius2, d2=want)
    bs, ba = kc.brute_realism_entry(q, x, radius2)
    assert (s == bs).all() and (a == ba).all()
    s, a = kc.realism_entry_restate(q, x, np.full([nx], -1.0), d2=want)
    assert not s.any() and (a == -1).all()


def test_exact_ties_are_ordered_by_index():
    q, x = kc.exact_inputs(33, 65, 3)
    dist, idx = kc.knn_restate(q, x, 32)
    ties = 0
    for r in range(33):
        for s in range(31):
            assert dist[r, s] < dist[r, s + 1] or (dist[r, s] == dist[r, s + 1] and idx[r, s] < idx[r, s + 1])
            ties += dist[r, s] == dist[r, s + 1]
    assert ties > 100          # integer rows in -3 .. 3 with D = 3: full of ties, which is what the exact cases are for


def test_exact_case_table_reaches_every_size():
    cases = kc.exact_cases()
    assert {c[0] for c in cases} == set(kc.EXACT_N) == {c[1] for c in cases}
    assert {(c[2], c[3]) for c in cases} == {(D, k) for D in kc.EXACT_D for k in kc.EXACT_K}
    assert any(k > nx for _, nx, _, k in cases)
    assert kc.col_splits(*kc.SPLIT_CASE[:2]) > 1 and kc.SPLIT_CASE in kc.FLOAT_CASES


def test_realism_at_full_keep_is_the_float64_precision_membership():
    real, gen = kc.two_blobs()
    for nhood in (1, 3, 5):
        r = kc.realism_restate(real, gen, nhood, keep_fraction=1.0)
        member = kc.membership64(real, gen, nhood)
        assert r['kept'].all() and ((r['realism'] >= 1.0) == member).all()
        assert 0 < member.sum() < len(member)          # both answers occur
    half = kc.realism_restate(real, gen, 3, 0.5)
    assert half['kept'].sum() == 75 and half['radii'][half['kept']].max() <= half['radii'][~half['kept']].min()
    assert (half['realism'] <= kc.realism_restate(real, gen, 3, 1.0)['realism']).all()


def test_authenticity_restatement_on_copies_and_far_samples():
    real, gen = kc.two_blobs()
    a = kc.authenticity_restate(real, gen)
    assert 0.0 < a['authenticity'] < 1.0
    assert kc.authenticity_restate(real, real[10:40].copy())['authenticity'] == 0.0
    assert kc.authenticity_restate(real, real + np.float32(100.0))['authenticity'] == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the float cases: no index comparison has to be left out

@pytest.mark.parametrize('i', range(len(kc.FLOAT_CASES)))
def test_float_cases_keep_compared_neighbours_apart(i):
    """Among the first k + 1 neighbours of every query, consecutive d2 differ by more than 1000 x the largest 2B of the case: two
    evaluations within B of the exact value order them alike, so test_hip_knn.py compares every index."""
    nq, nx, D, k = kc.FLOAT_CASES[i]
    q, x = kc.float_inputs(i)
    d2 = kc.dist2(q, x)
    first = np.sort(d2, axis=1)[:, :k + 1]
    gap = float(np.diff(first, axis=1).min())
    b2 = 2.0 * float(kc.bound(q, x).max())
    print(f'knn float case {i} {kc.FLOAT_CASES[i]}: smallest gap {gap:.2e}, largest 2B {b2:.2e}, ratio {gap / b2:.2e}')
    assert gap > 1000.0 * b2
    if i == 6:          # its queries among themselves, as test_exclude_self_float runs them
        dqq = kc.dist2(q, q)
        np.fill_diagonal(dqq, np.inf)
        assert float(np.diff(np.sort(dqq, axis=1)[:, :k + 1], axis=1).min()) > 1000.0 * 2.0 * float(kc.bound(q, q).max())


@pytest.mark.parametrize('i', range(len(kc.FLOAT_CASES)))
def test_float_cases_keep_the_best_realism_quotient_apart(i):
    """best against second-best quotient radius2 / d2: their relative gap is more than 1000 x twice the relative error B / d2"""
    nq, nx, D, k = kc.FLOAT_CASES[i]
    q, x = kc.float_inputs(i)
    radius2 = kc.realism_radii(i)
    d2 = kc.dist2(q, x)
    quot = np.where(radius2[None, :] >= 0, radius2[None, :] / d2, -1.0)
    top = np.sort(quot, axis=1)[:, -2:]
    rel_gap = float(((top[:, 1] - top[:, 0]) / top[:, 1]).min())
    rel_err = 2.0 * float((kc.bound(q, x) / d2).max())
    print(f'realism float case {i}: smallest relative gap {rel_gap:.2e}, largest relative error {rel_err:.2e}')
    assert (radius2 >= 0).sum() >= 2 and (radius2 < 0).any()
    assert rel_gap > 1000.0 * rel_err


def test_two_blobs_keep_every_compared_value_apart():
    """the Python-level GPU test compares indices, kept sets, args, the realism >= 1 membership and the authenticity flags on
    knn_cases.two_blobs: each of those decisions is clear of its error bound by a factor 1000"""
    real, gen = kc.two_blobs()
    b2 = 2.0 * max(float(kc.bound(gen, real).max()), float(kc.bound(real, real).max()))
    drr = kc.dist2(real, real)
    np.fill_diagonal(drr, np.inf)
    gaps = [np.diff(np.sort(kc.dist2(gen, real), axis=1)[:, :6], axis=1).min(), np.diff(np.sort(drr, axis=1)[:, :4], axis=1).min()]
    radius2 = np.sort(drr, axis=1)[:, 2]
    # which spheres are kept.  Equal radii are those of mutual neighbours -- one pair, the same d2 bits from either side in the
    # restatement and in the library (sums and products commute, one k order) -- and go by index in both; the others are apart
    assert len(np.unique(radius2)) < len(radius2)
    gaps.append(np.diff(np.unique(radius2)).min())
    print(f'two blobs: smallest gaps {[f"{g:.2e}" for g in gaps]}, largest 2B {b2:.2e}')
    assert min(gaps) > 1000.0 * b2
    for keep in (0.5, 1.0):
        w = kc.realism_restate(real, gen, 3, keep)
        rel = 2.0 * float(kc.realism_rel_bounds(real, gen, 3, keep)['realism'].max())
        quot = np.where(w['kept'][None, :], w['radius2'][None, :] / kc.dist2(gen, real), -1.0)
        top = np.sort(quot, axis=1)[:, -2:]
        assert ((top[:, 1] - top[:, 0]) / top[:, 1]).min() > 1000.0 * rel
        assert np.abs(w['realism'] - 1.0).min() > 1000.0 * rel          # realism >= 1 is decided alike
    a = kc.authenticity_restate(real, gen)
    rel = float(kc.dist_rel_bound(gen, real, a['nearest']).max()) + float(kc.dist_rel_bound(real, real, np.argmin(drr, axis=1)).max())
    assert (np.abs(a['d_gen'] - a['d_real']) / np.maximum(a['d_gen'], a['d_real'])).min() > 1000.0 * rel


# ---------------------------------------------------------------------------------------------------------------------------------
# host entries

def test_col_splits_and_scratch_bytes(lib):
    for nq, nx in [(1, 1), (8, 1572), (3, 5000), (64, 64), (65, 64), (1572, 1572), (375, 375), (100000, 70), (70, 100000)]:
        s = lib.la_knn_col_splits(nq, nx)
        assert s == kc.col_splits(nq, nx) and 1 <= s <= min(kc.cdiv(nx, 64), 64)
    assert lib.la_knn_col_splits(8, 1572) * kc.cdiv(8, 64) >= 20          # a batch of 8 against the bank: far more than one workgroup
    assert lib.la_knn_col_splits(3, 5000) > 1
    for bad in [(0, 5), (5, 0), (-1, 5), (1 << 31, 5), (5, 1 << 31)]:
        assert lib.la_knn_col_splits(*bad) == 0
        assert lib.la_knn_scratch_bytes(bad[0], bad[1], 4, 3) == 0
    for bad in [(5, 5, 0, 3), (5, 5, 4, 0), (5, 5, 4, 33)]:
        assert lib.la_knn_scratch_bytes(*bad) == 0
    # covers the norms of both sides and one list per row, split and slot; a multiple of 8 bytes
    for nq, nx, D, k in kc.FLOAT_CASES + [(8, 1572, 4096, 5), (1572, 1572, 4096, 32)]:
        n = lib.la_knn_scratch_bytes(nq, nx, D, k)
        rows = kc.cdiv(nq, 64) * 64
        assert n % 8 == 0 and n >= 8 * (nq + nx) + 12 * rows * lib.la_knn_col_splits(nq, nx) * k
    # non-decreasing in each argument
    sizes = [1, 2, 63, 64, 65, 128, 1000, 1572, 1601, 2688, 2689, 5000, 32768, 32769, 70000]
    for other in (1, 64, 300, 2688, 40000):
        for k in (1, 5, 32):
            byq = [lib.la_knn_scratch_bytes(n, other, 16, k) for n in sizes]
            byx = [lib.la_knn_scratch_bytes(other, n, 16, k) for n in sizes]
            assert byq == sorted(byq) and byx == sorted(byx) and min(byq + byx) > 0
    byk = [lib.la_knn_scratch_bytes(300, 5000, 16, k) for k in range(1, 33)]
    byd = [lib.la_knn_scratch_bytes(300, 5000, D, 5) for D in (1, 3, 64, 4096, 100000)]
    assert byk == sorted(byk) and byd == sorted(byd)


def test_refusals_come_before_any_launch(lib):
    """one host block stands in for every device pointer: a refused call dereferences nothing"""
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    big = 1 << 40

    def knn(nq=5, nx=7, D=4, k=3, excl=0, q=p, x=p, d=p, i=p, ws=p, nbytes=big):
        return lib.la_knn_f32(q, nq, x, nx, D, k, excl, d, i, ws, nbytes, None)

    def realism(nq=5, nx=7, D=4, r=p, ws=p, nbytes=big):
        return lib.la_realism_f32(p, nq, p, nx, D, r, p, p, ws, nbytes, None)

    for kw, word in [(dict(k=0), b'k must'), (dict(k=33), b'k must'), (dict(nq=0), b'at least one row'), (dict(nx=0), b'at least one row'),
                     (dict(D=0), b'dimension'), (dict(q=None), b'null'), (dict(x=None), b'null'), (dict(d=None), b'null'),
                     (dict(i=None), b'null'), (dict(ws=None), b'null'), (dict(excl=1), b'exclude_self')]:
        assert knn(**kw) == LA_ERR_ARG, kw
        assert word in lib.la_last_error() and lib.la_last_error().startswith(b'knn:'), (kw, lib.la_last_error())
    need = lib.la_knn_scratch_bytes(5, 7, 4, 3)
    assert need > 0 and knn(nbytes=need - 1) == LA_ERR_WORKSPACE and b'la_knn_scratch_bytes' in lib.la_last_error()
    for kw, word in [(dict(nq=0), b'at least one row'), (dict(D=0), b'dimension'), (dict(r=None), b'null'), (dict(ws=None), b'null')]:
        assert realism(**kw) == LA_ERR_ARG, kw
        assert word in lib.la_last_error() and lib.la_last_error().startswith(b'realism:')
    need1 = lib.la_knn_scratch_bytes(5, 7, 4, 1)
    assert realism(nbytes=need1 - 1) == LA_ERR_WORKSPACE and b'scratch' in lib.la_last_error()
