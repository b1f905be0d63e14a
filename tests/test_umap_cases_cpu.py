"""Without a GPU: the restatements of tests/umap_cases.py are right (Philox against the Random123 known answers, the CSR against the
dense union, trustworthiness against sklearn, find_ab_params against scipy's curve_fit), the cases reach what they claim, the
recorded figures of the whole runs are what the restatement gives with the real Philox stream, and the host side of the library
refuses what it must."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402


def test_philox_restatement_known_answers():
    kat = [((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, 0xffffffffffffffff, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0x299f31d0 << 32) | 0xa4093822, (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = uc.philox4x32_10(*[np.array([c], np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want
    from oracle import noise_ref
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, [4, 100], dtype=np.uint64)
    seed = 0x0123456789abcdef
    theirs = noise_ref.philox4x32_10(*[v.astype(np.uint32) for v in c], seed & 0xffffffff, seed >> 32)
    assert all((a == b).all() for a, b in zip(uc.philox4x32_10(*c, seed), theirs))
    # the initial layout: multiples of 10 * 2^-23 in (-10, 10), exact
    y = uc.init_layout(257, 5, 42, row0=3)
    assert (np.abs(y) < 10).all() and (y * 2.0 ** 23 / 10.0 % 1 == 0).all() and len(np.unique(y)) == y.size
    assert (uc.init_layout(4, 5, 42, row0=5) == y[2:6]).all()          # a function of the global row


@pytest.mark.parametrize('spread,min_dist', [(1.0, 0.1), (1.0, 0.0), (1.0, 0.5), (2.0, 0.25)])
def test_find_ab_params_against_curve_fit(spread, min_dist):
    pytest.importorskip('scipy.optimize')
    from latentaugment_amd.embedding import find_ab_params
    a, b = find_ab_params(spread, min_dist)
    ar, br = uc.find_ab_reference(spread, min_dist)
    print(f'find_ab_params({spread}, {min_dist}) = ({a!r}, {b!r}); relative to curve_fit {abs(a / ar - 1):.1e}, {abs(b / br - 1):.1e}')
    assert abs(a / ar - 1) <= 1e-6 and abs(b / br - 1) <= 1e-6


def test_default_ab_literals_and_no_scipy_in_the_module():
    from latentaugment_amd import embedding
    assert embedding.find_ab_params(1.0, 0.1) == (uc.A_DEFAULT, uc.B_DEFAULT)
    assert 'scipy' not in open(embedding.__file__).read().replace("scipy's curve_fit", '').replace('does not import scipy', '')
    with pytest.raises(ValueError):
        embedding.find_ab_params(0.0, 0.1)


@pytest.mark.parametrize('name', sorted(uc.graph_cases()))
def test_csr_restatement_against_the_dense_union(name):
    idx, w = uc.graph_cases()[name]
    row_ptr, col, val = uc.graph(idx, w)
    n = len(idx)
    _, S = uc.dense_union(idx, w)
    D = np.zeros([n, n])
    for i in range(n):
        c = col[row_ptr[i]:row_ptr[i + 1]]
        assert (np.diff(c) > 0).all()
        D[i, c] = val[row_ptr[i]:row_ptr[i + 1]]
    assert (D == S).all() and (D == D.T).all() and row_ptr[-1] == np.count_nonzero(S) <= 2 * idx.size
    if name == 'star':
        assert row_ptr[1] - row_ptr[0] == n - 1 > 64 and n - 1 > 2 * idx.shape[1]
    if name == 'knn65':
        A, _ = uc.dense_union(idx, w)
        assert ((A > 0) & (A.T > 0)).any() and ((A > 0) & (A.T == 0)).any()          # mutual and one-sided edges
    if name == 'empty_slots':
        assert (idx < 0).any()


def test_trustworthiness_against_sklearn():
    manifold = pytest.importorskip('sklearn.manifold')
    rng = np.random.default_rng(3)
    X = rng.standard_normal([150, 7])
    for Y, k in ((X[:, :2], 5), (rng.standard_normal([150, 2]), 15), (uc.pca(X), 10)):
        assert abs(uc.trustworthiness(X, Y, k) - manifold.trustworthiness(X, Y, n_neighbors=k)) < 1e-12


def test_smooth_knn_cases_and_their_budgets():
    for n in uc.SMOOTH_N:
        for k in uc.SMOOTH_K:
            d2, idx = uc.smooth_case(n, k)
            sk = uc.smooth_knn(d2, idx, k + 1)
            assert (idx < 0).any() == (n <= k)
            if n > 4:
                assert (d2[0, :3] == 0).all()          # duplicates: leading zero distances
            _check_smooth(sk, d2, idx, k + 1)
    d2, idx = uc.smooth_special()
    sk = uc.smooth_knn(d2, idx, 7)
    _check_smooth(sk, d2, idx, 7)
    assert (sk['w'][0] == 1).all() and (sk['w'][1] == 1).all() and sk['rho'][1] == 1.5 and sk['rho'][0] == 0
    assert (sk['w'][3] == 0).all() and sk['rho'][4] == 2.0 and sk['exact'][:5].all() and not sk['exact'][5:].any()


def _check_smooth(sk, d2, idx, n_neighbors):
    target = np.log2(n_neighbors)
    valid = idx >= 0
    x = np.where(valid, np.maximum(np.sqrt(np.where(valid, d2, 0)) - sk['rho'][:, None], 0), 0)
    free = ((x == 0) | ~valid).all(axis=1)
    # rows compared bit for bit never came near the target: their sums are exact integers or away from it by far more than eps_S
    ex = sk['exact']
    assert (free[ex] | (sk['margin'][ex] > 1000 * sk['eps_s'][ex])).all()
    # the others found a root: the final sum is at the target to within the slope times the bracket
    ne = ~ex
    if ne.any():
        s = np.where(valid[ne], np.exp(-(x[ne] / sk['mid'][ne][:, None])), 0).sum(1)
        assert (sk['sigma'][ne] >= sk['mid'][ne]).all() and (np.abs(s - target) < 1e-9).all()
        assert (sk['B_sigma'][ne] < 1e-9 * np.maximum(sk['sigma'][ne], 1e-3)).all()          # the budgets are tight, not a licence
    assert np.isfinite(sk['w']).all() and (sk['w'] <= 1).all() and (sk['w'][~valid] == 0).all()


def test_epoch_cases_reach_what_they_claim():
    seen_clip = seen_self = seen_idle = seen_zero = 0
    for name in uc.EPOCH_CASES:
        case = uc.epoch_case(name)
        n = len(case['yh'])
        yt = case['yh'] if case['yt'] is None else case['yt']
        assert n % 4 != 0 or name in ('transform',)          # n is not a multiple of the workgroup's rows
        for e in uc.EPOCH_EPOCHS:
            y, T, negs, clipped = uc.epoch(case['yh'], yt, *uc.epoch_args(case, e), detail=True)
            assert np.isfinite(y).all()
            idle = T == 0
            assert (y[idle] == case['yh'][idle]).all()
            if name == 'clip':
                seen_clip += clipped
            if name == 'small':
                seen_self += sum(int((r == h).sum()) for h, _, r in negs)
            if name == 'c2':
                act = uc.active_entries(case['row_ptr'], case['col'], case['val'], case['wmax'], e, len(yt))
                rows = np.repeat(np.arange(n), np.diff(case['row_ptr']))
                lens = np.diff(case['row_ptr'])
                seen_idle += int(((np.bincount(rows[act], minlength=n) == 0) & (lens > 0)).sum())
                assert lens[3] == 0
                j = case['col'][case['row_ptr'][1]]
                seen_zero += int((case['yh'][j] == case['yh'][1]).all())
        if name == 'star':
            assert case['row_ptr'][1] - case['row_ptr'][0] == n - 1 > 64
        if name == 'transform':
            assert case['yt'] is not None and case['row0'] != 0 and not case['skip_self'] and (case['col'] < 0).any()
    assert seen_clip > 0 and seen_self > 0 and seen_idle > 0 and seen_zero > 0
    assert uc.EPOCH_EPOCHS[0] == 0 and uc.EPOCH_EPOCHS[-1] == uc.EPOCH_E - 1 and set(c[0] for c in uc.EPOCH_CASES.values()) >= {1, 2, 3, 8}


def test_no_tested_entry_sits_on_the_edge_of_activity():
    """frac((e + 1) p) and frac(e p) of every entry of every case and tested epoch: exactly 0 with p == 1, or at least 1e-9 from an
    integer -- a device division one ulp off cannot flip an entry"""
    cases = [uc.epoch_case(name) for name in uc.EPOCH_CASES] + [uc.decode_case()]
    for case in cases:
        p = case['val'] / case['wmax']
        for e in set(uc.EPOCH_EPOCHS) | {1, 2, 3}:
            for m in (e, e + 1):
                v = m * p
                off = np.abs(v - np.round(v))
                assert (((off == 0) & ((p == 1) | (p == 0) | (m == 0))) | (off >= 1e-9)).all()          # (p == 0: an empty slot's 0 / wmax)


def test_recorded_amplification_covers_the_measured_one():
    for name in uc.EPOCH_CASES:
        case = uc.epoch_case(name)
        rng = np.random.default_rng(11)
        worst = 0.0
        for e in uc.EPOCH_EPOCHS:
            y0 = case['yh']
            y1 = y0 * (1.0 + 2.0 ** -50 * rng.choice([-1.0, 1.0], y0.shape))
            t0, t1 = (y0, y1) if case['yt'] is None else (case['yt'], case['yt'])
            d = np.abs(uc.epoch(y1, t1, *uc.epoch_args(case, e)) - uc.epoch(y0, t0, *uc.epoch_args(case, e))).max()
            worst = max(worst, d / np.abs(y1 - y0).max())
        print(f'amplification {name}: measured {worst:.1f}, recorded {uc.AMPLIFICATION[name]}')
        assert worst <= uc.AMPLIFICATION[name]


def test_decode_table_names_a_row():
    case = uc.decode_case()
    f = uc.decode_table(case)
    assert f[0] == 0 and (np.diff(f[1:]) > 1e-4).all() and (np.abs(f) < 4).all() and f[1] < -1e-2
    y, T, negs, clipped = uc.epoch(case['yh'], case['yt'], case['row_ptr'], case['col'], case['val'], 1.0, 2, uc.EPOCH_E, case['a'],
                                   case['b'], 3, case['lr'], case['seed'], case['row0'], False, detail=True)
    assert clipped == 0 and len({int(r) for _, _, rr in negs for r in rr}) > 20


@pytest.mark.parametrize('seed', uc.SHEET_SEEDS)
def test_restatement_quality_on_the_sheet(seed):
    X = uc.sheet(seed)
    fit = uc.fit_restate(X)
    t, tp = uc.trustworthiness(X, fit['y'], 15), uc.trustworthiness(X, uc.pca(X), 15)
    tr = uc.trustworthiness(X, uc.init_layout(len(X), 2, 42), 15)
    print(f'sheet {seed}: restatement {t:.4f} (recorded {uc.SHEET_TRUST[seed]}), PCA {tp:.4f} (recorded {uc.SHEET_TRUST_PCA[seed]}), random {tr:.3f}')
    assert np.isfinite(fit['y']).all()
    assert abs(t - uc.SHEET_TRUST[seed]) <= 0.005 and abs(tp - uc.SHEET_TRUST_PCA[seed]) <= 0.0005
    assert min(uc.SHEET_TRUST.values()) - 0.01 > max(uc.SHEET_TRUST_PCA.values()) and tr < 0.6


@pytest.mark.parametrize('i', range(len(uc.BLOBS)))
def test_restatement_quality_on_the_blobs(i):
    X, labels, Xq, lq = uc.blobs(i)
    fit = uc.fit_restate(X)
    yq = uc.transform_restate(fit, X, Xq)
    t = uc.trustworthiness(X, fit['y'], 15)
    pur, purq = uc.label_purity(fit['y'], labels), uc.label_purity(fit['y'], labels, 10, yq, lq)
    print(f'blobs {i}: restatement trustworthiness {t:.4f} (recorded {uc.BLOBS_TRUST[i]}), purity {pur}, of the transformed rows {purq}')
    assert np.isfinite(yq).all() and abs(t - uc.BLOBS_TRUST[i]) <= 0.005
    assert pur == purq == uc.BLOBS_PURITY[i] == 1.0


def test_scratch_size_and_refused_sizes_on_the_host():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    last = 0
    for n in (2, 3, 64, 65, 1000, 16384, 100000):
        row = [lib.la_umap_scratch_bytes(n, k) for k in (1, 2, 14, 32)]
        assert all(b >= a > 0 for a, b in zip(row, row[1:])) and row[0] >= last and (n < 64 or row[3] > row[0])
        last = row[0]
        assert row[2] >= 3 * 4 * n + 2 * n * 14 * 12
    for n, k in ((1, 5), (0, 5), (-1, 5), (10, 0), (10, 33), (1 << 30, 1), (40000000, 32)):
        assert lib.la_umap_scratch_bytes(n, k) == 0
    # argument checks come before any launch, so they answer without a device
    import ctypes as C
    buf = (C.c_double * 64)()
    p, which = C.addressof(buf), C.c_int(7)
    assert lib.la_umap_smooth_knn_f64(p, p, 4, 33, 2.0, p, p, p, None) == -1
    assert lib.la_umap_smooth_knn_f64(None, p, 4, 3, 2.0, p, p, p, None) == -1
    assert lib.la_umap_graph_f64(p, p, 1, 3, p, p, p, 6, p, p, 1 << 20, None) == -1
    assert lib.la_umap_graph_f64(p, p, 4, 3, p, p, p, 23, p, p, 1 << 20, None) == -1          # cap < 2 n k
    assert lib.la_umap_graph_f64(p, p, 4, 3, p, p, p, 24, p, p, lib.la_umap_scratch_bytes(4, 3) - 1, None) == -3
    assert lib.la_umap_init_f64(p, 4, 9, 1, 0, None) == -1
    assert lib.la_umap_epoch_f64(p, p, 4, p, 4, 2, p, p, p, 8, p, 0, 10, 1.5, 0.9, 5, 1.0, 1, 0, 1, None) == -1          # y_out is y_in
    assert lib.la_umap_epoch_f64(p, p + 256, 4, p, 4, 2, p, p, p, 8, p, 10, 10, 1.5, 0.9, 5, 1.0, 1, 0, 1, None) == -1          # e == E
    assert lib.la_umap_epoch_f64(p, p + 256, 4, p, 4, 2, p, p, p, 8, p, 0, 10, 1.5, 0.9, 33, 1.0, 1, 0, 1, None) == -1          # rate
    assert lib.la_umap_layout_f64(p, p, 4, None, 4, 2, p, p, p, 8, p, 0, 3, 10, 1.5, 0.9, 5, 1.0, 1, 0, 1, C.byref(which), None) == -1
    assert which.value == 7 and b'umap_layout' in lib.la_last_error()


def test_python_refuses_without_a_device_and_bad_options():
    from latentaugment_amd import _lib, embedding
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        embedding.LatentUMAP(device='cpu').fit(np.zeros([10, 3], np.float32))
    for kw in (dict(n_neighbors=1), dict(n_neighbors=34), dict(n_components=9), dict(negative_sample_rate=33), dict(init='spectral'),
               dict(n_epochs=0)):
        with pytest.raises(ValueError):
            embedding.LatentUMAP(**kw)
    with pytest.raises(ValueError, match='fit first'):
        embedding.LatentUMAP().transform(np.zeros([3, 3], np.float32))
