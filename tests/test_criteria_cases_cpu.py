"""The case tables of tests/criteria_cases.py are what the sweep needs, and its float64 restatements are right without any kernel:
they agree with the oracle, with the reference's goldens, and with plain definitions; every 'exact' input stays below 2^24 and its
float32 evaluation equals the float64 one; the membership patterns have the member fractions and separations the GPU test relies on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criteria_cases as cc  # noqa: E402

from oracle import latent_aug_ref as lar  # noqa: E402
from oracle import metrics_ref as mr  # noqa: E402
from oracle import sg2_networks as nets  # noqa: E402


def test_tables_hold_the_listed_values():
    assert set(cc.L2_K) >= {1, 3, 4, 255, 256, 257, 1024, 1025, 1028, 4096, 4100, 16384, 16385, 16388, 32761}
    assert set(cc.L2_NM) >= {(1, 1), (7, 9), (8, 8), (9, 7), (17, 64)} and len(cc.L2_CASES) == len(cc.L2_K) * len(cc.L2_NM)
    assert cc.L2_PREDICATE_PAIR == [(3, 1016, 16388), (3, 1017, 16388)]
    assert set(cc.PR_D) >= {16, 48, 112} and cc.PR_D_PADDED == 100 and cc.PR_D_PADDED % 16 != 0
    assert set(cc.PR_SHAPES) >= {(1, 9), (31, 33), (32, 32), (33, 127), (129, 128), (161, 130), (130, 257)}
    assert set(cc.PR_NHOOD) >= {0, 1, 3, 7} and max(cc.PR_NHOOD) + 1 == cc.PR_KMAX
    assert set(cc.MOM_D) >= {1, 15, 16, 17, 33} and set(cc.MOM_N) >= {1, 15, 16, 17, 50}
    assert set(cc.FC_IN) >= {1, 63, 64, 65, 512, 2044, 2047, 2048, 2052, 4100}
    assert set(cc.FC_OUT) >= {1, 4, 5} and set(cc.FC_B) >= {1, 8, 9, 17} and set(cc.FC_LR_MUL) >= {1.0, 0.01}
    assert {a for _, a in cc.FC_ACT} == {'linear', 'lrelu'}
    assert set(cc.MAP_DIMS) >= {(64, 64), (40, 72), (72, 40)} and set(cc.MAP_LAYERS) >= {0, 2, 8} and set(cc.MAP_B) >= {1, 9}
    assert set(cc.MAP_PSI) >= {1.0, 0.7} and set(cc.MAP_NUM_WS) >= {1, 6}
    assert set(cc.CENTER_CROP) >= {(32, 23, 5), (33, 23, 5), (16, 16, 0), (16, 1, 15)} and set(cc.CENTER_PLANES) >= {1, 6}
    assert set(cc.CROP_REP) >= {1, 3, 4} and set(cc.CROP_IMGC) >= {1, 2} and set(cc.CROP_B) >= {1, 3}
    assert any(y0 + S == R and x0 + S == R and S < R for R, S, y0, x0 in cc.CROP_WINDOWS)          # touches the last row and column
    assert set(cc.ADAM_N) >= {1, 256, 257, 1000} and cc.ADAM_STEPS == 5


def test_pairwise_plan_reaches_every_branch():
    plan = {(K, n, m): cc.l2_plan(K, n, m) for K, n, m in cc.L2_CASES}
    occ = {p['occupancy'] for p in plan.values()}
    assert {p['vec'] for p in plan.values()} == {True, False}
    assert {p['ksplit'] for p in plan.values()} == {4, 16}
    assert 'FFFF' in occ and any('P' in o for o in occ) and any(o.endswith('EE') for o in occ)          # full, partial, two empty slices
    assert any(o[0] == 'P' and set(o[1:]) == {'E'} for o in occ)          # all of K in slice 0: what the goldens reach
    assert any(o.startswith('FF') and 'P' in o for o in occ)              # data in slices 1..3 and a clamped kend behind them
    # the named example of the issue: K = 4100 in float4 form is two full slices, four elements in the third, an empty fourth
    p = cc.l2_plan(4100, 7, 9)
    assert p['vec'] and p['kper'] == 2048 and p['occupancy'] == 'FFPE' and 'K4100-vec-ks4-full+partial+empty-slice' in cc.l2_case_id(4100, 7, 9)
    # rounding kper down instead of up (1024) would leave elements 4096..4099 to no slice
    assert 4 * ((cc.cdiv(4100, 4) // 1024) * 1024) < 4100
    # both sides of K > 16384, in both forms
    assert cc.l2_plan(16384, 8, 8)['ksplit'] == 4 and cc.l2_plan(16385, 8, 8)['ksplit'] == 16 and cc.l2_plan(16388, 8, 8)['ksplit'] == 16
    assert not cc.l2_plan(16385, 8, 8)['vec'] and cc.l2_plan(16388, 8, 8)['vec'] and not cc.l2_plan(32761, 8, 8)['vec']
    # the other half of the predicate
    (n, m0, K), (_, m1, _) = cc.L2_PREDICATE_PAIR
    assert cc.l2_plan(K, n, m0)['ksplit'] == 16 and cc.l2_plan(K, n, m1)['ksplit'] == 4
    # the n0 chunk loop: one pass, a ragged pass, exactly full, a second ragged pass, three passes
    assert {(p['passes'], p['ragged_n']) for p in plan.values()} >= {(1, True), (1, False), (2, True), (3, True)}
    assert {p['ragged_m'] for p in plan.values()} == {True, False}
    assert not cc.l2_plan(1024, 7, 9, aligned=False)['vec'] and 'scalar-unaligned' in cc.l2_case_id(1024, 7, 9, aligned=False)
    ids = [cc.l2_case_id(*c) for c in cc.L2_CASES]
    assert len(set(ids)) == len(ids)


def test_pairwise_restatement_is_the_oracle_and_the_golden(golden_dir):
    gc = np.load(os.path.join(golden_dir, 'criteria.npz'))
    for tag in ('2d', '3d', '4d'):
        X, Y = gc[f'G5_{tag}_X'], gc[f'G5_{tag}_Y']
        D, mean, _ = cc.l2_restate(X, Y, np.float64)
        o_full = lar.l2_loss_vectorized(torch.from_numpy(X).double(), torch.from_numpy(Y).double(), compute_mean=False).numpy()
        o_mean = float(lar.l2_loss_vectorized(torch.from_numpy(X).double(), torch.from_numpy(Y).double()))
        scale = np.abs(o_full).max()
        assert np.abs(D - o_full).max() <= 1e-13 * scale and abs(mean - o_mean) <= 1e-13 * abs(o_mean)
        np.testing.assert_allclose(D, gc[f'G5_{tag}_full'], rtol=1e-5, atol=1e-4)          # the golden is float32
        np.testing.assert_allclose(mean, gc[f'G5_{tag}_mean'], rtol=1e-5)
        assert np.abs(D - cc.l2_direct(X, Y)).max() <= 1e-12 * scale
        D32, mean32, _ = cc.l2_restate(X, Y, np.float32)
        assert D32.dtype == np.float32 and type(mean32) is np.float32


@pytest.mark.parametrize('n,m', cc.L2_NM + [(3, 1017)])
def test_pairwise_exact_inputs_are_exact_in_float32(n, m):
    for K in cc.L2_K if m < 1000 else [16388]:
        X, Y = cc.l2_inputs(K, n, m, 'exact')
        assert np.abs(X).max() <= 3 and np.abs(Y).max() <= 3 and (X == np.rint(X)).all()
        D64, _, top = cc.l2_restate(X, Y, np.float64)
        D32, _, _ = cc.l2_restate(X, Y, np.float32)
        assert 36 * K < cc.TWO24 and D64.max() <= 36 * K and top <= 18 * K
        assert (D32.astype(np.float64) == D64).all() and (D64 == cc.l2_direct(X, Y)).all()
        Xf, Yf = cc.l2_inputs(K, n, m, 'float')
        assert abs(Xf.mean()) > 0.05 or K < 16
        assert (Xf < 0).any() and (Xf > 0).any() or K < 4


def test_pr_restatement_reproduces_the_oracle_on_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'metrics.npz'))
    for case in ('a', 'b'):
        real, gen = g[f'{case}_real'], g[f'{case}_gen']
        ref = mr.precision_recall_from_features(real, gen, nhood_size=3)
        got = cc.pr_from_features(real, gen, 3)
        for name in ('precision', 'recall'):
            # float64 against torch's float32 cdist: a radius may round to the neighbouring float16 (2^-10 relative)
            np.testing.assert_allclose(got[name + '_kth'], ref[name + '_kth'], rtol=2.0 ** -10, atol=0)
            assert (got[name + '_kth'] != ref[name + '_kth']).mean() <= 0.01
            assert (got[name + '_pred'] != ref[name + '_pred']).mean() <= 0.005
            assert got[name] == pytest.approx(float(g[f'{case}_{name}']), abs=0.005)
        d = cc.pr_dist(real[:40].astype(np.float16), gen[:50].astype(np.float16))
        np.testing.assert_allclose(d, g[f'{case}_dist40x50'], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('D', cc.PR_D + [cc.PR_D_PADDED])
def test_pr_exact_inputs_and_membership_patterns(D):
    for nr, nc in cc.PR_SHAPES:
        cols, rows = cc.pr_features(nc, D, 1), cc.pr_features(nr, D, 2)
        assert np.abs(cols.astype(np.float32)).max() <= 2
        d2 = cc.pr_dist2(rows, cols)
        d2_32 = cc.pr_dist2(rows, cols, np.float32)
        assert (d2 == np.rint(d2)).all() and 0 <= d2.min() and d2.max() <= 16 * D < cc.TWO24 and (d2_32.astype(np.float64) == d2).all()
        direct = ((rows.astype(np.float64)[:, None, :] - cols.astype(np.float64)[None, :, :]) ** 2).sum(2)
        assert (direct == d2).all()
        if D % 16:
            continue
        # (a) the member fraction lies in the window, or (too few probes for a fraction) both answers occur
        pats = cc.member_pattern_a(rows, cols, seed=D + nr)
        if nr >= 5:
            ((name, rad, want),) = pats
            assert name == 'window' and 0.2 <= want.mean() <= 0.8, (D, nr, nc, want.mean())
        else:
            assert [p[0] for p in pats] == ['admit', 'miss'] and pats[0][2][0] and not pats[0][2][1:].any() and not pats[1][2].any()
        for _, rad, want in pats:
            # no squared distance on a boundary: radius^2 = q + 1/2 with integer q (or radius 0, which admits nothing)
            q = np.where(rad > 0, rad.astype(np.float64) ** 2 - 0.5, -1.0)
            assert np.abs(q - np.rint(q)).max() < 1e-3
            assert ((d2 <= np.rint(q)[None, :]).any(axis=1) == want).all()
        # (b) planted
        probes, planted = cc.member_pattern_b(nr, cols, seed=D + nc)
        assert nr - 1 in planted and planted[nr - 1] == nc - 1
        assert set(planted.values()) == set([c for c in [nc - 1] + cc.PLANT_COLS if c < nc][:nr])
        pd2 = cc.pr_dist2(probes, cols)
        for i in range(nr):
            if i in planted:
                assert pd2[i, planted[i]] == 0
            else:
                assert pd2[i].min() >= 1
        want = cc.pr_member(probes, cols, np.full([nc], np.sqrt(0.5), np.float32))
        assert (np.flatnonzero(want) == np.array(sorted(planted))).all()
        # (c) the last column alone admits everything
        rad = cc.member_pattern_c(nc)
        assert cc.pr_member(rows, cols, rad).all() and not cc.pr_member(rows, cols[:-1], rad[:-1]).any()
    assert cc.sqrt_expect32(0.0) == np.float32(np.sqrt(np.float64(np.float32(1e-30)))) and cc.sqrt_expect32(0.0) > 0
    assert cc.within_one_ulp(np.float32(3), np.float32(3)) and cc.within_one_ulp(np.nextafter(np.float32(3), np.float32(4)), np.float32(3))
    assert not cc.within_one_ulp(np.float32(3) + 2 * np.spacing(np.float32(3)), np.float32(3))


def test_pr_end_to_end_case_has_no_borderline_probe():
    """compute_pr_from_features at D = 100 on exact inputs: the float64 restatement (radii through float16) has no distance within
    1e-5 (relative; 80 float32 ulps) of a radius it does not equal, so a float32 kernel must return the same bits; and both answers occur"""
    real, gen = cc.pr_features(161, cc.PR_D_PADDED, 11), cc.pr_features(130, cc.PR_D_PADDED, 12)
    r = cc.pr_from_features(real, gen, 3)
    assert r['gap'] > 1e-5
    assert 0 < r['precision'] < 1 or 0 < r['recall'] < 1, (r['precision'], r['recall'])


def test_moments_exact_inputs_and_restatement():
    for D in cc.MOM_D:
        for n in cc.MOM_N:
            x = cc.mom_inputs(n, D, 'exact')
            mean, cov, _, acov = cc.mom_restate(x)
            assert (x == np.rint(x)).all() and acov.max() <= 81 * n < 2 ** 24
            x32 = x
            assert ((x32.T @ x32).astype(np.float64) == cov).all() and (x32.sum(0).astype(np.float64) == mean).all()
            st = mr.FeatureStatsRef(capture_mean_cov=True)
            st.append(x)
            assert (st.raw_mean == mean).all() and (st.raw_cov == cov).all()
            m0, c0 = np.arange(D, dtype=np.float64) - 3, np.arange(D * D, dtype=np.float64).reshape(D, D) - 7
            mean1, cov1, _, _ = cc.mom_restate(x, m0, c0)
            assert (mean1 == mean + m0).all() and (cov1 == cov + c0).all()
            xf = cc.mom_inputs(n, D, 'float')
            assert (xf < 0).any() and (xf > 0).any() or n * D < 30


def test_fc_plan_and_restatement():
    forms = {n: cc.fc_plan(n) for n in cc.FC_IN}
    assert [forms[n]['form'] for n in (1, 63, 65, 2047)] == ['scalar'] * 4
    assert forms[64] == dict(form='float4', two='none') and forms[512] == dict(form='float4', two='all')
    assert forms[2044] == dict(form='float4', two='mixed')          # the widest float4 row: lane 63's last load has no second float4
    assert forms[2048] == dict(form='wide', ragged_quarter=False, last_quarter=128)
    assert forms[2052] == dict(form='wide', ragged_quarter=True, last_quarter=126) and forms[4100]['ragged_quarter']
    assert cc.fc_plan(2048, aligned=False)['form'] == 'scalar'
    assert cc.fc_case_id(2052) == 'in2052-wide-ragged-quarter' and cc.fc_case_id(2048, aligned=False) == 'in2048-scalar-x-unaligned'
    assert max(cc.FC_B) > 2 * cc.FC_MB and cc.FC_MB in cc.FC_B and cc.FC_MB + 1 in cc.FC_B and any(o % 4 for o in cc.FC_OUT)
    # the restatement is the oracle's FullyConnectedLayer
    for n_in, lr_mul, act in ((65, 0.01, 'lrelu'), (512, 1.0, 'linear')):
        x, W, b = cc.fc_inputs(9, n_in, 5, lr_mul)
        fc = nets.FullyConnectedLayer(n_in, 5, activation=act, lr_multiplier=lr_mul).double()
        with torch.no_grad():
            fc.weight.copy_(torch.from_numpy(W).double())
            fc.bias.copy_(torch.from_numpy(b).double())
            want = fc(torch.from_numpy(x).double()).numpy()
        gain = np.sqrt(2.0) if act == 'lrelu' else 1.0
        got = cc.fc_restate(x, W, b, lr_mul, act, 0.2, gain, np.float64)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert cc.fc_restate(x, W, b, lr_mul, act, 0.2, gain, np.float32).dtype == np.float32


@pytest.mark.parametrize('z_dim,w_dim', cc.MAP_DIMS)
def test_mapping_restatement_is_the_oracle(z_dim, w_dim):
    old = nets.COMPUTE_DTYPE
    nets.COMPUTE_DTYPE = torch.float64
    try:
        for L in cc.MAP_LAYERS:
            if L == 0 and z_dim != w_dim:
                continue          # no layer maps z_dim to w_dim: the oracle cannot take it and the kernel refuses it
            for psi in cc.MAP_PSI:
                z, Ws, bs, w_avg = cc.map_inputs(9, z_dim, w_dim, L)
                M = nets.MappingNetwork(z_dim, w_dim, num_ws=6, num_layers=L, lr_multiplier=cc.MAP_LR_MUL).double()
                with torch.no_grad():
                    for i in range(L):
                        getattr(M, f'fc{i}').weight.copy_(torch.from_numpy(Ws[i]).double())
                        getattr(M, f'fc{i}').bias.copy_(torch.from_numpy(bs[i]).double())
                    M.w_avg.copy_(torch.from_numpy(w_avg).double())
                    want = M(torch.from_numpy(z), truncation_psi=psi).numpy()
                got = cc.map_restate(z, Ws, bs, w_avg, psi, 6, np.float64)
                assert got.shape == want.shape == (9, 6, w_dim) and np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
                assert np.abs(want).max() > 0.1          # the seeded weights do not let the signal die
    finally:
        nets.COMPUTE_DTYPE = old


def test_crop_restatements():
    for R, c, off in cc.CENTER_CROP:
        src = np.arange(2 * R * R, dtype=np.float32).reshape(2, R, R)
        got = cc.center_crop_restate(src, c, off)
        assert got.shape == (2, c, c) and got[1, 0, 0] == src[1, off, off] and got[1, -1, -1] == src[1, off + c - 1, off + c - 1]
        assert off + c <= R
    img = torch.arange(32 * 32, dtype=torch.float32).reshape(1, 1, 32, 32)
    want = lar.center_crop(img, 22)[0].numpy()          # torchvision's offset for 32 -> 22 is 5
    assert (cc.center_crop_restate(img[0].numpy(), 22, 5) == want).all()
    rs = np.random.RandomState(0)
    for R, S, y0, x0 in cc.CROP_WINDOWS:
        for rep in cc.CROP_REP:
            B, imgc = 3, 2
            img = rs.standard_normal([B, imgc, R, R])
            g = rs.standard_normal([imgc * B, rep, S, S])
            xc = cc.crop_repeat_restate(img, S, y0, x0, rep, 0.5, 0.0)
            assert xc.shape == g.shape and (xc[1 * B + 2, rep - 1] == img[2, 1, y0:y0 + S, x0:x0 + S] * 0.5).all()          # row = c * B + b
            gi = cc.crop_repeat_grad_restate(g, np.zeros_like(img), S, y0, x0, rep, 0.5)
            assert abs((xc * g).sum() - (img * gi).sum()) <= 1e-12 * np.abs(xc * g).sum()          # adjoint identity
            outside = np.ones([R, R], bool)
            outside[y0:y0 + S, x0:x0 + S] = False
            assert (gi[:, :, outside] == 0).all()
