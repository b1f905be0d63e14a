"""CPU-only proof that tests/engine_cases.py is what test_hip_engine_shapes.py takes it for: the float64 restatements of the feature net
and of the discriminator equal float64 autograd of the oracle (to 1e-12 relative), every guarded case meets its guard at its recorded
seed (and no earlier seed does), every exact case holds small integers, the clamp case clamps, the tie case ties, the zero-pixel case
has zero pixels.  Prints the seed, the guard g and the float32 budgets of every case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_cases as ec  # noqa: E402

FEAT_ALL = ec.FEAT_CASES + [ec.FEAT_SHRINK]
DISC_ALL = ec.DISC_CASES + [ec.DISC_SHRINK]


def _rel(a, b):
    return ec.worst(a, b) / float(b.abs().max())


def _report(case, r32, r64, outs):
    g, m, where = ec.guard_of(r32['pre'], r64['pre'])
    line = f'{case.name}: kind {case.kind}, seed {case.seed}, guard g {g:.3e}, smallest margin {m:.3e} ({where})'
    for key in outs:
        line += f', f32 error of {key} {ec.worst(r32[key], r64[key]):.3e} (budget k=4: {ec.budget(4.0, r32[key], r64[key]):.3e})'
    print(line)
    return g, m


@pytest.mark.parametrize('case', FEAT_ALL, ids=[c.name for c in FEAT_ALL])
def test_feature_restatement_and_guard(case):
    ops, x, gfeat, r32, r64 = case.runs()
    feat, gx = ec.feat_oracle(ops, x, gfeat)
    assert _rel(r64['feat'], feat) <= 1e-12 and _rel(r64['gx'], gx) <= 1e-12
    g, m = _report(case, r32, r64, ('feat', 'gx'))
    assert case.kind == 'guarded' and m >= g, f'{case.name}: margin {m:.3e} below the guard {g:.3e}'


@pytest.mark.parametrize('case', DISC_ALL, ids=[c.name for c in DISC_ALL])
def test_discriminator_restatement_and_guard(case):
    D, img, dlogits, r32, r64 = case.runs()
    logits, gx = ec.disc_oracle(D, img, dlogits)
    assert _rel(r64['logits'], logits) <= 1e-12 and _rel(r64['gx'], gx) <= 1e-12
    g, m = _report(case, r32, r64, ('logits', 'gx'))
    if case.kind == 'guarded':
        assert m >= g, f'{case.name}: margin {m:.3e} below the guard {g:.3e}'
    else:
        assert case.kind == 'bulk' and case.R == 128
        print(f'{case.name}: f32 relative L2 of logits {ec.rel_l2(r32["logits"], r64["logits"]):.3e}, of gx {ec.rel_l2(r32["gx"], r64["gx"]):.3e}')


def test_recorded_seeds_are_the_first_that_meet_the_guard():
    """the search is over at most 64 seeds and the table records its result (two of the slower cases stand for all: the module's
    __main__ prints the whole search)"""
    for case in (ec.FEAT_BY_NAME['conv-conv-conv-pool'], ec.DISC_BY_NAME['imgc4'], ec.DISC_BY_NAME['clamp-0.5']):
        assert ec.search_seed(case) == case.seed < ec.MAX_SEEDS


def test_every_listed_shape_is_in_the_tables():
    names = set(ec.FEAT_BY_NAME)
    assert len(names) == len(ec.FEAT_CASES) and len(ec.DISC_BY_NAME) == len(ec.DISC_CASES)
    for C, r in [(1, 8), (3, 8), (5, 8), (28, 8), (29, 8), (32, 8), (33, 8), (36, 8), (3, 2), (64, 2), (512, 2), (513, 2), (8, 3), (8, 6), (8, 10), (8, 14)]:
        c = ec.FEAT_BY_NAME[f'tap-only-C{C}-res{r}']
        assert (c.in_ch, c.res, c.N, c.max_batch, c.kinds) == (C, r, 3, 4, ['tap'])
    for c in ec.FEAT_CASES:
        assert c.res <= 28 and max(c.widths + [c.in_ch]) <= (513 if c.res == 2 else 36) and (c.res == 2 or max(c.widths + [0]) <= 16)
    assert {c.group if c.B > c.group else c.B for c in ec.DISC_CASES if c.name.startswith('group')} == {1, 3, 4, 9, 16}
    assert [ec.DISC_BY_NAME[n].B // min(ec.DISC_BY_NAME[n].group, ec.DISC_BY_NAME[n].B) for n in ('group-B8-g4', 'group-B6-g3')] == [2, 2]
    for c in ec.DISC_CASES:
        assert max(c.table.values()) <= (36 if c.name.startswith('channels') else 16) and all(v % 4 == 0 for v in c.table.values())
    t = ec.DISC_BY_NAME['channels-12-20-36'].table
    assert sorted(set(t.values())) == [12, 20, 36] and all(t[r] != t[r // 2] for r in t if r > 4) and all(v % 16 for v in t.values())
    assert any(v % 4 for v in ec.DISC_BAD_TABLE.values())
    assert ec.DISC_GROUP_REFUSAL['B'] % ec.DISC_GROUP_REFUSAL['group'] != 0
    assert ec.DISC_BY_NAME['R128'].R ** 2 > 4096 and ec.DISC_BY_NAME['clamp-none'].clamp is None


@pytest.mark.parametrize('name', ec.DISC_CLAMP_CASES)
def test_clamp_case_clamps(name):
    """between 5 % and 50 % of the pre-activations of every conv0, conv1 and of the epilogue conv lie beyond the clamp"""
    case = ec.DISC_BY_NAME[name]
    _, _, _, _, r64 = case.runs()
    seen = 0
    for p in r64['pre']:
        if p.name.endswith(('conv0', 'conv1', 'b4.conv')):
            f = p.clamped_fraction()
            print(f'{name} {p.name}: clamp {p.clamp:.4f}, {100 * f:.1f} % beyond it')
            assert p.clamp is not None and 0.05 <= f <= 0.5, (p.name, f)
            seen += 1
    assert seen == 5
    assert abs(r64['pre'][2].clamp - ec.CLAMP * ec.RSQRT2) < 1e-15          # conv1: clamp * sqrt(1/2)


@pytest.mark.parametrize('pool,res', ec.POOL_EXACT)
def test_pool_exact_case_is_integers_with_all_three_ties(pool, res):
    x, lin, gfeat = ec.pool_exact_inputs(res)
    for t in (x, gfeat, lin * 4):
        assert bool((t == t.round()).all())
    assert 4 * float(x.abs().max()) < ec.TWO24          # every partial sum of a 2x2 window is an integer below 2^24
    y, route = ec.pool_exact_reference(pool, x)
    assert bool((y * 4 == (y * 4).round()).all()) and bool((y.float().double() == y).all())
    found = ec.tie_windows(x)
    assert all(found.values()), found
    if pool == 'maxpool':          # the restated routing is torch's own (first maximum in scan order), ties included
        xr = x.double().requires_grad_(True)
        (gt,) = torch.autograd.grad(torch.nn.functional.max_pool2d(xr, 2), [xr], gfeat.double().reshape(y.shape))
        assert torch.equal(route(gfeat), gt)
        # and a routing to the LAST maximum would differ by order 1
        assert float((route(gfeat) - route(gfeat).flip(0)).abs().max()) >= 1
    xs, _, _ = ec.pool_sign_inputs(res)
    assert bool((xs.abs() >= 1).all()) and bool((xs == xs.round()).all())


def test_tap_zero_case_has_zero_pixels_and_finite_answers():
    ops, x, gfeat = ec.tap_zero_inputs()
    zero = (x == 0).all(dim=1)
    assert int(zero.sum()) >= 1 and int((ops[0][1] == 0).sum()) == 2
    for dtype in (torch.float32, torch.float64):
        r = ec.feat_restate(ops, x, dtype, gfeat)
        assert bool(torch.isfinite(r['feat']).all()) and bool(torch.isfinite(r['gx']).all())
    feat, gx = ec.feat_oracle(ops, x, gfeat)
    r64 = ec.feat_restate(ops, x, torch.float64, gfeat)
    assert _rel(r64['feat'], feat) <= 1e-12 and _rel(r64['gx'], gx) <= 1e-12


def test_loss_restatement():
    l = torch.tensor(ec.LOSS_LOGITS, dtype=torch.float64, requires_grad=True)
    for nb in ec.LOSS_NORM_BATCH:
        n = nb if nb > 0 else len(ec.LOSS_LOGITS)
        loss = torch.nn.functional.softplus(-l).sum() / n * ec.LOSS_W
        (dl,) = torch.autograd.grad(loss, [l])
        want, dwant = ec.disc_loss_restate(ec.LOSS_LOGITS, ec.LOSS_W, nb)
        # (torch's softplus returns z itself above its threshold of 20: e^-20.5 / n * w away from the function restated here)
        assert abs(want - float(loss.detach())) <= 1e-12 * abs(want) + 2 * np.exp(-20.0) / n * ec.LOSS_W
        np.testing.assert_allclose(dwant, dl.numpy(), rtol=1e-12, atol=2 * np.exp(-20.0) / n * ec.LOSS_W)          # (its derivative: exactly 1 there)
    assert min(abs(abs(v) - 20) for v in ec.LOSS_LOGITS) == 0.5          # both sides of the threshold
