"""CPU-only proof that tests/loop_cases.py is what test_hip_loop_shapes.py takes it for: one step of `step_restate` in float64 equals
float64 autograd of the oracle loop (oracle.latent_aug_ref.LatentAugRef in W, tests/wplus_cpu.LatentAugRefWPlus in W+) for every
criterion mix, with norm_batch != B too (the oracle divides by B: its weights are scaled by B / norm_batch); `adam_restate` and
`gate_restate` give the oracle's latent after the step and its w_aug; `reach` over the table hits every item the sweep claims and the
table in the GPU file's docstring is the generated one; every guarded case meets the guard at its recorded seed and at no earlier one;
and `judge` accepts the float32 restatement's own free-running run of every case (the plumbing of the GPU test, without a GPU)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as lc  # noqa: E402
import wplus_cpu  # noqa: E402

from oracle import latent_aug_ref as lar  # noqa: E402
from oracle import sg2_networks as nets  # noqa: E402

# every mix, both spaces; norm_batch != B (5 and 8 against B 2 and 4) in a latent, a pixel and an all-criteria case
NORM_CASES = [
    lc.LoopCase('W-R32-wd64-B4-nb8', 32, 64, 4, Mw=4, steps=1, norm_batch=8, w_latent=0.5),
    lc.LoopCase('pix-R16-nb5', 16, 24, 2, Mx=9, imgc=3, w_pix=2.0, w_latent=0.3, Mw=4, norm_batch=5, kind='guarded'),
    lc.LoopCase('all-R32-nb5', 32, 32, 2, crop_pos=(3, 11), norm_batch=5, kind='guarded', **lc.ALL_MIX),
    lc.LoopCase('all-W+-R32-nb5', 32, 32, 2, 'w+', crop_pos=(11, 3), norm_batch=5, kind='guarded', **lc.ALL_MIX),
]
ORACLE_CASES = [c for c in lc.TAIL_CASES if c.steps > 0] + lc.GUARDED_CASES + NORM_CASES


def _oracle_step(case, b):
    """(losses [4], dL/dw, w after one Adam step, w_aug) of the oracle loop in float64"""
    B = case.B
    k = B / case.nb(B)
    mods = [m for m in (b.G, b.D, b.fnet) if m is not None]
    scale, shift = (torch.tensor(v, dtype=torch.float32).double().reshape(1, 3, 1, 1) for v in lc.PREPROC)
    dbl = (lambda t: None if t is None else t.double())
    nets.COMPUTE_DTYPE = torch.float64
    try:
        for m in mods:
            m.double()
        cls = wplus_cpu.LatentAugRefWPlus if case.wplus else lar.LatentAugRef
        ref = cls(b.G, b.D, W=dbl(b.W), X=dbl(b.X), fea=None if b.fea is None else [f.double() for f in b.fea],
                  feature_net=None if b.fnet is None else (lambda x: b.fnet(x * scale + shift)), res=case.R, num_epochs=1, opt_lr=lc.LR,
                  w_latent=case.w_latent * k, w_pix=case.w_pix * k, w_disc=case.w_disc * k, w_lpips=case.w_lpips * k, crop_size=lc.FEAT_CROP,
                  preprocess='center_random_crop', soft_aug=case.soft, alpha=case.alpha, final_noise_mode='const', fused_modconv=False,
                  dtype=torch.float64)
        _, w_aug = ref.forward(b.w0[:B], crop_pos=case.crop_pos, record=True)
        t = ref.trace
        L = torch.tensor([t['loss_latent'][0], t['loss_pix'][0], t['loss_disc'][0], t['loss_lpips'][0]], dtype=torch.float64)
        return L, t['grad'][0], t['w'][0], w_aug
    finally:
        nets.COMPUTE_DTYPE = torch.float32
        for m in mods:
            m.float()


@pytest.mark.parametrize('case', ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_one_step_equals_float64_autograd_of_the_oracle(case):
    b = case.build()
    L, g, w1, w_aug = _oracle_step(case, b)
    r = lc.step_restate(case, b.w0[:case.B], torch.float64, b)
    assert r['dw'].shape == g.shape == (case.B, case.rows, case.w_dim)
    eg = lc.worst(r['dw'], g) / float(g.abs().max())
    eL = float(((r['losses'] - L).abs() / L.abs().clamp_min(1e-300)).max())
    print(f'{case.name}: dw relative {eg:.2e}, losses relative {eL:.2e}, losses {L.tolist()}')
    assert eg <= 1e-10 and eL <= 1e-11
    for col, wgt in enumerate((case.w_latent, case.w_pix, case.w_disc, case.w_lpips)):
        assert (float(L[col]) != 0.0) == (wgt > 0)
    assert lc.worst(lc.adam_restate(b.w0[:case.B], [g], torch.float64), w1) <= 1e-14
    assert lc.worst(lc.gate_restate(case, w1, b.w0[:case.B], torch.float64), w_aug) <= 1e-14 and w_aug.shape[1] == case.num_ws


def test_adam_restate_rebuilds_the_moments_from_the_gradients():
    """step k from w_{k-1} and gradients 1..k equals the k-th step of a running AdamState, whatever the earlier latents were"""
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn([2, 1, 8], generator=g, dtype=torch.float64) for _ in range(4)]
    p = torch.randn([2, 1, 8], generator=g, dtype=torch.float64)
    st = lar.AdamState(p, lc.LR)
    for k, gr in enumerate(grads, 1):
        new = st.step(p, gr)
        assert lc.worst(lc.adam_restate(p, grads[:k], torch.float64), new) <= 1e-15
        p = new


def test_every_claimed_item_is_reached():
    table = lc.reach_table()
    for name, rows in table.items():
        assert rows, f'no case reaches: {name}'
    r = lc.reach(lc.BY_NAME['W-R16-wd88-B3'])
    assert r['tail'] == dict(kernel='w', workgroups=2, last_partial=True) and r['slots'] == dict(groups=0, remainder=6)
    assert lc.reach(lc.BY_NAME['W-R16-wd88-B3'], B=1)['tail']['workgroups'] == 1
    r = lc.reach(lc.BY_NAME['W+-R64-wd32-B4'])
    assert r['tail'] == dict(kernel='wplus', workgroups=2, last_partial=True) and r['colsums']['latent']['waves'] == [(2, 0), (1, 3), (1, 3), (1, 3)]
    assert lc.reach(lc.BY_NAME['W-R64-wd32-B2'])['slots'] == dict(groups=1, remainder=2)
    assert lc.colsum_plan(17)['waves'] == [(1, 1), (1, 0), (1, 0), (1, 0)] and lc.colsum_plan(5)['waves'] == [(0, 2), (0, 1), (0, 1), (0, 1)]
    p = lc.reach(lc.BY_NAME['pix-R256-imgc3-Mx3-B1'])['dots']['pix']
    assert [(q['K'], q['vec'], q['ksplit']) for q in p] == [(32761, False, 16)] * 3
    p = lc.reach(lc.BY_NAME['pix-R32-imgc2-Mx9'])['dots']['pix']
    assert [(q['K'], q['vec'], q['ksplit'], q['row_blocks']) for q in p] == [(484, True, 4, 2)] * 2
    p = lc.reach(lc.BY_NAME['pix-R16-imgc3-Mx9-B9'])['dots']['pix']
    assert all(q['K'] == 121 and not q['vec'] and q['passes'] == 2 for q in p)
    # the loop's strided forms are not the public op's (ldx = K, xmod = 0)
    for c in lc.CASES:
        for q in lc.reach(c)['dots'].get('latent', []):
            assert (q['ldx'], q['xmod']) == ((q['K'], 0) if c.wplus else (c.w_dim, c.w_dim))
        for q in lc.reach(c)['dots'].get('pix', []):
            assert q['ldx'] == c.imgc * q['K'] and (c.imgc == 1 or q['ldx'] != q['K'])
    assert {c.steps for c in lc.TAIL_CASES} == {0, 1, 2, 5} and {c.Mw for c in lc.TAIL_CASES} == {1, 4, 5, 17, 29}
    assert all(c.R == 32 and c.w_dim == 32 and c.B == 2 and c.steps == 3 for c in lc.GUARDED_CASES if c.name != 'pix-R16')


def test_the_reach_table_of_the_gpu_file_is_the_generated_one():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_hip_loop_shapes.py')) as f:
        assert lc.reach_text() in f.read(), 'regenerate the table: python tests/loop_cases.py --table'


@pytest.mark.parametrize('case', lc.GUARDED_CASES, ids=[c.name for c in lc.GUARDED_CASES])
def test_recorded_seed_is_the_first_that_meets_the_guard(case):
    assert lc.first_seed(case) == case.seed < 64
    _, r32, r64 = case.runs()
    g, m, where = lc.guard_of(r32['pre'], r64['pre'])
    neg = [float((p.a < 0).double().mean()) for p in r64['pre'] if p.clamp is None or p.a is not p.v]
    print(f'{case.name}: seed {case.seed}, guard g {g:.3e}, smallest margin {m:.3e} ({where}), {sum(p.a.numel() for p in r64["pre"])} pre-activations')
    assert m >= g
    # the kink is in use in every lrelu / relu layer of every step (the ToRGB records have only the clamp)
    assert all(0.0 < f < 1.0 for p, f in ((p, float((p.a < 0).double().mean())) for p in r64['pre']) if 'torgb' not in p.name), neg


@pytest.mark.parametrize('case', [c for c in lc.CASES if c.R <= 64], ids=[c.name for c in lc.CASES if c.R <= 64])
def test_judge_accepts_the_float32_restatement(case):
    b = case.build()
    v = lc.judge(case, b, lc.simulate(case, b, torch.float32))
    assert not v.bad, '\n'.join(v.bad)
    assert all(r <= 1.0 for r in v.ratios.values()) and ('gate' in v.ratios) and (case.steps == 0 or 'Adam' in v.ratios)
