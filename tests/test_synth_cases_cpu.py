"""CPU-only proof that tests/synth_cases.py is what test_hip_synth_shapes.py takes it for: the float64 restatement of the synthesis
network equals float64 autograd of the oracle built with the explicit channel table (image, every block's x, dws and the gradient of
every style row, to 1e-12 relative), every guarded case meets its guard at its recorded seed (and no earlier seed does), the clamp
case clamps in every layer, every branch the sweep claims is reached by some case, and the reach table in the GPU file's docstring is
the generated one.  Prints the seed, the guard g and the float32 budgets of every case."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

ALL = sc.SYNTH_CASES + [sc.SYNTH_SHRINK]
OUTS = ('img', 'styles', 'dstyles', 'dws')
_RUNS = {}


def _runs(case):
    if case.name not in _RUNS:
        _RUNS[case.name] = case.runs()
    return _RUNS[case.name]


def _rel(a, b):
    return sc.worst(a, b) / float(b.abs().max())


@pytest.mark.parametrize('case', ALL, ids=[c.name for c in ALL])
def test_restatement_equals_the_oracle_and_guard(case):
    G, ws, g_img, r32, r64 = _runs(case)
    assert G.synthesis.channels == case.table and G.num_ws == 2 * len(case.table)
    img, feats, dws, dstyles = sc.synth_oracle(G, ws, g_img)
    assert _rel(r64['img'], img) <= 1e-12 and _rel(r64['dws'], dws) <= 1e-12
    # the blocks' x: the output of every block's conv1
    conv1 = [r64['layers'][0]] + r64['layers'][2::2]
    assert len(conv1) == len(feats) and all(_rel(a, b) <= 1e-12 for a, b in zip(conv1, feats))
    # style gradients against hooks on the oracle's affine outputs (execution order: a block's conv layers, then its ToRGB, whose
    # affine output sits in front of the gain 1 / sqrt(cin))
    nconv, rows, off = len(case.noise), [], 0
    cins = [case.channels[0]] + [c for k, c in enumerate(case.channels[1:]) for c in (case.channels[k], c)]
    for cin in cins + case.channels:
        rows.append(r64['dstyles'][:, off:off + cin])
        off += cin
    assert off == r64['dstyles'].shape[1] == r64['styles'].shape[1]
    order, ci = [], 0
    for k in range(len(case.channels)):
        for _ in range(1 if k == 0 else 2):
            order.append((rows[ci], 1.0))
            ci += 1
        order.append((rows[nconv + k], 1.0 / math.sqrt(case.channels[k])))
    assert len(order) == len(dstyles)
    scale = max(float(g.abs().max()) for g in dstyles)
    for (mine, gain), want in zip(order, dstyles):
        assert sc.worst(mine * gain, want) <= 1e-12 * scale
    g, m, where = sc.guard_of(r32['pre'], r64['pre'])
    line = f'{case.name}: kind {case.kind}, seed {case.seed}, guard g {g:.3e}, smallest margin {m:.3e} ({where}), {sum(p.a.numel() for p in r64["pre"])} pre-activations'
    for key in OUTS:
        line += f', f32 error of {key} {sc.worst(r32[key], r64[key]):.3e} (budget k=4: {sc.budget(4.0, r32[key], r64[key]):.3e})'
    print(line)
    if case.kind == 'guarded':
        assert m >= g, f'{case.name}: margin {m:.3e} below the guard {g:.3e}'
    else:
        assert case.kind == 'bulk' and case.R >= 64
        print(f'{case.name}: f32 relative L2 ' + ', '.join(f'{key} {sc.rel_l2(r32[key], r64[key]):.3e}' for key in OUTS))


def test_recorded_seeds_are_the_first_that_meet_the_guard():
    for case in sc.SYNTH_GUARDED + [sc.SYNTH_SHRINK]:
        assert sc.first_seed(case) == case.seed < 64, case.name


def test_clamp_case_clamps_in_every_layer():
    """between 1 % and 50 % of the float64 values of EVERY conv layer and EVERY ToRGB layer lie beyond the clamp"""
    case = sc.SYNTH_BY_NAME[sc.SYNTH_CLAMP_CASE]
    _, _, _, _, r64 = _runs(case)
    lo, hi = sc.CLAMP_FRACTION
    assert len(r64['pre']) == len(case.noise) + len(case.channels)
    assert sc.clamp_binds(r64['pre'])
    for p in r64['pre']:
        f = p.clamped_fraction()
        print(f'{case.name} {p.name}: clamp {p.clamp}, {100 * f:.1f} % beyond it')
        assert p.clamp == sc.CLAMP_BINDS and lo <= f <= hi, (p.name, f)
    # ... and in no other guarded case does anything reach the clamp
    for other in sc.SYNTH_GUARDED:
        if other.clamp == 256.0:
            assert all(p.clamped_fraction() == 0 for p in _runs(other)[-1]['pre'])


def test_every_claimed_branch_is_reached():
    table = sc.reach_table()
    for name, rows in table.items():
        assert rows, f'no case reaches: {name}'
    # the fused ToRGB needs a 16-bit mode; f32 takes the seam kernel in every block, the 16-bit modes in the top block only
    for c in (1, 3, 4):
        assert table[f'ToRGB fused into the halo forward, IMGC = {c}'] == [(f'R64-rgbfuse-imgc{c}', ['bf16x3', 'f16x2'])]
    plan = sc.branch_plan(sc.SYNTH_BY_NAME['R256-imgc3-slabs'], 'f16x2')
    assert [b['slabs'] for b in plan['blocks']][-2:] == [1, 4] and plan['blocks'][-1]['seam'] == 'kernel' and plan['blocks'][-2]['seam'] == 'fused'
    assert all(b['seam'] == 'kernel' for b in sc.branch_plan(sc.SYNTH_BY_NAME['R256-imgc3-slabs'], 'f32')['blocks'])
    assert {name: (R, ch, imgc, wd) for name, R, ch, imgc, wd, _, _ in sc.SYNTH_REFUSALS} == {
        'table-entry-6': (16, (8, 6, 8), 2, 16), 'imgc-0': (8, (8, 8), 0, 16), 'imgc-5': (8, (8, 8), 5, 16), 'w_dim-18': (8, (8, 8), 2, 18)}
    for name, cols in sc.SYNTH_WINDOWED:
        case = sc.SYNTH_BY_NAME[name]
        lo, hi = sc.window_of(case.R)
        assert 0 < lo < hi < case.R and lo % 4 and hi % 4          # (no multiple of the 4-row tiles)
        g = sc.windowed_g_img(case, torch.ones([1, case.imgc, case.R, case.R]), cols)
        assert int(g.sum()) == case.imgc * (hi - lo) * ((hi - lo) if cols else case.R)


def test_the_reach_table_of_the_gpu_file_is_the_generated_one():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_hip_synth_shapes.py')) as f:
        assert sc.reach_text() in f.read(), 'regenerate the table: python tests/synth_cases.py --table'
