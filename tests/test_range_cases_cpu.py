"""range_cases.py checked without a GPU.

  * coverage: every kernel form (modconv_cases.form_key) of precisions 1-3 that modconv_cases.CASES reaches is reached by a uniform
    case, and by a mixed-batch case unless only B = 1 rows reach it (range_cases.B1_ONLY_FORMS, listed there);
  * the property belongs to the arithmetic, not to the kernels: for every pattern that test_hip_operand_range.py runs, the float32
    restatement of the scaled inputs equals the scaled float32 restatement of the unscaled inputs bit for bit, sample by sample, and no
    intermediate of the float64 restatement (nor a single product of the contraction) is subnormal or infinite in float32;
  * planted maxima and zero cases: both restatements are finite, the planted element is the largest of its operand by a factor of 16,
    and the per-sample yardstick (float32 against float64) and scale that the GPU test divides by are non-zero.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modconv_cases as mc  # noqa: E402
import range_cases as rc  # noqa: E402


def test_coverage_of_kernel_forms():
    every, mixed, uniform = rc.coverage()
    assert len(every) == 34      # the 38 forms of test_modconv_cases_cpu.py less the four of precision 0
    assert uniform == every, every - uniform
    assert every - mixed == set(rc.B1_ONLY_FORMS), (every - mixed) ^ set(rc.B1_ONLY_FORMS)
    # the exemption is what it says: no row with more than one sample reaches those forms, and a uniform-only case reaches each
    many = rc.forms_of([c['name'] for c in mc.CASES if c['B'] > 1])
    assert not set(many) & set(rc.B1_ONLY_FORMS)
    assert set(rc.B1_ONLY_FORMS) <= set(rc.forms_of(rc.UNIFORM_ONLY_BASES))
    assert all(mc.BY_NAME[n]['B'] == 1 for n in rc.UNIFORM_ONLY_BASES)


def test_base_cases_are_the_small_ones():
    for n in rc.UNIFORM_BASES + rc.PLANT_BASES + rc.ZERO_BASES:
        assert rc.base_case(n)['res'] <= 96 or n == 'pl_r128', n
    extra = rc.base_case('pl_r128')
    assert extra['res'] == 128 and len(rc.pm_segments(extra['res'] ** 2)) == 2 and 'pl_r128' not in mc.BY_NAME
    assert all(mc.plan(extra, p, True)['launches'][0].cls == 'conv_halo' for p in (1, 2, 3))
    B = mc.BY_NAME
    # the ways samples share a pixel tile
    for n in ('sk_r4_b3', 'uf_r4', 'ub_r4'):
        assert B[n]['B'] == 3 and B[n]['B'] * B[n]['res'] ** 2 <= mc.NT
    for n in ('sk_r6_b5', 'sk_r6_b5_f', 'sk_r34_m128'):
        assert mc.NT % B[n]['res'] ** 2 != 0 and B[n]['B'] > 1
    assert B['sk_3p2']['B'] == 30 and rc.mixed_exponents(30)[:6] == list(rc.MIXED_K5) + [rc.MIXED_K5[0]]
    assert B['arg_bwd']['opts']['xin_bstride0'] and set(rc.mixed_pattern(B['arg_bwd'])) == {'gz'}
    assert rc.mixed_exponents(3) == [-16, 0, 12] and rc.mixed_exponents(5) == [-16, 0, 12, 24, -40]
    # no product of the patterns leaves [2^-100, 2^100]
    for n in rc.UNIFORM_BASES:
        c = rc.homogeneous_case(n)
        pats = [k for _, k in rc.uniform_patterns(c)] + ([rc.mixed_pattern(c), rc.same_pattern(c)] if rc.mixed_pattern(c) else [])
        for k in pats:
            for exps in rc.out_exponents(c, k).values():
                assert all(-100 <= e <= 100 for e in exps)


def _patterns(c):
    pats = list(rc.uniform_patterns(c))
    if c['name'] in rc.MIXED_BASES and rc.mixed_pattern(c):
        pats += [('mixed', rc.mixed_pattern(c)), ('same', rc.same_pattern(c))]
    return pats


@pytest.mark.parametrize('name', rc.UNIFORM_BASES)
def test_float32_restatement_is_bit_homogeneous(name):
    c = rc.homogeneous_case(name)
    t = rc.tensors(c, True)
    base = mc.restate(c, t, torch.float32)
    for tag, k in _patterns(c):
        ts = rc.scaled(t, k)
        for key, v in rc.intermediates(c, ts).items():
            assert rc.in_normal_float32_range(v), (name, tag, key, 'leaves the normal float32 range')
        got = mc.restate(c, ts, torch.float32)
        for key, exps in rc.out_exponents(c, k).items():
            want = rc.times_pow2(base[key], exps)
            assert torch.equal(rc.bits(got[key]), rc.bits(want)), (name, tag, key)
            assert float(want.abs().max()) > 0


def _per_sample_nonzero(c, t, samples=None):
    r64 = mc.restate(c, t, torch.float64)
    r32 = mc.restate(c, t, torch.float32)
    for key, ref in r64.items():
        assert torch.isfinite(ref).all() and torch.isfinite(r32[key]).all(), key
        for b in range(c['B']) if samples is None else samples:
            assert float(ref[b].abs().max()) > 0, (key, b)
            assert float((r32[key][b].double() - ref[b]).abs().max()) > 0, (key, b, 'yardstick')
    return r64


@pytest.mark.parametrize('name', rc.PLANT_BASES)
def test_planted_cases(name):
    c = rc.base_case(name)
    t = rc.tensors(c, False)
    key, C, HW = rc.plant_operand(c)
    b = rc.plant_sample(c)
    pos = rc.plant_positions(c)
    tags = {tag for tag, _, _ in pos}
    assert {'first', 'last_of_last_plane', 'last_of_middle_plane'} <= tags and len(pos) >= 4
    assert ('seg0_first' in tags or pos[0][2] == 0) and 'seg0_last' in tags
    if name == 'pl_r128':      # the boundary between the two segments of a plane, from both sides
        assert ('seg0_last', 1, 8191) in pos and ('seg1_first', 1, 8192) in pos and ('seg1_last', 1, 16383) in pos
    assert sum(p1 - p0 for p0, p1 in rc.pm_segments(HW)) == HW
    for tag, ch, p in pos:
        tp = rc.planted(c, t, ch, p)
        op = tp[key].double()
        if key == 'x':
            op = op * tp['s'].double()[:, :, None, None]
        flat = op.abs().view(c['B'], C, HW)
        top = float(flat[b, ch, p])
        flat[b, ch, p] = 0
        assert top == pytest.approx(rc.PLANT_FACTOR * float(flat.max()), rel=1e-6), (name, tag)
        _per_sample_nonzero(c, tp)
        m = rc.reach(c, ch, p)
        for k2, v in m.items():
            assert v[b].any() and not v[[q for q in range(c['B']) if q != b]].any(), (name, tag, k2)
            if k2 != 'ds':
                assert int(v[b, 0].sum()) <= 9 and not v[b].all(), (name, tag, 'a 3x3 footprint at the most')
    # the one-channel chunk and the 2^31-free segment layout
    if name == 'ha_r64_m36':
        assert c['cin'] % mc.KCB == 1 and ('ragged_chunk', 32, HW // 2) in pos
    assert rc.pm_segments(8192 * 3 + 5) == [(0, 8196), (8196, 16392), (16392, 24581)]
    assert len(rc.pm_segments(1 << 20)) == mc.PM_NS and rc.pm_segments(90 * 90) == [(0, 8100)]


@pytest.mark.parametrize('name', rc.ZERO_BASES)
def test_zero_cases(name):
    c = mc.BY_NAME[name]
    t = rc.tensors(c, False)
    for tag, key, b, ch in rc.zero_variants(c):
        tz = rc.zeroed(t, key, b, ch)
        others = [q for q in range(c['B']) if q != b]
        r64 = _per_sample_nonzero(c, tz, samples=others if tag != 'plane' else None)
        if tag == 'sample' and not rc.is_fwd(c):
            assert not r64['gx'][b].any() and not r64['ds'][b].any()
        if tag == 'xin_sample':
            assert not r64['ds'][b].any() and r64['gx'][b].any()
