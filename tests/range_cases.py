"""Operand-magnitude patterns for the four modulated-conv layer entries: power-of-two scalings of x / gz / xin / W (one exponent for
the tensor, or one per sample), planted maxima and zero samples.  Shared by test_range_cases_cpu.py (no GPU) and
test_hip_operand_range.py (gpu).  Cases, tensors, the float64 restatement and the dispatch plan are modconv_cases'; a case here is one
of its rows with overridden opts.

The property.  Multiplying an operand by 2^k changes no significand bit while nothing leaves the normal float32 range, so every float32
rounding commutes with it; the data-derived power-of-two operand scales of LA_PREC_F16X2 (la_pow2_scale, la_common.h) then make the
packed 16-bit operands bit-identical.  Wherever an entry is linear (or positively homogeneous) in an operand the result of the scaled
call is 2^k times the result of the unscaled call, bit for bit and sample by sample:
  forward   y  ~ x * W          with noise_strength = 0, zero bias, clamp = -1 (homogeneous_case); lrelu, gain and d stay (d is an input)
  backward  gx ~ gz * W,  ds ~ gz * xin * W

Segment layout of the plane-maxima pass (la_conv_operand.hip: la_conv_act_grad_segments, la_plane_absmax_kernel, la_act_grad_pmax_kernel):
a plane of HW pixels is cut into ns = clamp(HW / 8192, 1, PM_NS = 8) segments of per = round_up(ceil(HW / ns), 4) pixels, segment s =
[s * per, min(s * per + per, HW)); one workgroup per (segment, plane, sample).  Below res 128 that is ONE segment, whose first and last
pixel are the ends of the plane; pl_r128 (EXTRA_CASES) has two, and test_hip_operand_range.py runs the feature engine's backward at
res 128 for la_act_grad_pmax_kernel.  The up-sampling backward entry takes the maxima of the FIR-adjoint scratch instead
(la_upfirdn2d.hip, la_fir4x4_segments: blocks of 64 columns x 32 rows of the (res + 1)^2 plane; one block at ub_r8); the first / last
pixel of a gz plane reaches the first / last pixel of that scratch plane.
"""
import torch

import modconv_cases as mc

UNIFORM_K = (-60, -24, -12, 12, 24, 60)                       # on x / gz alone, and on W alone
DS_PAIRS = ((-60, 24), (24, -60), (-24, -24), (12, 12))      # (k_gz, k_xin): no product leaves [2^-100, 2^100]
MIXED_K3 = (-16, 0, 12)
MIXED_K5 = MIXED_K3 + (24, -40)
SAME_K = 24                                                  # the call between two mixed calls: every sample at 2^24

# smallest case of each kernel form and of each way samples share a pixel tile; ex_up_m128 is there for the merged 128-row forms
MIXED_BASES = ('sk_r4_b3', 'sk_r6_b5', 'sk_r6_b5_f', 'sk_r34_m128', 'ha_r64_m28', 'ha_r64_m64', 'ha_r96_b', 'uf_r4', 'uf_r8', 'ub_r4', 'ub_r8',
               'arg_bwd', 'sk_3p2', 'ex_up_m128')
# forms that only B = 1 rows of modconv_cases.CASES reach (128-row halo tiles: the smallest such grid is res 64 with >= 128 rows): uniform
# exponents only
B1_ONLY_FORMS = ((1, 'conv_halo', 128, '32x32', False), (2, 'conv_halo', 128, '32x32', False), (3, 'conv_halo', 128, '16x16x32', False),
                 (3, 'conv_halo', 128, '32x32', False))
UNIFORM_ONLY_BASES = ('ha_r64_m128', 'ha_r64_m128_c32')
UNIFORM_BASES = MIXED_BASES + UNIFORM_ONLY_BASES
# pl_r128: not a row of modconv_cases.CASES -- the smallest same-resolution call whose planes hold TWO segments of the plane-maxima pass
# (res 128; 8 channels in and out: 38 MFLOP), so that a segment boundary inside a plane is planted too
EXTRA_CASES = {'pl_r128': dict(mc.BY_NAME['ha_r64_m28'], name='pl_r128', B=2, cin=8, cout=8, res=128,
                               why='res 128: two plane-maxima segments per plane; 32-row halo tiles')}
PLANT_BASES = ('sk_r6_b5_f', 'ha_r64_m36', 'sk_r33_b', 'ub_r8', 'pl_r128')
ZERO_BASES = ('sk_r4_b3', 'sk_r6_b5', 'sk_r6_b5_f', 'ha_r64_m28', 'ha_r64_m64', 'uf_r4', 'ub_r4')
PLANT_FACTOR = 16.0      # the scaled maximum lies in [2^14, 2^15): a missed maximum 16x larger reaches infinity in fp16


def base_case(name):
    return mc.BY_NAME[name] if name in mc.BY_NAME else EXTRA_CASES[name]


def case_index(name):
    """the seed index of modconv_cases.make_tensors: the row's own, or past the table for the extra cases"""
    return mc.CASES.index(mc.BY_NAME[name]) if name in mc.BY_NAME else len(mc.CASES) + sorted(EXTRA_CASES).index(name)


def is_fwd(case):
    return case['entry'] in ('fwd', 'up2_fwd')


def homogeneous_case(name):
    """The row `name` of modconv_cases.CASES; a forward row without noise and clamp (its bias is zeroed by tensors())."""
    base = mc.BY_NAME[name]
    if not is_fwd(base):
        return base
    return dict(base, opts=dict(base['opts'], noise_strength=0.0, clamp=-1.0))


def tensors(case, zero_bias):
    t = mc.make_tensors(case, case_index(case['name']))
    if zero_bias and is_fwd(case):
        t['bias'] = torch.zeros_like(t['bias'])
    return t


def operand_keys(case):
    return ('x',) if is_fwd(case) else ('gz', 'xin')


def broadcast(case, key):
    return bool(case['opts']['x_bstride0' if key == 'x' else 'xin_bstride0']) if key in ('x', 'xin') else False


def mixed_exponents(B, shift=0):
    """k_b of sample b: (-16, +12) for two samples, MIXED_K3 for three, else cycling through MIXED_K5; `shift` rotates the pattern."""
    if B == 2:
        pat = (MIXED_K3[0], MIXED_K3[2])
    elif B == 3:
        pat = MIXED_K3
    else:
        pat = MIXED_K5
    return [pat[(b + shift) % len(pat)] for b in range(B)]


def uniform_patterns(case):
    """[(tag, {operand: exponent})]: one exponent for a whole operand."""
    first = operand_keys(case)[0]
    pats = [(f'{first}{k:+d}', {first: k}) for k in UNIFORM_K] + [(f'w{k:+d}', {'w': k}) for k in UNIFORM_K]
    if not is_fwd(case):
        pats += [(f'gz{a:+d}_xin{b:+d}', {'gz': a, 'xin': b}) for a, b in DS_PAIRS]
    return pats


def mixed_pattern(case):
    """{operand: [k_b]}: the operands that hold one sample per row of the batch, gz and xin with independent exponents; None if none does."""
    B = case['B']
    k = {key: mixed_exponents(B, shift) for shift, key in enumerate(operand_keys(case)) if not broadcast(case, key)}
    return k if B > 1 and k else None


def same_pattern(case):
    return {key: [SAME_K] * case['B'] for key in mixed_pattern(case)}


def scaled(t, k):
    """The tensors t with operand `key` multiplied by 2^k[key] (an int, or one int per sample).  Exact in float32."""
    out = dict(t)
    for key, e in k.items():
        v = t[key]
        if isinstance(e, int):
            out[key] = v * torch.tensor(2.0 ** e, dtype=torch.float32)
        else:
            assert v.shape[0] == len(e), key
            out[key] = v * torch.tensor([2.0 ** q for q in e], dtype=torch.float32).view(-1, 1, 1, 1)
        assert out[key].dtype == torch.float32
    return out


def out_exponents(case, k):
    """{output: [exponent of sample b]} of the call on scaled(t, k): y ~ x W, gx ~ gz W, ds ~ gz xin W."""
    B = case['B']

    def per(key):
        e = k.get(key, 0)
        return [e] * B if isinstance(e, int) else list(e)

    if is_fwd(case):
        return {'y': [a + w for a, w in zip(per('x'), per('w'))]}
    return {'gx': [a + w for a, w in zip(per('gz'), per('w'))], 'ds': [a + b + w for a, b, w in zip(per('gz'), per('xin'), per('w'))]}


def times_pow2(v, exps):
    """v[b] * 2^exps[b] in v's dtype."""
    f = torch.tensor([2.0 ** e for e in exps], dtype=v.dtype, device=v.device)
    return v * f.view([-1] + [1] * (v.ndim - 1))


def bits(v):
    return v.contiguous().view(torch.int32 if v.dtype == torch.float32 else torch.int64)


def intermediates(case, t):
    """Every tensor that the float64 restatement forms on the way (named), plus the smallest and largest single product of the
    contraction as 1-element tensors: what must stay inside the normal float32 range for the property to hold."""
    d64 = torch.float64
    W, s = t['w'].to(d64), t['s'].to(d64)
    B = case['B']
    out = {'w': W}

    def nz_min(v):
        v = v.abs()
        return v[v > 0].min() if bool((v > 0).any()) else torch.ones([], dtype=d64)

    if is_fwd(case):
        x = t['x'].to(d64).expand(B, -1, -1, -1)
        xs = x * s[:, :, None, None]
        out.update(x=x, xs=xs)
        if case['entry'] == 'fwd':
            z = mc.corr3x3(xs, W)
        else:
            out['tconv'] = mc.tconv3x3_s2(xs, W)
            z = mc.fir_pad1(out['tconv'])
        out['z'] = z
        if t['d'] is not None:
            out['zd'] = z * t['d'].to(d64)[:, :, None, None]
        out['prod_min'] = (nz_min(W) * nz_min(xs)).view(1)
        out['prod_max'] = (W.abs().max() * xs.abs().max()).view(1)
    else:
        gz = t['gz'].to(d64)
        xin = t['xin'].to(d64).expand(B, -1, -1, -1)
        out.update(gz=gz, xin=xin)
        if case['entry'] == 'bwd':
            u = mc.corr3x3_adj(gz, W)
            a = gz
        else:
            a = out['adj'] = mc.fir_pad1_adj(gz)
            u = mc.tconv3x3_s2_adj(a, W)
        out.update(u=u, uxin=u * xin)
        out['prod_min'] = (nz_min(W) * nz_min(a)).view(1)
        out['prod_max'] = (W.abs().max() * a.abs().max()).view(1)
    out.update(mc.restate(case, t, d64))
    return out


F32_MIN_NORMAL, F32_MAX = 2.0 ** -126, float(torch.finfo(torch.float32).max)


def in_normal_float32_range(v):
    a = v.abs()
    a = a[a > 0]
    return bool(torch.isfinite(v).all()) and (a.numel() == 0 or (float(a.min()) >= F32_MIN_NORMAL and float(a.max()) <= F32_MAX))


# ---------------------------------------------------------------------------------------------------------------------------------
# planted maxima

def pm_segments(HW):
    """[p0, p1) of every segment of the plane-maxima pass over a plane of HW pixels (module docstring)."""
    ns = min(max(HW // 8192, 1), mc.PM_NS)
    per = (mc.cdiv(HW, ns) + 3) & ~3
    return [(s * per, min(s * per + per, HW)) for s in range(ns) if s * per < HW]


def plant_operand(case):
    """(key, C, HW) of the operand whose maxima set the per-sample scale: the launch input of the contraction."""
    if is_fwd(case):
        rin = case['res'] // 2 if case['entry'] == 'up2_fwd' else case['res']
        return 'x', case['cin'], rin * rin
    return 'gz', case['cout'], case['res'] ** 2


def plant_sample(case):
    return min(3, case['B'] - 1)      # sk_r6_b5_f: the sample inside which the second pixel tile starts


def plant_positions(case):
    """[(tag, channel, pixel)] in sample plant_sample(case), without repeats."""
    key, C, HW = plant_operand(case)
    ragged = (C - 1) // mc.KCB * mc.KCB      # first channel of the last chunk: the only one where C % 32 == 1
    pos = [('first', 0, 0), ('last_of_last_plane', C - 1, HW - 1), ('last_of_middle_plane', C // 2, HW - 1)]
    for i, (p0, p1) in enumerate(pm_segments(HW)):
        pos += [(f'seg{i}_first', 1 % C, p0), (f'seg{i}_last', 1 % C, p1 - 1)]
    pos.append(('ragged_chunk', ragged, HW // 2))
    seen, out = set(), []
    for tag, c, p in pos:
        if (c, p) not in seen:
            seen.add((c, p))
            out.append((tag, c, p))
    return out


def planted(case, t, c, p):
    """t with element (plant_sample, c, p) of the launch input set so that its magnitude in the operand the scale is taken from (the
    modulated input x * s forward, gz backward) is PLANT_FACTOR times the largest other one of the whole batch."""
    key, C, HW = plant_operand(case)
    b = plant_sample(case)
    v = t[key].clone()
    assert not broadcast(case, key)
    if key == 'x':
        mod = (t['x'].double() * t['s'].double()[:, :, None, None]).abs()
        mod.view(case['B'], C, HW)[b, c, p] = 0
        value = PLANT_FACTOR * float(mod.max()) / abs(float(t['s'][b, c]))
    else:
        other = t['gz'].double().abs()
        other.view(case['B'], C, HW)[b, c, p] = 0
        value = PLANT_FACTOR * float(other.max())
    v.view(case['B'], C, HW)[b, c, p] = value
    return dict(t, **{key: v})


def reach(case, c, p):
    """Boolean masks {output: [B, ...]} of the elements that the planted element can reach, from the float64 restatement of a one-hot
    input under all-ones weights, styles and xin.  ds sums over the pixels: the whole row of the sample is reached."""
    key, C, HW = plant_operand(case)
    b = plant_sample(case)
    B, cin, cout, res = case['B'], case['cin'], case['cout'], case['res']
    one = dict(case, opts=dict(case['opts'], noise_strength=0.0, clamp=-1.0, x_bstride0=False, xin_bstride0=False, no_demod=True))
    rin = int(round(HW ** 0.5))
    hot = torch.zeros([B, C, HW])
    hot[b, c, p] = 1.0
    t = {'w': torch.ones([cout, cin, 3, 3]), 's': torch.ones([B, cin]), 'd': None, 'noise': torch.zeros([res, res]), 'bias': torch.zeros([cout])}
    t[key] = hot.view(B, C, rin, rin)
    if key == 'gz':
        rx = res // 2 if case['entry'] == 'up2_bwd' else res
        t['xin'] = torch.ones([B, cin, rx, rx])
    return {k: v != 0 for k, v in mc.restate(one, t, torch.float64).items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# zero cases

def zero_variants(case):
    """[(tag, key, sample, channel or None)]: a whole sample of the launch input, one channel plane of it, xin of one sample."""
    key = operand_keys(case)[0]
    b = 1
    assert case['B'] > b and not broadcast(case, key)
    v = [('sample', key, b, None), ('plane', key, b, 1)]
    if not is_fwd(case) and not broadcast(case, 'xin'):
        v.append(('xin_sample', 'xin', b, None))
    return v


def zeroed(t, key, b, c):
    v = t[key].clone()
    if c is None:
        v[b] = 0
    else:
        v[b, c] = 0
    return dict(t, **{key: v})


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage

def forms_of(names):
    """{form_key: first case name} over precisions 1-3 and both workspace modes of the named rows."""
    seen = {}
    for name in names:
        c = mc.BY_NAME[name]
        for p in (1, 2, 3):
            for ws in (True, False):
                if ws or mc.splits(c, p):
                    for l in mc.plan(c, p, ws)['launches']:
                        seen.setdefault(mc.form_key(p, l), name)
    return seen


def coverage():
    """(all forms of precisions 1-3 in modconv_cases.CASES, those a mixed-batch case reaches, those a uniform case reaches)."""
    every = set(forms_of([c['name'] for c in mc.CASES]))
    mixed = set(forms_of([n for n in MIXED_BASES if mixed_pattern(homogeneous_case(n))]))
    return every, mixed, set(forms_of(UNIFORM_BASES))
