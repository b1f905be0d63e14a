"""Sweep of filtered_lrelu (la_filtered_lrelu.hip) over the shapes at which its kernels change form, against the float64 restatement of
tests/flrelu_cpu.py: all nine la_flrelu_fused_kernel<UP, DOWN> instantiations with several tiles in both axes, every reachable rung of
the tile ladder, both sides of the fused / generic predicate, tile seams and ragged edges, negative and unequal padding, the sign buffer
read directly through the C ABI (written bytes, untouched bytes, read mode with arbitrary offsets), la_filtered_lrelu_act_f32 in its
three modes, more than 65535 planes, and the parameter edges (clamp 0, slope 0, slope > 1, gain, absent filters).  Inputs come from a
seeded CPU generator; the filters are jittered Hann windows (asymmetric, so flip_filter and the tap order matter); the bias is on.

tile_plan below restates the host side of the fused launch (flr_fused_ok, flr_fused_lds and the candidate loop of la_filtered_lrelu_f32).
It only picks shapes and proves that the lists of cases reach what they claim to reach; it never produces an expected value.

Bounds (none tuned to the kernels):
  y, dx, db, g2   the rule of test_hip_filtered_lrelu.py: HIP error <= 4 x the float32 yardstick's own error + 2e-6 x the largest float64
                  magnitude, where the yardstick is the same restatement run in float32 on the CPU (held to the reference by
                  test_filtered_lrelu_cpu.py), and in addition <= 1e-5 x that magnitude (the bound of the StyleGAN3-size test).
  kinks           dx / g2 elements whose dependency cone holds a sample within KINK_RTOL of a branch edge are compared at 1e-2 x scale
                  only; at most 15 % of them (asserted from the float64 oracle before anything is compared).  y takes no exclusion.
  sign bits       exact against sign_bits of the float64 oracle outside kink samples, which may be at most 0.1 % of the samples; bytes
                  that lie wholly past the active extent must still hold the pre-fill, exactly.
  act entry       one multiply / compare per element: |err| <= 2^-23 x |expected| away from the clamp edge.

Rungs: {32x32, 32x16, 16x16, 16x8, 8x8} are reached by valid arguments; 4x4 is not (the 8x8 candidate needs at most 53072 bytes with the
largest filters of the envelope: test_case_lists_cover_every_form), so that rung of the ladder is dead code.

Measured on one MI355X: the whole file (300 cases) takes 22 s, most of it the CPU oracles (float64 and float32, second order); the
70000-plane case alone takes 6 s.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flrelu_cpu  # noqa: E402

pytestmark = pytest.mark.gpu

KINK_RTOL = 2e-6      # (test_hip_filtered_lrelu.py)
MAX_EXCLUDED = 0.15
MAX_KINK_SIGNS = 1e-3
SQRT2 = math.sqrt(2)
EPS32 = 2.0 ** -23

# ---------------------------------------------------------------- which kernel form a call reaches (host-side restatement; shapes only)
CANDIDATES = ((32, 32), (32, 16), (16, 16), (16, 8), (8, 8), (4, 4))
LDS_BYTES = 65536


def _cdiv(a, b):
    return -(-a // b)


def out_size(i, up, down, p0, p1, fut, fdt):
    return (i * up + p0 + p1 - (fut - 1) - (fdt - 1) + down - 1) // down


def lds_need(tow, toh, up, down, fu, fd):
    """Bytes of LDS of a fused tile of toh x tow outputs (flr_fused_lds)."""
    (fuh, fuw, fu2d), (fdh, fdw, fd2d) = fu, fd
    mw = (max((tow - 1) * down + fdw, tow * down) + 3) & ~3
    mh = max((toh - 1) * down + fdh, toh * down)
    iw, ih = (mw + fuw - 2) // up + 1, (mh + fuh - 2) // up + 1
    pin, pmid, pdh = iw | 1, mw | 1, tow | 1
    nfu = fuh * fuw if fu2d else fuw
    nfd = fdh * fdw if fd2d else fdw
    r1 = max(ih * pin + (0 if fu2d else ih * pmid), 0 if fd2d else mh * pdh)
    return 4 * (nfu + nfd + r1 + mh * pmid)


def tile_plan(oh, ow, up, down, fu, fd):
    """fu / fd: (rows, cols, is_2d).  -> dict(rung, tow, toh, tiles_x, tiles_y, lds) of the fused launch, or None = the generic path."""
    if not (up in (1, 2, 4) and down in (1, 2, 4) and max(fu[0], fu[1]) <= 8 * up and max(fd[0], fd[1]) <= 8 * down):
        return None
    for t in CANDIDATES:
        tow = (_cdiv(ow, _cdiv(ow, t[0])) + 3) & ~3
        toh = _cdiv(oh, _cdiv(oh, t[1]))
        need = lds_need(tow, toh, up, down, fu, fd)
        if need <= LDS_BYTES:
            return dict(rung=t, tow=tow, toh=toh, tiles_x=_cdiv(ow, tow), tiles_y=_cdiv(oh, toh), lds=need)
    return None


def taps_of(spec):
    """(rows, cols, is_2d) of a filter spec: None, ('1d', taps) or ('2d', rows, cols)."""
    return (1, 1, True) if spec is None else ((spec[1], spec[1], False) if spec[0] == '1d' else (spec[1], spec[2], True))


def size_for(o, up, down, p0, p1, fut, fdt):
    """Smallest input size, and the far-side padding (p1 or less), that give exactly o outputs."""
    i = 1
    while out_size(i, up, down, p0, p1, fut, fdt) < o:
        i += 1
    return i, o * down - (i * up + p0 - (fut - 1) - (fdt - 1) + down - 1)


def smallest_multitile(up, down, fus, fds, rung=None):
    """Smallest (oh, ow), ow = oh + 3, with at least 2 x 2 tiles (on the given rung of the ladder, if one is named)."""
    for o in range(2, 200):
        p = tile_plan(o, o + 3, up, down, taps_of(fus), taps_of(fds))
        if p and p['tiles_x'] >= 2 and p['tiles_y'] >= 2 and (rung is None or p['rung'] == rung):
            return o, o + 3
    raise AssertionError(f'no multi-tile size for up {up} down {down} {fus} {fds} rung {rung}')


# ---------------------------------------------------------------- cases
def _taps1d(n, gen):
    t = torch.from_numpy(np.hanning(n + 2)[1:-1].copy()).float() * (1 + 0.3 * torch.rand(n, generator=gen))
    return t / t.sum()


def make_filter(spec, gen):
    """Jittered Hann taps, normalised to sum 1: asymmetric, and a 2-D one is not separable."""
    if spec is None:
        return None
    if spec[0] == '1d':
        return _taps1d(spec[1], gen)
    t = torch.outer(_taps1d(spec[1], gen), _taps1d(spec[2], gen)) * (1 + 0.1 * torch.rand(spec[1], spec[2], generator=gen))
    return t / t.sum()


def case(name, up, down, fus, fds, out=None, inp=None, pad=None, n=1, c=2, flip=False, slope=0.2, clampq=None, clamp=None, gain=SQRT2,
         bias=True, seed=0):
    """A case spec.  out = (oh, ow): the input size and the far-side padding follow (pad = the [px0, px1, py0, py1] to start from, default
    about half the taps per side); inp = (h, w): pad is used exactly.  clampq = the share of the intermediate samples the clamp trips on."""
    return dict(name=name, up=up, down=down, fus=fus, fds=fds, out=out, inp=inp, pad=pad, n=n, c=c, flip=flip, slope=slope, clampq=clampq,
                clamp=clamp, gain=gain, bias=bias, seed=seed)


def geometry(s):
    """(h, w, [px0, px1, py0, py1], oh, ow, plan) of a case spec."""
    fut, fdt = taps_of(s['fus']), taps_of(s['fds'])
    up, down = s['up'], s['down']
    if s['inp'] is not None:
        (h, w), pad = s['inp'], list(s['pad'])
    else:
        half = lambda a, b: (a + b - 2) // 2      # noqa: E731
        pad = list(s['pad']) if s['pad'] is not None else [half(fut[1], fdt[1]) + 1, half(fut[1], fdt[1]), half(fut[0], fdt[0]) + 1, half(fut[0], fdt[0])]
        w, pad[1] = size_for(s['out'][1], up, down, pad[0], pad[1], fut[1], fdt[1])
        h, pad[3] = size_for(s['out'][0], up, down, pad[2], pad[3], fut[0], fdt[0])
    oh, ow = out_size(h, up, down, pad[2], pad[3], fut[0], fdt[0]), out_size(w, up, down, pad[0], pad[1], fut[1], fdt[1])
    assert oh >= 1 and ow >= 1 and (s['out'] is None or (oh, ow) == tuple(s['out'])), (s['name'], oh, ow)
    return h, w, pad, oh, ow, tile_plan(oh, ow, up, down, fut, fdt)


def materialise(s):
    """tensors (x, b, fu, fd, dy, v: float32, CPU) and the keyword arguments of a case spec."""
    h, w, pad, oh, ow, _ = geometry(s)
    gen = torch.Generator().manual_seed(1000 + s['seed'])
    fu, fd = make_filter(s['fus'], gen), make_filter(s['fds'], gen)
    x = torch.randn([s['n'], s['c'], h, w], generator=gen)
    b = 0.3 * torch.randn([s['c']], generator=gen) if s['bias'] else None
    if s['bias'] == 'distinct':      # (a wrong channel index must show)
        b = 0.5 * torch.arange(1, s['c'] + 1, dtype=torch.float32) * (-1.0) ** torch.arange(s['c'])
    kw = dict(up=s['up'], down=s['down'], padding=pad, gain=s['gain'], slope=s['slope'], clamp=s['clamp'], flip_filter=s['flip'])
    if s['clampq'] is not None:      # (half-way between two samples of |lrelu| of the unclamped intermediate: none sits on the edge)
        a = flrelu_cpu.act_stage(flrelu_cpu.up_stage(x, fu, b, s['up'], pad, s['flip']), s['gain'], s['slope'])
        v = np.sort(a.abs().numpy().ravel())
        v = v[v > 0]      # (zero-inserted samples that no filter spreads, and padding, are exact zeros: not part of the share)
        i = min(int((1 - s['clampq']) * v.size), v.size - 2)
        kw['clamp'] = float(np.float32((v[i] + v[i + 1]) / 2))
    dy = torch.randn([s['n'], s['c'], oh, ow], generator=gen)
    v = torch.randn(x.shape, generator=gen)
    return dict(x=x, b=b, fu=fu, fd=fd, dy=dy, v=v), kw


F_UP = {1: 5, 2: 12, 4: 24}      # taps per factor of the form sweep (the envelope allows 8 x the factor)


def _spec(kind, taps):
    return ('1d', taps) if kind == '1' else ('2d', taps - 1, taps)


def form_cases():
    """All nine (up, down) forms x {1-D, 2-D, mixed} filters x flip x clamp, each at the smallest output with 2 x 2 tiles or more.
    Reaches every la_flrelu_fused_kernel<UP, DOWN> (flr_launch_fused_up: `a.down == 1 ... else <UP, 4>`, and `up == 1 ... else <4>` in
    la_filtered_lrelu_f32), both up-FIR branches (`if (a.fu2d)`) and both down-FIR branches (`if (a.fd2d)`), with blockIdx.y and
    blockIdx.z above 0."""
    out = []
    for up in (1, 2, 4):
        for down in (1, 2, 4):
            for kinds in ('11', '22', '12', '21'):
                fus, fds = _spec(kinds[0], F_UP[up]), _spec(kinds[1], F_UP[down])
                combos = ((False, 0.3), (True, None), (True, 0.3), (False, None)) if kinds == '11' else ((False, 0.3), (True, None))
                for flip, cq in combos:
                    name = f'u{up}d{down}_f{kinds}_{"flip" if flip else "conv"}_{"clamp" if cq else "free"}'
                    out.append(case(name, up, down, fus, fds, out=smallest_multitile(up, down, fus, fds), flip=flip, clampq=cq, seed=len(out)))
    return out


REACHABLE = {(32, 32), (32, 16), (16, 16), (16, 8), (8, 8)}


def ladder_cases():
    """One case or more per reachable rung (the `need <= FLR_LDS_BYTES` test of the candidate loop fails for the rungs above), and both
    sides of the fused / generic predicate flr_fused_ok (`fut <= 8 * up`, `fdt <= 8 * down`, `up == 1 || up == 2 || up == 4`)."""
    rows = [
        ('r8x8', 1, 4, ('1d', 8), ('1d', 32), (8, 8)),
        ('r16x8', 1, 4, ('2d', 8, 8), ('2d', 32, 32), (16, 8)),
        ('r16x16', 2, 4, ('1d', 16), ('1d', 32), (16, 16)),
        ('r32x16', 4, 4, ('2d', 32, 32), ('2d', 32, 32), (32, 16)),
        ('r32x32_full_lds', 4, 4, ('1d', 32), ('1d', 32), (32, 32)),
    ]
    out = []
    for name, up, down, fus, fds, rung in rows:
        o = (37, 37) if name == 'r32x32_full_lds' else smallest_multitile(up, down, fus, fds, rung)
        out.append(case(name, up, down, fus, fds, out=o, c=1, clampq=0.3, seed=200 + len(out)))
    out += [
        case('fused_fu16_up2', 2, 2, ('1d', 16), ('1d', 16), out=(34, 37), clampq=0.3, seed=210),
        case('generic_fu17_up2', 2, 2, ('1d', 17), ('1d', 16), out=(34, 37), clampq=0.3, seed=211),
        case('generic_fd17_down2', 2, 2, ('1d', 16), ('1d', 17), out=(34, 37), flip=True, seed=212),
        case('generic_fu2d_9rows_up1', 1, 1, ('2d', 9, 4), ('1d', 5), out=(33, 35), clampq=0.3, seed=213),
        case('generic_up3', 3, 2, ('1d', 9), ('1d', 6), out=(34, 37), clampq=0.3, seed=214),
        case('generic_down3', 2, 3, ('1d', 12), ('2d', 5, 7), out=(13, 17), flip=True, seed=215),
    ]
    return out


SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65)


def seam_cases():
    """Output heights and widths around the tile sizes: OW < 4 (tow is rounded up to 4, past the output), OH == 1, one output past a tile
    (33, 65), the even spread (36 -> 2 tiles of 20, the last one owning 16), exact multiples (32, 64: `lastx` with o0x + tow == OW).
    fd of 3 taps with down 4 leaves intermediate samples between the outputs that nobody reads."""
    forms = [(2, 2, ('1d', 12), ('1d', 12)), (1, 1, ('2d', 3, 3), ('1d', 5)), (4, 2, ('1d', 24), ('2d', 12, 11)), (1, 4, None, ('1d', 3)),
             (4, 4, ('1d', 24), ('1d', 24))]
    out = []
    for fi, (up, down, fus, fds) in enumerate(forms):
        for i, oh in enumerate(SIZES):
            ow = SIZES[(i + 5 + fi) % len(SIZES)]
            out.append(case(f'u{up}d{down}_{oh}x{ow}', up, down, fus, fds, out=(oh, ow), c=1 if oh * ow > 2000 else 2, flip=bool(i & 1),
                            clampq=0.3 if i % 3 else None, seed=300 + len(out)))
    return out


def padding_cases():
    """Padding negative on each side in turn (flr_floordiv / flr_posmod with negative arguments: ix0, iy0 of the first tiles, kx0, ky0),
    unequal on the four sides, all negative, and much larger than the filters; H != W throughout."""
    out = []
    pads = {'x0neg': [-3, 10, 11, 10], 'x1neg': [11, -3, 10, 11], 'y0neg': [10, 11, -5, 10], 'y1neg': [11, 10, 11, -6], 'unequal': [13, 7, 4, 19],
            'allneg': [-1, -2, -3, -4], 'wide': [30, 27, 25, 33], 'x0neg_odd': [-7, 12, -1, 9]}
    for k, (pname, pad) in enumerate(pads.items()):
        out.append(case(f'u2d2_{pname}', 2, 2, ('1d', 12), ('1d', 12), inp=(27, 31), pad=pad, flip=bool(k & 1), clampq=0.3, seed=400 + k))
        out.append(case(f'u4d1_{pname}', 4, 1, ('2d', 20, 24), ('1d', 4), inp=(13, 11), pad=pad, flip=not (k & 1), clampq=0.3, seed=430 + k))
        out.append(case(f'u1d2_{pname}', 1, 2, ('1d', 7), ('2d', 9, 12), inp=(75, 83), pad=pad, c=1, seed=440 + k))
    return out


def parameter_cases():
    """slope 0 and slope 1.5 (bit 0 then bit 1 of flr_act in the other order of magnitude), gain != sqrt(2), fu / fd absent in each
    position (`a.fu ? ... : gu`, the 1 x 1 identity)."""
    return [
        case('slope0', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), slope=0.0, clampq=0.3, seed=500),
        case('slope0_free', 4, 2, ('1d', 24), ('1d', 12), out=(34, 37), slope=0.0, seed=501),
        case('slope15', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), slope=1.5, clampq=0.3, seed=502),
        case('slope15_u1d4', 1, 4, ('1d', 5), ('1d', 24), out=(18, 21), slope=1.5, clampq=0.2, seed=503),
        case('gain3', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), gain=3.0, clampq=0.3, seed=504),
        case('gain_small', 2, 4, ('1d', 12), ('1d', 24), out=(26, 29), gain=0.37, clampq=0.3, seed=505),
        case('fu_none', 2, 2, None, ('1d', 12), out=(34, 37), clampq=0.3, seed=506),
        case('fd_none', 2, 2, ('1d', 12), None, out=(34, 37), clampq=0.3, seed=507),
        case('both_none', 2, 2, None, None, inp=(19, 21), pad=[0, 2, 2, 3], clampq=0.3, seed=508),
        case('both_none_u1d1', 1, 1, None, None, inp=(35, 37), pad=[0, 0, 0, 0], clampq=0.3, seed=509),
        case('fu_none_u4d4', 4, 4, None, ('2d', 24, 20), out=(18, 21), flip=True, seed=510),
        case('no_bias', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), bias=False, clampq=0.3, seed=511),
        case('n3c5_distinct_bias', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), n=3, c=5, bias='distinct', clampq=0.3, seed=512),
        case('n3c5_distinct_bias_generic', 3, 2, ('1d', 9), ('1d', 6), out=(9, 11), n=3, c=5, bias='distinct', clampq=0.3, seed=513),
    ]


FORMS, LADDER, SEAMS, PADS, PARAMS = form_cases(), ladder_cases(), seam_cases(), padding_cases(), parameter_cases()


def ids(cases):
    return [s['name'] for s in cases]


# ---------------------------------------------------------------- running and checking
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


def oracle(t, kw, dtype):
    """y, dx, db, g2 of the CPU restatement in dtype, as float64 numpy arrays."""
    x = t['x'].to(dtype).requires_grad_(True)
    b = None if t['b'] is None else t['b'].to(dtype).requires_grad_(True)
    dy = t['dy'].to(dtype).requires_grad_(True)
    y = flrelu_cpu.filtered_lrelu(x, t['fu'], t['fd'], b, **kw, dtype=dtype)
    grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
    (g2,) = torch.autograd.grad((grads[0] * t['v'].to(dtype)).sum(), [dy])
    out = {'y': y, 'dx': grads[0], 'g2': g2}
    if b is not None:
        out['db'] = grads[1]
    return {k: v.detach().double().numpy() for k, v in out.items()}


def run_hip(t, kw, dev, noncontig=False):
    from latentaugment_amd import ops
    x = t['x'].to(dev)
    if noncontig:      # same values, a transposed view of a [N, C, W, H] tensor
        x = x.transpose(2, 3).contiguous().transpose(2, 3)
        assert not x.is_contiguous()
    x.requires_grad_(True)
    b = None if t['b'] is None else t['b'].to(dev).requires_grad_(True)
    fu = None if t['fu'] is None else t['fu'].to(dev)
    fd = None if t['fd'] is None else t['fd'].to(dev)
    dy = t['dy'].to(dev).requires_grad_(True)
    y = ops.filtered_lrelu(x, fu, fd, b, **kw)
    grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
    (g2,) = torch.autograd.grad((grads[0] * t['v'].to(dev)).sum(), [dy])
    out = {'y': y, 'dx': grads[0], 'g2': g2}
    if b is not None:
        out['db'] = grads[1]
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def masks(t, kw):
    """Excluded elements per quantity (bool arrays), from the float64 kink samples of the case (as test_hip_filtered_lrelu.py)."""
    mask, _ = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=KINK_RTOL)
    y_aff, x_aff = flrelu_cpu.affected(mask, t['x'].shape, t['fu'], t['fd'], kw['up'], kw['down'], kw['padding'], kw['flip_filter'])
    tight, _ = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=1e-6)
    ch = tight.sum(dim=(0, 2, 3)) > 0
    return {'y': np.zeros(y_aff.shape, bool), 'g2': y_aff.numpy(), 'dx': x_aff.numpy(), 'db': ch.numpy()}


def check(name, k, hip, ref64, ref32, excl):
    assert hip.shape == ref64.shape, (name, k, hip.shape, ref64.shape)
    assert np.isfinite(hip).all(), f'{name} {k}: non-finite output'
    scale = float(np.abs(ref64).max())
    err = np.abs(hip - ref64)
    budget = min(4.0 * float(np.abs(ref32 - ref64)[~excl].max(initial=0.0)) + 2e-6 * scale, 1e-5 * scale)
    worst = float(err[~excl].max(initial=0.0))
    print(f'{name} {k}: err {worst:.3e} budget {budget:.3e} scale {scale:.3e} excluded {excl.mean():.2%}')
    assert k == 'db' or excl.mean() <= MAX_EXCLUDED, f'{name} {k}: {excl.mean():.1%} of the elements sit in a kink cone'
    assert worst <= budget, f'{name} {k}: HIP error {worst:.3e} > budget {budget:.3e} (scale {scale:.3e})'
    assert err[excl].max(initial=0.0) <= 1e-2 * scale, f'{name} {k}: excluded elements off by {err[excl].max():.3e}'


def check_case(s, dev, noncontig=False):
    t, kw = materialise(s)
    r64, r32 = oracle(t, kw, torch.float64), oracle(t, kw, torch.float32)
    ex = masks(t, kw)
    for k in ('dx', 'g2'):      # (from the oracle alone, before the kernel runs)
        assert ex[k].mean() <= MAX_EXCLUDED, f'{s["name"]} {k}: {ex[k].mean():.1%} of the elements sit in a kink cone; pick another seed'
    hip = run_hip(t, kw, dev, noncontig)
    assert set(hip) == set(r64)
    for k in hip:
        check(s['name'], k, hip[k], r64[k], r32[k], ex[k])


# ---------------------------------------------------------------- the C ABI
def sign_shape(lib, t, kw):
    n, c, h, w = t['x'].shape
    fu_h, fu_w = _c_taps(t['fu'])
    fd_h, fd_w = _c_taps(t['fd'])
    rows, row_bytes = C.c_int(-1), C.c_int(-1)
    assert lib.la_filtered_lrelu_sign_shape(h, w, fu_h, fu_w, fd_h, fd_w, kw['up'], kw['down'], *kw['padding'], C.byref(rows), C.byref(row_bytes)) == 0
    return rows.value, row_bytes.value


def _c_taps(f):
    return (1, 1) if f is None else ((0, f.shape[0]) if f.ndim == 1 else tuple(f.shape))


def c_call(dev, t, kw, si=None, sx=0, sy=0, write=False, prefill=0):
    """la_filtered_lrelu_f32 itself.  -> (y [N, C, OH, OW] float64 CPU, so [N, C, rows, row_bytes] uint8 CPU or None)."""
    from latentaugment_amd import _lib
    lib = _lib.load()
    n, c, h, w = t['x'].shape
    fu_h, fu_w = _c_taps(t['fu'])
    fd_h, fd_w = _c_taps(t['fd'])
    px0, px1, py0, py1 = kw['padding']
    up, down = kw['up'], kw['down']
    oh = lib.la_filtered_lrelu_out_size(h, up, down, py0, py1, fu_h or fu_w, fd_h or fd_w)
    ow = lib.la_filtered_lrelu_out_size(w, up, down, px0, px1, fu_w, fd_w)
    rows, row_bytes = sign_shape(lib, t, kw)
    x = t['x'].to(dev).contiguous()
    fu = None if t['fu'] is None else t['fu'].to(dev).contiguous()
    fd = None if t['fd'] is None else t['fd'].to(dev).contiguous()
    b = None if t['b'] is None else t['b'].to(dev).contiguous()
    y = torch.full([n, c, oh, ow], float('nan'), device=dev)
    so = torch.full([n, c, rows, row_bytes], prefill, dtype=torch.uint8, device=dev) if write else None
    sid = None
    if si is not None:
        assert tuple(si.shape) == (n, c, rows, row_bytes) and si.dtype == torch.uint8
        sid = si.to(dev).contiguous()
    clamp = math.inf if kw['clamp'] is None else kw['clamp']
    _lib.check(lib.la_filtered_lrelu_f32(_lib.ptr(x), _lib.ptr(fu), _lib.ptr(fd), _lib.ptr(b), _lib.ptr(sid), _lib.ptr(so), _lib.ptr(y), n, c, h, w,
                                         fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1, sx, sy, kw['gain'], kw['slope'], clamp,
                                         int(kw['flip_filter']), int(write), _lib.stream_ptr()), 'filtered_lrelu')
    torch.cuda.synchronize()
    return y.double().cpu(), (None if so is None else so.cpu())


def check_written_signs(name, t, kw, so, prefill):
    """The written buffer against sign_bits of the float64 oracle (kink samples aside) and the pre-fill past the active extent."""
    want = flrelu_cpu.sign_bits(t['x'], t['fu'], t['fd'], t['b'], **kw)
    ah, aw = want.shape[2], want.shape[3]
    kink = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=KINK_RTOL)[0] > 0
    assert kink.shape == want.shape
    assert kink.double().mean() <= MAX_KINK_SIGNS, f'{name}: {kink.double().mean():.3%} of the samples are kinks'
    got = flrelu_cpu.unpack_signs(so, ah, aw)
    bad = (got != want) & ~kink
    assert not bad.any(), f'{name}: {int(bad.sum())} of {bad.numel()} sign samples differ, first at {bad.nonzero()[0].tolist()}'
    past = torch.ones(so.shape, dtype=torch.bool)
    past[:, :, :ah, :_cdiv(aw, 4)] = False
    assert past.any() or so.shape[2] == ah, name
    assert (so[past] == prefill).all(), f'{name}: {int((so[past] != prefill).sum())} bytes past the active extent were written'
    return int(kink.sum()), got.numel()


# ---------------------------------------------------------------- tests: values and gradients
def test_case_lists_cover_every_form():
    """The claims of this file about what it reaches, from tile_plan: nine (up, down) forms with 2 x 2 tiles or more, every reachable
    rung, both sides of the fused / generic predicate; and the 4 x 4 rung is reachable by no valid argument (the 8 x 8 candidate fits
    with the largest filters of the envelope, and its need grows with every tap count)."""
    multi = set()
    for s in FORMS:
        p = geometry(s)[5]
        assert p is not None and p['tiles_x'] >= 2 and p['tiles_y'] >= 2, s['name']
        multi.add((s['up'], s['down'], taps_of(s['fus'])[2], taps_of(s['fds'])[2]))
    assert multi == {(u, d, a, b) for u in (1, 2, 4) for d in (1, 2, 4) for a in (False, True) for b in (False, True)}
    rungs, generic = set(), set()
    for s in LADDER:
        p = geometry(s)[5]
        if p is None:
            generic.add(s['name'])
        else:
            assert p['tiles_x'] >= 2 and p['tiles_y'] >= 2, s['name']
            rungs.add(p['rung'])
            if s['name'] == 'r32x32_full_lds':
                assert p['lds'] == 65184 and p['rung'] == (32, 32)
    assert rungs == REACHABLE
    assert generic == {'generic_fu17_up2', 'generic_fd17_down2', 'generic_fu2d_9rows_up1', 'generic_up3', 'generic_down3'}
    assert geometry(LADDER[5])[5] is not None and LADDER[5]['name'] == 'fused_fu16_up2'      # 8 * up taps: still fused
    # (an 8 x 8 candidate gives a tile of at most 8 x 8 outputs, and lds_need grows with the tile and with every tap count)
    worst = max(lds_need(8, 8, up, down, (8 * up, 8 * up, a), (8 * down, 8 * down, b))
                for up in (1, 2, 4) for down in (1, 2, 4) for a in (False, True) for b in (False, True))
    assert worst == 53072 and worst <= LDS_BYTES
    seams = {(geometry(s)[3], geometry(s)[4]) for s in SEAMS}
    assert {o for o, _ in seams} == set(SIZES) and {o for _, o in seams} == set(SIZES)
    p = geometry(next(s for s in SEAMS if s['name'].endswith('x36')))[5]
    assert p['tow'] == 20 and p['tiles_x'] == 2      # (the even spread, and a last tile that owns less than a tile)


@pytest.mark.parametrize('s', FORMS, ids=ids(FORMS))
def test_all_nine_forms_multi_tile(s, dev):
    check_case(s, dev)


@pytest.mark.parametrize('s', LADDER, ids=ids(LADDER))
def test_tile_ladder_and_dispatch(s, dev):
    check_case(s, dev)


@pytest.mark.parametrize('s', SEAMS, ids=ids(SEAMS))
def test_seams_and_ragged_edges(s, dev):
    check_case(s, dev)


@pytest.mark.parametrize('s', PADS, ids=ids(PADS))
def test_negative_and_unequal_padding(s, dev):
    check_case(s, dev)


@pytest.mark.parametrize('s', PARAMS, ids=ids(PARAMS))
def test_parameter_edges(s, dev):
    check_case(s, dev)


def test_non_contiguous_input_multi_tile(dev):
    check_case(case('noncontig', 2, 2, ('1d', 12), ('2d', 11, 12), out=(35, 41), clampq=0.3, seed=600), dev, noncontig=True)
    check_case(case('noncontig_u4d4', 4, 4, ('1d', 24), ('1d', 24), out=(30, 33), clampq=0.3, seed=601), dev, noncontig=True)


def test_clamp_zero_gives_exact_zeros(dev):
    """clamp = 0 is valid: every non-zero sample is clamped to +-0, so y, dx and g2 are exactly 0 (db too), and bit 1 of every sample
    whose float64 value is not 0 is set.  (kink_mask cannot serve here: every sample sits on the clamp edge.)"""
    for s in (case('clamp0', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), clamp=0.0, seed=610),
              case('clamp0_u4d4', 4, 4, ('1d', 24), ('2d', 20, 24), out=(18, 21), clamp=0.0, seed=611),
              case('clamp0_generic', 3, 2, ('1d', 9), ('1d', 6), out=(9, 11), clamp=0.0, seed=612)):
        t, kw = materialise(s)
        hip = run_hip(t, kw, dev)
        for k, v in hip.items():
            assert (v == 0).all(), (s['name'], k, np.abs(v).max())
        _, so = c_call(dev, t, kw, write=True, prefill=0xA5)
        want = flrelu_cpu.sign_bits(t['x'], t['fu'], t['fd'], t['b'], **kw)
        got = flrelu_cpu.unpack_signs(so, want.shape[2], want.shape[3])
        mid = flrelu_cpu.up_stage(t['x'], t['fu'], t['b'], kw['up'], kw['padding'], kw['flip_filter'])[:, :, :want.shape[2], :want.shape[3]]
        sure = mid.abs() > 1e-5 * mid.abs().max()
        assert sure.double().mean() > 0.9 and torch.equal(got[sure], want[sure]) and (got[sure] & 2).all(), s['name']


def test_more_planes_than_a_grid_axis_of_65535(dev):
    """x [1, 70000, 4, 4]: planes ride on blockIdx.x (the fused kernel) and on the flat index (the generic kernels); forward and dx,
    with a bias that differs by channel."""
    from latentaugment_amd import ops
    gen = torch.Generator().manual_seed(77)
    x = torch.randn([1, 70000, 4, 4], generator=gen)
    b = torch.randn([70000], generator=gen)
    for up, down, ntap, pad in ((2, 2, 4, [2, 3, 3, 2]), (3, 1, 6, [2, 3, 3, 2])):
        f = _taps1d(ntap, gen)
        kw = dict(up=up, down=down, padding=pad, gain=SQRT2, slope=0.2, clamp=0.9, flip_filter=False)
        xd = x.to(dev).requires_grad_(True)
        y = ops.filtered_lrelu(xd, f.to(dev), f.to(dev), b.to(dev), **kw)
        dy = torch.randn(y.shape, generator=gen)
        (dx,) = torch.autograd.grad(y, [xd], dy.to(dev))
        ref = {}
        for dtype in (torch.float64, torch.float32):
            xr = x.to(dtype).requires_grad_(True)
            yr = flrelu_cpu.filtered_lrelu(xr, f, f, b, **kw, dtype=dtype)
            (dxr,) = torch.autograd.grad(yr, [xr], dy.to(dtype))
            ref[dtype] = {'y': yr.detach().double().numpy(), 'dx': dxr.double().numpy()}
        mask, _ = flrelu_cpu.kink_mask(x, f, f, b, **kw, rtol=KINK_RTOL)
        _, x_aff = flrelu_cpu.affected(mask, x.shape, f, f, up, down, pad, False)
        ex = {'y': np.zeros(y.shape, bool), 'dx': x_aff.numpy()}
        for k, v in (('y', y), ('dx', dx)):
            check(f'planes_u{up}d{down}', k, v.detach().double().cpu().numpy(), ref[torch.float64][k], ref[torch.float32][k], ex[k])


# ---------------------------------------------------------------- tests: fused against generic
def _append_zero(f):
    return torch.cat([f, f.new_zeros(1)])


@pytest.mark.parametrize('which', ['fu', 'fd'])
@pytest.mark.parametrize('flip', [False, True], ids=['conv', 'flip'])
@pytest.mark.parametrize('up,down', [(2, 2), (4, 1), (1, 4), (4, 4)])
def test_fused_and_generic_agree_on_the_same_operation(dev, up, down, flip, which):
    """A filter of exactly 8 * up (8 * down) taps runs fused (`fut <= 8 * up` in flr_fused_ok).  The same taps with a zero tap appended
    are one tap too many and run on la_flrelu_generic_kernel; moving the padding by one sample (the near side for a convolution, the far
    side for a correlation) makes it the same mathematical operation -- proved here first on the float64 oracle.  Both must meet the
    bound, and their sign buffers must agree sample for sample (an appended fd tap shifts the convolution's intermediate by one)."""
    s = case(f'fg_u{up}d{down}', up, down, ('1d', 8 * up), ('1d', 8 * down), out=smallest_multitile(up, down, ('1d', 8 * up), ('1d', 8 * down)),
             flip=flip, clampq=0.3, seed=700 + 10 * up + down)
    t, kw = materialise(s)
    t2 = dict(t, **{which: _append_zero(t[which])})
    px0, px1, py0, py1 = kw['padding']
    kw2 = dict(kw, padding=[px0, px1 + 1, py0, py1 + 1] if flip else [px0 + 1, px1, py0 + 1, py1])
    fut, fdt = taps_of(s['fus']), taps_of(s['fds'])
    assert geometry(s)[5] is not None
    assert tile_plan(*t['dy'].shape[2:], up, down, (fut[0] + (which == 'fu'),) * 2 + (False,), (fdt[0] + (which == 'fd'),) * 2 + (False,)) is None
    r64, r32 = oracle(t, kw, torch.float64), oracle(t, kw, torch.float32)
    same = oracle(t2, kw2, torch.float64)
    for k in r64:
        np.testing.assert_allclose(same[k], r64[k], rtol=0, atol=1e-12 * np.abs(r64[k]).max(), err_msg=f'{k}: not the same operation')
    ex = masks(t, kw)
    for name, tt, kk in (('fused', t, kw), ('generic', t2, kw2)):
        hip = run_hip(tt, kk, dev)
        for k in hip:
            check(f'{s["name"]} {name}', k, hip[k], r64[k], r32[k], ex[k])
    _, so_f = c_call(dev, t, kw, write=True, prefill=0xA5)
    _, so_g = c_call(dev, t2, kw2, write=True, prefill=0xA5)
    check_written_signs(s['name'] + ' fused', t, kw, so_f, 0xA5)
    want = flrelu_cpu.sign_bits(t['x'], t['fu'], t['fd'], t['b'], **kw)
    ah, aw = want.shape[2], want.shape[3]
    kink = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=KINK_RTOL)[0] > 0
    shift = 1 if (which == 'fd' and not flip) else 0
    got_f = flrelu_cpu.unpack_signs(so_f, ah, aw)
    got_g = flrelu_cpu.unpack_signs(so_g)[:, :, shift:shift + ah, shift:shift + aw]
    assert got_g.shape == got_f.shape
    assert torch.equal(got_f[~kink], got_g[~kink]), f'{int((got_f != got_g)[~kink].sum())} samples differ between the two paths'


# ---------------------------------------------------------------- tests: the sign buffer, read directly
SIGN_CASES = [
    case('s_u4d4_32taps', 4, 4, ('1d', 32), ('1d', 32), out=(30, 37), clampq=0.3, seed=800),
    case('s_u4d4_2d', 4, 4, ('2d', 20, 24), ('2d', 24, 18), out=(34, 37), flip=True, clampq=0.3, seed=801),
    case('s_u4d1', 4, 1, ('1d', 24), None, out=(67, 70), clampq=0.3, seed=802),
    case('s_u1d4_fd3', 1, 4, ('1d', 5), ('1d', 3), out=(35, 37), clampq=0.3, seed=803),
    case('s_u1d4_fd1', 1, 4, None, None, inp=(140, 135), pad=[0, 0, 0, 0], clampq=0.3, seed=804),
    case('s_u2d2_ow36', 2, 2, ('1d', 12), ('1d', 12), out=(33, 36), clampq=0.3, seed=805),
    case('s_u2d2_ow64', 2, 2, ('1d', 12), ('1d', 12), out=(64, 64), c=1, clampq=0.3, seed=806),
    case('s_u2d4_ow3', 2, 4, ('1d', 12), ('1d', 24), out=(40, 3), clampq=0.3, seed=807),
    case('s_u1d1_oh1', 1, 1, ('2d', 3, 3), ('1d', 5), out=(1, 70), clampq=0.3, seed=808),
    case('s_u2d1_negpad', 2, 1, ('1d', 12), ('2d', 3, 2), inp=(30, 33), pad=[-3, 9, 10, -5], clampq=0.3, seed=809),
    case('s_u1d2_free', 1, 2, ('1d', 7), ('1d', 12), out=(35, 41), seed=810),
    case('s_u4d2', 4, 2, ('1d', 24), ('1d', 12), out=(34, 37), flip=True, clampq=0.3, seed=811),
    case('s_u2d4_r16x16', 2, 4, ('1d', 16), ('1d', 32), out=(26, 29), c=1, clampq=0.3, seed=812),
    case('s_generic_up3', 3, 2, ('1d', 9), ('1d', 6), out=(34, 37), clampq=0.3, seed=813),
    case('s_generic_fu17', 2, 2, ('1d', 17), ('2d', 5, 6), out=(20, 23), n=2, clampq=0.3, seed=814),
]


@pytest.mark.parametrize('prefill', [0x00, 0xA5], ids=['fill00', 'fillA5'])
@pytest.mark.parametrize('s', SIGN_CASES, ids=ids(SIGN_CASES))
def test_written_sign_buffer(s, prefill, dev):
    """write_signs = 1 through the C ABI: which tile writes which byte (`ownx1`, `owny1`, `lastx`, `lasty`, `tx + q < ownx1`), and
    la_flrelu_generic_signs_kernel for the generic path.  Every sample of the active extent must equal the float64 oracle's bits
    (kinks aside, at most 0.1 %); the bytes past the active extent must keep the pre-fill; y must equal the plain call's bit for bit."""
    t, kw = materialise(s)
    p = geometry(s)[5]
    assert s['name'].startswith('s_generic') == (p is None) and (p is None or p['tiles_x'] * p['tiles_y'] >= 2), s['name']
    y, so = c_call(dev, t, kw, write=True, prefill=prefill)
    nk, total = check_written_signs(s['name'], t, kw, so, prefill)
    print(f'{s["name"]}: {nk} kink samples of {total}')
    y_plain, _ = c_call(dev, t, kw)
    assert torch.equal(y, y_plain)
    r64 = flrelu_cpu.filtered_lrelu(t['x'], t['fu'], t['fd'], t['b'], **kw).numpy()
    r32 = flrelu_cpu.filtered_lrelu(t['x'], t['fu'], t['fd'], t['b'], **kw, dtype=torch.float32).double().numpy()
    check(s['name'], 'y', y.numpy(), r64, r32, np.zeros(r64.shape, bool))


OFFSETS = (-5, -1, 0, 1, 3, 7)
READ_CASES = [SIGN_CASES[5], SIGN_CASES[3], SIGN_CASES[1], SIGN_CASES[13],
              case('s_slope15_read', 2, 2, ('1d', 12), ('1d', 12), out=(34, 37), slope=1.5, seed=820),
              case('s_slope0_read', 4, 1, ('1d', 24), ('1d', 3), out=(34, 37), slope=0.0, seed=821)]


@pytest.mark.parametrize('s', READ_CASES, ids=ids(READ_CASES))
def test_sign_read_with_arbitrary_offsets(s, dev):
    """si != NULL through the C ABI (`a.mode == 2`: flr_read_bits at (ty + sy, tx + sx), 0 outside the buffer): a buffer of random bits
    over the documented extent, every offset of OFFSETS on both axes, and windows wholly outside the buffer (every sample times gain)."""
    from latentaugment_amd import _lib
    t, kw = materialise(s)
    kw = dict(kw, clamp=None)      # (the clamp lives in the bits in read mode)
    rows, row_bytes = sign_shape(_lib.load(), t, kw)
    n, c, h, w = t['x'].shape
    fut, fdt = taps_of(s['fus']), taps_of(s['fds'])
    ah, aw = flrelu_cpu.active_shape(t['dy'].shape, t['fd'], kw['down'])
    ew = max(aw, (w - 1) * kw['up'] + fut[1])      # (flr_sign_extent: the samples a row of the buffer holds)
    assert rows == max(ah, (h - 1) * kw['up'] + fut[0]) and row_bytes == 4 * _cdiv(ew, 16)
    gen = torch.Generator().manual_seed(s['seed'])
    bits = torch.randint(0, 4, [n, c, rows, ew], generator=gen, dtype=torch.uint8)
    si = flrelu_cpu.pack_signs(bits, rows, row_bytes)
    mid64 = flrelu_cpu.up_stage(t['x'], t['fu'], t['b'], kw['up'], kw['padding'], kw['flip_filter'])
    mid32 = flrelu_cpu.up_stage(t['x'], t['fu'], t['b'], kw['up'], kw['padding'], kw['flip_filter'], dtype=torch.float32)
    pairs = [(sx, OFFSETS[(i + 2) % len(OFFSETS)]) for i, sx in enumerate(OFFSETS)] + [(0, 0), (7, 7), (-5, -5), (4 * row_bytes + 9, 0), (0, -rows - 3),
                                                                                         (-mid64.shape[3] - 1, 2)]
    for sx, sy in pairs:
        y, _ = c_call(dev, t, kw, si=si, sx=sx, sy=sy)
        a64 = flrelu_cpu.act_read(mid64, bits, sx, sy, kw['gain'], kw['slope'])
        a32 = flrelu_cpu.act_read(mid32, bits, sx, sy, kw['gain'], kw['slope'], dtype=torch.float32)
        r64 = flrelu_cpu.down_stage(a64, t['fd'], kw['down'], kw['flip_filter']).numpy()
        r32 = flrelu_cpu.down_stage(a32, t['fd'], kw['down'], kw['flip_filter'], dtype=torch.float32).double().numpy()
        if abs(sx) > 100 or abs(sy) > 100:
            assert torch.equal(a64, mid64 * kw['gain'])
        check(f'{s["name"]} sx {sx} sy {sy}', 'y', y.numpy(), r64, r32, np.zeros(r64.shape, bool))


# ---------------------------------------------------------------- tests: la_filtered_lrelu_act_f32
def act_call(dev, x, si=None, sx=0, sy=0, gain=SQRT2, slope=0.2, clamp=None, write=False, prefill=0):
    from latentaugment_amd import _lib
    lib = _lib.load()
    n, c, h, w = x.shape
    xd = x.to(dev).contiguous().clone()
    row_bytes = 4 * _cdiv(w, 16)
    so = torch.full([n, c, h, row_bytes], prefill, dtype=torch.uint8, device=dev) if write else None
    sid = None if si is None else si.to(dev).contiguous()
    _lib.check(lib.la_filtered_lrelu_act_f32(_lib.ptr(xd), _lib.ptr(sid), _lib.ptr(so), n, c, h, w, sx, sy, gain, slope,
                                             math.inf if clamp is None else clamp, int(write), _lib.stream_ptr()), 'filtered_lrelu_act')
    torch.cuda.synchronize()
    return xd.double().cpu(), (None if so is None else so.cpu())


ACT_W = (1, 3, 4, 5, 15, 16, 17, 64, 67)


def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize('slope,clamp', [(0.2, 0.75), (0.0, None), (1.5, 1.25), (0.2, 0.0)], ids=['usual', 'slope0', 'slope15', 'clamp0'])
@pytest.mark.parametrize('w', ACT_W)
def test_act_entry_plain_and_write_modes(dev, w, slope, clamp):
    """la_flrelu_act_kernel, modes 0 and 1: values against act_stage, the written bits against the float64 bits of the same float32
    products, the row padding bytes untouched, and the buffer byte for byte the one la_filtered_lrelu_f32 writes for up = down = 1
    without filters on the same x.  gain and slope are float32 values (the ABI's types), so each element is one or two roundings."""
    gain, slope = _f32(0.9 * SQRT2), _f32(slope)
    gen = torch.Generator().manual_seed(900 + w)
    x = torch.randn([2, 3, 7, w], generator=gen)
    want = flrelu_cpu.act_stage(x, gain, slope, clamp)
    a = x.double() * gain
    lre = torch.where(a < 0, a * slope, a)
    bits = (a < 0).to(torch.uint8) | ((lre.abs() > clamp).to(torch.uint8) * 2 if clamp is not None else 0)
    edge = torch.zeros(x.shape, dtype=torch.bool) if not clamp else (lre.abs() - clamp).abs() <= KINK_RTOL * float(a.abs().max())
    assert edge.double().mean() <= MAX_KINK_SIGNS
    y0, _ = act_call(dev, x, gain=gain, slope=slope, clamp=clamp)
    y1, so = act_call(dev, x, gain=gain, slope=slope, clamp=clamp, write=True, prefill=0xA5)
    assert torch.equal(y0, y1)
    assert ((y0 - want).abs() <= EPS32 * want.abs())[~edge].all(), float(((y0 - want).abs() - EPS32 * want.abs())[~edge].max())
    got = flrelu_cpu.unpack_signs(so, 7, w)
    assert torch.equal(got[~edge], bits[~edge])
    assert (so[:, :, :, _cdiv(w, 4):] == 0xA5).all()
    t = dict(x=x, b=None, fu=None, fd=None)
    kw = dict(up=1, down=1, padding=[0, 0, 0, 0], gain=gain, slope=slope, clamp=clamp, flip_filter=False)
    yf, sof = c_call(dev, t, kw, write=True, prefill=0xA5)
    assert torch.equal(sof, so) and torch.equal(yf, y0)


@pytest.mark.parametrize('w', ACT_W)
def test_act_entry_read_mode_with_offsets(dev, w):
    """la_flrelu_act_kernel, mode 2: gain, gain * slope or 0 from random bits at (h + sy, w + sx), gain outside the H x W buffer."""
    gain, slope = _f32(1.7), _f32(0.3)
    gen = torch.Generator().manual_seed(950 + w)
    x = torch.randn([2, 3, 9, w], generator=gen)
    bits = torch.randint(0, 4, [2, 3, 9, w], generator=gen, dtype=torch.uint8)
    si = flrelu_cpu.pack_signs(bits, 9, 4 * _cdiv(w, 16))
    for sx, sy in [(a, b) for a in OFFSETS for b in OFFSETS] + [(w, 0), (0, 9), (-w, -9), (1000, -1000)]:
        y, _ = act_call(dev, x, si=si, sx=sx, sy=sy, gain=gain, slope=slope)
        want = flrelu_cpu.act_read(x, bits, sx, sy, gain, slope)
        if abs(sx) >= w or abs(sy) >= 9:
            assert torch.equal(want, x.double() * gain)
        assert ((y - want).abs() <= EPS32 * want.abs()).all(), (sx, sy, float((y - want).abs().max()))
