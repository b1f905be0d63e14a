"""Cases, float64 restatement and dispatch plan of the four modulated-conv layer entries la_modconv3x3_{fwd,up2_fwd,bwd,up2_bwd}_f32
(include/latentaug_hip.h).  Shared by test_modconv_cases_cpu.py (no GPU) and test_hip_modconv_shapes.py (gpu).

Three parts:
  * `restate(case, t, dtype)`: what each entry computes, in plain torch (tap by tap, no library convolution), in the header's non-fused
    formulation.  The backward entries take gz already multiplied by act' and d, so all four are piecewise linear and continuous.
  * `plan(case, precision, with_ws)`: a Python restatement of the C dispatcher -- which kernel form every launch of the call takes.
  * `CASES`: the table.  One row = one entry call; `why` says which edge of the dispatcher or of a kernel the row is there for.
"""
import math
from collections import namedtuple

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------------------------
# constants of the C side
NT = 128                # pixels per tile (la_conv_device.h)
KC = 16                 # channels per chunk, exact-fp32 kernel (la_conv.hip)
KCB = 32                # channels per chunk, 16-bit kernels (la_conv_device.h)
SPLITK_MAX_G = 1156     # la_conv.hip
PM_NS = 8               # la_conv_operand.hip
PRESPLIT_HDR = 512      # la_conv_operand.hip
FIR_ROWS = 8            # la_upfirdn2d.hip
ACT_LINEAR, ACT_LRELU = 1, 3      # LA_ACT_* of include/latentaug_hip.h
SQRT2 = math.sqrt(2.0)
PRECISIONS = (0, 1, 2, 3)         # LA_PREC_F32, LA_PREC_BF16X3, LA_PREC_BF16X2, LA_PREC_F16X2
ENTRIES = ('fwd', 'up2_fwd', 'bwd', 'up2_bwd')


def cdiv(a, b):
    return -(-a // b)


def r256(n):
    return (n + 255) & ~255


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement

def fir_taps(dtype):
    """[1,3,3,1] outer product, normalised, with the up-sampling gain 4: every tap a multiple of 1/16."""
    f = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    return (torch.outer(f, f) / 64.0 * 4.0).to(dtype)


def corr3x3(x, W):
    """z[b,o,y,x] = sum_{i,ky,kx} W[o,i,ky,kx] * x[b,i,y+ky-1,x+kx-1], zeros outside (pad 1)."""
    B, C, H, Wd = x.shape
    xp = torch.zeros([B, C, H + 2, Wd + 2], dtype=x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    z = torch.zeros([B, W.shape[0], H, Wd], dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            z += torch.einsum('oi,bihw->bohw', W[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + Wd])
    return z


def corr3x3_adj(g, W):
    """u[b,i,y,x] = sum_{o,ky,kx} W[o,i,ky,kx] * g[b,o,y-ky+1,x-kx+1]: the adjoint of corr3x3 in x."""
    B, M, H, Wd = g.shape
    gp = torch.zeros([B, M, H + 2, Wd + 2], dtype=g.dtype)
    gp[:, :, 1:-1, 1:-1] = g
    u = torch.zeros([B, W.shape[1], H, Wd], dtype=g.dtype)
    for ky in range(3):
        for kx in range(3):
            u += torch.einsum('oi,bohw->bihw', W[:, :, ky, kx], gp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + Wd])
    return u


def tconv3x3_s2(x, W):
    """Stride-2 transposed convolution to (2h+1)^2: t[b,o,2y+ky,2x+kx] += W[o,i,ky,kx] * x[b,i,y,x]."""
    B, C, H, Wd = x.shape
    t = torch.zeros([B, W.shape[0], 2 * H + 1, 2 * Wd + 1], dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            t[:, :, ky:ky + 2 * H:2, kx:kx + 2 * Wd:2] += torch.einsum('oi,bihw->bohw', W[:, :, ky, kx], x)
    return t


def tconv3x3_s2_adj(a, W):
    """u[b,i,y,x] = sum_{o,ky,kx} W[o,i,ky,kx] * a[b,o,2y+ky,2x+kx]: the adjoint of tconv3x3_s2 (a stride-2 gather with corner taps)."""
    B, M, H1, W1 = a.shape
    H, Wd = (H1 - 1) // 2, (W1 - 1) // 2
    u = torch.zeros([B, W.shape[1], H, Wd], dtype=a.dtype)
    for ky in range(3):
        for kx in range(3):
            u += torch.einsum('oi,bohw->bihw', W[:, :, ky, kx], a[:, :, ky:ky + 2 * H:2, kx:kx + 2 * Wd:2])
    return u


def fir_pad1(t):
    """y[r,c] = sum_{i,j} k[i,j] * t[r+i-1, c+j-1], zeros outside: (n+1)^2 -> n^2.  (k is symmetric: convolution = correlation.)"""
    k = fir_taps(t.dtype)
    B, C, H1, W1 = t.shape
    n, m = H1 - 1, W1 - 1
    tp = torch.zeros([B, C, H1 + 2, W1 + 2], dtype=t.dtype)
    tp[:, :, 1:-1, 1:-1] = t
    y = torch.zeros([B, C, n, m], dtype=t.dtype)
    for i in range(4):
        for j in range(4):
            y += k[i, j] * tp[:, :, i:i + n, j:j + m]
    return y


def fir_pad1_adj(g):
    """a[R,C] = sum_{i,j} k[i,j] * g[R+1-i, C+1-j], zeros outside: n^2 -> (n+1)^2, the adjoint of fir_pad1."""
    k = fir_taps(g.dtype)
    B, C, n, m = g.shape
    gp = torch.zeros([B, C, n + 5, m + 5], dtype=g.dtype)      # g at offset 2: index R + 1 - i + 2 = R + 3 - i in [0, n + 3]
    gp[:, :, 2:2 + n, 2:2 + m] = g
    a = torch.zeros([B, C, n + 1, m + 1], dtype=g.dtype)
    for i in range(4):
        for j in range(4):
            a += k[i, j] * gp[:, :, 3 - i:3 - i + n + 1, 3 - j:3 - j + m + 1]
    return a


def epilogue(z, t, o, dtype):
    """y = clamp(act(z * d + noise * strength + bias) * gain)"""
    v = z
    if t['d'] is not None:
        v = v * t['d'].to(dtype)[:, :, None, None]
    nz = t['noise'].to(dtype)
    nz = nz[:, None] if nz.ndim == 3 else nz[None, None]
    v = v + nz * torch.tensor(o['noise_strength'], dtype=torch.float32).to(dtype) + t['bias'].to(dtype)[None, :, None, None]
    if o['act'] == 'lrelu':
        v = torch.where(v > 0, v, v * torch.tensor(o['alpha'], dtype=torch.float32).to(dtype))
    v = v * torch.tensor(o['gain'], dtype=torch.float32).to(dtype)
    if o['clamp'] >= 0:
        v = v.clamp(-o['clamp'], o['clamp'])
    return v


def restate(case, t, dtype):
    """The entry of `case` on the tensors `t` (float32, as the library gets them) evaluated in `dtype`: {'y'} or {'gx', 'ds'}."""
    o = case['opts']
    W, s = t['w'].to(dtype), t['s'].to(dtype)
    B = case['B']
    if case['entry'] in ('fwd', 'up2_fwd'):
        x = t['x'].to(dtype).expand(B, -1, -1, -1)
        xs = x * s[:, :, None, None]
        z = corr3x3(xs, W) if case['entry'] == 'fwd' else fir_pad1(tconv3x3_s2(xs, W))
        return {'y': epilogue(z, t, o, dtype)}
    gz = t['gz'].to(dtype)
    xin = t['xin'].to(dtype).expand(B, -1, -1, -1)
    u = corr3x3_adj(gz, W) if case['entry'] == 'bwd' else tconv3x3_s2_adj(fir_pad1_adj(gz), W)
    return {'gx': u * s[:, :, None, None], 'ds': (u * xin).sum(dim=[2, 3])}


def make_tensors(case, index):
    """float32 inputs of a case, from a CPU generator seeded by the case index.  opts (all optional):
    x_bstride0 / xin_bstride0, noise_per_sample, noise_strength, no_demod, s_pad / d_pad (extra row elements, filled with NaN by the GPU
    test), act / alpha / gain / clamp, exact (small integers: the float64 answer is a float32 number)."""
    o = case['opts']
    gen = torch.Generator().manual_seed(4000 + index)
    B, cin, cout, res = case['B'], case['cin'], case['cout'], case['res']
    up = case['entry'].startswith('up2')
    rin = res // 2 if up else res
    exact = o['exact']

    def rnd(shape, lo=-2, hi=2):
        if exact:
            return torch.randint(lo, hi + 1, shape, generator=gen).float()
        return torch.randn(shape, generator=gen)

    t = {}
    t['w'] = rnd([cout, cin, 3, 3])
    t['s'] = rnd([B, cin], 1, 2) if exact else torch.randn([B, cin], generator=gen) * 0.5 + 1.0
    if case['entry'] in ('fwd', 'up2_fwd'):
        t['x'] = rnd([1 if o['x_bstride0'] else B, cin, rin, rin])
        t['noise'] = rnd([B, res, res] if o['noise_per_sample'] else [res, res])
        t['bias'] = rnd([cout]) if exact else torch.randn([cout], generator=gen) * 0.1
        if o['no_demod']:
            t['d'] = None
        else:      # the coefficients are an INPUT of the entry: made here in float64 and rounded once
            wm = t['w'].double()[None] * t['s'].double()[:, None, :, None, None]
            t['d'] = (wm.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt().float()
    else:
        t['gz'] = rnd([B, cout, res, res])
        t['xin'] = rnd([1 if o['xin_bstride0'] else B, cin, rin, rin])
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatch plan

# cls: profiler class of the contraction launch; mt: row tile; mfma: '32x32x2' (fp32), '32x32' or '16x16x32' (16-bit forms);
# ksplit: K slices (1 = direct); presplit: a pre-split copy of the launch input was made; merged: the four phases in one launch
Launch = namedtuple('Launch', 'cls mt mfma ksplit presplit merged')


class Refused(Exception):
    """The entry returns an error code before the contraction launch."""


def choose_ksplit(bf, tiles, nck, taps, out_bytes):
    """la_conv.hip choose_ksplit, in its float32 arithmetic."""
    f = np.float32
    if bf:
        best, ks = f(1e30), 1
        for k in range(1, min(nck, 16) + 1):
            per = cdiv(nck, k)
            kk = cdiv(nck, per)
            if kk != k:
                continue
            slots = f(tiles * kk) / f(512)
            rounds = f(1) if slots <= f(1) else slots
            cost = rounds * (f(per) * f(taps) * f(1.7) + f(10))
            if kk > 1:
                cost = cost + (f(5) + f((kk + 1) * float(out_bytes) / 3.5e6))
            if cost < best - f(1e-3):
                best, ks = cost, kk
        return ks
    ks = min(cdiv(768, tiles), nck)
    if ks < 2:
        return 1
    return cdiv(nck, cdiv(nck, ks))


def splitk_floats_phases(B, M, C, grids, prec):
    """la_conv.hip la_conv_splitk_floats_phases (grids: [(Gy, Gx)])."""
    bf = prec != 0
    nck = cdiv(C, KCB if bf else KC)
    if nck < 2 or (len(grids) > 1 and not bf):
        return 0
    mtiles = cdiv(M, 128 if M >= 128 else 64)
    tiles = gsum = 0
    for gy, gx in grids:
        if gy * gx > SPLITK_MAX_G:
            return 0
        tiles += cdiv(B * gy * gx, NT)
        gsum += gy * gx
    out_bytes = 4.0 * B * M * gsum
    ks = max(choose_ksplit(bf, tiles * mtiles, nck, 2.25 if len(grids) > 1 else 9.0, out_bytes),
             choose_ksplit(bf, tiles * mtiles, nck, 1.0, out_bytes))
    return ks * B * M * gsum if ks >= 2 else 0


def presplit_hdr_bytes(B, C):
    """la_conv_operand.hip la_conv_presplit_hdr_bytes"""
    return r256(PRESPLIT_HDR + B * C * PM_NS * 4)


def presplit_bytes(B, C, Hin, Win):
    """la_conv_operand.hip la_conv_presplit_bytes"""
    return B * cdiv(C, KCB) * KCB * Hin * Win * 8 + 16 + presplit_hdr_bytes(B, C)


def fir4x4_segments(H, W):
    """la_upfirdn2d.hip la_fir4x4_segments"""
    return cdiv(W, 64) * cdiv(H, 4 * FIR_ROWS)


def phase_grids(hin):
    """la_conv.h la_conv_up2_phase, in the order la_modconv3x3_up2_fwd_ex walks them: (Gy, Gx, taps)."""
    return [(hin if py else hin + 1, hin if px else hin + 1, (1 if py else 2) * (1 if px else 2)) for py in (0, 1) for px in (0, 1)]


def workspace_bytes(B, cin, cout, res, up):
    """la_modconv.hip la_modconv_workspace_bytes"""
    need = 0
    hin = res // 2 if up else res
    for prec in PRECISIONS:
        qf = qb = 0
        if up:
            if prec == 0:
                f = splitk_floats_phases(B, cout, cin, [(hin + 1, hin + 1)], prec)
            else:
                f = splitk_floats_phases(B, cout, cin, [(hin + 1, hin + 1), (hin + 1, hin), (hin, hin + 1), (hin, hin)], prec)
            b = splitk_floats_phases(B, cin, cout, [(hin, hin)], prec)
            if prec:
                qf, qb = presplit_bytes(B, cin, hin, hin), presplit_bytes(B, cout, res + 1, res + 1)
        else:
            f = splitk_floats_phases(B, cout, cin, [(res, res)], prec)
            b = splitk_floats_phases(B, cin, cout, [(res, res)], prec)
            if prec:
                qf, qb = presplit_bytes(B, cin, res, res), presplit_bytes(B, cout, res, res)
        need = max(need, r256(qf) + f * 4, r256(qb) + b * 4)
    return need + r256(B * max(cin, cout) * fir4x4_segments(res + 1, res + 1) * 4)


def uses_halo(prec, in_q, dense3x3, Gy, Gx, C, Hin, Win):
    """la_conv.hip la_conv_bf16_uses_halo (dense3x3: unit strides, no offset, the nine taps within +-1, grid = output)."""
    return (prec != 0 and not in_q and dense3x3 and Gx % 32 == 0 and Gy % 4 == 0 and Gy * Gx >= SPLITK_MAX_G + 1
            and C * Hin * Win < (1 << 28) and C <= 4096)


def conv_launch(prec, B, C, M, grids, Hin, Win, dense3x3, ws_bytes, in_q, counts):
    """la_conv.hip la_conv_plan (what la_conv_launch, la_conv_prepare_input, la_conv_flat_launch and la_conv_halo_launch then read from
    the LaConvPlan): the form of ONE contraction launch.  grids: [(Gy, Gx, taps)], more than one = merged phases.  ws_bytes: what the
    caller hands to the launch.  counts: profiler brackets per class, updated."""
    if M % 4:
        raise Refused('conv: M must be a multiple of 4')
    bf = prec != 0
    merged = len(grids) > 1
    Gy, Gx = grids[0][0], grids[0][1]
    nck = cdiv(C, KCB if bf else KC)
    halo = not merged and uses_halo(prec, in_q, dense3x3, Gy, Gx, C, Hin, Win)
    mt = 128 if M >= 128 else (32 if (M <= 32 and halo) else 64)      # conv_mt
    mtiles = cdiv(M, mt)
    presplit = bool(in_q)
    if bf and not in_q:      # la_conv_prepare_input
        if halo:
            if prec == 3:
                counts['operand_prep'] += 1
                hb = presplit_hdr_bytes(B, C)
                if ws_bytes < hb:
                    raise Refused('conv: split precisions need a workspace')
                if B > 64:
                    raise Refused('conv: at most 64 samples')
                ws_bytes -= hb
        else:
            counts['operand_prep'] += 1
            qb = presplit_bytes(B, C, Hin, Win)
            if ws_bytes < qb:
                raise Refused('conv: split precisions need a workspace')
            if B > 64:
                raise Refused('conv: at most 64 samples')
            ws_bytes = ws_bytes - r256(qb) if ws_bytes > r256(qb) else 0
            presplit = True
    splitk_floats = ws_bytes // 4
    small = all(gy * gx <= SPLITK_MAX_G for gy, gx, _ in grids) and not halo and (bf or not merged)
    gsum = sum(gy * gx for gy, gx, _ in grids)
    tiles_flat = sum(cdiv(B * gy * gx, NT) for gy, gx, _ in grids)
    if splitk_floats >= 1 and small and nck >= 2:
        if merged:
            taps = np.float32(0)
            for gy, gx, nt in grids:
                taps = taps + np.float32(nt) * (np.float32(gy) * np.float32(gx) / np.float32(gsum))
        else:
            taps = np.float32(grids[0][2])
        ks = choose_ksplit(bf, tiles_flat * mtiles, nck, taps, 4.0 * B * M * gsum)
        if ks >= 2 and ks * B * M * gsum <= splitk_floats:
            cls = 'conv_splitk' if bf else 'conv_f32'
            counts[cls] += 1
            mfma = '32x32x2' if not bf else ('16x16x32' if prec == 3 and mt == 128 else '32x32')      # la_conv_flat.hip: FLAT_MF_16
            return Launch(cls, mt, mfma, ks, presplit, merged)
    if not bf:
        counts['conv_f32'] += 1
        return Launch('conv_f32', mt, '32x32x2', 1, False, False)
    if halo:      # la_conv_halo.hip: HALO_MF_F16_16
        counts['conv_halo'] += 1
        return Launch('conv_halo', mt, '16x16x32' if prec == 3 and mt == 128 and C > KCB else '32x32', 1, False, False)
    counts['conv_flat'] += 1      # la_conv_flat.hip: FLAT_MF_16_3BUF
    return Launch('conv_flat', mt, '16x16x32' if prec == 3 and mt == 128 else '32x32', 1, presplit, merged)


# geometry of a launch as la_conv_plan_query names it (LA_CONV_GEOM_* of include/latentaug_hip.h)
GEOM_SAME_FWD, GEOM_SAME_BWD, GEOM_DOWN2, GEOM_UP2_PHASE, GEOM_UP2_MERGED = 0, 1, 2, 3, 7


def launch_specs(case, prec):
    """The contraction launches of an entry call as arguments of conv_launch (geom: what la_conv_plan_query calls that launch), and the
    bytes of the workspace that the entry keeps in front of them: la_modconv.hip la_modconv3x3_{fwd,up2_fwd,bwd,up2_bwd}_ex."""
    B, cin, cout, res = case['B'], case['cin'], case['cout'], case['res']
    e = case['entry']
    hin = res // 2
    if e == 'fwd':
        return [dict(C=cin, M=cout, grids=[(res, res, 9)], Hin=res, dense3x3=True, geom=GEOM_SAME_FWD)], 0, None
    if e == 'bwd':
        return [dict(C=cout, M=cin, grids=[(res, res, 9)], Hin=res, dense3x3=True, geom=GEOM_SAME_BWD)], 0, None
    if e == 'up2_fwd':
        if prec == 0:      # one launch per phase
            return [dict(C=cin, M=cout, grids=[g], Hin=hin, dense3x3=False, geom=GEOM_UP2_PHASE + k)
                    for k, g in enumerate(phase_grids(hin))], 0, None
        # the input is split once, up front, for the merged launch
        return [dict(C=cin, M=cout, grids=phase_grids(hin), Hin=hin, dense3x3=False, geom=GEOM_UP2_MERGED)], 0, (cin, hin)
    # up2_bwd, the path of the public entry (no plane maxima handed in): FIR adjoint into the scratch, then the stride-2 gather;
    # fp16 x2 keeps the plane maxima of the scratch at the head of the workspace
    head = r256(B * cout * fir4x4_segments(res + 1, res + 1) * 4) if prec == 3 else 0
    return [dict(C=cout, M=cin, grids=[(hin, hin, 9)], Hin=res + 1, dense3x3=False, geom=GEOM_DOWN2)], head, None


def launch_inputs(case, prec, ws_bytes, counts):
    """The walk of an entry call up to its contraction launches: (specs, the workspace bytes each launch is handed, its input arrives
    pre-split)."""
    specs, head, up_front = launch_specs(case, prec)
    B = case['B']
    if case['entry'].startswith('up2') and case['res'] % 2:
        raise Refused('output resolution must be even')
    if head and ws_bytes > head:
        ws_bytes -= head
    in_q = False
    if up_front:      # la_conv_prepare_input in la_conv_up2_launch
        C, hin = up_front
        counts['operand_prep'] += 1
        qb = presplit_bytes(B, C, hin, hin)
        if ws_bytes < qb:
            raise Refused('conv: split precisions need a workspace')
        if B > 64:
            raise Refused('conv: at most 64 samples')
        ws_bytes = ws_bytes - r256(qb) if ws_bytes > r256(qb) else 0
        in_q = True
    return specs, ws_bytes, in_q


def new_counts():
    return dict(conv_halo=0, conv_flat=0, conv_splitk=0, conv_f32=0, operand_prep=0)


def _run_plan(case, prec, ws_bytes):
    counts = new_counts()
    specs, ws_bytes, in_q = launch_inputs(case, prec, ws_bytes, counts)
    launches = [conv_launch(prec, case['B'], sp['C'], sp['M'], sp['grids'], sp['Hin'], sp['Hin'], sp['dense3x3'], ws_bytes, in_q, counts)
                for sp in specs]
    return launches, counts


def plan(case, precision, with_ws):
    """Expected form of every contraction launch of the call: {'launches': [Launch], 'counts': {profiler class: brackets},
    'ws_bytes': bytes of workspace to hand in}.

    with_ws = True: the workspace of la_modconv_workspace_bytes.  False: the largest workspace that is one float short of the slice
    partials of every launch that would split, so that the direct kernels serve the call (equal to the full one where nothing splits).

    Mirrors (C function -> here): la_conv_plan (la_conv.hip) -> conv_launch, field by field: LaConvPlan::mt (conv_mt), ksplit (the
    `small` predicate, choose_ksplit -> choose_ksplit), mfma, prep / ws_head (the operand_prep counts and the bytes taken from the
    workspace), cls; its halo predicate la_conv_bf16_uses_halo -> uses_halo; la_modconv_workspace_bytes -> workspace_bytes; the four
    la_modconv3x3_*_ex -> launch_specs / launch_inputs.  test_conv_plan_cpu.py compares every field with la_conv_plan_query."""
    full = workspace_bytes(case['B'], case['cin'], case['cout'], case['res'], 1 if case['entry'].startswith('up2') else 0)
    launches, counts = _run_plan(case, precision, full)
    ws = full
    if not with_ws and any(l.ksplit > 1 for l in launches):
        B = case['B']
        specs, head, up_front = launch_specs(case, precision)
        prefix = head
        if precision:
            if up_front:
                prefix += r256(presplit_bytes(B, up_front[0], up_front[1], up_front[1]))
            else:
                prefix += r256(presplit_bytes(B, specs[0]['C'], specs[0]['Hin'], specs[0]['Hin']))
        need = min(l.ksplit * B * sp['M'] * sum(gy * gx for gy, gx, _ in sp['grids'])
                   for l, sp in zip(launches, specs) if l.ksplit > 1)
        ws = prefix + 4 * need - 4
        launches, counts = _run_plan(case, precision, ws)
        assert all(l.ksplit == 1 for l in launches), (case['name'], precision)
    return {'launches': launches, 'counts': counts, 'ws_bytes': ws}


def splits(case, precision):
    return any(l.ksplit > 1 for l in plan(case, precision, True)['launches'])


def form_key(precision, l):
    """What identifies a kernel instantiation: the template arguments that la_conv_halo_launch, la_conv_flat_launch and la_conv_launch read from the LaConvPlan."""
    return (precision, l.cls if l.cls != 'conv_f32' else ('conv_f32_split' if l.ksplit > 1 else 'conv_f32'), l.mt, l.mfma, l.merged)


def ds_tiles(grid_res):
    """la_conv.hip la_conv_tiles_per_sample"""
    return cdiv(grid_res * grid_res, NT)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table

_DEFAULT_OPTS = dict(x_bstride0=False, xin_bstride0=False, noise_per_sample=False, noise_strength=0.25, no_demod=False, s_pad=0, d_pad=0,
                     act='lrelu', alpha=0.2, gain=SQRT2, clamp=256.0, exact=False)
_EXACT = dict(exact=True, no_demod=True, act='linear', gain=1.0, clamp=-1.0, noise_strength=1.0)


def _c(name, entry, B, cin, cout, res, why, **opts):
    assert entry in ENTRIES and not set(opts) - set(_DEFAULT_OPTS), name
    return dict(name=name, entry=entry, B=B, cin=cin, cout=cout, res=res, why=why, opts=dict(_DEFAULT_OPTS, **opts))


# C = contraction depth (cin forward, cout backward), M = rows (cout forward, cin backward)
CASES = [
    # ---- split-K family, same-resolution entries
    _c('sk_r4_b3', 'fwd', 3, 33, 4, 4, 'B*G = 48: one pixel tile holds every sample; C = 33: second chunk of one channel; M = 4'),
    _c('sk_r6_b5', 'bwd', 5, 60, 64, 6, 'B*G = 180: the second pixel tile starts inside sample 3 and is ragged; M = 60'),
    _c('sk_r6_b5_f', 'fwd', 5, 64, 60, 6, 'the straddling tile through the forward finish pass (noise, bias, demod per sample)'),
    _c('sk_r33', 'fwd', 1, 160, 64, 33, 'odd resolution; C = 160: five chunks, one per 16-bit slice; M = 64'),
    _c('sk_r33_b', 'bwd', 2, 68, 160, 33, 'odd resolution backward, scalar finish pass (rows not multiples of 4); M = 68'),
    _c('sk_r32', 'fwd', 2, 64, 68, 32, 'res 32, vector finish pass; M = 68: second row tile holds 4 rows'),
    _c('sk_r34', 'bwd', 1, 124, 64, 34, 'G = 1156, the split-K bound, last tile holds 4 pixels; M = 124'),
    _c('sk_r34_m128', 'fwd', 2, 33, 128, 34, 'the bound with a 128-row tile and a one-channel chunk; tiles straddle samples'),
    _c('sk_c544', 'bwd', 2, 132, 544, 4, 'C = 544: 17 chunks against the 16-slice cap (9 slices of 2, the last of 1); M = 132'),
    _c('sk_c512', 'fwd', 2, 512, 124, 4, 'C = 512: 16 chunks, 16 slices of one chunk'),
    _c('sk_3p2', 'fwd', 30, 160, 4, 32, 'C = 160 on 240 pixel tiles: the cost model takes 2 slices of 3 + 2 chunks; 30 samples'),
    _c('sk_c32', 'fwd', 2, 32, 132, 8, 'C = 32: one 16-bit chunk, no split even with a workspace (two fp32 chunks); M = 132'),
    _c('sk_c15', 'fwd', 2, 15, 8, 8, 'fp32 chunk of 16: C = 15, one ragged chunk, never split'),
    _c('sk_c16', 'bwd', 2, 8, 16, 8, 'fp32 chunk of 16: C = 16, exactly one chunk'),
    _c('sk_c17', 'fwd', 2, 17, 8, 8, 'fp32 chunk of 16: C = 17, the second chunk holds one channel'),
    # ---- flat direct, same resolution: just past the bound, not whole 4 x 32 tiles
    _c('fl_r35', 'fwd', 2, 33, 36, 35, 'G = 1225, the first size past the bound: never split; ragged last tile, 10 tiles (plain tile order)'),
    _c('fl_r36', 'bwd', 2, 12, 40, 36, 'res 36 backward: rows of 36, tiles cross rows'),
    _c('fl_r48', 'fwd', 1, 40, 132, 48, 'res 48: 18 whole tiles, yet no 32-wide halo tiles; 128-row tile plus a ragged one'),
    # ---- halo
    _c('ha_r64_m28', 'fwd', 3, 8, 28, 64, '32-row halo tiles, ragged in M and C, three samples'),
    _c('ha_r64_m32', 'bwd', 1, 32, 32, 64, '32-row halo tiles, backward epilogue fast path, one chunk'),
    _c('ha_r64_m36', 'fwd', 1, 33, 36, 64, '64-row tile ragged in M; two chunks, the second of one channel'),
    _c('ha_r64_m64', 'bwd', 3, 64, 40, 64, '64-row tile, backward, ragged second chunk, three samples'),
    _c('ha_r64_m128', 'fwd', 1, 96, 128, 64, '128-row tile over three chunks: the 16x16x32 fp16 form'),
    _c('ha_r64_m128_c32', 'bwd', 1, 128, 32, 64, '128-row tile over ONE chunk: the 32x32x16 fp16 form on one halo buffer'),
    _c('ha_r64_m132', 'fwd', 1, 40, 132, 64, '128-row tile and a ragged second row tile'),
    _c('ha_r96', 'fwd', 1, 33, 64, 96, 'res 96: three tiles per row, 72 tiles'),
    _c('ha_r96_b', 'bwd', 3, 28, 8, 96, 'res 96 backward, 32-row tiles, three samples'),
    _c('ha_r160', 'fwd', 1, 40, 132, 160, 'res 160: five tiles per row, 200 tiles; the largest case (1 GFLOP)'),
    _c('ha_r160_b', 'bwd', 1, 128, 8, 160, 'res 160 backward, 128 rows over one chunk'),
    # ---- up-sampling forward, by output resolution
    _c('uf_r4', 'up2_fwd', 3, 33, 4, 4, 'phase grids 3x3 .. 2x2: one tile per phase holds every sample'),
    _c('uf_r8', 'up2_fwd', 2, 160, 60, 8, 'phase grids 5x5 .. 4x4, five chunks: the merged launch splits'),
    _c('uf_r34', 'up2_fwd', 1, 96, 64, 34, 'phase grids 18x18 .. 17x17 (odd rows), res % 4 != 0'),
    _c('uf_r66', 'up2_fwd', 1, 160, 128, 66, 'phase grids up to 34x34, at the bound; res % 4 != 0; 128-row tile'),
    _c('uf_r70', 'up2_fwd', 1, 33, 28, 70, 'phase grids of 36x36 and 35x35: the merged launch runs direct even with a workspace'),
    _c('uf_r128', 'up2_fwd', 1, 40, 32, 128, 'one merged direct launch over 64x64 inputs'),
    _c('uf_r128_m132', 'up2_fwd', 1, 8, 132, 128, 'the same with a 128-row tile and a ragged second one'),
    # ---- up-sampling backward: stride-2 reads, corner taps, M = cin, cout ragged against 32 in the adjoint scratch
    _c('ub_r4', 'up2_bwd', 3, 4, 33, 4, 'grid 2x2 over a 5x5 gradient; M = 4'),
    _c('ub_r8', 'up2_bwd', 2, 64, 40, 8, 'grid 4x4 over 9x9'),
    _c('ub_r34', 'up2_bwd', 1, 60, 33, 34, 'grid 17x17 over 35x35; M = 60'),
    _c('ub_r66', 'up2_bwd', 1, 128, 40, 66, 'grid 33x33 over 67x67: split-K with stride-2 reads; 128-row tile'),
    _c('ub_r70', 'up2_bwd', 1, 36, 8, 70, 'grid 35x35: direct'),
    _c('ub_r128', 'up2_bwd', 1, 32, 40, 128, 'grid 64x64 over 129x129: 32 whole tiles (XCD tile order)'),
    _c('ub_r128_m128', 'up2_bwd', 1, 128, 8, 128, 'the same on a 128-row tile'),
    # ---- argument forms
    _c('arg_fwd', 'fwd', 2, 40, 36, 8, 'x_bstride = 0, per-sample noise, padded style and demod rows, binding clamp, gain != sqrt 2',
       x_bstride0=True, noise_per_sample=True, s_pad=3, d_pad=5, clamp=0.75, gain=1.7),
    _c('arg_fwd_lin', 'fwd', 2, 40, 36, 8, 'd = NULL, noise_strength = 0, linear without clamp',
       no_demod=True, noise_strength=0.0, act='linear', gain=1.0, clamp=-1.0),
    _c('arg_fwd_halo', 'fwd', 3, 8, 28, 64, 'the same argument forms through the halo kernel epilogue',
       x_bstride0=True, noise_per_sample=True, s_pad=3, d_pad=5, clamp=0.75, gain=1.7),
    _c('arg_up', 'up2_fwd', 2, 40, 36, 8, 'x_bstride = 0, per-sample noise, padded rows, binding clamp, gain: the FIR epilogue',
       x_bstride0=True, noise_per_sample=True, s_pad=3, d_pad=5, clamp=0.75, gain=1.7),
    _c('arg_up_lin', 'up2_fwd', 2, 40, 36, 8, 'd = NULL, noise_strength = 0, linear without clamp: the FIR epilogue',
       no_demod=True, noise_strength=0.0, act='linear', gain=1.0, clamp=-1.0),
    _c('arg_bwd', 'bwd', 2, 36, 40, 8, 'xin_bstride = 0, padded style rows', xin_bstride0=True, s_pad=3),
    _c('arg_bwd_halo', 'bwd', 3, 28, 8, 64, 'xin_bstride = 0, padded style rows, halo epilogue', xin_bstride0=True, s_pad=3),
    _c('arg_ub', 'up2_bwd', 2, 36, 40, 8, 'xin_bstride = 0, padded style rows', xin_bstride0=True, s_pad=3),
    # ---- exact cases: integers, the float64 answer is a float32 number
    _c('ex_m64', 'fwd', 2, 64, 64, 8, 'split-K / flat direct on 64 rows; fp32 <64> split and direct', **_EXACT),
    _c('ex_m128', 'fwd', 2, 64, 128, 8, 'split-K / flat direct on 128 rows; fp32 <128> split and direct', **_EXACT),
    _c('ex_halo32', 'fwd', 1, 40, 32, 64, 'halo, 32 rows', **_EXACT),
    _c('ex_halo64', 'bwd', 1, 64, 40, 64, 'halo, 64 rows, backward epilogue', **_EXACT),
    _c('ex_halo128', 'fwd', 1, 40, 128, 64, 'halo, 128 rows, two chunks', **_EXACT),
    _c('ex_halo128_c32', 'fwd', 1, 32, 128, 64, 'halo, 128 rows, one chunk', **_EXACT),
    _c('ex_up_m64', 'up2_fwd', 2, 160, 64, 8, 'merged phases, split and direct, 64 rows', **_EXACT),
    _c('ex_up_m128', 'up2_fwd', 2, 160, 128, 8, 'merged phases, split and direct, 128 rows', **_EXACT),
    _c('ex_ub', 'up2_bwd', 2, 64, 64, 8, 'FIR adjoint (sixteenths) and the stride-2 gather', **_EXACT),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# a subset for the comparison with autograd through the oracle: every entry, both activations
ORACLE_SUBSET = ['sk_r4_b3', 'sk_r6_b5', 'sk_r33', 'fl_r36', 'uf_r8', 'uf_r34', 'ub_r8', 'ub_r34', 'arg_fwd', 'arg_fwd_lin', 'arg_up', 'arg_up_lin',
                 'arg_bwd', 'arg_ub']
