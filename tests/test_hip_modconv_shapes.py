"""The four modulated-conv layer entries la_modconv3x3_{fwd,up2_fwd,bwd,up2_bwd}_f32 on the GPU against their float64 restatement
(modconv_cases.restate), over every case of modconv_cases.CASES and every contraction precision 0..3.

Per case, precision and workspace mode (the full workspace; and, where the plan splits K, the largest one that is a float short of the
slice partials, so that the direct kernels serve the same call): weights packed by the library; y / gx, ds_part, the transposed-conv
scratch and the workspace filled with NaN; ONE call, bracketed by la_prof_begin / la_prof_end_classes.  Then
  * dispatch witness: the per-class launch counts (conv_halo, conv_flat, conv_splitk, conv_f32, operand_prep) equal modconv_cases.plan;
  * every output element is finite, every ds_part[b][i][tile] slot up to la_modconv_ds_tiles included: no entry relies on a zeroed
    ds_part (the header now says so);
  * y, gx and ds = ds_part.sum(-1) against float64 in max norm: err <= K * yardstick + 2e-6 * scale, yardstick = the same restatement
    run in float32 on the CPU, scale = the largest float64 magnitude; no element is left out;
  * exact cases (small integers, the float64 answer is a float32 number) equal it bit for bit, in every form and precision;
  * a second call into fresh NaN-filled buffers gives the same bits (the header's "deterministic slice sum").
test_refusals: M % 4 != 0, odd res on the up entries, null x / weights / y, a 16-bit precision without workspace, with one below the
pre-split copy, without wq, and B = 65: an error code, la_last_error() set, and the device computes on.

K.  Precision 0: 4, the project's rule (test_hip_conv2d_op.py).  Precisions 1-3: no multiple of the yardstick was known at layer level;
measured on one MI355X over the whole table, k = (err - 2e-6 * scale) / yardstick, and K = 2 x the largest k:
  precision 1 (bf16 x3)  largest k 0.63 at sk_c512 without room for the partials (the flat direct kernel: one accumulator walks all 4608
                         terms; err 9.65e-6, yardstick 1.25e-6, scale 4.43); every other row is below the 2e-6 * scale floor.  K = 1.26
  precision 2 (bf16 x2)  largest k 47.94 at arg_fwd_halo, y (err 4.48e-5, yardstick 9.03e-7, scale 0.75), then 41.2 arg_bwd_halo, 37.4
                         ha_r64_m28, 35.0 arg_up.  K = 95.88.  Largest err / scale 5.97e-5, also at arg_fwd_halo: its scale is the binding
                         clamp, 0.75, an order below the values in front of the clamp; 2.4e-5 at arg_up for the same reason; among the rows
                         without a binding clamp 7.3e-6 (ha_r64_m28), 7.0e-6 (sk_r4_b3): the "about 4e-6 per layer" of the header
  precision 3 (fp16 x2)  largest k -0.52 at arg_fwd_halo (err 1.03e-6, yardstick 9.03e-7, scale 0.75): NO row's error reaches the
                         2e-6 * scale floor, largest err / scale 1.38e-6.  Twice a negative k is no bound: K = 0, the floor alone
  (precision 0, for comparison: largest k 1.39 at arg_fwd, against the rule's 4.)
  No k of precision 1 or 3 comes near the 4 above which the issue behind this file asked for a look at the case.

Kernel form -> case (precision: 0 fp32, 1 bf16 x3, 2 bf16 x2, 3 fp16 x2; "/ws" = full workspace, "/no" = without room for the partials):
  la_conv_igemm_kernel<64, split> / <64, direct>      sk_r4_b3, sk_r6_b5, ex_m64 at precision 0, /ws and /no
  la_conv_igemm_kernel<128, split> / <128, direct>    sk_r34_m128, sk_c544, ex_m128 at precision 0, /ws and /no
  la_conv_bf16_kernel<64, split> / <64, direct>       sk_r4_b3 .. sk_r34, sk_c512, ex_m64, ub_r4 .. ub_r34 (stride-2 reads), /ws and /no
  la_conv_bf16_kernel<128, split> / <128, direct>     sk_r34_m128, sk_c544, ex_m128, ub_r66; precision 3: the 16x16x32 forms
                                                      (FLAT_MF_16 split, FLAT_MF_16_3BUF direct); direct only: sk_c32, fl_r48, ub_r128_m128
  ... merged phases, split / direct, 64 rows          uf_r8, uf_r34, ex_up_m64 /ws and /no; direct only: uf_r4, uf_r70, uf_r128
  ... merged phases, split / direct, 128 rows         uf_r66, ex_up_m128 /ws and /no; direct only: uf_r128_m132
  la_conv_bf16_halo_kernel<32>                        ha_r64_m28, ha_r64_m32, ha_r96_b, arg_fwd_halo, arg_bwd_halo, ex_halo32
  la_conv_bf16_halo_kernel<64>                        ha_r64_m36, ha_r64_m64, ha_r96, ex_halo64
  la_conv_bf16_halo_kernel<128>                       ha_r64_m128, ha_r64_m132, ha_r160, ex_halo128 (precision 3: HALO_MF_F16_16);
                                                      ha_r64_m128_c32, ha_r160_b, ex_halo128_c32 (precision 3: HALO_MF_F16_32, one buffer)
  la_conv_splitk_finish_kernel                        every /ws row above; vector form sk_r32, sk_3p2, scalar form the odd grids
  la_presplit_t_kernel, la_plane_absmax / la_xscale   every non-halo row at precisions 1-3 (operand_prep = 1); halo rows at precision 3
Edge -> case:
  one pixel tile holds every sample sk_r4_b3, uf_r4, ub_r4; a tile straddles samples sk_r6_b5, sk_r6_b5_f, sk_r34_m128
  odd resolution sk_r33, sk_r33_b; the 34x34 bound sk_r34, sk_r34_m128, uf_r66 (phases); first size past it fl_r35, uf_r70, ub_r70
  one-channel chunk sk_r4_b3, sk_r34_m128, ha_r64_m36 (16-bit), sk_c17 (fp32); C = 15 / 16 / 17 sk_c15, sk_c16, sk_c17
  slices: 2 sk_r4_b3; 3 + 2 sk_3p2; 16 sk_c512; the cap (17 chunks -> 9 slices of 2, 2, .., 1) sk_c544; one per chunk sk_r33
  M around 32 / 64 / 128: the sk_* rows (4, 60, 64, 68, 124, 128, 132) and the ha_* rows (28, 32, 36, 64, 128, 132)
  tile order: plain fl_r35, fl_r36, fl_r48 (10, 11, 18 tiles); XCD-contiguous every halo row, ub_r128 and the fp32 runs of the ha_* rows
    (a square halo grid always holds a multiple of eight tiles: test_modconv_cases_cpu.py)
  x_bstride = 0, per-sample noise, padded s / d rows with NaN, binding clamp, gain arg_fwd, arg_fwd_halo, arg_up;
  d = NULL, noise_strength = 0, linear arg_fwd_lin, arg_up_lin; xin_bstride = 0 arg_bwd, arg_bwd_halo, arg_ub

Inputs come from a CPU generator seeded by the case index.  Measured on one MI355X: the whole file (241 tests) takes 4 s, most
of it the float64 and float32 CPU restatements.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modconv_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

# err <= K * yardstick + 2e-6 * scale.  Precision 0: the project's rule.  1-3: twice the largest k measured over the table (docstring).
K = {0: 4.0, 1: 1.26, 2: 95.88, 3: 0.0}
PROF_CLASSES = ('conv_halo', 'conv_flat', 'conv_splitk', 'conv_f32', 'operand_prep')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def nan_floats(n, dev):
    return torch.full([max(int(n), 1)], float('nan'), device=dev)


@functools.lru_cache(maxsize=1)
def case_data(name):
    """Inputs and the two CPU restatements of a case, made once and shared by its four precisions; device copies and weight packs."""
    from latentaugment_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    c = mc.BY_NAME[name]
    t = mc.make_tensors(c, mc.CASES.index(c))
    r64 = mc.restate(c, t, torch.float64)
    r32 = {k: v.double() for k, v in mc.restate(c, t, torch.float32).items()}
    o = c['opts']
    B, cin, cout = c['B'], c['cin'], c['cout']
    st = _lib.stream_ptr()
    d = {k: (v.to(dev).contiguous() if v is not None else None) for k, v in t.items()}
    for key, n, pad in (('s', cin, o['s_pad']), ('d', cout, o['d_pad'])):      # padded rows, NaN in the padding
        if d.get(key) is not None and pad:
            p = torch.full([B, n + pad], float('nan'), device=dev)
            p[:, :n] = d[key]
            d[key] = p
    d['wf'] = torch.empty([9, cin, cout], device=dev)
    d['wb'] = torch.empty([9, cout, cin], device=dev)
    _lib.check(lib.la_pack_conv_weights_f32(_lib.ptr(d['w']), _lib.ptr(d['wf']), _lib.ptr(d['wb']), None, cout, cin, 9, st))
    for key, tr in (('wqf', 0), ('wqb', 1)):
        d[key] = torch.empty([lib.la_modconv_bf16_pack_bytes(cin, cout, tr, 3)], dtype=torch.uint8, device=dev)
        _lib.check(lib.la_pack_conv_weights_bf16_f32(_lib.ptr(d['w']), _lib.ptr(d[key]), cout, cin, 9, tr, 3, st))
    torch.cuda.synchronize()
    return c, d, r64, r32


FIR = np.ascontiguousarray((np.outer([1, 3, 3, 1], [1, 3, 3, 1]) / 64.0).astype(np.float32))


def call_entry(lib, c, d, prec, ws, ws_bytes, out, dev):
    """One call of the case's entry into the (NaN-filled) buffers of `out`; returns the library's code."""
    from latentaugment_amd import _lib
    o = c['opts']
    B, cin, cout, res = c['B'], c['cin'], c['cout'], c['res']
    e = c['entry']
    rin = res // 2 if e.startswith('up2') else res
    st = _lib.stream_ptr()
    p = _lib.ptr
    s_stride = cin + o['s_pad']
    wsp = p(ws) if ws_bytes else None
    if e in ('fwd', 'up2_fwd'):
        x_bs = 0 if o['x_bstride0'] else cin * rin * rin
        nz_bs = res * res if o['noise_per_sample'] else 0
        act = mc.ACT_LRELU if o['act'] == 'lrelu' else mc.ACT_LINEAR
        tail = (p(d['noise']), nz_bs, o['noise_strength'], p(d['bias']), act, o['alpha'], o['gain'], o['clamp'])
        head = (p(d['x']), x_bs, p(d['wf']), p(d['wqf']) if prec else None, prec, p(d['s']), s_stride, p(d['d']), cout + o['d_pad'])
        if e == 'fwd':
            return lib.la_modconv3x3_fwd_f32(*head, *tail, p(out['y']), wsp, ws_bytes, B, cin, cout, res, st)
        return lib.la_modconv3x3_up2_fwd_f32(*head, *tail, FIR.ctypes.data, p(out['scratch']), p(out['y']), wsp, ws_bytes, B, cin, cout, res, st)
    xin_bs = 0 if o['xin_bstride0'] else cin * rin * rin
    head = (p(d['gz']), p(d['wb']), p(d['wqb']) if prec else None, prec, p(d['s']), s_stride, p(d['xin']), xin_bs)
    if e == 'bwd':
        return lib.la_modconv3x3_bwd_f32(*head, p(out['gx']), p(out['ds_part']), wsp, ws_bytes, B, cin, cout, res, st)
    return lib.la_modconv3x3_up2_bwd_f32(*head, FIR.ctypes.data, p(out['scratch']), p(out['gx']), p(out['ds_part']), wsp, ws_bytes, B, cin, cout,
                                         res, st)


def fresh_buffers(lib, c, ws_bytes, dev):
    B, cin, cout, res = c['B'], c['cin'], c['cout'], c['res']
    up = c['entry'].startswith('up2')
    out = {}
    if up:
        out['scratch'] = nan_floats(B * cout * (res + 1) * (res + 1), dev)
    if c['entry'] in ('fwd', 'up2_fwd'):
        out['y'] = nan_floats(B * cout * res * res, dev).view(B, cout, res, res)
    else:
        rin = res // 2 if up else res
        tiles = lib.la_modconv_ds_tiles(rin)
        assert tiles == mc.ds_tiles(rin)
        out['gx'] = nan_floats(B * cin * rin * rin, dev).view(B, cin, rin, rin)
        out['ds_part'] = nan_floats(B * cin * tiles, dev).view(B, cin, tiles)
    ws = torch.full([max(ws_bytes, 16)], 0xFF, dtype=torch.uint8, device=dev)      # 0xFFFFFFFF: a NaN in every float
    return out, ws


def run_profiled(lib, c, d, prec, ws_bytes, dev):
    from latentaugment_amd import _lib
    out, ws = fresh_buffers(lib, c, ws_bytes, dev)
    n = lib.la_prof_num_classes()
    ms, launches, flops, nbytes = (C.c_double * n)(), (C.c_long * n)(), (C.c_double * n)(), (C.c_double * n)()
    _lib.check(lib.la_prof_begin())
    rc = call_entry(lib, c, d, prec, ws, ws_bytes, out, dev)
    _lib.check(lib.la_prof_end_classes(ms, launches, flops, nbytes, n))
    _lib.check(rc, c['name'])
    torch.cuda.synchronize()
    from latentaugment_amd.kernel_classes import CLASSES
    counts = {k: int(launches[CLASSES.index(k)]) for k in PROF_CLASSES}
    return out, counts


@pytest.mark.parametrize('prec', mc.PRECISIONS)
@pytest.mark.parametrize('name', [c['name'] for c in mc.CASES])
def test_case(name, prec, dev, lib):
    c, d, r64, r32 = case_data(name)
    up = 1 if c['entry'].startswith('up2') else 0
    assert int(lib.la_modconv_workspace_bytes(c['B'], c['cin'], c['cout'], c['res'], up)) == mc.workspace_bytes(c['B'], c['cin'], c['cout'], c['res'], up)
    for with_ws in (True, False):
        if not with_ws and not mc.splits(c, prec):
            continue
        pl = mc.plan(c, prec, with_ws)
        out, counts = run_profiled(lib, c, d, prec, pl['ws_bytes'], dev)
        tag = f"MODCONV {name} prec {prec} ws {int(with_ws)} {'+'.join(f'{l.cls}/{l.mt}/{l.mfma}/k{l.ksplit}' for l in pl['launches'])}"
        # dispatch witness
        assert counts == pl['counts'], (tag, counts, pl['counts'])
        got = {k: out[k].double().cpu() for k in r64 if k != 'ds'}
        if 'ds_part' in out:
            part = out['ds_part'].double().cpu()
            assert torch.isfinite(part).all(), (tag, 'ds_part has slots that no kernel wrote')
            got['ds'] = part.sum(-1)
        failures = []
        for k, ref in r64.items():
            hip = got[k]
            assert hip.shape == ref.shape
            assert torch.isfinite(hip).all(), (tag, k, 'not finite')
            scale = float(ref.abs().max())
            err = float((hip - ref).abs().max())
            yard = float((r32[k] - ref).abs().max())
            if c['opts']['exact']:
                print(f'{tag} {k} exact err {err:.3e} scale {scale:.3e}')
                if not torch.equal(hip, ref):
                    failures.append((k, 'not exact', err))
                continue
            kk = (err - 2e-6 * scale) / yard if yard > 0 else float('inf')
            bound = K[prec] * yard + 2e-6 * scale
            print(f'{tag} {k} err {err:.3e} yard {yard:.3e} scale {scale:.3e} k {kk:.3f} rel {err / scale:.3e} bound {bound:.3e}')
            if not err <= bound:
                failures.append((k, err, bound, yard, scale))
        assert not failures, (tag, failures)
        # the slice sum is deterministic: a second call into fresh NaN-filled buffers gives the same bits
        out2, ws2 = fresh_buffers(lib, c, pl['ws_bytes'], dev)
        from latentaugment_amd import _lib
        _lib.check(call_entry(lib, c, d, prec, ws2, pl['ws_bytes'], out2, dev))
        torch.cuda.synchronize()
        for k in out:
            if k != 'scratch':
                assert torch.equal(out[k], out2[k]), (tag, k, 'second run differs')


def _refused(lib, rc, what):
    assert rc != 0, what
    msg = lib.la_last_error()
    assert msg and what in msg.decode(), (what, msg)


def test_refusals(dev, lib):
    """Every refusal returns an error code with la_last_error() set, and the device computes on afterwards."""
    base = mc.BY_NAME['sk_r4_b3']

    def attempt(c, prec, what, ws_bytes=None, drop=(), no_wq=False):
        t = mc.make_tensors(c, 0)
        from latentaugment_amd import _lib
        d = {k: (v.to(dev).contiguous() if v is not None else None) for k, v in t.items()}
        B, cin, cout = c['B'], c['cin'], c['cout']
        d['wf'] = torch.zeros([9, cin, cout], device=dev)
        d['wb'] = torch.zeros([9, cout, cin], device=dev)
        for key, tr in (('wqf', 0), ('wqb', 1)):
            d[key] = None if no_wq else torch.zeros([lib.la_modconv_bf16_pack_bytes(cin, cout, tr, 3)], dtype=torch.uint8, device=dev)
        up = 1 if c['entry'].startswith('up2') else 0
        full = max(int(lib.la_modconv_workspace_bytes(B, cin, cout, c['res'] + c['res'] % 2, up)), 1 << 16)
        out, ws = fresh_buffers(lib, dict(c, res=c['res'] + c['res'] % 2), full, dev)
        for k in drop:
            if k in d:
                d[k] = None
            else:
                out[k] = None
        rc = call_entry(lib, c, d, prec, ws, full if ws_bytes is None else ws_bytes, out, dev)
        _refused(lib, rc, what)
        torch.cuda.synchronize()

    up_f, up_b = mc.BY_NAME['uf_r4'], mc.BY_NAME['ub_r4']
    for prec in (0, 1):
        attempt(dict(base, cout=6), prec, 'multiple of 4')
        attempt(dict(mc.BY_NAME['sk_c16'], cin=6), prec, 'multiple of 4')
        attempt(dict(up_f, res=5), prec, 'must be even')
        attempt(dict(up_b, res=5), prec, 'must be even')
    for c, outk in ((base, 'y'), (up_f, 'y'), (mc.BY_NAME['sk_c16'], 'gx'), (up_b, 'gx')):
        ink = 'x' if c['entry'].endswith('fwd') else 'gz'
        wk = 'wf' if c['entry'].endswith('fwd') else 'wb'
        for k in (ink, wk, outk):
            attempt(c, 0, 'null pointer', drop=(k,))
    for prec in (1, 2, 3):
        for c in (base, up_f, mc.BY_NAME['sk_c16'], up_b):
            attempt(c, prec, 'need a workspace', ws_bytes=0)
            C_, hin = (c['cin'], c['res']) if c['entry'] == 'fwd' else (c['cin'], c['res'] // 2) if c['entry'] == 'up2_fwd' else \
                (c['cout'], c['res']) if c['entry'] == 'bwd' else (c['cout'], c['res'] + 1)
            attempt(c, prec, 'need a workspace', ws_bytes=mc.presplit_bytes(c['B'], C_, hin, hin) - 16)
            attempt(c, prec, 'packed bf16 weights', no_wq=True)
        attempt(dict(base, B=65, cin=4, cout=4), prec, 'at most 64 samples')
    # the device is still usable
    c, d, r64, _ = case_data('sk_r4_b3')
    out, _ = run_profiled(lib, c, d, 0, 0, dev)
    assert float((out['y'].double().cpu() - r64['y']).abs().max()) <= 1e-4 * float(r64['y'].abs().max())
