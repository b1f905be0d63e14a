"""The synthesis engine (la_synth.hip, the affine / demod / ToRGB / seam / style-finish kernels of la_style.hip, the ToRGB and the seams fused
into the contraction epilogues; SynthesisEngine) against the float64 restatement of tests/synth_cases.py, layer by layer, at the shapes
no whole-network test runs: img_channels 1 / 3 / 4, a clamp that binds, no clamp, channel tables that are no powers of two, layers
without noise beside layers with it, one block, B < max_batch, B = 1.  Modes f32, bf16x3, f16x2 (bf16x2 is the approximate mode: its
tolerance class is 20 x looser and test_hip_synthesis.py covers it).

Compared per case: the image, every conv layer's saved output (`layer_output`), every style row (`styles`), the gradient of every
style row (`style_grads`) and dws.
GUARDED cases (no float64 pre-activation within g of a kink, proved in test_synth_cases_cpu.py): every element,
    worst |hip - f64| <= K[mode] x worst |f32-CPU - f64| + 2^-23 x max|f64|
with K = 4 / 6.7 / 4.2 for f32 / bf16x3 / f16x2 (the convention of test_hip_engine_shapes.py, not derived here), the image and dws
additionally inside the ceilings of test_synthesis_forward_backward_vs_oracle (image 1e-4 |ref| + 2e-5 max, dws 1e-3 |ref| + 2e-5 max).
BULK cases (R >= 64): relative L2 <= 1.5 x that of the float32 CPU run + 1e-6 on the same outputs.  Windowed cases
(la_synth_set_row_window / la_synth_set_col_window, 16-bit modes): the image inside the window, dws and style_grads as BULK against the
whole-frame float64 restatement with the same g_img (zero outside the window), then a whole frame again.  No element is excluded
anywhere.  The float32 CPU run of the restatement sets every budget; the code under test sets none.  Every comparison prints
`err / budget = ratio` and the k it would have needed.

Measured on an MI355X, largest k any guarded output needed (err minus the rounding floor, over the float32-CPU error) and the
err / budget ratio it had at the K above:
    f32 1.65 (R32-imgc3-B1 layer 5, 0.473)   bf16x3 2.69 (R16-clamp-binds layer 2, 0.431)   f16x2 1.35 (R16-imgc3-ch12-20-8 layer 3, 0.365)
No guarded output exceeded its budget in any mode, so none is judged by a ceiling alone.  Bulk cases, largest relative L2 / budget:
f32 0.318 (R64-rgbfuse-imgc4 layer 8), bf16x3 0.980 (R128-imgc3 dws), f16x2 0.888 (R128-imgc3 dws); windowed cases: 0.795 (R128-imgc3 rows,
dws, bf16x3).  The two 16-bit modes carry 2 .. 7 x the float32 CPU error in the conv-layer style gradients of the 8-channel layers at
32^2 .. 128^2 (largest b32.conv1 of R128-imgc3: 2.7e-6 against 3.7e-7; img_channels 1 and 4 on the same shapes: 1.7e-6, 1.4e-6), the ToRGB rows
stay at the float32 level: operand rounding in front of the cancellation ds_part - s * tot, inside the budget.  The sweep found no defect.
Wall time of the file on the MI355X: 4.6 s for 61 tests (the float64 and float32 CPU runs included; slowest test 1.1 s, the first, which
loads the library).

Which case reaches which branch (generated: python tests/synth_cases.py --table; test_synth_cases_cpu.py compares):
    small ToRGB kernel, IMGC = 1: R8-imgc1, R64-rgbfuse-imgc1, R128-imgc1
    small ToRGB kernel, IMGC = 2: R4-only, R16-clamp-binds, R16-clamp-none, R16-noise-mixed
    small ToRGB kernel, IMGC = 3: R16-imgc3-ch12-20-8, R32-imgc3-B1, R64-rgbfuse-imgc3, R128-imgc3, R256-imgc3-slabs, synth-shrinking-batch
    small ToRGB kernel, IMGC = 4: R16-imgc4, R64-rgbfuse-imgc4, R128-imgc4
    large ToRGB kernel with the up-2 skip, IMGC = 1: R128-imgc1
    large ToRGB kernel with the up-2 skip, IMGC = 3: R128-imgc3, R256-imgc3-slabs
    large ToRGB kernel with the up-2 skip, IMGC = 4: R128-imgc4
    ToRGB fused into the halo forward, IMGC = 1: R64-rgbfuse-imgc1 (bf16x3 f16x2)
    ToRGB fused into the halo forward, IMGC = 3: R64-rgbfuse-imgc3 (bf16x3 f16x2)
    ToRGB fused into the halo forward, IMGC = 4: R64-rgbfuse-imgc4 (bf16x3 f16x2)
    seam kernel with ToRGB backward, IMGC = 1: R8-imgc1, R64-rgbfuse-imgc1, R128-imgc1
    seam kernel with ToRGB backward, IMGC = 2: R4-only, R16-clamp-binds, R16-clamp-none, R16-noise-mixed
    seam kernel with ToRGB backward, IMGC = 3: R16-imgc3-ch12-20-8, R32-imgc3-B1, R64-rgbfuse-imgc3, R128-imgc3, R256-imgc3-slabs, synth-shrinking-batch
    seam kernel with ToRGB backward, IMGC = 4: R16-imgc4, R64-rgbfuse-imgc4, R128-imgc4
    ToRGB backward fused into the up layer's backward, imgc = 1: R8-imgc1 (bf16x3 f16x2), R64-rgbfuse-imgc1 (bf16x3 f16x2), R128-imgc1 (bf16x3 f16x2)
    ToRGB backward fused into the up layer's backward, imgc = 2: R16-clamp-binds (bf16x3 f16x2), R16-clamp-none (bf16x3 f16x2), R16-noise-mixed (bf16x3 f16x2)
    ToRGB backward fused into the up layer's backward, imgc = 3: R16-imgc3-ch12-20-8 (bf16x3 f16x2), R32-imgc3-B1 (bf16x3 f16x2), R64-rgbfuse-imgc3 (bf16x3 f16x2), R128-imgc3 (bf16x3 f16x2), R256-imgc3-slabs (bf16x3 f16x2), synth-shrinking-batch (bf16x3 f16x2)
    ToRGB backward fused into the up layer's backward, imgc = 4: R16-imgc4 (bf16x3 f16x2), R64-rgbfuse-imgc4 (bf16x3 f16x2), R128-imgc4 (bf16x3 f16x2)
    seam kernel in 4 slabs: R256-imgc3-slabs
    one block (backward ends at k == 0): R4-only
    image-gradient pyramid: R16-imgc3-ch12-20-8, R16-imgc4, R16-clamp-binds, R16-clamp-none, R16-noise-mixed, R32-imgc3-B1, R64-rgbfuse-imgc1, R64-rgbfuse-imgc3, R64-rgbfuse-imgc4, R128-imgc1, R128-imgc3, R128-imgc4, R256-imgc3-slabs, synth-shrinking-batch
    no pyramid with two blocks: R8-imgc1
    a clamp that binds: R16-clamp-binds
    conv_clamp None: R16-clamp-none
    channel counts that are no power of two: R16-imgc3-ch12-20-8
    cin < cout in an up layer: R16-imgc3-ch12-20-8, R64-rgbfuse-imgc1, R64-rgbfuse-imgc3, R64-rgbfuse-imgc4
    cin > cout in an up layer: R16-imgc3-ch12-20-8, R32-imgc3-B1, R128-imgc1, R128-imgc3, R128-imgc4, R256-imgc3-slabs
    4-channel layers: R32-imgc3-B1, R256-imgc3-slabs
    a layer without noise beside layers with noise: R16-noise-mixed
    B < max_batch: R16-imgc3-ch12-20-8, R32-imgc3-B1, synth-shrinking-batch
    B = 1: R32-imgc3-B1
    odd B: R4-only, R16-imgc4
    w_dim 24: R16-imgc3-ch12-20-8
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG = -1
MODES = sc.MODES
K = {'f32': 4.0, 'bf16x3': 6.7, 'f16x2': 4.2}
CEIL = {'img': (1e-4, 2e-5), 'dws': (1e-3, 2e-5)}          # (rtol, atol x max|ref|) of test_synthesis_forward_backward_vs_oracle


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _p(t):
    from latentaugment_amd import _lib
    return _lib.ptr(t)


def _s():
    from latentaugment_amd import _lib
    return _lib.stream_ptr()


def _err_text(lib):
    m = lib.la_last_error()
    return m.decode() if m else ''


_REFS = {}


def _ref(case):
    """(G, ws, g_img, float32 run, float64 run) of a case on the CPU, computed once and shared by the modes"""
    if case.name not in _REFS:
        _REFS[case.name] = case.runs()
    return _REFS[case.name]


def _windowed_ref(case, cols):
    """the whole-frame restatements of a case for the g_img that is zero outside the window"""
    key = (case.name, 'window', cols)
    if key not in _REFS:
        G, ws, g_img, _, _ = _ref(case)
        gw = sc.windowed_g_img(case, g_img, cols)
        _REFS[key] = (gw, case.restate(G, ws, gw, torch.float32), case.restate(G, ws, gw, torch.float64))
    return _REFS[key]


def _engine(dev, case, G, mode):
    from latentaugment_amd.synthesis import SynthesisEngine
    eng = SynthesisEngine(G.synthesis.state_dict(), dev, case.max_batch, conv_clamp=case.clamp, precision=mode)
    assert eng.channels == case.channels and eng.img_channels == case.imgc and eng.noise_strengths == case.noise
    return eng


def _run(eng, dev, ws, g_img):
    """dict of the five outputs (CPU copies; the saved activations and styles are read before the backward pass runs)"""
    B = ws.shape[0]
    img = eng.forward(ws.to(dev), noise_mode='const')
    torch.cuda.synchronize()
    out = dict(img=img.cpu(), layers=[eng.layer_output(k, B).cpu() for k in range(eng.num_layers)], styles=eng.styles(B).cpu())
    dws = eng.backward(g_img.to(dev))
    torch.cuda.synchronize()
    out.update(dws=dws.cpu(), dstyles=eng.style_grads(B).cpu())
    return out


def _outputs(got, r32, r64):
    """(name, got, float32 run, float64 run, ceiling) of every compared output, in the order of the pass"""
    rows = [('styles', got['styles'], r32['styles'], r64['styles'], None)]
    rows += [(f'layer {k}', g, a, b, None) for k, (g, a, b) in enumerate(zip(got['layers'], r32['layers'], r64['layers']))]
    rows += [('image', got['img'], r32['img'], r64['img'], 'img'), ('style_grads', got['dstyles'], r32['dstyles'], r64['dstyles'], None),
             ('dws', got['dws'], r32['dws'], r64['dws'], 'dws')]
    assert len(got['layers']) == len(r64['layers'])
    return rows


def _judge(name, mode, got, r32, r64, ceil):
    """guarded criterion on one output; returns the failure text or None (the caller asserts after every output has printed)"""
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, f'{name}: shape {tuple(got.shape)} != {tuple(r64.shape)}'
    err, err32 = sc.worst(got, r64), sc.worst(r32, r64)
    floor = 2.0 ** -23 * float(r64.abs().max())
    bud = K[mode] * err32 + floor
    need = max(err - floor, 0.0) / err32 if err32 > 0 else (0.0 if err <= floor else float('inf'))
    print(f'{name} [{mode}]: err {err:.3e} / budget {bud:.3e} = ratio {err / bud:.3f} (f32-CPU err {err32:.3e}, needs k = {need:.2f})')
    if not bool(torch.isfinite(got).all()):
        return f'{name} [{mode}]: not finite'
    if ceil:
        rtol, atol = CEIL[ceil]
        over = float(((got - r64).abs() - (rtol * r64.abs() + atol * float(r64.abs().max()))).max())
        if over > 0:
            return f'{name} [{mode}]: beyond the ceiling of the older tests by {over:.3e}'
    if not err <= bud:
        return f'{name} [{mode}]: err {err:.3e} > budget {bud:.3e} (needs k = {need:.2f})'
    return None


def _judge_bulk(name, mode, got, r32, r64):
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, f'{name}: shape {tuple(got.shape)} != {tuple(r64.shape)}'
    e, e32 = sc.rel_l2(got, r64), sc.rel_l2(r32, r64)
    bud = 1.5 * e32 + 1e-6
    print(f'{name} [{mode}]: relative L2 {e:.3e} / budget {bud:.3e} = ratio {e / bud:.3f} (f32-CPU {e32:.3e})')
    return None if e <= bud else f'{name} [{mode}]: relative L2 {e:.3e} > budget {bud:.3e}'


def _judge_all(case, mode, got, r32, r64, what=''):
    bad = []
    for name, g, a, b, ceil in _outputs(got, r32, r64):
        full = f'synth {case.name}{what} {name}'
        bad.append(_judge(full, mode, g, a, b, ceil) if case.kind == 'guarded' else _judge_bulk(full, mode, g, a, b))
    bad = [t for t in bad if t]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', sc.SYNTH_CASES, ids=[c.name for c in sc.SYNTH_CASES])
def test_synthesis_sweep(dev, case, mode):
    G, ws, g_img, r32, r64 = _ref(case)
    eng = _engine(dev, case, G, mode)
    _judge_all(case, mode, _run(eng, dev, ws, g_img), r32, r64)


@pytest.mark.parametrize('mode', MODES)
def test_synthesis_shrinking_batch_is_bit_identical_to_a_fresh_engine(dev, mode):
    """B = 4 with ws x 2^3 and g_img x 2^8, then B = 2 plain on the SAME engine: stale slot rows (f16x2: [nconv][B][LA_XS_FAN], their
    addresses move with B), activations and partials behind the live rows must not reach the result"""
    case = sc.SYNTH_SHRINK
    G, ws, g_img, r32, r64 = _ref(case)
    g = torch.Generator().manual_seed(79)
    wsb = torch.randn([case.max_batch, G.num_ws, case.w_dim], generator=g) * sc.SHRINK_WS
    gb = torch.randn([case.max_batch, case.imgc, case.R, case.R], generator=g) * sc.SHRINK_G
    used = _engine(dev, case, G, mode)
    big = _run(used, dev, wsb, gb)
    assert bool(torch.isfinite(big['img']).all()) and bool(torch.isfinite(big['dws']).all())
    one = _run(used, dev, ws, g_img)
    two = _run(_engine(dev, case, G, mode), dev, ws, g_img)
    for key in ('img', 'styles', 'dstyles', 'dws'):
        assert torch.equal(one[key], two[key]), key
    assert all(torch.equal(a, b) for a, b in zip(one['layers'], two['layers']))
    _judge_all(case, mode, one, r32, r64)


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x2'])          # (f32 ignores windows)
@pytest.mark.parametrize('name,cols', sc.SYNTH_WINDOWED, ids=[n + ('-cols' if c else '-rows') for n, c in sc.SYNTH_WINDOWED])
def test_synthesis_windowed(dev, lib, name, cols, mode):
    """image rows (and columns) [R / 4 + 1, 3 R / 4 - 2) after a pass on other latents has left older contents everywhere"""
    from latentaugment_amd import _lib
    case = sc.SYNTH_BY_NAME[name]
    G, ws, g_img, r32f, r64f = _ref(case)
    gw, r32, r64 = _windowed_ref(case, cols)
    lo, hi = sc.window_of(case.R)
    clo, chi = (lo, hi) if cols else (0, case.R)
    eng = _engine(dev, case, G, mode)
    eng.forward((ws * 3).to(dev), noise_mode='const')
    eng.backward((g_img * 5).to(dev))
    _lib.check(lib.la_synth_set_row_window(eng.handle, lo, hi), 'la_synth_set_row_window')
    if cols:
        _lib.check(lib.la_synth_set_col_window(eng.handle, clo, chi), 'la_synth_set_col_window')
    try:
        img = eng.forward(ws.to(dev), noise_mode='const')
        dws = eng.backward(gw.to(dev))
        torch.cuda.synchronize()
        ds = eng.style_grads(case.B).cpu()
        bad = [_judge_bulk(f'synth {name} window image', mode, img.cpu()[:, :, lo:hi, clo:chi], r32['img'][:, :, lo:hi, clo:chi],
                           r64['img'][:, :, lo:hi, clo:chi]),
               _judge_bulk(f'synth {name} window style_grads', mode, ds, r32['dstyles'], r64['dstyles']),
               _judge_bulk(f'synth {name} window dws', mode, dws, r32['dws'], r64['dws'])]
    finally:
        _lib.check(lib.la_synth_set_row_window(eng.handle, 0, 0), 'la_synth_set_row_window')
        _lib.check(lib.la_synth_set_col_window(eng.handle, 0, 0), 'la_synth_set_col_window')
    bad.append(_judge_bulk(f'synth {name} whole frame after the window', mode, eng.forward(ws.to(dev), noise_mode='const'), r32f['img'], r64f['img']))
    bad = [t for t in bad if t]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name,R,channels,imgc,w_dim,where,text', sc.SYNTH_REFUSALS, ids=[r[0] for r in sc.SYNTH_REFUSALS])
def test_synthesis_refusals(lib, dev, name, R, channels, imgc, w_dim, where, text):
    """LA_ERR_ARG with a message, and the device stays usable.  A channel count that is no multiple of 4 and img_channels outside 1..4 are
    refused when the engine is created (and by la_synth_workspace_bytes, which returns 0); w_dim % 4 != 0 is NOT refused at create: the
    first forward pass refuses it (la_affine_forward: 16-byte rows) before any launch."""
    from latentaugment_amd import _lib
    chan = (C.c_int * len(channels))(*channels)
    if where == 'create':
        assert lib.la_synth_workspace_bytes(R, imgc, w_dim, chan, 2) == 0 and text in _err_text(lib), _err_text(lib)
        buf = torch.zeros([1 << 16], dtype=torch.float32, device=dev)
        n, nl = lib.la_synth_num_params(R), 2 * len(channels) - 1
        params = (C.c_void_p * n)(*[buf.data_ptr()] * n)
        ns = (C.c_float * nl)(*[0.0] * nl)
        fir = np.zeros([16], np.float32)
        h = C.c_void_p()
        rc = lib.la_synth_create(R, imgc, w_dim, chan, 256.0, params, n, ns, nl, fir.ctypes.data, 4, 4, 2, _p(buf), buf.numel() * 4, _s(), C.byref(h))
        assert rc == LA_ERR_ARG and not h.value and text in _err_text(lib), _err_text(lib)
    else:
        case = sc.SynthCase(name, R, channels, imgc, 2, w_dim=w_dim)
        G, ws, _ = case.build()
        eng = _engine(dev, case, G, 'f32')
        img = torch.full([2, imgc, R, R], 7.0, device=dev)
        wd = ws.to(dev)
        rc = lib.la_synth_forward(eng.handle, _p(wd), wd.shape[1] * w_dim, w_dim, 2, 1, None, _p(img), _s())
        torch.cuda.synchronize()
        assert rc == LA_ERR_ARG and text in _err_text(lib), _err_text(lib)
        assert bool((img == 7.0).all())          # refused before anything was written
        with pytest.raises(_lib.LatentAugHipError, match=text):
            eng.forward(wd)
    # the device is still usable: a good engine runs and meets its budget
    good = sc.SYNTH_BY_NAME['R4-only']
    G, ws, g_img, r32, r64 = _ref(good)
    _judge_all(good, 'f32', _run(_engine(dev, good, G, 'f32'), dev, ws, g_img), r32, r64, what=f' after refusal {name}')


@pytest.mark.parametrize('mode', MODES)
def test_synthesis_repeat_is_bit_identical(dev, mode):
    case = sc.SYNTH_BY_NAME['R16-imgc3-ch12-20-8']
    G, ws, g_img, _, _ = _ref(case)
    eng = _engine(dev, case, G, mode)
    a, b = _run(eng, dev, ws, g_img), _run(eng, dev, ws, g_img)
    for key in ('img', 'styles', 'dstyles', 'dws'):
        assert torch.equal(a[key], b[key]), key
