"""The 16-bit contraction paths over operand magnitude and per-sample range (range_cases.py): the four modulated-conv layer entries
la_modconv3x3_{fwd,up2_fwd,bwd,up2_bwd}_f32 at precisions 0..3, and the engines in their f16x2 and bf16x3 modes.

The property that needs no tolerance: multiplying an operand by 2^k changes no significand bit, the data-derived power-of-two operand
scales of LA_PREC_F16X2 then leave the packed 16-bit operands bit-identical, and every float32 rounding commutes with the scaling.  So
out(2^k * operand) == 2^k * out(operand) AS BYTES, per sample, wherever the entry is linear in the operand.  The unscaled results are
judged against float64 by test_hip_modconv_shapes.py / test_hip_synth_shapes.py / test_hip_engine_shapes.py; this file adds no number
of its own to them, and fails on a scale row indexed by the wrong sample, a slot not reset between passes, a reduction that misses
its tail and a dequantisation applied per tile instead of per column.

Layer entries (y / gx, the transposed-conv scratch, ds_part and the workspace filled with NaN before every call but one, below):
  test_uniform   x / gz, W and (gz, xin) scaled by one exponent (range_cases.UNIFORM_K, DS_PAIRS): y / gx and every ds_part slot equal
                 2^k times the unscaled call's, in both workspace modes
  test_mixed     sample b scaled by 2^k_b (gz and xin independently): out[b] == 2^k_b out_unscaled[b]; the same call a second time;
                 then a call with every sample at 2^24 and the mixed call once more INTO THE SAME workspace and buffers, not refilled
                 (a stale scale would sit there): the same bits.  Every sample is also judged against float64 with the shape sweep's
                 K[precision] and floor, yardstick and scale taken per sample
  test_planted   one element at 16x the largest other magnitude, at the edges of the maxima reductions (pl_r128: of both segments of a
                 plane): finite and within the bound (per sample) at every position, and any two positions agree bit for bit where
                 neither plant reaches
  test_zero      a zero sample: forward act(noise_strength * noise + bias) clamped, exactly; backward exactly 0 in gx and every ds_part
                 slot; a zero xin sample: exactly 0 in ds_part, gx unchanged; a zero plane: within the bound; the other samples keep
                 their bits
Every kernel form of precisions 1-3 is under the equality (test_range_cases_cpu.py proves the coverage; the 128-row halo forms, which
only B = 1 rows reach, by the uniform exponents alone).  No form is exempt.

Engines (f16x2 and bf16x3; the smallest generators that reach the halo kernels, res 64 with channel_base = 4096, channel_max = 64, and
res 16 for the split-K family): see the tests' docstrings.

Measured on one MI355X: every equality held at the first run; largest per-sample err / scale against float64, mixed batches 1.8e-6 /
1.3e-6 / 9.6e-6 / 1.1e-6 and planted maxima 1.2e-6 / 1.2e-6 / 1.3e-5 / 8.7e-7 at precisions 0 / 1 / 2 / 3, all inside the shape
sweep's K[precision] and floor.  The whole file (184 tests) takes 5 s, the slowest test 0.3 s.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modconv_cases as mc  # noqa: E402
import range_cases as rc  # noqa: E402
import test_hip_modconv_shapes as shapes  # noqa: E402  (call_entry, fresh_buffers and the bound K of the shape sweep)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def on_device(lib, c, t, dev, prev=None):
    """Device copies of t (padded style / demod rows with NaN in the padding) and the weight packs; `prev`: an earlier result whose packs
    are kept where the weights are the same tensor."""
    from latentaugment_amd import _lib
    o = c['opts']
    B, cin, cout = c['B'], c['cin'], c['cout']
    st = _lib.stream_ptr()
    d = {k: (v.to(dev).contiguous() if v is not None else None) for k, v in t.items()}
    for key, n, pad in (('s', cin, o['s_pad']), ('d', cout, o['d_pad'])):
        if d.get(key) is not None and pad:
            p = torch.full([B, n + pad], float('nan'), device=dev)
            p[:, :n] = d[key]
            d[key] = p
    if prev is not None and prev['_w'] is t['w']:
        for k in ('wf', 'wb', 'wqf', 'wqb', '_w'):
            d[k] = prev[k]
        return d
    d['_w'] = t['w']
    d['wf'] = torch.empty([9, cin, cout], device=dev)
    d['wb'] = torch.empty([9, cout, cin], device=dev)
    _lib.check(lib.la_pack_conv_weights_f32(_lib.ptr(d['w']), _lib.ptr(d['wf']), _lib.ptr(d['wb']), None, cout, cin, 9, st))
    for key, tr in (('wqf', 0), ('wqb', 1)):
        d[key] = torch.full([lib.la_modconv_bf16_pack_bytes(cin, cout, tr, 3)], 0xFF, dtype=torch.uint8, device=dev)
        _lib.check(lib.la_pack_conv_weights_bf16_f32(_lib.ptr(d['w']), _lib.ptr(d[key]), cout, cin, 9, tr, 3, st))
    torch.cuda.synchronize()
    return d


def run(lib, c, d, prec, ws_bytes, dev, reuse=None):
    """One call into NaN-filled buffers and workspace (reuse = (out, ws) of an earlier call: into those, as they are)."""
    from latentaugment_amd import _lib
    out, ws = reuse if reuse is not None else shapes.fresh_buffers(lib, c, ws_bytes, dev)
    _lib.check(shapes.call_entry(lib, c, d, prec, ws, ws_bytes, out, dev), c['name'])
    torch.cuda.synchronize()
    return out, ws


def outputs(out):
    return {k: v for k, v in out.items() if k != 'scratch'}


def ws_modes(c, prec):
    return [(w, mc.plan(c, prec, w)['ws_bytes']) for w in (True, False) if w or mc.splits(c, prec)]


def part_key(k):
    return 'ds' if k == 'ds_part' else k


def assert_scaled(tag, base, got, exps):
    """got[k][b] == 2^exps[k][b] * base[k][b] as bytes, for y / gx and every ds_part slot."""
    for k, v in outputs(got).items():
        assert torch.isfinite(v).all(), (tag, k, 'not finite')
        want = rc.times_pow2(base[k], exps[part_key(k)])
        same = rc.bits(v) == rc.bits(want)
        if not bool(same.all()):
            bad = (~same).flatten(1).any(1).nonzero().flatten().tolist()
            raise AssertionError((tag, k, 'samples that are not 2^k times the unscaled call', bad,
                                  float((v - want).abs().max() / want.abs().max())))


def judge_per_sample(tag, c, got, r64, r32, prec, samples=None):
    """err <= K[prec] * yardstick + 2e-6 * scale with yardstick and scale of EACH sample (the shape sweep takes them over the batch)."""
    failures = []
    worst = 0.0
    res = {k: got[k].double().cpu() for k in r64 if k != 'ds'}
    if 'ds_part' in got:
        res['ds'] = got['ds_part'].double().cpu().sum(-1)
    for k, ref in r64.items():
        for b in range(c['B']) if samples is None else samples:
            scale = float(ref[b].abs().max())
            err = float((res[k][b] - ref[b]).abs().max())
            yard = float((r32[k][b] - ref[b]).abs().max())
            bound = shapes.K[prec] * yard + 2e-6 * scale
            if scale > 0:
                worst = max(worst, err / scale)
            if not err <= bound:
                failures.append((k, b, err, bound, yard, scale))
    print(f'{tag} worst per-sample err / scale {worst:.3e}')
    assert not failures, (tag, failures)


@functools.lru_cache(maxsize=None)
def restated(name, kind, arg=None):
    """(case, tensors, float64 and float32 restatements) of a derived case, shared by its four precisions."""
    if kind == 'mixed':
        c = rc.homogeneous_case(name)
        t = rc.scaled(rc.tensors(c, True), rc.mixed_pattern(c))
    elif kind == 'planted':
        c = rc.base_case(name)
        t = rc.planted(c, rc.tensors(c, False), arg[1], arg[2])
    else:
        c = mc.BY_NAME[name]
        t = rc.zeroed(rc.tensors(c, False), *arg[1:])
    r64 = mc.restate(c, t, torch.float64)
    r32 = {k: v.double() for k, v in mc.restate(c, t, torch.float32).items()}
    return c, t, r64, r32


@functools.lru_cache(maxsize=None)
def reach_of(name, pos):
    return rc.reach(rc.base_case(name), pos[1], pos[2])


@pytest.mark.parametrize('prec', mc.PRECISIONS)
@pytest.mark.parametrize('name', rc.UNIFORM_BASES)
def test_uniform(name, prec, dev, lib):
    c = rc.homogeneous_case(name)
    t = rc.tensors(c, True)
    d0 = on_device(lib, c, t, dev)
    packs = {}
    for with_ws, ws_bytes in ws_modes(c, prec):
        base = outputs(run(lib, c, d0, prec, ws_bytes, dev)[0])
        for k, v in base.items():
            assert torch.isfinite(v).all() and float(v.abs().max()) > 0, (name, k)
        for ptag, k in rc.uniform_patterns(c):
            ts = rc.scaled(t, k)
            if 'w' in k:
                if ptag not in packs:
                    packs[ptag] = on_device(lib, c, ts, dev)
                d = packs[ptag]
            else:
                ts['w'] = t['w']
                d = on_device(lib, c, ts, dev, prev=d0)
            got, _ = run(lib, c, d, prec, ws_bytes, dev)
            assert_scaled(f'RANGE uniform {name} prec {prec} ws {int(with_ws)} {ptag}', base, got, rc.out_exponents(c, k))


@pytest.mark.parametrize('prec', mc.PRECISIONS)
@pytest.mark.parametrize('name', [n for n in rc.MIXED_BASES if rc.mixed_pattern(rc.homogeneous_case(n))])
def test_mixed(name, prec, dev, lib):
    c, tm, r64, r32 = restated(name, 'mixed')
    t = rc.tensors(c, True)
    k = rc.mixed_pattern(c)
    exps = rc.out_exponents(c, k)
    d0 = on_device(lib, c, t, dev)
    tm = dict(tm, w=t['w'])
    dm = on_device(lib, c, tm, dev, prev=d0)
    dsame = on_device(lib, c, dict(rc.scaled(t, rc.same_pattern(c)), w=t['w']), dev, prev=d0)
    for with_ws, ws_bytes in ws_modes(c, prec):
        tag = f'RANGE mixed {name} prec {prec} ws {int(with_ws)}'
        base = outputs(run(lib, c, d0, prec, ws_bytes, dev)[0])
        first, _ = run(lib, c, dm, prec, ws_bytes, dev)
        assert_scaled(tag, base, first, exps)
        judge_per_sample(tag, c, first, r64, r32, prec)
        second, _ = run(lib, c, dm, prec, ws_bytes, dev)
        # every sample at 2^24, then the mixed call into the very same workspace and buffers: nothing of the earlier call's scales survives
        held = run(lib, c, dsame, prec, ws_bytes, dev)
        assert_scaled(tag + ' same', base, held[0], rc.out_exponents(c, rc.same_pattern(c)))
        third, _ = run(lib, c, dm, prec, ws_bytes, dev, reuse=held)
        for kk, v in outputs(first).items():
            assert torch.equal(rc.bits(v), rc.bits(second[kk])), (tag, kk, 'the second mixed call differs')
            assert torch.equal(rc.bits(v), rc.bits(third[kk])), (tag, kk, 'the mixed call after the 2^24 call differs: a stale scale')


@pytest.mark.parametrize('prec', mc.PRECISIONS)
@pytest.mark.parametrize('name', rc.PLANT_BASES)
def test_planted(name, prec, dev, lib):
    c = rc.base_case(name)
    b = rc.plant_sample(c)
    positions = rc.plant_positions(c)
    d0 = on_device(lib, c, rc.tensors(c, False), dev)
    for with_ws, ws_bytes in ws_modes(c, prec):
        results = []
        for pos in positions:
            _, tp, r64, r32 = restated(name, 'planted', pos)
            got, _ = run(lib, c, on_device(lib, c, dict(tp, w=d0['_w']), dev, prev=d0), prec, ws_bytes, dev)
            tag = f'RANGE planted {name} prec {prec} ws {int(with_ws)} {pos[0]}'
            for k, v in outputs(got).items():
                assert torch.isfinite(v).all(), (tag, k, 'not finite: the maximum was missed')
            judge_per_sample(tag, c, got, r64, r32, prec)
            results.append((pos, outputs(got), reach_of(name, pos)))
        # only the plant moved: the scale is the same wherever the maximum sits, so two positions agree wherever neither reaches
        (p0, g0, m0) = results[0]
        for (p1, g1, m1) in results[1:]:
            for k in g0:
                free = ~(m0[part_key(k)] | m1[part_key(k)]).to(dev)
                if k == 'ds_part':
                    free = free[:, :, None].expand_as(g0[k])
                assert not free[b].all() and free[[q for q in range(c['B']) if q != b]].all()
                same = (rc.bits(g0[k]) == rc.bits(g1[k])) | ~free
                assert bool(same.all()), (name, prec, with_ws, k, p0[0], p1[0], 'differ outside both footprints',
                                          (~same).flatten(1).any(1).nonzero().flatten().tolist())


@pytest.mark.parametrize('prec', mc.PRECISIONS)
@pytest.mark.parametrize('name', rc.ZERO_BASES)
def test_zero(name, prec, dev, lib):
    c = mc.BY_NAME[name]
    t = rc.tensors(c, False)
    d0 = on_device(lib, c, t, dev)
    for with_ws, ws_bytes in ws_modes(c, prec):
        base = outputs(run(lib, c, d0, prec, ws_bytes, dev)[0])
        for var in rc.zero_variants(c):
            vtag, key, b, ch = var
            _, tz, r64, r32 = restated(name, 'zero', var)
            got = outputs(run(lib, c, on_device(lib, c, dict(tz, w=t['w']), dev, prev=d0), prec, ws_bytes, dev)[0])
            tag = f'RANGE zero {name} prec {prec} ws {int(with_ws)} {vtag}'
            others = [q for q in range(c['B']) if q != b]
            for k, v in got.items():
                assert torch.isfinite(v).all(), (tag, k, 'not finite')
                assert torch.equal(rc.bits(v[others]), rc.bits(base[k][others])), (tag, k, 'another sample changed')
            if vtag == 'plane':
                judge_per_sample(tag, c, got, r64, r32, prec, samples=[b])
            elif vtag == 'xin_sample':
                assert not got['ds_part'][b].any(), (tag, 'ds_part of a zero xin')
                assert torch.equal(rc.bits(got['gx'][b]), rc.bits(base['gx'][b])), (tag, 'gx changed with xin')
            elif rc.is_fwd(c):
                want = mc.epilogue(torch.zeros([c['B'], c['cout'], c['res'], c['res']]), t, c['opts'], torch.float32)[b].to(dev)
                assert torch.equal(got['y'][b], want), (tag, 'not act(noise_strength * noise + bias)', float((got['y'][b] - want).abs().max()))
            else:
                assert not got['gx'][b].any() and not got['ds_part'][b].any(), (tag, 'a zero gradient sample')


# ---------------------------------------------------------------------------------------------------------------------------------
# engines

ENGINE_MODES = ['f16x2', 'bf16x3']
G_IMG_K = (-40, 20)


def _generator(res, **kw):
    from oracle import sg2_networks as nets
    return nets.make_generator(img_resolution=res, img_channels=2, channel_base=4096, channel_max=64, seed=3, w_dim=64, mapping_layers=1, **kw)


def _same_bits(a, b):
    return torch.equal(rc.bits(a), rc.bits(b))


@pytest.mark.parametrize('mode', ENGINE_MODES)
@pytest.mark.parametrize('res,windowed', [(16, False), (64, False), (64, True)], ids=['r16', 'r64', 'r64-window'])
def test_synthesis_backward_is_linear_in_g_img(dev, lib, res, windowed, mode):
    """SynthesisEngine.backward with g_img[b] scaled by 2^k_b, k = (-40, +20) and swapped: dws[b] and style_grads[b] are 2^k_b times the
    unscaled ones as bytes, whatever pass ran before on the handle (large then tiny, tiny then large, per sample and for the whole
    batch); one sample of g_img zero: exactly 0 for that sample, the other unchanged.  Windowed: rows and columns sc.window_of(res), g_img
    zero outside -- the windowed producers lower the slot rows from fewer workgroups."""
    import synth_cases as sc
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import SynthesisEngine
    G = _generator(res, noise_strength=0.1)
    eng = SynthesisEngine.from_generator(G, dev, max_batch=2, precision=mode)
    gen = torch.Generator().manual_seed(11)
    ws = torch.randn([2, G.num_ws, 64], generator=gen).to(dev)
    g = torch.randn([2, 2, res, res], generator=gen)
    if windowed:
        lo, hi = sc.window_of(res)
        gw = torch.zeros_like(g)
        gw[:, :, lo:hi, lo:hi] = g[:, :, lo:hi, lo:hi]
        g = gw
        _lib.check(lib.la_synth_set_row_window(eng.handle, lo, hi), 'la_synth_set_row_window')
        _lib.check(lib.la_synth_set_col_window(eng.handle, lo, hi), 'la_synth_set_col_window')
    g = g.to(dev)

    def backward(gi):
        eng.forward(ws, noise_mode='const')
        dws = eng.backward(gi).clone()
        torch.cuda.synchronize()
        return dws, eng.style_grads(2).clone()

    try:
        base = backward(g)
        assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in base)
        swapped = tuple(reversed(G_IMG_K))
        # per sample (tiny, large), then (large, tiny); then the whole batch large, tiny, large
        for ks in (G_IMG_K, swapped, (G_IMG_K[1],) * 2, (G_IMG_K[0],) * 2, (G_IMG_K[1],) * 2, G_IMG_K):
            got = backward(rc.times_pow2(g, ks))
            for what, v, b0 in zip(('dws', 'style_grads'), got, base):
                assert _same_bits(v, rc.times_pow2(b0, ks)), (res, mode, windowed, ks, what, 'not 2^k times the unscaled pass')
        gz = g.clone()
        gz[1] = 0
        for what, v, b0 in zip(('dws', 'style_grads'), backward(gz), base):
            assert not v[1].any(), (what, 'of a zero image gradient')
            assert _same_bits(v[0], b0[0]), (what, 'the other sample changed')
    finally:
        _lib.check(lib.la_synth_set_row_window(eng.handle, 0, 0), 'la_synth_set_row_window')
        _lib.check(lib.la_synth_set_col_window(eng.handle, 0, 0), 'la_synth_set_col_window')


@pytest.mark.parametrize('mode', ENGINE_MODES)
@pytest.mark.parametrize('res', [16, 64])
def test_synthesis_forward_is_homogeneous_in_the_constant(dev, res, mode):
    """A homogeneous generator (noise_strength = 0, conv and ToRGB biases zero, no conv_clamp): the constant input multiplied in place by
    2^k between two passes on the same engine, k = -30 and +10, gives 2^k times the first image as bytes."""
    from latentaugment_amd.synthesis import SynthesisEngine
    G = _generator(res, noise_strength=0.0, conv_clamp=None)
    with torch.no_grad():
        for n, p in G.synthesis.named_parameters():
            if n.endswith('.bias') and '.affine.' not in n:
                p.zero_()
    eng = SynthesisEngine(G.synthesis.state_dict(), dev, max_batch=2, conv_clamp=None, precision=mode)
    assert eng.conv_clamp == -1.0 and all(s == 0.0 for s in eng.noise_strengths)
    const = eng._keep[0]
    assert tuple(const.shape) == tuple(G.synthesis.b4.const.shape)
    ws = torch.randn([2, G.num_ws, 64], generator=torch.Generator().manual_seed(12)).to(dev)
    first = eng.forward(ws, noise_mode='const').clone()
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    for k in (-30, 10):
        const.mul_(2.0 ** k)
        img = eng.forward(ws, noise_mode='const').clone()
        const.mul_(2.0 ** -k)
        assert _same_bits(img, first * 2.0 ** k), (res, mode, k)
    assert _same_bits(eng.forward(ws, noise_mode='const'), first)


@pytest.mark.parametrize('mode', ENGINE_MODES)
def test_feature_backward_is_linear_in_gfeat(dev, mode):
    """la_feat_backward with gfeat[b] scaled per sample: gx[b] is 2^k_b times the unscaled one as bytes.  conv, maxpool, tap at res 128:
    the gradient reaches the conv behind a pool, i.e. la_act_grad_pmax_kernel (both modes), on planes of 128^2 pixels = two segments of
    the plane-maxima pass (no network of engine_cases is larger than res 28, one segment; the case is built from its FeatCase)."""
    import engine_cases as ec
    from latentaugment_amd.synthesis import FeatureEngine
    case = ec.FeatCase('range-res128', 'conv,maxpool,tap', 3, 128, 3, widths=(8,), seed=0)
    assert len(rc.pm_segments(case.res ** 2)) == 2
    ops, x, gfeat = case.build()
    eng = FeatureEngine(ops, dev, in_res=case.res, max_batch=case.N, in_ch=case.in_ch, precision=mode)
    x, gfeat = x.to(dev), gfeat.to(dev)

    def backward(gf):
        eng.forward(x)
        return eng.backward(gf).clone()

    base = backward(gfeat)
    assert torch.isfinite(base).all() and all(float(base[b].abs().max()) > 0 for b in range(case.N))
    for ks in (rc.MIXED_K3, tuple(reversed(rc.MIXED_K3)), (-40, 20, -40), (20, -40, 20)):
        assert _same_bits(backward(rc.times_pow2(gfeat, ks)), rc.times_pow2(base, ks)), (mode, ks)
    gz = gfeat.clone()
    gz[1] = 0
    got = backward(gz)
    assert not got[1].any() and _same_bits(got[[0, 2]], base[[0, 2]])


@pytest.mark.parametrize('mode', ENGINE_MODES)
@pytest.mark.parametrize('res', [16, 64])
def test_discriminator_backward_is_linear_in_dlogits(dev, lib, res, mode):
    """la_disc_backward with dlogits scaled by one 2^k for the whole batch (MinibatchStd couples the samples): g_img is 2^k times the
    unscaled one as bytes, with accumulate = 0 and, onto a preload scaled alike, with accumulate = 1."""
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import DiscriminatorEngine
    from oracle import sg2_networks as nets
    D = nets.make_discriminator(img_resolution=res, img_channels=2, channel_base=4096, channel_max=64, seed=2)
    eng = DiscriminatorEngine(D, dev, max_batch=4, precision=mode)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn([4, 2, res, res], generator=gen).to(dev)
    dl = torch.randn([4], generator=gen).to(dev)
    pre = torch.randn([4, 2, res, res], generator=gen).to(dev) * 1e-3

    def backward(d, preload):
        eng.forward(x)
        if preload is None:
            return eng.backward(d).clone()
        acc = preload.clone()
        _lib.check(lib.la_disc_backward(eng.handle, _lib.ptr(d.contiguous()), _lib.ptr(acc), 1, _lib.stream_ptr()), 'la_disc_backward')
        torch.cuda.synchronize()
        return acc

    plain, summed = backward(dl, None), backward(dl, pre)
    assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0 and not torch.equal(plain, summed)
    for k in (20, -40, 20):
        f = 2.0 ** k
        assert _same_bits(backward(dl * f, None), plain * f), (res, mode, k, 'accumulate 0')
        assert _same_bits(backward(dl * f, pre * f), summed * f), (res, mode, k, 'accumulate 1')
