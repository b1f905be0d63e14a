"""Deferred ToRGB launches of the synthesis pass (la_synth.hip deferred_images: la_torgb_forward_levels + la_image_chain_forward) against
the schedule they replace, one la_torgb_forward behind every block's conv1 and an up-FIR launch per skip image, which the handle still
runs on request (la_synth_set_torgb_schedule(h, 1)).  Same handle, same latents, same older contents in every buffer: every block
image, the final image and dL/dws of the backward pass behind it must be the same BITS.  The plan test needs no GPU."""
import ctypes as C

import pytest
import torch

PREC = {'f32': 0, 'bf16x3': 1, 'f16x2': 3}
# LA_SYNTH_PLAN_* of include/latentaug_hip.h
PASS_N, LAYER_N, BLOCK_N, MAX_LAYERS, MAX_BLOCKS = 8, 20, 6, 24, 12
B_FUSE_RGB, B_SKIP_UP, B_IMG_ROWS = 0, 1, 2
SKIP_LAUNCH, SKIP_CHAIN = 1, 2
CONFIG_F = [512, 512, 512, 512, 512, 256, 128, 64, 32]      # channels at 4^2 .. 1024^2


def plan_blocks(lib, channels, B, prec, imgc=2, rows=(0, 0), cols=(0, 0)):
    """-> per block (fuse_rgb, skip_up, img_lo, img_hi) of la_synth_plan_query"""
    info = (C.c_long * (PASS_N + LAYER_N * MAX_LAYERS + BLOCK_N * MAX_BLOCKS))()
    R = 4 << (len(channels) - 1)
    rc = lib.la_synth_plan_query(R, imgc, (C.c_int * len(channels))(*channels), B, PREC[prec], rows[0], rows[1], cols[0], cols[1], info)
    assert rc == 0, lib.la_last_error()
    base = PASS_N + LAYER_N * MAX_LAYERS
    return [tuple(info[base + BLOCK_N * k + i] for i in (B_FUSE_RGB, B_SKIP_UP, B_IMG_ROWS, B_IMG_ROWS + 1)) for k in range(len(channels))]


def deferral_blocks(blocks):
    return [k for k, b in enumerate(blocks) if b[1] == SKIP_CHAIN]


def test_plan_names_the_deferral_block():
    """config-f 256^2 in f16x2: the 256^2 block, the only one whose ToRGB is fused; f32: no block fuses, the run ends the pass; config-f
    1024^2: the first of its three fused blocks, the other two keep their up-FIR launch."""
    import os
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    b = plan_blocks(lib, CONFIG_F[:7], 8, 'f16x2')
    assert [x[0] for x in b] == [0] * 6 + [1] and deferral_blocks(b) == [6]
    b = plan_blocks(lib, CONFIG_F[:7], 8, 'f16x2', rows=(38, 218))      # (the loop's window: the 128^2 level of the run is windowed)
    assert deferral_blocks(b) == [6] and b[5][2:] == (18, 110)
    b = plan_blocks(lib, CONFIG_F[:7], 8, 'f32')
    assert [x[0] for x in b] == [0] * 7 and [x[1] for x in b] == [0] * 7
    b = plan_blocks(lib, CONFIG_F, 8, 'f16x2')
    assert [x[0] for x in b] == [0] * 6 + [1] * 3 and [x[1] for x in b] == [0] * 6 + [SKIP_CHAIN, SKIP_LAUNCH, SKIP_LAUNCH]


def state_dict(channels, imgc, wdim, seed):
    """random synthesis network with this channel table (keys as SynthesisEngine reads them), non-zero biases and noise"""
    g = torch.Generator().manual_seed(seed)
    f1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    sd = {}

    def conv(p, cin, cout, res):
        sd[f'{p}.affine.weight'] = torch.randn([cin, wdim], generator=g)
        sd[f'{p}.affine.bias'] = torch.ones([cin])
        sd[f'{p}.weight'] = torch.randn([cout, cin, 3, 3], generator=g)
        sd[f'{p}.bias'] = torch.randn([cout], generator=g) * 0.1
        sd[f'{p}.noise_const'] = torch.randn([res, res], generator=g)
        sd[f'{p}.noise_strength'] = torch.tensor(0.1)

    for k, c in enumerate(channels):
        res = 4 << k
        if k == 0:
            sd['b4.const'] = torch.randn([c, 4, 4], generator=g)
        else:
            conv(f'b{res}.conv0', channels[k - 1], c, res)
        conv(f'b{res}.conv1', c, c, res)
        sd[f'b{res}.torgb.affine.weight'] = torch.randn([c, wdim], generator=g)
        sd[f'b{res}.torgb.affine.bias'] = torch.ones([c])
        sd[f'b{res}.torgb.weight'] = torch.randn([imgc, c, 1, 1], generator=g)
        sd[f'b{res}.torgb.bias'] = torch.randn([imgc], generator=g) * 0.1
        sd[f'b{res}.resample_filter'] = torch.outer(f1, f1) / 64.0
    return sd


# channels at 4^2 .. R^2; `chain`: the blocks la_synth_plan_query must name as deferral points (empty: the run ends the pass)
CASES = {
    'r16_f32_end_of_pass': dict(channels=(16, 16, 8), B=3, prec='f32', imgc=2, chain=[]),
    'r64_f16x2': dict(channels=(32, 32, 32, 16, 16), B=2, prec='f16x2', imgc=2, chain=[]),      # (16 channels at 64^2: no fused ToRGB)
    'r64_f16x2_top_fuses': dict(channels=(32, 32, 32, 32, 32), B=2, prec='f16x2', imgc=2, chain=[4]),
    'r128_window': dict(channels=(32, 32, 32, 16, 16, 16), B=2, prec='f16x2', imgc=2, chain=[], rows=(40, 90), cols=(40, 90)),
    # 64^2 fuses, 128^2 (256 channels) does not: a run that starts above a fused block, on its image, and is windowed
    'r128_window_above_fused': dict(channels=(32, 32, 32, 32, 32, 256), B=2, prec='f16x2', imgc=2, chain=[4], rows=(40, 90), cols=(40, 90)),
    'r128_window_two_fused': dict(channels=(32, 32, 32, 32, 32, 32), B=2, prec='f16x2', imgc=2, chain=[4], rows=(40, 90), cols=(40, 90)),
    # the loop's shape in small: a windowed 128^2 level inside the run, the fused 256^2 block reads the chain's skip image
    'r256_window_top_fuses': dict(channels=(32, 32, 32, 32, 16, 16, 32), B=2, prec='f16x2', imgc=2, chain=[6], rows=(70, 180), cols=(70, 180)),
    'r256_window_end_of_pass': dict(channels=(16,) * 7, B=2, prec='f16x2', imgc=2, chain=[], rows=(70, 180), cols=(70, 180)),
    'r64_imgc1': dict(channels=(32, 32, 32, 32, 32), B=2, prec='f16x2', imgc=1, chain=[4]),
    'r64_imgc3': dict(channels=(32, 32, 32, 32, 32), B=2, prec='f16x2', imgc=3, chain=[4]),
    'r32_c12': dict(channels=(12, 12, 12, 12), B=2, prec='f16x2', imgc=3, chain=[]),
}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


def run_schedule(eng, lib, per_block, case, ws_old, ws, g_old, g_img):
    """whole-frame pass and backward on other latents (older contents everywhere), then the case's pass: -> block images below the top,
    final image, dws, and the block images the older pass left"""
    from latentaugment_amd import _lib
    B, imgc, nb = case['B'], case['imgc'], len(case['channels'])
    rows, cols = case.get('rows', (0, 0)), case.get('cols', (0, 0))
    _lib.check(lib.la_synth_set_torgb_schedule(eng.handle, per_block), 'la_synth_set_torgb_schedule')

    def block_images():
        return [eng._view(lib.la_synth_block_image(eng.handle, k), [B, imgc, 4 << k, 4 << k]).clone() for k in range(nb - 1)]
    eng.forward(ws_old, noise_mode='const')
    eng.backward(g_old)
    old = block_images()
    _lib.check(lib.la_synth_set_row_window(eng.handle, *rows), 'la_synth_set_row_window')
    _lib.check(lib.la_synth_set_col_window(eng.handle, *cols), 'la_synth_set_col_window')
    try:
        # (the top block writes the caller's buffer: known contents, so that the rows a windowed pass leaves alone compare as well)
        img = eng.forward(ws, noise_mode='const', out=torch.full([B, imgc, 4 << (nb - 1), 4 << (nb - 1)], 7.0, device=ws.device))
        blocks = block_images()
        dws = eng.backward(g_img).clone()
    finally:
        _lib.check(lib.la_synth_set_row_window(eng.handle, 0, 0), 'la_synth_set_row_window')
        _lib.check(lib.la_synth_set_col_window(eng.handle, 0, 0), 'la_synth_set_col_window')
        _lib.check(lib.la_synth_set_torgb_schedule(eng.handle, 0), 'la_synth_set_torgb_schedule')
    return blocks, img, dws, old


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_deferred_images_equal_the_per_block_launches(dev, name):
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import SynthesisEngine
    case = CASES[name]
    ch, B, imgc = list(case['channels']), case['B'], case['imgc']
    R, wdim = 4 << (len(ch) - 1), 32
    rows, cols = case.get('rows', (0, 0)), case.get('cols', (0, 0))
    lib = _lib.load()
    plan = plan_blocks(lib, ch, B, case['prec'], imgc, rows, cols)
    assert deferral_blocks(plan) == case['chain'], plan
    eng = SynthesisEngine(state_dict(ch, imgc, wdim, seed=5), dev, max_batch=B, precision=case['prec'])
    gen = torch.Generator().manual_seed(11)
    ws_old = (torch.randn([B, eng.num_ws, wdim], generator=gen) * 2).to(dev)
    ws = torch.randn([B, eng.num_ws, wdim], generator=gen).to(dev)
    g_old = torch.randn([B, imgc, R, R], generator=gen).to(dev)
    g_img = torch.zeros([B, imgc, R, R])
    lo, hi = rows if rows[1] else (0, R)
    clo, chi = cols if cols[1] else (0, R)
    g_img[:, :, lo:hi, clo:chi] = torch.randn([B, imgc, hi - lo, chi - clo], generator=gen)
    g_img = g_img.to(dev)
    want = run_schedule(eng, lib, 1, case, ws_old, ws, g_old, g_img)
    got = run_schedule(eng, lib, 0, case, ws_old, ws, g_old, g_img)
    for k, (a, b) in enumerate(zip(got[0], want[0])):
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, 'block image', k)
    assert torch.isfinite(got[1]).all() and torch.equal(got[1], want[1]), (name, 'final image')
    assert torch.isfinite(got[2]).all() and torch.equal(got[2], want[2]), (name, 'dws')
    assert float(got[2].abs().max()) > 0
    # the older pass left the same contents under both schedules, and a windowed level keeps them in the rows nobody asked for
    for k, (a, b) in enumerate(zip(got[3], want[3])):
        assert torch.equal(a, b), (name, 'older block image', k)
    for k, (_, _, ilo, ihi) in enumerate(plan[:-1]):
        if ihi > 0:
            keep = torch.ones(4 << k, dtype=torch.bool)
            keep[ilo:ihi] = False
            assert keep.any() and torch.equal(got[0][k][:, :, keep], got[3][k][:, :, keep]), (name, 'rows outside the window', k)
            assert not torch.equal(got[0][k][:, :, ilo:ihi], got[3][k][:, :, ilo:ihi]), (name, 'rows of the window', k)
