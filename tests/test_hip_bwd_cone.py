"""GPU: the backward pass of a windowed synthesis pass follows the gradient cone of the image window (la_synth.hip)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sg2_networks as nets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol)


# windows whose forward tile rounding is wider than the need: the benchmark's centre crop scaled to res, one row past a tile edge on either end
@pytest.mark.parametrize('res,cbase,cmax,win', [(64, 2048, 64, (10, 55)), (64, 2048, 64, (17, 45)), (128, 4096, 64, (19, 110)), (128, 4096, 64, (33, 93))])
def test_windowed_backward_equals_whole_frame_backward(dev, res, cbase, cmax, win):
    """Whole-frame forward and backward of OTHER latents and another image gradient first, so that every activation, gradient buffer and
    per-tile partial holds foreign finite values; then the windowed pass: image rows inside the window, dL/dws and the style gradients equal
    the whole-frame pass of the same latents (tolerances of test_synthesis_row_window), and the handle recorded the planned cone."""
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import SynthesisEngine
    lib = _lib.load()
    G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=cbase, channel_max=cmax, seed=3, noise_strength=0.1, w_dim=64,
                            mapping_layers=1)
    eng = SynthesisEngine.from_generator(G, dev, max_batch=2, precision='f16x2')
    gen = torch.Generator().manual_seed(11)
    ws_old = torch.randn([2, G.num_ws, 64], generator=gen) * 3
    ws = torch.randn([2, G.num_ws, 64], generator=gen)
    lo, hi = win
    g_img = torch.zeros([2, 2, res, res])
    g_img[:, :, lo:hi] = torch.randn([2, 2, hi - lo, res], generator=gen)
    img_f = eng.forward(ws.to(dev), noise_mode='const').clone()
    dws_f = eng.backward(g_img.to(dev)).clone()
    ds_f = eng.style_grads(2).clone()
    assert torch.isfinite(dws_f).all() and float(dws_f.abs().max()) > 0
    eng.forward(ws_old.to(dev), noise_mode='const')
    eng.backward((torch.randn(g_img.shape, generator=gen) * 5).to(dev))
    _lib.check(lib.la_synth_set_row_window(eng.handle, lo, hi), 'la_synth_set_row_window')
    try:
        img = eng.forward(ws.to(dev), noise_mode='const')
        scale = float(img_f.abs().max())
        close(img[:, :, lo:hi], img_f[:, :, lo:hi], rtol=1e-5, atol=1e-6 * scale)
        dws = eng.backward(g_img.to(dev))
        close(dws, dws_f, rtol=1e-5, atol=1e-6 * float(dws_f.abs().max()))
        close(eng.style_grads(2), ds_f, rtol=1e-5, atol=1e-6 * float(ds_f.abs().max()))
        nconv = 2 * len(G.synthesis.block_resolutions) - 1
        windowed = 0
        for ci in range(nconv):
            a, b, w = C.c_int(), C.c_int(), (C.c_int * 4)()
            _lib.check(lib.la_synth_bwd_rows(eng.handle, ci, C.byref(a), C.byref(b)), 'la_synth_bwd_rows')
            _lib.check(lib.la_synth_plan_bwd_window(res, lo, hi, 0, 0, ci, w), 'la_synth_plan_bwd_window')
            assert (a.value, b.value) == (w[0], w[1])
            windowed += b.value > 0
        assert windowed >= 2
    finally:
        _lib.check(lib.la_synth_set_row_window(eng.handle, 0, 0), 'la_synth_set_row_window')

