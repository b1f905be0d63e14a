"""GPU tests: the two flat contraction launches of the TOP up-sampling layer follow the column window of the loop (la_synth_set_col_window on
top of la_synth_set_row_window).  Forward: the merged-phase transposed conv computes the rectangle rows x columns of every phase that the
FIR reads, in 128-pixel tiles flattened over that rectangle.  Backward (fp16 mode): the stride-2 backward-data launch computes the columns of
the gradient at half the resolution that can be non-zero, zero-fills the others of its rows and zeroes the partials of the tile slots it no
longer has.  The reference of every check is the WHOLE-FRAME pass of the same build on the same inputs.

Engines (max_batch 2): 128^2 with channel_max 64 and 256^2 with channel_base 2048 / channel_max 16 -- phases of 65^2 and 129^2, above the
split-K sizes, so the direct flat kernel runs them.  Windows (rows, columns):
  * 128^2 (27, 101) x (27, 101): the 32-column tiles around these columns are the whole row, no column window is planned (rows only) --
    the launches must be today's;
  * 256^2 (38, 219) x (38, 219): the bench's crop; tile columns [32, 224), forward rectangle of a phase 95 rows x 102 columns = 75.7
    tiles (the whole rows: 96 tiles), so it ends inside a 128-pixel tile; backward 99 of 128 columns;
  * 256^2 (38, 219) x (5, 100): tile columns [0, 128) touch the left frame edge (phase columns from 0);
  * 128^2 (27, 101) x (70, 122): tile columns [64, 128) touch the right frame edge (the even phases' last column 64 is inside).
Tolerances: those of test_synthesis_row_window against the whole-frame pass (rtol 1e-5, atol 1e-6 x scale): inside the window the forward
sums are the same sums; the backward regroups per-tile partial sums of the style gradient (float32 sums of a few thousand terms)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sg2_networks as nets   # noqa: E402  (generator weights only; nothing is computed on the CPU)

ENGINES = {128: dict(channel_base=4096, channel_max=64), 256: dict(channel_base=2048, channel_max=16)}
# (res, rows, cols, a column window is planned)
WINDOWS = [
    pytest.param(128, (27, 101), (27, 101), False, id='128-square'),
    pytest.param(256, (38, 219), (38, 219), True, id='256-square'),
    pytest.param(256, (38, 219), (5, 100), True, id='256-left-edge'),
    pytest.param(128, (27, 101), (70, 122), True, id='128-right-edge'),
]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


_generators, _engines = {}, {}


def generator(res):
    if res not in _generators:
        _generators[res] = nets.make_generator(img_resolution=res, img_channels=2, seed=3, noise_strength=0.1, w_dim=64, mapping_layers=1,
                                               **ENGINES[res])
    return _generators[res]


def engine(res, precision, dev):
    from latentaugment_amd.synthesis import SynthesisEngine
    if (res, precision) not in _engines:
        _engines[res, precision] = SynthesisEngine.from_generator(generator(res), dev, max_batch=2, precision=precision)
    return _engines[res, precision]


def inputs(res, rows, cols, num_ws):
    gen = torch.Generator().manual_seed(9)
    ws_old = torch.randn([2, num_ws, 64], generator=gen) * 3
    ws = torch.randn([2, num_ws, 64], generator=gen)
    g_img = torch.zeros([2, 2, res, res])
    g_img[:, :, rows[0]:rows[1], cols[0]:cols[1]] = torch.randn([2, 2, rows[1] - rows[0], cols[1] - cols[0]], generator=gen)
    g_dense = torch.randn([2, 2, res, res], generator=gen) * 5
    return ws_old, ws, g_img, g_dense


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol)


def set_windows(lib, eng, rows, cols):
    from latentaugment_amd import _lib
    _lib.check(lib.la_synth_set_row_window(eng.handle, rows[0], rows[1]), 'la_synth_set_row_window')
    _lib.check(lib.la_synth_set_col_window(eng.handle, cols[0], cols[1]), 'la_synth_set_col_window')


@pytest.mark.parametrize('precision', ['f16x2', 'bf16x3'])
@pytest.mark.parametrize('res,rows,cols,planned', WINDOWS)
def test_top_up_layer_follows_columns(dev, res, rows, cols, planned, precision):
    """Whole-frame pass, then older contents in every buffer and partial, then the windowed pass: image inside the window and dL/dws equal
    the whole-frame pass; after the windows are cleared the whole-frame pass gives its earlier image and gradient again."""
    import ctypes as C
    from latentaugment_amd import _lib
    lib = _lib.load()
    eng = engine(res, precision, dev)
    nconv = 2 * len(eng.channels) - 1
    win = (C.c_int * 4)()
    _lib.check(lib.la_synth_plan_bwd_window(res, rows[0], rows[1], cols[0], cols[1], nconv - 2, win), 'la_synth_plan_bwd_window')
    assert (win[3] > 0) == planned, list(win)      # (the case exercises what its comment says)
    ws_old, ws, g_img, g_dense = inputs(res, rows, cols, eng.num_ws)
    img_f = eng.forward(ws.to(dev), noise_mode='const').clone()
    dws_f = eng.backward(g_img.to(dev)).clone()
    scale, gscale = float(img_f.abs().max()), float(dws_f.abs().max())
    assert scale > 0 and gscale > 0
    eng.forward(ws_old.to(dev), noise_mode='const')      # older contents everywhere: activations, the transposed conv's scratch ...
    eng.backward(g_dense.to(dev))                        # ... gradient buffers and per-tile partials, all dense and non-zero
    (r0, r1), (c0, c1) = rows, cols
    set_windows(lib, eng, rows, cols)
    try:
        img = eng.forward(ws.to(dev), noise_mode='const')
        ferr = float((img[:, :, r0:r1, c0:c1] - img_f[:, :, r0:r1, c0:c1]).abs().max())
        dws = eng.backward(g_img.to(dev)).clone()
        gerr = float((dws - dws_f).abs().max())
        print(f'res {res} {precision} rows {rows} cols {cols}: max |img - whole frame| in the window {ferr:.3e} of scale {scale:.3e}; '
              f'max |dws - whole frame| {gerr:.3e} of {gscale:.3e}')
        close(img[:, :, r0:r1, c0:c1], img_f[:, :, r0:r1, c0:c1], rtol=1e-5, atol=1e-6 * scale)
        close(dws, dws_f, rtol=1e-5, atol=1e-6 * gscale)
    finally:
        set_windows(lib, eng, (0, 0), (0, 0))
    close(eng.forward(ws.to(dev), noise_mode='const'), img_f, rtol=1e-5, atol=1e-6 * scale)
    close(eng.backward(g_img.to(dev)), dws_f, rtol=1e-5, atol=1e-6 * gscale)


_ZT_WORKER = r"""
import ctypes as C
import sys
sys.path.insert(0, sys.argv[1])
import torch
from latentaugment_amd import _lib
_lib.select_dev_build()
from latentaugment_amd.synthesis import SynthesisEngine
from oracle import sg2_networks as nets
res, rows, cols = 256, (38, 219), (38, 219)
dev = torch.device('cuda', 0)
G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=2048, channel_max=16, seed=3, noise_strength=0.1, w_dim=64, mapping_layers=1)
eng = SynthesisEngine.from_generator(G, dev, max_batch=2, precision='f16x2')
lib = _lib.load()
lib.la_synth_dev_zt.restype = C.c_void_p
lib.la_synth_dev_zt.argtypes = [C.c_void_p]
gen = torch.Generator().manual_seed(9)
ws_old = torch.randn([2, eng.num_ws, 64], generator=gen) * 3
ws = torch.randn([2, eng.num_ws, 64], generator=gen)
xhalf = (res // 2 + 1 + 3) & ~3
def zt():
    # sample 1 without its first channel: every up-sampling layer uses the same scratch from its start, and the 128^2 layer's
    # 2 x 16 x 129 x 136 floats end inside that channel (the top layer has 8 channels of 257 x 264 floats per sample)
    torch.cuda.synchronize()
    assert eng.channels[-1] == 8
    return eng._view(lib.la_synth_dev_zt(eng.handle), [2, 8, res + 1, 2 * xhalf])[1:, 1:].clone().cpu()
eng.forward(ws_old.to(dev), noise_mode='const')
z_old = zt()
_lib.check(lib.la_synth_set_row_window(eng.handle, *rows), 'row window')
_lib.check(lib.la_synth_set_col_window(eng.handle, *cols), 'col window')
eng.forward(ws.to(dev), noise_mode='const')
z_new = zt()
# intermediate rows 64 .. 191 are inside the wanted rows; even phase columns [13, 115) and odd ones [13, 115) are the rectangle
r = slice(64, 192)
for name, col in (('even phase, column 2', 2), ('even phase, column 126', 126), ('odd phase, column 2', xhalf + 2), ('odd phase, column 125', xhalf + 125)):
    a, b = z_new[:, :, r, col], z_old[:, :, r, col]
    assert float(b.abs().max()) > 0, name
    assert torch.equal(a, b), name + ': written although outside the rectangle'
for name, col in (('even phase, column 13', 13), ('even phase, column 114', 114), ('odd phase, column 60', xhalf + 60)):
    assert not torch.equal(z_new[:, :, r, col], z_old[:, :, r, col]), name + ': not written although inside the rectangle'
print('zt ok')
"""


def test_columns_outside_the_rectangle_are_not_computed(dev, tmp_path):
    """The transposed conv's scratch after a windowed pass still shows the earlier pass in phase columns outside the rectangle, and new
    values inside it (la_synth_dev_zt exists in the development build only, which a process selects before it loads the library: one
    child process)."""
    from latentaugment_amd import _lib
    assert os.path.isfile(_lib.DEV_LIB_PATH), 'development build missing (make -C latentaugment_amd/csrc dev)'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'zt_worker.py'
    script.write_text(_ZT_WORKER)
    p = subprocess.run([sys.executable, str(script), root], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b'zt ok' in p.stdout, p.stdout.decode()[-3000:]
