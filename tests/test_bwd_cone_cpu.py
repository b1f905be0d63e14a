"""Row windows of the synthesis engine's backward pass (la_synth_plan_bwd_window, host only: no GPU).  The backward pass of a windowed
forward pass computes, per conv output, the 4-row tiles around the CONE of the image window -- the rows in which the gradient of that
output can be non-zero.  Here the cone the library plans is set against the support that autograd finds in the float64 oracle: it must
hold all of it and must not be a tile wider on either side; and at the benchmark's geometry (256^2, centre crop 181 at 38) the backward
launches of the stride-1 layers must have exactly the tiles of the forward launches."""
import ctypes as C
import os

import pytest
import torch

from oracle import sg2_networks as nets

RES = (64, 128, 256)


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def plan(lib, res, rows, cols, conv_index):
    from latentaugment_amd import _lib
    w = (C.c_int * 4)()
    _lib.check(lib.la_synth_plan_bwd_window(res, rows[0], rows[1], cols[0], cols[1], conv_index, w), 'la_synth_plan_bwd_window')
    return tuple(w)


def windows(res):
    """Image row windows at which the forward pass's tile rounding and the need differ: the benchmark's centre crop scaled to res, windows
    that start (end) one row past a 4-row tile edge, a window at the top edge, a thin one."""
    from latentaugment_amd.latent_aug import center_crop_geometry
    crop, off = center_crop_geometry(res)
    q = res // 4
    return [(off, off + crop), (q + 1, 3 * q - 2), (q - 3, 2 * q + 1), (0, q + 2), (2 * q + 1, 2 * q + 3)]


@pytest.fixture(scope='module', params=RES)
def oracle_pass(request):
    """One float64 forward pass of a small generator per resolution, every conv output kept (engine layer order: b4.conv1, then conv0, conv1 of
    every block); the tests differentiate it once per window."""
    res = request.param
    G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=res * 8, channel_max=8, seed=5, noise_strength=0.1, w_dim=16,
                            mapping_layers=1).double()
    old = nets.COMPUTE_DTYPE
    nets.COMPUTE_DTYPE = torch.float64
    outs, hooks = [], []
    try:
        for r in G.synthesis.block_resolutions:
            blk = getattr(G.synthesis, f'b{r}')
            for name in (('conv1',) if r == 4 else ('conv0', 'conv1')):
                hooks.append(getattr(blk, name).register_forward_hook(lambda m, i, o: (o.retain_grad(), outs.append(o))[0]))
        ws = torch.randn([1, G.num_ws, 16], generator=torch.Generator().manual_seed(2), dtype=torch.float64).requires_grad_(True)
        img = G.synthesis(ws, noise_mode='const')
    finally:
        nets.COMPUTE_DTYPE = old
        for h in hooks:
            h.remove()
    assert img.dtype == torch.float64 and len(outs) == 2 * len(G.synthesis.block_resolutions) - 1
    return res, img, outs


def support_rows(g):
    rows = torch.nonzero(g.abs().amax(dim=(0, 1, 3)) > 0).flatten()
    return int(rows[0]), int(rows[-1]) + 1


@pytest.mark.parametrize('wi', range(5))
def test_planned_cone_holds_the_oracle_gradient_and_is_less_than_a_tile_wider(lib, oracle_pass, wi):
    res, img, outs = oracle_pass
    lo, hi = windows(res)[wi]
    g_img = torch.zeros_like(img)
    g_img[:, :, lo:hi] = torch.randn([1, 2, hi - lo, res], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for o in outs:
        o.grad = None
    img.backward(g_img, retain_graph=True)
    windowed = []
    for ci, o in enumerate(outs):
        r = o.shape[2]
        s_lo, s_hi = support_rows(o.grad)
        b_lo, b_hi, c_lo, c_hi = plan(lib, res, (lo, hi), (0, 0), ci)
        print(f'res {res} window [{lo}, {hi}) conv {ci} @{r}: support [{s_lo}, {s_hi}) planned [{b_lo}, {b_hi})')
        assert (c_lo, c_hi) == (0, 0)
        if b_hi == 0:      # whole plane (below 64^2, or the forward pass computes every row there: its backward has no window either)
            assert b_lo == 0
            continue
        windowed.append(ci)
        assert r >= 64 and 0 <= b_lo < b_hi <= r
        assert b_lo <= s_lo and s_hi <= b_hi, 'the gradient is non-zero outside the planned rows'
        assert s_lo - b_lo < 4 and b_hi - s_hi < 4, 'the planned rows exceed the support by a whole tile'
    assert len(outs) - 1 in windowed and len(outs) - 2 in windowed      # the top block is windowed for every window here


def test_whole_frames_have_no_window(lib):
    for ci in range(13):
        assert plan(lib, 256, (0, 0), (0, 0), ci) == (0, 0, 0, 0)
    assert lib.la_synth_plan_bwd_window(256, 0, 0, 0, 0, 13, (C.c_int * 4)()) != 0
    assert lib.la_synth_plan_bwd_window(256, 40, 30, 0, 0, 0, (C.c_int * 4)()) != 0


def test_benchmark_geometry_backward_halo_tiles_equal_the_forward_ones(lib):
    """256^2, image rows and columns [38, 219).  The stride-1 layers' launches work on 4-row x 32-column tiles.  Forward: conv1 at 128^2
    computes rows [16, 112) = 96 tiles per sample, conv1 at 256^2 rows [36, 220) x 6 of 8 tile columns = 276.  The backward contraction of a
    conv1 writes the gradient of conv0's output of its block: the tiles around that cone must be the same count (they were 104 and 288
    while the backward windows were the forward windows grown by a row and rounded again)."""
    def tiles(ci, r):
        b_lo, b_hi, c_lo, c_hi = plan(lib, 256, (38, 219), (38, 219), ci)
        rows = (b_hi + 3) // 4 - b_lo // 4
        return rows * ((c_hi - c_lo) // 32 if c_hi else r // 32)
    nconv = 13
    assert tiles(nconv - 4, 128) == 96       # d(conv0 output) at 128^2: written by the 256 -> 256 backward launch
    assert tiles(nconv - 2, 256) == 276      # d(conv0 output) at 256^2: written by the 128 -> 128 backward launch
    assert plan(lib, 256, (38, 219), (38, 219), nconv - 2)[2:] == (32, 224)
    # the gradients of the conv1 outputs (what those launches read): the image rows, and what the needed conv0 rows above read
    assert plan(lib, 256, (38, 219), (38, 219), nconv - 1) == (38, 219, 0, 0)
    assert tiles(nconv - 3, 128) == 96

