"""filtered_lrelu without a GPU: the Python entry point, the pure host queries of the C ABI, its host-side argument checks, and the
golden file (tests/golden/filtered_lrelu.npz, from the reference) against the float64 restatement in tests/flrelu_cpu.py."""
import ast
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flrelu_cpu  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'filtered_lrelu.npz'))


@pytest.fixture(scope='module')
def gs(golden_dir):
    return np.load(os.path.join(golden_dir, 'flrelu_shapes.npz'))


def cases(g):
    for name in g['cases']:
        name = str(name)
        yield name, ast.literal_eval(str(g[f'{name}_meta']))


def tensors(g, name):
    t = {k: torch.from_numpy(g[f'{name}_{k}']) if f'{name}_{k}' in g else None for k in ('x', 'b', 'fu', 'fd', 'dy', 'v')}
    return t


def taps(f):
    """(rows or 0 for 1-D, cols) of a golden filter."""
    return (1, 1) if f is None else ((0, f.shape[0]) if f.ndim == 1 else tuple(f.shape))


def test_entry_point_refuses_cpu_tensors():
    from latentaugment_amd import _lib, ops
    assert callable(ops.filtered_lrelu)
    with pytest.raises(_lib.LatentAugHipError):
        ops.filtered_lrelu(torch.zeros([1, 1, 4, 4]), up=2, down=2)


def test_out_size_matches_reference_formula(lib):
    for n in (1, 2, 7, 16, 36, 148):
        for up, down in ((1, 1), (2, 1), (1, 2), (2, 2), (4, 2), (2, 4), (3, 2)):
            for p0, p1 in ((0, 0), (11, 10), (-3, 2), (17, 16)):
                for fu, fd in ((1, 1), (12, 12), (24, 12), (5, 40)):
                    want = (n * up + (p0 + p1) - (fu - 1) - (fd - 1) + (down - 1)) // down      # filtered_lrelu.py:141-142
                    assert lib.la_filtered_lrelu_out_size(n, up, down, p0, p1, fu, fd) == want


def sign_shape(lib, *args):
    rows, row_bytes = C.c_int(-1), C.c_int(-1)
    rc = lib.la_filtered_lrelu_sign_shape(*args, C.byref(rows), C.byref(row_bytes))
    return rc, rows.value, row_bytes.value


def test_sign_shape_covers_the_intermediate_and_is_shared_with_the_backward(lib, g):
    for name, m in cases(g):
        t = tensors(g, name)
        (fu_h, fu_w), (fd_h, fd_w) = taps(t['fu']), taps(t['fd'])
        fuy, fdy = fu_h or fu_w, fd_h or fd_w
        _, _, h, w = t['x'].shape
        _, _, oh, ow = g[f'{name}_y'].shape
        up, down = m['up'], m['down']
        px0, px1, py0, py1 = m['padding']
        rc, rows, row_bytes = sign_shape(lib, h, w, fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1)
        assert rc == 0
        ah, aw = flrelu_cpu.active_shape((1, 1, oh, ow), t['fd'], down)
        assert rows >= ah and 4 * row_bytes >= aw and row_bytes % 4 == 0, name
        assert 4 * row_bytes < aw + 16 + 4 * ((w - 1) * up + fu_w), name
        # the backward call (filtered_lrelu.py:253-264: fu <-> fd, up <-> down, dy -> dx) reads the same buffer: same shape
        pp = [fu_w - 1 + fd_w - 1 - px0, w * up - ow * down + px0 - (up - 1), fuy - 1 + fdy - 1 - py0, h * up - oh * down + py0 - (up - 1)]
        assert lib.la_filtered_lrelu_out_size(ow, down, up, pp[0], pp[1], fd_w, fu_w) == w
        assert sign_shape(lib, oh, ow, fd_h, fd_w, fu_h, fu_w, down, up, *pp) == (0, rows, row_bytes), name


def test_invalid_arguments_are_refused_on_the_host(lib):
    """Every case fails a host-side check before any launch (so it is safe without a device: nothing is enqueued)."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(x=p, fu=None, fd=None, N=1, Cc=1, H=4, W=4, fu_h=1, fu_w=1, fd_h=1, fd_w=1, up=1, down=1, pad=(0, 0, 0, 0)):
        return lib.la_filtered_lrelu_f32(x, fu, fd, None, None, None, p, N, Cc, H, W, fu_h, fu_w, fd_h, fd_w, up, down, *pad, 0, 0,
                                         math.sqrt(2), 0.2, math.inf, 0, 0, None)

    for kw, msg in ((dict(x=None), 'NULL'), (dict(up=0), 'at least 1'), (dict(down=0), 'at least 1'),
                    (dict(fu=p, fu_h=0, fu_w=0), 'fu is empty'), (dict(fd=p, fd_h=2, fd_w=0), 'fd is empty'),
                    (dict(fu=p, fu_h=65, fu_w=3), '64'), (dict(fd=p, fd_h=0, fd_w=70), '64'),
                    (dict(fd=p, fd_h=3, fd_w=3, pad=(-2, 0, 0, 0)), 'downsampling filter'),
                    (dict(fd=p, fd_h=3, fd_w=3, down=2, pad=(0, 0, -3, 0)), 'downsampling filter'),
                    (dict(pad=(-2, -2, 0, 0)), 'downsampling filter'),
                    (dict(N=0), 'empty')):
        assert call(**kw) == -1, kw      # LA_ERR_ARG
        assert msg in lib.la_last_error().decode(), (kw, lib.la_last_error())
    # an output under 1 x 1 (above, the up-sampled buffer check of filtered_lrelu.cpp:71 catches it first); the host query refuses it too
    rc, _, _ = sign_shape(lib, 1, 4, 0, 1, 0, 1, 1, 2, 0, 0, -1, 0)
    assert rc == -1 and 'at least 1x1' in lib.la_last_error().decode()
    assert lib.la_filtered_lrelu_act_f32(None, None, None, 1, 1, 4, 4, 0, 0, 1.0, 0.2, math.inf, 0, None) == -1
    assert lib.la_filtered_lrelu_act_f32(p, None, None, 1, 1, 4, 4, 0, 0, 1.0, 0.2, math.inf, 1, None) == -1      # no sign buffer
    assert 'so' in lib.la_last_error().decode()


def test_golden_shapes_follow_the_output_formula(g):
    names = [str(n) for n in g['cases']]
    assert len(names) >= 12
    paths = set()
    for name, m in cases(g):
        t = tensors(g, name)
        (fu_h, fu_w), (fd_h, fd_w) = taps(t['fu']), taps(t['fd'])
        n, c, h, w = t['x'].shape
        px0, px1, py0, py1 = m['padding']
        up, down = m['up'], m['down']
        oh = (h * up + py0 + py1 - ((fu_h or fu_w) - 1) - ((fd_h or fd_w) - 1) + down - 1) // down
        ow = (w * up + px0 + px1 - (fu_w - 1) - (fd_w - 1) + down - 1) // down
        for k in ('y', 'y32', 'g2', 'g232'):
            assert g[f'{name}_{k}'].shape == (n, c, oh, ow), (name, k)
        for k in ('dx', 'dx32'):
            assert g[f'{name}_{k}'].shape == (n, c, h, w), (name, k)
        assert g[f'{name}_y'].dtype == np.float64 and g[f'{name}_y32'].dtype == np.float32
        paths.add(m['path'])
    assert paths == {'fused', 'generic'}


def test_cpu_restatement_reproduces_goldens(g):
    for name, m in cases(g):
        t = tensors(g, name)
        kw = dict(up=m['up'], down=m['down'], padding=m['padding'], gain=m['gain'], slope=m['slope'], clamp=m['clamp'],
                  flip_filter=m['flip_filter'])
        x = t['x'].double().requires_grad_(True)
        b = None if t['b'] is None else t['b'].double().requires_grad_(True)
        dy = t['dy'].double().requires_grad_(True)
        y = flrelu_cpu.filtered_lrelu(x, t['fu'], t['fd'], b, **kw)
        grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
        (g2,) = torch.autograd.grad((grads[0] * t['v'].double()).sum(), [dy])
        # (the reference scales float32 taps by the up-FIR gain before casting them: exact for up = 1, 2, 4, a float32 rounding of
        #  the taps otherwise)
        tol = 1e-9 if m['up'] & (m['up'] - 1) == 0 else 1e-6
        for k, v in (('y', y), ('dx', grads[0]), ('g2', g2)) + ((('db', grads[1]),) if b is not None else ()):
            ref = g[f'{name}_{k}']
            np.testing.assert_allclose(v.detach().numpy(), ref, rtol=tol, atol=tol * max(1.0, np.abs(ref).max()), err_msg=f'{name} {k}')


def _restated(g, name, m, dtype):
    t = tensors(g, name)
    kw = dict(up=m['up'], down=m['down'], padding=m['padding'], gain=m['gain'], slope=m['slope'], clamp=m['clamp'], flip_filter=m['flip_filter'])
    x = t['x'].to(dtype).requires_grad_(True)
    b = None if t['b'] is None else t['b'].to(dtype).requires_grad_(True)
    dy = t['dy'].to(dtype).requires_grad_(True)
    y = flrelu_cpu.filtered_lrelu(x, t['fu'], t['fd'], b, **kw, dtype=dtype)
    assert y.dtype == dtype
    grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
    (g2,) = torch.autograd.grad((grads[0] * t['v'].to(dtype)).sum(), [dy])
    out = {'y': y, 'dx': grads[0], 'g2': g2}
    if b is not None:
        out['db'] = grads[1]
    return t, kw, {k: v.detach().double().numpy() for k, v in out.items()}


def test_cpu_restatement_reproduces_shape_goldens(gs):
    """flrelu_shapes.npz (the three forms and the multi-tile sizes filtered_lrelu.npz lacks, clamp 0, slope 1.5): same bound."""
    from test_hip_flrelu_shapes import taps_of, tile_plan
    names = [n for n, _ in cases(gs)]
    assert len(names) == 17
    multi = set()
    for name, m in cases(gs):
        _, _, got = _restated(gs, name, m, torch.float64)
        for k, v in got.items():
            ref = gs[f'{name}_{k}']
            np.testing.assert_allclose(v, ref, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(ref).max()), err_msg=f'{name} {k}')
        p = tile_plan(*gs[f'{name}_y'].shape[2:], m['up'], m['down'], taps_of(m['fu']), taps_of(m['fd']))
        assert p is not None and (p['tiles_y'], p['tiles_x']) == m['tiles'], name
        if min(m['tiles']) >= 2:
            multi.add((m['up'], m['down']))
    assert multi == {(u, d) for u in (1, 2, 4) for d in (1, 2, 4)}
    assert {m['clamp'] for _, m in cases(gs)} >= {0.0, None} and 1.5 in {m['slope'] for _, m in cases(gs)}


@pytest.mark.parametrize('which', ['g', 'gs'])
def test_float32_restatement_is_as_good_as_the_reference_in_float32(which, request):
    """The float32 mode of flrelu_cpu is the yardstick of the GPU sweep where no golden exists, so it is held to the reference here: its
    error against the float64 golden is at most 4 x the reference's own float32 error + 2e-6 x the largest magnitude (the rule the GPU
    tests apply to the kernel), kink cones excluded as there, and the reference's float32 error meets the same bound measured from the
    restatement's -- neither yardstick is looser than the other by more than that."""
    from test_hip_flrelu_shapes import masks
    g = request.getfixturevalue(which)
    for name, m in cases(g):
        t, kw, got = _restated(g, name, m, torch.float32)
        if kw['clamp'] == 0:
            for k, v in got.items():
                assert (v == 0).all() and (g[f'{name}_{k}'] == 0).all(), (name, k)
            continue
        ex = masks(t, kw)
        for k, v in got.items():
            ref64, ref32 = g[f'{name}_{k}'], g[f'{name}_{k}32'].astype(np.float64)
            keep = ~ex[k]
            scale = float(np.abs(ref64).max())
            mine, theirs = np.abs(v - ref64)[keep].max(initial=0.0), np.abs(ref32 - ref64)[keep].max(initial=0.0)
            assert mine <= 4 * theirs + 2e-6 * scale, (name, k, mine, theirs, scale)
            assert theirs <= 4 * mine + 2e-6 * scale, (name, k, mine, theirs, scale)


def test_sign_helpers_round_trip_and_layout(lib, g, gs):
    """pack_signs / unpack_signs: the layout of include/latentaug_hip.h (sample t of a row at bits 2 * (t % 4) of byte t // 4), a round
    trip at the rows / row_bytes la_filtered_lrelu_sign_shape gives for every golden case, and sign_bits over exactly the active extent."""
    one = torch.zeros([1, 1, 2, 9], dtype=torch.uint8)
    one[0, 0, 0, 0], one[0, 0, 0, 1], one[0, 0, 0, 6], one[0, 0, 1, 8] = 1, 2, 3, 2
    buf = flrelu_cpu.pack_signs(one, 3, 4)
    assert buf.shape == (1, 1, 3, 4) and buf.dtype == torch.uint8
    assert buf[0, 0].tolist() == [[0x01 | 0x02 << 2, 0x03 << 4, 0, 0], [0, 0, 0x02, 0], [0, 0, 0, 0]]
    gen = torch.Generator().manual_seed(4)
    for gg in (g, gs):
        for name, m in cases(gg):
            t = tensors(gg, name)
            (fu_h, fu_w), (fd_h, fd_w) = taps(t['fu']), taps(t['fd'])
            n, c, h, w = t['x'].shape
            rc, rows, row_bytes = sign_shape(lib, h, w, fu_h, fu_w, fd_h, fd_w, m['up'], m['down'], *m['padding'])
            assert rc == 0
            kw = dict(up=m['up'], down=m['down'], padding=m['padding'], gain=m['gain'], slope=m['slope'], clamp=m['clamp'], flip_filter=m['flip_filter'])
            bits = flrelu_cpu.sign_bits(t['x'], t['fu'], t['fd'], t['b'], **kw)
            ah, aw = flrelu_cpu.active_shape(gg[f'{name}_y'].shape, t['fd'], m['down'])
            assert bits.shape == (n, c, ah, aw) and bits.dtype == torch.uint8 and int(bits.max()) <= 3, name
            assert (m['clamp'] is None) == (int(bits.max()) <= 1), name
            buf = flrelu_cpu.pack_signs(bits, rows, row_bytes)
            assert buf.shape == (n, c, rows, row_bytes)
            assert torch.equal(flrelu_cpu.unpack_signs(buf, ah, aw), bits), name
            assert int(flrelu_cpu.unpack_signs(buf).sum()) == int(bits.sum()), name      # (nothing set past the active extent)
            rnd = torch.randint(0, 4, [n, c, rows, 4 * row_bytes], generator=gen, dtype=torch.uint8)
            assert torch.equal(flrelu_cpu.unpack_signs(flrelu_cpu.pack_signs(rnd, rows, row_bytes)), rnd), name
            # the stored derivative: reading the written bits back at offset 0 differentiates the activation
            mid = flrelu_cpu.up_stage(t['x'], t['fu'], t['b'], m['up'], m['padding'], m['flip_filter'])[:, :, :ah, :aw]
            d = flrelu_cpu.act_read(torch.ones_like(mid), bits, 0, 0, m['gain'], m['slope'])
            z = mid.clone().requires_grad_(True)
            (want,) = torch.autograd.grad(flrelu_cpu.act_stage(z, m['gain'], m['slope'], m['clamp']).sum(), [z])
            live = mid != 0      # (at an exact zero, padding only, the two conventions of lrelu'(0) differ and nothing depends on it)
            assert torch.allclose(d[live], want[live], rtol=1e-7, atol=0), name      # (one of three well separated values)
