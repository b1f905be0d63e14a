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
