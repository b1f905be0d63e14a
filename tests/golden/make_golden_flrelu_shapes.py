#!/usr/bin/env python3
"""Golden vectors of filtered_lrelu at the forms and tile seams filtered_lrelu.npz does not reach, by RUNNING THE REFERENCE here.

    python tests/golden/make_golden_flrelu_shapes.py     ->  tests/golden/flrelu_shapes.npz

Same recipe as make_golden_filtered_lrelu.py, whose helpers (the reference import, the jittered filters, the float64 / float32 run) are
used as they are: the reference's filtered_lrelu(..., impl='ref') with autograd, per case in float64 and in float32: y, dx, db and
g2 = d<dx, v>/d(dy).  Cases:
  u4d4 / u1d4 / u4d1, 1-D and 2-D filters   the three (up, down) forms filtered_lrelu.npz has no case of (one tile each)
  mt_u<up>d<down>                           one case per (up, down) pair at the smallest output for which the fused launch has at least
                                            2 x 2 tiles (tests/test_hip_flrelu_shapes.py: tile_plan, a host-side restatement that only
                                            picks sizes), with negative padding, flip_filter and 2-D filters among them
  clamp0, slope15                           clamp = 0 (every non-zero sample is clamped) and slope = 1.5
To keep the file small the inputs x, dy, v are multiples of 1/16 (exact in float32, so both runs still start from the same values; the bias is not) and the
multi-tile cases have one plane and, where the input would be several times the output, a wide padding."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import flrelu_cpu  # noqa: E402
import make_golden_filtered_lrelu as base  # noqa: E402
from test_hip_flrelu_shapes import size_for, tile_plan  # noqa: E402

# name: (N, C, OH, OW, up, down, fu spec, fd spec, [px0, py0] (the far sides: as much again or less, whatever gives the output size), flip,
#        slope, clamp, bias); OH = OW = None: the smallest square output with 2 x 2 tiles
# clamp: ('q', k) -> set where it trips on ~30 % * k of the samples, as in make_golden_filtered_lrelu.py; a float -> that value
CASES = {
    'u4d4_1d': (1, 2, 4, 5, 4, 4, ('1d', 24), ('1d', 24), [23, 22], False, 0.2, ('q', 1.0), True),
    'u4d4_2d': (1, 2, 5, 3, 4, 4, ('2d', 13, 16), ('2d', 9, 14), [10, 14], True, 0.2, None, True),
    'u1d4_1d': (1, 2, 5, 4, 1, 4, ('1d', 5), ('1d', 24), [12, 11], True, 0.2, ('q', 0.8), True),
    'u1d4_2d': (2, 1, 3, 5, 1, 4, None, ('2d', 11, 18), [8, -1], False, 0.2, None, True),
    'u4d1_1d': (1, 2, 14, 17, 4, 1, ('1d', 24), None, [17, 15], False, 0.2, ('q', 1.0), True),
    'u4d1_2d': (2, 1, 15, 13, 4, 1, ('2d', 20, 15), ('1d', 3), [9, 12], True, 0.0, None, True),
    'mt_u1d1': (1, 1, None, None, 1, 1, ('1d', 5), ('2d', 3, 4), [-1, 6], True, 0.2, ('q', 0.8), True),
    'mt_u2d1': (1, 1, None, None, 2, 1, ('1d', 12), None, [9, -2], False, 0.2, None, True),
    'mt_u4d1': (1, 1, None, None, 4, 1, ('2d', 16, 18), ('1d', 2), [12, 15], True, 0.2, ('q', 1.0), True),
    'mt_u1d2': (1, 1, None, None, 1, 2, None, ('1d', 12), [24, 22], False, 0.2, None, True),
    'mt_u2d2': (1, 1, None, None, 2, 2, ('1d', 12), ('1d', 12), [-3, 20], False, 0.2, ('q', 1.0), True),
    'mt_u4d2': (1, 1, None, None, 4, 2, ('1d', 24), ('2d', 10, 12), [16, -5], True, 0.2, None, True),
    'mt_u1d4': (1, 1, None, None, 1, 4, ('1d', 8), ('1d', 32), [28, 27], False, 0.2, ('q', 0.9), True),
    'mt_u2d4': (1, 1, None, None, 2, 4, ('1d', 16), ('1d', 32), [27, 30], True, 0.2, None, True),
    'mt_u4d4': (1, 1, None, None, 4, 4, ('1d', 24), ('1d', 24), [30, -3], False, 0.2, ('q', 1.0), True),
    'clamp0': (1, 2, 6, 7, 2, 2, ('1d', 12), ('1d', 12), [11, 10], False, 0.2, 0.0, True),
    'slope15': (1, 2, 7, 6, 2, 2, ('1d', 12), ('2d', 5, 6), [9, 11], True, 1.5, ('q', 0.8), True),
}


def taps(spec):
    return (1, 1, True) if spec is None else ((spec[1], spec[1], False) if spec[0] == '1d' else (spec[1], spec[2], True))


def smallest_multitile(up, down, fut, fdt):
    for o in range(2, 200):
        p = tile_plan(o, o, up, down, fut, fdt)
        if p is not None and p['tiles_x'] >= 2 and p['tiles_y'] >= 2:
            return o
    raise AssertionError


def coarse(shape):
    return torch.round(torch.randn(shape) * 16) / 16


def main():
    torch.manual_seed(11)
    out, names = {}, []
    for name, (n, c, oh, ow, up, down, fus, fds, (px0, py0), flip, slope, clampk, has_b) in CASES.items():
        fu, fd = base.filt(fus), base.filt(fds)
        fut, fdt = taps(fus), taps(fds)
        if oh is None:
            oh = ow = smallest_multitile(up, down, fut, fdt)
        w, px1 = size_for(ow, up, down, px0, max(abs(px0), abs(py0)), fut[1], fdt[1])
        h, py1 = size_for(oh, up, down, py0, max(abs(px0), abs(py0)), fut[0], fdt[0])
        pad = [px0, px1, py0, py1]
        plan = tile_plan(oh, ow, up, down, fut, fdt)
        assert plan is not None and (not name.startswith('mt_') or (plan['tiles_x'] >= 2 and plan['tiles_y'] >= 2)), (name, plan)
        x = coarse([n, c, h, w])
        b = 0.3 * torch.randn([c]) if has_b else None      # (not coarse: x + b must not land on an exact 0, a tie of lrelu')
        kw = dict(up=up, down=down, padding=pad, gain=float(np.sqrt(2)), slope=slope, clamp=None, flip_filter=flip)
        if isinstance(clampk, tuple):      # (a quantile of |lrelu| of the unclamped intermediate)
            a = flrelu_cpu.act_stage(flrelu_cpu.up_stage(x, fu, b, up, pad, flip), kw['gain'], slope)
            v = np.sort(a.abs().numpy().ravel())
            v = v[v > 0]      # (the zeros of a wide padding are not part of the share)
            i = int((1 - 0.3 * clampk[1]) * v.size)
            kw['clamp'] = float(np.float32((v[i] + v[i + 1]) / 2))
        elif clampk is not None:
            kw['clamp'] = float(clampk)
        y0 = base.ref.filtered_lrelu(x.double(), fu, fd, None if b is None else b.double(), impl='ref', **kw)
        assert tuple(y0.shape) == (n, c, oh, ow), (name, y0.shape)
        dy = coarse(y0.shape)
        v = coarse(x.shape)
        r64 = base.run(x, b, fu, fd, dy, v, kw, torch.float64)
        r32 = base.run(x, b, fu, fd, dy, v, kw, torch.float32)
        names.append(name)
        meta = dict(kw, fu=fus, fd=fds, noncontig=False, path='fused', tiles=(plan['tiles_y'], plan['tiles_x']))
        out[f'{name}_meta'] = np.array(repr(meta))
        out[f'{name}_x'] = x.numpy()
        out[f'{name}_dy'] = dy.numpy()
        out[f'{name}_v'] = v.numpy()
        if b is not None:
            out[f'{name}_b'] = b.numpy()
        if fu is not None:
            out[f'{name}_fu'] = fu.numpy()
        if fd is not None:
            out[f'{name}_fd'] = fd.numpy()
        for k in r64:
            out[f'{name}_{k}'] = r64[k].numpy()
            out[f'{name}_{k}32'] = r32[k].numpy()
        print(name, tuple(x.shape), '->', tuple(y0.shape), 'pad', pad, 'clamp', kw['clamp'], 'tiles', meta['tiles'], plan['rung'])
    out['cases'] = np.array(names)
    path = os.path.join(HERE, 'flrelu_shapes.npz')
    np.savez_compressed(path, **out)
    print(len(names), 'cases,', os.path.getsize(path), 'bytes (filtered_lrelu.npz:', os.path.getsize(os.path.join(HERE, 'filtered_lrelu.npz')), ')')


if __name__ == '__main__':
    main()
