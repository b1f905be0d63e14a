#!/usr/bin/env python3
"""Golden vectors of bias_act and upfirdn2d in float64 AND float16, by RUNNING THE REFERENCE here.

    python tests/golden/make_golden_op_dtypes.py       ->  tests/golden/op_dtypes.npz

Executed from the reference (imported, never copied): models/stylegan3/torch_utils/ops/bias_act.py `bias_act(..., impl='ref')` and
upfirdn2d.py `setup_filter` / `upfirdn2d` / `upsample2d` / `downsample2d` / `filter2d` with impl='ref', plus autograd, on the CPU.
Every input is a float16 value: the same numbers run once in float64 (the expected values) and once in float16 (the reference's own
float16 result, whose error against float64 sets the budget of a float16 kernel's gradients).

  b<k>  bias_act: all nine activations x (default parameters, gain 0.7 / clamp 1.1 / alpha 0.3): x, b, dy, ddx (float16);
        y, dx, d2, db (float64) and y16, dx16, d216, db16 (the reference run in float16)
  u<k>  upfirdn2d family: x, dy (float16), the raw taps and setup_filter's float32 taps; y, dx (float64) and y16, dx16.
        The gains are powers of two: the reference's impl='ref' path rounds taps * gain to float32 (upfirdn2d.py:194), which is then
        exact, so the float64 expected values carry no rounding of their own."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/models/stylegan3')
from torch_utils.ops import bias_act as ref_ba      # noqa: E402
from torch_utils.ops import upfirdn2d as ref_fir    # noqa: E402

torch.manual_seed(23)
out, cases = {}, []


def h(t):
    """float16-exact values (returned as float64)."""
    return t.half().double()


# ---------------------------------------------------------------- bias_act
k = 0
for act in ref_ba.activation_funcs:
    for gain, clamp, alpha in ((None, None, None), (0.7, 1.1, 0.3)):
        x, b = h(torch.randn([2, 6, 5, 8]) * 2.0), h(torch.randn([6]) * 0.5)
        dy, ddx = h(torch.randn(x.shape)), h(torch.randn(x.shape))
        res = {}
        for dt, sfx in ((torch.float64, ''), (torch.float16, '16')):
            xr = x.to(dt, copy=True).requires_grad_(True)
            br = b.to(dt, copy=True).requires_grad_(True)
            y = ref_ba.bias_act(xr, br, dim=1, act=act, alpha=alpha, gain=gain, clamp=clamp, impl='ref')
            dx, db = torch.autograd.grad(y, [xr, br], dy.to(dt), create_graph=True)
            d2 = torch.zeros_like(xr)
            if dx.requires_grad:
                (g2,) = torch.autograd.grad(dx, [xr], ddx.to(dt), allow_unused=True)
                d2 = d2 if g2 is None else g2
            for key, t in (('y', y), ('dx', dx), ('d2', d2), ('db', db)):
                res[key + sfx] = t.detach().numpy().astype(np.float64 if dt == torch.float64 else np.float16)
        name = f'b{k}'
        cases.append((name, 'bias_act', act, repr(dict(gain=gain, clamp=clamp, alpha=alpha))))
        for key, t in (('x', x), ('b', b), ('dy', dy), ('ddx', ddx)):
            out[f'{name}_{key}'] = t.numpy().astype(np.float16)
        for key, v in res.items():
            out[f'{name}_{key}'] = v
        k += 1

# ---------------------------------------------------------------- upfirdn2d
taps3 = [[1.0, 2.0, 1.0], [3.0, 5.0, 2.0], [0.5, 1.0, 4.0]]                    # asymmetric 3x3
taps8 = (np.outer([1, 3, 4, 6, 5, 3, 2, 1], [2, 1, 4, 5, 6, 3, 1, 1]) + np.arange(64).reshape(8, 8) % 3).tolist()   # not rank one
taps12 = list(np.hanning(14)[1:-1])                                           # 12 taps: separable (setup_filter keeps it 1-D)
k = 0
for op, taps, kw, shape in (
        ('upsample2d', [1, 3, 3, 1], dict(), [2, 3, 12, 16]),
        ('downsample2d', [1, 3, 3, 1], dict(), [2, 3, 12, 16]),
        ('filter2d', [1, 3, 3, 1], dict(), [2, 3, 12, 16]),
        ('upfirdn2d', taps3, dict(up=2, down=1, padding=[1, 2, 0, 3], flip_filter=True, gain=2.0), [2, 3, 9, 11]),
        ('upfirdn2d', taps8, dict(up=1, down=2, padding=[3, 4, 2, 5], flip_filter=True, gain=0.5), [2, 3, 13, 16]),
        ('upfirdn2d', taps8, dict(up=2, down=1, padding=[4, 3, 5, 2], gain=4.0), [1, 2, 7, 9]),
        ('upsample2d', taps12, dict(), [1, 3, 10, 12]),
):
    f = ref_fir.setup_filter(taps)
    x = h(torch.randn(shape))
    y64 = getattr(ref_fir, op)(x, f, impl='ref', **kw)
    dy = h(torch.randn(y64.shape))
    res = {}
    for dt, sfx in ((torch.float64, ''), (torch.float16, '16')):
        xr = x.to(dt, copy=True).requires_grad_(True)
        y = getattr(ref_fir, op)(xr, f, impl='ref', **kw)
        (dx,) = torch.autograd.grad(y, [xr], dy.to(dt))
        for key, t in (('y', y), ('dx', dx)):
            res[key + sfx] = t.detach().numpy().astype(np.float64 if dt == torch.float64 else np.float16)
    name = f'u{k}'
    cases.append((name, op, repr(np.asarray(taps, dtype=np.float64).tolist()), repr(kw)))
    out[f'{name}_f'] = f.numpy()
    out[f'{name}_x'] = x.numpy().astype(np.float16)
    out[f'{name}_dy'] = dy.numpy().astype(np.float16)
    for key, v in res.items():
        out[f'{name}_{key}'] = v
    k += 1

out['cases'] = np.array([repr(c) for c in cases])
path = os.path.join(HERE, 'op_dtypes.npz')
np.savez_compressed(path, **out)
print(len(cases), 'cases ->', path, os.path.getsize(path), 'bytes')
