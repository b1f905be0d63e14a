#!/usr/bin/env python3
"""Golden vectors of upfirdn2d with UNEQUAL x / y factors, NON-SQUARE dense filters and unequal (also negative) pads, and of bias_act
along every axis, by RUNNING THE REFERENCE here in float64.

    python tests/golden/make_golden_op_shapes.py     ->  tests/golden/op_shapes.npz

Executed from the reference (imported, never copied): models/stylegan3/torch_utils/ops/upfirdn2d.py -- setup_filter (:70-114) and
upfirdn2d with impl='ref' (:118-211) -- and bias_act.py -- bias_act with impl='ref' (:52-120); forward and the gradients with respect to
the input (and the bias) by autograd through the reference implementation.  Every array is float64 except the taps, which are the
float32 tensor setup_filter returns."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/models/stylegan3')
from torch_utils.ops import bias_act as ref_ba      # noqa: E402
from torch_utils.ops import upfirdn2d as ref        # noqa: E402

torch.manual_seed(23)


def dense(fh, fw):
    """A dense fh x fw filter without any symmetry (so a transposed, flipped or shifted tap shows)."""
    return (torch.arange(fh * fw, dtype=torch.float32).reshape(fh, fw) % 5 + 1 + torch.arange(fw, dtype=torch.float32) * 0.25).tolist()


# (name of the taps, taps, input shape, arguments of upfirdn2d)
U = [
    ('1331', [1, 3, 3, 1], [2, 3, 11, 14], dict(up=(2, 1), padding=[2, 1, 1, 2])),
    ('d3x5', dense(3, 5), [1, 4, 9, 13], dict(up=(1, 3), padding=[2, 2, 2, 1])),
    ('d1x4', dense(1, 4), [2, 2, 12, 24], dict(down=(1, 2), padding=[1, 2, 0, 1])),
    ('d4x1', dense(4, 1), [2, 2, 23, 17], dict(down=(3, 2), padding=[0, 1, 2, 1], flip_filter=True)),
    ('d2x7', dense(2, 7), [1, 3, 10, 15], dict(up=(2, 3), down=(3, 2), padding=[3, 4, 1, 2], gain=1.7)),
    ('1331', [1, 3, 3, 1], [1, 3, 13, 16], dict(padding=[3, -1, 2, 4], gain=0.6)),
    ('d3x5', dense(3, 5), [2, 2, 14, 19], dict(padding=[-2, 5, -1, 3], flip_filter=True)),
    ('1331', [1, 3, 3, 1], [2, 2, 9, 12], dict(up=(2, 3), down=(3, 2), padding=[2, 3, 4, 1], flip_filter=True, gain=2.3)),
    ('d2x7', dense(2, 7), [1, 2, 24, 24], dict(down=(3, 2), padding=[4, -2, 0, 1], flip_filter=False, gain=0.37)),
]
# (shape of x, bias axis, activation, keyword arguments)
B = [
    ([4, 6, 5, 8], 0, 'lrelu', dict(clamp=0.75)),
    ([4, 6, 5, 8], 2, 'swish', dict()),
    ([4, 6, 5, 8], 3, 'linear', dict(gain=1.3)),
    ([7, 9], 1, 'lrelu', dict(alpha=0.1, gain=0.9, clamp=0.75)),
    ([4, 6, 5, 8], 3, 'swish', dict(clamp=0.75)),
]

out, cases = {}, []
for k, (tname, taps, shape, kw) in enumerate(U):
    f = ref.setup_filter(taps)
    assert f.ndim == 2 and f.dtype == torch.float32
    x = torch.randn(shape).double().requires_grad_(True)
    y = ref.upfirdn2d(x, f, impl='ref', **kw)
    dy = torch.randn(y.shape).double()
    (dx,) = torch.autograd.grad(y, [x], dy)
    name = f'u{k}'
    cases.append((name, tname, 'upfirdn2d', repr(kw)))
    out[f'{name}_f'] = f.numpy()
    for key, t in (('x', x.detach()), ('dy', dy), ('y', y.detach()), ('dx', dx)):
        out[f'{name}_{key}'] = t.numpy()
for k, (shape, dim, act, kw) in enumerate(B):
    x = torch.randn(shape).double().requires_grad_(True)
    b = torch.randn([shape[dim]]).double().requires_grad_(True)
    y = ref_ba.bias_act(x, b, dim=dim, act=act, impl='ref', **kw)
    dy = torch.randn(y.shape).double()
    dx, db = torch.autograd.grad(y, [x, b], dy)
    name = f'b{k}'
    cases.append((name, act, dim, repr(kw)))
    for key, t in (('x', x.detach()), ('b', b.detach()), ('dy', dy), ('y', y.detach()), ('dx', dx), ('db', db)):
        out[f'{name}_{key}'] = t.numpy()
out['cases'] = np.array([repr(c) for c in cases])
np.savez_compressed(os.path.join(HERE, 'op_shapes.npz'), **out)
print(len(cases), 'cases')
