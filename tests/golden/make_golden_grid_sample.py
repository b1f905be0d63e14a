#!/usr/bin/env python3
"""Golden vectors of grid_sample and fma, by RUNNING THE REFERENCE here on the CPU.

    python tests/golden/make_golden_grid_sample.py <reference root>     ->  tests/golden/grid_sample.npz

Executed from the reference (imported, never copied): models/stylegan3/torch_utils/ops/grid_sample_gradfix.py `grid_sample` on its
default path (`enabled = False`: torch.nn.functional.grid_sample with mode='bilinear', padding_mode='zeros', align_corners=False; the
custom path does not run on torch 2.10) and fma.py `fma`, plus autograd.  The inputs come from the case table of
tests/grid_sample_cases.py (seeds there; float32-exact values, float16-exact for the `h_` cases; grids redrawn until no position lies
within 1e-3 px of an integer, where dgrid jumps).

  g_<case>   x, grid, dy, ddx (stored in the float type that holds them exactly); y, dx, dgrid for the incoming gradient dy (float64);
             y32, dx32, dgrid32 = the reference's own float32 run, and for the float16-exact cases y16, dx16, dgrid16 = its float16
             run: their errors against float64 are the budgets of the float32 / float16 kernels.
             d2 = the second-order expectation, recorded as the reference's forward applied to ddx: the op is linear in `input`, so
             d(dx)/d(dy) contracted with ddx IS grid_sample(ddx, grid); torch cannot form it by autograd (no derivative of
             aten::grid_sampler_2d_backward), which is the gap the HIP op closes.
  f_<case>   a, b, c, dy; y, da, db, dc (float64; dc of the 0-d c, which the reference's _unbroadcast refuses, is sum(dy)); for the second-order case also dda (an incoming gradient of da) and
             d2_dy, d2_b = the gradients of <da, dda> with respect to dy and b.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], 'models', 'stylegan3'))
import grid_sample_cases as gc                              # noqa: E402
from torch_utils.ops import fma as ref_fma                  # noqa: E402
from torch_utils.ops import grid_sample_gradfix as ref_gs   # noqa: E402

assert ref_gs.enabled is False
out = {}
NP = {torch.float64: np.float64, torch.float32: np.float32, torch.float16: np.float16}

for case in gc.GS_CASES:
    name, half = case[0], case[-1]
    t = gc.gs_inputs(case)
    for k, v in t.items():
        out[f'g_{name}_{k}'] = v.astype(np.float16 if half else np.float32)      # (exact: the values were drawn that way)
    for dt, sfx in ((torch.float64, ''), (torch.float32, '32')) + (((torch.float16, '16'),) if half else ()):
        x = torch.tensor(t['x'], dtype=dt, requires_grad=True)
        grid = torch.tensor(t['grid'], dtype=dt, requires_grad=True)
        y = ref_gs.grid_sample(x, grid)
        dx, dgrid = torch.autograd.grad(y, [x, grid], torch.tensor(t['dy'], dtype=dt))
        for k, v in (('y', y), ('dx', dx), ('dgrid', dgrid)):
            out[f'g_{name}_{k}{sfx}'] = v.detach().numpy().astype(NP[dt])
    out[f'g_{name}_d2'] = ref_gs.grid_sample(torch.tensor(t['ddx']), torch.tensor(t['grid'])).numpy()

for case in gc.FMA_CASES:
    name = case[0]
    t = gc.fma_inputs(case)
    for k, v in t.items():
        out[f'f_{name}_{k}'] = v.astype(np.float32)
    a, b, c = (torch.tensor(t[k], requires_grad=t[k].ndim > 0) for k in 'abc')
    dy = torch.tensor(t['dy'], requires_grad=True)
    y = ref_fma.fma(a, b, c)
    if c.ndim:
        da, db, dc = torch.autograd.grad(y, [a, b, c], dy, create_graph=True)
    else:      # (the reference's _unbroadcast asserts on a 0-d operand, fma.py:55-57: dc of the scalar c is written out as what it is)
        (da, db), dc = torch.autograd.grad(y, [a, b], dy, create_graph=True), dy.sum()
    for k, v in (('y', y), ('da', da), ('db', db), ('dc', dc)):
        out[f'f_{name}_{k}'] = v.detach().numpy()
    if name == gc.FMA_SECOND_ORDER:
        dda = torch.tensor(np.random.default_rng(case[-1] + 100).standard_normal(da.shape).astype(np.float32).astype(np.float64))
        d2_dy, d2_b = torch.autograd.grad(da, [dy, b], dda)
        out[f'f_{name}_dda'], out[f'f_{name}_d2_dy'], out[f'f_{name}_d2_b'] = dda.numpy(), d2_dy.numpy(), d2_b.numpy()

path = os.path.join(HERE, 'grid_sample.npz')
np.savez_compressed(path, **out)
print(len(gc.GS_CASES), '+', len(gc.FMA_CASES), 'cases ->', path, os.path.getsize(path), 'bytes')
