"""The float64 oracle (oracle/sg2_ops.py) against the reference at the argument shapes the op sweep of test_hip_op_shapes.py leans on:
unequal x / y factors, non-square dense filters, four unequal pads (one or two negative), flip_filter both ways, non-power-of-two gains;
bias_act along axis 0, 2 and 3 of a 4-D tensor and axis 1 of a 2-D one.  tests/golden/op_shapes.npz was written by the reference's
impl='ref' path in float64 (make_golden_op_shapes.py); the oracle reproduces every array to 1e-12 x max(1, max |expected|)."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import sg2_ops as O


def _load(golden_dir):
    g = np.load(os.path.join(golden_dir, 'op_shapes.npz'))
    return g, [ast.literal_eval(str(r)) for r in g['cases']]


def _close(got, exp, what):
    assert got.dtype == torch.float64 and tuple(got.shape) == exp.shape, what
    err = float(np.abs(got.detach().numpy() - exp).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(exp).max())), (what, err)


def test_fixture_holds_the_argument_shapes(golden_dir):
    """The fixture is what the issue asks for, not merely something the oracle agrees with."""
    g, cases = _load(golden_dir)
    ups, downs, fshapes, pads, flips, dims = set(), set(), set(), [], set(), set()
    for name, _, third, kwrep in cases:
        kw = ast.literal_eval(kwrep)
        if name.startswith('u'):
            ups.add(kw.get('up', 1)); downs.add(kw.get('down', 1)); fshapes.add(g[f'{name}_f'].shape); pads.append(kw['padding'])
            flips.add(bool(kw.get('flip_filter', False)))
            assert max(g[f'{name}_x'].shape[2:]) <= 24
        else:
            dims.add((g[f'{name}_x'].ndim, third))
    assert {(2, 1), (1, 3), (2, 3)} <= ups and {(1, 2), (3, 2)} <= downs
    assert {(3, 5), (1, 4), (4, 1), (2, 7)} <= fshapes and flips == {False, True}
    assert any(sum(v < 0 for v in p) == 1 for p in pads) and any(sum(v < 0 for v in p) == 2 for p in pads)
    assert {(4, 0), (4, 2), (4, 3), (2, 1)} <= dims


def test_oracle_upfirdn2d_unequal_factors_and_filters(golden_dir):
    g, cases = _load(golden_dir)
    n = 0
    for name, _, op, kwrep in cases:
        if not name.startswith('u'):
            continue
        x = torch.tensor(g[f'{name}_x'], requires_grad=True)
        y = getattr(O, op)(x, torch.tensor(g[f'{name}_f']), **ast.literal_eval(kwrep))
        (dx,) = torch.autograd.grad(y, [x], torch.tensor(g[f'{name}_dy']))
        _close(y, g[f'{name}_y'], (name, 'y'))
        _close(dx, g[f'{name}_dx'], (name, 'dx'))
        n += 1
    assert n >= 8


def test_oracle_bias_act_every_axis(golden_dir):
    g, cases = _load(golden_dir)
    n = 0
    for name, act, dim, kwrep in cases:
        if not name.startswith('b'):
            continue
        x = torch.tensor(g[f'{name}_x'], requires_grad=True)
        b = torch.tensor(g[f'{name}_b'], requires_grad=True)
        y = O.bias_act(x, b, dim=dim, act=act, **ast.literal_eval(kwrep))
        dx, db = torch.autograd.grad(y, [x, b], torch.tensor(g[f'{name}_dy']))
        for k, got in (('y', y), ('dx', dx), ('db', db)):
            _close(got, g[f'{name}_{k}'], (name, act, dim, k))
        n += 1
    assert n >= 4


@pytest.mark.parametrize('shape', [(3, 5), (1, 4), (4, 1), (2, 7)])
def test_oracle_setup_filter_keeps_dense_shapes(shape):
    """setup_filter of a 2-D array: kept as it is, normalised (upfirdn2d.py:100-112)."""
    f = O.setup_filter(torch.arange(1, shape[0] * shape[1] + 1, dtype=torch.float32).reshape(shape).tolist())
    assert tuple(f.shape) == shape and abs(float(f.sum()) - 1) < 1e-6
