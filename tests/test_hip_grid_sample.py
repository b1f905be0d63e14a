"""ops.grid_sample and ops.fma on the GPU (la_grid_sample.hip) against the reference's golden (tests/golden/grid_sample.npz) and the
float64 restatement of tests/grid_sample_cases.py (pinned to that golden by tests/test_grid_sample_cpu.py).

Budgets
  exact inputs   integers and quarter-pixel positions on a 4 x 8 image: every product and sum is an exact dyadic, so y, dx, dgrid and
                 the second-order result equal the restatement bit for bit, whatever the order of the atomic adds, in every dtype.
  float64        1e-12 x max(1, max |expected|).
  float32        F32_MARGIN x the reference's own float32 error on the case + 1 float32 ulp of the largest magnitude.  The margin pays
                 for a different summation order.  It started at 4; the first GPU run measured kernel error / reference error per
                 case and quantity (the test prints them): 1.00 for every y, 0.64 - 1.24 for dx, 0.67 - 2.25 for dgrid (largest:
                 h_band_c5, 1.94e-6 against the reference's 8.63e-7).  Margin = 2 x the largest ratio = 4.5 (DESIGN 'grid_sample').
  float16        forward within 1 fp16 ulp of the float64 value + 1e-7 x the largest magnitude; gradients within 2 x the reference's
                 own float16 error + 1 fp16 ulp of the largest magnitude (the conventions of tests/test_hip_op_dtypes.py).
  fma            forward within 1 float32 ulp of the float64 value; un-broadcast sums within the error of the restatement run in float32
                 on the CPU + 1 float32 ulp of the largest magnitude; integer inputs bit for bit.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

F32_MARGIN = 4.5
F16_EPS32 = 1e-7
TORCH = {'f16': torch.float16, 'f32': torch.float32, 'f64': torch.float64}
H_CASES = [c for c in gc.GS_CASES if c[-1]]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'grid_sample.npz'))


def np64(t):
    return t.detach().double().cpu().numpy()


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def ulp16(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float16)).astype(np.float64)


def atomic_sum_tol(dy, x, grid, dtype):
    """How far two correctly rounded evaluations of dx may lie apart, whatever their order: a float32 sum of K terms differs from the
    exact one by at most (K + 2) x 2^-24 x the sum of the terms' magnitudes (K - 1 additions and the two products of each term);
    K is at most the outputs of one image, and the sum of magnitudes per pixel is dx of |dy|.  Twice that between two sums; float16
    adds the final rounding, 1 fp16 ulp of the largest magnitude."""
    mag, _ = gc.gs_backward(np.abs(dy), x, grid)
    if dtype == 'f64':
        return 1e-12 * max(1.0, float(mag.max()))
    tol = 2 * (grid.shape[1] * grid.shape[2] + 2) * 2.0 ** -24 * float(mag.max())
    return tol + (float(ulp16(mag.max())) if dtype == 'f16' else 0.0)


def run_first(ops, dev, dt, x, grid, dy, need=(True, True)):
    """y and (dx, dgrid) of ops.grid_sample for the incoming gradient dy; `need` says which of input / grid require grad."""
    xt = torch.tensor(x, device=dev, dtype=dt, requires_grad=need[0])
    gt = torch.tensor(grid, device=dev, dtype=dt, requires_grad=need[1])
    y = ops.grid_sample(xt, gt)
    grads = torch.autograd.grad(y, [t for t, n in ((xt, need[0]), (gt, need[1])) if n], torch.tensor(dy, device=dev, dtype=dt))
    grads = list(grads)
    return y, (grads.pop(0) if need[0] else None), (grads.pop(0) if need[1] else None)


def run_second(ops, dev, dt, x, grid, dy, ddx):
    """d/d(dy) of <dx, ddx>: the second-order result, with the grid a constant."""
    xt = torch.tensor(x, device=dev, dtype=dt, requires_grad=True)
    dyt = torch.tensor(dy, device=dev, dtype=dt, requires_grad=True)
    y = ops.grid_sample(xt, torch.tensor(grid, device=dev, dtype=dt))
    (dx,) = torch.autograd.grad(y, [xt], dyt, create_graph=True)
    (d2,) = torch.autograd.grad(dx, [dyt], torch.tensor(ddx, device=dev, dtype=dt))
    return d2


# ---------------------------------------------------------------------------------------------------------------- exact inputs
def _exact_inputs(amp):
    """4 x 8 image, N = 2, C = 3; every quarter-pixel position of [-1.5, size + 0.5] on both axes (25 x 41 outputs: several blocks per
    image), sample 1 walking them in the opposite order; x, dy, ddx integers in [-amp, amp]."""
    H, W, N, C = 4, 8, 2, 3
    px = np.arange(-6, 4 * W + 3) / 4.0
    py = np.arange(-6, 4 * H + 3) / 4.0
    gx, gy = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
    g0 = np.stack(np.broadcast_arrays(gx[None, :], gy[:, None]), axis=-1)
    grid = np.stack([g0, g0[::-1, ::-1]])
    assert np.array_equal(grid.astype(np.float16).astype(np.float64), grid)      # exact in float16, hence in float32
    qx, qy = gc.positions(grid, H, W)
    assert np.array_equal(qx[0], np.broadcast_to(px[None, :], qx[0].shape)) and np.array_equal(qy[0], np.broadcast_to(py[:, None], qy[0].shape))
    rng = np.random.default_rng(40 + amp)
    x, ddx = (rng.integers(-amp, amp + 1, (N, C, H, W)).astype(np.float64) for _ in range(2))
    dy = rng.integers(-amp, amp + 1, (N, C) + grid.shape[1:3]).astype(np.float64)
    return x, grid, dy, ddx


@pytest.mark.parametrize('dtype,amp', [('f32', 4), ('f64', 4), ('f16', 2)])
def test_exact_inputs_bit_for_bit(dev, dtype, amp):
    from latentaugment_amd import ops
    dt = TORCH[dtype]
    x, grid, dy, ddx = _exact_inputs(amp)
    exp = {'y': gc.gs_forward(x, grid), 'd2': gc.gs_forward(ddx, grid)}
    exp['dx'], exp['dgrid'] = gc.gs_backward(dy, x, grid)
    npdt = {'f16': np.float16, 'f32': np.float32, 'f64': np.float64}[dtype]
    for k, e in exp.items():      # the expectation itself is exact in the dtype under test
        assert np.array_equal(e.astype(npdt).astype(np.float64), e), (dtype, k)
        assert np.abs(e).max() > 1
    runs = []
    for _ in range(2):
        y, dx, dgrid = run_first(ops, dev, dt, x, grid, dy)
        runs.append({'y': y, 'dx': dx, 'dgrid': dgrid, 'd2': run_second(ops, dev, dt, x, grid, dy, ddx)})
    for k, e in exp.items():
        assert runs[0][k].dtype == dt
        assert np.array_equal(np64(runs[0][k]), e), (dtype, k, float(np.abs(np64(runs[0][k]) - e).max()))
        assert torch.equal(runs[0][k], runs[1][k]), (dtype, k)


# ---------------------------------------------------------------------------------------------------------------- float inputs
def _golden_case(gold, name):
    return {k: gold[f'g_{name}_{k}'].astype(np.float64) for k in ('x', 'grid', 'dy', 'ddx')}


@pytest.mark.parametrize('case', gc.GS_CASES, ids=gc.GS_NAMES)
def test_float64_vs_reference(dev, gold, case):
    from latentaugment_amd import ops
    name = case[0]
    t = _golden_case(gold, name)
    y, dx, dgrid = run_first(ops, dev, torch.float64, t['x'], t['grid'], t['dy'])
    d2 = run_second(ops, dev, torch.float64, t['x'], t['grid'], t['dy'], t['ddx'])
    for k, got in (('y', y), ('dx', dx), ('dgrid', dgrid), ('d2', d2)):
        e = gold[f'g_{name}_{k}']
        assert got.dtype == torch.float64 and tuple(got.shape) == e.shape
        err = float(np.abs(np64(got) - e).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(e).max())), (name, k, err)


@pytest.mark.parametrize('case', gc.GS_CASES, ids=gc.GS_NAMES)
def test_float32_vs_reference(dev, gold, case):
    from latentaugment_amd import ops
    name = case[0]
    t = _golden_case(gold, name)
    y, dx, dgrid = run_first(ops, dev, torch.float32, t['x'], t['grid'], t['dy'])
    d2 = run_second(ops, dev, torch.float32, t['x'], t['grid'], t['dy'], t['ddx'])
    for k, got in (('y', y), ('dx', dx), ('dgrid', dgrid)):
        e = gold[f'g_{name}_{k}']
        assert got.dtype == torch.float32 and tuple(got.shape) == e.shape
        ref_err = float(np.abs(gold[f'g_{name}_{k}32'].astype(np.float64) - e).max())
        err = float(np.abs(np64(got) - e).max())
        print(f'float32 {name} {k}: kernel error {err:.3e}, reference error {ref_err:.3e}, ratio {err / ref_err if ref_err else float("nan"):.2f}')
        assert err <= F32_MARGIN * ref_err + ulp32(np.abs(e).max()), (name, k, err, ref_err)
    # the second-order result is the forward on ddx: budgeted like y, with the float32 restatement on the CPU as the yardstick
    e = gold[f'g_{name}_d2']
    ref_err = float(np.abs(gc.gs_forward(t['ddx'], t['grid'], np.float32).astype(np.float64) - e).max())
    err = float(np.abs(np64(d2) - e).max())
    assert err <= F32_MARGIN * ref_err + ulp32(np.abs(e).max()), (name, 'd2', err, ref_err)


@pytest.mark.parametrize('case', H_CASES, ids=[c[0] for c in H_CASES])
def test_float16_vs_reference(dev, gold, case):
    from latentaugment_amd import ops
    name = case[0]
    t = _golden_case(gold, name)
    y, dx, dgrid = run_first(ops, dev, torch.float16, t['x'], t['grid'], t['dy'])
    d2 = run_second(ops, dev, torch.float16, t['x'], t['grid'], t['dy'], t['ddx'])
    for got in (y, dx, dgrid, d2):
        assert got.dtype == torch.float16
    for k, got in (('y', y), ('d2', d2)):      # forward values: 1 ulp of the float64 value, element by element
        e = gold[f'g_{name}_{k}']
        err = np.abs(np64(got) - e)
        assert (err <= ulp16(e) + F16_EPS32 * np.abs(e).max()).all(), (name, k, float(err.max()))
    for k, got in (('dx', dx), ('dgrid', dgrid)):
        e, e16 = gold[f'g_{name}_{k}'], gold[f'g_{name}_{k}16'].astype(np.float64)
        ref_err = float(np.abs(e16 - e).max())
        err = float(np.abs(np64(got) - e).max())
        print(f'float16 {name} {k}: kernel error {err:.3e}, reference error {ref_err:.3e}')
        assert err <= 2 * ref_err + float(ulp16(np.abs(e).max())), (name, k, err, ref_err)


# ---------------------------------------------------------------------------------------------------------------- autograd surface
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_output_mask(dev, gold, dtype):
    """Only input, or only grid, requiring grad: the other gradient is None (never computed: needs_input_grad reaches the launch as its
    NULL pointer) and the one returned is the both-on run's -- dgrid bit for bit, dx to the atomic sum's last bits."""
    from latentaugment_amd import ops
    dt = TORCH[dtype]
    t = _golden_case(gold, 'h_blocks_c3')
    _, dx, dgrid = run_first(ops, dev, dt, t['x'], t['grid'], t['dy'])
    _, dx_only, none_g = run_first(ops, dev, dt, t['x'], t['grid'], t['dy'], need=(True, False))
    _, none_x, dgrid_only = run_first(ops, dev, dt, t['x'], t['grid'], t['dy'], need=(False, True))
    assert none_g is None and none_x is None
    assert torch.equal(dgrid_only, dgrid)
    assert float((dx_only.double() - dx.double()).abs().max()) <= atomic_sum_tol(t['dy'], t['x'], t['grid'], dtype)
    # the Function itself hands back None for a masked output
    xt = torch.tensor(t['x'], device=dev, dtype=dt)
    gt = torch.tensor(t['grid'], device=dev, dtype=dt)
    a, b = ops._GridSampleBackward.apply(torch.tensor(t['dy'], device=dev, dtype=dt), xt, gt, (False, True))
    assert a is None and torch.equal(b, dgrid)


def test_orders(dev, gold):
    """Second order equals the golden (the forward on ddx), a third-order chain through input runs and is the backward again, and a
    second derivative through grid raises."""
    from latentaugment_amd import _lib, ops
    name = 'blocks_c3'
    t = _golden_case(gold, name)
    dt = torch.float64
    xt = torch.tensor(t['x'], device=dev, dtype=dt, requires_grad=True)
    gt = torch.tensor(t['grid'], device=dev, dtype=dt)
    dyt = torch.tensor(t['dy'], device=dev, dtype=dt, requires_grad=True)
    ddx = torch.tensor(t['ddx'], device=dev, dtype=dt, requires_grad=True)
    y = ops.grid_sample(xt, gt)
    (dx,) = torch.autograd.grad(y, [xt], dyt, create_graph=True)
    (d2,) = torch.autograd.grad(dx, [dyt], ddx, create_graph=True)
    e = gold[f'g_{name}_d2']
    assert float(np.abs(np64(d2) - e).max()) <= 1e-12 * max(1.0, float(np.abs(e).max()))
    # third order: d2 = grid_sample(ddx, grid), so its gradient with respect to ddx for the incoming dy3 is the backward's dx for dy3
    dy3 = np.random.default_rng(3).standard_normal(t['dy'].shape)
    (d3,) = torch.autograd.grad(d2, [ddx], torch.tensor(dy3, device=dev, dtype=dt))
    e3, _ = gc.gs_backward(dy3, t['x'], t['grid'])
    assert float(np.abs(np64(d3) - e3).max()) <= 1e-12 * max(1.0, float(np.abs(e3).max()))
    # dx does not depend on input: that gradient is identically zero and autograd says so by 'unused'
    assert torch.autograd.grad(dx, [xt], ddx, allow_unused=True, retain_graph=True)[0] is None
    # through grid: refused, not silently zero
    g2 = gt.clone().requires_grad_(True)
    y = ops.grid_sample(xt, g2)
    dx, dgrid = torch.autograd.grad(y, [xt, g2], dyt, create_graph=True)
    for out, arg in ((dx, torch.ones_like(dx)), (dgrid, torch.ones_like(dgrid))):
        with pytest.raises(_lib.LatentAugHipError, match='second derivatives that involve grid'):
            torch.autograd.grad(out, [g2], arg, retain_graph=True)
    with pytest.raises(_lib.LatentAugHipError, match='second derivatives that involve grid'):
        torch.autograd.grad(dgrid, [dyt], torch.ones_like(dgrid), retain_graph=True)


@pytest.mark.parametrize('dtype', ['f32', 'f16', 'f64'])
def test_out_of_range_finite_positions(dev, dtype):
    """Grids at +-3 and +-1e9 (float16: +-3 and +-60000), finite, on either axis: y and dgrid are exactly 0 there and dx receives nothing
    from those outputs (the host proof of the index function is tests/test_grid_sample_cpu.py's)."""
    from latentaugment_amd import ops
    dt = TORCH[dtype]
    far = 60000.0 if dtype == 'f16' else 1e9
    N, C, H, W, Ho, Wo = 2, 3, 5, 7, 4, 66
    rng = np.random.default_rng(9)
    grid = rng.uniform(-0.9, 0.9, (N, Ho, Wo, 2)).astype(np.float16).astype(np.float64)
    out = np.zeros((N, Ho, Wo), bool)
    vals = [3.0, -3.0, far, -far]
    for j in range(Wo):
        if j % 3 == 0:      # every third column is out of range: on x, on y, or on both, with each of the four values in turn
            v = vals[(j // 3) % 4]
            axis = (j // 12) % 3
            if axis in (0, 2):
                grid[:, :, j, 0] = v
            if axis in (1, 2):
                grid[:, :, j, 1] = -v
            out[:, :, j] = True
    x = rng.standard_normal((N, C, H, W)).astype(np.float16).astype(np.float64)
    dy = rng.standard_normal((N, C, Ho, Wo)).astype(np.float16).astype(np.float64)
    y, dx, dgrid = run_first(ops, dev, dt, x, grid, dy)
    yn, dgn = np64(y), np64(dgrid)
    assert not yn[np.broadcast_to(out[:, None], yn.shape)].any() and not dgn[out].any()
    assert np.abs(yn[np.broadcast_to(~out[:, None], yn.shape)]).min() > 0 and np.isfinite(np64(dx)).all()
    # dx is what the in-range outputs alone give: the same call with the out-of-range outputs' dy zeroed
    _, dx_in, _ = run_first(ops, dev, dt, x, grid, dy * ~out[:, None])
    edx, _ = gc.gs_backward(dy * ~out[:, None], x, grid)
    tol = atomic_sum_tol(dy, x, grid, dtype)      # (a stray contribution would be a whole term: ~0.1 and more)
    assert float(np.abs(np64(dx) - edx).max()) <= tol and float(np.abs(np64(dx_in) - edx).max()) <= tol


def test_non_contiguous_inputs(dev, gold):
    from latentaugment_amd import ops
    t = _golden_case(gold, 'rot_c5')
    x = torch.tensor(t['x'], device=dev, dtype=torch.float32)
    g = torch.tensor(t['grid'], device=dev, dtype=torch.float32)
    dy = torch.tensor(t['dy'], device=dev, dtype=torch.float32)
    xs = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)      # same values, other strides
    gs = torch.stack([g, g], dim=-1)[..., 0].requires_grad_(True)
    assert not xs.is_contiguous() and not gs.is_contiguous()
    xc, gc_ = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    ya, yb = ops.grid_sample(xs, gs), ops.grid_sample(xc, gc_)
    assert torch.equal(ya, yb)
    dys = torch.stack([dy, dy], dim=-1)[..., 1]
    (dxa, dga), (dxb, dgb) = torch.autograd.grad(ya, [xs, gs], dys), torch.autograd.grad(yb, [xc, gc_], dy)
    assert torch.equal(dga, dgb) and float((dxa - dxb).abs().max()) <= atomic_sum_tol(t['dy'], t['x'], t['grid'], 'f32')
    with pytest.raises(Exception):
        ops.grid_sample(x, g.double())


# ---------------------------------------------------------------------------------------------------------------- fma
def _fma_run(ops, dev, dt, t):
    a, b, c = (torch.tensor(t[k], device=dev, dtype=dt, requires_grad=True) for k in 'abc')
    y = ops.fma(a, b, c)
    da, db, dc = torch.autograd.grad(y, [a, b, c], torch.tensor(t['dy'], device=dev, dtype=dt))
    return dict(y=y, da=da, db=db, dc=dc)


@pytest.mark.parametrize('case', gc.FMA_CASES, ids=[c[0] for c in gc.FMA_CASES])
def test_fma_float32_vs_reference(dev, gold, case):
    from latentaugment_amd import ops
    name = case[0]
    t = {k: gold[f'f_{name}_{k}'].astype(np.float64) for k in ('a', 'b', 'c', 'dy')}
    r, r2 = _fma_run(ops, dev, torch.float32, t), _fma_run(ops, dev, torch.float32, t)
    cpu32 = gc.fma_all(t['a'], t['b'], t['c'], t['dy'], np.float32)
    e = gold[f'f_{name}_y']
    assert r['y'].dtype == torch.float32 and tuple(r['y'].shape) == e.shape
    assert (np.abs(np64(r['y']) - e) <= np.spacing(np.abs(e).astype(np.float32)).astype(np.float64)).all(), name
    for k in ('da', 'db', 'dc'):
        e = gold[f'f_{name}_{k}']
        assert tuple(r[k].shape) == e.shape and r[k].dtype == torch.float32, (name, k, r[k].shape)
        ref_err = float(np.abs(cpu32[k].astype(np.float64) - e).max())
        err = float(np.abs(np64(r[k]) - e).max())
        assert err <= ref_err + ulp32(np.abs(e).max()), (name, k, err, ref_err)
    for k in r:      # two runs: the same bits
        assert torch.equal(r[k], r2[k]), (name, k)


def test_fma_second_order(dev, gold):
    from latentaugment_amd import ops
    name = gc.FMA_SECOND_ORDER
    t = {k: torch.tensor(gold[f'f_{name}_{k}'], device=dev, dtype=torch.float32, requires_grad=True) for k in ('a', 'b', 'c', 'dy')}
    y = ops.fma(t['a'], t['b'], t['c'])
    (da,) = torch.autograd.grad(y, [t['a']], t['dy'], create_graph=True)
    d2_dy, d2_b = torch.autograd.grad(da, [t['dy'], t['b']], torch.tensor(gold[f'f_{name}_dda'], device=dev, dtype=torch.float32))
    for got, k in ((d2_dy, 'd2_dy'), (d2_b, 'd2_b')):
        e = gold[f'f_{name}_{k}']
        assert tuple(got.shape) == e.shape
        # one product and a sum of at most 16 float32 terms: 16 roundings of the largest magnitude at the very most
        assert float(np.abs(np64(got) - e).max()) <= 16 * ulp32(np.abs(e).max()), k


def test_fma_integers_dtypes_and_strides(dev):
    from latentaugment_amd import ops
    rng = np.random.default_rng(31)
    # integers in [-2, 2]: every product and every sum (at most 256 terms of magnitude <= 4) is exact in float16 as well
    t = dict(a=rng.integers(-2, 3, (2, 3, 8, 32)), b=rng.integers(-2, 3, (2, 3, 1, 1)), c=rng.integers(-2, 3, (1, 1, 8, 32)),
             dy=rng.integers(-2, 3, (2, 3, 8, 32)))
    t = {k: v.astype(np.float64) for k, v in t.items()}
    exp = gc.fma_all(t['a'], t['b'], t['c'], t['dy'])
    r = _fma_run(ops, dev, torch.float32, t)
    for k, e in exp.items():
        assert np.array_equal(np64(r[k]), e), k
    for dt in (torch.float16, torch.float64):
        rr = _fma_run(ops, dev, dt, t)
        for k, e in exp.items():
            assert rr[k].dtype == dt, (dt, k)
            assert np.array_equal(np64(rr[k]), e), (dt, k)
    # operands that are views: a transposed a and an expanded b give what their contiguous copies give
    a = torch.tensor(t['a'], device=dev, dtype=torch.float32)
    b = torch.tensor(t['b'], device=dev, dtype=torch.float32)
    c = torch.tensor(t['c'], device=dev, dtype=torch.float32)
    at = a.transpose(2, 3).contiguous().transpose(2, 3)
    assert not at.is_contiguous()
    assert torch.equal(ops.fma(at, b.expand(2, 3, 8, 32), c), ops.fma(a, b, c))
    with pytest.raises(Exception):
        ops.fma(a, b, torch.zeros([5], device=dev))
