"""float16 and float64 bias_act / upfirdn2d on the GPU (la_bias_act_ex_f16 / _f64, la_bias_sum_f16 / _f64, la_upfirdn2d_f16 / _f64).

float64: at most 1e-12 x max(1, max |expected|) from the reference's impl='ref' path run in float64 (bias_act_full.npz, upfirdn_sep.npz
with their float32 inputs widened, and the float64 cases of op_dtypes.npz).
float16: every output is float16.  A forward value is within 1 fp16 ULP of the float64 value (plus the float32 accumulation's own
rounding, 1e-7 x the largest magnitude, which only matters next to zero where fp16 is finer than that); a separable filter's two
passes round a float16 intermediate, as the reference's plugin path does, and add 2x the reference's own float16 error on that case (it
rounds the same intermediate).  A gradient may differ from float64 by at most 2x the reference's own float16 error on that case plus
1 fp16 ULP of its largest magnitude.  Kinks: where the pre-activation lies within 1e-3 of an activation kink or the pre-clamp value
within 1 fp16 ULP below the clamp, float16 rounding can take the other branch; those gradient elements are left out of the tight check
(and of the reference's error) and reported.
"""
import ast
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16_EPS32 = 1e-7      # float32 accumulation, relative to the largest magnitude of the case


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def od(golden_dir):
    return np.load(os.path.join(golden_dir, 'op_dtypes.npz'))


def _cases(od, kind):
    return [ast.literal_eval(str(r)) for r in od['cases'] if ast.literal_eval(str(r))[0].startswith(kind)]


def ulp16(v):
    """Spacing of float16 at |v| (2^-24 in the subnormal range), elementwise, as float64 numpy."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float16)).astype(np.float64)


def ulp16_t(v):
    """ulp16 on the device: 2^(e - 11) for |v| = m 2^e, m in [0.5, 1), at least 2^-24."""
    _, e = torch.frexp(v.float())
    return torch.clamp(torch.ldexp(torch.ones_like(v, dtype=torch.float32), e - 11), min=2.0 ** -24)


def np64(t):
    return t.detach().double().cpu().numpy()


def _ba_kw(kwrep):
    return {k: v for k, v in ast.literal_eval(kwrep).items() if v is not None}


def _run_bias_act(ops, x, b, dy, ddx, act, kw, has2):
    x = x.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    y = ops.bias_act(x, b, dim=1, act=act, **kw)
    dx, db = torch.autograd.grad(y, [x, b], dy, create_graph=True)
    d2 = torch.autograd.grad(dx, [x], ddx)[0] if has2 else torch.zeros_like(x)
    return {'y': y, 'dx': dx, 'd2': d2, 'db': db}


# ---------------------------------------------------------------- float64
def test_bias_act_float64_vs_reference(dev, golden_dir):
    """bias_act_full.npz (all activations, default and gain / clamp / alpha parameters): y, dx (grad 1), d2 (grad 2), db in float64."""
    from latentaugment_amd import ops
    gb = np.load(os.path.join(golden_dir, 'bias_act_full.npz'))
    for rep in gb['cases']:
        name, act, gain, clamp, alpha, _, _, _, _, has2 = ast.literal_eval(str(rep))
        kw = dict(gain=None if gain < 0 else gain, clamp=None if clamp < 0 else clamp, alpha=None if alpha < 0 else alpha)
        t = {k: torch.tensor(gb[f'{name}_{k}'], device=dev, dtype=torch.float64) for k in ('x', 'b', 'dy', 'ddx')}
        r = _run_bias_act(ops, t['x'], t['b'], t['dy'], t['ddx'], act, {k: v for k, v in kw.items() if v is not None}, has2)
        exp = {'y': gb[f'{name}_y'], 'dx': gb[f'{name}_dx'], 'd2': gb[f'{name}_d2'], 'db': gb[f'{name}_dx'].sum(axis=(0, 2, 3))}
        for k, e in exp.items():
            assert r[k].dtype == torch.float64, (name, k)
            err = float(np.abs(np64(r[k]) - e).max())
            assert err <= 1e-12 * max(1.0, float(np.abs(e).max())), (name, act, k, err)


def test_upfirdn2d_float64_vs_reference(dev, golden_dir, od):
    """upfirdn_sep.npz (8- and 12-tap separable filters, float32 inputs widened) and the 2-D cases of op_dtypes.npz in float64."""
    from latentaugment_amd import ops
    gs = np.load(os.path.join(golden_dir, 'upfirdn_sep.npz'))
    runs = []
    for rep in gs['cases']:
        name, _, op, kwrep = ast.literal_eval(str(rep))
        runs.append((name, op, ops.setup_filter(list(gs[f'{name}_taps'])), ast.literal_eval(kwrep), gs[f'{name}_x'], gs[f'{name}_dy'],
                     gs[f'{name}_y'], gs[f'{name}_dx']))
    for name, op, taps, kwrep in _cases(od, 'u'):
        runs.append((name, op, ops.setup_filter(ast.literal_eval(taps)), ast.literal_eval(kwrep), od[f'{name}_x'], od[f'{name}_dy'],
                     od[f'{name}_y'], od[f'{name}_dx']))
    assert len(runs) == 19
    for name, op, f, kw, x, dy, ey, edx in runs:
        xt = torch.tensor(x, device=dev, dtype=torch.float64, requires_grad=True)
        y = getattr(ops, op)(xt, f, **kw)
        (dx,) = torch.autograd.grad(y, [xt], torch.tensor(dy, device=dev, dtype=torch.float64))
        for k, got, e in (('y', y, ey), ('dx', dx, edx)):
            assert got.dtype == torch.float64 and tuple(got.shape) == e.shape, (name, k)
            err = float(np.abs(np64(got) - e).max())
            assert err <= 1e-12 * max(1.0, float(np.abs(e).max())), (name, op, k, err)


def test_bias_act_float64_on_float16_inputs(dev, od):
    """The float64 side of op_dtypes.npz's bias_act cases (the inputs the float16 test uses)."""
    from latentaugment_amd import ops
    for name, _, act, kwrep in _cases(od, 'b'):
        has2 = ops._ACTS[act][4]
        t = {k: torch.tensor(od[f'{name}_{k}'], device=dev, dtype=torch.float64) for k in ('x', 'b', 'dy', 'ddx')}
        r = _run_bias_act(ops, t['x'], t['b'], t['dy'], t['ddx'], act, _ba_kw(kwrep), has2)
        for k in ('y', 'dx', 'd2', 'db'):
            e = od[f'{name}_{k}']
            err = float(np.abs(np64(r[k]) - e).max())
            assert err <= 1e-12 * max(1.0, float(np.abs(e).max())), (name, act, k, err)


# ---------------------------------------------------------------- float16
def _kink_mask(act, kw, v, y64):
    """Elements whose gradient float16 rounding may legitimately flip (module docstring): v = x + b in float64, y64 the float64 output."""
    mask = np.zeros(v.shape, bool)
    if act in ('relu', 'lrelu', 'elu', 'selu'):
        mask |= np.abs(v) < 1e-3
    clamp = kw.get('clamp')
    if clamp is not None:
        mask |= (np.abs(y64) < clamp) & (np.abs(y64) >= clamp - ulp16(clamp))
    return mask


def test_bias_act_float16_vs_reference(dev, od):
    from latentaugment_amd import ops
    report = []
    for name, _, act, kwrep in _cases(od, 'b'):
        kw = _ba_kw(kwrep)
        has2 = ops._ACTS[act][4]
        t = {k: torch.tensor(od[f'{name}_{k}'], device=dev) for k in ('x', 'b', 'dy', 'ddx')}
        assert t['x'].dtype == torch.float16
        r = _run_bias_act(ops, t['x'], t['b'], t['dy'], t['ddx'], act, kw, has2)
        for k, v in r.items():
            assert v.dtype == torch.float16, (name, k, v.dtype)
        # forward: 1 ULP of the float64 value, element by element
        y64, y = od[f'{name}_y'], np64(r['y'])
        err = np.abs(y - y64)
        assert (err <= ulp16(y64) + F16_EPS32 * np.abs(y64).max()).all(), (name, act, float(err.max()))
        # gradients: 2x the reference's own float16 error + 1 ULP of the largest magnitude, kinks excluded
        v = od[f'{name}_x'].astype(np.float64) + od[f'{name}_b'].astype(np.float64)[None, :, None, None]
        excl = _kink_mask(act, kw, v, y64)
        report.append((name, act, int(excl.sum())))
        for k in ('dx', 'd2') if has2 else ('dx',):
            e, e16, got = od[f'{name}_{k}'], od[f'{name}_{k}16'].astype(np.float64), np64(r[k])
            ref_err = float(np.abs(e16 - e)[~excl].max(initial=0.0))
            err = float(np.abs(got - e)[~excl].max(initial=0.0))
            assert err <= 2 * ref_err + float(ulp16(np.abs(e).max())), (name, act, k, err, ref_err)
        # db sums dx: the excluded elements may add their own |dx| at most
        e, e16, got = od[f'{name}_db'], od[f'{name}_db16'].astype(np.float64), np64(r['db'])
        slack = float((np.abs(od[f'{name}_dx']) * excl).sum(axis=(0, 2, 3)).max())
        err = float(np.abs(got - e).max())
        assert err <= 2 * float(np.abs(e16 - e).max()) + float(ulp16(np.abs(e).max())) + slack, (name, act, 'db', err)
    print('float16 bias_act: kink-excluded elements per case', report)


def test_upfirdn2d_float16_vs_reference(dev, od):
    """2-D [1,3,3,1] through upsample2d / downsample2d / filter2d (the float16 4x4 kernels), 3x3 / 8x8 filters with pads, flip and gain,
    a 12-tap separable filter (two passes, float16 intermediate)."""
    from latentaugment_amd import ops
    for name, op, taps, kwrep in _cases(od, 'u'):
        f = ops.setup_filter(ast.literal_eval(taps))
        x = torch.tensor(od[f'{name}_x'], device=dev, requires_grad=True)
        y = getattr(ops, op)(x, f, **ast.literal_eval(kwrep))
        (dx,) = torch.autograd.grad(y, [x], torch.tensor(od[f'{name}_dy'], device=dev))
        assert y.dtype == torch.float16 and dx.dtype == torch.float16, name
        y64 = od[f'{name}_y']
        err = np.abs(np64(y) - y64)
        two_pass = 2 * float(np.abs(od[f'{name}_y16'].astype(np.float64) - y64).max()) if f.ndim == 1 else 0.0
        assert (err <= ulp16(y64) + F16_EPS32 * np.abs(y64).max() + two_pass).all(), (name, op, float(err.max()))
        e, e16 = od[f'{name}_dx'], od[f'{name}_dx16'].astype(np.float64)
        err = float(np.abs(np64(dx) - e).max())
        assert err <= 2 * float(np.abs(e16 - e).max()) + float(ulp16(np.abs(e).max())), (name, op, 'dx', err)


def _assert_within_ulp16(h, ref32, what):
    """float16 result h within 1 fp16 ULP of the float32 op's result, element by element (on the device)."""
    d = (h.float() - ref32).abs()
    tol = ulp16_t(ref32) + F16_EPS32 * float(ref32.abs().max())
    bad = int((d > tol).sum())
    assert bad == 0, (what, bad, float(d.max()))


def test_float16_matches_float32_at_sg2_size(dev):
    """[4,128,256,256], the size of an SG2 float16 layer: lrelu + clamp 256 (bias_act's defaults for a conv layer), upsample2d and
    downsample2d with [1,3,3,1] -- the float16 result equals the float32 op's on the same inputs to 1 fp16 ULP."""
    from latentaugment_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    x = (torch.randn([4, 128, 256, 256], device=dev, generator=g) * 120).half()
    b = (torch.randn([128], device=dev, generator=g) * 10).half()
    y16 = ops.bias_act(x, b, act='lrelu', clamp=256)
    y32 = ops.bias_act(x.float(), b.float(), act='lrelu', clamp=256)
    assert y16.dtype == torch.float16 and y32.dtype == torch.float32
    assert int((y32.abs() == 256).sum()) > 0      # (the clamp is active somewhere)
    _assert_within_ulp16(y16, y32, 'bias_act')
    del y16, y32
    f = ops.setup_filter([1, 3, 3, 1])
    for op in (ops.upsample2d, ops.downsample2d, ops.filter2d):
        h = op(x, f)
        r = op(x.float(), f)
        assert h.dtype == torch.float16 and h.shape == r.shape
        _assert_within_ulp16(h, r, op.__name__)
        del h, r


@pytest.mark.parametrize('dtype', [torch.float16, torch.float64])
def test_adjoint_identity_at_sg2_size(dev, dtype):
    """<up(x), r> == <x, up^T(r)> (and the same for down) at [4,128,256,256]: the backward launch is the forward's adjoint.  The sums are
    formed in float64; the tolerance is the dtype's rounding of every product's factor (2^-10 for float16, 1e-12 for float64) times the
    sum of the magnitudes."""
    from latentaugment_amd import ops
    g = torch.Generator(device=dev).manual_seed(6)
    f = ops.setup_filter([1, 3, 3, 1])
    rel = 2.0 ** -10 if dtype == torch.float16 else 1e-12
    x = torch.randn([4, 128, 256, 256], device=dev, generator=g).to(dtype).requires_grad_(True)
    for op in (ops.upsample2d, ops.downsample2d):
        y = op(x, f)
        r = torch.randn(y.shape, device=dev, generator=g).to(dtype)
        (xt,) = torch.autograd.grad(y, [x], r)
        assert y.dtype == dtype and xt.dtype == dtype
        lhs = (y.detach().double() * r.double()).sum()
        rhs = (x.detach().double() * xt.double()).sum()
        mag = float((y.detach().double() * r.double()).abs().sum() + (x.detach().double() * xt.double()).abs().sum())
        assert abs(float(lhs - rhs)) <= rel * mag, (op.__name__, float(lhs), float(rhs), mag)
        del y, r, xt


# ---------------------------------------------------------------- contract
def test_dtype_contract(dev):
    from latentaugment_amd import _lib, ops
    x16 = torch.randn([2, 4, 16, 16], device=dev).half()
    for x, b in ((x16, torch.zeros([4], device=dev)), (x16.double(), torch.zeros([4], device=dev, dtype=torch.float16))):
        with pytest.raises(_lib.LatentAugHipError, match='dtype'):
            ops.bias_act(x, b, act='lrelu')
    with pytest.raises(_lib.LatentAugHipError, match='8x8'):
        ops.upfirdn2d(x16, torch.ones([9, 9]))
    # every other dtype is computed and returned in float32, as before
    xb = x16.to(torch.bfloat16)
    assert ops.bias_act(xb, torch.zeros([4], device=dev, dtype=torch.bfloat16), act='lrelu').dtype == torch.float32
    assert ops.upsample2d(xb, ops.setup_filter([1, 3, 3, 1])).dtype == torch.float32
    # float32 stays float32 and a float32 call equals its float16 counterpart's float32 twin
    assert ops.bias_act(x16.float(), act='lrelu').dtype == torch.float32
    # empty tensors and no-bias calls keep the dtype too
    assert ops.bias_act(x16[:0], None).dtype == torch.float16
    assert ops.bias_act(x16.double(), None, act='tanh').dtype == torch.float64


def test_float16_graph_capture_replays_eager(dev):
    """One float16 bias_act + upsample2d captured in a graph and replayed: bit-identical to the eager launches."""
    from latentaugment_amd import ops
    f = ops.setup_filter([1, 3, 3, 1])
    x = (torch.randn([2, 16, 32, 32], device=dev) * 50).half()
    b = torch.randn([16], device=dev).half()

    def step():
        return ops.upsample2d(ops.bias_act(x, b, act='lrelu', clamp=256), f)
    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()      # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and torch.equal(out, eager)
    x.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, step())
    assert not math.isnan(float(out.float().abs().max()))
