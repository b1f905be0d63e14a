"""ops.conv2d_resample (la_conv_op.hip) on the GPU against the float64 CPU restatement oracle/sg2_ops.py:conv2d_resample: the ten G4
goldens of l0_ops.npz (y, gx, gw), a sweep over every case of conv2d_op_cases.CASES (both kernel paths of forward, data gradient and
weight gradient, strides 1 / 2 / 4, transposed forms, groups 1 / 2 / 3, ragged channel counts, 1x1 .. 7x7 kernels, rectangular images,
unequal and negative padding, flip_weight both ways, up with down, batch 1, one channel, one layer of real size), second-order gradients
on one case per path and on every branch that runs through upfirdn2d, run-to-run determinism of the split-K weight gradient, graph capture of forward + backward, and misuse.

Bound (the project's rule, nothing tuned to the kernels): HIP error <= 4 x the float32 yardstick's own error on that case (max norm) +
2e-6 x the largest float64 magnitude.  Yardstick: the reference's own float32 result for the goldens, the same oracle run in float32 on
the CPU for the sweep and the second-order checks.  The op is linear in each argument: no element is left out of any comparison.
Inputs come from a seeded CPU generator.

Measured on one MI355X: the whole file (65 tests) takes 4 s, most of it the CPU oracles (float64 and float32 of the 128 -> 128 layer).
"""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv2d_op_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'l0_ops.npz'))


def check(name, what, hip, ref64, yard):
    """yard: the float32 yardstick's result (its error against ref64 is the allowance)."""
    hip, ref64, yard = (np.asarray(v, dtype=np.float64) for v in (hip, ref64, yard))
    assert hip.shape == ref64.shape, (name, what, hip.shape, ref64.shape)
    scale = float(np.abs(ref64).max())
    err = float(np.abs(hip - ref64).max())
    own = float(np.abs(yard - ref64).max())
    bound = 4 * own + 2e-6 * scale
    print(f'{name:24s} {what:10s} err {err:.3e}  yardstick {own:.3e}  bound {bound:.3e}  scale {scale:.3e}')
    assert np.isfinite(hip).all(), (name, what)
    assert err <= bound, (name, what, err, bound, own, scale)


def first_order(mod, x, w, dy, f, kw):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = mod.conv2d_resample(x, w, f=f, **kw)
    gx, gw = torch.autograd.grad(y, [x, w], dy)
    return {'y': y.detach(), 'gx': gx, 'gw': gw}


def oracle_first_order(x, w, dy, f, kw, dtype):
    from oracle import sg2_ops
    return {k: v.double().numpy() for k, v in first_order(sg2_ops, x.to(dtype), w.to(dtype), dy.to(dtype), f, kw).items()}


def test_g4_goldens(g, dev):
    from latentaugment_amd import ops
    f = ops.setup_filter([1, 3, 3, 1])
    n = int(g['G4_count'])
    assert n == 10
    for k in range(n):
        groups, kw = [str(s) for s in g[f'G4_{k}_meta']]
        kw = dict(ast.literal_eval(kw), groups=int(groups))
        x, w, dy = (torch.from_numpy(g[f'G4_{k}_{q}']) for q in ('x', 'w', 'dy'))
        r64 = oracle_first_order(x, w, dy, f, kw, torch.float64)
        hip = first_order(ops, x.to(dev), w.to(dev), dy.to(dev), f, kw)
        for q in ('y', 'gx', 'gw'):
            check(f'G4_{k}', q, hip[q].cpu().numpy(), r64[q], g[f'G4_{k}_{q}'])


def case_tensors(c, seed):
    gen = torch.Generator().manual_seed(seed)
    n, cin, h, wd = c['x']
    x = torch.randn([n, cin, h, wd], generator=gen)
    w = torch.randn([c['cout'], cin // c['groups'], c['kh'], c['kw']], generator=gen)
    call = cc.path_plan(c)['call']
    from oracle import sg2_ops
    f = None if c['f'] is None else sg2_ops.setup_filter(list(c['f']))
    kw = dict(up=c['up'], down=c['down'], padding=c['padding'], groups=c['groups'], flip_weight=c['flip_weight'], flip_filter=c['flip_filter'])
    with torch.no_grad():
        yshape = sg2_ops.conv2d_resample(x[:1], w, f=f, **kw).shape
    dy = torch.randn([n, *yshape[1:]], generator=gen)
    return x, w, dy, f, kw, call


@pytest.mark.parametrize('name', [c['name'] for c in cc.CASES])
def test_sweep(name, dev):
    from latentaugment_amd import ops
    c = cc.BY_NAME[name]
    x, w, dy, f, kw, _ = case_tensors(c, 1000 + cc.CASES.index(c))
    r64 = oracle_first_order(x, w, dy, f, kw, torch.float64)
    r32 = oracle_first_order(x, w, dy, f, kw, torch.float32)
    hip = first_order(ops, x.to(dev), w.to(dev), dy.to(dev), f, kw)
    for q in ('y', 'gx', 'gw'):
        check(name, q, hip[q].cpu().numpy(), r64[q], r32[q])


def second_order(mod, x, w, dy, u, v, f, kw):
    """d<gx, v>/d(dy), d<gx, v>/dw, d<gw, u>/dx, d<gw, u>/d(dy)"""
    x, w, dy = (t.clone().requires_grad_(True) for t in (x, w, dy))
    y = mod.conv2d_resample(x, w, f=f, **kw)
    gx, gw = torch.autograd.grad(y, [x, w], dy, create_graph=True)
    a_dy, a_w = torch.autograd.grad((gx * v).sum(), [dy, w], retain_graph=True)
    c_x, c_dy = torch.autograd.grad((gw * u).sum(), [x, dy])
    return {'gxv_ddy': a_dy, 'gxv_dw': a_w, 'gwu_dx': c_x, 'gwu_ddy': c_dy}


@pytest.mark.parametrize('name', cc.SECOND_ORDER + cc.SECOND_ORDER_RESAMPLED)
def test_second_order(name, dev):
    from latentaugment_amd import ops
    from oracle import sg2_ops
    c = cc.BY_NAME[name]
    x, w, dy, f, kw, _ = case_tensors(c, 77)
    gen = torch.Generator().manual_seed(78)
    u, v = torch.randn(w.shape, generator=gen), torch.randn(x.shape, generator=gen)
    r64 = second_order(sg2_ops, *(t.double() for t in (x, w, dy, u, v)), f, kw)
    r32 = second_order(sg2_ops, x, w, dy, u, v, f, kw)
    hip = second_order(ops, *(t.to(dev) for t in (x, w, dy, u, v)), f, kw)
    for q in r64:
        check(name, q, hip[q].cpu().numpy(), r64[q].numpy(), r32[q].numpy())


def test_weight_gradient_is_deterministic(dev):
    from latentaugment_amd import ops
    c = cc.BY_NAME[cc.MANY_SLICES]
    assert cc.path_plan(c)['slices'] >= 32
    x, w, dy, f, kw, _ = case_tensors(c, 5)
    a = first_order(ops, x.to(dev), w.to(dev), dy.to(dev), f, kw)
    b = first_order(ops, x.to(dev), w.to(dev), dy.to(dev), f, kw)
    for q in ('y', 'gx', 'gw'):
        assert torch.equal(a[q], b[q]), q


def test_graph_capture_forward_and_backward(dev):
    """Forward plus autograd.grad of an engine-path case captured on one stream, replayed with new input contents: equal to the eager
    result bit for bit."""
    from latentaugment_amd import ops
    c = cc.BY_NAME[cc.GRAPH_CASE]
    x0, w0, dy0, f, kw, _ = case_tensors(c, 9)
    x, w, dy = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True), dy0.to(dev)

    def run():
        y = ops.conv2d_resample(x, w, f=f, **kw)
        gx, gw = torch.autograd.grad(y, [x, w], dy)
        return y.detach(), gx, gw

    eager = [t.clone() for t in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()      # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = run()
    with torch.no_grad():
        x.copy_(x0.to(dev) * 0.5 + 1)
        w.copy_(w0.to(dev) * -2)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, run()):
        assert torch.equal(a, b)
    with torch.no_grad():
        x.copy_(x0.to(dev))
        w.copy_(w0.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_misuse_raises_and_leaves_the_device_usable(dev):
    from latentaugment_amd import _lib, ops
    x = torch.randn([1, 4, 8, 8], device=dev)
    w = torch.randn([4, 4, 3, 3], device=dev)
    with pytest.raises(AssertionError):
        ops.conv2d_resample(x, w.double())
    with pytest.raises(_lib.LatentAugHipError, match='float32'):
        ops.conv2d_resample(x.half(), w.half())
    with pytest.raises(_lib.LatentAugHipError, match='7x7'):
        ops.conv2d_resample(x.new_zeros([1, 4, 16, 16]), torch.zeros([4, 4, 9, 9], device=dev), padding=4)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        ops.conv2d_resample(x, w.cpu())
    with pytest.raises(_lib.LatentAugHipError, match='smaller than 1x1'):
        ops.conv2d(x[:, :, :2, :2], w)
    y = ops.conv2d_resample(x, w, padding=1)
    ref = torch.nn.functional.conv2d(x.cpu().double(), w.cpu().double(), padding=1)
    torch.cuda.synchronize()
    assert float((y.cpu().double() - ref).abs().max()) <= 1e-4
