"""filtered_lrelu on the GPU: ops.filtered_lrelu (la_filtered_lrelu_f32) against the reference's goldens and the float64 restatement.

Error budget, per quantity (y, dx, db and the second-order product g2 = d<dx, v>/d(dy)): the HIP error against float64 must be at most
4x the reference's own float32 error on the same case, plus a floor of 2e-6 x the largest float64 magnitude of that quantity.
Kinks: where gain * intermediate sits within 2e-6 x its maximum of 0 or of the clamp edge, fp32 and float64 can legitimately take
different lrelu / clamp branches.  y needs no exception (a branch flip there moves y by that distance only), every element of it is
held to the budget.  The derivative quantities jump at a flip: only the dx and g2 elements whose dependency cone contains such a sample
(tests/flrelu_cpu.py, absolute taps) are taken out of the tight comparison, and db of a channel holding a sample within 1e-6.  At most
15 % of dx / g2 may be excluded, and the excluded ones must still agree to 1e-2 x the magnitude.  A sign-mask bug (wrong bit, offset or
byte) changes elements away from any kink and shows in y's own derivative products, so it cannot hide behind the exclusion.
"""
import ast
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flrelu_cpu  # noqa: E402

KINK_RTOL = 2e-6      # (an fp32 intermediate is off by ~1e-7 of the largest one: 20x margin)
MAX_EXCLUDED = 0.15


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'filtered_lrelu.npz'))


@pytest.fixture(scope='module')
def gs(golden_dir):
    """The forms and tile seams filtered_lrelu.npz has no case of (tests/golden/make_golden_flrelu_shapes.py)."""
    return np.load(os.path.join(golden_dir, 'flrelu_shapes.npz'))


def golden_case(g, name):
    m = ast.literal_eval(str(g[f'{name}_meta']))
    t = {k: torch.from_numpy(g[f'{name}_{k}']) if f'{name}_{k}' in g else None for k in ('x', 'b', 'fu', 'fd', 'dy', 'v')}
    kw = dict(up=m['up'], down=m['down'], padding=m['padding'], gain=m['gain'], slope=m['slope'], clamp=m['clamp'], flip_filter=m['flip_filter'])
    return m, t, kw


def run_hip(t, kw, dev, noncontig=False):
    from latentaugment_amd import ops
    x = t['x'].to(dev)
    if noncontig:      # same values, a transposed view of a [N, C, W, H] tensor
        x = x.transpose(2, 3).contiguous().transpose(2, 3)
        assert not x.is_contiguous()
    x.requires_grad_(True)
    b = None if t['b'] is None else t['b'].to(dev).requires_grad_(True)
    fu = None if t['fu'] is None else t['fu'].to(dev)
    fd = None if t['fd'] is None else t['fd'].to(dev)
    dy = t['dy'].to(dev).requires_grad_(True)
    y = ops.filtered_lrelu(x, fu, fd, b, **kw)
    grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
    (g2,) = torch.autograd.grad((grads[0] * t['v'].to(dev)).sum(), [dy])
    out = {'y': y, 'dx': grads[0], 'g2': g2}
    if b is not None:
        out['db'] = grads[1]
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def masks(t, kw):
    """Excluded elements per quantity (bool arrays), from the float64 kink samples of the case.  (clamp = 0: every result is an exact
    zero in any precision, nothing is excluded.)"""
    if kw['clamp'] == 0:
        z = {'y': t['dy'], 'g2': t['dy'], 'dx': t['x'], 'db': t['b']}
        return {k: np.zeros(tuple(v.shape), bool) for k, v in z.items() if v is not None}, 0
    mask, nk = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=KINK_RTOL)
    y_aff, x_aff = flrelu_cpu.affected(mask, t['x'].shape, t['fu'], t['fd'], kw['up'], kw['down'], kw['padding'], kw['flip_filter'])
    tight, _ = flrelu_cpu.kink_mask(t['x'], t['fu'], t['fd'], t['b'], **kw, rtol=1e-6)
    ch = tight.sum(dim=(0, 2, 3)) > 0
    return {'y': np.zeros(y_aff.shape, bool), 'g2': y_aff.numpy(), 'dx': x_aff.numpy(), 'db': ch.numpy()}, nk


def check(name, k, hip, ref64, ref32, excl):
    """(db: a channel is excluded only when a sample within 1e-6 x the maximum of a kink lies in it, and no share limit applies --
    every sample of a channel reaches its db)"""
    scale = float(np.abs(ref64).max())
    err = np.abs(hip - ref64)
    budget = 4.0 * float(np.abs(ref32.astype(np.float64) - ref64)[~excl].max(initial=0.0)) + 2e-6 * scale
    assert k == 'db' or excl.mean() <= MAX_EXCLUDED, f'{name} {k}: {excl.mean():.1%} of the elements sit in a kink cone'
    assert err[~excl].max(initial=0.0) <= budget, f'{name} {k}: HIP error {err[~excl].max():.3e} > budget {budget:.3e} (scale {scale:.3e})'
    assert err[excl].max(initial=0.0) <= 1e-2 * scale, f'{name} {k}: excluded elements off by {err[excl].max():.3e}'


def check_case(g, name, dev):
    m, t, kw = golden_case(g, name)
    hip = run_hip(t, kw, dev, m['noncontig'])
    ex, _ = masks(t, kw)
    for k in hip:
        check(name, k, hip[k], g[f'{name}_{k}'], g[f'{name}_{k}32'], ex[k])
    return m


def test_fused_envelope_cases_match_goldens(g, gs, dev):
    seen, multi = set(), set()
    for gg, least in ((g, 10), (gs, 17)):
        names = [str(n) for n in gg['cases'] if ast.literal_eval(str(gg[f'{n}_meta']))['path'] == 'fused']
        assert len(names) >= least
        for name in names:
            m = check_case(gg, name, dev)
            seen.add((m['up'], m['down']))
            if min(m.get('tiles', (1, 1))) >= 2:
                multi.add((m['up'], m['down']))
    nine = {(u, d) for u in (1, 2, 4) for d in (1, 2, 4)}
    assert seen >= {(1, 1), (2, 1), (1, 2), (2, 2), (4, 2), (2, 4)}
    assert seen == nine and multi == nine      # (every la_flrelu_fused_kernel<UP, DOWN>, each also with 2 x 2 tiles or more)


def test_generic_path_cases_match_goldens(g, dev):
    names = [str(n) for n in g['cases'] if ast.literal_eval(str(g[f'{n}_meta']))['path'] == 'generic']
    assert len(names) >= 3
    for name in names:
        check_case(g, name, dev)


def test_sign_round_trip_with_clamp_active(g, dev):
    """The gradients run on the sign mask the forward wrote: on the clamped cases (a real share of the samples clamped, slope 0 and
    0.2) dx and db must equal the goldens, and must differ from what an unclamped mask would give."""
    clamped = [str(n) for n in g['cases'] if ast.literal_eval(str(g[f'{n}_meta']))['clamp'] is not None]
    assert len(clamped) >= 4
    for name in clamped:
        m, t, kw = golden_case(g, name)
        a = flrelu_cpu.act_stage(flrelu_cpu.up_stage(t['x'], t['fu'], t['b'], kw['up'], kw['padding'], kw['flip_filter']), kw['gain'], kw['slope'])
        assert float((a.abs() > kw['clamp']).double().mean()) > 0.05, name
        hip = run_hip(t, kw, dev)
        ex, _ = masks(t, kw)
        for k in ('dx',) + (('db',) if t['b'] is not None else ()):
            check(name, k, hip[k], g[f'{name}_{k}'], g[f'{name}_{k}32'], ex[k])
        kw_free = dict(kw, clamp=None)
        x = t['x'].double().requires_grad_(True)
        (dx_free,) = torch.autograd.grad(flrelu_cpu.filtered_lrelu(x, t['fu'], t['fd'], t['b'], **kw_free), [x], t['dy'].double())
        assert np.abs(dx_free.numpy() - g[f'{name}_dx']).max() > 1e-2 * np.abs(g[f'{name}_dx']).max(), name


@pytest.mark.parametrize('two_d', [False, True])
def test_stylegan3_size_against_cpu_restatement(dev, two_d):
    """x [2, 64, 148, 148], up 2 / down 2, 12-tap filters, padding [11, 10, 11, 10]: many tiles and tile edges per plane."""
    from latentaugment_amd import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn([2, 64, 148, 148], generator=gen)
    b = 0.2 * torch.randn([64], generator=gen)
    t = torch.from_numpy(np.hanning(14)[1:-1]).float() * (1 + 0.2 * torch.rand(12, generator=gen))
    t = t / t.sum()
    fu = t
    fd = torch.outer(t, t.flip(0)) if two_d else t
    kw = dict(up=2, down=2, padding=[11, 10, 11, 10], gain=math.sqrt(2), slope=0.2, clamp=1.0, flip_filter=False)
    xd = x.to(dev).requires_grad_(True)
    y = ops.filtered_lrelu(xd, fu.to(dev), fd.to(dev), b.to(dev), **kw)
    dy = torch.randn(y.shape, generator=gen)
    (dx,) = torch.autograd.grad(y, [xd], dy.to(dev))
    x64 = x.double().requires_grad_(True)
    y64 = flrelu_cpu.filtered_lrelu(x64, fu, fd, b, **kw)
    (dx64,) = torch.autograd.grad(y64, [x64], dy.double())
    mask, _ = flrelu_cpu.kink_mask(x, fu, fd, b, **kw, rtol=KINK_RTOL)
    _, x_aff = flrelu_cpu.affected(mask, x.shape, fu, fd, 2, 2, kw['padding'], False)
    for hip, ref, ex in ((y, y64, torch.zeros(y64.shape, dtype=torch.bool)), (dx, dx64, x_aff)):
        hip, ref, ex = hip.detach().double().cpu().numpy(), ref.detach().numpy(), ex.numpy()
        scale = np.abs(ref).max()
        assert ex.mean() <= MAX_EXCLUDED
        err = np.abs(hip - ref)
        assert err[~ex].max() <= 1e-5 * scale, (err[~ex].max(), scale)
        assert err[ex].max(initial=0.0) <= 1e-2 * scale


def test_graph_capture_with_device_filters(g, dev):
    """Forward with device-resident taps captured once in a graph on one stream and replayed: equal to the eager launch."""
    from latentaugment_amd import ops
    _, t, kw = golden_case(g, 'u2d2')
    x = t['x'].to(dev)
    b, fu, fd = t['b'].to(dev), t['fu'].to(dev), t['fd'].to(dev)
    eager = ops.filtered_lrelu(x, fu, fd, b, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.filtered_lrelu(x, fu, fd, b, **kw)      # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ops.filtered_lrelu(x, fu, fd, b, **kw)
    x.copy_(t['x'].to(dev) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.filtered_lrelu(x, fu, fd, b, **kw))
    x.copy_(t['x'].to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_non_float32_is_refused(dev):
    from latentaugment_amd import _lib, ops
    with pytest.raises(_lib.LatentAugHipError, match='float32'):
        ops.filtered_lrelu(torch.zeros([1, 1, 8, 8], device=dev, dtype=torch.float16), up=2, down=2)
