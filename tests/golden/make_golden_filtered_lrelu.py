#!/usr/bin/env python3
"""Golden vectors of filtered_lrelu, by RUNNING THE REFERENCE here.

    python tests/golden/make_golden_filtered_lrelu.py     ->  tests/golden/filtered_lrelu.npz

Executed from the reference (imported, never copied): models/stylegan3/torch_utils/ops/filtered_lrelu.py, filtered_lrelu(..., impl='ref')
(:59-142: bias_act + upfirdn2d + bias_act + upfirdn2d on CPU), with autograd through it.  Per case, in float64 AND in float32 (the
reference's own float32 error sets the error budget of the HIP op): y, dx and db for an incoming gradient dy, and one second-order
product g2 = d<dx, v>/d(dy).  Inputs are stored in float32 and both runs start from those exact values."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/models/stylegan3')
from torch_utils.ops import filtered_lrelu as ref      # noqa: E402

rng = np.random.default_rng(7)


def taps1d(n):
    """Asymmetric low-pass taps (a Hann window, jittered so that flip_filter matters), normalised to sum 1."""
    t = np.hanning(n + 2)[1:-1] * (1 + 0.3 * rng.standard_normal(n))
    return t / t.sum()


def taps2d(h, w):
    t = np.outer(taps1d(h), taps1d(w)) + 0.02 * rng.standard_normal([h, w])
    return t / t.sum()


def radial(n):
    """2-D radially symmetric low-pass (a windowed jinc-like profile), normalised to sum 1."""
    c = (n - 1) / 2
    yy, xx = np.mgrid[:n, :n]
    r = np.hypot(yy - c, xx - c) / (n / 2)
    t = np.where(r < 1, np.cos(np.pi * r / 2) ** 2 * np.sinc(1.5 * r), 0)
    return t / t.sum()


def filt(spec):
    if spec is None:
        return None
    kind, *a = spec
    return torch.tensor({'1d': taps1d, '2d': taps2d, 'radial': radial}[kind](*a), dtype=torch.float32)


# name: (N, C, H, W, up, down, fu spec, fd spec, padding, flip, slope, clamp, bias, noncontig, path)
# clamp: k -> the clamp is set where it trips on ~30 % * k of the intermediate samples (a real share, not a corner case)
CASES = {
    'u1d1': (2, 3, 11, 13, 1, 1, ('2d', 3, 3), ('1d', 5), [2, 1, 1, 2], False, 0.2, None, True, False, 'fused'),
    'u2d1': (1, 3, 9, 11, 2, 1, ('1d', 12), None, [11, 10, 11, 10], False, 0.2, 0.8, True, False, 'fused'),
    'u1d2': (2, 2, 13, 15, 1, 2, None, ('1d', 12), [5, 6, 5, 6], True, 0.2, None, False, False, 'fused'),
    'u2d2': (2, 3, 13, 11, 2, 2, ('1d', 12), ('1d', 12), [11, 10, 11, 10], False, 0.2, 0.7, True, False, 'fused'),
    'u2d2_nc': (2, 2, 9, 13, 2, 2, ('1d', 12), ('1d', 12), [11, 10, 11, 10], False, 0.2, None, True, True, 'fused'),
    'u4d2': (1, 2, 9, 7, 4, 2, ('1d', 24), ('1d', 12), [17, 16, 17, 16], False, 0.2, 0.9, True, False, 'fused'),
    'u2d4': (1, 2, 15, 13, 2, 4, ('1d', 12), ('1d', 24), [9, 8, 9, 8], True, 0.2, None, True, False, 'fused'),
    'u2d2_rad': (1, 3, 11, 9, 2, 2, ('radial', 12), ('radial', 12), [11, 10, 11, 10], False, 0.2, 0.6, True, False, 'fused'),
    'u2d2_odd': (2, 2, 11, 13, 2, 2, ('1d', 11), ('2d', 7, 5), [-2, 3, 4, -1], True, 0.0, None, True, False, 'fused'),
    'u1d1_s0': (1, 2, 10, 9, 1, 1, ('2d', 3, 3), ('2d', 3, 3), [1, 1, 1, 1], False, 0.0, 0.5, False, False, 'fused'),
    'u2d1_flip': (1, 2, 12, 9, 2, 1, ('2d', 6, 8), ('1d', 1), [3, 4, 2, 5], True, 0.2, None, False, False, 'fused'),
    'u4d2_rad': (1, 2, 7, 8, 4, 2, ('radial', 16), ('1d', 8), [10, 9, 10, 9], False, 0.2, None, True, False, 'fused'),
    'g_u3d2': (1, 2, 9, 11, 3, 2, ('1d', 9), ('1d', 6), [4, 3, 5, 2], False, 0.2, 0.8, True, False, 'generic'),
    'g_tap40': (1, 2, 16, 12, 2, 2, ('1d', 40), ('1d', 12), [30, 20, 25, 24], True, 0.2, None, True, False, 'generic'),
    'g_u1d3': (1, 2, 17, 14, 1, 3, ('2d', 3, 2), ('2d', 10, 9), [4, 5, 3, 6], False, 0.0, 0.6, False, False, 'generic'),
    'g_u2d2_fd20': (1, 2, 10, 11, 2, 2, ('radial', 12), ('1d', 20), [14, 13, 16, 15], False, 0.2, None, True, False, 'generic'),
}


def run(x, b, fu, fd, dy, v, kw, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    b = None if b is None else b.to(dtype).clone().requires_grad_(True)
    dy = dy.to(dtype).clone().requires_grad_(True)
    y = ref.filtered_lrelu(x, fu, fd, b, impl='ref', **kw)
    grads = torch.autograd.grad(y, [x] + ([b] if b is not None else []), dy, create_graph=True)
    dx = grads[0]
    (g2,) = torch.autograd.grad((dx * v.to(dtype)).sum(), [dy])
    out = {'y': y.detach(), 'dx': dx.detach(), 'g2': g2.detach()}
    if b is not None:
        out['db'] = grads[1].detach()
    return out


def main():
    torch.manual_seed(3)
    out, names = {}, []
    for name, (n, c, h, w, up, down, fus, fds, pad, flip, slope, clampk, has_b, nc, path) in CASES.items():
        fu, fd = filt(fus), filt(fds)
        x = torch.randn([n, c, h, w])
        b = 0.3 * torch.randn([c]) if has_b else None
        kw = dict(up=up, down=down, padding=pad, gain=float(np.sqrt(2)), slope=slope, clamp=None, flip_filter=flip)
        if clampk is not None:      # (a quantile of |lrelu| of the unclamped intermediate)
            sys.path.insert(0, os.path.dirname(HERE))
            import flrelu_cpu
            a = flrelu_cpu.act_stage(flrelu_cpu.up_stage(x, fu, b, up, pad, flip), kw['gain'], slope)
            v = np.sort(a.abs().numpy().ravel())
            i = int((1 - 0.3 * clampk) * v.size)
            kw['clamp'] = float(np.float32((v[i] + v[i + 1]) / 2))      # (half-way between two samples: no sample sits on the edge)
        y0 = ref.filtered_lrelu(x.double(), fu, fd, None if b is None else b.double(), impl='ref', **kw)
        dy = torch.randn(y0.shape)
        v = torch.randn(x.shape)
        r64 = run(x, b, fu, fd, dy, v, kw, torch.float64)
        r32 = run(x, b, fu, fd, dy, v, kw, torch.float32)
        names.append(name)
        meta = dict(kw, fu=fus, fd=fds, noncontig=nc, path=path)
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
        print(name, tuple(x.shape), '->', tuple(y0.shape), 'clamp', kw['clamp'])
    out['cases'] = np.array(names)
    path = os.path.join(HERE, 'filtered_lrelu.npz')
    np.savez_compressed(path, **out)
    print(len(names), 'cases,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
