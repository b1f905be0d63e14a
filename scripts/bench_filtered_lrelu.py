"""Time ops.filtered_lrelu (one fused launch) against the same computation composed from ops.bias_act and ops.upfirdn2d (the
reference's impl='ref' recipe, filtered_lrelu.py:133-142), forward and forward + backward, at StyleGAN3 layer shapes.

    python scripts/bench_filtered_lrelu.py [--iters 20] [--warmup 5]

Prints one JSON line.  Per case and leg: mean time per call (HIP events around `iters` calls, after `warmup` calls), achieved GB/s under
the byte model below and its share of the measured HBM copy rate, the composite's time and the speed-up.  Outputs are compared first:
fused vs composite where the composite exists (la_upfirdn2d_f32 takes at most 8 x 8 taps in a 2-D pass, so a 2-D 12 x 12 fd has none),
else vs the float64 restatement (tests/flrelu_cpu.py) on the first few planes.
Byte model (the bytes an ideal kernel must move): forward = x read once + y written once (+ the sign buffer when it is written);
backward = dy read once + dx written once + the sign buffer read once.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from latentaugment_amd import ops  # noqa: E402

HBM_COPY_GBS = 6290.0      # measured device-to-device copy rate of the MI355X (GB/s)

# (x shape, up, down, fu taps (int: 1-D, tuple: 2-D), fd taps, padding)
CASES = [
    ([8, 512, 36, 36], 2, 2, 12, 12, [11, 10, 11, 10]),
    ([8, 256, 148, 148], 2, 2, 12, 12, [11, 10, 11, 10]),
    ([8, 512, 36, 36], 4, 2, 24, 12, [17, 16, 17, 16]),
    ([8, 256, 148, 148], 2, 2, 12, (12, 12), [11, 10, 11, 10]),
]


def lowpass(n, gen):
    t = torch.from_numpy(np.hanning(n + 2)[1:-1]).float() * (1 + 0.1 * torch.rand(n, generator=gen))
    return t / t.sum()


def make_filter(spec, gen):
    if isinstance(spec, int):
        return lowpass(spec, gen)
    return torch.outer(lowpass(spec[0], gen), lowpass(spec[1], gen))


def composite(x, fu, fd, b, up, down, padding, gain, slope, clamp):
    """filtered_lrelu from the existing ops (filtered_lrelu.py:139-142)."""
    y = ops.bias_act(x, b)
    y = ops.upfirdn2d(y, fu, up=up, padding=padding, gain=up ** 2)
    y = ops.bias_act(y, act='lrelu', alpha=slope, gain=gain, clamp=clamp)
    return ops.upfirdn2d(y, fd, down=down)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    gain, slope, clamp = math.sqrt(2), 0.2, 256.0
    results = []
    for shape, up, down, fus, fds, pad in CASES:
        fu, fd = make_filter(fus, gen).to(dev), make_filter(fds, gen).to(dev)
        x = torch.randn(shape, generator=gen).to(dev)
        b = (0.1 * torch.randn([shape[1]], generator=gen)).to(dev)
        kw = dict(up=up, down=down, padding=pad, gain=gain, slope=slope, clamp=clamp)
        fuc, fdc = fu.cpu(), fd.cpu()      # (ops.upfirdn2d takes its taps from the host)
        y = ops.filtered_lrelu(x, fu, fd, b, **kw)
        has_comp = fd.ndim == 1 or fd.numel() <= 64
        if has_comp:
            yc = composite(x, fuc, fdc, b, up, down, pad, gain, slope, clamp)
            check = 'composite'
            err = float((y - yc).abs().max() / yc.abs().max())
        else:
            import flrelu_cpu
            planes = slice(0, 4)
            y64 = flrelu_cpu.filtered_lrelu(x[:1, planes].cpu(), fu.cpu(), fd.cpu(), b[planes].cpu(), **kw, flip_filter=False)
            check = 'float64 restatement, 4 planes'
            err = float((y[:1, planes].cpu().double() - y64).abs().max() / y64.abs().max())
        assert err < 1e-4, (shape, err)
        dy = torch.randn(y.shape, generator=gen).to(dev)
        xg = x.clone().requires_grad_(True)
        rows, row_bytes = ops._flr_sign_shape(shape[2], shape[3], fu.shape[0] if fu.ndim == 2 else 0, fu.shape[-1],
                                              fd.shape[0] if fd.ndim == 2 else 0, fd.shape[-1], up, down, *pad)
        sign_bytes = shape[0] * shape[1] * rows * row_bytes
        bx, by = 4 * x.numel(), 4 * y.numel()
        legs = {
            'fwd': (lambda: ops.filtered_lrelu(x, fu, fd, b, **kw), bx + by,
                    (lambda: composite(x, fuc, fdc, b, up, down, pad, gain, slope, clamp)) if has_comp else None),
            'fwd_bwd': (lambda: torch.autograd.grad(ops.filtered_lrelu(xg, fu, fd, b, **kw), [xg], dy), bx + by + sign_bytes + by + bx + sign_bytes,
                        (lambda: torch.autograd.grad(composite(xg, fuc, fdc, b, up, down, pad, gain, slope, clamp), [xg], dy)) if has_comp else None),
        }
        case = dict(x=shape, up=up, down=down, fu=fus, fd=fds, padding=pad, check=check, max_rel_diff=err)
        for leg, (fn, nbytes, comp) in legs.items():
            us = timed(fn, args.iters, args.warmup)
            r = dict(us=round(us, 1), gbs=round(nbytes / us / 1e3, 1), hbm_share=round(nbytes / us / 1e3 / HBM_COPY_GBS, 3))
            if comp is not None:
                cus = timed(comp, args.iters, args.warmup)
                r.update(composite_us=round(cus, 1), speedup=round(cus / us, 2))
            else:
                r.update(composite_us=None, speedup=None)
            case[leg] = r
        results.append(case)
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench='filtered_lrelu', device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                          hbm_copy_gbs=HBM_COPY_GBS, cases=results)))


if __name__ == '__main__':
    main()
