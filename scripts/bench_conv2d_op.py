"""Micro-benchmark of ops.conv2d_resample: forward, data gradient and weight gradient of three layers, beside the
torch.nn.functional.conv2d / conv_transpose2d calls (and their autograd) that the reference's conv2d_gradfix makes on the same device.

  python scripts/bench_conv2d_op.py [--iters 20] [--warmup 5]

Shapes: b256.conv1 (x [8,128,256,256], w [128,128,3,3]), b256.conv0 (256 -> 128, up 2, x at 128^2) and one small-grid layer (512 -> 512 at
16^2).  Prints one JSON line per (shape, quantity): milliseconds (median of --iters, device events) of this package and of torch, and the
fraction of the fp32-MFMA peak (MI355X: 157.3 TFLOP/s dense fp32 matrix) that the algorithmic FLOPs of the convolution reach.  No ratio
is asserted anywhere.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import ops  # noqa: E402

PEAK_F32_MFMA = 157.3e12
SHAPES = [
    ('b256.conv1', (8, 128, 256, 256), 128, 3, 1),
    ('b256.conv0_up2', (8, 256, 128, 128), 128, 3, 2),
    ('b16.conv1', (8, 512, 16, 16), 512, 3, 1),
]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def torch_resample(x, w, f, up):
    """What the reference runs for these layers: conv2d, or conv_transpose2d + the filter pass (timed here without the filter, the
    contraction alone, so that the comparison is kernel against kernel)."""
    if up == 1:
        return torch.nn.functional.conv2d(x, w, padding=1)
    return torch.nn.functional.conv_transpose2d(x, w.transpose(0, 1), stride=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    f = ops.setup_filter([1, 3, 3, 1])
    for name, xs, cout, k, up in SHAPES:
        x = torch.randn(xs, generator=gen).to(dev).requires_grad_(True)
        w = torch.randn([cout, xs[1], k, k], generator=gen).to(dev).requires_grad_(True)
        flops = 2.0 * xs[0] * xs[1] * cout * k * k * xs[2] * xs[3]      # (up 2: the transposed conv does the MACs of the small grid)

        def ours_conv(x, w):
            if up == 1:
                return ops.conv2d(x, w, padding=1)
            return ops.conv_transpose2d(x, w.transpose(0, 1), stride=2)

        for who, fwd in (('hip', ours_conv), ('torch', lambda x, w: torch_resample(x, w, f, up))):
            # (one gradient at a time: only the tensor asked for requires grad, so that a backward runs that contraction alone)
            xd, wd = x.detach(), w.detach()
            y_x, y_w = fwd(x, wd), fwd(xd, w)
            dy = torch.randn_like(y_x)
            res = {
                'fwd': timed(lambda: fwd(xd, wd), args.iters, args.warmup),
                'dgrad': timed(lambda: torch.autograd.grad(y_x, [x], dy, retain_graph=True), args.iters, args.warmup),
                'wgrad': timed(lambda: torch.autograd.grad(y_w, [w], dy, retain_graph=True), args.iters, args.warmup),
            }
            for q, ms in res.items():
                print(json.dumps({'shape': name, 'impl': who, 'what': q, 'ms': round(ms, 4), 'peak_frac_f32_mfma': round(flops / (ms * 1e-3) / PEAK_F32_MFMA, 4)}))
            del y_x, y_w, dy
        # the whole op with its filter pass, forward and both gradients
        yy = ops.conv2d_resample(x, w, f=f, up=up, padding=1, flip_weight=(up == 1))
        dyy = torch.randn_like(yy)
        print(json.dumps({'shape': name, 'impl': 'hip', 'what': 'conv2d_resample fwd', 'ms': round(timed(lambda: ops.conv2d_resample(
            x, w, f=f, up=up, padding=1, flip_weight=(up == 1)), args.iters, args.warmup), 4)}))
        print(json.dumps({'shape': name, 'impl': 'hip', 'what': 'conv2d_resample gx+gw', 'ms': round(timed(lambda: torch.autograd.grad(
            yy, [x, w], dyy, retain_graph=True), args.iters, args.warmup), 4)}))
        del yy, dyy, x, w
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
