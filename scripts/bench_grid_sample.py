"""Micro-benchmark of ops.grid_sample: forward and backward (dx and dgrid in one launch) at [8,2,256,256] and [8,128,256,256] under a
small random affine warp, beside torch.nn.functional.grid_sample (and its autograd) on the same device.

  python scripts/bench_grid_sample.py [--iters 20] [--warmup 5] [--dtype float32]

Prints one JSON line per (shape, implementation): milliseconds (median of --iters, device events) and the achieved GB/s of algorithmic
traffic -- forward: x and the grid read once, y written once; backward: dy, x and the grid read once, dx and dgrid written once (the
zeroing of dx and the atomic read-modify-writes are not counted: they are the implementation's, not the algorithm's).  The backward line
also gives the bytes the dx scatter adds atomically (4 corners x 4 bytes per output and channel) and the time that alone takes at the
chip-wide float-atomic rate of 1.3 TB/s.  A report: no ratio is asserted anywhere.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import ops  # noqa: E402

SHAPES = [(8, 2, 256, 256), (8, 128, 256, 256)]
ATOMIC_RATE = 1.3e12


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


def torch_grid_sample(x, grid):
    return torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtype', default='float32', choices=['float16', 'float32', 'float64'])
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    dt = getattr(torch, args.dtype)
    gen = torch.Generator().manual_seed(0)
    for n, c, h, w in SHAPES:
        # a rotation of up to +-5 degrees, a scale within 5 % and a shift of up to 2 % of the image, one per sample
        ang = (torch.rand([n], generator=gen) - 0.5) * (10 * math.pi / 180)
        sc = 1 + (torch.rand([n], generator=gen) - 0.5) * 0.1
        theta = torch.zeros([n, 2, 3])
        theta[:, 0, 0], theta[:, 0, 1], theta[:, 1, 0], theta[:, 1, 1] = sc * ang.cos(), -sc * ang.sin(), sc * ang.sin(), sc * ang.cos()
        theta[:, :, 2] = (torch.rand([n, 2], generator=gen) - 0.5) * 0.04
        grid = torch.nn.functional.affine_grid(theta, [n, c, h, w], align_corners=False).to(dev, dt).requires_grad_(True)
        x = torch.randn([n, c, h, w], generator=gen).to(dev, dt).requires_grad_(True)
        es = x.element_size()
        fwd_bytes = (2 * x.numel() + grid.numel()) * es
        bwd_bytes = (3 * x.numel() + 2 * grid.numel()) * es
        atomic_bytes = 16 * x.numel()
        for who, fn in (('hip', ops.grid_sample), ('torch', torch_grid_sample)):
            y = fn(x, grid)
            dy = torch.randn_like(y)
            xd, gd = x.detach(), grid.detach()
            f_ms = timed(lambda: fn(xd, gd), args.iters, args.warmup)
            b_ms = timed(lambda: torch.autograd.grad(y, [x, grid], dy, retain_graph=True), args.iters, args.warmup)
            print(json.dumps({'shape': [n, c, h, w], 'dtype': args.dtype, 'impl': who,
                              'fwd_ms': round(f_ms, 4), 'fwd_GBps': round(fwd_bytes / f_ms / 1e6, 1),
                              'bwd_ms': round(b_ms, 4), 'bwd_GBps': round(bwd_bytes / b_ms / 1e6, 1),
                              'dx_atomic_MB': round(atomic_bytes / 1e6, 1), 'dx_atomic_floor_ms': round(atomic_bytes / ATOMIC_RATE * 1e3, 4)}))
            del y, dy
        del x, grid
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
