"""Benchmark of metrics.compute_kid_from_features (la_kid_poly3_f32) beside the same computation composed from torch.matmul on the same
GPU in the same process.

  python scripts/bench_kid.py [--iters 10] [--warmup 3] [--sizes 1572,50000] [--dim 2048]

The default recipe (num_subsets=100, max_subset_size=1000, seed=0) at N = 1572 (the Pelvis-scale bank) and N = 50 000 rows per side,
D = 2048, features resident on the device for both forms, the same index arrays.  A call is timed with a host clock from its start to
the Python float it returns (which ends in a device-to-host copy, so the device work is complete); the two forms alternate inside
every iteration; the median is reported.
  hip          compute_kid_from_features: rows gathered by the kernel, the kernel matrices stay in registers
  torch_loop   per subset: gather, three fp32 matmuls, (g / D + 1) ** 3, float64 sums, the diagonals subtracted
  torch_bmm    the same with one gather and three torch.bmm over all subsets at once ([S, m, m] kernel matrices in memory)
Prints one JSON line per (N, form): milliseconds, the KID value, and for `hip` the fraction of the 157.3 TFLOP/s fp32-MFMA peak that
the FLOPs of the tiles it computes reach (2 D per kernel value; upper triangles only for xx and yy).  No ratio is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import metrics  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def torch_loop(real, gen, ix, iy):
    D = real.shape[1]
    tot = torch.zeros([], dtype=torch.float64, device=real.device)
    for s in range(ix.shape[0]):
        x, y = gen[ix[s]], real[iy[s]]
        mx, my = x.shape[0], y.shape[0]
        kxx, kyy, kxy = ((x @ x.T) / D + 1) ** 3, ((y @ y.T) / D + 1) ** 3, ((x @ y.T) / D + 1) ** 3
        sxx = kxx.sum(dtype=torch.float64) - kxx.diagonal().sum(dtype=torch.float64)
        syy = kyy.sum(dtype=torch.float64) - kyy.diagonal().sum(dtype=torch.float64)
        tot += sxx / (mx * (mx - 1)) + syy / (my * (my - 1)) - 2 * kxy.sum(dtype=torch.float64) / (mx * my)
    return float(tot / ix.shape[0])


def torch_bmm(real, gen, ix, iy):
    D = real.shape[1]
    x, y = gen[ix], real[iy]                                   # [S, m, D]
    mx, my = x.shape[1], y.shape[1]
    k = lambda a, b: (torch.bmm(a, b.transpose(1, 2)) / D + 1) ** 3      # noqa: E731
    off = lambda g: g.sum(dim=(1, 2), dtype=torch.float64) - g.diagonal(dim1=1, dim2=2).sum(dim=1, dtype=torch.float64)      # noqa: E731
    mmd2 = off(k(x, x)) / (mx * (mx - 1)) + off(k(y, y)) / (my * (my - 1)) - 2 * k(x, y).sum(dim=(1, 2), dtype=torch.float64) / (mx * my)
    return float(mmd2.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', default='1572,50000')
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--num-subsets', type=int, default=100)
    ap.add_argument('--max-subset-size', type=int, default=1000)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    for n in (int(v) for v in args.sizes.split(',')):
        g = torch.Generator(device=dev).manual_seed(n)
        # non-negative, mean 0.5, as pooled detector features; the generated side 5 % larger
        real = torch.rand([n, args.dim], generator=g, device=dev) ** 2 * 1.5
        gen = torch.rand([n, args.dim], generator=g, device=dev) ** 2 * 1.575
        ix, iy = metrics.kid_subset_indices(n, n, args.num_subsets, args.max_subset_size, 0)
        S, m = ix.shape
        tiles = (m + 127) // 128
        flops = 2.0 * args.dim * S * 128 * 128 * (tiles * (tiles + 1) + tiles * tiles)
        forms = {
            'hip': lambda: metrics.compute_kid_from_features(real, gen, device=dev, indices=(ix, iy)),
            'torch_loop': lambda: torch_loop(real, gen, torch.from_numpy(ix).to(dev).long(), torch.from_numpy(iy).to(dev).long()),
            'torch_bmm': lambda: torch_bmm(real, gen, torch.from_numpy(ix).to(dev).long(), torch.from_numpy(iy).to(dev).long()),
        }
        times, vals = {k: [] for k in forms}, {}
        for it in range(args.warmup + args.iters):
            for name, fn in forms.items():          # alternating: drift of the shared machine hits all forms alike
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                vals[name] = fn()
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    times[name].append(dt * 1e3)
        for name in forms:
            ts = sorted(times[name])
            row = {'N': n, 'D': args.dim, 'S': S, 'm': m, 'form': name, 'ms_median': round(ts[len(ts) // 2], 3), 'ms_min': round(ts[0], 3),
                   'ms_max': round(ts[-1], 3), 'kid': vals[name], 'rel_diff_to_hip': abs(vals[name] - vals['hip']) / max(abs(vals['hip']), 1e-30)}
            if name == 'hip':
                row['peak_frac_f32_mfma'] = round(flops / (row['ms_median'] * 1e-3) / PEAK_F32_MFMA, 4)
            print(json.dumps(row), flush=True)
        del real, gen
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
