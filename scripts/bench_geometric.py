"""Micro-benchmark of the GeometricAugment pipeline: [8,2,256,256], flip + affine + elastic on every sample, our four launches
(latentaugment_amd.geometric) beside the same pipeline composed from torch's own affine_grid / grid_sample / conv2d on the same device.

  python scripts/bench_geometric.py [--iters 500] [--warmup 20] [--rounds 5]

The two implementations alternate in one process, --rounds times; each round times --iters batches per implementation with device events
after --warmup untimed ones.  Prints one JSON line per implementation: the median over the rounds of ms per batch (and the spread of the
rounds), and the achieved GB/s of algorithmic traffic -- each image once in and once out per resampling (two resamplings), the noise
written once and read once, the field written once and read once: 6 x B x 2 x H x W x 4 bytes.  The parameter draw and the inverse maps
are made once, outside the timed region, for both.  A report: no ratio is asserted anywhere.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import geometric  # noqa: E402

B, C, H, W = 8, 2, 256, 256


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn([B, C, H, W], generator=gen).to(dev)
    params = geometric.draw_params(gen, B, H, W, 1.0)
    minv = geometric.affine_inverse(params, H, W).to(dev)
    ones = torch.ones([B], dtype=torch.uint8, device=dev)
    taps = geometric.gaussian_taps(63, 32.0)
    seed = int(params['seed'])

    def ours():
        y = geometric.warp_affine(x, minv, ones)
        noise = geometric.noise_uniform(B, 2 * H * W, seed, device=dev).view(B, 2, H, W)
        return geometric.warp_elastic(y, geometric.elastic_field(noise, taps), ones)

    # torch: the same inverse maps as a normalised theta for affine_grid (align_corners=False), the blur as two 1-D conv2d passes
    m = minv.view(B, 2, 3).double()
    theta = torch.empty([B, 2, 3], dtype=torch.float64, device=dev)
    theta[:, 0, 0], theta[:, 0, 1] = m[:, 0, 0], m[:, 0, 1] * H / W
    theta[:, 1, 0], theta[:, 1, 1] = m[:, 1, 0] * W / H, m[:, 1, 1]
    theta[:, 0, 2] = (2 * m[:, 0, 2] + m[:, 0, 0] * (W - 1) + m[:, 0, 1] * (H - 1) + 1) / W - 1
    theta[:, 1, 2] = (2 * m[:, 1, 2] + m[:, 1, 0] * (W - 1) + m[:, 1, 1] * (H - 1) + 1) / H - 1
    theta = theta.float()
    kx, ky = taps.float().to(dev).view(1, 1, 1, 63), taps.float().to(dev).view(1, 1, 63, 1)
    base = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H, device=dev), torch.linspace(-1, 1, W, device=dev), indexing='ij')[::-1], dim=-1)[None]

    def composed():
        y = F.grid_sample(x, F.affine_grid(theta, [B, C, H, W], align_corners=False), mode='bilinear', padding_mode='reflection', align_corners=False)
        noise = torch.rand([B * 2, 1, H, W], device=dev) * 2 - 1
        d = F.conv2d(F.conv2d(noise, kx, padding=(0, 31)), ky, padding=(31, 0)).view(B, 2, H, W)
        grid = (base + d.permute(0, 2, 3, 1)).clamp(-1, 1)
        return F.grid_sample(y, grid, mode='bilinear', padding_mode='reflection', align_corners=False)

    # the two affine stages agree (same maps, same sampler definition) before anything is timed
    ya = geometric.warp_affine(x, minv, ones)
    yt = F.grid_sample(x, F.affine_grid(theta, [B, C, H, W], align_corners=False), mode='bilinear', padding_mode='reflection', align_corners=False)
    affine_diff = float((ya - yt).abs().max())
    nbytes = 6 * B * 2 * H * W * 4
    runs = {'hip': [], 'torch': []}
    for _ in range(args.rounds):
        runs['hip'].append(timed(ours, args.iters, args.warmup))
        runs['torch'].append(timed(composed, args.iters, args.warmup))
    for who, ts in runs.items():
        ts = sorted(ts)
        ms = ts[len(ts) // 2]
        print(json.dumps({'shape': [B, C, H, W], 'impl': who, 'ms_per_batch': round(ms, 4), 'ms_min': round(ts[0], 4), 'ms_max': round(ts[-1], 4),
                          'GBps': round(nbytes / ms / 1e6, 1), 'rounds': args.rounds, 'iters': args.iters,
                          'affine_stage_max_abs_diff_vs_torch': affine_diff}))


if __name__ == '__main__':
    main()
