"""Benchmark of the fused LPIPS pair distance (la_feat_pair_distance) beside the route that existed before it: la_feat_forward of both
batches, then subtract, square and sum the two feature matrices with torch -- same GPU, same process, same engine.

  python scripts/bench_lpips.py [--iters 20] [--warmup 3] [--precision f16x2] [--taps 5|3]

Workloads: full-width VGG16 (random weights, synthetic.make_vgg16_lpips_ops) on
  frames   [8, 2, 256, 256] image pairs as the paired metrics feed them: 16 rows of [3, 256, 256] per side, one pair call of 16 pairs
  crops    the criterion's 64 x 64 crops, the same 16 rows per side
Forms, each one call on resident inputs (outputs and workspaces allocated before any timed window):
  fused    la_feat_pair_distance on the 32-row batch: the trunk once, one pair launch per tap, the finish launch; writes [16, ntaps] float64
  route    la_feat_forward of x and of y (two trunk passes of 16 rows, the taps write 2 x 16 x F floats), then
           (fx - fy).square().sum(1) (reads them back)
  trunk2   la_feat_forward of x and of y alone (what `route` spends before it subtracts)
Timed with device events around one call, after --warmup untimed rounds; the forms alternate inside a round; the median of --iters
rounds is reported, with minimum and maximum.  Bytes: what the tap stage of each form writes and reads beyond the trunk's
activations (fused: the float64 partials and the result; route: the two feature matrices, written once and read once -- a lower
bound, torch's temporaries for the difference and its square come on top).
Prints ONE JSON line.  No ratio is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, synthetic  # noqa: E402
from latentaugment_amd.synthesis import FeatureEngine  # noqa: E402


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--taps', type=int, default=5, choices=(3, 5))
    ap.add_argument('--rows', type=int, default=16, help='images per side (8 pairs of 2 channels)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lpips.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    ops = synthetic.make_vgg16_lpips_ops(seed=7)
    if args.taps == 3:          # the reference's target_layers [16, 23, 30]: drop the first two taps
        seen, kept = 0, []
        for op in ops:
            if op[0] == 'tap':
                seen += 1
                if seen <= 2:
                    continue
            kept.append(op)
        ops = kept
    P = args.rows
    out = {'precision': args.precision, 'taps': args.taps, 'pairs': P}
    stream = torch.cuda.current_stream()
    for name, R in (('frames', 256), ('crops', 64)):
        eng = FeatureEngine(ops, dev, in_res=R, max_batch=2 * P, precision=args.precision)
        g = torch.Generator(device=dev).manual_seed(R)
        x = (torch.rand([P, 1, R, R], generator=g, device=dev) * 2 - 1).repeat(1, 3, 1, 1).contiguous()
        y = (x + 0.05 * (torch.rand([P, 3, R, R], generator=g, device=dev) * 2 - 1)).contiguous()
        xy = torch.cat([x, y]).contiguous()
        dist = torch.empty([P, eng.num_taps], dtype=torch.float64, device=dev)
        fx = torch.empty([P, eng.num_features], dtype=torch.float32, device=dev)
        fy = torch.empty_like(fx)
        eng.pair_distance_rows(xy, P, dist)          # (allocates the partials once)
        ws_bytes = int(lib.la_feat_pair_workspace_bytes(eng.handle, P))

        def fused():
            eng.pair_distance_rows(xy, P, dist)

        def trunk2():
            _lib.check(lib.la_feat_forward(eng.handle, _lib.ptr(x), P, _lib.ptr(fx), _lib.stream_ptr()), 'la_feat_forward')
            _lib.check(lib.la_feat_forward(eng.handle, _lib.ptr(y), P, _lib.ptr(fy), _lib.stream_ptr()), 'la_feat_forward')

        res = {}

        def route():
            trunk2()
            res['d'] = (fx - fy).square().sum(1)
        forms = {'fused': fused, 'route': route, 'trunk2': trunk2}
        for _ in range(args.warmup):
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.iters):
            for k, f in forms.items():
                times[k].append(timed(f, stream))
        route()
        fused()
        torch.cuda.synchronize()
        a, b = dist.sum(1).cpu().numpy(), res['d'].double().cpu().numpy()
        F = eng.num_features
        out[name] = {
            'res': R, 'num_features': F,
            **{k + '_ms': {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()},
            'fused_tap_bytes': ws_bytes * 2 + P * eng.num_taps * 8,                    # partials written and read, result written
            'route_tap_bytes': 2 * P * F * 4 * 2,          # the two feature matrices written, then read (torch's temporaries not counted)
            'largest_relative_difference': float(np.abs(a - b).max() / np.abs(b).max()),
        }
        del eng
    print(json.dumps(out))


if __name__ == '__main__':
    main()
