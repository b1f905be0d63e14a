"""Benchmark of the fused LPIPS pair distance (la_feat_pair_distance) beside the route that existed before it: la_feat_forward of both
batches, then subtract, square and sum the two feature matrices with torch -- same GPU, same process, same engine.

  python scripts/bench_lpips.py [--iters 20] [--warmup 3] [--precision f16x2] [--taps 5|3] [--net vgg|alex|squeeze]

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

--net alex | squeeze (the default, vgg, is everything above, unchanged): the full-width AlexNet / SqueezeNet 1.1 LPIPS net with seeded random
weights (synthetic.make_lpips_net_state_dicts; no file is downloaded) on the frames workload, 16 pairs of [3, 256, 256]:
  fused    la_feat_pair_distance, as above (these trunks compute in exact fp32 whatever --precision says)
  torch    the same net composed from torch's eager float32 ops on the same GPU in the same process (conv2d, relu, max_pool2d, cat, the
           normalisation and the weighted squared difference), measured twice (torch_a, torch_b: their spread is the margin of the
           comparison)
Medians over --iters timed calls (at least 20) after --warmup rounds, the forms alternating inside a round.
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


def bench_net(args, dev):
    """--net alex | squeeze: ms per pair_distance call beside the torch composition of the same net."""
    import torch.nn.functional as F
    from latentaugment_amd.synthesis import lpips_reference_net
    desc = lpips_reference_net(*synthetic.make_lpips_net_state_dicts(args.net, seed=7), args.net)
    P, R = args.rows, 256
    eng = FeatureEngine.from_net(desc, dev, in_res=R, max_batch=2 * P, precision=args.precision)
    g = torch.Generator(device=dev).manual_seed(R)
    x = (torch.rand([P, 1, R, R], generator=g, device=dev) * 2 - 1).repeat(1, 3, 1, 1).contiguous()
    y = (x + 0.05 * (torch.rand([P, 3, R, R], generator=g, device=dev) * 2 - 1)).contiguous()
    xy = torch.cat([x, y]).contiguous()
    dist = torch.empty([P, eng.num_taps], dtype=torch.float64, device=dev)
    eng.pair_distance_rows(xy, P, dist)          # (allocates the partials once)
    ops = [(op[0],) + tuple(t.to(dev) if torch.is_tensor(t) else t for t in op[1:]) for op in desc.ops]
    res = {}

    def composed():
        t, cols = xy, []
        for op in ops:
            if op[0] == 'conv':
                t = F.relu(F.conv2d(t, op[1], op[2], stride=op[3], padding=op[4]))
            elif op[0] == 'maxpool3':
                t = F.max_pool2d(t, 3, 2, ceil_mode=bool(op[1]))
            elif op[0] == 'fire':
                s = F.relu(F.conv2d(t, op[1], op[2]))
                t = torch.cat([F.relu(F.conv2d(s, op[3], op[4])), F.relu(F.conv2d(s, op[5], op[6], padding=1))], 1)
            else:
                n = t * torch.rsqrt(t.square().sum(1, keepdim=True) + 1e-10)
                cols.append(((n[:P] - n[P:]).square() * op[1].reshape(1, -1, 1, 1)).sum(1).mean((1, 2)))
        res['d'] = torch.stack(cols, dim=1)
    forms = {'fused': lambda: eng.pair_distance_rows(xy, P, dist), 'torch_a': composed, 'torch_b': composed}
    stream = torch.cuda.current_stream()
    with torch.no_grad():
        for _ in range(args.warmup):
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(max(args.iters, 20)):
            for k, f in forms.items():
                times[k].append(timed(f, stream))
    torch.cuda.synchronize()
    a, b = dist.cpu().numpy(), res['d'].double().cpu().numpy()
    print(json.dumps({'net': args.net, 'precision': args.precision, 'pairs': P, 'res': R, 'taps': eng.num_taps,
                      **{k + '_ms': {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()},
                      'largest_relative_difference': float(np.abs(a - b).max() / np.abs(b).max())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--taps', type=int, default=5, choices=(3, 5))
    ap.add_argument('--rows', type=int, default=16, help='images per side (8 pairs of 2 channels)')
    ap.add_argument('--net', default='vgg', choices=('vgg', 'alex', 'squeeze'), help='alex | squeeze: that trunk beside its torch composition')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lpips.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    if args.net != 'vgg':
        return bench_net(args, dev)
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
