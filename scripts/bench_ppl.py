"""Benchmark of metrics.compute_ppl beside the same quantity composed from the calls that existed before it -- same GPU, same process,
same engines.

  python scripts/bench_ppl.py [--samples 32] [--batch 8] [--iters 5] [--warmup 1] [--precision f16x2] [--res 256] [--space w|z]

Workload: the config-f generator at --res (random weights, synthetic.make_generator_state_dict, 8 mapping layers) and the full-width
VGG16 with five taps (synthetic.make_vgg16_lpips_ops) at the image resolution; --samples paths in chunks of --batch.
Forms, each one whole evaluation of --samples samples from the same draws (engines and their workspaces built before any timed window):
  ppl        metrics.compute_ppl: mapping of both ends, la_path_points_f32, ONE synthesis batch of 2 n rows per chunk, the crop / repeat
             launch on the batch as it lies, one pair-distance call
  composed   per chunk: MappingEngine.forward of both ends, torch.lerp at t and at t + epsilon (float32), TWO SynthesisEngine.forward
             calls of n rows, metrics.compute_lpips of the two batches (W space only: the calls of before have no slerp)
Both end with the copy of the distances to the host, so wall-clock time around a form is the whole cost; the forms alternate inside a
round; the median of --iters rounds is reported with minimum and maximum, in ms per sample.
Prints ONE JSON line.  No ratio is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import metrics, synthetic  # noqa: E402
from latentaugment_amd.synthesis import FeatureEngine, MappingEngine, SynthesisEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--batch', type=int, default=8, help='samples per chunk (2 x batch rows per synthesis call)')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--channel-base', type=int, default=32768, help='32768 = config-f')
    ap.add_argument('--space', default='w', choices=('w', 'z'))
    ap.add_argument('--epsilon', type=float, default=1e-4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ppl.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    N, n, eps = args.samples, args.batch, args.epsilon
    sd, meta = synthetic.make_generator_state_dict(img_resolution=args.res, img_channels=2, channel_base=args.channel_base, seed=0)
    mapping = MappingEngine(sd, dev)
    synth = SynthesisEngine.from_generator(sd, dev, max_batch=2 * n, precision=args.precision)
    net = FeatureEngine(synthetic.make_vgg16_lpips_ops(seed=7), dev, in_res=args.res, max_batch=2 * n * meta['img_channels'],
                        precision=args.precision)

    def ppl():
        return metrics.compute_ppl(mapping, synth, net, N, epsilon=eps, space=args.space, seed=0, batch=n)['dist']

    def composed():
        g = torch.Generator().manual_seed(0)
        z = torch.randn([2 * N, mapping.z_dim], generator=g)
        t = torch.rand([N], generator=g)
        z0, z1, t = z[:N].to(dev), z[N:].to(dev), t.to(dev)
        parts = []
        for p0 in range(0, N, n):
            w = mapping.forward(torch.cat([z0[p0:p0 + n], z1[p0:p0 + n]]), 1)
            m = w.shape[0] // 2
            tt = t[p0:p0 + n].reshape(-1, 1, 1)
            img0 = synth.forward(torch.lerp(w[:m], w[m:], tt))
            img1 = synth.forward(torch.lerp(w[:m], w[m:], tt + eps))
            parts.append(metrics.compute_lpips(img0, img1, net)['lpips'])
        return torch.cat(parts) / (eps * eps)
    forms = {'ppl': ppl} if args.space == 'z' else {'ppl': ppl, 'composed': composed}
    last = {}
    for _ in range(args.warmup):
        for k, f in forms.items():
            last[k] = f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.iters):
        for k, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / N)
    out = {'res': args.res, 'channel_base': args.channel_base, 'precision': args.precision, 'space': args.space, 'samples': N, 'batch': n,
           'epsilon': eps,
           **{k + '_ms_per_sample': {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
              for k, v in times.items()},
           'ppl': metrics.ppl_from_distances(last['ppl'])}
    if 'composed' in last:
        # the composed form makes t + epsilon in float32: its distances carry that error, this is not a correctness check
        out['composed_ppl'] = metrics.ppl_from_distances(last['composed'])
        out['largest_relative_difference'] = float(((last['ppl'] - last['composed']).abs() / last['ppl'].abs()).max())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
