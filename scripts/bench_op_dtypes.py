"""Time the op layer's bias_act and upsample2d / downsample2d / filter2d in float16, float32 and float64 at [8,128,256,256].

    python scripts/bench_op_dtypes.py [--reps 20] [--warmup 5]

Prints one JSON line.  Per op and dtype: the median time of one call (a HIP event pair around each of `reps` calls, after `warmup`
calls), the effective GB/s under the byte model below and its share of the measured HBM copy rate.  bias_act is lrelu with a bias and
clamp 256 (an SG2 conv layer's epilogue); the resamplers take setup_filter([1,3,3,1]).
Byte model (what an ideal kernel must move): x read once + y written once (bias_act: + the bias, negligible).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentaugment_amd import ops  # noqa: E402

HBM_COPY_GBS = 6290.0      # measured device-to-device copy rate of the MI355X (GB/s), as scripts/bench_filtered_lrelu.py
SHAPE = [8, 128, 256, 256]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for t0, t1 in ev:
        t0.record()
        fn()
        t1.record()
    torch.cuda.synchronize()
    return statistics.median(t0.elapsed_time(t1) * 1e3 for t0, t1 in ev)      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    x32 = torch.randn(SHAPE, device=dev, generator=gen) * 100
    b32 = torch.randn([SHAPE[1]], device=dev, generator=gen)
    f = ops.setup_filter([1, 3, 3, 1])
    ops_ = {
        'bias_act': lambda x, b: ops.bias_act(x, b, act='lrelu', clamp=256),
        'upsample2d': lambda x, b: ops.upsample2d(x, f),
        'downsample2d': lambda x, b: ops.downsample2d(x, f),
        'filter2d': lambda x, b: ops.filter2d(x, f),
    }
    results = {}
    for name, fn in ops_.items():
        row = {}
        for dt, tag in ((torch.float16, 'f16'), (torch.float32, 'f32'), (torch.float64, 'f64')):
            x, b = x32.to(dt), b32.to(dt)
            y = fn(x, b)
            assert y.dtype == dt
            nbytes = (x.numel() + y.numel()) * x.element_size()
            del y
            us = timed(lambda: fn(x, b), args.reps, args.warmup)
            row[tag] = dict(us=round(us, 1), gbs=round(nbytes / us / 1e3, 1), hbm_share=round(nbytes / us / 1e3 / HBM_COPY_GBS, 3))
            del x, b
            torch.cuda.empty_cache()
        row['f16_over_f32'] = round(row['f16']['us'] / row['f32']['us'], 2)
        results[name] = row
    print(json.dumps(dict(bench='op_dtypes', device=torch.cuda.get_device_name(0), shape=SHAPE, reps=args.reps, warmup=args.warmup,
                          hbm_copy_gbs=HBM_COPY_GBS, ops=results)))


if __name__ == '__main__':
    main()
