"""Benchmark of the detector path (DetectorEngine: la_detector_prep_f32, the 13 convolutions and 5 pools of the feature engine,
la_fc_bias_act_f32 twice) beside the same net composed from torch's own eager ops in float32 on the same GPU in the same process --
what a user who wants detector features of generated images runs today.

  python scripts/bench_detector.py [--iters 10] [--warmup 3] [--batches 64,1] [--width 64] [--precision f16x2]

Full-width VGG16 (width 64: 64 .. 512 channels, fc 25088 -> 4096 -> 4096) with random weights; inputs are [N, 1, 256, 256] images in
[-1, 1], quantised, repeated to three channels and area-resampled to 224 x 224.  Every form is timed with device events around the
calls on the current stream, after `--warmup` untimed rounds of every form at that batch; the forms alternate inside every round; the
median of `--iters` rounds is reported.  Stages of the HIP path (timed on their own, on the tensors the stage in front produced):
  prep     la_detector_prep_f32
  convs    the feature engine on the op list cut before fc1 is not a valid list, so this is total - prep - fc1 - fc2 of the same round
  fc1/fc2  la_fc_bias_act_f32 at [N, 25088] x [4096, 25088] and [N, 4096] x [4096, 4096]; for fc1 the implied weight bytes per
           second (K * O * 4 / time) beside the 8 TB/s HBM peak
  total    DetectorEngine.features
  torch    quantise, repeat, F.interpolate(mode='area'), 13 x (conv2d + relu), 5 x max_pool2d, 2 x (linear + relu), float32 eager
Prints one JSON line per (batch, form) and one line with fc1's N = 64 / N = 1 time ratio: the weights are the same 411 MB at both
batches, so a ratio above 3 would mean they are read more than once.  The outputs of the two paths are compared (relative L2) and
printed, not asserted.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import synthesis  # noqa: E402

CFG = [(1, 2), (2, 2), (4, 3), (8, 3), (8, 3)]


def build_ops(width, size, fc_width, g):
    ops, c = [], 3
    for mult, n in CFG:
        for _ in range(n):
            co = mult * width
            ops.append(('conv', torch.randn([co, c, 3, 3], generator=g) * (2.0 / (c * 9)) ** 0.5, torch.randn([co], generator=g) * 0.05))
            c = co
        ops.append(('maxpool',))
    k = c * (size // 32) ** 2
    for _ in range(2):
        ops.append(('fc', torch.randn([fc_width, k], generator=g) * (2.0 / k) ** 0.5, torch.randn([fc_width], generator=g) * 0.05, True))
        k = fc_width
    return ops


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', default='64,1')
    ap.add_argument('--width', type=int, default=64)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--fc-width', type=int, default=4096)
    ap.add_argument('--in-res', type=int, default=256)
    ap.add_argument('--precision', default='f16x2', choices=sorted(synthesis.PRECISIONS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_detector.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    batches = [int(v) for v in args.batches.split(',')]
    g = torch.Generator().manual_seed(0)
    ops = build_ops(args.width, args.size, args.fc_width, g)
    pre_scale = tuple(1.0 / s for s in (58.395, 57.12, 57.375))
    pre_shift = tuple(-m / s for m, s in zip((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)))
    det = synthesis.DetectorEngine(ops, dev, args.size, max(batches), 'area', pre_scale, pre_shift, precision=args.precision)
    dops = [tuple(t.to(dev) if torch.is_tensor(t) else t for t in op) for op in ops]
    fcs = [op for op in dops if op[0] == 'fc']
    sc, sh = torch.tensor(pre_scale, device=dev).reshape(1, 3, 1, 1), torch.tensor(pre_shift, device=dev).reshape(1, 3, 1, 1)

    def torch_form(img):
        x = (img * 127.5 + 128).clamp(0, 255).to(torch.uint8).repeat(1, 3, 1, 1).to(torch.float32)
        x = F.interpolate(x, size=(args.size, args.size), mode='area') * sc + sh
        for op in dops:
            if op[0] == 'conv':
                x = F.relu(F.conv2d(x, op[1], op[2], padding=1))
            elif op[0] == 'maxpool':
                x = F.max_pool2d(x, 2)
            else:
                x = F.relu(F.linear(x.flatten(1), op[1], op[2]))
        return x

    fc1_ms = {}
    for N in batches:
        img = (torch.rand([N, 1, args.in_res, args.in_res], generator=g) * 2 - 1).to(dev)
        h1 = torch.randn([N, fcs[0][1].shape[1]], generator=g).abs().to(dev)
        h2 = torch.randn([N, fcs[1][1].shape[1]], generator=g).abs().to(dev)
        forms = {'prep': lambda: det.prepare(img), 'fc1': lambda: synthesis.fc_bias_act(h1, fcs[0][1], fcs[0][2], True),
                 'fc2': lambda: synthesis.fc_bias_act(h2, fcs[1][1], fcs[1][2], True), 'total': lambda: det.features(img),
                 'torch': lambda: torch_form(img)}
        times, outs = {k: [] for k in forms}, {}
        for it in range(args.warmup + args.iters):
            for name, fn in forms.items():          # alternating: drift of a shared machine hits all forms alike
                ms, outs[name] = timed(fn)
                if it >= args.warmup:
                    times[name].append(ms)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        med['convs'] = med['total'] - med['prep'] - med['fc1'] - med['fc2']
        fc1_ms[N] = med['fc1']
        rel = float((outs['total'] - outs['torch']).norm() / outs['torch'].norm())
        for name in ('prep', 'convs', 'fc1', 'fc2', 'total', 'torch'):
            row = {'N': N, 'form': name, 'ms_median': round(med[name], 4), 'precision': args.precision}
            if name in times:
                row['ms_min'], row['ms_max'] = round(min(times[name]), 4), round(max(times[name]), 4)
            if name == 'fc1':
                wbytes = fcs[0][1].numel() * 4
                row['weight_TB_per_s'] = round(wbytes / (med['fc1'] * 1e-3) / 1e12, 3)
                row['of_8TB_per_s_peak'] = round(row['weight_TB_per_s'] / 8.0, 3)
            if name == 'total':
                row['images_per_s'] = round(N / (med['total'] * 1e-3), 1)
                row['rel_l2_vs_torch'] = rel
                row['speedup_vs_torch'] = round(med['torch'] / med['total'], 2)
            print(json.dumps(row), flush=True)
    if 64 in fc1_ms and 1 in fc1_ms:
        print(json.dumps({'fc1_ms_N64_over_N1': round(fc1_ms[64] / fc1_ms[1], 3), 'weights_read_once_if_below': 3.0}), flush=True)


if __name__ == '__main__':
    main()
