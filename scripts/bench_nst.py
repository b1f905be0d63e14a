"""Benchmark of the Gram-matrix style / content distance (metrics.compute_style_content, la_gram_pair_dist_f32) beside the same
quantities from torch's eager ops on the same GPU in the same process.

  python scripts/bench_nst.py [--iters 10] [--warmup 3] [--pairs 8] [--res 256] [--precision f32]

Workload: full-width VGG19 (64, 128, 256, 512, 512; taps relu1_1 .. relu5_1) with seeded He-scaled weights, `--pairs` pairs of
two-channel `--res`^2 images in [-1, 1]: 2 * pairs rows of both images of a pair per call, i.e. 4 * pairs rows through the trunk.
Every form is timed with device events around one call on the current stream (the call's host work included), after `--warmup` untimed
rounds of every form; the forms alternate inside every round; the median of `--iters` rounds is reported.
  hip_call        metrics.compute_style_content: crop + repeat, trunk, Gram and content step per tap, the copy of the results to the host
  torch_call      the same quantities from eager torch: clamp, affine, repeat, conv2d / relu / max_pool2d, per tap bmm Grams and mse
  hip_tap[k]      la_gram_pair_dist_f32 alone on the activations of tap k (style and content of 2 * pairs row pairs)
  torch_tap[k]    the bmm Grams and the two mse of the same activations
Prints ONE JSON line: milliseconds (median, minimum, maximum) per form; per tap C, HW, the K slices, the workgroups of the tile launch,
the rate of the MFMA work the tile launch issues (tiles x edge^2 x 2 chains x 2 HW FLOP, edge = 64 for C <= 64, else 128) over the
whole entry's time, as a fraction of the 157.3 TFLOP/s fp32 MFMA peak, and the rate of its compulsory HBM traffic (both images read
once by the tile launch and once by the content sum) as a fraction of 8 TB/s; the largest relative difference of the two forms' results.  No time is asserted.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, metrics, synthesis  # noqa: E402

WIDTHS, BLOCKS = (64, 128, 256, 512, 512), (2, 2, 4, 4, 4)
CONV_IDS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
TAP_AFTER, POOL_AFTER = (0, 5, 10, 19, 28), (2, 7, 16, 25)
MFMA_F32_PEAK, HBM_PEAK = 157.3e12, 8.0e12


def seeded_vgg19(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd, c, i = {}, 3, 0
    for width, n in zip(WIDTHS, BLOCKS):
        for _ in range(n):
            sd[f'features.{i}.weight'] = torch.randn([width, c, 3, 3], generator=g) * (2.0 / (9 * c)) ** 0.5
            sd[f'features.{i}.bias'] = torch.rand([width], generator=g) * 0.1
            c, i = width, i + 2
        i += 1
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--precision', default='f32', choices=sorted(synthesis.PRECISIONS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_nst.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr
    P, R = args.pairs, args.res
    sd = seeded_vgg19()
    eng = synthesis.FeatureEngine.from_net(synthesis.nst_reference_net(sd), dev, in_res=R, max_batch=4 * P, precision=args.precision)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand([P, 2, R, R], generator=g) * 2 - 1).to(dev)
    y = (x + 0.2 * (torch.rand([P, 2, R, R], generator=g) * 2 - 1).to(dev)).clamp(-1, 1)
    wd = {k: v.to(dev) for k, v in sd.items()}
    out = {}

    def torch_taps(img):
        h = (img.clamp(-128.0 / 127.5, 127.0 / 127.5) * 0.5 + 128.0 / 255.0).permute(1, 0, 2, 3).reshape(2 * P, 1, R, R).repeat(1, 3, 1, 1)
        taps = []
        for i in CONV_IDS:
            h = torch.relu(F.conv2d(h, wd[f'features.{i}.weight'], wd[f'features.{i}.bias'], padding=1))
            if i in TAP_AFTER:
                taps.append(h.reshape(h.shape[0], h.shape[1], -1))
            if i in POOL_AFTER:
                h = F.max_pool2d(h, 2)
        return taps

    def torch_tap(f1, f2):
        hw = f1.shape[2]
        g1, g2 = torch.bmm(f1, f1.transpose(1, 2)) / hw, torch.bmm(f2, f2.transpose(1, 2)) / hw
        return (g1 - g2).square().mean(dim=(1, 2)), (f1 - f2).square().mean(dim=(1, 2))

    def hip_call():
        out['hip'] = metrics.compute_style_content(x, y, eng)

    def torch_call():
        with torch.no_grad():
            tx, ty = torch_taps(x), torch_taps(y)
            res = [torch_tap(a, b) for a, b in zip(tx, ty)]
            out['torch'] = (torch.stack([r[0] for r in res], 1).cpu(), torch.stack([r[1] for r in res], 1).cpu())

    forms = {'hip_call': hip_call, 'torch_call': torch_call}
    # per tap: the activations of the torch trunk, both images of a pair in one [2 * rows] batch as the entry takes them
    with torch.no_grad():
        acts = [torch.cat([a, b]).contiguous() for a, b in zip(torch_taps(x), torch_taps(y))]
    tap_info = []
    for k, f in enumerate(acts):
        rows, C, HW = f.shape[0] // 2, f.shape[1], f.shape[2]
        nbytes = lib.la_gram_pair_scratch_bytes(rows, C, HW)
        ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
        s, c = torch.empty([rows], dtype=torch.float64, device=dev), torch.empty([rows], dtype=torch.float64, device=dev)

        def hip_tap(f=f, rows=rows, C=C, HW=HW, ws=ws, nbytes=nbytes, s=s, c=c):
            _lib.check(lib.la_gram_pair_dist_f32(p(f), rows, C, HW, p(s), p(c), p(ws), nbytes, st()), 'gram')

        def torch_tap_k(f=f, rows=rows, k=k):
            with torch.no_grad():
                out[f'torch_tap{k}'] = torch_tap(f[:rows], f[rows:])
        forms[f'hip_tap{k}'], forms[f'torch_tap{k}'] = hip_tap, torch_tap_k
        edge = 64 if C <= 64 else 128          # the tile edge of la_gram.hip
        T = -(-C // edge)
        tap_info.append(dict(C=C, HW=HW, rows=rows, slices=lib.la_gram_pair_slices(C, HW), ntile=T * (T + 1) // 2, edge=edge, s=s, c=c))
    times = {name: [] for name in forms}
    for it in range(args.warmup + args.iters):
        for name, fn in forms.items():          # alternating: drift of a shared machine hits all forms alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    result = {'bench': 'nst', 'pairs': P, 'res': R, 'precision': args.precision, 'iters': args.iters, 'device': torch.cuda.get_device_name(0),
              'forms': {}, 'taps': []}
    for name in forms:
        ts = sorted(times[name])
        result['forms'][name] = {'ms_median': round(ts[len(ts) // 2], 4), 'ms_min': round(ts[0], 4), 'ms_max': round(ts[-1], 4)}
    result['torch_call_over_hip_call'] = round(result['forms']['torch_call']['ms_median'] / result['forms']['hip_call']['ms_median'], 3)
    for k, t in enumerate(tap_info):
        sec = result['forms'][f'hip_tap{k}']['ms_median'] * 1e-3
        issued = t['rows'] * t['ntile'] * float(t['edge']) ** 2 * 2 * 2 * t['HW']
        traffic = 2.0 * (2 * t['rows']) * t['C'] * t['HW'] * 4
        ts_, tc_ = out[f'torch_tap{k}']
        result['taps'].append({
            'C': t['C'], 'HW': t['HW'], 'row_pairs': t['rows'], 'slices': t['slices'], 'tile_workgroups': t['rows'] * t['ntile'] * t['slices'],
            'mfma_issued_fraction_of_peak': round(issued / sec / MFMA_F32_PEAK, 4), 'hbm_fraction_of_peak': round(traffic / sec / HBM_PEAK, 4),
            'torch_tap_over_hip_tap': round(result['forms'][f'torch_tap{k}']['ms_median'] / result['forms'][f'hip_tap{k}']['ms_median'], 3),
            'style_rel_diff_vs_torch': float(((t['s'] - ts_.double()).abs() / ts_.double().abs().clamp_min(1e-300)).max()),
            'content_rel_diff_vs_torch': float(((t['c'] - tc_.double()).abs() / tc_.double().abs().clamp_min(1e-300)).max())})
    hs, hc = out['hip']['style_layers'], out['hip']['content_layers']          # [P, 2, 5]; the torch rows are c * P + b
    ts_, tc_ = (v.double().reshape(2, P, 5).permute(1, 0, 2) for v in out['torch'])
    result['call_style_rel_diff_vs_torch'] = float(((hs - ts_).abs() / ts_.abs().clamp_min(1e-300)).max())
    result['call_content_rel_diff_vs_torch'] = float(((hc - tc_).abs() / tc_.abs().clamp_min(1e-300)).max())
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
