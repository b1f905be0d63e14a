"""Benchmark of the paired image metrics (la_pair_metrics_f32, la_joint_hist_f32) beside the same quantities composed from torch ops on
the same GPU in the same process.

  python scripts/bench_pair_metrics.py [--iters 20] [--warmup 5] [--calls 50] [--shape 8x2x256x256] [--levels 5] [--bins 64]

Workload: [8, 2, 256, 256] image pairs in [-1, 1] (a -1 background with a textured disc, as a medical slice), 5 pyramid levels with
the 11-tap window, and the 64-bin joint histogram of the two channels of the same batch.  Images, workspaces and outputs are resident
on the device and allocated before any timed window.
  hip_pair     la_pair_metrics_f32: error sums, ssim / cs per level and ms of the 16 planes (5 level launches, finish, combine)
  torch_pair   the same: per level five depthwise conv2d calls per direction (rows, then columns) over mu_x, mu_y, xx, yy, xy, the two
               quotients, their means, avg_pool2d to the next level; the error sums; the product of the levels
  hip_hist     la_joint_hist_f32 (memset + one launch) of channel 0 against channel 1, read in place
  torch_hist   the float32 bin rule with torch ops, a flattened index and index_add_ of ones into a zeroed int32 table
Every form is timed with device events around `--calls` back-to-back calls on the current stream (one call is tens of microseconds:
a window of one call would measure the event pair), after `--warmup` untimed rounds of every form; the forms alternate inside every
round; the median over `--iters` rounds of the per-call time is reported.  Prints ONE JSON line: per form milliseconds per call
(median, minimum, maximum), and how far the torch forms are from the HIP ones (floats: largest difference; counts: cells differing).
No ratio is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, metrics  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50, help='back-to-back calls inside one timed window')
    ap.add_argument('--shape', default='8x2x256x256')
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--win', type=int, default=11)
    ap.add_argument('--bins', type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pair_metrics.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr
    N, C, H, W = (int(v) for v in args.shape.split('x'))
    levels, win, bins = args.levels, args.win, args.bins
    g = torch.Generator(device=dev).manual_seed(N + H)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    disc = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2) <= (0.35 * min(H, W)) ** 2
    tex = 0.2 + 0.5 * (torch.rand([N, C, H, W], generator=g, device=dev) * 2 - 1)
    x = torch.where(disc, tex, torch.full_like(tex, -1.0)).contiguous()
    y = torch.where(disc, tex + 0.1 * (torch.rand([N, C, H, W], generator=g, device=dev) * 2 - 1), torch.full_like(tex, -1.0)).contiguous()

    taps = metrics.gaussian_window(win, 1.5).astype(np.float32)
    wts = metrics.msssim_weights(levels)
    c1, c2 = float(np.float32(0.02 ** 2)), float(np.float32(0.06 ** 2))
    ws_bytes = lib.la_pair_metrics_workspace_bytes(N, C, H, W, win, levels)
    assert ws_bytes > 0, 'shape refused'
    ws = torch.empty([ws_bytes // 8], dtype=torch.float64, device=dev)
    err = torch.empty([N, C, 2], dtype=torch.float64, device=dev)
    ssim = torch.empty([N, C, levels], dtype=torch.float32, device=dev)
    cs = torch.empty([N, C, levels], dtype=torch.float32, device=dev)
    ms = torch.empty([N, C], dtype=torch.float32, device=dev)
    hist = torch.empty([N, bins, bins], dtype=torch.int32, device=dev)
    lo, scale = -1.0, float(np.float32(bins / 2.0))
    out = {}

    def hip_pair():
        _lib.check(lib.la_pair_metrics_f32(p(x), p(y), None, None, N, C, H, W, taps.ctypes.data, win, levels, wts.ctypes.data, c1, c2,
                                           p(err), p(ssim), p(cs), p(ms), p(ws), ws_bytes, st()), 'pair_metrics')

    g_row = torch.from_numpy(taps).to(dev).view(1, 1, 1, win).repeat(5 * C, 1, 1, 1)
    g_col = g_row.view(5 * C, 1, win, 1)
    wt = torch.from_numpy(wts).to(dev)

    def torch_pair():
        a, b = x, y
        d = a - b
        out['err'] = torch.stack([(d.double() ** 2).sum(dim=(2, 3)), d.double().abs().sum(dim=(2, 3))], dim=-1)
        s_l, c_l = [], []
        for lv in range(levels):
            m = torch.cat([a, b, a * a, b * b, a * b], dim=1)
            m = torch.nn.functional.conv2d(torch.nn.functional.conv2d(m, g_row, groups=5 * C), g_col, groups=5 * C)
            mx, my, exx, eyy, exy = m.split(C, dim=1)
            sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
            c_map = (2 * sxy + c2) / (sxx + syy + c2)
            s_map = (2 * mx * my + c1) / (mx * mx + my * my + c1) * c_map
            s_l.append(s_map.mean(dim=(2, 3)))
            c_l.append(c_map.mean(dim=(2, 3)))
            if lv + 1 < levels:
                a, b = torch.nn.functional.avg_pool2d(a, 2), torch.nn.functional.avg_pool2d(b, 2)
        out['ssim'], out['cs'] = torch.stack(s_l, dim=-1), torch.stack(c_l, dim=-1)
        f = torch.cat([out['cs'][..., :levels - 1], out['ssim'][..., levels - 1:]], dim=-1).clamp_min(0)
        out['ms'] = (f ** wt).prod(dim=-1)

    def hip_hist():
        _lib.check(lib.la_joint_hist_f32(x.data_ptr(), C * H * W, x.data_ptr() + 4 * H * W, C * H * W, N, H * W, bins, lo, scale, p(hist),
                                         st()), 'joint_hist')

    thist = torch.empty([N * bins * bins], dtype=torch.int32, device=dev)
    ones = torch.ones([N * H * W], dtype=torch.int32, device=dev)
    plane = (torch.arange(N, device=dev) * (bins * bins)).view(N, 1, 1)

    def torch_hist():
        ba = torch.floor((x[:, 0] - lo) * scale).clamp_(0, bins - 1).long()
        bb = torch.floor((x[:, 1] - lo) * scale).clamp_(0, bins - 1).long()
        thist.zero_()
        thist.index_add_(0, (plane + ba * bins + bb).flatten(), ones)

    forms = {'hip_pair': hip_pair, 'torch_pair': torch_pair, 'hip_hist': hip_hist, 'torch_hist': torch_hist}
    if C < 2:
        del forms['hip_hist'], forms['torch_hist']
    times = {k: [] for k in forms}
    for it in range(args.warmup + args.iters):
        for name, fn in forms.items():          # alternating: drift of a shared machine hits all forms alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1) / args.calls)
    row = {'shape': [N, C, H, W], 'levels': levels, 'win': win, 'bins': bins, 'calls_per_window': args.calls, 'windows': args.iters}
    for name in forms:
        ts = sorted(times[name])
        row[name] = {'ms_median': round(ts[len(ts) // 2], 5), 'ms_min': round(ts[0], 5), 'ms_max': round(ts[-1], 5)}
    row['torch_pair_max_abs_difference'] = {k: float((out[k].double() - v.double()).abs().max())
                                            for k, v in (('ssim', ssim), ('cs', cs), ('ms', ms))}
    row['torch_pair_error_sums_max_relative_difference'] = float(((out['err'] - err).abs() / err.clamp_min(1e-300)).max())
    if 'hip_hist' in forms:
        row['torch_hist_cells_differing'] = int((thist.view(N, bins, bins) != hist).sum())
        row['hist_total'] = int(hist.sum(dtype=torch.int64))
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
