"""Benchmark of la_dc_count_f16 (density and coverage, one pass over the generated x real pair grid) beside two yardsticks on the same
GPU in the same process.

  python scripts/bench_dc.py [--iters 20] [--warmup 5] [--shapes 1572x1572x4096,10000x10000x2048]

Shapes are (nr, ng, D): 1572 x 1572 x 4096 (the Pelvis-scale bank) and 10000 x 10000 x 2048.  Features are float16 and resident on the
device; the radii are computed once with la_pr_kth_f16 and are not part of any timed window.  Every form is timed with device events
around one call on the current stream, after `--warmup` untimed rounds of every form at that shape; the forms alternate inside every
round; the median of `--iters` rounds is reported.
  hip_dc       la_dc_count_f16: count[ng] and nearest[nr] from one launch sequence (init, two norm launches, the tiled kernel)
  torch        torch.cdist of the float16 features, a compare with the radii, a sum over the real axis and an any over the generated
               axis: the same two outputs (count, covered) with the [ng, nr] matrix in memory
  hip_member   la_pr_member_f16 at the same shape: the same MFMA work for ONE OR output per generated row, on ceil(ng / 128) workgroups
Prints one JSON line per (shape, form): milliseconds (median, minimum, maximum), the workgroups of the tiled launch, for the two HIP
forms the rate of the pair grid's 2 D FLOP per pair, and for `torch` whether its count and covered bits equal hip_dc's (float16 cdist
rounds differently, so a small number of differences is expected and is printed, not asserted).  No ratio is asserted.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shapes', default='1572x1572x4096,10000x10000x2048')
    ap.add_argument('--nhood-size', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_dc.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr
    for shape in args.shapes.split(','):
        nr, ng, D = (int(v) for v in shape.split('x'))
        g = torch.Generator(device=dev).manual_seed(nr + ng)
        # one draw split into the two sides (two draws with separate offsets would leave every ball empty): mostly positive, as pooled
        # detector features
        both = (torch.randn([nr + ng, D], generator=g, device=dev).abs() * 0.7 - 0.15 + 0.3 * torch.randn([1, D], generator=g, device=dev)).half()
        real, gen = both[:nr].contiguous(), both[nr:].contiguous()
        ws_bytes = max(lib.la_dc_workspace_bytes(ng, nr), 4 * lib.la_pr_workspace_floats(max(ng, nr), nr))
        ws = torch.empty([ws_bytes // 4], dtype=torch.float32, device=dev)
        radii = torch.empty([nr], dtype=torch.float32, device=dev)
        _lib.check(lib.la_pr_kth_f16(p(real), nr, p(real), nr, D, args.nhood_size, p(radii), p(ws), st()), 'pr_kth')
        count = torch.empty([ng], dtype=torch.int32, device=dev)
        nearest = torch.empty([nr], dtype=torch.float32, device=dev)
        member = torch.empty([ng], dtype=torch.uint8, device=dev)
        out = {}

        def hip_dc():
            _lib.check(lib.la_dc_count_f16(p(gen), ng, p(real), nr, D, p(radii), p(count), p(nearest), p(ws), ws_bytes, st()), 'dc_count')

        def torch_form():
            d = torch.cdist(gen, real)
            inside = d <= radii.to(d.dtype)[None, :]
            out['count'], out['covered'] = inside.sum(dim=1, dtype=torch.int32), inside.any(dim=0)

        def hip_member():
            _lib.check(lib.la_pr_member_f16(p(gen), ng, p(real), nr, D, p(radii), p(member), p(ws), st()), 'pr_member')

        forms = {'hip_dc': hip_dc, 'torch': torch_form, 'hip_member': hip_member}
        times = {k: [] for k in forms}
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
        covered = nearest <= radii
        flops = 2.0 * D * nr * ng
        wgs = {'hip_dc': -(-ng // 128) * lib.la_dc_col_splits(ng, nr), 'hip_member': -(-ng // 128)}
        for name in forms:
            ts = sorted(times[name])
            row = {'nr': nr, 'ng': ng, 'D': D, 'k': args.nhood_size, 'form': name, 'ms_median': round(ts[len(ts) // 2], 4), 'ms_min': round(ts[0], 4),
                   'ms_max': round(ts[-1], 4)}
            if name in wgs:
                row['workgroups'] = wgs[name]
                row['tflops_pair_grid'] = round(flops / (row['ms_median'] * 1e-3) / 1e12, 2)
            if name == 'hip_dc':
                row['density'] = int(count.sum(dtype=torch.int64)) / (args.nhood_size * ng)
                row['coverage'] = int(covered.sum()) / nr
            if name == 'torch':
                row['count_rows_differing_from_hip_dc'] = int((out['count'] != count).sum())
                row['covered_bits_differing_from_hip_dc'] = int((out['covered'] != covered).sum())
            if name == 'hip_member':
                row['member_bits_differing_from_count_gt_0'] = int((member.bool() != (count > 0)).sum())
            print(json.dumps(row), flush=True)
        del both, real, gen, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
