"""Benchmark of la_knn_f32 and la_realism_f32 (nearest bank rows and realism score in float64 on float32 features) beside two
yardsticks on the same GPU in the same process.

  python scripts/bench_knn.py [--iters 20] [--warmup 5] [--shapes 1572x1572x4096,375x375x4096,8x1572x4096] [--k 5]

Shapes are (nq, nx, D): 1572 x 1572 x 4096 (the Pelvis-scale bank against itself), 375 x 375 x 4096 and 8 x 1572 x 4096 (one batch
against the bank).  Features are float32 and resident on the device; the radii of the realism pass are computed once and are not part
of any timed window.  Every form is timed with device events around one call on the current stream, after `--warmup` untimed rounds of
every form at that shape; the forms alternate inside every round; the median of `--iters` rounds is reported.
  hip_knn      la_knn_f32 with k: the norm launch, the tiled launch, the finish launch
  hip_realism  la_realism_f32 at the same shape
  hip_fd_gram  la_fd_gram_f32 at the same shape where it accepts it (both sides >= 2 rows): the same float64 MFMA work with a plain store
               for an epilogue
  torch_f64    torch.cdist of the features widened to float64, then topk(k, largest=False): the same accuracy class, with the
               [nq, nx] matrix in memory (the widening is inside the timed window: the library's entries take float32 too)
  torch_f32    the same in float32
Prints ONE JSON line: per shape and form milliseconds (median, minimum, maximum), for the HIP forms the workgroups of the tiled launch
and the rate of the pair grid's 2 D FLOP per pair, per shape the ratio torch_f64 / hip_knn, and how many of hip_knn's indices the two
torch forms reproduce (float32 cdist rounds differently; printed, not asserted).  No ratio is asserted.
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
    ap.add_argument('--shapes', default='1572x1572x4096,375x375x4096,8x1572x4096')
    ap.add_argument('--k', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_knn.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr
    k = args.k
    result = {'bench': 'knn', 'k': k, 'iters': args.iters, 'device': torch.cuda.get_device_name(0), 'shapes': []}
    for shape in args.shapes.split(','):
        nq, nx, D = (int(v) for v in shape.split('x'))
        g = torch.Generator(device=dev).manual_seed(nq + nx)
        # one draw split into the two sides: mostly positive, as pooled detector features
        both = torch.randn([nq + nx, D], generator=g, device=dev).abs() * 0.7 - 0.15 + 0.3 * torch.randn([1, D], generator=g, device=dev)
        q, x = both[:nq].contiguous(), both[nq:].contiguous()
        nbytes = lib.la_knn_scratch_bytes(nq, nx, D, k)
        ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
        dist2 = torch.empty([nq, k], dtype=torch.float64, device=dev)
        idx = torch.empty([nq, k], dtype=torch.int32, device=dev)
        score2 = torch.empty([nq], dtype=torch.float64, device=dev)
        arg = torch.empty([nq], dtype=torch.int32, device=dev)
        # radii: the squared distance of every bank row to its 3rd nearest other bank row
        rb = lib.la_knn_scratch_bytes(nx, nx, D, 3)
        rws = torch.empty([rb // 8], dtype=torch.float64, device=dev)
        rd = torch.empty([nx, 3], dtype=torch.float64, device=dev)
        ri = torch.empty([nx, 3], dtype=torch.int32, device=dev)
        _lib.check(lib.la_knn_f32(p(x), nx, p(x), nx, D, 3, 1, p(rd), p(ri), p(rws), rb, st()), 'knn radii')
        radius2 = rd[:, 2].contiguous()
        del rws
        out = {}
        forms = {}

        def hip_knn():
            _lib.check(lib.la_knn_f32(p(q), nq, p(x), nx, D, k, 0, p(dist2), p(idx), p(ws), nbytes, st()), 'knn')

        def hip_realism():
            _lib.check(lib.la_realism_f32(p(q), nq, p(x), nx, D, p(radius2), p(score2), p(arg), p(ws), nbytes, st()), 'realism')

        def torch_f64():
            out['f64'] = torch.cdist(q.double(), x.double()).topk(k, dim=1, largest=False)

        def torch_f32():
            out['f32'] = torch.cdist(q, x).topk(k, dim=1, largest=False)

        forms.update(hip_knn=hip_knn, hip_realism=hip_realism)
        if nq >= 2 and nx >= 2 and min(nq, nx) <= 8192:
            fb = lib.la_fd_workspace_bytes(nq, nx, D)
            fws = torch.empty([fb // 8], dtype=torch.float64, device=dev)
            terms = torch.empty([4], dtype=torch.float64, device=dev)

            def hip_fd_gram():
                _lib.check(lib.la_fd_gram_f32(p(q), nq, p(x), nx, D, p(terms), p(fws), fb, st()), 'fd_gram')
            forms['hip_fd_gram'] = hip_fd_gram
        forms.update(torch_f64=torch_f64, torch_f32=torch_f32)
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
        flops = 2.0 * D * nq * nx
        wgs = -(-nq // 64) * lib.la_knn_col_splits(nq, nx)
        row = {'nq': nq, 'nx': nx, 'D': D, 'col_splits': lib.la_knn_col_splits(nq, nx), 'forms': {}}
        for name in forms:
            ts = sorted(times[name])
            f = {'ms_median': round(ts[len(ts) // 2], 4), 'ms_min': round(ts[0], 4), 'ms_max': round(ts[-1], 4)}
            if name.startswith('hip_'):
                f['tflops_pair_grid'] = round(flops / (f['ms_median'] * 1e-3) / 1e12, 2)
            if name in ('hip_knn', 'hip_realism'):
                f['workgroups'] = wgs
            row['forms'][name] = f
        row['torch_f64_over_hip_knn'] = round(row['forms']['torch_f64']['ms_median'] / row['forms']['hip_knn']['ms_median'], 3)
        row['torch_f32_over_hip_knn'] = round(row['forms']['torch_f32']['ms_median'] / row['forms']['hip_knn']['ms_median'], 3)
        row['indices_equal_torch_f64'] = int((out['f64'].indices == idx.long()).sum())
        row['indices_equal_torch_f32'] = int((out['f32'].indices == idx.long()).sum())
        row['indices'] = nq * k
        result['shapes'].append(row)
        del both, q, x, out
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
