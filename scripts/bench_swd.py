"""Benchmark of the sliced Wasserstein distance (la_swd.hip, la_sort.hip) stage by stage, beside the same quantities composed from torch
ops on the same GPU in the same process.

  python scripts/bench_swd.py [--iters 10] [--warmup 3] [--images 1572,375] [--features 1572x512,16384x512] [--sort 512x201216]

Image shapes are sets of N images [N, 2, 256, 256] (CT + MRI), 128 neighbourhoods of 7 x 7 per image and level, 512 directions:
N = 1572 gives M = 201 216 descriptor rows of D = 98 per level, five levels (256 .. 16).  Both sets are resident on the device (the
package fills its descriptor banks batch by batch; the stages are timed on the whole set so that one number belongs to one stage).
Every form is timed with device events around one call on the current stream, after `--warmup` untimed rounds of every form at that
shape; the forms alternate inside every round; the median of `--iters` rounds is reported.
  hip_pyramid    la_lap_pyr_down_f32 and la_lap_pyr_up_sub_f32 for all levels of one set
  hip_gather     la_swd_gather_f32, all levels of one set
  hip_normalize  la_swd_channel_stats_f64 + la_swd_normalize_f32, all levels of one set (the two-pass statistics and the rewrite)
  hip_directions la_swd_directions_f32, all levels
  hip_swd        la_swd_f32 (project, sort, mean |a - b|), all levels, with the scratch metrics.py would give it
  hip_total      metrics.compute_swd_from_images on the two resident sets in batches of 131 images (everything, with its host syncs)
  torch_pyramid  reflect pad + conv2d (stride 2; zero-stuffed for the up-sampling) + subtraction
  torch_gather   advanced indexing into the unfolded view at random corners
  torch_normalize  mean / std over rows and positions, then the quotient
  torch_swd      matmul, torch.sort of both [dirs, M] matrices, mean |a - b|
The features route is timed at (N, D) as hip_swd / torch_swd on N x D rows with 512 directions.  la_sort_columns_f32 is timed alone at
ncols x M beside torch.sort of the same matrix, with the bytes its passes move (one read and one write of every key per launch: the
tile sort and ceil(log2(tiles)) merges) over its time, against the 6.29 TB/s a copy kernel reaches on this part (8 TB/s on paper).
Prints ONE JSON line.  No ratio is asserted.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, metrics  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12
NHOOD, PER_IMAGE, NDIRS = 7, 128, 512


def timed(forms, iters, warmup):
    times = {name: [] for name in forms}
    for it in range(warmup + iters):
        for name, fn in forms.items():          # alternating: drift of a shared machine hits all forms alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    out = {}
    for name, ts in times.items():
        ts = sorted(ts)
        out[name] = {'ms_median': round(ts[len(ts) // 2], 4), 'ms_min': round(ts[0], 4), 'ms_max': round(ts[-1], 4)}
    return out


def swd_forms(lib, a, b, dirs):
    """hip_swd / torch_swd on a, b [M, D] and dirs [ndirs, D]; returns (forms, results dict)"""
    p, st = _lib.ptr, _lib.stream_ptr
    (M, D), ndirs = a.shape, dirs.shape[0]
    floor_bytes = lib.la_swd_scratch_bytes(M, D, ndirs)
    nbytes = max(floor_bytes, min(floor_bytes * -(-ndirs // 32), 1 << 30))
    ws = torch.empty([nbytes // 8], dtype=torch.float64, device=a.device)
    w1 = torch.empty([ndirs], dtype=torch.float64, device=a.device)
    res = {}

    def hip_swd():
        _lib.check(lib.la_swd_f32(p(a), p(b), M, D, p(dirs), ndirs, p(w1), p(ws), nbytes, st()), 'swd')
        res['hip'] = w1

    def torch_swd():
        sa, sb = torch.sort(dirs @ a.T, dim=1).values, torch.sort(dirs @ b.T, dim=1).values
        res['torch'] = (sa - sb).abs().mean(dim=1)
    return {'hip_swd': hip_swd, 'torch_swd': torch_swd}, res


def bench_images(lib, dev, N, iters, warmup):
    p, st = _lib.ptr, _lib.stream_ptr
    C, H = 2, 256
    g = torch.Generator(device=dev).manual_seed(N)
    real = torch.rand([N, C, H, H], generator=g, device=dev) * 2 - 1
    gen = (real + 0.2 * torch.randn([N, C, H, H], generator=g, device=dev)).clamp_(-1, 1)
    L, M, D = 5, N * PER_IMAGE, C * NHOOD * NHOOD
    k5 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=dev)
    k2 = (torch.outer(k5, k5) / 256)[None, None]
    levels = {}

    def hip_pyramid():
        levels['hip'] = metrics.laplacian_pyramid(real)

    def torch_pyramid():
        gs = [real.reshape(N * C, 1, H, H)]
        for _ in range(L - 1):
            gs.append(F.conv2d(F.pad(gs[-1], (2, 2, 2, 2), mode='reflect'), k2, stride=2))
        out = []
        for l in range(L - 1):
            z = torch.zeros_like(gs[l])
            z[:, :, ::2, ::2] = gs[l + 1]
            out.append(gs[l] - F.conv2d(F.pad(z, (2, 2, 2, 2), mode='reflect'), 4 * k2))
        levels['torch'] = out + [gs[-1]]
    hip_pyramid()
    torch_pyramid()
    torch.cuda.synchronize()
    pyr_err = max(float((a.reshape(b.shape) - b).abs().max()) for a, b in zip(levels['hip'], levels['torch']))
    lv_real = levels['hip']
    lv_gen = metrics.laplacian_pyramid(gen)
    del levels['torch']
    desc = [[torch.empty([M, D], device=dev) for _ in range(L)] for _ in range(2)]
    raw = [[None] * L for _ in range(2)]
    corners = [(torch.randint(0, (H >> l) - NHOOD + 1, [M], device=dev), torch.randint(0, (H >> l) - NHOOD + 1, [M], device=dev)) for l in range(L)]
    img_of_row = torch.arange(N, device=dev).repeat_interleave(PER_IMAGE)

    def gather_into(side, lvs):
        for l, lv in enumerate(lvs):
            _lib.check(lib.la_swd_gather_f32(p(lv), N, C, lv.shape[2], lv.shape[3], 0, l, NHOOD, PER_IMAGE, 0, p(desc[side][l]), st()), 'gather')

    def hip_gather():
        gather_into(0, lv_real)

    def torch_gather():
        for l, lv in enumerate(lv_real):
            y0, x0 = corners[l]
            raw[1][l] = lv.unfold(2, NHOOD, 1).unfold(3, NHOOD, 1)[img_of_row, :, y0, x0].reshape(M, D)
    stats = torch.empty([2, C], dtype=torch.float64, device=dev)
    sbytes = lib.la_swd_stats_scratch_bytes(M, C, NHOOD * NHOOD)
    sws = torch.empty([max(sbytes, 8) // 8], dtype=torch.float64, device=dev)

    def normalize_side(side):
        for l in range(L):
            d = desc[side][l]
            _lib.check(lib.la_swd_channel_stats_f64(p(d), M, C, NHOOD * NHOOD, p(stats[0]), p(stats[1]), p(sws), sbytes, st()), 'stats')
            _lib.check(lib.la_swd_normalize_f32(p(d), M, C, NHOOD * NHOOD, p(stats[0]), p(stats[1]), st()), 'normalize')

    def hip_normalize():          # (normalising normalised rows again costs the same)
        normalize_side(0)

    def torch_normalize():
        for l in range(L):
            x = desc[1][l].view(M, C, NHOOD * NHOOD)
            raw[0][l] = ((x - x.mean(dim=(0, 2), keepdim=True)) / x.std(dim=(0, 2), keepdim=True, unbiased=False)).view(M, D)
    dirs = [torch.empty([NDIRS, D], device=dev) for _ in range(L)]

    def hip_directions():
        for l in range(L):
            _lib.check(lib.la_swd_directions_f32(p(dirs[l]), NDIRS, D, l * metrics.SWD_LEVEL_DIR_STRIDE, 0, st()), 'directions')
    gather_into(0, lv_real)
    gather_into(1, lv_gen)
    normalize_side(0)
    normalize_side(1)
    hip_directions()
    per_level = [swd_forms(lib, desc[0][l], desc[1][l], dirs[l]) for l in range(L)]
    res = {}

    def hip_swd():
        for forms, _ in per_level:
            forms['hip_swd']()

    def torch_swd():
        for forms, _ in per_level:
            forms['torch_swd']()
    batches = lambda x: [x[i:i + 131] for i in range(0, N, 131)]          # noqa: E731

    def hip_total():
        res['total'] = metrics.compute_swd_from_images(batches(real), batches(gen))
    forms = dict(hip_pyramid=hip_pyramid, torch_pyramid=torch_pyramid, hip_gather=hip_gather, torch_gather=torch_gather,
                 hip_normalize=hip_normalize, torch_normalize=torch_normalize, hip_directions=hip_directions, hip_swd=hip_swd,
                 torch_swd=torch_swd, hip_total=hip_total)
    row = {'images': N, 'C': C, 'H': H, 'levels': L, 'M': M, 'D': D, 'ndirs': NDIRS, 'forms': timed(forms, iters, warmup)}
    row['pyramid_max_abs_diff_vs_torch'] = pyr_err
    row['w1_max_abs_diff_vs_torch'] = max(float((r['hip'] - r['torch'].double()).abs().max()) for _, r in per_level)
    row['swd'] = res['total']
    f = row['forms']
    for stage in ('pyramid', 'gather', 'normalize', 'swd'):
        row[f'torch_over_hip_{stage}'] = round(f[f'torch_{stage}']['ms_median'] / f[f'hip_{stage}']['ms_median'], 3)
    return row


def bench_features(lib, dev, N, D, iters, warmup):
    g = torch.Generator(device=dev).manual_seed(N + D)
    a = torch.randn([N, D], generator=g, device=dev)
    b = torch.randn([N, D], generator=g, device=dev) * 1.1 + 0.1
    dirs = torch.empty([NDIRS, D], device=dev)
    _lib.check(lib.la_swd_directions_f32(_lib.ptr(dirs), NDIRS, D, 0, 0, _lib.stream_ptr()), 'directions')
    forms, res = swd_forms(lib, a, b, dirs)
    row = {'rows': N, 'D': D, 'ndirs': NDIRS, 'forms': timed(forms, iters, warmup)}
    row['w1_max_abs_diff_vs_torch'] = float((res['hip'] - res['torch'].double()).abs().max())
    row['torch_over_hip_swd'] = round(row['forms']['torch_swd']['ms_median'] / row['forms']['hip_swd']['ms_median'], 3)
    return row


def bench_sort(lib, dev, ncols, M, iters, warmup):
    g = torch.Generator(device=dev).manual_seed(ncols + M)
    src = torch.randn([ncols, M], generator=g, device=dev)
    keys = torch.empty_like(src)
    nbytes = lib.la_sort_columns_scratch_bytes(ncols, M)
    ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
    res = {}

    def copy_only():          # the refill of `keys` that hip_sort's window contains
        keys.copy_(src)

    def hip_sort():
        keys.copy_(src)
        _lib.check(lib.la_sort_columns_f32(_lib.ptr(keys), ncols, M, M, _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'sort')

    def torch_sort():
        res['torch'] = torch.sort(src, dim=1).values
    row = {'ncols': ncols, 'M': M, 'tile_keys': lib.la_sort_tile_keys(), 'forms': timed(dict(copy_only=copy_only, hip_sort=hip_sort, torch_sort=torch_sort), iters, warmup)}
    f = row['forms']
    tiles = -(-M // row['tile_keys'])
    launches = 1 + (math.ceil(math.log2(tiles)) if tiles > 1 else 0)
    ms = f['hip_sort']['ms_median'] - f['copy_only']['ms_median']
    moved = launches * 2.0 * ncols * M * 4
    row.update(launches=launches, hip_sort_ms_without_refill=round(ms, 4), bytes_moved=moved,
               bytes_per_s=round(moved / (ms * 1e-3), 1), share_of_copy_rate=round(moved / (ms * 1e-3) / HBM_COPY_BYTES_PER_S, 4),
               equal_to_torch_sort=bool(torch.equal(keys, res['torch'])),
               torch_over_hip_sort=round(f['torch_sort']['ms_median'] / ms, 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--images', default='1572,375')
    ap.add_argument('--features', default='1572x512,16384x512')
    ap.add_argument('--sort', default='512x201216')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_swd.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    result = {'bench': 'swd', 'iters': args.iters, 'device': torch.cuda.get_device_name(0), 'images': [], 'features': [], 'sort': []}
    for shape in filter(None, args.sort.split(',')):
        ncols, M = (int(v) for v in shape.split('x'))
        result['sort'].append(bench_sort(lib, dev, ncols, M, args.iters, args.warmup))
        torch.cuda.empty_cache()
    for shape in filter(None, args.features.split(',')):
        N, D = (int(v) for v in shape.split('x'))
        result['features'].append(bench_features(lib, dev, N, D, args.iters, args.warmup))
        torch.cuda.empty_cache()
    for n in filter(None, args.images.split(',')):
        result['images'].append(bench_images(lib, dev, int(n), args.iters, args.warmup))
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
