"""Benchmark of metrics.compute_fd_from_features (la_frechet.hip: la_fd_gram_f32, la_fd_jacobi_sweep_f64, la_fd_finish_f64) and, on
request, of the host route it stands beside (FeatureStats moments + compute_fid_from_stats: scipy.linalg.sqrtm of a D x D product).

  python scripts/bench_fd.py [--iters 5] [--warmup 2] [--sizes 1572,375] [--dim 4096] [--host]

N = 1572 (the real-image bank of preset E) and N = 375 rows per side with the VGG16 detector's D = 4096, features resident on the
device.  Per size, one JSON line each:
  entries   the three entries timed apart with device events on the launch stream (one run after the warm-up): the Gram entry, every
            sweep (their number, the median and the sum), the finish entry; the Gram entry's fraction of the 78.6 TFLOP/s float64 MFMA
            peak (2 nx ny D FLOPs) and a sweep's bytes per second (n' - 1 rounds, each reading and at most writing n' m doubles).
  whole     compute_fd_from_features from its start to the Python float it returns, host clock, median of --iters calls.
  host      only with --host, ONCE (it may take minutes): the features through FeatureStats(capture_mean_cov=True) and
            compute_fid_from_stats, host clock; the value and its difference to the device route's relative to the size of the terms.
No ratio is asserted.
"""
import argparse
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, metrics  # noqa: E402

PEAK_F64_MFMA = 78.6e12


def timed_entries(real, gen, dev, max_sweeps=60):
    lib = _lib.load()
    ng, nr, D = gen.shape[0], real.shape[0], gen.shape[1]
    n, m = min(ng, nr), max(ng, nr)
    ws_bytes = lib.la_fd_workspace_bytes(ng, nr, D)
    ws = torch.empty([ws_bytes // 8], dtype=torch.float64, device=dev)
    out = torch.empty([4 + n], dtype=torch.float64, device=dev)
    rot = torch.empty([1], dtype=torch.int32, device=dev)
    p, st = _lib.ptr, _lib.stream_ptr

    def timed(call, what):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(call(), what)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    with torch.cuda.device(dev):
        gram_ms = timed(lambda: lib.la_fd_gram_f32(p(gen), ng, p(real), nr, D, p(out), p(ws), ws_bytes, st()), 'fd_gram')
        sweep_ms, rotations = [], []
        while len(sweep_ms) < max_sweeps:
            sweep_ms.append(timed(lambda: lib.la_fd_jacobi_sweep_f64(p(ws), n, m, p(rot), st()), 'fd_jacobi_sweep'))
            rotations.append(int(rot.item()))
            if rotations[-1] == 0:
                break
        finish_ms = timed(lambda: lib.la_fd_finish_f64(p(ws), ws_bytes, ng, nr, D, p(out[4:]), p(out), st()), 'fd_finish')
    n2 = n + (n & 1)
    med = sorted(sweep_ms)[len(sweep_ms) // 2]
    return dict(gram_ms=round(gram_ms, 3), gram_peak_frac_f64_mfma=round(2.0 * ng * nr * D / (gram_ms * 1e-3) / PEAK_F64_MFMA, 4),
                sweeps=len(sweep_ms), converged=rotations[-1] == 0, rotations=rotations, sweep_ms_median=round(med, 3),
                sweep_ms_sum=round(sum(sweep_ms), 3), launches_per_sweep=n2 - 1, us_per_round=round(med * 1e3 / (n2 - 1), 3),
                sweep_gbytes_per_s=round(2.0 * (n2 - 1) * n2 * m * 8 / (med * 1e-3) / 1e9, 1), finish_ms=round(finish_ms, 3),
                workspace_mb=round(ws_bytes / 2 ** 20, 2))


def host_route(real, gen, dev):
    """FeatureStats moments (on the device) and compute_fid_from_stats (scipy on the host)"""
    alive = threading.Event()

    def beat():
        t0 = time.perf_counter()
        while not alive.wait(60.0):
            print(f'# host route still running after {time.perf_counter() - t0:.0f} s', flush=True)
    th = threading.Thread(target=beat, daemon=True)
    th.start()
    try:
        t0 = time.perf_counter()
        sr, sg = metrics.FeatureStats(capture_mean_cov=True, device=dev), metrics.FeatureStats(capture_mean_cov=True, device=dev)
        sr.append_torch(real)
        sg.append_torch(gen)
        (mu_r, sig_r), (mu_g, sig_g) = sr.get_mean_cov(), sg.get_mean_cov()
        t1 = time.perf_counter()
        fid = metrics.compute_fid_from_stats(mu_r, sig_r, mu_g, sig_g)
        t2 = time.perf_counter()
    finally:
        alive.set()
    return dict(moments_ms=round((t1 - t0) * 1e3, 1), sqrtm_ms=round((t2 - t1) * 1e3, 1), fid=fid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', default='1572,375')
    ap.add_argument('--dim', type=int, default=4096)
    ap.add_argument('--host', action='store_true', help='also time the host route once per size (may take minutes)')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    for n in (int(v) for v in args.sizes.split(',')):
        g = torch.Generator(device=dev).manual_seed(n)
        # non-negative with a few strong directions, as fully connected detector features after a ReLU; the generated side 5 % larger
        real = torch.relu(torch.randn([n, args.dim], generator=g, device=dev) + 0.3) * 1.5
        gen = torch.relu(torch.randn([n, args.dim], generator=g, device=dev) + 0.3) * 1.575
        base = dict(N=n, D=args.dim)
        times, fd, det = [], None, None
        for it in range(args.warmup + args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fd, det = metrics.compute_fd_from_features(real, gen, device=dev, return_details=True, max_sweeps=60)
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                times.append(dt * 1e3)
        print(json.dumps(dict(base, form='entries', **timed_entries(real, gen, dev))), flush=True)
        ts = sorted(times)
        scale = det['mean_term'] + det['trace_gen'] + det['trace_real']
        print(json.dumps(dict(base, form='whole', ms_median=round(ts[len(ts) // 2], 3), ms_min=round(ts[0], 3), ms_max=round(ts[-1], 3),
                              fd=fd, sweeps=det['sweeps'], terms_scale=scale)), flush=True)
        if args.host:
            h = host_route(real, gen, dev)
            print(json.dumps(dict(base, form='host', **h, diff_to_device_over_terms=abs(h['fid'] - fd) / scale)), flush=True)
        del real, gen
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
