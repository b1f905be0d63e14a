"""Benchmark of the UMAP embedding (la_umap.hip, latentaugment_amd.embedding) stage by stage.

  python scripts/bench_umap.py [--iters 10] [--warmup 3] [--shapes 1572x512,1572x4096,16384x512] [--cpu-fit-rows 2000]

Shapes are (rows, features): 1572 x 512 (the W codes of a Pelvis-scale inverted set), 1572 x 4096 (detector features of the same set)
and 16 384 x 512.  n_neighbors 15, 2 components, the default epochs (500 up to 10 000 rows, 200 above), 5 negatives.  Inputs are
seeded clusters, float32, resident on the device for the stage timings.
  knn, smooth_knn, graph   one call each, device events around it
  epoch                    la_umap_layout_f64 over 50 epochs from the middle of the schedule on the fitted positions, divided by 50
  fit                      LatentUMAP.fit from a host array to embedding_ on the host: a host clock around it (it ends in a copy)
  transform_300            LatentUMAP.transform of 300 new rows, the same way
Every GPU form runs `--warmup` untimed rounds first; the median, minimum and maximum of `--iters` rounds are reported.
Beside each, `cpu_numpy_s`: the wall time of the float64 numpy restatement of the same stage (tests/umap_cases.py) on the host CPU,
one run -- a restatement written for clarity, not a tuned CPU implementation, and labelled as that.  Its whole fit is run up to
`--cpu-fit-rows` rows; above, only its stages and one epoch are.  No GPU UMAP (cuML) and no umap-learn exist on these machines, so
there is no other implementation to compare with.  Prints ONE JSON line; no ratio is asserted.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from latentaugment_amd import _lib, metrics  # noqa: E402
from latentaugment_amd.embedding import LatentUMAP  # noqa: E402
import umap_cases as uc  # noqa: E402


def clusters(n, D, seed):
    rng = np.random.default_rng(seed)
    c = 8
    centers = 4.0 * rng.standard_normal([c, D]) / np.sqrt(D / 16.0)
    return (centers[np.arange(n) % c] + rng.standard_normal([n, D]) / np.sqrt(D / 16.0)).astype(np.float32)


def stats(ts):
    ts = sorted(ts)
    return {'ms_median': round(ts[len(ts) // 2], 4), 'ms_min': round(ts[0], 4), 'ms_max': round(ts[-1], 4)}


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def knn_chunked(X, k):
    """the restatement's neighbour search in float64, in row blocks (the [n, n] matrix of 16 384 rows does not fit comfortably)"""
    X = X.astype(np.float64)
    sq = (X * X).sum(1)
    d2s, ids = [], []
    for lo in range(0, len(X), 2048):
        d2 = np.maximum(sq[lo:lo + 2048, None] + sq[None, :] - 2.0 * (X[lo:lo + 2048] @ X.T), 0.0)
        d2[np.arange(d2.shape[0]), lo + np.arange(d2.shape[0])] = np.inf
        part = np.argpartition(d2, k, axis=1)[:, :k]
        pd = np.take_along_axis(d2, part, axis=1)
        order = np.argsort(pd, axis=1, kind='stable')
        d2s.append(np.take_along_axis(pd, order, axis=1))
        ids.append(np.take_along_axis(part, order, axis=1).astype(np.int32))
    return np.concatenate(d2s), np.concatenate(ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='1572x512,1572x4096,16384x512')
    ap.add_argument('--cpu-fit-rows', type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_umap.py measures on the GPU; a measurement path that finds none fails'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr
    nn, Cc, rate = 15, 2, 5
    k = nn - 1
    result = {'bench': 'umap', 'n_neighbors': nn, 'n_components': Cc, 'negative_sample_rate': rate, 'iters': args.iters,
              'device': torch.cuda.get_device_name(0), 'cpu_numpy_s': 'float64 numpy restatement (tests/umap_cases.py), one run, host CPU',
              'shapes': []}
    for shape in args.shapes.split(','):
        n, D = (int(v) for v in shape.split('x'))
        X = clusters(n, D, n + D)
        Xq = clusters(300, D, n + D + 1)
        um = LatentUMAP(n_neighbors=nn, n_components=Cc, negative_sample_rate=rate, device=dev)
        E = um._epochs(n)
        x = torch.from_numpy(X).to(dev)
        dist2 = torch.empty([n, k], dtype=torch.float64, device=dev)
        idx = torch.empty([n, k], dtype=torch.int32, device=dev)
        kb = lib.la_knn_scratch_bytes(n, n, D, k)
        kws = torch.empty([kb // 8], dtype=torch.float64, device=dev)
        rho, sigma = (torch.empty([n], dtype=torch.float64, device=dev) for _ in range(2))
        w = torch.empty([n, k], dtype=torch.float64, device=dev)
        gb = lib.la_umap_scratch_bytes(n, k)
        gws = torch.empty([gb // 8], dtype=torch.float64, device=dev)
        cap = 2 * n * k
        row_ptr = torch.empty([n + 1], dtype=torch.int32, device=dev)
        col = torch.empty([cap], dtype=torch.int32, device=dev)
        val = torch.empty([cap], dtype=torch.float64, device=dev)
        wmax = torch.empty([1], dtype=torch.float64, device=dev)
        um.fit(X)
        ya, yb = um._y.clone(), torch.empty_like(um._y)
        which = C.c_int(0)
        e0 = E // 2

        def knn():
            _lib.check(lib.la_knn_f32(p(x), n, p(x), n, D, k, 1, p(dist2), p(idx), p(kws), kb, st()), 'knn')

        def smooth_knn():
            _lib.check(lib.la_umap_smooth_knn_f64(p(dist2), p(idx), n, k, float(np.log2(nn)), p(rho), p(sigma), p(w), st()), 'smooth')

        def graph():
            _lib.check(lib.la_umap_graph_f64(p(idx), p(w), n, k, p(row_ptr), p(col), p(val), cap, p(wmax), p(gws), gb, st()), 'graph')

        def epochs50():
            _lib.check(lib.la_umap_layout_f64(p(ya), p(yb), n, None, n, Cc, p(row_ptr), p(col), p(val), cap, p(wmax), e0, e0 + 50, E, um.a, um.b,
                                              rate, 1.0, 42, 0, 1, C.byref(which), st()), 'layout')
        forms = dict(knn=knn, smooth_knn=smooth_knn, graph=graph, epochs50=epochs50)
        times = {name: [] for name in forms}
        host = {'fit': [], 'transform_300': []}
        for it in range(args.warmup + args.iters):
            for name, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(t0.elapsed_time(t1))
            for name, fn in (('fit', lambda: um.fit(X)), ('transform_300', lambda: um.transform(Xq))):
                torch.cuda.synchronize()
                _, dt = wall(fn)
                if it >= args.warmup:
                    host[name].append(dt * 1e3)
        row = {'rows': n, 'features': D, 'epochs': E, 'graph_entries': int(row_ptr[n].item()), 'longest_row': int(torch.diff(row_ptr).max().item()),
               'gpu': {name: stats(ts) for name, ts in list(times.items()) + list(host.items())}}
        row['gpu']['epoch'] = {key: round(v / 50.0, 5) for key, v in row['gpu'].pop('epochs50').items()}
        # the numpy restatement, one run
        cpu = {}
        (d2c, idc), cpu['knn'] = wall(lambda: knn_chunked(X, k))
        sk, cpu['smooth_knn'] = wall(lambda: uc.smooth_knn(d2c, idc, nn))
        csr, cpu['graph'] = wall(lambda: uc.graph(idc, sk['w']))
        y_mid = um.embedding_
        _, cpu['epoch'] = wall(lambda: uc.epoch(y_mid, y_mid, *csr, float(csr[2].max()), e0, E, um.a, um.b, rate, 1.0, 42))
        if n <= args.cpu_fit_rows:
            fit, cpu['fit'] = wall(lambda: uc.fit_restate(X, nn, Cc, E, um.a, um.b, rate, 1.0, 42))
            _, cpu['transform_300'] = wall(lambda: uc.transform_restate(fit, X, Xq, nn, um.a, um.b, rate, 1.0, 42))
        else:
            cpu['fit'] = cpu['transform_300'] = 'not measured'
        row['cpu_numpy_s'] = {name: (round(v, 4) if not isinstance(v, str) else v) for name, v in cpu.items()}
        result['shapes'].append(row)
        print(f'bench_umap: {n} x {D} done', file=sys.stderr, flush=True)
        del x, kws, gws, col, val
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
