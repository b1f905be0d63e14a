"""Dev tool: are the op layer's outputs byte-equal on two builds of the library?
    python scripts/check_op_bits.py tmp_libs/base/liblatentaug_hip.so latentaugment_amd/liblatentaug_hip.so
Each library runs the same calls in a fresh process of its own (`--dump LIB OUT.npz`, the library path replacing _lib.LIB_PATH before
anything loads it, as scripts/bench_with_lib.py does); this process only compares the bytes and prints one line.  In float16, float32 and
float64: bias_act for the nine activations, with a clamp and without, forward, first order (dx, db) and second order, the bias on axis 1
of a 4-D tensor and on the last axis, aligned and at a one-element storage offset; upfirdn2d / filter2d / upsample2d / downsample2d
forward and dx with setup_filter([1,3,3,1]), a dense 3x5 filter at gain 1.7 and a separable 12-tap filter.  In float32: conv2d / conv_transpose2d forward,
dx and dw on split-K and direct grids, stride 2 and groups; the KID sums and MMD^2 and the density / coverage outputs (radii, count, nearest) at
the smallest shapes that reach every form of their tile kernels.  Inputs: seeded CPU generator."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(lib_path, out_path):
    sys.path.insert(0, ROOT)
    import torch
    from latentaugment_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    import ctypes
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for k in list(_lib.SIGNATURES):      # (entries the other build lacks are dropped from the binding table, as scripts/bench_with_lib.py does)
        if not hasattr(probe, k):
            del _lib.SIGNATURES[k]
    from latentaugment_amd import ops
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    res = {}

    def draw(shape, dt, offset=0):
        """a contiguous tensor of `shape` whose storage starts `offset` elements into its allocation"""
        n = int(np.prod(shape))
        buf = torch.zeros([n + offset], dtype=dt, device=dev)
        buf[offset:] = torch.randn([n], generator=gen, dtype=torch.float64).to(dt).to(dev)
        return buf[offset:].view(shape)

    def keep(key, t):
        if t is not None:
            res[key] = t.detach().contiguous().cpu().view(torch.uint8).numpy().ravel()

    for dt in (torch.float16, torch.float32, torch.float64):
        for act in ops._ACTS:
            for clamp in (None, 0.6):
                for dim, shape in ((1, [3, 5, 4, 8]), (3, [2, 3, 5, 7])):
                    for off in (0, 1):
                        x = draw(shape, dt, off).requires_grad_()
                        b = draw([shape[dim]], dt).requires_grad_()
                        gy = draw(shape, dt, off).requires_grad_()
                        g2x, g2b = draw(shape, dt, off), draw([shape[dim]], dt)
                        key = f'bias_act/{dt}/{act}/{clamp}/{dim}/{off}/'
                        y = ops.bias_act(x, b, dim=dim, act=act, clamp=clamp)
                        dx, db = torch.autograd.grad(y, [x, b], gy, create_graph=True)
                        second = torch.autograd.grad([dx, db], [gy, x, b], [g2x, g2b], allow_unused=True)
                        for name, t in zip(('y', 'dx', 'db', 'd_gy', 'd_x', 'd_b'), (y, dx, db) + tuple(second)):
                            keep(key + name, t)
        filters = {'1331': (ops.setup_filter([1, 3, 3, 1]), 1), 'dense3x5': (torch.randn([3, 5], generator=gen), 1.7),
                   'sep12': (ops.setup_filter(list(range(1, 7)) + list(range(6, 0, -1))), 1)}
        for fname, (f, gain) in filters.items():
            calls = {'upfirdn2d': lambda x: ops.upfirdn2d(x, f, up=2, down=3, padding=[1, 2, 0, 3], gain=gain),
                     'filter2d': lambda x: ops.filter2d(x, f, gain=gain), 'upsample2d': lambda x: ops.upsample2d(x, f, gain=gain),
                     'downsample2d': lambda x: ops.downsample2d(x, f, gain=gain)}
            for cname, call in calls.items():
                x = draw([2, 3, 16, 24], dt).requires_grad_()
                y = call(x)
                dx, = torch.autograd.grad(y, [x], draw(list(y.shape), dt))
                keep(f'{cname}/{dt}/{fname}/y', y)
                keep(f'{cname}/{dt}/{fname}/dx', dx)
    # the conv op (float32 only; its contractions go through la_conv_launch): split-K and direct grids, 64- and 128-row tiles, stride 2, groups
    convs = {'sk_8x8': (ops.conv2d, [2, 40, 8, 8], [12, 40, 3, 3], dict(padding=1)),
             'direct_40x40': (ops.conv2d, [1, 17, 40, 40], [132, 17, 3, 3], dict(padding=1)),
             's2_g2': (ops.conv2d, [2, 8, 17, 19], [8, 4, 3, 3], dict(stride=2, padding=(1, 0), groups=2)),
             't_s2': (ops.conv_transpose2d, [2, 36, 9, 9], [36, 8, 3, 3], dict(stride=2))}
    for cname, (call, xs, wsh, kw) in convs.items():
        x, w = draw(xs, torch.float32).requires_grad_(), draw(wsh, torch.float32).requires_grad_()
        y = call(x, w, **kw)
        dx, dw = torch.autograd.grad(y, [x, w], draw(list(y.shape), torch.float32))
        for name, t in zip(('y', 'dx', 'dw'), (y, dx, dw)):
            keep(f'conv/{cname}/{name}', t)
    # (dw of every case above runs la_conv_wgrad_mfma_kernel; sk_8x8 in 2 K slices on a grid 8 wide, direct_40x40 in 15 on one 40 wide:
    #  more than one slice and a width that is no multiple of the 16-pixel chunk are both there)
    # the metric entries on the tile loop of la_f32_tile.h.  KID: S = 2, mx = 130 (an off-diagonal and a diagonal xx tile), my = 3 (a
    # ragged y side); D = 130: scalar loads, 9 chunks (one fold after chunk 7, a ragged last chunk), D = 256: 16-byte loads, two full chains
    from latentaugment_amd import metrics
    ix = torch.randint(0, 140, [2, 130], generator=gen).numpy()
    iy = torch.randint(0, 5, [2, 3], generator=gen).numpy()
    for D in (130, 256):
        _, det = metrics.compute_kid_from_features(draw([5, D], torch.float32), draw([140, D], torch.float32), indices=(ix, iy), device=dev,
                                                   return_details=True)
        res[f'kid/{D}/sums'], res[f'kid/{D}/mmd2'] = det['sums'].view(np.uint8).ravel(), det['mmd2'].view(np.uint8).ravel()
    # density and coverage: la_pr_kth_f16 (radii) and la_dc_count_f16 (count, nearest) at 130 x 130 x 80: two row blocks, D past one
    # 64-wide K chunk with a ragged second one
    _, _, det = metrics.compute_dc_from_features(draw([130, 80], torch.float32), draw([130, 80], torch.float32), device=dev, return_details=True)
    for name in ('radii', 'count', 'nearest'):
        res[f'dc/{name}'] = det[name].view(np.uint8).ravel()
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def main():
    if sys.argv[1] == '--dump':
        return dump(sys.argv[2], sys.argv[3])
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, f'op_bits_{i}.npz')
            subprocess.run([sys.executable, os.path.abspath(__file__), '--dump', lib, out], check=True, timeout=300)
            outs.append(dict(np.load(out)))
    a, b = outs
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not np.array_equal(a[k], b[k])]
    print(f'op_bits: {len(a)} outputs, {sum(a[k].size for k in a)} bytes, {len(differ)} differ' +
          ''.join(f'\n  {k}' for k in differ[:20]))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
