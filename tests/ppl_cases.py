"""Cases, float64 numpy restatements and the CPU oracle for perceptual path length (la_path_points_f32, metrics.compute_ppl,
compute_path_length).  TEST INFRASTRUCTURE: runs in float64 (the anchor) or float32 (the yardstick), never on the GPU.

The restatements are the definitions as published (Karras et al. 2019, metrics/perceptual_path_length.py of StyleGAN2): lerp
a + (b - a) s; slerp with acos of the dot product of the normalised rows, plus the library's one rule for the place where the
published form has none: |b' - d a'| == 0 gives the normalised a.  The oracle composes the CPU generator and mapping under oracle/ with
tests/lpips_cases.pair_distance."""
import copy
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402

from oracle import sg2_networks as nets  # noqa: E402

KERNEL_D = (1, 3, 64, 512, 520)          # one element, odd, one wave, two / three strides of the 256 threads with a ragged tail
KERNEL_N = (1, 5)
KERNEL_REPS = (1, 14)
KERNEL_T = (1, 2, 17)


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements (float64 numpy; the caller rounds to float32 once)

def _params(t, dt):
    return np.asarray(t).astype(np.float64)[None, :] + np.asarray(dt, dtype=np.float64)[:, None]          # [T, N]


def lerp_points(a, b, t, dt, reps=1):
    """[T, N, reps, D] float64: a + (b - a) * ((double)t + dt)."""
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    s = _params(t, dt)
    p = a[None] + (b - a)[None] * s[:, :, None]
    return np.repeat(p[:, :, None, :], reps, axis=2)


def slerp_points(a, b, t, dt, reps=1):
    """[T, N, reps, D] float64: the published slerp, row by row; where |b' - d a'| == 0 every point is the normalised a."""
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    s = _params(t, dt)
    out = np.empty([s.shape[0], a.shape[0], a.shape[1]], np.float64)
    for p in range(a.shape[0]):
        au, bu = a[p] / np.sqrt((a[p] * a[p]).sum()), b[p] / np.sqrt((b[p] * b[p]).sum())
        d = (au * bu).sum()
        c = bu - d * au
        nc = np.sqrt((c * c).sum())
        if nc == 0.0:
            out[:, p] = au[None]
            continue
        c = c / nc
        th = s[:, p] * np.arccos(d)
        q = au[None] * np.cos(th)[:, None] + c[None] * np.sin(th)[:, None]
        out[:, p] = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    return np.repeat(out[:, :, None, :], reps, axis=2)


def percentile(d, q, rule):
    try:
        return np.percentile(d, q, method=rule)
    except TypeError:          # numpy < 1.22
        return np.percentile(d, q, interpolation=rule)


def ppl_filter(d):
    """The published filter: mean of the distances between the 1st percentile ('lower') and the 99th ('higher'), both included."""
    d = np.asarray(d, dtype=np.float64)
    lo, hi = percentile(d, 1, 'lower'), percentile(d, 99, 'higher')
    return float(np.extract(np.logical_and(lo <= d, d <= hi), d).mean())


def exact_rows(D, sign, seed=0):
    """Rows a, b = sign * 3 a whose norms and dot product are exact in any summation order: min(D, 4) entries of +-2^k, the rest 0 (a sum of
    1 or 4 equal powers of two is a power of 4 times 1 or 4, its root exact).  b' - d a' is then exactly 0."""
    rs = np.random.RandomState(seed + D)
    a = np.zeros([2, D], np.float32)
    for r in range(2):
        idx = rs.choice(D, min(D, 4) if D >= 4 else 1, replace=False)
        a[r, idx] = rs.choice([-1.0, 1.0], idx.size) * 2.0 ** (r - 1)
    return a, (sign * 3.0 * a).astype(np.float32)


def one_ulp(got, ref64):
    """got (float32) lies within one float32 step of the float64 value."""
    got, ref64 = np.asarray(got), np.asarray(ref64, np.float64)
    step = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return bool((np.abs(got.astype(np.float64) - ref64) <= step).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# toy nets and the oracle

RES, WDIM, IMG_CH = 32, 32, 2
PRE_SCALE, PRE_SHIFT = (0.9, 1.1, 1.0), (0.1, -0.05, 0.02)


@functools.lru_cache(maxsize=None)
def toy_generator():
    """Resolution 32, two image channels, a small channel table, two mapping layers, as the synthesis tests build theirs; w_avg is set so
    that truncation does something."""
    G = nets.make_generator(img_resolution=RES, img_channels=IMG_CH, channel_base=256, channel_max=16, seed=0, noise_strength=0.1,
                            w_dim=WDIM, mapping_layers=2)
    with torch.no_grad():
        G.mapping.w_avg.copy_(0.1 * torch.randn([WDIM], generator=torch.Generator().manual_seed(11)))
    return G


@functools.lru_cache(maxsize=None)
def toy_ops():
    """conv 3 -> 8, tap, maxpool, conv 8 -> 8, tap, avgpool, conv 8 -> 12, tap: float32 values.  Positive biases keep the tapped
    activations away from 0, where the tap's normalisation would amplify every rounding."""
    g = torch.Generator().manual_seed(7)

    def conv(cin, cout):
        return ('conv', 0.3 * torch.randn([cout, cin, 3, 3], generator=g), 0.5 + torch.rand([cout], generator=g))
    return [conv(3, 8), ('tap', torch.rand([8], generator=g)), ('maxpool',), conv(8, 8), ('tap', torch.rand([8], generator=g)),
            ('avgpool',), conv(8, 12), ('tap', torch.rand([12], generator=g))]


def draws(N, z_dim, seed, sampling):
    """The draws of compute_ppl: z0, z1 = the halves of randn([2 N, z_dim]), then t = rand([N]) or zeros, one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn([2 * N, z_dim], generator=g)
    t = torch.rand([N], generator=g) if sampling == 'full' else torch.zeros([N])
    return z[:N], z[N:], t


class _Dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = nets.COMPUTE_DTYPE
        nets.COMPUTE_DTYPE = self.dtype

    def __exit__(self, *exc):
        nets.COMPUTE_DTYPE = self.old


@functools.lru_cache(maxsize=None)
def _generator_as(dtype):
    return copy.deepcopy(toy_generator()).to(dtype)


def _points(fn, a, b, t, dt, dtype):
    """Points in float64; the float32 composition holds them as float32 (rounded once, the kernel's contract)."""
    p = fn(a, b, t, dt)[:, :, 0]
    return torch.from_numpy(p.astype(np.float32) if dtype == torch.float32 else p).to(dtype)


def channel_lpips(img_a, img_b, in_res, dtype):
    """[n, C]: LPIPS of every channel of img_a[p] against img_b[p], the sum over the taps; the channel reduced by area to in_res, repeated
    to three and given the input affine."""
    ops = lc.cast_ops(toy_ops(), dtype)
    cols = []
    for c in range(img_a.shape[1]):
        fed = []
        for img in (img_a, img_b):
            x = img[:, c:c + 1]
            if x.shape[2] != in_res:
                x = F.avg_pool2d(x, x.shape[2] // in_res)
            fed.append(lc.affine(x.repeat(1, 3, 1, 1), PRE_SCALE, PRE_SHIFT))
        cols.append(lc.pair_distance(ops, fed[0], fed[1], 'engine').sum(1))
    return torch.stack(cols, dim=1)


@functools.lru_cache(maxsize=None)
def ppl_oracle(N, eps, space, sampling, psi, seed, in_res, dtype):
    """'dist_per_channel' [N, C] float64 numpy of the composition in `dtype`."""
    G = _generator_as(dtype)
    z0, z1, t = draws(N, WDIM, seed, sampling)
    with _Dtype(dtype), torch.no_grad():
        if space == 'w':
            w = G.mapping(torch.cat([z0, z1]).to(dtype), None, truncation_psi=psi)[:, 0]
            p = _points(lerp_points, w[:N].numpy(), w[N:].numpy(), t.numpy(), [0.0, eps], dtype)
            ws = p.reshape(2 * N, 1, WDIM).repeat(1, G.num_ws, 1)
        else:
            p = _points(slerp_points, z0.numpy(), z1.numpy(), t.numpy(), [0.0, eps], dtype)
            ws = G.mapping(p.reshape(2 * N, WDIM), None, truncation_psi=psi)
        img = G.synthesis(ws, noise_mode='const')
        d = channel_lpips(img[:N], img[N:], in_res, dtype)
    return d.double().numpy() / (eps * eps)


def path_latents(N, L, seed=3, step=0.3):
    """w0 and an 'augmented' w1 = w0 + step * noise, [N, L, w_dim] float32."""
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn([N, L, WDIM], generator=g)
    return w0, w0 + step * torch.randn([N, L, WDIM], generator=g)


def path_oracle_from(w0, w1, segments, in_res, dtype):
    """{'length', 'chord', 'ratio', 'segment_lpips'} float64 numpy of the composition in `dtype`; w0, w1 [N, L, w_dim] float32."""
    G = _generator_as(dtype)
    N, L = w0.shape[0], w0.shape[1]
    S = segments
    with _Dtype(dtype), torch.no_grad():
        p = _points(lerp_points, w0.reshape(N, -1).numpy(), w1.reshape(N, -1).numpy(), np.zeros([N], np.float32),
                    [k / S for k in range(S + 1)], dtype)          # [S + 1, N, L * w_dim]
        ws = p.reshape((S + 1) * N, L, WDIM)
        if L == 1:
            ws = ws.repeat(1, G.num_ws, 1)
        img = G.synthesis(ws, noise_mode='const').reshape(S + 1, N, IMG_CH, RES, RES)
        seg = torch.stack([channel_lpips(img[k], img[k + 1], in_res, dtype).mean(1) for k in range(S)], dim=1).double()
        chord = channel_lpips(img[0], img[S], in_res, dtype).mean(1).double().sqrt()
    length = seg.sqrt().sum(1)
    return {'length': length.numpy(), 'chord': chord.numpy(), 'ratio': (length / chord).numpy(), 'segment_lpips': seg.numpy()}


@functools.lru_cache(maxsize=None)
def path_oracle(N, L, segments, in_res, dtype):
    return path_oracle_from(*path_latents(N, L), segments, in_res, dtype)
