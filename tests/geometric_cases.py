"""Case tables of the GeometricAugment tests and a numpy restatement of what the kernels compute (include/latentaug_hip.h
'GeometricAugment', DESIGN 'GeometricAugment'): the sampling rule S for the three padding modes, the affine warp, the separable
zero-border blur and the elastic warp.

Everything runs in the dtype of its `dt` argument: float64 for expected values (tests/test_geometric_cpu.py pins it to torch's CPU
grid_sample / conv2d in float64 within 1e-12), float32 as the yardstick of a float32 computation's error.  x is the column index, y the
row index, pixel centres at integer coordinates.
"""
import numpy as np

MODES = ('zeros', 'border', 'reflection')
MODE_IDS = {'zeros': 0, 'border': 1, 'reflection': 2}
PMAX = 2.0 ** 23

# (H, W) of the GPU tests: one 256-pixel block / one 16 x 64 field tile or less (5x7, 16x16), several with a ragged edge (33x70), whole (64x64)
SHAPES = [(5, 7), (16, 16), (33, 70), (64, 64)]
# (B, C, apply flags): mixed flags wherever there is more than one sample
BATCHES = [(1, 1, (1,)), (3, 2, (1, 0, 1)), (5, 3, (0, 1, 1, 0, 1))]
# exact blur: (H, W) smaller than the half-width of 31, several tiles with a ragged edge, more than one tile row and column
BLUR_SHAPES = [(16, 16), (33, 70), (96, 80)]
BLUR_NTAPS = [1, 3, 63]


def axis(p, size, mode, dt=np.float64):
    """One axis (csrc/la_geom_index.h la_geom_axis): lower neighbour i0, weights of i0 and i0 + 1, whether each is addressable."""
    p = np.asarray(p).astype(dt)
    with np.errstate(invalid='ignore', over='ignore'):
        ok = np.abs(p) <= dt(PMAX)
    ps = np.where(ok, p, dt(0)).astype(dt)
    if mode == 'zeros':
        ok = ok & (ps >= dt(-1)) & (ps < dt(size))
        ps = np.where(ok, ps, dt(0)).astype(dt)
        f = np.floor(ps)
        i0 = f.astype(np.int64)
        in0, in1 = ok & (i0 >= 0), ok & (i0 + 1 < size)
        w0 = np.where(in0, (f + dt(1)) - ps, dt(0)).astype(dt)
        w1 = np.where(in1, ps - f, dt(0)).astype(dt)
        return i0, w0, w1, in0, in1
    assert mode in ('border', 'reflection'), mode
    if size == 1:
        ps = np.zeros_like(ps)
    else:
        if mode == 'reflection':
            span = dt(size)
            d = np.abs(ps + dt(0.5))
            r = np.fmod(d, span)
            flips = ((d - r) / span).astype(np.int64)
            ps = np.where(flips & 1, (span - r) - dt(0.5), r - dt(0.5)).astype(dt)
        ps = np.clip(ps, dt(0), dt(size - 1)).astype(dt)
    f = np.floor(ps)
    i0 = np.where(ok, f.astype(np.int64), 0)
    in0, in1 = ok, ok & (i0 + 1 < size)
    w0 = np.where(in0, (f + dt(1)) - ps, dt(0)).astype(dt)
    w1 = np.where(in1, ps - f, dt(0)).astype(dt)
    return i0, w0, w1, in0, in1


def sample(x, px, py, mode, dt=np.float64):
    """S: x [B, C, H, W], positions px, py [B, Ho, Wo] -> [B, C, Ho, Wo]; the corners nw, ne, sw, se are added in this order."""
    x = np.asarray(x).astype(dt)
    B, C, H, W = x.shape
    ix, wx0, wx1, inx0, inx1 = axis(px, W, mode, dt)
    iy, wy0, wy1, iny0, iny1 = axis(py, H, mode, dt)
    b = np.arange(B)[:, None, None]
    y = np.zeros((B, C) + ix.shape[1:], dt)
    for r, c, w, inside in ((iy, ix, wx0 * wy0, inx0 & iny0), (iy, ix + 1, wx1 * wy0, inx1 & iny0),
                            (iy + 1, ix, wx0 * wy1, inx0 & iny1), (iy + 1, ix + 1, wx1 * wy1, inx1 & iny1)):
        v = x[b, :, np.where(inside, r, 0), np.where(inside, c, 0)]      # [B, Ho, Wo, C]
        v = np.moveaxis(np.where(inside[..., None], v, dt(0)), -1, 1)
        y = (y + (w.astype(dt)[:, None] * v).astype(dt)).astype(dt)
    return y


def _keep(x, y, apply, dt):
    apply = np.asarray(apply).astype(bool)
    return np.where(apply[:, None, None, None], y, np.asarray(x).astype(dt))


def affine_positions(minv, H, W, dt=np.float64):
    """px, py [B, H, W] of Minv (x, y, 1), from the float32 matrix, in dt: m0 x + (m1 y + m2)."""
    m = np.asarray(minv, dtype=np.float32).reshape(-1, 6).astype(dt)[:, :, None, None]
    xs = np.arange(W).astype(dt)[None, None, :]
    ys = np.arange(H).astype(dt)[None, :, None]
    px = (m[:, 0] * xs + (m[:, 1] * ys + m[:, 2]).astype(dt)).astype(dt)
    py = (m[:, 3] * xs + (m[:, 4] * ys + m[:, 5]).astype(dt)).astype(dt)
    return px, py


def warp_affine(x, minv, apply, mode, dt=np.float64):
    H, W = np.asarray(x).shape[2:]
    px, py = affine_positions(minv, H, W, dt)
    return _keep(x, sample(x, px, py, mode, dt), apply, dt)


def blur(noise, taps, alpha=(1.0, 1.0), dt=np.float64):
    """noise [B, 2, H, W] -> alpha_p * (taps along y) (taps along x) noise, zero border, a correlation; rows first, taps ascending."""
    n = np.asarray(noise).astype(dt)
    t = np.asarray(taps).astype(dt)
    R = len(t) // 2
    B, P, H, W = n.shape
    pad = np.zeros((B, P, H + 2 * R, W + 2 * R), dt)
    pad[:, :, R:R + H, R:R + W] = n
    rows = np.zeros((B, P, H + 2 * R, W), dt)
    for k in range(len(t)):
        rows = (rows + (t[k] * pad[:, :, :, k:k + W]).astype(dt)).astype(dt)
    out = np.zeros((B, P, H, W), dt)
    for k in range(len(t)):
        out = (out + (t[k] * rows[:, :, k:k + H, :]).astype(dt)).astype(dt)
    a = np.asarray(alpha).astype(dt).reshape(1, 2, 1, 1)
    return (a * out).astype(dt)


def elastic_positions(disp, dt=np.float64):
    """px, py [B, H, W] of the displaced normalised grid: g = clamp(-1 + 2 i / (size - 1) + d, -1, 1), 0 on a one-pixel axis."""
    d = np.asarray(disp).astype(dt)
    H, W = d.shape[2:]
    out = []
    for plane, size, shape in ((0, W, (1, 1, W)), (1, H, (1, H, 1))):
        if size == 1:
            g = np.zeros(d[:, plane].shape, dt)
        else:
            base = (dt(-1) + (dt(2) * np.arange(size).astype(dt)) / dt(size - 1)).astype(dt).reshape(shape)
            g = np.clip((base + d[:, plane]).astype(dt), dt(-1), dt(1)).astype(dt)      # (np.clip keeps NaN)
        out.append((((g + dt(1)) * dt(size) - dt(1)) / dt(2)).astype(dt))
    return out[0], out[1]


def warp_elastic(x, disp, apply, mode, dt=np.float64):
    px, py = elastic_positions(disp, dt)
    return _keep(x, sample(x, px, py, mode, dt), apply, dt)


def pipeline(x, minv, warp_flags, noise, taps, alpha, elastic_flags, dt=np.float64, mode='reflection'):
    """The plugin's batch: flip + affine as one resampling, then the elastic warp of that result (both only where flagged)."""
    y = warp_affine(x, minv, warp_flags, mode, dt) if np.any(warp_flags) else np.asarray(x).astype(dt)
    if np.any(elastic_flags):
        y = warp_elastic(y, blur(noise, taps, alpha, dt), elastic_flags, mode, dt)
    return y


def int_image(rng, B, C, H, W):
    """Integer-valued pixels in [-8, 8]: every bilinear sum with weights 0, 0.5 and 1 is exact in float32."""
    return rng.integers(-8, 9, size=(B, C, H, W)).astype(np.float64)


def translation(tx, ty, B=1):
    """[B, 6] inverse map of a shift of the picture by (tx, ty): position = (x - tx, y - ty)."""
    return np.tile(np.array([1, 0, -tx, 0, 1, -ty], np.float32), (B, 1))


def ulp32(v):
    return float(np.spacing(np.float32(max(float(v), np.finfo(np.float32).tiny))))
