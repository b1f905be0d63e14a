"""Case table of the grid_sample / fma tests and a numpy restatement of both ops.

The restatement follows include/latentaug_hip.h ('grid_sample and fma'): 2-D, bilinear, zero padding, align_corners=False; pixel position
((g + 1) * size - 1) / 2; a position outside [-1, size) -- NaN and infinities included -- has zero weights and touches nothing.  It runs
in the dtype of its `dt` argument: float64 for expected values (tests/test_grid_sample_cpu.py pins it to the reference's golden within
1e-12), float32 as the yardstick of a float32 sum's error.

tests/golden/make_golden_grid_sample.py builds its inputs from the same table, so the golden file and the GPU tests agree on them.
"""
import numpy as np

# (name, N, C, H, W, Ho, Wo, kind of grid, seed, float16-exact inputs)
#   H x W in {4x8, 5x7, 1x1}, Ho x Wo in {3x5, 9x2, 1x130} and 2x130 (260 outputs per image: more than one 256-thread block), C in {1, 3, 5}
GS_CASES = [
    ('ident_c3', 2, 3, 4, 8, 3, 5, 'identity', 1, False),
    ('ident_wide_c1', 2, 1, 4, 8, 1, 130, 'identity', 2, False),
    ('rot_c5', 2, 5, 5, 7, 9, 2, 'rotation', 3, False),
    ('rot_wide_c3', 2, 3, 4, 8, 1, 130, 'rotation', 4, False),
    ('band_c3', 2, 3, 5, 7, 3, 5, 'band', 5, False),
    ('outside_c1', 2, 1, 4, 8, 9, 2, 'outside', 6, False),
    ('pixel_c5', 2, 5, 1, 1, 3, 5, 'random', 7, False),
    ('blocks_c3', 2, 3, 5, 7, 2, 130, 'random', 8, False),
    ('h_rot_c3', 2, 3, 4, 8, 3, 5, 'rotation', 11, True),
    ('h_band_c5', 2, 5, 5, 7, 9, 2, 'band', 12, True),
    ('h_wide_c1', 2, 1, 4, 8, 1, 130, 'random', 13, True),
    ('h_blocks_c3', 2, 3, 5, 7, 2, 130, 'random', 14, True),
]
GS_NAMES = [c[0] for c in GS_CASES]
FRAC_MARGIN = 1e-3      # px: every drawn position's fractional part stays this far from 0 and 1 (dgrid jumps where floor flips)

# (name, shape of a, of b, of c, seed)
FMA_CASES = [
    ('noise', (2, 3, 4, 4), (2, 3, 1, 1), (1, 1, 4, 4), 21),      # the SG2 noise form
    ('low_rank', (3, 4, 4), (4,), (2, 1, 1, 1), 22),
    ('full', (2, 3, 4, 5), (2, 3, 4, 5), (2, 3, 4, 5), 23),
    ('scalar_c', (2, 3, 4, 4), (1, 3, 1, 4), (), 24),
    ('rows', (2, 3, 8, 32), (2, 3, 1, 1), (1, 1, 8, 32), 25),     # dc has 256 outputs with the inner axis kept: the one-thread-per-output sum
]
FMA_SECOND_ORDER = 'noise'


def _round_to(a, half):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float16 if half else np.float32).astype(np.float64)


def positions(grid, H, W):
    """float64 pixel positions (px, py) of a grid."""
    g = np.asarray(grid, dtype=np.float64)
    return ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2


def frac_ok(grid, H, W):
    px, py = positions(grid, H, W)
    ok = True
    for p in (px, py):
        fr = p - np.floor(p)
        ok &= bool(((fr >= FRAC_MARGIN) & (fr <= 1 - FRAC_MARGIN)).all())
    return ok


def _draw_grid(kind, rng, N, H, W, Ho, Wo):
    ys = (2 * np.arange(Ho) + 1) / Ho - 1
    xs = (2 * np.arange(Wo) + 1) / Wo - 1
    base = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=-1)      # affine_grid of the identity, align_corners=False
    if kind == 'identity':
        return np.broadcast_to(base, (N, Ho, Wo, 2)).copy()
    if kind == 'rotation':      # a small rotation plus a shift, per sample
        out = np.empty((N, Ho, Wo, 2))
        for n in range(N):
            a = rng.uniform(-0.3, 0.3)
            t = rng.uniform(-0.2, 0.2, size=2)
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            out[n] = base @ rot.T + t
        return out
    if kind == 'band':          # positions in the half-pixel bands [-1, 0) and (size - 1, size) on at least one axis
        px = np.where(rng.random((N, Ho, Wo)) < 0.5, rng.uniform(-1, 0, (N, Ho, Wo)), rng.uniform(W - 1, W, (N, Ho, Wo)))
        py = np.where(rng.random((N, Ho, Wo)) < 0.5, rng.uniform(-1, 0, (N, Ho, Wo)), rng.uniform(H - 1, H, (N, Ho, Wo)))
        inside = rng.random((N, Ho, Wo)) < 0.3      # some with the other axis well inside
        px = np.where(inside, rng.uniform(0, max(W - 1, 1e-9), (N, Ho, Wo)), px)
        return np.stack([(2 * px + 1) / W - 1, (2 * py + 1) / H - 1], axis=-1)
    if kind == 'outside':       # wholly outside the image: |g| in [1.6, 3] on at least the x axis
        sx = np.where(rng.random((N, Ho, Wo)) < 0.5, -1.0, 1.0)
        gx = sx * rng.uniform(1.6, 3.0, (N, Ho, Wo))
        gy = rng.uniform(-3.0, 3.0, (N, Ho, Wo))
        return np.stack([gx, gy], axis=-1)
    assert kind == 'random'
    return rng.uniform(-1.3, 1.3, (N, Ho, Wo, 2))


def gs_inputs(case):
    """x, grid, dy, ddx of a case as float64 arrays holding float32-exact (float16-exact for the `half` cases) values.  The grid is
    redrawn until every position, as the rounded grid value gives it, keeps FRAC_MARGIN from the next integer."""
    name, N, C, H, W, Ho, Wo, kind, seed, half = case
    rng = np.random.default_rng(seed)
    x = _round_to(rng.standard_normal((N, C, H, W)), half)
    dy = _round_to(rng.standard_normal((N, C, Ho, Wo)), half)
    ddx = _round_to(rng.standard_normal((N, C, H, W)), half)
    grid = _round_to(_draw_grid(kind, rng, N, H, W, Ho, Wo), half)
    for _ in range(1000):
        bad = ~_elementwise_ok(grid, H, W)
        if not bad.any():
            return dict(x=x, grid=grid, dy=dy, ddx=ddx)
        assert kind != 'identity', f'{name}: the identity grid of this shape has a position within {FRAC_MARGIN} px of an integer'
        grid[bad] = _round_to(_draw_grid(kind, rng, N, H, W, Ho, Wo), half)[bad]      # only the offending entries are redrawn
    raise AssertionError(name)


def _elementwise_ok(grid, H, W):
    px, py = positions(grid, H, W)
    ok = np.ones(px.shape, bool)
    for p in (px, py):
        fr = p - np.floor(p)
        ok &= (fr >= FRAC_MARGIN) & (fr <= 1 - FRAC_MARGIN)
    return ok


def fma_inputs(case):
    name, sa, sb, sc, seed = case
    rng = np.random.default_rng(seed)
    a, b, c = (_round_to(rng.standard_normal(s), False) for s in (sa, sb, sc))
    shape = np.broadcast_shapes(sa, sb, sc)
    dy = _round_to(rng.standard_normal(shape), False)
    return dict(a=a, b=b, c=c, dy=dy)


# ------------------------------------------------------------------------------------------------------------ restatement
def gs_axis(g, size, dt=np.float64):
    """One axis (csrc/la_grid_sample_index.h la_gs_axis): lower neighbour i0, weights of i0 and i0 + 1, whether each is a pixel."""
    g = np.asarray(g).astype(dt)
    with np.errstate(invalid='ignore', over='ignore'):
        p = ((g + dt(1)) * dt(size) - dt(1)) / dt(2)
        ok = (p >= dt(-1)) & (p < dt(size))
    ps = np.where(ok, p, dt(0))
    f = np.floor(ps)
    i0 = f.astype(np.int64)
    in0, in1 = ok & (i0 >= 0), ok & (i0 + 1 < size)
    w0 = np.where(in0, (f + dt(1)) - ps, dt(0)).astype(dt)      # (a neighbour outside the image: weight 0)
    w1 = np.where(in1, ps - f, dt(0)).astype(dt)
    return i0, w0, w1, in0, in1


def _corners(grid, H, W, dt):
    ix, wx0, wx1, inx0, inx1 = gs_axis(grid[..., 0], W, dt)
    iy, wy0, wy1, iny0, iny1 = gs_axis(grid[..., 1], H, dt)
    # nw, ne, sw, se: (row, column, weight, inside)
    cs = [(iy, ix, wx0 * wy0, inx0 & iny0), (iy, ix + 1, wx1 * wy0, inx1 & iny0),
          (iy + 1, ix, wx0 * wy1, inx0 & iny1), (iy + 1, ix + 1, wx1 * wy1, inx1 & iny1)]
    return cs, (wx0, wx1, wy0, wy1)


def _gather(x, r, c, inside):
    """x[n, :, r, c] where inside, else 0: [N, C, Ho, Wo]."""
    N = x.shape[0]
    n = np.arange(N)[:, None, None]
    v = x[n, :, np.where(inside, r, 0), np.where(inside, c, 0)]      # [N, Ho, Wo, C]
    return np.moveaxis(v * inside[..., None], -1, 1)


def gs_forward(x, grid, dt=np.float64):
    x, grid = np.asarray(x).astype(dt), np.asarray(grid).astype(dt)
    H, W = x.shape[2:]
    cs, _ = _corners(grid, H, W, dt)
    y = np.zeros((x.shape[0], x.shape[1]) + grid.shape[1:3], dt)
    for r, c, w, inside in cs:
        y = y + (w[:, None] * _gather(x, r, c, inside)).astype(dt)
    return y


def gs_backward(dy, x, grid, dt=np.float64):
    """(dx, dgrid) of <dy, grid_sample(x, grid)>; the terms of dgrid in the order of torch's grid_sampler_2d_backward."""
    dy, x, grid = (np.asarray(t).astype(dt) for t in (dy, x, grid))
    N, C, H, W = x.shape
    cs, (wx0, wx1, wy0, wy1) = _corners(grid, H, W, dt)
    dx = np.zeros_like(x)
    n = np.broadcast_to(np.arange(N)[:, None, None, None], dy.shape)
    ch = np.broadcast_to(np.arange(C)[None, :, None, None], dy.shape)
    v = []
    for r, c, w, inside in cs:
        m = np.broadcast_to(inside[:, None], dy.shape)
        rr = np.broadcast_to(np.where(inside, r, 0)[:, None], dy.shape)
        cc = np.broadcast_to(np.where(inside, c, 0)[:, None], dy.shape)
        np.add.at(dx, (n[m], ch[m], rr[m], cc[m]), (w[:, None] * dy)[m])
        v.append(_gather(x, r, c, inside))
    e = lambda t: t[:, None]      # noqa: E731
    gix = (-v[0] * e(wy0) * dy + v[1] * e(wy0) * dy - v[2] * e(wy1) * dy + v[3] * e(wy1) * dy).sum(axis=1)
    giy = (-v[0] * e(wx0) * dy - v[1] * e(wx1) * dy + v[2] * e(wx0) * dy + v[3] * e(wx1) * dy).sum(axis=1)
    dgrid = np.stack([gix * (dt(W) / dt(2)), giy * (dt(H) / dt(2))], axis=-1).astype(dt)
    return dx, dgrid


def unbroadcast(x, shape):
    """fma.py:49-58."""
    shape = tuple(shape)
    extra = x.ndim - len(shape)
    dims = tuple(i for i in range(x.ndim) if x.shape[i] > 1 and (i < extra or shape[i - extra] == 1))
    if dims:
        x = x.sum(axis=dims, keepdims=True)
    return x.reshape(shape)


def fma_all(a, b, c, dy, dt=np.float64):
    """y, da, db, dc of fma(a, b, c) with the incoming gradient dy, every product and sum in dt."""
    a, b, c, dy = (np.asarray(t).astype(dt) for t in (a, b, c, dy))
    y = (a * b + c).astype(dt)
    return dict(y=y, da=unbroadcast((dy * b).astype(dt), a.shape), db=unbroadcast((dy * a).astype(dt), b.shape), dc=unbroadcast(dy, c.shape))
