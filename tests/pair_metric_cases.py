"""Case tables, seeded input generators and float64 restatements for the paired image metrics (la_pairmetrics.hip:
la_pair_metrics_f32, la_joint_hist_f32, and their Python layer in latentaugment_amd/metrics.py).  Shared by
test_pair_metric_cases_cpu.py (which proves, without a GPU, that the restatements are right and that every budget is tight) and by
test_hip_pair_metrics.py.  Nothing here reads a file; every input is synthetic and seeded.

The definitions (images float32 [N][C][H][W], one plane at a time):
  window    g[k] = exp(-(k - win//2)^2 / (2 sigma^2)) / sum, float64 on the host, handed over as float32: the float32 values ARE the taps.
  level     mu_x = g*x, s_xx = g*(x x) - mu_x^2 (likewise s_yy, s_xy), 'valid' extent (h-win+1) x (w-win+1);
            cs = (2 s_xy + C2) / (s_xx + s_yy + C2);  ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs;  level outputs: their means.
  pyramid   2 x 2 mean with stride 2 of both images.
  MS-SSIM   prod_{l<levels-1} max(cs_l, 0)^w_l * max(ssim_last, 0)^w_last.
  errors    d = x - y in float32; sum d^2 and sum |d| over the plane.
  histogram bin(v) = min(bins-1, max(0, (int)floorf((v - lo) * scale))) in float32, scale = float32(bins / (hi - lo)).

Float budget (criteria_cases.budget): 4 x the error of the restatement run in float32 on the CPU + 2^-23, where the float32 error is
the LARGER of two float32 summation orders -- separable (rows, then columns, taps ascending) and dense (the win x win window, row
major).  The float32 CPU runs set the budget, never the kernel."""
import functools

import numpy as np

from criteria_cases import EPS32, budget

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win, sigma=1.5):
    k = np.arange(win, dtype=np.float64) - win // 2
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum()


def weights_for(levels, weights=None):
    """float32, as the C entry receives them"""
    if weights is not None:
        return np.asarray(weights, np.float64).astype(np.float32)
    w = np.asarray(MS_WEIGHTS[:levels], np.float64)
    return (w / w.sum() if levels < 5 else w).astype(np.float32)


def constants(data_range=2.0):
    """(C1, C2) as the float32 values the C entry receives"""
    return np.float32((0.01 * data_range) ** 2), np.float32((0.03 * data_range) ** 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements; x, y: [..., h, w]; dtype float64 is the reference, float32 gives the two yardstick orders

def _conv_separable(a, g):
    win = len(g)
    ow, oh = a.shape[-1] - win + 1, a.shape[-2] - win + 1
    rows = np.zeros(a.shape[:-1] + (ow,), a.dtype)
    for k in range(win):
        rows = rows + g[k] * a[..., :, k:k + ow]
    out = np.zeros(a.shape[:-2] + (oh, ow), a.dtype)
    for k in range(win):
        out = out + g[k] * rows[..., k:k + oh, :]
    return out


def _conv_dense(a, g):
    win = len(g)
    ow, oh = a.shape[-1] - win + 1, a.shape[-2] - win + 1
    g2 = (g[:, None] * g[None, :]).astype(a.dtype)
    out = np.zeros(a.shape[:-2] + (oh, ow), a.dtype)
    for i in range(win):
        for j in range(win):
            out = out + g2[i, j] * a[..., i:i + oh, j:j + ow]
    return out


def level_maps(x, y, g, c1, c2, dtype=np.float64, form='separable'):
    """(ssim map, cs map) of one level, every operation in `dtype`"""
    conv = _conv_separable if form == 'separable' else _conv_dense
    x, y, g = x.astype(dtype), y.astype(dtype), np.asarray(g).astype(dtype)
    c1, c2, two = dtype(c1), dtype(c2), dtype(2)
    mx, my = conv(x, g), conv(y, g)
    exx, eyy, exy = conv(x * x, g), conv(y * y, g), conv(x * y, g)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    cs = (two * sxy + c2) / (sxx + syy + c2)
    lum = (two * mx * my + c1) / (mx * mx + my * my + c1)
    return lum * cs, cs


def pool2(a):
    return ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])) * a.dtype.type(0.25)


def combine(ssim, cs, w):
    """MS-SSIM from level means [..., levels] (float64) and float32 weights"""
    w = np.asarray(w, np.float32).astype(np.float64)
    levels = ssim.shape[-1]
    f = np.concatenate([cs[..., :levels - 1], ssim[..., levels - 1:]], axis=-1)
    return np.prod(np.power(np.maximum(f, 0.0), w), axis=-1)


def pair_restate(x, y, win, levels, sigma=1.5, weights=None, data_range=2.0, dtype=np.float64, form='separable'):
    """{'ssim', 'cs': float64 [..., levels] (means of maps evaluated in `dtype`), 'ms': float64 [...]} for x, y [..., H, W] float32"""
    g = window(win, sigma).astype(np.float32)
    c1, c2 = constants(data_range)
    x, y = np.asarray(x, np.float32).astype(dtype), np.asarray(y, np.float32).astype(dtype)
    ssim, cs = [], []
    for lv in range(levels):
        s, c = level_maps(x, y, g, c1, c2, dtype, form)
        ssim.append(s.astype(np.float64).mean(axis=(-2, -1)))
        cs.append(c.astype(np.float64).mean(axis=(-2, -1)))
        if lv + 1 < levels:
            x, y = pool2(x), pool2(y)
    ssim, cs = np.stack(ssim, axis=-1), np.stack(cs, axis=-1)
    return dict(ssim=ssim, cs=cs, ms=combine(ssim, cs, weights_for(levels, weights)))


def error_sums(x, y):
    """(sum d^2, sum |d|, sum of |terms| of each) per plane in extended precision; d = x - y in float32"""
    d = (np.asarray(x, np.float32) - np.asarray(y, np.float32)).astype(np.longdouble)
    return np.stack([(d * d).sum(axis=(-2, -1)), np.abs(d).sum(axis=(-2, -1))], axis=-1).astype(np.float64)


def pair_budgets(x, y, win, levels, **kw):
    """(float64 reference, {'ssim', 'cs', 'ms': budget}, the two float32 restatements)"""
    r64 = pair_restate(x, y, win, levels, dtype=np.float64, **kw)
    sep = pair_restate(x, y, win, levels, dtype=np.float32, form='separable', **kw)
    den = pair_restate(x, y, win, levels, dtype=np.float32, form='dense', **kw)
    bud = {k: max(budget(sep[k], r64[k], EPS32), budget(den[k], r64[k], EPS32)) for k in ('ssim', 'cs', 'ms')}
    return r64, bud, (sep, den)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded images in [-1, 1]: (x, y) float32 [P, C, H, W]

KINDS = ('smooth', 'texture', 'background', 'identical', 'constant', 'negated')


def _smooth(rs, shape):
    P, C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros(shape)
    for _ in range(4):
        fy, fx, ph = rs.uniform(0.02, 0.25, [P, C, 1, 1]), rs.uniform(0.02, 0.25, [P, C, 1, 1]), rs.uniform(0, 6.28, [P, C, 1, 1])
        out += 0.2 * np.sin(fy * yy + fx * xx + ph)
    return out


def images(kind, P, C, H, W, seed=0):
    rs = np.random.RandomState(seed)
    shape = (P, C, H, W)
    if kind == 'smooth':
        x = _smooth(rs, shape) + 0.1
        y = x + 0.05 * _smooth(rs, shape) + 0.02 * rs.standard_normal(shape)
    elif kind == 'texture':
        x = rs.uniform(-1, 1, shape)
        y = 0.7 * x + 0.3 * rs.uniform(-1, 1, shape)
    elif kind == 'background':          # a -1 background with a textured disc, as a medical slice
        yy, xx = np.mgrid[0:H, 0:W]
        disc = ((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2) <= (0.35 * min(H, W)) ** 2
        tex = 0.2 + 0.5 * rs.uniform(-1, 1, shape)
        x = np.where(disc, tex, -1.0)
        y = np.where(disc, tex + 0.1 * rs.uniform(-1, 1, shape), -1.0)
    elif kind == 'identical':
        x = rs.uniform(-1, 1, shape)
        y = x
    elif kind == 'constant':
        x, y = np.full(shape, 0.25), np.full(shape, -0.125)
    elif kind == 'negated':             # y = -x with s_xx far above C2 on every level the product reads: cs < 0
        x = rs.uniform(-1, 1, shape)
        y = -x
    else:
        raise ValueError(kind)
    return np.clip(x, -1, 1).astype(np.float32), np.clip(y, -1, 1).astype(np.float32)


def integer_images(P, C, H, W, seed=0):
    """integers in -3 .. 3: every d, d^2 and every partial sum is exact in float64 whatever the order"""
    rs = np.random.RandomState(seed)
    return rs.randint(-3, 4, [P, C, H, W]).astype(np.float32), rs.randint(-3, 4, [P, C, H, W]).astype(np.float32)


# (H, W, win, C, P, kind): single level.  win 11: one output, one row of outputs across three tiles, one full tile (32 x 32 outputs),
# one output row / column past the tile seam in either direction, both seams with ragged edges, whole tiles only.
SINGLE = [(11, 11, 11, 1, 1, 'texture'), (11, 75, 11, 1, 1, 'smooth'), (42, 42, 11, 1, 1, 'texture'), (43, 42, 11, 2, 1, 'background'),
          (42, 43, 11, 1, 3, 'smooth'), (74, 75, 11, 3, 1, 'texture'), (64, 96, 11, 2, 3, 'background'),
          (8, 8, 1, 1, 1, 'texture'), (8, 8, 3, 2, 1, 'smooth'), (8, 8, 7, 1, 3, 'texture'),
          (33, 34, 1, 3, 1, 'smooth'), (33, 34, 3, 1, 1, 'background'), (33, 34, 7, 2, 3, 'texture'),
          # windows 5 and 9 (no other case selects la_pm_level_kernel<5, .> / <9, .> at the C ABI): the smallest legal plane, H = W = win,
          # and one size above
          (5, 5, 5, 1, 1, 'texture'), (6, 6, 5, 2, 1, 'texture'), (9, 9, 9, 1, 1, 'texture'), (10, 10, 9, 1, 2, 'smooth')]
# (H, W, levels, win, C, P, kind)
MULTI = [(192, 176, 5, 11, 2, 1, 'background'), (176, 352, 5, 11, 1, 2, 'smooth'), (32, 32, 2, 11, 3, 1, 'texture'),
         (48, 80, 3, 3, 1, 3, 'texture'),
         # two levels at windows 1, 5, 7 and 9 (the deeper-level kernel form of each window): the smallest legal plane, H = W = 2 win, and
         # the next legal size above it (H and W are multiples of 2^(levels-1))
         (2, 2, 2, 1, 1, 1, 'texture'), (4, 4, 2, 1, 2, 1, 'smooth'), (10, 10, 2, 5, 1, 1, 'texture'), (12, 12, 2, 5, 2, 1, 'smooth'),
         (14, 14, 2, 7, 1, 1, 'texture'), (16, 16, 2, 7, 1, 2, 'texture'), (18, 18, 2, 9, 1, 1, 'texture'), (20, 20, 2, 9, 1, 2, 'smooth')]
# special inputs, all at 64 x 96, 3 levels, win 11, C 2, P 2
SPECIAL = [(64, 96, 3, 11, 2, 2, k) for k in ('identical', 'constant', 'background', 'negated')]


def case_id(c):
    return '-'.join(str(v) for v in c)


def all_float_cases():
    return [(H, W, 1, win, C, P, kind) for H, W, win, C, P, kind in SINGLE] + MULTI + SPECIAL


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(x, y, float64 reference, budgets, float32 restatements) of a (H, W, levels, win, C, P, kind) case; computed once per process"""
    H, W, levels, win, C, P, kind = case
    x, y = images(kind, P, C, H, W, seed=H * 1000 + W + win)
    for a in (x, y):
        a.setflags(write=False)
    r64, bud, r32 = pair_budgets(x, y, win, levels)
    return x, y, r64, bud, r32


# ---------------------------------------------------------------------------------------------------------------------------------
# joint histogram and mutual information

HIST_BINS = [1, 2, 16, 64]
HIST_NPIX = [1, 63, 64, 65, 16384, 16385, 65539]


def bin_rule(v, lo, scale, bins):
    """the float32 rule, op by op"""
    t = (np.asarray(v, np.float32) - np.float32(lo)) * np.float32(scale)
    assert t.dtype == np.float32
    return np.minimum(bins - 1, np.maximum(0, np.floor(t))).astype(np.int64)


def hist_scale(bins, lo, hi):
    return np.float32(bins / (float(hi) - float(lo)))


def joint_hist_restate(a, b, bins, lo=-1.0, hi=1.0):
    """counts int64 [planes, bins, bins] of a, b [planes, npix]"""
    s = hist_scale(bins, lo, hi)
    k = bin_rule(a, lo, s, bins) * bins + bin_rule(b, lo, s, bins)
    return np.stack([np.bincount(r, minlength=bins * bins).reshape(bins, bins) for r in k])


def hist_values(kind, planes, npix, bins, seed=0, lo=-1.0, hi=1.0):
    """(a, b) float32 [planes, npix]"""
    rs = np.random.RandomState(seed)
    if kind == 'off_edges':          # bin centres +- 0.3 of a bin width: far from every edge in float32 and float64 alike
        width = (hi - lo) / bins
        mk = lambda: lo + (rs.randint(0, bins, [planes, npix]) + 0.5 + rs.uniform(-0.3, 0.3, [planes, npix])) * width      # noqa: E731
        return mk().astype(np.float32), mk().astype(np.float32)
    if kind == 'edges':              # exactly on the edges, one float32 step either side of them, and outside the range
        edges = (lo + np.arange(bins + 1) * ((hi - lo) / bins)).astype(np.float32)
        pool = np.concatenate([edges, np.nextafter(edges, np.float32(10)), np.nextafter(edges, np.float32(-10)),
                               np.float32([lo - 0.5, hi + 0.5, -1e30, 1e30, np.inf, -np.inf])]).astype(np.float32)
        return pool[rs.randint(0, len(pool), [planes, npix])], pool[rs.randint(0, len(pool), [planes, npix])]
    if kind == 'constant':
        return np.full([planes, npix], -1.0, np.float32), np.full([planes, npix], -1.0, np.float32)
    if kind == 'slice':              # mostly background (long runs of one bin pair) with a textured block
        a, b = np.full([planes, npix], -1.0, np.float32), np.full([planes, npix], -1.0, np.float32)
        n0, n1 = npix // 3, max(npix // 3 + 1, 2 * npix // 3)
        a[:, n0:n1] = rs.uniform(-0.9, 0.9, [planes, n1 - n0])
        b[:, n0:n1] = np.clip(0.8 * a[:, n0:n1] + 0.2 * rs.uniform(-0.9, 0.9, [planes, n1 - n0]), -1, 1)
        return a, b
    raise ValueError(kind)


def mi_restate(counts):
    """(MI, NMI) of one [bins, bins] count table, float64, natural logarithms, written as the sums of the definition"""
    c = np.asarray(counts, np.float64)
    n = c.sum()
    pab, pa, pb = c / n, c.sum(1) / n, c.sum(0) / n
    mi = sum(pab[i, j] * np.log(pab[i, j] / (pa[i] * pb[j])) for i in range(c.shape[0]) for j in range(c.shape[1]) if pab[i, j] > 0)
    ent = lambda p: -sum(v * np.log(v) for v in np.ravel(p) if v > 0)      # noqa: E731
    hab = ent(pab)
    if hab == 0:
        return 0.0, 2.0
    return float(mi), float((ent(pa) + ent(pb)) / hab)


def diversity_pairs(n, num_pairs, seed):
    """the documented rule of metrics.msssim_diversity_pairs, restated"""
    total = n * (n - 1) // 2
    if total <= num_pairs:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    rs = np.random.RandomState(seed)
    keep = []
    while len(keep) < num_pairs:
        for a, b in rs.randint(0, n, [num_pairs, 2]).tolist():
            if a != b and (min(a, b), max(a, b)) not in keep and len(keep) < num_pairs:
                keep.append((min(a, b), max(a, b)))
    return keep
