"""The sliced Wasserstein distance restated in numpy, stage by stage, with the case tables and the derived bounds of
test_swd_cases_cpu.py, test_hip_sort.py and test_hip_swd.py.  Nothing here touches a GPU or the library.

Every function computes in the dtype of its input (float64 in the tests; float32 to check what float32 arithmetic can represent), so
the restatement is the definition and not a second implementation of the kernels' arithmetic: the filters are applied as full 5 x 5
sums over mirrored index arrays (the up-sampling really multiplies the inserted zeros), the positions are integer arithmetic on the
Philox words of oracle/noise_ref.py, the directions are its float32 normals divided in float64.

BOUNDS (u = 2^-24, the float32 unit round-off; v = 2^-53).  None of them is a measured figure.
  pyramid     Every G_l and every up(G) is a convex combination of input pixels, so all of them are at most X = max|x| in magnitude.
              down: 25 products and 25 additions of terms whose partial sums stay below X -- at most 26 u X of new error whether or
              not the multiply-adds are fused (the weights k_a k_b / 256 are exact), and the input's error passes through a convex
              combination unamplified: err G_l <= 26 l u X.  up: at most 9 terms, 10 u X of new error plus err G_{l+1}.  The
              subtraction rounds a value of at most 2 X once: 2 u X.  err L_l <= (26 l + 26 (l + 1) + 10 + 2) u X = (52 l + 38) u X,
              and the last level (G itself, 26 l u X) is inside the same expression.  A fused implementation saves one u per stage
              (50 l + 36); the bound is kept at the form that does not depend on fusing.
  mean        a float64 sum of n terms in any order is within (n - 1) v sum|x| of the exact sum; the division adds one rounding:
              |mean - exact| <= n v sum|x| / n.  The tests compare against math.fsum, which is exact.
  std         S = sum (x - m)^2 with m off by dm changes by n dm^2 (the linear term vanishes at the exact mean); every term carries
              two roundings and the sum n - 1 more: relative (n + 2) v; the division and the root (which halves a relative error) add
              one rounding each: |std - exact| / std <= ((n + 3) / 2 + 1) v + dm^2 / (2 var).  The reference's squares are rounded before
              math.fsum adds them exactly, and its division and root round too: 3 v more.
  la_swd_f32  a float32 dot product of length D in any order, fused or not, is within D u sum|a_k d_k| of the exact one and the stored
              value rounds once more.  sum|a_k d_k| <= |a|_2 |d|_2 <= sqrt(D) max|a| |d|_2 is what always holds; the form asserted,
              (D + 1) u (max|a| + max|b|) |d|_2 with max over the whole set, is the one the issue states and is sqrt(D) tighter than
              that worst case, so passing it says more, not less.  Sorting is 1-Lipschitz in the max norm and the mean of |a - b|
              moves by at most the sum of the two sides' errors; the float64 sum's own error is below 2^-40 of these.
  end to end  see composed_bound().
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import noise_ref  # noqa: E402

U32 = 2.0 ** -24
U64 = 2.0 ** -53
STREAM_POS = 0x53574450          # LA_RNG_STREAM_SWD_POS
STREAM_DIR = 0x53574444          # LA_RNG_STREAM_SWD_DIR
LEVEL_DIR_STRIDE = 1 << 20       # metrics.py: global direction index = level * 2^20 + j
K5 = (1.0, 4.0, 6.0, 4.0, 1.0)
DIR_TOL = 2e-5                   # the directions stage: per component, numerator and norm each carry the normals' 1e-5


# ---------------------------------------------------------------------------------------------------------------- pyramid
def mirror_index(i, n):
    """d c b | a b c d | c b a: index i of a line of n >= 2 samples, any distance"""
    period = 2 * (n - 1)
    i = np.mod(np.asarray(i), period)
    return np.where(i < n, i, period - i)


def _filter5(x, rows, cols, gain):
    """sum over the 25 taps of k_a k_b gain / 256 * x[..., rows[a], cols[b]]; rows, cols: [5][out] index arrays"""
    dt = x.dtype.type
    acc = np.zeros(x.shape[:-2] + (rows.shape[1], cols.shape[1]), dtype=x.dtype)
    for a in range(5):
        xr = x[..., rows[a], :]
        for b in range(5):
            acc = acc + dt(K5[a] * K5[b] * gain / 256.0) * xr[..., :, cols[b]]
    return acc


def down(x):
    H, W = x.shape[-2:]
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2
    rows = np.stack([mirror_index(2 * np.arange(H // 2) + d - 2, H) for d in range(5)])
    cols = np.stack([mirror_index(2 * np.arange(W // 2) + d - 2, W) for d in range(5)])
    return _filter5(x, rows, cols, 1.0)


def up(c):
    h, w = c.shape[-2:]
    z = np.zeros(c.shape[:-2] + (2 * h, 2 * w), dtype=c.dtype)
    z[..., ::2, ::2] = c
    rows = np.stack([mirror_index(np.arange(2 * h) + d - 2, 2 * h) for d in range(5)])
    cols = np.stack([mirror_index(np.arange(2 * w) + d - 2, 2 * w) for d in range(5)])
    return _filter5(z, rows, cols, 4.0)


def num_levels(H, W, min_resolution=16):
    n, r = 1, min(H, W)
    while r % 2 == 0 and H % 2 == 0 and W % 2 == 0 and r // 2 >= min_resolution:
        n, r, H, W = n + 1, r // 2, H // 2, W // 2
    return n


def pyramid(x, levels):
    g = [x]
    for _ in range(levels - 1):
        g.append(down(g[-1]))
    return [g[l] - up(g[l + 1]) for l in range(levels - 1)] + [g[-1]]


def reconstruct(levels):
    x = levels[-1]
    for lap in levels[-2::-1]:
        x = lap + up(x)
    return x


def pyramid_bound(level, xmax):
    return (52 * level + 38) * U32 * xmax


# ---------------------------------------------------------------------------------------------------------------- descriptors
def positions(n, img0, level, per_image, H, W, nhood, seed):
    """(x0, y0) int64 [n][per_image]"""
    j = np.arange(per_image, dtype=np.uint32)[None, :].repeat(n, 0)
    i = (np.arange(n, dtype=np.uint64) + np.uint64(img0)).astype(np.uint32)[:, None].repeat(per_image, 1)
    w = noise_ref.philox4x32_10(j, i, np.uint32(STREAM_POS), np.uint32(level), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x0 = (w[0].astype(np.uint64) * np.uint64(W - nhood + 1)) >> np.uint64(32)
    y0 = (w[1].astype(np.uint64) * np.uint64(H - nhood + 1)) >> np.uint64(32)
    return x0.astype(np.int64), y0.astype(np.int64)


def descriptors(img, img0, level, nhood, per_image, seed):
    """[n * per_image][C nhood^2] in (channel, y, x) order, the dtype of img"""
    n, C, H, W = img.shape
    x0, y0 = positions(n, img0, level, per_image, H, W, nhood, seed)
    out = np.empty([n, per_image, C, nhood, nhood], dtype=img.dtype)
    for i in range(n):
        for j in range(per_image):
            out[i, j] = img[i, :, y0[i, j]:y0[i, j] + nhood, x0[i, j]:x0[i, j] + nhood]
    return out.reshape(n * per_image, C * nhood * nhood)


def channel_stats(desc, C):
    M, D = desc.shape
    x = desc.reshape(M, C, D // C)
    return x.mean(axis=(0, 2)), x.std(axis=(0, 2))


def channel_stats_exact(desc, C):
    """(mean, std, sum|x|) per channel with math.fsum: exact sums of the float64 values (the squares are rounded once each)"""
    M, D = desc.shape
    x = np.asarray(desc, np.float64).reshape(M, C, D // C)
    mean, std, sabs = np.empty(C), np.empty(C), np.empty(C)
    for c in range(C):
        v = x[:, c, :].ravel()
        mean[c] = math.fsum(v) / v.size
        std[c] = math.sqrt(math.fsum((v - mean[c]) ** 2) / v.size)
        sabs[c] = math.fsum(np.abs(v))
    return mean, std, sabs


def mean_bound(n, sabs):
    return n * U64 * sabs / n


def std_rel_bound(n, dm, var):
    return ((n + 3) / 2 + 1 + 3) * U64 + dm * dm / (2 * var)


def normalize(desc, mean, std, C):
    M, D = desc.shape
    x = desc.reshape(M, C, D // C)
    return ((x - mean[None, :, None]) / std[None, :, None]).reshape(M, D)


# ---------------------------------------------------------------------------------------------------------------- directions
def raw_normals(ndirs, D, dir0, seed):
    return noise_ref.noise_normal(ndirs, D, seed, STREAM_DIR, row0=dir0)


def directions(ndirs, D, dir0, seed):
    """float64 [ndirs][D]: the float32 normals divided by their float64 norm (the device then rounds once to float32)"""
    z = raw_normals(ndirs, D, dir0, seed).astype(np.float64)
    return z / np.sqrt((z * z).sum(axis=1, keepdims=True))


# ---------------------------------------------------------------------------------------------------------------- sort and W1
def key_image(bits):
    bits = np.asarray(bits, np.uint32)
    return np.where(bits >> np.uint32(31), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def key_bits(image):
    image = np.asarray(image, np.uint32)
    return np.where(image >> np.uint32(31), image ^ np.uint32(0x80000000), ~image).astype(np.uint32)


def sort_columns_bits(bits):
    """uint32 bit patterns [ncols][M] -> the patterns of every row in the order of their images"""
    return key_bits(np.sort(key_image(bits), axis=1))


def w1(a, b, dirs):
    """[ndirs]: mean_i |sort(a d_j)_i - sort(b d_j)_i| in the dtype of a"""
    d = np.asarray(dirs, a.dtype)
    pa, pb = np.sort(a @ d.T, axis=0), np.sort(b @ d.T, axis=0)
    return np.abs(pa - pb).sum(axis=0) / a.dtype.type(a.shape[0])


def w1_bound(D, amax, bmax, dirs):
    return (D + 1) * U32 * (amax + bmax) * np.sqrt((np.asarray(dirs, np.float64) ** 2).sum(axis=1))


def swd_features(a, b, num_dirs, seed):
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    d = directions(num_dirs, a.shape[1], 0, seed).astype(np.float32).astype(np.float64)
    return float(w1(a, b, d).mean())


def swd_images(real, gen, nhood_size=7, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, min_resolution=16, seed=0):
    """({'swd_<res>', 'swd_avg'} times 1e3, details) of two [n, C, H, W] float64 sets, every stage in float64"""
    n, C, H, W = real.shape
    L = num_levels(H, W, min_resolution)
    ndirs = dir_repeats * dirs_per_repeat
    D = C * nhood_size ** 2
    out, details = {}, []
    pr, pg = pyramid(real, L), pyramid(gen, L)
    for l in range(L):
        sides = []
        for lv in (pr[l], pg[l]):
            d = descriptors(lv, 0, l, nhood_size, nhoods_per_image, seed)
            mean, std = channel_stats(d, C)
            sides.append(dict(raw=d, mean=mean, std=std, desc=normalize(d, mean, std, C)))
        dirs = directions(ndirs, D, l * LEVEL_DIR_STRIDE, seed)
        w = w1(sides[0]['desc'], sides[1]['desc'], dirs)
        out[f'swd_{lv.shape[-2]}'] = float(w.mean()) * 1e3
        details.append(dict(w1=w, dirs=dirs, sides=sides, xmax=max(float(np.abs(real).max()), float(np.abs(gen).max()))))
    out['swd_avg'] = float(np.mean([out[k] for k in out]))
    return out, details


def composed_bound(details, level, C):
    """|w1_j(device) - w1_j(restatement)| for every direction of one level of swd_images, composed from the stage bounds:
      e     the pyramid's bound on a descriptor value (the gather copies);
      mean  moves by at most e, and std by at most e (std is 1-Lipschitz in the rms of a perturbation); float64 errors are below
            1e-12 of these and are covered by the factor 1.001;
      norm  n = (d - m) / s:  |n' - n| <= (2 e + |n| e) / (s - e), then one float32 rounding u |n'|;
      proj  |n'.d' - n.d| <= |n' - n|_2 |d'|_2 + |n|_2 |d' - d|_2 with |d' - d|_2 <= sqrt(D) DIR_TOL (the directions stage's tolerance, plus
            its float32 rounding u), |d'|_2 <= 1 + 2^-22, and the float32 dot product's (D + 1) u |n'|_2 |d'|_2;
      w1    sorting is 1-Lipschitz in the max norm; the mean of |a - b| moves by at most the sum of the two sides' bounds."""
    det = details[level]
    e = pyramid_bound(level, det['xmax'])
    total = 0.0
    for side in det['sides']:
        nref = side['desc']
        D = nref.shape[1]
        s = float(side['std'].min())
        assert s > 10 * e
        nmax = float(np.abs(nref).max())
        dn = (2 + nmax) * e / (s - e) * 1.001
        dn = dn + U32 * (nmax + dn)
        row2 = float(np.sqrt((nref ** 2).sum(axis=1)).max())
        dd = math.sqrt(D) * (DIR_TOL + U32)
        total += math.sqrt(D) * dn * (1 + 2.0 ** -22) + row2 * dd + (D + 1) * U32 * (row2 + math.sqrt(D) * dn) * (1 + 2.0 ** -22)
    return total


# ---------------------------------------------------------------------------------------------------------------- case tables
SORT_M = ('1', '2', '63', '65', 'T-1', 'T', 'T+1', '2T', '2T+1', '3T+5', '5T-3', '8T')
SORT_NCOLS = (1, 3, 130)
SORT_CONTENTS = ('normal', 'duplicates', 'equal', 'sorted', 'reversed', 'special')


def sort_m(name, T):
    """a size named in SORT_M / SWD_EXACT_M for the library's tile of T keys"""
    return {'1': 1, '2': 2, '5': 5, '63': 63, '65': 65, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T': 2 * T, '2T+1': 2 * T + 1, '3T+5': 3 * T + 5,
            '5T-3': 5 * T - 3, '8T': 8 * T}[name]


def sort_keys(content, ncols, M, seed):
    """float32 [ncols][M] without a NaN"""
    rng = np.random.RandomState(seed)
    if content == 'normal':
        k = rng.standard_normal([ncols, M])
    elif content == 'duplicates':
        k = rng.randint(-3, 4, [ncols, M]) * 0.5
    elif content == 'equal':
        k = np.full([ncols, M], 1.25)
    elif content == 'sorted':
        k = np.sort(rng.standard_normal([ncols, M]), axis=1)
    elif content == 'reversed':
        k = -np.sort(rng.standard_normal([ncols, M]), axis=1)
    else:
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 3.4e38, -3.4e38, 1.17549435e-38], np.float32)
        k = pool[rng.randint(0, pool.size, [ncols, M])]
    return np.ascontiguousarray(k, np.float32)


PYR_EXACT_SHAPES = ((16, 16), (32, 24), (64, 16))          # three levels: grids 2^-8, 2^-14, 2^-22 with values under 8
PYR_PLANES = (1, 3)
SWD_EXACT_D = (1, 7, 98, 147, 200)
SWD_EXACT_M = ('5', 'T-1', 'T+1', '3T+5')
SWD_EXACT_NDIRS = (1, 5, 129)


def integer_images(planes, H, W, seed):
    return np.random.RandomState(seed).randint(-4, 5, [planes, H, W]).astype(np.float64)
