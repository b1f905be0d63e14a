"""Case tables, seeded inputs and float64 restatements for the per-sample neighbour queries (la_knn_f32, la_realism_f32,
metrics.knn_from_features / compute_realism_from_features / compute_authenticity_from_features).  Shared by test_knn_cases_cpu.py
(which proves, without a GPU, that the restatement is right and that the cases reach what they claim) and test_hip_knn.py.  Helpers
only; nothing here reads a file.

Definitions (include/latentaug_hip.h): queries Q [nq][D], bank X [nx][D], float32.
  d2(q, x)   the squared Euclidean distance, here in DIFFERENCE form sum_d (q_d - x_d)^2 (the library uses |q|^2 + |x|^2 - 2 q.x): the
             differences of these inputs are exact in float64, and the sum of squares runs in numpy's longdouble (64 mantissa bits on
             x86: its error is below 2^-10 of the bound B below) or, where longdouble is no wider than double, in math.fsum.
  knn        per query the k smallest d2 in the order (d2, index), by a stable sort; exclude_self drops bank row i for query i; slots
             beyond the number of candidates are (+inf, -1).
  realism    score2[j] = max over the kept i of radius2[i] / d2(q_j, x_i) (the quotient in float64, d2 == 0 -> +inf), arg the lowest
             maximising i; no kept sphere: (0, -1).  From features: radius2[i] = d2 of real i to its nhood_size-th nearest OTHER real,
             kept are the ceil(keep_fraction nr) smallest radii (ties by lower index), realism = sqrt(score2).
  authentic  for generated j with nearest real i*: d_gen = dist(g_j, x_i*) > d_real = distance of x_i* to its nearest other real.
  B(q, x)    (2 D + 4) 2^-53 (|q|^2 + |x|^2): what any float64 evaluation of the library's form may differ from the exact d2 by --
             three sums of D exact products each (relative to the sum of their terms' magnitudes at most D 2^-53 whatever the order,
             and 2 sum |q_d x_d| <= |q|^2 + |x|^2), then two roundings to combine them, each of a value at most 2 (|q|^2 + |x|^2).
             Derived, not measured.

EXACT inputs: integers in -3 .. 3, every sum exact in any order, full of exact ties: the test of the (d2, index) order.
FLOAT inputs: numpy.random.default_rng(1000 + i).standard_normal rounded through float32, one draw of nq + nx rows split into queries
and bank.  test_knn_cases_cpu.py shows that in every float case the neighbours a test compares are further apart than 1000 x 2B, so
every index is compared, none left out."""
import functools
import math

import numpy as np

KNN_TARGET_WG = 512          # la_knn.hip
KNN_MAX_SPLITS = 64
TILE = 64

# (nq, nx, D, k): case i draws from default_rng(1000 + i)
FLOAT_CASES = [(200, 300, 48, 5), (129, 127, 17, 3), (33, 31, 130, 32), (3, 5000, 8, 32), (64, 64, 1, 3), (127, 200, 4, 5),
               (256, 256, 64, 5)]
EXACT_N = [1, 2, 31, 33, 63, 64, 65, 127, 129]
EXACT_D = [1, 3, 4, 17, 33, 130]
EXACT_K = [1, 3, 5, 32]
SPLIT_CASE = (3, 5000, 8, 32)          # more than one column chunk is merged
SMALL_CASES = [(5, 7, 3, 3), (4, 4, 1, 2), (9, 6, 17, 8), (3, 2, 5, 4)]          # brute force in Python loops


def cdiv(a, b):
    return -(-a // b)


def exact_cases():
    """[(nq, nx, D, k)]: every (nq, nx) of EXACT_N x EXACT_N once, D and k rotated so that the first 24 hold every (D, k)"""
    out = []
    for i, (nq, nx) in enumerate((a, b) for a in EXACT_N for b in EXACT_N):
        out.append((nq, nx, EXACT_D[i % len(EXACT_D)], EXACT_K[(i // len(EXACT_D)) % len(EXACT_K)]))
    return out


def col_splits(nq, nx):
    """restatement of la_knn.hip's split rule.  It names cases; the GPU tests read the library's own la_knn_col_splits."""
    rb, ct = cdiv(nq, TILE), cdiv(nx, TILE)
    want = min(cdiv(KNN_TARGET_WG, rb), ct)
    return cdiv(ct, max(ct // want, cdiv(ct, KNN_MAX_SPLITS)))


@functools.lru_cache(maxsize=None)
def _float_inputs(i):
    nq, nx, D, _ = FLOAT_CASES[i]
    both = np.random.default_rng(1000 + i).standard_normal((nq + nx, D)).astype(np.float32)
    q, x = both[:nq].copy(), both[nq:].copy()
    q.setflags(write=False)
    x.setflags(write=False)
    return q, x


def float_inputs(i):
    """(Q, X) float32 of FLOAT_CASES[i], read-only and shared between the tests"""
    return _float_inputs(i)


@functools.lru_cache(maxsize=None)
def exact_inputs(nq, nx, D, seed=0):
    rs = np.random.RandomState([nq, nx, D, seed])
    q = rs.randint(-3, 4, size=[nq, D]).astype(np.float32)
    x = rs.randint(-3, 4, size=[nx, D]).astype(np.float32)
    q.setflags(write=False)
    x.setflags(write=False)
    return q, x


def two_blobs(nr=150, ng=90, D=24, seed=7):
    """real and generated features: two Gaussian blobs a little apart, so that realism falls on both sides of 1 and authenticity
    strictly between 0 and 1"""
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((nr, D)).astype(np.float32)
    gen = (0.8 * rng.standard_normal((ng, D)) + 0.4).astype(np.float32)
    return real, gen


_WIDE = np.finfo(np.longdouble).nmant >= 63


def dist2(q, x):
    """d2 [nq][nx] float64 from float32 (or integer-valued) rows, difference form, summed wider than float64 (see the module text)"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    out = np.empty([q.shape[0], x.shape[0]], np.float64)
    if _WIDE:
        xl = x.astype(np.longdouble)
        for lo in range(0, q.shape[0], 16):
            d = q[lo:lo + 16, None, :].astype(np.longdouble) - xl[None, :, :]
            out[lo:lo + 16] = (d * d).sum(axis=2).astype(np.float64)
    else:
        for i in range(q.shape[0]):
            for j in range(x.shape[0]):
                out[i, j] = math.fsum(float(a - b) ** 2 for a, b in zip(q[i], x[j]))
    return out


def bound(q, x):
    """B [nq][nx] of the module text"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    D = q.shape[1]
    return (2 * D + 4) * 2.0 ** -53 * ((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :])


def knn_from_d2(d2, k, exclude_self=False):
    """(dist2 [nq][k] float64 ascending, idx [nq][k] int64) in the order (d2, index); empty slots (+inf, -1)"""
    d2 = np.array(d2, np.float64)
    nq, nx = d2.shape
    if exclude_self:
        assert nq == nx
        d2[np.arange(nq), np.arange(nq)] = np.inf
    order = np.argsort(d2, axis=1, kind='stable')[:, :k]
    val = np.take_along_axis(d2, order, axis=1)
    dist = np.full([nq, k], np.inf)
    idx = np.full([nq, k], -1, np.int64)
    dist[:, :order.shape[1]] = val
    idx[:, :order.shape[1]] = np.where(np.isfinite(val), order, -1)
    return dist, idx


def knn_restate(q, x, k, exclude_self=False):
    return knn_from_d2(dist2(q, x), k, exclude_self)


def realism_entry_restate(q, x, radius2, d2=None):
    """(score2 [nq] float64, arg [nq] int64) of la_realism_f32's definition"""
    d2 = dist2(q, x) if d2 is None else d2
    r2 = np.asarray(radius2, np.float64)
    kept = r2 >= 0
    if not kept.any():
        return np.zeros([d2.shape[0]]), np.full([d2.shape[0]], -1, np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        quot = np.where(d2 == 0, np.inf, r2[None, :] / d2)
    quot = np.where(kept[None, :], quot, -1.0)
    arg = quot.argmax(axis=1)          # (the first of equal maxima)
    return quot[np.arange(d2.shape[0]), arg], arg.astype(np.int64)


@functools.lru_cache(maxsize=None)
def realism_radii(i):
    """radius2 [nx] of float case i for the entry-level realism tests: hand-set, uniform in [0.5, 1.5) from default_rng(2000 + i) (the
    entry takes any radii), every third sphere dropped (negative)"""
    radius2 = np.random.default_rng(2000 + i).uniform(0.5, 1.5, FLOAT_CASES[i][1])
    radius2[1::3] = -1.0
    radius2.setflags(write=False)
    return radius2


def kept_spheres(radius2, keep_fraction):
    """bool [nr]: the ceil(keep_fraction nr) smallest radii, ties by lower index"""
    nr = len(radius2)
    keep = np.zeros([nr], bool)
    keep[np.argsort(radius2, kind='stable')[:int(math.ceil(keep_fraction * nr))]] = True
    return keep


def realism_restate(real, gen, nhood_size=3, keep_fraction=0.5):
    """dict(realism [ng], radii [nr], kept bool [nr], arg [ng], score2, radius2)"""
    radius2 = knn_restate(real, real, nhood_size, exclude_self=True)[0][:, nhood_size - 1]
    kept = kept_spheres(radius2, keep_fraction)
    score2, arg = realism_entry_restate(gen, real, np.where(kept, radius2, -1.0))
    return dict(realism=np.sqrt(score2), radii=np.sqrt(radius2), kept=kept, arg=arg, score2=score2, radius2=radius2)


def dist_rel_bound(q, x, idx):
    """[nq]: relative bound on dist(q_j, x_idx[j]) = sqrt(d2): B / d2 for the d2 (the root at most halves it), 2^-52 for the two roots"""
    rows = np.arange(len(idx))
    return bound(q, x)[rows, idx] / dist2(q, x)[rows, idx] + 2.0 ** -52


def realism_rel_bounds(real, gen, nhood_size, keep_fraction):
    """dict(radii [nr], realism [ng]): relative bounds on what metrics.compute_realism_from_features may differ from realism_restate by,
    given equal kept sets and args.  radius2 carries b_r = B / radius2 of its pair, the distance to the winning sphere b_d = B / d2; the
    quotient is off by (1 + b_r) / (1 - b_d) and its own rounding; roots only shrink relative errors, and round once on each side."""
    d2rr, irr = knn_restate(real, real, nhood_size, exclude_self=True)
    b_r = bound(real, real)[np.arange(len(real)), irr[:, nhood_size - 1]] / d2rr[:, nhood_size - 1]
    arg = realism_restate(real, gen, nhood_size, keep_fraction)['arg']
    rows = np.arange(len(gen))
    b_d = bound(gen, real)[rows, arg] / dist2(gen, real)[rows, arg]
    return dict(radii=b_r + 2.0 ** -52, realism=(1.0 + b_r[arg]) / (1.0 - b_d) * (1.0 + 2.0 ** -53) - 1.0 + 2.0 ** -51)


def authenticity_restate(real, gen):
    """dict(authenticity, authentic bool [ng], nearest [ng], d_gen [ng], d_real [ng])"""
    d2g, ig = knn_restate(gen, real, 1)
    d2r, _ = knn_restate(real, real, 1, exclude_self=True)
    d_gen, d_real = np.sqrt(d2g[:, 0]), np.sqrt(d2r[ig[:, 0], 0])
    flags = d_gen > d_real
    return dict(authenticity=float(flags.mean()), authentic=flags, nearest=ig[:, 0], d_gen=d_gen, d_real=d_real)


def membership64(real, gen, nhood_size):
    """float64 precision membership: generated j lies inside the sphere of some real i, whose radius reaches its nhood_size-th nearest
    other real (precision_recall.py:80-84 in float64, on squared distances)"""
    radius2 = knn_restate(real, real, nhood_size, exclude_self=True)[0][:, nhood_size - 1]
    return (dist2(gen, real) <= radius2[None, :]).any(axis=1)


# ------------------------------------------------------------------------------------------------ independent brute force (small cases)
def brute_d2(q, x):
    return [[math.fsum((float(a) - float(b)) ** 2 for a, b in zip(qi, xj)) for xj in x] for qi in q]


def brute_knn(q, x, k, exclude_self=False):
    dist, idx = [], []
    d2 = brute_d2(q, x)
    for i, row in enumerate(d2):
        cand = sorted((d, j) for j, d in enumerate(row) if not (exclude_self and j == i))[:k]
        cand += [(math.inf, -1)] * (k - len(cand))
        dist.append([c[0] for c in cand])
        idx.append([c[1] for c in cand])
    return np.array(dist), np.array(idx, np.int64)


def brute_realism_entry(q, x, radius2):
    score, arg = [], []
    for row in brute_d2(q, x):
        best, at = 0.0, -1
        for i, d in enumerate(row):
            if radius2[i] < 0:
                continue
            s = math.inf if d == 0 else float(radius2[i]) / d
            if at < 0 or s > best:
                best, at = s, i
        score.append(best)
        arg.append(at)
    return np.array(score), np.array(arg, np.int64)
