"""Case tables, seeded inputs and float64 restatements for density and coverage (la_dc_count_f16, metrics.compute_dc_from_features).
Shared by test_dc_cases_cpu.py (which proves, without a GPU, that the cases reach what they claim) and test_hip_dc.py.  Helpers only;
nothing here reads a file.  Built on criteria_cases.pr_features / pr_dist / pr_kth.

Definitions (include/latentaug_hip.h): real X [nr][D], generated Y [ng][D], float16; r_i = (k+1)-th smallest distance from real i to all
reals, its own zero included; count[j] = #{i : dist(Y_j, X_i) <= r_i}; nearest[i] = min_j dist(Y_j, X_i); covered[i] = nearest[i] <= r_i;
density = sum_j count[j] / (k ng); coverage = mean_i covered[i].

EXACT inputs: integers in -2..2, every squared distance an integer that float32 holds exactly, so every comparison, a tie included, has
one right answer and the kernel must return it.
FLOAT inputs: ONE draw of nr + ng detector-like rows, split into real and generated.  Two separate draws of criteria_cases.pr_features
have different per-feature offsets, and as D grows next to no generated row lies in any real ball (density and coverage at or near 0),
which a kernel that returns zeros would all but pass.  A float32 kernel may disagree with float64 only inside the bracket of `dc_brackets`."""
import functools

import numpy as np

import criteria_cases as cc

DC_SHAPES = [(9, 1), (33, 31), (32, 32), (127, 33), (128, 129), (130, 161), (257, 130), (300, 700)]          # (nr, ng)
DC_D = [16, 48, 112]
DC_K = [1, 5]
DC_D_PADDED = 100                       # through metrics.py: padded to 112 on the host
DC_TARGET_WG = 512                      # la_metrics.hip: DC_TARGET_WG
# (nr, ng) for the column-chunk rule: ONE chunk of three 128-column steps (516 row blocks already exceed the target), and TWO chunks of
# 256 and 44 columns (258 row blocks: two steps in the first chunk, a short last chunk).  Every listed shape with nr > 128 has one
# 128-column step per chunk.
DC_SPLIT_SHAPES = [(300, 66000), (300, 33000)]
DC_SPLIT_D = 16
FLOAT_SEED = 21
# seeds of the exact draws: 35 is the first generated-side seed with which every listed case, the single generated row of (9, 1) included,
# has density and coverage above 0 in the float64 restatement
EXACT_SEED_REAL, EXACT_SEED_GEN = 1, 35


def dc_chunk_cols(ng, nr):
    """restatement of la_metrics.hip's dc_chunk_cols: columns per chunk.  It only names cases; it never produces an expected value."""
    rb, ct = cc.cdiv(ng, 128), cc.cdiv(nr, 128)
    want = min(cc.cdiv(DC_TARGET_WG, rb), ct)
    return cc.cdiv(ct, want) * 128


def dc_col_splits(ng, nr):
    return cc.cdiv(nr, dc_chunk_cols(ng, nr))


def dc_case_id(D, nr, ng):
    chunk, s = dc_chunk_cols(ng, nr), dc_col_splits(ng, nr)
    w = [f'D{D}', f'real{nr}', f'gen{ng}', f'{s}chunk' + ('s' if s > 1 else ''), f'{chunk // 128}step' + ('s' if chunk > 128 else '')]
    if ng < 32:
        w.append('lt32rows')
    if nr % 128 in (1, 2):
        w.append('col-past-seam')
    if s > 1 and nr % chunk:
        w.append('short-last-chunk')
    return '-'.join(w)


@functools.lru_cache(maxsize=None)
def _inputs(nr, ng, D, kind):
    if kind == 'exact':
        real, gen = cc.pr_features(nr, D, EXACT_SEED_REAL), cc.pr_features(ng, D, EXACT_SEED_GEN)
    else:
        both = cc.pr_features(nr + ng, D, FLOAT_SEED, 'float')
        real, gen = both[:nr].copy(), both[nr:].copy()
    real.setflags(write=False)
    gen.setflags(write=False)
    return real, gen


def dc_inputs(nr, ng, D, kind):
    """(real [nr][D], gen [ng][D]) float16, read-only and shared between the tests"""
    return _inputs(nr, ng, D, kind)


def dc_from_radii(real16, gen16, radii):
    """count, nearest, covered, ties with the float64 distances and the radii given"""
    d = cc.pr_dist(np.asarray(gen16), np.asarray(real16))          # [ng][nr]
    r = np.asarray(radii, np.float64)[None, :]
    nearest = d.min(axis=0)
    return dict(count=(d <= r).sum(axis=1).astype(np.int64), nearest=nearest, covered=nearest <= r[0], ties=int((d == r).sum()),
                nearest_d2=cc.pr_dist2(np.asarray(gen16), np.asarray(real16)).min(axis=0))


def dc_restate(real16, gen16, k):
    """density and coverage in float64 from float16 features: dict(radii, count, nearest, covered, density, coverage, ties).  `ties` is the
    number of (generated, real) pairs whose distance equals the real sample's radius exactly: where <= and prdc's < differ."""
    real16, gen16 = np.asarray(real16), np.asarray(gen16)
    assert real16.dtype == np.float16 and gen16.dtype == np.float16 and 1 <= k <= real16.shape[0] - 1
    radii = cc.pr_kth(real16, real16, k)
    out = dc_from_radii(real16, gen16, radii)
    out['radii'] = radii
    out['density'] = int(out['count'].sum()) / (k * gen16.shape[0])
    out['coverage'] = int(out['covered'].sum()) / real16.shape[0]
    return out


@functools.lru_cache(maxsize=None)
def dc_restate_case(nr, ng, D, kind, k):
    return dc_restate(*dc_inputs(nr, ng, D, kind), k)


def dc_delta(a2, b2, d, D):
    """First-order worst case of the kernel's float32 formula sqrt(|a|^2 + |b|^2 - 2 a.b) against float64:
        delta(a, b) = (D + 2) 2^-24 (|a|^2 + |b|^2) / d + 2^-23 d.
    Each of |a|^2, |b|^2 and a.b is a float32 sum of D exact products (float16 x float16 is exact in float32): relative to the sum of the
    absolute values of its terms at most D 2^-24 whatever the order, and sum_k |a_k b_k| <= (|a|^2 + |b|^2) / 2, so d^2 is off by at most
    D 2^-24 2 (|a|^2 + |b|^2); the two additions that combine the three sums add 2 2^-24 2 (|a|^2 + |b|^2) at most (every intermediate is
    at most 2 (|a|^2 + |b|^2)); an error e in d^2 is e / (2 d) in d; the root itself rounds once more, 2^-23 d with slack for a root that
    is not correctly rounded.  Derived, not tuned."""
    return (D + 2) * 2.0 ** -24 * (a2 + b2) / d + 2.0 ** -23 * d


def dc_brackets(real16, gen16, k, D=None):
    """What a float32 kernel that follows the formula may return: per generated row lower <= count <= upper, per real sample covered is
    forced where cov_lower == cov_upper.  The bracket of pair (j, i) is delta(Y_j, X_i) + the delta of the pair whose distance is r_i.
    D: the dimension the kernel sums over (the padded one), by default the features'."""
    real, gen = np.asarray(real16).astype(np.float64), np.asarray(gen16).astype(np.float64)
    D = real.shape[1] if D is None else D
    r2, g2 = (real * real).sum(1), (gen * gen).sum(1)
    drr = cc.pr_dist(np.asarray(real16), np.asarray(real16))
    order = np.argsort(drr, axis=1, kind='stable')[:, k]
    radii = drr[np.arange(real.shape[0]), order]
    rad_delta = dc_delta(r2, r2[order], radii, D)                                    # [nr]
    d = cc.pr_dist(np.asarray(gen16), np.asarray(real16))                            # [ng][nr]
    width = dc_delta(g2[:, None], r2[None, :], d, D) + rad_delta[None, :]
    lo, hi = d <= radii[None, :] - width, d <= radii[None, :] + width
    return dict(radii=radii, rad_delta=rad_delta, lower=lo.sum(1), upper=hi.sum(1), cov_lower=lo.any(0), cov_upper=hi.any(0))


@functools.lru_cache(maxsize=None)
def dc_brackets_case(nr, ng, D, k):
    return dc_brackets(*dc_inputs(nr, ng, D, 'float'), k)


def dc_radii_pattern(real16, gen16, seed):
    """Hand-set radii sqrt(q_i + 1/2), q_i = max(0, base + s_i) with s_i in -2..2 (the pattern of criteria_cases.member_pattern_a):
    integer squared distances never lie on a boundary.  base is the median over the real samples of the squared distance to their
    nearest generated row, so about half of them are covered."""
    d2 = np.rint(cc.pr_dist2(np.asarray(gen16), np.asarray(real16))).astype(np.int64)
    s = np.random.RandomState([seed, 78]).randint(-2, 3, size=[real16.shape[0]])
    q = np.maximum(int(np.median(d2.min(axis=0))) + s, 0)
    return np.sqrt(q + 0.5).astype(np.float32)


def dc_planted(real16, ng, seed):
    """(gen, planted {generated row: real column}): fresh generated rows, except that the rows on both sides of the 32- and 128-row seams
    (and the last) are copies of the real columns on both sides of the 32-, 128-column and column-chunk seams (and the last); the last
    row carries the last column.  With every radius sqrt(1/2) exactly the planted pairs are inside a ball."""
    nr, D = real16.shape
    chunk = dc_chunk_cols(ng, nr)
    cols = [c for c in dict.fromkeys([nr - 1, 0, 31, 32, 127, 128, chunk - 1, chunk]) if 0 <= c < nr]
    rows = [r for r in dict.fromkeys([ng - 1, 0, 31, 32, 127, 128, 33, 129, ng // 2]) if 0 <= r < ng]
    planted = dict(zip(rows, cols))
    gen = cc.pr_features(ng, D, seed + 500).copy()
    for j, i in planted.items():
        gen[j] = real16[i]
    return gen, planted


def dc_last_column_only(nr):
    """only the last real column admits anything, and it admits everything"""
    return cc.member_pattern_c(nr)
