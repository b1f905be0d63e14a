"""Case table, seeded inputs and float64 restatements for the Frechet distance of two feature sets (la_frechet.hip,
metrics.compute_fd_from_features).  No GPU and no oracle import.

  fd_ref64(real, gen)      FD = |mu_g - mu_r|^2 + |A|_F^2 / Ng + |B|_F^2 / Nr - 2 nuc(A B^T) / sqrt(Ng Nr) with numpy.linalg.svd
  round_pair(n, r, k)      pair k of round r of the circle method (la_fd_round_pair)
  jacobi_sweep(V, tol)     one sweep of one-sided Jacobi over the rows of V in that pair order (la_fd_jacobi_sweep_f64)
  jacobi_ref(C, tol)       sweeps until one makes no rotation
"""
import numpy as np

EPS = 2.0 ** -52


def fd_terms64(real, gen):
    """(mean_term, trace_gen, trace_real, nuclear, singular values of A B^T) in float64"""
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    ng, nr = gen.shape[0], real.shape[0]
    mu_g, mu_r = gen.mean(0), real.mean(0)
    a, b = gen - mu_g, real - mu_r
    sv = np.linalg.svd(a @ b.T, compute_uv=False)
    return (float(np.square(mu_g - mu_r).sum()), float(np.square(a).sum()) / ng, float(np.square(b).sum()) / nr,
            float(sv.sum()) / float(np.sqrt(float(ng) * float(nr))), sv)


def fd_ref64(real, gen):
    m, tg, tr, nuc, _ = fd_terms64(real, gen)
    return m + tg + tr - 2.0 * nuc


def fd_scale(real, gen):
    """the size of the terms FD is a difference of: every bound on an FD error is stated against it"""
    m, tg, tr, _, _ = fd_terms64(real, gen)
    return m + tg + tr


def round_pair(n, r, k):
    """(p, q), p < q: pair k (0 .. n'/2 - 1) of round r (0 .. n' - 2), n' = n rounded up to even.  Player n' - 1 stays, the others
    rotate; index n of an odd n is the padding vector."""
    n2 = n + (n & 1)
    r1 = n2 - 1
    a, b = (r1, r) if k == 0 else ((r + k) % r1, (r - k + r1) % r1)
    return (a, b) if a < b else (b, a)


def jacobi_tol(m):
    return float(np.sqrt(float(m))) * EPS          # LAPACK dgesvj's criterion


def jacobi_sweep(V, tol, margin=None):
    """One sweep, in place, over the rows of V [n'][m] (n' even; an odd n: the zero row last).  Returns the number of rotations.
    margin (a list): receives, per pair with alpha beta > 0, |gamma| / (tol sqrt(alpha beta)) -- how far the pair was from the
    threshold; a value near 1 is a decision that another summation order may take the other way."""
    n2, m = V.shape
    assert n2 % 2 == 0
    rot = 0
    for r in range(n2 - 1):
        pq = np.array([round_pair(n2, r, k) for k in range(n2 // 2)])
        p, q = pq[:, 0], pq[:, 1]
        cp, cq = V[p], V[q]
        alpha, beta, gamma = (cp * cp).sum(1), (cq * cq).sum(1), (cp * cq).sum(1)
        ab = alpha * beta
        live = ab > 0
        if margin is not None:
            margin.extend((np.abs(gamma[live]) / (tol * np.sqrt(ab[live]))).tolist())
        go = live & (np.abs(gamma) > tol * np.sqrt(np.where(live, ab, 1.0)))
        if not go.any():
            continue
        g = np.where(go, gamma, 1.0)
        zeta = (beta - alpha) / (2.0 * g)
        with np.errstate(over='ignore'):
            t = np.where(zeta == 0, 1.0, np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta)))
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = c * t
        c, s = np.where(go, c, 1.0)[:, None], np.where(go, s, 0.0)[:, None]
        V[p], V[q] = c * cp - s * cq, s * cp + c * cq
        rot += int(go.sum())
    return rot


def vectors_of(C):
    """the n' x m float64 array the kernels work on: the shorter side of C [a][b] as rows, a zero row appended when their number is odd"""
    C = np.asarray(C, np.float64)
    V = C if C.shape[0] <= C.shape[1] else C.T
    n, m = V.shape
    out = np.zeros([n + (n & 1), m])
    out[:n] = V
    return out


def jacobi_ref(C, tol=None, max_sweeps=30):
    """(singular values in vector order, sweeps) of C by one-sided Jacobi; the last sweep is the one that made no rotation"""
    V = vectors_of(C)
    n = min(np.shape(C))
    tol = jacobi_tol(V.shape[1]) if tol is None else tol
    for sweeps in range(1, max_sweeps + 1):
        if jacobi_sweep(V, tol) == 0:
            return np.sqrt((V * V).sum(1))[:n], sweeps
    raise RuntimeError(f'jacobi_ref: no convergence in {max_sweeps} sweeps')


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
def features(n, d, seed, shift=0.0, scale=1.0):
    """detector-like float32 features: non-negative, a few dominant directions"""
    rs = np.random.RandomState(seed)
    base = rs.randn(n, d) * (1.0 + 3.0 * (np.arange(d) % 7 == 0)) + 0.3 * rs.randn(n, 1)
    return (np.maximum(base * scale + 0.5 + shift, 0.0)).astype(np.float32)


def integer_features(half_rows, d, seed):
    """integer values in [-8, 8], the negated rows appended: every column mean is exactly 0 and every sum below is exact in float64"""
    x = np.random.RandomState(seed).randint(-8, 9, size=(half_rows, d)).astype(np.float32)
    return np.concatenate([x, -x])


# (nx, ny, D) of the exact Gram test; nx and ny are even (negated rows appended)
GRAM_EXACT_SIZES = [(16, 16, 4), (18, 34, 5), (2, 3, 1), (33, 17, 130)]


def gram_exact_inputs(nx, ny, d, seed=0):
    """(x [nx'][d], y [ny'][d]) integer-valued with zero column means.  An odd count cannot be made of negated pairs alone: it gets one
    all-zero row, which keeps the means at 0."""
    def one(n, s):
        v = integer_features(n // 2, d, s)
        return np.concatenate([v, np.zeros([n & 1, d], np.float32)])
    return one(nx, seed), one(ny, seed + 1)


# the whole-function cases: name -> (real, gen)
def fd_cases():
    cases = {
        'rank-deficient 40/48 x 96': (features(48, 96, 1), features(40, 96, 2, scale=1.1)),
        'rank-deficient 33/17 x 256': (features(17, 256, 3), features(33, 256, 4, shift=0.2)),
        'full rank 200/150 x 64': (features(150, 64, 5), features(200, 64, 6, scale=0.9)),
        'n = 2': (features(2, 16, 9), features(5, 16, 10)),
    }
    same = features(48, 80, 7)
    cases['gen = real 48/48 x 80'] = (same, same.copy())
    dup = features(30, 64, 8)
    dup[20:30] = dup[0:10]          # ten duplicated rows: equal columns of A B^T -> 45-degree rotations, then zero columns
    cases['ten duplicated rows 30/36 x 64'] = (dup, features(36, 64, 11))
    return cases


# matrices for jacobi_ref against numpy.linalg.svd: the cross-Gram matrices of the cases above and a few plain ones
def jacobi_cases():
    out = {}
    for name, (real, gen) in fd_cases().items():
        a, b = gen.astype(np.float64), real.astype(np.float64)
        out[name] = (a - a.mean(0)) @ (b - b.mean(0)).T
    rs = np.random.RandomState(12)
    out['48 x 40'] = rs.randn(48, 40)
    out['17 x 33'] = rs.randn(17, 33)
    out['64 x 64'] = rs.randn(64, 64)
    c = rs.randn(20, 24)
    out['centred 20 x 24'] = c - c.mean(0)
    out['7 x 5'] = rs.randn(7, 5)
    out['2 x 2'] = rs.randn(2, 2)
    out['300 x 9'] = rs.randn(300, 9)
    # vector lengths on both sides of the seams at which la_fd_jacobi_sweep_f64 changes its round kernel (m <= 2048, <= 4096, <= 8192
    # elements in registers; streaming above), a few vectors each
    out['2048 x 4'] = rs.randn(2048, 4)
    out['2049 x 3'] = rs.randn(2049, 3)
    out['8192 x 5'] = rs.randn(8192, 5)
    out['8193 x 6'] = rs.randn(8193, 6)
    return out


# the matrices of the one-sweep test at the C ABI (test_hip_fd.test_sweeps_follow_the_restatement)
SWEEP_CASES = ('7 x 5', '2 x 2', '300 x 9', '2048 x 4', '2049 x 3', '8192 x 5', '8193 x 6')
