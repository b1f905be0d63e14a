"""Kernel Inception Distance restated on the CPU (numpy), in float64 by default: the yardstick of tests/test_hip_kid.py.

  k(a, b) = (a.b / D + 1)^3
  mmd2    = sum_{i != j} k(x_i, x_j) / (mx (mx - 1)) + sum_{i != j} k(y_i, y_j) / (my (my - 1)) - 2 sum_{i, j} k(x_i, y_j) / (mx my)
  KID     = mean of mmd2 over the subsets

x are rows of the GENERATED features, y rows of the REAL ones.  The indices are taken explicitly; `subset_indices` restates the
draw: m = min(Nr, Ng, max_subset_size) rows per side without replacement from numpy.random.RandomState(seed), generated side first,
then the real side, subset after subset; max_subset_size=None (one subset) is every row once in its given order.
`dtype=np.float32` runs the same statements in float32 from end to end: the products, the cube, the sums and the combination.
"""
import numpy as np


def subset_indices(num_real, num_gen, num_subsets=100, max_subset_size=1000, seed=0):
    if max_subset_size is None:
        assert num_subsets == 1
        return np.arange(num_gen, dtype=np.int32)[None], np.arange(num_real, dtype=np.int32)[None]
    m = min(num_real, num_gen, max_subset_size)
    assert m >= 2
    rs = np.random.RandomState(seed)
    ix, iy = [], []
    for _ in range(num_subsets):
        ix.append(rs.choice(num_gen, m, replace=False))
        iy.append(rs.choice(num_real, m, replace=False))
    return np.asarray(ix, dtype=np.int32), np.asarray(iy, dtype=np.int32)


def _offdiag_sum(k):
    return k[~np.eye(k.shape[0], dtype=bool)].sum()


def kid_from_indices(real, gen, ix, iy, dtype=np.float64):
    """-> dict(kid, mmd2 [S], sums [S][3] raw (xx off-diagonal, yy off-diagonal, xy), nsums [S][3] the same divided by their counts),
    every array in `dtype`.  real / gen: [N, D], used from their float32 values."""
    real = np.asarray(real, dtype=np.float32).astype(dtype)
    gen = np.asarray(gen, dtype=np.float32).astype(dtype)
    D = dtype(real.shape[1])
    one = dtype(1)
    S = ix.shape[0]
    sums = np.zeros([S, 3], dtype)
    nsums = np.zeros([S, 3], dtype)
    mmd2 = np.zeros([S], dtype)
    for s in range(S):
        x, y = gen[ix[s]], real[iy[s]]
        mx, my = x.shape[0], y.shape[0]
        sums[s, 0] = _offdiag_sum((x @ x.T / D + one) ** 3)
        sums[s, 1] = _offdiag_sum((y @ y.T / D + one) ** 3)
        sums[s, 2] = ((x @ y.T / D + one) ** 3).sum()
        nsums[s] = sums[s] / np.array([mx * (mx - 1), my * (my - 1), mx * my], dtype)
        mmd2[s] = nsums[s, 0] + nsums[s, 1] - dtype(2) * nsums[s, 2]
    return dict(kid=mmd2.mean(), mmd2=mmd2, sums=sums, nsums=nsums)


def kid(real, gen, num_subsets=100, max_subset_size=1000, seed=0, dtype=np.float64):
    ix, iy = subset_indices(real.shape[0], gen.shape[0], num_subsets, max_subset_size, seed)
    return kid_from_indices(real, gen, ix, iy, dtype)


def detector_like_features(n, d, seed, scale=1.0):
    """Seeded features with the scale of pooled detector activations: non-negative, mean about 0.5, about one coordinate in a hundred
    large (4..12), so that a.b / D is of order 0.3..1 and the cube reaches well above 1."""
    rs = np.random.RandomState(seed)
    f = rs.gamma(0.6, 0.7, size=[n, d])
    f += (rs.uniform(size=[n, d]) < 0.01) * rs.uniform(4.0, 12.0, size=[n, d])
    return (f * scale).astype(np.float32)
