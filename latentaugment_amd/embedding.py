"""UMAP embedding of latents and features on HIP (la_umap.hip): the reference's headline figure (analysis/umap_analysis.py fits
umap-learn on the W codes of the inverted training set and transforms real, LatentAugment and random-GAN codes into that map).

  LatentUMAP        fit / fit_transform / transform, embedding_, graph_
  find_ab_params    the curve parameters a, b of (spread, min_dist): numpy only
  embed_aug_runs    the reference's script as a function: fit on a latent zip, transform the dumps of run directories

The method is UMAP (McInnes, Healy, Melville 2018) with four deliberate differences from the umap-learn library:
  (1) an epoch is synchronous: all forces are computed from the positions at the start of the epoch;
  (2) the randomness is the library's Philox stream (counter convention: csrc/la_rng.h), keyed by `seed`;
  (3) the initial layout is random or supplied by the caller, never spectral;
  (4) the sigma bisection of the smooth-kNN step always runs its 64 iterations (no early exit on a tolerance).
Because of (1) and (2) a run is reproducible bit for bit, which umap-learn's parallel layout is not; a transformed row depends on
itself and the fitted bank only and gives the same bits in any batch.  All stages after the float32 neighbour search are float64.

This module is plumbing: every stage is a HIP entry and there is no CPU fallback (LatentAugHipError without a device).  The
neighbour search is the brute-force la_knn_f32, so the intended range is up to about 1e5 rows.  Metric: Euclidean only."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, metrics

MIN_NEIGHBORS, MAX_NEIGHBORS = 2, metrics.KNN_MAX_K + 1
MAX_COMPONENTS = 8
MAX_RATE = 32


def find_ab_params(spread=1.0, min_dist=0.1):
    """(a, b) of the layout's curve 1 / (1 + a x^(2b)): the least-squares fit on 300 points of [0, 3 spread] to the target that is 1
    for x <= min_dist and exp(-(x - min_dist) / spread) above -- umap-learn's find_ab_params, which calls scipy's curve_fit; here a
    few lines of Levenberg-Marquardt from (1, 1) in numpy (the product does not import scipy for it)."""
    spread, min_dist = float(spread), float(min_dist)
    if not spread > 0 or not 0 <= min_dist < 3 * spread:
        raise ValueError(f'spread must be positive and 0 <= min_dist < 3 spread (got spread={spread}, min_dist={min_dist})')
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x <= min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    lx = np.log(np.where(x > 0, x, 1.0))

    def model(p):
        xp = np.where(x > 0, np.exp(2.0 * p[1] * lx), 0.0)          # x^(2b), 0 at x = 0
        f = 1.0 / (1.0 + p[0] * xp)
        return f, np.stack([-xp * f * f, -2.0 * p[0] * xp * lx * f * f], axis=1)

    p, lam = np.array([1.0, 1.0]), 1e-3
    f, J = model(p)
    cost = float(((f - y) ** 2).sum())
    for _ in range(500):
        g, H = J.T @ (f - y), J.T @ J
        step = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        q = p + step
        if q[0] > 0 and q[1] > 0:
            fq, Jq = model(q)
            cq = float(((fq - y) ** 2).sum())
        else:
            cq = np.inf
        if cq <= cost:
            small = bool(np.all(np.abs(step) <= 1e-14 * np.abs(q)))
            p, f, J, cost, lam = q, fq, Jq, cq, max(lam * 0.1, 1e-12)
            if small:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


class LatentUMAP:
    """UMAP of [N, D] latents or features (numpy arrays or tensors of a float dtype, read as float32) into `n_components` (1 .. 8)
    dimensions on the HIP path; see the module docstring for the method and its four differences from umap-learn.

    n_neighbors 2 .. 33 counts the point itself, as umap-learn's does: a fit uses the n_neighbors - 1 nearest OTHER rows.  n_epochs
    None: 500 up to 10 000 rows and 200 above.  init: 'random' (10 * the stream's unit uniform, under `seed`) or an [N, n_components]
    array.  negative_sample_rate 0 .. 32.  fit(X) leaves embedding_ (float64 [N, n_components]) and graph_ = (row_ptr int32 [N + 1],
    col int32, val float64): the fuzzy union as a symmetric CSR, columns ascending within a row.  transform(Xq, row0) embeds new rows
    against the fitted ones: n_neighbors nearest fitted rows, the same smooth-kNN, the weighted mean of their positions, then
    max(1, n_epochs // 3) epochs in which only the new rows move; row i draws with the Philox counter of global row row0 + i, so a
    batch equals its rows transformed one at a time with the matching row0, bit for bit.  Two fits give the same bits."""

    def __init__(self, n_neighbors=15, n_components=2, n_epochs=None, min_dist=0.1, spread=1.0, negative_sample_rate=5,
                 learning_rate=1.0, seed=42, init='random', device='cuda:0'):
        if int(n_neighbors) != n_neighbors or not MIN_NEIGHBORS <= n_neighbors <= MAX_NEIGHBORS:
            raise ValueError(f'n_neighbors must lie in {MIN_NEIGHBORS} .. {MAX_NEIGHBORS} (got {n_neighbors})')
        if int(n_components) != n_components or not 1 <= n_components <= MAX_COMPONENTS:
            raise ValueError(f'n_components must lie in 1 .. {MAX_COMPONENTS} (got {n_components})')
        if n_epochs is not None and (int(n_epochs) != n_epochs or not 1 <= n_epochs <= 1 << 28):
            raise ValueError(f'n_epochs must be None or lie in 1 .. 2^28 (got {n_epochs})')
        if int(negative_sample_rate) != negative_sample_rate or not 0 <= negative_sample_rate <= MAX_RATE:
            raise ValueError(f'negative_sample_rate must lie in 0 .. {MAX_RATE} (got {negative_sample_rate})')
        if isinstance(init, str) and init != 'random':
            raise ValueError(f"init must be 'random' or an array (got {init!r}; there is no spectral initialisation)")
        self.n_neighbors, self.n_components = int(n_neighbors), int(n_components)
        self.n_epochs, self.negative_sample_rate = n_epochs, int(negative_sample_rate)
        self.min_dist, self.spread, self.learning_rate = float(min_dist), float(spread), float(learning_rate)
        self.seed, self.init, self.device = int(seed) & 0xFFFFFFFFFFFFFFFF, init, device
        self.a, self.b = find_ab_params(self.spread, self.min_dist)
        self.embedding_ = self.graph_ = None
        self._bank = self._y = None

    # ---- stages (device tensors in, device tensors out)
    def _smooth_knn(self, dist2, idx):
        lib, (n, k), dev = _lib.load(), dist2.shape, dist2.device
        rho = torch.empty([n], dtype=torch.float64, device=dev)
        sigma = torch.empty([n], dtype=torch.float64, device=dev)
        w = torch.empty([n, k], dtype=torch.float64, device=dev)
        p = _lib.ptr
        _lib.check(lib.la_umap_smooth_knn_f64(p(dist2), p(idx), n, k, float(np.log2(self.n_neighbors)), p(rho), p(sigma), p(w), _lib.stream_ptr()),
                   'umap_smooth_knn')
        return rho, sigma, w

    def _layout(self, ya, yb, y_tail, n_tail, csr, wmax, epochs, row0, skip_self):
        lib, which = _lib.load(), C.c_int(-1)
        (row_ptr, col, val), p = csr, _lib.ptr
        _lib.check(lib.la_umap_layout_f64(p(ya), p(yb), ya.shape[0], p(y_tail), n_tail, self.n_components, p(row_ptr), p(col), p(val), col.numel(),
                                          p(wmax), 0, epochs, epochs, self.a, self.b, self.negative_sample_rate, self.learning_rate, self.seed,
                                          int(row0), int(skip_self), C.byref(which), _lib.stream_ptr()), 'umap_layout')
        return (ya, yb)[which.value]

    def _epochs(self, n):
        return int(self.n_epochs) if self.n_epochs is not None else (500 if n <= 10000 else 200)

    def fit(self, X):
        dev, (x,) = metrics._query_features(self.device, X=X)
        lib, p, n, k, Cc = _lib.load(), _lib.ptr, x.shape[0], self.n_neighbors - 1, self.n_components
        if n < 2:
            raise ValueError('a fit needs at least 2 rows')
        init = None
        if not isinstance(self.init, str):
            init = torch.as_tensor(self.init).detach().to(dev).to(torch.float64).contiguous()
            if tuple(init.shape) != (n, Cc):
                raise ValueError(f'init must be [N, n_components] = [{n}, {Cc}] (got {list(init.shape)})')
        dist2, idx = metrics._knn_device(x, x, k, True)
        nbytes = lib.la_umap_scratch_bytes(n, k)
        if nbytes == 0:
            raise ValueError(f'{n} rows with {self.n_neighbors} neighbours exceed what the graph stage indexes (2 n k < 2^31)')
        cap = 2 * n * k
        row_ptr = torch.empty([n + 1], dtype=torch.int32, device=dev)
        col = torch.empty([cap], dtype=torch.int32, device=dev)
        val = torch.empty([cap], dtype=torch.float64, device=dev)
        wmax = torch.empty([1], dtype=torch.float64, device=dev)
        ya = torch.empty([n, Cc], dtype=torch.float64, device=dev)
        yb = torch.empty([n, Cc], dtype=torch.float64, device=dev)
        scratch = _lib.workspace(nbytes, dev, torch.float64)
        with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
            _, _, w = self._smooth_knn(dist2, idx)
            _lib.check(lib.la_umap_graph_f64(p(idx), p(w), n, k, p(row_ptr), p(col), p(val), cap, p(wmax), p(scratch), nbytes, _lib.stream_ptr()),
                       'umap_graph')
            if init is None:
                _lib.check(lib.la_umap_init_f64(p(ya), n, Cc, self.seed, 0, _lib.stream_ptr()), 'umap_init')
            else:
                ya.copy_(init)
            y = self._layout(ya, yb, None, n, (row_ptr, col, val), wmax, self._epochs(n), 0, True)
        nnz = int(row_ptr[n].item())
        self._bank, self._y = x, y
        self.embedding_ = y.cpu().numpy()
        self.graph_ = (row_ptr.cpu().numpy(), col[:nnz].cpu().numpy(), val[:nnz].cpu().numpy())
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_

    def transform(self, Xq, row0=0):
        if self._y is None:
            raise ValueError('transform needs a fitted embedding: call fit first')
        dev, (q,) = metrics._query_features(self.device, Xq=Xq)
        if q.shape[1] != self._bank.shape[1]:
            raise ValueError(f'rows of {q.shape[1]} features against a fit on {self._bank.shape[1]}')
        lib, p, n, k, Cc, nb = _lib.load(), _lib.ptr, q.shape[0], self.n_neighbors, self.n_components, self._bank.shape[0]
        if int(row0) != row0 or row0 < 0:
            raise ValueError(f'row0 must be a non-negative integer (got {row0})')
        k = min(k, metrics.KNN_MAX_K)          # (33 neighbours of a fit are 32 other rows; a query has no self to leave out)
        dist2, idx = metrics._knn_device(q, self._bank, k, False)
        row_ptr = torch.empty([n + 1], dtype=torch.int32, device=dev)
        wmax = torch.empty([1], dtype=torch.float64, device=dev)
        ya = torch.empty([n, Cc], dtype=torch.float64, device=dev)
        yb = torch.empty([n, Cc], dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _, _, w = self._smooth_knn(dist2, idx)
            _lib.check(lib.la_umap_transform_init_f64(p(idx), p(w), n, k, p(self._y), nb, Cc, p(ya), p(row_ptr), p(wmax), _lib.stream_ptr()),
                       'umap_transform_init')
            y = self._layout(ya, yb, self._y, nb, (row_ptr, idx.view(-1), w.view(-1)), wmax, max(1, self._epochs(nb) // 3), row0, False)
        return y.cpu().numpy()


def _run_codes(fname, w_row):
    """[n, w_dim] float32 of one dump of the reference's drivers: a pickled batch of latents ([w_dim] for a batch of one, [n, w_dim],
    [n, 1, w_dim] or [n, num_ws, w_dim]: row w_row), or the dict with key 'w' that analysis/umap_analysis.py reads"""
    from .formats import _restricted_load
    with open(fname, 'rb') as f:
        obj = _restricted_load(f)
    if isinstance(obj, dict):
        obj = obj['w']
    w = torch.as_tensor(obj).detach().to(torch.float32).cpu().numpy()
    if w.ndim == 1:
        w = w[None]
    if w.ndim == 3:
        w = w[:, 0 if w.shape[1] == 1 else w_row]
    if w.ndim != 2:
        raise ValueError(f'{fname}: latents must be [w_dim], [n, w_dim], [n, 1, w_dim] or [n, num_ws, w_dim] (got {list(w.shape)})')
    return w


def _run_group(datadir, sub, stem, n_per_group, w_row):
    parts, i, have = [], 0, 0
    while have < n_per_group and os.path.isfile(os.path.join(datadir, sub, f'{stem}_{i}')):
        parts.append(_run_codes(os.path.join(datadir, sub, f'{stem}_{i}'), w_row))
        have += parts[-1].shape[0]
        i += 1
    if not parts:
        raise FileNotFoundError(f'no {sub}/{stem}_0 under {datadir}')
    return np.concatenate(parts, axis=0)[:n_per_group]


def embed_aug_runs(latent_zip, split, run_dirs, n_per_group=100, w_row=0, **umap_kw):
    """The reference's analysis/umap_analysis.py as a function: fit a LatentUMAP (**umap_kw) on row `w_row` of every inverted code of
    `split` in the latent zip (formats.LatentCodeDataset), then transform up to `n_per_group` real codes (`latent/w_{i}` of the first
    run directory) and up to `n_per_group` augmented codes of every run directory (`latent_aug/w_aug_{i}`), read through the allow-list
    loader of formats.py.  Returns (embedding float64 [M, n_components], labels int64 [M]): label 0 the real codes, 1 + r the codes of
    run_dirs[r].  Plotting stays with the caller."""
    from .formats import LatentCodeDataset
    run_dirs = [run_dirs] if isinstance(run_dirs, (str, os.PathLike)) else list(run_dirs)
    if not run_dirs:
        raise ValueError('embed_aug_runs needs at least one run directory')
    ds = LatentCodeDataset(latent_zip, split, w_dim=None, num_ws=None)
    W = np.stack([ds[i][0][w_row] for i in range(len(ds))])
    groups = [_run_group(run_dirs[0], 'latent', 'w', n_per_group, w_row)]
    groups += [_run_group(d, 'latent_aug', 'w_aug', n_per_group, w_row) for d in run_dirs]
    labels = np.concatenate([np.full([g.shape[0]], i, dtype=np.int64) for i, g in enumerate(groups)])
    umap = LatentUMAP(**umap_kw).fit(W)
    return umap.transform(np.concatenate(groups, axis=0)), labels
