"""Host-side mirror of the reference's quality metrics (metrics/) over the HIP C ABI: the VGG16 detector features of images and
everything downstream of detector features.

  FeatureStats                 metrics/metric_utils.py:79-155   (same fields, append / append_torch / get_all / get_mean_cov,
                                                                 save / load of the reference's pickle layout)
  compute_fid_from_stats       metrics/frechet_inception_distance.py:41-45
  compute_distances            metrics/precision_recall.py:19-32
  compute_pr_from_features     metrics/precision_recall.py:72-85
  compute_kid_from_features    (not in the reference) Kernel Inception Distance, the community's kid50k_full recipe
  compute_fd_from_features     the Frechet distance of frechet_inception_distance.py from the features themselves: singular values of
                               the cross-Gram matrix by Jacobi sweeps on the GPU (la_frechet.hip), exact where N < D
  compute_dc_from_features     (not in the reference) density and coverage, Naeem et al., ICML 2020 (the `prdc` package)
  compute_prdc_from_features   precision, recall, density and coverage in one dict
  knn_from_features            (not in the reference) the k nearest bank rows of every query row, float64 on float32 features (la_knn_f32)
  compute_realism_from_features        realism score per generated sample, Kynkaanniemi et al. 2019, section 5 (la_realism_f32)
  compute_authenticity_from_features   authenticity, Alaa et al. 2022: the share of generated samples that are not near-copies
  compute_feature_stats_for_images        images -> FeatureStats through a `synthesis.DetectorEngine` (metric_utils.py:314-320)
  compute_feature_stats_for_aug_dataset   metrics/metric_utils.py:264-328: the `img_aug/` pickles of the reference's drivers
  compute_metrics_from_images             precision / recall / density / coverage / KID of two image sets
  compute_pair_metrics                    (not in the reference) MSE / MAE / PSNR / SSIM / MS-SSIM of image PAIRS (la_pair_metrics_f32)
  compute_pair_metrics_for_aug_dataset    the same for `img/img_{i}` against `img_aug/img_aug_{i}` of a run directory of the drivers
  compute_msssim_diversity                MS-SSIM over random pairs of one image set (the usual collapse check)
  laplacian_pyramid, compute_swd_from_images, compute_swd_from_features, compute_swd_for_aug_dataset
                                          (not in the reference) sliced Wasserstein distance of two image sets per Laplacian pyramid
                                          level, Karras et al. 2018, and of two feature sets: no detector (la_swd.hip, la_sort.hip)
  compute_modality_mi, compute_pair_mi    mutual information of two planes from their joint histogram (la_joint_hist_f32)
  compute_ppl, ppl_from_distances         (not in the reference) perceptual path length of the generator, Karras et al. 2019 / 2020
  compute_path_length                     perceptual length of the straight segment between two latents (la_path_points_f32)
  compute_path_length_for_aug_dataset     the same for `latent/w_{i}` against `latent_aug/w_aug_{i}` of a run directory of the drivers

The detectors (Inception-v3 and VGG16 pickles hosted by NVIDIA, metric_utils.py:46-60) cannot be fetched offline.  The VGG16 one has a
local counterpart -- the TorchScript `vgg16.pt` the LPIPS criterion already needs -- and `synthesis.DetectorEngine.from_torchscript`
runs its `return_features=True` branch on the HIP path, so precision / recall, density / coverage and KID start from images.  The
Inception-v3 pickle has none: FID keeps taking features (compute_fd_from_features) or moments (compute_fid_from_stats) that the
caller supplies; from images, the Frechet distance is that of the VGG16 features.
torch only owns the device memory; the moments, distances, radii, membership tests and kernel sums are HIP kernels (la_metrics.hip).
"""
import ctypes as C
import glob
import os
import pickle
import uuid

import numpy as np
import scipy.linalg
import torch

from . import _lib


class FeatureStats:
    """Running feature statistics.  Device tensors handed to `append_torch` are accumulated ON the GPU (float64
    accumulators, `la_feature_moments_f64`); numpy input goes through the same kernel after an upload."""

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None, device='cuda:0'):
        self.capture_all = capture_all
        self.capture_mean_cov = capture_mean_cov
        self.max_items = max_items
        self.num_items = 0
        self.num_features = None
        self.all_features = None
        self._dev = torch.device(device)
        self._mean = None      # float64 device accumulators
        self._cov = None

    def set_num_features(self, num_features):
        if self.num_features is not None:
            assert num_features == self.num_features
            return
        self.num_features = num_features
        self.all_features = []
        if self.capture_mean_cov:
            self._mean = torch.zeros([num_features], dtype=torch.float64, device=self._dev)
            self._cov = torch.zeros([num_features, num_features], dtype=torch.float64, device=self._dev)

    def is_full(self):
        return (self.max_items is not None) and (self.num_items >= self.max_items)

    def append_torch(self, x, num_gpus=1, rank=0):
        assert isinstance(x, torch.Tensor) and x.ndim == 2
        assert 0 <= rank < num_gpus
        if num_gpus > 1:      # interleave the ranks' samples, as the reference does with broadcasts (metric_utils.py:120-128)
            ys = [torch.empty_like(x) for _ in range(num_gpus)]
            torch.distributed.all_gather(ys, x.contiguous())
            x = torch.stack(ys, dim=1).flatten(0, 1)
        _lib.require_gpu(x)
        x = x.detach().to(torch.float32).contiguous()
        if (self.max_items is not None) and (self.num_items + x.shape[0] > self.max_items):
            if self.num_items >= self.max_items:
                return
            x = x[:self.max_items - self.num_items].contiguous()
        self.set_num_features(x.shape[1])
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x.cpu().numpy())
        if self.capture_mean_cov:
            lib = _lib.load()
            with torch.cuda.device(x.device):
                _lib.check(lib.la_feature_moments_f64(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(self._mean), _lib.ptr(self._cov),
                                                      _lib.stream_ptr()), 'feature_moments')

    def append(self, x):
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2
        self.append_torch(torch.from_numpy(x).to(self._dev))

    def get_all(self):
        assert self.capture_all
        return np.concatenate(self.all_features, axis=0)

    def get_all_torch(self):
        return torch.from_numpy(self.get_all())

    @property
    def raw_mean(self):
        return None if self._mean is None else self._mean.cpu().numpy()

    @property
    def raw_cov(self):
        return None if self._cov is None else self._cov.cpu().numpy()

    def get_mean_cov(self):
        assert self.capture_mean_cov
        mean = self.raw_mean / self.num_items
        cov = self.raw_cov / self.num_items
        cov = cov - np.outer(mean, mean)
        return mean, cov

    def save(self, pkl_file):
        """The reference's cache layout: a pickle of the object's fields (metric_utils.py:138-140)."""
        d = dict(capture_all=self.capture_all, capture_mean_cov=self.capture_mean_cov, max_items=self.max_items,
                 num_items=self.num_items, num_features=self.num_features, all_features=self.all_features,
                 raw_mean=self.raw_mean, raw_cov=self.raw_cov)
        with open(pkl_file, 'wb') as f:
            pickle.dump(d, f)

    @staticmethod
    def load(pkl_file, device='cuda:0'):
        from .formats import _restricted_load          # cache files are data (dict of numpy / python values): never a full unpickle
        with open(pkl_file, 'rb') as f:
            s = _restricted_load(f)
        obj = FeatureStats(capture_all=s['capture_all'], capture_mean_cov=s.get('capture_mean_cov', False),
                           max_items=s['max_items'], device=device)
        obj.num_items, obj.num_features, obj.all_features = s['num_items'], s['num_features'], s['all_features']
        if s.get('raw_mean') is not None and obj.capture_mean_cov:
            obj._mean = torch.from_numpy(np.asarray(s['raw_mean'], dtype=np.float64)).to(obj._dev)
            obj._cov = torch.from_numpy(np.asarray(s['raw_cov'], dtype=np.float64)).to(obj._dev)
        return obj


def compute_fid_from_stats(mu_real, sigma_real, mu_gen, sigma_gen):
    """Frechet distance of two Gaussians (the matrix square root runs on the host with scipy, as in the reference)."""
    m = np.square(mu_gen - mu_real).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_gen, sigma_real), disp=False)
    return float(np.real(m + np.trace(sigma_gen + sigma_real - s * 2)))


def _f16_padded(x, dev):
    """float16 [n][D'] on the device, D' = D rounded up to a multiple of 16 with zero columns (distances unchanged)."""
    x = torch.as_tensor(x).to(dev).to(torch.float16)
    assert x.ndim == 2
    pad = -x.shape[1] % 16
    if pad:
        x = torch.nn.functional.pad(x, [0, pad])
    return x.contiguous()


def compute_distances(row_features, col_features, num_gpus=1, rank=0, col_batch_size=None, device='cuda:0'):
    """Euclidean distance matrix [rows, cols] (float32, on the host like the reference's rank-0 result)."""
    assert num_gpus == 1 and rank == 0, 'the metric path is single-process in every reference driver (SURVEY 2c)'
    dev = torch.device(device)
    lib = _lib.load()
    r, c = _f16_padded(row_features, dev), _f16_padded(col_features, dev)
    dist = torch.empty([r.shape[0], c.shape[0]], dtype=torch.float32, device=dev)
    ws = _lib.workspace(4 * lib.la_pr_workspace_floats(r.shape[0], c.shape[0]), dev, torch.float32)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_cdist_f16(_lib.ptr(r), r.shape[0], _lib.ptr(c), c.shape[0], r.shape[1], _lib.ptr(dist), _lib.ptr(ws),
                                    _lib.stream_ptr()), 'cdist')
    return dist.cpu()


def compute_pr_from_features(real_features, gen_features, nhood_size=3, row_batch_size=10000, col_batch_size=10000,
                             device='cuda:0', return_details=False):
    """(precision, recall) of `gen_features` against `real_features`.  The batch sizes are accepted for interface parity; the
    kernels stream over the columns and never build the distance matrix, so the result does not depend on them."""
    dev = torch.device(device)
    lib = _lib.load()
    feats = {'real': _f16_padded(real_features, dev), 'gen': _f16_padded(gen_features, dev)}
    results, details = {}, {}
    for name, mk, pk in (('precision', 'real', 'gen'), ('recall', 'gen', 'real')):
        manifold, probes = feats[mk], feats[pk]
        nm, npb, D = manifold.shape[0], probes.shape[0], manifold.shape[1]
        ws = _lib.workspace(4 * lib.la_pr_workspace_floats(max(nm, npb), nm), dev, torch.float32)
        kth = torch.empty([nm], dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.la_pr_kth_f16(_lib.ptr(manifold), nm, _lib.ptr(manifold), nm, D, nhood_size, _lib.ptr(kth), _lib.ptr(ws),
                                         _lib.stream_ptr()), 'pr_kth')
        kth = kth.to(torch.float16).to(torch.float32)          # the reference keeps the radii in float16 (precision_recall.py:78)
        member = torch.empty([npb], dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.la_pr_member_f16(_lib.ptr(probes), npb, _lib.ptr(manifold), nm, D, _lib.ptr(kth), _lib.ptr(member),
                                            _lib.ptr(ws), _lib.stream_ptr()), 'pr_member')
        results[name] = float(member.to(torch.float32).mean())
        details[name + '_kth'] = kth.cpu().numpy()
        details[name + '_pred'] = member.cpu().numpy().astype(bool)
    if return_details:
        return results['precision'], results['recall'], details
    return results['precision'], results['recall']


def kid_subset_indices(num_real, num_gen, num_subsets=100, max_subset_size=1000, seed=0):
    """(ix [S][mx] into the generated rows, iy [S][my] into the real rows), int32: per subset m = min(num_real, num_gen,
    max_subset_size) rows of each side without replacement from numpy.random.RandomState(seed), the generated side drawn first.
    max_subset_size=None with num_subsets=1 is the full-set estimator: every row once, in its given order (mx != my allowed)."""
    if num_subsets < 1:
        raise ValueError('num_subsets must be at least 1')
    if max_subset_size is None:
        if num_subsets != 1:
            raise ValueError('max_subset_size=None is the full-set estimator: it needs num_subsets=1')
        ix, iy = np.arange(num_gen, dtype=np.int32)[None], np.arange(num_real, dtype=np.int32)[None]
    else:
        m = min(num_real, num_gen, max_subset_size)
        if m < 2:
            raise ValueError(f'KID needs at least 2 rows per side in a subset (got m = {m})')
        rs = np.random.RandomState(seed)
        ix, iy = np.empty([num_subsets, m], np.int32), np.empty([num_subsets, m], np.int32)
        for s in range(num_subsets):
            ix[s] = rs.choice(num_gen, m, replace=False)
            iy[s] = rs.choice(num_real, m, replace=False)
    if min(ix.shape[1], iy.shape[1]) < 2:
        raise ValueError(f'KID needs at least 2 rows per side (got {ix.shape[1]} generated, {iy.shape[1]} real)')
    return ix, iy


def _f32_features(x, dev):
    x = torch.as_tensor(x)
    if x.ndim != 2 or not x.is_floating_point():
        raise ValueError('features must be a [N, D] array of a float dtype')
    return x.detach().to(dev).to(torch.float32).contiguous()


def compute_kid_from_features(real_features, gen_features, num_subsets=100, max_subset_size=1000, seed=0, device='cuda:0',
                              return_details=False, indices=None):
    """Kernel Inception Distance of `gen_features` against `real_features` ([N, D] numpy arrays or torch tensors of any float dtype,
    computed from their float32 values; FeatureStats(capture_all=True).get_all() is such an array): the mean over `num_subsets`
    subsets of the unbiased MMD^2 estimator with k(a, b) = (a.b / D + 1)^3.  The subsets are those of `kid_subset_indices`;
    `indices=(ix, iy)` supplies them instead ([S][mx] generated rows, [S][my] real rows).  The rows are gathered by the kernel and the
    kernel matrices never leave it (la_kid_poly3_f32); the result is the same bits on every run.
    return_details=True: (kid, {'mmd2': float64 [S], 'sums': float64 [S][3] (xx and yy off-diagonal, xy), 'ix', 'iy'})."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got device ' + str(dev))
    nr, ng = np.shape(real_features)[0], np.shape(gen_features)[0]
    if indices is None:
        ix, iy = kid_subset_indices(nr, ng, num_subsets, max_subset_size, seed)
    else:
        ix, iy = (np.ascontiguousarray(i, dtype=np.int32) for i in indices)
        if ix.ndim != 2 or iy.ndim != 2 or ix.shape[0] != iy.shape[0] or ix.shape[0] < 1 or min(ix.shape[1], iy.shape[1]) < 2:
            raise ValueError('indices: ([S][mx], [S][my]) with S >= 1 and at least 2 rows per side')
        if ix.min() < 0 or ix.max() >= ng or iy.min() < 0 or iy.max() >= nr:
            raise ValueError('indices: a row number outside its feature matrix')
    if not torch.cuda.is_available():
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); none is available')
    lib = _lib.load()
    real, gen = _f32_features(real_features, dev), _f32_features(gen_features, dev)
    if real.shape[1] != gen.shape[1] or real.shape[1] < 1:
        raise ValueError(f'feature dimensions differ or are empty: real {tuple(real.shape)}, generated {tuple(gen.shape)}')
    S, mx, my = ix.shape[0], ix.shape[1], iy.shape[1]
    ixd, iyd = torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev)
    out = torch.empty([S * 4 + 1], dtype=torch.float64, device=dev)          # sums [S][3], mmd2 [S], kid [1]
    ws_bytes = lib.la_kid_workspace_bytes(S, mx, my)
    ws = _lib.workspace(ws_bytes, dev, torch.float64)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_kid_poly3_f32(_lib.ptr(gen), gen.shape[0], _lib.ptr(real), real.shape[0], gen.shape[1], _lib.ptr(ixd),
                                        _lib.ptr(iyd), S, mx, my, _lib.ptr(out), _lib.ptr(out[S * 3:]), _lib.ptr(out[S * 4:]),
                                        _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'kid_poly3')
    out = out.cpu().numpy()
    kid = float(out[S * 4])
    if return_details:
        return kid, dict(mmd2=out[S * 3:S * 4].copy(), sums=out[:S * 3].reshape(S, 3).copy(), ix=ix, iy=iy)
    return kid


FD_MAX_SMALL_SIDE = 8192        # la_frechet.hip rotates min(Ng, Nr) vectors; beyond this the moments route is the right one


def compute_fd_from_features(real_features, gen_features, device='cuda:0', return_details=False, max_sweeps=30):
    """Frechet distance of `gen_features` against `real_features` ([N, D] numpy arrays or device tensors of any float dtype, computed
    from their float32 values) -- the number `compute_fid_from_stats` gives for the moments of the same features, without a covariance
    matrix or a matrix square root.  With A [Ng][D], B [Nr][D] the two sets minus their column means and the reference's 1/N covariance:
        FD = |mu_g - mu_r|^2 + |A|_F^2 / Ng + |B|_F^2 / Nr - 2 nuc(A B^T) / sqrt(Ng Nr)
    nuc = the sum of the singular values of the Ng x Nr cross-Gram matrix, which one-sided Jacobi sweeps (la_fd_jacobi_sweep_f64) find in
    float64: singular values of a singular matrix are well conditioned where its square root is not, so the result is exact in the
    few-samples regime (N < D) too.  Sweeps run until one makes no rotation; `max_sweeps` reached raises.  The value is not clamped at 0
    (the reference's is not either); two calls give the same bits.  Like compute_fid_from_stats it is features-in: the Inception-v3
    detector of the published FID is not available offline, so the name of the number depends on the detector the features came from.
    min(Ng, Nr) > 8192 is refused: that regime belongs to FeatureStats moments and compute_fid_from_stats.  There is no CPU fallback.
    return_details=True: (fd, {'mean_term', 'trace_gen' and 'trace_real' (divided by N), 'nuclear' (divided by sqrt(Ng Nr)), 'sweeps',
    'singular_values': float64 [min(Ng, Nr)] of A B^T in vector order, 'terms': the four raw float64 sums})."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got device ' + str(dev))
    for f in (real_features, gen_features):
        if torch.is_tensor(f):
            _lib.require_gpu(f)
    rshape, gshape = tuple(np.shape(real_features)), tuple(np.shape(gen_features))
    if len(rshape) != 2 or len(gshape) != 2 or rshape[1] != gshape[1] or rshape[1] < 1:
        raise _lib.LatentAugHipError(f'features must be two [N, D] arrays of one D >= 1: real {rshape}, generated {gshape}')
    nr, ng, D = rshape[0], gshape[0], rshape[1]
    if min(nr, ng) < 2:
        raise _lib.LatentAugHipError(f'the Frechet distance needs at least 2 samples per side (got {nr} real, {ng} generated)')
    if min(nr, ng) > FD_MAX_SMALL_SIDE:
        raise _lib.LatentAugHipError(f'min(Ng, Nr) = {min(nr, ng)} > {FD_MAX_SMALL_SIDE}: the many-samples regime belongs to FeatureStats '
                                     'moments and compute_fid_from_stats')
    if not torch.cuda.is_available():
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); none is available')
    lib = _lib.load()
    real, gen = _f32_features(real_features, dev), _f32_features(gen_features, dev)
    n, m = min(ng, nr), max(ng, nr)
    ws_bytes = lib.la_fd_workspace_bytes(ng, nr, D)
    ws = _lib.workspace(ws_bytes, dev, torch.float64)          # the n' vectors of m doubles come first
    out = torch.empty([4 + n], dtype=torch.float64, device=dev)                # terms [4], singular values [n]
    rot = torch.empty([1], dtype=torch.int32, device=dev)
    sweeps = 0
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_fd_gram_f32(_lib.ptr(gen), ng, _lib.ptr(real), nr, D, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()),
                   'fd_gram')
        while True:
            _lib.check(lib.la_fd_jacobi_sweep_f64(_lib.ptr(ws), n, m, _lib.ptr(rot), _lib.stream_ptr()), 'fd_jacobi_sweep')
            sweeps += 1
            if int(rot.item()) == 0:          # one integer per sweep: the number of sweeps depends on the data
                break
            if sweeps >= max_sweeps:
                raise _lib.LatentAugHipError(f'Frechet distance: the Jacobi sweeps did not converge in max_sweeps = {max_sweeps} '
                                             f'({int(rot.item())} rotations in the last one); sets with D < N or many duplicated rows '
                                             'need the most sweeps: raise max_sweeps, or use compute_fid_from_stats there')
        _lib.check(lib.la_fd_finish_f64(_lib.ptr(ws), ws_bytes, ng, nr, D, _lib.ptr(out[4:]), _lib.ptr(out), _lib.stream_ptr()), 'fd_finish')
    out = out.cpu().numpy()
    mean_term, trace_gen, trace_real = float(out[0]), float(out[1]) / ng, float(out[2]) / nr
    nuclear = float(out[3]) / float(np.sqrt(float(ng) * float(nr)))
    fd = mean_term + trace_gen + trace_real - 2.0 * nuclear
    if return_details:
        return fd, dict(mean_term=mean_term, trace_gen=trace_gen, trace_real=trace_real, nuclear=nuclear, sweeps=sweeps,
                        singular_values=out[4:].copy(), terms=out[:4].copy())
    return fd


def compute_dc_from_features(real_features, gen_features, nhood_size=5, device='cuda:0', return_details=False):
    """(density, coverage) of `gen_features` against `real_features` ([N, D] arrays or tensors, rounded to float16 as the precision /
    recall path does): Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", ICML 2020.  Only the balls of the
    real samples are used.  With r_i the (nhood_size + 1)-th smallest distance from real i to all reals, its own zero included
    (la_pr_kth_f16(real, real), kept in float32 -- unlike compute_pr_from_features, whose radii pass through float16 as the
    reference's do):
        count[j] = #{ i : dist(gen_j, real_i) <= r_i },   density  = sum_j count[j] / (nhood_size * ng)   (the sum in integers)
        nearest[i] = min_j dist(gen_j, real_i),           coverage = mean_i (nearest[i] <= r_i)
    The comparison is <=, as in compute_pr_from_features (precision_recall.py:83); the `prdc` package uses <.  The two differ only
    where a distance equals a radius exactly.  One pass over the pair grid (la_dc_count_f16) gives count and nearest; the distance
    matrix is never built and two runs give the same bits.  nhood_size must lie in 1 .. min(7, nr - 1): the radii kernel keeps 8
    candidates per row.  There is no CPU fallback.
    return_details=True: (density, coverage, {'radii': float32 [nr], 'count': int32 [ng], 'nearest': float32 [nr], 'covered': bool [nr]})."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got device ' + str(dev))
    rshape, gshape = tuple(np.shape(real_features)), tuple(np.shape(gen_features))
    if len(rshape) != 2 or len(gshape) != 2 or rshape[1] != gshape[1] or rshape[1] < 1 or rshape[0] < 1 or gshape[0] < 1:
        raise ValueError(f'features must be two non-empty [N, D] arrays of one D: real {rshape}, generated {gshape}')
    nr, ng = rshape[0], gshape[0]
    if int(nhood_size) != nhood_size or not 1 <= nhood_size <= min(7, nr - 1):
        raise ValueError(f'nhood_size must lie in 1 .. min(7, nr - 1) = {min(7, nr - 1)} (got {nhood_size} with nr = {nr})')
    k = int(nhood_size)
    if not torch.cuda.is_available():
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); none is available')
    lib = _lib.load()
    real, gen = _f16_padded(real_features, dev), _f16_padded(gen_features, dev)
    D = real.shape[1]
    radii = torch.empty([nr], dtype=torch.float32, device=dev)
    count = torch.empty([ng], dtype=torch.int32, device=dev)
    nearest = torch.empty([nr], dtype=torch.float32, device=dev)
    ws_bytes = max(lib.la_dc_workspace_bytes(ng, nr), 4 * lib.la_pr_workspace_floats(nr, nr))
    ws = _lib.workspace(ws_bytes, dev, torch.float32)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_pr_kth_f16(_lib.ptr(real), nr, _lib.ptr(real), nr, D, k, _lib.ptr(radii), _lib.ptr(ws), _lib.stream_ptr()),
                   'pr_kth')
        _lib.check(lib.la_dc_count_f16(_lib.ptr(gen), ng, _lib.ptr(real), nr, D, _lib.ptr(radii), _lib.ptr(count), _lib.ptr(nearest),
                                       _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'dc_count')
    covered = nearest <= radii
    density = int(count.sum(dtype=torch.int64)) / (k * ng)
    coverage = int(covered.sum()) / nr
    if return_details:
        return density, coverage, dict(radii=radii.cpu().numpy(), count=count.cpu().numpy(), nearest=nearest.cpu().numpy(),
                                       covered=covered.cpu().numpy())
    return density, coverage


def compute_prdc_from_features(real_features, gen_features, nhood_size=5, device='cuda:0'):
    """{'precision', 'recall', 'density', 'coverage'} with one nhood_size: compute_pr_from_features (radii of the real and of the
    generated manifold, rounded to float16 as the reference keeps them) and compute_dc_from_features (radii of the real samples only,
    float32), each with its own documented convention."""
    precision, recall = compute_pr_from_features(real_features, gen_features, nhood_size=nhood_size, device=device)
    density, coverage = compute_dc_from_features(real_features, gen_features, nhood_size=nhood_size, device=device)
    return dict(precision=precision, recall=recall, density=density, coverage=coverage)


# ------------------------------------------------------------------------------------------------------------
# questions about a SINGLE sample (la_knn.hip; float64 arithmetic on the float32 features, no CPU fallback)
KNN_MAX_K = 32


def _query_features(device, **named):
    """The device and the float32 device copies of [N, D] feature arrays that must agree in D, in the order given."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got device ' + str(dev))
    shapes = {n: tuple(np.shape(f)) for n, f in named.items()}
    if any(len(s) != 2 or s[0] < 1 or s[1] < 1 for s in shapes.values()) or len({s[1] for s in shapes.values()}) != 1:
        raise ValueError(f'features must be non-empty [N, D] arrays of one D: {shapes}')
    if not torch.cuda.is_available():
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); none is available')
    return dev, [_f32_features(f, dev) for f in named.values()]


def _knn_device(query, bank, k, exclude_self):
    """la_knn_f32 on float32 device tensors -> (dist2 float64 [nq, k], idx int32 [nq, k]) on the device"""
    lib = _lib.load()
    dev, (nq, D), nx = query.device, query.shape, bank.shape[0]
    dist2 = torch.empty([nq, k], dtype=torch.float64, device=dev)
    idx = torch.empty([nq, k], dtype=torch.int32, device=dev)
    nbytes = lib.la_knn_scratch_bytes(nq, nx, D, k)
    scratch = _lib.workspace(nbytes, dev, torch.float64)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_knn_f32(_lib.ptr(query), nq, _lib.ptr(bank), nx, D, k, int(bool(exclude_self)), _lib.ptr(dist2), _lib.ptr(idx),
                                  _lib.ptr(scratch), nbytes, _lib.stream_ptr()), 'knn')
    return dist2, idx


def knn_from_features(query, bank, k, exclude_self=False, device='cuda:0'):
    """The `k` nearest rows of `bank` for every row of `query` ([N, D] numpy arrays or tensors of any float dtype, computed from their
    float32 values): (dist float64 [nq, k] ascending, idx int64 [nq, k]) as numpy arrays -- the Euclidean distance, the square root
    of la_knn_f32's d2 = max(0, |q|^2 + |x|^2 - 2 q.x) with all three sums in float64 (off the exact value by at most
    (2 D + 4) 2^-53 (|q|^2 + |x|^2)).  The order is (distance, index): of two equally distant rows the lower index comes first.
    exclude_self=True (query and bank of one length: the same set) leaves row i out of the neighbours of query i.  Where a query has
    fewer than k candidates the remaining slots hold idx = -1 and dist = inf.  1 <= k <= 32.  The distance matrix is never built and
    two calls give the same bits.  (idx, dist) is the `precomputed_knn` form of a UMAP of the latents.  There is no CPU fallback."""
    if int(k) != k or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f'k must lie in 1 .. {KNN_MAX_K} (got {k})')
    dev, (q, x) = _query_features(device, query=query, bank=bank)
    if exclude_self and q.shape[0] != x.shape[0]:
        raise ValueError(f'exclude_self needs query and bank of one length (got {q.shape[0]} and {x.shape[0]})')
    dist2, idx = _knn_device(q, x, int(k), exclude_self)
    return np.sqrt(dist2.cpu().numpy()), idx.cpu().numpy().astype(np.int64)


def compute_realism_from_features(real_features, gen_features, nhood_size=3, keep_fraction=0.5, device='cuda:0', return_details=False):
    """Realism score of every generated sample (Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative
    Models", NeurIPS 2019, section 5): float64 [ng],
        realism[j] = max over the kept real i of radius[i] / dist(gen_j, real_i)
    radius[i] is the distance of real i to its `nhood_size`-th nearest OTHER real sample (knn of the reals among themselves with
    exclude_self).  Only the ceil(keep_fraction nr) spheres with the smallest radii are kept, ties by lower index: the paper prunes
    the large spheres of outliers at its 0.5.  A generated sample that equals a kept real one scores inf.  With keep_fraction=1,
    realism >= 1 is exactly "inside some real sphere", the membership behind `precision` -- here in float64 arithmetic on the float32
    features (la_realism_f32: the quotient of squared distances, then one square root), where compute_pr_from_features stays on the
    reference's float16 distances and float16 radii; near a sphere's surface the two can differ.  1 <= nhood_size <= min(32, nr - 1).
    Two calls give the same bits.  There is no CPU fallback.
    return_details=True: (realism, {'radii': float64 [nr], 'kept': bool [nr], 'arg': int64 [ng], the real sample whose sphere gives
    the score (ties to the lower index)})."""
    dev, (real, gen) = _query_features(device, real=real_features, gen=gen_features)
    nr, ng, D = real.shape[0], gen.shape[0], real.shape[1]
    if int(nhood_size) != nhood_size or not 1 <= nhood_size <= min(KNN_MAX_K, nr - 1):
        raise ValueError(f'nhood_size must lie in 1 .. min({KNN_MAX_K}, nr - 1) = {min(KNN_MAX_K, nr - 1)} (got {nhood_size} with nr = {nr})')
    if not 0 < keep_fraction <= 1:
        raise ValueError(f'keep_fraction must lie in (0, 1] (got {keep_fraction})')
    lib = _lib.load()
    radius2 = _knn_device(real, real, int(nhood_size), True)[0][:, int(nhood_size) - 1].cpu().numpy()
    kept = np.zeros([nr], dtype=bool)
    kept[np.argsort(radius2, kind='stable')[:int(np.ceil(keep_fraction * nr))]] = True
    r2 = torch.from_numpy(np.where(kept, radius2, -1.0)).to(dev)          # a negative radius drops the sphere
    score2 = torch.empty([ng], dtype=torch.float64, device=dev)
    arg = torch.empty([ng], dtype=torch.int32, device=dev)
    nbytes = lib.la_knn_scratch_bytes(ng, nr, D, 1)
    scratch = _lib.workspace(nbytes, dev, torch.float64)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_realism_f32(_lib.ptr(gen), ng, _lib.ptr(real), nr, D, _lib.ptr(r2), _lib.ptr(score2), _lib.ptr(arg),
                                      _lib.ptr(scratch), nbytes, _lib.stream_ptr()), 'realism')
    realism = np.sqrt(score2.cpu().numpy())
    if return_details:
        return realism, dict(radii=np.sqrt(radius2), kept=kept, arg=arg.cpu().numpy().astype(np.int64))
    return realism


def compute_authenticity_from_features(real_features, gen_features, device='cuda:0', return_details=False):
    """Authenticity (Alaa et al., "How Faithful is your Synthetic Data?", ICML 2022): the share of generated samples that are not
    near-copies of a real one.  For generated j with nearest real i*: d_gen = dist(gen_j, real_i*), d_real = the distance of real i*
    to its nearest other real; j is authentic iff d_gen > d_real -- a copy sits closer to its source than any other real sample does.
    Distances as in knn_from_features (float64 on the float32 features; a float16 distance has no digits left at the distance of a
    near-copy).  Needs at least 2 real samples.  Two calls give the same bits.  There is no CPU fallback.
    return_details=True: (authenticity, {'authentic': bool [ng], 'nearest': int64 [ng] (i*), 'd_gen', 'd_real': float64 [ng]})."""
    dev, (real, gen) = _query_features(device, real=real_features, gen=gen_features)
    if real.shape[0] < 2:
        raise ValueError('authenticity needs at least 2 real samples')
    d2g, ig = _knn_device(gen, real, 1, False)
    d2r, _ = _knn_device(real, real, 1, True)
    nearest = ig[:, 0].cpu().numpy().astype(np.int64)
    d_gen, d_real = np.sqrt(d2g[:, 0].cpu().numpy()), np.sqrt(d2r[:, 0].cpu().numpy())[nearest]
    authentic = d_gen > d_real
    authenticity = float(authentic.mean())
    if return_details:
        return authenticity, dict(authentic=authentic, nearest=nearest, d_gen=d_gen, d_real=d_real)
    return authenticity


# ------------------------------------------------------------------------------------------------------------
# images -> detector features -> FeatureStats (synthesis.DetectorEngine; no CPU fallback)
def _batch_images(batch, mode):
    if isinstance(batch, dict):
        if mode not in ('A', 'B'):
            raise ValueError("batches of output dicts need mode='A' or mode='B'")
        batch = batch[mode]
    if not torch.is_tensor(batch) or batch.ndim != 4:
        raise ValueError('a batch must be a [N, 1|3, H, W] tensor, or a dict that holds one under its mode')
    return batch


def compute_feature_stats_for_images(batches, detector, mode=None, max_items=None, **stats_kwargs):
    """FeatureStats of the detector features of `batches`: an iterable of [N, 1|3, H, W] tensors in the generator's [-1, 1] range, or
    of the augmentation plugins' output dicts (then `mode` in {'A', 'B'} picks the modality).  Each batch is quantised to the uint8
    grid, repeated to three channels and run through `detector` (metrics/metric_utils.py:314-319) on the device; `max_items` cuts
    the last batch as FeatureStats does."""
    stats = FeatureStats(max_items=max_items, device=detector.device, **stats_kwargs)
    for batch in batches:
        x = _batch_images(batch, mode).to(detector.device)
        stats.append_torch(detector.features(x, quantize=True))
        if stats.is_full():
            break
    return stats


def compute_feature_stats_for_aug_dataset(datadir, mode, detector, max_items=None, cache_file=None, **stats_kwargs):
    """metrics/metric_utils.py:264-328 for a local detector: the `img_aug/` pickles that the reference's drivers write
    (backbone_latentaug.py: one dict of image batches per file) -> FeatureStats.  The pickles are read through the allow-list
    loader of formats.py, never a plain unpickle.  `cache_file`: loaded if it exists, else written (atomically) in the
    FeatureStats.save layout."""
    if cache_file is not None and os.path.isfile(cache_file):
        return FeatureStats.load(cache_file, device=detector.device)
    from .formats import _restricted_load
    files = sorted(f for f in glob.glob(os.path.join(datadir, 'img_aug', '*')) if os.path.isfile(f))
    if not files:
        raise FileNotFoundError(f"no augmented batches under {os.path.join(datadir, 'img_aug')}")

    def batches():
        for fname in files:
            with open(fname, 'rb') as f:
                yield _restricted_load(f)
    stats = compute_feature_stats_for_images(batches(), detector, mode=mode, max_items=max_items, **stats_kwargs)
    if cache_file is not None:
        os.makedirs(os.path.dirname(os.path.abspath(cache_file)), exist_ok=True)
        tmp = cache_file + '.' + uuid.uuid4().hex
        stats.save(tmp)
        os.replace(tmp, cache_file)
    return stats


def compute_metrics_from_images(real_batches, gen_batches, detector, nhood_size=3, mode=None, max_items=None, kid_num_subsets=100,
                                kid_max_subset_size=1000, kid_seed=0, frechet=False, realism=False, authenticity=False, swd=False, **swd_kwargs):
    """{'precision', 'recall', 'density', 'coverage', 'kid'} of generated against real images, through `detector` and the functions
    above (precision_recall.py:36-85 with nhood_size=3 is the reference's pr50k3).  frechet=True adds 'fd', the Frechet distance of the
    same detector features (compute_fd_from_features; with the VGG16 detector it is not the published Inception FID).  realism=True
    adds 'realism', the mean realism score of the generated images (compute_realism_from_features with this nhood_size), and
    authenticity=True adds 'authenticity' (compute_authenticity_from_features), both from the same features.  swd=True adds the
    'swd_<res>' and 'swd_avg' keys of compute_swd_from_images (to which `swd_kwargs` go) from the same batches, which are then held as
    lists; it needs no detector features.  With swd=False nothing of it is launched."""
    if swd:
        real_batches, gen_batches = list(real_batches), list(gen_batches)
    real = compute_feature_stats_for_images(real_batches, detector, mode=mode, max_items=max_items, capture_all=True).get_all()
    gen = compute_feature_stats_for_images(gen_batches, detector, mode=mode, max_items=max_items, capture_all=True).get_all()
    out = compute_prdc_from_features(real, gen, nhood_size=nhood_size, device=detector.device)
    out['kid'] = compute_kid_from_features(real, gen, num_subsets=kid_num_subsets, max_subset_size=kid_max_subset_size, seed=kid_seed,
                                           device=detector.device)
    if frechet:
        out['fd'] = compute_fd_from_features(real, gen, device=detector.device)
    if realism:
        out['realism'] = float(compute_realism_from_features(real, gen, nhood_size=nhood_size, device=detector.device).mean())
    if authenticity:
        out['authenticity'] = compute_authenticity_from_features(real, gen, device=detector.device)
    if swd:
        held = min(sum(int(_batch_images(b, mode).shape[0]) for b in side) for side in (real_batches, gen_batches))
        out.update(compute_swd_from_images(real_batches, gen_batches, mode=mode, num_items=held if max_items is None else min(held, max_items),
                                           device=detector.device, **swd_kwargs))
    return out


# ------------------------------------------------------------------------------------------------------------
# paired image metrics (la_pairmetrics.hip; no reference counterpart, no CPU fallback)
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)          # Wang, Simoncelli, Bovik 2003
_PAIR_WORKSPACE_BYTES = 256 << 20                                   # pairs are chunked so that one call's workspace stays below this


def gaussian_window(win_size=11, win_sigma=1.5):
    """The `win_size` taps g[k] = exp(-(k - win_size // 2)^2 / (2 sigma^2)) normalised to sum 1, float64."""
    if int(win_size) != win_size or not 1 <= win_size <= 11 or win_size % 2 == 0:
        raise ValueError(f'win_size must be odd and lie in 1 .. 11 (got {win_size})')
    if not win_sigma > 0:
        raise ValueError(f'win_sigma must be positive (got {win_sigma})')
    k = np.arange(int(win_size), dtype=np.float64) - int(win_size) // 2
    g = np.exp(-(k * k) / (2.0 * float(win_sigma) ** 2))
    return g / g.sum()


def msssim_weights(levels, weights=None):
    """float32 level weights of MS-SSIM: the caller's, or the first `levels` of MS_SSIM_WEIGHTS (divided by their sum when levels < 5)."""
    if int(levels) != levels or not 1 <= levels <= 5:
        raise ValueError(f'levels must lie in 1 .. 5 (got {levels})')
    if weights is None:
        w = np.asarray(MS_SSIM_WEIGHTS[:levels], dtype=np.float64)
        if levels < 5:
            w = w / w.sum()
    else:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (levels,) or not (w >= 0).all():
            raise ValueError(f'weights: {levels} non-negative numbers, one per level')
    return w.astype(np.float32)


def _device_images(t, name):
    if not torch.is_tensor(t):
        raise _lib.LatentAugHipError(f'{name}: latentaugment_amd needs a ROCm device tensor (no CPU fallback); got {type(t).__name__}')
    _lib.require_gpu(t)
    if t.dtype != torch.float32:
        raise _lib.LatentAugHipError(f'{name}: the paired metrics take float32 images; got {t.dtype}')
    if t.ndim != 4 or min(t.shape) < 1:
        raise ValueError(f'{name}: images must be a non-empty [N, C, H, W] tensor; got {tuple(t.shape)}')
    return t.detach().contiguous()


def _pair_indices(pairs, nx, ny):
    ix, iy = (np.ascontiguousarray(i, dtype=np.int32) for i in pairs)
    if ix.ndim != 1 or ix.shape != iy.shape or ix.size < 1:
        raise ValueError('pairs: (ix [P], iy [P]) with P >= 1')
    if ix.min() < 0 or ix.max() >= nx or iy.min() < 0 or iy.max() >= ny:
        raise ValueError('pairs: an image number outside its batch')
    return ix, iy


def _pair_row_batches(x, y, net, pairs, name, entry, clamp=None):
    """The plumbing compute_lpips and compute_style_content share: checks the images against the engine (`entry`: the method of
    synthesis.FeatureEngine the caller needs), then yields (p0, n, xy) per chunk of `chunk` pairs -- xy [2 C n, 3, R, R] float32, every
    channel of the n pairs from p0 on repeated to three channels with the net's input affine, rows c * n + b, the x rows then the y
    rows (la_crop_repeat_affine_f32).  pairs=(ix, iy) are gathered chunk by chunk with index_select; clamp=(lo, hi) clamps the images
    first.  Returns (P, C, device, chunk, the generator); the generator runs under torch.cuda.device(device)."""
    x, y = _device_images(x, 'x'), _device_images(y, 'y')
    if x.device != y.device or x.shape[1:] != y.shape[1:]:
        raise ValueError(f'x and y must be on one device and agree in [C, H, W]: {tuple(x.shape)} on {x.device}, {tuple(y.shape)} on {y.device}')
    if not hasattr(net, entry):
        raise _lib.LatentAugHipError(f'{name}: net must be a synthesis.FeatureEngine; got {type(net).__name__}')
    per_call = net.pair_rows()          # (refuses a detector engine)
    C_, H, W = (int(s) for s in x.shape[1:])
    if net.in_ch != 3 or H != net.in_res or W != net.in_res:
        raise ValueError(f'{name}: the net takes [3, {net.in_res}, {net.in_res}] inputs (in_ch {net.in_ch}); the images are [{C_}, {H}, {W}]')
    if x.device != net.device:
        raise ValueError(f'{name}: images on {x.device}, net on {net.device}')
    dev, R = x.device, H
    if pairs is None:
        if x.shape[0] != y.shape[0]:
            raise ValueError('without pairs, x and y must hold the same number of images')
        P, ixd, iyd = int(x.shape[0]), None, None
    else:
        ix, iy = _pair_indices(pairs, x.shape[0], y.shape[0])
        P, ixd, iyd = int(ix.size), torch.from_numpy(ix).to(dev).long(), torch.from_numpy(iy).to(dev).long()
    chunk = per_call // C_
    if chunk < 1:
        raise _lib.LatentAugHipError(f'{name}: one pair of {C_}-channel images is {2 * C_} rows; the net has max_batch = {net.max_batch}')
    lib = _lib.load()
    sc, sh = (C.c_float * 3)(*net.pre_scale), (C.c_float * 3)(*net.pre_shift)

    def batches():
        with torch.cuda.device(dev):
            for p0 in range(0, P, chunk):
                n = min(chunk, P - p0)
                xa = x[p0:p0 + n] if pairs is None else x.index_select(0, ixd[p0:p0 + n])
                ya = y[p0:p0 + n] if pairs is None else y.index_select(0, iyd[p0:p0 + n])
                if clamp is not None:
                    xa, ya = xa.clamp(*clamp), ya.clamp(*clamp)
                xy = torch.empty([2 * C_ * n, 3, R, R], dtype=torch.float32, device=dev)          # rows c * n + b, x then y
                for half, src in enumerate((xa, ya)):
                    _lib.check(lib.la_crop_repeat_affine_f32(_lib.ptr(src), _lib.ptr(xy[half * C_ * n:]), n, C_, R, R, 0, 0, 3, sc, sh,
                                                             _lib.stream_ptr()), 'la_crop_repeat')
                yield p0, n, xy
    return P, C_, dev, chunk, batches()


def compute_lpips(x, y, net, pairs=None):
    """LPIPS distance per pair of images, modality by modality, the way the perceptual criterion feeds its net
    (util_latent_aug.py:387-409): every channel of x[p] and of y[p] is repeated to three channels, given the net's input affine
    (`net.pre_scale`, `net.pre_shift`) and sent through `net`, a synthesis.FeatureEngine of three input channels; the distance comes
    from one fused launch per tap (FeatureEngine.pair_distance_rows), no feature vector is written.  x, y: float32 device tensors
    [N, C, R, R] with R == net.in_res (whole frames, not crops), values in the range the net expects ([-1, 1] for
    lpips_reference_net, whose net_type 'alex' gives the LPIPS-Alex number most papers report).  Pair p is (x[p], y[p]), or (x[ix[p]], y[iy[p]]) with pairs=(ix, iy), gathered chunk by chunk with
    index_select.  Returns float64 CPU tensors: 'lpips' [P] (mean over channels), 'lpips_per_channel' [P, C] (sum over taps),
    'lpips_layers' [P, C, ntaps].  Two calls give the same bits.  There is no CPU fallback."""
    P, C_, dev, _, batches = _pair_row_batches(x, y, net, pairs, 'compute_lpips', 'pair_distance_rows')
    out = torch.empty([P, C_, net.num_taps], dtype=torch.float64, device=dev)
    for p0, n, xy in batches:
        d = torch.empty([C_ * n, net.num_taps], dtype=torch.float64, device=dev)
        net.pair_distance_rows(xy, C_ * n, d)
        out[p0:p0 + n] = d.reshape(C_, n, net.num_taps).permute(1, 0, 2)
    layers = out.cpu()
    per_channel = layers.sum(dim=2)
    return {'lpips': per_channel.mean(dim=1), 'lpips_per_channel': per_channel, 'lpips_layers': layers}


NST_CONTENT_TAP = 3                                                  # synthesis.NST_CONTENT_TAP (networks.py:11: content_layers ['19'])
_NST_CLAMP = (-128.0 / 127.5, 127.0 / 127.5)                        # where (x * 127.5 + 128).clamp(0, 255) of networks.py:38 acts, in x


def compute_style_content(x, y, net, pairs=None, content_tap=NST_CONTENT_TAP, clamp=True):
    """Gram-matrix style distance and content distance per pair of images: the reference's `NSTLoss` on the taps of its `VGG19Net`
    (augments/criteria/nst), which says in WHICH way a sample moved from its source -- texture (feature co-occurrence, the modality's
    look) or spatial content (the anatomy).  Plumbing of compute_lpips: modality by modality, every channel of x[p] and y[p] repeated
    to three channels with the net's input affine (`net.pre_scale`, `net.pre_shift`), both images of a pair rows of one batch, chunks
    of max_batch // 2 rows; `net` is a synthesis.FeatureEngine of a tap list, e.g. of synthesis.nst_reference_net.  clamp=True clamps
    the images to [-128/127.5, 127/127.5] first: the reference's clamp(0, 255), moved in front of the affine.  Per pair, channel and
    tap (la_feat_style_distance): style = mean over C^2 of (G1 - G2)^2 with G = F F^T / HW, content = mean over C HW of (f1 - f2)^2.
    Returns float64 CPU tensors: 'style' [P] (sum over taps, mean over channels), 'content' [P] (tap `content_tap`, mean over
    channels), 'style_per_channel', 'content_per_channel' [P, C], 'style_layers', 'content_layers' [P, C, ntaps].  d(x, x) is exactly
    0, d(x, y) = d(y, x) and two calls give the same bits.  There is no CPU fallback."""
    P, C_, dev, chunk, batches = _pair_row_batches(x, y, net, pairs, 'compute_style_content', 'style_distance_rows',
                                                   _NST_CLAMP if clamp else None)
    nt = net.num_taps
    if not 0 <= int(content_tap) < nt:
        raise ValueError(f'content_tap must lie in 0 .. {nt - 1} (got {content_tap})')
    style = torch.empty([P, C_, nt], dtype=torch.float64, device=dev)
    content = torch.empty([P, C_, nt], dtype=torch.float64, device=dev)
    scratch = _lib.workspace(net.style_scratch_bytes(C_ * min(chunk, P)), dev, torch.float64)
    for p0, n, xy in batches:
        s = torch.empty([C_ * n, nt], dtype=torch.float64, device=dev)
        c = torch.empty([C_ * n, nt], dtype=torch.float64, device=dev)
        net.style_distance_rows(xy, C_ * n, s, c, scratch)
        style[p0:p0 + n] = s.reshape(C_, n, nt).permute(1, 0, 2)
        content[p0:p0 + n] = c.reshape(C_, n, nt).permute(1, 0, 2)
    style_layers, content_layers = style.cpu(), content.cpu()
    style_pc, content_pc = style_layers.sum(dim=2), content_layers[:, :, int(content_tap)].contiguous()
    return {'style': style_pc.mean(dim=1), 'content': content_pc.mean(dim=1), 'style_per_channel': style_pc, 'content_per_channel': content_pc,
            'style_layers': style_layers, 'content_layers': content_layers}


def compute_lpips_diversity(images, net, num_pairs=1000, seed=0):
    """Mean LPIPS distance over `msssim_diversity_pairs(N, num_pairs, seed)` of one image set [N, C, R, R] (float32, on the device):
    near 0 means that the samples resemble one another.  The trunk is recomputed for both images of every pair (about 0.1 ms per
    256^2 image: cheaper than keeping the activations of every image).  Returns {'mean': float, 'lpips': float64 [P], 'ix', 'iy'}."""
    images = _device_images(images, 'images')
    ix, iy = msssim_diversity_pairs(images.shape[0], num_pairs, seed)
    d = compute_lpips(images, images, net, pairs=(ix, iy))['lpips']
    return dict(mean=float(d.mean()), lpips=d, ix=ix, iy=iy)


def compute_pair_metrics(x, y, pairs=None, data_range=2.0, win_size=11, win_sigma=1.5, levels=5, weights=None, lpips_net=None, nst_net=None):
    """Per pair of images: MSE, MAE, PSNR, SSIM and MS-SSIM.  x, y: float32 device tensors [N, C, H, W] in a range of width
    `data_range` (2 for the generator's [-1, 1]).  Pair p is (x[p], y[p]), or (x[ix[p]], y[iy[p]]) with pairs=(ix, iy); the kernel
    gathers, the images are not copied.  A Gaussian window of `win_size` taps (odd, 1 .. 11) and `win_sigma`, 'valid' extent;
    `levels` pyramid levels (1 .. 5) by 2 x 2 means, so H and W must be multiples of 2^(levels-1) and the last level at least the
    window; levels=1 is plain SSIM.  MS-SSIM is prod_{l<levels-1} max(cs_l, 0)^w_l * max(ssim_last, 0)^w_last with `msssim_weights`.
    Returns float64 CPU tensors: 'mse', 'mae', 'psnr', 'ssim', 'ms_ssim' [P] -- the mean over channels, psnr = 10 log10(L^2 / mse) of
    that mean (inf at 0) -- their '*_per_channel' forms [P, C], and 'ssim_levels', 'cs_levels' [P, C, levels].
    Two calls give the same bits (la_pair_metrics_f32).  There is no CPU fallback.
    lpips_net (a synthesis.FeatureEngine, e.g. of lpips_reference_net, with in_res == H == W): adds the keys of compute_lpips for the
    same pairs; without it the result is what it was.
    nst_net (a synthesis.FeatureEngine of synthesis.nst_reference_net, in_res == H == W): adds the keys of compute_style_content for
    the same pairs, likewise."""
    x, y = _device_images(x, 'x'), _device_images(y, 'y')
    if x.device != y.device or x.shape[1:] != y.shape[1:]:
        raise ValueError(f'x and y must be on one device and agree in [C, H, W]: {tuple(x.shape)} on {x.device}, {tuple(y.shape)} on {y.device}')
    if not data_range > 0:
        raise ValueError('data_range must be positive')
    taps = gaussian_window(win_size, win_sigma).astype(np.float32)
    w = msssim_weights(levels, weights)
    win, levels = int(win_size), int(levels)
    C, H, W = (int(s) for s in x.shape[1:])
    dev = x.device
    if pairs is None:
        if x.shape[0] != y.shape[0]:
            raise ValueError('without pairs, x and y must hold the same number of images')
        P, ixd, iyd = int(x.shape[0]), None, None
    else:
        ix, iy = _pair_indices(pairs, x.shape[0], y.shape[0])
        P, ixd, iyd = int(ix.size), torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev)
    lib = _lib.load()
    per_pair = lib.la_pair_metrics_workspace_bytes(1, C, H, W, win, levels)
    if per_pair == 0:
        raise ValueError(f'pair metrics: [{C}, {H}, {W}] images with win_size {win} and {levels} levels are refused: H and W must be '
                         'multiples of 2^(levels-1) and the last level at least win_size x win_size')
    chunk = max(1, min(P, _PAIR_WORKSPACE_BYTES // per_pair))
    ws_bytes = lib.la_pair_metrics_workspace_bytes(chunk, C, H, W, win, levels)
    ws = _lib.workspace(ws_bytes, dev, torch.float64)
    err =torch.empty([P, C, 2], dtype=torch.float64, device=dev)
    ssim = torch.empty([P, C, levels], dtype=torch.float32, device=dev)
    cs = torch.empty([P, C, levels], dtype=torch.float32, device=dev)
    ms = torch.empty([P, C], dtype=torch.float32, device=dev)
    c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            xa, ya = (x, y) if pairs is not None else (x[p0:], y[p0:])
            _lib.check(lib.la_pair_metrics_f32(
                _lib.ptr(xa), _lib.ptr(ya), _lib.ptr(ixd[p0:]) if pairs is not None else None,
                _lib.ptr(iyd[p0:]) if pairs is not None else None, n, C, H, W, taps.ctypes.data, win, levels, w.ctypes.data, c1, c2,
                _lib.ptr(err[p0:]), _lib.ptr(ssim[p0:]), _lib.ptr(cs[p0:]), _lib.ptr(ms[p0:]), _lib.ptr(ws), ws_bytes,
                _lib.stream_ptr()), 'pair_metrics')
    err = err.cpu()
    out = {'mse_per_channel': err[..., 0] / (H * W), 'mae_per_channel': err[..., 1] / (H * W),
           'ssim_per_channel': ssim[..., 0].cpu().double(), 'ms_ssim_per_channel': ms.cpu().double(),
           'ssim_levels': ssim.cpu().double(), 'cs_levels': cs.cpu().double()}
    for k in ('mse', 'mae', 'ssim', 'ms_ssim'):
        out[k] = out[k + '_per_channel'].mean(dim=1)
    for k in ('psnr', 'psnr_per_channel'):
        out[k] = 10.0 * torch.log10(float(data_range) ** 2 / out[k.replace('psnr', 'mse')])          # x / 0 = inf in float64 tensors
    if lpips_net is not None:
        out.update(compute_lpips(x, y, lpips_net, pairs=pairs))
    if nst_net is not None:
        out.update(compute_style_content(x, y, nst_net, pairs=pairs))
    return out


def _aug_pair_files(datadir):
    i, files = 0, []
    while os.path.isfile(os.path.join(datadir, 'img', f'img_{i}')) and os.path.isfile(os.path.join(datadir, 'img_aug', f'img_aug_{i}')):
        files.append((os.path.join(datadir, 'img', f'img_{i}'), os.path.join(datadir, 'img_aug', f'img_aug_{i}')))
        i += 1
    return files


def _aug_two_channels(fname, dev):
    """the 'A' and 'B' batches ([n, 1, H, W]) of one pickled dict of a run directory as the two channels of a float32 device tensor"""
    from .formats import _restricted_load
    with open(fname, 'rb') as f:
        d = _restricted_load(f)
    planes = [torch.as_tensor(d[m]).to(torch.float32) for m in ('A', 'B')]
    if any(p.ndim != 4 or p.shape[1] != 1 for p in planes):
        raise ValueError(f"{fname}: 'A' and 'B' must be [n, 1, H, W] batches")
    return torch.cat(planes, dim=1).to(dev)


def _aug_pair_run(datadir, device):
    """(device, [(img/img_{i}, img_aug/img_aug_{i})]) of a run directory; raises without a ROCm device or without a first pair"""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got device ' + str(dev))
    files = _aug_pair_files(datadir)
    if not files:
        raise FileNotFoundError(f"no img/img_0 with img_aug/img_aug_0 under {datadir}")
    return dev, files


def compute_pair_metrics_for_aug_dataset(datadir, device='cuda:0', **kw):
    """compute_pair_metrics of every source image against its augmented version in a run directory of the reference's drivers
    (backbone_latentaug.py:112-118): `img/img_{i}` and `img_aug/img_aug_{i}`, i = 0, 1, .., each a pickled dict of image batches whose
    'A' and 'B' entries ([n, 1, H, W]) become the two channels.  The pickles are read through the allow-list loader of formats.py,
    never a plain unpickle.  Returns the per-sample tensors of compute_pair_metrics over all files, a float '<key>_mean' for each of
    'mse', 'mae', 'psnr', 'ssim', 'ms_ssim', and 'num_items'.  With `lpips_net=` (see compute_pair_metrics) the LPIPS keys and
    'lpips_mean' are added, with `nst_net=` the style / content keys and 'style_mean', 'content_mean'."""
    dev, files = _aug_pair_run(datadir, device)
    parts = [compute_pair_metrics(_aug_two_channels(src, dev), _aug_two_channels(aug, dev), **kw) for src, aug in files]
    out = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
    out['num_items'] = int(out['mse'].shape[0])
    for k in ('mse', 'mae', 'psnr', 'ssim', 'ms_ssim') + (('lpips',) if 'lpips' in out else ()) + (('style', 'content') if 'style' in out else ()):
        out[k + '_mean'] = float(out[k].mean())
    return out


# ------------------------------------------------------------------------------------------------------------
# sliced Wasserstein distance (la_swd.hip, la_sort.hip; no reference counterpart, no detector, no CPU fallback)
SWD_LEVEL_DIR_STRIDE = 1 << 20          # global direction index of direction j of pyramid level l: l * 2^20 + j


def _pyramid_levels(H, W, min_resolution):
    n, r = 1, min(H, W)
    while H % 2 == 0 and W % 2 == 0 and r // 2 >= min_resolution:
        n, r, H, W = n + 1, r // 2, H // 2, W // 2
    return n


def laplacian_pyramid(images, min_resolution=16):
    """The Laplacian pyramid of `images` [N, C, H, W] (a float32 device tensor): the list of level tensors at resolutions H, H/2, ..
    down to the last one whose smaller side is still >= `min_resolution` (halving stops earlier at an odd side).  G_0 = x,
    G_{l+1} = down(G_l) with the 5 x 5 binomial filter, mirrored borders, every second sample; level l is G_l - up(G_{l+1}), the
    last level is G itself (la_lap_pyr_down_f32, la_lap_pyr_up_sub_f32), so level 0 + up(level 1 + up(..)) gives the images back."""
    x = _device_images(images, 'images')
    lib = _lib.load()
    N, C, H, W = x.shape
    g = [x.clone()]
    with torch.cuda.device(x.device):
        for _ in range(_pyramid_levels(H, W, min_resolution) - 1):
            h, w = g[-1].shape[2:]
            y = torch.empty([N, C, h // 2, w // 2], dtype=torch.float32, device=x.device)
            _lib.check(lib.la_lap_pyr_down_f32(_lib.ptr(g[-1]), _lib.ptr(y), N * C, h, w, _lib.stream_ptr()), 'lap_pyr_down')
            g.append(y)
        for l in range(len(g) - 1):
            h, w = g[l].shape[2:]
            _lib.check(lib.la_lap_pyr_up_sub_f32(_lib.ptr(g[l]), _lib.ptr(g[l + 1]), N * C, h, w, _lib.stream_ptr()), 'lap_pyr_up_sub')
    return g


def _swd_directions(ndirs, D, dir0, seed, dev):
    lib = _lib.load()
    dirs = torch.empty([ndirs, D], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.la_swd_directions_f32(_lib.ptr(dirs), ndirs, D, dir0, seed, _lib.stream_ptr()), 'swd_directions')
    return dirs


def _swd_w1(a, b, dirs):
    """la_swd_f32 on float32 device tensors a, b [M, D] and dirs [ndirs, D] -> w1 float64 [ndirs] (numpy)"""
    lib = _lib.load()
    dev, (M, D), ndirs = a.device, a.shape, dirs.shape[0]
    w1 = torch.empty([ndirs], dtype=torch.float64, device=dev)
    floor_bytes = lib.la_swd_scratch_bytes(M, D, ndirs)
    # the documented minimum holds chunks of 32 directions; give every direction room (up to 1 GiB): the bits do not depend on it
    nbytes = max(floor_bytes, min(floor_bytes * -(-ndirs // 32), 1 << 30))
    scratch = _lib.workspace(nbytes, dev, torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.la_swd_f32(_lib.ptr(a), _lib.ptr(b), M, D, _lib.ptr(dirs), ndirs, _lib.ptr(w1), _lib.ptr(scratch), nbytes,
                                  _lib.stream_ptr()), 'swd')
    return w1.cpu().numpy()


def compute_swd_from_features(a, b, num_dirs=512, seed=0, device='cuda:0', return_details=False):
    """Sliced Wasserstein distance of two sets of rows ([N, D] numpy arrays or tensors of any float dtype, computed from their float32
    values; equal N): the mean over `num_dirs` random unit directions d_j of W1_j = mean_i |sort(a d_j)_i - sort(b d_j)_i|, the
    1-Wasserstein distance of the two projected samples (Rabin et al. 2011).  The rows are taken as they are -- scale them yourself if
    the columns should weigh alike -- and the result is not multiplied by 1e3.  Directions are those of la_swd_directions_f32 for
    global indices 0 .. num_dirs - 1 under `seed`.  A translation by t gives W1_j = |t . d_j|; two calls give the same bits.
    There is no CPU fallback.  return_details=True: (swd, {'w1': float64 [num_dirs], 'dirs': float32 [num_dirs, D]})."""
    dev, (fa, fb) = _query_features(device, a=a, b=b)
    if fa.shape[0] != fb.shape[0]:
        raise ValueError(f'the sliced Wasserstein distance needs sets of one size (got {fa.shape[0]} and {fb.shape[0]} rows)')
    if int(num_dirs) != num_dirs or num_dirs < 1:
        raise ValueError(f'num_dirs must be a positive integer (got {num_dirs})')
    dirs = _swd_directions(int(num_dirs), fa.shape[1], 0, int(seed), dev)
    w1 = _swd_w1(fa, fb, dirs)
    swd = float(w1.mean())
    if return_details:
        return swd, dict(w1=w1, dirs=dirs.cpu().numpy())
    return swd


def _swd_descriptor_banks(batches, mode, num_items, nhood_size, nhoods_per_image, min_resolution, seed, device):
    """Per pyramid level the descriptor rows of the first `num_items` images of `batches` (all of them: None), batch by batch:
    ([level][rows, D] float32 device tensors, number of images, (C, H, W)).  The images themselves are never resident as a set."""
    lib = _lib.load()
    banks, count, shape = None, 0, None
    for batch in batches:
        x = _batch_images(batch, mode)
        x = _device_images(x if device is None else x.to(device, torch.float32), 'images')
        if num_items is not None:
            x = x[:num_items - count]
        if x.shape[0] == 0:
            break
        if shape is None:
            shape = tuple(x.shape[1:])
            if min(shape[1:]) < nhood_size:
                raise ValueError(f'images of {shape[1]} x {shape[2]} hold no {nhood_size} x {nhood_size} neighbourhood')
            banks = [[] for _ in range(_pyramid_levels(shape[1], shape[2], max(min_resolution, nhood_size)))]
        elif tuple(x.shape[1:]) != shape:
            raise ValueError(f'every batch must hold [N, {shape[0]}, {shape[1]}, {shape[2]}] images (got {tuple(x.shape)})')
        n, C = x.shape[:2]
        levels = laplacian_pyramid(x, max(min_resolution, nhood_size))
        with torch.cuda.device(x.device):
            for l, lv in enumerate(levels):
                desc = torch.empty([n * nhoods_per_image, C * nhood_size ** 2], dtype=torch.float32, device=x.device)
                _lib.check(lib.la_swd_gather_f32(_lib.ptr(lv), n, C, lv.shape[2], lv.shape[3], count, l, nhood_size, nhoods_per_image, seed,
                                                 _lib.ptr(desc), _lib.stream_ptr()), 'swd_gather')
                banks[l].append(desc)
        count += n
        if num_items is not None and count >= num_items:
            break
    if banks is None:
        raise ValueError('no images')
    return [torch.cat(b, dim=0) for b in banks], count, shape


def _swd_normalize(desc, C, what):
    """desc [M, C P] in place -> (mean, std) float64 [C] numpy; a constant channel is an error"""
    lib = _lib.load()
    M, P, dev = desc.shape[0], desc.shape[1] // C, desc.device
    stats = torch.empty([2, C], dtype=torch.float64, device=dev)
    nbytes = lib.la_swd_stats_scratch_bytes(M, C, P)
    scratch = _lib.workspace(nbytes, dev, torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.la_swd_channel_stats_f64(_lib.ptr(desc), M, C, P, _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(scratch), nbytes,
                                                _lib.stream_ptr()), 'swd_channel_stats')
        mean, std = stats.cpu().numpy()
        if not (std > 0).all():
            raise ValueError(f'{what}: channel(s) {np.flatnonzero(~(std > 0)).tolist()} are constant over all neighbourhoods (standard deviation '
                             '0): a constant channel has no descriptor')
        _lib.check(lib.la_swd_normalize_f32(_lib.ptr(desc), M, C, P, _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.stream_ptr()), 'swd_normalize')
    return mean, std


def compute_swd_from_images(real_batches, gen_batches, mode=None, num_items=None, nhood_size=7, nhoods_per_image=128, dir_repeats=4,
                            dirs_per_repeat=128, min_resolution=16, seed=0, return_details=False, device=None):
    """Sliced Wasserstein distance of two image sets on a Laplacian pyramid (Karras, Aila, Laine, Lehtinen, ICLR 2018, section 5): the
    one established GAN metric that needs no network and no weight file.  `real_batches`, `gen_batches`: iterables of [N, C, H, W]
    float32 device tensors in [-1, 1] (C = 1, 2 or 3: any C the descriptors can hold), or of the augmentation plugins' output dicts
    with `mode`, as for compute_feature_stats_for_images; with `device=` every batch is first moved there as float32.  Both sides use their first `num_items` images (default: the smaller count; an
    explicit num_items that a side cannot fill is an error).  Per pyramid level (laplacian_pyramid): `nhoods_per_image` patches of
    nhood_size^2 pixels over all channels at positions drawn from the library's Philox stream (keyed by patch, global image index,
    level and `seed`: a set gives the same descriptors in whatever batches it arrives), each channel normalised to mean 0 and
    standard deviation 1 over the set, then the mean over dir_repeats * dirs_per_repeat random unit directions -- shared by both
    sets, keyed by level and seed only -- of the 1-Wasserstein distance of the projections.  Returns {'swd_<res>': .., 'swd_avg': ..}
    times 1e3 as published, <res> the height of the level: coarse levels say whether the anatomy moved, fine ones whether the texture
    did.  The descriptor banks are filled batch by batch.  Two calls give the same bits; a set against itself gives exactly 0.
    There is no CPU fallback.  return_details=True: (dict, {'levels': [{'res', 'w1': float64 [dirs], 'mean', 'std': float64 [2, C]
    (real, gen)}], 'num_items'})."""
    if num_items is not None and (int(num_items) != num_items or num_items < 1):
        raise ValueError(f'num_items must be a positive integer (got {num_items})')
    if min(nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat) < 1 or dir_repeats * dirs_per_repeat > SWD_LEVEL_DIR_STRIDE:
        raise ValueError('nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat must be positive and at most 2^20 directions asked for')
    seed, ndirs = int(seed), int(dir_repeats) * int(dirs_per_repeat)
    sides = [_swd_descriptor_banks(b, mode, num_items, int(nhood_size), int(nhoods_per_image), int(min_resolution), seed, device)
             for b in (real_batches, gen_batches)]
    (rb, rn, rshape), (gb, gn, gshape) = sides
    if rshape != gshape:
        raise ValueError(f'real and generated images differ in shape: {rshape} and {gshape}')
    n = min(rn, gn) if num_items is None else int(num_items)
    if min(rn, gn) < n:
        raise ValueError(f'num_items = {n}, but the sets hold {rn} real and {gn} generated images')
    C, rows = rshape[0], n * int(nhoods_per_image)
    out, levels = {}, []
    for l, (a, b) in enumerate(zip(rb, gb)):
        a, b = a[:rows], b[:rows]
        res = rshape[1] >> l
        stats = [_swd_normalize(d, C, f'swd_{res}, {who} images') for d, who in ((a, 'real'), (b, 'generated'))]
        dirs = _swd_directions(ndirs, a.shape[1], l * SWD_LEVEL_DIR_STRIDE, seed, a.device)
        w1 = _swd_w1(a, b, dirs)
        out[f'swd_{res}'] = float(w1.mean()) * 1e3
        levels.append(dict(res=res, w1=w1, mean=np.stack([s[0] for s in stats]), std=np.stack([s[1] for s in stats])))
    out['swd_avg'] = float(np.mean([out[k] for k in out]))
    if return_details:
        return out, dict(levels=levels, num_items=n)
    return out


def compute_swd_for_aug_dataset(datadir, device='cuda:0', **kw):
    """compute_swd_from_images of the source images against their augmented versions in a run directory of the reference's drivers:
    `img/img_{i}` and `img_aug/img_aug_{i}`, i = 0, 1, .., read like compute_pair_metrics_for_aug_dataset reads them -- the allow-list
    loader of formats.py, 'A' and 'B' as the two channels -- one file a batch."""
    dev, files = _aug_pair_run(datadir, device)
    return compute_swd_from_images((_aug_two_channels(src, dev) for src, _ in files), (_aug_two_channels(aug, dev) for _, aug in files), **kw)


def msssim_diversity_pairs(num_images, num_pairs=1000, seed=0):
    """(ix, iy) int32: `num_pairs` distinct unordered pairs i < j of `num_images` images.  When the set has no more than `num_pairs`
    pairs: all of them, in lexicographic order.  Otherwise numpy.random.RandomState(seed) draws batches of `num_pairs` candidates
    `randint(0, num_images, [num_pairs, 2])`; a candidate with i == j or equal (as an unordered pair) to an earlier one is dropped,
    and the first `num_pairs` survivors are kept in the order drawn."""
    n = int(num_images)
    if n < 2 or num_pairs < 1:
        raise ValueError('MS-SSIM diversity needs at least 2 images and 1 pair')
    total = n * (n - 1) // 2
    if total <= num_pairs:
        i, j = np.triu_indices(n, k=1)
        return i.astype(np.int32), j.astype(np.int32)
    rs = np.random.RandomState(seed)
    seen, keep = set(), []
    while len(keep) < num_pairs:
        for a, b in rs.randint(0, n, [num_pairs, 2]):
            key = (min(a, b), max(a, b))
            if a != b and key not in seen and len(keep) < num_pairs:
                seen.add(key)
                keep.append(key)
    keep = np.asarray(keep, dtype=np.int32)
    return np.ascontiguousarray(keep[:, 0]), np.ascontiguousarray(keep[:, 1])


def compute_msssim_diversity(images, num_pairs=1000, seed=0, **kw):
    """Mean MS-SSIM over `msssim_diversity_pairs(N, num_pairs, seed)` of one image set [N, C, H, W] (float32, on the device): near 1
    means that the samples resemble one another (mode collapse).  The kernel gathers the pairs; the images are never copied.
    Returns {'mean': float, 'ms_ssim': float64 [P], 'ix', 'iy'}; **kw goes to compute_pair_metrics."""
    images = _device_images(images, 'images')
    ix, iy = msssim_diversity_pairs(images.shape[0], num_pairs, seed)
    ms = compute_pair_metrics(images, images, pairs=(ix, iy), **kw)['ms_ssim']
    return dict(mean=float(ms.mean()), ms_ssim=ms, ix=ix, iy=iy)


def mi_from_counts(counts):
    """(mi, nmi) float64 [...] from joint-histogram counts [..., bins, bins], natural logarithms: MI = sum p_ab log(p_ab / (p_a p_b)),
    NMI = (H_a + H_b) / H_ab; where H_ab = 0 (all of a plane in one bin) NMI = 2, the value for identical images, and MI = 0."""
    c = np.asarray(counts).astype(np.float64)
    n = c.sum(axis=(-2, -1), keepdims=True)
    if not (n > 0).all():
        raise ValueError('mi_from_counts: an empty histogram')
    pab = c / n
    pa, pb = pab.sum(axis=-1, keepdims=True), pab.sum(axis=-2, keepdims=True)

    def entropy(p, axes):
        return -np.sum(p * np.log(np.where(p > 0, p, 1.0)), axis=axes)
    ha, hb, hab = entropy(pa, (-2, -1)), entropy(pb, (-2, -1)), entropy(pab, (-2, -1))
    ratio = np.where(pab > 0, pab, 1.0) / np.where(pab > 0, pa * pb, 1.0)
    mi = np.sum(pab * np.log(ratio), axis=(-2, -1))
    one_bin = c.max(axis=(-2, -1)) == n[..., 0, 0]
    nmi = np.where(one_bin, 2.0, (ha + hb) / np.where(one_bin, 1.0, hab))
    return np.where(one_bin, 0.0, mi), nmi


def _joint_hist(a, a_stride, b, b_stride, planes, npix, bins, value_range, dev):
    lo, hi = float(value_range[0]), float(value_range[1])
    if int(bins) != bins or not 1 <= bins <= 64:
        raise ValueError(f'bins must lie in 1 .. 64 (got {bins})')
    if not hi > lo:
        raise ValueError('value_range must be (lo, hi) with hi > lo')
    lib = _lib.load()
    hist = torch.empty([planes, int(bins), int(bins)], dtype=torch.int32, device=dev)          # uint32 counts
    with torch.cuda.device(dev):
        _lib.check(lib.la_joint_hist_f32(a, a_stride, b, b_stride, planes, npix, int(bins), float(np.float32(lo)),
                                         float(np.float32(bins / (hi - lo))), _lib.ptr(hist), _lib.stream_ptr()), 'joint_hist')
    counts = hist.cpu().numpy().view(np.uint32).astype(np.int64)
    mi, nmi = mi_from_counts(counts)
    return dict(mi=mi, nmi=nmi, counts=counts)


def compute_modality_mi(images, channels=(0, 1), bins=64, value_range=(-1.0, 1.0)):
    """Mutual information of two channels (the generator's CT and MRI) of every sample of `images` [N, C, H, W] (float32, on the
    device), read in place.  The joint histogram has `bins` x `bins` cells (1 .. 64) over `value_range`, values outside it counted in
    the edge bins (la_joint_hist_f32: float32 bin rule, integer counts, the same on every run).
    Returns {'mi', 'nmi': float64 [N], 'counts': int64 [N, bins, bins]} (mi_from_counts)."""
    images = _device_images(images, 'images')
    N, C, H, W = (int(s) for s in images.shape)
    ca, cb = (int(c) for c in channels)
    if not (0 <= ca < C and 0 <= cb < C):
        raise ValueError(f'channels {channels} outside the {C} channels of the images')
    base = images.data_ptr()
    return _joint_hist(base + 4 * ca * H * W, C * H * W, base + 4 * cb * H * W, C * H * W, N, H * W, bins, value_range, images.device)


def compute_pair_mi(x, y, channel=0, bins=64, value_range=(-1.0, 1.0)):
    """compute_modality_mi between plane `channel` of x[i] and the same plane of y[i] (two batches of one shape)."""
    x, y = _device_images(x, 'x'), _device_images(y, 'y')
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f'x and y must agree in shape and device: {tuple(x.shape)}, {tuple(y.shape)}')
    N, C, H, W = (int(s) for s in x.shape)
    c = int(channel)
    if not 0 <= c < C:
        raise ValueError(f'channel {channel} outside the {C} channels of the images')
    return _joint_hist(x.data_ptr() + 4 * c * H * W, C * H * W, y.data_ptr() + 4 * c * H * W, C * H * W, N, H * W, bins, value_range,
                       x.device)


# ------------------------------------------------------------------------------------------------------------
# perceptual path length (la_pathpoints.hip; Karras et al. 2019 / 2020; no reference counterpart, no CPU fallback)
def ppl_from_distances(d):
    """The published PPL filter over per-sample distances d [N] (any real array or tensor, NaN-free): the mean of the d with
    lo <= d <= hi, lo = the 1st percentile by the 'lower' rule (sorted[floor(0.01 (N - 1))]) and hi = the 99th by the 'higher' rule
    (sorted[ceil(0.99 (N - 1))]).  Runs on the host in float64; returns a float."""
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 1 or d.size < 1:
        raise ValueError(f'ppl_from_distances: a non-empty [N] array of distances; got shape {d.shape}')
    s = np.sort(d)
    lo = s[int(np.floor(0.01 * (d.size - 1)))]
    hi = s[int(np.ceil(0.99 * (d.size - 1)))]
    return float(d[(d >= lo) & (d <= hi)].mean())


def _path_points(a, b, t, dt, reps, mode):
    """la_path_points_f32: a, b [N, D], t [N] float32 on one device, dt a sequence of T floats -> [T, N, reps, D] float32."""
    N, D = (int(s) for s in a.shape)
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    out = torch.empty([dt.size, N, int(reps), D], dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().la_path_points_f32(_lib.ptr(a), _lib.ptr(b), _lib.ptr(t), dt.ctypes.data, int(dt.size), N, D, int(reps),
                                                  int(mode), _lib.ptr(out), _lib.stream_ptr()), 'path_points')
    return out


def _path_engines(synth, net, what):
    """The checks the path metrics share; returns the pairs one call of the net takes."""
    if not hasattr(synth, 'num_ws') or not hasattr(synth, 'max_batch'):
        raise _lib.LatentAugHipError(f'{what}: synth must be a synthesis.SynthesisEngine; got {type(synth).__name__}')
    if not hasattr(net, 'pair_distance_rows'):
        raise _lib.LatentAugHipError(f'{what}: net must be a synthesis.FeatureEngine; got {type(net).__name__}')
    per_call = net.pair_rows()          # (refuses a detector engine)
    if net.in_ch != 3:
        raise ValueError(f'{what}: the net must take three input channels (in_ch {net.in_ch})')
    if synth.device != net.device:
        raise ValueError(f'{what}: generator on {synth.device}, net on {net.device}')
    R = synth.img_resolution
    if R % net.in_res != 0:
        raise ValueError(f'{what}: the image resolution {R} must be the net\'s in_res {net.in_res} or an integer multiple of it')
    if synth.max_batch < 2:
        raise _lib.LatentAugHipError(f'{what}: both ends of a step go through one batch; the generator has max_batch = {synth.max_batch}')
    return per_call


def _lpips_rows(img, net):
    """[M, C, R, R] images -> the net's input [M * C, 3, in_res, in_res] (row m * C + c): every channel on its own, reduced by area when
    R is a multiple of in_res (la_detector_prep_f32, no quantisation), repeated to three and given the net's input affine."""
    M, C_, R = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
    lib = _lib.load()
    sc, sh = (C.c_float * 3)(*net.pre_scale), (C.c_float * 3)(*net.pre_shift)
    rows = torch.empty([M * C_, 3, net.in_res, net.in_res], dtype=torch.float32, device=img.device)
    if R == net.in_res:
        _lib.check(lib.la_crop_repeat_affine_f32(_lib.ptr(img), _lib.ptr(rows), M * C_, 1, R, R, 0, 0, 3, sc, sh, _lib.stream_ptr()),
                   'la_crop_repeat')
    else:
        _lib.check(lib.la_detector_prep_f32(_lib.ptr(img), _lib.ptr(rows), M * C_, 1, R, R, net.in_res, 3, 0, 0, sc, sh,
                                            _lib.stream_ptr()), 'la_detector_prep_f32')
    return rows


def compute_ppl(mapping, synth, net, num_samples, epsilon=1e-4, space='w', sampling='full', truncation_psi=1.0, seed=0, batch=None):
    """Perceptual path length of a generator (Karras et al. 2019 / 2020): per sample, the LPIPS distance of the images at two latent
    points `epsilon` apart on the path between two random latents, divided by epsilon^2.  `mapping` is a synthesis.MappingEngine, `synth`
    a SynthesisEngine, `net` a FeatureEngine of three input channels whose in_res is the image resolution or divides it (then the images
    are reduced by area first).  z0, z1 = the halves of randn([2 N, z_dim]), then t = rand([N]) ('full') or 0 ('end'), from one CPU
    torch.Generator(seed): the draws do not depend on the chunking.  space='w': both z are mapped (truncation_psi applies) and the
    points are the lerp at t and t + epsilon, broadcast to num_ws; space='z': the points are the slerp at t and t + epsilon, then
    mapped (la_path_points_f32 forms t + epsilon in double).  Chunks of n <= min(synth.max_batch // 2, batch) samples: both points of
    a chunk are one synthesis batch (noise_mode='const'), every image channel goes through the net as compute_lpips feeds it.
    Returns float64 CPU tensors: 'dist' [N] (mean over channels), 'dist_per_channel' [N, C] (sum over taps / epsilon^2), 'ppl' (0-dim,
    ppl_from_distances of 'dist') and 'ppl_per_channel' [C].  Two calls give the same bits.  There is no CPU fallback."""
    if space not in ('w', 'z') or sampling not in ('full', 'end'):
        raise ValueError(f"compute_ppl: space 'w' | 'z' and sampling 'full' | 'end' (got {space!r}, {sampling!r})")
    if int(num_samples) != num_samples or num_samples < 1 or not epsilon > 0:
        raise ValueError('compute_ppl: num_samples must be a positive integer and epsilon positive')
    if not hasattr(mapping, 'z_dim') or not hasattr(mapping, 'forward'):
        raise _lib.LatentAugHipError(f'compute_ppl: mapping must be a synthesis.MappingEngine; got {type(mapping).__name__}')
    per_call = _path_engines(synth, net, 'compute_ppl')
    if mapping.device != synth.device or mapping.w_dim != synth.w_dim:
        raise ValueError(f'compute_ppl: mapping (w_dim {mapping.w_dim}, {mapping.device}) and generator (w_dim {synth.w_dim}, '
                         f'{synth.device}) do not belong together')
    if batch is not None and (int(batch) != batch or batch < 1):
        raise ValueError('compute_ppl: batch must be a positive integer')
    N, C_, dev = int(num_samples), synth.img_channels, synth.device
    chunk = min(synth.max_batch // 2, max(1, per_call // C_), N if batch is None else int(batch))
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn([2 * N, mapping.z_dim], generator=g)
    t = torch.rand([N], generator=g) if sampling == 'full' else torch.zeros([N])
    z0, z1, t = z[:N].to(dev), z[N:].to(dev), t.to(dev)
    eps = float(epsilon)
    out = torch.empty([N, C_, net.num_taps], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for p0 in range(0, N, chunk):
            n = min(chunk, N - p0)
            if space == 'w':
                w = mapping.forward(torch.cat([z0[p0:p0 + n], z1[p0:p0 + n]]), 1, truncation_psi).reshape(2 * n, synth.w_dim)
                ws = _path_points(w[:n], w[n:], t[p0:p0 + n], [0.0, eps], synth.num_ws, 0)
            else:
                zz = _path_points(z0[p0:p0 + n].contiguous(), z1[p0:p0 + n].contiguous(), t[p0:p0 + n], [0.0, eps], 1, 1)
                ws = mapping.forward(zz.reshape(2 * n, mapping.z_dim), synth.num_ws, truncation_psi)
            img = synth.forward(ws.reshape(2 * n, synth.num_ws, synth.w_dim), noise_mode='const')          # rows p and p + n: a pair
            rows, P = _lpips_rows(img, net), n * C_
            if P <= per_call:
                d = torch.empty([P, net.num_taps], dtype=torch.float64, device=dev)
                net.pair_distance_rows(rows, P, d)
            else:          # (a net whose batch is smaller than one sample's channels)
                d = net.pair_distance(rows[:P], rows[P:])
            out[p0:p0 + n] = d.reshape(n, C_, net.num_taps)
    per_channel = out.cpu().sum(dim=2) / (eps * eps)
    dist = per_channel.mean(dim=1)
    return {'dist': dist, 'dist_per_channel': per_channel,
            'ppl': torch.tensor(ppl_from_distances(dist.numpy()), dtype=torch.float64),
            'ppl_per_channel': torch.tensor([ppl_from_distances(per_channel[:, c].numpy()) for c in range(C_)], dtype=torch.float64)}


def compute_path_length(synth, net, w0, w1, segments=8):
    """Perceptual length of the straight segments from w0[p] to w1[p] (e.g. an inverted latent and its augmented version): the
    segment is cut into `segments` equal steps (1 .. 63), every one of the segments + 1 points is synthesised once (noise_mode='const')
    and consecutive images are compared with `net` as compute_lpips compares them.  sqrt(LPIPS) is the metric whose steps add up; the
    chord is the same between the two ends.  w0, w1: float32 device tensors [N, w_dim], [N, 1, w_dim] (W) or [N, num_ws, w_dim] (W+,
    the lerp then runs over the num_ws * w_dim values of a row).  `synth`, `net`: as compute_ppl takes them.
    Returns float64 CPU tensors: 'length' [N] (sum over the steps of sqrt of the mean over channels of LPIPS), 'chord' [N], 'ratio' [N]
    = length / chord, 1 where the chord is 0 (w0 == w1: a path that does not move is as straight as it can be), and 'segment_lpips'
    [N, segments] (mean over channels).  With segments=1 length is chord bit for bit.  Two calls give the same bits."""
    for name, w in (('w0', w0), ('w1', w1)):
        if not torch.is_tensor(w):
            raise _lib.LatentAugHipError(f'{name}: latentaugment_amd needs a ROCm device tensor (no CPU fallback); got {type(w).__name__}')
        _lib.require_gpu(w)
    _path_engines(synth, net, 'compute_path_length')
    if int(segments) != segments or not 1 <= segments <= 63:
        raise ValueError(f'compute_path_length: segments must lie in 1 .. 63 (got {segments})')
    S = int(segments)
    if w0.shape != w1.shape or w0.device != w1.device or w0.device != synth.device:
        raise ValueError(f'w0 and w1 must agree in shape and sit on the generator\'s device: {tuple(w0.shape)} on {w0.device}, '
                         f'{tuple(w1.shape)} on {w1.device}')
    if w0.ndim == 2:
        w0, w1 = w0[:, None], w1[:, None]
    if w0.ndim != 3 or w0.shape[0] < 1 or w0.shape[1] not in (1, synth.num_ws) or w0.shape[2] != synth.w_dim:
        raise ValueError(f'w0, w1: [N, {synth.w_dim}], [N, 1, {synth.w_dim}] or [N, {synth.num_ws}, {synth.w_dim}]; got {tuple(w0.shape)}')
    N, L = int(w0.shape[0]), int(w0.shape[1])
    C_, dev, T = synth.img_channels, synth.device, S + 1
    npairs = S if S == 1 else S + 1          # the steps, then the chord (with one step the chord IS the step)
    chunk = max(1, min(N, 256 // T))          # paths per round: at most 256 images at a time
    a = w0.detach().to(torch.float32).reshape(N, L * synth.w_dim).contiguous()
    b = w1.detach().to(torch.float32).reshape(N, L * synth.w_dim).contiguous()
    t = torch.zeros([N], dtype=torch.float32, device=dev)
    dt = [k / S for k in range(T)]
    R = synth.img_resolution
    out = torch.empty([N, npairs, C_, net.num_taps], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for p0 in range(0, N, chunk):
            n = min(chunk, N - p0)
            ws = _path_points(a[p0:p0 + n], b[p0:p0 + n], t[p0:p0 + n], dt, 1, 0).reshape(T * n, L, synth.w_dim)      # row k * n + p
            img = torch.empty([T * n, C_, R, R], dtype=torch.float32, device=dev)
            for r0 in range(0, T * n, synth.max_batch):
                synth.forward(ws[r0:r0 + synth.max_batch], noise_mode='const', out=img[r0:r0 + synth.max_batch])
            rows = _lpips_rows(img, net)          # row (k * n + p) * C + c
            first = torch.arange(S * n * C_, device=dev)
            ia = first if S == 1 else torch.cat([first, first[:n * C_]])
            ib = first + n * C_ if S == 1 else torch.cat([first + n * C_, first[:n * C_] + S * n * C_])
            d = net.pair_distance(rows.index_select(0, ia), rows.index_select(0, ib))
            out[p0:p0 + n] = d.reshape(npairs, n, C_, net.num_taps).permute(1, 0, 2, 3)
    lp = out.cpu().sum(dim=3).mean(dim=2)          # [N, npairs]
    seg, chord = lp[:, :S], lp[:, npairs - 1].sqrt()
    length = seg.sqrt().sum(dim=1)
    ratio = torch.where(chord > 0, length / torch.where(chord > 0, chord, torch.ones_like(chord)), torch.ones_like(chord))
    return {'length': length, 'chord': chord, 'ratio': ratio, 'segment_lpips': seg.contiguous()}


def compute_path_length_for_aug_dataset(datadir, synth, net, segments=8):
    """compute_path_length from every inverted latent to its augmented version in a run directory of the reference's drivers
    (backbone_latentaug.py:112-118): `latent/w_{i}` and `latent_aug/w_aug_{i}`, i = 0, 1, .., each a pickled batch of latents
    ([n, w_dim] as the drivers squeeze them -- [w_dim] for a batch of one --, [n, 1, w_dim] or [n, num_ws, w_dim]; a W file against a W+
    file is broadcast).  The pickles are read through the
    allow-list loader of formats.py, never a plain unpickle.  Returns the per-sample tensors of compute_path_length over all files, a
    float '<key>_mean' for 'length', 'chord' and 'ratio', and 'num_items'."""
    from .formats import _restricted_load
    _path_engines(synth, net, 'compute_path_length_for_aug_dataset')
    files, i = [], 0
    while os.path.isfile(os.path.join(datadir, 'latent', f'w_{i}')) and os.path.isfile(os.path.join(datadir, 'latent_aug', f'w_aug_{i}')):
        files.append((os.path.join(datadir, 'latent', f'w_{i}'), os.path.join(datadir, 'latent_aug', f'w_aug_{i}')))
        i += 1
    if not files:
        raise FileNotFoundError(f"no latent/w_0 with latent_aug/w_aug_0 under {datadir}")

    def latents(fname):
        with open(fname, 'rb') as f:
            w = torch.as_tensor(_restricted_load(f)).to(torch.float32)
        if w.ndim == 1:          # the drivers squeeze what they dump: a batch of one is [w_dim]
            w = w[None]
        if w.ndim == 2:
            w = w[:, None]
        if w.ndim != 3 or w.shape[1] not in (1, synth.num_ws) or w.shape[2] != synth.w_dim:
            raise ValueError(f'{fname}: latents must be [n, {synth.w_dim}], [n, 1, {synth.w_dim}] or [n, {synth.num_ws}, {synth.w_dim}]')
        return w
    parts = []
    for src, aug in files:
        w0, w1 = latents(src), latents(aug)
        if w0.shape[1] != w1.shape[1]:
            w0, w1 = (w.expand(-1, synth.num_ws, -1) for w in (w0, w1))
        parts.append(compute_path_length(synth, net, w0.contiguous().to(synth.device), w1.contiguous().to(synth.device), segments=segments))
    out = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
    out['num_items'] = int(out['length'].shape[0])
    for k in ('length', 'chord', 'ratio'):
        out[k + '_mean'] = float(out[k].mean())
    return out
