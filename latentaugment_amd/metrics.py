"""Host-side mirror of the reference's quality metrics (metrics/) over the HIP C ABI: the VGG16 detector features of images and
everything downstream of detector features.

  FeatureStats                 metrics/metric_utils.py:79-155   (same fields, append / append_torch / get_all / get_mean_cov,
                                                                 save / load of the reference's pickle layout)
  compute_fid_from_stats       metrics/frechet_inception_distance.py:41-45
  compute_distances            metrics/precision_recall.py:19-32
  compute_pr_from_features     metrics/precision_recall.py:72-85
  compute_kid_from_features    (not in the reference) Kernel Inception Distance, the community's kid50k_full recipe
  compute_dc_from_features     (not in the reference) density and coverage, Naeem et al., ICML 2020 (the `prdc` package)
  compute_prdc_from_features   precision, recall, density and coverage in one dict
  compute_feature_stats_for_images        images -> FeatureStats through a `synthesis.DetectorEngine` (metric_utils.py:314-320)
  compute_feature_stats_for_aug_dataset   metrics/metric_utils.py:264-328: the `img_aug/` pickles of the reference's drivers
  compute_metrics_from_images             precision / recall / density / coverage / KID of two image sets

The detectors (Inception-v3 and VGG16 pickles hosted by NVIDIA, metric_utils.py:46-60) cannot be fetched offline.  The VGG16 one has a
local counterpart -- the TorchScript `vgg16.pt` the LPIPS criterion already needs -- and `synthesis.DetectorEngine.from_torchscript`
runs its `return_features=True` branch on the HIP path, so precision / recall, density / coverage and KID start from images.  The
Inception-v3 pickle has none: FID keeps taking features or moments that the caller supplies.
torch only owns the device memory; the moments, distances, radii, membership tests and kernel sums are HIP kernels (la_metrics.hip).
"""
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
    ws = torch.empty([lib.la_pr_workspace_floats(r.shape[0], c.shape[0])], dtype=torch.float32, device=dev)
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
        ws = torch.empty([lib.la_pr_workspace_floats(max(nm, npb), nm)], dtype=torch.float32, device=dev)
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
    ws = torch.empty([ws_bytes // 8], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):          # the stream must be `dev`'s, not the current device's
        _lib.check(lib.la_kid_poly3_f32(_lib.ptr(gen), gen.shape[0], _lib.ptr(real), real.shape[0], gen.shape[1], _lib.ptr(ixd),
                                        _lib.ptr(iyd), S, mx, my, _lib.ptr(out), _lib.ptr(out[S * 3:]), _lib.ptr(out[S * 4:]),
                                        _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'kid_poly3')
    out = out.cpu().numpy()
    kid = float(out[S * 4])
    if return_details:
        return kid, dict(mmd2=out[S * 3:S * 4].copy(), sums=out[:S * 3].reshape(S, 3).copy(), ix=ix, iy=iy)
    return kid


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
    ws = torch.empty([ws_bytes // 4], dtype=torch.float32, device=dev)
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
                                kid_max_subset_size=1000, kid_seed=0):
    """{'precision', 'recall', 'density', 'coverage', 'kid'} of generated against real images, through `detector` and the functions
    above (precision_recall.py:36-85 with nhood_size=3 is the reference's pr50k3)."""
    real = compute_feature_stats_for_images(real_batches, detector, mode=mode, max_items=max_items, capture_all=True).get_all()
    gen = compute_feature_stats_for_images(gen_batches, detector, mode=mode, max_items=max_items, capture_all=True).get_all()
    out = compute_prdc_from_features(real, gen, nhood_size=nhood_size, device=detector.device)
    out['kid'] = compute_kid_from_features(real, gen, num_subsets=kid_num_subsets, max_subset_size=kid_max_subset_size, seed=kid_seed,
                                           device=detector.device)
    return out
