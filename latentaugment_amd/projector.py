"""Projector: invert images into W / W+ on the HIP engines (Karras et al. 2020, "Analyzing and Improving the Image Quality of
StyleGAN", Appendix D; `optimize_noise=True` optimises the per-layer noise maps beside the latent, with the published regulariser
and re-normalisation, and discards them).  DESIGN.md 'Projector' holds the definition.

The reference reads one inverted latent per slice (augments/latent_aug.py:310-324, `init_w == 'inv'`) and has no code that makes them;
`project_dataset` writes the zip it reads.  A step is an eager sequence of launches: SynthesisEngine forward, the perceptual
preparation (box average, repeat to three channels, the net's input affine), FeatureEngine forward, the distance kernel, the two
backward passes, and one fused tail (Adam + the next step's noised latent); with the noise maps, the channel reductions inside the
synthesis backward pass, the regulariser and the maps' own tail.  Nothing is read back inside the step loop.  There is no
CPU fallback: a missing library or a host tensor is a `LatentAugHipError`.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .synthesis import FeatureEngine, MappingEngine, SynthesisEngine, _state_dict_of

SPACES = ('w', 'w+')
BOX_FACTORS = (1, 2, 4, 8)
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
NOISE_LAYER0 = 0x40000000      # layer slot of map li in the noise stream: NOISE_LAYER0 + li, disjoint from the step indices of the latent noise


def schedule(t, num_steps, w_std, initial_lr=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25, lr_rampup_length=0.05,
             noise_ramp_length=0.75):
    """(lr_t, sigma_t) of step t of num_steps, in float64 on the host: the noise falls quadratically to zero at tau = noise_ramp_length,
    the learning rate rises linearly over lr_rampup_length and falls by a half cosine over the last lr_rampdown_length."""
    tau = t / num_steps
    sigma = w_std * initial_noise_factor * max(0.0, 1.0 - tau / noise_ramp_length) ** 2
    ramp = min(1.0, (1.0 - tau) / lr_rampdown_length)
    ramp = 0.5 - 0.5 * math.cos(math.pi * ramp)
    ramp = ramp * min(1.0, tau / lr_rampup_length)
    return initial_lr * ramp, sigma


def box_factor(img_resolution, lpips_res):
    """k of the perceptual preparation: the generator's resolution over the feature net's, refused unless it is 1, 2, 4 or 8."""
    k = img_resolution // lpips_res if lpips_res >= 1 and img_resolution % lpips_res == 0 else 0
    if k not in BOX_FACTORS:
        raise _lib.LatentAugHipError(f'Projector: the generator makes {img_resolution}^2 images and the feature net takes {lpips_res}^2; '
                                     f'their ratio must be one of {BOX_FACTORS}')
    return k


def check_feature_batch(feat_max_batch, img_channels, max_batch):
    if feat_max_batch < img_channels * max_batch:
        raise _lib.LatentAugHipError(f'Projector: every modality of every sample is a row of the feature net: its max_batch must be at '
                                     f'least img_channels * max_batch = {img_channels} * {max_batch}; got {feat_max_batch}')


def check_project_args(targets_shape, img_channels, img_resolution, num_ws, w_dim, num_steps, space, w_pix, w_start_shape=None,
                       regularize_noise_weight=0.0):
    """The refusals of project(), before anything is launched.  Returns the rows L of the optimised latent (1 or num_ws)."""
    if space not in SPACES:
        raise _lib.LatentAugHipError(f'project: space = {space!r}; expected one of {SPACES}')
    if not isinstance(num_steps, (int, float)) or int(num_steps) != num_steps or num_steps < 1:
        raise _lib.LatentAugHipError(f'project: num_steps must be a whole number of at least 1; got {num_steps!r}')
    if not (w_pix >= 0.0 and math.isfinite(w_pix)):
        raise _lib.LatentAugHipError(f'project: w_pix must be finite and not negative; got {w_pix!r}')
    if not (regularize_noise_weight >= 0.0 and math.isfinite(regularize_noise_weight)):
        raise _lib.LatentAugHipError(f'project: regularize_noise_weight must be finite and not negative; got {regularize_noise_weight!r}')
    want = (img_channels, img_resolution, img_resolution)
    if len(targets_shape) != 4 or tuple(targets_shape[1:]) != want or targets_shape[0] < 1:
        raise _lib.LatentAugHipError(f'project: targets must be [N, {want[0]}, {want[1]}, {want[2]}] with N at least 1; got {tuple(targets_shape)}')
    L = num_ws if space == 'w+' else 1
    if w_start_shape is not None:
        ok = [(targets_shape[0], r, w_dim) for r in {1, L}] + [(r, w_dim) for r in {1, L}] + [(w_dim,)]
        if tuple(w_start_shape) not in ok:
            raise _lib.LatentAugHipError(f'project: w_start has shape {tuple(w_start_shape)}; expected [N, {L}, {w_dim}] (or one code '
                                         f'[{L}, {w_dim}] / [{w_dim}] for every sample)')
    return L


class NoiseMaps:
    """The noise maps of one batch of B samples: per layer with noise_strength != 0 a map [B, res, res] with its Adam moments and its
    gradient, and the tables the kernels take.  Map li of sample b starts as the unit normals of (seed, NOISE_LAYER0 + li, row0 + b): a
    function of the sample's global row, not of the batch it sits in."""

    def __init__(self, synth, B, seed, row0):
        lib = _lib.load()
        self.layers = [li for li, ns in enumerate(synth.noise_strengths) if ns != 0.0]
        self.res = [synth.layer_resolutions[li] for li in self.layers]
        self.B, self.num_layers = B, synth.num_layers
        f32 = dict(device=synth.device, dtype=torch.float32)
        self.n = [torch.empty([B, r, r], **f32) for r in self.res]
        self.m = [torch.zeros([B, r, r], **f32) for r in self.res]
        self.v = [torch.zeros([B, r, r], **f32) for r in self.res]
        self.g = [torch.empty([B, r, r], **f32) for r in self.res]
        for li, t, r in zip(self.layers, self.n, self.res):
            _lib.check(lib.la_noise_normal_f32(_lib.ptr(t), B, r * r, int(seed) & 0xFFFFFFFFFFFFFFFF, NOISE_LAYER0 + li, row0, _lib.stream_ptr()),
                       'la_noise_normal_f32')
        self.res_table = (C.c_int * len(self.res))(*self.res)
        self.tables = {k: (C.c_void_p * len(self.res))(*[t.data_ptr() for t in getattr(self, k)]) for k in 'nmvg'}

    def per_layer(self, maps):
        """The engine's list: one entry per layer, None where the layer has no noise."""
        out = [None] * self.num_layers
        for li, t in zip(self.layers, maps):
            out[li] = t
        return out


class Projector:
    def __init__(self, generator, feature_net, device, max_batch, precision='f16x2', lpips_res=None):
        """generator: the module or state dict SynthesisEngine.from_generator takes (its `mapping.*` tensors are optional).
        feature_net: a tap-list FeatureEngine with three input channels, or a described net (`lpips_reference_net`, a candidate of
        `vgg16_from_torchscript`: `.ops`, `.pre_scale`, `.pre_shift`), or a bare op list; the latter two are built at `lpips_res`
        (default: the generator's resolution) with max_batch = img_channels * max_batch."""
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.LatentAugHipError('Projector needs a ROCm device (no CPU fallback)')
        if int(max_batch) < 1:
            raise _lib.LatentAugHipError(f'Projector: max_batch must be at least 1; got {max_batch!r}')
        self.max_batch = int(max_batch)
        sd = _state_dict_of(generator)
        res = max(int(k.split('.')[0][1:]) for k in sd if k.startswith('b'))
        imgc = int(sd[f'b{res}.torgb.weight'].shape[0])
        if isinstance(feature_net, FeatureEngine):
            if lpips_res is not None and int(lpips_res) != feature_net.in_res:
                raise _lib.LatentAugHipError(f'Projector: lpips_res = {lpips_res} but the feature engine was built at {feature_net.in_res}')
            lpips_res = feature_net.in_res
            if feature_net.in_ch != 3 or feature_net.num_taps < 1:
                raise _lib.LatentAugHipError('Projector: the feature engine must be a tap list with three input channels')
            check_feature_batch(feature_net.max_batch, imgc, self.max_batch)
        lpips_res = res if lpips_res is None else int(lpips_res)
        self.k = box_factor(res, lpips_res)
        self.synth = SynthesisEngine.from_generator(generator, self.device, self.max_batch, precision=precision)
        self.img_resolution, self.img_channels = self.synth.img_resolution, self.synth.img_channels
        self.num_ws, self.w_dim = self.synth.num_ws, self.synth.w_dim
        self.lpips_res = lpips_res
        if isinstance(feature_net, FeatureEngine):
            self.feat = feature_net
        elif hasattr(feature_net, 'ops'):
            self.feat = FeatureEngine.from_net(feature_net, self.device, lpips_res, imgc * self.max_batch, precision=precision)
        else:
            self.feat = FeatureEngine(feature_net, self.device, lpips_res, imgc * self.max_batch, precision=precision)
        full = generator if isinstance(generator, dict) else generator.state_dict()
        self.mapping = MappingEngine(generator, self.device) if any(k.startswith('mapping.fc') for k in full) else None
        self.z_dim = self.mapping.z_dim if self.mapping is not None else self.w_dim
        self._lib = _lib.load()
        self._stats = {}
        self._sc = (C.c_float * 3)(*self.feat.pre_scale)
        self._sh = (C.c_float * 3)(*self.feat.pre_shift)
        # the adjoint entry of the preparation takes one scale: a net whose three scales differ gets them applied to the gradient first
        s = tuple(float(v) for v in self.feat.pre_scale)
        self._grad_scale = s[0] if s[0] == s[1] == s[2] else 1.0
        self._grad_scale_rows = None if s[0] == s[1] == s[2] else torch.tensor(s, device=self.device).reshape(1, 3, 1, 1)
        Cc, R, S, F = self.img_channels, self.img_resolution, lpips_res, self.feat.num_features
        f32 = dict(device=self.device, dtype=torch.float32)
        self._gfeat = torch.empty([Cc * self.max_batch, F], **f32)
        self._g_img = torch.empty([self.max_batch, Cc, R, R], **f32)
        self._small = torch.empty([self.max_batch, Cc, S, S], **f32) if self.k > 1 else None
        self._g_small = torch.empty([self.max_batch, Cc, S, S], **f32) if self.k > 1 else None
        self._xc = torch.empty([Cc * self.max_batch, 3, S, S], **f32)
        nbytes = max(self._lib.la_row_dist_workspace_bytes(Cc * self.max_batch, F), self._lib.la_row_dist_workspace_bytes(self.max_batch, Cc * R * R))
        # one allocation: the scratch of the noise regulariser and of the noise tail (for max_batch samples; a smaller batch's layout fits
        # inside), then the row distance's partials; every part starts on a 64-byte boundary
        noisy = [r for r, ns in zip(self.synth.layer_resolutions, self.synth.noise_strengths) if ns != 0.0]
        table = (C.c_int * len(noisy))(*noisy)
        reg_b = self._lib.la_noise_reg_scratch_bytes(table, len(noisy), self.max_batch) if noisy else 0
        tail_b = self._lib.la_proj_noise_tail_scratch_bytes(table, len(noisy), self.max_batch) if noisy else 0
        whole = _lib.workspace(reg_b + tail_b + nbytes, self.device, torch.float64)
        self._noise_ws = (whole[:reg_b // 8], whole[reg_b // 8:(reg_b + tail_b) // 8])
        self._ws = whole[(reg_b + tail_b) // 8:]

    # ---- the start
    def w_stats(self, w_avg_samples=10000, seed=123):
        """(w_avg [w_dim] float64, w_std: one float) of mapping(z, psi = 1)[:, 0] over `w_avg_samples` z of a seeded host generator; the
        moments are taken in float64 on the host from the MappingEngine's output.  Once per (samples, seed)."""
        key = (int(w_avg_samples), int(seed))
        if key not in self._stats:
            if self.mapping is None:
                raise _lib.LatentAugHipError('Projector: the generator has no mapping.fc* tensors; pass w_start, or w_avg and w_std')
            z = torch.from_numpy(np.random.RandomState(key[1]).randn(key[0], self.z_dim).astype(np.float32))
            w = torch.cat([self.mapping.forward(z[i:i + 4096].to(self.device), 1, truncation_psi=1.0)[:, 0] for i in range(0, key[0], 4096)])
            w = w.cpu().double().numpy()
            avg = w.mean(axis=0)
            self._stats[key] = (avg, float(np.sqrt(np.sum((w - avg) ** 2) / key[0])))
        return self._stats[key]

    # ---- launches
    def _prepare(self, img, B):
        """[B, C, R, R] -> the feature net's batch [C * B, 3, S, S] (rows modality-major): box average, repeat, input affine."""
        Cc, R, S = self.img_channels, self.img_resolution, self.lpips_res
        src = img
        if self.k > 1:
            src = self._small[:B]
            _lib.check(self._lib.la_box_down_f32(_lib.ptr(img), _lib.ptr(src), B * Cc, R, self.k, _lib.stream_ptr()), 'la_box_down_f32')
        xc = self._xc[:Cc * B]
        _lib.check(self._lib.la_crop_repeat_affine_f32(_lib.ptr(src), _lib.ptr(xc), B, Cc, S, S, 0, 0, 3, self._sc, self._sh, _lib.stream_ptr()),
                   'la_crop_repeat_affine_f32')
        return xc

    def _prepare_adjoint(self, gxc, B):
        """d / d(prepared batch) [C * B, 3, S, S] -> d / d(img), written to the [B, C, R, R] gradient buffer."""
        Cc, R, S = self.img_channels, self.img_resolution, self.lpips_res
        if self._grad_scale_rows is not None:
            gxc.mul_(self._grad_scale_rows)
        g_img = self._g_img[:B]
        dst = g_img if self.k == 1 else self._g_small[:B]
        dst.zero_()
        _lib.check(self._lib.la_crop_repeat_grad_f32(_lib.ptr(gxc), _lib.ptr(dst), B, Cc, S, S, 0, 0, 3, self._grad_scale, _lib.stream_ptr()),
                   'la_crop_repeat_grad_f32')
        if self.k > 1:
            _lib.check(self._lib.la_box_up_f32(_lib.ptr(dst), _lib.ptr(g_img), B * Cc, R, self.k, _lib.stream_ptr()), 'la_box_up_f32')
        return g_img

    def _row_dist(self, a, t, rows, K, fold, scale, gscale, g, accumulate, loss, loss_index):
        _lib.check(self._lib.la_row_dist_f32(_lib.ptr(a), _lib.ptr(t), rows, K, fold, scale, gscale, _lib.ptr(g), accumulate,
                                             C.c_void_p(loss.data_ptr() + 8 * loss_index), loss.shape[-1], _lib.ptr(self._ws), self._ws.numel() * 8,
                                             _lib.stream_ptr()), 'la_row_dist_f32')

    def target_features(self, targets):
        """F(T) of one batch [B, C, R, R]: [C * B, num_features], rows modality-major."""
        return self.feat.forward(self._prepare(targets, targets.shape[0])).clone()

    def loss_and_grad(self, ws, targets, target_feat, w_pix, loss, maps=None, reg_weight=0.0):
        """One evaluation at `ws` ([B, 1 or num_ws, w_dim]): the per-sample terms go to loss [B, 2] float64 (perceptual, pixel), the
        return value is d(sum of both) / d(ws) per style slot, [B, num_ws, w_dim].  Also returns the image.  With `maps` (NoiseMaps) the
        image is made with them, loss is [B, 3] with reg_weight * regulariser as its third column, and maps.g receives
        d(sum of the three) / d(map)."""
        B, Cc, R = ws.shape[0], self.img_channels, self.img_resolution
        img = self.synth.forward(ws, noise_mode='const') if maps is None else self.synth.forward(ws, noise_mode='random', noises=maps.per_layer(maps.n))
        feat = self.feat.forward(self._prepare(img, B))
        gfeat = self._gfeat[:Cc * B]
        self._row_dist(feat, target_feat, Cc * B, self.feat.num_features, Cc, 1.0 / Cc, 2.0 / Cc, gfeat, 0, loss, 0)
        g_img = self._prepare_adjoint(self.feat.backward(gfeat), B)
        if w_pix > 0.0:
            n = Cc * R * R
            self._row_dist(img, targets, B, n, 1, w_pix / n, 2.0 * w_pix / n, g_img, 1, loss, 1)
        if maps is None:
            return self.synth.backward(g_img), img
        dws, _ = self.synth.backward(g_img, noise_grads=maps.per_layer(maps.g))
        reg_ws, _ = self._noise_ws
        _lib.check(self._lib.la_noise_reg_f32(maps.tables['n'], maps.res_table, len(maps.res), B, reg_weight, reg_weight, maps.tables['g'], 1,
                                              C.c_void_p(loss.data_ptr() + 16), loss.shape[-1], _lib.ptr(reg_ws), reg_ws.numel() * 8, _lib.stream_ptr()),
                   'la_noise_reg_f32')
        return dws, img

    def noise_tail(self, maps, step, lr):
        """Adam step `step` (1-based, the latent's lr, betas and eps) on every map from maps.g, then n -= mean(n); n *= rsqrt(mean(n^2))."""
        _, tail_ws = self._noise_ws
        _lib.check(self._lib.la_proj_noise_tail_f32(maps.tables['g'], maps.tables['n'], maps.tables['m'], maps.tables['v'], maps.res_table, len(maps.res),
                                                    maps.B, step, lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, _lib.ptr(tail_ws), tail_ws.numel() * 8,
                                                    _lib.stream_ptr()), 'la_proj_noise_tail_f32')

    def step_tail(self, dws, w_opt, m, v, ws, step, lr, sigma, seed, layer, row0):
        """Adam step `step` (1-based) on w_opt from dws (None: no update), then ws = w_opt + sigma * n(seed, layer, row0 + b, element)."""
        B, L = w_opt.shape[0], w_opt.shape[1]
        _lib.check(self._lib.la_proj_step_tail_f32(_lib.ptr(dws), _lib.ptr(w_opt), _lib.ptr(m), _lib.ptr(v), _lib.ptr(ws), B, self.num_ws, self.w_dim,
                                                   int(L != 1), step, lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, sigma,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, layer, row0, _lib.stream_ptr()), 'la_proj_step_tail_f32')

    # ---- the optimisation
    def project(self, targets, num_steps=1000, space='w', w_pix=0.0, seed=0, w_start=None, w_avg=None, w_std=None, w_avg_samples=10000,
                w_avg_seed=123, row0=0, optimize_noise=False, regularize_noise_weight=1e5, **sched):
        """targets [N, C, R, R] float32 in the generator's range (device tensor) -> {'w' [N, num_ws, w_dim], 'img' [N, C, R, R],
        'loss' float64 [num_steps, N, 2] (perceptual, pixel term per step and sample)}, all on the device.  Batches of max_batch, the last
        one ragged; sample n draws the noise of global row row0 + n, whatever max_batch is and however a data set is cut into calls.  `sched`: the keywords of `schedule` (initial_lr, initial_noise_factor, lr_rampdown_length, lr_rampup_length,
        noise_ramp_length).
        optimize_noise: every layer with noise_strength != 0 gets a map [res, res] per sample, started from the unit normals of
        (seed, NOISE_LAYER0 + layer, row0 + n), optimised by the same Adam beside the latent under regularize_noise_weight * the published
        regulariser and re-normalised after every step; 'img' is made with the optimised maps, the result gains 'noises' (per engine
        layer [N, res, res], None where the strength is 0) and 'loss' is [num_steps, N, 3] (..., regularize_noise_weight * reg)."""
        _lib.require_gpu(targets)
        L = check_project_args(tuple(targets.shape), self.img_channels, self.img_resolution, self.num_ws, self.w_dim, num_steps, space, float(w_pix),
                               None if w_start is None else tuple(w_start.shape), float(regularize_noise_weight))
        T = int(num_steps)
        schedule(0, T, 1.0, **sched)      # (an unknown keyword is refused here, before the first launch)
        N = targets.shape[0]
        targets = targets.to(self.device, torch.float32).contiguous()
        if w_std is None or (w_start is None and w_avg is None):
            avg_m, std_m = self.w_stats(w_avg_samples, w_avg_seed)
            w_avg = avg_m if w_avg is None else w_avg
            w_std = std_m if w_std is None else w_std
        w_std = float(w_std)
        if w_start is None:
            w_start = torch.as_tensor(np.asarray(w_avg, dtype=np.float64)).to(torch.float32).reshape(1, 1, self.w_dim)
        start = torch.as_tensor(w_start).to(self.device, torch.float32)
        start = start.reshape((1,) * (3 - start.ndim) + tuple(start.shape)).expand(N, L, self.w_dim)
        out_w = torch.empty([N, self.num_ws, self.w_dim], device=self.device, dtype=torch.float32)
        out_img = torch.empty_like(targets)
        optimize_noise = bool(optimize_noise) and any(ns != 0.0 for ns in self.synth.noise_strengths)
        ncol = 3 if optimize_noise else 2
        out_loss = torch.zeros([T, N, ncol], device=self.device, dtype=torch.float64)
        out_noises = None
        if optimize_noise:
            out_noises = [None if ns == 0.0 else torch.empty([N, r, r], device=self.device, dtype=torch.float32)
                          for r, ns in zip(self.synth.layer_resolutions, self.synth.noise_strengths)]
        with torch.cuda.device(self.device):
            for n0 in range(0, N, self.max_batch):
                B = min(self.max_batch, N - n0)
                tgt = targets[n0:n0 + B]
                tfeat = self.target_features(tgt)
                w_opt = start[n0:n0 + B].contiguous().clone()
                m, v, ws = torch.zeros_like(w_opt), torch.zeros_like(w_opt), torch.empty_like(w_opt)
                loss = torch.zeros([T, B, ncol], device=self.device, dtype=torch.float64)
                maps = NoiseMaps(self.synth, B, seed, row0 + n0) if optimize_noise else None
                self.step_tail(None, w_opt, m, v, ws, 0, 0.0, schedule(0, T, w_std, **sched)[1], seed, 0, row0 + n0)
                for t in range(T):
                    dws, _ = self.loss_and_grad(ws, tgt, tfeat, float(w_pix), loss[t], maps, float(regularize_noise_weight))
                    lr = schedule(t, T, w_std, **sched)[0]
                    sigma = schedule(t + 1, T, w_std, **sched)[1] if t + 1 < T else 0.0
                    self.step_tail(dws, w_opt, m, v, ws, t + 1, lr, sigma, seed, t + 1, row0 + n0)
                    if maps is not None:
                        self.noise_tail(maps, t + 1, lr)
                out_w[n0:n0 + B] = w_opt.expand(B, self.num_ws, self.w_dim)
                if maps is None:
                    self.synth.forward(w_opt, noise_mode='const', out=out_img[n0:n0 + B])
                else:
                    self.synth.forward(w_opt, noise_mode='random', noises=maps.per_layer(maps.n), out=out_img[n0:n0 + B])
                    for li, t_map in zip(maps.layers, maps.n):
                        out_noises[li][n0:n0 + B] = t_map
                out_loss[:, n0:n0 + B] = loss
        res = {'w': out_w, 'img': out_img, 'loss': out_loss}
        if optimize_noise:
            res['noises'] = out_noises
        return res


def project_dataset(img_zip, out_zip, split, projector, modalities, num_steps=1000, space='w', seed=0, resolution=None, log=None, **kw):
    """Invert every slice of an image zip (formats.ImgDataset: raw 0 .. 255 per modality, scaled to the generator's [-1, 1] as the image
    bank is) and write the latent zip that opt.dataset_w_name points at: one member per slice under the image zip's own member name,
    a pickled float32 ndarray [num_ws, w_dim] (formats.write_latent_zip).  Slice i is global row i of the noise stream.  Returns the
    final per-slice terms, float64 [N, 2].  `kw` goes to project(): with optimize_noise=True the maps are optimised and, as in the published
    method, discarded -- only w is written -- and the returned array is [N, 3]."""
    from . import formats
    if os.path.splitext(out_zip)[1].lower() != '.zip':
        raise IOError('Path must point to a zip')
    ds = formats.ImgDataset(img_zip, split, list(modalities), resolution=projector.img_resolution if resolution is None else resolution)
    names, finals = [], []

    def codes():
        B = projector.max_batch
        for i0 in range(0, len(ds), B):
            items = [ds[i] for i in range(i0, min(i0 + B, len(ds)))]
            x = torch.from_numpy(np.stack([it[0] for it in items])) / 127.5 - 1
            # (one project() call per batch, with the batch's first global row: the whole data set never sits on the device at once)
            res = projector.project(x.to(projector.device), num_steps=num_steps, space=space, seed=seed, row0=i0, **kw)
            w = res['w'].cpu().numpy()
            finals.append(res['loss'][-1].cpu().numpy())
            for (_, fname), code in zip(items, w):
                names.append(fname)
                yield fname, code
            if log is not None:
                log(f'{len(names)} / {len(ds)} slices')
    part = os.path.splitext(out_zip)[0] + '.part.zip'      # (an interrupted run leaves no half-written zip under the final name)
    formats.write_latent_zip(part, codes())
    os.replace(part, out_zip)
    return np.concatenate(finals)
