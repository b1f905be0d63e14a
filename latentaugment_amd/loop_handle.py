"""What runs the N-step optimisation on one stream: `LoopHandle` (engines + the `la_latent_opt` handle + its workspaces) over `LoopBanks`
(the device-resident banks, built once and shared by reference).  `LatentAug` keeps one handle for the whole local batch and two more, of
half the batch each, for the stream lanes; all three read the same banks and build their feature engines from the one resolved net."""
import collections
import ctypes as C
import os

import torch

from . import _lib
from .loop_options import LATENT_SPACES, _preproc3, center_crop_geometry, get_params
from .synthesis import DiscriminatorEngine, FeatureEngine, ScriptedFeatureNet, SynthesisEngine

# The perceptual net of a configuration, loaded ONCE: `kind` of resolve_perceptual_net, `net` a described net for FeatureEngine.from_net
# (`.ops`, and the input affine the net brings: `.pre_scale`, `.pre_shift` -- carried here, never written to `opt`).
PerceptualNet = collections.namedtuple('PerceptualNet', 'kind net')


def load_perceptual_net(resolved, device, in_res):
    """resolve_perceptual_net's answer -> PerceptualNet (None stays None)."""
    if resolved is None:
        return None
    kind, src = resolved
    if kind == 'ops':
        return PerceptualNet(kind, ScriptedFeatureNet(src, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), False, None))
    if kind == 'reference':
        # LPIPS('vgg') of the reference: three taps, z-score input.  The tap vector makes squared L2 against a bank row the
        # reference's d(x, y_m), so sum / (n * M) per modality is its forward_tr (lpips.py:60-68) -- exactly at n = 1, the only
        # batch its broadcast (fx - fy) admits -- through the loop code of the TorchScript branch, unchanged.
        from .synthesis import lpips_reference_net
        # (src carries the trunk as a third element for LPIPS('alex') / LPIPS('squeeze'): five / seven taps, the same z-score)
        print(f'Loading {"VGG16" if len(src) == 2 else src[2]} / LPIPS lin weights from: {src[:2]}')
        return PerceptualNet(kind, lpips_reference_net(*src))
    # the script's own input layer, (x - mean_k) / std_k; the reference hands it the synthesised crop as it is (:394-395)
    print(f'Loading VGG16 from: {src}')
    return PerceptualNet(kind, FeatureEngine.verified_torchscript_net(src, device, in_res))


def lpips_preproc(options, pnet):
    """Input affine of the perceptual criterion: opt.lpips_preproc where given, else the net's own."""
    return options.lpips_preproc if options.lpips_preproc is not None else _preproc3((pnet.net.pre_scale, pnet.net.pre_shift))


class LoopBanks:
    """The banks of the criteria on the device: `W` [Mw, num_ws, w_dim], `Xc` (centre-cropped, modality-major [C][Mx][crop*crop]) and
    `Fbank` [C][Mf][F]; from the `banks=` dict ('W', 'X', 'fea'), else from the interim zips with their cache (reference :137-171).  A bank
    is built when the first handle asks for it -- the latent and pixel banks need the generator's latent shape, the feature bank a
    feature engine -- and every later handle gets the same tensor."""

    def __init__(self, options, phase, device, banks=None, latent_codes=None):
        self.options, self.phase, self.device = options, phase, device
        self.latent_codes = latent_codes
        self._from_zips = banks is None and bool(options.interim_dir and options.dataset_aug)
        self._src = dict(banks or {})
        self.center_crop, self.center_off = center_crop_geometry(options.img_resolution)
        self.W = self.Xc = self.Fbank = None
        self._built = False

    def _root(self):
        return os.path.join(self.options.interim_dir, self.options.dataset_aug)

    def _img_dataset(self):
        from . import formats
        o = self.options
        return formats.ImgDataset(os.path.join(self._root(), o.dataset_name_aug + '.zip'), split=self.phase, modalities=list(o.modalities),
                                  resolution=o.img_resolution)

    def latent_and_pixel(self, num_ws, w_dim):
        """(W, Xc), each None where its criterion is off."""
        if self._built:
            return self.W, self.Xc
        o, src = self.options, self._src
        if self._from_zips:
            # real-data banks from the interim zips (reference :137-158), cached as DatasetStats pickles
            from . import formats
            cache_dir = os.path.join(self._root(), 'cache_dir')
            wzip = os.path.join(self._root(), o.dataset_w_name + '.zip')
            if self.latent_codes is None and os.path.isfile(wzip):
                self.latent_codes = formats.LatentCodeDataset(wzip, split=self.phase, w_dim=w_dim, num_ws=num_ws)
            if o.w_latent > 0:
                src['W'] = formats.compute_stats(self.latent_codes, 'latent', cache_dir, step=o.step_w).get_all_torch()
            if o.w_pix > 0:
                src['X'] = formats.compute_stats(self._img_dataset(), 'img', cache_dir, step=o.step_img).get_all_torch()
        if o.w_latent > 0:
            self.W = src['W'].to(device=self.device, dtype=torch.float32).contiguous()
            assert self.W.shape[1:] == (num_ws, w_dim)
        if o.w_pix > 0:
            res, crop, off = o.img_resolution, self.center_crop, self.center_off
            X = src['X'].to(device=self.device, dtype=torch.float32).contiguous()     # [M, C, R, R] in [-1, 1]
            assert X.shape[1:] == (len(o.modalities), res, res)
            xc = torch.empty([X.shape[0], X.shape[1], crop, crop], device=self.device, dtype=torch.float32)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().la_center_crop_f32(_lib.ptr(X), _lib.ptr(xc), X.shape[0] * X.shape[1], res, crop, off,
                                                          _lib.stream_ptr()), 'la_center_crop')
            self.Xc = xc.permute(1, 0, 2, 3).contiguous()      # modality-major [C][M][crop*crop]
        src.pop('W', None)      # (the host-side sources are not kept)
        src.pop('X', None)
        self._built = True
        return self.W, self.Xc

    def features(self, feat, pnet):
        """Fbank for the feature engine `feat` of the perceptual net `pnet`."""
        if self.Fbank is None:
            if 'fea' not in self._src:
                if not (self.options.interim_dir and self.options.dataset_aug):
                    raise _lib.LatentAugHipError("w_lpips > 0 needs banks['fea'] or the interim image zip to build them from")
                self._src['fea'] = self._build_feature_banks(feat, pnet)
            fea = self._src.pop('fea')
            assert len(fea) == len(self.options.modalities)
            self.Fbank = torch.stack([t.to(device=self.device, dtype=torch.float32) for t in fea]).contiguous()   # [C][Mf][F]
        assert self.Fbank.shape[2] == feat.num_features, 'feature bank does not match the feature net'
        return self.Fbank

    def _build_feature_banks(self, feat, pnet):
        """fea_<mode> banks (reference :160-171 / extract_features_mode_torchscript :565-580): per real image and modality,
        a crop_size_aug^2 crop at a freshly drawn random position, repeated to 3 channels, through the feature net.
        `opt.lpips_bank_range`: 'unit' (default) feeds x/127.5-1, consistent with the synthesised images; 'raw' reproduces
        the reference's 0..255 input (SURVEY 3.4 defect f)."""
        from . import formats
        o = self.options
        ds = self._img_dataset()
        raw = o.lpips_bank_range == 'raw'
        scale, shift = lpips_preproc(o, pnet)
        sc_t = torch.tensor(scale, device=self.device).reshape(1, 3, 1, 1)
        sh_t = torch.tensor(shift, device=self.device).reshape(1, 3, 1, 1)
        out = []
        for mode_id, mode in enumerate(o.modalities):
            def feature_fn(x, mode_id=mode_id):
                t = torch.from_numpy(x[:, mode_id:mode_id + 1]).to(self.device)
                if not raw:
                    t = t / 127.5 - 1
                ax, ay = o.crop_window(get_params(o.img_resolution, o.crop_size_aug, o.preprocess_aug)['crop_pos'])
                t = t[:, :, ay:ay + o.crop_size_aug, ax:ax + o.crop_size_aug].repeat(1, 3, 1, 1) * sc_t + sh_t   # plumbing
                return feat.forward(t.contiguous()).cpu().numpy()
            # The reference names the cache '<mode>-<crop>-features_jit-...': its contents also depend on the input range, the
            # preprocess and the feature-net weights, so those are folded into the tag -- a cache written by the reference (raw
            # 0..255 inputs, NVIDIA's weights) or under other settings is never picked up silently.
            tag = f'{mode}-{o.crop_size_aug}'
            if not (raw and (scale, shift) == ((1.0,) * 3, (0.0,) * 3) and o.lpips_cache_compat):
                def fmt(v):
                    return f'{v[0]:g}' if v[0] == v[1] == v[2] else '_'.join(f'{t:g}' for t in v)
                tag += f"-{'raw' if raw else 'unit'}-s{fmt(scale)}-b{fmt(shift)}-w{feat.weights_digest}"
            # (the reference's LPIPS('vgg') branch caches under the 'features' manifold, util_latent_aug.py:184: its per-layer list is
            #  this engine's one tap vector, kept as [M, F, 1, 1])
            manifold = 'features' if pnet.kind == 'reference' else 'features_jit'
            st = formats.compute_stats(ds, manifold, os.path.join(self._root(), 'cache_dir'), cache_tag=tag,
                                       step=o.step_img, feature_fn=feature_fn)
            out.append(st.get_all_torch().flatten(1))
        return out


class LoopHandle:
    """One `la_latent_opt` handle with the engines and workspaces it runs on: a SynthesisEngine, a DiscriminatorEngine where w_disc > 0,
    a FeatureEngine where w_lpips > 0, for batches of at most `max_batch`."""

    def __init__(self, options, generator, discriminator, pnet, banks, max_batch, device):
        o = self.options = options
        self.device, self.max_batch = device, max_batch
        self.wplus, self.overlap_criteria = o.wplus, o.overlap_criteria
        lib = self._lib = _lib.load()
        self.engine = SynthesisEngine.from_generator(generator, device, max_batch, precision=o.precision)
        assert self.engine.img_resolution == o.img_resolution, 'opt.img_resolution does not match the generator'
        assert self.engine.img_channels == len(o.modalities), 'one image channel per modality expected'
        res, imgc, w_dim = o.img_resolution, self.engine.img_channels, self.engine.w_dim
        self.banks = banks
        W, Xc = banks.latent_and_pixel(self.engine.num_ws, w_dim)
        Mw, Mx = (W.shape[0] if W is not None else 0), (Xc.shape[1] if Xc is not None else 0)
        crop, off = banks.center_crop, banks.center_off
        cfg = _lib.OptConfig(steps=int(o.opt_num_epochs), lr=float(o.opt_lr), beta1=0.9, beta2=0.999, eps=1e-8,
                             w_latent=float(o.w_latent), w_pix=float(o.w_pix), w_disc=float(o.w_disc), w_lpips=float(o.w_lpips),
                             criterion_mode=o.criterion_code, soft_aug=int(o.soft_aug), alpha=float(o.alpha), loop_noise_mode=1,
                             final_noise_mode=o.final_noise_code, norm_batch=o.norm_batch, crop=crop, crop_off=off)
        self._cfg = cfg
        space = LATENT_SPACES[o.latent_space]
        nbytes = lib.la_latent_opt_workspace_bytes_ex(res, imgc, w_dim, C.byref(cfg), Mw, Mx, max_batch, space)
        self._workspace = _lib.workspace(max(nbytes, 64), device)
        h = C.c_void_p()
        _lib.check(lib.la_latent_opt_create_ex(self.engine.handle, res, imgc, w_dim, C.byref(cfg), _lib.ptr(W), Mw, _lib.ptr(Xc), Mx,
                                               max_batch, space, _lib.ptr(self._workspace), self._workspace.numel(), C.byref(h)),
                   'la_latent_opt_create')
        self._h = h
        # launch mode of the step loop: one captured step replayed (default) or every launch eager (`opt.hip_graph = False`)
        _lib.check(lib.la_latent_opt_set_graph(h, int(o.hip_graph)), 'la_latent_opt_set_graph')
        _lib.check(lib.la_latent_opt_set_overlap(h, o.overlap_criteria), 'la_latent_opt_set_overlap')
        # rows of the image that the loop's criteria read: the pixel criterion its centre crop (util_dataset.py:317-323), the perceptual
        # criterion a crop_size_aug window inside that crop when preprocess_aug is one of the centre modes -- the loop steps then
        # synthesise only what those rows depend on (la_latent_opt_set_row_window; `opt.loop_window = False`: whole frames in every step).
        # The discriminator reads whole frames: no window.
        self.loop_window = None
        if o.loop_window and o.w_disc <= 0 and (o.w_pix > 0 or o.w_lpips > 0) and \
                (o.w_lpips <= 0 or o.preprocess_aug in ('center_crop', 'center_random_crop')):
            self.loop_window = (off, off + crop)
            _lib.check(lib.la_latent_opt_set_row_window(h, off, off + crop), 'la_latent_opt_set_row_window')
            if o.loop_window_columns:      # (the crop is a square; the top block follows its columns too)
                _lib.check(lib.la_latent_opt_set_col_window(h, off, off + crop), 'la_latent_opt_set_col_window')
        self.disc = None
        if o.w_disc > 0:
            if discriminator is None:
                raise _lib.LatentAugHipError('w_disc > 0 needs the discriminator (pass `discriminator=` or a network pickle)')
            self.disc = DiscriminatorEngine(discriminator, device, max_batch, precision=o.precision)
            assert self.disc.img_resolution == res and self.disc.img_channels == imgc
            _lib.check(lib.la_latent_opt_set_disc(h, self.disc.handle), 'la_latent_opt_set_disc')
        self.feat = None
        if o.w_lpips > 0:
            # perceptual criterion (reference :160-171, :387-409): features of crop_size_aug^2 crops, one bank per modality
            self.feat = FeatureEngine.from_net(pnet.net, device, in_res=o.crop_size_aug, max_batch=imgc * max_batch, precision=o.precision)
            Fbank = banks.features(self.feat, pnet)
            Mf = Fbank.shape[1]
            scale, shift = lpips_preproc(o, pnet)
            nb = lib.la_latent_opt_lpips_workspace_bytes(imgc, self.feat.num_features, o.crop_size_aug, Mf, max_batch)
            self._lpips_ws = _lib.workspace(nb, device)
            _lib.check(lib.la_latent_opt_set_lpips(h, self.feat.handle, _lib.ptr(Fbank), Mf, o.crop_size_aug, float(scale[0]),
                                                   float(shift[0]), _lib.ptr(self._lpips_ws), nb), 'la_latent_opt_set_lpips')
            _lib.check(lib.la_latent_opt_set_lpips_preproc(h, (C.c_float * 3)(*scale), (C.c_float * 3)(*shift), 3),
                       'la_latent_opt_set_lpips_preproc')
        self._keep = None

    def close(self):
        """Destroys the loop handle; the engines it points into go after it (with this object)."""
        h = getattr(self, '_h', None)
        if h:
            self._lib.la_latent_opt_destroy(h)
            self._h = None

    __del__ = close

    @property
    def graph_state(self):
        """1: the optimisation step is replayed from a captured hipGraph; 0: eager launches (`opt.hip_graph = False`, or no batch has
        run yet); -1: eager because the runtime refused the capture."""
        return int(self._lib.la_latent_opt_graph_state(self._h))

    def empty_pair(self, b):
        """Uninitialised (img [b,C,R,R], w_aug [b,num_ws,w_dim]) on the current stream."""
        e, res = self.engine, self.options.img_resolution
        return (torch.empty([b, e.img_channels, res, res], device=self.device, dtype=torch.float32),
                torch.empty([b, e.num_ws, e.w_dim], device=self.device, dtype=torch.float32))

    def run(self, w, final_noises=None, want_losses=False, crop_window_xy=None, trace=None, out=None):
        """w [b,1,w_dim] on this device (W+: [b,num_ws,w_dim]) -> (img [b,C,R,R], w_aug [b,num_ws,w_dim], losses or None) on the current
        stream.  crop_window_xy: absolute (x, y) of the perceptual criterion's window (needed where w_lpips > 0); out, trace: see
        LatentAug.run_local."""
        o, e, lib, h = self.options, self.engine, self._lib, self._h
        if self.feat is not None:
            _lib.check(lib.la_latent_opt_set_crop_pos(h, crop_window_xy[0], crop_window_xy[1]), 'la_latent_opt_set_crop_pos')
        w = w.to(device=self.device, dtype=torch.float32).contiguous()
        b, steps, res = w.shape[0], o.opt_num_epochs, o.img_resolution
        rows = e.num_ws if o.wplus else 1
        assert w.ndim == 3 and w.shape[1:] == (rows, e.w_dim), \
            f'latent_space {o.latent_space!r} takes w [b, {rows}, {e.w_dim}], got {tuple(w.shape)}'
        img, w_aug = out if out is not None else self.empty_pair(b)
        if out is not None:
            assert img.shape == (b, e.img_channels, res, res) and w_aug.shape == (b, e.num_ws, e.w_dim)
            assert img.is_contiguous() and w_aug.is_contiguous() and img.dtype == w_aug.dtype == torch.float32
        losses = torch.zeros([max(steps, 1), 4], device=self.device) if want_losses else None
        fn = None
        if self._cfg.final_noise_mode == 2:
            if final_noises is None:
                final_noises = e.make_noises(b)
            fn = e.noise_pointer_array(final_noises)
        tw = ti = tg = None
        want_img = trace is not None and 'img' in trace.get('want', ('w', 'img'))
        if trace is not None and steps > 0:
            wshape = [steps, b] + ([e.num_ws] if o.wplus else []) + [e.w_dim]
            tw = torch.empty(wshape, device=self.device, dtype=torch.float32)
            if want_img:
                ti = torch.empty([steps, b, e.img_channels, res, res], device=self.device, dtype=torch.float32)
            if 'grad' in trace.get('want', ()):
                tg = torch.empty(wshape, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            if tw is not None:
                _lib.check(lib.la_latent_opt_set_trace(h, _lib.ptr(tw), _lib.ptr(ti)), 'la_latent_opt_set_trace')
                _lib.check(lib.la_latent_opt_set_grad_trace(h, _lib.ptr(tg)), 'la_latent_opt_set_grad_trace')
            try:
                _lib.check(lib.la_latent_opt_run(h, _lib.ptr(w), b, fn, _lib.ptr(img), _lib.ptr(w_aug), _lib.ptr(losses),
                                                 _lib.stream_ptr()), 'la_latent_opt_run')
            finally:
                if tw is not None:
                    _lib.check(lib.la_latent_opt_set_trace(h, None, None), 'la_latent_opt_set_trace')
                    _lib.check(lib.la_latent_opt_set_grad_trace(h, None), 'la_latent_opt_set_grad_trace')
        if tw is not None:
            trace['w'] = tw
            if ti is not None:
                trace['img'] = ti
            if tg is not None:
                trace['grad'] = tg
        # Lifetime hold: the run is only ENQUEUED when this returns, and it may sit on a side stream (a lane).  A noise tensor whose last
        # Python reference went away would go back to the caching allocator, which may hand the memory to the main stream while this
        # stream still reads it.  It stays alive until the handle's next run.
        self._keep = final_noises
        return img, w_aug, losses
