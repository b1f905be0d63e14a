"""Host wrapper of the HIP synthesis engine: the `G.synthesis(ws, noise_mode=...)` the reference calls at
augments/utils/util_latent_aug.py:227,488, plus its backward to ws.

`SynthesisEngine.from_generator(G)` accepts any module (or state_dict) that carries the reference's parameter names
(models/stylegan3/legacy.py:171-203: synthesis.b{res}.{const, conv0.*, conv1.*, torgb.*}) -- i.e. the G_ema of a
network pickle -- copies the tensors to the device once and hands their pointers to the C ABI.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib

_CONV_KEYS = ('affine.weight', 'affine.bias', 'weight', 'bias', 'noise_const')
_RGB_KEYS = ('affine.weight', 'affine.bias', 'weight', 'bias')
NOISE_MODES = {'none': 0, 'const': 1, 'random': 2}
PRECISIONS = {'f32': 0, 'bf16x3': 1, 'bf16x2': 2, 'f16x2': 3}


def _state_dict_of(G):
    sd = G if isinstance(G, dict) else G.state_dict()
    if any(k.startswith('synthesis.') for k in sd):
        sd = {k[len('synthesis.'):]: v for k, v in sd.items() if k.startswith('synthesis.')}
    return sd


class SynthesisEngine:
    def __init__(self, state_dict, device, max_batch, conv_clamp=256.0, precision='f32'):
        lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.LatentAugHipError('SynthesisEngine needs a ROCm device (no CPU fallback)')
        sd = state_dict
        res_list = sorted({int(k.split('.')[0][1:]) for k in sd if k.startswith('b')})
        assert res_list and res_list[0] == 4, 'expected synthesis blocks b4..bR'
        self.img_resolution = res_list[-1]
        self.block_resolutions = res_list
        self.channels = [int(sd[f'b{r}.conv1.weight'].shape[0]) for r in res_list]
        self.img_channels = int(sd[f'b{res_list[-1]}.torgb.weight'].shape[0])
        self.w_dim = int(sd['b4.conv1.affine.weight'].shape[1])
        self.num_ws = lib.la_synth_num_ws(self.img_resolution)
        self.max_batch = int(max_batch)
        self.conv_clamp = float(-1.0 if conv_clamp is None else conv_clamp)

        def dev(name):
            t = sd[name].detach().to(device=self.device, dtype=torch.float32).contiguous()
            self._keep.append(t)
            return t

        self._keep = []
        params = []
        strengths = []
        self.layer_resolutions = []
        for r in res_list:
            if r == 4:
                params.append(dev('b4.const'))
            layers = ('conv1',) if r == 4 else ('conv0', 'conv1')
            for ln in layers:
                for k in _CONV_KEYS:
                    params.append(dev(f'b{r}.{ln}.{k}'))
                strengths.append(float(sd[f'b{r}.{ln}.noise_strength']))
                self.layer_resolutions.append(r)
            for k in _RGB_KEYS:
                t = dev(f'b{r}.torgb.{k}')
                if k == 'weight':
                    t = t.reshape(t.shape[0], t.shape[1]).contiguous()   # [imgc][cin][1][1] -> [imgc][cin]
                    self._keep.append(t)
                params.append(t)
        fkey = f'b{res_list[-1]}.resample_filter'
        fir = sd[fkey].detach().cpu().float().numpy() if fkey in sd else None
        if fir is None:
            f1 = np.array([1, 3, 3, 1], dtype=np.float32)
            fir = np.outer(f1, f1) / 64.0
        assert fir.shape == (4, 4), 'resample filter must be the 4x4 setup_filter([1,3,3,1])'
        self._fir = np.ascontiguousarray(fir, dtype=np.float32)
        self.noise_strengths = strengths
        self.num_layers = len(strengths)

        chan = (C.c_int * len(self.channels))(*self.channels)
        nbytes = lib.la_synth_workspace_bytes(self.img_resolution, self.img_channels, self.w_dim, chan, self.max_batch)
        assert nbytes > 0
        self._workspace = _lib.workspace(nbytes, self.device)
        self.workspace_bytes = nbytes
        pp = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        ns = (C.c_float * len(strengths))(*strengths)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.la_synth_create(self.img_resolution, self.img_channels, self.w_dim, chan, self.conv_clamp, pp,
                                           len(params), ns, len(strengths), self._fir.ctypes.data, 4, 4, self.max_batch,
                                           _lib.ptr(self._workspace), nbytes, _lib.stream_ptr(), C.byref(h)),
                       'la_synth_create')
        self._h = h
        self._lib = lib
        self.set_precision(precision)

    # fp16 operand scales (f16x2 mode): since round 4 every forward contraction's scale is derived from the DATA of the pass by the kernel
    # that produces its input (la_style.hip: la_xscale_bound_block; la_common.h: slot rows) -- no a-priori bound, no calibration, nothing
    # to select.  `operand_scale` is kept as a read-only description for log lines.
    operand_scale = 'data (producer-lowered slot rows)'

    def operand_headroom(self, ws):
        """Diagnostic: smallest ratio, over the 3x3 layers after the first and the samples of `ws`, between the data maximum of a
        forward fp16 operand, max|x*s|, and conv_clamp * max|s| -- how far a generator's activations sit below their clamp bound (rounds
        2-3 derived the forward scales from that bound and needed this ratio >= 2^-11; the product no longer depends on it).  One
        forward pass of `ws`; read from the stored layer outputs and styles."""
        ws = ws.to(self.device, torch.float32).contiguous()
        self.forward(ws, noise_mode='const')
        b = ws.shape[0]
        s = self.styles(b).abs()
        cins = [self.channels[0]] + [self.channels[self.block_resolutions.index(r)] for r in self.layer_resolutions[:-1]]
        ratio, off = float('inf'), cins[0]
        for k in range(1, len(self.layer_resolutions)):
            sk = s[:, off:off + cins[k]]
            xm = self.layer_output(k - 1, b).abs().amax(dim=(2, 3))
            r = (xm * sk).amax(dim=1) / (self.conv_clamp * sk.amax(dim=1)).clamp_min(1e-30)
            ratio = min(ratio, float(r.min()))
            off += cins[k]
        return ratio

    def set_precision(self, precision):
        """'f32' exact fp32 MFMA | 'f16x2' scaled split-fp16, 3 MFMAs (fp32-class error) | 'bf16x3' split-bf16, 6 MFMAs
        (fp32-class error) | 'bf16x2' split-bf16, 3 MFMAs (approximate)."""
        _lib.check(self._lib.la_synth_set_precision(self._h, PRECISIONS[precision]), 'la_synth_set_precision')
        self.precision = precision

    @classmethod
    def from_generator(cls, G, device, max_batch, conv_clamp=None, precision='f32'):
        if conv_clamp is None and not isinstance(G, dict):
            try:
                conv_clamp = getattr(G.synthesis, f'b{G.img_resolution}').conv1.conv_clamp
            except AttributeError:
                conv_clamp = 256.0
        return cls(_state_dict_of(G), device, max_batch, conv_clamp=256.0 if conv_clamp is None else conv_clamp,
                   precision=precision)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.la_synth_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def make_noises(self, batch, generator=None, batch_seed=None, rows=None):
        """Unit-variance noise tensors for noise_mode='random': one [B,res,res] per SynthesisLayer, None where the layer's
        noise_strength is 0 (the term vanishes, nothing is drawn).  Without `batch_seed`: torch.randn on the device generator (or
        `generator`).  With `batch_seed` the draw is a pure function of (seed, layer, GLOBAL sample row, element) -- the counter-based
        generator of the library (la_noise_normal_f32: Philox4x32-10 + Box-Muller) -- and `rows = (lo, hi)` generates samples
        lo..hi-1 of a batch of `batch` ONLY: a rank holding a shard draws its rows and nothing else (one launch per layer, no
        transient of the global batch's size; rounds 3-4 drew the whole batch with torch.randn on every rank and kept a slice),
        and the gathered batch does not depend on how it was sharded."""
        lo, hi = (0, batch) if rows is None else rows
        assert 0 <= lo <= hi <= batch
        out = []
        lib = _lib.load()
        for li, (r, ns) in enumerate(zip(self.layer_resolutions, self.noise_strengths)):
            if ns == 0.0:
                out.append(None)
            elif batch_seed is None:
                assert rows is None
                out.append(torch.randn([batch, r, r], device=self.device, generator=generator))
            else:
                t = torch.empty([hi - lo, r, r], device=self.device, dtype=torch.float32)
                with torch.cuda.device(self.device):
                    _lib.check(lib.la_noise_normal_f32(_lib.ptr(t), hi - lo, r * r, int(batch_seed) & 0xFFFFFFFFFFFFFFFF, li, lo,
                                                       _lib.stream_ptr()), 'la_noise_normal_f32')
                out.append(t)
        return out

    def noise_pointer_array(self, noises):
        if noises is None:
            return None
        assert len(noises) == self.num_layers
        for t, r, ns in zip(noises, self.layer_resolutions, self.noise_strengths):
            if t is None:
                assert ns == 0.0, 'a layer with noise_strength != 0 needs its noise tensor'
                continue
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[-2:] == (r, r)
        return (C.c_void_p * len(noises))(*[t.data_ptr() if t is not None else None for t in noises])

    def forward(self, ws, noise_mode='const', noises=None, out=None):
        """ws [B,num_ws,w_dim] (or [B,1,w_dim] / [B,w_dim]: W space) -> img [B,C,R,R]."""
        _lib.require_gpu(ws)
        ws = ws.contiguous().float()
        if ws.ndim == 2:
            ws = ws[:, None]
        B = ws.shape[0]
        assert ws.shape[2] == self.w_dim and ws.shape[1] in (1, self.num_ws)
        lstride = 0 if ws.shape[1] == 1 else self.w_dim
        mode = NOISE_MODES[noise_mode]
        if mode == 2 and noises is None:
            noises = self.make_noises(B)
        np_arr = self.noise_pointer_array(noises) if mode == 2 else None
        img = out if out is not None else torch.empty([B, self.img_channels, self.img_resolution, self.img_resolution],
                                                      device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_synth_forward(self._h, _lib.ptr(ws), ws.shape[1] * self.w_dim, lstride, B, mode, np_arr,
                                                  _lib.ptr(img), _lib.stream_ptr()), 'la_synth_forward')
        self._last_noises = noises   # keep alive until the matching backward
        return img

    def backward(self, g_img, noise_grads=None):
        """d(loss)/d(img) [B,C,R,R] -> d(loss)/d(ws) [B,num_ws,w_dim] for the last forward.  With `noise_grads` the same pass also
        delivers d(loss)/d(noise) per layer (la_synth_backward_noise) and the result is (dws, list): `True` allocates a [B,res,res]
        tensor for every layer with noise_strength != 0 (None elsewhere); a list per layer names the layers wanted -- a tensor is
        written in place, True is allocated, None / False is skipped (a wanted layer without noise gets zeros)."""
        g_img = g_img.contiguous().float()
        B = g_img.shape[0]
        dws = torch.empty([B, self.num_ws, self.w_dim], device=self.device, dtype=torch.float32)
        if noise_grads is None:
            with torch.cuda.device(self.device):
                _lib.check(self._lib.la_synth_backward(self._h, _lib.ptr(g_img), _lib.ptr(dws), _lib.stream_ptr()),
                           'la_synth_backward')
            return dws
        if noise_grads is True:
            noise_grads = [ns != 0.0 for ns in self.noise_strengths]
        if len(noise_grads) != self.num_layers:
            raise _lib.LatentAugHipError(f'backward: noise_grads must have one entry per layer ({self.num_layers}); got {len(noise_grads)}')
        gns = []
        for t, r in zip(noise_grads, self.layer_resolutions):
            if t is None or t is False:
                gns.append(None)
            elif t is True:
                gns.append(torch.empty([B, r, r], device=self.device, dtype=torch.float32))
            else:
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, r, r)):
                    raise _lib.LatentAugHipError(f'backward: a noise gradient must be a contiguous float32 device tensor [{B}, {r}, {r}]')
                gns.append(t)
        arr = (C.c_void_p * len(gns))(*[t.data_ptr() if t is not None else None for t in gns])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_synth_backward_noise(self._h, _lib.ptr(g_img), _lib.ptr(dws), arr, _lib.stream_ptr()),
                       'la_synth_backward_noise')
        return dws, gns

    # debugging / test taps -------------------------------------------------------------------
    def _view(self, p, shape):
        n = int(np.prod(shape))
        base = self._workspace.data_ptr()
        off = p - base
        assert 0 <= off and off + 4 * n <= self.workspace_bytes
        return self._workspace[off:off + 4 * n].view(torch.float32).reshape(shape)

    def layer_output(self, k, batch):
        r = self.layer_resolutions[k]
        block = self.block_resolutions.index(r)
        return self._view(self._lib.la_synth_layer_output(self._h, k), [batch, self.channels[block], r, r])

    def styles(self, batch):
        rows = self._lib.la_synth_style_rows(self._h)
        return self._view(self._lib.la_synth_styles(self._h), [batch, rows])

    def style_grads(self, batch):
        rows = self._lib.la_synth_style_rows(self._h)
        return self._view(self._lib.la_synth_style_grads(self._h), [batch, rows])


class _SynthesisFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ws, engine, noise_mode, noises):
        ctx.engine = engine
        ctx.ws_shape = ws.shape
        return engine.forward(ws, noise_mode=noise_mode, noises=noises)

    @staticmethod
    def backward(ctx, g_img):
        dws = ctx.engine.backward(g_img)
        shape = ctx.ws_shape
        if len(shape) == 2:
            dws = dws.sum(dim=1)
        elif shape[1] == 1:
            dws = dws.sum(dim=1, keepdim=True)
        return dws, None, None, None


class _SynthesisNoiseFn(torch.autograd.Function):
    """The same call with the explicit noise tensors as inputs of the function, so that those which require grad get theirs."""
    @staticmethod
    def forward(ctx, ws, engine, noise_mode, *noises):
        ctx.engine = engine
        ctx.ws_shape = ws.shape
        ctx.want = [t is not None and t.requires_grad for t in noises]
        return engine.forward(ws, noise_mode=noise_mode, noises=[None if t is None else t.detach() for t in noises])

    @staticmethod
    def backward(ctx, g_img):
        dws, gns = ctx.engine.backward(g_img, noise_grads=ctx.want)
        shape = ctx.ws_shape
        if len(shape) == 2:
            dws = dws.sum(dim=1)
        elif shape[1] == 1:
            dws = dws.sum(dim=1, keepdim=True)
        return (dws, None, None) + tuple(gns)


def synthesis(engine, ws, noise_mode='const', noises=None):
    """Differentiable call of the HIP synthesis engine, autograd-compatible: with respect to ws, and with respect to the entries of
    `noises` (noise_mode 'random') that require grad."""
    if noises is not None and any(t is not None and t.requires_grad for t in noises):
        return _SynthesisNoiseFn.apply(ws, engine, noise_mode, *noises)
    return _SynthesisFn.apply(ws, engine, noise_mode, noises)


class MappingEngine:
    """G.mapping(z, c=None, truncation_psi=psi) on the HIP path (reference call sites util_latent_aug.py:203,460).

    Built from the `mapping.*` entries of the generator state_dict (legacy.py:172-176)."""

    def __init__(self, G, device, lr_multiplier=0.01):
        self._lib = _lib.load()
        self.device = torch.device(device)
        sd = G if isinstance(G, dict) else G.state_dict()
        sd = {k[len('mapping.'):]: v for k, v in sd.items() if k.startswith('mapping.')}
        n = 0
        while f'fc{n}.weight' in sd:
            n += 1
        if n == 0:
            raise _lib.LatentAugHipError('generator has no mapping.fc* tensors: z input / rand_aug needs the mapping network')
        self.num_layers = n
        self.weights = [sd[f'fc{i}.weight'].detach().to(self.device, torch.float32).contiguous() for i in range(n)]
        self.biases = [sd[f'fc{i}.bias'].detach().to(self.device, torch.float32).contiguous() for i in range(n)]
        self.z_dim = int(self.weights[0].shape[1])
        self.w_dim = int(self.weights[-1].shape[0])
        self.w_avg = sd['w_avg'].detach().to(self.device, torch.float32).contiguous() if 'w_avg' in sd else None
        self.lr_multiplier = float(lr_multiplier)
        self._wp = (C.c_void_p * n)(*[t.data_ptr() for t in self.weights])
        self._bp = (C.c_void_p * n)(*[t.data_ptr() for t in self.biases])

    def forward(self, z, num_ws, truncation_psi=1.0):
        _lib.require_gpu(z)
        z = z.contiguous().float()
        B = z.shape[0]
        assert z.shape[1] == self.z_dim
        tmp = _lib.workspace(4 * 2 * B * max(self.z_dim, self.w_dim), self.device, torch.float32)
        ws = torch.empty([B, num_ws, self.w_dim], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_mapping_forward_f32(_lib.ptr(z), B, self.z_dim, self.w_dim, self.num_layers, self._wp,
                                                        self._bp, self.lr_multiplier, _lib.ptr(self.w_avg),
                                                        float(truncation_psi), num_ws, _lib.ptr(tmp), _lib.ptr(ws),
                                                        _lib.stream_ptr()), 'la_mapping_forward')
        return ws


class DiscriminatorEngine:
    """D(x, c=None) and d(loss_disc)/dx on the HIP path (reference calc_loss_disc, util_latent_aug.py:363-371).

    Built from the discriminator's state_dict (names of legacy.py:271-288: b{res}.{fromrgb,conv0,conv1,skip}.*,
    b4.{conv,fc,out}.*); architecture 'resnet', MinibatchStd group 4."""

    def __init__(self, D, device, max_batch, conv_clamp=256.0, precision='f32', mbstd_group_size=4):
        lib = _lib.load()
        self._lib = lib
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.LatentAugHipError('DiscriminatorEngine needs a ROCm device (no CPU fallback)')
        sd = D if isinstance(D, dict) else D.state_dict()
        res_list = sorted({int(k.split('.')[0][1:]) for k in sd if k.startswith('b') and k.split('.')[0][1:].isdigit()})
        assert res_list[0] == 4 and len(res_list) >= 2, 'expected discriminator blocks b4..bR'
        R = res_list[-1]
        self.img_resolution = R
        self.img_channels = int(sd[f'b{R}.fromrgb.weight'].shape[1])
        # channel table at resolution 4 << k: C[res] = in-channels of b{res}.conv0 ; C[4] = out-channels of b8.conv1
        ch = {r: int(sd[f'b{r}.conv0.weight'].shape[1]) for r in res_list if r > 4}
        ch[4] = int(sd['b4.conv.weight'].shape[0])
        self.channels = [ch[r] for r in res_list]
        self._keep = []

        def dev(name):
            t = sd[name].detach().to(device=self.device, dtype=torch.float32).contiguous()
            self._keep.append(t)
            return t

        params = []
        for r in reversed(res_list[1:]):
            if r == R:
                params += [dev(f'b{r}.fromrgb.weight'), dev(f'b{r}.fromrgb.bias')]
            params += [dev(f'b{r}.conv0.weight'), dev(f'b{r}.conv0.bias'), dev(f'b{r}.conv1.weight'), dev(f'b{r}.conv1.bias'),
                       dev(f'b{r}.skip.weight')]
        params += [dev('b4.conv.weight'), dev('b4.conv.bias'), dev('b4.fc.weight'), dev('b4.fc.bias'), dev('b4.out.weight'),
                   dev('b4.out.bias')]
        assert len(params) == lib.la_disc_num_params(R)
        f1 = np.array([1, 3, 3, 1], dtype=np.float32)
        self._fir = np.ascontiguousarray(np.outer(f1, f1) / 64.0, dtype=np.float32)
        chan = (C.c_int * len(self.channels))(*self.channels)
        self.max_batch = int(max_batch)
        nbytes = lib.la_disc_workspace_bytes(R, self.img_channels, chan, self.max_batch)
        assert nbytes > 0
        self._workspace = _lib.workspace(nbytes, self.device)
        pp = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        h = C.c_void_p()
        clamp = float(-1.0 if conv_clamp is None else conv_clamp)
        with torch.cuda.device(self.device):
            _lib.check(lib.la_disc_create(R, self.img_channels, chan, clamp, pp, len(params), self._fir.ctypes.data,
                                          int(mbstd_group_size), self.max_batch, _lib.ptr(self._workspace), nbytes,
                                          _lib.stream_ptr(), C.byref(h)), 'la_disc_create')
        self._h = h
        _lib.check(lib.la_disc_set_precision(h, PRECISIONS[precision]), 'la_disc_set_precision')

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.la_disc_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def forward(self, img):
        """img [B,C,R,R] -> logits [B,1]."""
        _lib.require_gpu(img)
        img = img.contiguous().float()
        B = img.shape[0]
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_disc_forward(self._h, _lib.ptr(img), B, _lib.stream_ptr()), 'la_disc_forward')
            p = self._lib.la_disc_logits(self._h)
            off = p - self._workspace.data_ptr()
            return self._workspace[off:off + 4 * B].view(torch.float32).clone().reshape(B, 1)

    def backward(self, dlogits):
        """d(loss)/d(logits) [B,1] -> d(loss)/d(img) for the last forward."""
        dl = dlogits.contiguous().float().reshape(-1)
        B = dl.shape[0]
        g = torch.empty([B, self.img_channels, self.img_resolution, self.img_resolution], device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_disc_backward(self._h, _lib.ptr(dl), _lib.ptr(g), 0, _lib.stream_ptr()), 'la_disc_backward')
        return g


FEAT_CONV, FEAT_TAP, FEAT_MAXPOOL, FEAT_AVGPOOL, FEAT_FC_RELU, FEAT_FC = 0, 1, 2, 3, 4, 5
FEAT_CONV_EX, FEAT_MAXPOOL3S2, FEAT_FIRE, FEAT_OP_ARGS = 6, 7, 8, 9
RESIZE_MODES = {'area': 0, 'bilinear': 1}


class FeatureEngine:
    """LPIPS-style feature net on the HIP path: `vgg16(x, resize_images=False, return_lpips=True)` of
    util_latent_aug.py:395 and its backward.  `ops` is a list of ('conv', weight, bias) | ('tap', lin) | ('maxpool',) |
    ('avgpool',) in execution order; see `vgg16_lpips_ops` for the VGG16 layout.  ('fc', weight [O, K], bias [O], relu: bool) is a
    fully connected layer on the flattened activation (K = C * res * res in torch's NCHW order); a list that ends in one is a detector
    list (`DetectorEngine`): forward only, no taps, and its feature vector is the last fc's output.
    General ops (`alexnet_lpips_ops`, `squeezenet_lpips_ops`): ('conv', weight, bias, stride, pad) is a convolution + ReLU with any square
    kernel up to 11, stride 1 | 2 | 4 and pad 0 .. 5 (the three-tuple form stays "3x3, pad 1, the existing launch"); ('maxpool3', ceil_mode)
    a 3x3 stride-2 max pool; ('fire', sq_w, sq_b, e1_w, e1_b, e3_w, e3_b) SqueezeNet's Fire module.  They compute in exact fp32 whatever
    `precision` says; a list the library refuses raises LatentAugHipError with the op's index."""

    def __init__(self, ops, device, in_res, max_batch, in_ch=3, precision='f32'):
        lib = _lib.load()
        self._lib = lib
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.LatentAugHipError('FeatureEngine needs a ROCm device (no CPU fallback)')
        self._keep = []
        desc, params = [], []
        c = in_ch

        def dev(t):
            return t.detach().to(self.device, torch.float32).contiguous()
        for op in ops:
            if op[0] == 'conv' and len(op) == 5:      # general conv: any square kernel, exact fp32 (la_feat_conv.hip)
                w, b = dev(op[1]), dev(op[2])
                assert w.ndim == 4 and w.shape[1] == c and w.shape[2] == w.shape[3] and b.shape == (w.shape[0],)
                desc += [_lib.FeatOp(FEAT_CONV_EX, c, w.shape[0]), _lib.FeatOp(FEAT_OP_ARGS, w.shape[2], int(op[3])), _lib.FeatOp(FEAT_OP_ARGS, int(op[4]), 0)]
                c = w.shape[0]
                params += [w, b]
            elif op[0] == 'maxpool3':
                desc += [_lib.FeatOp(FEAT_MAXPOOL3S2, c, c), _lib.FeatOp(FEAT_OP_ARGS, 1 if op[1] else 0, 0)]
            elif op[0] == 'fire':
                t = [dev(v) for v in op[1:7]]
                sq, e1, e3 = t[0].shape[0], t[2].shape[0], t[4].shape[0]
                assert t[0].shape == (sq, c, 1, 1) and t[2].shape == (e1, sq, 1, 1) and t[4].shape == (e3, sq, 3, 3)
                assert t[1].shape == (sq,) and t[3].shape == (e1,) and t[5].shape == (e3,)
                desc += [_lib.FeatOp(FEAT_FIRE, c, e1 + e3), _lib.FeatOp(FEAT_OP_ARGS, sq, e1), _lib.FeatOp(FEAT_OP_ARGS, e3, 0)]
                c = e1 + e3
                params += t
            elif op[0] == 'conv':
                w = op[1].detach().to(self.device, torch.float32).contiguous()
                b = op[2].detach().to(self.device, torch.float32).contiguous()
                assert w.shape[1] == c and w.shape[2:] == (3, 3)
                desc.append(_lib.FeatOp(FEAT_CONV, c, w.shape[0]))
                c = w.shape[0]
                params += [w, b]
            elif op[0] == 'tap':
                lin = op[1].detach().to(self.device, torch.float32).contiguous()
                assert lin.shape == (c,)
                desc.append(_lib.FeatOp(FEAT_TAP, c, c))
                params.append(lin)
            elif op[0] in ('maxpool', 'avgpool'):
                desc.append(_lib.FeatOp(FEAT_MAXPOOL if op[0] == 'maxpool' else FEAT_AVGPOOL, c, c))
            elif op[0] == 'fc':
                w = op[1].detach().to(self.device, torch.float32).contiguous()
                b = op[2].detach().to(self.device, torch.float32).contiguous()
                assert w.ndim == 2 and b.shape == (w.shape[0],)
                desc.append(_lib.FeatOp(FEAT_FC_RELU if op[3] else FEAT_FC, w.shape[1], w.shape[0]))      # (the engine checks K)
                c = w.shape[0]
                params += [w, b]
            else:
                raise ValueError(op[0])
        self._keep = params
        # short content hash of the weights (host side, once): identifies which feature net a cached bank was built with
        import hashlib
        hsh = hashlib.sha1()
        for op in ops:
            hsh.update(op[0].encode())
            for t in op[1:]:
                hsh.update(t.detach().to('cpu', torch.float32).contiguous().numpy().tobytes() if torch.is_tensor(t) else repr(t).encode())
        self.weights_digest = hsh.hexdigest()[:10]
        self.in_ch, self.in_res, self.max_batch = in_ch, in_res, int(max_batch)
        # (a general op is its record followed by its LA_FEAT_OP_ARGS records: include/latentaug_hip.h)
        general = any(d.kind == FEAT_OP_ARGS for d in desc)
        arr = (_lib.FeatOp * len(desc))(*desc)
        nbytes = lib.la_feat_workspace_bytes(len(desc), arr, in_ch, in_res, self.max_batch)
        if nbytes == 0 and general:
            raise _lib.LatentAugHipError('invalid feature-net description: ' + (lib.la_last_error() or b'?').decode())
        assert nbytes > 0, 'invalid feature-net description: ' + (lib.la_last_error() or b'?').decode()
        self._workspace = _lib.workspace(nbytes, self.device)
        pp = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.la_feat_create(len(desc), arr, pp, len(params), in_ch, in_res, self.max_batch,
                                          _lib.ptr(self._workspace), nbytes, _lib.stream_ptr(), C.byref(h)), 'la_feat_create')
        self._h = h
        self.num_features = lib.la_feat_num_features(h)
        self.num_taps = lib.la_feat_num_taps(h)      # columns of pair_distance (0: a detector list)
        _lib.check(lib.la_feat_set_precision(h, PRECISIONS[precision]), 'la_feat_set_precision')
        # the net's own input layer, x_k * pre_scale[k] + pre_shift[k] on the three repeated channels: applied by whoever feeds the
        # engine (the criterion's crop + repeat, metrics.compute_lpips); from_torchscript / from_net set it
        self.pre_scale, self.pre_shift = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)

    @classmethod
    def from_net(cls, net, device, in_res, max_batch, precision='f32'):
        """Engine for a described net (`lpips_reference_net`, a candidate of `vgg16_from_torchscript`): its op list, with its input
        affine kept as `engine.pre_scale` / `engine.pre_shift` (and, of a TorchScript candidate, `engine.lin_is_sqrt`)."""
        eng = cls(net.ops, device, in_res, max_batch, precision=precision)
        eng.pre_scale, eng.pre_shift = tuple(float(v) for v in net.pre_scale), tuple(float(v) for v in net.pre_shift)
        if getattr(net, 'source', None) is not None:
            eng.lin_is_sqrt = net.lin_is_sqrt
        return eng

    @classmethod
    def from_torchscript(cls, src, device, in_res, max_batch, precision='f32', probe_seed=0, rtol=2e-3):
        """Engine for a local TorchScript `vgg16.pt` (reference: util_latent_aug.py:35-43, call :394-395): the verified candidate of
        `verified_torchscript_net`, with its input affine (`engine.pre_scale`, `engine.pre_shift`) and `engine.lin_is_sqrt`."""
        c, eng = cls._verify_torchscript(src, device, in_res, max_batch, probe_seed, rtol)
        if precision != 'f32' or max_batch != eng.max_batch:      # (otherwise the engine the probe ran on is the one asked for)
            eng = cls(c.ops, device, in_res, max_batch=max_batch, precision=precision)
        eng.pre_scale, eng.pre_shift, eng.lin_is_sqrt = c.pre_scale, c.pre_shift, c.lin_is_sqrt
        return eng

    @classmethod
    def verified_torchscript_net(cls, src, device, in_res, probe_seed=0, rtol=2e-3):
        """The `ScriptedFeatureNet` of a local TorchScript `vgg16.pt` that reproduces the module's own output (`.ops`, `.pre_scale`,
        `.pre_shift`, `.lin_is_sqrt`): resolve once, then build as many engines from it as needed (`from_net`)."""
        return cls._verify_torchscript(src, device, in_res, 2, probe_seed, rtol)[0]

    @classmethod
    def _verify_torchscript(cls, src, device, in_res, max_batch, probe_seed, rtol):
        """Every candidate mapping of `vgg16_from_torchscript` is checked ONCE, at load time, against the module's own
        `module(x, resize_images=False, return_lpips=True)` on a small probe batch (the scripted module runs on the host for this
        check only; the criterion itself never calls it); the first one that agrees is kept -- (candidate, the f32 engine it was
        probed on) -- otherwise loading fails loudly."""
        cands = vgg16_from_torchscript(src)
        g = torch.Generator().manual_seed(probe_seed)
        probe = torch.rand([2, 1, in_res, in_res], generator=g).repeat(1, 3, 1, 1) * 255.0      # the 0..255 range the script is written for
        with torch.no_grad():
            try:
                want = cands[0].source(probe, resize_images=False, return_lpips=True)
            except (RuntimeError, TypeError):
                want = cands[0].source(probe)
        want = want.reshape(2, -1).to(torch.float32)
        errs = []
        for c in cands:
            eng = cls(c.ops, device, in_res, max_batch=max(max_batch, 2), precision='f32')
            if eng.num_features != want.shape[1]:
                errs.append(float('inf'))
                continue
            x = probe * torch.tensor(c.pre_scale).reshape(1, 3, 1, 1) + torch.tensor(c.pre_shift).reshape(1, 3, 1, 1)      # plumbing
            got = eng.forward(x.to(eng.device)).cpu()
            err = float((got - want).norm() / want.norm().clamp_min(1e-30))
            errs.append(err)
            if err <= rtol:
                return c, eng
            del eng
        raise _lib.LatentAugHipError('TorchScript feature net: no mapping of its tensors onto the VGG16-LPIPS op list reproduces the '
                                     f"module's own output (relative errors of the candidates: {errs}); refusing to guess")

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.la_feat_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def forward(self, x):
        _lib.require_gpu(x)
        x = x.contiguous().float()
        N = x.shape[0]
        assert x.shape[1:] == (self.in_ch, self.in_res, self.in_res)
        f = torch.empty([N, self.num_features], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_feat_forward(self._h, _lib.ptr(x), N, _lib.ptr(f), _lib.stream_ptr()), 'la_feat_forward')
        self._x = x
        return f

    def backward(self, gfeat):
        gfeat = gfeat.contiguous().float()
        gx = torch.empty_like(self._x)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_feat_backward(self._h, _lib.ptr(gfeat), _lib.ptr(gx), _lib.stream_ptr()), 'la_feat_backward')
        return gx

    def pair_rows(self):
        """Pairs one la_feat_pair_distance call takes: both images of a pair are rows of one batch, so max_batch // 2."""
        if self.num_taps < 1:
            raise _lib.LatentAugHipError('pair_distance: a detector list (fc ops) has no taps')
        if self.max_batch < 2:
            raise _lib.LatentAugHipError('pair_distance: both images of a pair go through one batch; the engine needs max_batch >= 2')
        return self.max_batch // 2

    def pair_distance_rows(self, xy, P, dist):
        """la_feat_pair_distance on a prepared batch: xy [2P, in_ch, in_res, in_res] float32 (rows p and p + P are a pair, 2P <=
        max_batch) -> dist [P, num_taps] float64, both on the device and contiguous."""
        nbytes = self._lib.la_feat_pair_workspace_bytes(self._h, P)
        if nbytes == 0:
            raise _lib.LatentAugHipError(f'pair_distance: {P} pairs refused (detector list, or 2 * pairs > max_batch = {self.max_batch})')
        ws = getattr(self, '_pair_ws', None)
        if ws is None or ws.numel() * 8 < nbytes:
            ws = self._pair_ws = _lib.workspace(nbytes, self.device, torch.float64)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_feat_pair_distance(self._h, _lib.ptr(xy), P, _lib.ptr(dist), _lib.ptr(ws), ws.numel() * 8,
                                                       _lib.stream_ptr()), 'la_feat_pair_distance')

    def style_scratch_bytes(self, P):
        """Bytes of scratch la_feat_style_distance needs for P pairs (0: a detector list, or 2 * P > max_batch)."""
        return int(self._lib.la_feat_style_scratch_bytes(self._h, P))

    def style_distance_rows(self, xy, P, style, content, scratch):
        """la_feat_style_distance on a prepared batch: xy [2P, in_ch, in_res, in_res] float32 (rows p and p + P are a pair, 2P <=
        max_batch) -> style, content [P, num_taps] float64: per tap, the Gram-matrix style distance and the content distance of the
        raw activations (`lin` is not read).  All on the device and contiguous; scratch: a float64 tensor of at least
        style_scratch_bytes(P) bytes, any contents.  A later backward() needs a new forward() first."""
        if self.style_scratch_bytes(P) == 0:
            raise _lib.LatentAugHipError(f'style_distance: {P} pairs refused (detector list, or 2 * pairs > max_batch = {self.max_batch})')
        with torch.cuda.device(self.device):
            _lib.check(self._lib.la_feat_style_distance(self._h, _lib.ptr(xy), P, _lib.ptr(style), _lib.ptr(content), _lib.ptr(scratch),
                                                        scratch.numel() * scratch.element_size(), _lib.stream_ptr()), 'la_feat_style_distance')

    def pair_distance(self, x, y):
        """LPIPS distance of x[p] and y[p] per tap: float64 [P, num_taps] on the device, dist[p, t] = mean over the tap's pixels of
        sum_c lin_c (fx rx - fy ry)^2 -- what squared L2 of forward(x)[p] - forward(y)[p] gives tap by tap, from one fused launch per tap
        and without the feature vectors (la_feat_pair_distance).  x, y: [P, in_ch, in_res, in_res] as forward() takes them; chunks of
        max_batch // 2 pairs.  Two calls give the same bits.  A later backward() needs a new forward() first."""
        _lib.require_gpu(x)
        _lib.require_gpu(y)
        chunk = self.pair_rows()
        want = (self.in_ch, self.in_res, self.in_res)
        if x.ndim != 4 or x.shape != y.shape or tuple(x.shape[1:]) != want or x.shape[0] < 1:
            raise ValueError(f'pair_distance: x and y must both be [P, {want[0]}, {want[1]}, {want[2]}]; got {tuple(x.shape)}, {tuple(y.shape)}')
        x, y = x.contiguous().float(), y.contiguous().float()
        P = x.shape[0]
        dist = torch.empty([P, self.num_taps], dtype=torch.float64, device=self.device)
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            self.pair_distance_rows(torch.cat([x[p0:p0 + n], y[p0:p0 + n]]), n, dist[p0:p0 + n])
        return dist


def vgg16_lpips_ops(state_dict, lins, taps=(0, 1, 2, 3, 4)):
    """Op list of the LPIPS VGG16 from torchvision-style names (`features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight/bias`,
    cf. augments/criteria/lpips/networks.py:87-97) and per-channel lin weights.  `taps` selects among the five places relu1_2, 2_2,
    3_3, 4_3, 5_3 (0 .. 4, ascending); `lins` holds one weight vector per selected tap, in that order.  The default is all five;
    taps=(2, 3, 4) with three lins is the reference's `target_layers = [16, 23, 30]` (networks.py:94).  The list ends at its last tap."""
    conv_ids = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    tap_after = {2: 0, 7: 1, 14: 2, 21: 3, 28: 4}
    pool_after = {2, 7, 14, 21}
    taps = [int(t) for t in taps]
    if not taps or taps != sorted(set(taps)) or taps[0] < 0 or taps[-1] > 4:
        raise ValueError(f'taps: ascending, distinct places out of 0 .. 4 (got {taps})')
    if len(lins) != len(taps):
        raise ValueError(f'{len(taps)} taps need {len(taps)} lin weight vectors (got {len(lins)})')
    ops = []
    for i in conv_ids:
        ops.append(('conv', state_dict[f'features.{i}.weight'], state_dict[f'features.{i}.bias']))
        if tap_after.get(i) in taps:
            ops.append(('tap', lins[taps.index(tap_after[i])]))
            if tap_after[i] == taps[-1]:
                break
        if i in pool_after:
            ops.append(('maxpool',))
    return ops


def alexnet_lpips_ops(state_dict, lins):
    """Op list of the LPIPS AlexNet from torchvision's names (`features.{0,3,6,8,10}.weight/bias`, networks.py:73-84): conv 11x11
    stride 4 pad 2, 3x3 stride-2 pool, conv 5x5 pad 2, pool, three 3x3 pad-1 convs; taps after the ReLUs at `features` indices 1, 4, 7,
    9, 11 with `lins[0..4]`.  The list ends at its last tap (the third pool is never run).  Every conv is a general op: exact fp32."""
    if len(lins) != 5:
        raise ValueError(f'5 taps need 5 lin weight vectors (got {len(lins)})')
    geom = {0: (4, 2), 3: (1, 2), 6: (1, 1), 8: (1, 1), 10: (1, 1)}
    ops = []
    for t, i in enumerate((0, 3, 6, 8, 10)):
        ops.append(('conv', state_dict[f'features.{i}.weight'], state_dict[f'features.{i}.bias'], *geom[i]))
        ops.append(('tap', lins[t]))
        if i in (0, 3):
            ops.append(('maxpool3', False))
    return ops


def squeezenet_lpips_ops(state_dict, lins):
    """Op list of the LPIPS SqueezeNet 1.1 from torchvision's names (networks.py:60-70): `features.0` a 3x3 stride-2 conv without
    padding, Fire modules at 3, 4, 6, 7, 9, 10, 11, 12 (`.squeeze` / `.expand1x1` / `.expand3x3`), ceil-mode 3x3 stride-2 pools at 2, 5, 8;
    seven taps -- after the first ReLU and after the Fire modules 4, 7, 9, 10, 11, 12 -- with `lins[0..6]`.  The list ends at its last tap."""
    if len(lins) != 7:
        raise ValueError(f'7 taps need 7 lin weight vectors (got {len(lins)})')
    tap_after = {1: 0, 4: 1, 7: 2, 9: 3, 10: 4, 11: 5, 12: 6}      # networks.py:70, target_layers [2, 5, 8, 10, 11, 12, 13] (1-based)
    ops = [('conv', state_dict['features.0.weight'], state_dict['features.0.bias'], 2, 0), ('tap', lins[0])]
    for i in range(2, 13):
        if i in (2, 5, 8):
            ops.append(('maxpool3', True))
        else:
            ops.append(('fire',) + tuple(state_dict[f'features.{i}.{part}.{kind}'] for part in ('squeeze', 'expand1x1', 'expand3x3')
                                         for kind in ('weight', 'bias')))
        if i in tap_after:
            ops.append(('tap', lins[tap_after[i]]))
    return ops


LPIPS_ZSCORE_MEAN, LPIPS_ZSCORE_STD = (-.030, -.088, -.188), (.458, .448, .450)      # networks.py:40-43, images in [-1, 1]


def lpips_reference_net(vgg_state_dict, lin_state_dict, net_type='vgg'):
    """The reference's non-TorchScript perceptual net, `augments/criteria/lpips/lpips.py::LPIPS(net_type)`, as a described net for
    `FeatureEngine.from_net`.  'vgg': VGG16 tapped after relu3_3 / 4_3 / 5_3 (networks.py:94), the z-score (x - mean_k) / std_k as input affine
    (networks.py:40-50), and the LAST three `lin{k}.model.1.weight` tensors of the LPIPS weight file (what utils.py:32-52 keeps of
    its five).  'alex' / 'squeeze': `alexnet_lpips_ops` / `squeezenet_lpips_ops` on the first argument (torchvision's alexnet /
    squeezenet1_1 state dict) with all five / seven lin tensors (utils.py:32-37 skips nothing when the counts match) and the same
    z-score.  Each argument is a state dict or the path of one, read with torch.load(weights_only=True).  A negative lin weight
    is refused: the criterion's tap emits sqrt(lin)."""
    import re
    if net_type not in ('vgg', 'alex', 'squeeze'):
        raise ValueError(f"net_type must be 'vgg', 'alex' or 'squeeze' (got {net_type!r})")

    def read(src, what):
        if isinstance(src, dict):
            return src
        if not os.path.isfile(src):
            raise FileNotFoundError(f'{what}: no such file: {src}')
        return torch.load(src, map_location='cpu', weights_only=True)
    trunk_name = {'vgg': 'VGG16', 'alex': 'AlexNet', 'squeeze': 'SqueezeNet 1.1'}[net_type]
    vgg, lin = read(vgg_state_dict, f'{trunk_name} weights'), read(lin_state_dict, 'LPIPS lin weights')
    found = sorted((int(m.group(1)), v) for k, v in lin.items() for m in [re.fullmatch(r'lin(\d+)\.model\.1\.weight', k)] if m)
    need = {'vgg': 3, 'alex': 5, 'squeeze': 7}[net_type]
    if len(found) < need if net_type == 'vgg' else len(found) != need:
        raise _lib.LatentAugHipError(f'LPIPS lin weights: found {len(found)} `lin<k>.model.1.weight` tensors, need '
                                     + ('at least 3' if net_type == 'vgg' else f'{need} for {net_type!r}'))
    lins = [v.detach().to('cpu', torch.float32).reshape(-1) for _, v in found[-need:]]
    if any(float(v.min()) < 0.0 for v in lins):
        raise _lib.LatentAugHipError('LPIPS lin weights: a negative channel weight (the criterion takes its square root); refusing')
    if net_type == 'vgg':
        ops = vgg16_lpips_ops(vgg, lins, taps=(2, 3, 4))
    else:
        ops = (alexnet_lpips_ops if net_type == 'alex' else squeezenet_lpips_ops)(vgg, lins)
    return ScriptedFeatureNet(ops, tuple(1.0 / s for s in LPIPS_ZSCORE_STD),
                              tuple(-m / s for m, s in zip(LPIPS_ZSCORE_MEAN, LPIPS_ZSCORE_STD)), False, None)


NST_CONTENT_TAP = 3      # networks.py:11, content_layers ['19']: the fourth of the five style taps


def vgg19_nst_ops(state_dict):
    """Op list of the reference's style / content net, `augments/criteria/nst/networks.py::VGG19Net`, from torchvision's names of
    vgg19 (`features.{0,2,5,7,10,12,14,16,19,21,23,25,28}.weight/bias`): 13 convs + ReLU, 4 max pools, taps after the convs 0, 5, 10,
    19 and 28.  networks.py:12 names conv indices, but torchvision's ReLUs are in place, so the tensors its list holds are the
    post-ReLU activations relu1_1 .. relu5_1: a tap behind the conv + ReLU op.  The list ends at conv 28.  Every tap carries
    lin = ones (the style distance does not read it), so `forward` and `pair_distance` of such an engine work too."""
    conv_ids = [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28]
    tap_after, pool_after = {0, 5, 10, 19, 28}, {2, 7, 16, 25}
    ops = []
    for i in conv_ids:
        w = state_dict[f'features.{i}.weight']
        ops.append(('conv', w, state_dict[f'features.{i}.bias']))
        if i in tap_after:
            ops.append(('tap', torch.ones([w.shape[0]], dtype=torch.float32)))
        if i in pool_after:
            ops.append(('maxpool',))
    return ops


def nst_reference_net(vgg19_state_dict):
    """The reference's `VGG19Net` (augments/criteria/nst/networks.py) as a described net for `FeatureEngine.from_net`:
    `vgg19_nst_ops` with the input layer of `prepare_img(synthetic=True, normalize=True)`, (x * 127.5 + 128) / 255 = x * 0.5 + 128 / 255
    on the three repeated channels (`standardize` is never passed: no ImageNet mean / std); its clamp(0, 255) is the caller's
    (metrics.compute_style_content clamps the images in front of the affine).  The argument is torchvision's vgg19 state dict or the
    path of a local file of one, read with torch.load(weights_only=True)."""
    sd = vgg19_state_dict
    if not isinstance(sd, dict):
        if not os.path.isfile(sd):
            raise FileNotFoundError(f'VGG19 weights: no such file: {sd}')
        sd = torch.load(sd, map_location='cpu', weights_only=True)
    return ScriptedFeatureNet(vgg19_nst_ops(sd), (0.5,) * 3, (128.0 / 255.0,) * 3, False, None)


# ------------------------------------------------------------------------------------------------------------
# A local copy of the reference's default perceptual net: NVIDIA's TorchScript `vgg16.pt` (util_latent_aug.py:35-43 loads it
# with torch.jit.load from a URL; :394-395 calls it as vgg16(x, resize_images=False, return_lpips=True)).
class ScriptedFeatureNet:
    """What `vgg16_from_torchscript` extracts: the FeatureEngine op list plus the module's own input layer as a per-channel
    affine (`pre_scale`, `pre_shift`: x_k * scale_k + shift_k on the three repeated channels)."""

    def __init__(self, ops, pre_scale, pre_shift, lin_is_sqrt, source):
        self.ops, self.pre_scale, self.pre_shift, self.lin_is_sqrt, self.source = ops, pre_scale, pre_shift, lin_is_sqrt, source


def _script_tensors(module):
    sd = module.state_dict()
    return [(k, v.detach().to('cpu', torch.float32)) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()]


def vgg16_from_torchscript(src, map_location='cpu'):
    """Parameter tensors of a TorchScript VGG16-LPIPS module -> candidate `ScriptedFeatureNet`s.

    `src`: path / file object for torch.jit.load, or an already loaded ScriptModule.  The archive holds no Python source we
    could read names from, so the layout is recognised from the tensors themselves, in state_dict order:
      * the 3x3 convolutions: every 4-D [Co, Ci, 3, 3] tensor (13 of them, Ci of the first = 3) with the [Co] vector that follows
        it (or `<name>.bias`);
      * the five LPIPS channel weights: tensors with exactly C = 64, 128, 256, 512, 512 x (width / 64) elements that are not biases;
      * the input layer: 3-element tensors named *mean* / *shift* and *std* / *scale*  ->  (x - mean_k) / std_k.
    Two things cannot be read from the tensors: whether the stored channel weights are the lin weights or their square roots, and
    whether an input layer without buffers is hard-coded in the script.  The function therefore returns the candidates (at most
    four) and `FeatureEngine.from_torchscript` keeps the one that reproduces the module's OWN output on a probe batch; if none
    does, loading fails -- a mapping is never trusted unverified."""
    module = src if isinstance(src, torch.jit.ScriptModule) else torch.jit.load(src, map_location=map_location)
    module = module.eval()
    items = _script_tensors(module)
    convs, used = [], set()
    for idx, (k, v) in enumerate(items):
        if v.ndim == 4 and v.shape[2:] == (3, 3):
            bias = None
            cand = k[:-len('weight')] + 'bias' if k.endswith('weight') else None
            for j, (kj, vj) in enumerate(items):
                if j in used or vj.ndim != 1 or vj.shape[0] != v.shape[0]:
                    continue
                if (cand is not None and kj == cand) or (cand is None and j == idx + 1):
                    bias, _ = vj, used.add(j)
                    break
            if bias is None and idx + 1 < len(items) and items[idx + 1][1].ndim == 1 and items[idx + 1][1].shape[0] == v.shape[0]:
                bias = items[idx + 1][1]
                used.add(idx + 1)
            if bias is None:
                bias = torch.zeros([v.shape[0]])
            used.add(idx)
            convs.append((v, bias))
    if len(convs) != 13 or convs[0][0].shape[1] != 3:
        raise _lib.LatentAugHipError(f'TorchScript feature net: expected the 13 3x3 convolutions of VGG16 (first one on 3 channels), found '
                                     f'{len(convs)}: not a vgg16.pt layout')
    tap_convs = [1, 3, 6, 9, 12]                      # relu1_2, 2_2, 3_3, 4_3, 5_3
    want = [convs[i][0].shape[0] for i in tap_convs]
    lins, k = [], 0
    for idx, (name, v) in enumerate(items):
        if idx in used or k >= 5 or name.endswith('bias'):
            continue
        if v.numel() == want[k] and max(v.shape) == want[k] and float(v.min()) >= 0.0:
            lins.append(v.reshape(-1))
            used.add(idx)
            k += 1
    if len(lins) != 5:
        raise _lib.LatentAugHipError(f'TorchScript feature net: found {len(lins)} of the 5 LPIPS channel-weight tensors {want}')
    mean = std = None
    for idx, (name, v) in enumerate(items):
        if idx in used or v.numel() != 3:
            continue
        low = name.lower()
        if mean is None and ('mean' in low or 'shift' in low):
            mean = v.reshape(3)
        elif std is None and ('std' in low or 'scale' in low):
            std = v.reshape(3)
    pres = [((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))]
    if mean is not None or std is not None:
        m = mean if mean is not None else torch.zeros(3)
        sd_ = std if std is not None else torch.ones(3)
        pres.insert(0, (tuple(float(1.0 / t) for t in sd_), tuple(float(-a / t) for a, t in zip(m, sd_))))
    out = []
    for pre_scale, pre_shift in pres:
        for lin_is_sqrt in (False, True):
            ops = []
            for i, (w, b) in enumerate(convs):
                ops.append(('conv', w, b))
                if i in tap_convs:
                    ln = lins[tap_convs.index(i)]
                    ops.append(('tap', ln.square() if lin_is_sqrt else ln))
                    if i != tap_convs[-1]:
                        ops.append(('maxpool',))
            out.append(ScriptedFeatureNet(ops, pre_scale, pre_shift, lin_is_sqrt, module))
    return out


# ------------------------------------------------------------------------------------------------------------
# Detector features: the `return_features=True` branch of the same scripted VGG16, which the reference's precision / recall calls on
# uint8 images (metrics/precision_recall.py:36-85, metrics/metric_utils.py:264-328).
def detector_prep(images, size, resize_mode='area', quantize=True, pre_scale=(1.0, 1.0, 1.0), pre_shift=(0.0, 0.0, 0.0)):
    """[N, 1|3, H, W] float32 device images -> the detector's input [N, 3, size, size] in one launch (la_detector_prep_f32): optional
    quantisation to the uint8 grid, bit for bit torch's `(x * 127.5 + 128).clamp(0, 255).to(torch.uint8)` of metric_utils.py:316; one
    channel repeated three times (:314-315); resampling with F.interpolate's 'area' or 'bilinear' (align_corners=False) rule; then
    the per-channel input affine v * pre_scale[k] + pre_shift[k]."""
    _lib.require_gpu(images)
    if images.ndim != 4 or images.shape[1] not in (1, 3):
        raise ValueError(f'images must be [N, 1|3, H, W], got {tuple(images.shape)}')
    if resize_mode not in RESIZE_MODES:
        raise ValueError(f'resize_mode must be one of {sorted(RESIZE_MODES)}')
    lib = _lib.load()
    x = images.detach().to(torch.float32).contiguous()
    N, Cc, H, W = x.shape
    out = torch.empty([N, 3, size, size], dtype=torch.float32, device=x.device)
    sc, sh = (C.c_float * 3)(*[float(v) for v in pre_scale]), (C.c_float * 3)(*[float(v) for v in pre_shift])
    if N:
        with torch.cuda.device(x.device):
            _lib.check(lib.la_detector_prep_f32(_lib.ptr(x), _lib.ptr(out), N, Cc, H, W, size, 3 // Cc, RESIZE_MODES[resize_mode],
                                                1 if quantize else 0, sc, sh, _lib.stream_ptr()), 'la_detector_prep_f32')
    return out


def fc_bias_act(x, weight, bias, relu=False):
    """act(x @ weight.T + bias) on the HIP path (la_fc_bias_act_f32): float32, exact fp32 products, the same bits on every run."""
    for t in (x, weight, bias):
        _lib.require_gpu(t)
    lib = _lib.load()
    x, weight, bias = (t.detach().to(torch.float32).contiguous() for t in (x, weight, bias))
    N, K = x.shape
    O = weight.shape[0]
    assert weight.shape == (O, K) and bias.shape == (O,)
    y = torch.empty([N, O], dtype=torch.float32, device=x.device)
    nbytes = lib.la_fc_workspace_bytes(N, K, O)
    if nbytes == 0:
        raise _lib.LatentAugHipError('la_fc_workspace_bytes refused the shape: ' + (lib.la_last_error() or b'?').decode())
    ws = _lib.workspace(nbytes, x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.la_fc_bias_act_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), N, K, O, 2 if relu else 1, _lib.ptr(ws),
                                          nbytes, _lib.stream_ptr()), 'la_fc_bias_act_f32')
    return y


class ScriptedDetectorNet:
    """One candidate reading of a scripted VGG16's `return_features=True` branch (`vgg16_detector_candidates`): the detector op list
    (13 convolutions, 5 max-pools, `fc_depth` fully connected layers with ReLU), the input affine, the net's input size and the resize
    rule."""

    def __init__(self, ops, pre_scale, pre_shift, size, resize_mode, fc_depth, source):
        self.ops, self.pre_scale, self.pre_shift, self.size = ops, pre_scale, pre_shift, size
        self.resize_mode, self.fc_depth, self.source = resize_mode, fc_depth, source


def vgg16_detector_candidates(src, map_location='cpu'):
    """Parameter tensors of a TorchScript VGG16 -> candidate `ScriptedDetectorNet`s (host only).  The 13 convolutions and the input
    layer are those `vgg16_from_torchscript` finds; the fully connected layers are the 2-D tensors with the [O] vector that follows
    each (or `<name>.bias`), in state_dict order; the input size S follows from fc1's width, K1 = C5 * (S / 32)^2.  What the tensors
    cannot tell -- the resize rule ('area' | 'bilinear') and whether `return_features=True` returns the activation after fc1 + ReLU
    or after fc2 + ReLU -- is enumerated (together with the input-affine candidates of the LPIPS loader);
    `DetectorEngine.from_torchscript` keeps the candidate that reproduces the module's own output."""
    lp = vgg16_from_torchscript(src, map_location=map_location)
    module = lp[0].source
    items = _script_tensors(module)
    fcs = []
    for idx, (k, v) in enumerate(items):
        if v.ndim != 2 or min(v.shape) < 2:
            continue
        bias = None
        want = k[:-len('weight')] + 'bias' if k.endswith('weight') else None
        for j, (kj, vj) in enumerate(items):
            if vj.ndim == 1 and vj.shape[0] == v.shape[0] and ((want is not None and kj == want) or (want is None and j == idx + 1)):
                bias = vj
                break
        if bias is None and idx + 1 < len(items) and items[idx + 1][1].ndim == 1 and items[idx + 1][1].shape[0] == v.shape[0]:
            bias = items[idx + 1][1]
        fcs.append((v, bias if bias is not None else torch.zeros([v.shape[0]])))
    if len(fcs) < 2 or fcs[1][0].shape[1] != fcs[0][0].shape[0]:
        raise _lib.LatentAugHipError(f'TorchScript detector: expected at least two chained fully connected layers, found '
                                     f'{[tuple(w.shape) for w, _ in fcs]}: not a vgg16.pt layout')
    convs = [op for op in lp[0].ops if op[0] == 'conv']
    c5, k1 = convs[-1][1].shape[0], fcs[0][0].shape[1]
    side = math.isqrt(k1 // c5) if k1 % c5 == 0 else 0
    if side < 1 or side * side * c5 != k1:
        raise _lib.LatentAugHipError(f'TorchScript detector: fc1 takes {k1} inputs, which is not {c5} x a square: not a vgg16.pt layout')
    size = 32 * side
    out, seen = [], set()
    for cand in lp:
        if (cand.pre_scale, cand.pre_shift) in seen:
            continue
        seen.add((cand.pre_scale, cand.pre_shift))
        trunk = [op for op in cand.ops if op[0] != 'tap'] + [('maxpool',)]          # the LPIPS list stops before the fifth pool
        for depth in (2, 1):
            ops = trunk + [('fc', w, b, True) for w, b in fcs[:depth]]
            for mode in ('area', 'bilinear'):
                out.append(ScriptedDetectorNet(ops, cand.pre_scale, cand.pre_shift, size, mode, depth, module))
    return out


def detector_probe(size, n=2, seed=0):
    """The probe batch of the load-time check: uint8-valued images with three different channels and a side that is no multiple of
    the net's input size (so the resize rule shows)."""
    g = torch.Generator().manual_seed(seed)
    side = size + size // 2 + 3
    return torch.randint(0, 256, [n, 3, side, side], generator=g).to(torch.float32)


def run_scripted_detector(module, images_u8):
    """`module(x, return_features=True)` as the reference calls it (uint8 images, metric_utils.py:316-318); on the host."""
    with torch.no_grad():
        try:
            out = module(images_u8.to(torch.uint8), return_features=True)
        except (RuntimeError, TypeError):
            out = module(images_u8.to(torch.float32), return_features=True)
    return out.reshape(images_u8.shape[0], -1).to(torch.float32)


class DetectorEngine:
    """Images -> detector features on the HIP path: `detector(x, return_features=True)` of metrics/metric_utils.py:318 with the
    quantisation and channel repeat of :314-316 in front.  A thin class over a detector-list `FeatureEngine` (13 convolutions on the
    contraction engine in `precision`, 5 max-pools, the fully connected layers in exact fp32) plus the image preparation kernel.
    There is no CPU fallback."""

    def __init__(self, ops, device, size, max_batch, resize_mode='area', pre_scale=(1.0, 1.0, 1.0), pre_shift=(0.0, 0.0, 0.0),
                 precision='f32'):
        if resize_mode not in RESIZE_MODES:
            raise ValueError(f'resize_mode must be one of {sorted(RESIZE_MODES)}')
        if not ops or ops[-1][0] != 'fc':
            raise ValueError('a detector op list ends in an fc op')
        self.engine = FeatureEngine(ops, device, in_res=size, max_batch=max_batch, in_ch=3, precision=precision)
        self.device, self.max_batch = self.engine.device, self.engine.max_batch
        self.S, self.resize_mode = int(size), resize_mode
        self.pre_scale, self.pre_shift = tuple(float(v) for v in pre_scale), tuple(float(v) for v in pre_shift)
        self.num_features = self.engine.num_features
        self.weights_digest = self.engine.weights_digest
        self.fc_depth = sum(1 for op in ops if op[0] == 'fc')

    @classmethod
    def from_torchscript(cls, src, device, max_batch, precision='f32', rtol=2e-3, probe_seed=0):
        """Engine for a local TorchScript `vgg16.pt`, the file the LPIPS criterion already needs.  Every candidate of
        `vgg16_detector_candidates` is run once, in exact fp32, on a probe batch and compared with the module's own
        `module(x, return_features=True)` (the scripted module runs on the host for this check only); the first one within relative
        L2 `rtol` is kept, otherwise loading fails with the candidates' errors -- a mapping is never trusted unverified."""
        cands = vgg16_detector_candidates(src)
        probe = detector_probe(cands[0].size, seed=probe_seed)
        want = run_scripted_detector(cands[0].source, probe)
        errs, engines = [], {}
        for c in cands:
            key = (c.pre_scale, c.pre_shift, c.fc_depth)
            if key not in engines:          # (the two resize rules of one reading share the engine and its uploaded weights)
                engines.clear()
                engines[key] = cls(c.ops, device, c.size, max(max_batch, probe.shape[0]), 'area', c.pre_scale, c.pre_shift, 'f32')
            det = engines[key]
            det.resize_mode = c.resize_mode
            if det.num_features != want.shape[1]:
                errs.append((c.resize_mode, c.fc_depth, float('inf')))
                continue
            got = det.features(probe.to(det.device), quantize=False).cpu()
            err = float((got - want).norm() / want.norm().clamp_min(1e-30))
            errs.append((c.resize_mode, c.fc_depth, err))
            if err <= rtol:
                if precision != 'f32' or max_batch != det.max_batch:
                    engines.clear()
                    del det
                    det = cls(c.ops, device, c.size, max_batch, c.resize_mode, c.pre_scale, c.pre_shift, precision)
                return det
        raise _lib.LatentAugHipError('TorchScript detector: no reading of its tensors (resize rule, fully connected depth, relative error: '
                                     f"{errs}) reproduces the module's own return_features output; refusing to guess")

    def prepare(self, images, quantize=True):
        return detector_prep(images, self.S, self.resize_mode, quantize, self.pre_scale, self.pre_shift)

    def features(self, images, quantize=True):
        """[N, 1|3, H, W] device images in the generator's [-1, 1] range (quantize=True: rounded to the uint8 grid as the reference
        does before the detector), or already on the 0..255 scale (quantize=False) -> [N, num_features] float32, in chunks of
        `max_batch`."""
        _lib.require_gpu(images)
        out = torch.empty([images.shape[0], self.num_features], dtype=torch.float32, device=self.device)
        for i in range(0, images.shape[0], self.max_batch):
            out[i:i + self.max_batch] = self.engine.forward(self.prepare(images[i:i + self.max_batch].to(self.device), quantize))
        return out
