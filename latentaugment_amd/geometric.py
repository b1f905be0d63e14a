"""Host side of the geometric warps (csrc/la_geom.hip; include/latentaug_hip.h 'GeometricAugment'): the taps of the elastic blur, the
random parameters of a batch, the float64 build and inversion of the affine map, and the launch wrappers.  Plumbing only: every pixel is
computed by the HIP kernels, host tensors are refused (LatentAugHipError) and nothing falls back to PyTorch.

Conventions: float32 NCHW, x the column index, y the row index, pixel centres at integer coordinates.  The forward map of a sample is
an optional flip x -> W - 1 - x, then a rotation by `angle` degrees about ((W - 1) / 2, (H - 1) / 2) with OpenCV's sign convention
(getRotationMatrix2D: [[c, s, .], [-s, c, .]], a positive angle turns the picture counter-clockwise on the screen), then a translation by
(tx, ty) pixels; the kernels take its inverse.
"""
import ctypes as C
import math

import torch

from . import _lib

PADDING_MODES = {'zeros': 0, 'border': 1, 'reflection': 2}
MAX_TAPS = 63
ELASTIC_KSIZE, ELASTIC_SIGMA, ELASTIC_ALPHA = 63, 32.0, 1.0      # kornia's elastic_transform2d defaults


def gaussian_taps(ksize, sigma):
    """Normalised Gaussian of odd length `ksize`: exp(-(i - (ksize - 1) / 2)^2 / (2 sigma^2)) / sum, float64 [ksize]."""
    if ksize < 1 or ksize % 2 == 0 or not sigma > 0:
        raise ValueError(f'gaussian_taps: ksize must be odd and positive and sigma positive, got {ksize}, {sigma}')
    i = torch.arange(ksize, dtype=torch.float64) - (ksize - 1) / 2
    t = torch.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return t / t.sum()


def draw_params(gen, B, H, W, p, flip=True, affine=True, elastic=True, rotate_limit=3.0, shift_limit=0.05):
    """Parameters of one batch, drawn on the CPU from `gen` (a torch.Generator, or None for torch's global CPU generator):
    flags 'flip', 'affine', 'elastic' [B] bool -- a stage that is switched on applies to a sample with probability p, independently per
    stage and sample; 'angle' [B] degrees in [-rotate_limit, rotate_limit); 'tx', 'ty' [B] pixels in [-shift_limit W, shift_limit W)
    and [-shift_limit H, shift_limit H); 'seed' a 0-dim int64 for the elastic noise.  Every number is drawn whether its stage is on or
    not, so switching a stage does not move the others' draws."""
    u = torch.rand([6, B], generator=gen, dtype=torch.float64)
    seed = torch.randint(0, 2 ** 62, [], generator=gen, dtype=torch.int64)
    on = lambda row, enabled: (u[row] < p) & bool(enabled)      # noqa: E731
    return {'flip': on(0, flip), 'affine': on(1, affine), 'elastic': on(2, elastic),
            'angle': (2 * u[3] - 1) * float(rotate_limit),
            'tx': (2 * u[4] - 1) * float(shift_limit) * W, 'ty': (2 * u[5] - 1) * float(shift_limit) * H, 'seed': seed}


def affine_forward(params, H, W):
    """The forward maps of a batch as float64 [B, 3, 3] (homogeneous pixel coordinates): translation . rotation . flip, each factor the
    identity for a sample whose flag is off."""
    B = params['flip'].shape[0]
    eye = torch.eye(3, dtype=torch.float64).expand(B, 3, 3)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    flip = eye.clone()
    flip[:, 0, 0], flip[:, 0, 2] = -1.0, W - 1.0
    flip = torch.where(params['flip'].view(B, 1, 1), flip, eye)
    rad = params['angle'].double() * (math.pi / 180.0)
    c, s = rad.cos(), rad.sin()
    rot = eye.clone()
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 0, 2] = c, s, (1 - c) * cx - s * cy
    rot[:, 1, 0], rot[:, 1, 1], rot[:, 1, 2] = -s, c, s * cx + (1 - c) * cy
    shift = eye.clone()
    shift[:, 0, 2], shift[:, 1, 2] = params['tx'].double(), params['ty'].double()
    aff = torch.where(params['affine'].view(B, 1, 1), shift @ rot, eye)
    return aff @ flip


def affine_inverse(params, H, W):
    """[B, 6] float32 (CPU): the first two rows of the inverse of affine_forward, built and inverted in float64 and rounded once."""
    inv = torch.linalg.inv(affine_forward(params, H, W))
    return inv[:, :2, :].reshape(-1, 6).to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------ launches
def _mode(padding_mode):
    if padding_mode not in PADDING_MODES:
        raise _lib.LatentAugHipError(f'padding_mode must be one of {sorted(PADDING_MODES)}, got {padding_mode!r}')
    return PADDING_MODES[padding_mode]


def _image(x, what):
    if not isinstance(x, torch.Tensor) or x.ndim != 4 or not x.dtype.is_floating_point:
        raise _lib.LatentAugHipError(f'{what}: a floating-point [B, C, H, W] tensor is needed')
    _lib.require_gpu(x)
    return x.detach().to(torch.float32).contiguous()


def _flags(apply, B, device):
    _lib.require_gpu(apply)
    if apply.numel() != B:
        raise _lib.LatentAugHipError(f'apply must have one entry per sample ({B}), got {tuple(apply.shape)}')
    if apply.dtype in (torch.uint8, torch.bool) and apply.device == device and apply.is_contiguous():
        return apply.view(torch.uint8)      # (bytes already: no launch)
    return (apply != 0).to(device=device, dtype=torch.uint8).contiguous()


def noise_uniform(rows, row_elems, seed, stream_id=0, row0=0, device=None):
    """[rows, row_elems] float32 on `device`, uniform in (-1, 1): element e of global row row0 + r is a pure function of
    (seed, stream_id, row0 + r, e), so shards that split the rows agree with the whole (la_noise_uniform_f32)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise _lib.LatentAugHipError('latentaugment_amd needs a ROCm device (no CPU fallback); got ' + str(device))
    with torch.cuda.device(device):
        out = torch.empty([rows, row_elems], device=device, dtype=torch.float32)
        _lib.check(_lib.load().la_noise_uniform_f32(_lib.ptr(out), rows, row_elems, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id), int(row0),
                                                    _lib.stream_ptr()), 'la_noise_uniform_f32')
    return out


def elastic_field(noise, taps, alpha=(ELASTIC_ALPHA, ELASTIC_ALPHA)):
    """noise [B, 2, H, W] -> displacement [B, 2, H, W]: both planes filtered with the separable odd-length kernel `taps` (at most 63,
    zero border), plane 0 times alpha[0] (x), plane 1 times alpha[1] (y) (la_elastic_field_f32)."""
    n = _image(noise, 'elastic_field')
    if n.shape[1] != 2:
        raise _lib.LatentAugHipError(f'elastic_field: noise must be [B, 2, H, W], got {tuple(noise.shape)}')
    taps = [float(t) for t in (taps.tolist() if isinstance(taps, torch.Tensor) else taps)]
    B, _, H, W = n.shape
    with torch.cuda.device(n.device):
        disp = torch.empty_like(n)
        _lib.check(_lib.load().la_elastic_field_f32(_lib.ptr(n), (C.c_float * max(len(taps), 1))(*taps), len(taps), float(alpha[0]), float(alpha[1]),
                                                    _lib.ptr(disp), None, B, H, W, _lib.stream_ptr()), 'la_elastic_field_f32')
    return disp if noise.dtype == torch.float32 else disp.to(noise.dtype)


def _warp(entry, x, par, apply, padding_mode):
    mode = _mode(padding_mode)
    xin = _image(x, entry)
    _lib.require_gpu(par)
    B, Cn, H, W = xin.shape
    par = par.detach().to(device=xin.device, dtype=torch.float32).contiguous()
    flags = _flags(apply, B, xin.device)
    with torch.cuda.device(xin.device):
        y = torch.empty_like(xin)
        _lib.check(getattr(_lib.load(), entry)(_lib.ptr(xin), _lib.ptr(par), _lib.ptr(flags), _lib.ptr(y), B, Cn, H, W, mode, _lib.stream_ptr()), entry)
    return y if x.dtype == torch.float32 else y.to(x.dtype)


def warp_affine(x, minv, apply, padding_mode='reflection'):
    """out[b, c, y, x] = S(in[b, c], Minv[b] (x, y, 1)) for samples with apply[b] != 0, a bit-for-bit copy otherwise.  x [B, C, H, W];
    minv [B, 6] (or [B, 2, 3]) on the device, the inverse map in pixel coordinates (affine_inverse); apply [B] on the device.
    float32 kernels: other floating dtypes are computed in float32 and cast back (la_warp_affine_f32)."""
    if minv.numel() != 6 * x.shape[0]:
        raise _lib.LatentAugHipError(f'warp_affine: minv must be [B, 6], got {tuple(minv.shape)}')
    return _warp('la_warp_affine_f32', x, minv, apply, padding_mode)


def warp_elastic(x, disp, apply, padding_mode='reflection'):
    """out[b, c, y, x] = S(in[b, c], px, py) with g = clamp(-1 + 2 x / (W - 1) + disp[b, 0, y, x], -1, 1) (0 along a one-pixel axis),
    px = ((g + 1) W - 1) / 2, and py likewise from plane 1 and H; apply as in warp_affine.  disp [B, 2, H, W] on the device
    (elastic_field) (la_warp_elastic_f32)."""
    if tuple(disp.shape) != (x.shape[0], 2) + tuple(x.shape[2:]):
        raise _lib.LatentAugHipError(f'warp_elastic: disp must be [B, 2, H, W] of the image, got {tuple(disp.shape)}')
    return _warp('la_warp_elastic_f32', x, disp, apply, padding_mode)
