"""Host-side mirror of the reference op layer (models/stylegan3/torch_utils/ops/) over the HIP C ABI.

Same names, argument meaning and error behaviour as the reference's Python wrappers:
  bias_act(x, b, dim, act, alpha, gain, clamp)                      bias_act.py:52-86
  setup_filter / upfirdn2d / filter2d / upsample2d / downsample2d   upfirdn2d.py:70-387
  filtered_lrelu(x, fu, fd, b, up, down, padding, gain, slope, clamp, flip_filter)   filtered_lrelu.py:59-108
  conv2d / conv_transpose2d(x, w, stride, padding, groups)          conv2d_gradfix.py:24-33
  conv2d_resample(x, w, f, up, down, padding, groups, flip_weight, flip_filter)       conv2d_resample.py:46-141
  grid_sample(input, grid)                                          grid_sample_gradfix.py:28-31
  fma(a, b, c)                                                      fma.py:15
Each op is a torch.autograd.Function whose forward AND backward are HIP launches (bias_act: every activation of the reference's
table with first- and second-order gradients; upfirdn2d: linear, its backward is the same op on the adjoint arguments, so gradients of
every order; filtered_lrelu: one
fused launch whose backward is the same kernel reading the sign mask its forward wrote, so gradients of every order; conv2d /
conv_transpose2d: forward, data gradient and weight gradient are three bilinear maps that are each other's backward, so gradients of
every order with respect to x, w and incoming gradients; float32 only; grid_sample: forward and a one-launch backward for input and
grid, the backward's own backward being the forward again, so gradients of every order between input and output; fma: one launch, its
gradients the same launch and a fixed-order un-broadcast sum).  torch only owns the device memory and the stream.

Dtypes of bias_act and the upfirdn2d family (upfirdn2d, filter2d, upsample2d, downsample2d), as the reference's plugins dispatch them
(bias_act.cpp:77, upfirdn2d.cpp:63): float16, float32 and float64 run on kernels of their own and return their own dtype (float16 with
fp32 arithmetic inside, float64 in double throughout).  Any other dtype (bfloat16, ...) is computed in float32 and returned as float32.
A float16 or float64 x needs a bias of its own dtype (bias_act.cpp:36).  filtered_lrelu is float32 only.  grid_sample has float16 /
float32 / float64 kernels too; fma has a float32 kernel, other float dtypes are computed in float32 and cast back to their own dtype.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

# activation table of the reference (bias_act.py:20-30): name -> (plugin id, default alpha, default gain, what the backward is formed from,
# whether a second derivative exists)
_ACTS = {
    'linear': (1, 0.0, 1.0, '', False), 'relu': (2, 0.0, math.sqrt(2.0), 'y', False), 'lrelu': (3, 0.2, math.sqrt(2.0), 'y', False),
    'tanh': (4, 0.0, 1.0, 'y', True), 'sigmoid': (5, 0.0, 1.0, 'y', True), 'elu': (6, 0.0, 1.0, 'y', True), 'selu': (7, 0.0, 1.0, 'y', True),
    'softplus': (8, 0.0, 1.0, 'y', True), 'swish': (9, 0.0, math.sqrt(2.0), 'x', True),
}


# dtypes of the C ABI's entries (suffix of la_bias_act_ex_* / la_bias_sum_* / la_upfirdn2d_*); they keep their dtype through the op
_DTYPES = {torch.float16: 'f16', torch.float32: 'f32', torch.float64: 'f64'}


def _op_input(x):
    """x as the op's kernels read it: float16 / float32 / float64 as they are, every other dtype converted to float32."""
    return x.contiguous() if x.dtype in _DTYPES else x.contiguous().float()


def _bias_act_launch(x, b, xref, yref, dy, grad, stepb, nb, act, alpha, gain, clamp):
    """One launch of the general op (include/latentaug_hip.h: la_bias_act_ex_f32 = the plugin's bias_act(x, b, xref, yref, dy, grad, ...),
    or its _f16 / _f64 form)."""
    fn = getattr(_lib.load(), 'la_bias_act_ex_' + _DTYPES[x.dtype])
    out = torch.empty_like(x)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(b), _lib.ptr(xref), _lib.ptr(yref), _lib.ptr(dy), _lib.ptr(out), x.numel(), stepb, nb, grad, act,
                  alpha, gain, clamp, _lib.stream_ptr()), 'bias_act')
    return out


class _BiasSum(torch.autograd.Function):
    """db = dx summed over every axis but the bias axis (bias_act.py:187,206), as a launch; its own gradient is a broadcast view."""

    @staticmethod
    def forward(ctx, dx, stepb, nb):
        dx = dx.contiguous()
        db = torch.empty([nb], device=dx.device, dtype=dx.dtype)
        fn = getattr(_lib.load(), 'la_bias_sum_' + _DTYPES[dx.dtype])
        if dx.numel():
            _lib.check(fn(_lib.ptr(dx), _lib.ptr(db), dx.numel(), stepb, nb, _lib.stream_ptr()), 'bias_sum')
        else:
            db.zero_()
        ctx.meta = (tuple(dx.shape), stepb, nb)
        return db

    @staticmethod
    def backward(ctx, d_db):
        shape, stepb, nb = ctx.meta
        lead = int(np.prod(shape)) // (stepb * nb) if stepb * nb else 0
        return d_db.reshape(1, nb, 1).expand(lead, nb, stepb).reshape(shape), None, None


class _BiasAct(torch.autograd.Function):
    """Forward of the op; first- and second-order gradients as HIP launches too (the reference: bias_act.py:130-210)."""

    @staticmethod
    def forward(ctx, x, b, dim, act, alpha, gain, clamp, ref, has2):
        _lib.require_gpu(x)
        x = _op_input(x)
        stepb, nb = 1, 1
        if b is not None:
            assert b.ndim == 1 and 0 <= dim < x.ndim and b.shape[0] == x.shape[dim]
            if x.dtype != torch.float32 and b.dtype != x.dtype:
                raise _lib.LatentAugHipError(f'bias_act: b must have the dtype of x ({x.dtype}), got {b.dtype}')
            b = b.contiguous().to(x.dtype)      # (a float32 x converts its bias, as it always has)
            nb = x.shape[dim]
            stepb = int(np.prod(x.shape[dim + 1:])) if dim + 1 < x.ndim else 1
        y = _bias_act_launch(x, b, None, None, None, 0, stepb, nb, act, alpha, gain, clamp)
        # (y is also kept for 'linear' when a clamp is set: the reference's CPU path -- `impl='ref'`, the parity target -- masks the gradient
        #  where the clamp is active for every activation; its CUDA plugin, which saves no y for 'linear', does not)
        ctx.save_for_backward(x if (ref == 'x' or has2) else None, b if (ref == 'x' or has2) else None,
                              y if (ref == 'y' or has2 or clamp >= 0) else None)
        ctx.meta = (stepb, nb, act, alpha, gain, clamp, b is not None, has2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, b, y = ctx.saved_tensors
        stepb, nb, act, alpha, gain, clamp, has_b, has2 = ctx.meta
        dx = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dx = _BiasActGrad.apply(dy.contiguous(), x, b, y, ctx.meta)
        if ctx.needs_input_grad[1] and has_b:
            db = _BiasSum.apply(dx, stepb, nb)
        return dx, db, None, None, None, None, None, None, None


class _BiasActGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, x, b, y, meta):
        stepb, nb, act, alpha, gain, clamp, has_b, has2 = meta
        dx = _bias_act_launch(dy, b, x, y, None, 1, stepb, nb, act, alpha, gain, clamp)
        ctx.save_for_backward(dy if has2 else None, x, b, y)
        ctx.meta = meta
        return dx

    @staticmethod
    def backward(ctx, d_dx):
        dy, x, b, y = ctx.saved_tensors
        stepb, nb, act, alpha, gain, clamp, has_b, has2 = ctx.meta
        d_dx = d_dx.contiguous()
        d_dy = d_x = d_b = None
        if ctx.needs_input_grad[0]:
            d_dy = _BiasActGrad.apply(d_dx, x, b, y, ctx.meta)
        if has2 and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            d_x = _bias_act_launch(d_dx, b, x, y, dy, 2, stepb, nb, act, alpha, gain, clamp)
            if has_b and ctx.needs_input_grad[2]:
                d_b = _BiasSum.apply(d_x, stepb, nb)
        return d_dy, d_x, d_b, None, None


def bias_act(x, b=None, dim=1, act='linear', alpha=None, gain=None, clamp=None, impl='hip'):
    """Fused bias + activation + gain + clamp (reference: bias_act.py:52-86); every activation of the reference's table, first- and
    second-order gradients.  float16 / float64 x (with b of the same dtype) returns its own dtype; float32 likewise; any other dtype
    is computed and returned in float32."""
    assert isinstance(x, torch.Tensor)
    assert clamp is None or clamp >= 0
    if act not in _ACTS:
        raise KeyError(act)      # (the reference indexes its activation table the same way)
    idx, def_alpha, def_gain, ref, has2 = _ACTS[act]
    alpha = float(def_alpha if alpha is None else alpha)
    gain = float(def_gain if gain is None else gain)
    clamp = float(-1 if clamp is None else clamp)
    return _BiasAct.apply(x, b, dim, idx, alpha, gain, clamp, ref, has2)


def setup_filter(f, device=torch.device('cpu'), normalize=True, flip_filter=False, gain=1, separable=None):
    """FIR taps for upfirdn2d (reference: upfirdn2d.py:70-114).  Always returned on the HOST: the HIP kernels take
    the (<= 8x8) taps as launch arguments."""
    if f is None:
        f = 1
    f = torch.as_tensor(f, dtype=torch.float32)
    assert f.ndim in [0, 1, 2] and f.numel() > 0
    if f.ndim == 0:
        f = f[None]
    if separable is None:
        separable = (f.ndim == 1 and f.numel() >= 8)
    if f.ndim == 1 and not separable:
        f = torch.outer(f, f)
    if separable:
        assert f.ndim == 1      # (kept 1-D: upfirdn2d then runs one pass per axis, upfirdn2d.py:188-201)
        if f.numel() > 32:
            raise NotImplementedError('separable filters of more than 32 taps')
    if normalize:
        f = f / f.sum()
    if flip_filter:
        f = f.flip(list(range(f.ndim)))
    return (f * (gain ** (f.ndim / 2))).cpu()


def _parse_scaling(s):
    if isinstance(s, int):
        return s, s
    sx, sy = s
    return int(sx), int(sy)


def _parse_padding(p):
    if isinstance(p, int):
        p = [p, p]
    p = list(p)
    if len(p) == 2:
        p = [p[0], p[0], p[1], p[1]]
    assert len(p) == 4
    return [int(v) for v in p]


def _launch_upfirdn2d(x, f, upx, upy, dnx, dny, px0, px1, py0, py1, flip, gain):
    lib = _lib.load()
    n, c, h, w = x.shape
    fh, fw = f.shape
    ow = lib.la_upfirdn2d_out_size(w, upx, dnx, px0, px1, fw)
    oh = lib.la_upfirdn2d_out_size(h, upy, dny, py0, py1, fh)
    assert ow >= 1 and oh >= 1
    fh_ = np.ascontiguousarray(f.numpy(), dtype=np.float32)
    y = torch.empty([n, c, oh, ow], device=x.device, dtype=x.dtype)
    fn = getattr(lib, 'la_upfirdn2d_' + _DTYPES[x.dtype])
    _lib.check(fn(_lib.ptr(x), fh_.ctypes.data, _lib.ptr(y), n, c, h, w, fh, fw, upx, upy, dnx, dny, px0, px1, py0, py1, int(flip), float(gain),
                  _lib.stream_ptr()), 'upfirdn2d')
    return y


class _Upfirdn2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f, up, down, padding, flip_filter, gain):
        _lib.require_gpu(x)
        x = _op_input(x)
        ctx.meta = (f, up, down, padding, flip_filter, gain, x.shape)
        return _launch_upfirdn2d(x, f, *up, *down, *padding, flip_filter, gain)

    @staticmethod
    def backward(ctx, dy):
        # same op with up <-> down, flipped filter and the pads of upfirdn2d.py:255-266
        f, (upx, upy), (dnx, dny), (px0, px1, py0, py1), flip, gain, xs = ctx.meta
        _, _, ih, iw = xs
        _, _, oh, ow = dy.shape
        fh, fw = f.shape
        p = [fw - px0 - 1, iw * upx - ow * dnx + px0 - upx + 1, fh - py0 - 1, ih * upy - oh * dny + py0 - upy + 1]
        # (an apply, not a bare launch: the op is linear and its adjoint is the op itself, so gradients of every order exist)
        dx = _Upfirdn2d.apply(dy, f, (dnx, dny), (upx, upy), tuple(p), not flip, gain)
        return dx, None, None, None, None, None, None


def upfirdn2d(x, f, up=1, down=1, padding=0, flip_filter=False, gain=1, impl='hip'):
    """Pad, upsample, filter, downsample (reference: upfirdn2d.py:118-162).  A 1-D (separable) filter runs as one pass per axis,
    each with the square root of the gain, exactly as the reference's plugin path applies it (upfirdn2d.py:188-201); the intermediate
    keeps the dtype of the result.  float16 / float32 / float64 x returns its own dtype, any other dtype is computed and returned in
    float32; the taps are float32 for every dtype (upfirdn2d.cpp:21)."""
    assert isinstance(x, torch.Tensor) and x.ndim == 4
    if f is None:
        f = torch.ones([1, 1], dtype=torch.float32)
    assert isinstance(f, torch.Tensor) and f.ndim in (1, 2) and f.dtype == torch.float32
    (upx, upy), (dnx, dny) = _parse_scaling(up), _parse_scaling(down)
    px0, px1, py0, py1 = _parse_padding(padding)
    if f.ndim == 1:
        g = float(gain) ** 0.5
        fc = f.cpu()
        y = _Upfirdn2d.apply(x, fc[None, :], (upx, 1), (dnx, 1), (px0, px1, 0, 0), bool(flip_filter), g)
        return _Upfirdn2d.apply(y, fc[:, None], (1, upy), (1, dny), (0, 0, py0, py1), bool(flip_filter), g)
    return _Upfirdn2d.apply(x, f.cpu(), (upx, upy), (dnx, dny), (px0, px1, py0, py1), bool(flip_filter), float(gain))


def _fshape(f):
    """(fh, fw) of a 2-D or separable 1-D filter (upfirdn2d.py:55-66 _get_filter_size)."""
    return (f.shape[0], f.shape[0]) if f.ndim == 1 else tuple(f.shape)


def filter2d(x, f, padding=0, flip_filter=False, gain=1, impl='hip'):
    """reference: upfirdn2d.py:277-309"""
    px0, px1, py0, py1 = _parse_padding(padding)
    fh, fw = _fshape(f)
    p = [px0 + fw // 2, px1 + (fw - 1) // 2, py0 + fh // 2, py1 + (fh - 1) // 2]
    return upfirdn2d(x, f, padding=p, flip_filter=flip_filter, gain=gain)


def upsample2d(x, f, up=2, padding=0, flip_filter=False, gain=1, impl='hip'):
    """reference: upfirdn2d.py:313-348"""
    upx, upy = _parse_scaling(up)
    px0, px1, py0, py1 = _parse_padding(padding)
    fh, fw = _fshape(f)
    p = [px0 + (fw + upx - 1) // 2, px1 + (fw - upx) // 2, py0 + (fh + upy - 1) // 2, py1 + (fh - upy) // 2]
    return upfirdn2d(x, f, up=up, padding=p, flip_filter=flip_filter, gain=gain * upx * upy)


def downsample2d(x, f, down=2, padding=0, flip_filter=False, gain=1, impl='hip'):
    """reference: upfirdn2d.py:352-387"""
    dnx, dny = _parse_scaling(down)
    px0, px1, py0, py1 = _parse_padding(padding)
    fh, fw = _fshape(f)
    p = [px0 + (fw - dnx + 1) // 2, px1 + (fw - dnx) // 2, py0 + (fh - dny + 1) // 2, py1 + (fh - dny) // 2]
    return upfirdn2d(x, f, down=down, padding=p, flip_filter=flip_filter, gain=gain)


def _flr_filter(f, dev, name):
    """(device taps or None, rows (0 = 1-D), taps per row) of an fu / fd argument; None is the 1 x 1 identity."""
    if f is None:
        return None, 1, 1
    assert isinstance(f, torch.Tensor) and 1 <= f.ndim <= 2
    if f.dtype != torch.float32:
        raise _lib.LatentAugHipError(f'filtered_lrelu: {name} must be float32, got {f.dtype}')
    f = f.to(dev).contiguous()
    return f, (f.shape[0] if f.ndim == 2 else 0), f.shape[-1]


def _flr_sign_shape(h, w, fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1):
    lib = _lib.load()
    rows, row_bytes = C.c_int(0), C.c_int(0)
    _lib.check(lib.la_filtered_lrelu_sign_shape(h, w, fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1, C.byref(rows), C.byref(row_bytes)),
               'filtered_lrelu_sign_shape')
    return rows.value, row_bytes.value


class _FilteredLRelu(torch.autograd.Function):
    """One launch of la_filtered_lrelu_f32.  The backward is the same Function in sign-read mode (filtered_lrelu.py:239-268); it is linear
    in dy, so its own backward is that recipe again and every order of gradient is a launch of the same kernel."""

    @staticmethod
    def forward(ctx, x, b, fu, fd, si, cfg):
        up, down, px0, px1, py0, py1, gain, slope, clamp, flip, sx, sy = cfg
        (fut, fu_h, fu_w), (fdt, fd_h, fd_w) = fu, fd
        lib = _lib.load()
        n, c, h, w = x.shape
        fuy, fdy = fu_h or fu_w, fd_h or fd_w
        ow = lib.la_filtered_lrelu_out_size(w, up, down, px0, px1, fu_w, fd_w)
        oh = lib.la_filtered_lrelu_out_size(h, up, down, py0, py1, fuy, fdy)
        if ow < 1 or oh < 1:
            raise _lib.LatentAugHipError(f'filtered_lrelu: output must be at least 1x1 (got {oh}x{ow})')
        y = torch.empty([n, c, oh, ow], device=x.device, dtype=torch.float32)
        so = None
        write = si is None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])      # (filtered_lrelu.py:206)
        if write:
            rows, row_bytes = _flr_sign_shape(h, w, fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1)
            so = _lib.workspace(n * c * rows * row_bytes, x.device)
        _lib.check(lib.la_filtered_lrelu_f32(_lib.ptr(x), _lib.ptr(fut), _lib.ptr(fdt), _lib.ptr(b), _lib.ptr(si), _lib.ptr(so), _lib.ptr(y),
                                             n, c, h, w, fu_h, fu_w, fd_h, fd_w, up, down, px0, px1, py0, py1, sx, sy, gain, slope, clamp,
                                             int(flip), int(write), _lib.stream_ptr()), 'filtered_lrelu')
        ctx.fu, ctx.fd, ctx.signs = fu, fd, (si if si is not None else so)
        ctx.meta = (cfg, tuple(x.shape), (oh, ow))
        return y

    @staticmethod
    def backward(ctx, dy):
        (up, down, px0, px1, py0, py1, gain, slope, clamp, flip, sx, sy), (n, c, h, w), (oh, ow) = ctx.meta
        fu, fd = ctx.fu, ctx.fd
        fu_w, fuy, fd_w, fdy = fu[2], fu[1] or fu[2], fd[2], fd[1] or fd[2]
        dx = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            pp = [fu_w - 1 + fd_w - 1 - px0, w * up - ow * down + px0 - (up - 1), fuy - 1 + fdy - 1 - py0, h * up - oh * down + py0 - (up - 1)]
            cfg = (down, up, *pp, gain * up ** 2 / down ** 2, slope, math.inf, not flip, sx - (fu_w - 1) + px0, sy - (fuy - 1) + py0)
            dx = _FilteredLRelu.apply(dy.contiguous(), None, fd, fu, ctx.signs, cfg)
        if ctx.needs_input_grad[1]:
            db = _BiasSum.apply(dx, h * w, c)
        return dx, db, None, None, None, None


def filtered_lrelu(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=np.sqrt(2), slope=0.2, clamp=None, flip_filter=False, impl='hip'):
    """Filtered leaky ReLU (reference: filtered_lrelu.py:59-108): bias, zero-insert up, pad / crop, FIR fu with gain up**2, gain, leaky
    ReLU, clamp, FIR fd, keep every down-th sample -- one fused HIP launch per call.  fu / fd: float32 [taps] (separable), [h, w] or
    None (identity); they are used from device memory.  Gradients with respect to x and b of every order (sign-read launches of the same
    kernel); none with respect to the filters, as in the reference."""
    assert isinstance(x, torch.Tensor)
    _lib.require_gpu(x)
    if x.dtype != torch.float32:
        raise _lib.LatentAugHipError(f'filtered_lrelu: x must be float32 (got {x.dtype}); there is no other-precision kernel')
    assert x.ndim == 4
    if b is not None:
        assert isinstance(b, torch.Tensor) and b.dtype == x.dtype
        assert b.shape == (x.shape[1],), b.shape
        _lib.require_gpu(b)
    assert isinstance(up, (int, np.integer)) and up >= 1
    assert isinstance(down, (int, np.integer)) and down >= 1
    if isinstance(padding, (int, np.integer)):
        padding = [padding, padding]
    assert isinstance(padding, (list, tuple)) and all(isinstance(v, (int, np.integer)) for v in padding)
    px0, px1, py0, py1 = _parse_padding(padding)
    assert gain == float(gain) and gain > 0
    assert slope == float(slope) and slope >= 0
    assert clamp is None or (clamp == float(clamp) and clamp >= 0)
    fu_ = _flr_filter(fu, x.device, 'fu')
    fd_ = _flr_filter(fd, x.device, 'fd')
    cfg = (int(up), int(down), px0, px1, py0, py1, float(gain), float(slope), math.inf if clamp is None else float(clamp), bool(flip_filter), 0, 0)
    return _FilteredLRelu.apply(x.contiguous(), None if b is None else b.contiguous(), fu_, fd_, None, cfg)


def l2_loss_vectorized(X, Y, compute_mean=True):
    """Pairwise squared-L2 in GEMM form (reference: util_latent_aug.py:315-361); forward only."""
    _lib.require_gpu(X)
    lib = _lib.load()
    assert X.ndim == Y.ndim and X.ndim in (2, 3, 4)
    n, m = X.shape[0], Y.shape[0]
    Xf = X.reshape(n, -1).contiguous().float()
    Yf = Y.reshape(m, -1).contiguous().float()
    K = Xf.shape[1]
    assert Yf.shape[1] == K
    D = torch.empty([m, n], device=X.device, dtype=torch.float32)
    mean = torch.empty([1], device=X.device, dtype=torch.float32)
    ws = _lib.workspace(4 * lib.la_pairwise_l2_workspace_floats(n, m), X.device, torch.float32)
    _lib.check(lib.la_pairwise_l2_f32(_lib.ptr(Xf), n, _lib.ptr(Yf), m, K, _lib.ptr(D), _lib.ptr(mean), _lib.ptr(ws),
                                      _lib.stream_ptr()), 'pairwise_l2')
    return mean[0] if compute_mean else D


# ---------------------------------------------------------------------------------------------------------------------------------
# conv2d / conv_transpose2d / conv2d_resample

def _conv_geo_toggle(geo):
    """The convolution whose forward is the data gradient of `geo`: transpose toggled, the two image shapes exchanged, the same w."""
    t, s, py, px, groups, corr, xs, ws, ys = geo
    return (not t, s, py, px, groups, corr, ys, ws, xs)


def _conv_dims(geo):
    t, s, py, px, groups, corr, xs, ws, ys = geo
    return (xs[0], xs[1], xs[2], xs[3], ys[1], ws[2], ws[3], ys[2], ys[3], s)


def _conv_scratch(op, geo, dev):
    t, s, py, px, groups = geo[:5]
    n = _lib.load().la_conv2d_workspace_bytes(op, *_conv_dims(geo), groups, int(t))
    return _lib.workspace(n, dev)


def _conv_launch_y(x, w, geo):
    t, s, py, px, groups, corr, xs, ws, ys = geo
    assert tuple(x.shape) == tuple(xs) and tuple(w.shape) == tuple(ws), (x.shape, w.shape, geo)
    x, w = x.contiguous(), w.contiguous()
    y = torch.empty(ys, device=x.device, dtype=torch.float32)
    scratch = _conv_scratch(0, geo, x.device)
    _lib.check(_lib.load().la_conv2d_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(y), _lib.ptr(scratch), scratch.numel(), *_conv_dims(geo), py, px, groups,
                                         int(corr), int(t), _lib.stream_ptr()), 'conv2d')
    return y


def _conv_launch_w(x, dy, geo):
    t, s, py, px, groups, corr, xs, ws, ys = geo
    assert tuple(x.shape) == tuple(xs) and tuple(dy.shape) == tuple(ys), (x.shape, dy.shape, geo)
    x, dy = x.contiguous(), dy.contiguous()
    dw = torch.empty(ws, device=x.device, dtype=torch.float32)
    scratch = _conv_scratch(1, geo, x.device)
    _lib.check(_lib.load().la_conv2d_wgrad_f32(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(scratch), scratch.numel(), *_conv_dims(geo), py, px,
                                               groups, int(corr), int(t), _lib.stream_ptr()), 'conv2d_wgrad')
    return dw


class _ConvY(torch.autograd.Function):
    """y = conv(x, w) of a geometry (la_conv2d_f32).  Bilinear: its backward is the same map of the toggled geometry (data gradient) and
    _ConvW (weight gradient), whose backwards are these maps again -- gradients of every order are launches of the same kernels."""

    @staticmethod
    def forward(ctx, x, w, geo):
        ctx.save_for_backward(x, w)
        ctx.geo = geo
        return _conv_launch_y(x, w, geo)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        gx = _ConvY.apply(dy, w, _conv_geo_toggle(ctx.geo)) if ctx.needs_input_grad[0] else None
        gw = _ConvW.apply(x, dy, ctx.geo) if ctx.needs_input_grad[1] else None
        return gx, gw, None


class _ConvW(torch.autograd.Function):
    """dw = weight gradient of <dy, conv(x, w)> (la_conv2d_wgrad_f32), bilinear in (x, dy)."""

    @staticmethod
    def forward(ctx, x, dy, geo):
        ctx.save_for_backward(x, dy)
        ctx.geo = geo
        return _conv_launch_w(x, dy, geo)

    @staticmethod
    def backward(ctx, ddw):
        x, dy = ctx.saved_tensors
        gx = _ConvY.apply(dy, ddw, _conv_geo_toggle(ctx.geo)) if ctx.needs_input_grad[0] else None
        gdy = _ConvY.apply(x, ddw, ctx.geo) if ctx.needs_input_grad[1] else None
        return gx, gdy, None


def _conv_op(x, w, stride, padding, groups, transpose, flip_weight, name):
    assert isinstance(x, torch.Tensor) and isinstance(w, torch.Tensor)
    _lib.require_gpu(x)
    _lib.require_gpu(w)
    assert x.ndim == 4 and w.ndim == 4
    assert w.dtype == x.dtype
    if x.dtype != torch.float32:
        raise _lib.LatentAugHipError(f'{name}: x and w must be float32 (got {x.dtype}); there is no other-precision kernel')
    assert isinstance(stride, (int, np.integer)) and isinstance(groups, (int, np.integer)) and groups >= 1
    py, px = (padding, padding) if isinstance(padding, (int, np.integer)) else padding
    s, py, px, groups = int(stride), int(py), int(px), int(groups)
    n, cin, h, wd = x.shape
    kh, kw = w.shape[2:]
    if s < 1:
        raise _lib.LatentAugHipError(f'{name}: stride must be at least 1')
    if transpose:
        assert w.shape[0] == cin, (x.shape, w.shape)
        cout, oh, ow = w.shape[1] * groups, (h - 1) * s - 2 * py + kh, (wd - 1) * s - 2 * px + kw
    else:
        assert w.shape[1] * groups == cin, (x.shape, w.shape)
        cout, oh, ow = w.shape[0], (h + 2 * py - kh) // s + 1, (wd + 2 * px - kw) // s + 1
    if oh < 1 or ow < 1:
        raise _lib.LatentAugHipError(f'{name}: output smaller than 1x1 (got {oh}x{ow})')
    geo = (bool(transpose), s, py, px, groups, bool(flip_weight), tuple(x.shape), tuple(w.shape), (n, cout, oh, ow))
    return _ConvY.apply(x, w, geo)


def conv2d(x, w, stride=1, padding=0, groups=1):
    """torch.nn.functional.conv2d(x, w, None, stride, padding, 1, groups) as conv2d_gradfix.py:24 provides it: float32 device tensors,
    one stride for both axes, padding an int or (py, px).  Gradients of every order with respect to x and w."""
    return _conv_op(x, w, stride, padding, groups, False, True, 'conv2d')


def conv_transpose2d(x, w, stride=1, padding=0, groups=1):
    """torch.nn.functional.conv_transpose2d(x, w, None, stride, padding, 0, groups) (conv2d_gradfix.py:29); w [Cin][Cout/groups][kh][kw]."""
    return _conv_op(x, w, stride, padding, groups, True, True, 'conv_transpose2d')


def _conv2d_wrapper(x, w, stride=1, padding=0, groups=1, transpose=False, flip_weight=True):
    """conv2d_resample.py:26-40.  flip_weight=True is correlation; False runs on the flipped kernel -- the kernels index it that
    way themselves, no flipped copy of w is made."""
    return _conv_op(x, w, stride, padding, groups, transpose, flip_weight, 'conv2d_resample')


def conv2d_resample(x, w, f=None, up=1, down=1, padding=0, groups=1, flip_weight=True, flip_filter=False, impl='hip'):
    """2-D convolution with optional up / down-sampling (reference: conv2d_resample.py:46-141): x [N][Cin][H][W], w
    [Cout][Cin/groups][kh][kw], f a filter of setup_filter() or None, up / down integer factors, padding with respect to the upsampled
    image (an int, [x, y] or [x0, x1, y0, y1]), flip_weight=False for a true convolution.  float32 device tensors; composed of
    conv2d / conv_transpose2d and upfirdn2d, with gradients of every order with respect to x and w."""
    assert isinstance(x, torch.Tensor) and x.ndim == 4
    assert isinstance(w, torch.Tensor) and w.ndim == 4 and w.dtype == x.dtype
    assert f is None or (isinstance(f, torch.Tensor) and f.ndim in [1, 2] and f.dtype == torch.float32)
    assert isinstance(up, (int, np.integer)) and up >= 1
    assert isinstance(down, (int, np.integer)) and down >= 1
    assert isinstance(groups, (int, np.integer)) and groups >= 1
    _lib.require_gpu(x)
    _lib.require_gpu(w)
    if x.dtype != torch.float32:
        raise _lib.LatentAugHipError(f'conv2d_resample: x and w must be float32 (got {x.dtype}); there is no other-precision kernel')
    up, down, groups = int(up), int(down), int(groups)
    cout, cin_g, kh, kw = (int(v) for v in w.shape)
    fh, fw = (1, 1) if f is None else _fshape(f)
    px0, px1, py0, py1 = _parse_padding(padding)

    # padding with respect to the upsampled image -> padding of the resampling steps
    if up > 1:
        px0 += (fw + up - 1) // 2
        px1 += (fw - up) // 2
        py0 += (fh + up - 1) // 2
        py1 += (fh - up) // 2
    if down > 1:
        px0 += (fw - down + 1) // 2
        px1 += (fw - down) // 2
        py0 += (fh - down + 1) // 2
        py1 += (fh - down) // 2

    # 1x1 kernel and downsampling only: filter and decimate first, convolve the small image
    if kw == 1 and kh == 1 and down > 1 and up == 1:
        x = upfirdn2d(x, f, down=down, padding=[px0, px1, py0, py1], flip_filter=flip_filter)
        return _conv2d_wrapper(x, w, groups=groups, flip_weight=flip_weight)

    # 1x1 kernel and upsampling only: convolve the small image first
    if kw == 1 and kh == 1 and up > 1 and down == 1:
        x = _conv2d_wrapper(x, w, groups=groups, flip_weight=flip_weight)
        return upfirdn2d(x, f, up=up, padding=[px0, px1, py0, py1], gain=up ** 2, flip_filter=flip_filter)

    # downsampling only: filter, then a strided convolution
    if down > 1 and up == 1:
        x = upfirdn2d(x, f, padding=[px0, px1, py0, py1], flip_filter=flip_filter)
        return _conv2d_wrapper(x, w, stride=down, groups=groups, flip_weight=flip_weight)

    # upsampling (and possibly downsampling after it): transposed strided convolution, then the filter
    if up > 1:
        if groups == 1:
            wt = w.transpose(0, 1)
        else:
            wt = w.reshape(groups, cout // groups, cin_g, kh, kw).transpose(1, 2).reshape(groups * cin_g, cout // groups, kh, kw)
        px0 -= kw - 1
        px1 -= kw - up
        py0 -= kh - 1
        py1 -= kh - up
        pxt = max(min(-px0, -px1), 0)
        pyt = max(min(-py0, -py1), 0)
        x = _conv2d_wrapper(x, wt, stride=up, padding=[pyt, pxt], groups=groups, transpose=True, flip_weight=(not flip_weight))
        x = upfirdn2d(x, f, padding=[px0 + pxt, px1 + pxt, py0 + pyt, py1 + pyt], gain=up ** 2, flip_filter=flip_filter)
        if down > 1:
            x = upfirdn2d(x, f, down=down, flip_filter=flip_filter)
        return x

    # no resampling and a symmetric non-negative padding: the convolution pads itself
    if up == 1 and down == 1 and px0 == px1 and py0 == py1 and px0 >= 0 and py0 >= 0:
        return _conv2d_wrapper(x, w, padding=[py0, px0], groups=groups, flip_weight=flip_weight)

    # anything else: pad / crop through upfirdn2d, convolve, decimate
    x = upfirdn2d(x, (f if up > 1 else None), up=up, padding=[px0, px1, py0, py1], gain=up ** 2, flip_filter=flip_filter)
    x = _conv2d_wrapper(x, w, groups=groups, flip_weight=flip_weight)
    if down > 1:
        x = upfirdn2d(x, f, down=down, flip_filter=flip_filter)
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# grid_sample (grid_sample_gradfix.py) and fma (fma.py)

def _grid_sample_dims(x, grid):
    n, c, h, w = x.shape
    return n, c, h, w, grid.shape[1], grid.shape[2]


def _grid_sample_launch(x, grid):
    n, c, h, w, ho, wo = _grid_sample_dims(x, grid)
    y = torch.empty([n, c, ho, wo], device=x.device, dtype=x.dtype)
    if y.numel() and x.numel():
        fn = getattr(_lib.load(), 'la_grid_sample_' + _DTYPES[x.dtype])
        _lib.check(fn(_lib.ptr(x), _lib.ptr(grid), _lib.ptr(y), n, c, h, w, ho, wo, _lib.stream_ptr()), 'grid_sample')
    else:
        y.zero_()
    return y


class _GridSampleForward(torch.autograd.Function):
    """y = grid_sample(input, grid) (la_grid_sample_*); the reference's _GridSample2dForward (grid_sample_gradfix.py:40-53)."""

    @staticmethod
    def forward(ctx, input, grid):
        ctx.save_for_backward(input, grid)
        return _grid_sample_launch(input, grid)

    @staticmethod
    def backward(ctx, grad_output):
        input, grid = ctx.saved_tensors
        return _GridSampleBackward.apply(grad_output, input, grid, (ctx.needs_input_grad[0], ctx.needs_input_grad[1]))


class _GridSampleBackward(torch.autograd.Function):
    """(grad_input, grad_grid) of one launch of la_grid_sample_grad_*; `mask` is torch's output_mask, an output not asked for is None.
    grad_input is linear in grad_output and does not depend on input: its gradient with respect to grad_output is the forward op on the
    incoming gradient (grid_sample_gradfix.py:70-81), which is again differentiable, so every order between input and output exists.
    Nothing is defined for second derivatives that involve grid -- asking for one raises."""

    @staticmethod
    def forward(ctx, grad_output, input, grid, mask):
        ctx.set_materialize_grads(False)
        grad_output = grad_output.contiguous()
        n, c, h, w, ho, wo = _grid_sample_dims(input, grid)
        assert tuple(grad_output.shape) == (n, c, ho, wo) and grad_output.dtype == input.dtype
        dx = torch.empty_like(input) if mask[0] else None
        dgrid = torch.empty_like(grid) if mask[1] else None
        if input.numel() and grad_output.numel() and (mask[0] or mask[1]):
            lib = _lib.load()
            args = [_lib.ptr(grad_output), _lib.ptr(input), _lib.ptr(grid), _lib.ptr(dx), _lib.ptr(dgrid)]
            if input.dtype == torch.float16:
                ws = _lib.workspace(4 * lib.la_grid_sample_grad_workspace_floats(n, c, h, w), input.device, torch.float32) if mask[0] else None
                args.append(_lib.ptr(ws))
            fn = getattr(lib, 'la_grid_sample_grad_' + _DTYPES[input.dtype])
            _lib.check(fn(*args, n, c, h, w, ho, wo, _lib.stream_ptr()), 'grid_sample_grad')
        else:
            for t in (dx, dgrid):
                if t is not None:
                    t.zero_()
        ctx.save_for_backward(grid)
        return dx, dgrid

    @staticmethod
    def backward(ctx, grad2_grad_input, grad2_grad_grid):
        grid, = ctx.saved_tensors
        if grad2_grad_grid is not None or ctx.needs_input_grad[2]:
            raise _lib.LatentAugHipError(
                'grid_sample: second derivatives that involve grid are not defined (as in the reference, grid_sample_gradfix.py:70-81): '
                'a gradient of grad_grid, or a gradient with respect to a grid that requires grad, was asked for. Detach the grid '
                'where gradients of gradients are taken.')
        grad2_grad_output = None
        if ctx.needs_input_grad[0] and grad2_grad_input is not None:
            grad2_grad_output = _GridSampleForward.apply(grad2_grad_input.contiguous(), grid)
        return grad2_grad_output, None, None, None


def grid_sample(input, grid):
    """torch.nn.functional.grid_sample(input, grid, mode='bilinear', padding_mode='zeros', align_corners=False) for 2-D images, as the
    reference's grid_sample_gradfix.grid_sample (grid_sample_gradfix.py:28-31): input [N, C, H, W], grid [N, Ho, Wo, 2] of (x, y) in
    [-1, 1] -> [N, C, Ho, Wo] in the input's dtype.  float16 (fp32 arithmetic inside), float32 and float64 run on kernels of their own;
    any other dtype is computed and returned in float32.  Gradients of every order between input and output; first-order gradients
    with respect to grid; a second derivative that involves grid raises LatentAugHipError."""
    assert isinstance(input, torch.Tensor) and isinstance(grid, torch.Tensor)
    _lib.require_gpu(input)
    _lib.require_gpu(grid)
    assert input.ndim == 4
    assert grid.ndim == 4
    assert grid.shape[0] == input.shape[0] and grid.shape[3] == 2, (input.shape, grid.shape)
    if grid.dtype != input.dtype:
        raise _lib.LatentAugHipError(f'grid_sample: input and grid must have the same dtype, got {input.dtype} and {grid.dtype}')
    return _GridSampleForward.apply(_op_input(input), _op_input(grid))


def _pad4(shape):
    return (1,) * (4 - len(shape)) + tuple(int(v) for v in shape)


def _long4(v):
    return (C.c_long * 4)(*v)


def _fma_launch(a, b, c, shape):
    """a * b + c (c None: a * b) of contiguous float32 operands over the broadcast `shape` (rank <= 4), one launch of la_fma_f32."""
    s4 = _pad4(shape)

    def strides(t):
        ts = _pad4(t.shape)
        st = (0,) * (4 - t.ndim) + tuple(t.stride())
        return _long4([0 if ts[k] == 1 else st[k] for k in range(4)])
    y = torch.empty(shape, device=a.device, dtype=torch.float32)
    if y.numel():
        _lib.check(_lib.load().la_fma_f32(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(y), _long4(s4), strides(a), strides(b),
                                          strides(c) if c is not None else None, _lib.stream_ptr()), 'fma')
    return y


class _Unbroadcast(torch.autograd.Function):
    """x summed over the axes along which `shape` was broadcast to x.shape (fma.py:49-58), one launch of la_unbroadcast_sum_f32 with
    a fixed summation order; its own gradient is a broadcast view."""

    @staticmethod
    def forward(ctx, x, shape):
        x = x.contiguous()
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
        ctx.xshape = tuple(x.shape)
        if x.numel():
            _lib.check(_lib.load().la_unbroadcast_sum_f32(_lib.ptr(x), _lib.ptr(out), _long4(_pad4(x.shape)), _long4(_pad4(shape)),
                                                          _lib.stream_ptr()), 'unbroadcast_sum')
        else:
            out.zero_()
        return out

    @staticmethod
    def backward(ctx, d_out):
        return d_out.expand(ctx.xshape), None


def _unbroadcast(x, shape):
    shape = tuple(shape)
    return x if tuple(x.shape) == shape else _Unbroadcast.apply(x, shape)


class _Fma(torch.autograd.Function):
    """a * b + c; the gradients are the same Function (and _Unbroadcast) applied to the incoming gradient (fma.py:20-45), so autograd
    gives every higher order."""

    @staticmethod
    def forward(ctx, a, b, c, shape):
        ctx.save_for_backward(a, b)
        ctx.shapes = (tuple(a.shape), tuple(b.shape), None if c is None else tuple(c.shape))
        return _fma_launch(a.contiguous(), b.contiguous(), None if c is None else c.contiguous(), shape)

    @staticmethod
    def backward(ctx, dout):
        a, b = ctx.saved_tensors
        sa, sb, sc = ctx.shapes
        shape = tuple(dout.shape)
        da = _unbroadcast(_Fma.apply(dout, b, None, shape), sa) if ctx.needs_input_grad[0] else None
        db = _unbroadcast(_Fma.apply(dout, a, None, shape), sb) if ctx.needs_input_grad[1] else None
        dc = _unbroadcast(dout, sc) if ctx.needs_input_grad[2] else None
        return da, db, dc, None


def fma(a, b, c):
    """a * b + c with un-broadcast gradients (reference: fma.py:15): the operands broadcast against each other (rank <= 4), one fused
    multiply-add per element.  float32 kernels; other floating dtypes are computed in float32 and returned in the operands' promoted
    dtype."""
    assert all(isinstance(t, torch.Tensor) for t in (a, b, c))
    for t in (a, b, c):
        _lib.require_gpu(t)
    shape = tuple(torch.broadcast_shapes(a.shape, b.shape, c.shape))
    if len(shape) > 4:
        raise _lib.LatentAugHipError(f'fma: at most 4 dimensions, got {len(shape)}')
    dtype = torch.promote_types(torch.promote_types(a.dtype, b.dtype), c.dtype)
    if not dtype.is_floating_point:
        raise _lib.LatentAugHipError(f'fma: floating-point operands only, got {dtype}')
    y = _Fma.apply(a.float(), b.float(), c.float(), shape)
    return y if dtype == torch.float32 else y.to(dtype)
