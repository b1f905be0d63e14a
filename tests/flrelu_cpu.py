"""float64 torch-CPU restatement of filtered_lrelu, written from the nine steps of its docstring (reference filtered_lrelu.py:59-108).

Test helper only: the checker of the HIP op on shapes the goldens do not cover, and the source of the sign-kink masks the GPU tests use.
"""
import math

import torch
import torch.nn.functional as F


def _pad4(padding):
    if isinstance(padding, int):
        padding = [padding, padding]
    p = [int(v) for v in padding]
    return [p[0], p[0], p[1], p[1]] if len(p) == 2 else p


def _fir(z, f, flip_filter):
    """'valid' FIR of every plane of z [N, C, H, W] with f ([taps]: along x then y; [h, w]: 2-D); convolution unless flip_filter."""
    if f is None:
        return z
    f = f.to(torch.float64)
    n, c, h, w = z.shape
    z = z.reshape(n * c, 1, h, w)
    if f.ndim == 1:
        k = f if flip_filter else f.flip(0)
        z = F.conv2d(z, k.reshape(1, 1, 1, -1))
        z = F.conv2d(z, k.reshape(1, 1, -1, 1))
    else:
        k = f if flip_filter else f.flip([0, 1])
        z = F.conv2d(z, k[None, None])
    return z.reshape(n, c, z.shape[2], z.shape[3])


def up_stage(x, fu=None, b=None, up=1, padding=0, flip_filter=False):
    """Steps 1-4: bias, zero-insert, pad / crop, FIR fu with gain up**2 -> the full intermediate."""
    px0, px1, py0, py1 = _pad4(padding)
    x = x.to(torch.float64)
    if b is not None:
        x = x + b.to(torch.float64).reshape(1, -1, 1, 1)
    n, c, h, w = x.shape
    z = x.new_zeros([n, c, h * up, w * up])
    z[:, :, ::up, ::up] = x
    z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    return _fir(z, fu, flip_filter) * (up ** 2)


def act_stage(z, gain=math.sqrt(2), slope=0.2, clamp=None):
    """Steps 5-7: gain, leaky ReLU, clamp."""
    z = F.leaky_relu(z * gain, slope)
    return z if clamp is None else z.clamp(-clamp, clamp)


def down_stage(z, fd=None, down=1, flip_filter=False):
    """Steps 8-9: FIR fd, keep every down-th sample."""
    return _fir(z, fd, flip_filter)[:, :, ::down, ::down]


def filtered_lrelu(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=math.sqrt(2), slope=0.2, clamp=None, flip_filter=False):
    z = up_stage(x, fu, b, up, padding, flip_filter)
    return down_stage(act_stage(z, gain, slope, clamp), fd, down, flip_filter)


def active_shape(y_shape, fd, down):
    """(rows, cols) of the intermediate the outputs read: (O - 1) * down + fd taps per axis."""
    fh, fw = (1, 1) if fd is None else ((fd.shape[0], fd.shape[0]) if fd.ndim == 1 else tuple(fd.shape))
    return (y_shape[2] - 1) * down + fh, (y_shape[3] - 1) * down + fw


def kink_mask(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=math.sqrt(2), slope=0.2, clamp=None, flip_filter=False, rtol=1e-5):
    """Intermediate samples (active extent) where fp32 and float64 may legitimately take different lrelu / clamp branches: gain * value
    within rtol * max|gain * value| of 0, or its lrelu within that distance of +-clamp.  Returns (mask [N, C, ah, aw] float64, count)."""
    a = up_stage(x, fu, b, up, padding, flip_filter) * gain
    out = filtered_lrelu(x, fu, fd, b, up, down, padding, gain, slope, clamp, flip_filter)
    ah, aw = active_shape(out.shape, fd, down)
    a = a[:, :, :ah, :aw]
    # (samples whose up-FIR footprint holds padding only are exact zeros in every precision: not a kink, and nothing reaches x from them)
    absf = None if fu is None else fu.abs()
    live = up_stage(torch.ones_like(x, dtype=torch.float64), absf, None, up, padding, flip_filter)[:, :, :ah, :aw] > 0
    tau = rtol * float(a.abs().max())
    m = (a.abs() <= tau) & live
    if clamp is not None:
        m |= ((a.clamp(min=0) - clamp).abs() <= tau) | ((a.clamp(max=0) * slope + clamp).abs() <= tau)
    return m.to(torch.float64), int(m.sum())


def affected(mask, x_shape, fu=None, fd=None, up=1, down=1, padding=0, flip_filter=False):
    """Which outputs ([N, C, OH, OW]) and which input gradients ([N, C, H, W]) a set of intermediate samples can reach (bool masks): the
    down-FIR cone of the mask, and the transpose of the up-FIR cone (absolute taps, so nothing cancels)."""
    def absf(f):
        return None if f is None else f.abs()
    y_aff = down_stage(mask, absf(fd), down, flip_filter) > 0
    xx = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    z = up_stage(xx, absf(fu), None, up, padding, flip_filter)
    ah, aw = mask.shape[2], mask.shape[3]
    (gx,) = torch.autograd.grad((z[:, :, :ah, :aw] * mask).sum(), [xx])
    return y_aff, gx > 0
