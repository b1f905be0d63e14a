"""float64 torch-CPU restatement of filtered_lrelu, written from the nine steps of its docstring (reference filtered_lrelu.py:59-108).

Test helper only: the checker of the HIP op on shapes the goldens do not cover, and the source of the sign-kink masks the GPU tests use.
Every stage takes a dtype (default float64); run in float32 it is the float32 yardstick of the cases that have no golden.  The sign
helpers (sign_bits, pack_signs, unpack_signs, act_read) restate the sign buffer of include/latentaug_hip.h.
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
    f = f.to(z.dtype)
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


def up_stage(x, fu=None, b=None, up=1, padding=0, flip_filter=False, dtype=torch.float64):
    """Steps 1-4: bias, zero-insert, pad / crop, FIR fu with gain up**2 -> the full intermediate."""
    px0, px1, py0, py1 = _pad4(padding)
    x = x.to(dtype)
    if b is not None:
        x = x + b.to(dtype).reshape(1, -1, 1, 1)
    n, c, h, w = x.shape
    z = x.new_zeros([n, c, h * up, w * up])
    z[:, :, ::up, ::up] = x
    z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    return _fir(z, fu, flip_filter) * (up ** 2)


def act_stage(z, gain=math.sqrt(2), slope=0.2, clamp=None, dtype=torch.float64):
    """Steps 5-7: gain, leaky ReLU, clamp."""
    z = F.leaky_relu(z.to(dtype) * gain, slope)
    return z if clamp is None else z.clamp(-clamp, clamp)


def down_stage(z, fd=None, down=1, flip_filter=False, dtype=torch.float64):
    """Steps 8-9: FIR fd, keep every down-th sample."""
    return _fir(z.to(dtype), fd, flip_filter)[:, :, ::down, ::down]


def filtered_lrelu(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=math.sqrt(2), slope=0.2, clamp=None, flip_filter=False,
                   dtype=torch.float64):
    z = up_stage(x, fu, b, up, padding, flip_filter, dtype)
    return down_stage(act_stage(z, gain, slope, clamp, dtype), fd, down, flip_filter, dtype)


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


# ------------------------------------------------------------------------------------------------------------ the sign buffer
def _active(z, fd, down):
    """z (the full intermediate) cut to the active extent: the samples some output reads."""
    fh, fw = (1, 1) if fd is None else ((fd.shape[0], fd.shape[0]) if fd.ndim == 1 else tuple(fd.shape))
    oh, ow = (z.shape[2] - fh) // down + 1, (z.shape[3] - fw) // down + 1
    return z[:, :, :(oh - 1) * down + fh, :(ow - 1) * down + fw]


def sign_bits(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=math.sqrt(2), slope=0.2, clamp=None, flip_filter=False):
    """The two sign bits of every sample of the active extent, uint8 [N, C, ah, aw] with values 0..3, from the float64 intermediate:
    bit 0 = gain * mid < 0, bit 1 = |lrelu| > clamp."""
    a = _active(up_stage(x, fu, b, up, padding, flip_filter), fd, down) * gain
    bits = (a < 0).to(torch.uint8)
    if clamp is not None:
        bits = bits | (F.leaky_relu(a, slope).abs() > clamp).to(torch.uint8) * 2
    return bits


def pack_signs(bits, rows, row_bytes):
    """bits [N, C, h, w] (0..3) -> the buffer layout, uint8 [N, C, rows, row_bytes]: 4 samples per byte, sample t of a row at bits
    2 * (t % 4) of byte t // 4; everything past [h, w] is 0."""
    n, c, h, w = bits.shape
    assert h <= rows and w <= 4 * row_bytes
    full = torch.zeros([n, c, rows, 4 * row_bytes], dtype=torch.int32)
    full[:, :, :h, :w] = bits.to(torch.int32)
    q = full.reshape(n, c, rows, row_bytes, 4)
    return (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).to(torch.uint8)


def unpack_signs(buf, h=None, w=None):
    """The inverse: uint8 [N, C, rows, row_bytes] -> bits [N, C, h, w] (default: every sample the buffer holds)."""
    n, c, rows, row_bytes = buf.shape
    b = buf.to(torch.int32)
    bits = torch.stack([(b >> (2 * q)) & 3 for q in range(4)], dim=-1).reshape(n, c, rows, 4 * row_bytes).to(torch.uint8)
    return bits[:, :, :rows if h is None else h, :4 * row_bytes if w is None else w]


def act_read(z, bits, sx=0, sy=0, gain=math.sqrt(2), slope=0.2, dtype=torch.float64):
    """The sign-read activation (float64 unless dtype says otherwise): sample (ty, tx) of z times the stored derivative of sample (ty + sy, tx + sx) of bits
    [N, C, bh, bw] -- gain, gain * slope where bit 0 is set, 0 where bit 1 is set, and gain outside the buffer."""
    n, c, h, w = z.shape
    bh, bw = bits.shape[2], bits.shape[3]
    ry = torch.arange(h) + sy
    rx = torch.arange(w) + sx
    inside = ((ry >= 0) & (ry < bh))[:, None] & ((rx >= 0) & (rx < bw))[None, :]
    got = bits[:, :, ry.clamp(0, bh - 1)][:, :, :, rx.clamp(0, bw - 1)].to(torch.int32) * inside.to(torch.int32)
    one = torch.ones([], dtype=torch.float64)
    d = torch.where((got & 1) > 0, one * (gain * slope), one * gain)
    d = torch.where((got & 2) > 0, one * 0.0, d).to(dtype)
    return z.to(dtype) * d
