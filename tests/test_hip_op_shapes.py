"""Sweep of the op layer's public entries (bias_act, upfirdn2d, filter2d, upsample2d, downsample2d) over the shapes at which their kernels
change form -- workgroup-tile seams, ragged work-item counts, both sides of every host-side dispatch predicate, the plane and grid-stride
loops, unequal x / y factors, every filter extent -- in float16, float32 and float64, each against the oracle (oracle/sg2_ops.py) run on
the CPU in float64.  Every case checks the forward and the input gradient (bias_act: also db, and the second order for swish), output
shape and dtype.  Inputs come from a seeded CPU generator; a float16 (float32) case rounds x, b, dy to its dtype first and the oracle gets
those rounded values widened, so input rounding is part of no error.  Each group of cases says which kernel form it reaches, read from
the predicates in la_upfirdn2d.hip (fir_launch_inner), la_ops.hip (fir_h_mode, fir_op_launch, la_bias_act_op_kernel).

Tolerances (none tuned to the kernels):
  float64   |err| <= 1e-12 x max(1, max |expected|)                                             (test_hip_op_dtypes.py)
  float32   |err| <= 1e-5 x |expected| + 1e-5 x max(1, max |expected|), element by element      (test_hip_ops.py)
  float16   one launch (2-D filters forward, their dx = one launch of the same op on a float16 dy, bias_act forward and gradients -- one
            fp32 evaluation from the saved float16 tensors, one rounding):  |err| <= ulp16(expected) + 1e-7 x max |expected|
  float16   separable filters, two launches with a float16 intermediate t: the oracle is restated as pass 1 (x axis, gain sqrt(g)) ->
            t rounded to float16 -> pass 2 (y axis, gain sqrt(g)), the backward as the adjoint of pass 2 -> rounded to float16 -> the
            adjoint of pass 1.  The kernel's intermediate is within the one-launch bound of the unrounded t, hence at most one float16
            step (ulp16(max |t|)) from the restated rounded one; pass 2 is linear with taps sqrt(g) f[k], so that difference reaches an
            output multiplied by at most sqrt(g) x sum |f[k]|.  Allowed: the one-launch bound + sqrt(g) x sum|f| x ulp16(max |t|).
  kinks     float16 bias_act gradients leave out the elements of _kink_mask (test_hip_op_dtypes.py, imported as it is); their share is
            asserted below 2 % from the float64 oracle alone.  float32 gradients leave out elements whose clamp test float32 cannot
            decide: the unclamped |y| within 4 float32 steps of the clamp (same 2 % assertion; normally none).
  db        sums dx: float32 / float64 as above; float16 accumulates the float16 dx in fp32 and rounds once, so it is allowed the sum over
            its channel of the per-element dx bound, one float16 step of the result, and |dx| of the left-out elements (the slack rule of
            test_hip_op_dtypes.py).
  bit for bit: an unaligned but contiguous input (storage offset of one element) gives the aligned call's result exactly (torch.equal).

Measured on one MI355X: the whole file (660 cases) takes 10 s, most of it the CPU float64 oracle.
"""
import ast
import math
import os

import numpy as np
import pytest
import torch

from oracle import sg2_ops as O
from test_hip_op_dtypes import F16_EPS32, _kink_mask, ulp16

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.float32, torch.float64]
DT_ID = {torch.float16: 'f16', torch.float32: 'f32', torch.float64: 'f64'}
dtypes = pytest.mark.parametrize('dtype', DTYPES, ids=[DT_ID[d] for d in DTYPES])
EPS32 = 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


# ---------------------------------------------------------------- helpers
def _draw(shape, g, dtype, scale=1.0):
    """Seeded CPU draw, as the dtype under test holds it (float64 cases draw in float64)."""
    if dtype == torch.float64:
        return torch.randn(shape, generator=g, dtype=torch.float64) * scale
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(got, exp, dtype, what, extra=0.0, keep=None):
    """got (device tensor) against exp (float64 numpy) under the module's bound for dtype; extra widens the float16 bound (a derived
    amount, see the module docstring); keep = boolean mask of the elements that are compared."""
    assert got.dtype == dtype, (what, got.dtype)
    assert tuple(got.shape) == exp.shape, (what, tuple(got.shape), exp.shape)
    if exp.size == 0:
        return
    err = np.abs(_np(got) - exp)
    top = float(np.abs(exp).max())
    if dtype == torch.float64:
        tol = np.full(exp.shape, 1e-12 * max(1.0, top))
    elif dtype == torch.float32:
        tol = 1e-5 * np.abs(exp) + 1e-5 * max(1.0, top)
    else:
        tol = ulp16(exp) + F16_EPS32 * top + extra
    bad = err > tol
    if keep is not None:
        bad &= keep
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err - tol, -np.inf))), exp.shape)
        raise AssertionError((what, 'elements over the bound', int(bad.sum()), 'of', exp.size, 'worst at', i, 'err', float(err[i]),
                              'tol', float(tol[i]), 'expected', float(exp[i])))


def _unaligned(t, dev):
    """The values of t in a contiguous device tensor whose data pointer is one element past a 16-byte boundary."""
    base = torch.empty([t.numel() + 1], device=dev, dtype=t.dtype)
    u = base[1:].view(t.shape)
    u.copy_(t)
    assert u.is_contiguous() and u.data_ptr() % 16 != 0
    return u.detach()


def _fir_oracle(opname, x64, f, kw, dy_of, half_intermediate):
    """(y, dx, dy, extra_y, extra_dx) of the oracle in float64; dy_of(y) supplies the (already rounded) dy.  half_intermediate: the two-pass
    restatement with float16 intermediates (module docstring), only for upfirdn2d with a 1-D filter."""
    x64 = x64.clone().requires_grad_(True)
    if not half_intermediate:
        y = getattr(O, opname)(x64, f, **kw)
        dy = dy_of(y.detach())
        (dx,) = torch.autograd.grad(y, [x64], dy.double())
        return y.detach(), dx, dy, 0.0, 0.0
    assert opname == 'upfirdn2d' and f.ndim == 1
    (upx, upy), (dnx, dny) = O._xy(kw.get('up', 1)), O._xy(kw.get('down', 1))
    px0, px1, py0, py1 = O._pad4(kw.get('padding', 0))
    flip, sg = kw.get('flip_filter', False), float(kw.get('gain', 1)) ** 0.5
    t = O.upfirdn2d(x64, f[None, :], up=(upx, 1), down=(dnx, 1), padding=[px0, px1, 0, 0], flip_filter=flip, gain=sg)
    t16 = t.detach().half().double().requires_grad_(True)
    y = O.upfirdn2d(t16, f[:, None], up=(1, upy), down=(1, dny), padding=[0, 0, py0, py1], flip_filter=flip, gain=sg)
    dy = dy_of(y.detach())
    (gt,) = torch.autograd.grad(y, [t16], dy.double())
    (dx,) = torch.autograd.grad(t, [x64], gt.half().double())
    amp = sg * float(f.abs().sum())
    return y.detach(), dx, dy, amp * float(ulp16(float(t.detach().abs().max()))), amp * float(ulp16(float(gt.abs().max())))


def _run_fir(dev, dtype, opname, f, shape, kw, seed, also_unaligned=False):
    """One upfirdn2d-family case: forward and dx of the HIP op against the float64 oracle; returns (y, dx) of the HIP op."""
    from latentaugment_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = _draw(shape, g, dtype)
    two_pass16 = dtype == torch.float16 and f.ndim == 1
    ey, edx, dy, extra_y, extra_dx = _fir_oracle(opname, x.double(), f, kw, lambda y: _draw(y.shape, g, dtype), two_pass16)
    xd = x.to(dev).requires_grad_(True)
    y = getattr(ops, opname)(xd, f, **kw)
    (dx,) = torch.autograd.grad(y, [xd], dy.to(dev))
    what = (opname, DT_ID[dtype], tuple(shape), tuple(f.shape), kw)
    _check(y, ey.numpy(), dtype, what + ('y',), extra_y)
    _check(dx, edx.numpy(), dtype, what + ('dx',), extra_dx)
    if also_unaligned:
        xu = _unaligned(x.to(dev), dev).requires_grad_(True)
        yu = getattr(ops, opname)(xu, f, **kw)
        (dxu,) = torch.autograd.grad(yu, [xu], dy.to(dev))
        assert torch.equal(yu, y) and torch.equal(dxu, dx), what + ('unaligned input differs from the aligned call',)
        _check(yu, ey.numpy(), dtype, what + ('y, unaligned',), extra_y)
    return y, dx


def _f1331():
    from latentaugment_amd import ops
    return ops.setup_filter([1, 3, 3, 1])


def _seed(*parts):
    """A seed that depends on the case (stable across runs and processes)."""
    s = 0
    for c in repr(parts):
        s = (s * 131 + ord(c)) % 1000003
    return s


# ---------------------------------------------------------------- upfirdn2d family, [1,3,3,1] x [1,3,3,1] (the 4x4 fast forms)
# Stride 1.  float32: la_fir4x4_s1_kernel for EVERY pad (fir_launch_inner: up = down = 1 and 4x4 taps is the whole predicate), workgroup
# tile 64 columns x 32 rows (4 waves x FIR_ROWS = 8).  float16: la_fir4x4_h_kernel<0, padx0> iff Win % 8 == 0, Wout % 8 == 0, padx0 in
# {1, 2} and aligned pointers (fir_h_mode) -- of the sizes below filter2d at W = 64 and 200; everything else, and float64 always,
# runs la_upfirdn2d_op_kernel (tile 64 x 4).
S1_SIZES = [(37, 131), (64, 64), (65, 129), (33, 200)]
S1_CALLS = [('filter2d', {}), ('upfirdn2d', {'padding': [1, 1, 1, 1]}), ('upfirdn2d', {'padding': [2, 2, 2, 2]})]


@dtypes
@pytest.mark.parametrize('hw', S1_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('call', S1_CALLS, ids=['filter2d', 'pad1', 'pad2'])
def test_stride1_tile_seams(dev, dtype, hw, call):
    _run_fir(dev, dtype, call[0], _f1331(), [1, 3, *hw], call[1], _seed('s1', hw, call))


# Free pads through the same stride-1 forms: unequal, zero, negative (crop) and Wout > Win.  float16 at 40x72 (Win % 8 == 0): [2,9,2,1]
# gives Wout = 80 -> la_fir4x4_h_kernel<0, 2> with output columns beyond the input's; the other three have Wout = 73, 71, 72 with
# padx0 = -1 -> generic.  41x70: Win % 8 != 0 -> generic.
S1_PADS = [[1, 3, 0, 2], [2, 0, 1, 1], [-1, 3, -2, 4], [2, 9, 2, 1]]


@dtypes
@pytest.mark.parametrize('hw', [(40, 72), (41, 70)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('pad', S1_PADS, ids=lambda p: 'pad' + '_'.join(str(v) for v in p).replace('-', 'm'))
def test_stride1_free_pads(dev, dtype, hw, pad):
    _run_fir(dev, dtype, 'upfirdn2d', _f1331(), [2, 2, *hw], {'padding': pad}, _seed('s1pad', hw, pad))


# upsample2d.  float32: la_fir4x4_up2_kernel iff Wout % 4 == 0 (W even): W = 64 (32 items per row), 66 (33: rows do not fill waves
# evenly, items straddle rows), 136; W = 65 -> Wout = 130 -> la_upfirdn2d_kernel.  float16: la_fir4x4_h_kernel<1, 2> iff W % 8 == 0
# (64, 136), else generic.  float64: generic.
@dtypes
@pytest.mark.parametrize('h', [5, 33, 64])
@pytest.mark.parametrize('w', [64, 66, 65, 136])
def test_upsample2d_fast_path_and_fallback(dev, dtype, h, w):
    _run_fir(dev, dtype, 'upsample2d', _f1331(), [2, 3, h, w], {}, _seed('up2', h, w))


# downsample2d.  float32: la_fir4x4_down2_kernel iff Wout % 2 == 0 and Hin, Win even: W = 128, 132; W = 130, 66 -> Wout = 65, 33 ->
# generic.  float16: la_fir4x4_h_kernel<2, 1> iff Win % 8 == 0 and Wout % 8 == 0 (128 only; 132 -> Win % 8 != 0), else generic.
@dtypes
@pytest.mark.parametrize('h', [6, 34, 64])
@pytest.mark.parametrize('w', [128, 132, 130, 66])
def test_downsample2d_fast_path_and_fallback(dev, dtype, h, w):
    _run_fir(dev, dtype, 'downsample2d', _f1331(), [2, 3, h, w], {}, _seed('down2', h, w))


# fir_h_mode from both sides (float16; the other dtypes run the same cases on their own forms).  Win % 8: 8, 16, 24, 64, 72 take the
# float16 4x4 forms (downsample2d also needs Wout % 8: 16, 64 only), 12, 20, 60 the generic kernel.
@dtypes
@pytest.mark.parametrize('w', [8, 16, 24, 64, 72, 12, 20, 60])
@pytest.mark.parametrize('opname', ['filter2d', 'upsample2d', 'downsample2d'])
def test_float16_width_predicate_both_sides(dev, dtype, opname, w):
    _run_fir(dev, dtype, opname, _f1331(), [2, 2, 10, w], {}, _seed('w8', opname, w))


# W = 64: [2,1,2,1] is filter2d's (mode 0); [2,2,2,1] breaks Wout % 8 by padx1 (65 -> generic); [1,2,1,2] is mode 0 with PADX = 1;
# [2,1,1,2] and [1,2,2,1] are padx0 = 2 with pady0 = 1 and the reverse (mode 0 takes any pady0); [1,2,-3,5] a cropping pady0 in mode 0;
# [3,0,2,1] has Wout % 8 == 0 but padx0 = 3 -> generic.
H_PADS = [[2, 1, 2, 1], [2, 2, 2, 1], [1, 2, 1, 2], [2, 1, 1, 2], [1, 2, 2, 1], [1, 2, -3, 5], [3, 0, 2, 1]]


@dtypes
@pytest.mark.parametrize('pad', H_PADS, ids=lambda p: 'pad' + '_'.join(str(v) for v in p).replace('-', 'm'))
def test_float16_pad_predicate_both_sides(dev, dtype, pad):
    _run_fir(dev, dtype, 'upfirdn2d', _f1331(), [2, 2, 13, 64], {'padding': pad}, _seed('hpad', pad))


# An unaligned but contiguous input: float16 leaves all three la_fir4x4_h_kernel modes for the generic kernel, float32's
# la_fir4x4_down2_kernel leaves its 16-byte row loads for dword loads; the result is the aligned call's bit for bit (same taps, same
# accumulation order in every form) and meets the oracle bound.
@dtypes
@pytest.mark.parametrize('opname', ['filter2d', 'upsample2d', 'downsample2d'])
def test_unaligned_contiguous_input_equals_aligned(dev, dtype, opname):
    _run_fir(dev, dtype, opname, _f1331(), [2, 3, 10, 64], {}, _seed('unal', opname), also_unaligned=True)


# Plane loops.  P = 4500 / 4200 is above the grid-z cap of la_fir4x4_s1_kernel (4096: float32 filter2d) and of the generic kernels
# (1024: float64 everything); float32 upsample2d / downsample2d and float16 at W = 8 run the flat work-item kernels, where the plane
# is a quotient of the item index.  [2, 600, 5, 12] (P = 1200, Win % 8 != 0) takes float16 to the generic kernel's loop as well.
@dtypes
@pytest.mark.parametrize('shape', [[5, 900, 8, 8], [3, 1400, 4, 8], [2, 600, 5, 12]], ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('opname', ['filter2d', 'upsample2d', 'downsample2d'])
def test_plane_loop(dev, dtype, opname, shape):
    if opname == 'downsample2d' and shape[2] % 2:
        shape = shape[:2] + [shape[2] + 1, shape[3]]      # (an even height keeps float32 on la_fir4x4_down2_kernel)
    _run_fir(dev, dtype, opname, _f1331(), shape, {}, _seed('planes', opname, shape))


@dtypes
def test_plane_loop_generic_3x3(dev, dtype):
    """3x3 taps: the generic kernel in every dtype, P = 1400 above its grid-z cap of 1024."""
    from latentaugment_amd import ops
    _run_fir(dev, dtype, 'upfirdn2d', ops.setup_filter([1, 2, 1]), [2, 700, 9, 7], {'padding': 1}, _seed('planes3x3'))


@dtypes
@pytest.mark.parametrize('opname', ['upsample2d', 'downsample2d', 'filter2d'])
def test_at_size_against_oracle(dev, dtype, opname):
    """[2, 8, 256, 256]: the fast forms of each dtype at many tiles per plane, against float64 (not HIP against HIP)."""
    _run_fir(dev, dtype, opname, _f1331(), [2, 8, 256, 256], {}, _seed('size', opname))


# ---------------------------------------------------------------- upfirdn2d, generic kernel
def _shape_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, 'op_shapes.npz'))
    return g, [ast.literal_eval(str(r)) for r in g['cases']]


# The argument sets of op_shapes.npz (unequal x / y factors, dense 3x5 / 1x4 / 4x1 / 2x7 filters, unequal and negative pads, flip, gains
# 1.7 / 0.6 / 2.3 / 0.37) at planes that cross a 64-column and a 4-row tile in every case.  All generic (la_upfirdn2d_kernel /
# la_upfirdn2d_op_kernel) except u5 = 4x4 stride 1, which float32 runs on la_fir4x4_s1_kernel.
@dtypes
@pytest.mark.parametrize('hw', [(70, 150), (33, 129)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('k', range(9))
def test_unequal_factors_at_tile_crossing_planes(dev, golden_dir, dtype, hw, k):
    g, cases = _shape_cases(golden_dir)
    name, _, op, kwrep = cases[k]
    assert name == f'u{k}'
    _run_fir(dev, dtype, op, torch.tensor(g[f'{name}_f']), [1, 2, *hw], ast.literal_eval(kwrep), _seed('uneq', hw, k))


def _dense(fh, fw):
    from latentaugment_amd import ops
    return ops.setup_filter((torch.arange(fh * fw, dtype=torch.float32).reshape(fh, fw) % 7 + 1 + torch.arange(fw) * 0.5).tolist())


def _sep(n):
    from latentaugment_amd import ops
    return ops.setup_filter(list(np.hanning(n + 2)[1:-1] + 0.05 * np.arange(n) / n), separable=True)


FILTERS = {'d8x8': lambda: _dense(8, 8), 'd1x8': lambda: _dense(1, 8), 'd8x1': lambda: _dense(8, 1), 'd5x3': lambda: _dense(5, 3),
           'sep8': lambda: _sep(8), 'sep12': lambda: _sep(12), 'sep32': lambda: _sep(32)}
# (up, down, input width): with pads p0 + p1 = P the output width is (Win up + P - fw + down) // down
FACTORS = {'up2': (2, 1, 30), 'down2': (1, 2, 125), 'up4down2': (4, 2, 32)}


def _extent_case(fname, facname, wout):
    f = FILTERS[fname]()
    fh, fw = (f.shape[0], f.shape[0]) if f.ndim == 1 else tuple(f.shape)
    up, down, win = FACTORS[facname]
    p = wout * down - down + fw - win * up      # the smallest total pad with that output width
    px0 = p // 2
    kw = {'up': up, 'down': down, 'padding': [px0, p - px0, fh // 2, fh // 2 + 1], 'gain': up * up}
    assert (win * up + p - fw + down) // down == wout
    return f, [1, 3, 9, win], kw


# Filter extents on the generic kernel (every dtype): dense 8x8 (the 64-tap limit), 1x8, 8x1, 5x3; separable 8, 12 and 32 taps (two
# launches of 1 x n / n x 1 taps).  Output widths 63, 64, 65 sit on either side of the 64-column tile; the up4down2 cases need a negative
# (cropping) pad for the short filters.
@dtypes
@pytest.mark.parametrize('wout', [63, 64, 65])
@pytest.mark.parametrize('facname', list(FACTORS))
@pytest.mark.parametrize('fname', list(FILTERS))
def test_filter_extents(dev, dtype, fname, facname, wout):
    f, shape, kw = _extent_case(fname, facname, wout)
    y, _ = _run_fir(dev, dtype, 'upfirdn2d', f, shape, kw, _seed('ext', fname, facname, wout))
    assert y.shape[3] == wout


# Smallest legal outputs: padded size equal to the filter (1x1 output), one input row, one input column, a 1x1 plane upsampled.
SMALL = [('upfirdn2d', [2, 3, 4, 4], {}), ('upfirdn2d', [2, 3, 2, 3], {'padding': [1, 0, 0, 2]}), ('upfirdn2d', [2, 3, 1, 9], {'padding': [1, 2, 2, 1]}),
         ('upfirdn2d', [2, 3, 9, 1], {'padding': [2, 1, 1, 2]}), ('upsample2d', [2, 3, 1, 1], {}), ('downsample2d', [2, 3, 2, 2], {}),
         ('filter2d', [2, 3, 1, 1], {}), ('upfirdn2d', [1, 1, 1, 1], {'up': (4, 1), 'down': (1, 1), 'padding': [0, 0, 2, 1]})]


@dtypes
@pytest.mark.parametrize('k', range(len(SMALL)))
def test_smallest_legal_outputs(dev, dtype, k):
    opname, shape, kw = SMALL[k]
    y, _ = _run_fir(dev, dtype, opname, _f1331(), shape, kw, _seed('small', k))
    if k < 2:
        assert tuple(y.shape[2:]) == (1, 1)


# ---------------------------------------------------------------- the reference's own vectors (op_shapes.npz) through the HIP ops
@dtypes
def test_reference_vectors_upfirdn2d(dev, golden_dir, dtype):
    """float64: against the arrays the reference wrote.  float16 / float32: the same arguments and (rounded) inputs against the oracle,
    which test_op_shapes_cpu.py pins to those arrays."""
    from latentaugment_amd import ops
    g, cases = _shape_cases(golden_dir)
    n = 0
    for name, _, op, kwrep in cases:
        if not name.startswith('u'):
            continue
        n += 1
        f, kw = torch.tensor(g[f'{name}_f']), ast.literal_eval(kwrep)
        x, dy = torch.tensor(g[f'{name}_x']).to(dtype), torch.tensor(g[f'{name}_dy']).to(dtype)
        if dtype == torch.float64:
            ey, edx = g[f'{name}_y'], g[f'{name}_dx']
        else:
            ey, edx, _, _, _ = _fir_oracle(op, x.double(), f, kw, lambda y: dy, False)
            ey, edx = ey.numpy(), edx.numpy()
        xd = x.to(dev).requires_grad_(True)
        y = getattr(ops, op)(xd, f, **kw)
        (dx,) = torch.autograd.grad(y, [xd], dy.to(dev))
        _check(y, ey, dtype, (name, kw, 'y'))
        _check(dx, edx, dtype, (name, kw, 'dx'))
    assert n == 9


def test_float64_gain_rounds_to_float32_with_the_taps(dev, golden_dir):
    """Regression, found by this sweep: the reference multiplies the float32 filter tensor by the gain BEFORE widening it to the dtype of x
    (upfirdn2d.py:196-197), so in float64 a gain that is not a power of two acts rounded to float32.  The float64 entry multiplied in
    double and was 4e-8 (relative) away from the reference at gain 1.7 -- far outside the 1e-12 bound, unseen because every float64
    fixture had gain 1 or 4.  The gains of op_shapes.npz are 1.7, 0.6, 2.3, 0.37; also through upsample2d (gain x 4) on separable taps,
    where each pass takes sqrt(gain) in float32."""
    from latentaugment_amd import ops
    g, cases = _shape_cases(golden_dir)
    seen = []
    for name, _, op, kwrep in cases:
        kw = ast.literal_eval(kwrep) if name.startswith('u') else {}
        if kw.get('gain', 1) in (1, 2, 4):
            continue
        seen.append(kw['gain'])
        y = getattr(ops, op)(torch.tensor(g[f'{name}_x'], device=dev), torch.tensor(g[f'{name}_f']), **kw)
        _check(y, g[f'{name}_y'], torch.float64, (name, kw, 'y against the reference'))
    assert sorted(seen) == [0.37, 0.6, 1.7, 2.3]
    _run_fir(dev, torch.float64, 'upsample2d', _sep(8), [1, 2, 9, 11], {'gain': 1.7}, _seed('gain-sep'))


# ---------------------------------------------------------------- bias_act
ACTS = [('lrelu', {'clamp': 0.75}), ('swish', {}), ('linear', {})]
acts = pytest.mark.parametrize('act', ACTS, ids=[a for a, _ in ACTS])


def _bias_oracle(x64, b64, dim, act, kw, dy64, ddx64):
    x64 = x64.clone().requires_grad_(True)
    ins = [x64]
    if b64 is not None:
        b64 = b64.clone().requires_grad_(True)
        ins.append(b64)
    y = O.bias_act(x64, b64, dim=dim, act=act, **kw)
    grads = torch.autograd.grad(y, ins, dy64, create_graph=ddx64 is not None)
    d2 = torch.autograd.grad(grads[0], [x64], ddx64)[0] if ddx64 is not None else None
    return y.detach(), grads[0].detach(), (grads[1].detach() if b64 is not None else None), d2


def _run_bias_act(dev, dtype, shape, dim, act, kw, seed, has_b=True, also_unaligned=False, scale=1.0):
    from latentaugment_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = _draw(shape, g, dtype, scale)
    b = _draw([shape[dim]], g, dtype) if has_b else None
    dy = _draw(shape, g, dtype)
    second = act == 'swish'                     # (the activation of the three that has a second derivative)
    ddx = _draw(shape, g, dtype) if second else None
    ey, edx, edb, ed2 = _bias_oracle(x.double(), None if b is None else b.double(), dim, act, kw, dy.double(), None if ddx is None else ddx.double())
    ey, edx = ey.numpy(), edx.numpy()
    what = ('bias_act', DT_ID[dtype], tuple(shape), 'dim', dim, act, kw)

    # elements whose gradient the dtype's rounding may legitimately flip (module docstring), from float64 values alone
    bshape = [1] * len(shape)
    bshape[dim] = -1
    v = x.double().numpy() + (0.0 if b is None else b.double().numpy().reshape(bshape))
    excl = np.zeros(v.shape, bool)
    if dtype == torch.float16:
        excl = _kink_mask(act, kw, v, ey)
    elif dtype == torch.float32 and kw.get('clamp') is not None:
        # (x + b is one correctly rounded float32 addition, so its sign is exact; only the clamp test can fall the other way)
        pre = O.bias_act(x.double(), None if b is None else b.double(), dim=dim, act=act, **{k: w for k, w in kw.items() if k != 'clamp'})
        excl = np.abs(np.abs(pre.numpy()) - kw['clamp']) <= 4 * EPS32 * kw['clamp']
    assert excl.mean() < 0.02, what + ('kink share', float(excl.mean()))

    def run(xin):
        xd = xin.requires_grad_(True)
        bd = None if b is None else b.to(dev).requires_grad_(True)
        ins = [xd] if bd is None else [xd, bd]
        y = ops.bias_act(xd, bd, dim=dim, act=act, **kw)
        grads = torch.autograd.grad(y, ins, dy.to(dev), create_graph=second)
        d2 = torch.autograd.grad(grads[0], [xd], ddx.to(dev))[0] if second else None
        return y.detach(), grads[0].detach(), (grads[1].detach() if bd is not None else None), d2

    y, dx, db, d2 = run(x.to(dev))
    _check(y, ey, dtype, what + ('y',))
    _check(dx, edx, dtype, what + ('dx',), keep=~excl)
    if second:
        _check(d2, ed2.numpy(), dtype, what + ('d2',), keep=~excl)
    if db is not None:
        edb = edb.numpy()
        axes = tuple(i for i in range(len(shape)) if i != dim)
        slack = (np.abs(edx) * excl).sum(axis=axes)
        assert db.dtype == dtype and tuple(db.shape) == edb.shape, what + ('db',)
        err = np.abs(_np(db) - edb)
        top = float(np.abs(edb).max())
        if dtype == torch.float64:
            tol = 1e-12 * max(1.0, top) + slack
        elif dtype == torch.float32:
            tol = 1e-5 * np.abs(edb) + 1e-5 * max(1.0, top) + slack
        else:
            tol = (ulp16(edx) + F16_EPS32 * float(np.abs(edx).max())).sum(axis=axes) + ulp16(edb) + slack
        assert (err <= tol).all(), what + ('db', float((err - tol).max()), float(err.max()))
    if also_unaligned:
        yu, dxu, dbu, d2u = run(_unaligned(x.to(dev), dev))
        assert torch.equal(yu, y) and torch.equal(dxu, dx), what + ('unaligned input differs from the aligned call',)
        assert (db is None or torch.equal(dbu, db)) and (d2 is None or torch.equal(d2u, d2)), what + ('unaligned: db / d2',)
        _check(yu, ey, dtype, what + ('y, unaligned',))


# Per-element bias branch of la_bias_act_op_kernel (stepb % V != 0; V = 8 halves / 4 floats / 2 doubles) and its scalar tail
# (numel % V != 0).  stepb = 21, 9, 25; [13] has no bias (stepb = nb = 1).
@dtypes
@acts
@pytest.mark.parametrize('shape', [[3, 5, 7, 3], [2, 7, 1, 9], [1, 3, 5, 5], [13]], ids=lambda s: 'x'.join(str(v) for v in s))
def test_bias_act_per_element_bias_and_tail(dev, dtype, act, shape):
    assert math.prod(shape) % 16 != 0
    has_b = len(shape) > 1
    _run_bias_act(dev, dtype, shape, 1 if has_b else 0, act[0], act[1], _seed('ragged', shape, act[0]), has_b=has_b)


# The bias axis: dim = 0 (stepb 240, one entry per group), 2 (stepb 8: one entry per float16 group), 3 (stepb 1) on [4, 6, 5, 8]; the FC
# layout [64, 1000] with dim = 1 (stepb 1, nb 1000: every element its own entry) and dim = 0 (stepb 1000); nb = 1.
AXES = [([4, 6, 5, 8], 0), ([4, 6, 5, 8], 2), ([4, 6, 5, 8], 3), ([64, 1000], 1), ([64, 1000], 0), ([3, 1, 5, 7], 1)]


@dtypes
@acts
@pytest.mark.parametrize('case', AXES, ids=lambda c: 'x'.join(str(v) for v in c[0]) + f'-dim{c[1]}')
def test_bias_act_bias_axis(dev, dtype, act, case):
    _run_bias_act(dev, dtype, case[0], case[1], act[0], act[1], _seed('axis', case, act[0]))


# x one element past a 16-byte boundary: p.vec == 0 in the forward (x), the first-order launch (xref / yref) and the second-order one.
@dtypes
@acts
@pytest.mark.parametrize('shape', [[3, 5, 7, 3], [2, 6, 4, 8]], ids=lambda s: 'x'.join(str(v) for v in s))
def test_bias_act_unaligned_contiguous_input_equals_aligned(dev, dtype, act, shape):
    _run_bias_act(dev, dtype, shape, 1, act[0], act[1], _seed('unal-ba', shape, act[0]), also_unaligned=True)


# Just above one sweep of the grid (8192 workgroups x 256 work items x V elements, V = 8 / 1 / 2), stepb not a multiple of V, numel odd:
# group index, bias index and tail beyond the first sweep.
GRID_STRIDE = {torch.float16: ([3, 1331, 4203], 'lrelu', {'clamp': 0.75}), torch.float32: ([3, 131, 5337], 'swish', {}),
               torch.float64: ([3, 131, 10673], 'lrelu', {'clamp': 0.75})}


@dtypes
def test_bias_act_grid_stride_loop(dev, dtype):
    shape, act, kw = GRID_STRIDE[dtype]
    v = {torch.float16: 8, torch.float32: 1, torch.float64: 2}[dtype]
    n = math.prod(shape)
    assert 8192 * 256 * v < n < 8192 * 256 * v * 1.01 and n % 2 == 1 and shape[2] % 2 == 1      # (odd stepb: no multiple of V = 8, 2)
    _run_bias_act(dev, dtype, shape, 1, act, kw, _seed('stride', shape))


@dtypes
def test_reference_vectors_bias_act(dev, golden_dir, dtype):
    """op_shapes.npz's bias_act cases (dim = 0, 2, 3 on 4-D, dim = 1 on 2-D): float64 against the reference's arrays, float16 / float32
    against the oracle on the rounded inputs."""
    from latentaugment_amd import ops
    g, cases = _shape_cases(golden_dir)
    n = 0
    for name, act, dim, kwrep in cases:
        if not name.startswith('b'):
            continue
        n += 1
        kw = ast.literal_eval(kwrep)
        x, b, dy = (torch.tensor(g[f'{name}_{k}']).to(dtype) for k in ('x', 'b', 'dy'))
        if dtype == torch.float64:
            ey, edx, edb = g[f'{name}_y'], g[f'{name}_dx'], g[f'{name}_db']
        else:
            ey, edx, edb, _ = (None if t is None else t.numpy() for t in _bias_oracle(x.double(), b.double(), dim, act, kw, dy.double(), None))
        xd, bd = x.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        y = ops.bias_act(xd, bd, dim=dim, act=act, **kw)
        dx, db = torch.autograd.grad(y, [xd, bd], dy.to(dev))
        bshape = [1] * x.ndim
        bshape[dim] = -1
        excl = _kink_mask(act, kw, x.detach().double().numpy() + b.detach().double().numpy().reshape(bshape), ey) if dtype == torch.float16 else np.zeros(ey.shape, bool)
        assert excl.mean() < 0.02
        _check(y, ey, dtype, (name, act, dim, 'y'))
        _check(dx, edx, dtype, (name, act, dim, 'dx'), keep=~excl)
        if dtype != torch.float16:      # (float16 db: the derived bound of _run_bias_act, on the cases above)
            _check(db, edb, dtype, (name, act, dim, 'db'))
    assert n == 5


@pytest.mark.parametrize('dtype', [torch.float16, torch.float64], ids=['f16', 'f64'])
def test_bias_act_empty_and_unknown_activation(dev, dtype):
    """The float16 / float64 twins of test_bias_act_ragged_and_empty's empty-tensor and KeyError lines."""
    from latentaugment_amd import ops
    x = torch.randn([3, 5, 7, 3], device=dev).to(dtype)
    b = torch.randn([5], device=dev).to(dtype)
    e = torch.empty([0, 5, 4, 4], device=dev, dtype=dtype)
    y = ops.bias_act(e, b)
    assert y.shape == (0, 5, 4, 4) and y.dtype == dtype
    with pytest.raises(KeyError):
        ops.bias_act(x, b, act='gelu')
