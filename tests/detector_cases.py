"""Case tables, seeded inputs and float64 restatements for the detector path: the image preparation kernel (la_detector_prep_f32), the
fully connected kernel (la_fc_bias_act_f32) and detector op lists of the feature engine (conv, pool, fc).  Shared by
test_detector_cases_cpu.py (which proves, without a GPU, that the restatements equal torch's own F.interpolate, adaptive_avg_pool2d
and F.linear in float64, that the quantisation restatement equals torch's expression bit for bit, and that the FC cases reach both
sides of every predicate of the kernel's plan) and by test_hip_detector.py.  No GPU and no ctypes here; every input is synthetic and
seeded.  This module picks shapes; it never produces an expected value from the code under test.

The restatements are written with explicit bins, neighbours and sums, in any dtype: float64 is the answer, float32 sets the budget
    worst |hip - f64| <= 4 x worst |f32 - f64| + 2^-23 x max|f64|          (the K = 4 convention of test_hip_engine_shapes.py)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
K_F32 = 4.0

# (H, W, S): copy, integer ratio, non-integer ratios with overlapping bins, up-sampling, H != W, the loader's 40 -> 32
PREP_SIZES = [(8, 8, 8), (16, 16, 8), (9, 9, 6), (10, 10, 7), (7, 7, 10), (6, 10, 4), (40, 40, 32)]
PREP_MODES = ['area', 'bilinear']
PREP_CHANNELS = [1, 3]
PREP_N = 3
PREP_SCALE, PREP_SHIFT = (0.75, -1.25, 2.0), (0.5, 3.0, -0.125)


def worst(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def budget(ref32, ref64, k=K_F32):
    return k * worst(ref32, ref64) + EPS32 * float(torch.as_tensor(ref64).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# quantisation

def bin_edge_inputs():
    """the 765 float32 values at, and one ulp either side of, the 255 bin edges (k - 128) / 127.5, k = 1 .. 255"""
    e = (np.arange(1, 256, dtype=np.float64) - 128.0) / 127.5
    e = e.astype(np.float32)
    lo, hi = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
    return torch.from_numpy(np.stack([lo, e, hi], axis=1).reshape(-1).copy())


def quant_restate(x):
    """floor(clamp(x * 127.5 + 128, 0, 255)) with the product and the sum each rounded to float32 (numpy float32 scalars never
    fuse), as float32 integers"""
    v = x.detach().cpu().numpy().astype(np.float32)
    v = (v * np.float32(127.5)).astype(np.float32)
    v = (v + np.float32(128.0)).astype(np.float32)
    return torch.from_numpy(np.floor(np.clip(v, np.float32(0), np.float32(255))).astype(np.float32))


def quant_torch(x):
    """torch's own expression (metrics/metric_utils.py:316 of the reference)"""
    return (x * 127.5 + 128).clamp(0, 255).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# resampling

def area_bins(n_in, n_out):
    """[(lo, hi)] per output index: floor(i * in / out) .. ceil((i + 1) * in / out), in integers"""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def area_restate(x, S, dtype=torch.float64):
    """x [N][C][H][W] -> [N][C][S][S]: the sum over each bin, divided by its size"""
    x = x.to(dtype)
    H, W = x.shape[2:]
    by, bx = area_bins(H, S), area_bins(W, S)
    out = torch.empty(list(x.shape[:2]) + [S, S], dtype=dtype)
    for oy, (y0, y1) in enumerate(by):
        for ox, (x0, x1) in enumerate(bx):
            s = torch.zeros(x.shape[:2], dtype=dtype)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    s = s + x[:, :, yy, xx]
            out[:, :, oy, ox] = s / float((y1 - y0) * (x1 - x0))
    return out


def area_pow2_mask(H, W, S):
    """[S][S] bool: outputs whose bin holds a power-of-two number of pixels (the division is exact there)"""
    by, bx = area_bins(H, S), area_bins(W, S)
    m = torch.zeros([S, S], dtype=torch.bool)
    for oy, (y0, y1) in enumerate(by):
        for ox, (x0, x1) in enumerate(bx):
            n = (y1 - y0) * (x1 - x0)
            m[oy, ox] = (n & (n - 1)) == 0
    return m


def _lerp_axis(n_in, n_out, dtype):
    """(i0, i1, w0, w1) per output index for align_corners=False: src = (i + 0.5) * (in / out) - 0.5 clipped at 0, in `dtype`"""
    i = torch.arange(n_out, dtype=dtype)
    scale = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    src = ((i + 0.5) * scale - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    w1 = src - i0.to(dtype)
    return i0, i1, 1 - w1, w1


def bilinear_restate(x, S, dtype=torch.float64):
    x = x.to(dtype)
    H, W = x.shape[2:]
    y0, y1, wy0, wy1 = _lerp_axis(H, S, dtype)
    x0, x1, wx0, wx1 = _lerp_axis(W, S, dtype)
    top = x[:, :, y0][:, :, :, x0] * wx0 + x[:, :, y0][:, :, :, x1] * wx1
    bot = x[:, :, y1][:, :, :, x0] * wx0 + x[:, :, y1][:, :, :, x1] * wx1
    return top * wy0.reshape(-1, 1) + bot * wy1.reshape(-1, 1)


def prep_restate(img, S, mode, quantize, scale, shift, dtype=torch.float64):
    """the whole preparation: quantise (float32 by definition), repeat to 3 channels, resample, per-channel affine"""
    x = img.detach().cpu().float()
    if quantize:
        x = quant_restate(x)
    x = x.to(dtype)
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    if x.shape[2] != S or x.shape[3] != S:
        x = area_restate(x, S, dtype) if mode == 'area' else bilinear_restate(x, S, dtype)
    sc = torch.tensor(scale, dtype=torch.float32).to(dtype).reshape(1, 3, 1, 1)
    sh = torch.tensor(shift, dtype=torch.float32).to(dtype).reshape(1, 3, 1, 1)
    return x * sc + sh


def prep_inputs(C, H, W, seed=0, integers=False):
    g = torch.Generator().manual_seed(7000 + 100 * H + 10 * W + C + seed)
    if integers:
        return torch.randint(-8, 9, [PREP_N, C, H, W], generator=g).float()
    return torch.rand([PREP_N, C, H, W], generator=g) * 2 - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# fully connected kernel

FC_OT, FC_KC, FC_WG_TARGET, FC_KS_MAX, FC_MIN_CHUNKS = 128, 32, 768, 64, 4


def fc_plan(N, K, O):
    """host restatement of the kernel's tiling (la_fc_plan in la_detector_index.h): batch blocks and tiles, feature tiles, K chunks,
    chunks per slice, slices, 16-byte loads"""
    nb = 2 if N > 32 else 1
    ntiles = -(-N // (32 * nb))
    otiles = -(-O // FC_OT)
    nchunk = -(-K // FC_KC)
    ks = min(-(-FC_WG_TARGET // (ntiles * otiles)), FC_KS_MAX, max(nchunk // FC_MIN_CHUNKS, 1))
    ks = max(ks, 1)
    per = -(-nchunk // ks)
    ks = -(-nchunk // per)
    return dict(nb=nb, ntiles=ntiles, otiles=otiles, nchunk=nchunk, per=per, ks=ks, vec=K % 4 == 0,
                ragged_n=N % (32 * nb) != 0, ragged_k=K % FC_KC != 0, ragged_o=O % FC_OT != 0,
                ragged_slice=nchunk % per != 0)


def fc_workspace_bytes(N, K, O):
    ks1 = fc_plan(1, K, O)['ks']
    return 256 + (ks1 * N * O * 4 if ks1 > 1 else 0)


FC_N, FC_K, FC_O = (1, 5, 33, 64, 65), (4, 36, 100, 1568), (4, 6, 130)
# beyond the grid: K % 4 != 0 (scalar loads) with one slice and with several, a whole number of tiles in every direction
FC_EXTRA = [(5, 37, 6), (33, 230, 130), (64, 256, 128), (32, 1024, 256)]
FC_SHAPES = [(n, k, o) for n in FC_N for k in FC_K for o in FC_O] + FC_EXTRA
FC_REAL = dict(N=3, K=25088, O=4096)          # fc1 of the real net: slice counts and offsets of that size, small integers
FC_SHRINK = dict(K=1568, O=130, N_first=64, N_then=5)


def fc_inputs(N, K, O, seed=0, integers=False):
    g = torch.Generator().manual_seed(9000 + 131 * N + 17 * K + O + seed)
    if integers:
        # |sum| <= K * 1 * 2 + 8 < 2^24: every partial sum is an exact float32 whatever the order
        x = torch.randint(-1, 2, [N, K], generator=g).float()
        w = torch.randint(-2, 3, [O, K], generator=g).float()
        b = torch.randint(-8, 9, [O], generator=g).float()
        return x, w, b
    x = torch.randn([N, K], generator=g)
    w = torch.randn([O, K], generator=g) * (1.0 / K) ** 0.5
    b = torch.randn([O], generator=g) * 0.5
    return x, w, b


def fc_restate(x, w, b, relu, dtype=torch.float64):
    """act(sum_k x[n][k] w[o][k] + b[o])"""
    y = torch.matmul(x.to(dtype), w.to(dtype).t()) + b.to(dtype)
    return torch.where(y > 0, y, torch.zeros_like(y)) if relu else y


# ---------------------------------------------------------------------------------------------------------------------------------
# detector op lists

def detector_restate(ops, x, dtype=torch.float64):
    """ops: ('conv', w, b) | ('maxpool',) | ('avgpool',) | ('fc', w, b, relu); conv 3x3 pad 1 + bias + ReLU, 2x2 pools, NCHW flatten"""
    cur = x.detach().to(dtype)
    for op in ops:
        if op[0] == 'conv':
            a = F.conv2d(cur, op[1].to(dtype), op[2].to(dtype), padding=1)
            cur = torch.where(a > 0, a, torch.zeros_like(a))
        elif op[0] == 'maxpool':
            v = [cur[:, :, 0::2, 0::2], cur[:, :, 0::2, 1::2], cur[:, :, 1::2, 0::2], cur[:, :, 1::2, 1::2]]
            cur = torch.maximum(torch.maximum(v[0], v[1]), torch.maximum(v[2], v[3]))
        elif op[0] == 'avgpool':
            cur = 0.25 * ((cur[:, :, 0::2, 0::2] + cur[:, :, 0::2, 1::2]) + (cur[:, :, 1::2, 0::2] + cur[:, :, 1::2, 1::2]))
        elif op[0] == 'fc':
            cur = fc_restate(cur.reshape(cur.shape[0], -1), op[1], op[2], op[3], dtype)
        else:
            raise ValueError(op[0])
    return cur


class DetCase:
    """kinds: 'conv' | 'maxpool' | 'avgpool' | 'fc_relu' | 'fc'; widths: cout of every conv, fcs: outputs of every fc, in order"""

    def __init__(self, name, kinds, res, N, max_batch, widths, fcs, in_ch=3, seed=0):
        self.name, self.kinds, self.res, self.N, self.max_batch = name, kinds.split(','), res, N, max_batch
        self.widths, self.fcs, self.in_ch, self.seed = list(widths), list(fcs), in_ch, seed

    def build(self):
        g = torch.Generator().manual_seed(1000 * self.seed + 29)
        ops, c, r, wi, fi, flat = [], self.in_ch, self.res, 0, 0, None
        for k in self.kinds:
            if k == 'conv':
                co = self.widths[wi]
                wi += 1
                ops.append(('conv', torch.randn([co, c, 3, 3], generator=g) * (2.0 / (c * 9)) ** 0.5, torch.randn([co], generator=g) * 0.2 + 0.1))
                c = co
            elif k in ('fc_relu', 'fc'):
                kin = c * r * r if flat is None else flat
                o = self.fcs[fi]
                fi += 1
                ops.append(('fc', torch.randn([o, kin], generator=g) * (2.0 / kin) ** 0.5, torch.randn([o], generator=g) * 0.2 + 0.1, k == 'fc_relu'))
                flat = o
            else:
                ops.append((k,))
                r //= 2
        x = torch.randn([self.N, self.in_ch, self.res, self.res], generator=g) + 0.2
        return ops, x


# res 8, widths (8, 12): 12 channels at 2 x 2 = 48 -> 20 -> 12; N = 3 of max_batch 4
DET_CASES = [
    DetCase('vgg-like-relu', 'conv,maxpool,conv,maxpool,fc_relu,fc_relu', 8, 3, 4, (8, 12), (20, 12)),
    DetCase('linear-last', 'conv,maxpool,conv,maxpool,fc_relu,fc', 8, 3, 4, (8, 12), (20, 12), seed=1),
    DetCase('avgpool-one-fc', 'conv,avgpool,fc_relu', 8, 3, 4, (8,), (10,), seed=2),
]

# refusals at create: (name, ops as (kind code, cin, cout), in_ch, res, fragment of the message); codes as in the public header
CONV, TAP, MAXPOOL, AVGPOOL, FC_RELU, FC = 0, 1, 2, 3, 4, 5
DET_REFUSALS = [
    ('tap-then-fc', [(CONV, 3, 8), (TAP, 8, 8), (MAXPOOL, 8, 8), (FC_RELU, 8 * 16, 12)], 3, 8, 'taps and fc ops cannot be mixed'),
    ('fc-then-tap', [(CONV, 3, 8), (MAXPOOL, 8, 8), (FC_RELU, 8 * 16, 12), (TAP, 12, 12)], 3, 8, 'only fc ops may follow an fc op'),
    ('fc-cin-wrong', [(CONV, 3, 8), (MAXPOOL, 8, 8), (FC_RELU, 8 * 16 + 1, 12)], 3, 8, 'fc cin must be C*res*res'),
    ('fc-chain-cin-wrong', [(CONV, 3, 8), (MAXPOOL, 8, 8), (FC_RELU, 8 * 16, 12), (FC, 13, 4)], 3, 8, 'fc cin must be C*res*res'),
    ('fc-no-output', [(CONV, 3, 8), (FC, 8 * 64, 0)], 3, 8, 'at least one output'),
    ('conv-after-fc', [(FC_RELU, 3 * 64, 8), (CONV, 8, 8)], 3, 8, 'only fc ops may follow an fc op'),
]
