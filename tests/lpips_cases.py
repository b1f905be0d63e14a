"""Cases and torch-CPU restatement for the LPIPS distance (la_tap_pair_dist_kernel, la_feat_pair_distance, metrics.compute_lpips, the
LPIPS('vgg') branch of the plugin).  TEST INFRASTRUCTURE: runs in float64 (the anchor) or float32 (the yardstick), never on the GPU.

The restatement walks a FeatureEngine op list -- ('conv', w, b) = conv3x3 + bias + ReLU, ('maxpool',), ('avgpool',), ('tap', lin) --
and normalises a tapped activation either the reference's way, f / (sqrt(sum_c f^2) + 1e-10) (utils.py::normalize_activation;
`form='reference'`, pinned to the reference's own float64 run by tests/golden/lpips.npz), or the engine's way,
f * rsqrt(sum_c f^2 + 1e-10) (`form='engine'`: the contract of the tap kernels, used where the inputs are not conditioned to make
the two agree)."""
import numpy as np
import torch
import torch.nn.functional as F

# (C, R) of the tapped activation, kernel alone.  The first eight rows are the issue's table; the last four sit on both sides of the
# two register thresholds of the pair kernel at 4 channel groups (a thread's share of the channels: 32 | 33, 64 | 65 -> the 32-channel
# and 64-channel register forms and the re-reading form, whose 8-way unroll then has a tail of one).
KERNEL_CASES = [(1, 2), (3, 2), (5, 6), (33, 10), (31, 8), (32, 8), (64, 8), (520, 2), (128, 8), (132, 8), (256, 8), (260, 8)]
KERNEL_PAIRS = (1, 3)

CONV_IDS = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
TAPS = {'t3': (2, 3, 4), 't5': (0, 1, 2, 3, 4)}


def bound(ref64, yard):
    """The project's rule (test_hip_conv2d_op.py): 4 x the float32 yardstick's own error (max norm) + 2e-6 x the largest float64 magnitude."""
    ref64, yard = np.asarray(ref64, np.float64), np.asarray(yard, np.float64)
    return 4.0 * float(np.abs(yard - ref64).max()) + 2e-6 * float(np.abs(ref64).max())


def check(name, got, ref64, yard):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err, b = float(np.abs(got - ref64).max()), bound(ref64, yard)
    print(f'{name:40s} err {err:.3e}  bound {b:.3e}  scale {float(np.abs(ref64).max()):.3e}')
    assert np.isfinite(got).all(), name
    assert err <= b, (name, err, b)


def cast_ops(ops, dtype):
    return [(op[0],) + tuple(torch.as_tensor(t).to(dtype) for t in op[1:]) for op in ops]


def tapped(ops, x, form='reference'):
    """[(normalised activation [N, C, h, w], lin [C])] of every tap; x already carries the input affine."""
    out, t = [], x
    for op in ops:
        if op[0] == 'conv':
            t = F.relu(F.conv2d(t, op[1], op[2], padding=1))
        elif op[0] == 'maxpool':
            t = F.max_pool2d(t, 2)
        elif op[0] == 'avgpool':
            t = F.avg_pool2d(t, 2)
        elif op[0] == 'tap':
            s = t.square().sum(1, keepdim=True)
            out.append((t / (s.sqrt() + 1e-10) if form == 'reference' else t * torch.rsqrt(s + 1e-10), op[1]))
        else:
            raise ValueError(op[0])
    return out


def pair_distance(ops, x, y, form='reference'):
    """[P, ntaps]: per tap, mean over pixels of sum_c lin_c (nx - ny)^2 (lpips.py:49-58 for N = 1, layer by layer)."""
    cols = [((fx - fy).square() * lin.reshape(1, -1, 1, 1)).sum(1).mean((1, 2)) for (fx, lin), (fy, _) in zip(tapped(ops, x, form), tapped(ops, y, form))]
    return torch.stack(cols, dim=1)


def distance_of_rows(tl, ia, ib):
    """pair_distance from the `tapped` list of one batch: rows ia[p] against rows ib[p] -> [P, ntaps]."""
    return torch.stack([((f[ia] - f[ib]).square() * lin.reshape(1, -1, 1, 1)).sum(1).mean((1, 2)) for f, lin in tl], dim=1)


def affine(x, scale, shift):
    """x_k * float32(scale_k) + float32(shift_k): the input affine as the crop kernel is handed it."""
    sc = torch.tensor(np.float32(scale).astype(np.float64)).to(x.dtype).reshape(1, 3, 1, 1)
    sh = torch.tensor(np.float32(shift).astype(np.float64)).to(x.dtype).reshape(1, 3, 1, 1)
    return x * sc + sh


def feature_vector(ops, x, form='reference'):
    """[N, F]: what the engine's taps write, n * sqrt(lin) / sqrt(HW) -- squared L2 of two rows is sum_t pair_distance[., t]."""
    return torch.cat([(f * lin.reshape(1, -1, 1, 1).sqrt() / (f.shape[2] * f.shape[3]) ** 0.5).flatten(1) for f, lin in tapped(ops, x, form)], dim=1)


def forward_tr(ops, x, bank, form='reference'):
    """lpips.py:60-68 for x [1, 3, R, R] against a bank [M, 3, R, R]: sum_m d(x, bank_m) / M."""
    return pair_distance(ops, x.expand(bank.shape[0], -1, -1, -1), bank, form).sum() / bank.shape[0]


def zscore(x, mean, std):
    return (x - torch.as_tensor(mean).to(x.dtype).reshape(1, 3, 1, 1)) / torch.as_tensor(std).to(x.dtype).reshape(1, 3, 1, 1)


def golden_state_dicts(gl, tag):
    """(vgg state dict, lin state dict in the LPIPS weight file's names) of the fixture's narrow net; `tag`: 't3' | 't5'.  The lin file
    always holds five tensors, as the published one does."""
    vgg = {f'features.{i}.{p}': torch.tensor(gl[f'features.{i}.{p}']) for i in CONV_IDS for p in ('weight', 'bias')}
    lin = {f'lin{k}.model.1.weight': torch.tensor(gl[f'lin{k}']).reshape(1, -1, 1, 1) for k in range(5)}
    return vgg, lin


def golden_ops(gl, tag):
    """The fixture's net as a FeatureEngine op list, built by hand (independent of synthesis.vgg16_lpips_ops)."""
    ops = []
    for i in CONV_IDS:
        ops.append(('conv', torch.tensor(gl[f'features.{i}.weight']), torch.tensor(gl[f'features.{i}.bias'])))
        place = {2: 0, 7: 1, 14: 2, 21: 3, 28: 4}.get(i)
        if place in TAPS[tag]:
            ops.append(('tap', torch.tensor(gl[f'lin{place}'])))
        if i in (2, 7, 14, 21):
            ops.append(('maxpool',))
    return ops


def kernel_inputs(C, R, P, seed=0):
    """Tapped activations as a ReLU leaves them (about half the values exactly 0, whole pixels 0 at small C) and non-negative lin
    weights (a sum of mixed signs would cancel and leave the bound's scale below the terms; the sign has a test of its own).  With more than one pair the first is close, like an augmented image and its source."""
    g = torch.Generator().manual_seed(1000 * C + 10 * R + P + seed)
    x = torch.randn([P, C, R, R], generator=g, dtype=torch.float64).clamp_min(0)
    y = torch.randn([P, C, R, R], generator=g, dtype=torch.float64).clamp_min(0)
    if P > 1:
        y[0] = (x[0] + 1e-3 * torch.randn([C, R, R], generator=g, dtype=torch.float64)).clamp_min(0)
    lin = torch.randn([C], generator=g, dtype=torch.float64).abs()
    # (values that float32 holds exactly, so that the float64 anchor and the GPU start from the same numbers)
    return x.float().double(), y.float().double(), lin.float().double()
