"""Cases and torch-CPU restatement for the LPIPS nets on AlexNet and SqueezeNet 1.1 trunks (la_feat_conv.hip, the general ops of the
feature engine).  TEST INFRASTRUCTURE: runs in float64 (the anchor) or float32 (the yardstick), never on the GPU.

The restatement walks a FeatureEngine op list with the general ops -- ('conv', w, b, stride, pad), ('maxpool3', ceil_mode),
('fire', sq_w, sq_b, e1_w, e1_b, e3_w, e3_b) -- beside those of lpips_cases.tapped, with the same two normalisation forms."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_cases as lc

ALEX_CONVS = (0, 3, 6, 8, 10)
ALEX_GEOM = {0: (4, 2), 3: (1, 2), 6: (1, 1), 8: (1, 1), 10: (1, 1)}
ALEX_FULL = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))
SQUEEZE_FIRES = (3, 4, 6, 7, 9, 10, 11, 12)
SQUEEZE_POOLS = (2, 5, 8)
SQUEEZE_TAP_AFTER = (1, 4, 7, 9, 10, 11, 12)
SQUEEZE_FULL = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128), 9: (256, 48, 192, 192),
                10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}
SIZES = {'alex': (35, 67), 'squeeze': (17, 34)}
MIN_RES = {'alex': 31, 'squeeze': 17}
NTAPS = {'alex': 5, 'squeeze': 7}
PLUGIN = {'squeeze': (32, 18), 'alex': (64, 32)}

# (cin, cout, k, stride, pad, R, N) of the conv kernel alone
CONV_CASES = [(3, 8, 11, 4, 2, 35, 2), (3, 8, 11, 4, 2, 37, 1), (3, 64, 11, 4, 2, 31, 1), (8, 12, 5, 1, 2, 8, 3), (64, 192, 5, 1, 2, 7, 2),
              (3, 16, 3, 2, 0, 17, 2), (3, 16, 3, 2, 0, 18, 1), (16, 4, 1, 1, 0, 5, 3), (192, 384, 3, 1, 1, 1, 1), (384, 256, 3, 1, 1, 3, 2)]
POOL_RES = (3, 4, 5, 7, 8, 15, 16)
FIRE_CASES = [(16, 4, 16, 16), (128, 16, 64, 64)]


def cast_ops(ops, dtype):
    return [(op[0],) + tuple(t.to(dtype) if torch.is_tensor(t) else t for t in op[1:]) for op in ops]


def tapped(ops, x, form='reference'):
    """[(normalised activation [N, C, h, w], lin [C])] of every tap; x already carries the input affine."""
    out, t = [], x
    for op in ops:
        if op[0] == 'conv' and len(op) == 5:
            t = F.relu(F.conv2d(t, op[1], op[2], stride=op[3], padding=op[4]))
        elif op[0] == 'conv':
            t = F.relu(F.conv2d(t, op[1], op[2], padding=1))
        elif op[0] == 'maxpool3':
            t = F.max_pool2d(t, 3, 2, ceil_mode=bool(op[1]))
        elif op[0] == 'maxpool':
            t = F.max_pool2d(t, 2)
        elif op[0] == 'fire':
            s = F.relu(F.conv2d(t, op[1], op[2]))
            t = torch.cat([F.relu(F.conv2d(s, op[3], op[4])), F.relu(F.conv2d(s, op[5], op[6], padding=1))], 1)
        elif op[0] == 'tap':
            s = t.square().sum(1, keepdim=True)
            out.append((t / (s.sqrt() + 1e-10) if form == 'reference' else t * torch.rsqrt(s + 1e-10), op[1]))
        else:
            raise ValueError(op[0])
    return out


def pair_distance(ops, x, y, form='reference'):
    cols = [((fx - fy).square() * lin.reshape(1, -1, 1, 1)).sum(1).mean((1, 2)) for (fx, lin), (fy, _) in zip(tapped(ops, x, form), tapped(ops, y, form))]
    return torch.stack(cols, dim=1)


def feature_vector(ops, x, form='reference'):
    return torch.cat([(f * lin.reshape(1, -1, 1, 1).sqrt() / (f.shape[2] * f.shape[3]) ** 0.5).flatten(1) for f, lin in tapped(ops, x, form)], dim=1)


def forward_tr(ops, x, bank, form='reference'):
    return pair_distance(ops, x.expand(bank.shape[0], -1, -1, -1), bank, form).sum() / bank.shape[0]


def golden_state_dicts(gn, net):
    """(trunk state dict in torchvision's names, lin state dict in the LPIPS weight file's names) of the fixture's narrow net."""
    pre = f'{net}.features.'
    trunk = {'features.' + k[len(pre):]: torch.tensor(gn[k]) for k in gn.files if k.startswith(pre)}
    lin = {f'lin{k}.model.1.weight': torch.tensor(gn[f'{net}.lin{k}']).reshape(1, -1, 1, 1) for k in range(NTAPS[net])}
    return trunk, lin


def golden_ops(gn, net):
    """The fixture's net as a FeatureEngine op list, built by hand (independent of the builders in synthesis.py)."""
    trunk, lin = golden_state_dicts(gn, net)
    lins = [lin[f'lin{k}.model.1.weight'].reshape(-1) for k in range(NTAPS[net])]
    ops = []
    if net == 'alex':
        for t, i in enumerate(ALEX_CONVS):
            ops += [('conv', trunk[f'features.{i}.weight'], trunk[f'features.{i}.bias'], *ALEX_GEOM[i]), ('tap', lins[t])]
            if i in (0, 3):
                ops.append(('maxpool3', False))
        return ops
    ops += [('conv', trunk['features.0.weight'], trunk['features.0.bias'], 2, 0), ('tap', lins[0])]
    for i in range(2, 13):
        if i in SQUEEZE_POOLS:
            ops.append(('maxpool3', True))
        else:
            ops.append(('fire',) + tuple(trunk[f'features.{i}.{p}.{w}'] for p in ('squeeze', 'expand1x1', 'expand3x3') for w in ('weight', 'bias')))
        if i in SQUEEZE_TAP_AFTER:
            ops.append(('tap', lins[SQUEEZE_TAP_AFTER.index(i)]))
    return ops


def _he(g, shape):
    fan = shape[1] * shape[2] * shape[3]
    return (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5).float().double()


def _bias(g, n):
    return (torch.rand([n], generator=g, dtype=torch.float64) * 0.3 + 0.3).float().double()


def full_width_state_dicts(net, seed=0):
    """Seeded He-scaled float64 weights (values float32 holds) at the real channel tables, in torchvision's names, and lin weights."""
    g = torch.Generator().manual_seed(seed)
    sd, chans = {}, []
    if net == 'alex':
        for i, (cin, cout, k) in zip(ALEX_CONVS, ALEX_FULL):
            sd[f'features.{i}.weight'], sd[f'features.{i}.bias'] = _he(g, [cout, cin, k, k]), _bias(g, cout)
            chans.append(cout)
    else:
        sd['features.0.weight'], sd['features.0.bias'] = _he(g, [64, 3, 3, 3]), _bias(g, 64)
        chans.append(64)
        for i in SQUEEZE_FIRES:
            cin, sq, e1, e3 = SQUEEZE_FULL[i]
            for part, shape in (('squeeze', [sq, cin, 1, 1]), ('expand1x1', [e1, sq, 1, 1]), ('expand3x3', [e3, sq, 3, 3])):
                sd[f'features.{i}.{part}.weight'], sd[f'features.{i}.{part}.bias'] = _he(g, shape), _bias(g, shape[0])
            if i in SQUEEZE_TAP_AFTER:
                chans.append(e1 + e3)
    lin = {f'lin{k}.model.1.weight': torch.rand([1, c, 1, 1], generator=g, dtype=torch.float64).float().double() for k, c in enumerate(chans)}
    return sd, lin


def small_ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def gray3(a, dtype=torch.float64):
    return torch.as_tensor(a).to(dtype).repeat(1, 3, 1, 1)


def fed(net_desc, a, dtype=torch.float64):
    """[n, 1, R, R] fixture images as the net's input: repeated to three channels with the net's affine."""
    return lc.affine(gray3(a, dtype), net_desc.pre_scale, net_desc.pre_shift)


bound, check = lc.bound, lc.check      # the project's rule, imported and not edited
