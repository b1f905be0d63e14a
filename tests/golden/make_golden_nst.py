#!/usr/bin/env python3
"""Generate tests/golden/nst.npz by RUNNING THE REFERENCE's NSTLoss and VGG19Net on the CPU.

Run from the repo root:   python tests/golden/make_golden_nst.py      (needs /root/reference, read-only)

Executed from the reference (imported, never copied): augments/criteria/nst/nst.py::NSTLoss (gram_matrix, _style_loss, _content_loss,
forward) and networks.py::VGG19Net (prepare_img with synthetic=True, normalize=True; the tapped walk of forward).  Shims: `torchvision`
is not installed and is stubbed in sys.modules, the `augments` package is entered without its __init__ (which imports the whole
plugin), and VGG19Net is built with __new__: its __init__ downloads torchvision's VGG19.  It is handed a narrow nn.Sequential of our own
in the layout of torchvision's vgg19().features -- 16 conv3x3 + ReLU(inplace=True), 5 max pools, 37 modules -- with widths 8, 12, 16,
20, 20 per block, He-scaled weights and biases uniform in [0.3, 0.6].  The in-place ReLUs matter: the tensors VGG19Net.forward keeps at
the conv indices 0, 5, 10, 19, 28 are overwritten by the ReLU behind each, so what NSTLoss sees are relu1_1 .. relu5_1 (asserted
below: the minimum of every tapped tensor is exactly 0).

Recorded per input size R (32: the last tap is 2 x 2, 48: 3 x 3), in float32 and float64: NSTLoss(batch_size=1) style and content of
three pairs of [3, 2, R, R] images in [-1, 1], per pair, modality and tap (one tap at a time, so `style` is that tap's and `content`
is taken at every tap; the reference's own content tap is index 3) -> `nst{R}_style32/64`, `nst{R}_content32/64` [3, 2, 5]; the
inputs `nst{R}_x`, `nst{R}_y` (pair 0 is close: y = x + 0.01 (y' - x); some values lie above 127 / 127.5, where prepare_img's
clamp(0, 255) acts -- asserted) and the weights `features.{i}.weight/bias`.

Condition asserted, searched over up to 50 input seeds per size (the seed is recorded): the reference's own float32 result lies
within 1e-4 of the float64 result's maximum, entry by entry relative to the largest entry of its tap: no ReLU or pool argmax flip
between the two precisions dominates the yardstick.
"""
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, REF)
tv = types.ModuleType('torchvision')
tv.models = types.ModuleType('torchvision.models')
pkg = types.ModuleType('augments')
pkg.__path__ = [os.path.join(REF, 'augments')]
sys.modules.update({'torchvision': tv, 'torchvision.models': tv.models, 'augments': pkg})

from augments.criteria.nst.networks import VGG19Net  # noqa: E402
from augments.criteria.nst.nst import NSTLoss  # noqa: E402

WIDTHS = (8, 12, 16, 20, 20)
BLOCKS = (2, 2, 4, 4, 4)            # convs per block of vgg19
SIZES = (32, 48)
TAPS = ('0', '5', '10', '19', '28')
F32_TOL, SEEDS = 1e-4, 50


def make_features(g):
    seq, c = [], 3
    for width, n in zip(WIDTHS, BLOCKS):
        for _ in range(n):
            seq += [nn.Conv2d(c, width, 3, padding=1), nn.ReLU(inplace=True)]
            c = width
        seq.append(nn.MaxPool2d(2, 2))
    net = nn.Sequential(*seq)
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            fan = m.weight.shape[1] * 9
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.3 + 0.3)
    assert len(net) == 37 and all(isinstance(net[int(i)], nn.Conv2d) for i in TAPS)
    return net.eval().requires_grad_(False)


def make_vgg19net(features, dtype):
    """The reference's VGG19Net around `features`, without its downloading __init__."""
    net = VGG19Net.__new__(VGG19Net)
    nn.Module.__init__(net)
    net.cnn = copy.deepcopy(features).to(dtype)
    net.content_layers, net.style_layers = ['19'], list(TAPS)
    return net


def record(features, x, y):
    """style, content [P, 2, 5] in both precisions."""
    out = {}
    for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
        net = make_vgg19net(features, dtype)
        P = x.shape[0]
        style, content = np.zeros([P, 2, 5], np.float64), np.zeros([P, 2, 5], np.float64)
        for p in range(P):
            for mode in range(2):
                with torch.no_grad():
                    fx, _ = net(x[p:p + 1].to(dtype), mode_dict={'mode_idx': mode}, synthetic=True, normalize=True)
                    fy, _ = net(y[p:p + 1].to(dtype), mode_dict={'mode_idx': mode}, synthetic=True, normalize=True)
                    assert len(fx) == 5 and all(float(f.min()) == 0.0 for f in fx + fy)      # post-ReLU: see the docstring
                    for t in range(5):
                        loss = NSTLoss(batch_size=1)
                        loss([fx[t]], [fx[t]], [fy[t]], [fy[t]])
                        assert loss.style_loss.dtype == dtype
                        style[p, mode, t], content[p, mode, t] = float(loss.style_loss), float(loss.content_loss)
        out['style' + sfx], out['content' + sfx] = style, content
    return out


def main():
    g = torch.Generator().manual_seed(1900)
    features = make_features(g)
    out = {}
    for R in SIZES:
        for seed in range(SEEDS):
            gi = torch.Generator().manual_seed(seed)
            x, y = torch.rand([3, 2, R, R], generator=gi) * 2 - 1, torch.rand([3, 2, R, R], generator=gi) * 2 - 1
            y[0] = x[0] + 0.01 * (y[0] - x[0])
            nclamp = int((x > 127 / 127.5).sum() + (y > 127 / 127.5).sum())
            assert nclamp > 0 and float(x.abs().max()) <= 1.0 and float(y.abs().max()) <= 1.0
            case = record(features, x, y)
            worst = 0.0
            for k in ('style', 'content'):
                a32, a64 = case[k + '32'], case[k + '64']
                worst = max(worst, float((np.abs(a32 - a64) / np.abs(a64).max(axis=(0, 1), keepdims=True)).max()))
            print(f'R {R} inputs {seed}: clamped values {nclamp}, float32 error relative to the tap maximum {worst:.2e}')
            if worst <= F32_TOL:
                out.update({f'nst{R}_{k}': v for k, v in case.items()})
                out.update({f'nst{R}_x': x.numpy(), f'nst{R}_y': y.numpy(), f'nst{R}_seed': np.int64(seed), f'nst{R}_f32_err': np.float64(worst)})
                break
        else:
            raise SystemExit(f'R = {R}: no seed met the condition')
    for k, v in features.state_dict().items():
        out[f'features.{k}'] = v.numpy()
    path = os.path.join(HERE, 'nst.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
