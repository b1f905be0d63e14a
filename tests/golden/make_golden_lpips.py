#!/usr/bin/env python3
"""Generate tests/golden/lpips.npz by RUNNING THE REFERENCE's LPIPS class on the CPU.

Run from the repo root:   python tests/golden/make_golden_lpips.py      (needs /root/reference, read-only)

Executed from the reference (imported, never copied): augments/criteria/lpips/lpips.py::LPIPS (forward, forward_tr,
extract_features) with networks.py::BaseNet (z-score, tapped walk over `layers`) and LinLayers, utils.py::normalize_activation.
Shims: `torchvision` and `utils.util_reports` are not installed / not needed and are stubbed in sys.modules, and the `augments`
package is entered without its __init__ (which imports the whole plugin).  LPIPS is built with __new__: its __init__ downloads
torchvision's VGG16 and the lin weights and moves everything to cuda.  It is handed a narrow VGG16-shaped nn.Sequential of our
own -- torchvision's `features` layout (13 conv3x3 + ReLU, 5 max-pools at the same indices) with widths 4, 8, 16, 32, 32,
He-scaled random weights -- and random non-negative lin weights; inputs are 32 x 32.

Recorded, in float32 and in float64, for the reference's three taps (target_layers [16, 23, 30]) and for the five-tap list
([4, 9, 16, 23, 30]):  forward(x, y) of every pair (N = 1 calls), the same with the class restricted to one tap at a time (the
per-layer values), forward_tr(x, feat) against per-layer banks and its autograd gradient with respect to x; plus weights, lins,
the z-score buffers and the inputs.  For the plugin test: forward_tr of the three-tap net on the 16 x 16 crop that the toy
generator of the GPU tests produces at step 0 (this repository's CPU oracle of it), per modality, against 16 x 16 banks.

Condition asserted here: the smallest channel norm over every tapped pixel of every input is >= 0.03.  The reference divides by
sqrt(sum) + 1e-10, the engine multiplies by rsqrt(sum + 1e-10); above that norm the two differ by less than float32 resolution.
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
ut = types.ModuleType('utils')
ut.util_reports = types.ModuleType('utils.util_reports')
pkg = types.ModuleType('augments')
pkg.__path__ = [os.path.join(REF, 'augments')]
sys.modules.update({'torchvision': tv, 'torchvision.models': tv.models, 'utils': ut, 'utils.util_reports': ut.util_reports,
                    'augments': pkg})

from augments.criteria.lpips.lpips import LPIPS  # noqa: E402
from augments.criteria.lpips.networks import BaseNet, LinLayers  # noqa: E402

WIDTHS = (4, 8, 16, 32, 32)
BLOCKS = (2, 2, 3, 3, 3)                       # convs per block: torchvision's vgg16 `features`
TAP_LAYERS = {'t3': [16, 23, 30], 't5': [4, 9, 16, 23, 30]}
MIN_NORM = 0.03
PLUG_M, PLUG_POS = 5, (1, 2)


def make_layers(g):
    layers, cin = [], 3
    for width, n in zip(WIDTHS, BLOCKS):
        for _ in range(n):
            conv = nn.Conv2d(cin, width, 3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * 9)) ** 0.5)
                conv.bias.copy_(torch.rand(conv.bias.shape, generator=g) * 0.2 + 0.05)
            layers += [conv, nn.ReLU(inplace=False)]
            cin = width
        layers.append(nn.MaxPool2d(2, 2))
    return nn.Sequential(*layers)


def make_lpips(layers, target_layers, lins, dtype):
    """The reference's LPIPS around `layers`, without its downloading __init__."""
    net = BaseNet()
    net.layers = copy.deepcopy(layers)
    net.target_layers = list(target_layers)
    net.n_channels_list = [int(v.numel()) for v in lins]
    net.report_dir = None
    net.set_requires_grad(False)
    lp = LPIPS.__new__(LPIPS)
    nn.Module.__init__(lp)
    lp.net = net
    lp.lin = LinLayers(net.n_channels_list)
    with torch.no_grad():
        for seq, v in zip(lp.lin, lins):
            seq[1].weight.copy_(v.reshape(1, -1, 1, 1))
    lp.target_layers = net.target_layers
    return lp.to(dtype).eval()


def _raw_norms(lp, x):
    """Smallest channel norm of the RAW tapped activations (the walk of BaseNet.forward, before normalize_activation)."""
    t, lo = lp.net.z_score(x), float('inf')
    with torch.no_grad():
        for i, (_, layer) in enumerate(lp.net.layers._modules.items(), 1):
            t = layer(t)
            if i in lp.net.target_layers:
                lo = min(lo, float(t.square().sum(1).sqrt().min()))
            if i >= max(lp.net.target_layers):
                break
    return lo


def record(tag, layers, lins, x, y, x1, bank, out):
    """x, y [P, 3, R, R] pairs; x1 [1, 3, R, R] against bank [M, 3, R, R]."""
    tl = TAP_LAYERS[tag]
    for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
        lp = make_lpips(layers, tl, lins, dtype)
        xs, ys, x1s, banks = (t.to(dtype) for t in (x, y, x1, bank))
        lo = min(_raw_norms(lp, t) for t in (xs, ys, x1s, banks))
        assert lo >= MIN_NORM, f'{tag}: smallest channel norm {lo:.4f} < {MIN_NORM}: choose another seed'
        with torch.no_grad():
            total = torch.stack([lp.forward(xs[p:p + 1], ys[p:p + 1]) for p in range(x.shape[0])])
            per_layer = torch.empty([x.shape[0], len(tl)], dtype=dtype)
            for k, layer_id in enumerate(tl):
                one = make_lpips(layers, [layer_id], [lins[k]], dtype)
                for p in range(x.shape[0]):
                    per_layer[p, k] = one.forward(xs[p:p + 1], ys[p:p + 1])
            feat = lp.extract_features(banks)
        xg = x1s.clone().requires_grad_(True)
        tr = lp.forward_tr(xg, feat)
        (grad,) = torch.autograd.grad(tr, [xg])
        out.update({f'{tag}_pair{sfx}': total.numpy(), f'{tag}_layers{sfx}': per_layer.numpy(), f'{tag}_tr{sfx}': tr.detach().numpy(),
                    f'{tag}_tr_grad{sfx}': grad.numpy()})
        print(tag, sfx, 'min norm', f'{lo:.4f}', 'pairs', total.numpy(), 'forward_tr', float(tr))
    return lo


def record_plugin(layers, lins, banks, out):
    """The criterion of the reference's LPIPS('vgg') branch at step 0 of the toy loop the GPU tests run (tiny generator of
    tests/golden/latent_loop.npz, first sample of its w0, batch 1): calc_loss_lpips_tr (util_latent_aug.py:411-424) is forward_tr of
    each modality's crop against that modality's bank; recorded per modality, the generator being this repository's CPU oracle."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import latent_aug_ref as lar
    from oracle import sg2_networks as nets
    gl = np.load(os.path.join(HERE, 'latent_loop.npz'))
    res = int(gl['res'])
    for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
        G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=int(gl['cbase']), channel_max=int(gl['cmax']), seed=0,
                                noise_strength=0.1, w_dim=int(gl['wdim']), mapping_layers=2)
        nets.COMPUTE_DTYPE = dtype
        try:
            G = G.to(dtype)
            ws = torch.tensor(gl['w0'])[:1].to(dtype).repeat(1, G.num_ws, 1)
            with torch.no_grad():
                img = G.synthesis(ws, noise_mode='const', fused_modconv=dtype == torch.float32)
        finally:
            nets.COMPUTE_DTYPE = torch.float32
        crop = lar.apply_aug_transform(img, res, 16, 'center_random_crop', PLUG_POS)
        lp = make_lpips(layers, TAP_LAYERS['t3'], lins, dtype)
        vals = []
        for mode in range(2):
            x3 = crop[:, mode:mode + 1].repeat(1, 3, 1, 1)
            bank = banks[mode].to(dtype)
            lo = min(_raw_norms(lp, x3), _raw_norms(lp, bank))
            assert lo >= MIN_NORM, f'plugin case: smallest channel norm {lo:.4f} < {MIN_NORM}'
            with torch.no_grad():
                vals.append(float(lp.forward_tr(x3, lp.extract_features(bank))))
        out[f'plug_tr{sfx}'] = np.asarray(vals, dtype=np.float64)
        print('plugin', sfx, vals)
    out['plug_pos'] = np.asarray(PLUG_POS, dtype=np.int64)


def gray3(g, n, res):
    """n single-channel images in [-1, 1], repeated to three channels the way the criterion feeds the net."""
    return (torch.rand([n, 1, res, res], generator=g) * 2 - 1).repeat(1, 3, 1, 1)


def main():
    for seed in range(50):
        g = torch.Generator().manual_seed(seed)
        layers = make_layers(g)
        lins5 = [torch.rand([w], generator=g) for w in WIDTHS]
        x, y, x1, bank = gray3(g, 3, 32), gray3(g, 3, 32), gray3(g, 1, 32), gray3(g, 4, 32)
        y[0] = x[0] + 0.01 * (y[0] - x[0])          # a close pair: what an augmented image is to its source
        pbank = gray3(g, 2 * PLUG_M, 16)              # plugin case: a bank of PLUG_M crops per modality
        probe = make_lpips(layers, TAP_LAYERS['t5'], lins5, torch.float64)
        lo = min(_raw_norms(probe, t.double()) for t in (x, y, x1, bank, pbank))
        print('seed', seed, 'smallest channel norm', f'{lo:.4f}')
        if lo >= MIN_NORM:
            break
    else:
        raise SystemExit('no seed met the channel-norm condition')
    out = {'seed': np.int64(seed), 'x': x[:, :1].numpy(), 'y': y[:, :1].numpy(), 'x1': x1[:, :1].numpy(), 'bank': bank[:, :1].numpy(),
           'plug_bank': pbank[:, :1].reshape(2, PLUG_M, 1, 16, 16).numpy(), 'min_norm': np.float64(lo),
           'mean': probe.net.mean.reshape(3).float().numpy(), 'std': probe.net.std.reshape(3).float().numpy()}
    for k, v in layers.state_dict().items():
        out['features.' + k] = v.numpy()
    for k, v in enumerate(lins5):
        out[f'lin{k}'] = v.numpy()
    record('t3', layers, lins5[2:], x, y, x1, bank, out)
    record('t5', layers, lins5, x, y, x1, bank, out)
    record_plugin(layers, lins5[2:], pbank.reshape(2, PLUG_M, 3, 16, 16), out)
    path = os.path.join(HERE, 'lpips.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
