#!/usr/bin/env python3
"""Generate tests/golden/lpips_nets.npz by RUNNING THE REFERENCE's LPIPS class on the CPU around AlexNet- and SqueezeNet-1.1-shaped trunks.

Run from the repo root:   python tests/golden/make_golden_lpips_nets.py      (needs /root/reference, read-only)

Executed from the reference (imported, never copied), with the shims of make_golden_lpips.py: lpips.py::LPIPS (forward, forward_tr,
extract_features), networks.py::BaseNet (z-score, tapped walk over `layers`) and LinLayers, utils.py::normalize_activation.  The class
is handed narrow nn.Sequentials of our own in torchvision's `features` layouts:
  alex     conv 11x11 s4 p2, pool 3/2, conv 5x5 p2, pool 3/2, three conv 3x3 p1, pool 3/2; widths 8, 12, 16, 12, 12;
           target_layers [2, 5, 8, 10, 12] (networks.py:81)
  squeeze  conv 3x3 s2, ceil-mode pools at 2, 5, 8, Fire modules at 3, 4, 6, 7, 9, 10, 11, 12 at torchvision's widths / 4 (torchvision
           is not installed: the Fire module is a small nn.Module here); target_layers [2, 5, 8, 10, 11, 12, 13] (networks.py:70)
Weights He-scaled, biases uniform in [0.3, 0.6], lin weights uniform in [0, 1).

Recorded per net and input size (alex 35 and 67, squeeze 17 and 34), in float32 and float64: forward(x, y) of three pairs (N = 1
calls; the first pair is close, y = x + 0.01 (y - x)), the same per tap, forward_tr of one image against a bank of four and its autograd
gradient; plus weights, lins and inputs.  Plugin cases: forward_tr per modality of the step-0 crop of this repository's CPU oracle of
the toy generator (squeeze: resolution 32, crop 18; alex: resolution 64, crop 32) against banks of crops.

Conditions asserted, searched over up to 50 seeds per case (the seed is recorded):
  (i)  every tapped pixel's channel norm is >= 0.03, so the reference's x / (sqrt + 1e-10) and the engine's x * rsqrt(sum + 1e-10)
       agree to float32 resolution;
  (ii) the reference's own float32 gradient lies within 1e-5 of the float64 gradient's maximum: no ReLU or pool argmax flips between
       the two precisions.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_lpips as base  # noqa: E402  (installs the sys.modules shims and imports the reference's classes)

ALEX_WIDTHS = (8, 12, 16, 12, 12)
SQUEEZE_CONV = 16
SQUEEZE_FIRES = {3: (4, 16, 16), 4: (4, 16, 16), 6: (8, 32, 32), 7: (8, 32, 32), 9: (12, 48, 48), 10: (12, 48, 48), 11: (16, 64, 64), 12: (16, 64, 64)}
TARGETS = {'alex': [2, 5, 8, 10, 12], 'squeeze': [2, 5, 8, 10, 11, 12, 13]}
SIZES = {'alex': (35, 67), 'squeeze': (17, 34)}
PLUGIN = {'squeeze': (32, 18), 'alex': (64, 32)}      # net -> (toy resolution, crop)
MIN_NORM, GRAD_TOL, SEEDS = 0.03, 1e-5, 50
PLUG_M, PLUG_POS = 4, (1, 2)


class Fire(nn.Module):
    def __init__(self, cin, sq, e1, e3):
        super().__init__()
        self.squeeze, self.expand1x1, self.expand3x3 = nn.Conv2d(cin, sq, 1), nn.Conv2d(sq, e1, 1), nn.Conv2d(sq, e3, 3, padding=1)

    def forward(self, x):
        s = torch.relu(self.squeeze(x))
        return torch.cat([torch.relu(self.expand1x1(s)), torch.relu(self.expand3x3(s))], 1)


def _init(module, g):
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.3 + 0.3)
    return module


def make_layers(net, g):
    if net == 'alex':
        w = ALEX_WIDTHS
        seq = [nn.Conv2d(3, w[0], 11, 4, 2), nn.ReLU(), nn.MaxPool2d(3, 2), nn.Conv2d(w[0], w[1], 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
               nn.Conv2d(w[1], w[2], 3, padding=1), nn.ReLU(), nn.Conv2d(w[2], w[3], 3, padding=1), nn.ReLU(),
               nn.Conv2d(w[3], w[4], 3, padding=1), nn.ReLU(), nn.MaxPool2d(3, 2)]
        return _init(nn.Sequential(*seq), g), list(w)
    seq, c, chans = [nn.Conv2d(3, SQUEEZE_CONV, 3, 2), nn.ReLU()], SQUEEZE_CONV, [SQUEEZE_CONV]
    for i in range(2, 13):
        if i in SQUEEZE_FIRES:
            sq, e1, e3 = SQUEEZE_FIRES[i]
            seq.append(Fire(c, sq, e1, e3))
            c = e1 + e3
        else:
            seq.append(nn.MaxPool2d(3, 2, ceil_mode=True))
        if i + 1 in TARGETS['squeeze']:
            chans.append(c)
    return _init(nn.Sequential(*seq), g), chans


def record(net, R, layers, lins, x, y, x1, bank, out):
    """Both precisions of one case; returns (smallest channel norm, float32 gradient error / float64 gradient maximum)."""
    tl, grads, lo_all = TARGETS[net], {}, float('inf')
    for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
        lp = base.make_lpips(layers, tl, lins, dtype)
        xs, ys, x1s, banks = (t.to(dtype) for t in (x, y, x1, bank))
        lo_all = min([lo_all] + [base._raw_norms(lp, t) for t in (xs, ys, x1s, banks)])
        with torch.no_grad():
            total = torch.stack([lp.forward(xs[p:p + 1], ys[p:p + 1]) for p in range(x.shape[0])])
            per_layer = torch.empty([x.shape[0], len(tl)], dtype=dtype)
            for k, layer_id in enumerate(tl):
                one = base.make_lpips(layers, [layer_id], [lins[k]], dtype)
                for p in range(x.shape[0]):
                    per_layer[p, k] = one.forward(xs[p:p + 1], ys[p:p + 1])
            feat = lp.extract_features(banks)
        xg = x1s.clone().requires_grad_(True)
        tr = lp.forward_tr(xg, feat)
        (grad,) = torch.autograd.grad(tr, [xg])
        grads[sfx] = grad.double()
        key = f'{net}{R}'
        out.update({f'{key}_pair{sfx}': total.numpy(), f'{key}_layers{sfx}': per_layer.numpy(), f'{key}_tr{sfx}': tr.detach().numpy(),
                    f'{key}_tr_grad{sfx}': grad.numpy()})
    return lo_all, float((grads['32'] - grads['64']).abs().max() / grads['64'].abs().max())


def plugin_crops(res, crop):
    """The step-0 crop of the toy loop's generator (this repository's CPU oracle) at `res`, in float32 and float64."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import latent_aug_ref as lar
    from oracle import sg2_networks as nets
    gl = np.load(os.path.join(HERE, 'latent_loop.npz'))
    crops = {}
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
        crops[sfx] = lar.apply_aug_transform(img, res, crop, 'center_random_crop', PLUG_POS)
    return crops


def record_plugin(net, layers, lins, crops, pbank, out):
    lo_all = float('inf')
    for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
        lp = base.make_lpips(layers, TARGETS[net], lins, dtype)
        vals = []
        for mode in range(2):
            x3 = crops[sfx][:, mode:mode + 1].repeat(1, 3, 1, 1)
            bank = pbank[mode].to(dtype)
            lo_all = min(lo_all, base._raw_norms(lp, x3), base._raw_norms(lp, bank))
            with torch.no_grad():
                vals.append(float(lp.forward_tr(x3, lp.extract_features(bank))))
        out[f'{net}_plug_tr{sfx}'] = np.asarray(vals, dtype=np.float64)
    return lo_all


def main():
    out = {'plug_pos': np.asarray(PLUG_POS, dtype=np.int64)}
    for net in ('alex', 'squeeze'):
        crops = plugin_crops(*PLUGIN[net])
        for wseed in range(SEEDS):
            g = torch.Generator().manual_seed(1000 + wseed)
            layers, chans = make_layers(net, g)
            lins = [torch.rand([c], generator=g) for c in chans]
            part, ok = {}, True
            for R in SIZES[net]:
                for seed in range(SEEDS):
                    gi = torch.Generator().manual_seed(seed)
                    x, y, x1, bank = base.gray3(gi, 3, R), base.gray3(gi, 3, R), base.gray3(gi, 1, R), base.gray3(gi, 4, R)
                    y[0] = x[0] + 0.01 * (y[0] - x[0])
                    case = {}
                    lo, gerr = record(net, R, layers, lins, x, y, x1, bank, case)
                    print(net, R, 'weights', wseed, 'inputs', seed, f'min norm {lo:.4f}  f32 gradient error {gerr:.2e}')
                    if lo >= MIN_NORM and gerr <= GRAD_TOL:
                        case.update({f'{net}{R}_seed': np.int64(seed), f'{net}{R}_x': x[:, :1].numpy(), f'{net}{R}_y': y[:, :1].numpy(),
                                     f'{net}{R}_x1': x1[:, :1].numpy(), f'{net}{R}_bank': bank[:, :1].numpy(),
                                     f'{net}{R}_min_norm': np.float64(lo), f'{net}{R}_grad_err': np.float64(gerr)})
                        part.update(case)
                        break
                else:
                    ok = False
                    break
            if not ok:
                continue
            crop = PLUGIN[net][1]
            for seed in range(SEEDS):
                gi = torch.Generator().manual_seed(seed)
                pbank = base.gray3(gi, 2 * PLUG_M, crop).reshape(2, PLUG_M, 3, crop, crop)
                case = {}
                lo = record_plugin(net, layers, lins, crops, pbank, case)
                print(net, 'plugin', 'weights', wseed, 'bank', seed, f'min norm {lo:.4f}')
                if lo >= MIN_NORM:
                    case.update({f'{net}_plug_seed': np.int64(seed), f'{net}_plug_bank': pbank[:, :, :1].numpy()})
                    part.update(case)
                    break
            else:
                continue
            break
        else:
            raise SystemExit(f'{net}: no seed met the conditions')
        out.update(part)
        out[f'{net}_wseed'] = np.int64(wseed)
        for k, v in layers.state_dict().items():
            out[f'{net}.features.{k}'] = v.numpy()
        for k, v in enumerate(lins):
            out[f'{net}.lin{k}'] = v.numpy()
    probe = base.BaseNet()
    out['mean'], out['std'] = probe.mean.reshape(3).float().numpy(), probe.std.reshape(3).float().numpy()
    path = os.path.join(HERE, 'lpips_nets.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
