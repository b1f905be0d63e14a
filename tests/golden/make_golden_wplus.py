#!/usr/bin/env python3
"""Golden vectors of the W+ loop (tests/golden/wplus_loop.npz) -- made by RUNNING THE REFERENCE in the build container.

Run from the repo root:   python tests/golden/make_golden_wplus.py
Needs /root/reference (read-only).  Never runs on the GPU box; only the .npz travels.

The W+ contract is the reference's LatentAug.forward (augments/utils/util_latent_aug.py:207-310) with exactly three methods
replaced: broadcasting(latent) is the identity for a [b, num_ws, w_dim] latent, hard_aug(w, w_tilde) returns w_tilde, and
smooth_aug(w, w_tilde) = alpha * w_tilde + (1 - alpha) * w row by row.  The module is built as make_golden.py::build_ref_module
builds it and then given that subclass; nothing else of the reference changes.  Toy geometry of latent_loop.npz (32^2, batch 2,
5 epochs) with distinct rows in w0 and in the bank W.

Stored per case: the final image, w_aug, the crop position and the per-step loss scalars (weighted {latent, pix, disc, lpips}, the
columns of la_latent_opt_run's losses_out).  The scalars are observed by wrapping the instance's calc_loss_* methods (harness code:
each wrapper calls the reference's own method and records `.item()` of its result).  The final synthesis of the reference draws
'random' noise from torch's generator; the draws are reproduced here, checked against the reference's image, and stored
(`noise_<k>`, unit noise [B, r, r] per synthesis layer) so that a GPU run can pass them as explicit noise.
A second run of the 'all' case in float64 through the pinned W+ oracle (tests/wplus_cpu.py; the reference casts its latent to
float32 at :212) is the tolerance anchor (`all_f64_*`).
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402  (installs the absent-module stand-ins, imports the reference)

sys.path.insert(0, os.path.dirname(HERE))
from oracle import feature_net as our_fnet      # noqa: E402
from oracle import sg2_networks as our_nets     # noqa: E402
from oracle import sg2_ops as our_ops           # noqa: E402
import wplus_cpu                                # noqa: E402

RES, CBASE, CMAX, WDIM, B, EPOCHS, LR, CROP = 32, 256, 16, 32, 2, 5, 0.01, 8
CASES = {
    'latent': dict(w_latent=0.5, w_pix=0.0, w_disc=0.0, w_lpips=0.0),
    'pix':    dict(w_latent=0.0, w_pix=2.0, w_disc=0.0, w_lpips=0.0),
    'disc':   dict(w_latent=0.0, w_pix=0.0, w_disc=1.0, w_lpips=0.0),
    'lpips':  dict(w_latent=0.0, w_pix=0.0, w_disc=0.0, w_lpips=3.0),
    'all':    dict(w_latent=0.3, w_pix=1.0, w_disc=0.5, w_lpips=2.0),
    'soft':   dict(w_latent=0.3, w_pix=1.0, w_disc=0.0, w_lpips=0.0, soft_aug=True, alpha=0.7),
}
LOSS_COLS = (('calc_loss_latent', 0), ('calc_loss_pix', 1), ('calc_loss_disc', 2), ('calc_loss_lpips_torchscript', 3))


class RefLatentAugWPlus(mg.ref_ula.LatentAug):
    """The reference's LatentAug with the three W+ replacements."""

    def broadcasting(self, latent):
        assert latent.shape[1] == self.num_ws
        return latent

    def hard_aug(self, w, w_tilde):
        assert w_tilde.shape == (self.batch_size // self.world_size, self.num_ws, self.w_dim)
        return w_tilde

    def smooth_aug(self, w, w_tilde):
        assert w.shape == w_tilde.shape == (self.batch_size // self.world_size, self.num_ws, self.w_dim)
        return (self.alpha * w_tilde) + ((1 - self.alpha) * w)


def main():
    our_nets.ops = mg._RefOpsAdapter
    try:
        G = our_nets.make_generator(img_resolution=RES, img_channels=2, channel_base=CBASE, channel_max=CMAX,
                                    seed=0, noise_strength=0.1, w_dim=WDIM, mapping_layers=2)
        D = our_nets.make_discriminator(img_resolution=RES, img_channels=2, channel_base=CBASE, channel_max=CMAX, seed=0)
        fnet = our_fnet.TinyFeatureNet(seed=5)
        g = torch.Generator().manual_seed(31)
        num_ws = G.num_ws
        # distinct rows: a per-sample base plus a per-row offset (as W+ inversions look), in the start latents and in the bank
        w0 = torch.randn([B, 1, WDIM], generator=g) + 0.5 * torch.randn([B, num_ws, WDIM], generator=g)
        W = torch.randn([12, 1, WDIM], generator=g) + 0.5 * torch.randn([12, num_ws, WDIM], generator=g)
        X = torch.rand([9, 2, RES, RES], generator=g) * 2 - 1
        fea = [torch.randn([9, fnet.out_features], generator=g) for _ in range(2)]
        out = dict(res=np.array(RES), cbase=np.array(CBASE), cmax=np.array(CMAX), wdim=np.array(WDIM), epochs=np.array(EPOCHS),
                   lr=np.array(LR), crop=np.array(CROP), w0=w0.numpy(), W=W.numpy(), X=X.numpy(), fea0=fea[0].numpy(),
                   fea1=fea[1].numpy())
        for name, kw in CASES.items():
            m = mg.build_ref_module(G, D, W, X, fea, fnet, res=RES, batch=B, epochs=EPOCHS, lr=LR, crop=CROP, **kw)
            m.__class__ = RefLatentAugWPlus
            steps = []
            for fname, col in LOSS_COLS:
                fn = getattr(m, fname)

                def wrapped(*a, _fn=fn, _col=col, **k):
                    v = _fn(*a, **k)
                    steps[-1][_col] = float(v.item())
                    return v
                setattr(m, fname, wrapped)
            syn = G.synthesis
            base_forward = syn.forward

            def synth_hook(*a, **k):
                if k.get('noise_mode') == 'const':      # a loop step starts with its synthesis (:227)
                    steps.append([0.0] * 4)
                return base_forward(*a, **k)
            syn.forward = synth_hook
            random.seed(6)
            torch.manual_seed(123)
            try:
                img, w_aug = m.forward(w0.clone(), ['a', 'b'])
            finally:
                del syn.forward
            assert len(steps) == EPOCHS
            out[f'{name}_img'] = img.detach().numpy()
            out[f'{name}_w_aug'] = w_aug.detach().numpy()
            out[f'{name}_losses'] = np.array(steps, dtype=np.float32)
            random.seed(6)
            out[f'{name}_crop_pos'] = np.array(mg.ref_ud.get_params(RES, CROP, 'center_random_crop')['crop_pos'])
            # the final synthesis' 'random' noise, reproduced: same seed, nothing else draws from torch's generator in the loop
            torch.manual_seed(123)
            noises = [torch.randn([B, 1, r, r]) for r in _layer_resolutions(G)]
            img_n = G.synthesis(w_aug.detach(), noises=noises)
            np.testing.assert_allclose(img_n.detach().numpy(), out[f'{name}_img'], rtol=0, atol=1e-6)
            print(name, float(img.abs().mean()), float((w_aug - w0).abs().max()), out[f'{name}_losses'][0])
        for k, n in enumerate(noises):
            out[f'noise_{k}'] = n[:, 0].numpy()
        out['num_noises'] = np.array(len(noises))
        # float64 anchor of the 'all' case through the pinned W+ oracle (our networks on our ops, as the oracle runs them)
    finally:
        our_nets.ops = our_ops
    G = our_nets.make_generator(img_resolution=RES, img_channels=2, channel_base=CBASE, channel_max=CMAX, seed=0, noise_strength=0.1,
                                w_dim=WDIM, mapping_layers=2)
    D = our_nets.make_discriminator(img_resolution=RES, img_channels=2, channel_base=CBASE, channel_max=CMAX, seed=0)
    fnet = our_fnet.TinyFeatureNet(seed=5)
    kw = {k: v for k, v in CASES['all'].items()}
    ref_kw = dict(res=RES, num_epochs=EPOCHS, opt_lr=LR, crop_size=CROP, final_noise_mode='const', **kw)
    img64, w64, tr = wplus_cpu.run_f64(ref_kw, G, D, W, X, fea, fnet, w0, tuple(int(v) for v in out['all_crop_pos']))
    out['all_f64_w_aug'] = w64.numpy()
    out['all_f64_w_steps'] = torch.stack(tr['w']).numpy()
    out['all_f64_img_const'] = img64.numpy()
    np.savez_compressed(os.path.join(HERE, 'wplus_loop.npz'), **out)
    print('wplus_loop.npz', len(out), 'arrays', os.path.getsize(os.path.join(HERE, 'wplus_loop.npz')), 'bytes')


def _layer_resolutions(G):
    """Resolution of every synthesis layer in execution order (what noise_mode='random' draws for, one [B,1,r,r] each)."""
    out = []
    for mod in G.synthesis.modules():
        if hasattr(mod, 'noise_const') and hasattr(mod, 'resolution'):
            out.append(int(mod.resolution))
    return out


if __name__ == '__main__':
    main()
