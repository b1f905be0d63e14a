"""W vs W+ latent optimisation at config B (config-f 256^2, batch 8, 20 latent steps, w_latent 0.001, w_pix 0.1), through the plugin API
(create_augment -> set_input -> forward -> get_output, the reference driver's loop body).

    python scripts/bench_wplus.py [--rounds 5] [--batches 3] [--warmup 2]

One augmenter per latent space, built once.  The two are timed in alternating rounds of `batches` batches each (after `warmup` batches
each), so that clock and thermal drift fall on both alike.  W+ starts from the same inverted latents broadcast to every slot plus a
small per-row offset.  Prints one JSON line: median and spread of the ms per batch of each mode, and their ratio.
"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_aug(space, sd, W, X, codes, batch):
    from latentaugment_amd.augments import create_augment
    opt = types.SimpleNamespace(
        aug='latent', gpu_ids=[0], gpu_ids_aug='0', checkpoints_dir='/tmp', name='bench_wplus', phase='train', img_resolution=256,
        batch_size=batch, modalities_aug='A,B', opt_num_epochs=20, opt_lr=0.01, truncation_psi=1.0, w_pix=0.1, w_lpips=0.0,
        w_latent=0.001, w_disc=0.0, crop_size_aug=64, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False,
        rand_aug=False, lower_bound_clip=False, p_thres=0.0, init_w='inv', final_noise_mode='random', latent_space=space)
    opt.inject = dict(generator=sd, banks={'W': W, 'X': X}, latent_codes=codes)
    with contextlib.redirect_stdout(io.StringIO()):
        return create_augment(opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    from latentaugment_amd import synthetic
    from latentaugment_amd.latent_aug import InMemoryLatentCodes
    batch = 8
    sd, meta = synthetic.make_generator_state_dict(img_resolution=256, img_channels=2, channel_base=32768, seed=0)
    nws = meta['num_ws']
    W, X = synthetic.make_banks(nws, res=256, M_w=1024, M_x=256)
    data = synthetic.make_batch(batch, res=256, seed=2)
    w0 = synthetic.make_latents(batch, seed=1)
    offs = 0.1 * torch.randn([batch, nws, 512], generator=torch.Generator().manual_seed(3))
    augs = {}
    for space in ('w', 'w+'):
        codes = {p: (w0[i, 0] + offs[i]).numpy() if space == 'w+' else w0[i, 0].numpy() for i, p in enumerate(data['A_paths'])}
        augs[space] = make_aug(space, sd, W, X, InMemoryLatentCodes(codes), batch)

    def run(aug, n):
        times = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aug.set_input(data)
            aug.forward()
            aug.get_output()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return times

    random.seed(6)
    for aug in augs.values():
        run(aug, args.warmup)
    ms = {s: [] for s in augs}
    for r in range(args.rounds):
        for s in (('w', 'w+') if r % 2 == 0 else ('w+', 'w')):
            ms[s] += run(augs[s], args.batches)
    out = {'config': 'B: config-f 256^2, batch 8, 20 latent steps, w_latent 0.001, w_pix 0.1', 'batches_per_mode': len(ms['w'])}
    for s, v in ms.items():
        key = s.replace('+', 'plus')
        out[f'{key}_ms_per_batch_median'] = round(statistics.median(v), 2)
        out[f'{key}_ms_per_batch_min'] = round(min(v), 2)
        out[f'{key}_ms_per_batch_max'] = round(max(v), 2)
        out[f'{key}_lanes'] = bool(augs[s].latent_aug.lanes_active)
        out[f'{key}_graph_state'] = int(augs[s].latent_aug.graph_state)
    out['wplus_over_w'] = round(out['wplus_ms_per_batch_median'] / out['w_ms_per_batch_median'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
