"""Invert every slice of an image zip into W / W+ and write the latent zip `opt.dataset_w_name` points at
(latentaugment_amd.projector.project_dataset; INTEGRATION.md 'From an image zip to the latent zip').

  python scripts/project_dataset.py --network-pkl RUN/network-snapshot-005320.pkl --img-zip INTERIM/DS/DSNAME.zip \\
      --out-zip INTERIM/DS/DSNAME-expinv_00001.zip --modalities MR_nonrigid_CT,MR_MR_T2 \\
      (--vgg16-pt MODELS/vgg16.pt | --lpips-vgg MODELS/vgg16.pth --lpips-lin MODELS/lpips_vgg.pth) \\
      [--split train] [--steps 1000] [--space w|w+] [--w-pix 0.0] [--batch 8] [--lpips-res 256] [--precision f16x2] [--seed 0] [--gpu 0]
      [--optimize-noise] [--regularize-noise-weight 1e5]

The generator is read from the pickle without running its embedded source (formats.load_network_pkl); the perceptual net is a LOCAL
copy of NVIDIA's TorchScript vgg16.pt or the two state dicts of the reference's LPIPS('vgg').  One line of progress per batch.
--optimize-noise optimises the per-layer noise maps beside the latent (regularised, re-normalised every step) and discards them: the
zip holds the latents alone, as without it.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import formats  # noqa: E402
from latentaugment_amd.projector import Projector, project_dataset  # noqa: E402
from latentaugment_amd.synthesis import FeatureEngine, lpips_reference_net  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--network-pkl', required=True)
    ap.add_argument('--img-zip', required=True)
    ap.add_argument('--out-zip', required=True)
    ap.add_argument('--modalities', required=True, help='comma-separated, in the generator\'s channel order')
    ap.add_argument('--vgg16-pt', default=None, help="local copy of NVIDIA's TorchScript vgg16.pt")
    ap.add_argument('--lpips-vgg', default=None, help="state dict of torchvision's VGG16")
    ap.add_argument('--lpips-lin', default=None, help='state dict of the LPIPS lin layers')
    ap.add_argument('--split', default='train')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--space', default='w', choices=('w', 'w+'))
    ap.add_argument('--w-pix', type=float, default=0.0)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--lpips-res', type=int, default=None, help='resolution of the perceptual net (default: min(generator resolution, 256))')
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--optimize-noise', action='store_true', help='optimise the per-layer noise maps beside the latent (then discard them)')
    ap.add_argument('--regularize-noise-weight', type=float, default=1e5)
    args = ap.parse_args()
    if (args.vgg16_pt is None) == (args.lpips_vgg is None or args.lpips_lin is None):
        ap.error('give either --vgg16-pt, or both --lpips-vgg and --lpips-lin')
    assert torch.cuda.is_available(), 'project_dataset.py runs on the GPU; there is no CPU form'
    dev = torch.device('cuda', args.gpu)
    G = formats.load_network_pkl(args.network_pkl)['G_ema']
    mods = [m for m in args.modalities.split(',') if m]
    res = int(G.img_resolution)
    lpips_res = args.lpips_res or min(res, 256)
    if args.vgg16_pt is not None:
        net = FeatureEngine.from_torchscript(args.vgg16_pt, dev, lpips_res, len(mods) * args.batch, precision=args.precision)
    else:
        net = lpips_reference_net(args.lpips_vgg, args.lpips_lin)
    proj = Projector(G, net, dev, args.batch, precision=args.precision, lpips_res=lpips_res)
    finals = project_dataset(args.img_zip, args.out_zip, args.split, proj, mods, num_steps=args.steps, space=args.space, seed=args.seed,
                             w_pix=args.w_pix, optimize_noise=args.optimize_noise, regularize_noise_weight=args.regularize_noise_weight,
                             log=lambda s: print(s, flush=True))
    print(f'wrote {len(finals)} codes [{proj.num_ws}, {proj.w_dim}] to {args.out_zip}; final perceptual distance: mean {finals[:, 0].mean():.4g}, '
          f'worst {finals[:, 0].max():.4g}')


if __name__ == '__main__':
    main()
