"""UMAP of the latent space, the reference's analysis/umap_analysis.py on the HIP path (latentaugment_amd.embedding.embed_aug_runs):
fit on the W codes of the inverted training set, transform the real and the augmented codes of run directories into that map, write
an .npz.  Plotting stays with the caller.

  python scripts/umap_latents.py --latent-zip INTERIM/DS/DSNAME-expinv_00001.zip --runs REPORTS/DS/latent_augment_umap-.. REPORTS/DS/random_augment_umap-.. \\
      --out umap.npz [--split train] [--n-per-group 100] [--w-row 0] [--n-neighbors 15] [--n-components 2] [--n-epochs N] [--min-dist 0.1]
      [--spread 1.0] [--negative-sample-rate 5] [--learning-rate 1.0] [--seed 42] [--gpu 0]

The .npz holds `embedding` float64 [M, n_components] and `labels` int64 [M]: 0 the real codes (latent/w_{i} of the first run), 1 + r the
augmented codes (latent_aug/w_aug_{i}) of run r.  The same arguments give the same bytes: the fit is reproducible bit for bit.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd.embedding import embed_aug_runs  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--latent-zip', required=True)
    ap.add_argument('--runs', required=True, nargs='+', help='run directories with latent/ and latent_aug/ dumps')
    ap.add_argument('--out', required=True)
    ap.add_argument('--split', default='train')
    ap.add_argument('--n-per-group', type=int, default=100)
    ap.add_argument('--w-row', type=int, default=0)
    ap.add_argument('--n-neighbors', type=int, default=15)
    ap.add_argument('--n-components', type=int, default=2)
    ap.add_argument('--n-epochs', type=int, default=None)
    ap.add_argument('--min-dist', type=float, default=0.1)
    ap.add_argument('--spread', type=float, default=1.0)
    ap.add_argument('--negative-sample-rate', type=int, default=5)
    ap.add_argument('--learning-rate', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--gpu', type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'umap_latents.py runs on the GPU; there is no CPU form'
    emb, labels = embed_aug_runs(args.latent_zip, args.split, args.runs, n_per_group=args.n_per_group, w_row=args.w_row,
                                 n_neighbors=args.n_neighbors, n_components=args.n_components, n_epochs=args.n_epochs, min_dist=args.min_dist,
                                 spread=args.spread, negative_sample_rate=args.negative_sample_rate, learning_rate=args.learning_rate,
                                 seed=args.seed, device=f'cuda:{args.gpu}')
    np.savez(args.out, embedding=emb, labels=labels)
    print(f'{args.out}: {emb.shape[0]} codes in {emb.shape[1]} dimensions, groups {np.bincount(labels).tolist()}')


if __name__ == '__main__':
    main()
