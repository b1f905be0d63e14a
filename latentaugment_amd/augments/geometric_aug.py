"""GeometricAugment plugin: drop-in for the reference's augments/geometric_aug.py::GeometricAugment, the baseline its LatentAugment
results are compared against (driver: backbone_geoaug.py).  Same command-line options (names, types, defaults: reference :24-30) and the
same methods (set_input / forward / get_output / sanity_check, stats_time: reference :75-98, :142-151).

The reference composes the pipeline from kornia (RandomHorizontalFlip, RandomAffine, RandomElasticTransform in an AugmentationSequential);
this one runs it on HIP kernels of its own (latentaugment_amd.geometric, csrc/la_geom.hip) and needs no kornia.  What is kept is the
pipeline, not kornia's random stream or its last bits -- the contract is the pixel-space definition in DESIGN 'GeometricAugment':

  1. flip      x -> W - 1 - x
  2. affine    rotation by U(-rotate_limit, rotate_limit) degrees about the image centre and a shift by U(-shift_limit, shift_limit) of
               the width / height, reflection padding
  3. elastic   kornia's elastic_transform2d with its defaults (63-tap Gaussian, sigma 32, alpha 1), reflection padding

each applied to a sample with probability 1 - p_thres, drawn independently per stage and sample.  Flip and affine are one resampling
(the flip is exact, so composing it loses nothing); the elastic warp is a second resampling of that result.  The A|B pair is warped as one
2-channel image: both modalities get the same deformation.

Deliberate decisions where the reference's text does not settle things:
- The reference passes `translate=shift_limit` as a scalar, which kornia's range check most likely refuses (it expects a pair); it is
  read here as the symmetric fraction (-shift_limit, shift_limit) of the width and of the height, as the option's help text says.
- phase 'val' / 'test' is the identity.  The reference leaves `self.transform` undefined there and would crash in forward().
- `opt.seed_aug` (optional, this package's own) seeds a CPU torch.Generator for the parameter draw; without it the draw comes from torch's
  global CPU generator.  The parameters of the last batch are kept in `last_params`, so a batch can be reproduced.
- sanity_check asserts shapes and dtype only: no matplotlib, no pictures.
"""
import time

import torch

from .. import geometric
from .base_aug import BaseAugment


class GeometricAugment(BaseAugment):
    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--p_thres', type=float, default=0.5, help='a stage is applied to a sample with probability 1 - p_thres')
        parser.add_argument('--horizontal_flip', action='store_true', help='switch the horizontal flip on')
        parser.add_argument('--affine', action='store_true', help='switch the rotation / shift on')
        parser.add_argument('--elastic_deform', action='store_true', help='switch the elastic deformation on')
        parser.add_argument('--rotate_limit', type=float, default=3, help='rotation drawn from (-rotate_limit, rotate_limit) degrees')
        parser.add_argument('--shift_limit', type=float, default=0.05, help='shift drawn from (-shift_limit, shift_limit) of the width / height')
        parser.add_argument('--verbose_log', type=bool, default=False, help='print the time of every batch')
        return parser

    def __init__(self, opt):
        BaseAugment.__init__(self, opt)
        self.phase = opt.phase
        self.p_thres = opt.p_thres
        self.horizontal_flip = opt.horizontal_flip
        self.affine = opt.affine
        self.elastic_deform = opt.elastic_deform
        self.rotate_limit = opt.rotate_limit
        self.shift_limit = opt.shift_limit
        self.verbose_log = opt.verbose_log
        self.stats_time = []
        self.last_params = None
        self.transform = None
        if self.phase == 'train':
            self.transform = self.get_train_transform()
        elif self.phase in ['val', 'test']:
            pass      # all augmentation disabled
        else:
            raise NotImplementedError

    def get_train_transform(self):
        """The pipeline as plain settings (the reference returns a kornia AugmentationSequential here): which stages are on, their
        ranges, the blur of the elastic field and the generator the parameters are drawn from."""
        seed = getattr(self.opt, 'seed_aug', None)
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        return {'gen': gen, 'p': 1.0 - self.p_thres, 'flip': bool(self.horizontal_flip), 'affine': bool(self.affine),
                'elastic': bool(self.elastic_deform), 'rotate_limit': float(self.rotate_limit), 'shift_limit': float(self.shift_limit),
                'taps': geometric.gaussian_taps(geometric.ELASTIC_KSIZE, geometric.ELASTIC_SIGMA).tolist(),
                'alpha': (geometric.ELASTIC_ALPHA, geometric.ELASTIC_ALPHA)}

    @staticmethod
    def input_sanity_check(img):
        assert isinstance(img, torch.Tensor) and img.dtype == torch.float32 and img.ndim == 3 and img.shape[0] == 1, \
            'expected one float32 [1, H, W] slice per modality'

    output_sanity_check = input_sanity_check

    def set_input(self, data):
        """data = {'A', 'B': [B,1,H,W] float32 tensors, 'A_paths', 'B_paths': per-sample file names (identical lists)}.  The pair is
        joined along the channels and goes to the device as one [B,2,H,W] tensor."""
        assert data['A_paths'] == data['B_paths']
        self.fname = data['A_paths']
        self.real_A, self.real_B = data['A'], data['B']
        self.real_AB = torch.cat((self.real_A, self.real_B), dim=1).to(self.device, non_blocking=True)

    def get_output(self):
        both = self.real_AB_aug.detach().cpu()
        return {'A': both[:, 0:1], 'B': both[:, 1:2], 'A_paths': self.fname, 'B_paths': self.fname}

    def _apply(self, x):
        t = self.transform
        B, _, H, W = x.shape
        params = geometric.draw_params(t['gen'], B, H, W, t['p'], t['flip'], t['affine'], t['elastic'], t['rotate_limit'], t['shift_limit'])
        self.last_params = params
        warp = params['flip'] | params['affine']
        # one page-locked record per batch -- [B][6] inverse maps, [B] affine-launch flags, [B] elastic flags -- and one copy of it
        host = torch.empty([26 * B], dtype=torch.uint8, pin_memory=x.is_cuda)
        host[:24 * B].view(torch.float32).view(B, 6).copy_(geometric.affine_inverse(params, H, W))
        host[24 * B:25 * B].copy_(warp)
        host[25 * B:].copy_(params['elastic'])
        dev = host.to(x.device, non_blocking=True)
        if bool(warp.any()):
            x = geometric.warp_affine(x, dev[:24 * B].view(torch.float32).view(B, 6), dev[24 * B:25 * B], 'reflection')
        if bool(params['elastic'].any()):
            noise = geometric.noise_uniform(B, 2 * H * W, int(params['seed']), device=x.device).view(B, 2, H, W)
            x = geometric.warp_elastic(x, geometric.elastic_field(noise, t['taps'], t['alpha']), dev[25 * B:], 'reflection')
        return x

    def forward(self):
        """One batch: at most four launches (flip + affine, noise, field, elastic warp) on the current stream and nothing that waits for
        the device -- get_output does.  The host time of the call is appended to stats_time, as in the reference."""
        since = time.time()
        self.real_AB_aug = self.real_AB if self.transform is None else self._apply(self.real_AB)
        time_elapsed = time.time() - since
        self.stats_time.append(time_elapsed)
        if self.verbose_log:
            print('Augmentation completed in {:.0f}m {:.3f}s'.format(time_elapsed // 60, time_elapsed % 60))

    def sanity_check(self):
        self.input_sanity_check(self.real_A[0])
        self.input_sanity_check(self.real_B[0])
        self.forward()
        data = self.get_output()
        for key, src in (('A', self.real_A), ('B', self.real_B)):
            self.output_sanity_check(data[key][0])
            assert data[key].shape == src.shape
