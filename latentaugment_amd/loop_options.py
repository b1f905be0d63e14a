"""The option surface of the latent loop, parsed once: `LoopOptions.from_opt(opt)` is the only place the package reads `opt`, and it
never writes to it.  Nothing here touches a device: no torch, no library -- the module is host logic that a CPU test imports alone.

Also here, because they are functions of the options only: which perceptual net a configuration asks for (`resolve_perceptual_net`) and
whether a batch goes through the two stream lanes (`lanes_eligible`)."""
import dataclasses
import os
import random
from typing import Any, Optional, Tuple

import numpy as np

from ._lib import LatentAugHipError

LATENT_SPACES = {'w': 0, 'w+': 1}      # opt.latent_space -> latent_space of la_latent_opt_create_ex
CRITERION_MODES = {'gemm': 0, 'collapsed': 1}
FINAL_NOISE_MODES = {'none': 0, 'const': 1, 'random': 2}
STREAM_LANES = ('auto', 1, 2)
# opt.lpips_net: the trunk of the reference's LPIPS class (augments/criteria/lpips/networks.py:12-20) -> the file names looked for under
# <model_dir> (torchvision's state dict, the LPIPS lin weights) and the smallest crop its stack takes (alex 31 -> conv 7 -> pools 3, 1;
# squeeze 17 -> conv 8 -> ceil-mode pools 4, 2, 1)
LPIPS_NET_FILES = {'vgg': ('vgg16.pth', 'lpips_vgg.pth'), 'alex': ('alexnet.pth', 'lpips_alex.pth'), 'squeeze': ('squeezenet1_1.pth', 'lpips_squeeze.pth')}
LPIPS_NET_MIN_RES = {'alex': 31, 'squeeze': 17}


def center_crop_geometry(load_size):
    """(crop, offset) of util_dataset.get_center_crop: CenterCrop(int(sqrt(res^2/2))), torchvision offset."""
    crop = int(np.sqrt((load_size * load_size) / 2))
    return crop, int(round((load_size - crop) / 2.0))


def get_params(load_size, crop_size, preprocess='center_random_crop'):
    """Random-crop position, drawn ONCE per forward on the host (util_dataset.py:284-296)."""
    assert preprocess in ['center_random_crop', 'random_crop']
    new = load_size
    if preprocess == 'center_random_crop':
        new = int(np.sqrt((load_size * load_size) / 2))
    x = random.randint(0, max(0, new - crop_size))
    y = random.randint(0, max(0, new - crop_size))
    return {'crop_pos': (x, y)}


def _preproc3(p):
    """opt.lpips_preproc -> ((s0, s1, s2), (b0, b1, b2)): a scalar pair applies to all three repeated channels."""
    scale, shift = p
    scale = tuple(float(v) for v in scale) if hasattr(scale, '__len__') else (float(scale),) * 3
    shift = tuple(float(v) for v in shift) if hasattr(shift, '__len__') else (float(shift),) * 3
    assert len(scale) == 3 and len(shift) == 3
    return scale, shift


def _one_of(name, value, accepted):
    if value not in accepted:
        raise LatentAugHipError(f'opt.{name} = {value!r}: expected one of {list(accepted)}')
    return value


@dataclasses.dataclass(frozen=True)
class LoopOptions:
    """Every option `LatentAug` consumes.  The first block is the reference's own surface (augments/latent_aug.py:57-96 there; required
    unless a default is given); the second is this package's, each with its default."""
    # ---- the reference's options
    img_resolution: int
    batch_size: int
    modalities: Tuple[str, ...]          # opt.modalities_aug, split at the commas
    opt_num_epochs: int                  # Adam steps on the latent per batch
    opt_lr: float
    truncation_psi: float
    w_pix: float
    w_lpips: float
    w_latent: float
    w_disc: float
    crop_size_aug: int                   # side of the window the perceptual criterion looks at
    preprocess_aug: str                  # window policy: center_crop | random_crop | center_random_crop | original
    soft_aug: bool
    alpha: float
    verbose_log: bool                    # losses / times / snapshots of the FIRST batch
    # 'lpips_script': the TorchScript vgg16.pt; anything else: the LPIPS class from two state dicts -- LPIPS('vgg'), or with an ':alex' /
    # ':squeeze' suffix (from_opt appends opt.lpips_net; read back by the `lpips_net` property) LPIPS('alex') / LPIPS('squeeze')
    lpips_script: str = 'lpips_script'
    model_dir: Optional[str] = None      # read where the generator or the perceptual net comes from disk
    interim_dir: Optional[str] = None    # read where banks come from the interim zips
    dataset_aug: Optional[str] = None
    dataset_name_aug: Optional[str] = None
    dataset_w_name: str = ''
    exp_stylegan: Optional[str] = None
    network_pkl_stylegan: Optional[str] = None
    step_img: Optional[int] = None       # every n-th slice of a patient in the image / feature banks
    step_w: Optional[int] = None         # ... in the latent bank
    # ---- this package's options
    criterion_mode: str = 'gemm'         # 'gemm' | 'collapsed' (criterion_code)
    final_noise_mode: str = 'random'     # 'none' | 'const' | 'random' (final_noise_code)
    # contraction arithmetic: 'f16x2' = fp32 operands scaled by powers of two and split into 2 fp16 terms (3 fp16 MFMAs
    # per product, fp32 accumulate); 'bf16x3' = 3 bf16 terms (6 MFMAs, no range scaling needed).  Both pass every fp32 parity test at
    # unchanged tolerances.  'f32' = exact fp32 MFMA; 'bf16x2' approximate.
    precision: str = 'f16x2'
    # latent space of the optimisation: 'w' (the reference's: one row per sample, broadcast to every style slot) or 'w+' (one row per
    # sample and slot: broadcasting() the identity, hard_aug / smooth_aug row by row -- DESIGN.md 'W+'); lower-cased
    latent_space: str = 'w'
    lpips_script_path: Optional[str] = None      # a local vgg16.pt (else <model_dir>/vgg16.pt)
    lpips_vgg_path: Optional[str] = None         # local state dicts of the LPIPS('vgg') branch (else <model_dir>/vgg16.pth,
    lpips_lin_path: Optional[str] = None         # <model_dir>/lpips_vgg.pth)
    # input affine of the perceptual net, ((s0, s1, s2), (b0, b1, b2)); None = not given: the net's own (a bare op list: identity)
    lpips_preproc: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None
    lpips_bank_range: str = 'unit'       # feature banks from x/127.5-1 ('unit') or from the reference's 0..255 input ('raw')
    lpips_cache_compat: bool = False     # 'raw' banks without an input affine under the reference's own cache name
    max_local_batch: int = 0             # per-process capacity; 0 = the batch, or its share of a process group
    norm_batch: int = 0                  # n of the criteria's 1/(m*n); 0 = the batch of each run
    # stream lanes: 'auto' (two lanes where lanes_eligible says they pay), 1 (never) or 2 (whenever the batch allows it)
    stream_lanes: Any = 'auto'
    lanes_selfcheck: bool = True         # first full batch through the lanes serially AND side by side; they must agree bit for bit
    hip_graph: bool = True               # one captured step replayed; False: every launch eager
    # discriminator and perceptual criterion of a step: 0 one after the other, 1 split replay, 2 fork / join inside the step
    # (opt.overlap_criteria True -> 2, False -> 0); bit-identical results (la_latent_opt_set_overlap in include/latentaug_hip.h)
    overlap_criteria: int = 2
    loop_window: bool = True             # the loop steps synthesise only the rows the criteria read; False: whole frames
    loop_window_columns: bool = True     # ... and, in the top block, only their columns
    # (opt.operand_scale of rounds 2-3 -- 'auto' | 'bound' | 'data' -- is accepted and ignored: every fp16 operand scale is derived from
    #  the data of each pass by the producing kernels now, batch by batch; there is no calibration to freeze)

    @classmethod
    def from_opt(cls, opt):
        def get(name, default=None):
            return getattr(opt, name, default)
        space = get('latent_space')
        latent_space = 'w' if space is None else str(space).lower()
        if latent_space not in LATENT_SPACES:
            raise LatentAugHipError(f'opt.latent_space = {space!r}: expected one of {sorted(LATENT_SPACES)}')
        oc = get('overlap_criteria', True)
        preproc = get('lpips_preproc')
        # opt.lpips_net ('vgg' | 'alex' | 'squeeze') and opt.lpips_trunk_path are read only on the LPIPS-class branch (lpips_script !=
        # 'lpips_script').  The record keeps its fields: another trunk than 'vgg' is carried as a ':alex' / ':squeeze' suffix of lpips_script
        # (`lpips_net` reads it back), the trunk's state dict in lpips_vgg_path (`lpips_trunk_path`), so the 'vgg' default changes nothing.
        script, trunk_path = get('lpips_script', 'lpips_script'), get('lpips_vgg_path')
        if script != 'lpips_script':
            net = _one_of('lpips_net', get('lpips_net', 'vgg') or 'vgg', tuple(LPIPS_NET_FILES))
            if net != 'vgg':
                script, trunk_path = f'{script}:{net}', get('lpips_trunk_path')
            elif get('lpips_trunk_path'):
                trunk_path = get('lpips_trunk_path')
        return cls(
            img_resolution=opt.img_resolution, batch_size=opt.batch_size,
            modalities=tuple(m for m in str(opt.modalities_aug).split(',') if m),
            opt_num_epochs=opt.opt_num_epochs, opt_lr=opt.opt_lr, truncation_psi=opt.truncation_psi,
            w_pix=opt.w_pix, w_lpips=opt.w_lpips, w_latent=opt.w_latent, w_disc=opt.w_disc,
            crop_size_aug=opt.crop_size_aug, preprocess_aug=opt.preprocess_aug, soft_aug=bool(opt.soft_aug), alpha=opt.alpha,
            verbose_log=bool(opt.verbose_log),
            lpips_script=script, model_dir=get('model_dir'), interim_dir=get('interim_dir'),
            dataset_aug=get('dataset_aug'), dataset_name_aug=get('dataset_name_aug'), dataset_w_name=str(get('dataset_w_name', '')),
            exp_stylegan=get('exp_stylegan'), network_pkl_stylegan=get('network_pkl_stylegan'),
            step_img=get('step_img'), step_w=get('step_w'),
            criterion_mode=_one_of('criterion_mode', get('criterion_mode', 'gemm'), CRITERION_MODES),
            final_noise_mode=_one_of('final_noise_mode', get('final_noise_mode', 'random'), FINAL_NOISE_MODES),
            precision=get('precision', 'f16x2'), latent_space=latent_space,
            lpips_script_path=get('lpips_script_path'), lpips_vgg_path=trunk_path, lpips_lin_path=get('lpips_lin_path'),
            lpips_preproc=_preproc3(preproc) if preproc is not None else None,
            lpips_bank_range=get('lpips_bank_range', 'unit'), lpips_cache_compat=bool(get('lpips_cache_compat', False)),
            max_local_batch=int(get('max_local_batch', 0) or 0), norm_batch=int(get('norm_batch', 0) or 0),
            stream_lanes=_one_of('stream_lanes', get('stream_lanes', 'auto'), STREAM_LANES),
            lanes_selfcheck=bool(get('lanes_selfcheck', True)), hip_graph=bool(get('hip_graph', True)),
            overlap_criteria=int(oc) if not isinstance(oc, bool) else (2 if oc else 0),
            loop_window=bool(get('loop_window', True)), loop_window_columns=bool(get('loop_window_columns', True)))

    @property
    def criterion_code(self):
        return CRITERION_MODES[self.criterion_mode]

    @property
    def final_noise_code(self):
        return FINAL_NOISE_MODES[self.final_noise_mode]

    @property
    def lpips_net(self):
        """Trunk of the LPIPS-class branch: 'vgg' unless from_opt recorded opt.lpips_net = 'alex' | 'squeeze' behind lpips_script."""
        head, sep, tail = self.lpips_script.rpartition(':')
        return tail if sep and tail in LPIPS_NET_MIN_RES else 'vgg'

    @property
    def lpips_trunk_path(self):
        return self.lpips_vgg_path

    @property
    def wplus(self):
        return self.latent_space == 'w+'

    def crop_window(self, crop_pos):
        """Absolute (x, y) of the crop_size_aug window for a position drawn by get_params (relative to the centre crop
        when preprocess is 'center_random_crop'; util_dataset.py:298-315)."""
        x1, y1 = crop_pos
        off = center_crop_geometry(self.img_resolution)[1] if self.preprocess_aug in ('center_crop', 'center_random_crop') else 0
        return off + int(x1), off + int(y1)

    def lane(self, full_local_batch):
        """The record one of the two stream lanes runs with: half the full local batch, the criteria's 1/(m*n) of the whole one.  Two
        lanes that each fork inside their captured step lose badly (preset E: 185 against 142 ms): a lane's criteria branches are
        replayed as graphs of their own on two streams instead (bit-identical; la_latent_opt_set_overlap mode 1)."""
        half = full_local_batch // 2
        return dataclasses.replace(self, batch_size=half, max_local_batch=half, norm_batch=full_local_batch, verbose_log=False,
                                   stream_lanes=1, overlap_criteria=1 if self.overlap_criteria == 2 else self.overlap_criteria)


def resolve_perceptual_net(options, feature_net=None):
    """Which perceptual net a configuration asks for, decided before anything touches a device: ('ops', feature_net) |
    ('script', path) | ('reference', (trunk_path, lin_path)) -- with opt.lpips_net = 'alex' | 'squeeze': (trunk_path, lin_path, net) -- |
    None (w_lpips <= 0).  Only os.path.isfile is asked about the files."""
    if options.w_lpips <= 0:
        return None
    if feature_net is not None:
        return 'ops', feature_net

    def first_file(cands):
        return next((c for c in cands if c and os.path.isfile(c)), None)
    # the reference's default perceptual net (`lpips_script`): NVIDIA's TorchScript vgg16.pt, fetched from a URL by load_vgg()
    # (:35-43).  There is no network here: a LOCAL copy is accepted at opt.lpips_script_path or <model_dir>/vgg16.pt.
    cands = [options.lpips_script_path]
    if options.lpips_script == 'lpips_script' and options.model_dir:
        cands.append(os.path.join(options.model_dir, 'vgg16.pt'))
    script = first_file(cands)
    # the reference's other perceptual branch (`lpips_script != 'lpips_script'`: augments/criteria/lpips/lpips.py::LPIPS('vgg'),
    # util_latent_aug.py:129-131, which downloads torchvision's VGG16 and the LPIPS lin weights): LOCAL state dicts at
    # opt.lpips_vgg_path / opt.lpips_lin_path, or <model_dir>/vgg16.pth and <model_dir>/lpips_vgg.pth
    if not options.lpips_script_path and options.lpips_script != 'lpips_script':
        net = options.lpips_net
        pair = []
        for given, name in zip((options.lpips_trunk_path, options.lpips_lin_path), LPIPS_NET_FILES[net]):
            pair.append(first_file([given] + ([os.path.join(options.model_dir, name)] if options.model_dir else [])))
        if all(pair):
            if net == 'vgg':
                return 'reference', tuple(pair)
            if options.crop_size_aug < LPIPS_NET_MIN_RES[net]:
                raise LatentAugHipError(f'opt.crop_size_aug = {options.crop_size_aug} is too small for opt.lpips_net = {net!r}: its stack '
                                        f'needs a crop of at least {LPIPS_NET_MIN_RES[net]}')
            return 'reference', tuple(pair) + (net,)
        if net != 'vgg' and script is None:
            raise NotImplementedError(
                f"w_lpips > 0 with opt.lpips_net = {net!r} needs local state dicts of torchvision's {LPIPS_NET_FILES[net][0][:-4]} at "
                f'opt.lpips_trunk_path or <model_dir>/{LPIPS_NET_FILES[net][0]}, and of the LPIPS lin layers at opt.lpips_lin_path or '
                f'<model_dir>/{LPIPS_NET_FILES[net][1]} (the reference downloads both; there is no network here); looked for '
                f'{[options.lpips_trunk_path, options.lpips_lin_path]} and under model_dir = {options.model_dir!r}')
    if script is not None:
        return 'script', script
    raise NotImplementedError(
        'w_lpips > 0 needs `feature_net=` (op list for synthesis.FeatureEngine, e.g. vgg16_lpips_ops(...)) or a local copy '
        "of NVIDIA's TorchScript vgg16.pt at opt.lpips_script_path / <model_dir>/vgg16.pt (the reference downloads it, "
        "util_latent_aug.py:36; there is no network here), or -- with opt.lpips_script != 'lpips_script' -- local state dicts of "
        "torchvision's VGG16 and the LPIPS lin layers at opt.lpips_vgg_path / opt.lpips_lin_path (<model_dir>/vgg16.pth, "
        "<model_dir>/lpips_vgg.pth), and banks['fea'] or the interim image zip to build them from")


def lanes_eligible(options, max_local, b):
    """`options`: a LoopOptions, or anything that carries its `stream_lanes`, `w_disc`, `w_lpips` and `overlap_criteria`.
    Two lanes need the FULL local batch (the criteria's 1/(m*n) is fixed per handle), an even one of at least 4 (measured: +3 % at
    4 x 256^2, +5 % at 4 x 512^2, +3.5 % at 16 x 256^2; four lanes lose), and -- with the discriminator --
    a multiple of 8: MinibatchStd groups sample n with n + b/4, n + 2b/4, n + 3b/4 (MinibatchStdLayer: `x.reshape(G, -1, F, c, H, W)`, group size 4, as the pickled discriminators of the reference carry it), and the even /
    odd halves of the batch keep exactly those groups only then."""
    if options.stream_lanes == 1 or b != max_local or b < 4 or b % 2:
        return False
    if options.w_disc > 0 and b % 8:
        return False
    if options.stream_lanes == 2 or options.w_lpips <= 0:
        return True
    # perceptual criterion: lanes pay only beside the discriminator, with the criteria branches of a lane replayed on two streams
    # (overlap mode 1, LoopOptions.lane): preset E 144.1 -> 141.7 ms, three alternating pairs on one box (round 5); with the criteria
    # one after the other (mode 0) 148.9, with the fork inside each lane's captured step (mode 2) 185
    return options.w_disc > 0 and options.overlap_criteria >= 1
