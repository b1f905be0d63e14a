"""Configurations whose workspace byte counts are pinned in tests/golden/workspace_sizes.json, and the calls that measure them.
Shared by tests/golden/make_golden_workspace_sizes.py (which records the counts from a given build of the library) and
test_workspace_sizes_cpu.py (which compares the in-tree build against the record).  Every call here only computes a size: no GPU,
no allocation, no tensor data -- the op lists are (kind, cin, cout) descriptors."""
import ctypes as C

import torch

from latentaugment_amd import _lib, synthesis, synthetic

RESOLUTIONS = (32, 128, 1024)
IMG_CHANNELS = (1, 2)
MAX_BATCH = (1, 3, 8)
W_DIM = 512
MW, MX, MF = 64, 16, 16          # rows of the latent, pixel and feature banks
STEPS = 5
LPIPS_RES = (32, 64)


def _descs(ops, in_ch):
    """FeatureEngine's descriptor list of an op list (the tensors may be shape-only)"""
    kinds = {'maxpool': synthesis.FEAT_MAXPOOL, 'avgpool': synthesis.FEAT_AVGPOOL}
    desc, c = [], in_ch
    for op in ops:
        if op[0] == 'conv':
            desc.append(_lib.FeatOp(synthesis.FEAT_CONV, c, op[1].shape[0]))
            c = op[1].shape[0]
        elif op[0] == 'tap':
            desc.append(_lib.FeatOp(synthesis.FEAT_TAP, c, c))
        elif op[0] == 'fc':
            desc.append(_lib.FeatOp(synthesis.FEAT_FC_RELU if op[3] else synthesis.FEAT_FC, op[1].shape[1], op[1].shape[0]))
            c = op[1].shape[0]
        else:
            desc.append(_lib.FeatOp(kinds[op[0]], c, c))
    return (_lib.FeatOp * len(desc))(*desc), len(desc)


def vgg16_lpips_descs():
    """descriptors of synthesis.vgg16_lpips_ops for the real VGG16 widths (shape-only tensors)"""
    widths = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
    sd, c = {}, 3
    for i, co in zip([0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28], widths):
        sd[f'features.{i}.weight'] = torch.empty([co, c, 3, 3], device='meta')
        sd[f'features.{i}.bias'] = torch.empty([co], device='meta')
        c = co
    lins = [torch.empty([n], device='meta') for n in (64, 128, 256, 512, 512)]
    return _descs(synthesis.vgg16_lpips_ops(sd, lins), 3)


def detector_descs(in_res):
    """a detector list: two convs with a pool each, then two fully connected ops"""
    e = lambda *s: torch.empty(list(s), device='meta')      # noqa: E731
    k = 16 * (in_res // 4) ** 2
    ops = [('conv', e(8, 3, 3, 3), e(8)), ('maxpool',), ('conv', e(16, 8, 3, 3), e(16)), ('avgpool',), ('fc', e(64, k), e(64), True),
           ('fc', e(10, 64), e(10), False)]
    return _descs(ops, 3)


def tap_features(in_res):
    """feature count of the one-op list [tap] on a 3-channel input: the smallest list an engine accepts, created without a launch"""
    return 3 * in_res * in_res


def opt_config(res):
    crop = int(res * 0.7)
    return _lib.OptConfig(steps=STEPS, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, w_latent=0.3, w_pix=1.0, crop=crop, crop_off=(res - crop) // 2)


def measure(lib):
    """{name: bytes} of every pinned configuration, from `lib`"""
    out = {}
    for res in RESOLUTIONS:
        ch = synthetic.channels_dict(res)
        chan = (C.c_int * len(ch))(*[ch[r] for r in sorted(ch)])
        cfg = opt_config(res)
        for imgc in IMG_CHANNELS:
            for mb in MAX_BATCH:
                tag = f'res{res}-c{imgc}-b{mb}'
                out[f'synth-{tag}'] = lib.la_synth_workspace_bytes(res, imgc, W_DIM, chan, mb)
                out[f'disc-{tag}'] = lib.la_disc_workspace_bytes(res, imgc, chan, mb)
                out[f'latent_opt-w-{tag}'] = lib.la_latent_opt_workspace_bytes_ex(res, imgc, W_DIM, C.byref(cfg), MW, MX, mb, 0)
                out[f'latent_opt-wplus-{tag}'] = lib.la_latent_opt_workspace_bytes_ex(res, imgc, W_DIM, C.byref(cfg), MW, MX, mb, 1)
    vgg, nvgg = vgg16_lpips_descs()
    for in_res in LPIPS_RES:
        feats = {'vgg16': synthetic.lpips_num_features(crop=in_res), 'tap': tap_features(in_res)}
        det, ndet = detector_descs(in_res)
        for mb in MAX_BATCH:
            out[f'feat-vgg16-res{in_res}-b{mb}'] = lib.la_feat_workspace_bytes(nvgg, vgg, 3, in_res, mb)
            out[f'feat-detector-res{in_res}-b{mb}'] = lib.la_feat_workspace_bytes(ndet, det, 3, in_res, mb)
            for imgc in IMG_CHANNELS:
                for net, F in feats.items():
                    out[f'lpips-{net}-S{in_res}-c{imgc}-b{mb}'] = lib.la_latent_opt_lpips_workspace_bytes(imgc, F, in_res, MF, mb)
    return out
