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
    out.update(measure_metrics(lib))
    return out


# Entries whose workspace is one buffer of exactly what it holds: their sizes are not rounded to 64 (and 'pr' counts floats).  The
# other single-buffer entries (sort, swd_stats, row_dist, fc) do round.
UNROUNDED = ('kid', 'dc', 'pr')
# Row counts around the places where a layout rounds: the byte count of an array of them is 0, 4, 8, 60 or 64 (mod 64) for 4- and
# 8-byte elements.
EDGE_ROWS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def metric_cases():
    """[(name, size entry, argument tuple)] of the stand-alone size entries of the metric side: a handful of shapes each, chosen where
    the layout rounds or takes another branch.  Integer arguments only, but the two `res` tables (tuples, passed as int arrays)."""
    cases = []
    add = lambda kind, entry, *args: cases.append((f'{kind}-' + '-'.join(                                   # noqa: E731
        'x'.join(map(str, a)) if isinstance(a, tuple) else str(a) for a in args), entry, args))
    for nx, ny in [(2, 2), (2, 3), (3, 2), (7, 9), (8, 8), (63, 65), (64, 64), (65, 200), (129, 64), (1000, 1001)]:
        for D in (1, 8, 9, 2048):                      # odd and even min(nx, ny); D on both sides of 8 doubles
            add('fd', 'la_fd_workspace_bytes', nx, ny, D)
    for k in (1, 5, 32):
        for nq, nx in [(1, 1), (1, 63), (63, 1), (63, 64), (64, 63), (64, 65), (65, 65), (7, 4097), (65, 4161), (1089, 4161), (40000, 129)]:
            add('knn', 'la_knn_scratch_bytes', nq, nx, 16, k)      # 4097 .. columns: past KNN_MAX_SPLITS tiles; 1089, 40000: the other bound
    for n in (2, 3, 15, 16, 17, 63, 64, 65, 1001):
        for k in (1, 3, 15, 32):                       # odd n k among them
            add('umap', 'la_umap_scratch_bytes', n, k)
    for ncols in (1, 2, 3, 64):
        for M in (1, 15, 16, 17, 4096, 4097):
            add('sort', 'la_sort_columns_scratch_bytes', ncols, M)
    for M in (1, 7, 8, 9, 4097):
        for ndirs in (1, 3, 31, 32, 33, 128):
            add('swd', 'la_swd_scratch_bytes', M, 48, ndirs)
    for M, Cc, P in [(1, 1, 1), (7, 3, 9), (100, 8, 49), (4097, 9, 49), (100000, 64, 4096)]:
        add('swd_stats', 'la_swd_stats_scratch_bytes', M, Cc, P)
    for P in (1, 3, 8):
        for Cc, HW in [(1, 1), (3, 7), (64, 256), (65, 256), (128, 1024), (129, 100), (512, 16), (512, 4096)]:
            add('gram', 'la_gram_pair_scratch_bytes', P, Cc, HW)
    for P, Cc in [(1, 1), (3, 1), (2, 3)]:
        for H, W, win, levels in [(11, 11, 11, 1), (16, 16, 1, 1), (33, 47, 7, 1), (32, 48, 3, 2), (176, 176, 11, 5), (192, 208, 7, 5)]:
            add('pair_metrics', 'la_pair_metrics_workspace_bytes', P, Cc, H, W, win, levels)
    for S, mx, my in [(1, 2, 2), (1, 3, 2), (3, 63, 65), (7, 64, 129), (100, 1000, 1000)]:
        add('kid', 'la_kid_workspace_bytes', S, mx, my)
    for ng in EDGE_ROWS:
        add('dc', 'la_dc_workspace_bytes', ng, 1)
        add('dc', 'la_dc_workspace_bytes', 5, ng)
        add('pr', 'la_pr_workspace_floats', ng, 3)
        add('pr', 'la_pr_workspace_floats', 129, ng + 1000)
    for rows in (1, 2, 7, 8, 9):
        for K in (1, 8192, 8193, 100000):
            add('row_dist', 'la_row_dist_workspace_bytes', rows, K)
    for res in [(4,), (8,), (16,), (4, 8, 8, 16, 16), (4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128), (1024,)]:
        for B in (1, 3, 8):
            add('noise_reg', 'la_noise_reg_scratch_bytes', res, len(res), B)
            add('noise_tail', 'la_proj_noise_tail_scratch_bytes', res, len(res), B)
    for N, K, O in [(1, 1, 1), (3, 7, 5), (8, 4096, 1000), (17, 25088, 4096), (64, 64, 10)]:
        add('fc', 'la_fc_workspace_bytes', N, K, O)
    return cases


def measure_metrics(lib):
    out = {}
    for name, entry, args in metric_cases():
        out[name] = getattr(lib, entry)(*[(C.c_int * len(a))(*a) if isinstance(a, tuple) else a for a in args])
    return out
