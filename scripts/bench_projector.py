"""Benchmark of the projector (latentaugment_amd/projector.py): one optimisation step at config-f 256 x 256, B = 8, both modalities
through a full-width VGG16 with five taps at 256 x 256 (random weights, synthetic.make_vgg16_lpips_ops), and its parts.

  python scripts/bench_projector.py [--iters 10] [--warmup 2] [--precision f16x2] [--batch 8] [--space w|w+] [--w-pix 0.1] [--optimize-noise]

step      `--steps-per-window` whole steps (Projector.loss_and_grad + Projector.step_tail, as project() runs them) between two device
          events, per step; images per hour at 1000 steps = batch * 3600 s / (1000 * step).
parts     each part of a step between two device events of its own, on the buffers the step uses: synthesis forward / backward, the
          preparation and its adjoint, feature forward / backward, la_row_dist_f32 on the feature rows and on the pixels.  (The parts
          do not have to add up to the step: a part timed alone starts on an idle device.)
tail      la_proj_step_tail_f32 against the composition it replaces -- the row sum of dws (torch, W space only), la_adam_step_f32,
          la_noise_normal_f32 and torch's add -- `--tail-reps` times each between two events, per call: the calls are a few
          microseconds, one event pair around one of them would measure the events.
dist      la_row_dist_f32 on the feature rows against the same two quantities from torch ops (the difference, its square summed per row
          and folded per sample, the scaled difference), one call each between two events.
box       la_box_down_f32 / la_box_up_f32 of the 16 planes of a 512 x 512 batch to 256 x 256 (k = 2; config-f 256 itself has k = 1).
noise     with --optimize-noise the step is the one project(optimize_noise=True) runs (explicit maps in the forward pass, the channel
          reductions inside the synthesis backward pass, the regulariser, the noise tail), and its three additions are also timed alone:
          the synthesis backward pass with and without noise gradients (their difference is the reductions, whose bytes -- every stored
          gradient read once -- give the GB/s), la_noise_reg_f32 and la_proj_noise_tail_f32 over all maps.
Every form runs --warmup untimed rounds first; the forms of a comparison alternate inside a round; medians of --iters rounds, with
minimum and maximum.  Prints ONE JSON line.  No ratio is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentaugment_amd import _lib, synthetic  # noqa: E402
from latentaugment_amd.projector import ADAM_BETAS, ADAM_EPS, NoiseMaps, Projector, schedule  # noqa: E402


def timed(fn, stream, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--precision', default='f16x2')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--space', default='w', choices=('w', 'w+'))
    ap.add_argument('--w-pix', type=float, default=0.1)
    ap.add_argument('--steps-per-window', type=int, default=5)
    ap.add_argument('--tail-reps', type=int, default=200)
    ap.add_argument('--optimize-noise', action='store_true')
    ap.add_argument('--noise-strength', type=float, default=None, help='noise_strength of every layer (default 0, with --optimize-noise 0.05)')
    ap.add_argument('--regularize-noise-weight', type=float, default=1e5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_projector.py measures on the GPU; there is no CPU form'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    B, R = args.batch, args.res
    # (a generator without noise has no maps to optimise: the flag's default strength is that of a trained network's order, 0.05)
    strength = args.noise_strength if args.noise_strength is not None else (0.05 if args.optimize_noise else 0.0)
    sd, _ = synthetic.make_generator_state_dict(img_resolution=R, seed=0, noise_strength=strength)
    proj = Projector(sd, synthetic.make_vgg16_lpips_ops(seed=7), dev, B, precision=args.precision)
    Cc, nws, wd, F = proj.img_channels, proj.num_ws, proj.w_dim, proj.feat.num_features
    L = nws if args.space == 'w+' else 1
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(1)
    w_opt = torch.randn([B, L, wd], generator=g, device=dev)
    m, v, ws = torch.zeros_like(w_opt), torch.zeros_like(w_opt), torch.empty_like(w_opt)
    with torch.no_grad():
        tgt = proj.synth.forward(torch.randn([B, 1, wd], generator=g, device=dev)).clone()
    tfeat = proj.target_features(tgt)
    maps = NoiseMaps(proj.synth, B, 0, 0) if args.optimize_noise else None
    loss = torch.zeros([B, 3 if maps is not None else 2], dtype=torch.float64, device=dev)
    T = 1000
    state = {'t': 0}

    def step():
        t = state['t']
        dws, _ = proj.loss_and_grad(ws, tgt, tfeat, args.w_pix, loss, maps, args.regularize_noise_weight)
        proj.step_tail(dws, w_opt, m, v, ws, t + 1, schedule(t, T, 1.0)[0], schedule(t + 1, T, 1.0)[1], 0, t + 1, 0)
        if maps is not None:
            proj.noise_tail(maps, t + 1, schedule(t, T, 1.0)[0])
        state['t'] = t + 1
    proj.step_tail(None, w_opt, m, v, ws, 0, 0.0, schedule(0, T, 1.0)[1], 0, 0, 0)

    # ---- parts, on the step's own buffers
    buf = {}

    def p_synth_fwd():
        buf['img'] = proj.synth.forward(ws, noise_mode='const') if maps is None else proj.synth.forward(ws, noise_mode='random', noises=maps.per_layer(maps.n))

    def p_prepare():
        buf['xc'] = proj._prepare(buf['img'], B)

    def p_feat_fwd():
        buf['feat'] = proj.feat.forward(buf['xc'])

    def p_dist_feat():
        proj._row_dist(buf['feat'], tfeat, Cc * B, F, Cc, 1.0 / Cc, 2.0 / Cc, proj._gfeat[:Cc * B], 0, loss, 0)

    def p_feat_bwd():
        buf['gxc'] = proj.feat.backward(proj._gfeat[:Cc * B])

    def p_prepare_adj():
        buf['g_img'] = proj._prepare_adjoint(buf['gxc'], B)

    def p_dist_pix():
        n = Cc * R * R
        proj._row_dist(buf['img'], tgt, B, n, 1, args.w_pix / n, 2.0 * args.w_pix / n, buf['g_img'], 1, loss, 1)

    def p_synth_bwd():
        buf['dws'] = proj.synth.backward(buf['g_img'])
    parts = {'synthesis_forward': p_synth_fwd, 'prepare': p_prepare, 'feature_forward': p_feat_fwd, 'row_dist_features': p_dist_feat,
             'feature_backward': p_feat_bwd, 'prepare_adjoint': p_prepare_adj, 'row_dist_pixels': p_dist_pix, 'synthesis_backward': p_synth_bwd}

    # ---- tail against its composition
    dws_fixed = torch.randn([B, nws, wd], generator=g, device=dev)
    tw, tm, tv, tws = (torch.zeros([B, L, wd], device=dev) for _ in range(4))
    cw, cm, cv, cn = (torch.zeros([B, L, wd], device=dev) for _ in range(4))
    cws = torch.empty_like(cw)

    def tail_fused():
        proj.step_tail(dws_fixed, tw, tm, tv, tws, 7, 0.05, 0.03, 0, 7, 0)

    def tail_composed():
        grad = dws_fixed.sum(dim=1, keepdim=True) if L == 1 else dws_fixed
        _lib.check(lib.la_adam_step_f32(_lib.ptr(cw), _lib.ptr(grad), _lib.ptr(cm), _lib.ptr(cv), cw.numel(), 7, 0.05, ADAM_BETAS[0], ADAM_BETAS[1],
                                        ADAM_EPS, _lib.stream_ptr()), 'la_adam_step_f32')
        _lib.check(lib.la_noise_normal_f32(_lib.ptr(cn), B, L * wd, 0, 7, 0, _lib.stream_ptr()), 'la_noise_normal_f32')
        torch.add(cw, cn, alpha=0.03, out=cws)

    # ---- kernel 1 against torch
    a_rows = torch.randn([Cc * B, F], generator=g, device=dev)
    t_rows = a_rows + 0.05 * torch.randn([Cc * B, F], generator=g, device=dev)
    g_rows = torch.empty_like(a_rows)
    res = {}

    def dist_kernel():
        proj._row_dist(a_rows, t_rows, Cc * B, F, Cc, 1.0 / Cc, 2.0 / Cc, g_rows, 0, loss, 0)

    def dist_torch():
        d = a_rows - t_rows
        res['loss'] = d.square().sum(1).reshape(Cc, B).sum(0) * (1.0 / Cc)
        res['g'] = d * (2.0 / Cc)

    # ---- kernel 2 at k = 2
    planes, R2 = Cc * B, 2 * R
    x2 = torch.randn([planes, R2, R2], generator=g, device=dev)
    y2, gx2 = torch.empty([planes, R, R], device=dev), torch.empty([planes, R2, R2], device=dev)

    def box_down():
        _lib.check(lib.la_box_down_f32(_lib.ptr(x2), _lib.ptr(y2), planes, R2, 2, _lib.stream_ptr()), 'la_box_down_f32')

    def box_up():
        _lib.check(lib.la_box_up_f32(_lib.ptr(y2), _lib.ptr(gx2), planes, R2, 2, _lib.stream_ptr()), 'la_box_up_f32')

    noise_parts = {}
    if maps is not None:
        def p_synth_bwd_noise():
            proj.synth.backward(buf['g_img'], noise_grads=maps.per_layer(maps.g))

        def p_noise_reg():
            reg_ws = proj._noise_ws[0]
            w = args.regularize_noise_weight
            _lib.check(lib.la_noise_reg_f32(maps.tables['n'], maps.res_table, len(maps.res), B, w, w, maps.tables['g'], 1, _lib.ptr(loss[:, 2:]), 3,
                                            _lib.ptr(reg_ws), reg_ws.numel() * 8, _lib.stream_ptr()), 'la_noise_reg_f32')

        def p_noise_tail():
            proj.noise_tail(maps, 7, 0.05)
        noise_parts = {'synthesis_backward_with_noise_grads': p_synth_bwd_noise, 'noise_regulariser': p_noise_reg, 'noise_tail': p_noise_tail}
        parts.update(noise_parts)

    singles = {**parts, 'dist_kernel': dist_kernel, 'dist_torch': dist_torch, 'box_down_k2': box_down, 'box_up_k2': box_up}
    with torch.cuda.device(dev):
        for _ in range(args.warmup):
            step()
            for f in singles.values():
                f()
            tail_fused()
            tail_composed()
        torch.cuda.synchronize()
        times = {k: [] for k in list(singles) + ['step', 'tail_fused', 'tail_composed']}
        for _ in range(args.iters):
            times['step'].append(timed(step, stream, args.steps_per_window))
            for k, f in singles.items():
                times[k].append(timed(f, stream))
            times['tail_fused'].append(timed(tail_fused, stream, args.tail_reps))
            times['tail_composed'].append(timed(tail_composed, stream, args.tail_reps))
        dist_kernel()
        dist_torch()
        torch.cuda.synchronize()
    step_ms = float(np.median(times['step']))
    lk, lt = loss[:, 0].cpu().numpy(), res['loss'].double().cpu().numpy()
    out = {
        'config': {'res': R, 'batch': B, 'img_channels': Cc, 'num_ws': nws, 'w_dim': wd, 'space': args.space, 'w_pix': args.w_pix,
                   'precision': args.precision, 'noise_strength': strength, 'optimize_noise': bool(args.optimize_noise), 'num_features': F, 'lpips_res': proj.lpips_res, 'iters': args.iters, 'warmup': args.warmup},
        'step_ms': stats(times['step']),
        'images_per_hour_at_1000_steps': B * 3600.0e3 / (1000.0 * step_ms),
        'parts_ms': {k: stats(times[k]) for k in parts},
        'new_kernels_ms': {'row_dist_features': stats(times['row_dist_features']), 'row_dist_pixels': stats(times['row_dist_pixels']),
                           'box_down_k2': stats(times['box_down_k2']), 'box_up_k2': stats(times['box_up_k2']), 'step_tail': stats(times['tail_fused'])},
        'tail_us': {'fused_one_launch': stats([1e3 * x for x in times['tail_fused']]),
                    'composed_%d_launches' % (4 if L == 1 else 3): stats([1e3 * x for x in times['tail_composed']])},
        'dist_ms': {'kernel': stats(times['dist_kernel']), 'torch': stats(times['dist_torch']),
                    'bytes_kernel': 3 * Cc * B * F * 4, 'largest_relative_difference_of_loss': float(np.abs(lk - lt).max() / np.abs(lt).max()),
                    'largest_difference_of_g': float((g_rows - res['g']).abs().max())},
    }
    if maps is not None:
        # the channel reductions read the stored gradient of every layer with noise once: B * cout * res^2 floats each
        nbytes = sum(4 * B * proj.synth.channels[proj.synth.block_resolutions.index(r)] * r * r for r in maps.res)
        extra_ms = float(np.median(times['synthesis_backward_with_noise_grads'])) - float(np.median(times['synthesis_backward']))
        out['noise'] = {'maps': len(maps.res), 'map_elements_per_sample': sum(r * r for r in maps.res), 'reduction_bytes': nbytes,
                        'reduction_ms_by_difference': extra_ms, 'reduction_GBps': nbytes / (extra_ms * 1e6) if extra_ms > 0 else None,
                        'regulariser_ms': stats(times['noise_regulariser']), 'tail_ms': stats(times['noise_tail'])}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
