"""Dev tool: are the outputs of the four engines byte-equal on two builds of the library?
    python scripts/check_engine_bits.py tmp_libs/base/liblatentaug_hip.so latentaugment_amd/liblatentaug_hip.so
Each library runs the same calls in a fresh process of its own (`--dump LIB OUT.npz`, the library path replacing _lib.LIB_PATH before
anything loads it, as scripts/check_op_bits.py does); this process only compares the bytes and prints one line.  The cases are the
smallest that reach every host branch of the engines' launch set-up (la_synth.hip / la_modconv.hip, la_disc.hip, la_feat.hip), each in
f32, bf16x3 and f16x2:
  generator      64^2, channel cap 64, B = 3, const noise: split-K grids, merged up-2 phases, the fused ToRGB at 64^2 x 64 channels;
                 image, then d/d(ws) of a seeded image gradient; once more with the row window (13, 52) (gradient zero outside it)
  discriminator  128^2, channel cap 32, B = 4: the packed FIR operand, blocks whose gradient arrives with slot rows, the masked FromRGB
                 backward above 64^2; logits and image gradient.  And 16^2, B = 8, MinibatchStd group 4
  feature net    conv, conv, tap, maxpool, conv, tap on a 3-channel 12^2 input, N = 3: the padded first-conv gradient copy, both sources
                 of the ReLU mask; features and input gradient
  detector       conv, maxpool, conv, fc + ReLU, fc: features (its fc layers are 3 x 128 -> 12 and 3 x 12 -> 5: la_fc_mfma_kernel<1, true>,
                 one slice, 4 chunks and 1)
  fc             la_fc_bias_act_f32 itself, f32 only: (N, K, O) = (3, 70, 5), one 32-row block, scalar loads, 3 chunks in one slice, ragged
                 everywhere; (33, 288, 130), two blocks, 16-byte loads, 9 chunks in slices of 5 and 4, two output tiles, the finish pass
  general convs  f32 only, 13^2 input, N = 2: conv 3 -> 8 k 5 stride 2 pad 2, 3x3 stride-2 pool (ceil), conv 8 -> 32, conv 32 -> 8, tap.  The
                 last conv's forward and the 8 -> 32 layer's data gradient split K (288 = 9 chunks in 2 slices), the others run in one slice,
                 the first layer takes the gather backward; features and input gradient
  loop           LatentAug above them (la_latent_opt.hip): every branch of its schedule decision.  The 64^2 generator, a 64^2 discriminator
                 (channel cap 32), the feature net at crop_size_aug 12, banks W [16], X [8], fea [8]; 3 steps, const noise, f16x2; one loop per
                 handle (stream_lanes 1, so that a handle re-captures) except in c.  img and w_aug of every batch of
                   a  w_latent + w_pix, batches of 4, 4, 2, 4 (windowed steps; re-capture on a new batch size), captured and eager
                   b  all four criteria, overlap_criteria 0 / 1 / 2 x captured / eager, batches of 4, 4, 2, crop at (0, 0), (3, 1), (3, 1)
                   c  all four criteria, batch 8 on two stream lanes (split replay in each lane; the first-batch self-check), two batches
                   d  W+ with w_latent + w_pix + w_lpips, batch 2, two batches
                   e  all four criteria, batch 1 with loss scalars, per-criterion timers and the w / img / grad traces: those too
Inputs: seeded CPU generators."""
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('f32', 'bf16x3', 'f16x2')


def dump(lib_path, out_path):
    sys.path.insert(0, ROOT)
    import torch
    from latentaugment_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    import ctypes
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for k in list(_lib.SIGNATURES):      # (entries the other build lacks are dropped from the binding table, as scripts/bench_with_lib.py does)
        if not hasattr(probe, k):
            del _lib.SIGNATURES[k]
    from latentaugment_amd import synthesis, synthetic
    lib = _lib.load()
    assert _lib.LOADED_PATH == os.path.realpath(lib_path)
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    res = {}

    def draw(*shape):
        return torch.randn(shape, generator=gen).to(dev)

    def keep(key, t):
        res[key] = t.detach().contiguous().cpu().view(torch.uint8).numpy().ravel()

    g_sd, meta = synthetic.make_generator_state_dict(64, 2, channel_max=64, w_dim=64, noise_strength=0.1)
    ws, g_img = draw(3, meta['num_ws'], 64), draw(3, 2, 64, 64)
    g_win = torch.zeros_like(g_img)
    g_win[:, :, 13:52] = g_img[:, :, 13:52]
    d128 = synthetic.make_discriminator_state_dict(128, 2, channel_max=32)
    d16 = synthetic.make_discriminator_state_dict(16, 2, channel_max=32)
    x128, dl4, x16, dl8 = draw(4, 2, 128, 128), draw(4, 1), draw(8, 2, 16, 16), draw(8, 1)

    def conv(cin, cout):
        return ('conv', draw(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, draw(cout) * 0.1)

    f_ops = [conv(3, 8), conv(8, 8), ('tap', draw(8).abs()), ('maxpool',), conv(8, 16), ('tap', draw(16).abs())]
    d_ops = [conv(3, 8), ('maxpool',), conv(8, 8), ('fc', draw(12, 8 * 4 * 4) * 0.1, draw(12) * 0.1, True), ('fc', draw(5, 12), draw(5), False)]
    xf, xd = draw(3, 3, 12, 12), draw(3, 3, 8, 8)

    for mode in MODES:
        G = synthesis.SynthesisEngine.from_generator(g_sd, dev, max_batch=3, conv_clamp=256.0, precision=mode)
        keep(f'gen/{mode}/img', G.forward(ws, noise_mode='const'))
        keep(f'gen/{mode}/dws', G.backward(g_img))
        _lib.check(lib.la_synth_set_row_window(G.handle, 13, 52), 'la_synth_set_row_window')
        img = G.forward(ws, noise_mode='const', out=torch.zeros_like(g_img))
        keep(f'gen/{mode}/window/img', img[:, :, 13:52])      # (the rows outside are not written)
        keep(f'gen/{mode}/window/dws', G.backward(g_win))
        for name, sd, x, dl, group in (('disc128', d128, x128, dl4, 4), ('disc16', d16, x16, dl8, 4)):
            D = synthesis.DiscriminatorEngine(sd, dev, max_batch=x.shape[0], precision=mode, mbstd_group_size=group)
            keep(f'{name}/{mode}/logits', D.forward(x))
            keep(f'{name}/{mode}/gx', D.backward(dl))
        F = synthesis.FeatureEngine(f_ops, dev, in_res=12, max_batch=3, precision=mode)
        f = F.forward(xf)
        keep(f'feat/{mode}/f', f)
        keep(f'feat/{mode}/gx', F.backward(torch.randn(f.shape, generator=torch.Generator().manual_seed(1)).to(dev)))
        keep(f'detector/{mode}/f', synthesis.FeatureEngine(d_ops, dev, in_res=8, max_batch=3, precision=mode).forward(xd))
    for N, K, O in ((3, 70, 5), (33, 288, 130)):
        for relu in (False, True):
            keep(f'fc/{N}x{K}x{O}/relu{int(relu)}', synthesis.fc_bias_act(draw(N, K), draw(O, K) * K ** -0.5, draw(O), relu=relu))

    def convg(cin, cout, k, stride, pad):
        return ('conv', draw(cout, cin, k, k) * (2.0 / (k * k * cin)) ** 0.5, draw(cout) * 0.1, stride, pad)

    g_ops = [convg(3, 8, 5, 2, 2), ('maxpool3', True), convg(8, 32, 3, 1, 1), convg(32, 8, 3, 1, 1), ('tap', draw(8).abs())]
    Fg = synthesis.FeatureEngine(g_ops, dev, in_res=13, max_batch=2, precision='f32')
    f = Fg.forward(draw(2, 3, 13, 13))
    keep('featconv/f', f)
    keep('featconv/gx', Fg.backward(torch.randn(f.shape, generator=torch.Generator().manual_seed(2)).to(dev)))
    loop_cases(dev, lib, g_sd, meta, f_ops, draw, keep)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def loop_cases(dev, lib, g_sd, meta, f_ops, draw, keep):
    import ctypes
    import torch
    from latentaugment_amd import _lib, synthesis, synthetic
    from latentaugment_amd.latent_aug import LatentAug
    d64 = synthetic.make_discriminator_state_dict(64, 2, channel_max=32)
    F = synthesis.FeatureEngine(f_ops, dev, in_res=12, max_batch=2, precision='f16x2').num_features
    banks = {'W': draw(16, meta['num_ws'], 64), 'X': draw(8, 2, 64, 64).clamp(-1, 1), 'fea': [draw(8, F) * (1.0 / F) ** 0.5 for _ in range(2)]}
    w, wp = draw(8, 1, 64), draw(2, meta['num_ws'], 64)
    all4 = dict(w_latent=0.3, w_pix=1.0, w_disc=0.5, w_lpips=2.0)

    def make(batch, **kw):
        opt = types.SimpleNamespace(img_resolution=64, batch_size=batch, modalities_aug='A,B', opt_num_epochs=3, opt_lr=0.01, truncation_psi=1.0,
                                    w_pix=0.0, w_lpips=0.0, w_latent=0.0, w_disc=0.0, crop_size_aug=12, preprocess_aug='center_random_crop',
                                    soft_aug=False, alpha=1.0, verbose_log=False, criterion_mode='gemm', final_noise_mode='const',
                                    precision='f16x2', stream_lanes=1)
        opt.__dict__.update(kw)
        return LatentAug('train', opt, None, [0], generator=g_sd, discriminator=d64 if opt.w_disc > 0 else None, banks=dict(banks),
                         feature_net=f_ops if opt.w_lpips > 0 else None)

    def batches(key, la, runs):
        for i, (wb, pos) in enumerate(runs):
            la.crop_params = {'crop_pos': pos}      # (what forward() draws once per batch)
            img, w_aug, _ = la.run_batch(wb)
            keep(f'loop/{key}/batch{i}/img', img)
            keep(f'loop/{key}/batch{i}/w_aug', w_aug)

    for graph in (True, False):
        batches(f'a/graph{int(graph)}', make(4, w_latent=0.3, w_pix=1.0, hip_graph=graph), [(w[:4], (0, 0)), (w[4:], (0, 0)), (w[:2], (0, 0)), (w[:4], (0, 0))])
        for overlap in (0, 1, 2):
            batches(f'b/overlap{overlap}/graph{int(graph)}', make(4, hip_graph=graph, overlap_criteria=overlap, **all4),
                    [(w[:4], (0, 0)), (w[4:], (3, 1)), (w[:2], (3, 1))])
    la = make(8, stream_lanes=2, **all4)
    batches('c', la, [(w, (3, 1)), (w.flip(0), (3, 1))])
    assert la.lanes_active and la.lanes_selfcheck == 'bit-identical', la.lanes_selfcheck
    batches('d', make(2, latent_space='w+', w_latent=0.3, w_pix=1.0, w_lpips=2.0), [(wp, (3, 1)), (wp.flip(0), (3, 1))])
    la, trace = make(1, **all4), {'want': ('w', 'img', 'grad')}
    _lib.check(lib.la_latent_opt_set_time_trace(la._h, 1), 'la_latent_opt_set_time_trace')
    img, w_aug, losses = la.run_local(w[:1], want_losses=True, crop_pos=(3, 1), trace=trace)
    torch.cuda.synchronize()
    _lib.check(lib.la_latent_opt_get_times(la._h, (ctypes.c_float * 15)()), 'la_latent_opt_get_times')
    for name, t in (('img', img), ('w_aug', w_aug), ('losses', losses), ('trace_w', trace['w']), ('trace_img', trace['img']), ('trace_grad', trace['grad'])):
        keep(f'loop/e/{name}', t)


def main():
    if sys.argv[1] == '--dump':
        return dump(sys.argv[2], sys.argv[3])
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, f'engine_bits_{i}.npz')
            subprocess.run([sys.executable, os.path.abspath(__file__), '--dump', lib, out], check=True, timeout=300)
            outs.append(dict(np.load(out)))
    a, b = outs
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not np.array_equal(a[k], b[k])]
    print(f'engine_bits: {len(a)} outputs, {sum(a[k].size for k in a)} bytes, {len(differ)} differ' +
          ''.join(f'\n  {k}' for k in differ[:20]))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
