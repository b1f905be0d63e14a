"""W+ latent optimisation on the GPU (opt.latent_space = 'w+'): the HIP loop against the reference's W+ run (tests/golden/wplus_loop.npz),
its exact link to the W loop, its schedules (captured step, stream lanes, two ranks) and a full-size run against float64."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import feature_net as fnets   # noqa: E402
from oracle import sg2_networks as nets   # noqa: E402
import wplus_cpu                          # noqa: E402

CASES = {
    'latent': dict(w_latent=0.5),
    'pix': dict(w_pix=2.0),
    'disc': dict(w_disc=1.0),
    'lpips': dict(w_lpips=3.0),
    'all': dict(w_latent=0.3, w_pix=1.0, w_disc=0.5, w_lpips=2.0),
    'soft': dict(w_latent=0.3, w_pix=1.0, soft_aug=True, alpha=0.7),
}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gw(golden_dir):
    return np.load(os.path.join(golden_dir, 'wplus_loop.npz'))


def close(a, b, rtol=1e-4, atol=1e-5):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def _opt(**kw):
    o = types.SimpleNamespace(
        img_resolution=32, batch_size=2, modalities_aug='A,B', opt_num_epochs=5, opt_lr=0.01, truncation_psi=1.0,
        w_pix=0.0, w_lpips=0.0, w_latent=0.0, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop',
        soft_aug=False, alpha=1.0, verbose_log=False, criterion_mode='gemm', final_noise_mode='const', precision='f32',
        latent_space='w+')
    o.__dict__.update(kw)
    return o


def _nets(gw):
    kw = dict(img_resolution=int(gw['res']), img_channels=2, channel_base=int(gw['cbase']), channel_max=int(gw['cmax']), seed=0)
    G = nets.make_generator(noise_strength=0.1, w_dim=int(gw['wdim']), mapping_layers=2, **kw)
    D = nets.make_discriminator(**kw)
    return G, D


def _banks(gw):
    return {'W': torch.tensor(gw['W']), 'X': torch.tensor(gw['X']), 'fea': [torch.tensor(gw['fea0']), torch.tensor(gw['fea1'])]}


def _aug(gw, **kw):
    from latentaugment_amd.latent_aug import LatentAug
    G, D = _nets(gw)
    fnet = fnets.TinyFeatureNet(seed=5, crop=8)
    return LatentAug('train', _opt(**kw), '/tmp', [0], generator=G, discriminator=D, banks=_banks(gw), feature_net=fnets.tiny_ops(fnet))


@pytest.mark.parametrize('name', list(CASES))
def test_wplus_loop_vs_reference_golden(dev, gw, name):
    """Every case of the reference's W+ run: w_aug after 5 Adam steps, the final image (the reference's own 'random' noise draws, passed
    as explicit noise) and the weighted loss scalars of every step."""
    la = _aug(gw, final_noise_mode='random', **CASES[name])
    assert la.wplus and la.latent_rows == la.num_ws
    noises = [torch.tensor(gw[f'noise_{k}']).to(dev) for k in range(int(gw['num_noises']))]
    assert [n.shape[-1] for n in noises] == list(la.engine.layer_resolutions)
    pos = tuple(int(v) for v in gw[f'{name}_crop_pos'])
    img, w_aug, losses = la.run_local(torch.tensor(gw['w0']).to(dev), noises, want_losses=True, crop_pos=pos)
    close(w_aug, gw[f'{name}_w_aug'], rtol=1e-4, atol=3e-5)
    ref_img = gw[f'{name}_img']
    close(img, ref_img, rtol=1e-3, atol=5e-4 * float(np.abs(ref_img).max()))
    L, Lr = losses.cpu().numpy(), gw[f'{name}_losses']
    for col in range(4):
        close(L[:, col], Lr[:, col], rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(Lr[:, col]).max())))
    # the replayed step (second batch, captured graph) gives the same latents
    _, w_aug2, _ = la.run_local(torch.tensor(gw['w0']).to(dev), noises, crop_pos=pos)
    assert la.graph_state == 1
    close(w_aug2, w_aug, rtol=0, atol=0)


def test_wplus_float64_anchor(dev, gw):
    """The 'all' case against its float64 run: the HIP loop is no further from float64 than the float32 reference run is (plus a
    float32 floor)."""
    la = _aug(gw, **CASES['all'])
    pos = tuple(int(v) for v in gw['all_crop_pos'])
    _, w_aug, _ = la.run_local(torch.tensor(gw['w0']).to(dev), crop_pos=pos)
    e_h = np.abs(w_aug.cpu().numpy().astype(np.float64) - gw['all_f64_w_aug'])
    e_r = np.abs(gw['all_w_aug'].astype(np.float64) - gw['all_f64_w_aug'])
    print(f'[W+ all] vs float64: HIP max {e_h.max():.2e} rms {np.sqrt((e_h ** 2).mean()):.2e}; reference float32 max {e_r.max():.2e}')
    assert np.sqrt((e_h ** 2).mean()) <= 1.5 * np.sqrt((e_r ** 2).mean()) + 1e-6 and e_h.max() <= 2 * e_r.max() + 1e-5


@pytest.mark.parametrize('kw', [dict(w_pix=1.0), dict(w_pix=1.0, w_disc=0.5, w_lpips=2.0)])
def test_wplus_gradient_is_the_per_slot_w_gradient(dev, gw, kw):
    """From a broadcast W latent with w_latent = 0, the step-1 W+ gradient dL/dw+ [b, num_ws, w_dim] summed over the slots is the W
    loop's dL/dw: the same synthesis backward feeds both, W sums its slots inside la_step_tail."""
    w = torch.tensor(gw['w0'])[:, :1].contiguous()
    pos = tuple(int(v) for v in gw['all_crop_pos'])
    grads = {}
    for space in ('w', 'w+'):
        la = _aug(gw, latent_space=space, **kw)
        x = w if space == 'w' else w.repeat(1, la.num_ws, 1)
        tr = {'want': ('w', 'grad')}
        la.run_local(x.to(dev), crop_pos=pos, trace=tr)
        grads[space] = tr['grad'][0].double().cpu().numpy()
    assert grads['w'].shape == (2, 32) and grads['w+'].shape == (2, grads['w+'].shape[1], 32)
    gsum = grads['w+'].sum(axis=1)
    assert np.abs(grads['w+'] - grads['w+'][:, :1]).max() > 0          # the slots do get different gradients
    np.testing.assert_allclose(gsum, grads['w'], rtol=1e-6, atol=1e-6 * float(np.abs(grads['w']).max()))


@pytest.mark.parametrize('kw', [dict(w_latent=0.3, w_pix=1.0), dict(w_latent=0.3, w_pix=1.0, w_disc=0.5, w_lpips=2.0)])
def test_wplus_graph_replay_is_bit_identical_to_eager(dev, gw, kw):
    g = torch.Generator().manual_seed(8)
    w = torch.cat([torch.tensor(gw['w0']), torch.randn([2, gw['w0'].shape[1], 32], generator=g)]).to(dev)       # 4 samples
    runs = {}
    for mode in (True, False):
        la = _aug(gw, batch_size=4, hip_graph=mode, precision='f16x2', **kw)
        out = []
        for wb, pos in ((w, (0, 0)), (w, (0, 0)), (w[:2], (3, 1)), (w, (5, 2))):
            img, w_aug, _ = la.run_local(wb, crop_pos=pos)
            out.append((img.clone(), w_aug.clone()))
        assert la.graph_state == (1 if mode else 0)
        runs[mode] = out
    for (ig, wg), (ie, we) in zip(runs[True], runs[False]):
        assert torch.equal(wg, we) and torch.equal(ig, ie)


def test_wplus_stream_lanes(dev, gw):
    """Batch 8: the lanes take it, their first-batch self-check finds side by side == one after the other, and the result is the
    single loop's (batch of 8 normalisation in both) at the plain loop tolerance."""
    g = torch.Generator().manual_seed(8)
    w = torch.cat([torch.tensor(gw['w0']), torch.randn([6, gw['w0'].shape[1], 32], generator=g)]).to(dev)
    kw = dict(w_latent=0.3, w_pix=1.0, batch_size=8, precision='f16x2')
    la = _aug(gw, **kw)
    la.crop_params = {'crop_pos': (3, 1)}
    img, w_aug, _ = la.run_batch(w)
    assert la.lanes_active and la.lanes_selfcheck == 'bit-identical' and la._lanes[0].wplus
    one = _aug(gw, stream_lanes=1, **kw)
    img1, w1, _ = one.run_local(w, crop_pos=(3, 1))
    d = (w_aug - w1).abs().cpu().numpy()
    assert (d > 3e-5 + 1e-4 * w1.abs().cpu().numpy()).mean() <= 0.01 and d.max() <= 2e-3, float(d.max())
    close(img, img1, rtol=1e-3, atol=2e-3 * float(img1.abs().max()))


_RANK_WORKER = r"""
import os, sys, types, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from latentaugment_amd.latent_aug import LatentAug
from oracle import sg2_networks as nets
rank = int(sys.argv[3])
if rank >= 0:
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % sys.argv[2], rank=rank, world_size=2)
gw = np.load(os.path.join(sys.argv[1], 'tests', 'golden', 'wplus_loop.npz'))
G = nets.make_generator(img_resolution=32, img_channels=2, channel_base=256, channel_max=16, seed=0, noise_strength=0.1, w_dim=32,
                        mapping_layers=2)
opt = types.SimpleNamespace(img_resolution=32, batch_size=3, modalities_aug='A,B', opt_num_epochs=5, opt_lr=0.01, truncation_psi=1.0,
                            w_pix=1.0, w_lpips=0.0, w_latent=0.3, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop',
                            soft_aug=False, alpha=1.0, verbose_log=False, criterion_mode='gemm', final_noise_mode='const', precision='f32',
                            latent_space='w+', max_local_batch=2)
la = LatentAug('train', opt, '/tmp', [0], generator=G, banks={'W': torch.tensor(gw['W']), 'X': torch.tensor(gw['X'])})
g = torch.Generator().manual_seed(4)
w = torch.cat([torch.tensor(gw['w0']), torch.randn([1, G.num_ws, 32], generator=g)])      # B = 3 over 2 ranks: shards of 2 and 1
if rank >= 0:
    img, w_aug = la.forward(w.cuda(), ['a', 'b', 'c'])                                      # sharded + ONE all_gather
else:                                                                                       # single process, shard by shard
    outs = [la.forward(w[s].cuda(), None) for s in (slice(0, 2), slice(2, 3))]
    img, w_aug = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
assert img.shape == (3, 2, 32, 32) and w_aug.shape == (3, G.num_ws, 32)
np.save(sys.argv[4] + f'/w_aug_{rank}.npy', w_aug.cpu().numpy())
np.save(sys.argv[4] + f'/img_{rank}.npy', img.cpu().numpy())
if rank >= 0:
    dist.barrier(); dist.destroy_process_group()
print('ok', rank)
"""


def test_wplus_two_rank_sharded_forward_matches_single_process(dev, tmp_path):
    """2 ranks (gloo rendezvous, both on cuda:0) shard a W+ batch of 3 and gather once; every rank holds the batch a single process
    computes shard by shard (the criteria normalise by the local batch, as a DataParallel replica's do)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'rank.py'
    script.write_text(_RANK_WORKER)
    port = str(29700 + (os.getpid() + 500) % 1000)
    procs = [subprocess.Popen([sys.executable, str(script), root, port, str(r), str(tmp_path)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]
    single = subprocess.run([sys.executable, str(script), root, port, '-1', str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            timeout=300)
    assert single.returncode == 0, single.stdout.decode()[-2000:]
    w0, w1, ws = (np.load(tmp_path / f'w_aug_{r}.npy') for r in (0, 1, -1))
    np.testing.assert_array_equal(w0, w1)
    np.testing.assert_array_equal(np.load(tmp_path / 'img_0.npy'), np.load(tmp_path / 'img_1.npy'))
    close(w0, ws, rtol=1e-5, atol=1e-6)
    close(np.load(tmp_path / 'img_0.npy'), np.load(tmp_path / 'img_-1.npy'), rtol=1e-4, atol=1e-5)


def test_wplus_full_size_vs_float64(dev):
    """Config-f 256^2, batch 4, 3 steps, pixel + latent criteria, W+ latents and bank with distinct rows: at every step the HIP loop
    (default f16x2 contraction) is no further from the float64 W+ oracle than the float32 W+ oracle is (rms over the batch's latents,
    slack 1.5 as for the full-size W configurations), and so is the first step's gradient."""
    from latentaugment_amd import synthetic
    from latentaugment_amd.latent_aug import LatentAug
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd, meta = synthetic.make_generator_state_dict(img_resolution=256, img_channels=2, channel_base=32768, seed=0)
    G = nets.Generator(img_resolution=256, img_channels=2, channel_base=32768)
    G.load_state_dict(sd, strict=False)
    G = G.eval().requires_grad_(False)
    nws = meta['num_ws']
    g = torch.Generator().manual_seed(11)
    W, X = synthetic.make_banks(nws, res=256, M_w=256, M_x=64)
    W = W + 0.3 * torch.randn(W.shape, generator=g)
    w0 = synthetic.make_latents(4).repeat(1, nws, 1) + 0.3 * torch.randn([4, nws, 512], generator=g)
    kw = dict(res=256, num_epochs=3, opt_lr=0.01, crop_size=64, w_latent=0.001, w_pix=0.1, final_noise_mode='const')
    ref = wplus_cpu.LatentAugRefWPlus(G, None, W=W, X=X, **kw)
    _, w32 = ref.forward(w0, crop_pos=(0, 0), record=True)
    s32, g32 = torch.stack(ref.trace['w']).double().numpy(), ref.trace['grad'][0].double().numpy()
    _, w64, tr64 = wplus_cpu.run_f64(kw, G, None, W, X, None, None, w0, (0, 0))
    s64, g64 = torch.stack(tr64['w']).double().numpy(), tr64['grad'][0].double().numpy()
    opt = _opt(img_resolution=256, batch_size=4, opt_num_epochs=3, w_latent=0.001, w_pix=0.1, crop_size_aug=64, precision='f16x2')
    la = LatentAug('train', opt, '/tmp', [0], generator=sd, banks={'W': W, 'X': X})
    tr = {'want': ('w', 'grad')}
    _, w_aug, _ = la.run_local(w0.to(dev), trace=tr)
    sh, gh = tr['w'].double().cpu().numpy(), tr['grad'][0].double().cpu().numpy()
    assert sh.shape == s64.shape == (3, 4, nws, 512)
    rms = (lambda e: float(np.sqrt((e ** 2).mean())))
    eg_h, eg_r = rms(gh - g64), rms(g32 - g64)
    print(f'[W+ full size] dL/dw+ step 1 vs float64: HIP rms {eg_h:.2e}, float32 oracle {eg_r:.2e}')
    assert eg_h <= 1.5 * eg_r + 1e-12
    for s in range(3):
        e_h, e_r = rms(sh[s] - s64[s]), rms(s32[s] - s64[s])
        print(f'[W+ full size] step {s + 1} latent vs float64: HIP rms {e_h:.2e}, float32 oracle {e_r:.2e}')
        assert e_h <= 1.5 * e_r + 1e-9, (s, e_h, e_r)
    close(w_aug, sh[-1], rtol=0, atol=0)
