"""The AlexNet / SqueezeNet LPIPS nets on the GPU: the general convolution, the 3x3 stride-2 pool and the Fire op alone, the reference's own
LPIPS class around both trunks (tests/golden/lpips_nets.npz), exactness properties, the full-width nets, the plugin's lpips_net option,
the LPIPS metrics on an alex engine, misuse and guard bands.

Bound (the project's rule, lpips_cases.bound, nothing tuned): error <= 4 x the float32 yardstick's own error + 2e-6 x the largest float64
magnitude.  Yardstick: the reference's float32 run for the goldens, the float32 restatement of tests/lpips_net_cases.py otherwise; anchor:
the reference's float64 run / the float64 restatement (pinned to the reference to 1e-12 by test_lpips_net_cases_cpu.py).

Bit-for-bit checks go through a twin: the engine has no layer-level access, but a tap-only engine fed the expected activation runs the
same tap kernels on it, so [op, tap] and the twin give the same bits exactly when the op's output has the expected bits ("the tap's
rsqrt aside"); the twin's backward likewise hands out the bits of the gradient that enters the op."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import lpips_net_cases as nc  # noqa: E402
import ppl_cases as pc  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
NETS = ('alex', 'squeeze')
CASES = [(net, R) for net in NETS for R in nc.SIZES[net]]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gn(golden_dir):
    return np.load(os.path.join(golden_dir, 'lpips_nets.npz'))


def _engine_of(ops, dev, R, N, in_ch=3, precision='f32'):
    from latentaugment_amd.synthesis import FeatureEngine
    return FeatureEngine(ops, dev, in_res=R, max_batch=N, in_ch=in_ch, precision=precision)


def _f32(ops):
    return nc.cast_ops(ops, torch.float32)


def _restated(ops64, x64, gfeat64):
    """(feature vector, d(sum gfeat . feat)/dx) of the restatement in float64 and in float32: ((f64, g64), (f32, g32)) numpy."""
    out = []
    for dtype in (torch.float64, torch.float32):
        x = x64.to(dtype).clone().requires_grad_(True)
        f = nc.feature_vector(nc.cast_ops(ops64, dtype), x, 'engine')
        (g,) = torch.autograd.grad((f * gfeat64.to(dtype)).sum(), [x])
        out.append((f.detach().double().numpy(), g.double().numpy()))
    return out


def _check_op(name, dev, ops64, x64, in_ch, seed=5):
    """forward and backward of the list on x against the restatement under the budget; returns the engine and its feature vector."""
    N, R = x64.shape[0], x64.shape[2]
    eng = _engine_of(_f32(ops64), dev, R, N, in_ch)
    f = eng.forward(x64.float().to(dev))
    gfeat = torch.randn(list(f.shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float().double()
    gx = eng.backward(gfeat.float().to(dev))
    (f64, g64), (f32, g32) = _restated(ops64, x64, gfeat)
    lc.check(f'{name} forward', f.cpu(), f64, f32)
    lc.check(f'{name} gradient', gx.cpu(), g64, g32)
    assert torch.equal(eng.forward(x64.float().to(dev)), f) and torch.equal(eng.backward(gfeat.float().to(dev)), gx)      # repeat bits
    return eng, f, gfeat


def _twin(dev, lin, y, gfeat):
    """A tap-only engine on the activation y [N, C, r, r]: (its feature vector, the gradient that enters whatever produced y)."""
    if y.shape[2] == 1:
        # one pixel: a tap-only list needs a 2 x 2 input.  [ceil-mode pool, tap] on the plane filled with y pools to y exactly, and the
        # pool's gradient lands on the first maximum, the corner pixel (torch's tie rule, tested on its own)
        eng = _engine_of([('maxpool3', True), ('tap', lin.float())], dev, 2, y.shape[0], in_ch=y.shape[1])
        f = eng.forward(y.float().expand(-1, -1, 2, 2).contiguous().to(dev))
        g = eng.backward(gfeat.float().to(dev))
        assert not bool(g[:, :, 1:, :].any()) and not bool(g[:, :, :, 1:].any())
        return f, g[:, :, :1, :1].contiguous()
    eng = _engine_of([('tap', lin.float())], dev, y.shape[2], y.shape[0], in_ch=y.shape[1])
    f = eng.forward(y.float().to(dev))
    return f, eng.backward(gfeat.float().to(dev))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the convolution alone

@pytest.mark.parametrize('cin,cout,k,s,p,R,N', nc.CONV_CASES)
def test_conv_alone_exact_integers(dev, cin, cout, k, s, p, R, N):
    """Small-integer inputs, weights and biases: every float32 product and partial sum is an integer below 2^24, so the convolution is
    exact in any summation order and its output must have the bits of the float64 answer -- through the twin, which also hands out the
    gradient entering the convolution; the input gradient is then checked under the budget (its incoming gradient is no integer)."""
    g = torch.Generator().manual_seed(100 * cin + k + R)
    x = nc.small_ints(g, [N, cin, R, R], -3, 3)
    w, b = nc.small_ints(g, [cout, cin, k, k], -2, 2), nc.small_ints(g, [cout], 0, 6)
    lin = torch.ones([cout], dtype=torch.float64)
    ops = [('conv', w, b, s, p), ('tap', lin)]
    y = F.relu(F.conv2d(x, w, b, stride=s, padding=p))
    assert float(y.abs().max()) < 2 ** 24 and float((y > 0).double().mean()) > 0.2
    eng, f, gfeat = _check_op(f'conv int {cin}->{cout} k{k} s{s} p{p} R{R}', dev, ops, x, cin)
    f_twin, g_y = _twin(dev, lin, y, gfeat)
    assert torch.equal(f, f_twin)
    # the data gradient from the bits of the gradient that enters it: float64 transposed convolution of the masked g_y
    gy64 = g_y.cpu().double() * (y > 0)
    want = torch.nn.grad.conv2d_input(list(x.shape), w, gy64, stride=s, padding=p)
    gx = eng.backward(gfeat.float().to(dev)).cpu()
    x32 = x.float()
    yard = torch.nn.grad.conv2d_input(list(x32.shape), w.float(), gy64.float(), stride=s, padding=p)
    lc.check('gradient from the twin', gx, want, yard)


@pytest.mark.parametrize('cin,cout,k,s,p,R,N', nc.CONV_CASES)
def test_conv_alone_floats(dev, cin, cout, k, s, p, R, N):
    g = torch.Generator().manual_seed(200 * cin + k + R)
    x = torch.randn([N, cin, R, R], generator=g, dtype=torch.float64).float().double()
    w = (torch.randn([cout, cin, k, k], generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5).float().double()
    b = (torch.rand([cout], generator=g, dtype=torch.float64) * 0.3 + 0.3).float().double()
    lin = torch.rand([cout], generator=g, dtype=torch.float64).float().double()
    _check_op(f'conv {cin}->{cout} k{k} s{s} p{p} R{R}', dev, [('conv', w, b, s, p), ('tap', lin)], x, cin)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the pool alone

def _pool_case(dev, x, ceil):
    """x [N, C, R, R] float32 values: forward and backward of [maxpool3, tap] against torch, bit for bit (through the twin)."""
    N, C, R = x.shape[0], x.shape[1], x.shape[2]
    lin = torch.ones([C])
    eng = _engine_of([('maxpool3', ceil), ('tap', lin)], dev, R, N, in_ch=C)
    xg = x.clone().requires_grad_(True)
    y = F.max_pool2d(xg, 3, 2, ceil_mode=ceil)
    f = eng.forward(x.to(dev))
    assert f.shape[1] == C * y.shape[2] * y.shape[3]      # torch's output size, partial and dropped windows included
    gfeat = torch.randn(list(f.shape), generator=torch.Generator().manual_seed(R))
    f_twin, g_y = _twin(dev, lin, y.detach(), gfeat)
    assert torch.equal(f, f_twin)
    (want,) = torch.autograd.grad(y, [xg], g_y.cpu())
    assert torch.equal(eng.backward(gfeat.to(dev)).cpu(), want)


@pytest.mark.parametrize('ceil', [False, True])
@pytest.mark.parametrize('R', nc.POOL_RES)
def test_pool_alone(dev, R, ceil):
    g = torch.Generator().manual_seed(R)
    N, C = 2, 5
    distinct = torch.randperm(N * C * R * R, generator=g).float().reshape(N, C, R, R) - 40.0
    _pool_case(dev, distinct, ceil)
    # ties: torch gives the gradient to the first maximum in scan order.  An all-zero plane is what a dead ReLU channel leaves; which
    # of its zeros is "first" cannot reach the net's input, because the ReLU mask of the convolution below multiplies them all by zero.
    _pool_case(dev, torch.full([N, C, R, R], 1.5), ceil)
    _pool_case(dev, torch.zeros([N, C, R, R]), ceil)
    mixed = distinct.clone().clamp_min(0)
    _pool_case(dev, mixed, ceil)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the Fire op alone

@pytest.mark.parametrize('R', [4, 1])
@pytest.mark.parametrize('cin,sq,e1,e3', nc.FIRE_CASES)
def test_fire_alone(dev, cin, sq, e1, e3, R):
    g = torch.Generator().manual_seed(cin + R)
    he = lambda co, ci, k: (torch.randn([co, ci, k, k], generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5).float().double()      # noqa: E731
    bias = lambda n: (torch.rand([n], generator=g, dtype=torch.float64) * 0.3 + 0.1).float().double()      # noqa: E731
    fire = ('fire', he(sq, cin, 1), bias(sq), he(e1, sq, 1), bias(e1), he(e3, sq, 3), bias(e3))
    lin = torch.rand([e1 + e3], generator=g, dtype=torch.float64).float().double()
    x = torch.randn([2, cin, R, R], generator=g, dtype=torch.float64).float().double()
    if R > 1:
        _check_op(f'fire {cin} {sq} {e1} {e3} R{R}', dev, [fire, ('tap', lin)], x, cin)
    else:      # one pixel: the engine's input is at least 2 x 2; a 1 x 1 general conv and a ceil-mode pool bring it down to one pixel
        pre_w, pre_b = he(cin, cin, 1), bias(cin)
        x2 = torch.randn([2, cin, 2, 2], generator=g, dtype=torch.float64).float().double()
        _check_op(f'fire {cin} {sq} {e1} {e3} R1', dev, [('conv', pre_w, pre_b, 1, 0), ('maxpool3', True), fire, ('tap', lin)], x2, cin)
    # small integers: the three convolutions are exact, the output has the bits of the float64 answer (through the twin)
    xi = nc.small_ints(g, [2, cin, 2 if R == 1 else R, 2 if R == 1 else R], -2, 2)
    ints = ('fire', nc.small_ints(g, [sq, cin, 1, 1], -1, 1), nc.small_ints(g, [sq], 0, 3), nc.small_ints(g, [e1, sq, 1, 1], -1, 1),
            nc.small_ints(g, [e1], 0, 3), nc.small_ints(g, [e3, sq, 3, 3], -1, 1), nc.small_ints(g, [e3], 0, 3))
    ones = torch.ones([e1 + e3], dtype=torch.float64)
    y = nc.tapped([ints, ('tap', ones)], xi, 'engine')
    s = F.relu(F.conv2d(xi, ints[1], ints[2]))
    y = torch.cat([F.relu(F.conv2d(s, ints[3], ints[4])), F.relu(F.conv2d(s, ints[5], ints[6], padding=1))], 1)
    eng = _engine_of(_f32([ints, ('tap', ones)]), dev, xi.shape[2], 2, in_ch=cin)
    f = eng.forward(xi.float().to(dev))
    f_twin, _ = _twin(dev, ones, y, torch.zeros(list(f.shape)))
    assert float(y.max()) > 0 and torch.equal(f, f_twin)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. goldens: the reference's own class

def _net(gn, net):
    from latentaugment_amd.synthesis import lpips_reference_net
    return lpips_reference_net(*nc.golden_state_dicts(gn, net), net)


_ENGINES = {}


def _engine(gn, dev, net, R, precision='f32', max_batch=8):
    from latentaugment_amd.synthesis import FeatureEngine
    key = (net, R, precision, max_batch)
    if key not in _ENGINES:
        _ENGINES[key] = FeatureEngine.from_net(_net(gn, net), dev, in_res=R, max_batch=max_batch, precision=precision)
    return _ENGINES[key]


def _fed(eng, a, dev):
    return lc.affine(nc.gray3(a, torch.float32), eng.pre_scale, eng.pre_shift).to(dev)


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
@pytest.mark.parametrize('net,R', CASES)
def test_golden_pairs(dev, gn, net, R, precision):
    from latentaugment_amd import metrics
    eng, key = _engine(gn, dev, net, R, precision), f'{net}{R}'
    assert eng.num_taps == nc.NTAPS[net]
    out = metrics.compute_lpips(torch.tensor(gn[f'{key}_x']).to(dev), torch.tensor(gn[f'{key}_y']).to(dev), eng)
    assert out['lpips_layers'].shape == (3, 1, eng.num_taps) and out['lpips_layers'].dtype == torch.float64
    lc.check(f'{key} {precision} per layer', out['lpips_layers'][:, 0], gn[f'{key}_layers64'], gn[f'{key}_layers32'])
    lc.check(f'{key} {precision} per pair', out['lpips'], gn[f'{key}_pair64'], gn[f'{key}_pair32'])
    d = eng.pair_distance(_fed(eng, gn[f'{key}_x'], dev), _fed(eng, gn[f'{key}_y'], dev)).cpu()
    lc.check(f'{key} {precision} pair_distance', d, gn[f'{key}_layers64'], gn[f'{key}_layers32'])


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
@pytest.mark.parametrize('net,R', CASES)
def test_golden_criterion_side(dev, gn, net, R, precision):
    """forward_tr and its gradient from what the criterion uses: the tap vectors, the pairwise L2 and FeatureEngine.backward."""
    from latentaugment_amd import ops as la_ops
    eng, key = _engine(gn, dev, net, R, precision), f'{net}{R}'
    fb = eng.forward(_fed(eng, gn[f'{key}_bank'], dev))
    f = eng.forward(_fed(eng, gn[f'{key}_x1'], dev))
    M = fb.shape[0]
    tr = la_ops.l2_loss_vectorized(f, fb, compute_mean=False).double().sum() / M
    lc.check(f'{key} {precision} forward_tr', tr.cpu().reshape(1), gn[f'{key}_tr64'].reshape(1), gn[f'{key}_tr32'].reshape(1))
    gfeat = 2.0 * (f - fb.mean(0, keepdim=True))
    gx = eng.backward(gfeat) * torch.tensor(eng.pre_scale, device=dev).reshape(1, 3, 1, 1)
    lc.check(f'{key} {precision} forward_tr gradient', gx.cpu(), gn[f'{key}_tr_grad64'], gn[f'{key}_tr_grad32'])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. exactness and history

@pytest.mark.parametrize('net,R', CASES)
def test_exactness_and_history(dev, gn, net, R):
    from latentaugment_amd.synthesis import FeatureEngine
    key = f'{net}{R}'
    eng = _engine(gn, dev, net, R)
    x, y = _fed(eng, gn[f'{key}_x'], dev), _fed(eng, gn[f'{key}_y'], dev)
    dxy = eng.pair_distance(x, y)
    assert torch.equal(eng.pair_distance(x, x), torch.zeros_like(dxy))
    assert torch.equal(eng.pair_distance(y, x), dxy) and torch.equal(eng.pair_distance(x, y), dxy)
    assert bool((dxy >= 0).all()) and bool((dxy > 0).any())
    # an engine used at N = 6 and then at N = 2 gives the bits of a fresh one (forward, backward, pair distance)
    used = FeatureEngine.from_net(_net(gn, net), dev, in_res=R, max_batch=6)
    six = torch.cat([x, y])
    gf6 = torch.randn([6, used.num_features], generator=torch.Generator().manual_seed(1)).to(dev)
    used.forward(six)
    used.backward(gf6)
    used.pair_distance(x, y)
    fresh = FeatureEngine.from_net(_net(gn, net), dev, in_res=R, max_batch=6)
    for e in (used, fresh):
        e.out = (e.forward(six[:2]), e.backward(gf6[:2]), e.pair_distance(x[:1], y[:1]))
    assert all(torch.equal(a, b) for a, b in zip(used.out, fresh.out))
    assert torch.equal(used.out[2], dxy[:1])      # (the pair kernel's value does not depend on the batch it ran in)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the real channel tables

@pytest.mark.parametrize('net,R', [('alex', 35), ('squeeze', 17)])
def test_full_width(dev, net, R):
    from latentaugment_amd.synthesis import FeatureEngine, lpips_reference_net
    sd, lin = nc.full_width_state_dicts(net)
    desc = lpips_reference_net({k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in lin.items()}, net)
    eng = FeatureEngine.from_net(desc, dev, in_res=R, max_batch=4)
    assert eng.num_taps == nc.NTAPS[net]
    g = torch.Generator().manual_seed(3)
    x, y = (lc.affine((torch.rand([2, 3, R, R], generator=g, dtype=torch.float64) * 2 - 1).float().double(), desc.pre_scale, desc.pre_shift).float().double()
            for _ in range(2))
    ops64 = nc.cast_ops(desc.ops, torch.float64)
    ref64 = nc.pair_distance(ops64, x, y, 'engine')
    yard = nc.pair_distance(_f32(desc.ops), x.float(), y.float(), 'engine')
    lc.check(f'{net} full width pair_distance', eng.pair_distance(x.float().to(dev), y.float().to(dev)).cpu(), ref64, yard)
    f = eng.forward(x.float().to(dev))
    gfeat = torch.randn(list(f.shape), generator=g, dtype=torch.float64).float().double()
    (f64, g64), (f32, g32) = _restated(ops64, x, gfeat)
    lc.check(f'{net} full width features', f.cpu(), f64, f32)
    lc.check(f'{net} full width input gradient', eng.backward(gfeat.float().to(dev)).cpu(), g64, g32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the plugin's lpips_net option

@pytest.mark.parametrize('net', NETS)
def test_plugin_lpips_net(dev, gn, golden_dir, tmp_path, net):
    """opt.lpips_script = 'lpips', opt.lpips_net = net with the two weight files on disk: the step-0 LPIPS loss of the toy loop (batch 1) is
    the reference's forward_tr of each modality's crop against its bank, as the fixture recorded it."""
    from latentaugment_amd import _lib
    from latentaugment_amd.latent_aug import LatentAug
    from latentaugment_amd.loop_options import LPIPS_NET_FILES
    from latentaugment_amd.synthesis import FeatureEngine, lpips_reference_net
    from oracle import sg2_networks as nets
    res, crop = nc.PLUGIN[net]
    ll = np.load(os.path.join(golden_dir, 'latent_loop.npz'))
    G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=int(ll['cbase']), channel_max=int(ll['cmax']),
                            seed=0, noise_strength=0.1, w_dim=int(ll['wdim']), mapping_layers=2)
    trunk, lin = nc.golden_state_dicts(gn, net)
    names = LPIPS_NET_FILES[net]
    torch.save(trunk, tmp_path / names[0])
    torch.save(lin, tmp_path / names[1])
    bank_eng = FeatureEngine.from_net(lpips_reference_net(trunk, lin, net), dev, in_res=crop, max_batch=8)
    fea = [bank_eng.forward(_fed(bank_eng, gn[f'{net}_plug_bank'][m], dev)).cpu() for m in range(2)]
    w_lpips = 3.0
    opt = types.SimpleNamespace(img_resolution=res, batch_size=1, modalities_aug='A,B', opt_num_epochs=2, opt_lr=0.01, truncation_psi=1.0,
                                w_pix=0.0, w_lpips=w_lpips, w_latent=0.0, w_disc=0.0, crop_size_aug=crop, preprocess_aug='center_random_crop',
                                soft_aug=False, alpha=1.0, verbose_log=False, criterion_mode='gemm', final_noise_mode='const', precision='f32',
                                lpips_script='lpips', lpips_net=net, lpips_trunk_path=str(tmp_path / names[0]), lpips_lin_path=str(tmp_path / names[1]))
    before = dict(vars(opt))
    pos = tuple(int(v) for v in gn['plug_pos'])
    w0 = torch.tensor(ll['w0'])[:1]
    la = LatentAug('train', opt, str(tmp_path), [0], generator=G, banks={'fea': fea})
    assert vars(opt) == before and la.feat.num_taps == nc.NTAPS[net] and la.feat.pre_scale == bank_eng.pre_scale
    img, w_aug, losses = la.run_local(w0.to(dev), want_losses=True, crop_pos=pos)
    got = losses.cpu().numpy()[0, 3]
    lc.check(f'{net} plugin step-0 lpips loss', np.array([got]), np.array([gn[f'{net}_plug_tr64'].mean() * w_lpips]),
             np.array([gn[f'{net}_plug_tr32'].mean() * w_lpips]))
    # a second LatentAug from the same `opt`: the same bits; eager launches instead of the captured step: the same bits
    for extra in (dict(), dict(hip_graph=False)):
        again = LatentAug('train', types.SimpleNamespace(**vars(opt), **extra), str(tmp_path), [0], generator=G, banks={'fea': fea})
        img_b, w_aug_b, losses_b = again.run_local(w0.to(dev), want_losses=True, crop_pos=pos)
        assert torch.equal(img_b, img) and torch.equal(w_aug_b, w_aug) and torch.equal(losses_b, losses), extra
    # through <model_dir> instead of the two options
    opt2 = types.SimpleNamespace(**{k: v for k, v in vars(opt).items() if k not in ('lpips_trunk_path', 'lpips_lin_path')}, model_dir=str(tmp_path))
    la2 = LatentAug('train', opt2, str(tmp_path), [0], generator=G, banks={'fea': fea})
    assert la2.feat.weights_digest == la.feat.weights_digest
    # a crop too small for the net: refused at construction, with the minimum named
    small = types.SimpleNamespace(**{**vars(opt), 'crop_size_aug': nc.MIN_RES[net] - 1})
    with pytest.raises(_lib.LatentAugHipError, match=f'at least {nc.MIN_RES[net]}'):
        LatentAug('train', small, str(tmp_path), [0], generator=G, banks={'fea': fea})


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the LPIPS metrics on an alex engine

def _channel_lpips(ops, desc, img_a, img_b, dtype):
    cols = []
    for c in range(img_a.shape[1]):
        fed = [lc.affine(img[:, c:c + 1].repeat(1, 3, 1, 1), desc.pre_scale, desc.pre_shift) for img in (img_a, img_b)]
        cols.append(nc.pair_distance(nc.cast_ops(ops, dtype), fed[0], fed[1], 'engine').sum(1))
    return torch.stack(cols, dim=1)


def test_metrics_with_an_alex_engine(dev, gn):
    from latentaugment_amd import metrics
    from latentaugment_amd.synthesis import FeatureEngine, SynthesisEngine
    desc = _net(gn, 'alex')
    eng = FeatureEngine.from_net(desc, dev, in_res=pc.RES, max_batch=32)
    # diversity of a set of the toy generator's images
    G = pc.toy_generator()
    ws = torch.randn([6, 1, pc.WDIM], generator=torch.Generator().manual_seed(2)).repeat(1, G.num_ws, 1)
    with torch.no_grad():
        imgs = G.synthesis(ws, noise_mode='const').float()
    out = metrics.compute_lpips_diversity(imgs.to(dev), eng, num_pairs=7, seed=3)
    ix, iy = metrics.msssim_diversity_pairs(6, 7, 3)
    ref64 = _channel_lpips(desc.ops, desc, imgs.double()[ix], imgs.double()[iy], torch.float64).mean(1)
    yard = _channel_lpips(desc.ops, desc, imgs[ix], imgs[iy], torch.float32).mean(1)
    lc.check('alex diversity', out['lpips'], ref64, yard)
    assert out['mean'] == float(out['lpips'].mean())
    # path length from w0 to w1 on the generator's engine
    synth = SynthesisEngine.from_generator(G, dev, max_batch=16, precision='f32')
    N, S = 3, 4
    w0, w1 = pc.path_latents(N, 1)
    got = metrics.compute_path_length(synth, eng, w0.to(dev), w1.to(dev), segments=S)
    both = {}
    for dtype in (torch.float64, torch.float32):
        Gd = pc._generator_as(dtype)
        with pc._Dtype(dtype), torch.no_grad():
            p = pc._points(pc.lerp_points, w0.reshape(N, -1).numpy(), w1.reshape(N, -1).numpy(), np.zeros([N], np.float32), [k / S for k in range(S + 1)], dtype)
            img = Gd.synthesis(p.reshape((S + 1) * N, 1, pc.WDIM).repeat(1, Gd.num_ws, 1), noise_mode='const').reshape(S + 1, N, pc.IMG_CH, pc.RES, pc.RES)
            seg = torch.stack([_channel_lpips(desc.ops, desc, img[k], img[k + 1], dtype).mean(1) for k in range(S)], dim=1).double()
            chord = _channel_lpips(desc.ops, desc, img[0], img[S], dtype).mean(1).double().sqrt()
        both[dtype] = {'segment_lpips': seg.numpy(), 'chord': chord.numpy(), 'length': seg.sqrt().sum(1).numpy()}
    for k in ('segment_lpips', 'chord', 'length'):
        lc.check(f'alex path {k}', got[k], both[torch.float64][k], both[torch.float32][k])
    again = metrics.compute_path_length(synth, eng, w0.to(dev), w1.to(dev), segments=S)
    assert all(torch.equal(got[k], again[k]) for k in got)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. misuse

def test_misuse_leaves_the_device_usable(dev, gn):
    from latentaugment_amd import _lib
    t = lambda *s: torch.zeros(list(s))      # noqa: E731
    tap8 = ('tap', torch.ones([8]))
    bad = {
        'k > 11': [('conv', t(8, 3, 13, 13), t(8), 4, 2), tap8],
        'stride 3': [('conv', t(8, 3, 5, 5), t(8), 3, 2), tap8],
        'pad 6': [('conv', t(8, 3, 11, 11), t(8), 1, 6), tap8],
        'cout % 4': [('conv', t(6, 3, 3, 3), t(6), 1, 1), ('tap', torch.ones([6]))],
        'resolution too small': [('conv', t(8, 3, 11, 11), t(8), 4, 2), ('maxpool3', False), ('maxpool3', False), ('maxpool3', False), tap8],
        'fire squeeze % 4': [('conv', t(16, 3, 3, 3), t(16), 1, 1), ('fire', t(6, 16, 1, 1), t(6), t(8, 6, 1, 1), t(8), t(8, 6, 3, 3), t(8)),
                             ('tap', torch.ones([16]))],
    }
    for name, ops in bad.items():
        with pytest.raises(_lib.LatentAugHipError, match='op '):
            _engine_of(ops, dev, 35, 2)
    with pytest.raises(AssertionError):      # a fire whose expand weights do not fit its squeeze: refused before the library sees it
        _engine_of([('conv', t(16, 3, 3, 3), t(16), 1, 1), ('fire', t(4, 16, 1, 1), t(4), t(8, 8, 1, 1), t(8), t(8, 4, 3, 3), t(8)),
                    ('tap', torch.ones([16]))], dev, 35, 2)
    eng = _engine(gn, dev, 'alex', 35)
    with pytest.raises(ValueError):
        eng.pair_distance(torch.zeros([1, 3, 34, 34], device=dev), torch.zeros([1, 3, 34, 34], device=dev))
    with pytest.raises(_lib.LatentAugHipError):
        eng.pair_distance(torch.zeros([1, 3, 35, 35]), torch.zeros([1, 3, 35, 35]))
    torch.cuda.synchronize()
    d = eng.pair_distance(_fed(eng, gn['alex35_x'], dev), _fed(eng, gn['alex35_y'], dev)).cpu()
    lc.check('after misuse', d, gn['alex35_layers64'], gn['alex35_layers32'])


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. guard bands

@pytest.mark.parametrize('pattern', ['ones', 'bytes'])
@pytest.mark.parametrize('net', NETS)
def test_guard_bands(dev, gn, monkeypatch, net, pattern):
    """One forward, backward and pair_distance of each net on guarded workspaces that start as NaN / seeded bytes: the bands are intact
    and the results are those of an ordinary engine, bit for bit (nothing is read before it is written)."""
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import FeatureEngine
    R = nc.SIZES[net][0]
    plain = _engine(gn, dev, net, R)
    key = f'{net}{R}'
    x, y = _fed(plain, gn[f'{key}_x'], dev), _fed(plain, gn[f'{key}_y'], dev)
    gf = torch.randn([3, plain.num_features], generator=torch.Generator().manual_seed(2)).to(dev)
    want = (plain.forward(x), plain.backward(gf), plain.pair_distance(x, y))
    guard = Guarded(pattern)
    monkeypatch.setattr(_lib, 'workspace', guard.alloc)
    eng = FeatureEngine.from_net(_net(gn, net), dev, in_res=R, max_batch=8)
    got = (eng.forward(x), eng.backward(gf), eng.pair_distance(x, y))
    guard.check()
    assert len(guard.records) >= 2 and all(torch.equal(a, b) for a, b in zip(got, want))
