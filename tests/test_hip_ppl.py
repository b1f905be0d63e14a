"""Perceptual path length on the GPU: la_path_points_f32 against its float64 restatement, metrics.compute_ppl and compute_path_length
against the float64 composition of the CPU generator and mapping under oracle/ with tests/lpips_cases.pair_distance.

Bounds.  Lerp points: the float64 restatement rounded to float32, bit for bit.  Slerp points: within one float32 step of the float64
restatement (device and host acos / sin / cos may differ in the last double bit; a correctly rounded result is within half a step).
compute_ppl / compute_path_length: the project's rule (test_hip_conv2d_op.check, nothing tuned): error against float64 <= 4 x the error of
the same composition in float32 on the CPU + 2e-6 x the largest float64 magnitude.  The float32 composition holds the path points as
the kernel's contract gives them (float64 arithmetic, rounded once), so its error is that of the float32 nets on float32 latents.
Both engines run in 'f32' precision; no sample is left out."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import ppl_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

N_PPL = 8


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


def _points(dev, a, b, t, dt, reps, mode):
    """The C entry itself: numpy float32 in, numpy float32 [T, N, reps, D] out."""
    from latentaugment_amd import _lib
    lib = _lib.load()
    ad, bd, td = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in (a, b, t))
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    N, D = a.shape
    out = torch.full([dt.size, N, reps, D], float('nan'), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.la_path_points_f32(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(td), dt.ctypes.data, int(dt.size), N, D, reps, mode,
                                          _lib.ptr(out), _lib.stream_ptr()), 'path_points')
    return out.cpu().numpy()


def _dt(T, rs):
    """T steps: 0 and 1e-4 first (the PPL pair), then values that carry t + dt below 0 and above 1."""
    return np.concatenate([[0.0, 1e-4], rs.uniform(-1.5, 1.5, 15)])[:T]


def _sweep():
    return [(N, reps, T) for N in pc.KERNEL_N for reps in pc.KERNEL_REPS for T in pc.KERNEL_T]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the points kernel

@pytest.mark.parametrize('D', pc.KERNEL_D)
def test_lerp_points_bit_for_bit(dev, D):
    for N, reps, T in _sweep():
        rs = np.random.RandomState(1000 * D + 100 * N + 10 * reps + T)
        a, b = rs.randn(N, D).astype(np.float32), (3.0 * rs.randn(N, D)).astype(np.float32)
        t, dt = rs.rand(N).astype(np.float32), _dt(T, rs)
        got = _points(dev, a, b, t, dt, reps, 0)
        want = pc.lerp_points(a, b, t, dt, reps).astype(np.float32)
        assert got.shape == want.shape == (T, N, reps, D)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, N, reps, T)
        # integer-valued rows with dyadic parameters inside and outside [0, 1]: every product and sum is exact
        a, b = rs.randint(-8, 9, [N, D]).astype(np.float32), rs.randint(-8, 9, [N, D]).astype(np.float32)
        t, dt = rs.choice([0.0, 0.25, 0.5, 1.0], N).astype(np.float32), (np.arange(T) * 0.125 - 0.5)
        got = _points(dev, a, b, t, dt, reps, 0)
        s = t.astype(np.float64)[None, :] + dt[:, None]
        exact = a[None].astype(np.float64) + (b.astype(np.float64) - a)[None] * s[:, :, None]
        assert np.array_equal(got.astype(np.float64), np.repeat(exact[:, :, None], reps, axis=2)), (D, N, reps, T)


@pytest.mark.parametrize('D', pc.KERNEL_D)
def test_slerp_points_within_one_ulp(dev, D):
    for N, reps, T in _sweep():
        rs = np.random.RandomState(2000 * D + 100 * N + 10 * reps + T)
        a, b = rs.randn(N, D).astype(np.float32), rs.randn(N, D).astype(np.float32)
        if D == 1:
            b = np.where(rs.rand(N, 1) < 0.5, a, -a).astype(np.float32) * 2          # one dimension: only +- directions exist
        t, dt = rs.rand(N).astype(np.float32), _dt(T, rs)
        got = _points(dev, a, b, t, dt, reps, 1)
        want = pc.slerp_points(a, b, t, dt, reps)
        assert got.shape == want.shape and np.isfinite(got).all()
        assert pc.one_ulp(got, want), (D, N, reps, T, float(np.abs(got - want).max()))
        assert np.array_equal(got[:, :, :1].repeat(reps, axis=2), got)


@pytest.mark.parametrize('D', pc.KERNEL_D)
def test_slerp_degenerate_and_unequal_norms(dev, D):
    t, dt = np.array([0.0, 0.6], np.float32), [0.0, 0.5, 1.3, -0.4]
    # identical / opposite directions whose sums are exact: |b' - d a'| is exactly 0 and every point the normalised a, bit for bit
    for sign in (1.0, -1.0):
        a, b = pc.exact_rows(D, sign)
        got = _points(dev, a, b, t, dt, 2, 1)
        want = pc.slerp_points(a, b, t, dt, 2)
        unit = a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)
        assert np.array_equal(want, np.broadcast_to(unit[None, :, None], want.shape))
        assert np.array_equal(got, want.astype(np.float32)), (D, sign)
    # a == b, ordinary rows: d rounds next to 1 and b' - d a' is rounding noise; the points stay the normalised a (not NaN)
    rs = np.random.RandomState(D)
    a = rs.randn(2, D).astype(np.float32)
    got = _points(dev, a, a.copy(), t, dt, 1, 1)
    unit = a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)
    assert np.isfinite(got).all() and pc.one_ulp(got, np.broadcast_to(unit[None, :, None], got.shape)), D
    # rows of very different norm: only the directions count
    if D > 1:
        b = rs.randn(2, D).astype(np.float32)
        big, small = (a * np.float32(2.0 ** 40)), (b * np.float32(2.0 ** -30))
        got = _points(dev, big, small, t, dt, 1, 1)
        assert pc.one_ulp(got, pc.slerp_points(big, small, t, dt, 1)), D
        assert pc.one_ulp(got, pc.slerp_points(a, b, t, dt, 1)), D          # (scaling by powers of two changes nothing)


def test_points_two_runs_same_bits(dev):
    rs = np.random.RandomState(9)
    a, b, t = rs.randn(5, 520).astype(np.float32), rs.randn(5, 520).astype(np.float32), rs.rand(5).astype(np.float32)
    dt = _dt(17, rs)
    for mode in (0, 1):
        first = _points(dev, a, b, t, dt, 14, mode)
        assert np.array_equal(first.view(np.uint32), _points(dev, a, b, t, dt, 14, mode).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. engines of the toy nets

class _Toy:
    def __init__(self, dev):
        from latentaugment_amd.synthesis import FeatureEngine, MappingEngine, ScriptedFeatureNet, SynthesisEngine
        G = pc.toy_generator()
        self.dev = dev
        self.mapping = MappingEngine(G, dev)
        self.synth = SynthesisEngine.from_generator(G, dev, max_batch=2 * N_PPL, precision='f32')
        desc = ScriptedFeatureNet(pc.toy_ops(), pc.PRE_SCALE, pc.PRE_SHIFT, False, None)
        self.nets = {r: FeatureEngine.from_net(desc, dev, in_res=r, max_batch=2 * N_PPL * pc.IMG_CH, precision='f32') for r in (32, 16)}


@pytest.fixture(scope='module')
def toy(dev):
    return _Toy(dev)


def _check(name, got, ref64, yard):
    lc.check(name, got.numpy() if torch.is_tensor(got) else got, ref64, yard)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. compute_ppl

PPL_CASES = [(1e-2, 'w', 'full', 1.0, 32), (1e-2, 'w', 'end', 1.0, 32), (1e-2, 'z', 'full', 1.0, 32), (1e-2, 'z', 'end', 1.0, 32),
             (1e-2, 'w', 'full', 0.7, 16), (1e-2, 'z', 'full', 0.7, 16), (1e-4, 'w', 'full', 1.0, 32), (1e-4, 'z', 'full', 1.0, 16)]


@pytest.mark.parametrize('eps,space,sampling,psi,in_res', PPL_CASES)
def test_compute_ppl(toy, eps, space, sampling, psi, in_res):
    from latentaugment_amd import metrics
    kw = dict(epsilon=eps, space=space, sampling=sampling, truncation_psi=psi, seed=4)
    out = metrics.compute_ppl(toy.mapping, toy.synth, toy.nets[in_res], N_PPL, **kw)
    ref64 = pc.ppl_oracle(N_PPL, eps, space, sampling, psi, 4, in_res, torch.float64)
    yard = pc.ppl_oracle(N_PPL, eps, space, sampling, psi, 4, in_res, torch.float32)
    assert set(out) == {'dist', 'dist_per_channel', 'ppl', 'ppl_per_channel'}
    assert all(v.dtype == torch.float64 and v.device.type == 'cpu' for v in out.values())
    assert out['dist_per_channel'].shape == (N_PPL, pc.IMG_CH) and out['dist'].shape == (N_PPL,) and out['ppl_per_channel'].shape == (pc.IMG_CH,)
    name = f'ppl eps={eps} {space} {sampling} psi={psi} r={in_res}'
    _check(name, out['dist_per_channel'], ref64, yard)
    assert float(ref64.min()) > 0 and float(out['dist_per_channel'].min()) > 0
    assert torch.equal(out['dist'], out['dist_per_channel'].mean(dim=1))
    assert float(out['ppl']) == metrics.ppl_from_distances(out['dist']) == pc.ppl_filter(out['dist'].numpy())
    for c in range(pc.IMG_CH):
        assert float(out['ppl_per_channel'][c]) == pc.ppl_filter(out['dist_per_channel'][:, c].numpy())
    again = metrics.compute_ppl(toy.mapping, toy.synth, toy.nets[in_res], N_PPL, **kw)
    for k in out:
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize('space', ['w', 'z'])
def test_compute_ppl_chunked(toy, space):
    """batch=2: four chunks of two samples.  The draws are those of the unchunked run; the engines' slice counts depend on the batch, so
    the distances agree within the bound, not bit for bit."""
    from latentaugment_amd import metrics
    ref64 = pc.ppl_oracle(N_PPL, 1e-2, space, 'full', 1.0, 4, 32, torch.float64)
    yard = pc.ppl_oracle(N_PPL, 1e-2, space, 'full', 1.0, 4, 32, torch.float32)
    whole = metrics.compute_ppl(toy.mapping, toy.synth, toy.nets[32], N_PPL, epsilon=1e-2, space=space, seed=4)
    for batch in (2, 3):          # 3: a ragged last chunk
        part = metrics.compute_ppl(toy.mapping, toy.synth, toy.nets[32], N_PPL, epsilon=1e-2, space=space, seed=4, batch=batch)
        _check(f'ppl {space} batch={batch}', part['dist_per_channel'], ref64, yard)
        err = float((part['dist_per_channel'] - whole['dist_per_channel']).abs().max())
        print(f'chunked against whole: {err:.3e}')
        assert err <= lc.bound(ref64, yard)
    other = metrics.compute_ppl(toy.mapping, toy.synth, toy.nets[32], N_PPL, epsilon=1e-2, space=space, seed=5)
    assert not torch.equal(other['dist'], whole['dist'])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. compute_path_length

N_PATH = 3


@pytest.mark.parametrize('L', [1, 8])
@pytest.mark.parametrize('segments', [1, 4])
@pytest.mark.parametrize('in_res', [32, 16])
def test_compute_path_length(toy, L, segments, in_res):
    from latentaugment_amd import metrics
    assert toy.synth.num_ws == 8
    w0, w1 = pc.path_latents(N_PATH, L)
    out = metrics.compute_path_length(toy.synth, toy.nets[in_res], w0.to(toy.dev), w1.to(toy.dev), segments=segments)
    ref64 = pc.path_oracle(N_PATH, L, segments, in_res, torch.float64)
    yard = pc.path_oracle(N_PATH, L, segments, in_res, torch.float32)
    assert set(out) == set(ref64) and out['segment_lpips'].shape == (N_PATH, segments)
    for k in ('length', 'chord', 'ratio', 'segment_lpips'):
        assert out[k].dtype == torch.float64 and out[k].device.type == 'cpu'
        _check(f'path L={L} S={segments} r={in_res} {k}', out[k], ref64[k], yard[k])
    if segments == 1:
        assert torch.equal(out['length'], out['chord']) and torch.equal(out['ratio'], torch.ones_like(out['ratio']))
    else:
        assert bool((out['ratio'] >= 1 - 1e-6).all())          # sqrt(LPIPS) of the toy net behaves like a metric here: the path is no shorter
    again = metrics.compute_path_length(toy.synth, toy.nets[in_res], w0.to(toy.dev), w1.to(toy.dev), segments=segments)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    if L == 1:          # [N, w_dim] is [N, 1, w_dim]
        flat = metrics.compute_path_length(toy.synth, toy.nets[in_res], w0[:, 0].to(toy.dev), w1[:, 0].to(toy.dev), segments=segments)
        for k in out:
            assert torch.equal(out[k], flat[k]), k


@pytest.mark.parametrize('L', [1, 8])
def test_path_that_does_not_move(toy, L):
    """w0 == w1: every point of the lerp is w0 exactly, every image the same bits, every distance exactly 0; ratio is defined as 1."""
    from latentaugment_amd import metrics
    w0, _ = pc.path_latents(N_PATH, L)
    out = metrics.compute_path_length(toy.synth, toy.nets[32], w0.to(toy.dev), w0.clone().to(toy.dev), segments=4)
    assert float(out['length'].abs().max()) == 0.0 and float(out['chord'].abs().max()) == 0.0
    assert float(out['segment_lpips'].abs().max()) == 0.0
    assert torch.equal(out['ratio'], torch.ones([N_PATH], dtype=torch.float64))


def test_path_length_in_rounds(toy):
    """A generator of max_batch 2 and a net of max_batch 4 take the 5 points of a path and its pairs in several calls."""
    from latentaugment_amd import metrics
    from latentaugment_amd.synthesis import FeatureEngine, ScriptedFeatureNet, SynthesisEngine
    synth = SynthesisEngine.from_generator(pc.toy_generator(), toy.dev, max_batch=2, precision='f32')
    net = FeatureEngine.from_net(ScriptedFeatureNet(pc.toy_ops(), pc.PRE_SCALE, pc.PRE_SHIFT, False, None), toy.dev, in_res=32, max_batch=4)
    w0, w1 = pc.path_latents(N_PATH, 1)
    out = metrics.compute_path_length(synth, net, w0.to(toy.dev), w1.to(toy.dev), segments=4)
    ref64, yard = pc.path_oracle(N_PATH, 1, 4, 32, torch.float64), pc.path_oracle(N_PATH, 1, 4, 32, torch.float32)
    for k in ('length', 'chord', 'segment_lpips'):
        _check(f'small engines {k}', out[k], ref64[k], yard[k])
    ppl = metrics.compute_ppl(toy.mapping, synth, net, N_PPL, epsilon=1e-2, seed=4)
    _check('small engines ppl', ppl['dist_per_channel'], pc.ppl_oracle(N_PPL, 1e-2, 'w', 'full', 1.0, 4, 32, torch.float64),
           pc.ppl_oracle(N_PPL, 1e-2, 'w', 'full', 1.0, 4, 32, torch.float32))


def test_path_length_for_aug_dataset(toy, tmp_path):
    """A run directory in the drivers' layout: numpy latents, squeezed as the drivers dump them ([n, w_dim]; [w_dim] for a batch of one)."""
    from latentaugment_amd import metrics
    w0, w1 = pc.path_latents(N_PATH, 1)
    run = tmp_path / 'run'
    os.makedirs(run / 'latent')
    os.makedirs(run / 'latent_aug')
    for i, (lo, hi) in enumerate(((0, 2), (2, 3))):
        with open(run / 'latent' / f'w_{i}', 'wb') as f:
            pickle.dump(w0[lo:hi].numpy().squeeze(), f)
        with open(run / 'latent_aug' / f'w_aug_{i}', 'wb') as f:
            pickle.dump(w1[lo:hi].numpy().squeeze(), f)
    out = metrics.compute_path_length_for_aug_dataset(str(run), toy.synth, toy.nets[32], segments=4)
    ref64, yard = pc.path_oracle(N_PATH, 1, 4, 32, torch.float64), pc.path_oracle(N_PATH, 1, 4, 32, torch.float32)
    assert out['num_items'] == N_PATH
    for k in ('length', 'chord', 'ratio', 'segment_lpips'):
        _check(f'aug dataset {k}', out[k], ref64[k], yard[k])
        if k != 'segment_lpips':
            assert out[k + '_mean'] == float(out[k].mean())
    with pytest.raises(FileNotFoundError):
        metrics.compute_path_length_for_aug_dataset(str(tmp_path / 'absent'), toy.synth, toy.nets[32])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. misuse

def test_misuse_leaves_the_device_usable(toy):
    from latentaugment_amd import _lib, metrics
    from latentaugment_amd.synthesis import FeatureEngine, ScriptedFeatureNet, SynthesisEngine
    dev, net = toy.dev, toy.nets[32]
    w0, w1 = pc.path_latents(N_PATH, 1)
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        metrics.compute_path_length(toy.synth, net, w0, w1.to(dev))
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        metrics.compute_path_length(toy.synth, net, w0.to(dev), w1)
    with pytest.raises(ValueError):
        metrics.compute_path_length(toy.synth, net, w0.to(dev), w1[:2].to(dev))
    with pytest.raises(ValueError):
        metrics.compute_path_length(toy.synth, net, w0[:, :, :16].contiguous().to(dev), w1[:, :, :16].contiguous().to(dev))
    for bad in (0, 64, 2.5):
        with pytest.raises(ValueError, match='segments'):
            metrics.compute_path_length(toy.synth, net, w0.to(dev), w1.to(dev), segments=bad)
    g = torch.Generator().manual_seed(1)
    det = FeatureEngine([('fc', torch.randn([5, 3 * 32 * 32], generator=g) * 0.01, torch.zeros([5]), False)], dev, in_res=32, max_batch=4)
    with pytest.raises(_lib.LatentAugHipError, match='detector'):
        metrics.compute_ppl(toy.mapping, toy.synth, det, 4)
    with pytest.raises(_lib.LatentAugHipError, match='detector'):
        metrics.compute_path_length(toy.synth, det, w0.to(dev), w1.to(dev))
    one = SynthesisEngine.from_generator(pc.toy_generator(), dev, max_batch=1, precision='f32')
    with pytest.raises(_lib.LatentAugHipError, match='max_batch = 1'):
        metrics.compute_ppl(toy.mapping, one, net, 4)
    with pytest.raises(_lib.LatentAugHipError, match='max_batch = 1'):
        metrics.compute_path_length(one, net, w0.to(dev), w1.to(dev))
    net24 = FeatureEngine.from_net(ScriptedFeatureNet(pc.toy_ops()[:2], pc.PRE_SCALE, pc.PRE_SHIFT, False, None), dev, in_res=24, max_batch=8)
    with pytest.raises(ValueError, match='24'):
        metrics.compute_ppl(toy.mapping, toy.synth, net24, 4)
    one_ch = FeatureEngine([('tap', torch.ones([1]))], dev, in_res=32, max_batch=8, in_ch=1)
    with pytest.raises(ValueError, match='three'):
        metrics.compute_ppl(toy.mapping, toy.synth, one_ch, 4)
    for kw in (dict(space='x'), dict(sampling='middle'), dict(epsilon=0.0), dict(batch=0)):
        with pytest.raises(ValueError):
            metrics.compute_ppl(toy.mapping, toy.synth, net, 4, **kw)
    with pytest.raises(ValueError):
        metrics.compute_ppl(toy.mapping, toy.synth, net, 0)
    # the C entry on device pointers: refused with LA_ERR_ARG before any launch
    lib = _lib.load()
    buf = torch.zeros([64], dtype=torch.float32, device=dev)
    dt = np.zeros([64], np.float64)
    p = _lib.ptr(buf)
    assert lib.la_path_points_f32(p, p, p, dt.ctypes.data, 65, 1, 4, 1, 0, p, _lib.stream_ptr()) == -1
    assert lib.la_path_points_f32(p, p, p, dt.ctypes.data, 2, 1, 4, 1, 7, p, _lib.stream_ptr()) == -1
    assert lib.la_path_points_f32(p, None, p, dt.ctypes.data, 2, 1, 4, 1, 0, p, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    out = metrics.compute_ppl(toy.mapping, toy.synth, net, N_PPL, epsilon=1e-2, seed=4)
    _check('after misuse', out['dist_per_channel'], pc.ppl_oracle(N_PPL, 1e-2, 'w', 'full', 1.0, 4, 32, torch.float64),
           pc.ppl_oracle(N_PPL, 1e-2, 'w', 'full', 1.0, 4, 32, torch.float32))
