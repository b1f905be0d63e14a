"""GeometricAugment on the GPU (csrc/la_geom.hip through latentaugment_amd/geometric.py and the plugin) against the float64 restatement
of tests/geometric_cases.py, which tests/test_geometric_cpu.py pins to torch's CPU grid_sample / conv2d.

Exact cases (integer-valued pixels or noise, weights and taps dyadic: every sum is exact in float32) are compared bit for bit.
Float cases: the kernel's error against the float64 restatement may be at most MARGIN x the error of the same restatement run in float32
on the CPU for that case, + 1 float32 ulp of the largest magnitude.  MARGIN started at 4 (the convention of test_hip_grid_sample.py);
every float case prints `kernel error / float32-restatement error`, and MARGIN is twice the largest ratio of the first GPU run:

    affine (theta <= 30 degrees, shifts <= 1.5 size; 4 shapes x 3 modes)   0.33 - 1.24   (largest: 33x70 zeros, 2.37e-5 against 1.91e-5;
                                                                                         16x16 zeros, one sample wholly outside: 0 / 0)
    63-tap Gaussian field (16x16, 33x70, 96x80; alpha 1 and 40)            0.91 - 1.07
    elastic warp (alpha 1 and 40, reflection and zeros; 4 shapes)          1.00 - 1.08
    displacement with NaN / infinite entries (3 modes)                     1.00
    plugin end to end, 4x2x64x64                                           0.73 (all stages), 1.00 (p_thres 0.5)

so MARGIN = 2 x 1.24 = 2.48 (DESIGN 'GeometricAugment').
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometric_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 2.48


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def geo():
    from latentaugment_amd import geometric
    return geometric


def _gpu(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def _exact(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    assert np.array_equal(got.astype(np.float64), exp), (what, float(np.abs(got - exp).max()))


def _within_budget(got, exp64, exp32, what):
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - exp64).max())
    ref_err = float(np.abs(exp32.astype(np.float64) - exp64).max())
    print(f'{what}: kernel error {err:.3e}, float32-restatement error {ref_err:.3e}, ratio {err / ref_err if ref_err else float("nan"):.2f}')
    assert got.shape == exp64.shape and err <= MARGIN * ref_err + gc.ulp32(np.abs(exp64).max()), (what, err, ref_err)


def _batch(shape_index):
    """(B, C, flags): the shapes walk through the batch table, so every B and C meets a small and a large image."""
    return gc.BATCHES[shape_index % len(gc.BATCHES)]


# ------------------------------------------------------------------------------------------------------------ exact warps
@pytest.mark.parametrize('si', range(len(gc.SHAPES)), ids=[f'{h}x{w}' for h, w in gc.SHAPES])
def test_flip_alone_is_exact(dev, geo, si):
    H, W = gc.SHAPES[si]
    for B, C, flags in (_batch(si), _batch(si + 1)):
        x = gc.int_image(np.random.default_rng(si), B, C, H, W)
        f = torch.tensor(flags, dtype=torch.bool)
        params = {'flip': f, 'affine': torch.zeros(B, dtype=torch.bool), 'angle': torch.zeros(B, dtype=torch.float64),
                  'tx': torch.zeros(B, dtype=torch.float64), 'ty': torch.zeros(B, dtype=torch.float64)}
        minv = geo.affine_inverse(params, H, W)
        y = geo.warp_affine(_gpu(x, dev), minv.to(dev), f.to(dev))
        exp = np.where(np.array(flags, bool)[:, None, None, None], x[..., ::-1], x)
        _exact(y, exp, ('flip', H, W, B, C))
        _exact(y, gc.warp_affine(x, minv.numpy(), flags, 'reflection'), ('flip restated', H, W, B, C))


@pytest.mark.parametrize('mode', gc.MODES)
@pytest.mark.parametrize('si', range(len(gc.SHAPES)), ids=[f'{h}x{w}' for h, w in gc.SHAPES])
def test_integer_and_half_pixel_translations_are_exact(dev, geo, si, mode):
    """The picture leaves the image on each side by 1, by `size` and by 2 size + 3 pixels (integer shifts: weights 0 and 1), and by the
    same amounts plus a half (weights 0.5); samples with apply == 0 keep their input bit for bit next to applied ones."""
    H, W = gc.SHAPES[si]
    B, C, flags = _batch(si + 1)
    x = gc.int_image(np.random.default_rng(10 + si), B, C, H, W)
    xg, fg = _gpu(x, dev), torch.tensor(flags, dtype=torch.uint8, device=dev)
    for half in (0.0, 0.5):
        for sign in (1, -1):
            for tx, ty in ((1, 0), (0, 1), (W, 0), (0, H), (2 * W + 3, 0), (0, 2 * H + 3), (1, H), (2 * W + 3, 2 * H + 3)):
                minv = gc.translation(sign * (tx + half if tx else 0), sign * (ty + half if ty else 0), B)
                y = geo.warp_affine(xg, _gpu(minv, dev), fg, padding_mode=mode)
                exp = gc.warp_affine(x, minv, flags, mode)
                _exact(y, exp, (mode, H, W, sign, tx, ty, half))
                for b, on in enumerate(flags):
                    if not on:
                        assert torch.equal(y[b], xg[b])
    if mode == 'zeros':      # far enough out, nothing is left; border and reflection always show the picture
        y = geo.warp_affine(xg, _gpu(gc.translation(2 * W + 3, 0, B), dev), fg, padding_mode=mode)
        assert not y[[b for b, on in enumerate(flags) if on]].any()


@pytest.mark.parametrize('size,bi', [(5, 0), (16, 1), (64, 2)])
def test_quarter_turn_of_a_square_is_exact(dev, geo, size, bi):
    B, C, flags = gc.BATCHES[bi]
    x = gc.int_image(np.random.default_rng(20 + size), B, C, size, size)
    minv = np.tile(np.array([0, 1, 0, -1, 0, size - 1], np.float32), (B, 1))
    for mode in gc.MODES:
        y = geo.warp_affine(_gpu(x, dev), _gpu(minv, dev), torch.tensor(flags, device=dev), padding_mode=mode)
        exp = gc.warp_affine(x, minv, flags, mode)
        _exact(y, exp, ('turn', size, mode))
        on = np.array(flags, bool)
        assert np.array_equal(exp[on], np.rot90(x[on], k=-1, axes=(2, 3)))      # out[y][x] = in[size - 1 - x][y]


def test_refused_positions_and_other_dtypes(dev, geo):
    """NaN / infinite / huge entries of Minv and of the displacement give 0 and address nothing; float64 and float16 images are computed
    in float32 and cast back."""
    x = gc.int_image(np.random.default_rng(30), 4, 2, 5, 7)
    minv = gc.translation(1, 0, 4)
    minv[0, 2], minv[1, 5], minv[2, 0] = np.nan, np.inf, 1e30
    for mode in gc.MODES:
        y = geo.warp_affine(_gpu(x, dev), _gpu(minv, dev), torch.ones(4, device=dev), padding_mode=mode)
        _exact(y, gc.warp_affine(x, minv, [1] * 4, mode), ('refused', mode))
        assert not y[:2].any()
        d = np.zeros((4, 2, 5, 7))
        d[0, 0, 2, 3], d[1, 1, 0, 0], d[2, 0, 4, 6] = np.nan, np.inf, -np.inf
        y = geo.warp_elastic(_gpu(x, dev), _gpu(d, dev), torch.ones(4, device=dev), padding_mode=mode)
        _within_budget(y, gc.warp_elastic(x, d, [1] * 4, mode), gc.warp_elastic(x, d, [1] * 4, mode, np.float32), f'refused displacement {mode}')
        assert y[0, :, 2, 3].abs().max() == 0
    for dt in (torch.float64, torch.float16):
        y = geo.warp_affine(_gpu(x, dev, dt), _gpu(gc.translation(0.5, 0, 4), dev), torch.ones(4, device=dev))
        assert y.dtype == dt and np.array_equal(y.cpu().double().numpy(), gc.warp_affine(x, gc.translation(0.5, 0, 4), [1] * 4, 'reflection'))


# ------------------------------------------------------------------------------------------------------------ exact blur
@pytest.mark.parametrize('shape', gc.BLUR_SHAPES, ids=[f'{h}x{w}' for h, w in gc.BLUR_SHAPES])
def test_blur_with_dyadic_taps_is_exact(dev, geo, shape):
    """Every tap 2^-6 on integer noise: sums of at most 63 x 63 x 8 units of 2^-12, exact in float32.  16 x 16 is smaller than the
    half-width of 31; 33 x 70 and 96 x 80 span several tiles with ragged edges.  alpha (2, -0.5) tells the planes apart."""
    H, W = shape
    rng = np.random.default_rng(H)
    for ntaps, B in zip(gc.BLUR_NTAPS, (1, 3, 5)):
        noise = rng.integers(-8, 9, size=(B, 2, H, W)).astype(np.float64)
        taps = [2.0 ** -6] * ntaps
        for alpha in ((1.0, 1.0), (2.0, -0.5)):
            d = geo.elastic_field(_gpu(noise, dev), taps, alpha)
            _exact(d, gc.blur(noise, taps, alpha), ('blur', H, W, ntaps, alpha))
        assert torch.equal(d, geo.elastic_field(_gpu(noise, dev), taps, alpha))      # run to run


# ------------------------------------------------------------------------------------------------------------ float cases
@pytest.mark.parametrize('mode', gc.MODES)
@pytest.mark.parametrize('si', range(len(gc.SHAPES)), ids=[f'{h}x{w}' for h, w in gc.SHAPES])
def test_random_affine_within_budget(dev, geo, si, mode):
    """theta up to 30 degrees, shifts up to 1.5 size, with and without the flip."""
    H, W = gc.SHAPES[si]
    B, C, flags = _batch(si + 2)
    rng = np.random.default_rng(40 + si)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32).astype(np.float64)
    p = geo.draw_params(torch.Generator().manual_seed(si), B, H, W, 1.0, rotate_limit=30, shift_limit=1.5)
    p['flip'] = torch.arange(B) % 2 == 0
    minv = geo.affine_inverse(p, H, W)
    y = geo.warp_affine(_gpu(x, dev), minv.to(dev), torch.tensor(flags, device=dev), padding_mode=mode)
    _within_budget(y, gc.warp_affine(x, minv.numpy(), flags, mode), gc.warp_affine(x, minv.numpy(), flags, mode, np.float32),
                   f'affine {H}x{W} B{B} C{C} {mode}')


@pytest.mark.parametrize('shape', gc.BLUR_SHAPES, ids=[f'{h}x{w}' for h, w in gc.BLUR_SHAPES])
def test_gaussian_field_within_budget(dev, geo, shape):
    H, W = shape
    noise = np.random.default_rng(50 + H).uniform(-1, 1, (3, 2, H, W)).astype(np.float32).astype(np.float64)
    taps = np.array(geo.gaussian_taps(63, 32.0).tolist(), np.float32).astype(np.float64)      # the float32 taps the kernel is given
    for alpha in ((1.0, 1.0), (40.0, 40.0)):
        d = geo.elastic_field(_gpu(noise, dev), taps.tolist(), alpha)
        _within_budget(d, gc.blur(noise, taps, alpha), gc.blur(noise, taps, alpha, np.float32), f'field {H}x{W} alpha {alpha[0]}')


@pytest.mark.parametrize('alpha', [1.0, 40.0])
@pytest.mark.parametrize('si', range(len(gc.SHAPES)), ids=[f'{h}x{w}' for h, w in gc.SHAPES])
def test_elastic_warp_within_budget(dev, geo, si, alpha):
    """The displacement is the float64 blur rounded to float32, given to kernel and restatement alike.  At alpha 40 the clamp to [-1, 1]
    bites on a visible share of the pixels."""
    H, W = gc.SHAPES[si]
    B, C, flags = _batch(si)
    rng = np.random.default_rng(60 + si)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32).astype(np.float64)
    noise = rng.uniform(-1, 1, (B, 2, H, W))
    disp = gc.blur(noise, geo.gaussian_taps(63, 32.0).numpy(), (alpha, alpha)).astype(np.float32).astype(np.float64)
    px, _ = gc.elastic_positions(disp)
    clamped = float(((px == -0.5) | (px == W - 0.5)).mean())
    assert alpha == 1.0 or clamped > 0.02, clamped
    for mode in ('reflection', 'zeros'):
        y = geo.warp_elastic(_gpu(x, dev), _gpu(disp, dev), torch.tensor(flags, device=dev), padding_mode=mode)
        _within_budget(y, gc.warp_elastic(x, disp, flags, mode), gc.warp_elastic(x, disp, flags, mode, np.float32),
                       f'elastic {H}x{W} B{B} C{C} alpha {alpha} {mode} (clamped {clamped:.2f})')
        for b, on in enumerate(flags):
            if not on:
                assert np.array_equal(y[b].cpu().numpy().astype(np.float64), x[b])


# ------------------------------------------------------------------------------------------------------------ noise
def test_noise_uniform(dev, geo):
    from oracle import noise_ref
    n = geo.noise_uniform(16, 65536, seed=1234567890123, stream_id=3, device=dev)
    v = n.cpu().numpy().astype(np.float64)
    assert n.dtype == torch.float32 and v.shape == (16, 65536) and v.min() > -1 and v.max() < 1
    assert abs(v.mean()) < 5 / (np.sqrt(3) * 1024) and abs(v.var() - 1 / 3) < 0.005, (v.mean(), v.var())
    # rows split at different row0 agree with the whole, bit for bit; a ragged row length (not a multiple of 4) as well
    for elems in (65536, 1001):
        whole = geo.noise_uniform(16, elems, 77, 1, device=dev)
        for cut in (5, 11):
            parts = torch.cat([geo.noise_uniform(cut, elems, 77, 1, row0=0, device=dev), geo.noise_uniform(16 - cut, elems, 77, 1, row0=cut, device=dev)])
            assert torch.equal(parts, whole), (elems, cut)
    base = geo.noise_uniform(4, 1001, 77, 1, device=dev)
    assert not torch.equal(base, geo.noise_uniform(4, 1001, 77, 2, device=dev)) and not torch.equal(base, geo.noise_uniform(4, 1001, 78, 1, device=dev))
    assert not torch.equal(base, geo.noise_uniform(4, 1001, 77 + (1 << 32), 1, device=dev))      # the high word of the seed counts
    assert len({tuple(r) for r in base.cpu().numpy()[:, :8].tolist()}) == 4
    # the words are Philox4x32-10's (oracle/noise_ref.py, pinned by Random123's known answers): (k + 0.5) 2^-22 - 1 of the top 23 bits
    q = np.arange(251, dtype=np.uint32)[None, :].repeat(4, 0)
    r = (np.arange(4, dtype=np.uint32) + np.uint32(0))[:, None].repeat(251, 1)
    words = noise_ref.philox4x32_10(q, r, np.uint32(1), np.uint32(0), 77, 0)
    exp = np.stack([((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -22 - 1 for w in words], axis=-1).reshape(4, 1004)[:, :1001]
    assert np.array_equal(base.cpu().numpy().astype(np.float64), exp)


# ------------------------------------------------------------------------------------------------------------ the plugin
def _opt(**kw):
    base = dict(aug='geometric', phase='train', gpu_ids=[0], checkpoints_dir='/tmp', name='geo', p_thres=0.0, horizontal_flip=True, affine=True,
                elastic_deform=True, rotate_limit=3, shift_limit=0.05, verbose_log=False, seed_aug=11)
    base.update(kw)
    return SimpleNamespace(**base)


def _data():
    g = torch.Generator().manual_seed(5)
    names = ['s0', 's1', 's2', 's3']
    return {'A': torch.randn([4, 1, 64, 64], generator=g), 'B': torch.randn([4, 1, 64, 64], generator=g), 'A_paths': names, 'B_paths': list(names)}


def _run(opt, data):
    from latentaugment_amd.augments import create_augment
    aug = create_augment(opt)
    aug.set_input(data)
    aug.forward()
    return aug, aug.get_output()


def test_plugin_end_to_end(dev, geo):
    data = _data()
    aug, out = _run(_opt(), data)
    for k in 'AB':
        assert out[k].dtype == torch.float32 and out[k].device.type == 'cpu' and not out[k].requires_grad and out[k].shape == data[k].shape
    assert out['A_paths'] == data['A_paths'] and out['B_paths'] == data['A_paths'] and len(aug.stats_time) == 1
    p = aug.last_params
    assert all(bool(p[k].all()) for k in ('flip', 'affine', 'elastic'))      # p_thres = 0: every stage, every sample
    # the restatement driven by the batch's parameters; the noise regenerated through la_noise_uniform_f32
    x = torch.cat([data['A'], data['B']], dim=1).numpy().astype(np.float64)
    minv = geo.affine_inverse(p, 64, 64).numpy()
    noise = geo.noise_uniform(4, 2 * 64 * 64, int(p['seed']), device=dev).view(4, 2, 64, 64).cpu().numpy().astype(np.float64)
    taps = np.array(geo.gaussian_taps(63, 32.0).tolist(), np.float32).astype(np.float64)
    ones = np.ones(4, bool)
    exp64 = gc.pipeline(x, minv, ones, noise, taps, (1.0, 1.0), ones)
    exp32 = gc.pipeline(x, minv, ones, noise, taps, (1.0, 1.0), ones, np.float32)
    _within_budget(torch.cat([out['A'], out['B']], dim=1), exp64, exp32, 'plugin 4x2x64x64, all stages')
    assert float(np.abs(exp64 - x).max()) > 0.5
    # A and B of a sample carry the same deformation: warping the pair with the modalities swapped gives the swapped result
    aug2, swapped = _run(_opt(), dict(data, A=data['B'], B=data['A']))
    assert torch.equal(swapped['A'], out['B']) and torch.equal(swapped['B'], out['A'])
    assert all(torch.equal(aug2.last_params[k], p[k]) for k in p)      # same seed: same batch, bit for bit
    aug.forward()
    assert len(aug.stats_time) == 2 and not torch.equal(aug.last_params['angle'], p['angle'])      # the generator moves on
    aug.sanity_check()
    assert len(aug.stats_time) == 3


def test_plugin_mixed_flags_match_the_restatement(dev, geo):
    data = _data()
    aug, out = _run(_opt(p_thres=0.5, seed_aug=6), data)
    p = aug.last_params
    warp = (p['flip'] | p['affine']).numpy()
    assert 0 < int(p['elastic'].sum()) < 4 and 0 < int(warp.sum()) < 4 and not (warp | p['elastic'].numpy()).all()      # this seed: mixed flags, one sample untouched
    x = torch.cat([data['A'], data['B']], dim=1).numpy().astype(np.float64)
    noise = geo.noise_uniform(4, 2 * 64 * 64, int(p['seed']), device=dev).view(4, 2, 64, 64).cpu().numpy().astype(np.float64)
    taps = np.array(geo.gaussian_taps(63, 32.0).tolist(), np.float32).astype(np.float64)
    args = (x, geo.affine_inverse(p, 64, 64).numpy(), warp, noise, taps, (1.0, 1.0), p['elastic'].numpy())
    got = torch.cat([out['A'], out['B']], dim=1)
    _within_budget(got, gc.pipeline(*args), gc.pipeline(*args, np.float32), 'plugin 4x2x64x64, p_thres 0.5')
    for b in range(4):
        if not warp[b] and not p['elastic'][b]:
            assert np.array_equal(got[b].numpy().astype(np.float64), x[b])


def test_plugin_identity_cases(dev):
    data = _data()
    for opt in (_opt(p_thres=1.0), _opt(phase='test'), _opt(phase='val'), _opt(horizontal_flip=False, affine=False, elastic_deform=False)):
        aug, out = _run(opt, data)
        assert torch.equal(out['A'], data['A']) and torch.equal(out['B'], data['B']) and len(aug.stats_time) == 1
        assert out['A'].device.type == 'cpu' and out['A'].dtype == torch.float32
