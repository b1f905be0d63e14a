"""Style and content distance through the trunk and the metric: la_feat_style_distance, FeatureEngine.style_distance_rows,
metrics.compute_style_content and compute_pair_metrics(nst_net=) against the reference's NSTLoss / VGG19Net run recorded in
tests/golden/nst.npz (narrow VGG19, 32^2 and 48^2 inputs: the last tap is 2 x 2 and 3 x 3, HW = 4 and HW = 9 through the trunk path).

The engine runs in precision 'f32' and is held against the reference's float64 values under the project's rule
lpips_cases.bound(ref64, ref32): 4 x the error of the reference's own float32 run + 2e-6 x the largest value -- per tap, per channel
and for the totals.  Chunked calls, a used handle and the pair-metrics route must give the same BITS as the plain call.

Measured on an MI355X: the largest error / bound over layers, per-channel values and totals is 0.48 (style, tap 3, R = 32), and 0.47 for
the close pair alone; wall time of the file 3 s.
"""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import nst_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'style', 'content', 'style_per_channel', 'content_per_channel', 'style_layers', 'content_layers'}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'nst.npz'))


def _engine(fx, dev, R, max_batch=12):
    from latentaugment_amd import synthesis
    net = synthesis.nst_reference_net(nc.fixture_state_dict(fx))
    assert net.pre_scale == (0.5,) * 3 and net.pre_shift == (128.0 / 255.0,) * 3
    eng = synthesis.FeatureEngine.from_net(net, dev, in_res=R, max_batch=max_batch, precision='f32')
    assert eng.num_taps == 5
    return eng


_PLAIN = {}


def _plain(fx, dev, R):
    """compute_style_content of the fixture's three pairs on an engine that takes them at once, computed once"""
    from latentaugment_amd import metrics
    if R not in _PLAIN:
        x, y = torch.tensor(fx[f'nst{R}_x']).to(dev), torch.tensor(fx[f'nst{R}_y']).to(dev)
        _PLAIN[R] = (x, y, metrics.compute_style_content(x, y, _engine(fx, dev, R)))
    return _PLAIN[R]


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == torch.float64 and a[k].shape == b[k].shape and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


@pytest.mark.parametrize('R', [32, 48])
def test_against_the_reference_fixture(fx, dev, R):
    """Measured: see the module docstring."""
    from latentaugment_amd import synthesis
    _, _, got = _plain(fx, dev, R)
    assert set(got) == KEYS and all(v.dtype == torch.float64 and v.device.type == 'cpu' for v in got.values())
    s64, s32, c64, c32 = (fx[f'nst{R}_{k}'] for k in ('style64', 'style32', 'content64', 'content32'))
    assert got['style_layers'].shape == (3, 2, 5) and got['content_per_channel'].shape == (3, 2) and got['style'].shape == (3,)
    for t in range(5):
        lc.check(f'R {R} style tap {t}', got['style_layers'][:, :, t], s64[:, :, t], s32[:, :, t])
        lc.check(f'R {R} content tap {t}', got['content_layers'][:, :, t], c64[:, :, t], c32[:, :, t])
    ct = synthesis.NST_CONTENT_TAP
    assert ct == 3
    lc.check(f'R {R} style per channel', got['style_per_channel'], s64.sum(2), s32.sum(2))
    lc.check(f'R {R} content per channel', got['content_per_channel'], c64[:, :, ct], c32[:, :, ct])
    lc.check(f'R {R} style', got['style'], s64.sum(2).mean(1), s32.sum(2).mean(1))
    lc.check(f'R {R} content', got['content'], c64[:, :, ct].mean(1), c32[:, :, ct].mean(1))
    # the close pair on its own: the reference's float32 run forms G1 - G2 from two rounded Grams, this library from D and S
    lc.check(f'R {R} style, close pair', got['style_layers'][0], s64[0], s32[0])
    lc.check(f'R {R} content, close pair', got['content_layers'][0], c64[0], c32[0])


def test_exactness_of_the_metric(fx, dev):
    from latentaugment_amd import metrics
    x, y, got = _plain(fx, dev, 32)
    eng = _engine(fx, dev, 32)
    zero = metrics.compute_style_content(x, x, eng)
    assert all(float(v.abs().max()) == 0.0 for v in zero.values())
    _same(metrics.compute_style_content(y, x, eng), got)
    _same(metrics.compute_style_content(x, y, eng), got)
    assert bool((got['style_layers'] > 0).all()) and bool((got['content_layers'] > 0).all())
    # content_tap selects the column; clamp=False differs where the clamp acts
    other = metrics.compute_style_content(x, y, eng, content_tap=0)
    assert torch.equal(other['content_per_channel'], got['content_layers'][:, :, 0]) and torch.equal(other['style'], got['style'])
    unclamped = metrics.compute_style_content(x, y, eng, clamp=False)
    assert not torch.equal(unclamped['style_layers'], got['style_layers'])
    lo, hi = -128.0 / 127.5, 127.0 / 127.5
    _same(metrics.compute_style_content(x.clamp(lo, hi), y.clamp(lo, hi), eng, clamp=False), got)
    # gathered pairs
    ix, iy = np.array([2, 0, 1, 1], np.int32), np.array([2, 0, 1, 0], np.int32)
    gathered = metrics.compute_style_content(x, y, eng, pairs=(ix, iy))
    for k in got:
        assert gathered[k][:3].numpy().tobytes() == got[k][[2, 0, 1]].numpy().tobytes(), k
    assert gathered['style'].shape == (4,) and float(gathered['style'][3]) > 0


@pytest.mark.parametrize('R', [32, 48])
def test_chunking_gives_the_same_bits(fx, dev, R):
    """max_batch = 4: one two-channel pair per call; max_batch = 9: two pairs, then one."""
    from latentaugment_amd import metrics
    x, y, got = _plain(fx, dev, R)
    for mb in (4, 9):
        _same(metrics.compute_style_content(x, y, _engine(fx, dev, R, max_batch=mb)), got)


def test_history_contract(fx, dev):
    """After la_feat_style_distance a forward / pair_distance gives the bits of a fresh handle, and backward refuses until the next
    forward; the style call after them gives its own bits again."""
    from latentaugment_amd import _lib, metrics
    x, y, got = _plain(fx, dev, 32)
    used, fresh = _engine(fx, dev, 32), _engine(fx, dev, 32)
    rows = (torch.cat([x[:, :1], y[:, :1]]).repeat(1, 3, 1, 1) * 0.5 + 128.0 / 255.0).contiguous()
    f_fresh = fresh.forward(rows)
    d_fresh = fresh.pair_distance(rows[:3], rows[3:])
    f_used = used.forward(rows)
    metrics.compute_style_content(x, y, used)
    with pytest.raises(_lib.LatentAugHipError):
        used.backward(torch.zeros_like(f_used))
    assert torch.equal(used.forward(rows), f_fresh)
    gx = used.backward(torch.ones_like(f_used))          # and after a forward it runs again
    assert gx.shape == rows.shape and bool(torch.isfinite(gx).all())
    metrics.compute_style_content(x, y, used)
    assert torch.equal(used.pair_distance(rows[:3], rows[3:]), d_fresh)
    _same(metrics.compute_style_content(x, y, used), got)


def test_pair_metrics_route(fx, dev):
    from latentaugment_amd import metrics
    x, y, got = _plain(fx, dev, 32)
    eng = _engine(fx, dev, 32)
    base = metrics.compute_pair_metrics(x, y, levels=2)
    assert set(base) == {'mse', 'mae', 'psnr', 'ssim', 'ms_ssim', 'mse_per_channel', 'mae_per_channel', 'psnr_per_channel', 'ssim_per_channel',
                         'ms_ssim_per_channel', 'ssim_levels', 'cs_levels'}
    with_ = metrics.compute_pair_metrics(x, y, levels=2, nst_net=eng)
    assert set(with_) == set(base) | KEYS
    for k in base:
        assert base[k].dtype == with_[k].dtype and np.array_equal(base[k].numpy(), with_[k].numpy(), equal_nan=True), k
    _same({k: with_[k] for k in KEYS}, got)
    ix, iy = np.array([1, 2], np.int32), np.array([1, 0], np.int32)
    _same({k: v for k, v in metrics.compute_pair_metrics(x, y, pairs=(ix, iy), levels=2, nst_net=eng).items() if k in KEYS},
          metrics.compute_style_content(x, y, eng, pairs=(ix, iy)))


def test_aug_dataset_route(fx, dev, tmp_path):
    """compute_pair_metrics_for_aug_dataset passes nst_net through: the keys of compute_style_content over all files, and their means."""
    from latentaugment_amd import metrics
    x, y, got = _plain(fx, dev, 32)
    eng = _engine(fx, dev, 32)
    run = tmp_path / 'run'
    os.makedirs(run / 'img')
    os.makedirs(run / 'img_aug')
    for i, (a, b) in enumerate(((0, 2), (2, 3))):
        src, aug = x[a:b].cpu().numpy(), y[a:b].cpu().numpy()
        with open(run / 'img' / f'img_{i}', 'wb') as f:
            pickle.dump({'A': src[:, :1].copy(), 'B': src[:, 1:].copy()}, f)
        with open(run / 'img_aug' / f'img_aug_{i}', 'wb') as f:
            pickle.dump({'A': aug[:, :1].copy(), 'B': aug[:, 1:].copy()}, f)
    out = metrics.compute_pair_metrics_for_aug_dataset(str(run), levels=2, nst_net=eng)
    assert out['num_items'] == 3
    _same({k: out[k] for k in KEYS}, got)
    assert out['style_mean'] == float(got['style'].mean()) and out['content_mean'] == float(got['content'].mean())
    plain = metrics.compute_pair_metrics_for_aug_dataset(str(run), levels=2)
    assert not (set(plain) & (KEYS | {'style_mean', 'content_mean'})) and plain['mse_mean'] == out['mse_mean']


def test_refusals_leave_the_device_usable(fx, dev):
    from latentaugment_amd import _lib, metrics
    from latentaugment_amd.synthesis import FeatureEngine
    x, y, got = _plain(fx, dev, 32)
    eng = _engine(fx, dev, 32, max_batch=4)
    with pytest.raises(ValueError, match='32'):
        metrics.compute_style_content(x[:, :, :16, :16].contiguous(), y[:, :, :16, :16].contiguous(), eng)
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        metrics.compute_style_content(x.cpu(), y, eng)
    with pytest.raises(ValueError):
        metrics.compute_style_content(x, y[:1], eng)
    with pytest.raises(ValueError, match='content_tap'):
        metrics.compute_style_content(x, y, eng, content_tap=5)
    with pytest.raises(_lib.LatentAugHipError, match='max_batch'):
        metrics.compute_style_content(x, y, _engine(fx, dev, 32, max_batch=2))          # one two-channel pair is four rows
    g = torch.Generator().manual_seed(1)
    det = FeatureEngine([('fc', torch.randn([5, 3 * 32 * 32], generator=g) * 0.01, torch.zeros([5]), False)], dev, in_res=32, max_batch=4)
    with pytest.raises(_lib.LatentAugHipError, match='detector'):
        metrics.compute_style_content(x, y, det)
    # the C entries themselves: refused before any launch
    lib = _lib.load()
    buf = torch.full([4096], -7.0, dtype=torch.float64, device=dev)
    xy = torch.zeros([4, 3, 32, 32], device=dev)
    assert lib.la_feat_style_scratch_bytes(det.handle, 1) == 0 and lib.la_feat_style_scratch_bytes(eng.handle, 3) == 0
    assert lib.la_feat_style_scratch_bytes(eng.handle, 0) == 0 and lib.la_feat_style_scratch_bytes(None, 1) == 0
    need = lib.la_feat_style_scratch_bytes(eng.handle, 2)
    assert need > 0 and need >= lib.la_feat_style_scratch_bytes(eng.handle, 1) > 0
    ws = torch.empty([need // 8], dtype=torch.float64, device=dev)

    def call(h, P, nbytes):
        with torch.cuda.device(dev):
            return lib.la_feat_style_distance(h, _lib.ptr(xy), P, _lib.ptr(buf), _lib.ptr(buf[2048:]), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    assert call(det.handle, 1, need) == -1 and call(eng.handle, 3, need) == -1 and call(eng.handle, 0, need) == -1
    assert call(eng.handle, 2, need - 1) == -3 and b'la_feat_style_scratch_bytes' in lib.la_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())          # nothing was launched
    _same(metrics.compute_style_content(x, y, eng), got)
