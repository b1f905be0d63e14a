"""The sliced Wasserstein distance on the GPU: every la_lap_pyr_* / la_swd_* entry at the C ABI and the metrics.py functions above
them, against the float64 restatement of tests/swd_cases.py.

EXACT where float32 can represent every intermediate value (bit for bit against float64): the pyramid of integer pixels, the patch
positions and the gathered rows, la_swd_f32 on integer descriptors and integer "directions" (minimum and ample scratch, swd(A, A) = 0,
swd(A, B) = swd(B, A)), the Python route against the stages run by hand, a set against itself and against its half.
BOUNDED elsewhere, by the bounds derived in swd_cases.py (never measured): the pyramid of float pixels, mean and std, the normalised
rows (one float32 ulp), the directions, la_swd_f32 on float inputs, compute_swd_from_images end to end.  Every bounded case prints
its measured fraction of the bound.

Largest measured on an MI355X, as fractions of the bounds: pyramid 0.051 (2 x 32 x 32, level 0; deeper levels less: 0.026, 0.004,
0.001); mean 3e-4 and std 1e-3 of their float64 summation bounds; normalised rows equal to the float64 quotient rounded once (bound: one
ulp); directions 0.002 of the 2e-5 tolerance, unit norm within 2^-22; la_swd_f32 on floats 0.0006 (M 500, D 98); the image route end to
end below 1e-4 of the composed bound, which the directions' 2e-5 dominates; the features route against the translation identity
0.0006.  Wall time of the file: 3 s for 94 tests.
"""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_cases as sc  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _p(t):
    from latentaugment_amd import _lib
    return _lib.ptr(t)


def _s():
    from latentaugment_amd import _lib
    return _lib.stream_ptr()


def _to(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype))).to(dev)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ok(lib, rc):
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()


# ------------------------------------------------------------------------------------------------------------ the stages by hand
def _pyramid(lib, dev, x, levels):
    """x float [planes][H][W] numpy -> the level arrays (float32 numpy) through the two entries; every output between guard bands"""
    planes, H, W = x.shape
    g = Guarded('ones')
    gs = [g.tensor([planes, H, W], torch.float32, dev, -7.0)]
    gs[0].copy_(_to(x, np.float32, dev))
    with torch.cuda.device(dev):
        for l in range(levels - 1):
            h, w = gs[-1].shape[1:]
            y = g.tensor([planes, h // 2, w // 2], torch.float32, dev, -7.0)
            _ok(lib, lib.la_lap_pyr_down_f32(_p(gs[-1]), _p(y), planes, h, w, _s()))
            gs.append(y)
        for l in range(levels - 1):
            h, w = gs[l].shape[1:]
            _ok(lib, lib.la_lap_pyr_up_sub_f32(_p(gs[l]), _p(gs[l + 1]), planes, h, w, _s()))
    g.check()
    return [t.cpu().numpy() for t in gs]


def _gather(lib, dev, img, img0, level, nhood, per_image, seed):
    n, Cc, H, W = img.shape
    x = _to(img, np.float32, dev)
    g = Guarded('ones')
    desc = g.tensor([n * per_image, Cc * nhood * nhood], torch.float32, dev, -7.0)
    with torch.cuda.device(dev):
        _ok(lib, lib.la_swd_gather_f32(_p(x), n, Cc, H, W, img0, level, nhood, per_image, seed, _p(desc), _s()))
    g.check()
    return desc


def _stats(lib, dev, desc, Cc, pattern='ones'):
    M, P = desc.shape[0], desc.shape[1] // Cc
    g = Guarded(pattern)
    mean, std = g.tensor([Cc], torch.float64, dev, -7.0), g.tensor([Cc], torch.float64, dev, -7.0)
    nbytes = lib.la_swd_stats_scratch_bytes(M, Cc, P)
    ws = g.alloc(nbytes, dev, torch.float64)
    with torch.cuda.device(dev):
        _ok(lib, lib.la_swd_channel_stats_f64(_p(desc), M, Cc, P, _p(mean), _p(std), _p(ws), nbytes, _s()))
    g.check()
    return mean, std


def _normalize(lib, dev, desc, Cc, mean, std):
    with torch.cuda.device(dev):
        _ok(lib, lib.la_swd_normalize_f32(_p(desc), desc.shape[0], Cc, desc.shape[1] // Cc, _p(mean), _p(std), _s()))


def _directions(lib, dev, ndirs, D, dir0, seed):
    g = Guarded('ones')
    d = g.tensor([ndirs, D], torch.float32, dev, -7.0)
    with torch.cuda.device(dev):
        _ok(lib, lib.la_swd_directions_f32(_p(d), ndirs, D, dir0, seed, _s()))
    g.check()
    return d


def _w1(lib, dev, a, b, dirs, ample, pattern='ones'):
    a, b, dirs = (t if torch.is_tensor(t) else _to(t, np.float32, dev) for t in (a, b, dirs))
    (M, D), ndirs = a.shape, dirs.shape[0]
    nbytes = lib.la_swd_scratch_bytes(M, D, ndirs)
    assert nbytes > 0
    if ample:
        nbytes = 16 * M * ndirs + 4096
    g = Guarded(pattern)
    ws = g.alloc(nbytes, dev, torch.float64)
    w = g.tensor([ndirs], torch.float64, dev, -7.0)
    with torch.cuda.device(dev):
        _ok(lib, lib.la_swd_f32(_p(a), _p(b), M, D, _p(dirs), ndirs, _p(w), _p(ws), nbytes, _s()))
    g.check()
    return w.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize('planes', sc.PYR_PLANES)
@pytest.mark.parametrize('shape', sc.PYR_EXACT_SHAPES)
def test_pyramid_of_integer_pixels_is_exact(lib, dev, shape, planes):
    x = sc.integer_images(planes, *shape, seed=11 + planes)
    want = sc.pyramid(x, 3)
    got = _pyramid(lib, dev, x, 3)
    for l, (w, g) in enumerate(zip(want, got)):
        assert g.dtype == np.float32 and _same_bits(g.astype(np.float64), w), f'level {l}: {np.abs(g - w).max()}'


@pytest.mark.parametrize('planes,H,W,levels', [(3, 64, 48, 4), (2, 32, 32, 2), (1, 16, 40, 2), (5, 130, 66, 2)])
def test_pyramid_of_float_pixels_is_bounded(lib, dev, planes, H, W, levels):
    x = np.random.RandomState(H + W).uniform(-1, 1, [planes, H, W]).astype(np.float32)
    want = sc.pyramid(x.astype(np.float64), levels)
    got = _pyramid(lib, dev, x, levels)
    xmax = float(np.abs(x).max())
    for l, (w, g) in enumerate(zip(want, got)):
        err, bound = float(np.abs(g - w).max()), sc.pyramid_bound(l, xmax)
        print(f'pyramid {planes}x{H}x{W} level {l}: measured / bound = {err / bound:.3f}')
        assert err <= bound


def test_python_pyramid_is_the_entries(lib, dev):
    from latentaugment_amd import metrics
    x = np.random.RandomState(3).uniform(-1, 1, [2, 2, 64, 32]).astype(np.float32)
    got = metrics.laplacian_pyramid(_to(x, np.float32, dev), min_resolution=8)
    want = _pyramid(lib, dev, x.reshape(4, 64, 32), 3)
    assert [tuple(t.shape) for t in got] == [(2, 2, 64, 32), (2, 2, 32, 16), (2, 2, 16, 8)]
    assert all(_same_bits(g.cpu().numpy().reshape(w.shape), w) for g, w in zip(got, want))
    assert len(metrics.laplacian_pyramid(_to(x, np.float32, dev))) == 2          # 32 x 16 is the last level at min_resolution 16


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize('Cc', [1, 2, 3])
def test_gather_is_the_restatement_in_any_batches(lib, dev, Cc):
    img = np.random.RandomState(Cc).uniform(-1, 1, [5, Cc, 16, 24]).astype(np.float32)
    want = sc.descriptors(img, 0, 1, 7, 16, seed=5)
    whole = _gather(lib, dev, img, 0, 1, 7, 16, 5).cpu().numpy()
    assert _same_bits(whole, want)
    parts = np.concatenate([_gather(lib, dev, img[:2], 0, 1, 7, 16, 5).cpu().numpy(), _gather(lib, dev, img[2:], 2, 1, 7, 16, 5).cpu().numpy()])
    assert _same_bits(parts, want)
    assert not _same_bits(_gather(lib, dev, img, 0, 2, 7, 16, 5).cpu().numpy(), want)          # another level, other positions
    # the positions themselves, decoded from an image whose pixels are their own coordinates
    coord = (np.arange(16)[:, None] * 32 + np.arange(24)[None, :]).astype(np.float32)
    d = _gather(lib, dev, np.broadcast_to(coord, [5, 1, 16, 24]), 0, 1, 7, 16, 5).cpu().numpy()
    x0, y0 = sc.positions(5, 0, 1, 16, 16, 24, 7, 5)
    assert np.array_equal(d[:, 0].astype(np.int64), (y0 * 32 + x0).ravel())
    assert x0.min() == 0 and x0.max() == 24 - 7 and y0.max() == 16 - 7


# ------------------------------------------------------------------------------------------------------------ stats, normalise
@pytest.mark.parametrize('M,Cc,P', [(80, 2, 49), (700, 3, 49), (5, 1, 9), (3000, 2, 25)])
def test_channel_stats_and_normalisation(lib, dev, M, Cc, P):
    rng = np.random.RandomState(M)
    x = (rng.standard_normal([M, Cc, P]) * (1 + np.arange(Cc))[None, :, None] + 3 * np.arange(Cc)[None, :, None]).astype(np.float32).reshape(M, Cc * P)
    desc = _to(x, np.float32, dev)
    mean, std = _stats(lib, dev, desc, Cc, 'bytes')
    m, s = mean.cpu().numpy(), std.cpu().numpy()
    me, se, sabs = sc.channel_stats_exact(x, Cc)
    n = M * P
    mb = sc.mean_bound(n, sabs)
    sb = sc.std_rel_bound(n, mb, se ** 2) * se
    print(f'stats M {M} C {Cc} P {P}: mean measured / bound = {(np.abs(m - me) / mb).max():.1e}, std {(np.abs(s - se) / sb).max():.1e}')
    assert (np.abs(m - me) <= mb).all() and (np.abs(s - se) <= sb).all()
    _normalize(lib, dev, desc, Cc, mean, std)
    got = desc.cpu().numpy()
    want = sc.normalize(x.astype(np.float64), m, s, Cc)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= ulp).all()
    assert _same_bits(got, want.astype(np.float32))          # in fact the same quotient, rounded once


def test_constant_channel_raises_in_python(dev):
    from latentaugment_amd import metrics
    x = torch.rand([4, 2, 16, 16], device=dev) * 2 - 1
    x[:, 1] = 0.25
    with pytest.raises(ValueError, match='constant'):
        metrics.compute_swd_from_images([x], [x.clone()], nhoods_per_image=8, dir_repeats=1, dirs_per_repeat=4)


# ------------------------------------------------------------------------------------------------------------ directions
@pytest.mark.parametrize('D', [16, 98, 147, 301])
def test_directions(lib, dev, D):
    d = _directions(lib, dev, 12, D, 0, seed=9).cpu().numpy()
    assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 1).max() <= 2.0 ** -22
    assert np.sqrt((sc.raw_normals(12, D, 0, 9).astype(np.float64) ** 2).sum(1)).min() >= 1
    err = np.abs(d - sc.directions(12, D, 0, 9)).max()
    print(f'directions D {D}: measured / tolerance = {err / sc.DIR_TOL:.3f}')
    assert err <= sc.DIR_TOL
    assert _same_bits(_directions(lib, dev, 7, D, 5, seed=9).cpu().numpy(), d[5:])
    assert _same_bits(_directions(lib, dev, 5, D, 0, seed=9).cpu().numpy(), d[:5])
    assert not _same_bits(_directions(lib, dev, 12, D, 0, seed=10).cpu().numpy(), d)


# ------------------------------------------------------------------------------------------------------------ la_swd_f32
@pytest.mark.parametrize('ndirs', sc.SWD_EXACT_NDIRS)
@pytest.mark.parametrize('mname', sc.SWD_EXACT_M)
@pytest.mark.parametrize('D', sc.SWD_EXACT_D)
def test_swd_on_integers_is_exact(lib, dev, D, mname, ndirs):
    M = sc.sort_m(mname, lib.la_sort_tile_keys())
    rng = np.random.RandomState(D * 1000 + ndirs)
    a, b = rng.randint(-3, 4, [M, D]).astype(np.float64), rng.randint(-3, 4, [M, D]).astype(np.float64)
    dirs = rng.randint(-2, 3, [ndirs, D]).astype(np.float64)
    want = sc.w1(a, b, dirs)
    lean = _w1(lib, dev, a, b, dirs, ample=False, pattern='bytes')
    ample = _w1(lib, dev, a, b, dirs, ample=True)
    assert _same_bits(lean, want) and _same_bits(ample, want)
    assert _same_bits(_w1(lib, dev, b, a, dirs, ample=True), want)
    assert _same_bits(_w1(lib, dev, a, a, dirs, ample=False), np.zeros(ndirs))


@pytest.mark.parametrize('M,D,ndirs', [(500, 98, 40), (5000, 147, 33), (9001, 7, 5), (301, 200, 129)])
def test_swd_on_floats_is_bounded(lib, dev, M, D, ndirs):
    rng = np.random.RandomState(M)
    a = rng.standard_normal([M, D]).astype(np.float32)
    b = (rng.standard_normal([M, D]) * 1.5 + 0.3).astype(np.float32)
    dirs = _directions(lib, dev, ndirs, D, 0, seed=M)
    d = dirs.cpu().numpy().astype(np.float64)
    want = sc.w1(a.astype(np.float64), b.astype(np.float64), d)
    bound = sc.w1_bound(D, float(np.abs(a).max()), float(np.abs(b).max()), d)
    got = _w1(lib, dev, a, b, dirs, ample=False)
    print(f'swd M {M} D {D} ndirs {ndirs}: measured / bound = {(np.abs(got - want) / bound).max():.4f}')
    assert (np.abs(got - want) <= bound).all()
    assert _same_bits(_w1(lib, dev, a, b, dirs, ample=True, pattern='bytes'), got)


# ------------------------------------------------------------------------------------------------------------ Python
_KW = dict(nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8)


@pytest.fixture(scope='module')
def sets():
    rng = np.random.RandomState(8)
    real = rng.uniform(-1, 1, [6, 2, 32, 32]).astype(np.float32)
    gen = np.clip(real + 0.3 * rng.standard_normal(real.shape), -1, 1).astype(np.float32)
    return real, gen


@pytest.fixture(scope='module')
def python_result(dev, sets):
    from latentaugment_amd import metrics
    real, gen = sets
    return metrics.compute_swd_from_images([_to(real, np.float32, dev)], [_to(gen, np.float32, dev)], return_details=True, **_KW)


def test_python_is_the_stages_by_hand(lib, dev, sets, python_result):
    out, det = python_result
    assert set(out) == {'swd_32', 'swd_16', 'swd_avg'} and det['num_items'] == 6
    hand = {}
    pyr = [_pyramid(lib, dev, s.reshape(12, 32, 32), 2) for s in sets]
    for l, res in enumerate((32, 16)):
        descs, stats = [], []
        for p in pyr:
            d = _gather(lib, dev, p[l].reshape(6, 2, res, res), 0, l, 7, 16, 0)
            mean, std = _stats(lib, dev, d, 2)
            _normalize(lib, dev, d, 2, mean, std)
            descs.append(d)
            stats.append((mean.cpu().numpy(), std.cpu().numpy()))
        dirs = _directions(lib, dev, 16, 98, l * sc.LEVEL_DIR_STRIDE, 0)
        w = _w1(lib, dev, descs[0], descs[1], dirs, ample=True)
        hand[f'swd_{res}'] = float(w.mean()) * 1e3
        assert _same_bits(det['levels'][l]['w1'], w) and det['levels'][l]['res'] == res
        assert _same_bits(det['levels'][l]['mean'], np.stack([s[0] for s in stats])) and _same_bits(det['levels'][l]['std'], np.stack([s[1] for s in stats]))
    hand['swd_avg'] = float(np.mean([hand['swd_32'], hand['swd_16']]))
    assert hand == {k: out[k] for k in hand}


def test_python_is_within_the_composed_bound_of_the_restatement(sets, python_result):
    out, det = python_result
    real, gen = (s.astype(np.float64) for s in sets)
    want, wdet = sc.swd_images(real, gen, **_KW)
    for l in range(2):
        bound = sc.composed_bound(wdet, l, 2)
        err = np.abs(det['levels'][l]['w1'] - wdet[l]['w1']).max()
        print(f'end to end level {l}: measured / bound = {err / bound:.1e}')
        assert err <= bound
        assert abs(out[f'swd_{32 >> l}'] - want[f'swd_{32 >> l}']) <= 1e3 * bound


def test_python_identities(dev, sets, python_result):
    from latentaugment_amd import metrics
    real, gen = (_to(s, np.float32, dev) for s in sets)
    assert all(v == 0.0 for v in metrics.compute_swd_from_images([real], [real.clone()], **_KW).values())
    assert all(v == 0.0 for v in metrics.compute_swd_from_images([real], [0.5 * real], **_KW).values())
    split = metrics.compute_swd_from_images([real[:4], real[4:]], [gen[:3], gen[3:]], **_KW)
    assert split == python_result[0]
    # the first num_items of each side; a side that cannot fill them is an error
    four = metrics.compute_swd_from_images([real], [gen[:4]], **_KW)
    assert four == metrics.compute_swd_from_images([real[:3], real[3:]], [gen], num_items=4, **_KW) and four != python_result[0]
    with pytest.raises(ValueError, match='num_items'):
        metrics.compute_swd_from_images([real], [gen[:4]], num_items=5, **_KW)
    dicts = metrics.compute_swd_from_images([{'A': real, 'B': gen}], [{'A': gen, 'B': real}], mode='A', **_KW)
    assert dicts == python_result[0]


def test_features_route(lib, dev):
    from latentaugment_amd import metrics
    rng = np.random.RandomState(12)
    a = (np.round(rng.standard_normal([700, 64]) * 1024) / 1024).astype(np.float32)
    t = np.round(rng.standard_normal(64) * 4) / 4          # both on a 2^-10 grid: a + t is exact in float32, the clouds differ by t only
    b = (a.astype(np.float64) + t).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), a.astype(np.float64) + t)
    swd, det = metrics.compute_swd_from_features(a, b, num_dirs=24, seed=3, return_details=True)
    d = det['dirs'].astype(np.float64)
    bound = sc.w1_bound(64, float(np.abs(a).max()), float(np.abs(b).max()), d)
    print(f'features: translation identity measured / bound = {(np.abs(det["w1"] - np.abs(d @ t)) / bound).max():.4f}')
    assert (np.abs(det['w1'] - np.abs(d @ t)) <= bound).all() and swd == float(det['w1'].mean())
    assert _same_bits(det['dirs'], _directions(lib, dev, 24, 64, 0, 3).cpu().numpy())
    # against the restatement end to end: its own directions are within DIR_TOL per component of the device's
    row2 = max(np.sqrt((a.astype(np.float64) ** 2).sum(1)).max(), np.sqrt((b.astype(np.float64) ** 2).sum(1)).max())
    assert abs(swd - sc.swd_features(a, b, 24, 3)) <= bound.max() + 2 * row2 * np.sqrt(64) * (sc.DIR_TOL + sc.U32)
    assert metrics.compute_swd_from_features(a, a.copy(), num_dirs=24) == 0.0
    assert metrics.compute_swd_from_features(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev).double(), num_dirs=24, seed=3) == swd
    with pytest.raises(ValueError, match='one size'):
        metrics.compute_swd_from_features(a, b[:-1])


def test_aug_dataset(dev, sets, python_result, tmp_path):
    from latentaugment_amd import metrics
    real, gen = sets
    run = tmp_path / 'run'
    os.makedirs(run / 'img')
    os.makedirs(run / 'img_aug')
    for i, (lo, hi) in enumerate(((0, 2), (2, 6))):          # as the reference's driver writes them: one dict of batches per file
        with open(run / 'img' / f'img_{i}', 'wb') as f:
            pickle.dump({'A': torch.from_numpy(real[lo:hi, :1].copy()), 'B': torch.from_numpy(real[lo:hi, 1:].copy()), 'A_paths': ['p'] * (hi - lo)}, f)
        with open(run / 'img_aug' / f'img_aug_{i}', 'wb') as f:
            pickle.dump({'A': gen[lo:hi, :1].copy(), 'B': gen[lo:hi, 1:].copy()}, f, protocol=pickle.HIGHEST_PROTOCOL)
    assert metrics.compute_swd_for_aug_dataset(str(run), **_KW) == python_result[0]


def test_metrics_from_images_flag(dev, tmp_path, monkeypatch):
    import helpers_script_detector as hsd
    from latentaugment_amd import metrics
    from latentaugment_amd.synthesis import DetectorEngine
    path = tmp_path / 'det.pt'
    hsd.save_scripted_detector(path)          # the small scripted detector of the detector tests
    det = DetectorEngine.from_torchscript(str(path), dev, max_batch=4)
    g = torch.Generator().manual_seed(31)
    real = [torch.rand([4, 1, 40, 40], generator=g) * 2 - 1 for _ in range(3)]
    gen = [torch.rand([4, 1, 40, 40], generator=g) * 1.6 - 0.8 for _ in range(2)]
    called = []
    monkeypatch.setattr(metrics, '_swd_descriptor_banks', lambda *a, **k: called.append(1))
    plain = metrics.compute_metrics_from_images(real, gen, det, nhood_size=3)
    assert set(plain) == {'precision', 'recall', 'density', 'coverage', 'kid'} and not called          # off: nothing of it runs
    monkeypatch.undo()
    out = metrics.compute_metrics_from_images(iter(real), iter(gen), det, nhood_size=3, swd=True, **_KW)
    assert set(out) == set(plain) | {'swd_40', 'swd_20', 'swd_avg'} and all(out[k] == plain[k] for k in plain)
    want = metrics.compute_swd_from_images([torch.cat(real)[:8].to(dev)], [torch.cat(gen).to(dev)], **_KW)
    assert {k: out[k] for k in want} == want and want['swd_avg'] > 0
