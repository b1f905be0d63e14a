"""Host side of GeometricAugment (csrc/la_geom.hip, latentaugment_amd/geometric.py, augments/geometric_aug.py).  No GPU:
- the numpy restatement of tests/geometric_cases.py equals torch on the CPU in float64 -- F.grid_sample (bilinear, align_corners=False)
  for the three padding modes, F.conv2d with zero padding for the blur -- within 1e-12 x max(1, max |expected|), so the GPU tests may use
  it as their float64 expectation; the reference's own plugin needs kornia, which is not a dependency here, so there is no golden file;
- the registry finds the plugin and its options are the reference's (names and defaults of geometric_aug.py:24-30);
- draw_params / affine_inverse: determinism, ranges, p = 0 and p = 1, M Minv = I, flip composed with affine = flip then affine;
- the new header entries are exported and refuse bad arguments before any launch; the wrappers refuse host tensors;
- the position-to-corner function (csrc/la_geom_index.h) is compiled into a stand-alone host program with -fsanitize=undefined,address
  and fed NaN, infinities, huge values, +-2^23 and every quarter-pixel position across several periods: nothing it marks as addressable
  lies outside the image, and its weights are the restatement's, bit for bit."""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometric_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('la_noise_uniform_f32', 'la_elastic_field_f32', 'la_warp_affine_f32', 'la_warp_elastic_f32')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _close(got, exp, what):
    exp = np.asarray(exp, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - exp).max(initial=0.0))
    assert got.shape == exp.shape and err <= 1e-12 * max(1.0, float(np.abs(exp).max(initial=0.0))), (what, err)


def _torch_sample(x, px, py, mode):
    """F.grid_sample at float64 pixel positions: the grid value whose un-normalisation ((g + 1) size - 1) / 2 is the position."""
    H, W = x.shape[2:]
    grid = np.stack([(2 * px + 1) / W - 1, (2 * py + 1) / H - 1], axis=-1)
    return F.grid_sample(torch.from_numpy(x), torch.from_numpy(grid), mode='bilinear', padding_mode=mode, align_corners=False).numpy()


def _matrices(rng, H, W):
    """float32 inverse maps: shifts to exactly -0.5 and size - 0.5, integer and fractional shifts beyond 2 size (several bounces), rotations."""
    ms = [gc.translation(0.5, 0)[0], gc.translation(-0.5, 0.5)[0], gc.translation(0, -0.5)[0], gc.translation(1, -1)[0],
          gc.translation(W, -H)[0], gc.translation(2 * W + 3, -(2 * H + 3))[0], gc.translation(-(2 * W + 3.25), 4 * H + 0.75)[0],
          gc.translation(5.5 * W, -7.25 * H)[0]]
    for _ in range(4):
        a = rng.uniform(-np.pi, np.pi)
        s = rng.uniform(0.5, 2.0)
        ms.append(np.array([s * np.cos(a), s * np.sin(a), rng.uniform(-3 * W, 3 * W), -s * np.sin(a), s * np.cos(a), rng.uniform(-3 * H, 3 * H)], np.float32))
    return np.stack(ms).astype(np.float32)


@pytest.mark.parametrize('mode', gc.MODES)
@pytest.mark.parametrize('shape', [(5, 7), (8, 8), (1, 6), (4, 1), (1, 1), (2, 9)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_restatement_equals_torch_grid_sample(mode, shape):
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    minv = _matrices(rng, H, W)
    B = minv.shape[0]
    x = rng.standard_normal((B, 2, H, W))
    px, py = gc.affine_positions(minv, H, W)
    if H > 1 and W > 1:      # the table really holds the positions it claims
        assert (px == -0.5).any() and (px == W - 0.5).any() and (py == -0.5).any() and (py == H - 0.5).any()
        assert (np.abs(px) > 4 * W).any() and (np.abs(py) > 4 * H).any()
    _close(gc.warp_affine(x, minv, np.ones(B), mode), _torch_sample(x, px, py, mode), (mode, shape))
    # the elastic warp's positions through the same sampler; a displacement of 40 x noise makes the clamp bite
    disp = 0.4 * rng.standard_normal((B, 2, H, W))
    ex, ey = gc.elastic_positions(disp)
    assert W == 1 or ((ex == -0.5).any() and (ex == W - 0.5).any())      # (g clamped to -1 and to 1)
    _close(gc.warp_elastic(x, disp, np.ones(B), mode), _torch_sample(x, ex, ey, mode), (mode, shape, 'elastic'))


def test_restatement_refuses_what_the_kernels_refuse():
    x = np.ones((1, 1, 4, 4))
    for mode in gc.MODES:
        for bad in (np.nan, np.inf, -np.inf, 1e30, 2.0 ** 23 + 1):
            y = gc.sample(x, np.full((1, 1, 1), bad), np.full((1, 1, 1), 1.0), mode)
            assert y.shape == (1, 1, 1, 1) and y[0, 0, 0, 0] == 0, (mode, bad)
    assert gc.sample(x, np.full((1, 1, 1), 2.0 ** 23), np.full((1, 1, 1), 1.0), 'border')[0, 0, 0, 0] == 1
    d = np.zeros((1, 2, 4, 4))
    d[0, 0, 1, 2] = np.nan
    y = gc.warp_elastic(x, d, [1], 'reflection')
    assert y[0, 0, 1, 2] == 0 and np.count_nonzero(y) == 15
    keep = gc.warp_affine(np.arange(32.0).reshape(2, 1, 4, 4), gc.translation(1, 0, 2), [0, 1], 'zeros')
    assert np.array_equal(keep[0, 0], np.arange(16.0).reshape(4, 4)) and keep[1, 0, 0, 0] == 0 and keep[1, 0, 0, 1] == 16


@pytest.mark.parametrize('ntaps', [1, 3, 9, 63])
def test_restatement_equals_torch_conv2d(ntaps):
    from latentaugment_amd import geometric
    rng = np.random.default_rng(ntaps)
    taps = geometric.gaussian_taps(ntaps, 32.0).numpy() if ntaps > 1 else np.array([0.75])
    if ntaps == 9:
        taps = rng.standard_normal(9)      # not symmetric: a correlation, as conv2d, not a convolution
    for H, W in ((16, 16), (33, 70)):
        noise = rng.uniform(-1, 1, (2, 2, H, W))
        w = torch.from_numpy(np.outer(taps, taps))[None, None]
        exp = F.conv2d(torch.from_numpy(noise).reshape(4, 1, H, W), w, padding=ntaps // 2).reshape(2, 2, H, W).numpy()
        exp = exp * np.array([1.5, -0.25]).reshape(1, 2, 1, 1)
        _close(gc.blur(noise, taps, (1.5, -0.25)), exp, (ntaps, H, W))


def test_gaussian_taps():
    from latentaugment_amd import geometric
    t = geometric.gaussian_taps(63, 32.0)
    assert t.dtype == torch.float64 and t.shape == (63,) and abs(float(t.sum()) - 1) < 1e-15
    assert torch.equal(t, t.flip(0)) and int(t.argmax()) == 31
    assert abs(float(t[0] / t[31]) - np.exp(-31 ** 2 / (2 * 32.0 ** 2))) < 1e-15
    for bad in ((4, 1.0), (0, 1.0), (3, 0.0)):
        with pytest.raises(ValueError):
            geometric.gaussian_taps(*bad)


# ------------------------------------------------------------------------------------------------------------ registry and options
def test_registry_finds_the_plugin_with_the_reference_options():
    from latentaugment_amd.augments import find_augment_using_name, get_option_setter
    from latentaugment_amd.augments.base_aug import BaseAugment
    cls = find_augment_using_name('geometric')
    assert cls.__name__ == 'GeometricAugment' and issubclass(cls, BaseAugment)
    parser = get_option_setter('geometric')(argparse.ArgumentParser(), True)
    got = vars(parser.parse_args([]))
    assert got == {'p_thres': 0.5, 'horizontal_flip': False, 'affine': False, 'elastic_deform': False, 'rotate_limit': 3, 'shift_limit': 0.05,
                   'verbose_log': False}
    on = vars(parser.parse_args(['--horizontal_flip', '--affine', '--elastic_deform', '--rotate_limit', '7.5', '--p_thres', '0.25']))
    assert on['horizontal_flip'] and on['affine'] and on['elastic_deform'] and on['rotate_limit'] == 7.5 and on['p_thres'] == 0.25
    types = {a.dest: a.type for a in parser._actions}
    assert types['p_thres'] is float and types['rotate_limit'] is float and types['shift_limit'] is float and types['verbose_log'] is bool


def test_plugin_phases_without_a_device():
    from types import SimpleNamespace
    from latentaugment_amd.augments import create_augment
    base = dict(aug='geometric', gpu_ids=[], checkpoints_dir='/tmp', name='geo', p_thres=0.5, horizontal_flip=True, affine=True,
                elastic_deform=True, rotate_limit=3, shift_limit=0.05, verbose_log=False)
    with pytest.raises(NotImplementedError):
        create_augment(SimpleNamespace(phase='other', **base))
    aug = create_augment(SimpleNamespace(phase='val', **base))
    a, b = torch.randn([2, 1, 6, 5]), torch.randn([2, 1, 6, 5])
    aug.set_input({'A': a, 'B': b, 'A_paths': ['p', 'q'], 'B_paths': ['p', 'q']})
    aug.forward()
    out = aug.get_output()
    assert torch.equal(out['A'], a) and torch.equal(out['B'], b) and out['A_paths'] == ['p', 'q'] and len(aug.stats_time) == 1
    aug.sanity_check()
    assert len(aug.stats_time) == 2
    # the training pipeline has no host implementation: a CPU batch is refused, never computed elsewhere
    from latentaugment_amd import _lib
    aug = create_augment(SimpleNamespace(phase='train', seed_aug=1, **{**base, 'p_thres': 0.0}))
    aug.set_input({'A': a, 'B': b, 'A_paths': ['p', 'q'], 'B_paths': ['p', 'q']})
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        aug.forward()


# ------------------------------------------------------------------------------------------------------------ parameters
def test_draw_params_are_deterministic_and_in_range():
    from latentaugment_amd import geometric
    B, H, W = 64, 40, 100
    draw = lambda seed, p, **kw: geometric.draw_params(torch.Generator().manual_seed(seed), B, H, W, p, **kw)      # noqa: E731
    a, b, c = draw(5, 0.5), draw(5, 0.5), draw(6, 0.5)
    assert set(a) == {'flip', 'affine', 'elastic', 'angle', 'tx', 'ty', 'seed'}
    assert all(torch.equal(a[k], b[k]) for k in a) and not all(torch.equal(a[k], c[k]) for k in a)
    for k in ('flip', 'affine', 'elastic'):
        assert a[k].dtype == torch.bool and a[k].shape == (B,) and 0 < int(a[k].sum()) < B
    assert not torch.equal(a['flip'], a['affine']) and not torch.equal(a['affine'], a['elastic'])      # drawn independently
    assert float(a['angle'].abs().max()) <= 3 and float(a['angle'].abs().max()) > 2
    assert float(a['tx'].abs().max()) <= 0.05 * W and float(a['tx'].abs().max()) > 0.03 * W
    assert float(a['ty'].abs().max()) <= 0.05 * H and float(a['ty'].abs().max()) > 0.03 * H
    assert a['seed'].dtype == torch.int64 and a['seed'].ndim == 0 and int(a['seed']) >= 0
    wide = draw(5, 0.5, rotate_limit=30, shift_limit=1.5)
    assert 20 < float(wide['angle'].abs().max()) <= 30 and W < float(wide['tx'].abs().max()) <= 1.5 * W
    none, every = draw(7, 0.0), draw(7, 1.0)
    assert not any(bool(none[k].any()) for k in ('flip', 'affine', 'elastic'))
    assert all(bool(every[k].all()) for k in ('flip', 'affine', 'elastic'))
    off = draw(7, 1.0, flip=False, elastic=False)
    assert not off['flip'].any() and off['affine'].all() and not off['elastic'].any()
    assert torch.equal(off['angle'], every['angle'])      # switching a stage does not move the others' draws
    g = torch.Generator().manual_seed(9)
    first, second = geometric.draw_params(g, 4, H, W, 0.5), geometric.draw_params(g, 4, H, W, 0.5)
    assert not torch.equal(first['angle'], second['angle']) and int(first['seed']) != int(second['seed'])


def test_affine_inverse_inverts_in_float64_and_composes_the_flip():
    from latentaugment_amd import geometric
    B, H, W = 16, 33, 70
    p = geometric.draw_params(torch.Generator().manual_seed(3), B, H, W, 0.5, rotate_limit=30, shift_limit=1.5)
    assert 0 < int(p['flip'].sum()) < B and 0 < int(p['affine'].sum()) < B
    M = geometric.affine_forward(p, H, W)
    assert M.dtype == torch.float64 and M.shape == (B, 3, 3)
    Minv = torch.linalg.inv(M)
    assert float((M @ Minv - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12
    m32 = geometric.affine_inverse(p, H, W)
    assert m32.dtype == torch.float32 and m32.shape == (B, 6) and m32.is_contiguous()
    assert torch.equal(m32, Minv[:, :2].reshape(B, 6).float())
    # neither flag: the identity, exactly; flip alone: x -> W - 1 - x, exactly
    for b in range(B):
        if not p['affine'][b]:
            assert m32[b].tolist() == ([-1, 0, W - 1, 0, 1, 0] if p['flip'][b] else [1, 0, 0, 0, 1, 0])
    # OpenCV's convention: a positive angle turns the picture counter-clockwise on the screen (y down) -- the point right of the centre goes up
    one = {'flip': torch.tensor([False]), 'affine': torch.tensor([True]), 'angle': torch.tensor([90.0], dtype=torch.float64),
           'tx': torch.tensor([2.0], dtype=torch.float64), 'ty': torch.tensor([-1.0], dtype=torch.float64)}
    q = geometric.affine_forward(one, 9, 9)[0] @ torch.tensor([6.0, 4.0, 1.0], dtype=torch.float64)
    assert float((q - torch.tensor([4.0 + 2, 2.0 - 1, 1.0], dtype=torch.float64)).abs().max()) < 1e-12
    # flip composed with the affine map = the flip (exact), then the affine warp of the flipped picture; in float64 throughout
    rng = np.random.default_rng(0)
    x = rng.standard_normal((B, 2, H, W))
    composed = gc.sample(x, *_positions64(Minv, H, W), 'reflection')
    only_affine = dict(p, flip=torch.zeros(B, dtype=torch.bool))
    flipped = np.where(p['flip'].numpy()[:, None, None, None], x[..., ::-1], x)
    in_sequence = gc.sample(flipped, *_positions64(torch.linalg.inv(geometric.affine_forward(only_affine, H, W)), H, W), 'reflection')
    assert float(np.abs(composed - in_sequence).max()) <= 1e-9      # positions agree to ~1e-13 px; a pixel's slope is a few units
    assert float(np.abs(composed - x).max()) > 0.5


def _positions64(minv, H, W):
    m = minv.numpy()[:, :2].reshape(-1, 6)[:, :, None, None]
    xs, ys = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    return m[:, 0] * xs + m[:, 1] * ys + m[:, 2], m[:, 3] * xs + m[:, 4] * ys + m[:, 5]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_bound_and_exported(lib):
    from latentaugment_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    for name in NEW:
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    P, I, L, Fl = C.c_void_p, C.c_int, C.c_long, C.c_float
    S = _lib.SIGNATURES
    assert S['la_noise_uniform_f32'] == S['la_noise_normal_f32'] == (I, [P, L, L, C.c_ulonglong, C.c_uint, L, P])
    assert S['la_elastic_field_f32'] == (I, [P, P, I, Fl, Fl, P, P, I, I, I, P])
    assert S['la_warp_affine_f32'] == S['la_warp_elastic_f32'] == (I, [P] * 4 + [I] * 5 + [P])


def _err(lib):
    return (lib.la_last_error() or b'').decode()


def test_arguments_are_checked_before_any_launch(lib):
    buf, other = (C.c_double * 64)(), (C.c_double * 64)()      # never dereferenced by a kernel: every call below is refused before a launch
    p, q = C.addressof(buf), C.addressof(other)
    taps = (C.c_float * 63)(*([1.0] * 63))
    for name in ('la_warp_affine_f32', 'la_warp_elastic_f32'):
        fn = getattr(lib, name)
        good = (2, 3, 4, 8)
        for k in range(4):
            args = [p, p, p, q]
            args[k] = None
            assert fn(*args, *good, 2, None) != 0 and 'null pointer' in _err(lib), (name, k)
        assert fn(p, q, q, p, *good, 2, None) != 0 and 'alias' in _err(lib), name
        for k in range(4):
            dims = list(good)
            dims[k] = 0
            assert fn(p, p, p, q, *dims, 2, None) != 0 and 'empty' in _err(lib), (name, k)
        for mode in (-1, 3, 7):
            assert fn(p, p, p, q, *good, mode, None) != 0 and 'unknown padding mode' in _err(lib), (name, mode)
        assert fn(p, p, p, q, 4, 1024, 1024, 1024, 2, None) != 0 and 'INT_MAX' in _err(lib), name
        assert fn(p, p, p, q, 65536, 1, 1, 1, 2, None) != 0 and '65535' in _err(lib), name
    ef = lib.la_elastic_field_f32
    for k in (0, 1, 5):
        args = [p, taps, 63, 1.0, 1.0, q]
        args[k] = None
        assert ef(*args, None, 2, 8, 8, None) != 0 and 'null pointer' in _err(lib), k
    assert ef(p, taps, 63, 1.0, 1.0, p, None, 2, 8, 8, None) != 0 and 'alias' in _err(lib)
    for ntaps in (0, -1, 2, 62, 64, 65):
        assert ef(p, taps, ntaps, 1.0, 1.0, q, None, 2, 8, 8, None) != 0 and 'ntaps' in _err(lib), ntaps
    for dims in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
        assert ef(p, taps, 3, 1.0, 1.0, q, None, *dims, None) != 0 and 'empty' in _err(lib), dims
    assert ef(p, taps, 3, 1.0, 1.0, q, None, 1024, 1024, 1024, None) != 0 and 'INT_MAX' in _err(lib)
    nu = lib.la_noise_uniform_f32
    assert nu(None, 2, 8, 1, 0, 0, None) != 0 and 'bad arguments' in _err(lib)
    assert nu(p, -1, 8, 1, 0, 0, None) != 0 and nu(p, 2, 0, 1, 0, 0, None) != 0 and nu(p, 2, 8, 1, 0, -1, None) != 0
    assert nu(p, 2, 8, 1, 0, 0xffffffff, None) != 0 and '32 bits' in _err(lib)
    assert nu(None, 0, 8, 1, 0, 0, None) == 0      # no rows: nothing to do


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from latentaugment_amd import _lib, geometric
    x = torch.zeros([2, 2, 4, 4])
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        geometric.warp_affine(x, torch.zeros([2, 6]), torch.ones([2]))
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        geometric.warp_elastic(x, torch.zeros([2, 2, 4, 4]), torch.ones([2]))
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        geometric.elastic_field(torch.zeros([2, 2, 4, 4]), [1.0])
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        geometric.noise_uniform(2, 8, 1, device='cpu')
    with pytest.raises(_lib.LatentAugHipError, match='padding_mode'):
        geometric.warp_affine(x, torch.zeros([2, 6]), torch.ones([2]), padding_mode='wrap')
    with pytest.raises(_lib.LatentAugHipError, match='minv'):
        geometric.warp_affine(x, torch.zeros([2, 5]), torch.ones([2]))
    with pytest.raises(_lib.LatentAugHipError, match='disp'):
        geometric.warp_elastic(x, torch.zeros([2, 2, 4, 5]), torch.ones([2]))


# ------------------------------------------------------------------------------------------------------------ the index header
def test_index_function_under_sanitizers(tmp_path):
    """csrc/la_geom_index.h in a stand-alone host program (tests/tools/geom_index_check.cpp) built with -fsanitize=undefined,address and
    run as its own process: the program reads a `size`-element array through every neighbour the function marks as addressable and fails
    on a weighted or marked neighbour outside [0, size); its printed rows are compared here with the restatement's axis, bit for bit, in
    float32 and float64, for the three modes and sizes 1, 2, 5, 8."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = tmp_path / 'geom_index_check'
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=undefined,address', '-fno-sanitize-recover=all',
                        '-I' + os.path.join(ROOT, 'latentaugment_amd', 'csrc'), os.path.join(ROOT, 'tests', 'tools', 'geom_index_check.cpp'),
                        '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) > 5000
    seen = set()
    for typ, dt in (('f32', np.float32), ('f64', np.float64)):
        for mode in gc.MODES:
            for size in (1, 2, 5, 8):
                sel = [w for w in rows if w[0] == typ and int(w[1]) == gc.MODE_IDS[mode] and int(w[2]) == size]
                p = np.array([float.fromhex(w[3]) if w[3] not in ('inf', '-inf', 'nan', '-nan') else float(w[3]) for w in sel])
                assert len(p) == 17 + 72 * size + 1
                i0, w0, w1, in0, in1 = gc.axis(p, size, mode, dt)
                got_i0 = np.array([int(w[4]) for w in sel])
                got_w0, got_w1 = (np.array([float.fromhex(w[k]) for w in sel]) for k in (5, 6))
                got_in0, got_in1 = (np.array([bool(int(w[k])) for w in sel]) for k in (7, 8))
                key = (typ, mode, size)
                assert np.array_equal(got_in0, in0) and np.array_equal(got_in1, in1), key
                used = in0 | in1
                assert np.array_equal(got_i0[used], i0[used]) and not got_i0[~used].any(), key
                assert np.array_equal(got_w0, w0.astype(np.float64)) and np.array_equal(got_w1, w1.astype(np.float64)), key
                assert ((got_w0 == 0) | (got_in0 & (got_i0 >= 0) & (got_i0 < size))).all(), key
                assert ((got_w1 == 0) | (got_in1 & (got_i0 + 1 >= 0) & (got_i0 + 1 < size))).all(), key
                refused = ~(np.abs(p) <= 2.0 ** 23)
                assert refused.sum() >= 11 and not (got_in0 | got_in1)[refused].any() and not (got_w0 + got_w1)[refused].any(), key
                if mode != 'zeros':      # every accepted position has weights that sum to 1 and a lower neighbour inside
                    assert (got_w0 + got_w1)[~refused].min() == 1 and (got_w0 + got_w1)[~refused].max() == 1 and got_in0[~refused].all(), key
                seen.add(key)
    assert len(seen) == 24
