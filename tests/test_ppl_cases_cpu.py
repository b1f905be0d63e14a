"""Perceptual path length without a GPU: the restatements of tests/ppl_cases.py against their definitions, ppl_from_distances against
np.percentile, the host side of la_path_points_f32 (declared, bound, exported, every bad argument refused before a launch) and the
refusals of the wrappers that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppl_cases as pc  # noqa: E402


def _lib_loaded():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def test_lerp_restatement():
    rs = np.random.RandomState(0)
    a, b = rs.randn(3, 5).astype(np.float32), rs.randn(3, 5).astype(np.float32)
    t = np.array([0.0, 0.25, 1.0], np.float32)
    p = pc.lerp_points(a, b, t, [0.0, 1.0, -0.5, 1e-4], reps=2)
    assert p.shape == (4, 3, 2, 5) and p.dtype == np.float64
    assert np.array_equal(p[:, :, 0], p[:, :, 1])
    assert np.array_equal(p[0, 0, 0], a[0].astype(np.float64))                          # t = 0
    assert np.array_equal(p[1, 0, 0], b[0].astype(np.float64))                          # t + dt = 1: a + (b - a) is b up to one rounding
    np.testing.assert_allclose(p[2, 2, 0], 0.5 * (a[2].astype(np.float64) + b[2]), rtol=0, atol=1e-15)      # 1 - 0.5
    # t + dt is formed in double: 0.25f + 1e-4 in float32 would be off by 1e-9
    step = p[3, 1, 0] - p[0, 1, 0]
    np.testing.assert_allclose(step, 1e-4 * (b[1].astype(np.float64) - a[1]), rtol=1e-10, atol=1e-18)


def test_slerp_restatement():
    rs = np.random.RandomState(1)
    a, b = rs.randn(4, 16).astype(np.float32), (5.0 * rs.randn(4, 16)).astype(np.float32)
    t = np.array([0.0, 0.3, 0.7, 1.0], np.float32)
    dt = [0.0, 1.0, 0.5, -0.2]
    p = pc.slerp_points(a, b, t, dt)[:, :, 0]
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)      # noqa: E731
    au, bu = unit(a.astype(np.float64)), unit(b.astype(np.float64))
    np.testing.assert_allclose(np.linalg.norm(p, axis=-1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(p[0, 0], au[0], rtol=0, atol=1e-15)          # s = 0
    np.testing.assert_allclose(p[1, 0], bu[0], rtol=0, atol=1e-14)          # s = 1: the other end, whatever the norms
    # constant angular speed: the angle from a' to the point is s * omega, also outside [0, 1]
    omega = np.arccos(np.clip((au * bu).sum(1), -1, 1))
    for k in range(4):
        s = t.astype(np.float64) + dt[k]
        ang = np.arccos(np.clip((p[k] * au).sum(1), -1, 1))
        np.testing.assert_allclose(ang, np.abs(s) * omega, rtol=0, atol=1e-7)
    # the degenerate rule: identical and opposite directions give the normalised a at every parameter
    for sign in (1.0, -1.0):
        for D in pc.KERNEL_D:
            ea, eb = pc.exact_rows(D, sign)
            q = pc.slerp_points(ea, eb, np.array([0.0, 0.6], np.float32), [0.0, 0.5, 1.3])[:, :, 0]
            assert np.isfinite(q).all()
            assert np.array_equal(q, np.broadcast_to(unit(ea.astype(np.float64)), q.shape)), (sign, D)


def _inputs():
    rs = np.random.RandomState(5)
    ties = np.concatenate([np.full(40, 2.0), np.full(40, 3.0), np.full(20, 1.0), [0.5, 9.0]])
    return {'n100': rs.rand(100), 'n101': rs.rand(101) * 7, 'n3': np.array([3.0, 1.0, 2.0]), 'ties': ties, 'all equal': np.full(17, 4.0),
            'n1': np.array([2.5]), 'n1000': rs.standard_exponential(1000)}


@pytest.mark.parametrize('name', sorted(_inputs()))
def test_ppl_from_distances_is_the_percentile_filter(name):
    from latentaugment_amd import metrics
    d = _inputs()[name]
    lo, hi = pc.percentile(d, 1, 'lower'), pc.percentile(d, 99, 'higher')
    want = d[(d >= lo) & (d <= hi)].mean()
    got = metrics.ppl_from_distances(d)
    assert isinstance(got, float) and got == want == pc.ppl_filter(d), (name, got, want)
    assert metrics.ppl_from_distances(torch.from_numpy(d)) == want          # tensors too
    assert metrics.ppl_from_distances(d[::-1].astype(np.float32)) == pc.ppl_filter(d.astype(np.float32))


def test_ppl_from_distances_cuts_the_tails():
    from latentaugment_amd import metrics
    d = np.arange(101, dtype=np.float64)                       # 1st percentile 1, 99th 99: 0 and 100 leave
    assert metrics.ppl_from_distances(d) == 50.0
    d[100] = 1e9
    assert metrics.ppl_from_distances(d) == 50.0
    assert metrics.ppl_from_distances(np.array([1.0, 2.0, 6.0])) == 3.0          # 3 elements: lower -> the min, higher -> the max
    for bad in (np.zeros([0]), np.zeros([2, 2])):
        with pytest.raises(ValueError):
            metrics.ppl_from_distances(bad)


def test_header_declares_binds_and_exports_the_entry():
    _lib, lib = _lib_loaded()
    with open(_lib.HEADER_PATH) as f:
        assert 'int la_path_points_f32(' in f.read()
    res, args = _lib.SIGNATURES['la_path_points_f32']
    assert res is C.c_int
    assert args == [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]
    fn = getattr(lib, 'la_path_points_f32')
    assert fn.argtypes == args and fn.restype is C.c_int


def test_bad_arguments_are_refused_before_any_launch():
    """There is no device here: a call that got as far as a launch would fail with the HIP error, not LA_ERR_ARG."""
    _lib, lib = _lib_loaded()
    f = (C.c_float * 64)()
    dt = (C.c_double * 64)()
    good = dict(a=f, b=f, t=f, dt=dt, T=2, N=1, D=4, reps=1, mode=0, out=f)

    def call(**kw):
        g = dict(good, **kw)
        return lib.la_path_points_f32(g['a'], g['b'], g['t'], g['dt'], g['T'], g['N'], g['D'], g['reps'], g['mode'], g['out'], None)
    for bad in (dict(a=None), dict(b=None), dict(t=None), dict(dt=None), dict(out=None)):
        assert call(**bad) == -1, bad
        assert b'null' in lib.la_last_error()
    for bad in (dict(N=0), dict(N=-3), dict(D=0), dict(D=-1), dict(reps=0), dict(reps=-2)):
        assert call(**bad) == -1, bad
        assert b'at least 1' in lib.la_last_error()
    for bad in (dict(T=0), dict(T=-1), dict(T=65)):
        assert call(**bad) == -1, bad
        assert b'1 .. 64' in lib.la_last_error()
    for bad in (dict(mode=-1), dict(mode=2)):
        assert call(**bad) == -1, bad
        assert b'mode' in lib.la_last_error()


class _FakeNet:
    """Stands where a FeatureEngine would: the refusals under test come before anything reads more of it."""
    in_ch, in_res, max_batch, num_taps = 3, 32, 8, 1
    pre_scale, pre_shift = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)

    def __init__(self, device):
        self.device = torch.device(device)

    def pair_rows(self):
        return self.max_batch // 2

    def pair_distance_rows(self, xy, P, dist):
        raise AssertionError('not reached')


class _FakeSynth:
    num_ws, w_dim, img_channels, img_resolution = 8, 32, 2, 32

    def __init__(self, device, max_batch=8):
        self.device, self.max_batch = torch.device(device), max_batch


def test_wrappers_refuse_without_a_device():
    from latentaugment_amd import _lib, metrics
    w = torch.zeros([2, 32])
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        metrics.compute_path_length(None, None, w, w)
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        metrics.compute_path_length(None, None, w.numpy(), w.numpy())
    with pytest.raises(_lib.LatentAugHipError, match='MappingEngine'):
        metrics.compute_ppl(object(), None, None, 4)
    with pytest.raises(ValueError):
        metrics.compute_ppl(object(), None, None, 4, space='x')
    with pytest.raises(ValueError):
        metrics.compute_ppl(object(), None, None, 4, sampling='middle')
    with pytest.raises(ValueError):
        metrics.compute_ppl(object(), None, None, 0)
    with pytest.raises(ValueError):
        metrics.compute_ppl(object(), None, None, 4, epsilon=0.0)
    synth, net = _FakeSynth('cuda:0'), _FakeNet('cuda:0')
    # a net on another device, a generator of batch 1, a resolution the net's does not divide, a net that is no engine
    with pytest.raises(ValueError, match='cuda:1'):
        metrics._path_engines(synth, _FakeNet('cuda:1'), 'x')
    with pytest.raises(_lib.LatentAugHipError, match='max_batch = 1'):
        metrics._path_engines(_FakeSynth('cuda:0', max_batch=1), net, 'x')
    odd = _FakeNet('cuda:0')
    odd.in_res = 24
    with pytest.raises(ValueError, match='24'):
        metrics._path_engines(synth, odd, 'x')
    with pytest.raises(_lib.LatentAugHipError, match='FeatureEngine'):
        metrics._path_engines(synth, object(), 'x')
    assert metrics._path_engines(synth, net, 'x') == 4
    with pytest.raises(FileNotFoundError):
        metrics.compute_path_length_for_aug_dataset(os.path.join(os.path.dirname(__file__), 'no_such_run'), synth, net)


def test_draws_do_not_depend_on_the_sampling_of_t():
    z0, z1, t = pc.draws(8, 32, 0, 'full')
    e0, e1, te = pc.draws(8, 32, 0, 'end')
    assert torch.equal(z0, e0) and torch.equal(z1, e1) and float(te.abs().max()) == 0.0 and 0.0 <= float(t.min()) and float(t.max()) < 1.0
    assert not torch.equal(z0, z1)
