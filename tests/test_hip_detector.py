"""The detector path on the GPU: image preparation (la_detector_prep_f32), the fully connected kernel (la_fc_bias_act_f32), detector op
lists of the feature engine, the TorchScript loader (DetectorEngine.from_torchscript) and the image -> FeatureStats -> metrics
pipeline, against the float64 restatements of tests/detector_cases.py.

EXACT: the quantisation on the bin-edge set (every byte torch's), area resampling of small integers where the bin size is a power of
two, the FC kernel on small integers (|sum| < 2^24, every shape, and fc1's real size), two runs of anything.
BOUNDED: float inputs, worst |hip - f64| <= K x worst |f32-CPU - f64| + 2^-23 x max|f64| with K = 4 (f32), 6.7 (bf16x3), 4.2 (f16x2)
as in test_hip_engine_shapes.py, and for features never beyond its ceiling 1e-4 |ref| + 1e-5 max|ref|.  The float32 CPU run of the
restatement sets every budget; the code under test sets none.  Every case prints err / budget.
"""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_cases as dc  # noqa: E402
import helpers_script_detector as hsd  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3
ACT_LINEAR, ACT_RELU = 1, 2
MODES = ['f32', 'bf16x3', 'f16x2']
K = {'f32': 4.0, 'bf16x3': 6.7, 'f16x2': 4.2}
FEAT_CEIL = (1e-4, 1e-5)          # (rtol, atol x max|ref|)


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


def _err_text(lib):
    m = lib.la_last_error()
    return m.decode() if m else ''


def _judge(name, got, r32, r64, k=4.0, ceil=None):
    got = got.detach().cpu().double()
    err, bud = dc.worst(got, r64), dc.budget(r32, r64, k)
    print(f'{name}: err {err:.3e} / budget {bud:.3e} = ratio {err / bud if bud > 0 else float(err > 0):.3f}')
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    if ceil is not None:
        over = (got - r64).abs() - (ceil[0] * r64.abs() + ceil[1] * float(r64.abs().max()))
        assert float(over.max()) <= 0, f'{name}: beyond the feature ceiling by {float(over.max()):.3e}'
    assert err <= bud, f'{name}: err {err:.3e} > budget {bud:.3e}'


def _unaligned(t, dev):
    """a device copy whose base pointer is 4 bytes past a 16-byte boundary"""
    buf = torch.empty([t.numel() + 1], dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# image preparation

@pytest.mark.parametrize('Cc', dc.PREP_CHANNELS)
@pytest.mark.parametrize('mode', dc.PREP_MODES)
@pytest.mark.parametrize('H,W,S', dc.PREP_SIZES)
def test_prep_float_inputs(dev, H, W, S, mode, Cc):
    from latentaugment_amd.synthesis import detector_prep
    img = dc.prep_inputs(Cc, H, W)
    for quantize in (False, True):
        r64 = dc.prep_restate(img, S, mode, quantize, dc.PREP_SCALE, dc.PREP_SHIFT, torch.float64)
        r32 = dc.prep_restate(img, S, mode, quantize, dc.PREP_SCALE, dc.PREP_SHIFT, torch.float32)
        got = detector_prep(_unaligned(img, dev), S, mode, quantize, dc.PREP_SCALE, dc.PREP_SHIFT)
        torch.cuda.synchronize()
        assert got.shape == (dc.PREP_N, 3, S, S)
        _judge(f'prep {H}x{W}->{S} {mode} C{Cc} quantize={quantize}', got, r32, r64)


def test_prep_quantisation_is_torchs_uint8_on_the_bin_edges(dev):
    from latentaugment_amd.synthesis import detector_prep
    x = dc.bin_edge_inputs()
    img = torch.zeros([3 * 16 * 16])
    img[:x.numel()] = x
    img = img.reshape(3, 1, 16, 16)
    want = dc.quant_torch(img.repeat(1, 3, 1, 1))
    for mode in dc.PREP_MODES:          # H == W == S: a copy in either mode, nothing is averaged
        got = detector_prep(img.to(dev), 16, mode, True).cpu()
        bad = (got != want.float()).nonzero()
        assert bad.numel() == 0, f'{len(bad)} of {want.numel()} bytes differ from torch, first at {bad[0].tolist()}'
        assert torch.equal(got.to(torch.uint8), want)


@pytest.mark.parametrize('Cc', dc.PREP_CHANNELS)
@pytest.mark.parametrize('H,W,S', [s for s in dc.PREP_SIZES if s[0] != s[2]])
def test_prep_area_of_small_integers_is_exact_on_power_of_two_bins(dev, H, W, S, Cc):
    from latentaugment_amd.synthesis import detector_prep
    img = dc.prep_inputs(Cc, H, W, integers=True)
    r64 = dc.prep_restate(img, S, 'area', False, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    got = detector_prep(img.to(dev), S, 'area', False).cpu()
    mask = dc.area_pow2_mask(H, W, S)          # (6 x 10 -> 4 has bins of 2 x 3 only: nothing to compare exactly there)
    assert bool(mask.any()) or (H, W, S) == (6, 10, 4)
    assert torch.equal(got[:, :, mask].double(), r64[:, :, mask]), 'area sums over power-of-two bins must be exact'
    r32 = dc.prep_restate(img, S, 'area', False, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), torch.float32)
    _judge(f'prep-int {H}x{W}->{S} C{Cc}', got, r32, r64)


def test_prep_refuses_bad_arguments(lib, dev):
    img = torch.zeros([2, 1, 8, 8], device=dev)
    out = torch.full([2, 3, 4, 4], 7.0, device=dev)
    sc, sh = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
    for args, text in [((_p(img), _p(out), 2, 2, 8, 8, 4, 1, 0, 0, sc, sh), 'channels * rep must be 3'),
                       ((_p(img), _p(out), 2, 1, 8, 8, 4, 3, 2, 0, sc, sh), 'mode must be'),
                       ((None, _p(out), 2, 1, 8, 8, 4, 3, 0, 0, sc, sh), 'null pointer'),
                       ((_p(img), _p(out), 2, 1, 8, 0, 4, 3, 0, 0, sc, sh), 'sizes must lie')]:
        assert lib.la_detector_prep_f32(*args, _s()) == LA_ERR_ARG and text in _err_text(lib), _err_text(lib)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# fully connected kernel

def _fc(lib, dev, x, w, b, relu, ws=None):
    N, Kk = x.shape
    O = w.shape[0]
    y = torch.empty([N, O], dtype=torch.float32, device=dev)
    if ws is None:
        ws = torch.empty([lib.la_fc_workspace_bytes(N, Kk, O)], dtype=torch.uint8, device=dev)
    rc = lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, Kk, O, ACT_RELU if relu else ACT_LINEAR, _p(ws), ws.numel(), _s())
    assert rc == 0, _err_text(lib)
    return y


@pytest.mark.parametrize('N,Kk,O', dc.FC_SHAPES, ids=[f'N{n}-K{k}-O{o}' for n, k, o in dc.FC_SHAPES])
def test_fc_shapes(lib, dev, N, Kk, O):
    assert lib.la_fc_workspace_bytes(N, Kk, O) == dc.fc_workspace_bytes(N, Kk, O)
    xi, wi, bi = dc.fc_inputs(N, Kk, O, integers=True)
    x, w, b = dc.fc_inputs(N, Kk, O)
    for relu in (False, True):
        got = _fc(lib, dev, xi.to(dev), wi.to(dev), bi.to(dev), relu).cpu()
        want = dc.fc_restate(xi, wi, bi, relu)
        bad = (got.double() != want).nonzero()
        assert bad.numel() == 0, f'integers, relu={relu}: {len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}'
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
        g1, g2 = _fc(lib, dev, xd, wd, bd, relu), _fc(lib, dev, xd, wd, bd, relu)
        assert torch.equal(g1, g2), 'two runs differ'
        _judge(f'fc N{N} K{Kk} O{O} relu={relu} plan={dc.fc_plan(N, Kk, O)["ks"]} slices', g1,
               dc.fc_restate(x, w, b, relu, torch.float32), dc.fc_restate(x, w, b, relu))


def test_fc_unaligned_operands_take_the_scalar_loads(lib, dev):
    N, Kk, O = 33, 100, 130
    xi, wi, bi = dc.fc_inputs(N, Kk, O, integers=True)
    got = _fc(lib, dev, _unaligned(xi, dev), _unaligned(wi, dev), bi.to(dev), True).cpu()
    assert torch.equal(got.double(), dc.fc_restate(xi, wi, bi, True))


def test_fc_smaller_batch_on_the_same_workspace(lib, dev):
    t = dc.FC_SHRINK
    ws = torch.empty([lib.la_fc_workspace_bytes(t['N_first'], t['K'], t['O'])], dtype=torch.uint8, device=dev)
    x, w, b = dc.fc_inputs(t['N_first'], t['K'], t['O'])
    big = _fc(lib, dev, (x * 256).to(dev), w.to(dev), b.to(dev), False, ws)
    assert bool(torch.isfinite(big).all())
    xs = x[:t['N_then']].contiguous()
    used = _fc(lib, dev, xs.to(dev), w.to(dev), b.to(dev), False, ws)
    fresh = _fc(lib, dev, xs.to(dev), w.to(dev), b.to(dev), False)
    assert torch.equal(used, fresh)
    _judge('fc shrinking batch', used, dc.fc_restate(xs, w, b, False, torch.float32), dc.fc_restate(xs, w, b, False))


def test_fc_real_size_small_integers_bit_for_bit(lib, dev):
    t = dc.FC_REAL
    x, w, b = dc.fc_inputs(t['N'], t['K'], t['O'], integers=True)
    want = dc.fc_restate(x, w, b, False)
    got = _fc(lib, dev, x.to(dev), w.to(dev), b.to(dev), False).cpu()
    bad = (got.double() != want).nonzero()
    assert bad.numel() == 0, f'{len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}'
    assert torch.equal(_fc(lib, dev, x.to(dev), w.to(dev), b.to(dev), True).cpu().double(), want.clamp_min(0))


def test_fc_misuse_fails_before_any_launch(lib, dev):
    N, Kk, O = 5, 1568, 130
    x, w, b = (t.to(dev) for t in dc.fc_inputs(N, Kk, O))
    y = torch.full([N, O], 7.0, device=dev)
    need = lib.la_fc_workspace_bytes(N, Kk, O)
    ws = torch.empty([need], dtype=torch.uint8, device=dev)
    assert lib.la_fc_bias_act_f32(None, _p(w), _p(b), _p(y), N, Kk, O, ACT_RELU, _p(ws), need, _s()) == LA_ERR_ARG
    assert 'null pointer' in _err_text(lib)
    assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, Kk, O, ACT_RELU, None, need, _s()) == LA_ERR_ARG
    assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, Kk, O, ACT_RELU, _p(ws), need - 1, _s()) == LA_ERR_WORKSPACE
    assert 'workspace too small' in _err_text(lib)
    assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, Kk, 0, ACT_RELU, _p(ws), need, _s()) == LA_ERR_ARG
    assert 'at least 1' in _err_text(lib)
    assert lib.la_fc_workspace_bytes(N, Kk, 0) == 0 and lib.la_fc_workspace_bytes(0, Kk, O) == 0
    assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, Kk, O, 3, _p(ws), need, _s()) == LA_ERR_ARG
    assert 'linear or relu' in _err_text(lib)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())          # nothing was written
    got = _fc(lib, dev, x, w, b, True, ws)          # and the device is still usable
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# detector lists on the feature engine

_REFS = {}


def _det_ref(case):
    if case.name not in _REFS:
        ops, x = case.build()
        _REFS[case.name] = (ops, x, dc.detector_restate(ops, x, torch.float32), dc.detector_restate(ops, x, torch.float64))
    return _REFS[case.name]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', dc.DET_CASES, ids=[c.name for c in dc.DET_CASES])
def test_detector_list_sweep(dev, case, mode):
    from latentaugment_amd.synthesis import FeatureEngine
    ops, x, r32, r64 = _det_ref(case)
    eng = FeatureEngine(ops, dev, in_res=case.res, max_batch=case.max_batch, in_ch=case.in_ch, precision=mode)
    assert eng.num_features == case.fcs[-1]
    f1 = eng.forward(x.to(dev))
    f2 = eng.forward(x.to(dev))
    torch.cuda.synchronize()
    assert f1.shape == r64.shape and torch.equal(f1, f2)
    _judge(f'detector {case.name} [{mode}]', f1, r32, r64, K[mode], FEAT_CEIL)


def test_detector_list_refuses_backward(lib, dev):
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import FeatureEngine
    case = dc.DET_CASES[0]
    ops, x, _, _ = _det_ref(case)
    eng = FeatureEngine(ops, dev, in_res=case.res, max_batch=case.max_batch, in_ch=case.in_ch)
    eng.forward(x.to(dev))
    gx = torch.full_like(x, 7.0).to(dev)
    gf = torch.ones([case.N, eng.num_features], device=dev)
    rc = lib.la_feat_backward(eng.handle, _p(gf), _p(gx), _s())
    torch.cuda.synchronize()
    assert rc == LA_ERR_ARG and 'forward only' in _err_text(lib), _err_text(lib)
    assert bool((gx == 7.0).all())
    with pytest.raises(_lib.LatentAugHipError, match='forward only'):
        eng.backward(gf)


@pytest.mark.parametrize('name,ops,in_ch,res,text', dc.DET_REFUSALS, ids=[r[0] for r in dc.DET_REFUSALS])
def test_detector_list_refusals_at_create(lib, dev, name, ops, in_ch, res, text):
    from latentaugment_amd import _lib
    arr = (_lib.FeatOp * len(ops))(*[_lib.FeatOp(*o) for o in ops])
    assert lib.la_feat_workspace_bytes(len(ops), arr, in_ch, res, 2) == 0
    assert text in _err_text(lib), _err_text(lib)
    buf = torch.zeros([1 << 16], dtype=torch.float32, device=dev)
    params = (C.c_void_p * 8)(*[buf.data_ptr()] * 8)
    h = C.c_void_p()
    rc = lib.la_feat_create(len(ops), arr, params, 8, in_ch, res, 2, _p(buf), buf.numel() * 4, _s(), C.byref(h))
    assert rc == LA_ERR_ARG and not h.value and text in _err_text(lib), _err_text(lib)


# ---------------------------------------------------------------------------------------------------------------------------------
# loader

def _images(n_batches, seed=0, n=4):
    g = torch.Generator().manual_seed(400 + seed)
    return [torch.rand([n, 1, 40, 40], generator=g) * 2 - 1 for _ in range(n_batches)]


def _feature_check(name, got, want):
    got, want = got.detach().cpu().double(), want.double()
    over = (got - want).abs() - (FEAT_CEIL[0] * want.abs() + FEAT_CEIL[1] * float(want.abs().max()))
    print(f'{name}: worst |hip - script| {float((got - want).abs().max()):.3e}, max|script| {float(want.abs().max()):.3e}, '
          f'over the ceiling by {float(over.max()):.3e}')
    assert got.shape == want.shape and float(over.max()) <= 0


@pytest.mark.parametrize('after', [1, 2])
@pytest.mark.parametrize('resize', ['area', 'bilinear'])
def test_loader_picks_the_variant_that_was_built(dev, tmp_path, resize, after):
    from latentaugment_amd.synthesis import DetectorEngine
    path = tmp_path / 'det.pt'
    module = hsd.save_scripted_detector(path, resize=resize, features_after=after)
    det = DetectorEngine.from_torchscript(str(path), dev, max_batch=4)
    assert det.S == 32 and det.resize_mode == resize and det.fc_depth == after
    assert det.num_features == (40, 24)[after - 1] and len(det.weights_digest) == 10
    x = _images(1, seed=after)[0]
    _feature_check(f'loader {resize} after fc{after}', det.features(x.to(dev)), hsd.reference_side_features(module, x))


def test_loader_refuses_a_module_no_candidate_reproduces(dev, tmp_path):
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import DetectorEngine
    path = tmp_path / 'det.pt'
    hsd.save_scripted_detector(path, features_after=3)          # return_features gives fc3's raw logits
    with pytest.raises(_lib.LatentAugHipError, match='refusing to guess') as e:
        DetectorEngine.from_torchscript(str(path), dev, max_batch=4)
    assert "'area'" in str(e.value) and "'bilinear'" in str(e.value) and 'inf' in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# pipeline

@pytest.fixture(scope='module')
def detector(dev, tmp_path_factory):
    from latentaugment_amd.synthesis import DetectorEngine
    path = tmp_path_factory.mktemp('det') / 'det.pt'
    module = hsd.save_scripted_detector(path)
    return DetectorEngine.from_torchscript(str(path), dev, max_batch=4), module


def test_pipeline_feature_stats_rows_are_the_scripted_modules(detector, tmp_path):
    from latentaugment_amd import metrics
    det, module = detector
    batches = _images(3)
    stats = metrics.compute_feature_stats_for_images(batches, det, capture_all=True, capture_mean_cov=True)
    want = torch.cat([hsd.reference_side_features(module, b) for b in batches])
    assert stats.num_items == 12 and stats.num_features == det.num_features
    _feature_check('pipeline rows', torch.from_numpy(stats.get_all()), want)
    mean, cov = stats.get_mean_cov()
    np.testing.assert_allclose(mean, want.double().mean(0).numpy(), rtol=1e-4, atol=1e-5 * float(want.abs().max()))
    assert cov.shape == (det.num_features, det.num_features)
    cut = metrics.compute_feature_stats_for_images(batches, det, max_items=10, capture_all=True)
    assert cut.num_items == 10 and np.array_equal(cut.get_all(), stats.get_all()[:10])
    stats.save(str(tmp_path / 'stats.pkl'))
    back = metrics.FeatureStats.load(str(tmp_path / 'stats.pkl'))
    assert back.num_items == 12 and np.array_equal(back.get_all(), stats.get_all())
    np.testing.assert_array_equal(back.raw_mean, stats.raw_mean)
    np.testing.assert_array_equal(back.raw_cov, stats.raw_cov)


def test_pipeline_dict_batches_read_their_mode(detector):
    from latentaugment_amd import metrics
    det, _ = detector
    a, b = _images(2, seed=1), _images(2, seed=2)
    dicts = [{'A': x, 'B': y} for x, y in zip(a, b)]
    fa = metrics.compute_feature_stats_for_images(dicts, det, mode='A', capture_all=True).get_all()
    fb = metrics.compute_feature_stats_for_images(dicts, det, mode='B', capture_all=True).get_all()
    assert np.array_equal(fa, metrics.compute_feature_stats_for_images(a, det, capture_all=True).get_all())
    assert np.array_equal(fb, metrics.compute_feature_stats_for_images(b, det, capture_all=True).get_all())
    assert not np.array_equal(fa, fb)
    with pytest.raises(ValueError, match='mode'):
        metrics.compute_feature_stats_for_images(dicts, det, capture_all=True)


class _Callable:
    def __reduce__(self):
        return (os.getcwd, ())


def test_pipeline_directory_reader(detector, tmp_path):
    from latentaugment_amd import metrics
    det, _ = detector
    a, b = _images(2, seed=3), _images(2, seed=4)
    os.makedirs(tmp_path / 'run' / 'img_aug')
    for i, (x, y) in enumerate(zip(a, b)):          # as the reference's driver writes them: one dict of batches per file
        with open(tmp_path / 'run' / 'img_aug' / f'img_aug_{i}', 'wb') as f:
            pickle.dump({'A': x, 'B': y}, f, protocol=pickle.HIGHEST_PROTOCOL)
    cache = str(tmp_path / 'cache' / 'stats.pkl')
    got = metrics.compute_feature_stats_for_aug_dataset(str(tmp_path / 'run'), 'B', det, cache_file=cache, capture_all=True)
    assert np.array_equal(got.get_all(), metrics.compute_feature_stats_for_images(b, det, capture_all=True).get_all())
    assert os.path.isfile(cache)
    again = metrics.compute_feature_stats_for_aug_dataset(str(tmp_path / 'nowhere'), 'B', det, cache_file=cache, capture_all=True)
    assert np.array_equal(again.get_all(), got.get_all())
    assert metrics.compute_feature_stats_for_aug_dataset(str(tmp_path / 'run'), 'A', det, max_items=5, capture_all=True).num_items == 5
    os.makedirs(tmp_path / 'bad' / 'img_aug')
    with open(tmp_path / 'bad' / 'img_aug' / 'img_aug_0', 'wb') as f:
        pickle.dump({'A': a[0], 'B': _Callable()}, f, protocol=pickle.HIGHEST_PROTOCOL)
    with pytest.raises(pickle.UnpicklingError, match='allow-list'):
        metrics.compute_feature_stats_for_aug_dataset(str(tmp_path / 'bad'), 'A', det, capture_all=True)


def test_pipeline_metrics_of_a_set_against_itself(detector):
    from latentaugment_amd import metrics
    det, _ = detector
    real = _images(3, seed=5)
    out = metrics.compute_metrics_from_images(real, real, det, nhood_size=3)
    assert set(out) == {'precision', 'recall', 'density', 'coverage', 'kid'}
    assert out['precision'] == 1.0 and out['recall'] == 1.0 and out['coverage'] == 1.0
    assert np.isfinite(out['density']) and np.isfinite(out['kid'])
