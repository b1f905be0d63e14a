"""The LPIPS distance without a GPU: the float64 restatement of tests/lpips_cases.py against the reference's own float64 run
(tests/golden/lpips.npz, written by tests/golden/make_golden_lpips.py), the host side of the new C entries (exports, the workspace
query), the op-list builders and the refusals of lpips_reference_net and of the plugin."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402

NEW_ENTRIES = ('la_feat_num_taps', 'la_feat_pair_workspace_bytes', 'la_feat_pair_distance')


@pytest.fixture(scope='module')
def gl(golden_dir):
    return np.load(os.path.join(golden_dir, 'lpips.npz'))


def _lib_loaded():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def _gray3(a, dtype):
    return torch.tensor(a).to(dtype).repeat(1, 3, 1, 1)


@pytest.mark.parametrize('tag', ['t3', 't5'])
def test_float64_restatement_reproduces_the_reference(gl, tag):
    ops = lc.cast_ops(lc.golden_ops(gl, tag), torch.float64)
    z = lambda a: lc.zscore(_gray3(a, torch.float64), gl['mean'], gl['std'])      # noqa: E731
    x, y, x1, bank = z(gl['x']), z(gl['y']), z(gl['x1']), z(gl['bank'])
    d = lc.pair_distance(ops, x, y).numpy()
    np.testing.assert_allclose(d, gl[f'{tag}_layers64'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d.sum(1), gl[f'{tag}_pair64'], rtol=1e-12, atol=0)
    xg = x1.clone().requires_grad_(True)
    tr = lc.forward_tr(ops, xg, bank)
    np.testing.assert_allclose(float(tr.detach()), float(gl[f'{tag}_tr64']), rtol=1e-12, atol=0)
    (g,) = torch.autograd.grad(tr, [xg])
    g_x = g / torch.tensor(gl['std']).double().reshape(1, 3, 1, 1)          # d/dx of the z-score
    scale = float(np.abs(gl[f'{tag}_tr_grad64']).max())
    np.testing.assert_allclose(g_x.numpy(), gl[f'{tag}_tr_grad64'], rtol=0, atol=1e-12 * scale)
    # the feature-vector form the criterion uses: squared L2 of two tap vectors is the distance
    fx, fy = lc.feature_vector(ops, x), lc.feature_vector(ops, y)
    np.testing.assert_allclose((fx - fy).square().sum(1).numpy(), gl[f'{tag}_pair64'], rtol=1e-11, atol=0)


def test_fixture_condition_and_float32_yardstick(gl):
    """The condition the maker asserts, and that the reference's float32 run is a usable yardstick (close to its float64 run)."""
    assert float(gl['min_norm']) >= 0.03
    for tag in ('t3', 't5'):
        for k in ('pair', 'layers', 'tr'):
            a64, a32 = gl[f'{tag}_{k}64'], gl[f'{tag}_{k}32']
            assert a32.dtype == np.float32 and a64.dtype == np.float64
            assert float(np.abs(a32 - a64).max()) <= 1e-5 * float(np.abs(a64).max())
    # the engine's rsqrt(sum + 1e-10) against the reference's 1 / (sqrt(sum) + 1e-10) at this condition: below float32 resolution
    ops = lc.cast_ops(lc.golden_ops(gl, 't5'), torch.float64)
    x = lc.zscore(_gray3(gl['x'], torch.float64), gl['mean'], gl['std'])
    y = lc.zscore(_gray3(gl['y'], torch.float64), gl['mean'], gl['std'])
    a, b = lc.pair_distance(ops, x, y, 'reference'), lc.pair_distance(ops, x, y, 'engine')
    assert float(((a - b).abs() / a).max()) < 2.0 ** -23


def test_header_exports_the_new_entries():
    _lib, lib = _lib_loaded()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        getattr(lib, name)
    assert _lib.SIGNATURES['la_feat_pair_workspace_bytes'][0] is C.c_size_t
    assert _lib.SIGNATURES['la_feat_num_taps'] == (C.c_int, [C.c_void_p])
    assert len(_lib.SIGNATURES['la_feat_pair_distance'][1]) == 7


def _host_handle(lib, _lib, kinds, in_ch, in_res, max_batch):
    """A tap-only engine needs no launch to create: host memory stands in for its workspace and weights."""
    desc = (_lib.FeatOp * len(kinds))(*[_lib.FeatOp(1, in_ch, in_ch) for _ in kinds])
    nbytes = lib.la_feat_workspace_bytes(len(kinds), desc, in_ch, in_res, max_batch)
    assert nbytes > 0
    ws = (C.c_char * nbytes)()
    lin = (C.c_float * in_ch)(*([1.0] * in_ch))
    params = (C.c_void_p * len(kinds))(*[C.cast(lin, C.c_void_p).value for _ in kinds])
    h = C.c_void_p()
    rc = lib.la_feat_create(len(kinds), desc, params, len(kinds), in_ch, in_res, max_batch, ws, nbytes, None, C.byref(h))
    assert rc == 0, lib.la_last_error()
    return h, (ws, lin, params)


def test_pair_workspace_query():
    _lib, lib = _lib_loaded()
    h, keep = _host_handle(lib, _lib, ['tap', 'tap'], in_ch=5, in_res=24, max_batch=16)
    try:
        assert lib.la_feat_num_taps(h) == 2
        sizes = [lib.la_feat_pair_workspace_bytes(h, P) for P in range(1, 9)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
        assert sizes[-1] >= 8 * 8 * 2 * ((24 * 24 + 63) // 64)          # [P][ntaps][tiles] float64
        assert lib.la_feat_pair_workspace_bytes(h, 9) == 0               # 2P > max_batch
        assert lib.la_feat_pair_workspace_bytes(h, 0) == 0
        assert lib.la_feat_pair_workspace_bytes(None, 1) == 0 and lib.la_feat_num_taps(None) == 0
        # refused before any launch (there is no device here): null pointers, too many pairs, a short workspace
        buf = (C.c_double * 64)()
        assert lib.la_feat_pair_distance(h, None, 1, buf, buf, 512, None) != 0
        assert lib.la_feat_pair_distance(h, buf, 9, buf, buf, 1 << 20, None) != 0
        assert b'max_batch' in lib.la_last_error()
        assert lib.la_feat_pair_distance(h, buf, 8, buf, buf, 8, None) != 0
        assert b'workspace' in lib.la_last_error()
    finally:
        lib.la_feat_destroy(h)


def test_vgg16_lpips_ops_taps(gl):
    from latentaugment_amd.synthesis import vgg16_lpips_ops
    vgg, _ = lc.golden_state_dicts(gl, 't5')
    lins = [torch.tensor(gl[f'lin{k}']) for k in range(5)]

    def same(a, b):
        return len(a) == len(b) and all(p[0] == q[0] and all(torch.equal(s, t) for s, t in zip(p[1:], q[1:])) for p, q in zip(a, b))
    assert same(vgg16_lpips_ops(vgg, lins), lc.golden_ops(gl, 't5'))                      # the default is the five-tap list
    assert same(vgg16_lpips_ops(vgg, lins, taps=(0, 1, 2, 3, 4)), lc.golden_ops(gl, 't5'))
    assert same(vgg16_lpips_ops(vgg, lins[2:], taps=(2, 3, 4)), lc.golden_ops(gl, 't3'))
    short = vgg16_lpips_ops(vgg, lins[:2], taps=(0, 1))
    assert [op[0] for op in short] == ['conv', 'conv', 'tap', 'maxpool', 'conv', 'conv', 'tap']      # ends at its last tap
    for bad_taps, bad_lins in (((2, 3, 4), lins), ((3, 2), lins[:2]), ((0, 5), lins[:2]), ((), []), ((1, 1), lins[:2])):
        with pytest.raises(ValueError):
            vgg16_lpips_ops(vgg, bad_lins, taps=bad_taps)


def test_lpips_reference_net(gl, tmp_path):
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import lpips_reference_net
    vgg, lin = lc.golden_state_dicts(gl, 't3')
    net = lpips_reference_net(vgg, lin)
    want = lc.golden_ops(gl, 't3')
    assert [op[0] for op in net.ops] == [op[0] for op in want]
    for a, b in zip(net.ops, want):
        assert all(torch.equal(s.reshape(t.shape), t) for s, t in zip(a[1:], b[1:]))
    # the z-score of networks.py:40-50 as x * scale + shift, against the buffers the reference's class held
    np.testing.assert_allclose(net.pre_scale, 1.0 / gl['std'].astype(np.float64), rtol=1e-7)
    np.testing.assert_allclose(net.pre_shift, -gl['mean'].astype(np.float64) / gl['std'].astype(np.float64), rtol=1e-7)
    # from files, read with weights_only=True
    torch.save(vgg, tmp_path / 'vgg16.pth')
    torch.save(lin, tmp_path / 'lpips_vgg.pth')
    net2 = lpips_reference_net(str(tmp_path / 'vgg16.pth'), str(tmp_path / 'lpips_vgg.pth'))
    assert all(torch.equal(s, t) for a, b in zip(net.ops, net2.ops) for s, t in zip(a[1:], b[1:]))
    with pytest.raises(FileNotFoundError):
        lpips_reference_net(str(tmp_path / 'absent.pth'), str(tmp_path / 'lpips_vgg.pth'))
    with pytest.raises(FileNotFoundError):
        lpips_reference_net(str(tmp_path / 'vgg16.pth'), str(tmp_path / 'absent.pth'))
    neg = dict(lin)
    neg['lin3.model.1.weight'] = lin['lin3.model.1.weight'].clone()
    neg['lin3.model.1.weight'][0, 1] = -1e-3
    with pytest.raises(_lib.LatentAugHipError, match='negative'):
        lpips_reference_net(vgg, neg)
    neg01 = dict(lin)
    neg01['lin0.model.1.weight'] = -lin['lin0.model.1.weight']          # not among the three that are used
    lpips_reference_net(vgg, neg01)
    with pytest.raises(_lib.LatentAugHipError, match='need at least 3'):
        lpips_reference_net(vgg, {k: v for k, v in lin.items() if k[3] in '01'})


def test_plugin_raises_without_the_weight_files(tmp_path):
    """opt.lpips_script = 'lpips' with neither opt.lpips_vgg_path / lpips_lin_path nor <model_dir>/vgg16.pth + lpips_vgg.pth: the
    NotImplementedError of the TorchScript branch, before anything touches a device; one file of the two is not enough."""
    from latentaugment_amd.latent_aug import LatentAug
    torch.save({}, tmp_path / 'vgg16.pth')
    for extra in (dict(), dict(model_dir=str(tmp_path)), dict(lpips_vgg_path=str(tmp_path / 'vgg16.pth'), lpips_lin_path=str(tmp_path / 'no.pth'))):
        opt = types.SimpleNamespace(img_resolution=32, batch_size=1, modalities_aug='A,B', opt_num_epochs=1, opt_lr=0.01, truncation_psi=1.0,
                                    w_pix=0.0, w_lpips=1.0, w_latent=0.0, w_disc=0.0, crop_size_aug=16, preprocess_aug='center_random_crop',
                                    soft_aug=False, alpha=1.0, verbose_log=False, lpips_script='lpips', **extra)
        with pytest.raises(NotImplementedError, match='lpips_vgg_path'):
            LatentAug('train', opt, str(tmp_path), [0], generator=object())
