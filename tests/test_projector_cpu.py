"""The projector without a GPU: the schedule against its definition, the hand-written gradients of tests/projector_cases.py against
torch autograd in float64, the latent-zip writer read back by LatentCodeDataset, the refusals that come before any launch, and the
host side of the new entries (declared, bound, exported)."""
import ctypes as C
import math
import os
import pickle
import sys
import zipfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projector_cases as pj  # noqa: E402

ENTRIES = ('la_row_dist_workspace_bytes', 'la_row_dist_f32', 'la_box_down_f32', 'la_box_up_f32', 'la_proj_step_tail_f32')


def _lib_loaded():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def test_schedule_values():
    from latentaugment_amd import projector
    T, w_std = 1000, 2.5
    for t in range(T + 1):
        lr, sigma = projector.schedule(t, T, w_std)
        lr_r, sigma_r = pj.schedule(t, T, w_std)
        assert lr == pytest.approx(lr_r, rel=1e-15, abs=1e-18) and sigma == pytest.approx(sigma_r, rel=1e-15, abs=1e-18)
        tau = t / T
        if t == 0:
            assert lr == 0.0 and sigma == w_std * 0.05
        if 0.05 <= tau <= 0.75:
            assert lr == 0.1, (t, lr)
        if tau < 0.05:
            assert lr == pytest.approx(0.1 * tau / 0.05, rel=1e-12)
        if tau > 0.75:
            assert 0.0 <= lr < 0.1
        if tau >= 0.75:
            assert sigma == 0.0, (t, sigma)
        else:
            assert sigma > 0.0
    assert projector.schedule(T - 1, T, w_std)[0] < 0.1 * 1e-3 and projector.schedule(T, T, w_std)[0] == 0.0      # lr -> 0 at the end
    lrs = [projector.schedule(t, T, w_std)[0] for t in range(750, T + 1)]
    assert all(a > b for a, b in zip(lrs, lrs[1:]))
    # the keywords
    lr, sigma = projector.schedule(10, 100, 1.0, initial_lr=0.2, initial_noise_factor=0.1, lr_rampup_length=0.2, noise_ramp_length=0.5)
    assert lr == pytest.approx(0.1) and sigma == pytest.approx(0.1 * 0.8 ** 2)
    with pytest.raises(TypeError):
        projector.schedule(0, 10, 1.0, no_such_keyword=1)


@pytest.mark.parametrize('space,w_pix,k,affine', [('w', 0.0, 1, False), ('w+', 0.1, 1, False), ('w', 0.1, 2, True)])
def test_restated_gradients_agree_with_autograd(space, w_pix, k, affine):
    """d loss / d w_opt by the chain the product runs (distance gradients, preparation adjoint, W-space row sum written out) against
    autograd of the whole expression, in float64, with noise on the latent."""
    case = pj.make_case(space, w_pix, k, affine)
    tgt = pj.targets()
    B, G = tgt.shape[0], pj.generator()
    avg, std = pj.w_stats()
    g = torch.Generator().manual_seed(3)
    w = torch.from_numpy(avg).reshape(1, 1, -1) + 0.3 * torch.randn([B, case.L, G.w_dim], generator=g, dtype=torch.float64)
    n, sigma = pj.noise(B, case.L, G.w_dim, case.seed, 2), 0.05 * std
    loss, dws, _ = pj.terms(case, w + sigma * n, tgt, torch.float64)
    gw = dws.sum(1, keepdim=True) if space == 'w' else dws
    loss_a, gw_a = pj.autograd_terms(case, w, sigma, n, tgt)
    assert float(loss[:, 0].min()) > 1e-3 and (w_pix == 0.0 or float(loss[:, 1].min()) > 1e-6)
    np.testing.assert_allclose(loss.numpy(), loss_a.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(gw.numpy(), gw_a.numpy(), rtol=1e-9, atol=1e-11 * float(gw_a.abs().max()))
    assert float(gw_a.abs().max()) > 1e-6


@pytest.mark.parametrize('key', pj.STEP_CASES)
def test_recorded_step_seeds_keep_the_compared_points_off_the_kinks(key):
    """STEP_SEEDS of projector_cases.py: at the recorded seed no pre-activation of the float64 run lies within KINK_MARGIN of its kink at
    any step the teacher-forced GPU test compares (`python tests/projector_cases.py` repeats the search from seed 0)."""
    margins = pj.point_margins(pj.make_case(*key))
    assert [t for t, _, _ in margins] == list(pj.STEP_POINTS)
    assert all(m >= pj.KINK_MARGIN for _, m, _ in margins), margins


def test_box_restatement_is_an_adjoint_pair_and_exact_on_integers():
    rs = np.random.RandomState(0)
    for R, k in ((8, 1), (8, 2), (24, 4), (16, 8)):
        x = torch.from_numpy(rs.randint(-8, 9, (3, R, R)).astype(np.float64))
        y = torch.from_numpy(rs.randint(-8, 9, (3, R // k, R // k)).astype(np.float64))
        d = pj.box_down(x, k)
        assert torch.equal(d, torch.nn.functional.avg_pool2d(x[None], k)[0]) if k > 1 else torch.equal(d, x)
        assert float((d * y).sum()) == float((x * pj.box_up(y, k)).sum())


def test_adam_restatement_against_torch_optim():
    g = torch.Generator().manual_seed(0)
    w = torch.randn([2, 1, 8], generator=g, dtype=torch.float64)
    p = w.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], betas=(pj.B1, pj.B2), eps=pj.EPS, lr=0.1)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    for step in range(1, 6):
        grad = torch.randn([2, 3, 8], generator=g, dtype=torch.float64)
        lr = 0.02 * step
        for group in opt.param_groups:
            group['lr'] = lr
        p.grad = grad.sum(1, keepdim=True)
        opt.step()
        w, m, v, ws = pj.step_tail(grad, w, m, v, step, lr, 0.0, torch.zeros_like(w))
        np.testing.assert_allclose(w.numpy(), p.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert torch.equal(ws, w)


def test_latent_zip_is_read_back_with_equal_bits(tmp_path):
    from latentaugment_amd import formats
    rs = np.random.RandomState(1)
    names = [f'train/p{p:03d}/s_{s:05d}.pickle' for p in range(2) for s in (10, 15, 20)] + ['val/p900/s_00010.pickle']
    codes = {n: rs.randn(6, 32).astype(np.float32) for n in names}
    path = str(tmp_path / 'w.zip')
    assert formats.write_latent_zip(path, codes.items()) == len(names)
    ds = formats.LatentCodeDataset(path, 'train', w_dim=32, num_ws=6)
    assert len(ds) == 6
    for i in range(len(ds)):
        w, fname = ds[i]
        assert w.dtype == np.float32 and w.tobytes() == codes[fname].tobytes()
    for n in names:
        assert ds.lookup(n).tobytes() == codes[n].tobytes()
    with zipfile.ZipFile(path) as z:      # the members are plain ndarray pickles, as the reference's inversion step leaves them
        assert sorted(z.namelist()) == sorted(names)
        w = pickle.loads(z.read(names[0]))
        assert type(w) is np.ndarray and w.dtype == np.float32 and w.shape == (6, 32)
    # refusals: a float64 [w_dim] code, a second shape, a name twice, a name that is no pickle, a path that is no zip
    for bad in ([(names[0], np.zeros(32))], [(names[0], np.zeros((6, 32))), (names[1], np.zeros((1, 32)))],
                [(names[0], np.zeros((6, 32))), (names[0], np.zeros((6, 32)))], [('train/x.npy', np.zeros((6, 32)))]):
        with pytest.raises(ValueError):
            formats.write_latent_zip(str(tmp_path / 'bad.zip'), bad)
    with pytest.raises(IOError):
        formats.write_latent_zip(str(tmp_path / 'w.tar'), codes.items())


def test_python_refusals_reach_no_launch():
    """There is no device here: anything that got as far as an engine or a launch would fail differently."""
    from latentaugment_amd import _lib, projector
    G = pj.generator()
    with pytest.raises(_lib.LatentAugHipError, match='no CPU fallback'):
        projector.Projector(G, pj.vgg_ops(8), 'cpu', 2)
    with pytest.raises(_lib.LatentAugHipError, match='img_channels \\* max_batch = 2 \\* 4'):
        projector.check_feature_batch(7, 2, 4)
    projector.check_feature_batch(8, 2, 4)
    assert [projector.box_factor(256 * k, 256) for k in (1, 2, 4, 8)] == [1, 2, 4, 8]
    for R, S in ((256, 96), (256, 512), (256, 16), (96, 32), (32, 0)):
        with pytest.raises(_lib.LatentAugHipError, match='ratio'):
            projector.box_factor(R, S)
    good = dict(targets_shape=(5, 2, 32, 32), img_channels=2, img_resolution=32, num_ws=10, w_dim=32, num_steps=20, space='w', w_pix=0.0)
    assert projector.check_project_args(**good) == 1 and projector.check_project_args(**dict(good, space='w+')) == 10
    for ok in ((5, 1, 32), (1, 32), (32,)):
        assert projector.check_project_args(**dict(good, w_start_shape=ok)) == 1
    assert projector.check_project_args(**dict(good, space='w+', w_start_shape=(5, 10, 32))) == 10
    for bad, word in ((dict(space='z'), 'space'), (dict(num_steps=0), 'num_steps'), (dict(num_steps=2.5), 'num_steps'), (dict(w_pix=-1.0), 'w_pix'),
                      (dict(w_pix=math.nan), 'w_pix'), (dict(targets_shape=(5, 3, 32, 32)), 'targets'), (dict(targets_shape=(5, 2, 32, 16)), 'targets'),
                      (dict(targets_shape=(0, 2, 32, 32)), 'targets'), (dict(targets_shape=(2, 32, 32)), 'targets'),
                      (dict(w_start_shape=(5, 10, 32)), 'w_start'), (dict(w_start_shape=(4, 1, 32)), 'w_start'), (dict(w_start_shape=(5, 1, 16)), 'w_start')):
        with pytest.raises(_lib.LatentAugHipError, match=word):
            projector.check_project_args(**dict(good, **bad))
    with pytest.raises(_lib.LatentAugHipError):
        _lib.require_gpu(torch.zeros([1, 2, 32, 32]))


def test_header_declares_binds_and_exports_the_entries():
    _lib, lib = _lib_loaded()
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    P, I, L, D, F_, Z, U = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_float, C.c_size_t, C.c_uint
    want = {'la_row_dist_workspace_bytes': (Z, [I, L]),
            'la_row_dist_f32': (I, [P, P, I, L, I, D, F_, P, I, P, L, P, Z, P]),
            'la_box_down_f32': (I, [P, P, L, I, I, P]),
            'la_box_up_f32': (I, [P, P, L, I, I, P]),
            'la_proj_step_tail_f32': (I, [P] * 5 + [I] * 5 + [F_] * 5 + [C.c_ulonglong, U, L, P])}
    assert set(want) == set(ENTRIES)
    for name in ENTRIES:
        assert f' {name}(' in text
        assert _lib.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.argtypes == want[name][1] and fn.restype is want[name][0]


def test_entry_refusals_reach_no_launch():
    """LA_ERR_ARG / LA_ERR_WORKSPACE with a message, on a machine where a launch would be LA_ERR_HIP."""
    _lib, lib = _lib_loaded()
    f = (C.c_float * 64)()
    d = (C.c_double * 64)()
    err = lambda: (lib.la_last_error() or b'').decode()      # noqa: E731
    assert lib.la_row_dist_workspace_bytes(0, 4) == 0 and lib.la_row_dist_workspace_bytes(2, 0) == 0
    assert lib.la_row_dist_workspace_bytes(3, 8192) == 64 and lib.la_row_dist_workspace_bytes(3, 8193) == 64 and lib.la_row_dist_workspace_bytes(5, 16385) == 128
    good = dict(a=f, t=f, rows=4, K=8, fold=2, scale=1.0, gscale=1.0, g=f, acc=0, loss=d, stride=1, ws=d, ws_bytes=64)

    def dist(**kw):
        a = dict(good, **kw)
        return lib.la_row_dist_f32(a['a'], a['t'], a['rows'], a['K'], a['fold'], a['scale'], a['gscale'], a['g'], a['acc'], a['loss'], a['stride'],
                                   a['ws'], a['ws_bytes'], None)
    for bad, word in ((dict(a=None), 'null'), (dict(t=None), 'null'), (dict(loss=None), 'null'), (dict(ws=None), 'null'), (dict(rows=0), 'rows'),
                      (dict(rows=65536), 'rows'), (dict(K=0), 'K at least 1'), (dict(fold=0), 'fold'), (dict(fold=3), 'fold'), (dict(stride=0), 'loss_stride'),
                      (dict(a=C.c_void_p(C.addressof(f) + 2)), 'aligned'), (dict(loss=C.c_void_p(C.addressof(d) + 4)), 'aligned')):
        assert dist(**bad) == -1 and word in err(), (bad, err())
    assert dist(ws_bytes=63) == -3 and 'workspace' in err()
    for fn in (lib.la_box_down_f32, lib.la_box_up_f32):
        for args, word in (((None, f, 1, 8, 2), 'null'), ((f, None, 1, 8, 2), 'null'), ((f, f, 0, 8, 2), 'planes'), ((f, f, 1, 8, 3), '1, 2, 4 or 8'),
                           ((f, f, 1, 8, 0), '1, 2, 4 or 8'), ((f, f, 1, 8, 16), '1, 2, 4 or 8'), ((f, f, 1, 6, 4), 'multiple of k'), ((f, f, 1, 2, 4), 'multiple of k')):
            assert fn(*args, None) == -1 and word in err(), (args, err())
    good = dict(dws=f, p=f, m=f, v=f, ws=f, B=1, num_ws=2, wdim=8, wplus=0, step=1, row0=0)

    def tail(**kw):
        a = dict(good, **kw)
        return lib.la_proj_step_tail_f32(a['dws'], a['p'], a['m'], a['v'], a['ws'], a['B'], a['num_ws'], a['wdim'], a['wplus'], a['step'], 0.1, 0.9, 0.999,
                                         1e-8, 0.0, 7, 0, a['row0'], None)
    for bad, word in ((dict(p=None), 'null'), (dict(ws=None), 'null'), (dict(m=None), 'null'), (dict(v=None), 'null'), (dict(B=0), 'at least 1'),
                      (dict(num_ws=0), 'at least 1'), (dict(wdim=0), 'at least 1'), (dict(step=0), '1-based'), (dict(row0=-1), '32 bits'),
                      (dict(row0=2 ** 32), '32 bits')):
        assert tail(**bad) == -1 and word in err(), (bad, err())
