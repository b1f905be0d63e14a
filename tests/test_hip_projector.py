"""The projector on the GPU (latentaugment_amd/projector.py, la_projector.hip) against the float64 restatement of
tests/projector_cases.py: the three kernels on their own, one teacher-forced step of the whole chain, recovery of images the generator
made, and a data set projected into the latent zip the augmenter reads.

Error rule: 4 x the error of the float32 restatement + 2e-6 x the largest float64 magnitude (lpips_cases.bound); integer-valued inputs
whose sums are exact must give the float64 answer bit for bit."""
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import projector_cases as pj  # noqa: E402
from helpers_formats import write_zip  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _s():
    from latentaugment_amd import _lib
    return _lib.stream_ptr()


def _shifted(x, off, dev):
    """A device copy of x whose first element sits `off` floats behind an allocation's base."""
    buf = torch.empty([x.numel() + off], dtype=torch.float32, device=dev)
    view = buf[off:].reshape(x.shape)
    view.copy_(x)
    return view


# ------------------------------------------------------------------------------------------------------------ kernel 1
def _row_dist(lib, dev, a, t, fold, scale, gscale, g0, off):
    """(loss float64 [rows / fold], g float32 [rows][K]) of one call; g0 None: written, else accumulated onto g0."""
    rows, K = a.shape
    ad, td = _shifted(a, off, dev), _shifted(t, off, dev)
    gd = _shifted(g0 if g0 is not None else torch.full([rows, K], float('nan')), off, dev)
    nbytes = lib.la_row_dist_workspace_bytes(rows, K)
    ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
    loss = torch.full([rows // fold, 3], -1.0, dtype=torch.float64, device=dev)      # stride 3: the other columns stay untouched
    rc = lib.la_row_dist_f32(ad.data_ptr(), td.data_ptr(), rows, K, fold, scale, gscale, gd.data_ptr(), int(g0 is not None),
                             loss.data_ptr() + 8, 3, ws.data_ptr(), nbytes, _s())
    assert rc == 0, lib.la_last_error()
    loss = loss.cpu()
    assert (loss[:, 0] == -1.0).all() and (loss[:, 2] == -1.0).all()
    return loss[:, 1].clone(), gd.cpu().clone()


@pytest.mark.parametrize('K', [1, 3, 255, 256, 257, 4099, 8192, 16388])
@pytest.mark.parametrize('rows', [1, 2, 5])
def test_row_distance_kernel(dev, lib, rows, K):
    """K below, at and past the 256-thread stride, the 8192-element chunk (16388: three chunks, the last one ragged, on the float4 path);
    the base pointer on a 16-byte boundary (float4 path where K % 4 == 0) and one float past it (scalar path); written and accumulated."""
    rs = np.random.RandomState(1000 * rows + K)
    for off in (0, 1):
        for acc in (False, True):
            # integers: every product and sum is exact, so the float64 answer is the only right one
            a = torch.from_numpy(rs.randint(-8, 9, (rows, K)).astype(np.float32))
            t = torch.from_numpy(rs.randint(-8, 9, (rows, K)).astype(np.float32))
            g0 = torch.from_numpy(rs.randint(-8, 9, (rows, K)).astype(np.float32)) if acc else None
            loss, g = _row_dist(lib, dev, a, t, 1, 0.25, 0.5, g0, off)
            loss_r, g_r = pj.row_dist(a.double(), t.double(), 1, 0.25, 0.5)
            g_r = g_r + g0.double() if acc else g_r
            assert torch.equal(loss, loss_r), (off, acc)
            assert torch.equal(g.double(), g_r), (off, acc)
            # floats, targets close to the rows as in a late step: the rule
            a = torch.from_numpy(rs.randn(rows, K).astype(np.float32))
            t = a + torch.from_numpy((0.05 * rs.randn(rows, K)).astype(np.float32))
            g0 = torch.from_numpy(rs.randn(rows, K).astype(np.float32)) if acc else None
            scale, gscale = 1.0 / K, float(np.float32(2.0 / K))
            loss, g = _row_dist(lib, dev, a, t, 1, scale, gscale, g0, off)
            loss2, g2 = _row_dist(lib, dev, a, t, 1, scale, gscale, g0, off)
            assert torch.equal(loss, loss2) and torch.equal(g, g2)      # two runs, equal bits
            l64, g64 = pj.row_dist(a.double(), t.double(), 1, scale, gscale)
            l32, g32 = pj.row_dist(a, t, 1, scale, gscale)
            if acc:
                g64, g32 = g64 + g0.double(), g32 + g0
            lc.check(f'loss rows {rows} K {K} off {off} acc {acc}', loss, l64, l32)
            lc.check(f'g    rows {rows} K {K} off {off} acc {acc}', g, g64, g32)


def test_row_distance_folds_modality_major_rows(dev, lib):
    """fold = C: output j sums rows j, B + j, 2 B + j -- the rows of one sample in the feature net's batch; no gradient asked for."""
    rs = np.random.RandomState(5)
    C_, B, K = 3, 4, 8197
    a = torch.from_numpy(rs.randint(-8, 9, (C_ * B, K)).astype(np.float32))
    t = torch.from_numpy(rs.randint(-8, 9, (C_ * B, K)).astype(np.float32))
    ad, td = a.to(dev), t.to(dev)
    nbytes = lib.la_row_dist_workspace_bytes(C_ * B, K)
    ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
    loss = torch.empty([B], dtype=torch.float64, device=dev)
    assert lib.la_row_dist_f32(ad.data_ptr(), td.data_ptr(), C_ * B, K, C_, 0.5, 1.0, None, 0, loss.data_ptr(), 1, ws.data_ptr(), nbytes, _s()) == 0
    want = 0.5 * (a.double() - t.double()).square().sum(1).reshape(C_, B).sum(0)
    assert torch.equal(loss.cpu(), want)


# ------------------------------------------------------------------------------------------------------------ kernel 2
@pytest.mark.parametrize('planes', [1, 3])
@pytest.mark.parametrize('k', [1, 2, 4])
@pytest.mark.parametrize('R', [8, 24])
def test_box_down_and_its_adjoint(dev, lib, R, k, planes):
    rs = np.random.RandomState(100 * R + 10 * k + planes)
    S = R // k
    x = torch.from_numpy(rs.randint(-8, 9, (planes, R, R)).astype(np.float32))
    y = torch.from_numpy(rs.randint(-8, 9, (planes, S, S)).astype(np.float32))
    xd, yd = x.to(dev), y.to(dev)
    down = torch.full([planes, S, S], float('nan'), device=dev)
    up = torch.full([planes, R, R], float('nan'), device=dev)
    assert lib.la_box_down_f32(xd.data_ptr(), down.data_ptr(), planes, R, k, _s()) == 0, lib.la_last_error()
    assert lib.la_box_up_f32(yd.data_ptr(), up.data_ptr(), planes, R, k, _s()) == 0, lib.la_last_error()
    down, up = down.cpu().double(), up.cpu().double()
    assert torch.equal(down, pj.box_down(x.double(), k))                      # exact on integers
    assert torch.equal(up, pj.box_up(y.double(), k))
    assert float((down * y.double()).sum()) == float((x.double() * up).sum())      # <down(x), y> == <x, up(y)>
    # floats: the rule
    xf = torch.from_numpy(rs.randn(planes, R, R).astype(np.float32))
    xfd, out = xf.to(dev), torch.empty([planes, S, S], device=dev)
    assert lib.la_box_down_f32(xfd.data_ptr(), out.data_ptr(), planes, R, k, _s()) == 0
    lc.check(f'box_down R {R} k {k}', out.cpu(), pj.box_down(xf.double(), k), pj.box_down(xf, k))


# ------------------------------------------------------------------------------------------------------------ kernel 3
def _tail(lib, dev, dws, w, m, v, num_ws, wplus, step, lr, sigma, seed, layer, row0):
    B, L, wdim = w.shape
    wd, md, vd = w.to(dev), m.to(dev), v.to(dev)
    ws = torch.full([B, L, wdim], float('nan'), device=dev)
    dd = dws.to(dev) if dws is not None else None
    rc = lib.la_proj_step_tail_f32(dd.data_ptr() if dd is not None else None, wd.data_ptr(), md.data_ptr(), vd.data_ptr(), ws.data_ptr(), B, num_ws, wdim,
                                   wplus, step, lr, 0.9, 0.999, 1e-8, sigma, seed, layer, row0, _s())
    assert rc == 0, lib.la_last_error()
    return wd.cpu(), md.cpu(), vd.cpu(), ws.cpu()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('num_ws', [1, 6, 14])
@pytest.mark.parametrize('w_dim', [30, 32, 512])
def test_step_tail_kernel(dev, lib, w_dim, num_ws, B):
    """W and W+, Adam steps 1 and 7, sigma zero and positive, against the float64 restatement with noise_ref's stream.  The normals of two
    float32 libraries differ by an ulp or two of log / sincos: 1e-5 absolute on N(0, 1) values, as the noise test allows, times sigma.
    (w_dim = 30: rows that are no multiple of the four normals of one counter.)"""
    rs = np.random.RandomState(10000 * w_dim + 100 * num_ws + B)
    seed, row0 = 2 ** 47 + 11, 3
    for wplus in (0, 1):
        L = num_ws if wplus else 1
        for step in (1, 7):
            for sigma in (0.0, 0.37):
                dws = torch.from_numpy(rs.randn(B, num_ws, w_dim).astype(np.float32))
                w = torch.from_numpy(rs.randn(B, L, w_dim).astype(np.float32))
                m = torch.from_numpy((0.1 * rs.randn(B, L, w_dim)).astype(np.float32)) if step > 1 else torch.zeros([B, L, w_dim])
                v = torch.from_numpy((0.1 * rs.randn(B, L, w_dim) ** 2).astype(np.float32)) if step > 1 else torch.zeros([B, L, w_dim])
                lr = float(np.float32(0.03 * step))
                sig = float(np.float32(sigma))
                got = _tail(lib, dev, dws, w, m, v, num_ws, wplus, step, lr, sig, seed, step, row0)
                n = pj.noise(B, L, w_dim, seed, step, row0)
                r64 = pj.step_tail(dws.double(), w.double(), m.double(), v.double(), step, lr, sig, n)
                r32 = pj.step_tail(dws, w, m, v, step, lr, sig, n)
                for name, g, a, b in zip(('w', 'm', 'v'), got, r64, r32):
                    lc.check(f'{name} wdim {w_dim} num_ws {num_ws} B {B} wplus {wplus} step {step} sigma {sigma}', g, a, b)
                err = float((got[3].double() - r64[3]).abs().max())
                bound = lc.bound(r64[3], r32[3]) + 1e-5 * sig
                print(f'ws err {err:.3e} bound {bound:.3e}')
                assert torch.isfinite(got[3]).all() and err <= bound


def test_step_tail_draws_the_library_stream_and_can_skip_the_update(dev, lib):
    """dws null: p, m, v untouched, and with p = 0, sigma = 1 the output IS the normal: the bits of la_noise_normal_f32 for rows of
    L * w_dim elements, at a shard's first row."""
    B, L, w_dim, seed, layer, row0 = 3, 6, 30, 0x123456789abc, 9, 5
    z = torch.zeros([B, L, w_dim])
    mv = torch.full([B, L, w_dim], 0.25)
    wd, md, vd, ws = _tail(lib, dev, None, z, mv, mv, L, 1, 0, 0.1, 1.0, seed, layer, row0)
    assert torch.equal(wd, z) and torch.equal(md, mv) and torch.equal(vd, mv)
    ref = torch.full([B, L * w_dim], float('nan'), device=dev)
    assert lib.la_noise_normal_f32(ref.data_ptr(), B, L * w_dim, seed, layer, row0, _s()) == 0
    assert torch.equal(ws.reshape(B, -1), ref.cpu())


# ------------------------------------------------------------------------------------------------------------ one step, teacher-forced
def _projector(dev, case, precision, max_batch=3):
    from latentaugment_amd.projector import Projector
    net = types.SimpleNamespace(ops=case.ops, pre_scale=case.pre_scale, pre_shift=case.pre_shift)
    return Projector(pj.generator(), net, dev, max_batch, precision=precision, lpips_res=pj.TINY['img_resolution'] // case.k)


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
@pytest.mark.parametrize('space,w_pix,k,affine', pj.STEP_CASES)
def test_one_step_teacher_forced(dev, space, w_pix, k, affine, precision):
    """At the float64 oracle's own w_opt of steps 0, 1 and 5 (never a free-running comparison: Adam divides by |g|, and float32 and
    float64 paths separate within a few steps): the noised latent, the per-sample losses and d loss / d w_opt of the HIP chain against the
    oracle chain evaluated at the latent the device drew.  k = 2: a 16^2 net behind the box average, with an input affine whose three
    scales differ.  The noise seed of each case is the first whose compared points keep every pre-activation of the float64 run away from
    its kink (projector_cases.KINK_MARGIN): nearer than that, which side a float32 sum lands on is chance, and so is the gradient."""
    case = pj.make_case(space, w_pix, k, affine)
    proj = _projector(dev, case, precision)
    G, tgt = pj.generator(), pj.targets()
    B = tgt.shape[0]
    assert (proj.k, proj.num_ws, proj.w_dim) == (k, G.num_ws, G.w_dim)
    _, std = pj.w_stats()
    sim = pj.simulate(pj.case_key(case), torch.float64, 6)
    tgt_d = tgt.to(dev)
    tfeat = proj.target_features(tgt_d)
    lc.check('F(T)', tfeat.cpu(), pj.features(case, tgt, torch.float64), pj.features(case, tgt, torch.float32))
    for t in (0, 1, 5):
        w64 = sim['w'][t]
        w_opt = w64.float().to(dev)
        ws = torch.empty_like(w_opt)
        sigma = float(np.float32(pj.schedule(t, case.T, std)[1]))
        proj.step_tail(None, w_opt, None, None, ws, 0, 0.0, sigma, case.seed, t, 0)
        ws_r = w64.float().double() + sigma * pj.noise(B, case.L, G.w_dim, case.seed, t)
        assert sigma > 0 and float((ws.cpu().double() - ws_r).abs().max()) <= 1e-5 * sigma + 2.0 ** -23 * float(ws_r.abs().max())
        loss = torch.zeros([B, 2], dtype=torch.float64, device=dev)
        dws, img = proj.loss_and_grad(ws, tgt_d, tfeat, w_pix, loss)
        at = ws.cpu().double()
        l64, d64, i64 = pj.terms(case, at, tgt, torch.float64)
        l32, d32, i32 = pj.terms(case, at, tgt, torch.float32)
        fold = (lambda d: d.double().sum(1)) if space == 'w' else (lambda d: d.double())
        tag = f'{case.name} {precision} t {t}'
        lc.check('img  ' + tag, img.cpu(), i64, i32)
        lc.check('d    ' + tag, loss[:, 0].cpu(), l64[:, 0], l32[:, 0])
        if w_pix > 0:
            lc.check('p    ' + tag, loss[:, 1].cpu(), l64[:, 1], l32[:, 1])
        else:
            assert float(loss[:, 1].abs().max()) == 0.0
        lc.check('grad ' + tag, fold(dws.cpu()), fold(d64), fold(d32))
        # the loss the free-running oracle saw at this step is the same quantity (its own noise differs by the normals' ulps)
        np.testing.assert_allclose(l64.numpy(), sim['loss'][t].numpy(), rtol=1e-3, atol=1e-9)


def test_w_stats_against_the_oracle_mapping(dev):
    proj = _projector(dev, pj.make_case('w', 0.0), 'f32')
    avg, std = proj.w_stats(1000, 123)
    a64, s64 = pj.w_stats(1000, 123, torch.float64)
    a32, s32 = pj.w_stats(1000, 123, torch.float32)
    lc.check('w_avg', avg, a64, a32)
    lc.check('w_std', [std], [s64], [s32])
    assert proj.w_stats(1000, 123)[0] is avg      # once per (samples, seed)


# ------------------------------------------------------------------------------------------------------------ recovery
def test_recovery_of_generated_targets(dev):
    """Targets G(mapping(z)) of three seeded z, 200 steps of the default schedule from w_avg: every sample's perceptual distance at the
    last step is at most 1 % of its distance at step 0.  The restatement of projector_cases.py on these targets starts at 0.79, 0.79, 1.14
    and ends at 3.5e-4, 9.1e-6, 1.4e-5 in float64 and at 9.2e-5, 2.0e-5, 1.2e-4 in float32: more than twentyfold room.  Two calls with
    one seed return equal bits."""
    proj = _projector(dev, pj.make_case('w', 0.0), 'f16x2')
    tgt = pj.targets().to(dev)
    a = proj.project(tgt, num_steps=200, seed=0)
    d = a['loss'][:, :, 0].cpu()
    print('step-0 distance', d[0].tolist(), 'final', d[-1].tolist())
    assert a['w'].shape == (3, proj.num_ws, proj.w_dim) and a['img'].shape == tgt.shape and a['loss'].shape == (200, 3, 2)
    assert torch.isfinite(a['loss']).all() and float(a['loss'][:, :, 1].abs().max()) == 0.0
    assert (d[-1] <= 0.01 * d[0]).all(), (d[0].tolist(), d[-1].tolist())
    assert torch.equal(a['w'][:, :1].expand_as(a['w']), a['w'])      # W space: one row, broadcast
    i64, i32 = (pj.synthesis(a['w'].cpu(), dt).detach() for dt in (torch.float64, torch.float32))
    lc.check('final image', a['img'].cpu(), i64, i32)
    b = proj.project(tgt, num_steps=200, seed=0)
    assert all(torch.equal(a[key], b[key]) for key in ('w', 'img', 'loss'))
    c = proj.project(tgt, num_steps=200, seed=1)
    assert not torch.equal(a['w'], c['w'])      # (another seed draws other noise)


# ------------------------------------------------------------------------------------------------------------ data set
def test_projected_dataset_feeds_the_augmenter(dev, tmp_path):
    """Five slices, max_batch = 2 (a ragged last batch), 20 steps: the latent zip carries the image zip's member names and [num_ws, w_dim]
    float32 codes, the last slice (a batch of one at global row 4) equals a call of its own with row0 = 4, and create_augment (generator injected, everything else from the
    two zips) runs set_input -> forward -> get_output from it, in W and in W+."""
    from latentaugment_amd import formats
    from latentaugment_amd.augments import create_augment
    from latentaugment_amd.projector import project_dataset
    G = pj.generator()
    idir = tmp_path / 'interim' / 'DS'
    idir.mkdir(parents=True)
    raw = ((pj.targets(5, seed=21) + 1) * 127.5).numpy()
    names = [f'train/p000/s_{sl:05d}.pickle' for sl in (10, 15, 20, 25, 30)]
    write_zip(str(idir / 'DSNAME.zip'), {n: {'A': raw[i, 0], 'B': raw[i, 1]} for i, n in enumerate(names)})
    proj = _projector(dev, pj.make_case('w', 0.0), 'f16x2', max_batch=2)
    finals = {}
    for space, wname in (('w', 'WNAME'), ('w+', 'WPNAME')):
        finals[space] = project_dataset(str(idir / 'DSNAME.zip'), str(idir / f'{wname}.zip'), 'train', proj, ['A', 'B'], num_steps=20, space=space, seed=3)
        assert finals[space].shape == (5, 2) and np.isfinite(finals[space]).all()
        ds = formats.LatentCodeDataset(str(idir / f'{wname}.zip'), 'train', w_dim=G.w_dim, num_ws=G.num_ws)
        assert [ds[i][1] for i in range(len(ds))] == names
        codes = np.stack([ds.lookup(n) for n in names])
        assert codes.dtype == np.float32 and codes.shape == (5, G.num_ws, G.w_dim) and np.isfinite(codes).all()
        assert (codes[:, :1] == codes).all() == (space == 'w')
        # the last slice was a batch of one, at global row 4
        x = torch.from_numpy(raw[4:5]) / 127.5 - 1
        alone = proj.project(x.to(dev), num_steps=20, space=space, seed=3, row0=4)
        assert np.array_equal(alone['w'][0].cpu().numpy(), codes[4])
        assert not np.array_equal(proj.project(x.to(dev), num_steps=20, space=space, seed=3)['w'][0].cpu().numpy(), codes[4])
    for space, wname in (('w', 'WNAME'), ('w+', 'WPNAME')):
        shutil.rmtree(idir / 'cache_dir', ignore_errors=True)      # (the bank cache is keyed by the folder, not by the zip's name)
        opt = types.SimpleNamespace(
            img_resolution=32, batch_size=2, modalities_aug='A,B', opt_num_epochs=3, opt_lr=0.01, truncation_psi=1.0, w_pix=1.0, w_lpips=0.0,
            w_latent=0.3, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False,
            criterion_mode='gemm', final_noise_mode='const', precision='f32', latent_space=space, aug='latent', gpu_ids=[0], gpu_ids_aug='0',
            checkpoints_dir=str(tmp_path), name='t', phase='train', rand_aug=False, lower_bound_clip=False, p_thres=0.0, init_w='inv',
            interim_dir=str(tmp_path / 'interim'), dataset_aug='DS', dataset_name_aug='DSNAME', dataset_w_name=wname, step_w=5, step_img=20,
            inject=dict(generator=G))
        aug = create_augment(opt)
        paths = [names[1], names[4]]
        aug.set_input({'A': torch.zeros([2, 1, 32, 32]), 'B': torch.zeros([2, 1, 32, 32]), 'A_paths': paths, 'B_paths': list(paths)})
        aug.forward()
        out = aug.get_output()
        assert out['A'].shape == out['B'].shape == (2, 1, 32, 32) and out['A_paths'] == paths
        assert torch.isfinite(out['A']).all() and torch.isfinite(out['B']).all()
        ds = formats.LatentCodeDataset(str(idir / f'{wname}.zip'), 'train', w_dim=G.w_dim, num_ws=G.num_ws)
        want = np.stack([ds.lookup(p) for p in paths])
        got = aug.get_latent_input()['w']
        assert np.array_equal(got, want if space == 'w+' else want[:, 0])      # the start of the optimisation is the projected code
