"""The perceptual feature engine (la_feat.hip, FeatureEngine) and the discriminator engine (la_disc.hip, DiscriminatorEngine) against the
float64 restatements of tests/engine_cases.py, at the shapes where their kernels and seams change form.  Modes f32, bf16x3, f16x2.

EXACT cases (the pools on small integers with planted ties): bit for bit what exact routing gives.
GUARDED cases (no float64 pre-activation within g of a kink, proved in test_engine_cases_cpu.py): features / logits and the input gradient,
every element, worst |hip - f64| <= K[mode] x worst |f32-CPU - f64| + 2^-23 x max|f64|, and never beyond the ceilings the older tests
allow (features 1e-4 |ref| + 1e-5 max, logits 1e-4 |ref| + 1e-4 max, gradients 1e-3 |ref| + 2e-5 max for D, + 3e-5 max for the feature
net).  BULK (R = 128): relative L2 <= 1.5 x that of the float32 CPU run + 1e-6.  No element is excluded anywhere.  The float32 CPU run of
the restatement sets every budget; the code under test sets none.  Every case prints `err / budget = ratio` and the k it would need.

K: 4 for f32 (the criteria sweep's convention); for the 16-bit modes twice the largest k any guarded case needed on an MI355X.
Measured on an MI355X, largest k any guarded output needed (err minus the rounding floor, over the float32-CPU error) and the
err / budget ratio it had at K = 4:
    feature engine   f32 1.61 (tap-only-C1-res8 gradient, 0.403)   bf16x3 2.64 (odd-res-20 gradient, 0.669)   f16x2 1.63 (cin-odd-in2 gradient, 0.486)
    discriminator    f32 2.45 (group-B8-g4 logits, 0.624)          bf16x3 3.34 (clamp-none logits, 0.841)     f16x2 2.10 (clamp-none logits, 0.540)
hence K = 6.7 for bf16x3 and 4.2 for f16x2.  No output came near a ceiling except the one noted at the tap-only sweep.  Bulk R128, relative
L2 / budget: logits 0.419 / 0.548 / 0.754, gradient 0.285 / 0.209 / 0.236 (f32 / bf16x3 / f16x2).  la_disc_loss: 0.118 in every mode.
With the K above instead of 4 the ratios of the two 16-bit modes are NOT MEASURED (they can only be smaller).

Which case reaches which branch.  la_feat.hip: first conv with cin % 4 == 0 (dst = gx): cin4-*; op list starting with a pool or a tap
(final copy-out): tap-only-*, pool-exact, tap-zero; f16x2 tap behind a pool (unfused tap, la_conv_act_grad_pmax in slot mode):
tap-behind-maxpool, tap-behind-avgpool; f16x2 conv on conv (`below`): conv-conv, conv-conv-conv-pool; max-pool ties: pool-exact;
tap lanes at HW 9 / 36 / 100 / 196: tap-only-C8-res3 / 6 / 10 / 14; the c + 7 CG < C boundary: tap-only C 28 / 29 / 32 / 33 / 36 at res 8,
C 512 / 513 at res 2; C < CG: tap-only C 1 / 3 at res 8, C 3 at res 2; zero pixels and lin == 0: tap-zero; resolutions 6, 10, 12, 14, 20,
28: cin-odd, tap-between, conv-conv, odd-res-20 / 28; N < max_batch: every case with N 3 / 4, 1 / 8, 5 / 8; small N after large N:
feat-shrinking-batch; non-first conv with cin % 4 != 0: refusals[second-conv-cin3].  la_disc.hip: R * R > 4096 in f16x2: R128 (sweep and
accumulate); R = 8: R8, group-*; img_channels 1 / 3 / 4: imgc*; MinibatchStd G = 1, G = 3, G = 4 and G = 3 with two groups, G = 9 and G = 16 (the generic loops): group-*;
batch not divisible by G: the group refusal; a clamp that binds: clamp-0.5; conv_clamp None: clamp-none; channel tables 12 / 20 / 36 and
their refusal: channels-12-20-36, the multiple-of-4 refusal; la_disc_loss: the loss kernel test; accumulate != 0: backward_accumulate;
B < max_batch after a full batch: disc-shrinking-batch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG = -1
MODES = ['f32', 'bf16x3', 'f16x2']
K = {'f32': 4.0, 'bf16x3': 6.7, 'f16x2': 4.2}
CEIL = {'feat': (1e-4, 1e-5), 'logits': (1e-4, 1e-4), 'gx_feat': (1e-3, 3e-5), 'gx_disc': (1e-3, 2e-5)}          # (rtol, atol x max|ref|)


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


_REFS = {}


def _ref(case):
    """the float32 and float64 CPU runs of a case, computed once and shared by the modes"""
    if case.name not in _REFS:
        _REFS[case.name] = case.runs()
    return _REFS[case.name]


def _judge(name, mode, got, r32, r64, ceil):
    """guarded criterion on one output; returns the k this output would have needed"""
    got = got.detach().cpu().double()
    err, err32 = ec.worst(got, r64), ec.worst(r32, r64)
    floor = ec.EPS32 * float(r64.abs().max())
    bud = K[mode] * err32 + floor
    need = max(err - floor, 0.0) / err32 if err32 > 0 else (0.0 if err <= floor else float('inf'))
    print(f'{name} [{mode}]: err {err:.3e} / budget {bud:.3e} = ratio {err / bud:.3f} (f32-CPU err {err32:.3e}, needs k = {need:.2f})')
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    rtol, atol = CEIL[ceil] if ceil else (0.0, float('inf'))
    over = (got - r64).abs() - (rtol * r64.abs() + atol * float(r64.abs().max()))
    assert float(over.max()) <= 0, f'{name} [{mode}]: beyond the ceiling of the older tests by {float(over.max()):.3e}'
    assert err <= bud, f'{name} [{mode}]: err {err:.3e} > budget {bud:.3e}'
    return need


# ---------------------------------------------------------------------------------------------------------------------------------
# feature engine

def _feat_engine(dev, ops, in_ch, res, max_batch, mode):
    from latentaugment_amd.synthesis import FeatureEngine
    return FeatureEngine(ops, dev, in_res=res, max_batch=max_batch, in_ch=in_ch, precision=mode)


def _feat_run(eng, dev, x, gfeat):
    f = eng.forward(x.to(dev))
    gx = eng.backward(gfeat.to(dev))
    torch.cuda.synchronize()
    return f.cpu(), gx.cpu()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ec.FEAT_CASES, ids=[c.name for c in ec.FEAT_CASES])
def test_feature_engine_sweep(dev, case, mode):
    ops, x, gfeat, r32, r64 = _ref(case)
    eng = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
    assert eng.num_features == r64['feat'].shape[1]
    f, gx = _feat_run(eng, dev, x, gfeat)
    _judge(f'feat {case.name} features', mode, f, r32['feat'], r64['feat'], 'feat')
    # (a tap on ONE channel has the gradient 0 by construction -- the normalised value is +-1 -- so max|ref| is the rounding residue of a
    #  cancellation and a ceiling relative to it says nothing: the budget alone judges that case)
    _judge(f'feat {case.name} gradient', mode, gx, r32['gx'], r64['gx'], None if (case.kinds == ['tap'] and case.in_ch == 1) else 'gx_feat')


@pytest.mark.parametrize('mode', MODES)
def test_feature_tap_on_zero_pixels_and_zero_lin(dev, mode):
    """all-zero channel vectors (rsqrt(1e-10)) and lin[c] == 0 (sqrt(0)): finite, and within the budget"""
    ops, x, gfeat = ec.tap_zero_inputs()
    t = ec.TAP_ZERO
    r32, r64 = ec.feat_restate(ops, x, torch.float32, gfeat), ec.feat_restate(ops, x, torch.float64, gfeat)
    eng = _feat_engine(dev, ops, t['C'], t['res'], t['N'], mode)
    f, gx = _feat_run(eng, dev, x, gfeat)
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(gx).all())
    fz = f.reshape(t['N'], t['C'], t['res'], t['res'])
    for n, yy, xx in t['zero_pixels']:
        assert bool((fz[n, :, yy, xx] == 0).all())
    assert bool((fz[:, t['zero_lin']] == 0).all()) and bool((gx.reshape(x.shape)[:, t['zero_lin']] != 0).any())
    _judge('feat tap-zero features', mode, f, r32['feat'], r64['feat'], 'feat')
    _judge('feat tap-zero gradient', mode, gx, r32['gx'], r64['gx'], 'gx_feat')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('pool,res', ec.POOL_EXACT)
def test_feature_pool_exact_with_ties(dev, pool, res, mode):
    """`pool, tap` on integers with the three tie patterns.  The pooled integers are exact in float32, so the engine's features must be
    BIT FOR BIT those of a `tap`-only engine fed the float64-pooled values, and its input gradient BIT FOR BIT the exact routing (first
    maximum in scan order; a quarter each for the average) of that engine's gradient.  The float64 restatement of the whole list is
    judged as a guarded case on top (a wrong routing is a difference of order 1 there)."""
    x, lin, gfeat = ec.pool_exact_inputs(res)
    pooled, route = ec.pool_exact_reference(pool, x)
    ops = [(pool,), ('tap', lin)]
    eng = _feat_engine(dev, ops, ec.POOL_C, res, ec.POOL_N, mode)
    f, gx = _feat_run(eng, dev, x, gfeat)
    tap = _feat_engine(dev, [('tap', lin)], ec.POOL_C, res // 2, ec.POOL_N, mode)
    ft, gt = _feat_run(tap, dev, pooled.float(), gfeat)
    assert torch.equal(f, ft), f'{pool} res {res}: the pool forward is not exact'
    want = route(gt).float()          # (a copy, or an exact quarter, of float32 values)
    bad = (gx != want).nonzero()
    assert bad.numel() == 0, f'{pool} res {res}: {len(bad)} gradient elements differ from the exact routing, first at {bad[0].tolist()}'
    r32, r64 = ec.feat_restate(ops, x, torch.float32, gfeat), ec.feat_restate(ops, x, torch.float64, gfeat)
    _judge(f'feat pool-exact {pool} res{res} features', mode, f, r32['feat'], r64['feat'], 'feat')
    _judge(f'feat pool-exact {pool} res{res} gradient', mode, gx, r32['gx'], r64['gx'], 'gx_feat')


@pytest.mark.parametrize('pool,res', ec.POOL_EXACT)
def test_feature_pool_sign_variant(dev, pool, res):
    """C = 1, inputs +-k: behind the pool the normalised value is +-1 (times sqrt(lin) / sqrt(HW)) and the tap's gradient vanishes by
    construction, so the features show the pool forward alone.  The gradient is a difference of two terms of size |u| r: it must
    vanish to one float32 rounding of that size (plus 4 x what the float32 CPU run leaves)."""
    x, lin, gfeat = ec.pool_sign_inputs(res)
    ops = [(pool,), ('tap', lin)]
    r32, r64 = ec.feat_restate(ops, x, torch.float32, gfeat), ec.feat_restate(ops, x, torch.float64, gfeat)
    eng = _feat_engine(dev, ops, 1, res, ec.POOL_N, 'f32')
    f, gx = _feat_run(eng, dev, x, gfeat)
    _judge(f'feat pool-sign {pool} res{res} features', 'f32', f, r32['feat'], r64['feat'], 'feat')
    pooled, _ = ec.pool_exact_reference(pool, x)
    nz = pooled.flatten(1) != 0          # (an average of +-k can be 0: no sign there)
    assert torch.equal(torch.sign(f)[nz], torch.sign(pooled.flatten(1).float())[nz])
    term = float((gfeat.double().abs() / (res // 2) * torch.rsqrt(pooled.flatten(1) ** 2 + 1e-10)).max())          # |u| r
    bud = 4.0 * ec.worst(r32['gx'], r64['gx']) + 4 * ec.EPS32 * term          # (y, y * dot, u - y * dot, r * (...): four roundings)
    err = ec.worst(gx, r64['gx'])
    print(f'feat pool-sign {pool} res{res} gradient: err {err:.3e} / budget {bud:.3e} = ratio {err / bud:.3f}')
    assert err <= bud


@pytest.mark.parametrize('mode', MODES)
def test_feature_shrinking_batch_is_bit_identical_to_a_fresh_engine(dev, mode):
    """N = 8 with inputs x 2^8, then N = 3 plain on the SAME engine: stale slot rows and activations behind the live rows must not
    reach the result"""
    case = ec.FEAT_SHRINK
    ops, x, gfeat, r32, r64 = _ref(case)
    g = torch.Generator().manual_seed(77)
    xb = torch.randn([case.max_batch, case.in_ch, case.res, case.res], generator=g) * ec.FEAT_SHRINK_BIG
    gb = torch.randn([case.max_batch, gfeat.shape[1]], generator=g) * ec.FEAT_SHRINK_BIG
    used = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
    fb, gxb = _feat_run(used, dev, xb, gb)
    assert bool(torch.isfinite(fb).all()) and bool(torch.isfinite(gxb).all())
    f1, gx1 = _feat_run(used, dev, x, gfeat)
    fresh = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
    f2, gx2 = _feat_run(fresh, dev, x, gfeat)
    assert torch.equal(f1, f2) and torch.equal(gx1, gx2)
    _judge('feat shrinking-batch features', mode, f1, r32['feat'], r64['feat'], 'feat')
    _judge('feat shrinking-batch gradient', mode, gx1, r32['gx'], r64['gx'], 'gx_feat')


@pytest.mark.parametrize('mode', MODES)
def test_feature_repeat_is_bit_identical(dev, mode):
    case = ec.FEAT_BY_NAME['conv-conv-conv-pool']
    ops, x, gfeat, _, _ = _ref(case)
    eng = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
    xd, gd = x.to(dev), gfeat.to(dev)
    f1, f2 = eng.forward(xd).cpu(), eng.forward(xd).cpu()
    g1, g2 = eng.backward(gd).cpu(), eng.backward(gd).cpu()
    assert torch.equal(f1, f2) and torch.equal(g1, g2)


def _feat_desc(kinds, in_ch, widths):
    from latentaugment_amd import _lib
    code = {'conv': 0, 'tap': 1, 'maxpool': 2, 'avgpool': 3}
    desc, c, wi = [], in_ch, 0
    for k in kinds.split(','):
        co = c
        if k == 'conv':
            co = widths[wi]
            wi += 1
        desc.append(_lib.FeatOp(code[k], c, co))
        c = co
    return (_lib.FeatOp * len(desc))(*desc), len(desc)


@pytest.mark.parametrize('name,kinds,in_ch,res,widths,where,text', ec.FEAT_REFUSALS, ids=[r[0] for r in ec.FEAT_REFUSALS])
def test_feature_refusals(lib, dev, name, kinds, in_ch, res, widths, where, text):
    """argument checks that return LA_ERR_ARG before any launch.  A non-first conv with cin % 4 != 0 is refused when the engine is
    created (the backward used to refuse it half way through)."""
    from latentaugment_amd import _lib
    arr, n = _feat_desc(kinds, in_ch, widths)
    if where == 'create':
        assert lib.la_feat_workspace_bytes(n, arr, in_ch, res, 2) == 0
        assert text in _err_text(lib)
        buf = torch.zeros([1 << 16], dtype=torch.float32, device=dev)
        params = (C.c_void_p * 8)(*[buf.data_ptr()] * 8)
        h = C.c_void_p()
        rc = lib.la_feat_create(n, arr, params, 8, in_ch, res, 2, _p(buf), buf.numel() * 4, _s(), C.byref(h))
        assert rc == LA_ERR_ARG and not h.value and text in _err_text(lib), _err_text(lib)
        return
    case = ec.FeatCase(name, kinds, in_ch, res, 2, 2, widths)
    ops, x, _ = case.build()
    eng = _feat_engine(dev, ops, in_ch, res, 2, 'f32')
    eng.forward(x.to(dev))
    gx = torch.full_like(x, 7.0).to(dev)
    gf = torch.ones([2, eng.num_features], device=dev)
    rc = lib.la_feat_backward(eng.handle, _p(gf), _p(gx), _s())
    torch.cuda.synchronize()
    assert rc == LA_ERR_ARG and text in _err_text(lib), _err_text(lib)
    assert bool((gx == 7.0).all())          # refused before anything was written
    with pytest.raises(_lib.LatentAugHipError, match=text):
        eng.backward(gf)


# ---------------------------------------------------------------------------------------------------------------------------------
# discriminator

def _disc_engine(dev, case, D, mode, max_batch=None):
    from latentaugment_amd.synthesis import DiscriminatorEngine
    return DiscriminatorEngine(D, dev, max_batch=case.max_batch if max_batch is None else max_batch, conv_clamp=case.clamp, precision=mode,
                               mbstd_group_size=case.group)


def _disc_run(eng, dev, img, dlogits):
    logits = eng.forward(img.to(dev))
    gx = eng.backward(dlogits.to(dev))
    torch.cuda.synchronize()
    return logits.cpu(), gx.cpu()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ec.DISC_CASES, ids=[c.name for c in ec.DISC_CASES])
def test_discriminator_sweep(dev, case, mode):
    D, img, dlogits, r32, r64 = _ref(case)
    eng = _disc_engine(dev, case, D, mode)
    assert eng.channels == [case.table[r] for r in sorted(case.table)]
    logits, gx = _disc_run(eng, dev, img, dlogits)
    if case.kind == 'bulk':
        for key, got in (('logits', logits), ('gx', gx)):
            e, e32 = ec.rel_l2(got, r64[key]), ec.rel_l2(r32[key], r64[key])
            bud = 1.5 * e32 + 1e-6
            print(f'disc {case.name} {key} [{mode}]: relative L2 {e:.3e} / budget {bud:.3e} = ratio {e / bud:.3f}')
            assert e <= bud
        return
    _judge(f'disc {case.name} logits', mode, logits, r32['logits'], r64['logits'], 'logits')
    _judge(f'disc {case.name} gradient', mode, gx, r32['gx'], r64['gx'], 'gx_disc')


def test_discriminator_refuses_a_batch_the_group_does_not_divide(lib, dev):
    from latentaugment_amd import _lib
    r = ec.DISC_GROUP_REFUSAL
    case = ec.DiscCase('group-refusal', 8, ec.T8, r['B'], group=r['group'])
    D, img, _ = case.build()
    eng = _disc_engine(dev, case, D, 'f32')
    rc = lib.la_disc_forward(eng.handle, _p(img.to(dev)), r['B'], _s())
    assert rc == LA_ERR_ARG and 'group size' in _err_text(lib)
    with pytest.raises(_lib.LatentAugHipError, match='group size'):
        eng.forward(img.to(dev))


def test_discriminator_refuses_a_channel_count_that_is_no_multiple_of_4(lib, dev):
    t = ec.DISC_BAD_TABLE
    chan = (C.c_int * len(t))(*[t[r] for r in sorted(t)])
    R = max(t)
    assert lib.la_disc_workspace_bytes(R, 2, chan, 2) == 0 and 'multiples of 4' in _err_text(lib)
    buf = torch.zeros([1 << 16], dtype=torch.float32, device=dev)
    n = lib.la_disc_num_params(R)
    params = (C.c_void_p * n)(*[buf.data_ptr()] * n)
    fir = np.zeros([16], np.float32)
    h = C.c_void_p()
    rc = lib.la_disc_create(R, 2, chan, 256.0, params, n, fir.ctypes.data, 4, 2, _p(buf), buf.numel() * 4, _s(), C.byref(h))
    assert rc == LA_ERR_ARG and not h.value and 'multiples of 4' in _err_text(lib), _err_text(lib)


@pytest.mark.parametrize('mode', MODES)
def test_discriminator_shrinking_batch_is_bit_identical_to_a_fresh_engine(dev, mode):
    """B = 8 with inputs x 2^8, then B = 4 plain on the SAME engine: stale xs_f / xs_b rows must not reach the result"""
    case = ec.DISC_SHRINK
    D, img, dlogits, r32, r64 = _ref(case)
    g = torch.Generator().manual_seed(78)
    big = torch.randn([case.max_batch, case.imgc, case.R, case.R], generator=g) * ec.DISC_SHRINK_BIG
    dlb = torch.randn([case.max_batch, 1], generator=g) * ec.DISC_SHRINK_BIG
    used = _disc_engine(dev, case, D, mode)
    lb, gb = _disc_run(used, dev, big, dlb)
    assert bool(torch.isfinite(lb).all()) and bool(torch.isfinite(gb).all())
    l1, g1 = _disc_run(used, dev, img, dlogits)
    fresh = _disc_engine(dev, case, D, mode)
    l2, g2 = _disc_run(fresh, dev, img, dlogits)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _judge('disc shrinking-batch logits', mode, l1, r32['logits'], r64['logits'], 'logits')
    _judge('disc shrinking-batch gradient', mode, g1, r32['gx'], r64['gx'], 'gx_disc')


@pytest.mark.parametrize('mode', MODES)
def test_discriminator_repeat_is_bit_identical(dev, mode):
    case = ec.DISC_BY_NAME['imgc3']
    D, img, dlogits, _, _ = _ref(case)
    eng = _disc_engine(dev, case, D, mode)
    xd, dl = img.to(dev), dlogits.to(dev)
    l1, l2 = eng.forward(xd).cpu(), eng.forward(xd).cpu()
    g1, g2 = eng.backward(dl).cpu(), eng.backward(dl).cpu()
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['imgc3', 'R128'])
def test_discriminator_backward_accumulate(lib, dev, name, mode):
    """la_disc_backward(accumulate = 1) onto a preloaded g_img = preload + the plain result, to one float32 rounding of the sum, element
    by element (R128: the fused FromRGB backward of f16x2)"""
    case = ec.DISC_BY_NAME[name]
    D, img, dlogits, _, _ = _ref(case)
    eng = _disc_engine(dev, case, D, mode)
    eng.forward(img.to(dev))
    plain = eng.backward(dlogits.to(dev))
    pre = torch.randn(plain.shape, generator=torch.Generator().manual_seed(9)).to(dev) * float(plain.abs().max())
    acc = pre.clone()
    dl = dlogits.to(dev).reshape(-1).contiguous()
    rc = lib.la_disc_backward(eng.handle, _p(dl), _p(acc), 1, _s())
    torch.cuda.synchronize()
    assert rc == 0, _err_text(lib)
    want = pre.double() + plain.double()
    over = (acc.double() - want).abs() - ec.EPS32 * want.abs()
    print(f'disc accumulate {name} [{mode}]: worst excess over one rounding of the sum {float(over.max()):.3e}')
    assert float(over.max()) <= 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('norm_batch', ec.LOSS_NORM_BATCH)
def test_discriminator_loss_kernel(lib, dev, norm_batch, mode):
    """la_disc_loss on planted logits (both sides of softplus' threshold at 20, saturation at +-100) against float64, and the backward
    from the kept dlogits against the backward from the float64 dlogits: the backward is linear in them"""
    case = ec.DISC_BY_NAME['group-B8-g4']
    D, img, _, _, _ = _ref(case)
    eng = _disc_engine(dev, case, D, mode)
    eng.forward(img.to(dev))
    off = lib.la_disc_logits(eng.handle) - eng._workspace.data_ptr()          # a view into the workspace, as DiscriminatorEngine.forward takes it
    view = eng._workspace[off:off + 4 * case.B].view(torch.float32)
    view.copy_(torch.tensor(ec.LOSS_LOGITS, dtype=torch.float32))
    l32 = view.cpu().numpy()
    loss = torch.full([1], float('nan'), device=dev)
    assert lib.la_disc_loss(eng.handle, ec.LOSS_W, norm_batch, _p(loss), _s()) == 0, _err_text(lib)
    want, dwant = ec.disc_loss_restate(l32, ec.LOSS_W, norm_batch)
    n = norm_batch if norm_batch > 0 else case.B
    z = -torch.from_numpy(l32)
    want32 = float(torch.where(z > 20, z, torch.log1p(torch.exp(z))).sum() / n * ec.LOSS_W)
    bud = 4.0 * abs(want32 - want) + ec.EPS32 * abs(want)
    err = abs(float(loss.cpu()[0]) - want)
    print(f'disc loss n{norm_batch} [{mode}]: err {err:.3e} / budget {bud:.3e} = ratio {err / bud:.3f}')
    assert err <= bud
    g_kept = torch.empty([case.B, case.imgc, case.R, case.R], device=dev)
    assert lib.la_disc_backward(eng.handle, None, _p(g_kept), 0, _s()) == 0, _err_text(lib)
    dl = torch.from_numpy(dwant.astype(np.float32)).reshape(-1, 1)
    g_given = eng.backward(dl.to(dev))
    torch.cuda.synchronize()
    dl32 = (-torch.sigmoid(z) * ec.LOSS_W / n).reshape(-1, 1)          # the float32 CPU run's own dlogits
    r32 = case.restate(D, img, dl32, torch.float32)
    r64 = case.restate(D, img, torch.from_numpy(dwant).reshape(-1, 1), torch.float64)
    _judge(f'disc loss n{norm_batch} gradient from the kept dlogits', mode, g_kept, r32['gx'], r64['gx'], 'gx_disc')
    _judge(f'disc loss n{norm_batch} gradient from the given dlogits', mode, g_given, r32['gx'], r64['gx'], 'gx_disc')
