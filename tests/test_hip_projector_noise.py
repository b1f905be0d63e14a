"""The projector's noise-map optimisation on the GPU (la_noise.hip, la_synth_backward_noise, the regulariser and the noise tail of
la_projector.hip, Projector.project(optimize_noise=True)) against the float64 restatement of tests/noise_cases.py.

Error rule: 4 x the error of the float32 restatement + 2e-6 x the largest float64 magnitude (lpips_cases.bound); integer-valued inputs
whose sums are exact must give the float64 answer bit for bit."""
import copy
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import noise_cases as nc  # noqa: E402
import projector_cases as pj  # noqa: E402
import synth_cases as sc  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

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


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ints(v):
    return (C.c_int * len(v))(*v)


# ------------------------------------------------------------------------------------------------------------ the channel reduction
@pytest.mark.parametrize('HW,Cc,B', nc.GRAD_SHAPES)
def test_noise_grad_kernel(dev, lib, HW, Cc, B):
    """Planes below and above the switch between the wave-per-pixel kernel and the float4 kernel (256 pixels), channel counts below, at and
    past the 64 lanes and the 4 / 16 channel slices (132: a ragged last round), d read with a row stride that is no multiple of 4 from a
    base one float past an allocation's."""
    rs = np.random.RandomState(HW + 7 * Cc + B)
    stride = Cc + 3

    def run(gz, d, strength):
        gzd = gz.to(dev)
        dbuf = torch.full([1 + B * stride], float('nan'), device=dev)
        dbuf[1:].reshape(B, stride)[:, :Cc] = d.to(dev)
        out = torch.full([B, HW], float('nan'), device=dev)
        rc = lib.la_noise_grad_f32(gzd.data_ptr(), dbuf.data_ptr() + 4, stride, B, Cc, HW, strength, out.data_ptr(), _s())
        assert rc == 0, lib.la_last_error()
        return out.cpu()
    # integers over powers of two, times a power of two: every quotient and every partial sum is exact in float32
    gz = torch.from_numpy(rs.randint(-8, 9, (B, Cc, HW)).astype(np.float32))
    d = torch.from_numpy((2.0 ** rs.randint(-2, 3, (B, Cc))).astype(np.float32))
    assert torch.equal(run(gz, d, 0.5).double(), nc.noise_grad(gz.double(), d.double(), 0.5))
    gz = torch.from_numpy(rs.randn(B, Cc, HW).astype(np.float32))
    d = torch.from_numpy((0.5 + rs.rand(B, Cc)).astype(np.float32))
    strength = float(np.float32(0.05))
    got, again = run(gz, d, strength), run(gz, d, strength)
    assert torch.equal(got, again)      # two runs, equal bits
    lc.check(f'noise_grad HW {HW} C {Cc} B {B}', got, nc.noise_grad(gz.double(), d.double(), strength), nc.noise_grad(gz, d, strength))


# ------------------------------------------------------------------------------------------------------------ the regulariser
def _reg(lib, dev, maps, scale, weight, g0=None, guard=None, short=0):
    """(reg [B] float64, [g]) of one call over a table of maps; g0: accumulated onto.  The workspace comes poisoned and between guard bands."""
    B = maps[0].shape[0]
    res = [m.shape[-1] for m in maps]
    guard = Guarded('ones') if guard is None else guard
    md = [m.to(dev) for m in maps]
    gd = [guard.tensor(m.shape, torch.float32, dev, float('nan')) for m in maps]
    for i, g in enumerate(gd):
        if g0 is not None:
            g.copy_(g0[i])
    nbytes = lib.la_noise_reg_scratch_bytes(_ints(res), len(res), B)
    assert nbytes > 0, lib.la_last_error()
    ws = guard.alloc(nbytes - short, dev, torch.float64)
    reg = guard.tensor([B, 3], torch.float64, dev, -1.0)
    rc = lib.la_noise_reg_f32(_ptrs(md), _ints(res), len(res), B, scale, weight, _ptrs(gd), int(g0 is not None), reg.data_ptr() + 16, 3,
                              ws.data_ptr(), nbytes - short, _s())
    if short:
        return rc
    assert rc == 0, lib.la_last_error()
    guard.check()
    reg = reg.cpu()
    assert (reg[:, :2] == -1.0).all()      # the other columns of the loss table stay untouched
    return reg[:, 2].clone(), [g.cpu().clone() for g in gd]


def _wrap_only(r, B, rs):
    """non-zero in the first and last row and column only: products of neighbours inside the frame and across the cyclic wrap"""
    n = torch.zeros([B, r, r])
    for sl in ((slice(None), 0), (slice(None), r - 1), (0, slice(None)), (r - 1, slice(None))):
        n[(slice(None),) + sl] = torch.from_numpy(rs.randn(B, r).astype(np.float32))
    return n


@pytest.mark.parametrize('r,B', nc.REG_SHAPES)
def test_noise_regulariser(dev, lib, r, B):
    """Loss and gradient, written and accumulated, of one map of 1 (4^2, 8^2) to 6 (256^2) levels.  Integer maps of one level: the two sums
    are integers, the means have at most 18 bits and their squares are exact, so float64 is matched bit for bit; with more levels a mean's
    square is rounded, and the rule applies.  A map that is non-zero on its frame only has its wrap terms checked by the same rule."""
    rs = np.random.RandomState(10 * r + B)
    if r <= 8:
        n = torch.from_numpy(rs.randint(-3, 4, (B, r, r)).astype(np.float32))
        reg, (g,) = _reg(lib, dev, [n], 0.5, 2.0)
        reg64, (g64,) = nc.regulariser([n.double()], 0.5, 2.0)
        assert torch.equal(reg, reg64) and torch.equal(g.double(), g64)
    for name, n in (('normal', torch.from_numpy(rs.randn(B, r, r).astype(np.float32))), ('frame', _wrap_only(r, B, rs))):
        for acc in (False, True):
            g0 = [torch.from_numpy(rs.randn(B, r, r).astype(np.float32))] if acc else None
            w = float(np.float32(nc.REG_WEIGHT))
            reg, (g,) = _reg(lib, dev, [n], nc.REG_WEIGHT, w, g0)
            reg2, (g2,) = _reg(lib, dev, [n], nc.REG_WEIGHT, w, g0)
            assert torch.equal(reg, reg2) and torch.equal(g, g2)
            reg64, (g64,) = nc.regulariser([n.double()], nc.REG_WEIGHT, w)
            reg32, (g32,) = nc.regulariser([n], nc.REG_WEIGHT, w)
            if acc:
                g64, g32 = g64 + g0[0].double(), g32 + g0[0]
            assert float(reg64.min()) > 0
            lc.check(f'reg  {name} r {r} B {B} acc {acc}', reg, reg64, reg32)
            lc.check(f'greg {name} r {r} B {B} acc {acc}', g, g64, g32)


def test_noise_regulariser_table_of_mixed_resolutions(dev, lib):
    """One call over maps of 4, 16, 8, 64, 32 (the level launches cover maps with 1 to 4 levels at once); the workspace size the entry
    reports is accepted with intact guard bands around it and every output, and 64 bytes fewer are refused."""
    rs = np.random.RandomState(77)
    B, res = 3, (4, 16, 8, 64, 32)
    maps = [torch.from_numpy(rs.randn(B, r, r).astype(np.float32)) for r in res]
    w = float(np.float32(3.0))
    for pattern in ('ones', 'bytes'):
        reg, g = _reg(lib, dev, maps, 3.0, w, guard=Guarded(pattern))
        reg64, g64 = nc.regulariser([m.double() for m in maps], 3.0, w)
        reg32, g32 = nc.regulariser(maps, 3.0, w)
        lc.check(f'reg table {pattern}', reg, reg64, reg32)
        for r, a, b, c in zip(res, g, g64, g32):
            lc.check(f'greg table r {r} {pattern}', a, b, c)
    assert _reg(lib, dev, maps, 3.0, w, short=64) == -3 and b'workspace too small' in lib.la_last_error()


# ------------------------------------------------------------------------------------------------------------ the noise tail
def _noise_tail(lib, dev, n, m, v, g, step, lr):
    res, B = [t.shape[-1] for t in n], n[0].shape[0]
    guard = Guarded('ones')
    dev_t = {k: [guard.tensor(t.shape, torch.float32, dev, 0.0) for t in ts] for k, ts in (('n', n), ('m', m), ('v', v), ('g', g))}
    for k, ts in (('n', n), ('m', m), ('v', v), ('g', g)):
        for d, t in zip(dev_t[k], ts):
            d.copy_(t)
    nbytes = lib.la_proj_noise_tail_scratch_bytes(_ints(res), len(res), B)
    assert nbytes > 0
    ws = guard.alloc(nbytes, dev, torch.float64)
    rc = lib.la_proj_noise_tail_f32(_ptrs(dev_t['g']), _ptrs(dev_t['n']), _ptrs(dev_t['m']), _ptrs(dev_t['v']), _ints(res), len(res), B, step, lr,
                                    0.9, 0.999, 1e-8, ws.data_ptr(), nbytes, _s())
    assert rc == 0, lib.la_last_error()
    guard.check()
    return [[t.cpu().clone() for t in dev_t[k]] for k in 'nmv']


@pytest.mark.parametrize('r,B', nc.TAIL_SHAPES)
def test_noise_tail_kernel(dev, lib, r, B):
    """Step 1 from zero moments and step 7 from non-zero ones: one chunk (r <= 32) and 64 chunks per sample (256^2).  The result has mean 0
    and mean square 1 to float32 rounding; a map of equal values with equal gradients comes out as zeros."""
    rs = np.random.RandomState(100 * r + B)
    for step in (1, 7):
        n = torch.from_numpy(rs.randn(B, r, r).astype(np.float32))
        g = torch.from_numpy(rs.randn(B, r, r).astype(np.float32))
        m = torch.from_numpy((0.1 * rs.randn(B, r, r)).astype(np.float32)) if step > 1 else torch.zeros([B, r, r])
        v = torch.from_numpy((0.1 * rs.randn(B, r, r) ** 2).astype(np.float32)) if step > 1 else torch.zeros([B, r, r])
        lr = float(np.float32(0.03 * step))
        got = [x[0] for x in _noise_tail(lib, dev, [n], [m], [v], [g], step, lr)]
        again = [x[0] for x in _noise_tail(lib, dev, [n], [m], [v], [g], step, lr)]
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        r64 = nc.noise_tail(n.double(), m.double(), v.double(), g.double(), step, lr)
        r32 = nc.noise_tail(n, m, v, g, step, lr)
        for name, a, b, c in zip('nmv', got, r64, r32):
            lc.check(f'tail {name} r {r} B {B} step {step}', a, b, c)
        mean, ms = got[0].double().mean((1, 2)), got[0].double().square().mean((1, 2))
        print('mean', mean.tolist(), 'mean square - 1', (ms - 1).tolist())
        # every element is rounded to float32 once: |mean| <= 2^-24 max|n|, |mean square - 1| <= 2^-23 (+ the rounding of the sums)
        assert float(mean.abs().max()) <= 2.0 ** -24 * float(got[0].abs().max()) and float((ms - 1).abs().max()) <= 2.0 ** -22
    flat = torch.full([B, r, r], 0.75)
    out = _noise_tail(lib, dev, [flat], [torch.zeros_like(flat)], [torch.zeros_like(flat)], [torch.full([B, r, r], 2.0)], 1, 0.05)[0][0]
    assert torch.equal(out, torch.zeros_like(out))


def test_noise_tail_table_of_mixed_resolutions(dev, lib):
    rs = np.random.RandomState(9)
    B, res = 3, (4, 64, 8, 32)
    n, g = ([torch.from_numpy(rs.randn(B, r, r).astype(np.float32)) for r in res] for _ in range(2))
    m = [torch.from_numpy((0.1 * rs.randn(B, r, r)).astype(np.float32)) for r in res]
    v = [torch.from_numpy((0.1 * rs.randn(B, r, r) ** 2).astype(np.float32)) for r in res]
    got = _noise_tail(lib, dev, n, m, v, g, 3, 0.05)
    for i, r in enumerate(res):
        r64 = nc.noise_tail(n[i].double(), m[i].double(), v[i].double(), g[i].double(), 3, 0.05)
        r32 = nc.noise_tail(n[i], m[i], v[i], g[i], 3, 0.05)
        for k, name in enumerate('nmv'):
            lc.check(f'tail table {name} r {r}', got[k][i], r64[k], r32[k])


# ------------------------------------------------------------------------------------------------------------ the synthesis backward pass
def _engine(dev, G, max_batch, precision, clamp=None):
    from latentaugment_amd.synthesis import SynthesisEngine
    if clamp is not None:
        return SynthesisEngine(G.synthesis.state_dict(), dev, max_batch, conv_clamp=clamp, precision=precision)
    return SynthesisEngine.from_generator(G, dev, max_batch, precision=precision)


def _synth_inputs(G, B, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn([B, G.w_dim], generator=g)
    with torch.no_grad():
        ws = G.mapping(z, None, truncation_psi=1.0).float()
    maps = [torch.randn([B, r, r], generator=g) for r in nc.layer_resolutions(G)]
    g_img = torch.randn([B, G.img_channels, G.img_resolution, G.img_resolution], generator=g)
    return ws, maps, g_img


def _check_noise_grads(tag, eng, dev, G, ws, maps, g_img):
    """dws bit-identical to la_synth_backward, every gn against float64 autograd of the oracle"""
    md = [None if ns == 0.0 else m.to(dev) for m, ns in zip(maps, eng.noise_strengths)]
    eng.forward(ws.to(dev), noise_mode='random', noises=md)
    dws0 = eng.backward(g_img.to(dev)).clone()
    eng.forward(ws.to(dev), noise_mode='random', noises=md)
    want = [torch.full(m.shape, float('nan'), device=dev) for m in maps]
    dws1, gns = eng.backward(g_img.to(dev), noise_grads=want)
    assert torch.equal(dws0, dws1), tag
    _, w64, g64 = nc.synth_noise_grads(G, ws, maps, g_img, torch.float64)
    _, w32, g32 = nc.synth_noise_grads(G, ws, maps, g_img, torch.float32)
    lc.check(f'dws {tag}', dws1.cpu(), w64, w32)
    for li, (a, b, c, ns) in enumerate(zip(gns, g64, g32, eng.noise_strengths)):
        if ns == 0.0:
            assert torch.equal(a.cpu(), torch.zeros_like(maps[li])) and float(b.abs().max()) == 0.0, (tag, li)
        else:
            assert float(b.abs().max()) > 0
            lc.check(f'gn[{li}] {tag}', a.cpu(), b, c)
    return gns


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
@pytest.mark.parametrize('B', [1, 3])
def test_synth_backward_noise(dev, lib, B, precision):
    from latentaugment_amd import _lib
    G = pj.generator()
    eng = _engine(dev, G, 3, precision)
    with pytest.raises(_lib.LatentAugHipError, match='no forward pass'):
        eng.backward(torch.zeros([B, 2, 32, 32], device=dev), noise_grads=True)
    ws, maps, g_img = _synth_inputs(G, B, 40 + B)
    _check_noise_grads(f'TINY B {B} {precision}', eng, dev, G, ws, maps, g_img)
    # the gradient does not depend on the noise mode of the forward pass beyond the image it made: const noise, gradients asked for
    eng.forward(ws.to(dev), noise_mode='const')
    dws, gns = eng.backward(g_img.to(dev), noise_grads=True)
    assert all(g is not None and torch.isfinite(g).all() for g in gns)
    # refused while a window is set
    _lib.check(lib.la_synth_set_row_window(eng.handle, 8, 16), 'la_synth_set_row_window')
    try:
        eng.forward(ws.to(dev), noise_mode='const')
        with pytest.raises(_lib.LatentAugHipError, match='window'):
            eng.backward(g_img.to(dev), noise_grads=True)
        eng.backward(g_img.to(dev))      # (the plain pass still runs)
    finally:
        _lib.check(lib.la_synth_set_row_window(eng.handle, 0, 0), 'la_synth_set_row_window')


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
def test_synth_backward_noise_with_a_layer_without_noise(dev, precision):
    """A copy of the generator with the strength of b8.conv1 (layer 2) set to 0: a NULL entry is accepted, a tensor gets zeros"""
    G = copy.deepcopy(pj.generator())
    with torch.no_grad():
        G.synthesis.b8.conv1.noise_strength.fill_(0.0)
    eng = _engine(dev, G, 3, precision)
    assert eng.noise_strengths[2] == 0.0 and all(ns != 0.0 for i, ns in enumerate(eng.noise_strengths) if i != 2)
    ws, maps, g_img = _synth_inputs(G, 3, 50)
    gns = _check_noise_grads(f'TINY strength 0 {precision}', eng, dev, G, ws, maps, g_img)
    md = [None if ns == 0.0 else m.to(dev) for m, ns in zip(maps, eng.noise_strengths)]
    eng.forward(ws.to(dev), noise_mode='random', noises=md)
    _, some = eng.backward(g_img.to(dev), noise_grads=[True, None, None, True, False, None, True])
    assert [g is None for g in some] == [False, True, True, False, True, True, False]
    assert all(torch.equal(some[i], gns[i]) for i in (0, 3, 6))


# R8-imgc1 is the smallest case of synth_cases.SYNTH_CASES with a conv0 layer.  la_synth_plan_query (test_noise_cases_cpu.py) reports for it
# in f32 every seam as a kernel, in f16x2 the conv0 seam of block 8 fused into its conv1's backward and the conv1 seam of block 4 fused into
# the up layer's backward: G1 and G0 are read behind both kinds of producer.  R16-noise-mixed adds layers without noise in both.
@pytest.mark.parametrize('mode', ['f32', 'f16x2'])
@pytest.mark.parametrize('name', ['R8-imgc1', 'R16-noise-mixed'])
def test_synth_backward_noise_behind_kernel_and_fused_seams(dev, name, mode):
    case = sc.SYNTH_BY_NAME[name]
    G, ws, g_img = case.build()
    eng = _engine(dev, G, case.max_batch, mode, clamp=case.clamp)
    assert eng.noise_strengths == case.noise
    maps = [torch.randn([case.B, r, r], generator=torch.Generator().manual_seed(5 + r)) for r in nc.layer_resolutions(G)]
    _check_noise_grads(f'{name} {mode}', eng, dev, G, ws, maps, g_img)


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
def test_autograd_wrapper_returns_noise_gradients(dev, precision):
    from latentaugment_amd.synthesis import synthesis
    G = pj.generator()
    eng = _engine(dev, G, 3, precision)
    ws, maps, g_img = _synth_inputs(G, 3, 60)
    md = [m.to(dev) for m in maps]
    eng.forward(ws.to(dev), noise_mode='random', noises=md)
    dws, gns = eng.backward(g_img.to(dev), noise_grads=True)
    w = ws.to(dev).requires_grad_(True)
    nz = [m.clone().requires_grad_(i % 2 == 0) for i, m in enumerate(md)]
    img = synthesis(eng, w, 'random', nz)
    (img * g_img.to(dev)).sum().backward()
    assert torch.equal(w.grad, dws)
    for i, (t, g) in enumerate(zip(nz, gns)):
        assert (t.grad is None) if i % 2 else torch.equal(t.grad, g), i
    # no entry requires grad: the existing path, the same image and latent gradient
    w2 = ws.to(dev).requires_grad_(True)
    img2 = synthesis(eng, w2, 'random', md)
    (img2 * g_img.to(dev)).sum().backward()
    assert torch.equal(img2, img) and torch.equal(w2.grad, dws)


# ------------------------------------------------------------------------------------------------------------ one step, teacher-forced
def _projector(dev, case, precision, max_batch=3):
    from latentaugment_amd.projector import Projector
    net = types.SimpleNamespace(ops=case.ops, pre_scale=case.pre_scale, pre_shift=case.pre_shift)
    return Projector(pj.generator(), net, dev, max_batch, precision=precision, lpips_res=pj.TINY['img_resolution'] // case.k)


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
@pytest.mark.parametrize('space,w_pix,k,affine', nc.STEP_CASES)
def test_one_step_with_noise_teacher_forced(dev, monkeypatch, space, w_pix, k, affine, precision):
    """Step t = 3 (1-based Adam step 4, from non-zero moments) of project(optimize_noise=True) from a given state -- the latent the device
    draws, maps of the library's stream, moments -- against the float64 restatement from the same state: the three loss columns, w after
    the latent tail, the maps and their moments after the noise tail.  Every workspace between guard bands."""
    from latentaugment_amd import _lib
    from latentaugment_amd.projector import NoiseMaps
    guard = Guarded('ones')
    monkeypatch.setattr(_lib, 'workspace', guard.alloc)
    case = pj.make_case(space, w_pix, k, affine)
    proj = _projector(dev, case, precision)
    G, tgt = pj.generator(), pj.targets()
    B, t = tgt.shape[0], 3
    avg, std = pj.w_stats()
    rs = np.random.RandomState(17)
    w = (torch.from_numpy(avg).float().reshape(1, 1, -1) + torch.from_numpy((0.1 * rs.randn(B, case.L, G.w_dim)).astype(np.float32)))
    m = torch.from_numpy((0.01 * rs.randn(B, case.L, G.w_dim)).astype(np.float32))
    v = torch.from_numpy((0.01 * rs.randn(B, case.L, G.w_dim) ** 2).astype(np.float32))
    maps = NoiseMaps(proj.synth, B, case.seed, 0)
    n0 = [x.cpu() for x in maps.n]
    ref0 = nc.initial_maps(B, case.seed)
    assert all(float((a - b).abs().max()) <= 1e-5 for a, b in zip(n0, ref0))      # (the normals of two float32 libraries: as the noise test allows)
    nm = [torch.from_numpy((1e-4 * rs.randn(*x.shape)).astype(np.float32)) for x in n0]
    nv = [torch.from_numpy((1e-4 * rs.randn(*x.shape) ** 2).astype(np.float32)) for x in n0]
    for dst, src in zip(maps.m + maps.v, nm + nv):
        dst.copy_(src)
    w_d, m_d, v_d = w.to(dev), m.to(dev), v.to(dev)
    ws = torch.empty_like(w_d)
    sigma = float(np.float32(pj.schedule(t, case.T, std)[1]))
    proj.step_tail(None, w_d, None, None, ws, 0, 0.0, sigma, case.seed, t, 0)
    at = ws.cpu()
    tgt_d = tgt.to(dev)
    tfeat = proj.target_features(tgt_d)
    loss = torch.zeros([B, 3], dtype=torch.float64, device=dev)
    dws, img = proj.loss_and_grad(ws, tgt_d, tfeat, w_pix, loss, maps, nc.REG_WEIGHT)
    lr = pj.schedule(t, case.T, std)[0]
    sigma1 = pj.schedule(t + 1, case.T, std)[1]
    proj.step_tail(dws, w_d, m_d, v_d, ws, t + 1, lr, sigma1, case.seed, t + 1, 0)
    proj.noise_tail(maps, t + 1, lr)
    guard.check()
    # the restatement from the same state; the next latent's normals are the device's own (ws - w) / sigma is not needed: w is compared
    zero = torch.zeros([B, case.L, G.w_dim], dtype=torch.float64)
    runs = []
    for dt in (torch.float64, torch.float32):
        runs.append(nc.step(case, w.to(dt), m.to(dt), v.to(dt), [x.to(dt) for x in n0], [x.to(dt) for x in nm], [x.to(dt) for x in nv], at.to(dt), tgt, t, dt,
                            n_next=zero))
    r64, r32 = runs
    tag = f'{case.name} {precision}'
    lc.check('d    ' + tag, loss[:, 0].cpu(), r64['loss'][:, 0], r32['loss'][:, 0])
    if w_pix > 0:
        lc.check('p    ' + tag, loss[:, 1].cpu(), r64['loss'][:, 1], r32['loss'][:, 1])
    else:
        assert float(loss[:, 1].abs().max()) == 0.0
    lc.check('reg  ' + tag, loss[:, 2].cpu(), r64['loss'][:, 2], r32['loss'][:, 2])
    lc.check('w    ' + tag, w_d.cpu(), r64['w'], r32['w'])
    for li in range(len(n0)):
        lc.check(f'map[{li}] ' + tag, maps.n[li].cpu(), r64['maps'][li], r32['maps'][li])
        lc.check(f'm[{li}]   ' + tag, maps.m[li].cpu(), r64['nm'][li], r32['nm'][li])
        lc.check(f'v[{li}]   ' + tag, maps.v[li].cpu(), r64['nv'][li], r32['nv'][li])


# ------------------------------------------------------------------------------------------------------------ project(), end to end
def test_project_with_noise_end_to_end(dev):
    """3 targets, 20 steps: two runs give the same bits; max_batch 2 and 3 give the same bits per sample; row0 shifts the streams; the
    returned maps are normalised; the shapes are as documented; without the flag nothing changes its shape."""
    case = pj.make_case('w', 0.1)
    tgt = pj.targets().to(dev)
    p3, p2 = _projector(dev, case, 'f16x2', 3), _projector(dev, case, 'f16x2', 2)
    a = p3.project(tgt, num_steps=20, w_pix=0.1, seed=4, optimize_noise=True)
    b = p3.project(tgt, num_steps=20, w_pix=0.1, seed=4, optimize_noise=True)
    c = p2.project(tgt, num_steps=20, w_pix=0.1, seed=4, optimize_noise=True)
    res = nc.layer_resolutions()
    assert a['loss'].shape == (20, 3, 3) and a['w'].shape == (3, p3.num_ws, p3.w_dim) and a['img'].shape == tgt.shape
    assert len(a['noises']) == len(res) and all(n.shape == (3, r, r) for n, r in zip(a['noises'], res))
    assert torch.isfinite(a['loss']).all() and float(a['loss'][:, :, 2].min()) > 0
    for other in (b, c):
        assert all(torch.equal(a[key], other[key]) for key in ('w', 'img', 'loss'))
        assert all(torch.equal(x, y) for x, y in zip(a['noises'], other['noises']))
    for n in a['noises']:
        n = n.double()
        assert float(n.mean((1, 2)).abs().max()) <= 2.0 ** -24 * float(n.abs().max()) and float((n.square().mean((1, 2)) - 1).abs().max()) <= 2.0 ** -22
    # the image is the one the optimised maps make
    img = p3.synth.forward(a['w'], noise_mode='random', noises=a['noises'])
    assert torch.equal(img, a['img'])
    # row0: sample 1 of a call at row0 = 0 is sample 0 of a call at row0 = 1
    d = p3.project(tgt[1:], num_steps=20, w_pix=0.1, seed=4, optimize_noise=True, row0=1)
    assert torch.equal(d['w'][0], a['w'][1]) and all(torch.equal(x[0], y[1]) for x, y in zip(d['noises'], a['noises']))
    e = p3.project(tgt[1:], num_steps=20, w_pix=0.1, seed=4, optimize_noise=True)
    assert not torch.equal(e['w'][0], a['w'][1])
    # the flag off: the result of the existing path
    f = p3.project(tgt, num_steps=20, w_pix=0.1, seed=4)
    assert f['loss'].shape == (20, 3, 2) and 'noises' not in f and not torch.equal(f['w'], a['w'])
