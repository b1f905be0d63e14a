"""Guard bands and poisoned contents for every caller-owned workspace ("Workspace contract").

The float64 sweeps ask whether the values in the output buffers are right.  This file asks the two questions they leave open:

  1. does a launch write outside what it was given?  Every workspace the package allocates goes through `_lib.workspace`; here
     tests/guarded_alloc.py stands in for it, so each one sits between two 4096-byte bands of 0xA5 that start exactly at its first and
     behind its last byte, and `check()` must find both intact after every call.  Outputs that a test hands over through ctypes sit in
     `guarded_tensor`s, pre-filled with a value no correct run leaves.
  2. does a result depend on what the workspace held before?  Each case runs once per pattern -- zeros, 0xFF bytes (NaN in every float
     format, -1 / the maximum as integers), seeded random bytes -- and every output must be the same BITS in all three.  A buffer that
     starts at zero hides a missing atomicMax reset, one that starts at 0xFF a missing atomicMin reset, hence more than one pattern.

No new oracle: the inputs are the seeded ones of the case tables in tests/, at the smallest case of each table that reaches each kernel
form (the reach tables of the sweep files say which).  No tolerance except the grid-sample gradient's, which sums with float atomics and
is compared within test_hip_grid_sample.atomic_sum_tol; everything else is equality of bits.  Entries that take `workspace_bytes` are
also handed 64 bytes less than their size entry reports: LA_ERR_WORKSPACE, and the outputs keep their pre-fill.  (The modulated-conv
entries are the exception the header documents: a workspace that holds the operand copy but not the slice partials is valid and selects
the direct kernels -- tested below as `ws short of the partials`, with the bands at that size.)

The synthesis engine clears its workspace at create, so its cases exercise the bands only; every other entry is shown independent of
the contents it was handed.

Found on the MI355X: no band was touched and no output depended on the pattern; la_latent_opt_set_lpips refused a short workspace with
LA_ERR_ARG instead of LA_ERR_WORKSPACE (fixed).  Three scratch mutations of the library -- an edge test, a re-arm and the clear of the
Adam moments removed -- make 3, 18 and 7 of these tests fail ("Workspace contract").
Wall time of the file on the MI355X: 6.5 s for 133 tests (slowest test 0.8 s, the first conv2d_resample call of the process).
"""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as ga  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_WORKSPACE = -3
MODES = ['f32', 'bf16x3', 'f16x2']
SHORT = 64


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


def _err(lib):
    m = lib.la_last_error()
    return m.decode() if m else ''


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8)


def _as_tensors(out):
    return {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).detach().cpu() for k, v in out.items() if v is not None}


def _first_difference(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f'shape / dtype {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}'
    n = a.element_size()
    diff = (_bits(a).reshape(-1, n) != _bits(b).reshape(-1, n)).any(dim=1).nonzero().reshape(-1)
    if diff.numel() == 0:
        return None
    i = int(diff[0])
    return f'{diff.numel()} of {a.numel()} elements differ, first at flat index {i}: {a.reshape(-1)[i].item()!r} against {b.reshape(-1)[i].item()!r}'


def across_patterns(monkeypatch, run, name, compare=None):
    """run(g) -> {key: tensor} once per pattern with `_lib.workspace` replaced by g.alloc (run calls g.check() between its own calls where
    it makes several; one more check follows here, after a synchronise).  Every output must be the same bits under every pattern;
    `compare(key, a, b)` -> message or None replaces that for the keys it knows (it returns NotImplemented for the others)."""
    from latentaugment_amd import _lib
    res = {}
    for pattern in ga.PATTERNS:
        g = Guarded(pattern)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'workspace', g.alloc)
            out = run(g)
            torch.cuda.synchronize()
        g.check()
        res[pattern] = _as_tensors(out)
    base = res['zeros']
    assert base, name
    bad = []
    for pattern in ga.PATTERNS[1:]:
        assert res[pattern].keys() == base.keys(), name
        for k in base:
            msg = compare(k, base[k], res[pattern][k]) if compare else NotImplemented
            if msg is NotImplemented:
                msg = _first_difference(base[k], res[pattern][k])
            if msg:
                bad.append(f'{name}: {k} under pattern {pattern!r} is not what it is under zeros: {msg}')
    assert not bad, '\n'.join(bad)
    return base


class short_size:
    """Within the block, the size entry `entry` of the library reports 64 bytes less: a package call that sizes its workspace by it then
    hands over a short (guarded) buffer with the short byte count, which the library must refuse with LA_ERR_WORKSPACE before any launch."""

    def __init__(self, lib, entry, unit=1):
        self.lib, self.entry, self.unit = lib, entry, unit

    def __enter__(self):
        self.real = getattr(self.lib, self.entry)
        self.full = []

        def less(*a):
            n = self.real(*a)
            self.full.append(n)
            return n - SHORT // self.unit if n * self.unit > SHORT else n
        setattr(self.lib, self.entry, less)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.entry, self.real)


def refused_short(monkeypatch, lib, entry, call, unit=1):
    """`call()` (a package call) with the size entry 64 bytes short: LA_ERR_WORKSPACE (code -3 in the raised error), bands intact."""
    from latentaugment_amd import _lib
    g = Guarded('ones')
    with monkeypatch.context() as m:
        m.setattr(_lib, 'workspace', g.alloc)
        with short_size(lib, entry, unit) as sh:
            with pytest.raises(_lib.LatentAugHipError, match=r'code -3'):
                call()
            assert sh.full and sh.full[0] * unit > SHORT, f'{entry}: {sh.full} bytes leave nothing to take 64 from'
    torch.cuda.synchronize()
    g.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# the allocator itself on device memory (the CPU file proves the rest)

def test_guarded_allocator_on_the_device(dev):
    g = Guarded('bytes')
    t = g.alloc(1000, dev, torch.float32)
    o = g.tensor([3, 5], torch.float64, dev, -7.0)
    assert t.is_cuda and t.numel() == 250 and t.data_ptr() % 256 == 0 and bool((o == -7.0).all())
    t.fill_(1.0)
    o.zero_()
    g.check()
    g.records[0][0][ga.GUARD + 1000] = 0
    with pytest.raises(ga.GuardError, match='payload offset 1000'):
        g.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# synthesis engine: the bands only (create clears the workspace)

def _synth_engine(dev, case, G, mode):
    from latentaugment_amd.synthesis import SynthesisEngine
    return SynthesisEngine(G.synthesis.state_dict(), dev, case.max_batch, conv_clamp=case.clamp, precision=mode)


_SYNTH_BUILT = {}


def _synth_inputs(name):
    import synth_cases as sc
    if name not in _SYNTH_BUILT:
        _SYNTH_BUILT[name] = sc.SYNTH_BY_NAME[name].build()
    return sc.SYNTH_BY_NAME[name], _SYNTH_BUILT[name]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['R4-only', 'R16-imgc3-ch12-20-8', 'R64-rgbfuse-imgc3'])
def test_synthesis_engine(dev, lib, monkeypatch, name, mode):
    case, (G, ws, g_img) = _synth_inputs(name)

    def run(g):
        eng = _synth_engine(dev, case, G, mode)
        g.check()
        img = eng.forward(ws.to(dev), noise_mode='const')
        g.check()
        dws = eng.backward(g_img.to(dev))
        g.check()
        return dict(img=img, dws=dws, dstyles=eng.style_grads(case.B).clone(), styles=eng.styles(case.B).clone())

    across_patterns(monkeypatch, run, f'synth {name} {mode}')
    if mode == 'f32':
        refused_short(monkeypatch, lib, 'la_synth_workspace_bytes', lambda: _synth_engine(dev, case, G, mode))


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x2'])
@pytest.mark.parametrize('cols', [False, True], ids=['rows', 'rows-cols'])
def test_synthesis_engine_first_pass_windowed(dev, lib, monkeypatch, cols, mode):
    """the first pass on a fresh engine is the windowed one: nothing outside the window was ever written by a pass"""
    import synth_cases as sc
    from latentaugment_amd import _lib
    case, (G, ws, g_img) = _synth_inputs('R64-rgbfuse-imgc3')
    lo, hi = sc.window_of(case.R)
    gw = sc.windowed_g_img(case, g_img, cols)

    def run(g):
        eng = _synth_engine(dev, case, G, mode)
        _lib.check(lib.la_synth_set_row_window(eng.handle, lo, hi), 'la_synth_set_row_window')
        if cols:
            _lib.check(lib.la_synth_set_col_window(eng.handle, lo, hi), 'la_synth_set_col_window')
        img = eng.forward(ws.to(dev), noise_mode='const')
        g.check()
        dws = eng.backward(gw.to(dev))
        g.check()
        clo, chi = (lo, hi) if cols else (0, case.R)
        return dict(img=img[:, :, lo:hi, clo:chi].clone(), dws=dws, dstyles=eng.style_grads(case.B).clone())

    across_patterns(monkeypatch, run, f'synth windowed cols={cols} {mode}')


# ---------------------------------------------------------------------------------------------------------------------------------
# discriminator and feature engines

def _disc_engine(dev, case, D, mode):
    from latentaugment_amd.synthesis import DiscriminatorEngine
    return DiscriminatorEngine(D, dev, max_batch=case.max_batch, conv_clamp=case.clamp, precision=mode, mbstd_group_size=case.group)


_ENGINE_BUILT = {}


def _built(case):
    if case.name not in _ENGINE_BUILT:
        _ENGINE_BUILT[case.name] = case.build()
    return _ENGINE_BUILT[case.name]


def _disc_passes(lib, eng, dev, img, dlogits, g):
    """forward, backward, backward-accumulate onto a preloaded gradient"""
    logits = eng.forward(img.to(dev))
    g.check()
    gx = eng.backward(dlogits.to(dev))
    g.check()
    acc = g.tensor(list(gx.shape), torch.float32, dev, 0.0)
    acc.copy_(torch.arange(gx.numel(), dtype=torch.float32).reshape(gx.shape) % 7 - 3)
    dl = dlogits.to(dev).reshape(-1).contiguous()
    assert lib.la_disc_backward(eng.handle, _p(dl), _p(acc), 1, _s()) == 0, _err(lib)
    g.check()
    return logits, gx, acc


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['R8', 'imgc3', 'R128'])
def test_discriminator_engine(dev, lib, monkeypatch, name, mode):
    """R8: the smallest guarded case; imgc3: R16, three channels; R128: R * R > 4096, the halo forms and the fused FromRGB backward of f16x2"""
    import engine_cases as ec
    case = ec.DISC_BY_NAME[name]
    D, img, dlogits = _built(case)

    def run(g):
        eng = _disc_engine(dev, case, D, mode)
        logits, gx, acc = _disc_passes(lib, eng, dev, img, dlogits, g)
        return dict(logits=logits, gx=gx, acc=acc)

    across_patterns(monkeypatch, run, f'disc {name} {mode}')
    if mode == 'f32' and name == 'R8':
        refused_short(monkeypatch, lib, 'la_disc_workspace_bytes', lambda: _disc_engine(dev, case, D, mode))


@pytest.mark.parametrize('mode', MODES)
def test_discriminator_shrinking_batch_on_one_poisoned_workspace(dev, lib, monkeypatch, mode):
    import engine_cases as ec
    case = ec.DISC_SHRINK
    D, img, dlogits = _built(case)
    gen = torch.Generator().manual_seed(78)
    big = torch.randn([case.max_batch, case.imgc, case.R, case.R], generator=gen) * ec.DISC_SHRINK_BIG
    dlb = torch.randn([case.max_batch, 1], generator=gen) * ec.DISC_SHRINK_BIG

    def run(g):
        eng = _disc_engine(dev, case, D, mode)
        lb, gb, _ = _disc_passes(lib, eng, dev, big, dlb, g)
        logits, gx, acc = _disc_passes(lib, eng, dev, img, dlogits, g)
        return dict(big_logits=lb, big_gx=gb, logits=logits, gx=gx, acc=acc)

    across_patterns(monkeypatch, run, f'disc shrinking {mode}')


def _feat_engine(dev, ops, in_ch, res, max_batch, mode):
    from latentaugment_amd.synthesis import FeatureEngine
    return FeatureEngine(ops, dev, in_res=res, max_batch=max_batch, in_ch=in_ch, precision=mode)


def _feat_passes(eng, dev, x, gfeat, g):
    f = eng.forward(x.to(dev))
    g.check()
    gx = eng.backward(gfeat.to(dev))
    g.check()
    return f, gx


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['tap-only-C1-res8', 'cin4-in4-N1', 'odd-res-28'])
def test_feature_engine(dev, lib, monkeypatch, name, mode):
    """the smallest guarded case (a lone tap), the smallest with a conv (N 1 of max_batch 8), and the largest grid of the table (28 x 28,
    three convs behind pools)"""
    import engine_cases as ec
    case = ec.FEAT_BY_NAME[name]
    ops, x, gfeat = _built(case)

    def run(g):
        eng = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
        f, gx = _feat_passes(eng, dev, x, gfeat, g)
        return dict(f=f, gx=gx)

    across_patterns(monkeypatch, run, f'feat {name} {mode}')
    if mode == 'f32' and name == 'cin4-in4-N1':
        refused_short(monkeypatch, lib, 'la_feat_workspace_bytes', lambda: _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode))


@pytest.mark.parametrize('mode', MODES)
def test_feature_shrinking_batch_on_one_poisoned_workspace(dev, monkeypatch, mode):
    import engine_cases as ec
    case = ec.FEAT_SHRINK
    ops, x, gfeat = _built(case)
    gen = torch.Generator().manual_seed(77)
    xb = torch.randn([case.max_batch, case.in_ch, case.res, case.res], generator=gen) * ec.FEAT_SHRINK_BIG
    gb = torch.randn([case.max_batch, gfeat.shape[1]], generator=gen) * ec.FEAT_SHRINK_BIG

    def run(g):
        eng = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, mode)
        fb, gxb = _feat_passes(eng, dev, xb, gb, g)
        f, gx = _feat_passes(eng, dev, x, gfeat, g)
        return dict(big_f=fb, big_gx=gxb, f=f, gx=gx)

    across_patterns(monkeypatch, run, f'feat shrinking {mode}')


@pytest.mark.parametrize('mode', ['f32', 'f16x2'])
def test_lpips_pair_workspace(dev, lib, monkeypatch, mode):
    """FeatureEngine.pair_distance: la_feat_pair_workspace_bytes, a chunk of max_batch // 2 pairs and a ragged last one"""
    import engine_cases as ec
    case = ec.FEAT_BY_NAME['tap-between']          # conv, tap, conv, tap at 10 x 10
    ops, _, _ = _built(case)
    gen = torch.Generator().manual_seed(5)
    x, y = (torch.randn([3, case.in_ch, case.res, case.res], generator=gen) for _ in range(2))

    def run(g):
        eng = _feat_engine(dev, ops, case.in_ch, case.res, 4, mode)
        d = eng.pair_distance(x.to(dev), y.to(dev))
        g.check()
        return dict(dist=d)

    across_patterns(monkeypatch, run, f'lpips pair {mode}')
    if mode == 'f32':          # (8 pairs of the 28 x 28, three-tap list: the first size of the table whose workspace exceeds 64 bytes)
        big = ec.FEAT_BY_NAME['odd-res-28']
        xb, yb = (torch.randn([8, big.in_ch, big.res, big.res], generator=gen).to(dev) for _ in range(2))
        eng = _feat_engine(dev, _built(big)[0], big.in_ch, big.res, 16, mode)
        refused_short(monkeypatch, lib, 'la_feat_pair_workspace_bytes', lambda: eng.pair_distance(xb, yb))


# ---------------------------------------------------------------------------------------------------------------------------------
# detector list and la_fc

@pytest.mark.parametrize('name', ['vgg-like-relu', 'avgpool-one-fc'])
def test_detector_list(dev, monkeypatch, name):
    import detector_cases as dc
    case = next(c for c in dc.DET_CASES if c.name == name)
    ops, x = case.build()

    def run(g):
        eng = _feat_engine(dev, ops, case.in_ch, case.res, case.max_batch, 'f32')
        f = eng.forward(x.to(dev))
        g.check()
        return dict(f=f)

    across_patterns(monkeypatch, run, f'detector {name}')


@pytest.mark.parametrize('N,K,O', [(5, 37, 6), (33, 230, 130), (64, 256, 128)], ids=['scalar-loads-one-slice', 'scalar-loads-slices', 'whole-tiles'])
def test_fc(dev, lib, monkeypatch, N, K, O):
    """la_fc_bias_act_f32: K % 4 != 0 (the unaligned scalar-load form) with one K slice and with several, and whole tiles"""
    import detector_cases as dc
    x, w, b = (t.to(dev) for t in dc.fc_inputs(N, K, O))
    need = lib.la_fc_workspace_bytes(N, K, O)
    assert need > SHORT

    def run(g):
        y = g.tensor([N, O], torch.float32, dev, -777.0)
        ws = g.alloc(need, dev)
        assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y), N, K, O, 2, _p(ws), need, _s()) == 0, _err(lib)
        g.check()
        y2 = g.tensor([N, O], torch.float32, dev, -777.0)
        assert lib.la_fc_bias_act_f32(_p(x), _p(w), _p(b), _p(y2), N, K, O, 2, _p(ws), need - SHORT, _s()) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((y2 == -777.0).all())
        assert not bool((y == -777.0).any())
        return dict(y=y)

    across_patterns(monkeypatch, run, f'fc {N}x{K}x{O}')


# ---------------------------------------------------------------------------------------------------------------------------------
# modulated-conv layer entries (the workspace and the bf16 pack buffers are both guarded)

MODCONV = ['sk_r4_b3', 'fl_r35', 'ha_r64_m28', 'uf_r4', 'uf_r8', 'sk_c16', 'fl_r36', 'ha_r64_m32', 'ub_r4', 'ub_r8']
_MODCONV_T = {}


def _modconv_tensors(name):
    import modconv_cases as mc
    if name not in _MODCONV_T:
        c = mc.BY_NAME[name]
        _MODCONV_T[name] = (c, mc.make_tensors(c, mc.CASES.index(c)))
    return _MODCONV_T[name]


@pytest.mark.parametrize('prec', [0, 1, 2, 3])
@pytest.mark.parametrize('name', MODCONV)
def test_modconv_entries(dev, lib, monkeypatch, name, prec):
    """per entry the smallest split-K, flat and halo case (up = 1: uf_* / ub_*); where the plan splits K also with a workspace one float
    short of the slice partials, which selects the direct kernels"""
    import modconv_cases as mc
    import test_hip_modconv_shapes as tms
    from latentaugment_amd import _lib
    c, t = _modconv_tensors(name)
    o = c['opts']
    B, cin, cout, res = c['B'], c['cin'], c['cout'], c['res']
    up = c['entry'].startswith('up2')
    plans = [('full ws', mc.plan(c, prec, True)['ws_bytes'])]
    if mc.splits(c, prec):
        plans.append(('ws short of the partials', mc.plan(c, prec, False)['ws_bytes']))

    def run(g):
        d = {k: (v.to(dev).contiguous() if v is not None else None) for k, v in t.items()}
        for key, n, pad in (('s', cin, o['s_pad']), ('d', cout, o['d_pad'])):
            if d.get(key) is not None and pad:
                p = torch.full([B, n + pad], float('nan'), device=dev)
                p[:, :n] = d[key]
                d[key] = p
        d['wf'] = g.tensor([9, cin, cout], torch.float32, dev, float('nan'))
        d['wb'] = g.tensor([9, cout, cin], torch.float32, dev, float('nan'))
        _lib.check(lib.la_pack_conv_weights_f32(_p(d['w']), _p(d['wf']), _p(d['wb']), None, cout, cin, 9, _s()))
        for key, tr in (('wqf', 0), ('wqb', 1)):
            d[key] = g.alloc(lib.la_modconv_bf16_pack_bytes(cin, cout, tr, 3), dev)
            _lib.check(lib.la_pack_conv_weights_bf16_f32(_p(d['w']), _p(d[key]), cout, cin, 9, tr, 3, _s()))
        g.check()
        res_out = {}
        for tag, ws_bytes in plans:
            out = {}
            if up:
                out['scratch'] = g.tensor([B * cout * (res + 1) * (res + 1)], torch.float32, dev, float('nan'))
            if c['entry'] in ('fwd', 'up2_fwd'):
                out['y'] = g.tensor([B, cout, res, res], torch.float32, dev, float('nan'))
            else:
                rin = res // 2 if up else res
                out['gx'] = g.tensor([B, cin, rin, rin], torch.float32, dev, float('nan'))
                out['ds_part'] = g.tensor([B, cin, lib.la_modconv_ds_tiles(rin)], torch.float32, dev, float('nan'))
            ws = g.alloc(max(ws_bytes, 16), dev)
            _lib.check(tms.call_entry(lib, c, d, prec, ws, ws_bytes, out, dev), f'{name} {tag}')
            g.check()
            for k, v in out.items():
                if k != 'scratch':
                    assert bool(torch.isfinite(v).all()), (name, prec, tag, k, 'an element that no kernel wrote')
                    res_out[f'{tag}: {k}'] = v
        return res_out

    across_patterns(monkeypatch, run, f'modconv {name} prec {prec}')


# ---------------------------------------------------------------------------------------------------------------------------------
# conv2d / conv_transpose2d / weight gradient

def _conv_dims(x, w, stride, py, px):
    B, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * py - kh) // stride + 1, (W + 2 * px - kw) // stride + 1
    return (B, Cin, H, W, Cout, kh, kw, Ho, Wo, stride), (B, Cout, Ho, Wo)


@pytest.mark.parametrize('name', ['same3x3', 'k5', 'small_grid_splitk'])
def test_conv2d_entries(dev, lib, monkeypatch, name):
    """la_conv2d_f32 and la_conv2d_wgrad_f32 with la_conv2d_workspace_bytes: the smallest engine-path case, the smallest direct-path case
    (25 taps) and the engine's split-K / sliced weight gradient (64 channels on an 8 x 8 grid)"""
    import conv2d_op_cases as cc
    import test_hip_conv2d_op as tco
    c = cc.BY_NAME[name]
    x, w, dy, f, kw, call = tco.case_tensors(c, 3)
    assert call['branch'] == 'plain' and not call['transpose']
    dims, ys = _conv_dims(x, w, 1, call['py'], call['px'])
    assert tuple(dy.shape) == ys
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)

    def run(g):
        out = {}
        for op, key, shape, a, b in ((0, 'y', ys, xd, wd), (1, 'dw', tuple(w.shape), xd, dyd)):
            need = lib.la_conv2d_workspace_bytes(op, *dims, 1, 0)
            fn = lib.la_conv2d_f32 if op == 0 else lib.la_conv2d_wgrad_f32
            res = g.tensor(shape, torch.float32, dev, -777.0)
            ws = g.alloc(max(need, 16), dev)
            assert fn(_p(a), _p(b), _p(res), _p(ws), need, *dims, call['py'], call['px'], 1, 1, 0, _s()) == 0, _err(lib)
            g.check()
            assert not bool((res == -777.0).any()), key
            out[key] = res
            if need > SHORT:
                res2 = g.tensor(shape, torch.float32, dev, -777.0)
                assert fn(_p(a), _p(b), _p(res2), _p(ws), need - SHORT, *dims, call['py'], call['px'], 1, 1, 0, _s()) == LA_ERR_WORKSPACE, (key, _err(lib))
                torch.cuda.synchronize()
                assert bool((res2 == -777.0).all()), key
        return out

    across_patterns(monkeypatch, run, f'conv2d {name}')


@pytest.mark.parametrize('name', ['same3x3', 'up2_3x3', 'down2_3x3', 'k5', 'small_grid_splitk'])
def test_conv2d_resample_op(dev, monkeypatch, name):
    """ops.conv2d_resample with both gradients: _conv_scratch of the forward, the data gradient (the toggled geometry) and the weight
    gradient; plain, transposed (up 2), strided (down 2), the direct path (k5) and the sliced weight gradient"""
    import conv2d_op_cases as cc
    import test_hip_conv2d_op as tco
    from latentaugment_amd import ops
    x0, w0, dy0, f, kw, _ = tco.case_tensors(cc.BY_NAME[name], 3)
    fd = None if f is None else f.to(dev)

    def run(g):
        x, w = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True)
        y = ops.conv2d_resample(x, w, f=fd, **kw)
        g.check()
        gx, gw = torch.autograd.grad(y, [x, w], dy0.to(dev))
        g.check()
        assert len(g.records) >= 3
        return dict(y=y, gx=gx, gw=gw)

    across_patterns(monkeypatch, run, f'conv2d_resample {name}')


# ---------------------------------------------------------------------------------------------------------------------------------
# filtered_lrelu: the written sign buffer at its exact size

def _flrelu_case(name):
    import test_hip_flrelu_shapes as tfs
    s = next(c for c in tfs.SIGN_CASES if c['name'] == name)
    return tfs, s, tfs.materialise(s)


@pytest.mark.parametrize('name', ['s_u2d2_ow36', 's_generic_up3'], ids=['fused', 'generic'])
def test_filtered_lrelu_sign_buffer(dev, lib, monkeypatch, name):
    """la_filtered_lrelu_f32 with write_signs = 1 into a sign buffer of exactly la_filtered_lrelu_sign_shape bytes and an output of exactly
    its size, both between bands.  The bytes a run writes are the same under every pattern; the bytes it leaves keep the pattern."""
    from latentaugment_amd import _lib
    tfs, s, (t, kw) = _flrelu_case(name)
    n, c, h, w = t['x'].shape
    fu_h, fu_w = tfs._c_taps(t['fu'])
    fd_h, fd_w = tfs._c_taps(t['fd'])
    px0, px1, py0, py1 = kw['padding']
    up, down = kw['up'], kw['down']
    oh = lib.la_filtered_lrelu_out_size(h, up, down, py0, py1, fu_h or fu_w, fd_h or fd_w)
    ow = lib.la_filtered_lrelu_out_size(w, up, down, px0, px1, fu_w, fd_w)
    rows, row_bytes = tfs.sign_shape(lib, t, kw)
    x, fu, fd, b = (None if v is None else v.to(dev).contiguous() for v in (t['x'], t['fu'], t['fd'], t['b']))
    clamp = math.inf if kw['clamp'] is None else kw['clamp']
    got = {}
    for pattern in ga.PATTERNS:
        g = Guarded(pattern)
        y = g.tensor([n, c, oh, ow], torch.float32, dev, float('nan'))
        so = g.alloc(n * c * rows * row_bytes, dev)
        _lib.check(lib.la_filtered_lrelu_f32(_p(x), _p(fu), _p(fd), _p(b), None, _p(so), _p(y), n, c, h, w, fu_h, fu_w, fd_h, fd_w, up, down,
                                             px0, px1, py0, py1, 0, 0, kw['gain'], kw['slope'], clamp, int(kw['flip_filter']), 1, _s()), 'filtered_lrelu')
        g.check()
        got[pattern] = (y.cpu(), so.cpu().reshape(n, c, rows, row_bytes))
    yz, sz = got['zeros']
    assert bool(torch.isfinite(yz).all())
    written = sz == got['ones'][1]          # a byte the kernel wrote is the same under 0x00 and 0xFF; one it left is 0x00 and 0xFF
    assert bool((sz[~written] == 0).all()) and bool((got['ones'][1][~written] == 0xFF).all())
    assert bool(written.any()) and bool((written == written[0, 0]).all()), 'the written extent differs between planes'
    r_used, c_used = written[0, 0].any(dim=1), written[0, 0].any(dim=0)
    ah, aw = int(r_used.sum()), int(c_used.sum())
    assert bool(written[0, 0, :ah, :aw].all()) and int(written[0, 0].sum()) == ah * aw, 'the written bytes are not one rectangle at the origin'
    print(f'{name}: sign buffer {rows} x {row_bytes} bytes per plane, written {ah} x {aw}')
    block = Guarded('bytes').alloc(n * c * rows * row_bytes, 'cpu').reshape(n, c, rows, row_bytes)
    for pattern in ga.PATTERNS[1:]:
        yp, sp = got[pattern]
        assert _first_difference(yz, yp) is None, (pattern, _first_difference(yz, yp))
        assert torch.equal(sp[written], sz[written]), pattern
    assert torch.equal(got['bytes'][1][~written], block[~written]), 'bytes beyond the last used row / column were written'


@pytest.mark.parametrize('name', ['s_u2d2_ow36', 's_generic_up3'], ids=['fused', 'generic'])
def test_filtered_lrelu_op(dev, monkeypatch, name):
    """ops.filtered_lrelu with a gradient: the op's own sign buffer (the `filtered_lrelu` scratch of ops.py) guarded and poisoned"""
    from latentaugment_amd import ops
    tfs, s, (t, kw) = _flrelu_case(name)

    def run(g):
        x = t['x'].to(dev).requires_grad_(True)
        y = ops.filtered_lrelu(x, fu=t['fu'].to(dev), fd=None if t['fd'] is None else t['fd'].to(dev), b=None if t['b'] is None else t['b'].to(dev), **kw)
        g.check()
        (dx,) = torch.autograd.grad(y, [x], t['dy'].to(dev))
        g.check()
        assert len(g.records) == 1
        return dict(y=y, dx=dx)

    across_patterns(monkeypatch, run, f'filtered_lrelu op {name}')


# ---------------------------------------------------------------------------------------------------------------------------------
# grid_sample gradient (float atomics: the one tolerance of this file)

@pytest.mark.parametrize('dtype', ['f16', 'f32', 'f64'])
def test_grid_sample_gradient(dev, monkeypatch, dtype):
    """h_blocks_c3: 260 outputs per image, more than one block.  float16 accumulates dx in the workspace (the only dtype with one)."""
    import grid_sample_cases as gc
    import test_hip_grid_sample as tgs
    from latentaugment_amd import ops
    case = next(c for c in gc.GS_CASES if c[0] == 'h_blocks_c3')
    t = gc.gs_inputs(case)
    dt = tgs.TORCH[dtype]
    tol = tgs.atomic_sum_tol(t['dy'], t['x'], t['grid'], dtype)

    def run(g):
        y, dx, dgrid = tgs.run_first(ops, dev, dt, t['x'], t['grid'], t['dy'])
        g.check()
        assert len(g.records) == (1 if dtype == 'f16' else 0)
        return dict(y=y, dx=dx, dgrid=dgrid)

    def compare(key, a, b):
        if key != 'dx':
            return NotImplemented
        err = float((a.double() - b.double()).abs().max())
        print(f'grid_sample {dtype} dx: {err:.3e} between two patterns, atomic_sum_tol {tol:.3e}')
        return None if err <= tol and bool(torch.isfinite(b).all()) else f'dx differs by {err:.3e} > atomic_sum_tol {tol:.3e}'

    across_patterns(monkeypatch, run, f'grid_sample {dtype}', compare)


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics

def test_pr_and_cdist(dev, lib, monkeypatch):
    """la_pr_workspace_floats: the radii, the membership and the distance tile at (130, 257) rows x columns, D = 48 -- ragged in both"""
    import criteria_cases as cc
    nr, nc, D = 130, 257, 48
    rows, cols = (torch.from_numpy(cc.pr_features(n, D, seed)).to(dev) for n, seed in ((nr, 1), (nc, 2)))
    need = lib.la_pr_workspace_floats(nr, nc)

    def run(g):
        ws = g.alloc(4 * need, dev, torch.float32)
        kth = g.tensor([nr], torch.float32, dev, -777.0)
        assert lib.la_pr_kth_f16(_p(rows), nr, _p(cols), nc, D, 3, _p(kth), _p(ws), _s()) == 0, _err(lib)
        g.check()
        member = g.tensor([nr], torch.uint8, dev, 0x5A)
        radius = torch.full([nc], 9.0, device=dev)
        assert lib.la_pr_member_f16(_p(rows), nr, _p(cols), nc, D, _p(radius), _p(member), _p(ws), _s()) == 0, _err(lib)
        g.check()
        dist = g.tensor([nr, nc], torch.float32, dev, -777.0)
        assert lib.la_cdist_f16(_p(rows), nr, _p(cols), nc, D, _p(dist), _p(ws), _s()) == 0, _err(lib)
        g.check()
        assert not bool((kth == -777.0).any()) and not bool((dist == -777.0).any()) and not bool((member == 0x5A).any())
        return dict(kth=kth, member=member, dist=dist)

    across_patterns(monkeypatch, run, 'pr / cdist')


def test_pr_through_the_package(dev, monkeypatch):
    import criteria_cases as cc
    from latentaugment_amd import metrics
    real, gen = cc.pr_features(161, 100, 3, 'float'), cc.pr_features(130, 100, 4, 'float')

    def run(g):
        p, r, d = metrics.compute_pr_from_features(real, gen, device=dev, return_details=True)
        g.check()
        dist = metrics.compute_distances(real, gen, device=dev)
        g.check()
        assert len(g.records) == 3
        return dict(pr=[p, r], dist=dist, **d)

    across_patterns(monkeypatch, run, 'compute_pr_from_features')


@pytest.mark.parametrize('S,m,D', [(3, 130, 20), (2, 300, 7)], ids=['two-tiles', 'three-tiles-ragged-D'])
def test_kid(dev, lib, monkeypatch, S, m, D):
    """la_kid_poly3_f32 beyond one 128-row tile per side (3 + 3 + 4 resp. 6 + 6 + 9 tile partials per subset), D % 4 != 0 in the second"""
    import kid_cpu
    real, gen = kid_cpu.detector_like_features(m + 20, D, 1), kid_cpu.detector_like_features(m + 9, D, 2)
    ix, iy = kid_cpu.subset_indices(real.shape[0], gen.shape[0], S, m, seed=0)
    xd, yd, ixd, iyd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (gen, real, ix, iy))
    need = lib.la_kid_workspace_bytes(S, m, m)
    assert need > SHORT

    def call(out, ws, nbytes):
        return lib.la_kid_poly3_f32(_p(xd), gen.shape[0], _p(yd), real.shape[0], D, _p(ixd), _p(iyd), S, m, m, _p(out), _p(out[S * 3:]),
                                    _p(out[S * 4:]), _p(ws), nbytes, _s())

    def run(g):
        ws = g.alloc(need, dev, torch.float64)
        out = g.tensor([S * 4 + 1], torch.float64, dev, -777.0)
        assert call(out, ws, need) == 0, _err(lib)
        g.check()
        out2 = g.tensor([S * 4 + 1], torch.float64, dev, -777.0)
        assert call(out2, ws, need - SHORT) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((out2 == -777.0).all()) and not bool((out == -777.0).any())
        return dict(out=out)

    across_patterns(monkeypatch, run, f'kid S{S} m{m} D{D}')


@pytest.mark.parametrize('nr,ng,D', [(130, 161, 48), (257, 130, 16)], ids=['two-steps-ragged', 'col-past-seam'])
def test_dc(dev, lib, monkeypatch, nr, ng, D):
    """la_dc_count_f16 behind la_pr_kth_f16 on one workspace, as compute_dc_from_features runs them: count and nearest are lowered and
    raised with atomics from values la_dc_init_kernel arms, the workspace holds the squared norms"""
    import dc_cases as dcc
    real, gen = (torch.from_numpy(a.copy()).to(dev) for a in dcc.dc_inputs(nr, ng, D, 'float'))
    need = max(lib.la_dc_workspace_bytes(ng, nr), 4 * lib.la_pr_workspace_floats(nr, nr))
    assert lib.la_dc_workspace_bytes(ng, nr) > SHORT

    def run(g):
        ws = g.alloc(need, dev, torch.float32)
        radii = g.tensor([nr], torch.float32, dev, -777.0)
        assert lib.la_pr_kth_f16(_p(real), nr, _p(real), nr, D, 5, _p(radii), _p(ws), _s()) == 0, _err(lib)
        g.check()
        count = g.tensor([ng], torch.int32, dev, -777)
        nearest = g.tensor([nr], torch.float32, dev, -777.0)
        assert lib.la_dc_count_f16(_p(gen), ng, _p(real), nr, D, _p(radii), _p(count), _p(nearest), _p(ws), need, _s()) == 0, _err(lib)
        g.check()
        c2 = g.tensor([ng], torch.int32, dev, -777)
        n2 = g.tensor([nr], torch.float32, dev, -777.0)
        short = lib.la_dc_workspace_bytes(ng, nr) - SHORT
        assert lib.la_dc_count_f16(_p(gen), ng, _p(real), nr, D, _p(radii), _p(c2), _p(n2), _p(ws), short, _s()) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((c2 == -777).all()) and bool((n2 == -777.0).all())
        assert not bool((count == -777).any()) and not bool((nearest == -777.0).any())
        return dict(radii=radii, count=count, nearest=nearest)

    across_patterns(monkeypatch, run, f'dc {nr}/{ng} D{D}')


@pytest.mark.parametrize('name', ['rank-deficient 33/17 x 256', 'full rank 200/150 x 64'])
def test_fd(dev, lib, monkeypatch, name):
    """la_fd_gram_f32, the sweeps and la_fd_finish_f64 on one workspace.  33 / 17: n odd (the padding vector of the vector region),
    two column chunks; 200 / 150: several 64-row colsum chunks per side and more than one Gram tile"""
    import fd_cases as fc
    real, gen = fc.fd_cases()[name]
    nr, ng, D = real.shape[0], gen.shape[0], real.shape[1]
    n, m = min(ng, nr), max(ng, nr)
    xd, yd = torch.from_numpy(gen).to(dev), torch.from_numpy(real).to(dev)
    need = lib.la_fd_workspace_bytes(ng, nr, D)

    def run(g):
        ws = g.alloc(need, dev, torch.float64)
        out = g.tensor([4 + n], torch.float64, dev, -777.0)
        rot = g.tensor([1], torch.int32, dev, -777)
        assert lib.la_fd_gram_f32(_p(xd), ng, _p(yd), nr, D, _p(out), _p(ws), need, _s()) == 0, _err(lib)
        g.check()
        sweeps = 0
        while True:
            assert lib.la_fd_jacobi_sweep_f64(_p(ws), n, m, _p(rot), _s()) == 0, _err(lib)
            sweeps += 1
            if int(rot.item()) == 0:
                break
            assert sweeps < 30
        g.check()
        assert lib.la_fd_finish_f64(_p(ws), need, ng, nr, D, _p(out[4:]), _p(out), _s()) == 0, _err(lib)
        g.check()
        out2 = g.tensor([4 + n], torch.float64, dev, -777.0)
        assert lib.la_fd_gram_f32(_p(xd), ng, _p(yd), nr, D, _p(out2), _p(ws), need - SHORT, _s()) == LA_ERR_WORKSPACE
        assert lib.la_fd_finish_f64(_p(ws), need - SHORT, ng, nr, D, _p(out2[4:]), _p(out2), _s()) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((out2 == -777.0).all()) and not bool((out == -777.0).any())
        return dict(out=out, sweeps=[sweeps])

    across_patterns(monkeypatch, run, f'fd {name}')


def test_fd_through_the_package(dev, monkeypatch):
    import fd_cases as fc
    from latentaugment_amd import metrics
    real, gen = fc.fd_cases()['n = 2']

    def run(g):
        fd, d = metrics.compute_fd_from_features(real, gen, device=dev, return_details=True)
        g.check()
        assert len(g.records) == 1
        return dict(fd=[fd], sv=d['singular_values'], terms=d['terms'])

    across_patterns(monkeypatch, run, 'compute_fd_from_features')


@pytest.mark.parametrize('H,W,levels,win,Cn,P,kind', [(64, 96, 3, 11, 2, 2, 'background'), (43, 43, 1, 11, 2, 2, 'texture'), (48, 80, 3, 3, 1, 3, 'texture')],
                         ids=['64x96-3-levels', '43x43-ragged-tile-both-axes', '48x80-ragged-next-level'])
def test_pair_metrics(dev, lib, monkeypatch, H, W, levels, win, Cn, P, kind):
    """la_pair_metrics_f32: the 3-level case (a level writes the next level's pyramid images into the workspace), win 11 on 43 x 43 (33 x 33
    outputs, one more than a 32-tile in both axes), and the 48 x 80 case of pair_metric_cases.MULTI, whose 32-tiles hang over the image
    in both axes at levels 0 and 1: the next-level writes of those tiles are the ones an edge test has to stop, and the last level's
    images are the last region of the workspace"""
    import pair_metric_cases as pc
    x, y = pc.images(kind, P, Cn, H, W, seed=H * 1000 + W + win)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    taps = pc.window(win, 1.5).astype(np.float32)
    w = pc.weights_for(levels, None)
    c1, c2 = pc.constants()
    need = lib.la_pair_metrics_workspace_bytes(P, Cn, H, W, win, levels)
    assert need > SHORT

    def outputs(g):
        return (g.tensor([P, Cn, 2], torch.float64, dev, -7.0), g.tensor([P, Cn, levels], torch.float32, dev, -7.0),
                g.tensor([P, Cn, levels], torch.float32, dev, -7.0), g.tensor([P, Cn], torch.float32, dev, -7.0))

    def call(o, ws, nbytes):
        return lib.la_pair_metrics_f32(_p(xd), _p(yd), None, None, P, Cn, H, W, taps.ctypes.data, win, levels, w.ctypes.data, float(c1), float(c2),
                                       _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), _p(ws), nbytes, _s())

    def run(g):
        ws = g.alloc(need, dev, torch.float64)
        o = outputs(g)
        assert call(o, ws, need) == 0, _err(lib)
        g.check()
        o2 = outputs(g)
        assert call(o2, ws, need - SHORT) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in o2) and not any(bool((t == -7.0).any()) for t in o)
        return dict(err=o[0], ssim=o[1], cs=o[2], ms=o[3])

    across_patterns(monkeypatch, run, f'pair metrics {H}x{W}')


def test_pair_metrics_through_the_package(dev, monkeypatch):
    import pair_metric_cases as pc
    from latentaugment_amd import metrics
    x, y = pc.images('smooth', 3, 1, 48, 80, seed=1)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)

    def run(g):
        out = metrics.compute_pair_metrics(xd, yd, win_size=3, levels=3)
        g.check()
        assert len(g.records) == 1
        return out

    across_patterns(monkeypatch, run, 'compute_pair_metrics')


@pytest.mark.parametrize('bins', [1, 64])
@pytest.mark.parametrize('npix', [2047, 2048, 2049])
def test_joint_histogram(dev, lib, bins, npix):
    """la_joint_hist_f32 takes no workspace: the table between bands, at npix one short of, equal to and one beyond JH_CHUNK = 2048.  It
    is cleared by the entry, so its pre-fill (the pattern) must not reach the counts."""
    import pair_metric_cases as pc
    a, b = pc.hist_values('off_edges', 3, npix, bins, seed=bins + npix)
    ad, bd = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    want = pc.joint_hist_restate(a, b, bins)
    for fill in (0, -1, 0x5A5A5A5A):
        g = Guarded('zeros')
        hist = g.tensor([3, bins, bins], torch.int32, dev, fill)
        rc = lib.la_joint_hist_f32(_p(ad), npix, _p(bd), npix, 3, npix, bins, -1.0, float(pc.hist_scale(bins, -1.0, 1.0)), _p(hist), _s())
        assert rc == 0, _err(lib)
        g.check()
        got = hist.cpu().numpy().view(np.uint32).astype(np.int64)
        assert (got == want).all(), (fill, int((got != want).sum()))


@pytest.mark.parametrize('mode', [0, 1])
def test_path_points(dev, lib, mode):
    """la_path_points_f32 takes no workspace: its output between bands, N = 3, D = 37 (no multiple of 4), reps = 2, T = 2"""
    N, D, reps, T = 3, 37, 2, 2
    gen = torch.Generator().manual_seed(11)
    a, b = torch.randn([N, D], generator=gen).to(dev), torch.randn([N, D], generator=gen).to(dev)
    t = torch.rand([N], generator=gen).to(dev)
    dt = (C.c_double * T)(0.0, 1e-4)
    outs = []
    for fill in (0.0, float('nan')):
        g = Guarded('zeros')
        out = g.tensor([T, N, reps, D], torch.float32, dev, fill)
        assert lib.la_path_points_f32(_p(a), _p(b), _p(t), dt, T, N, D, reps, mode, _p(out), _s()) == 0, _err(lib)
        g.check()
        assert bool(torch.isfinite(out).all())
        outs.append(out.cpu())
    assert _first_difference(outs[0], outs[1]) is None


# ---------------------------------------------------------------------------------------------------------------------------------
# mapping

@pytest.mark.parametrize('z_dim,w_dim', [(40, 72), (72, 40)])
def test_mapping_tmp(dev, monkeypatch, z_dim, w_dim):
    """the mapping network's `tmp` (two rows of max(z_dim, w_dim) per sample) at z_dim != w_dim, both ways; B = 9, two layers"""
    from latentaugment_amd.synthesis import MappingEngine
    gen = torch.Generator().manual_seed(1000 + z_dim)
    sd = {'mapping.fc0.weight': torch.randn([w_dim, z_dim], generator=gen), 'mapping.fc0.bias': torch.randn([w_dim], generator=gen),
          'mapping.fc1.weight': torch.randn([w_dim, w_dim], generator=gen), 'mapping.fc1.bias': torch.randn([w_dim], generator=gen),
          'mapping.w_avg': torch.randn([w_dim], generator=gen)}
    z = torch.randn([9, z_dim], generator=gen)
    eng = MappingEngine(sd, dev)

    def run(g):
        ws = eng.forward(z.to(dev), 6, truncation_psi=0.7)
        g.check()
        assert len(g.records) == 1 and g.records[0][1] == 4 * 2 * 9 * max(z_dim, w_dim)
        return dict(ws=ws)

    out = across_patterns(monkeypatch, run, f'mapping {z_dim}->{w_dim}')
    assert bool(torch.isfinite(out['ws']).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# latent loop

def _loop_case(kind):
    import loop_cases as lc
    if kind == 'latent+pix':          # no perceptual workspace, no discriminator; the row / column window is on
        return lc.LoopCase('guard-pix-R16', 16, 24, 2, Mx=9, imgc=3, steps=2, w_pix=2.0, w_latent=0.3, Mw=4, kind='scalars')
    if kind == 'lpips':               # the perceptual workspace alone (windowed synthesis passes: no discriminator)
        return lc.LoopCase('guard-lpips-R32', 32, 32, 2, steps=2, w_lpips=3.0, Mf=5, crop_pos=(9, 4), kind='scalars')
    if kind == 'disc':                # the discriminator alone
        return lc.LoopCase('guard-disc-R32', 32, 32, 2, steps=2, w_disc=1.0, kind='scalars')
    space = 'w+' if kind == 'all-w+' else 'w'
    return lc.LoopCase(f'guard-{kind}-R32', 32, 32, 2, space, steps=2, crop_pos=(3, 11), kind='scalars', **lc.ALL_MIX)


_LOOP_BUILT = {}


def _aug(case, b, graph):
    import loop_cases as lc
    from latentaugment_amd.latent_aug import LatentAug
    opt = types.SimpleNamespace(
        img_resolution=case.R, batch_size=case.max_batch, modalities_aug=','.join('ABC'[:case.imgc]), opt_num_epochs=case.steps, opt_lr=lc.LR,
        truncation_psi=1.0, w_pix=case.w_pix, w_lpips=case.w_lpips, w_latent=case.w_latent, w_disc=case.w_disc, crop_size_aug=lc.FEAT_CROP,
        preprocess_aug='center_random_crop', soft_aug=case.soft, alpha=case.alpha, verbose_log=False, criterion_mode='gemm',
        final_noise_mode='const', precision='f32', latent_space=case.space, norm_batch=case.norm_batch, stream_lanes=1, lpips_preproc=lc.PREPROC,
        hip_graph=graph)
    return LatentAug('train', opt, None, [0], generator=b.G, discriminator=b.D, banks=b.banks(), feature_net=b.ops)


@pytest.mark.parametrize('kind,graph', [('latent+pix', False), ('latent+pix', True), ('lpips', False), ('disc', True), ('all', False), ('all', True),
                                        ('all-w+', True)],
                         ids=['pix-eager', 'pix-graph', 'lpips-eager', 'disc-graph', 'all-eager', 'all-graph', 'all-wplus-graph'])
def test_latent_loop(dev, monkeypatch, kind, graph):
    """two steps of la_latent_opt: the loop workspace (latent, Adam moments, step counter and ticket, crop position, loss scalars), the
    perceptual workspace and the three engines' workspaces all come from the guarded allocator.  Eager and as a captured graph (run twice:
    the second run replays the capture), W and W+; losses, the final latent and the images are the same bits under every pattern."""
    if kind not in _LOOP_BUILT:
        _LOOP_BUILT[kind] = _loop_case(kind)
    case = _LOOP_BUILT[kind]
    b = case.build()

    def run(g):
        la = _aug(case, b, graph)
        g.check()
        w0 = b.w0[:case.B].to(dev)
        img, w_aug, losses = la.run_local(w0, want_losses=True, crop_pos=case.crop_pos)
        g.check()
        img2, w_aug2, _ = la.run_local(w0, crop_pos=case.crop_pos)
        g.check()
        assert la.graph_state == (1 if graph else 0)
        return dict(img=img, w_aug=w_aug, losses=losses, img_again=img2, w_aug_again=w_aug2)

    out = across_patterns(monkeypatch, run, f'latent loop {kind} graph={graph}')
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert _first_difference(out['w_aug'], out['w_aug_again']) is None and _first_difference(out['img'], out['img_again']) is None
    assert float((out['w_aug'] - b.w0[:case.B].expand_as(out['w_aug'])).abs().max()) > 0          # (the steps moved the latent)


def test_latent_loop_refuses_a_short_workspace(dev, lib, monkeypatch):
    case = _LOOP_BUILT.setdefault('latent+pix', _loop_case('latent+pix'))
    b = case.build()
    refused_short(monkeypatch, lib, 'la_latent_opt_workspace_bytes_ex', lambda: _aug(case, b, False))
    case = _LOOP_BUILT.setdefault('lpips', _loop_case('lpips'))
    b = case.build()
    refused_short(monkeypatch, lib, 'la_latent_opt_lpips_workspace_bytes', lambda: _aug(case, b, False))


# ---------------------------------------------------------------------------------------------------------------------------------
# projector

def test_projector_step_and_row_distance(dev, lib, monkeypatch):
    """one teacher-forced step of the projector (w, w_pix 0.1) with every workspace guarded -- synthesis, feature engine, row distance --
    and la_row_dist_f32 alone at K = 8195 (no multiple of the 256-thread block or of 4: scalar path; two chunks, the second of three elements)"""
    import projector_cases as pj
    from latentaugment_amd.projector import Projector
    case = pj.make_case('w', 0.1)
    tgt = pj.targets()
    B = tgt.shape[0]
    gen = torch.Generator().manual_seed(3)
    w_host = torch.randn([B, 1, pj.TINY['w_dim']], generator=gen)

    def run(g):
        net = types.SimpleNamespace(ops=case.ops, pre_scale=case.pre_scale, pre_shift=case.pre_shift)
        proj = Projector(pj.generator(), net, dev, 3, precision='f32', lpips_res=pj.TINY['img_resolution'])
        g.check()
        tgt_d = tgt.to(dev)
        tfeat = proj.target_features(tgt_d)
        g.check()
        w_opt = w_host.to(dev)
        ws = torch.empty_like(w_opt)
        proj.step_tail(None, w_opt, None, None, ws, 0, 0.0, 0.05, case.seed, 1, 0)
        loss = torch.zeros([B, 2], dtype=torch.float64, device=dev)
        dws, img = proj.loss_and_grad(ws, tgt_d, tfeat, 0.1, loss)
        g.check()
        return dict(tfeat=tfeat, ws=ws, loss=loss, dws=dws, img=img)

    across_patterns(monkeypatch, run, 'projector step')

    rows, K = 5, 8195
    rs = np.random.RandomState(7)
    a = torch.from_numpy(rs.randn(rows, K).astype(np.float32)).to(dev)
    t = torch.from_numpy(rs.randn(rows, K).astype(np.float32)).to(dev)
    need = lib.la_row_dist_workspace_bytes(rows, K)
    assert need > SHORT

    def run_rows(g):
        ws = g.alloc(need, dev, torch.float64)
        grad = g.tensor([rows, K], torch.float32, dev, float('nan'))
        loss = g.tensor([rows], torch.float64, dev, -1.0)
        assert lib.la_row_dist_f32(_p(a), _p(t), rows, K, 1, 1.0 / K, 2.0 / K, _p(grad), 0, _p(loss), 1, _p(ws), need, _s()) == 0, _err(lib)
        g.check()
        g2 = g.tensor([rows, K], torch.float32, dev, -777.0)
        l2 = g.tensor([rows], torch.float64, dev, -1.0)
        assert lib.la_row_dist_f32(_p(a), _p(t), rows, K, 1, 1.0 / K, 2.0 / K, _p(g2), 0, _p(l2), 1, _p(ws), need - SHORT, _s()) == LA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((g2 == -777.0).all()) and bool((l2 == -1.0).all()) and bool(torch.isfinite(grad).all()) and bool((loss > 0).all())
        return dict(grad=grad, loss=loss)

    across_patterns(monkeypatch, run_rows, 'row distance K 8195')


# ---------------------------------------------------------------------------------------------------------------------------------
# geometric kernels: no workspace, the outputs between bands

def test_geometric_kernels(dev, lib):
    """la_noise_uniform_f32 (row_elems 5), la_elastic_field_f32 (63 taps; H, W = 17, 65: the kernel is wider than the image is high),
    la_warp_affine_f32 and la_warp_elastic_f32 write exactly their outputs, whatever those held before"""
    B, Cn, H, W, ntaps = 3, 2, 17, 65, 63
    gen = torch.Generator().manual_seed(21)
    x = torch.randn([B, Cn, H, W], generator=gen).to(dev)
    taps = np.exp(-0.5 * ((np.arange(ntaps) - 31) / 9.0) ** 2)
    taps = (C.c_float * ntaps)(*(taps / taps.sum()).tolist())
    minv = torch.tensor([[0.9, 0.1, 1.5, -0.1, 0.9, -0.5], [1, 0, 0, 0, 1, 0], [-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0]], dtype=torch.float32).to(dev)
    apply = torch.tensor([1, 0, 1], dtype=torch.uint8).to(dev)
    res = []
    for fill in (0.0, float('nan'), -777.0):
        g = Guarded('zeros')
        noise = g.tensor([B * 2 * H * W // 5, 5], torch.float32, dev, fill)
        assert noise.numel() == B * 2 * H * W
        assert lib.la_noise_uniform_f32(_p(noise), noise.shape[0], 5, 1234, 2, 7, _s()) == 0, _err(lib)
        g.check()
        disp = g.tensor([B, 2, H, W], torch.float32, dev, fill)
        assert lib.la_elastic_field_f32(_p(noise), taps, ntaps, 3.0, 2.0, _p(disp), None, B, H, W, _s()) == 0, _err(lib)
        g.check()
        ya = g.tensor([B, Cn, H, W], torch.float32, dev, fill)
        assert lib.la_warp_affine_f32(_p(x), _p(minv), _p(apply), _p(ya), B, Cn, H, W, 2, _s()) == 0, _err(lib)
        g.check()
        ye = g.tensor([B, Cn, H, W], torch.float32, dev, fill)
        assert lib.la_warp_elastic_f32(_p(x), _p(disp), _p(apply), _p(ye), B, Cn, H, W, 2, _s()) == 0, _err(lib)
        g.check()
        out = dict(noise=noise.cpu(), disp=disp.cpu(), ya=ya.cpu(), ye=ye.cpu())
        assert all(bool(torch.isfinite(v).all()) for v in out.values()) and bool((out['noise'].abs() < 1).all())
        assert torch.equal(out['ya'][1], x[1].cpu()) and torch.equal(out['ye'][1], x[1].cpu())          # apply = 0: a copy
        res.append(out)
    for other in res[1:]:
        for k in res[0]:
            assert _first_difference(res[0][k], other[k]) is None, (k, _first_difference(res[0][k], other[k]))
