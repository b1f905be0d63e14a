"""A used handle must give the bits of a fresh one.  Every history of tests/history_cases.py (the hand-written PAIRWISE lists and the seeded
RANDOM ones) runs on one `la_synth` / `la_disc` / `la_feat` handle, or one whole loop stack (synthesis, discriminator, feature engine and
`la_latent_opt`), followed by the probe; a newly created handle (stack) gets the probe's settings and runs the probe once.

THE RULE: `torch.equal` on every compared output, no tolerance anywhere in this file.  Synthesis, whole-frame probe: image, every block
image, every layer output, styles, style gradients, dws, every layer's noise gradient; windowed probe: the image inside the window,
every layer output on its planned L_FWD rows / columns (la_synth_plan_query), styles, style gradients, dws.  Discriminator: logits, loss,
g_img written and accumulated onto a seeded g_img.  Feature engine: features, gx, the pair distances.  Loop: img_out, w_aug_out, the loss
scalars when asked, and la_latent_opt_graph_state against the state model.  A refused call must return LA_ERR_ARG and leave no trace.

So that a real reference stays in the picture, the FRESH probe is also judged against float64 with the helpers and budgets of the existing
sweeps, unchanged: test_hip_synth_shapes._judge_all / _judge_bulk, test_hip_engine_shapes._judge, loop_cases.judge (on a traced run of
the fresh stack, as test_hip_loop_shapes.py makes it).  History passes run on inputs scaled by 2^3 (latents, images) and 2^8 (gradients)
or by 2^-6, alternating (history_cases.pass_scale).

Found by this file: the discriminator and the feature engine read their precision again in the backward pass (a setter between forward and
backward made the backward run in another precision than the forward); the loop replayed a step captured under the old settings after a
setter of an ATTACHED engine (la_synth_set_precision, la_synth_set_torgb_schedule, la_disc_set_precision, la_feat_set_precision).
Both are fixed in the library ("Handle history").

Measured on an MI355X: every equality held, and every fresh probe was inside its float64 budget.  Against the parent library (without the
two fixes) test_loop_history[synth-precision-stays-changed], [all-precisions-changed-and-back] and [win64-synth-precision-changed] fail.
Wall time of the file: 9.2 s for 125 tests, the float64 and float32 CPU runs included; slowest test 1.15 s (the first, which loads the
library), every other below 0.31 s.
"""
import copy
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_cases as ec  # noqa: E402
import history_cases as hc  # noqa: E402
import loop_cases as lc  # noqa: E402
import synth_cases as sc  # noqa: E402
import test_hip_engine_shapes as tes  # noqa: E402
import test_hip_image_chain as chain  # noqa: E402
import test_hip_loop_shapes as tls  # noqa: E402
import test_hip_synth_shapes as tss  # noqa: E402
from test_synth_plan_cpu import PREC, query  # noqa: E402

pytestmark = pytest.mark.gpu
lc.G_CHANNELS.setdefault(128, hc.LOOP_R128_CHANNELS)          # the 128^2 generator of the column-window loop case


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


def _ok(lib, rc, what):
    assert rc == 0, f'{what}: {rc} {lib.la_last_error()}'


def _refused(lib, rc, what):
    assert rc == hc.LA_ERR_ARG and lib.la_last_error(), f'{what}: expected LA_ERR_ARG, got {rc}'


def _ids(hs):
    return [h.name for h in hs]


def _same(name, a, b, bad):
    if not torch.equal(a, b):
        d = (a.double() - b.double()).abs()
        bad.append(f'{name}: {int((a != b).sum())} of {a.numel()} elements differ, largest |difference| {float(d.max()):.3e}')


# ---------------------------------------------------------------------------------------------------------------------------------
# synthesis engine

class _ChainCase:
    """a channel table of test_hip_image_chain.py in the form of a synth_cases.SynthCase (bulk: R = 64)"""
    kind, clamp, w_dim, B, seed = 'bulk', 256.0, 32, hc.SYNTH_PROBE_B, 5

    def __init__(self, name):
        c = chain.CASES[name[6:]]
        self.name, self.channels, self.imgc = name, list(c['channels']), c['imgc']
        self.R = 4 << (len(self.channels) - 1)
        self.noise = [float(torch.tensor(0.1, dtype=torch.float32))] * (2 * len(self.channels) - 1)

    def state_dict(self):
        return chain.state_dict(self.channels, self.imgc, self.w_dim, seed=self.seed)

    def inputs(self):
        g = torch.Generator().manual_seed(1000 * self.seed + 31)
        nws = 2 * len(self.channels)
        return torch.randn([self.B, nws, self.w_dim], generator=g), torch.randn([self.B, self.imgc, self.R, self.R], generator=g)

    def restate(self, sd, ws, g_img, dtype):
        return sc.synth_restate(sd, self.R, self.imgc, self.clamp, self.noise, ws, dtype, g_img)


_SYNTH = {}


def _synth_shape(name):
    """(case, state dict, ws, g_img) of a synthesis shape, built once"""
    if name not in _SYNTH:
        if name.startswith('chain:'):
            case = _ChainCase(name)
            sd = case.state_dict()
            ws, g_img = case.inputs()
        else:
            case = sc.SYNTH_SHRINK if name == sc.SYNTH_SHRINK.name else sc.SYNTH_BY_NAME[name]
            G, ws, g_img = case.build()
            sd = G.synthesis.state_dict()
        assert ws.shape[0] == hc.SYNTH_PROBE_B
        _SYNTH[name] = (case, sd, ws, g_img)
    return _SYNTH[name]


_SREF = {}


def _synth_ref(name, rows, cols):
    """(g_img zero outside the window, float32 run, float64 run) of the probe of a shape under a window, computed once"""
    key = (name, rows, cols)
    if key not in _SREF:
        case, sd, ws, g_img = _synth_shape(name)
        g = _masked(g_img, rows, cols)
        src = sd if isinstance(case, _ChainCase) else types.SimpleNamespace(synthesis=types.SimpleNamespace(state_dict=lambda: sd))
        _SREF[key] = (g, case.restate(src, ws, g, torch.float32), case.restate(src, ws, g, torch.float64))
    return _SREF[key]


def _masked(g_img, rows, cols):
    if rows[1] == 0:
        return g_img
    R = g_img.shape[-1]
    clo, chi = cols if cols[1] else (0, R)
    g = torch.zeros_like(g_img)
    g[:, :, rows[0]:rows[1], clo:chi] = g_img[:, :, rows[0]:rows[1], clo:chi]
    return g


_SHIST = {}


def _synth_history_inputs(name, index, dev):
    """seeded inputs of the index-th forward pass of a history at a shape (max_batch rows, on the device): ws, g_img, noise per layer"""
    key = (name, index)
    if key not in _SHIST:
        case, _, ws, g_img = _synth_shape(name)
        g = torch.Generator().manual_seed(7000 + 13 * index)
        sw, sg = hc.pass_scale(index)
        nl = 2 * len(case.channels) - 1
        res = [4 << ((k + 1) // 2) for k in range(nl)]
        _SHIST[key] = ((torch.randn([hc.MAX_BATCH] + list(ws.shape[1:]), generator=g) * sw).to(dev),
                       (torch.randn([hc.MAX_BATCH] + list(g_img.shape[1:]), generator=g) * sg).to(dev),
                       [torch.randn([hc.MAX_BATCH, r, r], generator=g).to(dev) for r in res])
    return _SHIST[key]


def _synth_engine(dev, name):
    from latentaugment_amd.synthesis import SynthesisEngine
    case, sd, _, _ = _synth_shape(name)
    eng = SynthesisEngine(sd, dev, hc.MAX_BATCH, conv_clamp=case.clamp, precision='f32')
    assert eng.channels == list(case.channels) and eng.img_channels == case.imgc
    return eng


def _synth_forward(lib, eng, ws, B, noise_mode, noises, wplus, out):
    ws = (ws[:B] if wplus else ws[:B, :1]).contiguous()
    arr = None
    if noise_mode == 2:
        noises = [n[:B].contiguous() for n in noises]
        arr = (C.c_void_p * len(noises))(*[n.data_ptr() for n in noises])
    img = torch.full([B, eng.img_channels, eng.img_resolution, eng.img_resolution], 7.0, device=ws.device) if out else None
    rc = lib.la_synth_forward(eng.handle, _p(ws), ws.shape[1] * eng.w_dim, eng.w_dim if wplus else 0, B, noise_mode, arr, _p(img), _s())
    return rc, img, (ws, noises)


def _noise_buffers(eng, B, dev):
    gn = [torch.full([B, r, r], 7.0, device=dev) for r in eng.layer_resolutions]
    return gn, (C.c_void_p * len(gn))(*[t.data_ptr() for t in gn])


def _synth_set_window(lib, eng, rows, cols):
    _ok(lib, lib.la_synth_set_row_window(eng.handle, *rows), 'la_synth_set_row_window')
    _ok(lib, lib.la_synth_set_col_window(eng.handle, *cols), 'la_synth_set_col_window')


def _run_synth_history(lib, dev, eng, h):
    from latentaugment_amd import _lib
    m, keep = hc.SynthModel(), []
    for op in h.ops:
        name = op[0]
        fwd_before = m.fwd
        want = m.apply(op)
        if name == 'forward':
            ws, _, noises = _synth_history_inputs(h.case, m.fwd['index'], dev)
            rc, img, k = _synth_forward(lib, eng, ws, op[1], op[2], noises, op[3], op[4])
            keep.append((img, k))
            _ok(lib, rc, 'la_synth_forward')
        elif name in ('backward', 'backward_noise', 'refused_noise'):
            f = m.fwd
            _, g, _ = _synth_history_inputs(h.case, f['index'], dev)
            g = _masked(g[:f['B']], f['rows'], f['cols']).contiguous()
            dws = torch.empty([f['B'], eng.num_ws, eng.w_dim], device=dev)
            if name == 'backward':
                rc = lib.la_synth_backward(eng.handle, _p(g), _p(dws), _s())
            else:
                gn, arr = _noise_buffers(eng, f['B'], dev)
                rc = lib.la_synth_backward_noise(eng.handle, _p(g), _p(dws), arr, _s())
                keep.append(gn)
            keep.append((g, dws))
            (_refused if want else _ok)(lib, rc, name)
        elif name == 'refused_forward':
            ws, _, noises = _synth_history_inputs(h.case, 0, dev)
            out = torch.full([hc.MAX_BATCH, eng.img_channels, eng.img_resolution, eng.img_resolution], 7.0, device=dev)
            rc = lib.la_synth_forward(eng.handle, _p(ws), ws.shape[1] * eng.w_dim, eng.w_dim, hc.MAX_BATCH + 1, 1, None, _p(out), _s())
            _refused(lib, rc, name)
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()) and m.fwd is fwd_before
        elif name == 'set_precision':
            eng.set_precision(op[1])
        elif name == 'set_schedule':
            _lib.check(lib.la_synth_set_torgb_schedule(eng.handle, op[1]), 'la_synth_set_torgb_schedule')
        elif name in ('set_rows', 'set_cols', 'clear_windows'):
            _synth_set_window(lib, eng, m.rows, m.cols)
        else:
            raise ValueError(name)
    torch.cuda.synchronize()
    return keep


def _synth_probe(lib, dev, eng, h):
    """the probe's setters and its pass -> dict of CPU tensors"""
    from latentaugment_amd import _lib
    p = h.probe
    case, _, ws, _ = _synth_shape(h.case)
    B, nb = p['B'], len(case.channels)
    g_img = _synth_ref(h.case, p['rows'], p['cols'])[0]
    eng.set_precision(p['prec'])
    _lib.check(lib.la_synth_set_torgb_schedule(eng.handle, p['sched']), 'la_synth_set_torgb_schedule')
    _synth_set_window(lib, eng, p['rows'], p['cols'])
    rc, img, keep = _synth_forward(lib, eng, ws.to(dev), B, 1, None, True, True)
    _ok(lib, rc, 'la_synth_forward (probe)')
    torch.cuda.synchronize()
    out = dict(img=img.cpu(), layers=[eng.layer_output(k, B).cpu() for k in range(eng.num_layers)], styles=eng.styles(B).cpu(),
               blocks=[eng._view(lib.la_synth_block_image(eng.handle, k), [B, case.imgc, 4 << k, 4 << k]).cpu() for k in range(nb - 1)])
    g = g_img.to(dev).contiguous()
    dws = torch.empty([B, eng.num_ws, eng.w_dim], device=dev)
    if p['rows'][1] == 0:
        gn, arr = _noise_buffers(eng, B, dev)
        _ok(lib, lib.la_synth_backward_noise(eng.handle, _p(g), _p(dws), arr, _s()), 'la_synth_backward_noise (probe)')
        torch.cuda.synchronize()
        out['gnoises'] = [t.cpu() for t in gn]
    else:
        _ok(lib, lib.la_synth_backward(eng.handle, _p(g), _p(dws), _s()), 'la_synth_backward (probe)')
        torch.cuda.synchronize()
    out.update(dws=dws.cpu(), dstyles=eng.style_grads(B).cpu())
    _synth_set_window(lib, eng, (0, 0), (0, 0))
    return out


def _synth_compare(lib, h, used, fresh):
    p, bad = h.probe, []
    case = _synth_shape(h.case)[0]
    R = case.R
    for key in ('styles', 'dstyles', 'dws'):
        _same(f'{h.name} {key}', used[key], fresh[key], bad)
    if p['rows'][1] == 0:
        _same(f'{h.name} image', used['img'], fresh['img'], bad)
        for k, (a, b) in enumerate(zip(used['blocks'], fresh['blocks'])):
            _same(f'{h.name} block image {k}', a, b, bad)
        for k, (a, b) in enumerate(zip(used['layers'], fresh['layers'])):
            _same(f'{h.name} layer {k}', a, b, bad)
        for k, (a, b) in enumerate(zip(used['gnoises'], fresh['gnoises'])):
            _same(f'{h.name} noise gradient {k}', a, b, bad)
        return bad
    (lo, hi), (clo, chi) = p['rows'], (p['cols'] if p['cols'][1] else (0, R))
    _same(f'{h.name} image in the window', used['img'][:, :, lo:hi, clo:chi], fresh['img'][:, :, lo:hi, clo:chi], bad)
    rc, plan = query(lib, R, case.imgc, list(case.channels), p['B'], PREC[p['prec']], p['rows'], p['cols'])
    assert rc == 0
    for k, (a, b) in enumerate(zip(used['layers'], fresh['layers'])):
        r0, r1, c0, c1 = plan['layers'][k]['fwd']
        r0, r1 = (r0, r1) if r1 > 0 else (0, a.shape[2])
        c0, c1 = (c0, c1) if c1 > 0 else (0, a.shape[3])
        _same(f'{h.name} layer {k} rows {r0}..{r1} columns {c0}..{c1}', a[:, :, r0:r1, c0:c1], b[:, :, r0:r1, c0:c1], bad)
    return bad


def _synth_judge(h, fresh):
    """the fresh probe against float64: the sweep's own judges and budgets"""
    p = h.probe
    case = _synth_shape(h.case)[0]
    _, r32, r64 = _synth_ref(h.case, p['rows'], p['cols'])
    if p['rows'][1] == 0:
        tss._judge_all(case, p['prec'], fresh, r32, r64, what=f' history {h.name}')
        return
    R = case.R
    (lo, hi), (clo, chi) = p['rows'], (p['cols'] if p['cols'][1] else (0, R))
    tag = f'synth {h.case} history {h.name} window'
    bad = [tss._judge_bulk(f'{tag} image', p['prec'], fresh['img'][:, :, lo:hi, clo:chi], r32['img'][:, :, lo:hi, clo:chi], r64['img'][:, :, lo:hi, clo:chi]),
           tss._judge_bulk(f'{tag} style_grads', p['prec'], fresh['dstyles'], r32['dstyles'], r64['dstyles']),
           tss._judge_bulk(f'{tag} dws', p['prec'], fresh['dws'], r32['dws'], r64['dws'])]
    bad = [t for t in bad if t]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('h', hc.all_histories('synth'), ids=_ids(hc.all_histories('synth')))
def test_synthesis_history(dev, lib, h):
    used = _synth_engine(dev, h.case)
    keep = _run_synth_history(lib, dev, used, h)
    got = _synth_probe(lib, dev, used, h)
    fresh = _synth_probe(lib, dev, _synth_engine(dev, h.case), h)
    del keep
    bad = _synth_compare(lib, h, got, fresh)
    assert not bad, '\n'.join(bad)
    _synth_judge(h, fresh)


# ---------------------------------------------------------------------------------------------------------------------------------
# discriminator and feature engine

_EHIST = {}
LOSS_W = 0.5


def _disc_inputs(case, index, dev):
    key = ('disc', case.name, index)
    if key not in _EHIST:
        g = torch.Generator().manual_seed(7100 + 13 * index)
        sx, sg = hc.pass_scale(index)
        _EHIST[key] = ((torch.randn([hc.MAX_BATCH, case.imgc, case.R, case.R], generator=g) * sx).to(dev),
                       (torch.randn([hc.MAX_BATCH], generator=g) * sg).to(dev),
                       (torch.randn([hc.MAX_BATCH, case.imgc, case.R, case.R], generator=g) * sg).to(dev))
    return _EHIST[key]


def _run_disc_history(lib, dev, eng, case, h):
    m, keep, loss_valid, index, B = hc.EngineModel('disc'), [], False, 0, 0
    for op in h.ops:
        name = op[0]
        want = m.apply(op)
        if name == 'forward':
            index, B, loss_valid = m.passes - 1, op[1], False
            x = _disc_inputs(case, index, dev)[0][:B].contiguous()
            keep.append(x)
            _ok(lib, lib.la_disc_forward(eng.handle, _p(x), B, _s()), name)
        elif name == 'loss':
            buf = torch.empty([1], device=dev)
            keep.append(buf)
            _ok(lib, lib.la_disc_loss(eng.handle, LOSS_W, 0, _p(buf), _s()), name)
            loss_valid = True
        elif name == 'backward':
            _, dl, pre = _disc_inputs(case, index, dev)
            dl, g = dl[:B].contiguous(), pre[:B].clone()
            keep.append((dl, g))
            _ok(lib, lib.la_disc_backward(eng.handle, None if loss_valid else _p(dl), _p(g), op[1], _s()), name)
        elif name == 'set_precision':
            _ok(lib, lib.la_disc_set_precision(eng.handle, PREC[op[1]]), name)
        elif name == 'refused_forward':
            x = _disc_inputs(case, 0, dev)[0]
            _refused(lib, lib.la_disc_forward(eng.handle, _p(x), hc.MAX_BATCH + 1, _s()), name)
            assert want == hc.LA_ERR_ARG
        else:
            raise ValueError(name)
    torch.cuda.synchronize()


def _disc_probe(lib, dev, eng, case, img, dlogits, prec):
    """forward, logits, loss, backward from the case's dlogits (written), backward from the kept dlogits accumulated onto a seeded g_img"""
    _ok(lib, lib.la_disc_set_precision(eng.handle, PREC[prec]), 'la_disc_set_precision')
    logits = eng.forward(img.to(dev))
    loss = torch.full([1], 7.0, device=dev)
    _ok(lib, lib.la_disc_loss(eng.handle, LOSS_W, 0, _p(loss), _s()), 'la_disc_loss')
    gx = eng.backward(dlogits.to(dev))
    acc = torch.randn(list(gx.shape), generator=torch.Generator().manual_seed(9)).to(dev)
    _ok(lib, lib.la_disc_backward(eng.handle, None, _p(acc), 1, _s()), 'la_disc_backward')
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), loss=loss.cpu(), gx=gx.cpu(), acc=acc.cpu())


@pytest.mark.parametrize('h', hc.all_histories('disc'), ids=_ids(hc.all_histories('disc')))
def test_discriminator_history(dev, lib, h):
    case = ec.DISC_BY_NAME[h.case]
    assert case.B == hc.DISC_SHAPES[h.case] and case.kind == 'guarded'
    D, img, dlogits, r32, r64 = tes._ref(case)
    used = tes._disc_engine(dev, case, D, 'f32', max_batch=hc.MAX_BATCH)
    _run_disc_history(lib, dev, used, case, h)
    got = _disc_probe(lib, dev, used, case, img, dlogits, h.probe['prec'])
    fresh = _disc_probe(lib, dev, tes._disc_engine(dev, case, D, 'f32', max_batch=hc.MAX_BATCH), case, img, dlogits, h.probe['prec'])
    bad = []
    for key in ('logits', 'loss', 'gx', 'acc'):
        _same(f'{h.name} {key}', got[key], fresh[key], bad)
    assert not bad, '\n'.join(bad)
    tes._judge(f'disc {case.name} history {h.name} logits', h.probe['prec'], fresh['logits'], r32['logits'], r64['logits'], 'logits')
    tes._judge(f'disc {case.name} history {h.name} gradient', h.probe['prec'], fresh['gx'], r32['gx'], r64['gx'], 'gx_disc')


def _feat_inputs(case, F, index, dev):
    key = ('feat', case.name, index)
    if key not in _EHIST:
        g = torch.Generator().manual_seed(7200 + 13 * index)
        sx, sg = hc.pass_scale(index)
        _EHIST[key] = (((torch.randn([hc.MAX_BATCH, case.in_ch, case.res, case.res], generator=g) + 0.2) * sx).to(dev),
                       (torch.randn([hc.MAX_BATCH, F], generator=g) * sg).to(dev))
    return _EHIST[key]


def _run_feat_history(lib, dev, eng, case, h):
    m, keep, N, index = hc.EngineModel('feat'), [], 0, 0
    F = eng.num_features
    for op in h.ops:
        name = op[0]
        want = m.apply(op)
        if name == 'forward':
            index, N = m.passes - 1, op[1]
            x, out = _feat_inputs(case, F, index, dev)[0][:N].contiguous(), torch.empty([op[1], F], device=dev)
            keep.append((x, out))
            _ok(lib, lib.la_feat_forward(eng.handle, _p(x), N, _p(out), _s()), name)
        elif name in ('backward', 'refused_backward'):
            gf = _feat_inputs(case, F, index, dev)[1][:max(N, 1)].contiguous()
            gx = torch.full([max(N, 1), case.in_ch, case.res, case.res], 7.0, device=dev)
            keep.append((gf, gx))
            rc = lib.la_feat_backward(eng.handle, _p(gf), _p(gx), _s())
            (_refused if want else _ok)(lib, rc, name)
            if want:
                torch.cuda.synchronize()
                assert bool((gx == 7.0).all())
        elif name == 'pair_distance':
            index, N = m.passes - 1, 0
            xy = _feat_inputs(case, F, index, dev)[0][:2 * op[1]].contiguous()
            dist = torch.empty([op[1], eng.num_taps], dtype=torch.float64, device=dev)
            keep.append((xy, dist))
            eng.pair_distance_rows(xy, op[1], dist)
        elif name == 'set_precision':
            _ok(lib, lib.la_feat_set_precision(eng.handle, PREC[op[1]]), name)
        elif name == 'refused_forward':
            x, out = _feat_inputs(case, F, 0, dev)[0], torch.full([hc.MAX_BATCH + 1, F], 7.0, device=dev)
            _refused(lib, lib.la_feat_forward(eng.handle, _p(x), hc.MAX_BATCH + 1, _p(out), _s()), name)
            torch.cuda.synchronize()
            assert bool((out == 7.0).all())
        else:
            raise ValueError(name)
    torch.cuda.synchronize()


def _feat_probe(lib, dev, eng, x, gfeat, prec):
    _ok(lib, lib.la_feat_set_precision(eng.handle, PREC[prec]), 'la_feat_set_precision')
    f = eng.forward(x.to(dev))
    gx = eng.backward(gfeat.to(dev))
    dist = eng.pair_distance(x[:1].to(dev), x[1:2].to(dev))
    torch.cuda.synchronize()
    return dict(feat=f.cpu(), gx=gx.cpu(), dist=dist.cpu())


@pytest.mark.parametrize('h', hc.all_histories('feat'), ids=_ids(hc.all_histories('feat')))
def test_feature_engine_history(dev, lib, h):
    case = ec.FEAT_BY_NAME[h.case]
    assert case.N == hc.FEAT_SHAPES[h.case] and case.kind == 'guarded'
    ops, x, gfeat, r32, r64 = tes._ref(case)
    used = tes._feat_engine(dev, ops, case.in_ch, case.res, hc.MAX_BATCH, 'f32')
    _run_feat_history(lib, dev, used, case, h)
    got = _feat_probe(lib, dev, used, x, gfeat, h.probe['prec'])
    fresh = _feat_probe(lib, dev, tes._feat_engine(dev, ops, case.in_ch, case.res, hc.MAX_BATCH, 'f32'), x, gfeat, h.probe['prec'])
    bad = []
    for key in ('feat', 'gx', 'dist'):
        _same(f'{h.name} {key}', got[key], fresh[key], bad)
    assert not bad, '\n'.join(bad)
    tes._judge(f'feat {case.name} history {h.name} features', h.probe['prec'], fresh['feat'], r32['feat'], r64['feat'], 'feat')
    tes._judge(f'feat {case.name} history {h.name} gradient', h.probe['prec'], fresh['gx'], r32['gx'], r64['gx'], 'gx_feat')


PAIRS = [(a, b) for a in hc.MODES for b in hc.MODES if a != b]


@pytest.mark.parametrize('p1,p2', PAIRS, ids=[f'{a}-then-{b}' for a, b in PAIRS])
def test_backward_runs_in_the_precision_of_its_forward(dev, lib, p1, p2):
    """forward(P1), set_precision(P2), backward == forward(P1), backward, bit for bit (include/latentaug_hip.h, History contract); the setter
    then takes effect: the next forward / backward pair equals an engine created in P2"""
    case = ec.DISC_BY_NAME['imgc3']
    D, img, dlogits, _, _ = tes._ref(case)
    a, b, c = (tes._disc_engine(dev, case, D, p, max_batch=hc.MAX_BATCH) for p in (p1, p1, p2))
    xd, dl = img.to(dev), dlogits.to(dev)
    la, lb = a.forward(xd), b.forward(xd)
    _ok(lib, lib.la_disc_set_precision(b.handle, PREC[p2]), 'la_disc_set_precision')
    ga, gb = a.backward(dl), b.backward(dl)
    assert torch.equal(la, lb) and torch.equal(ga, gb), 'discriminator: the backward pass followed the setter'
    lc_, lb2 = c.forward(xd), b.forward(xd)
    assert torch.equal(lc_, lb2) and torch.equal(c.backward(dl), b.backward(dl)), 'discriminator: the setter did not take effect at the next forward'
    fcase = ec.FEAT_BY_NAME['conv-conv-conv-pool']
    ops, x, gfeat, _, _ = tes._ref(fcase)
    a, b, c = (tes._feat_engine(dev, ops, fcase.in_ch, fcase.res, hc.MAX_BATCH, p) for p in (p1, p1, p2))
    xd, gd = x.to(dev), gfeat.to(dev)
    fa, fb = a.forward(xd), b.forward(xd)
    _ok(lib, lib.la_feat_set_precision(b.handle, PREC[p2]), 'la_feat_set_precision')
    ga, gb = a.backward(gd), b.backward(gd)
    assert torch.equal(fa, fb) and torch.equal(ga, gb), 'feature engine: the backward pass followed the setter'
    assert torch.equal(c.forward(xd), b.forward(xd)) and torch.equal(c.backward(gd), b.backward(gd)), 'feature engine: the setter did not take effect'


# ---------------------------------------------------------------------------------------------------------------------------------
# latent loop

PREPROCS = (lc.PREPROC, ((1.2, 0.7, 1.0), (-0.1, 0.0, 0.3)))
_WIN = dict(w_lpips=3.0, Mf=5, kind='scalars')
LOOP_CASES = {
    'all-R32': lc.BY_NAME['all-R32'], 'all-W+-R32': lc.BY_NAME['all-W+-R32'],
    # (kind 'scalars': loop_cases.judge takes the loss scalars from the traced image, Adam and the gate; no seed search for a guard here)
    'win-R64': lc.LoopCase('win-R64', 64, 32, 2, Mx=3, w_pix=2.0, crop_pos=(9, 4), **_WIN),
    'win-R128-cols': lc.LoopCase('win-R128-cols', 128, 32, 2, crop_pos=(61, 45), **_WIN),
}


def _banks(case, b, gen):
    """the case's networks with the gen-th seeded bank contents (0: the case's own)"""
    if gen == 0:
        return b
    g = torch.Generator().manual_seed(9000 + gen)
    n = copy.copy(b)
    n.W = torch.randn(b.W.shape, generator=g) * 0.6 - 0.2 if b.W is not None else None
    n.X = torch.rand(b.X.shape, generator=g) * 1.6 - 0.9 if b.X is not None else None
    if b.fea is not None:
        with torch.no_grad():
            n.fea = [b.fnet(torch.rand([case.Mf, 3, lc.FEAT_CROP, lc.FEAT_CROP], generator=g) * 2 - 1).contiguous() for _ in range(case.imgc)]
    return n


def _rewrite_banks(la, case, nb):
    """the new bank contents written IN PLACE into the device tensors the loop handle was created on"""
    if nb.W is not None:
        la.W.copy_(nb.W)
    if nb.X is not None:
        off, cc = la.center_off, la.center_crop
        la.Xc.copy_(nb.X[:, :, off:off + cc, off:off + cc].permute(1, 0, 2, 3).reshape(la.Xc.shape))
    if nb.fea is not None:
        la.Fbank.copy_(torch.stack(nb.fea))


def _loop_w0(case, b, index, dev):
    g = torch.Generator().manual_seed(7300 + 13 * index)
    return (torch.randn(list(b.w0.shape), generator=g) * hc.pass_scale(index)[0]).to(dev)


def _rel(la, crop, case):
    return case.crop_pos if crop is None else (crop[0] - la.center_off, crop[1] - la.center_off)


def _loop_set_engine_precision(lib, la, which, mode):
    if which == 'g':
        la.engine.set_precision(mode)
    elif which == 'd':
        _ok(lib, lib.la_disc_set_precision(la.disc.handle, PREC[mode]), 'la_disc_set_precision')
    else:
        _ok(lib, lib.la_feat_set_precision(la.feat.handle, PREC[mode]), 'la_feat_set_precision')


def _loop_set_preproc(lib, la, k):
    scale, shift = PREPROCS[k]
    _ok(lib, lib.la_latent_opt_set_lpips_preproc(la._h, (C.c_float * 3)(*scale), (C.c_float * 3)(*shift), 3), 'la_latent_opt_set_lpips_preproc')


def _run_loop_history(lib, dev, la, case, b, h):
    m, index = hc.LoopModel(h.case, h.probe['prec']), 0
    assert (m.rows, m.cols) == ((la.loop_window, la.loop_window) if la.loop_window else ((0, 0), (0, 0)))
    for op in h.ops:
        name = op[0]
        want = m.apply(op)
        if name == 'run':
            _, B, losses, trace, crop = op
            tr = None if trace is None else {'want': {'w': ('w',), 'w+img': ('w', 'img'), 'grad': ('w', 'grad')}[trace]}
            la.run_local(_loop_w0(case, b, index, dev)[:B], want_losses=losses, crop_pos=_rel(la, crop, case), trace=tr)
            index += 1
        elif name == 'refused_run':
            w0 = _loop_w0(case, b, 0, dev)
            img, w_aug = la._empty_pair(case.max_batch)
            img.fill_(7.0)
            rc = lib.la_latent_opt_run(la._h, _p(w0), case.max_batch + 1, None, _p(img), _p(w_aug), None, _s())
            _refused(lib, rc, name)
            torch.cuda.synchronize()
            assert bool((img == 7.0).all()) and want == hc.LA_ERR_ARG
        elif name == 'set_graph':
            _ok(lib, lib.la_latent_opt_set_graph(la._h, op[1]), name)
        elif name == 'set_overlap':
            _ok(lib, lib.la_latent_opt_set_overlap(la._h, op[1]), name)
        elif name == 'set_rows':
            _ok(lib, lib.la_latent_opt_set_row_window(la._h, op[1], op[2]), name)
        elif name == 'set_cols':
            _ok(lib, lib.la_latent_opt_set_col_window(la._h, op[1], op[2]), name)
        elif name == 'set_time_trace':
            _ok(lib, lib.la_latent_opt_set_time_trace(la._h, op[1]), name)
        elif name == 'set_preproc':
            _loop_set_preproc(lib, la, op[1])
        elif name == 'engine_precision':
            _loop_set_engine_precision(lib, la, op[1], op[2])
        elif name == 'engine_schedule':
            _ok(lib, lib.la_synth_set_torgb_schedule(la.engine.handle, op[1]), name)
        elif name == 'invalidate_banks':
            torch.cuda.synchronize()
            _rewrite_banks(la, case, _banks(case, b, m.banks))
            _ok(lib, lib.la_latent_opt_invalidate_banks(la._h), name)
        else:
            raise ValueError(name)
    torch.cuda.synchronize()
    return m


def _fresh_loop(lib, dev, case, b, m, prec):
    """a new stack (synthesis, discriminator, feature engine, loop) on the bank contents and in the settings the history left"""
    la = tls._aug(case, _banks(case, b, m.banks), prec)
    _ok(lib, lib.la_latent_opt_set_graph(la._h, m.graph_mode), 'la_latent_opt_set_graph')
    if m.overlap != 2:
        _ok(lib, lib.la_latent_opt_set_overlap(la._h, m.overlap), 'la_latent_opt_set_overlap')
    if m.rows != (la.loop_window or (0, 0)) or m.cols != (la.loop_window or (0, 0)):
        _ok(lib, lib.la_latent_opt_set_row_window(la._h, *m.rows), 'la_latent_opt_set_row_window')
        _ok(lib, lib.la_latent_opt_set_col_window(la._h, *m.cols), 'la_latent_opt_set_col_window')
    _ok(lib, lib.la_latent_opt_set_time_trace(la._h, m.time_trace), 'la_latent_opt_set_time_trace')
    if m.preproc:
        _loop_set_preproc(lib, la, m.preproc)
    for which, mode in m.prec.items():
        if mode != prec and getattr(la, dict(g='engine', d='disc', f='feat')[which]) is not None:
            _loop_set_engine_precision(lib, la, which, mode)
    _ok(lib, lib.la_synth_set_torgb_schedule(la.engine.handle, m.sched), 'la_synth_set_torgb_schedule')
    return la


def _loop_probe(dev, la, case, b, probe):
    _, B, losses, _, crop = probe
    img, w_aug, L = la.run_local(b.w0[:B].to(dev), want_losses=losses, crop_pos=_rel(la, crop, case))
    torch.cuda.synchronize()
    return dict(img=img.cpu(), w_aug=w_aug.cpu(), losses=L.cpu() if losses else None, graph_state=la.graph_state)


@pytest.mark.parametrize('h', hc.all_histories('loop'), ids=_ids(hc.all_histories('loop')))
def test_loop_history(dev, lib, monkeypatch, h):
    case = LOOP_CASES[h.case]
    sh = hc.LOOP_SHAPES[h.case]
    assert (case.R, case.max_batch, case.w_disc > 0, case.w_lpips > 0, case.steps) == (sh['R'], sh['max_batch'], sh['disc'], sh['feat'], hc.LOOP_STEPS)
    assert case.window() == sh['crop']
    b = case.build()
    prec, probe = h.probe['prec'], h.probe['run']
    used = tls._aug(case, b, prec)
    m = _run_loop_history(lib, dev, used, case, b, h)
    got = _loop_probe(dev, used, case, b, probe)
    fresh_la = _fresh_loop(lib, dev, case, b, m, prec)
    fresh = _loop_probe(dev, fresh_la, case, b, probe)
    bad = []
    _same(f'{h.name} img_out', got['img'], fresh['img'], bad)
    _same(f'{h.name} w_aug_out', got['w_aug'], fresh['w_aug'], bad)
    if probe[2]:
        _same(f'{h.name} losses_out', got['losses'], fresh['losses'], bad)
    _, B, losses, _, crop = probe
    want_used, want_fresh = m.graph_state_after(B, losses, None, crop), 1 if m.replayable(losses, None) else 0
    if (got['graph_state'], fresh['graph_state']) != (want_used, want_fresh):
        bad.append(f"{h.name}: graph_state used {got['graph_state']} (model {want_used}), fresh {fresh['graph_state']} (model {want_fresh})")
    assert not bad, '\n'.join(bad)
    # the fresh stack against float64: a traced run of it, judged as test_hip_loop_shapes.py judges (the engines' K of the loosest mode in use)
    modes = [m.prec['g']] + ([m.prec['d']] if sh['disc'] else []) + [m.prec['f']]
    mode = max(modes, key=lambda k: lc.K_ENGINE[k])
    monkeypatch.setattr(lc, 'PREPROC', PREPROCS[m.preproc])
    jcase = copy.copy(case)
    jcase.crop_pos = _rel(fresh_la, crop, case)
    nb = _banks(case, b, m.banks)
    run, img, w_aug = tls._traced(fresh_la, jcase, nb, dev, B)
    v = lc.judge(jcase, nb, run, mode)
    assert not v.bad, '\n'.join(v.bad)
    if not m.windowed(sh['crop'] if crop is None else crop):          # (a windowed step is held against whole frames by budgets only: test_hip_synth_shapes.py)
        assert torch.equal(run['w_aug'], fresh['w_aug']) and torch.equal(img.cpu(), fresh['img']), 'the traced run of the fresh stack is not its probe'


# ---------------------------------------------------------------------------------------------------------------------------------
# package level

def _smoke_like_aug(dev, B):
    from latentaugment_amd.latent_aug import LatentAug
    from oracle import sg2_networks as nets
    res, wdim = 32, 64
    G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=512, channel_max=32, seed=0, noise_strength=0.05, w_dim=wdim, mapping_layers=1)
    g = torch.Generator().manual_seed(1)
    w0 = torch.randn([B, 1, wdim], generator=g)
    W = torch.randn([16, 1, wdim], generator=g).repeat(1, G.num_ws, 1)
    X = torch.rand([8, 2, res, res], generator=g) * 2 - 1
    opt = types.SimpleNamespace(img_resolution=res, batch_size=B, modalities_aug='A,B', opt_num_epochs=3, opt_lr=0.01, truncation_psi=1.0, w_pix=1.0, w_lpips=0.0,
                                w_latent=0.3, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False,
                                criterion_mode='gemm', final_noise_mode='const', precision='f16x2')
    return LatentAug('train', opt, None, [0], generator=G, banks={'W': W, 'X': X}), w0.to(dev)


def test_latent_aug_forward_after_other_batches_and_precisions(dev):
    """a lanes-eligible batch, an odd smaller one, the first batch again, with engine.set_precision to another mode and back in between: the
    last call is the first call of a fresh LatentAug"""
    B = 4
    used, w0 = _smoke_like_aug(dev, B)
    assert used.lanes_eligible(B) and not used.lanes_eligible(3)
    first = [t.clone() for t in used.forward(w0)]
    assert used.lanes_active
    used.engine.set_precision('bf16x3')
    used.forward(w0[:3] * 8.0)
    assert not used.lanes_active
    used.engine.set_precision('f16x2')
    last = used.forward(w0)
    fresh, _ = _smoke_like_aug(dev, B)
    want = fresh.forward(w0)
    torch.cuda.synchronize()
    for name, a, b_, c in (('img', first[0], last[0], want[0]), ('w_aug', first[1], last[1], want[1])):
        assert torch.equal(b_, c), f'{name}: the used LatentAug differs from a fresh one'
        assert torch.equal(a, c), f'{name}: the first call differs from a fresh one'


def test_projector_without_noise_after_a_run_with_noise(dev):
    """project(optimize_noise=True), then project(other targets) without the flag on the same Projector == a fresh Projector's call"""
    import projector_cases as pj
    from test_hip_projector_noise import _projector
    case = pj.make_case('w', 0.1)
    tgt = pj.targets().to(dev)
    used, fresh = _projector(dev, case, 'f16x2', 3), _projector(dev, case, 'f16x2', 3)
    used.project(tgt, num_steps=3, w_pix=0.1, seed=4, optimize_noise=True)
    other = tgt.flip(0).contiguous()
    a = used.project(other[:2], num_steps=3, w_pix=0.1, seed=5)
    b = fresh.project(other[:2], num_steps=3, w_pix=0.1, seed=5)
    torch.cuda.synchronize()
    assert 'noises' not in a and set(a) == set(b)
    for key in ('w', 'img', 'loss'):
        assert torch.equal(a[key], b[key]), key
