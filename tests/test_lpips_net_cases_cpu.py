"""The AlexNet / SqueezeNet LPIPS nets without a GPU: the float64 restatement of tests/lpips_net_cases.py against the reference's own
float64 run (tests/golden/lpips_nets.npz, written by tests/golden/make_golden_lpips_nets.py), the op-list builders,
lpips_reference_net, the lpips_net option, the host side of la_feat_workspace_bytes, the minimum input sizes and torch's tie rule
of the max pool."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as lc  # noqa: E402
import lpips_net_cases as nc  # noqa: E402
import workspace_cases as wc  # noqa: E402
from latentaugment_amd.synthesis import alexnet_lpips_ops, squeezenet_lpips_ops  # noqa: E402,F401  (every test here is about these nets)

CASES = [(net, R) for net in ('alex', 'squeeze') for R in nc.SIZES[net]]


@pytest.fixture(scope='module')
def gn(golden_dir):
    return np.load(os.path.join(golden_dir, 'lpips_nets.npz'))


def _lib_loaded():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


@pytest.mark.parametrize('net,R', CASES)
def test_float64_restatement_reproduces_the_reference(gn, net, R):
    ops = nc.cast_ops(nc.golden_ops(gn, net), torch.float64)
    z = lambda a: lc.zscore(nc.gray3(a), gn['mean'], gn['std'])      # noqa: E731
    key = f'{net}{R}'
    x, y, x1, bank = (z(gn[f'{key}_{k}']) for k in ('x', 'y', 'x1', 'bank'))
    d = nc.pair_distance(ops, x, y).numpy()
    assert d.shape == (3, nc.NTAPS[net])
    np.testing.assert_allclose(d, gn[f'{key}_layers64'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d.sum(1), gn[f'{key}_pair64'], rtol=1e-12, atol=0)
    xg = x1.clone().requires_grad_(True)
    tr = nc.forward_tr(ops, xg, bank)
    np.testing.assert_allclose(float(tr.detach()), float(gn[f'{key}_tr64']), rtol=1e-12, atol=0)
    (g,) = torch.autograd.grad(tr, [xg])
    g_x = g / torch.tensor(gn['std']).double().reshape(1, 3, 1, 1)
    scale = float(np.abs(gn[f'{key}_tr_grad64']).max())
    np.testing.assert_allclose(g_x.numpy(), gn[f'{key}_tr_grad64'], rtol=0, atol=1e-12 * scale)
    fx, fy = nc.feature_vector(ops, x), nc.feature_vector(ops, y)
    np.testing.assert_allclose((fx - fy).square().sum(1).numpy(), gn[f'{key}_pair64'], rtol=1e-11, atol=0)


@pytest.mark.parametrize('net,R', CASES)
def test_fixture_conditions(gn, net, R):
    """What the maker asserts: channel norms, the float32 gradient beside the float64 one, and the two normalisation forms agreeing."""
    key = f'{net}{R}'
    assert float(gn[f'{key}_min_norm']) >= 0.03 and 0 <= int(gn[f'{key}_seed']) < 50
    g64, g32 = gn[f'{key}_tr_grad64'], gn[f'{key}_tr_grad32']
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    assert float(np.abs(g32 - g64).max()) <= 1e-5 * float(np.abs(g64).max())
    ops = nc.cast_ops(nc.golden_ops(gn, net), torch.float64)
    x = lc.zscore(nc.gray3(gn[f'{key}_x']), gn['mean'], gn['std'])
    y = lc.zscore(nc.gray3(gn[f'{key}_y']), gn['mean'], gn['std'])
    a, b = nc.pair_distance(ops, x, y, 'reference'), nc.pair_distance(ops, x, y, 'engine')
    assert float(((a - b).abs() / a).max()) < 2.0 ** -23
    # the first pair is the close one
    assert float(np.abs(gn[f'{key}_y'][0] - gn[f'{key}_x'][0]).max()) <= 0.0201
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_nets.npz')) < 1 << 20


@pytest.mark.parametrize('net', ['alex', 'squeeze'])
def test_builders_and_reference_net(gn, net):
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import LPIPS_ZSCORE_MEAN, LPIPS_ZSCORE_STD, alexnet_lpips_ops, lpips_reference_net, squeezenet_lpips_ops
    trunk, lin = nc.golden_state_dicts(gn, net)
    lins = [lin[f'lin{k}.model.1.weight'].reshape(-1) for k in range(nc.NTAPS[net])]
    ops = (alexnet_lpips_ops if net == 'alex' else squeezenet_lpips_ops)(trunk, lins)
    want = nc.golden_ops(gn, net)
    assert [op[0] for op in ops] == [op[0] for op in want] and ops[-1][0] == 'tap'
    for a, b in zip(ops, want):
        assert len(a) == len(b)
        assert all(torch.equal(u, v) if torch.is_tensor(u) else u == v for u, v in zip(a[1:], b[1:]))
    kinds = [op[0] for op in ops]
    if net == 'alex':
        assert kinds == ['conv', 'tap', 'maxpool3', 'conv', 'tap', 'maxpool3', 'conv', 'tap', 'conv', 'tap', 'conv', 'tap']
        assert [op[3:] for op in ops if op[0] == 'conv'] == [(4, 2), (1, 2), (1, 1), (1, 1), (1, 1)]
        assert [op[1] for op in ops if op[0] == 'maxpool3'] == [False, False]
    else:
        assert kinds == ['conv', 'tap', 'maxpool3', 'fire', 'fire', 'tap', 'maxpool3', 'fire', 'fire', 'tap', 'maxpool3', 'fire', 'tap', 'fire', 'tap',
                         'fire', 'tap', 'fire', 'tap']
        assert ops[0][3:] == (2, 0) and all(op[1] is True for op in ops if op[0] == 'maxpool3')
    with pytest.raises(ValueError):
        (alexnet_lpips_ops if net == 'alex' else squeezenet_lpips_ops)(trunk, lins[:-1])
    desc = lpips_reference_net(trunk, lin, net)
    assert sum(op[0] == 'tap' for op in desc.ops) == nc.NTAPS[net]
    assert all(torch.equal(a[1], b) for a, b in zip([op for op in desc.ops if op[0] == 'tap'], lins))      # every lin kept, in order
    np.testing.assert_allclose(desc.pre_scale, [1 / s for s in LPIPS_ZSCORE_STD])
    np.testing.assert_allclose(desc.pre_shift, [-m / s for m, s in zip(LPIPS_ZSCORE_MEAN, LPIPS_ZSCORE_STD)])
    bad = dict(lin)
    bad['lin1.model.1.weight'] = -lin['lin1.model.1.weight'] - 0.1
    with pytest.raises(_lib.LatentAugHipError, match='negative'):
        lpips_reference_net(trunk, bad, net)
    with pytest.raises(_lib.LatentAugHipError, match='need'):
        lpips_reference_net(trunk, {k: v for k, v in lin.items() if k != 'lin0.model.1.weight'}, net)
    with pytest.raises(ValueError, match='net_type'):
        lpips_reference_net(trunk, lin, 'resnet')


REQUIRED = dict(img_resolution=64, batch_size=1, modalities_aug='A,B', opt_num_epochs=1, opt_lr=0.01, truncation_psi=1.0, w_pix=0.0, w_lpips=1.0,
                w_latent=0.0, w_disc=0.0, crop_size_aug=32, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False)


def test_lpips_net_option_and_paths(tmp_path):
    import argparse
    from latentaugment_amd._lib import LatentAugHipError
    from latentaugment_amd.augments.latent_aug import LatentAugment
    from latentaugment_amd.loop_options import LoopOptions, resolve_perceptual_net
    parser = lambda: LatentAugment.modify_commandline_options(argparse.ArgumentParser(), True)      # noqa: E731
    base = ['--model_dir', 'm', '--interim_dir', 'i']
    assert parser().parse_args(base).lpips_net == 'vgg' and parser().parse_args(base).lpips_trunk_path is None
    assert parser().parse_args(base + ['--lpips_net', 'alex']).lpips_net == 'alex'
    with pytest.raises(SystemExit):
        parser().parse_args(base + ['--lpips_net', 'resnet'])

    def opts(**kw):
        return LoopOptions.from_opt(types.SimpleNamespace(**{**REQUIRED, **kw}))

    def res(**kw):
        return resolve_perceptual_net(opts(**kw))
    assert opts().lpips_net == 'vgg' and opts(lpips_script='lpips').lpips_net == 'vgg'
    assert opts(lpips_net='alex').lpips_net == 'vgg'      # read only on the LPIPS-class branch
    assert opts(lpips_script='lpips', lpips_net='alex').lpips_net == 'alex' and opts(lpips_script='lpips', lpips_net='squeeze').lpips_net == 'squeeze'
    with pytest.raises(LatentAugHipError, match='lpips_net'):
        opts(lpips_script='lpips', lpips_net='resnet')
    lane = opts(lpips_script='lpips', lpips_net='alex', batch_size=4).lane(4)
    assert lane.lpips_net == 'alex'
    d = tmp_path / 'models'
    d.mkdir()
    files = {n: str(d / n) for n in ('alexnet.pth', 'lpips_alex.pth', 'squeezenet1_1.pth', 'lpips_squeeze.pth', 'vgg16.pth', 'lpips_vgg.pth', 't.pth', 'l.pth')}
    for net, names in (('alex', ('alexnet.pth', 'lpips_alex.pth')), ('squeeze', ('squeezenet1_1.pth', 'lpips_squeeze.pth'))):
        # nothing on disk: the message names what is looked for
        for extra in (dict(), dict(model_dir=str(d)), dict(lpips_trunk_path=files['t.pth'])):
            with pytest.raises(NotImplementedError) as e:
                res(lpips_script='lpips', lpips_net=net, **extra)
            assert names[0] in str(e.value) and names[1] in str(e.value) and 'lpips_trunk_path' in str(e.value)
    for n in files:
        open(files[n], 'w').close()
    assert res(lpips_script='lpips', lpips_net='alex', model_dir=str(d)) == ('reference', (files['alexnet.pth'], files['lpips_alex.pth'], 'alex'))
    assert res(lpips_script='lpips', lpips_net='squeeze', model_dir=str(d)) == ('reference', (files['squeezenet1_1.pth'], files['lpips_squeeze.pth'], 'squeeze'))
    assert res(lpips_script='lpips', lpips_net='alex', model_dir=str(d), lpips_trunk_path=files['t.pth'], lpips_lin_path=files['l.pth']) == \
        ('reference', (files['t.pth'], files['l.pth'], 'alex'))
    # lpips_vgg_path is the 'vgg' trunk's option: another trunk does not take it
    assert res(lpips_script='lpips', lpips_net='alex', model_dir=str(d), lpips_vgg_path=files['vgg16.pth'])[1][0] == files['alexnet.pth']
    # 'vgg': unchanged, and lpips_trunk_path comes before lpips_vgg_path
    assert res(lpips_script='lpips', model_dir=str(d)) == ('reference', (files['vgg16.pth'], files['lpips_vgg.pth']))
    assert res(lpips_script='lpips', lpips_net='vgg', model_dir=str(d), lpips_vgg_path=files['t.pth']) == ('reference', (files['t.pth'], files['lpips_vgg.pth']))
    assert res(lpips_script='lpips', model_dir=str(d), lpips_trunk_path=files['l.pth'], lpips_vgg_path=files['t.pth'])[1][0] == files['l.pth']
    # a crop too small for the net: refused with the minimum named, before anything touches a device
    for net, lo in nc.MIN_RES.items():
        with pytest.raises(LatentAugHipError, match=f'at least {lo}'):
            res(lpips_script='lpips', lpips_net=net, model_dir=str(d), crop_size_aug=lo - 1)
        assert res(lpips_script='lpips', lpips_net=net, model_dir=str(d), crop_size_aug=lo)[1][2] == net


def _ex(records):
    """(la_feat_op array, record count) of ops written as (kind, cin, cout, k, stride, pad, ceil_mode, squeeze, expand1, expand3), short
    tuples padded with zeros: a general op becomes its record followed by its LA_FEAT_OP_ARGS records, as the header describes."""
    from latentaugment_amd import _lib
    out = []
    for r in records:
        kind, cin, cout, k, stride, pad, ceil, sq, e1, e3 = (tuple(r) + (0,) * 10)[:10]
        out.append((kind, cin, cout))
        if kind == CONV:
            out += [(ARGS, k, stride), (ARGS, pad, 0)]
        elif kind == POOL3:
            out.append((ARGS, ceil, 0))
        elif kind == FIRE:
            out += [(ARGS, sq, e1), (ARGS, e3, 0)]
    return (_lib.FeatOp * len(out))(*[_lib.FeatOp(*o) for o in out]), len(out)


def test_old_lists_keep_their_bytes_and_the_entries_are_the_two_there_were():
    _lib, lib = _lib_loaded()
    feat_entries = sorted(n for n in _lib.SIGNATURES if n.startswith('la_feat_') and ('create' in n or 'workspace' in n))
    assert feat_entries == ['la_feat_create', 'la_feat_pair_workspace_bytes', 'la_feat_workspace_bytes']
    import json
    pinned = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_sizes.json')))
    got = wc.measure(lib)
    assert all(got[k] == v for k, v in pinned.items() if k.startswith('feat-')) and any(k.startswith('feat-') for k in pinned)
    # an argument record without its op, an op without its argument records
    for recs in ([(ARGS, 3, 1), (TAP, 3, 3)], [(CONV, 3, 8), (TAP, 8, 8)], [(CONV, 3, 8), (ARGS, 3, 1), (TAP, 8, 8)], [(POOL3, 3, 3), (TAP, 3, 3)]):
        arr = (_lib.FeatOp * len(recs))(*[_lib.FeatOp(*o) for o in recs])
        assert lib.la_feat_workspace_bytes(len(recs), arr, 3, 32, 1) == 0 and lib.la_last_error().startswith(b'feat')
    # a one-pixel input: only in front of a general op
    one = (_lib.FeatOp * 1)(_lib.FeatOp(TAP, 4, 4))
    assert lib.la_feat_workspace_bytes(1, one, 4, 1, 1) == 0
    arr, n = _ex([(CONV, 4, 8, 3, 1, 1), (TAP, 8, 8)])
    assert lib.la_feat_workspace_bytes(n, arr, 4, 1, 1) > 0


CONV, TAP, POOL3, FIRE, ARGS = 6, 1, 7, 8, 9
MALFORMED = {
    'k > 11': [(CONV, 3, 8, 13, 4, 2), (TAP, 8, 8)],
    'stride 3': [(CONV, 3, 8, 5, 3, 2), (TAP, 8, 8)],
    'pad 6': [(CONV, 3, 8, 11, 1, 6), (TAP, 8, 8)],
    'cout % 4': [(CONV, 3, 6, 3, 1, 1), (TAP, 6, 6)],
    'cin 3 behind the first op': [(TAP, 3, 3), (TAP, 3, 3), (CONV, 3, 8, 3, 1, 1), (TAP, 8, 8)],
    'cin mismatch': [(CONV, 4, 8, 3, 1, 1), (TAP, 8, 8)],
    'fire cout != e1 + e3': [(CONV, 3, 16, 3, 1, 1), (FIRE, 16, 24, 0, 0, 0, 0, 4, 16, 16), (TAP, 24, 24)],
    'fire cin mismatch': [(CONV, 3, 16, 3, 1, 1), (FIRE, 8, 32, 0, 0, 0, 0, 4, 16, 16), (TAP, 32, 32)],
    'fire squeeze % 4': [(CONV, 3, 16, 3, 1, 1), (FIRE, 16, 32, 0, 0, 0, 0, 6, 16, 16), (TAP, 32, 32)],
    'kernel larger than the padded input': [(CONV, 3, 8, 11, 4, 2), (TAP, 8, 8), (POOL3, 8, 8), (CONV, 8, 8, 11, 1, 0), (TAP, 8, 8)],
    'pool on one pixel': [(CONV, 3, 8, 11, 4, 2), (POOL3, 8, 8), (POOL3, 8, 8, 0, 0, 0, 1), (POOL3, 8, 8, 0, 0, 0, 1), (TAP, 8, 8)],
    'floor pool on two pixels': [(CONV, 3, 8, 11, 4, 2), (POOL3, 8, 8), (CONV, 8, 8, 2, 1, 0), (POOL3, 8, 8), (TAP, 8, 8)],
    'no tap': [(CONV, 3, 8, 3, 1, 1)],
    'unknown kind': [(10, 3, 3), (TAP, 3, 3)],
}


@pytest.mark.parametrize('name', sorted(MALFORMED))
def test_general_lists_refused_before_any_launch(name):
    _lib, lib = _lib_loaded()
    arr, n = _ex(MALFORMED[name])
    assert lib.la_feat_workspace_bytes(n, arr, 3, 35, 2) == 0, name
    msg = lib.la_last_error().decode()
    assert msg.startswith('feat'), msg
    if name not in ('no tap', 'unknown kind'):
        bad = {'cin 3 behind the first op': 2, 'fire cout != e1 + e3': 1, 'fire cin mismatch': 1, 'fire squeeze % 4': 1,
               'kernel larger than the padded input': 3, 'pool on one pixel': 3, 'floor pool on two pixels': 3}.get(name, 0)
        assert f'op {bad}:' in msg, (name, msg)      # the index of the op that is refused
    # create refuses the same list before it touches the workspace or the stream
    h = C.c_void_p()
    buf = (C.c_char * 64)()
    params = (C.c_void_p * 16)(*[C.cast(buf, C.c_void_p).value] * 16)
    assert lib.la_feat_create(n, arr, params, 16, 3, 35, 2, buf, 64, None, C.byref(h)) == -1 and not h.value
    # a well-formed neighbour is measured
    ok, m = _ex([(CONV, 3, 8, 11, 4, 2), (TAP, 8, 8), (POOL3, 8, 8), (FIRE, 8, 32, 0, 0, 0, 0, 4, 16, 16), (TAP, 32, 32)])
    assert lib.la_feat_workspace_bytes(m, ok, 3, 35, 2) > 0


def _descs_of(ops):
    """records of an op list (shape-only tensors), as FeatureEngine writes them"""
    rec, c = [], 3
    for op in ops:
        if op[0] == 'conv':
            rec.append((CONV, c, op[1].shape[0], op[1].shape[2], op[3], op[4]))
            c = op[1].shape[0]
        elif op[0] == 'tap':
            rec.append((TAP, c, c))
        elif op[0] == 'maxpool3':
            rec.append((POOL3, c, c, 0, 0, 0, int(op[1])))
        else:
            sq, e1, e3 = op[1].shape[0], op[3].shape[0], op[5].shape[0]
            rec.append((FIRE, c, e1 + e3, 0, 0, 0, 0, sq, e1, e3))
            c = e1 + e3
    return _ex(rec)


def _torch_taps(ops, R):
    x = torch.zeros([1, 3, R, R])
    return [tuple(f.shape) for f, _ in nc.tapped(ops, x, 'engine')]


@pytest.mark.parametrize('net', ['alex', 'squeeze'])
def test_minimum_input_size_against_torch(net):
    """alex >= 31 and squeeze >= 17: one less raises in torch and is refused by la_feat_workspace_bytes; from the minimum on both agree."""
    from latentaugment_amd.synthesis import alexnet_lpips_ops, squeezenet_lpips_ops
    _lib, lib = _lib_loaded()
    sd, lin = nc.full_width_state_dicts(net)
    sd = {k: v.float() for k, v in sd.items()}
    lins = [lin[f'lin{k}.model.1.weight'].reshape(-1).float() for k in range(nc.NTAPS[net])]
    ops = (alexnet_lpips_ops if net == 'alex' else squeezenet_lpips_ops)(sd, lins)
    arr, n = _descs_of(ops)
    lo = nc.MIN_RES[net]
    with pytest.raises(RuntimeError):
        _torch_taps(ops, lo - 1)
    assert lib.la_feat_workspace_bytes(n, arr, 3, lo - 1, 2) == 0 and b'op ' in lib.la_last_error()
    for R in (lo, lo + 1, lo + 2, lo + 3, 64):
        shapes = _torch_taps(ops, R)
        assert shapes[-1][2] >= 1
        assert lib.la_feat_workspace_bytes(n, arr, 3, R, 2) > 0, (R, lib.la_last_error())
    assert _torch_taps(ops, lo)[-1][2:] == (1, 1)


def test_torch_takes_the_first_maximum():
    """The rule the pool's gradient restates: among equal maxima of a window the first in row-major scan order takes the gradient, in
    floor and in ceil mode, partial windows included."""
    for ceil in (False, True):
        for R in (3, 4, 5, 8):
            x = torch.ones([1, 1, R, R], dtype=torch.float64, requires_grad=True)
            y = F.max_pool2d(x, 3, 2, ceil_mode=ceil)
            (g,) = torch.autograd.grad(y.sum(), [x])
            want = torch.zeros([R, R], dtype=torch.float64)
            for oy in range(y.shape[2]):
                for ox in range(y.shape[3]):
                    want[2 * oy, 2 * ox] += 1
            assert torch.equal(g[0, 0], want), (ceil, R)
    x = torch.tensor([[0., 2., 2.], [2., 1., 2.], [0., 0., 0.]], dtype=torch.float64).reshape(1, 1, 3, 3).requires_grad_(True)
    (g,) = torch.autograd.grad(F.max_pool2d(x, 3, 2).sum(), [x])
    assert g.flatten().tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
