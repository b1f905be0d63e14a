"""Host side of the conv2d op (la_conv_op.hip, ops.conv2d_resample): exported symbols, argument checks that refuse a call before any
launch, the workspace query, dtype / device refusals of the Python wrapper, and the proof that the case list of test_hip_conv2d_op.py
reaches every kernel path it claims to.  No GPU."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv2d_op_cases as cc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('la_conv2d_f32', 'la_conv2d_wgrad_f32', 'la_conv2d_workspace_bytes', 'la_conv2d_uses_engine', 'la_conv2d_wgrad_slices')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    from latentaugment_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    for name in NEW:
        assert name + '(' in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.la_abi_version() == 1


# a valid call: B, Cin, H, W, Cout, kh, kw, Hout, Wout, stride, pady, padx, groups, flip_weight, transpose
GOOD = dict(B=2, Cin=4, H=8, W=8, Cout=6, kh=3, kw=3, Hout=8, Wout=8, stride=1, pady=1, padx=1, groups=1, flip_weight=1, transpose=0)
ORDER = list(GOOD)


def _call(lib, entry, ptrs=True, **over):
    a = dict(GOOD, **over)
    buf = (C.c_float * 4)()      # never dereferenced: every call below is refused before a launch
    p = C.addressof(buf) if ptrs else None
    rc = getattr(lib, entry)(p, p, p, p, 16, *[a[k] for k in ORDER], None)
    return rc, (lib.la_last_error() or b'').decode()


@pytest.mark.parametrize('entry', ['la_conv2d_f32', 'la_conv2d_wgrad_f32'])
def test_arguments_are_checked_before_any_launch(lib, entry):
    rc, msg = _call(lib, entry, ptrs=False)
    assert rc != 0 and 'null pointer' in msg
    for over, word in [
        (dict(B=0), 'empty'), (dict(Cin=0), 'empty'), (dict(H=0), 'empty'), (dict(kw=0), 'empty'),
        (dict(groups=3), 'groups'), (dict(groups=4), 'groups'), (dict(groups=0), 'groups'),
        (dict(kh=8, pady=4, Hout=9), '7x7'), (dict(kw=8, padx=4, Wout=9), '7x7'),
        (dict(stride=9, Hout=1, Wout=1), 'stride'), (dict(stride=0), 'stride'),
        (dict(pady=-1, Hout=6), 'negative padding'), (dict(padx=-1, Wout=6), 'negative padding'),
        (dict(H=2, pady=0, Hout=0), 'smaller than 1x1'), (dict(W=1, padx=0, Wout=-1), 'smaller than 1x1'),
        (dict(transpose=1, H=1, kh=1, pady=1, Hout=-1), 'smaller than 1x1'),
        (dict(Hout=9), 'output size'), (dict(transpose=1, Hout=9, Wout=8), 'output size'),
    ]:
        rc, msg = _call(lib, entry, **over)
        assert rc != 0 and word in msg, (over, rc, msg)


def test_missing_workspace_is_refused(lib):
    a = dict(GOOD, Cout=8)      # engine path: needs scratch
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    rc = lib.la_conv2d_f32(p, p, p, None, 0, *[a[k] for k in ORDER], None)
    assert rc != 0 and 'workspace' in lib.la_last_error().decode()
    wsbuf = (C.c_float * 12)()      # 16 aligned bytes inside a live buffer: too small for the 2304 bytes this call needs
    ws = (C.addressof(wsbuf) + 15) & ~15
    rc = lib.la_conv2d_wgrad_f32(p, p, p, ws, 16, *[a[k] for k in ORDER], None)
    assert rc != 0 and 'workspace' in lib.la_last_error().decode()


def test_workspace_query(lib):
    shapes = [(4, 4, 8, 8, 6, 3, 3, 8, 8, 1, 1, 0), (8, 8, 8, 8, 8, 3, 3, 8, 8, 1, 1, 0), (64, 64, 8, 8, 64, 3, 3, 8, 8, 1, 1, 0),
              (8, 8, 8, 8, 8, 3, 3, 17, 17, 2, 1, 1), (8, 8, 17, 17, 8, 3, 3, 8, 8, 2, 1, 0), (3, 3, 9, 9, 5, 5, 5, 9, 9, 1, 1, 0),
              (512, 512, 16, 16, 512, 3, 3, 16, 16, 1, 1, 0), (8, 8, 8, 8, 16, 3, 3, 8, 8, 1, 2, 0)]
    for op in (0, 1):
        for s in shapes:
            prev = 0
            for b in (1, 2, 3, 4, 6, 8, 13, 16, 32):
                n = lib.la_conv2d_workspace_bytes(op, b, *s[1:])
                assert n > 0 and n >= prev, (op, s, b, n, prev)
                prev = n
    # a real layer: packed weights (+ nothing else at 256^2) forward, 64 slices of dW for the weight gradient
    assert lib.la_conv2d_workspace_bytes(0, 8, 128, 256, 256, 128, 3, 3, 256, 256, 1, 1, 0) >= 128 * 128 * 9 * 4
    assert lib.la_conv2d_workspace_bytes(1, 8, 128, 256, 256, 128, 3, 3, 256, 256, 1, 1, 0) >= 64 * 128 * 128 * 9 * 4


def test_wrapper_refuses_cpu_and_float16():
    from latentaugment_amd import _lib, ops
    x, w = torch.zeros([1, 4, 8, 8]), torch.zeros([4, 4, 3, 3])
    for fn in (ops.conv2d_resample, ops.conv2d, ops.conv_transpose2d):
        with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
            fn(x, w)
        with pytest.raises(_lib.LatentAugHipError):
            fn(x.half(), w.half())
    with pytest.raises(AssertionError):
        ops.conv2d_resample(x, w.half())


def test_path_plan_restates_the_library(lib):
    """path_plan's predicate and slice rule are the library's own (la_conv2d_uses_engine, la_conv2d_wgrad_slices) on every case."""
    for c in cc.CASES:
        p = cc.path_plan(c)
        g = p['call']
        k = (g['kh'], g['kw'], g['stride'], g['groups'])
        assert (p['fwd'] == 'engine') == bool(lib.la_conv2d_uses_engine(0, g['cout'], *k)), c['name']
        assert (p['dgrad'] == 'engine') == bool(lib.la_conv2d_uses_engine(0, g['cin'], *k)), c['name']
        assert (p['wgrad'] == 'engine') == bool(lib.la_conv2d_uses_engine(1, g['cout'], *k)), c['name']
        assert p['slices'] == lib.la_conv2d_wgrad_slices(g['n'], g['cin'], g['h'], g['w'], g['cout'], g['kh'], g['kw'], g['oh'], g['ow'],
                                                         g['stride'], g['groups'], int(g['transpose'])), c['name']
        assert g['oh'] >= 1 and g['ow'] >= 1, c['name']


def test_case_list_covers_every_form():
    plans = {c['name']: cc.path_plan(c) for c in cc.CASES}
    for q in ('fwd', 'dgrad', 'wgrad'):
        assert {p[q] for p in plans.values()} == {'engine', 'generic'}, q
    for path in ('engine', 'generic'):
        # stride 1 and 2 and the transposed form on the engine; the generic path sees them too (ragged channels, 5x5 / 7x7, stride 4)
        sel = [p['call'] for p in plans.values() if p['fwd'] == path]
        assert {1, 2} <= {g['stride'] for g in sel}, path
        assert any(g['transpose'] for g in sel) and any(not g['transpose'] for g in sel), path
        assert any(g['transpose'] and g['stride'] == 2 for g in sel), path
    assert any(p['call']['stride'] == 4 and p['call']['transpose'] for p in plans.values())
    assert {1, 2, 3} <= {c['groups'] for c in cc.CASES}
    for grp in (1, 2):
        assert any(p['fwd'] == 'engine' and p['call']['groups'] == grp for p in plans.values())
    assert any(p['wgrad'] == 'engine' and p['call']['groups'] == 3 for p in plans.values())
    assert any((c['cout'] // c['groups']) % 4 != 0 for c in cc.CASES)
    assert {(1, 1), (1, 3), (3, 1), (3, 3), (5, 5), (7, 7)} <= {(c['kh'], c['kw']) for c in cc.CASES}
    assert {p['call']['branch'] for p in plans.values()} == {'k1_down', 'k1_up', 'down', 'up', 'plain', 'fallback'}
    assert {True, False} <= {c['flip_weight'] for c in cc.CASES}
    assert any(c['up'] == 2 and c['down'] == 2 for c in cc.CASES) and any(c['up'] == 4 for c in cc.CASES)
    assert any(c['x'][0] == 1 for c in cc.CASES) and any(c['x'][1] == 1 for c in cc.CASES) and any(c['cout'] == 1 for c in cc.CASES)
    assert any(c['x'][2] != c['x'][3] for c in cc.CASES)
    assert any(min(cc._pad4(c['padding'])) < 0 and plans[c['name']]['call']['branch'] == 'fallback' for c in cc.CASES)
    assert any(len(set(cc._pad4(c['padding']))) > 2 for c in cc.CASES)
    # weight gradient: several K slices, several row / column tiles with ragged tails, a ragged 16-pixel chunk
    assert sum(p['slices'] > 1 for p in plans.values()) >= 3
    assert plans[cc.MANY_SLICES]['slices'] >= 32 and plans[cc.MANY_SLICES]['wgrad'] == 'engine'
    assert all(plans[n]['wgrad'] == w and plans[n]['fwd'] == w for n, w in zip(cc.SECOND_ORDER, ('engine', 'generic')))
    assert {plans[n]['call']['branch'] for n in cc.SECOND_ORDER_RESAMPLED} == {'up', 'down', 'k1_up', 'k1_down', 'fallback'}
    assert {plans[n]['fwd'] for n in cc.SECOND_ORDER_RESAMPLED} == {'engine', 'generic'}
    assert plans[cc.GRAPH_CASE]['fwd'] == plans[cc.GRAPH_CASE]['dgrad'] == plans[cc.GRAPH_CASE]['wgrad'] == 'engine'
    t = plans['tiles_132x144']['call']
    assert t['cout'] > cc.WG_TILE and t['cout'] % cc.WG_TILE and t['cin'] * 9 > cc.WG_TILE
    assert any(p['call']['ow'] % cc.WG_CHUNK and p['call']['ow'] > cc.WG_CHUNK for p in plans.values())
