"""The history tables of tests/history_cases.py without a GPU: every required pair of (state before the probe, state of the probe) is reached
by a hand-written history, the random histories are a pure function of their seeds, every history keeps the length limit and is valid under
the state model, every window a history or a probe uses is really PLANNED at its shape (la_synth_plan_query, host only), and
la_latent_opt_invalidate_banks is declared and bound."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_cases as hc  # noqa: E402
import loop_cases as lc  # noqa: E402
import synth_cases as sc  # noqa: E402
import test_hip_image_chain as chain  # noqa: E402
from test_synth_plan_cpu import PREC, query  # noqa: E402

KINDS = ('synth', 'disc', 'feat', 'loop')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('kind', KINDS)
def test_every_required_pair_is_reached(kind):
    table = hc.reach(kind)
    missing = [(axis, p) for axis, want in hc.REQUIRED[kind].items() for p in want if not table[axis][p]]
    assert not missing, missing
    # nothing is reached that the tables do not name (a typo in a state class would hide here)
    extra = [(axis, p) for axis, row in table.items() for p in row if p not in hc.REQUIRED[kind][axis]]
    assert not extra, extra


@pytest.mark.parametrize('kind', KINDS)
def test_random_histories_are_a_function_of_their_seeds(kind):
    assert len(hc.RANDOM_SEEDS[kind]) == len(set(hc.RANDOM_SEEDS[kind])) == 8
    again = [hc.random_history(kind, s) for s in hc.RANDOM_SEEDS[kind]]
    assert [repr(h) for h in again] == [repr(h) for h in hc.RANDOM[kind]]
    assert len({repr(h.ops) for h in again}) == 8


def _model(kind, h):
    return hc.SynthModel() if kind == 'synth' else hc.EngineModel(kind) if kind in ('disc', 'feat') else hc.LoopModel(h.case, h.probe['prec'])


@pytest.mark.parametrize('kind', KINDS)
def test_histories_keep_the_length_limit_and_are_valid(kind):
    names = [h.name for h in hc.all_histories(kind)]
    assert len(names) == len(set(names))
    shapes = dict(synth=hc.SYNTH_SHAPES, disc=hc.DISC_SHAPES, feat=hc.FEAT_SHAPES, loop=hc.LOOP_SHAPES)[kind]
    for h in hc.all_histories(kind):
        assert hc.LEN_MIN <= len(h.ops) <= hc.LEN_MAX, h.name
        assert h.case in shapes, h.name
        m = _model(kind, h)
        passes = 0
        for op in h.ops:
            assert m.valid(op), (h.name, op)
            rc = m.apply(op)
            assert (rc == hc.LA_ERR_ARG) == op[0].startswith('refused'), (h.name, op)
            passes += op[0] in ('forward', 'run', 'pair_distance')
        assert passes >= 1, h.name
        if kind == 'synth':
            sh = hc.SYNTH_SHAPES[h.case]
            for op in h.ops:
                if op[0] == 'forward':
                    assert 1 <= op[1] <= hc.MAX_BATCH
                if op[0] == 'set_rows':
                    assert tuple(op[1:]) in sh['rows'], (h.name, op)
                if op[0] == 'set_cols':
                    assert tuple(op[1:]) in sh['cols'], (h.name, op)
            p = h.probe
            assert p['rows'] == (0, 0) or p['rows'] in sh['rows'], h.name
            assert p['cols'] == (0, 0) or (p['cols'] in sh['cols'] and p['rows'] != (0, 0)), h.name
            assert p['sched'] == 0 or sh['R'] >= 64


def test_history_scales_alternate():
    assert hc.pass_scale(0) == (2.0 ** 3, 2.0 ** 8) and hc.pass_scale(1) == (2.0 ** -6, 2.0 ** -6) and hc.pass_scale(2) == hc.pass_scale(0)


def _table(name):
    """(R, imgc, channels) of a synthesis shape"""
    if name.startswith('chain:'):
        c = chain.CASES[name[6:]]
        return 4 << (len(c['channels']) - 1), c['imgc'], list(c['channels'])
    c = sc.SYNTH_SHRINK if name == sc.SYNTH_SHRINK.name else sc.SYNTH_BY_NAME[name]
    return c.R, c.imgc, c.channels


def _fwd_windows(lib, R, imgc, channels, mode, rows, cols):
    rc, plan = query(lib, R, imgc, channels, 2, PREC[mode], rows, cols)
    assert rc == 0, lib.la_last_error()
    return [L['fwd'] for L in plan['layers'][:plan['nconv']]], plan


def _windows_used(h):
    """every (rows, cols) a forward pass of the history or its probe runs under"""
    m, used = hc.SynthModel(), set()
    for op in h.ops:
        m.apply(op)
        if op[0] == 'forward':
            used.add((m.rows, m.cols, m.prec))
    used.add((h.probe['rows'], h.probe['cols'], h.probe['prec']))
    return used


def test_every_synthesis_window_is_planned_at_its_shape(lib):
    seen = set()
    for h in hc.all_histories('synth'):
        R, imgc, channels = _table(h.case)
        assert R == hc.SYNTH_SHAPES[h.case]['R']
        for rows, cols, mode in _windows_used(h):
            fw, plan = _fwd_windows(lib, R, imgc, channels, mode, rows, cols)
            seen.add((h.case, rows, cols, mode))
            if rows == (0, 0) or mode == 'f32':          # whole frames, and the exact-fp32 kernels, which follow no window: nothing is planned
                assert all(w == (0, 0, 0, 0) for w in fw), (h.name, rows, cols, mode, fw)
                assert all(b['img_rows'] == (0, 0) for b in plan['blocks']), h.name
                continue
            narrower = [w for w in fw if w[1] > 0 and (w[0] > 0 or w[1] < R)]
            assert narrower and fw[-1][1] > 0 and fw[-1][1] - fw[-1][0] < R, (h.name, rows, fw)
            assert fw[-1][0] <= rows[0] and fw[-1][1] >= rows[1]
            if cols == (0, 0):
                assert all(w[2:] == (0, 0) for w in fw), (h.name, fw)
            elif cols == hc.COLS_PLANNED_AWAY:          # named so in the issue: its tiles are the whole row, the plan drops the column window
                assert all(w[2:] == (0, 0) for w in fw), (h.name, fw)
            else:
                top = fw[-1]
                assert top[3] > 0 and top[3] - top[2] < R and top[2] <= cols[0] and top[3] >= cols[1], (h.name, cols, top)
    # every window of the tables is used by some history in a 16-bit mode
    for case, sh in hc.SYNTH_SHAPES.items():
        for r in sh['rows']:
            assert any(k[0] == case and k[1] == r and k[3] != 'f32' for k in seen), (case, r)
        for c in sh['cols']:
            assert any(k[0] == case and k[2] == c and k[3] != 'f32' for k in seen), (case, c)


def test_loop_windows_are_planned(lib):
    """64^2 is the smallest resolution at which the centre crop of the pixel criterion is a planned row window; the 128^2 case plans rows and
    the columns (70, 122); the all-criteria cases run whole frames (the discriminator reads them)"""
    cc, off = lc.crop_geometry(32)
    fw, _ = _fwd_windows(lib, 32, 2, list(lc.G_CHANNELS[32]), hc.LOOP_WIN_PREC, (off, off + cc), (0, 0))
    assert all(w == (0, 0, 0, 0) for w in fw)          # nothing below 64^2 follows a window
    cc, off = lc.crop_geometry(64)
    assert (off, off + cc) == (10, 55) and hc.crop_geometry(64) == (cc, off) and hc.crop_geometry(128) == lc.crop_geometry(128)
    fw, _ = _fwd_windows(lib, 64, 2, list(lc.G_CHANNELS[64]), hc.LOOP_WIN_PREC, (10, 55), (10, 55))
    assert 0 < fw[-1][1] - fw[-1][0] < 64 and fw[-1][1] > 0
    for rows in ((8, 60),):
        fw, _ = _fwd_windows(lib, 64, 2, list(lc.G_CHANNELS[64]), hc.LOOP_WIN_PREC, rows, (10, 55))
        assert 0 < fw[-1][1] - fw[-1][0] < 64
    for w in (hc.R128_WIN_A, hc.R128_WIN_B):
        fw, _ = _fwd_windows(lib, 128, 2, list(hc.LOOP_R128_CHANNELS), hc.LOOP_WIN_PREC, w['rows'], w['cols'])
        top = fw[-1]
        assert 0 < top[1] - top[0] < 128 and 0 < top[3] - top[2] < 128 and top[2] <= 70 and top[3] >= 122, top
        x, y = w['crop']
        assert w['rows'][0] <= y and y + hc.FEAT_CROP <= w['rows'][1] and w['cols'][0] <= x and x + hc.FEAT_CROP <= w['cols'][1]
    # each window's crop lies outside the other window
    a, b = hc.R128_WIN_A, hc.R128_WIN_B
    assert not (b['rows'][0] <= a['crop'][1] and a['crop'][1] + hc.FEAT_CROP <= b['rows'][1])
    assert not (a['rows'][0] <= b['crop'][1] and b['crop'][1] + hc.FEAT_CROP <= a['rows'][1])
    for name, sh in hc.LOOP_SHAPES.items():
        assert sh['window'] == (not sh['disc'])


def test_loop_model_follows_the_window_hint():
    m = hc.LoopModel('win-R64', 'f16x2')
    assert m.rows == (10, 55) and m.windowed(hc.LOOP_SHAPES['win-R64']['crop'])
    assert not m.windowed((2, 2))                        # the perceptual crop outside the window: whole frames
    m.apply(('set_rows', 20, 40))
    assert not m.windowed(hc.LOOP_SHAPES['win-R64']['crop'])          # the pixel criterion's crop outside
    m = hc.LoopModel('win-R128-cols', 'f16x2')
    m.apply(('set_rows', *hc.R128_WIN_A['rows']))
    m.apply(('set_cols', *hc.R128_WIN_A['cols']))
    assert m.windowed(hc.R128_WIN_A['crop']) and not m.windowed(hc.R128_WIN_B['crop'])
    assert not hc.LoopModel('all-R32', 'f32').windowed((8, 16))


def test_invalidate_banks_is_declared_and_bound(lib):
    from latentaugment_amd import _lib
    assert _lib.SIGNATURES['la_latent_opt_invalidate_banks'] == (C.c_int, [C.c_void_p])
    assert hasattr(lib, 'la_latent_opt_invalidate_banks')
    assert lib.la_latent_opt_invalidate_banks(None) == hc.LA_ERR_ARG and b'null handle' in lib.la_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'latentaug_hip.h')).read()
    assert 'la_latent_opt_invalidate_banks' in header and 'History contract' in header
