"""The plan of a synthesis pass (la_synth.hip plan_pass through la_synth_plan_query, host only: no GPU) against its Python restatement
synth_cases.branch_plan: per block the ToRGB form, the skip image's launch, where the conv1 and the conv0 seam run, the segment counts of
every layer's partials, the plane-maxima buffers, the down-FIR launches and the pyramid block -- for every case of the synthesis sweep in
f32, bf16x3 and f16x2 and at the channel tables and batches of the bench configurations B, C, D and E.  For the windowed cases the window and
cone fields: the cone is the one la_synth_plan_bwd_window gives (test_bwd_cone_cpu.py holds that against autograd on the float64 oracle),
every backward launch reads and writes the 4-row tiles around it, the forward windows hold it."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_cases as sc  # noqa: E402

PREC = {'f32': 0, 'bf16x3': 1, 'f16x2': 3}
# LA_SYNTH_PLAN_* of include/latentaug_hip.h
PASS = ('nblocks', 'nconv', 'B', 'precision', 'f16', 'xs_handoff', 'zt_dense', 'cone')
LAYER_N, BLOCK_N, MAX_LAYERS, MAX_BLOCKS = 20, 6, 24, 12
NINFO = len(PASS) + LAYER_N * MAX_LAYERS + BLOCK_N * MAX_BLOCKS
SEAM = ('kernel', 'fused')                                  # LA_SYNTH_SEAM_*
PMAX = (None, 'shared', 'up-fused', 'conv1-fused')          # LA_SYNTH_PMAX_*


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def query(lib, R, imgc, channels, B, prec, rows=(0, 0), cols=(0, 0)):
    """-> (rc, dict(pass fields, layers=[dict], blocks=[dict]))"""
    info = (C.c_long * NINFO)()
    rc = lib.la_synth_plan_query(R, imgc, (C.c_int * len(channels))(*channels), B, prec, rows[0], rows[1], cols[0], cols[1], info)
    v = list(info)
    plan = dict(zip(PASS, v))
    layers, blocks = [], []
    for ci in range(MAX_LAYERS):
        r = v[len(PASS) + LAYER_N * ci:len(PASS) + LAYER_N * (ci + 1)]
        layers.append(dict(fwd=tuple(r[0:4]), cone=tuple(r[4:6]), win=r[6], rows_in=tuple(r[7:11]), rows_out=tuple(r[11:15]),
                           seam=SEAM[r[15]] if 0 <= r[15] < 2 else r[15], seam_pmax=PMAX[r[16]] if 0 <= r[16] < 4 else r[16],
                           pmax_in=PMAX[r[17]] if 0 <= r[17] < 4 else r[17], nseg=r[18], ntiles=r[19]))
    base = len(PASS) + LAYER_N * MAX_LAYERS
    for k in range(MAX_BLOCKS):
        r = v[base + BLOCK_N * k:base + BLOCK_N * (k + 1)]
        blocks.append(dict(fuse_rgb=r[0], skip_up=r[1], img_rows=tuple(r[2:4]), down_fir=r[4], pyramid=r[5]))
    plan.update(layers=layers, blocks=blocks)
    return rc, plan


def ask(lib, case, mode, B=None, rows=(0, 0), cols=(0, 0)):
    rc, plan = query(lib, case.R, case.imgc, case.channels, case.B if B is None else B, PREC[mode], rows, cols)
    assert rc == 0, (case.name, mode, lib.la_last_error())
    return plan


def check_against_the_model(lib, case, mode, B):
    got, want = ask(lib, case, mode, B), sc.branch_plan(case, mode)
    where = (case.name, mode, B)
    nb = want['nblocks']
    f16 = mode == 'f16x2'
    assert (got['nblocks'], got['nconv'], got['B'], got['precision']) == (nb, 2 * nb - 1, B, PREC[mode]), where
    # the product library has no development switch: slot rows whenever the mode is f16x2, column-planar scratch, and the cone where the
    # seams are fused and the rows handed on
    assert (got['f16'], got['xs_handoff'], got['zt_dense'], got['cone']) == (f16, f16, 0, f16), where
    for k, b in enumerate(want['blocks']):
        g, l1 = got['blocks'][k], got['layers'][2 * k]
        assert bool(g['fuse_rgb']) == (b['torgb'] == 'fused'), (where, k)
        assert bool(g['skip_up']) == b['skip_launch'] and b['up2_skip'] == (k > 0 and not g['skip_up']), (where, k)
        assert bool(g['down_fir']) == b['down_fir'] and bool(g['pyramid']) == (want['pyramid_block'] == k), (where, k)
        assert g['img_rows'] == (0, 0), (where, k)
        assert (l1['seam'], l1['nseg'], l1['ntiles']) == (b['seam'], b['nseg1'], b['tiles1']), (where, k)
        # a seam kernel writes the shared buffer unless it lowers the slot row; a fused seam writes the buffer of its kind; the
        # contraction behind the seam reads where it wrote (f16x2 only: no other mode has an fp16 operand scale)
        assert l1['pmax_in'] == ((('conv1-fused' if b['seam'] == 'fused' else 'shared')) if f16 else None), (where, k)
        assert l1['seam_pmax'] == ('conv1-fused' if f16 and b['seam'] == 'fused' else None), (where, k)
        if b['seam'] == 'kernel':
            assert l1['nseg'] == b['slabs'], (where, k)
        if k == 0:
            continue
        l0 = got['layers'][2 * k - 1]
        assert (l0['seam'], l0['nseg'], l0['ntiles']) == (b['seam0'], b['nseg0'], b['tiles0']), (where, k)
        assert l0['pmax_in'] == (('up-fused' if b['seam0'] == 'fused' else 'shared') if f16 else None), (where, k)
        assert l0['seam_pmax'] == ('up-fused' if f16 and b['seam0'] == 'fused' else None), (where, k)
    # nothing is windowed, and nothing stands behind the engine's layers and blocks
    empty_layer = dict(fwd=(0,) * 4, cone=(0, 0), win=0, rows_in=(0,) * 4, rows_out=(0,) * 4, seam='kernel', seam_pmax=None, pmax_in=None, nseg=0, ntiles=0)
    for ci, l in enumerate(got['layers']):
        assert (l['fwd'], l['cone'], l['win'], l['rows_in'], l['rows_out']) == ((0,) * 4, (0, 0), 0, (0,) * 4, (0,) * 4), (where, ci)
        assert ci < 2 * nb - 1 or l == empty_layer, (where, ci)
    assert all(not any(g['img_rows'] + (g['fuse_rgb'], g['skip_up'], g['down_fir'], g['pyramid'])) for g in got['blocks'][nb:]), where
    assert sum(g['pyramid'] for g in got['blocks']) == int(want['pyramid']), where


@pytest.mark.parametrize('case', sc.SYNTH_CASES + [sc.SYNTH_SHRINK], ids=[c.name for c in sc.SYNTH_CASES + [sc.SYNTH_SHRINK]])
def test_query_equals_branch_plan_on_the_sweep(lib, case):
    for mode in sc.MODES:
        for B in sorted({case.B, case.max_batch}):
            check_against_the_model(lib, case, mode, B)


# the bench configurations (BASELINE.json): resolution, channel_base (channels = min(base / res, 512)), samples per GPU -- and half of them,
# what one of two stream lanes runs
BENCH = {'B': (256, 32768, 8), 'C': (512, 32768, 4), 'D': (1024, 32768, 2), 'E': (256, 16384, 8)}


@pytest.mark.parametrize('name', sorted(BENCH))
def test_query_equals_branch_plan_at_the_bench_configurations(lib, name):
    R, base, batch = BENCH[name]
    case = sc.SynthCase(f'bench-{name}', R, [min(base // r, 512) for r in sc.block_resolutions(R)], 2, batch, kind='bulk')
    for mode in sc.MODES:
        for B in (batch, batch // 2):
            check_against_the_model(lib, case, mode, B)
    # the blocks of at most 128 channels at >= 64^2 carry their ToRGB in conv1's launch; the pyramid starts where the level below is <= 256^2
    plan = sc.branch_plan(case, 'f16x2')
    fused = [b['res'] for b in plan['blocks'] if b['torgb'] == 'fused']
    assert fused == {'B': [256], 'C': [256, 512], 'D': [256, 512, 1024], 'E': [128, 256]}[name]
    assert plan['pyramid_block'] == {256: 6, 512: 7, 1024: 7}[R]


def round4(lo, hi, res):
    return lo // 4 * 4, min((hi + 3) // 4 * 4, res)


def bwd_window(lib, R, rows, cols, ci):
    from latentaugment_amd import _lib
    w = (C.c_int * 4)()
    _lib.check(lib.la_synth_plan_bwd_window(R, rows[0], rows[1], cols[0], cols[1], ci, w), 'la_synth_plan_bwd_window')
    return tuple(w)


@pytest.mark.parametrize('name,with_cols', sc.SYNTH_WINDOWED + [('R256-imgc3-slabs', True)],
                         ids=[f'{n}{"-cols" if c else ""}' for n, c in sc.SYNTH_WINDOWED + [('R256-imgc3-slabs', True)]])
def test_window_and_cone_fields(lib, name, with_cols):
    case = sc.SYNTH_BY_NAME[name]
    R, nb = case.R, len(case.channels)
    nconv, rows = 2 * nb - 1, sc.window_of(case.R)
    cols = rows if with_cols else (0, 0)
    # exact fp32 has no windowed kernels: the plan of a windowed pass is the plan of a whole-frame pass
    f32 = ask(lib, case, 'f32', rows=rows, cols=cols)
    assert f32 == ask(lib, case, 'f32')
    for mode in ('bf16x3', 'f16x2'):
        got, whole = ask(lib, case, mode, rows=rows, cols=cols), ask(lib, case, mode)
        assert got['cone'] == (mode == 'f16x2')
        windowed = []
        for ci in range(nconv):
            l, res = got['layers'][ci], 4 << ((ci + 1) // 2)
            b_lo, b_hi, c_lo, c_hi = bwd_window(lib, R, rows, cols, ci)
            assert l['cone'] == (b_lo, b_hi), (name, mode, ci)
            # the decisions that do not depend on the window are those of the whole-frame pass
            assert all(l[f] == whole['layers'][ci][f] for f in ('seam', 'seam_pmax', 'pmax_in', 'nseg', 'ntiles')), (name, mode, ci)
            if b_hi == 0:      # whole plane: below 64^2, or every row is needed
                assert l['fwd'][:2] == (0, 0) and not l['win'] and l['rows_in'] == (0,) * 4, (name, mode, ci)
                continue
            windowed.append(ci)
            f_lo, f_hi = l['fwd'][:2]
            assert res >= 64 and 0 <= f_lo <= b_lo < b_hi <= f_hi <= res, (name, mode, ci)
            if ci % 2 == 0:      # conv1: whole 4-row tiles; conv0 (the FIR output): one row more on either side
                assert (f_lo, f_hi) == round4(f_lo, f_hi, res) and got['layers'][ci - 1]['fwd'][:2] == (max(f_lo - 1, 0), min(f_hi + 1, res)), (name, mode, ci)
            assert l['win'] == got['cone'], (name, mode, ci)
            if not l['win']:
                assert l['rows_in'] == l['rows_out'] == (0,) * 4, (name, mode, ci)
                continue
            # a backward launch reads the tiles around the cone of its layer's output and writes those around the cone of its input
            assert l['rows_in'][:2] == round4(b_lo, b_hi, res), (name, mode, ci)
            if ci % 2 == 0:      # conv1 writes d(conv0 output) at the same resolution, for the up layer's backward to read
                below = got['layers'][ci - 1]
                assert l['rows_out'][:2] == round4(*below['cone'], res) and below['rows_in'] == l['rows_out'], (name, mode, ci)
            else:                # the up layer writes d(conv1 output of the block below) at half the resolution, where that has a cone
                below = got['layers'][ci - 1]
                assert l['rows_out'] == ((round4(*below['cone'], res // 2) + (0, 0)) if below['cone'][1] else (0,) * 4), (name, mode, ci)
        assert windowed and windowed[-2:] == [nconv - 2, nconv - 1] and windowed == list(range(windowed[0], nconv)), (name, mode)
        # columns: the top block only -- conv1 in whole 32-column tiles with a tile column to spare, conv0 one column more; the backward of
        # conv1 writes those tile columns, the up layer's reads them
        c1, c0 = got['layers'][nconv - 1], got['layers'][nconv - 2]
        tile_cols = bwd_window(lib, R, rows, cols, nconv - 2)[2:]
        assert c1['fwd'][2:] == tile_cols and all(got['layers'][ci]['fwd'][2:] == (0, 0) for ci in range(nconv - 2)), (name, mode)
        if with_cols and R >= 128:
            lo, hi = tile_cols
            assert lo % 32 == 0 and hi % 32 == 0 and 0 < hi - lo < R and lo <= cols[0] - 1 and cols[1] + 1 <= hi, (name, mode)
            assert c0['fwd'][2:] == (max(lo - 1, 0), min(hi + 1, R)), (name, mode)
        else:
            assert tile_cols == (0, 0) and c0['fwd'][2:] == (0, 0), (name, mode)
        if got['cone']:
            assert c1['rows_out'][2:] == tile_cols and c0['rows_in'][2:] == tile_cols and c1['rows_in'][2:] == (0, 0) and c0['rows_out'][2:] == (0, 0)
        # image rows handed to the large ToRGB kernel: the window at the top; a block below delivers what the 4-tap up-sampling (up 2, pad
        # (2, 1, 2, 1)) of the rows above reads
        need = rows
        for k in range(nb - 1, -1, -1):
            large = 2 * k in windowed and (4 << k) ** 2 > sc.TORGB_SMALL_MAX_HW
            assert got['blocks'][k]['img_rows'] == (need if large else (0, 0)), (name, mode, k)
            assert [got['blocks'][k][f] for f in ('fuse_rgb', 'skip_up', 'down_fir', 'pyramid')] == [whole['blocks'][k][f] for f in ('fuse_rgb', 'skip_up', 'down_fir', 'pyramid')]
            need = (max((need[0] - 2) >> 1, 0), min((need[1] >> 1) + 1, (4 << k) // 2))


def test_benchmark_geometry(lib):
    """256^2, image rows and columns [38, 219) (test_bwd_cone_cpu.py): the tiles of the two top blocks and the tile columns (32, 224)"""
    case = sc.SynthCase('bench-B', 256, [min(32768 // r, 512) for r in sc.block_resolutions(256)], 2, 4, kind='bulk')
    got = ask(lib, case, 'f16x2', rows=(38, 219), cols=(38, 219))
    top1, top0, mid1 = got['layers'][12], got['layers'][11], got['layers'][10]
    assert top1['fwd'] == (36, 220, 32, 224) and top0['fwd'] == (35, 221, 31, 225) and mid1['fwd'][:2] == (16, 112)
    assert top1['cone'] == (38, 219) and top1['rows_in'] == (36, 220, 0, 0) and top1['rows_out'] == (36, 220, 32, 224) == top0['rows_in']
    assert got['blocks'][6]['img_rows'] == (38, 219) and got['blocks'][6]['fuse_rgb'] and got['cone']


def test_refusals_carry_a_message(lib):
    ch = (8, 8, 8)
    bad = [dict(R=12), dict(R=8192, channels=(8,) * 12), dict(R=2), dict(imgc=0), dict(imgc=5), dict(B=0), dict(prec=-1), dict(prec=4),
           dict(channels=(8, 6, 8)), dict(channels=(8, 8, 0)), dict(rows=(5, 4)), dict(rows=(3, 0)), dict(rows=(0, 17)), dict(rows=(-1, 4)),
           dict(cols=(5, 4)), dict(cols=(0, 17)), dict(cols=(2, 0))]
    for change in bad:
        a = dict(dict(R=16, imgc=2, channels=ch, B=2, prec=3, rows=(0, 0), cols=(0, 0)), **change)
        rc, _ = query(lib, a['R'], a['imgc'], a['channels'], a['B'], a['prec'], a['rows'], a['cols'])
        assert rc != 0 and lib.la_last_error().startswith(b'synth_plan_query: '), change
    info = (C.c_long * NINFO)()
    assert lib.la_synth_plan_query(16, 2, None, 2, 3, 0, 0, 0, 0, info) != 0
    assert lib.la_synth_plan_query(16, 2, (C.c_int * 3)(*ch), 2, 3, 0, 0, 0, 0, None) != 0
    assert query(lib, 16, 2, ch, 2, 3, (4, 12), (4, 12))[0] == 0
