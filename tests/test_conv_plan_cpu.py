"""The kernel-form decision of the contraction launches (la_conv_plan through la_conv_plan_query, host only: no GPU) against its Python
restatement modconv_cases.conv_launch: profiler class, row tile, MFMA form, K slices, pre-split copy, merged phases, operand-preparation
brackets, grid and the workspace bytes taken in front of the slice partials -- for every case of the table, every precision and both
workspace modes; the boundary rows by name; and synth_cases.uses_halo against the class the library plans."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modconv_cases as mc  # noqa: E402
import synth_cases as sc  # noqa: E402

CLS = ('conv_halo', 'conv_flat', 'conv_splitk', 'conv_f32')      # LA_PC_CONV_* (la_prof_end_classes order)
MFMA = ('32x32x2', '32x32', '16x16x32')                          # LA_CONV_MFMA_*
NINFO = 11                                                       # LA_CONV_PLAN_NINFO
BIG_WS = 1 << 40


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def query(lib, prec, B, Cc, M, geom, res, in_q, ws_bytes):
    """-> (rc, dict of the info fields)"""
    info = (C.c_long * NINFO)()
    rc = lib.la_conv_plan_query(prec, B, Cc, M, geom, res, int(in_q), ws_bytes, info)
    v = list(info)
    return rc, dict(launch=mc.Launch(CLS[v[0]] if 0 <= v[0] < 4 else v[0], v[1], MFMA[v[2]] if 0 <= v[2] < 3 else v[2], v[3], bool(v[4]), bool(v[5])),
                    prep=v[6], grid=tuple(v[7:10]), ws_head=v[10])


def expected(case, prec, sp, ws_bytes, in_q):
    """The model's Launch of one spec, its operand-preparation brackets, grid and workspace head."""
    counts = mc.new_counts()
    B = case['B']
    l = mc.conv_launch(prec, B, sp['C'], sp['M'], sp['grids'], sp['Hin'], sp['Hin'], sp['dense3x3'], ws_bytes, in_q, counts)
    prep = counts['operand_prep']
    if l.ksplit > 1:
        grid = (sum(mc.cdiv(B * gy * gx, mc.NT) for gy, gx, _ in sp['grids']), mc.cdiv(sp['M'], l.mt), l.ksplit)
    else:
        grid = (max(mc.cdiv(gy * gx, mc.NT) for gy, gx, _ in sp['grids']), mc.cdiv(sp['M'], l.mt), B * len(sp['grids']))
    head = 0
    if prep:
        head = mc.presplit_hdr_bytes(B, sp['C']) if l.cls == 'conv_halo' else min(mc.r256(mc.presplit_bytes(B, sp['C'], sp['Hin'], sp['Hin'])), ws_bytes)
    return l, prep, grid, head


def walk(case, prec, ws_bytes):
    specs, ws_l, in_q = mc.launch_inputs(case, prec, ws_bytes, mc.new_counts())
    return [(sp, ws_l, in_q) for sp in specs]


def ask(lib, case, prec, sp, ws_l, in_q):
    return query(lib, prec, case['B'], sp['C'], sp['M'], sp['geom'], case['res'], in_q, ws_l)


@pytest.mark.parametrize('name', [c['name'] for c in mc.CASES])
def test_query_equals_the_model_on_the_whole_table(lib, name):
    case = mc.BY_NAME[name]
    for prec in mc.PRECISIONS:
        for with_ws in (True, False):
            pl = mc.plan(case, prec, with_ws)
            launches = walk(case, prec, pl['ws_bytes'])
            assert len(launches) == len(pl['launches'])
            for (sp, ws_l, in_q), want in zip(launches, pl['launches']):
                l, prep, grid, head = expected(case, prec, sp, ws_l, in_q)
                assert l == want
                rc, got = ask(lib, case, prec, sp, ws_l, in_q)
                where = (name, prec, with_ws, sp['geom'])
                assert rc == 0, (where, lib.la_last_error())
                assert got['launch'] == l, where
                assert (got['prep'], got['grid'], got['ws_head']) == (prep, grid, head), where


def test_library_workspace_bytes_equal_the_model(lib):
    for c in mc.CASES:
        up = 1 if c['entry'].startswith('up2') else 0
        assert lib.la_modconv_workspace_bytes(c['B'], c['cin'], c['cout'], c['res'], up) == mc.workspace_bytes(c['B'], c['cin'], c['cout'], c['res'], up), c['name']


def _one(lib, name, prec, with_ws=True, **change):
    case = dict(mc.BY_NAME[name], **change)
    (sp, ws_l, in_q), = walk(case, prec, mc.plan(case, prec, with_ws)['ws_bytes'])
    rc, got = ask(lib, case, prec, sp, ws_l, in_q)
    assert rc == 0, (name, prec, lib.la_last_error())
    return got


def test_boundary_rows(lib):
    for prec in (1, 2, 3):
        # grid 1156, the last split-K grid, against the first halo grid (res 64)
        assert mc.BY_NAME['sk_r34']['res'] ** 2 == mc.SPLITK_MAX_G
        assert _one(lib, 'sk_r34', prec)['launch'].cls == 'conv_splitk'
        assert _one(lib, 'sk_r34', prec, with_ws=False)['launch'].cls == 'conv_flat'
        assert _one(lib, 'fl_r35', prec)['launch'].cls == 'conv_flat'
        assert _one(lib, 'ha_r64_m64', prec)['launch'][:4] == ('conv_halo', 64, '32x32', 1)
        # rows around the 32-row halo tile and the 128-row tile
        assert [_one(lib, n, prec)['launch'].mt for n in ('ha_r64_m28', 'ha_r64_m32', 'ha_r64_m36')] == [32, 32, 64]
        assert [_one(lib, n, prec)['grid'][1] for n in ('ha_r64_m28', 'ha_r64_m32', 'ha_r64_m36')] == [1, 1, 1]
        assert [_one(lib, n, prec)['launch'].mt for n in ('sk_r34', 'sk_r34_m128', 'sk_c544')] == [64, 128, 128]      # M = 124, 128, 132
        assert [_one(lib, n, prec)['grid'][1] for n in ('sk_r34', 'sk_r34_m128', 'sk_c544', 'ha_r64_m132')] == [2, 1, 2, 2]
        # 17 chunks under the 16-slice cap: 9 slices
        assert mc.cdiv(mc.BY_NAME['sk_c544']['cout'], mc.KCB) == 17 and _one(lib, 'sk_c544', prec)['launch'].ksplit == 9
    assert _one(lib, 'sk_c544', 0)['launch'][:4] == ('conv_f32', 128, '32x32x2', 34)
    assert [_one(lib, n, 0)['launch'].mt for n in ('ha_r64_m28', 'ha_r64_m32', 'ha_r64_m36')] == [64, 64, 64]      # no 32-row tiles off the halo kernel
    # the C > KCB switch of the fp16 halo kernel on 128-row tiles: one chunk runs the 32x32 form, more the 16x16x32 form
    forms = {}
    for Cc in (32, 33, 64):
        rc, got = query(lib, 3, 1, Cc, 128, mc.GEOM_SAME_FWD, 64, False, BIG_WS)
        assert rc == 0 and got['launch'][:2] == ('conv_halo', 128)
        forms[Cc] = got['launch'].mfma
    assert forms == {32: '32x32', 33: '16x16x32', 64: '16x16x32'}
    assert _one(lib, 'ha_r64_m128_c32', 3)['launch'].mfma == '32x32' and _one(lib, 'ha_r64_m128', 3)['launch'].mfma == '16x16x32'
    assert _one(lib, 'ha_r64_m128', 1)['launch'].mfma == '32x32'


@pytest.mark.parametrize('name', [c['name'] for c in mc.CASES if c['entry'] != 'up2_fwd'])
def test_one_float_short_of_the_partials_runs_direct(lib, name):
    """modconv_cases.plan(with_ws=False) hands in one float less than the slice partials need: direct there, split with that float."""
    case = mc.BY_NAME[name]
    for prec in mc.PRECISIONS:
        if not mc.splits(case, prec):
            continue
        short = mc.plan(case, prec, False)['ws_bytes']
        for ws, split in ((short, False), (short + 4, True)):
            (sp, ws_l, in_q), = walk(case, prec, ws)
            rc, got = ask(lib, case, prec, sp, ws_l, in_q)
            assert rc == 0 and (got['launch'].ksplit > 1) == split, (name, prec, ws, got)
            assert got['launch'].ksplit == (mc.plan(case, prec, True)['launches'][0].ksplit if split else 1)


def test_refusals_carry_a_message(lib):
    c = mc.BY_NAME['sk_r4_b3']
    refused = [
        dict(prec=0, B=3, Cc=33, M=6, ws=1 << 20),        # rows not a multiple of 4
        dict(prec=1, B=3, Cc=33, M=4, ws=0),              # a 16-bit launch without a workspace
        dict(prec=3, B=65, Cc=4, M=4, ws=1 << 24),        # more than 64 samples
    ]
    for r in refused:
        with pytest.raises(mc.Refused):
            mc.conv_launch(r['prec'], r['B'], r['Cc'], r['M'], [(c['res'], c['res'], 9)], c['res'], c['res'], True, r['ws'], False, mc.new_counts())
        rc, _ = query(lib, r['prec'], r['B'], r['Cc'], r['M'], mc.GEOM_SAME_FWD, c['res'], False, r['ws'])
        assert rc != 0 and lib.la_last_error().startswith(b'conv: '), r
    # an odd output resolution has no up-sampling geometry; merged phases arrive pre-split
    with pytest.raises(mc.Refused):
        mc.launch_inputs(dict(mc.BY_NAME['uf_r4'], res=5), 1, 1 << 20, mc.new_counts())
    assert query(lib, 1, 3, 33, 4, mc.GEOM_UP2_MERGED, 5, True, 1 << 20)[0] != 0 and lib.la_last_error()
    assert query(lib, 1, 3, 33, 4, mc.GEOM_UP2_MERGED, 4, False, 1 << 20)[0] != 0 and b'merged phases' in lib.la_last_error()
    assert query(lib, 0, 3, 33, 4, mc.GEOM_UP2_MERGED, 4, True, 1 << 20)[0] != 0
    assert query(lib, 1, 3, 33, 4, 8, 4, False, 1 << 20)[0] != 0 and query(lib, 4, 3, 33, 4, 0, 4, False, 1 << 20)[0] != 0


def test_synth_cases_uses_halo_agrees_with_the_planned_class(lib):
    channels = sorted({ch for cs in sc.SYNTH_CASES for ch in cs.channels} | {256, 512, 4096})
    prec_of = {'f32': 0, 'bf16x3': 1, 'f16x2': 3}
    for mode in sc.MODES:
        for res in (4 << k for k in range(9)):
            for cin in channels:
                rc, got = query(lib, prec_of[mode], 1, cin, 64, mc.GEOM_SAME_FWD, res, False, BIG_WS)
                # (a 16-bit launch too large for the halo kernel AND for a pre-split copy is refused: no halo launch either)
                assert (rc == 0 and got['launch'].cls == 'conv_halo') == sc.uses_halo(mode, cin, res), (mode, res, cin)
                assert rc == 0 or b'too large' in lib.la_last_error()
