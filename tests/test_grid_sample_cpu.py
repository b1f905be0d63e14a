"""Host side of grid_sample and fma (la_grid_sample.hip, ops.grid_sample, ops.fma).  No GPU:
- the numpy restatement of tests/grid_sample_cases.py reproduces the reference's golden (tests/golden/grid_sample.npz) within
  1e-12 x max(1, max |expected|), so the GPU tests may use it as their float64 expectation on inputs the golden file does not hold;
- the new header entries parse, are exported and have the expected pointer / scalar layout; bad arguments are refused before any launch;
- ops.grid_sample / ops.fma refuse host tensors;
- the position-to-corner function (csrc/la_grid_sample_index.h) is compiled into a stand-alone host program with
  -fsanitize=undefined,address and fed huge, infinite, NaN and every quarter-pixel position: nothing it marks as addressable lies
  outside the image, and its weights are the restatement's, bit for bit."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_FWD = ('la_grid_sample_f32', 'la_grid_sample_f16', 'la_grid_sample_f64')
GS_BWD = ('la_grid_sample_grad_f32', 'la_grid_sample_grad_f16', 'la_grid_sample_grad_f64')
NEW = GS_FWD + GS_BWD + ('la_grid_sample_grad_workspace_floats', 'la_fma_f32', 'la_unbroadcast_sum_f32')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'grid_sample.npz'))


def _close(got, exp, what):
    err = float(np.abs(np.asarray(got, np.float64) - exp).max(initial=0.0))
    assert got.shape == exp.shape and err <= 1e-12 * max(1.0, float(np.abs(exp).max(initial=0.0))), (what, err)


@pytest.mark.parametrize('case', gc.GS_CASES, ids=gc.GS_NAMES)
def test_restatement_reproduces_the_golden_grid_sample(gold, case):
    name, half = case[0], case[-1]
    t = gc.gs_inputs(case)
    for k, v in t.items():      # the table's inputs are the golden file's
        stored = gold[f'g_{name}_{k}']
        assert stored.dtype == (np.float16 if half else np.float32) and np.array_equal(stored.astype(np.float64), v), (name, k)
    assert gc.frac_ok(t['grid'], case[3], case[4])
    _close(gc.gs_forward(t['x'], t['grid']), gold[f'g_{name}_y'], (name, 'y'))
    dx, dgrid = gc.gs_backward(t['dy'], t['x'], t['grid'])
    _close(dx, gold[f'g_{name}_dx'], (name, 'dx'))
    _close(dgrid, gold[f'g_{name}_dgrid'], (name, 'dgrid'))
    _close(gc.gs_forward(t['ddx'], t['grid']), gold[f'g_{name}_d2'], (name, 'd2'))
    if case[7] == 'outside':
        assert not gold[f'g_{name}_y'].any() and not gold[f'g_{name}_dx'].any() and not gold[f'g_{name}_dgrid'].any()
    else:
        assert np.abs(gold[f'g_{name}_dgrid']).max() > 0.1 and np.abs(gold[f'g_{name}_dx']).max() > 0.1


@pytest.mark.parametrize('case', gc.FMA_CASES, ids=[c[0] for c in gc.FMA_CASES])
def test_restatement_reproduces_the_golden_fma(gold, case):
    name = case[0]
    t = gc.fma_inputs(case)
    for k, v in t.items():
        assert np.array_equal(gold[f'f_{name}_{k}'].astype(np.float64), v), (name, k)
    r = gc.fma_all(t['a'], t['b'], t['c'], t['dy'])
    for k in ('y', 'da', 'db', 'dc'):
        _close(r[k], gold[f'f_{name}_{k}'], (name, k))
    if name == gc.FMA_SECOND_ORDER:      # da = unbroadcast(dy * b): its gradients for an incoming dda are dda (broadcast) * b and unbroadcast(dda * dy)
        dda = gold[f'f_{name}_dda']
        _close(np.broadcast_to(dda, t['dy'].shape) * t['b'], gold[f'f_{name}_d2_dy'], (name, 'd2_dy'))
        _close(gc.unbroadcast(np.broadcast_to(dda, t['dy'].shape) * t['dy'], t['b'].shape), gold[f'f_{name}_d2_b'], (name, 'd2_b'))


def test_case_table_covers_what_it_claims():
    shapes = {(c[3], c[4]) for c in gc.GS_CASES}
    outs = {(c[5], c[6]) for c in gc.GS_CASES}
    assert shapes == {(4, 8), (5, 7), (1, 1)} and {(3, 5), (9, 2), (1, 130)} <= outs
    assert {c[2] for c in gc.GS_CASES} == {1, 3, 5} and all(c[1] == 2 for c in gc.GS_CASES)
    assert any(c[5] * c[6] > 256 for c in gc.GS_CASES) and any(c[-1] and c[5] * c[6] > 256 for c in gc.GS_CASES)
    assert {c[7] for c in gc.GS_CASES} == {'identity', 'rotation', 'band', 'outside', 'random'}
    band = next(c for c in gc.GS_CASES if c[7] == 'band')
    px, py = gc.positions(gc.gs_inputs(band)['grid'], band[3], band[4])
    assert (((py > -1) & (py < 0)) | ((py > band[3] - 1) & (py < band[3]))).all()
    assert (((px > -1) & (px < 0)) | ((px > band[4] - 1) & (px < band[4]))).any()
    out = next(c for c in gc.GS_CASES if c[7] == 'outside')
    px, _ = gc.positions(gc.gs_inputs(out)['grid'], out[3], out[4])
    assert ((px < -1) | (px > out[4])).all()


def test_symbols_declared_bound_and_exported(lib):
    from latentaugment_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    for name in NEW:
        assert name + '(' in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    P, I, L = C.c_void_p, C.c_int, C.c_long
    S = _lib.SIGNATURES
    for name in GS_FWD:
        assert S[name] == (I, [P] * 3 + [I] * 6 + [P]), name
    assert S['la_grid_sample_grad_f32'] == S['la_grid_sample_grad_f64'] == (I, [P] * 5 + [I] * 6 + [P])
    assert S['la_grid_sample_grad_f16'] == (I, [P] * 6 + [I] * 6 + [P])
    assert S['la_grid_sample_grad_workspace_floats'] == (L, [I] * 4)
    assert S['la_fma_f32'] == (I, [P] * 9) and S['la_unbroadcast_sum_f32'] == (I, [P] * 5)
    assert lib.la_abi_version() == 1


def _err(lib):
    return (lib.la_last_error() or b'').decode()


def test_arguments_are_checked_before_any_launch(lib):
    buf = (C.c_double * 4)()      # never dereferenced: every call below is refused before a launch
    p = C.addressof(buf)
    good = (2, 3, 4, 8, 3, 5)
    for name in GS_FWD:
        fn = getattr(lib, name)
        assert fn(None, p, p, *good, None) != 0 and 'null pointer' in _err(lib)
        for k in range(6):
            dims = list(good)
            dims[k] = 0
            assert fn(p, p, p, *dims, None) != 0 and 'empty' in _err(lib), (name, k)
        # element counts beyond INT_MAX are refused, never truncated: x, y and the grid in turn
        for dims in ((4, 1024, 1024, 1024, 1, 1), (4, 1024, 1, 1, 1024, 1024), (2, 1, 1, 1, 32768, 32768)):
            assert fn(p, p, p, *dims, None) != 0 and 'INT_MAX' in _err(lib), (name, dims)
    for name in GS_BWD:
        fn = getattr(lib, name)
        ws = (p,) if name.endswith('f16') else ()
        assert fn(None, p, p, p, p, *ws, *good, None) != 0 and 'null pointer' in _err(lib)
        assert fn(p, p, p, None, None, *ws, *good, None) != 0 and 'neither' in _err(lib)
        assert fn(p, None, p, None, p, *ws, *good, None) != 0 and 'needs x' in _err(lib)
        assert fn(p, p, p, p, p, *ws, 4, 1024, 1024, 1024, 1, 1, None) != 0 and 'INT_MAX' in _err(lib)
    assert lib.la_grid_sample_grad_f16(p, p, p, p, p, None, *good, None) != 0 and 'workspace' in _err(lib)
    assert lib.la_grid_sample_grad_workspace_floats(2, 3, 4, 8) == 192
    assert lib.la_grid_sample_grad_workspace_floats(4, 1024, 1024, 1024) == 0 and lib.la_grid_sample_grad_workspace_floats(0, 1, 1, 1) == 0
    L4 = C.c_long * 4
    s, z = L4(2, 3, 4, 4), L4(0, 0, 0, 0)
    assert lib.la_fma_f32(None, p, p, p, s, z, z, z, None) != 0 and 'null pointer' in _err(lib)
    assert lib.la_fma_f32(p, p, p, p, L4(2, 0, 4, 4), z, z, z, None) != 0 and 'empty' in _err(lib)
    assert lib.la_fma_f32(p, p, p, p, s, L4(0, -1, 0, 0), z, z, None) != 0 and 'negative stride' in _err(lib)
    assert lib.la_fma_f32(p, p, p, p, L4(65536, 65536, 1, 1), z, z, z, None) != 0 and 'INT_MAX' in _err(lib)
    assert lib.la_unbroadcast_sum_f32(p, None, s, s, None) != 0 and 'null pointer' in _err(lib)
    assert lib.la_unbroadcast_sum_f32(p, p, s, L4(2, 3, 2, 4), None) != 0 and 'neither' in _err(lib)
    assert lib.la_unbroadcast_sum_f32(p, p, L4(65536, 65536, 1, 1), L4(1, 1, 1, 1), None) != 0 and 'INT_MAX' in _err(lib)


def test_wrappers_refuse_host_tensors():
    from latentaugment_amd import _lib, ops
    x, g = torch.zeros([1, 2, 4, 4]), torch.zeros([1, 3, 3, 2])
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        ops.grid_sample(x, g)
    with pytest.raises(_lib.LatentAugHipError, match='ROCm device'):
        ops.fma(x, x, x)


def test_index_function_under_sanitizers(tmp_path):
    """csrc/la_grid_sample_index.h in a stand-alone host program (tests/tools/gs_index_check.cpp) built with
    -fsanitize=undefined,address and run as its own process: the program reads a `size`-element array through every neighbour the
    function marks as inside and fails on a weighted or marked neighbour outside [0, size); its printed rows are compared here with
    the restatement's gs_axis, bit for bit, in float32 and float64."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = tmp_path / 'gs_index_check'
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=undefined,address', '-fno-sanitize-recover=all',
                        '-I' + os.path.join(ROOT, 'latentaugment_amd', 'csrc'), os.path.join(ROOT, 'tests', 'tools', 'gs_index_check.cpp'),
                        '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) > 2000
    seen = set()
    for typ, dt in (('f32', np.float32), ('f64', np.float64)):
        for size in sorted({int(w[1]) for w in rows}):
            sel = [w for w in rows if w[0] == typ and int(w[1]) == size]
            g = np.array([float.fromhex(w[2]) if w[2] not in ('inf', '-inf', 'nan', '-nan') else float(w[2]) for w in sel])
            i0, w0, w1, in0, in1 = gc.gs_axis(g, size, dt)
            got_i0 = np.array([int(w[3]) for w in sel])
            got_w0, got_w1 = (np.array([float.fromhex(w[k]) for w in sel]) for k in (4, 5))
            got_in0, got_in1 = (np.array([bool(int(w[k])) for w in sel]) for k in (6, 7))
            assert np.array_equal(got_in0, in0) and np.array_equal(got_in1, in1), (typ, size)
            used = in0 | in1
            assert np.array_equal(got_i0[used], i0[used]) and not got_i0[~used].any(), (typ, size)
            assert np.array_equal(got_w0, w0.astype(np.float64)) and np.array_equal(got_w1, w1.astype(np.float64)), (typ, size)
            # nothing with a weight or an inside mark lies outside the image
            assert ((got_w0 == 0) | (got_in0 & (got_i0 >= 0) & (got_i0 < size))).all(), (typ, size)
            assert ((got_w1 == 0) | (got_in1 & (got_i0 + 1 >= 0) & (got_i0 + 1 < size))).all(), (typ, size)
            special = ~np.isfinite(g) | (np.abs(g) >= 3)
            assert special.sum() >= 11 and not (got_in0 | got_in1)[special].any() and not (got_w0 + got_w1)[special].any()
            seen.add((typ, size))
    assert len(seen) == 12
