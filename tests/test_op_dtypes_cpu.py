"""float16 / float64 op layer, host side: the fixture tests/golden/op_dtypes.npz is what the GPU tests take it for, and the six new
C entries are declared, bound and exported."""
import ast
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('la_bias_act_ex_f16', 'la_bias_sum_f16', 'la_bias_act_ex_f64', 'la_bias_sum_f64', 'la_upfirdn2d_f16', 'la_upfirdn2d_f64')


@pytest.fixture(scope='module')
def od(golden_dir):
    return np.load(os.path.join(golden_dir, 'op_dtypes.npz'))


def _cases(od):
    return [ast.literal_eval(str(r)) for r in od['cases']]


def test_fixture_inputs_are_float16_values(od):
    """The inputs are stored as float16 and the float64 expected values were computed from the very same numbers: widening them to
    float64 and narrowing back is exact, and the float64 outputs have the shapes the float16 ones have."""
    cases = _cases(od)
    assert sum(c[0].startswith('b') for c in cases) == 18 and sum(c[0].startswith('u') for c in cases) == 7
    for c in cases:
        name = c[0]
        ins = ('x', 'b', 'dy', 'ddx') if name.startswith('b') else ('x', 'dy')
        outs = ('y', 'dx', 'd2', 'db') if name.startswith('b') else ('y', 'dx')
        for k in ins:
            v = od[f'{name}_{k}']
            assert v.dtype == np.float16, (name, k)
            assert np.array_equal(v.astype(np.float64).astype(np.float16), v) and np.isfinite(v).all()
        for k in outs:
            assert od[f'{name}_{k}'].dtype == np.float64 and od[f'{name}_{k}16'].dtype == np.float16
            assert od[f'{name}_{k}'].shape == od[f'{name}_{k}16'].shape, (name, k)


def test_reference_float16_error_is_nonzero_in_every_case(od):
    """The float16 budgets of the GPU tests are multiples of the reference's own float16 error: it must exist in every case."""
    for c in _cases(od):
        name = c[0]
        outs = ('y', 'dx', 'd2', 'db') if name.startswith('b') else ('y', 'dx')
        errs = [float(np.abs(od[f'{name}_{k}16'].astype(np.float64) - od[f'{name}_{k}']).max()) for k in outs]
        assert errs[0] > 0 and max(errs) > 0, (c, errs)


def test_fixture_taps_are_setup_filter_taps(od):
    """The stored float32 taps are what ops.setup_filter makes of the raw taps (the GPU tests pass the raw taps through it)."""
    import torch
    from latentaugment_amd import ops
    for c in _cases(od):
        if c[0].startswith('u'):
            f = ops.setup_filter(ast.literal_eval(c[2]))
            assert f.dtype == torch.float32
            assert np.array_equal(f.numpy(), od[f'{c[0]}_f']), c[0]


def test_new_entries_declared_bound_and_exported():
    from latentaugment_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    declared = set(re.findall(r'\b(la_[a-z0-9_]+)\s*\(', hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the float64 entries take double scalars, the float16 ones float scalars (as the plugin does)
    import ctypes as C
    assert _lib.SIGNATURES['la_bias_act_ex_f64'][1][-4:-1] == [C.c_double] * 3
    assert _lib.SIGNATURES['la_upfirdn2d_f64'][1][-2] is C.c_double
    assert _lib.SIGNATURES['la_bias_act_ex_f16'][1][-4:-1] == [C.c_float] * 3
    assert lib.la_abi_version() == 1


def test_new_entries_check_arguments_on_the_host():
    """Argument errors are refused before any launch, with the float32 entries' messages (no device needed)."""
    import ctypes as C
    from latentaugment_amd import _lib
    lib = _lib.load()
    taps = (C.c_float * 81)(*([1.0 / 81] * 81))
    host = (C.c_double * 512)()      # (a real host buffer; the checks refuse before anything reads or writes it)
    buf = C.cast(host, C.c_void_p)
    for fn in (lib.la_upfirdn2d_f16, lib.la_upfirdn2d_f64):
        assert fn(buf, taps, buf, 1, 1, 16, 16, 9, 9, 1, 1, 1, 1, 4, 4, 4, 4, 0, 1.0, None) != 0
        assert b'8x8' in lib.la_last_error()
    for fn in (lib.la_bias_act_ex_f16, lib.la_bias_act_ex_f64):
        assert fn(buf, None, None, None, None, buf, 8, 1, 1, 0, 10, 0.0, 1.0, -1.0, None) != 0
        assert b'activation id' in lib.la_last_error()
    for fn in (lib.la_bias_sum_f16, lib.la_bias_sum_f64):
        assert fn(buf, buf, 10, 3, 2, None) != 0 and b'bias_sum' in lib.la_last_error()
