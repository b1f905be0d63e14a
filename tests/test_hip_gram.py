"""la_gram_pair_dist_f32 on the GPU against the restatement of tests/nst_cases.py, over the case table proven in
test_nst_cases_cpu.py: C in {4, 12, 64, 65, 128, 132, 260} (ragged single tile, one tile of either edge and the first C past the
small edge, one plus 4 with an off-diagonal tile, three tile rows) x HW in {1, 4, 9, 33, 1110} (below a K chunk, odd, three K slices with a shorter last one), P in {1, 3}.

EXACT: integer inputs in -2 .. 2 give the float64 restatement bit for bit, style and content; a pair alone (P = 1) gives the bits it
gives at every position of P = 3.
BOUNDED: float inputs (a close pair y = x + 1e-3 noise, an independent pair, an identical pair): style within the dot-product bound
of nst_cases.bounds (derived, nothing tuned), content within (C HW + 2) 2^-53; the identical pair exactly 0.0; swapped halves and a
second run give the same bits.  Scratch between guard bands in the 'ones' and 'bytes' patterns: bands intact, the same bits.
Every bounded case prints its figures.

Largest measured on an MI355X: style error 0.079 of its bound (C = 4, HW = 1), content error 0.057 of its bound (C = 68, HW = 1; most
cases 0: the same bits as the restatement); the close pairs no worse than the independent ones.  Wall time of the file: 3 s for 95 tests.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nst_cases as nc  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _run(lib, dev, f, pattern='ones', content=True):
    """la_gram_pair_dist_f32 -> (style [P], content [P]) as numpy float64; outputs and scratch between guard bands."""
    from latentaugment_amd import _lib
    fd = torch.from_numpy(np.array(f, np.float32)).to(dev)
    P, C, HW = fd.shape[0] // 2, fd.shape[1], fd.shape[2]
    nbytes = lib.la_gram_pair_scratch_bytes(P, C, HW)
    assert nbytes > 0
    g = Guarded(pattern)
    ws = g.alloc(nbytes, dev, torch.float64)
    style = g.tensor([P], torch.float64, dev, -7.0)
    cont = g.tensor([P], torch.float64, dev, -7.0)
    with torch.cuda.device(dev):
        rc = lib.la_gram_pair_dist_f32(_lib.ptr(fd), P, C, HW, _lib.ptr(style), _lib.ptr(cont) if content else None, _lib.ptr(ws), nbytes,
                                       _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    return style.cpu().numpy(), cont.cpu().numpy()


_FLOAT = {}


def _float_case(lib, dev, C, HW):
    """inputs, restatement, bounds and the GPU result of a float case, computed once"""
    if (C, HW) not in _FLOAT:
        f = nc.float_inputs(C, HW)
        f.setflags(write=False)
        _FLOAT[(C, HW)] = (f, nc.restate(f), nc.bounds(f), _run(lib, dev, f))
    return _FLOAT[(C, HW)]


@pytest.mark.parametrize('C,HW', nc.CASES)
def test_integer_inputs_are_exact_and_position_independent(lib, dev, C, HW):
    f = nc.int_inputs(C, HW, 3)
    want_s, want_c = nc.restate(f)
    got_s, got_c = _run(lib, dev, f)
    assert got_s.tobytes() == want_s.tobytes(), (got_s, want_s)
    assert got_c.tobytes() == want_c.tobytes(), (got_c, want_c)
    assert (want_s > 0).all() and (want_c > 0).all()
    for p in range(3):          # P = 1: the pair alone
        s1, c1 = _run(lib, dev, f[[p, p + 3]])
        assert s1.tobytes() == got_s[p:p + 1].tobytes() and c1.tobytes() == got_c[p:p + 1].tobytes()


@pytest.mark.parametrize('C,HW', nc.CASES)
def test_float_inputs_lie_inside_the_bound(lib, dev, C, HW):
    """Measured: see the module docstring."""
    f, (want_s, want_c), (sb, cb), (got_s, got_c) = _float_case(lib, dev, C, HW)
    es, ec = np.abs(got_s - want_s), np.abs(got_c - want_c)
    print(f'C {C:4d} HW {HW:5d}: style err / bound close {es[0] / sb[0]:.3e} far {es[1] / sb[1]:.3e}   content err / bound close '
          f'{ec[0] / cb[0]:.3e} far {ec[1] / cb[1]:.3e}   style bound / style close {sb[0] / want_s[0]:.2e} far {sb[1] / want_s[1]:.2e}')
    assert np.isfinite(got_s).all() and np.isfinite(got_c).all()
    assert got_s[2] == 0.0 and got_c[2] == 0.0          # d(f, f) is exactly 0
    assert (es <= sb).all(), (es, sb)
    assert (ec <= cb).all(), (ec, cb)


@pytest.mark.parametrize('C,HW', nc.CASES)
def test_swapped_halves_position_and_second_run_give_the_same_bits(lib, dev, C, HW):
    f, _, _, (got_s, got_c) = _float_case(lib, dev, C, HW)
    again_s, again_c = _run(lib, dev, f)
    assert again_s.tobytes() == got_s.tobytes() and again_c.tobytes() == got_c.tobytes()
    swap_s, swap_c = _run(lib, dev, np.concatenate([f[3:], f[:3]]))
    assert swap_s.tobytes() == got_s.tobytes() and swap_c.tobytes() == got_c.tobytes()
    for p in (0, 1):
        s1, c1 = _run(lib, dev, f[[p, p + 3]])
        assert s1.tobytes() == got_s[p:p + 1].tobytes() and c1.tobytes() == got_c[p:p + 1].tobytes()


@pytest.mark.parametrize('C,HW', [(12, 9), (132, 33), (260, nc.HW_SPLIT), (65, nc.HW_SPLIT), (64, nc.HW_SPLIT)])
def test_scratch_contents_do_not_matter(lib, dev, C, HW):
    """The scratch is written before it is read: NaN bytes and seeded random bytes give the bits of each other, the bands stay intact
    (checked inside _run), and a call without `content` gives the same style."""
    f, _, _, (got_s, got_c) = _float_case(lib, dev, C, HW)
    for pattern in ('ones', 'bytes'):
        s, c = _run(lib, dev, f, pattern)
        assert s.tobytes() == got_s.tobytes() and c.tobytes() == got_c.tobytes(), pattern
    s, c = _run(lib, dev, f, 'bytes', content=False)
    assert s.tobytes() == got_s.tobytes() and (c == -7.0).all()


def test_refusals_come_before_any_launch(lib, dev):
    from latentaugment_amd import _lib
    f = nc.float_inputs(12, 33)
    fd = torch.from_numpy(f).to(dev)
    need = lib.la_gram_pair_scratch_bytes(3, 12, 33)
    g = Guarded('ones')
    ws = g.alloc(need, dev, torch.float64)
    style = g.tensor([3], torch.float64, dev, -7.0)
    cont = g.tensor([3], torch.float64, dev, -7.0)

    def call(P=3, C=12, HW=33, nbytes=need, fptr=None, sptr=None, wptr=None):
        with torch.cuda.device(dev):
            return lib.la_gram_pair_dist_f32(_lib.ptr(fd) if fptr is None else fptr, P, C, HW, _lib.ptr(style) if sptr is None else sptr,
                                             _lib.ptr(cont), _lib.ptr(ws) if wptr is None else wptr, nbytes, _lib.stream_ptr())
    assert call(nbytes=need - 1) == LA_ERR_WORKSPACE and b'la_gram_pair_scratch_bytes' in lib.la_last_error()
    assert call(nbytes=0) == LA_ERR_WORKSPACE
    for bad in (dict(P=0), dict(P=-1), dict(C=0), dict(HW=0), dict(HW=-3), dict(C=8193), dict(P=65536)):
        assert call(**bad) == LA_ERR_ARG, bad
    import ctypes
    assert call(wptr=ctypes.c_void_p(ws.data_ptr() + 4)) == LA_ERR_ARG          # scratch not 8-byte aligned
    torch.cuda.synchronize()
    assert (style == -7.0).all() and (cont == -7.0).all()          # nothing was launched
    assert call() == 0          # and the device is usable afterwards
    torch.cuda.synchronize()
    g.check()
    want_s, want_c = nc.restate(f)
    sb, cb = nc.bounds(f)
    assert (np.abs(style.cpu().numpy() - want_s) <= sb).all() and (np.abs(cont.cpu().numpy() - want_c) <= cb).all()
