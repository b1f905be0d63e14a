"""tests/guarded_alloc.py on CPU tensors: the bands hold, a write one byte outside the payload is found at the right offset, payload
writes are not, and the three patterns are what they say.  No GPU, no library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as ga      # noqa: E402
from guarded_alloc import GUARD, Guarded, GuardError, guarded_tensor      # noqa: E402


def _parent(g, i=-1):
    return g.records[i][0]


@pytest.mark.parametrize('pattern', ga.PATTERNS)
@pytest.mark.parametrize('nbytes', [0, 1, 63, 64, 4096, 100003])
def test_untouched_allocations_pass(pattern, nbytes):
    g = Guarded(pattern)
    t = g.alloc(nbytes, 'cpu')
    assert t.dtype == torch.uint8 and t.numel() == nbytes and t.is_contiguous()
    parent = _parent(g)
    assert parent.numel() == GUARD + nbytes + GUARD and (nbytes == 0 or t.data_ptr() == parent.data_ptr() + GUARD)
    assert bool((parent[:GUARD] == 0xA5).all()) and bool((parent[GUARD + nbytes:] == 0xA5).all())
    g.check()


def test_patterns():
    z, o, b, b2 = (Guarded(p).alloc(5000, 'cpu') for p in ('zeros', 'ones', 'bytes', 'bytes'))
    assert not z.any() and bool((o == 0xFF).all())
    assert torch.equal(b, b2) and len(b.unique()) > 200          # seeded: the same bytes each run, and really mixed
    f = Guarded('ones').alloc(64, 'cpu', torch.float32)
    assert f.dtype == torch.float32 and f.numel() == 16 and bool(f.isnan().all())
    assert bool(Guarded('ones').alloc(64, 'cpu', torch.float64).isnan().all()) and bool(Guarded('ones').alloc(64, 'cpu', torch.float16).isnan().all())
    assert bool((Guarded('ones').alloc(64, 'cpu', torch.int32) == -1).all())
    big = Guarded('bytes').alloc(ga._BLOCK + 777, 'cpu')          # longer than one seeded block
    assert torch.equal(big[:5000], b) and torch.equal(big[ga._BLOCK:], b[:777])
    with pytest.raises(ValueError):
        Guarded('random')


def test_same_size_as_the_package_allocator():
    """alloc() returns what _lib.workspace returns: nbytes // itemsize elements; the rear band starts right behind them."""
    from latentaugment_amd import _lib
    for nbytes, dtype in ((64, None), (100, torch.float64), (4100, torch.float32), (7, torch.float32), (24, torch.float64)):
        want = _lib.workspace(nbytes, 'cpu') if dtype is None else _lib.workspace(nbytes, 'cpu', dtype)
        g = Guarded('zeros')
        got = g.alloc(nbytes, 'cpu') if dtype is None else g.alloc(nbytes, 'cpu', dtype)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert g.records[-1][1] == want.numel() * want.element_size()
        assert got.data_ptr() % 8 == 0


@pytest.mark.parametrize('nbytes', [1, 100, 4097])
@pytest.mark.parametrize('where,offset', [('before', -1), ('after', 0), ('front_first', -GUARD), ('rear_last', GUARD - 1)])
def test_one_byte_outside_is_found_at_its_offset(nbytes, where, offset):
    g = Guarded('bytes')
    g.alloc(32, 'cpu')                                  # an untouched neighbour: the message must name allocation #1, not #0
    g.alloc(nbytes, 'cpu')
    parent = _parent(g)
    want = offset if offset < 0 else nbytes + offset      # relative to the payload
    parent[GUARD + want] = 0x00
    bad = g.damage()
    assert len(bad) == 1 and bad[0][0] == 1 and bad[0][1] == nbytes and bad[0][3] == want
    assert os.path.basename(bad[0][2]).startswith('test_guarded_alloc_cpu.py:')
    with pytest.raises(GuardError) as e:
        g.check()
    msg = str(e.value)
    assert 'allocation #1' in msg and f'({nbytes} bytes' in msg and f'payload offset {want}' in msg and 'test_guarded_alloc_cpu.py' in msg


def test_a_band_byte_rewritten_with_its_own_value_is_not_damage_but_any_other_is():
    g = Guarded('zeros')
    g.alloc(10, 'cpu')
    _parent(g)[GUARD + 10] = 0xA5
    g.check()
    _parent(g)[GUARD + 10] = 0xA4
    with pytest.raises(GuardError):
        g.check()


@pytest.mark.parametrize('pattern', ga.PATTERNS)
def test_payload_writes_never_trip(pattern):
    g = Guarded(pattern)
    a = g.alloc(1000, 'cpu')
    b = g.alloc(4096, 'cpu', torch.float64)
    a.fill_(0xA5)
    a[0], a[-1] = 1, 2
    b.fill_(float('nan'))
    b[0], b[-1] = 1.0, -1.0
    g.check()


def test_guarded_tensor_holds_its_fill_and_is_checked():
    g = Guarded('zeros')
    t = guarded_tensor([3, 5, 7], torch.float32, 'cpu', -777.0, g)
    assert t.shape == (3, 5, 7) and t.is_contiguous() and bool((t == -777.0).all())
    i = guarded_tensor([4], torch.int32, 'cpu', -3, g)
    assert bool((i == -3).all())
    t.zero_()
    g.check()
    _parent(g, 0)[GUARD + 3 * 5 * 7 * 4] = 0
    with pytest.raises(GuardError, match='payload offset 420'):
        g.check()
    own = guarded_tensor([2, 3], torch.float64, 'cpu', 1.5)          # without a guard: one of its own
    assert bool((own == 1.5).all()) and own.guard is not g and len(own.guard.records) == 1
    own.guard.check()
    _parent(own.guard)[GUARD - 1] = 0
    with pytest.raises(GuardError, match='payload offset -1 '):
        own.guard.check()


def test_replaces_the_package_allocator(monkeypatch):
    """The use the GPU tests make of it: monkeypatch.setattr(_lib, 'workspace', g.alloc); a call through the module attribute reaches it."""
    from latentaugment_amd import _lib
    g = Guarded('ones')
    monkeypatch.setattr(_lib, 'workspace', g.alloc)
    t = _lib.workspace(256, 'cpu', torch.float32)
    assert len(g.records) == 1 and bool(t.isnan().all())
    g.check()
