"""la_sort_columns_f32 on the GPU against numpy's sort of the mapped keys (tests/swd_cases.py), bit for bit: keys only, so the sorted
column is one bit pattern whatever the algorithm.  With T = la_sort_tile_keys() the sizes sit on the seams of the tile sort and of the
merge passes: one tile, a padded tile, an unpaired run in a pass, both parities of the pass count (the result must end in `keys`).
Keys and scratch lie between guard bands, the scratch pre-filled with 0xFF or seeded bytes; columns with a stride ld = M + 3 from a
base one float into the allocation keep their three spare elements; two runs give the same bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_cases as sc  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
SPARE = -7.5          # what the elements outside the columns hold


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _sort(lib, dev, keys, strided, pattern):
    """keys float32 [ncols][M] numpy -> the sorted bit patterns uint32 [ncols][M]; checks the bands and the spare elements"""
    from latentaugment_amd import _lib
    ncols, M = keys.shape
    ld, off = (M + 3, 1) if strided else (M, 0)
    g = Guarded(pattern)
    buf = g.tensor([off + ncols * ld], torch.float32, dev, SPARE)
    cols = buf[off:].view(ncols, ld)
    cols[:, :M] = torch.from_numpy(keys).to(dev)
    nbytes = lib.la_sort_columns_scratch_bytes(ncols, M)
    assert nbytes >= ncols * M * 4
    scratch = g.alloc(nbytes, dev)
    with torch.cuda.device(dev):
        rc = lib.la_sort_columns_f32(C.c_void_p(buf.data_ptr() + 4 * off), ncols, M, ld, _lib.ptr(scratch), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    assert bool((cols[:, M:] == SPARE).all()) and bool((buf[:off] == SPARE).all())          # elements [M, ld) and the float in front
    return np.ascontiguousarray(cols[:, :M].cpu().numpy()).view(np.uint32)


def _check(lib, dev, content, ncols, M, strided, pattern, seed):
    keys = sc.sort_keys(content, ncols, M, seed)
    want = sc.sort_columns_bits(keys.view(np.uint32))
    got = _sort(lib, dev, keys, strided, pattern)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{content} ncols {ncols} M {M}: {len(bad)} keys differ, first at column {bad[0][0]}, position {bad[0][1]}'
    return got


_GRID = [(m, n) for m in sc.SORT_M for n in sc.SORT_NCOLS]


@pytest.mark.parametrize('mname,ncols', _GRID)
def test_sizes_and_columns(lib, dev, mname, ncols):
    """every size x every column count; the contents, the stride and the scratch pattern rotate through the grid"""
    i = _GRID.index((mname, ncols))
    M = sc.sort_m(mname, lib.la_sort_tile_keys())
    _check(lib, dev, 'normal', ncols, M, strided=i % 2 == 1, pattern=('ones', 'bytes')[i // 2 % 2], seed=i)
    _check(lib, dev, sc.SORT_CONTENTS[1 + i % 5], ncols, M, strided=i % 2 == 0, pattern=('bytes', 'ones')[i // 2 % 2], seed=100 + i)


@pytest.mark.parametrize('content', sc.SORT_CONTENTS)
@pytest.mark.parametrize('mname', ['65', 'T+1', '3T+5', '5T-3'])
def test_contents(lib, dev, content, mname):
    """every kind of contents at a padded single tile, an odd and an even pass count and an unpaired run; twice: the same bits"""
    M = sc.sort_m(mname, lib.la_sort_tile_keys())
    a = _check(lib, dev, content, 3, M, strided=True, pattern='ones', seed=7)
    b = _check(lib, dev, content, 3, M, strided=False, pattern='bytes', seed=7)
    assert a.tobytes() == b.tobytes()


def test_signed_zeros_and_infinities_keep_their_places(lib, dev):
    keys = np.array([[0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 0.0, -0.0, 1.0]], np.float32)
    got = _sort(lib, dev, keys, False, 'ones').view(np.float32)[0]
    assert got[0] == -np.inf and got[-1] == np.inf
    assert np.signbit(got[2:4]).all() and (got[2:4] == 0).all() and not np.signbit(got[4:6]).any() and (got[4:6] == 0).all()
