"""The numpy restatement of the sliced Wasserstein distance (tests/swd_cases.py) checked against identities that do not involve the
library, and the host side of the new entries -- declared, bound, exported, size queries monotone, every refusal before anything
touches a device.  No test here needs a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_cases as sc  # noqa: E402

LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3
ENTRIES = ('la_sort_tile_keys', 'la_sort_columns_scratch_bytes', 'la_sort_columns_f32', 'la_lap_pyr_down_f32', 'la_lap_pyr_up_sub_f32',
           'la_swd_gather_f32', 'la_swd_stats_scratch_bytes', 'la_swd_channel_stats_f64', 'la_swd_normalize_f32', 'la_swd_directions_f32',
           'la_swd_scratch_bytes', 'la_swd_f32')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape', [(2, 64, 48), (1, 32, 32), (3, 16, 80)])
def test_pyramid_reconstructs_its_input(shape):
    x = np.random.RandomState(1).uniform(-1, 1, shape)
    levels = sc.pyramid(x, sc.num_levels(*shape[1:], min_resolution=4))
    assert len(levels) >= 3 and [lv.shape[-2] for lv in levels] == [shape[1] >> l for l in range(len(levels))]
    err = np.abs(sc.reconstruct(levels) - x).max()
    print(f'reconstruction {err:.2e}')
    assert err <= 1e-14 * np.abs(x).max()


def test_filters_keep_a_constant_and_mirror_without_repeating_the_edge():
    assert sc.mirror_index([-2, -1, 0, 3, 4, 5], 4).tolist() == [2, 1, 0, 3, 2, 1]
    one = np.ones([1, 8, 12])
    assert np.array_equal(sc.down(one), np.ones([1, 4, 6])) and np.array_equal(sc.up(one), np.ones([1, 16, 24]))
    # the polyphase form the kernel uses: [1, 6, 1] / 8 at even positions, [4, 4] / 8 at odd ones, on a 1-D ramp with both borders
    c = np.arange(5.0)[None, None, :].repeat(2, 1)          # [1][2][5] -> rows are identical, so up acts on columns alone
    u = sc.up(c)[0, 0]
    want = [(c[0, 0, 1] + 6 * c[0, 0, 0] + c[0, 0, 1]) / 8, (c[0, 0, 0] + c[0, 0, 1]) / 2, (c[0, 0, 0] + 6 * c[0, 0, 1] + c[0, 0, 2]) / 8]
    assert np.allclose(u[:3], want, rtol=0, atol=1e-15)
    assert np.allclose(u[-2:], [(c[0, 0, 3] + 6 * c[0, 0, 4] + c[0, 0, 4]) / 8, c[0, 0, 4]], rtol=0, atol=1e-15)


@pytest.mark.parametrize('shape', sc.PYR_EXACT_SHAPES)
def test_integer_pyramid_is_exact_in_float32(shape):
    """what test_hip_swd.py relies on: three levels of integer pixels in [-4, 4] are the same numbers in float32 and float64"""
    x = sc.integer_images(3, *shape, seed=5)
    p64, p32 = sc.pyramid(x, 3), sc.pyramid(x.astype(np.float32), 3)
    for a, b in zip(p64, p32):
        assert b.dtype == np.float32 and np.array_equal(a, b.astype(np.float64))


def test_translated_cloud():
    rng = np.random.RandomState(2)
    a = rng.standard_normal([300, 17])
    t = rng.standard_normal(17)
    d = sc.directions(40, 17, 0, seed=3)
    err = np.abs(sc.w1(a, a + t, d) - np.abs(d @ t)).max()
    print(f'translation {err:.2e}')
    assert err <= 3e-14
    assert np.array_equal(sc.w1(a, a, d), np.zeros(40))


def test_one_dimension_is_the_sorted_difference():
    rng = np.random.RandomState(4)
    a, b = rng.standard_normal([101, 1]), rng.standard_normal([101, 1]) * 2 + 1
    want = np.abs(np.sort(a[:, 0]) - np.sort(b[:, 0])).sum() / 101
    assert sc.w1(a, b, np.ones([1, 1]))[0] == want and sc.w1(a, b, -np.ones([1, 1]))[0] == want


def test_positions_reach_both_ends_and_do_not_depend_on_the_batch():
    n, per, H, W, nh = 6, 16, 16, 16, 7          # the smallest image case of test_hip_swd.py (the coarse level of 32 x 32)
    x0, y0 = sc.positions(n, 0, 1, per, H, W, nh, seed=0)
    assert x0.min() == 0 and x0.max() == W - nh and y0.min() == 0 and y0.max() == H - nh
    xa, ya = sc.positions(2, 0, 1, per, H, W, nh, seed=0)
    xb, yb = sc.positions(4, 2, 1, per, H, W, nh, seed=0)
    assert np.array_equal(np.concatenate([xa, xb]), x0) and np.array_equal(np.concatenate([ya, yb]), y0)
    assert not np.array_equal(sc.positions(n, 0, 0, per, H, W, nh, seed=0)[0], x0)          # the level is part of the counter


def test_directions_are_unit_and_chunkable():
    d = sc.directions(12, 98, 0, seed=7)
    assert np.abs(np.sqrt((d * d).sum(1)) - 1).max() < 1e-15
    assert np.array_equal(sc.directions(7, 98, 5, seed=7), d[5:])
    assert np.sqrt((sc.raw_normals(12, 98, 0, 7).astype(np.float64) ** 2).sum(1)).min() >= 1


def test_sort_restatement_orders_like_the_floats():
    k = sc.sort_keys('special', 2, 500, seed=1)
    out = sc.sort_columns_bits(k.view(np.uint32)).view(np.float32)
    assert np.array_equal(out, np.sort(k, axis=1))          # equal as values (-0.0 == 0.0) ..
    z = out[0][out[0] == 0]
    assert z.size > 2 and (np.diff(np.signbit(z).astype(int)) <= 0).all() and np.signbit(z[0]) and not np.signbit(z[-1])   # .. and -0.0 first
    assert np.array_equal(sc.key_bits(sc.key_image(k.view(np.uint32))), k.view(np.uint32))


def test_normalisation_removes_a_power_of_two_scale():
    rng = np.random.RandomState(6)
    d = rng.standard_normal([64, 2 * 9])
    m, s = sc.channel_stats(d, 2)
    m2, s2 = sc.channel_stats(0.5 * d, 2)
    assert np.array_equal(sc.normalize(d, m, s, 2), sc.normalize(0.5 * d, m2, s2, 2))
    me, se, _ = sc.channel_stats_exact(d, 2)
    assert np.abs(me - m).max() < 1e-15 and np.abs(se - s).max() < 1e-15


def test_end_to_end_restatement_and_its_bound():
    rng = np.random.RandomState(8)
    real = rng.uniform(-1, 1, [6, 2, 32, 32])
    out, det = sc.swd_images(real, real, nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8)
    assert set(out) == {'swd_32', 'swd_16', 'swd_avg'} and all(v == 0.0 for v in out.values())
    gen = np.clip(real + 0.3 * rng.standard_normal(real.shape), -1, 1)
    out, det = sc.swd_images(real, gen, nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8)
    assert out['swd_32'] > 0 and out['swd_avg'] == (out['swd_32'] + out['swd_16']) / 2
    for l in range(2):
        b = sc.composed_bound(det, l, 2)
        print(f'level {l}: w1 mean {det[l]["w1"].mean():.3e}, composed bound {b:.3e}')
        assert 0 < b < 0.1 * det[l]['w1'].mean()          # informative: a tenth of the value at most (the directions' 2e-5 dominates it)


# ------------------------------------------------------------------------------------------------------------ the host side
def test_entries_are_declared_bound_and_exported(lib):
    from latentaugment_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    declared = set(re.findall(r'\b(la_[a-z0-9_]+)\s*\(', hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES['la_swd_f32'][1][-1] is C.c_void_p and _lib.SIGNATURES['la_swd_f32'][0] is C.c_int
    rng = open(os.path.join(ROOT, 'latentaugment_amd', 'csrc', 'la_rng.h')).read()
    assert f'LA_RNG_STREAM_SWD_POS 0x{sc.STREAM_POS:08X}u' in rng and f'LA_RNG_STREAM_SWD_DIR 0x{sc.STREAM_DIR:08X}u' in rng
    src = open(os.path.join(ROOT, 'latentaugment_amd', 'csrc', 'Makefile')).read()
    assert 'la_sort.hip' in src and 'la_swd.hip' in src
    from latentaugment_amd import metrics
    assert metrics.SWD_LEVEL_DIR_STRIDE == sc.LEVEL_DIR_STRIDE


def test_scratch_queries_are_monotone(lib):
    T = lib.la_sort_tile_keys()
    assert T >= 256 and T & (T - 1) == 0
    rows = [1, 2, T - 1, T, T + 1, 3 * T + 5, 201216]
    for query, sizes in ((lambda m: lib.la_sort_columns_scratch_bytes(3, m), rows),
                         (lambda n: lib.la_sort_columns_scratch_bytes(n, 1000), [1, 2, 130, 65535]),
                         (lambda m: lib.la_swd_scratch_bytes(m, 98, 512), rows),
                         (lambda n: lib.la_swd_scratch_bytes(1000, 98, n), [1, 5, 31, 32, 33, 512]),
                         (lambda m: lib.la_swd_stats_scratch_bytes(m, 2, 49), rows)):
        got = [query(v) for v in sizes]
        assert all(g > 0 for g in got) and got == sorted(got), got
    assert lib.la_sort_columns_scratch_bytes(3, 1000) >= 3 * 1000 * 4
    # the documented minimum of la_swd_f32: chunks of 32 directions, both sets' projections and the sort's image of them
    assert lib.la_swd_scratch_bytes(1000, 98, 512) == lib.la_swd_scratch_bytes(1000, 98, 32) >= 16 * 1000 * 32
    for bad in (lib.la_sort_columns_scratch_bytes(0, 5), lib.la_sort_columns_scratch_bytes(5, 0), lib.la_sort_columns_scratch_bytes(65536, 5),
                lib.la_swd_scratch_bytes(0, 98, 4), lib.la_swd_scratch_bytes(5, 0, 4), lib.la_swd_scratch_bytes(5, 98, 0),
                lib.la_swd_stats_scratch_bytes(0, 2, 49), lib.la_swd_stats_scratch_bytes(5, 0, 49)):
        assert bad == 0


def test_every_refusal_happens_on_the_host(lib):
    """With pointers that are not device memory: a check that came after a launch would fault or report a HIP error, not -1 / -3."""
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 8192)
    big = 1 << 40
    assert lib.la_lap_pyr_down_f32(p, q, 1, 15, 16, None) == LA_ERR_ARG          # odd H
    assert lib.la_lap_pyr_down_f32(p, q, 1, 16, 0, None) == LA_ERR_ARG
    assert lib.la_lap_pyr_up_sub_f32(p, q, 1, 16, 17, None) == LA_ERR_ARG        # odd W
    assert lib.la_lap_pyr_up_sub_f32(p, None, 1, 16, 16, None) == LA_ERR_ARG
    assert b'even' in lib.la_last_error() or b'null' in lib.la_last_error()
    assert lib.la_sort_columns_f32(p, 2, 10, 9, q, big, None) == LA_ERR_ARG      # ld < M
    assert lib.la_sort_columns_f32(p, 2, 0, 9, q, big, None) == LA_ERR_ARG       # M < 1
    assert lib.la_sort_columns_f32(p, 0, 10, 10, q, big, None) == LA_ERR_ARG
    need = lib.la_sort_columns_scratch_bytes(2, 10)
    assert lib.la_sort_columns_f32(p, 2, 10, 10, q, need - 1, None) == LA_ERR_WORKSPACE
    assert lib.la_swd_gather_f32(p, 2, 2, 16, 16, 0, 0, 17, 4, 0, q, None) == LA_ERR_ARG      # the patch does not fit
    assert lib.la_swd_gather_f32(p, 0, 2, 16, 16, 0, 0, 7, 4, 0, q, None) == LA_ERR_ARG
    assert lib.la_swd_channel_stats_f64(p, 0, 2, 49, q, q, q, big, None) == LA_ERR_ARG
    need = lib.la_swd_stats_scratch_bytes(100, 2, 49)
    assert lib.la_swd_channel_stats_f64(p, 100, 2, 49, q, q, q, need - 1, None) == LA_ERR_WORKSPACE
    assert lib.la_swd_normalize_f32(p, 100, 0, 49, q, q, None) == LA_ERR_ARG
    assert lib.la_swd_directions_f32(p, 0, 98, 0, 0, None) == LA_ERR_ARG         # ndirs < 1
    assert lib.la_swd_directions_f32(p, 4, 0, 0, 0, None) == LA_ERR_ARG
    assert lib.la_swd_f32(p, p, 0, 98, q, 4, q, q, big, None) == LA_ERR_ARG      # M < 1
    assert lib.la_swd_f32(p, p, 100, 98, q, 0, q, q, big, None) == LA_ERR_ARG    # ndirs < 1
    need = lib.la_swd_scratch_bytes(100, 98, 4)
    assert lib.la_swd_f32(p, p, 100, 98, q, 4, q, q, need - 1, None) == LA_ERR_WORKSPACE
    assert b'la_swd_scratch_bytes' in lib.la_last_error()


def test_python_refusals_need_no_gpu():
    from latentaugment_amd import _lib, metrics
    a = np.zeros([5, 4], np.float32)
    with pytest.raises(_lib.LatentAugHipError):
        metrics.compute_swd_from_features(a, a, device='cpu')
    with pytest.raises(ValueError):
        metrics.compute_swd_from_images([], [], num_items=0)
    with pytest.raises(ValueError):
        metrics.compute_swd_from_images([], [], dir_repeats=0)
    with pytest.raises(FileNotFoundError):
        metrics.compute_swd_for_aug_dataset(os.path.join(ROOT, 'tests', 'no_such_run'))
