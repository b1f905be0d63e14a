"""The contract of every metric-side entry that takes a caller-owned workspace or scratch and has a public size entry, as one table:
one byte fewer than the size entry reports is LA_ERR_WORKSPACE with the message the entry has always given, and a workspace pointer
off its alignment (by 4 where 8 bytes are required, by 2 where 4 are) is LA_ERR_ARG.  Every row is refused before any launch -- one
host block stands in for every device pointer and nothing is dereferenced -- so the table needs no GPU, and no row here may ever be
one that the library accepts.  Acceptance at exactly the reported size is what the GPU tests of each entry run, between guard bands."""
import ctypes as C
import os

import pytest

LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3
RES = (4, 8, 8, 16)


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


_block = C.create_string_buffer(256)
_P = (C.addressof(_block) + 63) & ~63          # a 64-byte aligned address inside the block: every pointer of a call
_res = (C.c_int * len(RES))(*RES)
_maps = (C.c_void_p * len(RES))(*[_P] * len(RES))
_taps = (C.c_float * 11)(*[1.0 / 11] * 11)
_weights = (C.c_float * 5)(*[0.2] * 5)


def _rows():
    """[(id, size of the workspace, call(ws, nbytes), word of the size refusal, required alignment of the workspace or None)]"""
    p = C.c_void_p(_P)
    v = C.c_void_p
    return [
        ('fd_gram', lambda L: L.la_fd_workspace_bytes(5, 7, 4),
         lambda L, ws, n: L.la_fd_gram_f32(p, 5, p, 7, 4, p, v(ws), n, None), b'fd_gram: workspace smaller than la_fd_workspace_bytes', 8),
        ('fd_finish', lambda L: L.la_fd_workspace_bytes(5, 7, 4),
         lambda L, ws, n: L.la_fd_finish_f64(v(ws), n, 5, 7, 4, p, p, None), b'fd_finish: workspace smaller than la_fd_workspace_bytes', 8),
        ('knn', lambda L: L.la_knn_scratch_bytes(5, 7, 4, 3),
         lambda L, ws, n: L.la_knn_f32(p, 5, p, 7, 4, 3, 0, p, p, v(ws), n, None), b'knn: scratch smaller than la_knn_scratch_bytes', 8),
        ('realism', lambda L: L.la_knn_scratch_bytes(5, 7, 4, 1),
         lambda L, ws, n: L.la_realism_f32(p, 5, p, 7, 4, p, p, p, v(ws), n, None), b'realism: scratch smaller than la_knn_scratch_bytes', 8),
        ('umap_graph', lambda L: L.la_umap_scratch_bytes(9, 3),
         lambda L, ws, n: L.la_umap_graph_f64(p, p, 9, 3, p, p, p, 54, p, v(ws), n, None), b'umap_graph: scratch smaller than la_umap_scratch_bytes', 8),
        ('sort_columns', lambda L: L.la_sort_columns_scratch_bytes(3, 17),
         lambda L, ws, n: L.la_sort_columns_f32(p, 3, 17, 17, v(ws), n, None), b'sort_columns: scratch smaller than la_sort_columns_scratch_bytes', 4),
        ('swd', lambda L: L.la_swd_scratch_bytes(9, 6, 5),
         lambda L, ws, n: L.la_swd_f32(p, p, 9, 6, p, 5, p, v(ws), n, None), b'swd: scratch smaller than la_swd_scratch_bytes', 8),
        ('swd_channel_stats', lambda L: L.la_swd_stats_scratch_bytes(9, 3, 4),
         lambda L, ws, n: L.la_swd_channel_stats_f64(p, 9, 3, 4, p, p, v(ws), n, None),
         b'swd_channel_stats: scratch smaller than la_swd_stats_scratch_bytes', 8),
        ('gram_pair_dist', lambda L: L.la_gram_pair_scratch_bytes(2, 5, 12),
         lambda L, ws, n: L.la_gram_pair_dist_f32(p, 2, 5, 12, p, p, v(ws), n, None), b'gram_pair_dist: scratch smaller than la_gram_pair_scratch_bytes', 8),
        ('pair_metrics', lambda L: L.la_pair_metrics_workspace_bytes(2, 1, 16, 16, 3, 2),
         lambda L, ws, n: L.la_pair_metrics_f32(p, p, None, None, 2, 1, 16, 16, _taps, 3, 2, _weights, 1e-4, 9e-4, p, p, p, p, v(ws), n, None),
         b'pair_metrics: workspace smaller than la_pair_metrics_workspace_bytes', 8),
        ('kid', lambda L: L.la_kid_workspace_bytes(3, 5, 6),
         lambda L, ws, n: L.la_kid_poly3_f32(p, 9, p, 9, 4, p, p, 3, 5, 6, p, p, p, v(ws), n, None), b'kid: workspace smaller than la_kid_workspace_bytes', 8),
        ('dc', lambda L: L.la_dc_workspace_bytes(5, 7),
         lambda L, ws, n: L.la_dc_count_f16(p, 5, p, 7, 16, p, p, p, v(ws), n, None), b'dc: workspace smaller than la_dc_workspace_bytes', 4),
        ('row_dist', lambda L: L.la_row_dist_workspace_bytes(4, 100),
         lambda L, ws, n: L.la_row_dist_f32(p, p, 4, 100, 2, 1.0, 1.0, p, 0, p, 1, v(ws), n, None), b'row_dist: workspace too small (la_row_dist_workspace_bytes)', 8),
        ('noise_reg', lambda L: L.la_noise_reg_scratch_bytes(_res, len(RES), 2),
         lambda L, ws, n: L.la_noise_reg_f32(_maps, _res, len(RES), 2, 1.0, 1.0, _maps, 0, p, 1, v(ws), n, None),
         b'noise_reg: workspace too small (la_noise_reg_scratch_bytes)', 8),
        ('proj_noise_tail', lambda L: L.la_proj_noise_tail_scratch_bytes(_res, len(RES), 2),
         lambda L, ws, n: L.la_proj_noise_tail_f32(_maps, _maps, _maps, _maps, _res, len(RES), 2, 1, 0.1, 0.9, 0.999, 1e-8, v(ws), n, None),
         b'proj_noise_tail: workspace too small (la_proj_noise_tail_scratch_bytes)', 8),
        ('fc', lambda L: L.la_fc_workspace_bytes(3, 7, 5),
         lambda L, ws, n: L.la_fc_bias_act_f32(p, p, p, p, 3, 7, 5, 1, v(ws), n, None), b'fc: workspace too small', None),
    ]


ROWS = _rows()


@pytest.mark.parametrize('name,size,call,word,align', ROWS, ids=[r[0] for r in ROWS])
def test_one_byte_short_is_a_workspace_refusal(lib, name, size, call, word, align):
    need = size(lib)
    assert need > 0
    assert call(lib, _P, need - 1) == LA_ERR_WORKSPACE
    assert word in lib.la_last_error(), lib.la_last_error()


@pytest.mark.parametrize('name,size,call,word,align', [r for r in ROWS if r[4]], ids=[r[0] for r in ROWS if r[4]])
def test_a_misaligned_workspace_is_an_argument_refusal(lib, name, size, call, word, align):
    """(with room to spare behind the pointer: the alignment is what is refused, whichever of the two checks the entry makes first)"""
    assert call(lib, _P + align // 2, size(lib) + 64) == LA_ERR_ARG
    assert b'align' in lib.la_last_error(), lib.la_last_error()
