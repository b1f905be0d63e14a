"""Workspace byte counts of the engines, the loop and every stand-alone size entry of the metric side, pinned to
tests/golden/workspace_sizes.json (recorded by tests/golden/make_golden_workspace_sizes.py from the build of commit 1e856d4, the last
one before the metric entries' private layouts -- counted in doubles, in bytes, or as casts of float counts -- became typed takes of
LaCarver; the engines' sizes in it are those of the build before their own carvers were folded in, which that commit still gives):
the shared carver lays every buffer out where the private ones did.  No GPU needed: the library loads without one and every call here
returns before any launch."""
import ctypes as C
import json
import os

import pytest

import workspace_cases as wc


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'workspace_sizes.json')) as f:
        return json.load(f)


def test_table_covers_what_it_claims(golden):
    names = set(golden)
    for entry in ('synth', 'disc', 'latent_opt-w', 'latent_opt-wplus'):
        for res in wc.RESOLUTIONS:
            for imgc in wc.IMG_CHANNELS:
                for mb in wc.MAX_BATCH:
                    assert f'{entry}-res{res}-c{imgc}-b{mb}' in names
    for in_res in wc.LPIPS_RES:
        for mb in wc.MAX_BATCH:
            assert {f'feat-vgg16-res{in_res}-b{mb}', f'feat-detector-res{in_res}-b{mb}'} <= names
            assert {f'lpips-{net}-S{in_res}-c{imgc}-b{mb}' for net in ('vgg16', 'tap') for imgc in wc.IMG_CHANNELS} <= names
    assert {name for name, _, _ in wc.metric_cases()} <= names
    assert {name.split('-')[0] for name, _, _ in wc.metric_cases()} == {
        'fd', 'knn', 'umap', 'sort', 'swd', 'swd_stats', 'gram', 'pair_metrics', 'kid', 'dc', 'pr', 'row_dist', 'noise_reg', 'noise_tail', 'fc'}
    assert all(isinstance(v, int) and v > 0 for v in golden.values())
    assert [k for k, v in golden.items() if v % 64 and k.split('-')[0] not in wc.UNROUNDED] == []


def test_workspace_sizes_are_the_recorded_ones(lib, golden):
    got = wc.measure(lib)
    assert set(got) == set(golden)
    assert {k: v for k, v in got.items() if v != golden[k]} == {}


@pytest.mark.parametrize('S', wc.LPIPS_RES)
@pytest.mark.parametrize('imgc,mb', [(1, 1), (2, 3), (2, 8)])
def test_set_lpips_accepts_exactly_the_recorded_size(lib, golden, S, imgc, mb):
    """la_latent_opt_set_lpips carves what la_latent_opt_lpips_workspace_bytes measured: that many bytes are accepted, 64 fewer are
    refused.  Both handles are created without a launch (a tap-only feature list packs no weights) and no buffer is dereferenced, so
    one host block stands in for every device pointer."""
    from latentaugment_amd import _lib, synthesis
    res = 2 * S
    fake = C.create_string_buffer(64)
    p = C.cast(fake, C.c_void_p)
    cfg = wc.opt_config(res)
    h, f = C.c_void_p(), C.c_void_p()
    nbytes = lib.la_latent_opt_workspace_bytes_ex(res, imgc, wc.W_DIM, C.byref(cfg), wc.MW, wc.MX, mb, 0)
    _lib.check(lib.la_latent_opt_create_ex(p, res, imgc, wc.W_DIM, C.byref(cfg), p, wc.MW, p, wc.MX, mb, 0, p, nbytes, C.byref(h)),
               'la_latent_opt_create_ex')
    try:
        tap = (_lib.FeatOp * 1)(_lib.FeatOp(synthesis.FEAT_TAP, 3, 3))
        params = (C.c_void_p * 1)(p.value)
        ws = lib.la_feat_workspace_bytes(1, tap, 3, S, imgc * mb)
        _lib.check(lib.la_feat_create(1, tap, params, 1, 3, S, imgc * mb, p, ws, None, C.byref(f)), 'la_feat_create')
        F = lib.la_feat_num_features(f)
        assert F == wc.tap_features(S)
        need = lib.la_latent_opt_lpips_workspace_bytes(imgc, F, S, wc.MF, mb)
        assert need == golden[f'lpips-tap-S{S}-c{imgc}-b{mb}']
        assert lib.la_latent_opt_set_lpips(h, f, p, wc.MF, S, 1.0, 0.0, p, need - 64) == -3          # LA_ERR_WORKSPACE, as every entry that takes one
        assert b'workspace too small' in lib.la_last_error()
        assert lib.la_latent_opt_set_lpips(h, f, p, wc.MF, S, 1.0, 0.0, p, need) == 0
    finally:
        if f:
            lib.la_feat_destroy(f)
        lib.la_latent_opt_destroy(h)
