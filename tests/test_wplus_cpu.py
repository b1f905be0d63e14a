"""W+ latent optimisation, host side: the W+ oracle pinned to the reference's W+ run (tests/golden/wplus_loop.npz), the C entries
and their argument checks, the plugin option and the shapes sample_from_inversion hands the loop.  No GPU needed."""
import argparse
import ctypes as C
import os
import random
import types

import numpy as np
import pytest
import torch

from oracle import feature_net, sg2_networks as nets
from helpers_formats import make_interim
import wplus_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    'latent': dict(w_latent=0.5),
    'pix': dict(w_pix=2.0),
    'disc': dict(w_disc=1.0),
    'lpips': dict(w_lpips=3.0),
    'all': dict(w_latent=0.3, w_pix=1.0, w_disc=0.5, w_lpips=2.0),
    'soft': dict(w_latent=0.3, w_pix=1.0, soft_aug=True, alpha=0.7),
}


@pytest.fixture(scope='module')
def gw(golden_dir):
    return np.load(os.path.join(golden_dir, 'wplus_loop.npz'))


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def _nets(gw):
    res, cbase, cmax, wdim = int(gw['res']), int(gw['cbase']), int(gw['cmax']), int(gw['wdim'])
    G = nets.make_generator(img_resolution=res, img_channels=2, channel_base=cbase, channel_max=cmax, seed=0, noise_strength=0.1,
                            w_dim=wdim, mapping_layers=2)
    D = nets.make_discriminator(img_resolution=res, img_channels=2, channel_base=cbase, channel_max=cmax, seed=0)
    return G, D


def test_fixture_has_distinct_rows(gw):
    w0, W = gw['w0'], gw['W']
    assert w0.shape[1] == W.shape[1] > 1
    assert np.abs(w0 - w0[:, :1]).max() > 0.1 and np.abs(W - W[:, :1]).max() > 0.1


@pytest.mark.parametrize('name', list(CASES))
def test_wplus_oracle_matches_reference(gw, name):
    """The W+ oracle (tests/wplus_cpu.py) against the reference's LatentAug.forward with the three W+ replacements: latents, final image
    (the reference's 'random' noise under the same seed) and the per-step loss scalars."""
    G, D = _nets(gw)
    fnet = feature_net.TinyFeatureNet(seed=5)
    ref = wplus_cpu.LatentAugRefWPlus(G, D, W=t(gw['W']), X=t(gw['X']), fea=[t(gw['fea0']), t(gw['fea1'])], feature_net=fnet,
                                      res=int(gw['res']), num_epochs=int(gw['epochs']), opt_lr=float(gw['lr']), crop_size=int(gw['crop']),
                                      **CASES[name])
    random.seed(6)
    pos = ref_pos = tuple(int(v) for v in gw[f'{name}_crop_pos'])
    torch.manual_seed(123)
    img, w_aug = ref.forward(t(gw['w0']), crop_pos=pos, record=True)
    assert ref_pos == pos and w_aug.shape == gw['w0'].shape
    np.testing.assert_allclose(w_aug.numpy(), gw[f'{name}_w_aug'], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(img.numpy(), gw[f'{name}_img'], rtol=1e-3, atol=2e-4)
    L = gw[f'{name}_losses']
    for col, key in enumerate(('loss_latent', 'loss_pix', 'loss_disc', 'loss_lpips')):
        np.testing.assert_allclose(np.array(ref.trace[key]), L[:, col], rtol=1e-4, atol=1e-6)
    # the rows moved independently: W+ is not a broadcast W run
    moved = w_aug.numpy() - gw['w0']
    if not CASES[name].get('soft_aug'):
        assert np.abs(moved - moved[:, :1]).max() > 1e-3


def test_wplus_float64_anchor(gw):
    """The float64 run of the 'all' case (const final noise): the float32 W+ oracle is close to it, as float32 rounding allows."""
    G, D = _nets(gw)
    fnet = feature_net.TinyFeatureNet(seed=5)
    pos = tuple(int(v) for v in gw['all_crop_pos'])
    ref = wplus_cpu.LatentAugRefWPlus(G, D, W=t(gw['W']), X=t(gw['X']), fea=[t(gw['fea0']), t(gw['fea1'])], feature_net=fnet, res=32,
                                      num_epochs=5, opt_lr=0.01, crop_size=8, final_noise_mode='const', **CASES['all'])
    _, w32 = ref.forward(t(gw['w0']), crop_pos=pos)
    np.testing.assert_allclose(w32.numpy(), gw['all_f64_w_aug'], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(gw['all_f64_w_steps'][-1], gw['all_f64_w_aug'], rtol=0, atol=1e-12)


def test_wplus_entries_exported_and_checked(lib):
    from latentaugment_amd import _lib
    for name in ('la_latent_opt_workspace_bytes_ex', 'la_latent_opt_create_ex'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.la_abi_version() == 1
    cfg = _lib.OptConfig(steps=5, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, w_latent=0.3, w_pix=1.0, crop=181, crop_off=38)
    args = (256, 2, 512, C.byref(cfg), 64, 16, 8)
    w = lib.la_latent_opt_workspace_bytes_ex(*args, 0)
    wp = lib.la_latent_opt_workspace_bytes_ex(*args, 1)
    assert w == lib.la_latent_opt_workspace_bytes(*args) > 0
    # w_opt, m, v, dw grow from [B][w_dim] to [B][num_ws][w_dim]: 4 x 8 x 13 x 512 floats more at 256^2 (num_ws 14)
    assert wp >= w + 4 * 8 * 13 * 512 * 4
    for bad in (-1, 2, 7):
        assert lib.la_latent_opt_workspace_bytes_ex(*args, bad) == 0
        h = C.c_void_p()
        # refused before anything is touched: null generator / workspace are never dereferenced
        assert lib.la_latent_opt_create_ex(None, 256, 2, 512, C.byref(cfg), None, 0, None, 0, 8, bad, None, 0, C.byref(h)) == -1
        assert b'latent_space' in lib.la_last_error()
    h = C.c_void_p()
    assert lib.la_latent_opt_create_ex(None, 256, 2, 30, C.byref(cfg), None, 0, None, 0, 8, 1, None, 0, C.byref(h)) == -1   # w_dim % 4


def _parser():
    from latentaugment_amd.augments.latent_aug import LatentAugment
    return LatentAugment.modify_commandline_options(argparse.ArgumentParser(), True)


def test_plugin_option_and_default():
    base = ['--model_dir', 'm', '--interim_dir', 'i']
    assert _parser().parse_args(base).latent_space == 'w'
    assert _parser().parse_args(base + ['--latent_space', 'w+']).latent_space == 'w+'
    with pytest.raises(SystemExit):
        _parser().parse_args(base + ['--latent_space', 'z'])
    # the reference's options keep their defaults
    o = _parser().parse_args(base)
    assert (o.opt_num_epochs, o.opt_lr, o.w_latent, o.alpha, o.soft_aug, o.init_w) == (10, 0.01, 1.0, 1.0, False, 'random')


def test_latent_aug_refuses_other_spaces():
    from latentaugment_amd import _lib
    from latentaugment_amd.latent_aug import LatentAug
    opt = types.SimpleNamespace(img_resolution=32, batch_size=2, modalities_aug='A,B', opt_num_epochs=1, opt_lr=0.01, truncation_psi=1.0,
                                w_pix=0.0, w_lpips=0.0, w_latent=0.0, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop',
                                soft_aug=False, alpha=1.0, verbose_log=False, latent_space='z')
    with pytest.raises(_lib.LatentAugHipError, match='latent_space'):
        LatentAug('train', opt, '/tmp', [0], generator=object())


def _plugin(space, codes, num_ws=6, w_dim=32):
    from latentaugment_amd.augments.latent_aug import LatentAugment
    p = LatentAugment.__new__(LatentAugment)
    p.latent_space, p.rand_aug, p.num_ws, p.w_dim, p.stats_dataset_w = space, False, num_ws, w_dim, codes
    return p


def test_sample_from_inversion_shapes(tmp_path):
    from latentaugment_amd import formats
    from latentaugment_amd.latent_aug import InMemoryLatentCodes
    lat, _ = make_interim(str(tmp_path))
    ds = formats.LatentCodeDataset(str(tmp_path / 'w.zip'), split='train', w_dim=32, num_ws=6)
    names = sorted(k for k in lat if k.startswith('train'))[:3]
    w = _plugin('w', ds).sample_from_inversion(names)
    assert w.shape == (3, 1, 32)
    np.testing.assert_array_equal(w[:, 0].numpy(), np.stack([lat[n][0] for n in names]))
    wp = _plugin('w+', ds).sample_from_inversion(names)
    assert wp.shape == (3, 6, 32) and wp.dtype == torch.float32
    np.testing.assert_array_equal(wp.numpy(), np.stack([lat[n] for n in names]))
    # [w_dim] and [1, w_dim] codes are broadcast to every row; any other shape is refused
    rng = np.random.RandomState(1)
    v = rng.randn(32).astype('float32')
    codes = InMemoryLatentCodes({'a': v, 'b': v[None], 'c': rng.randn(3, 32), 'd': rng.randn(6, 31)})
    wb = _plugin('w+', codes).sample_from_inversion(['a', 'b'])
    assert wb.shape == (2, 6, 32)
    np.testing.assert_array_equal(wb.numpy(), np.broadcast_to(v, (2, 6, 32)))
    assert _plugin('w', codes).sample_from_inversion(['a', 'b']).shape == (2, 1, 32)
    for bad in ('c', 'd'):
        with pytest.raises(ValueError, match='w\\+'):
            _plugin('w+', codes).sample_from_inversion([bad])


def test_latent_outputs_by_space():
    p = _plugin('w+', None)
    p.fname = ['a', 'b']
    p.w_AB = torch.randn([2, 6, 32])
    p.w_AB_aug = torch.randn([2, 6, 32])
    assert p.get_latent_output()['w'].shape == (2, 6, 32) and p.get_latent_input()['w'].shape == (2, 6, 32)
    np.testing.assert_array_equal(p.get_latent_output()['w'], p.w_AB_aug.numpy())
    p.latent_space = 'w'
    assert p.get_latent_output()['w'].shape == (2, 32)
