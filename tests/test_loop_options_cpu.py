"""The host side of LatentAug without a GPU: the option record (`LoopOptions`), the record a stream lane runs with, which perceptual net
a configuration asks for, the lane rule as a pure function, and a source scan that keeps `opt` read-only and a lane a `LoopHandle`."""
import ast
import dataclasses
import os
import types

import pytest

from latentaugment_amd._lib import LatentAugHipError
from latentaugment_amd.loop_options import LoopOptions, lanes_eligible, resolve_perceptual_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latentaugment_amd')
OPTION_MODULE, LOOP_MODULES = 'loop_options.py', ('latent_aug.py', 'loop_handle.py', 'loop_options.py')

# the fields the reference's own LatentAug reads without a default (util_latent_aug.py:66-103)
REQUIRED = dict(img_resolution=32, batch_size=8, modalities_aug='A,B', opt_num_epochs=5, opt_lr=0.01, truncation_psi=1.0, w_pix=1.0, w_lpips=0.0,
                w_latent=0.3, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False)


def _opt(**kw):
    return types.SimpleNamespace(**{**REQUIRED, **kw})


def test_defaults_are_those_of_the_constructor_they_came_from():
    opt = _opt()
    before = dict(vars(opt))
    o = LoopOptions.from_opt(opt)
    assert vars(opt) == before
    want = dict(img_resolution=32, batch_size=8, modalities=('A', 'B'), opt_num_epochs=5, opt_lr=0.01, truncation_psi=1.0, w_pix=1.0, w_lpips=0.0,
                w_latent=0.3, w_disc=0.0, crop_size_aug=8, preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False,
                lpips_script='lpips_script', model_dir=None, interim_dir=None, dataset_aug=None, dataset_name_aug=None, dataset_w_name='',
                exp_stylegan=None, network_pkl_stylegan=None, step_img=None, step_w=None,
                criterion_mode='gemm', final_noise_mode='random', precision='f16x2', latent_space='w', lpips_script_path=None,
                lpips_vgg_path=None, lpips_lin_path=None, lpips_preproc=None, lpips_bank_range='unit', lpips_cache_compat=False,
                max_local_batch=0, norm_batch=0, stream_lanes='auto', lanes_selfcheck=True, hip_graph=True, overlap_criteria=2,
                loop_window=True, loop_window_columns=True)
    assert dataclasses.asdict(o) == want
    assert (o.criterion_code, o.final_noise_code, o.wplus) == (0, 2, False)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.batch_size = 4
    with pytest.raises(AttributeError):      # a required field stays required
        LoopOptions.from_opt(types.SimpleNamespace(**{k: v for k, v in REQUIRED.items() if k != 'w_pix'}))
    assert LoopOptions.from_opt(_opt(operand_scale='bound')) == o      # accepted and ignored


def test_option_module_needs_neither_torch_nor_the_library():
    tree = ast.parse(open(os.path.join(PKG, OPTION_MODULE)).read())
    mods = {a.name.split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    froms = {(n.level, n.module, a.name) for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) for a in n.names}
    assert mods <= {'dataclasses', 'os', 'random', 'typing', 'numpy'}
    assert {f for f in froms if f[1] != 'typing'} == {(1, '_lib', 'LatentAugHipError')}      # (the error class; nothing is loaded for it)
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr == 'load']


def test_conversions():
    f = LoopOptions.from_opt
    assert f(_opt(modalities_aug='MR,CT,')).modalities == ('MR', 'CT') and f(_opt(modalities_aug='A')).modalities == ('A',)
    assert [f(_opt(overlap_criteria=v)).overlap_criteria for v in (True, False, 0, 1, 2)] == [2, 0, 0, 1, 2]
    assert [f(_opt(latent_space=v)).latent_space for v in ('W+', 'w', None)] == ['w+', 'w', 'w']
    assert f(_opt(latent_space='W+')).wplus
    with pytest.raises(LatentAugHipError, match="latent_space = 'z'"):
        f(_opt(latent_space='z'))
    assert [f(_opt(criterion_mode=v)).criterion_code for v in ('gemm', 'collapsed')] == [0, 1]
    assert [f(_opt(final_noise_mode=v)).final_noise_code for v in ('none', 'const', 'random')] == [0, 1, 2]
    for name, bad, accepted in (('criterion_mode', 'fused', "'gemm', 'collapsed'"), ('final_noise_mode', 'fixed', "'none', 'const', 'random'"),
                                ('stream_lanes', 3, "'auto', 1, 2"), ('stream_lanes', '2', "'auto', 1, 2")):
        with pytest.raises(LatentAugHipError) as e:
            f(_opt(**{name: bad}))
        assert f'opt.{name}' in str(e.value) and accepted in str(e.value)
    assert [f(_opt(stream_lanes=v)).stream_lanes for v in ('auto', 1, 2)] == ['auto', 1, 2]
    # lpips_preproc: a scalar pair applies to all three repeated channels; not given stays distinguishable from the identity
    assert f(_opt(lpips_preproc=(2.0, -1))).lpips_preproc == ((2.0, 2.0, 2.0), (-1.0, -1.0, -1.0))
    assert f(_opt(lpips_preproc=([1, 2, 3], (0.5, 0.25, 0.0)))).lpips_preproc == ((1.0, 2.0, 3.0), (0.5, 0.25, 0.0))
    assert f(_opt(lpips_preproc=(1.0, 0.0))).lpips_preproc == ((1.0,) * 3, (0.0,) * 3) and f(_opt()).lpips_preproc is None
    with pytest.raises(AssertionError):
        f(_opt(lpips_preproc=((1.0, 2.0), 0.0)))
    # 0 or absent = derive
    assert [f(_opt(**kw)).norm_batch for kw in ({}, dict(norm_batch=0), dict(norm_batch=None), dict(norm_batch=16))] == [0, 0, 0, 16]
    assert [f(_opt(**kw)).max_local_batch for kw in ({}, dict(max_local_batch=0), dict(max_local_batch=4))] == [0, 0, 4]
    # the window of the perceptual criterion: relative to the centre crop in the centre modes
    assert f(_opt(img_resolution=256)).crop_window((3, 5)) == (41, 43)
    assert f(_opt(img_resolution=256, preprocess_aug='random_crop')).crop_window((3, 5)) == (3, 5)


@pytest.mark.parametrize('full', [4, 8, 16])
@pytest.mark.parametrize('overlap', [0, 1, 2])
def test_lane_record(full, overlap):
    parent = LoopOptions.from_opt(_opt(batch_size=full, verbose_log=True, stream_lanes=2, overlap_criteria=overlap, w_disc=0.5, w_lpips=2.0,
                                       lpips_preproc=(2.0, 0.5), latent_space='w+', norm_batch=0, hip_graph=False))
    lane = parent.lane(full)
    five = dict(batch_size=full // 2, max_local_batch=full // 2, norm_batch=full, verbose_log=False, stream_lanes=1)
    assert {k: getattr(lane, k) for k in five} == five
    assert lane.overlap_criteria == (1 if overlap == 2 else overlap)
    rest = set(LoopOptions.__dataclass_fields__) - set(five) - {'overlap_criteria'}
    assert len(rest) == len(LoopOptions.__dataclass_fields__) - 6 and all(getattr(lane, k) == getattr(parent, k) for k in rest)
    assert parent.batch_size == full and parent.stream_lanes == 2      # (the parent's record is not touched)


def test_resolve_perceptual_net(tmp_path):
    """Precedence, file names and refusals; os.path.isfile is all that is asked about a file (these are empty)."""
    d = tmp_path / 'models'
    d.mkdir()
    files = {n: str(d / n) for n in ('vgg16.pt', 'vgg16.pth', 'lpips_vgg.pth', 'mine.pt', 'v.pth', 'l.pth')}

    def touch(*names):
        for n in names:
            open(files[n], 'w').close()

    def res(feature_net=None, **kw):
        return resolve_perceptual_net(LoopOptions.from_opt(_opt(**{'w_lpips': 1.0, **kw})), feature_net)
    ops = [('maxpool',)]
    assert res(w_lpips=0.0) is None and res(ops, w_lpips=0.0) is None and res(w_lpips=0.0, lpips_script='lpips') is None
    assert res(ops) == ('ops', ops)
    # nothing on disk: the three failing cases of test_plugin_raises_without_the_weight_files, and the script branch's own
    touch('vgg16.pth')
    for kw in (dict(lpips_script='lpips'), dict(lpips_script='lpips', model_dir=str(d)),
               dict(lpips_script='lpips', lpips_vgg_path=files['vgg16.pth'], lpips_lin_path=str(d / 'no.pth')), dict(), dict(model_dir=str(d)),
               dict(lpips_script_path=str(d / 'no.pt'))):
        with pytest.raises(NotImplementedError, match='lpips_vgg_path'):
            res(**kw)
    assert res(ops, lpips_script='lpips') == ('ops', ops)      # feature_net= comes first, whatever is on disk
    # script: the given path before <model_dir>/vgg16.pt; <model_dir> only with lpips_script == 'lpips_script'
    touch('vgg16.pt')
    assert res(model_dir=str(d)) == ('script', files['vgg16.pt'])
    with pytest.raises(NotImplementedError):
        res(model_dir=str(d), lpips_script='lpips')      # (lpips_vgg.pth is still missing)
    touch('mine.pt')
    assert res(model_dir=str(d), lpips_script_path=files['mine.pt']) == ('script', files['mine.pt'])
    assert res(model_dir=str(d), lpips_script_path=str(d / 'no.pt')) == ('script', files['vgg16.pt'])
    assert res(lpips_script='lpips', lpips_script_path=files['mine.pt']) == ('script', files['mine.pt'])
    # reference weights: the two options before <model_dir>/vgg16.pth and <model_dir>/lpips_vgg.pth, each on its own
    touch('lpips_vgg.pth')
    assert res(model_dir=str(d), lpips_script='lpips') == ('reference', (files['vgg16.pth'], files['lpips_vgg.pth']))
    touch('v.pth', 'l.pth')
    assert res(lpips_script='lpips', lpips_vgg_path=files['v.pth'], lpips_lin_path=files['l.pth']) == ('reference', (files['v.pth'], files['l.pth']))
    assert res(model_dir=str(d), lpips_script='lpips', lpips_vgg_path=files['v.pth']) == ('reference', (files['v.pth'], files['lpips_vgg.pth']))
    # a script path given wins over the reference branch; with lpips_script == 'lpips_script' the state dicts are not looked at
    assert res(model_dir=str(d), lpips_script='lpips', lpips_script_path=files['mine.pt']) == ('script', files['mine.pt'])
    assert res(model_dir=str(d), lpips_vgg_path=files['v.pth'], lpips_lin_path=files['l.pth']) == ('script', files['vgg16.pt'])


def test_stream_lane_rule_as_a_function():
    """The truth table of test_host_cpu.py::test_stream_lane_rule against the pure function."""
    def rule(b, max_local, lanes='auto', w_disc=0.0, w_lpips=0.0):
        return lanes_eligible(LoopOptions.from_opt(_opt(batch_size=max_local, stream_lanes=lanes, w_disc=w_disc, w_lpips=w_lpips)), max_local, b)

    assert rule(8, 8) and rule(4, 4) and rule(16, 16) and rule(6, 6)
    assert not rule(2, 2) and not rule(5, 5) and not rule(4, 8)            # too small, odd, not the full batch
    assert rule(8, 8, w_disc=0.01) and rule(16, 16, w_disc=0.01) and not rule(4, 4, w_disc=0.01) and not rule(12, 12, w_disc=0.01)
    assert not rule(8, 8, w_lpips=10.0) and rule(8, 8, lanes=2, w_lpips=10.0) and not rule(8, 8, lanes=1)
    # beside the discriminator the perceptual criterion takes the lanes, unless its branches run one after the other
    assert rule(8, 8, w_disc=0.01, w_lpips=10.0)
    o = LoopOptions.from_opt(_opt(w_disc=0.01, w_lpips=10.0, overlap_criteria=False))
    assert not lanes_eligible(o, 8, 8) and lanes_eligible(dataclasses.replace(o, stream_lanes=2), 8, 8)


def _scan(name):
    return ast.parse(open(os.path.join(PKG, name)).read())


def _is_name(node, name):
    return isinstance(node, ast.Name) and node.id == name


def test_opt_is_read_only_and_a_lane_is_not_a_latentaug():
    for name in LOOP_MODULES:
        tree = _scan(name)
        for n in ast.walk(tree):
            where = f'{name}:{getattr(n, "lineno", 0)}'
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                a = n.args
                assert '_shared' not in [x.arg for x in a.posonlyargs + a.args + a.kwonlyargs + [y for y in (a.vararg, a.kwarg) if y]], where
            if isinstance(n, (ast.Assign, ast.AugAssign, ast.AnnAssign, ast.Delete)):
                targets = n.targets if isinstance(n, (ast.Assign, ast.Delete)) else [n.target]
                for t in targets:
                    for leaf in ast.walk(t):
                        assert not (isinstance(leaf, ast.Attribute) and _is_name(leaf.value, 'opt')), f'{where}: writes opt.{leaf.attr}'
            if isinstance(n, ast.Call):
                f = n.func
                if _is_name(f, 'setattr') or _is_name(f, 'delattr'):
                    assert not (n.args and _is_name(n.args[0], 'opt')), f'{where}: writes to opt'
                if (isinstance(f, ast.Attribute) and f.attr in ('copy', 'deepcopy') and _is_name(f.value, 'copy')) or _is_name(f, 'deepcopy'):
                    assert not (n.args and _is_name(n.args[0], 'opt')), f'{where}: copies opt'
                if _is_name(f, 'getattr') and n.args and _is_name(n.args[0], 'opt'):
                    assert name == OPTION_MODULE, f'{where}: getattr(opt, ...) outside {OPTION_MODULE}'
                if _is_name(f, 'LatentAug') or (isinstance(f, ast.Attribute) and f.attr == 'LatentAug'):
                    fn = next(d for d in ast.walk(tree) if isinstance(d, ast.FunctionDef) and any(c is n for c in ast.walk(d)))
                    assert (name, fn.name) == ('latent_aug.py', 'define_latentaugment'), f'{where}: LatentAug constructed in {fn.name}'
    # the scan itself finds what it is for
    assert 'getattr(opt' in open(os.path.join(PKG, OPTION_MODULE)).read()
    src = open(os.path.join(PKG, 'latent_aug.py')).read()
    assert 'LatentAug(phase, opt, save_dir, gpu_ids, **inject)' in src and 'getattr(opt' not in src
