"""CPU-side checks of the product's host logic: the C-ABI library loads and exports every symbol the header declares,
the plugin registry / option surface mirror the reference, sharding + single-collective gather work under gloo, and
the product refuses to run without a GPU (no fallback)."""
import argparse
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    from latentaugment_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()
    declared = set(re.findall(r'\b(la_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/latentaug_hip.h but not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
    assert lib.la_abi_version() == 1


def _header():
    return open(os.path.join(ROOT, 'include', 'latentaug_hip.h')).read()


def test_binding_is_parsed_from_every_header_prototype():
    """The ctypes table is read from the header: one row per entry it declares, none missing, none extra."""
    from latentaugment_amd import _lib
    declared = set(re.findall(r'\b(la_[a-z0-9_]+)\s*\(', _header()))
    assert len(declared) >= 100
    assert set(_lib.SIGNATURES) == declared and len(_lib.SIGNATURES) == len(declared)
    sigs, structs = _lib.parse_header(_header())
    assert sigs == _lib.SIGNATURES and set(structs) == {'la_feat_op', 'la_opt_config'}


def test_binding_type_map_pins():
    """One entry per scalar kind of the parser's type map, written out by hand."""
    import ctypes as C
    from latentaugment_amd._lib import SIGNATURES as S
    P, I, L, F = C.c_void_p, C.c_int, C.c_long, C.c_float
    assert S['la_noise_normal_f32'] == (I, [P, L, L, C.c_ulonglong, C.c_uint, L, P])
    assert S['la_conv2d_workspace_bytes'] == (C.c_size_t, [I] * 13)
    assert S['la_last_error'] == (C.c_char_p, [])
    assert S['la_synth_image'] == (P, [P])
    assert S['la_synth_destroy'] == (None, [P])
    assert S['la_pairwise_l2_workspace_floats'] == (L, [I, L])
    assert S['la_bias_act_ex_f64'] == (I, [P] * 6 + [L, L, I, I, I] + [C.c_double] * 3 + [P])
    assert S['la_bias_act_ex_f32'] == (I, [P] * 6 + [L, L, I, I, I] + [F] * 3 + [P])
    assert S['la_filtered_lrelu_f32'] == (I, [P] * 7 + [I] * 16 + [F, F, F, I, I, P])


def test_binding_structs_follow_the_header():
    import ctypes as C
    from latentaugment_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', ' ', _header(), flags=re.S)
    for cname, cls in (('la_opt_config', _lib.OptConfig), ('la_feat_op', _lib.FeatOp)):
        body = re.search(r'typedef\s+struct\s+%s\s*\{(.*?)\}' % cname, hdr, re.S).group(1)
        names = [n for n in re.findall(r'[A-Za-z_]\w*', body) if n not in ('int', 'float')]
        assert [f[0] for f in cls._fields_] == names, cname
        assert all(t in (C.c_int, C.c_float) for _, t in cls._fields_)
    assert C.sizeof(_lib.OptConfig) == 17 * 4 and C.sizeof(_lib.FeatOp) == 3 * 4
    assert dict(_lib.OptConfig._fields_)['lr'] is C.c_float and dict(_lib.OptConfig._fields_)['crop_off'] is C.c_int
    cfg = _lib.OptConfig(steps=5, lr=0.5, crop=181, crop_off=38)
    assert (cfg.steps, cfg.lr, cfg.crop, cfg.crop_off, cfg.w_pix) == (5, 0.5, 181, 38, 0.0)
    op = _lib.FeatOp(1, 2, 3)
    assert (op.kind, op.cin, op.cout) == (1, 2, 3)


@pytest.mark.parametrize('text', [
    'int la_x(int a, int b;',                       # cannot be split
    'int la_x(int a) int la_y(int b);',
    'int la_x(long long n);',                       # scalar types the map does not have
    'int la_x(short n);',
    'wchar_t la_x(void);',
    'int la_x(int);',                               # no parameter name: `unsigned long` could not be told from `unsigned x`
    'int la_x();',
    'int la_x(void); int la_x(void);',              # declared twice
    'int some_global;',
    'typedef struct s { char c; } s;',
    'typedef struct s { int* p; } s;',
])
def test_binding_parser_refuses_what_it_does_not_know(text):
    from latentaugment_amd import _lib
    with pytest.raises(_lib.LatentAugHipError) as e:
        _lib.parse_header(text)
    assert 'C header' in str(e.value)
    _lib.parse_header('int la_x(int a);')           # (the well-formed neighbour of these parses)


def test_binding_needs_the_header(monkeypatch, tmp_path):
    from latentaugment_amd import _lib
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'latentaug_hip.h'))
    with pytest.raises(_lib.LatentAugHipError, match='latentaug_hip.h'):
        _lib._read_header()


def test_product_library_has_no_development_switches(lib):
    """Kernel-variant knobs and LA_* environment switches exist in the development build (-DLA_DEV) only: the product library neither
    exports la_dev_knob_set nor contains the names of the environment variables the development build reads."""
    from latentaugment_amd import _lib
    assert not hasattr(lib, 'la_dev_knob_set')
    blob = open(_lib.LIB_PATH, 'rb').read()
    for name in (b'LA_DEV_KNOBS', b'LA_HALO_W3', b'LA_FLAT_W3', b'LA_FORCE_MT', b'LA_NO_XS_HANDOFF', b'LA_NO_SEAM_FUSE', b'LA_NO_RGB_FUSE',
                 b'LA_NO_ZT_PITCH'):
        assert name not in blob, name
    src = open(os.path.join(ROOT, 'latentaugment_amd', '_lib.py')).read()
    assert 'os.environ' not in src      # the loader takes no path from the environment


def test_no_packed_fp32_arithmetic_in_any_kernel(lib, tmp_path):
    """Round 4 traced the 'two streams disturb each other' non-reproducibility of rounds 2-3 to packed-FP32 arithmetic (v_pk_fma_f32 /
    v_pk_mul_f32 / v_pk_add_f32, emitted by the SLP vectoriser and by vector-typed float expressions): while kernels of another
    hardware queue run on the chip, the high half of such a result comes out wrong for 16-lane groups.  The library is
    therefore built without them: every gfx950 code object embedded in the product .so is disassembled here and must contain none."""
    import subprocess
    from latentaugment_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import kernel_symbols
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not (os.path.isfile(kernel_symbols.BUNDLER) and os.path.isfile(objdump)):
        pytest.skip('LLVM tools of the ROCm image not found')
    objs = kernel_symbols.code_objects(_lib.LIB_PATH, tmp_path)          # (asserts that every bundle unbundles to a non-empty object)
    assert len(objs) >= 8
    kernels = mfma = 0
    for i, obj in enumerate(objs):
        dis = subprocess.run([objdump, '-d', str(obj)], capture_output=True).stdout.decode(errors='replace')
        bad = re.findall(r'v_pk_(?:fma|mul|add)_f32', dis)
        assert not bad, f'code object {i}: {len(bad)} packed-FP32 instructions'
        kernels += len(re.findall(r's_endpgm', dis)); mfma += len(re.findall(r'v_mfma_', dis))
    assert kernels > 100 and mfma > 500      # (the disassembly really covered the kernels)


def test_pure_host_entry_points(lib):
    assert lib.la_synth_num_ws(256) == 14 and lib.la_synth_num_ws(512) == 16 and lib.la_synth_num_ws(1024) == 18
    assert lib.la_synth_num_params(4) == 10 and lib.la_synth_num_params(256) == 94
    # (in*up + pad0 + pad1 - taps + down) // down   (upfirdn2d.cpp:35-36)
    assert lib.la_upfirdn2d_out_size(128, 2, 1, 2, 1, 4) == 256
    assert lib.la_upfirdn2d_out_size(257, 1, 1, 1, 1, 4) == 256
    assert lib.la_upfirdn2d_out_size(256, 1, 2, 1, 1, 4) == 128
    assert lib.la_modconv_ds_tiles(256) == 512 and lib.la_modconv_ds_tiles(4) == 1
    import ctypes as C
    ch = (C.c_int * 7)(512, 512, 512, 512, 512, 256, 128)
    nbytes = lib.la_synth_workspace_bytes(256, 2, 512, ch, 8)
    assert 1 << 30 < nbytes < 8 << 30      # config-f 256^2, B=8: a few GB of activations + packed weights


def test_no_cpu_fallback():
    from latentaugment_amd import _lib, ops
    from latentaugment_amd.latent_aug import LatentAug
    with pytest.raises(_lib.LatentAugHipError):
        ops.bias_act(torch.zeros([2, 3]), None)
    with pytest.raises(_lib.LatentAugHipError):
        ops.upfirdn2d(torch.zeros([1, 1, 8, 8]), ops.setup_filter([1, 3, 3, 1]))
    opt = types.SimpleNamespace(img_resolution=32, batch_size=2, modalities_aug='A,B', opt_num_epochs=1, opt_lr=0.01,
                                truncation_psi=1.0, w_pix=0.0, w_lpips=0.0, w_latent=0.0, w_disc=0.0, crop_size_aug=8,
                                preprocess_aug='center_random_crop', soft_aug=False, alpha=1.0, verbose_log=False)
    with pytest.raises(_lib.LatentAugHipError):
        LatentAug('train', opt, '/tmp', [], generator={})


def test_product_never_imports_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, 'latentaugment_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(d, f)).read()
                if re.search(r'^\s*(from|import)\s+oracle\b', src, re.M):
                    bad.append(f)
    assert not bad, bad


_SIZE_ENTRY = re.compile(r'la_\w*(?:workspace|scratch)_(?:bytes|floats)\w*$')
_TORCH_ALLOCATORS = {'empty', 'zeros', 'ones', 'full', 'empty_like', 'zeros_like', 'ones_like', 'full_like', 'empty_strided', 'rand', 'randn',
                     'tensor', 'arange'}


def workspace_allocation_faults(src, name='<src>'):
    """Where a piece of package source sizes a buffer by a la_*_(workspace|scratch)_(bytes|floats) entry and allocates it with anything
    but `_lib.workspace`: per function, the names that carry such a size (the call's result, and what is computed from them) may reach
    `_lib.workspace(...)` and ordinary arithmetic, never a torch allocator.  Also: `workspace` taken out of `_lib` by an import, which a
    test's monkeypatch of the module attribute would no longer reach."""
    import ast
    tree = ast.parse(src)
    faults = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and (node.module or '').split('.')[-1] == '_lib' and any(a.name in ('workspace', '*') for a in node.names):
            faults.append(f'{name}:{node.lineno}: workspace imported out of _lib')
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Attribute) and node.value.attr == 'workspace' and \
                isinstance(node.value.value, ast.Name) and node.value.value.id == '_lib':
            faults.append(f'{name}:{node.lineno}: _lib.workspace bound to another name')

    def is_size_call(n):
        return isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and _SIZE_ENTRY.match(n.func.attr)

    def is_lib_workspace(n):
        return isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'workspace' and \
            isinstance(n.func.value, ast.Name) and n.func.value.id == '_lib'

    def carries(expr, tainted):
        """A size reaches `expr` other than through a _lib.workspace(...) call inside it."""
        stack = [expr]
        while stack:
            n = stack.pop()
            if is_lib_workspace(n):
                continue
            if is_size_call(n) or (isinstance(n, (ast.Name, ast.Attribute)) and ast.unparse(n) in tainted):
                return True
            stack.extend(ast.iter_child_nodes(n))
        return False

    funcs = [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
    for fn in funcs:
        body = [n for n in ast.walk(fn)]
        if not any(is_size_call(n) for n in body):
            continue
        tainted, grew = set(), True
        while grew:
            grew = False
            for n in body:
                if isinstance(n, (ast.Assign, ast.AugAssign, ast.AnnAssign)) and n.value is not None and carries(n.value, tainted):
                    targets = list(n.targets) if isinstance(n, ast.Assign) else [n.target]
                    while targets:          # a name, an attribute as its dotted path (`self.n`, not all of `self`), the container of an item
                        t = targets.pop()
                        if isinstance(t, (ast.Tuple, ast.List)):
                            targets += t.elts
                        elif isinstance(t, (ast.Subscript, ast.Starred)):
                            targets.append(t.value)
                        elif ast.unparse(t) not in tainted:
                            tainted.add(ast.unparse(t))
                            grew = True
        for n in body:
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in _TORCH_ALLOCATORS and \
                    isinstance(n.func.value, ast.Name) and n.func.value.id in ('torch', 'np', 'numpy') and \
                    any(carries(a, tainted) for a in list(n.args) + [k.value for k in n.keywords]):
                faults.append(f'{name}:{n.lineno}: {fn.name} sizes a buffer by a workspace entry and allocates it with {n.func.value.id}.{n.func.attr}')
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ('new_empty', 'new_zeros', 'new_full', 'new_ones') and \
                    any(carries(a, tainted) for a in n.args):
                faults.append(f'{name}:{n.lineno}: {fn.name} sizes a buffer by a workspace entry and allocates it with .{n.func.attr}')
    return faults


def test_every_workspace_is_allocated_by_lib_workspace():
    """One allocation point (latentaugment_amd/_lib.workspace) for every workspace and scratch buffer the package hands to the library, so
    that tests/guarded_alloc.py can stand in for it: no package file sizes a buffer by a la_*_workspace_* entry and allocates it otherwise,
    none takes `workspace` out of the module, and the call sites are these -- a new one is added here, a vanished one fails."""
    pkg = os.path.join(ROOT, 'latentaugment_amd')
    sites, faults, entries = {}, [], set()
    for d, _, files in os.walk(pkg):
        for f in sorted(files):
            if f.endswith('.py'):
                rel = os.path.relpath(os.path.join(d, f), pkg)
                src = open(os.path.join(d, f)).read()
                faults += workspace_allocation_faults(src, rel)
                n = len(re.findall(r'\b_lib\.workspace\(', src))
                if n and rel != '_lib.py':          # (its own docstring says how it is called)
                    sites[rel] = n
                entries |= set(re.findall(r'\b(la_\w*(?:workspace|scratch)_(?:bytes|floats)\w*)\(', src))
    assert not faults, faults
    # synthesis: synth, mapping tmp, disc, feat, LPIPS pair, fc | loop_handle: loop, loop LPIPS | metrics: cdist, PR, KID, FD, DC (+ its PR
    # part), kNN, realism, style distance, pair metrics, SWD, SWD channel statistics | embedding: UMAP graph | projector: row distance
    # with the noise regulariser and tail | ops: filtered_lrelu signs, pairwise L2, conv2d scratch, grid-sample gradient
    assert sites == {'synthesis.py': 6, 'loop_handle.py': 2, 'metrics.py': 11, 'embedding.py': 1, 'projector.py': 1, 'ops.py': 4}
    from latentaugment_amd import _lib
    declared = {n for n in _lib.SIGNATURES if _SIZE_ENTRY.match(n)}
    assert len(declared) == 27 and entries <= declared
    # the entries of the header that the package does not call are those of the layer-level C entries, which only tests and scripts drive,
    # and the two that the library itself calls for the package (the Gram scratch inside la_feat_style_scratch_bytes, the sort's inside
    # la_swd_scratch_bytes)
    assert declared - entries == {'la_latent_opt_workspace_bytes', 'la_modconv_workspace_bytes', 'la_gram_pair_scratch_bytes',
                                  'la_sort_columns_scratch_bytes'}, declared - entries
    # the scan itself: what it must find, and what it must leave alone
    bad = ('def f(lib, dev):\n    n = lib.la_kid_workspace_bytes(1, 2, 3)\n    m = max(n, 64) // 8\n'
           '    return torch.empty([m], dtype=torch.float64, device=dev)\n')
    assert len(workspace_allocation_faults(bad)) == 1
    assert len(workspace_allocation_faults('def f(lib):\n    return torch.zeros([lib.la_pr_workspace_floats(3, 4)])\n')) == 1
    assert len(workspace_allocation_faults('def f(x, lib):\n    n = lib.la_fc_workspace_bytes(1, 2, 3)\n    return x.new_empty([n])\n')) == 1
    assert len(workspace_allocation_faults('def f(lib, dev):\n    nbytes = lib.la_knn_scratch_bytes(5, 7, 4, 3)\n'
                                           '    return torch.empty([nbytes // 8], dtype=torch.float64, device=dev)\n')) == 1
    assert len(workspace_allocation_faults('def f(self, lib):\n    self.n = lib.la_umap_scratch_bytes(9, 3)\n    self.ws = torch.empty([self.n])\n'
                                           '    self.out = torch.empty([4], device=self.device)\n')) == 1
    assert len(workspace_allocation_faults('from ._lib import workspace\n')) == 1
    assert len(workspace_allocation_faults('from . import _lib\nalloc = _lib.workspace\n')) == 1
    good = ('def f(lib, dev):\n    n = lib.la_kid_workspace_bytes(1, 2, 3)\n    ws = _lib.workspace(max(n, 64), dev, torch.float64)\n'
            '    out = torch.empty([4], device=dev)\n    return ws, out, ws.numel() * 8\n')
    assert workspace_allocation_faults(good) == []


def test_registry_and_options_match_reference_surface():
    from latentaugment_amd.augments import find_augment_using_name, get_option_setter
    from latentaugment_amd.augments.base_aug import BaseAugment
    cls = find_augment_using_name('latent')
    assert cls.__name__ == 'LatentAugment' and issubclass(cls, BaseAugment)
    for m in ('set_input', 'forward', 'get_output', 'get_latent_input', 'get_latent_output', 'sanity_check',
              'sample_from_inversion', 'sample_from_randn', 'modify_commandline_options'):
        assert hasattr(cls, m), m
    p = get_option_setter('latent')(argparse.ArgumentParser(), True)
    opt = p.parse_args(['--model_dir', 'm', '--interim_dir', 'i'])
    # names + defaults at augments/latent_aug.py:57-96 of the reference
    want = dict(gpu_ids_aug='0', img_resolution=256, truncation_psi=1.0, rand_aug=False, lower_bound_clip=False, step_img=20,
                step_w=5, lpips_script='lpips_script', opt_num_epochs=10, opt_lr=0.01, init_w='random', crop_size_aug=64,
                preprocess_aug='center_random_crop', w_pix=1.0, w_lpips=1.0, w_latent=1.0, w_disc=1.0, p_thres=1.0,
                soft_aug=False, alpha=1.0, verbose_log=False, modalities_aug='MR_nonrigid_CT,MR_MR_T2')
    for k, v in want.items():
        assert getattr(opt, k) == v, k
    for k in ('dataset_aug', 'dataset_name_aug', 'exp_stylegan', 'network_pkl_stylegan', 'dataset_w_name', 'exp_inv',
              'network_pkl_inv'):
        assert hasattr(opt, k)
    with pytest.raises(ImportError):
        find_augment_using_name('nonexistent')


def test_crop_geometry_and_shards():
    from latentaugment_amd.latent_aug import center_crop_geometry, shard_bounds
    assert center_crop_geometry(256) == (181, 38)      # round(37.5) -> 38 (python banker's rounding, as torchvision)
    assert center_crop_geometry(512) == (362, 75)
    assert center_crop_geometry(1024) == (724, 150)
    assert [shard_bounds(8, 2, r)[:2] for r in range(2)] == [(0, 4), (4, 8)]
    assert [shard_bounds(5, 4, r)[:2] for r in range(4)] == [(0, 2), (2, 4), (4, 5), (5, 5)]
    assert [shard_bounds(32, 8, r)[:2] for r in range(8)][-1] == (28, 32)


def test_synthetic_state_dict_matches_reference_names():
    from latentaugment_amd.synthetic import make_generator_state_dict
    sd, meta = make_generator_state_dict(img_resolution=16, img_channels=2, channel_base=256, channel_max=16, w_dim=32)
    from oracle import sg2_networks as nets
    G = nets.make_generator(img_resolution=16, img_channels=2, channel_base=256, channel_max=16, w_dim=32)
    missing, unexpected = G.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all('resample_filter' in k for k in missing), missing
    assert meta['num_ws'] == G.num_ws == 6


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import random
from latentaugment_amd.latent_aug import shard_bounds, gather_shards, broadcast_controls, get_params
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % sys.argv[2], rank=int(sys.argv[3]), world_size=2)
rank = dist.get_rank()
for B in (5, 8, 1):
    full = torch.arange(B * 6, dtype=torch.float32).reshape(B, 6)
    lo, hi, per = shard_bounds(B, 2, rank)
    local = full[lo:hi] * 2.0          # stand-in for the per-rank optimisation of its own samples
    out = gather_shards(local, per, B)
    assert torch.equal(out, full * 2.0), (B, rank, out)
# per-forward host draws: every rank ends with RANK 0's crop position and noise seed, whatever its own RNG state
random.seed(100 + rank)
mine = get_params(256, 64)['crop_pos']
cx, cy, seed = broadcast_controls(mine)
random.seed(100)
want = get_params(256, 64)['crop_pos']
assert (cx, cy) == tuple(want) and seed == random.getrandbits(48), (rank, cx, cy, seed)
dist.barrier()
dist.destroy_process_group()
print('ok', rank)
'''


def test_shard_gather_gloo_world2(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text(_WORKER)
    port = str(29500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, port, str(r)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert 'ok' in o


def test_torchscript_vgg16_mapping(tmp_path):
    """A local TorchScript `vgg16.pt` (the reference torch.jit.load()s NVIDIA's from a URL, util_latent_aug.py:35-43, and calls it
    with resize_images=False, return_lpips=True, :395): the loader recognises the 13 convolutions, the five LPIPS channel weights
    and the input layer from the tensors of a synthetic scripted module, and exactly ONE of its candidates reproduces the module's
    own output -- which one depends on whether the script stores the lin weights or their square roots, so nothing is assumed."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers_script import eval_ops_cpu, save_scripted_vgg
    from latentaugment_amd import _lib
    from latentaugment_amd.synthesis import vgg16_from_torchscript
    for lin_sqrt in (False, True):
        path = tmp_path / f'vgg16_{int(lin_sqrt)}.pt'
        save_scripted_vgg(path, width=8, seed=3, lin_sqrt=lin_sqrt)
        cands = vgg16_from_torchscript(str(path))
        assert [op[0] for op in cands[0].ops].count('conv') == 13 and [op[0] for op in cands[0].ops].count('tap') == 5
        assert [op[0] for op in cands[0].ops].count('maxpool') == 4
        assert abs(cands[0].pre_scale[0] - 1 / 58.395) < 1e-7 and abs(cands[0].pre_shift[2] + 103.53 / 57.375) < 1e-5
        x = torch.rand([2, 1, 32, 32], generator=torch.Generator().manual_seed(1)).repeat(1, 3, 1, 1) * 255
        want = torch.jit.load(str(path))(x, resize_images=False, return_lpips=True)
        good = []
        for c in cands:
            xx = x * torch.tensor(c.pre_scale).reshape(1, 3, 1, 1) + torch.tensor(c.pre_shift).reshape(1, 3, 1, 1)
            good.append(float((eval_ops_cpu(c.ops, xx) - want).norm() / want.norm()) < 1e-5)
        assert good.count(True) == 1 and cands[good.index(True)].lin_is_sqrt == lin_sqrt
    # a scripted module that is not a VGG16 is refused
    m = torch.jit.script(torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1)))
    with pytest.raises(_lib.LatentAugHipError):
        vgg16_from_torchscript(m)


def test_curve_png_writer(tmp_path):
    """The verbose_log curves (reference snapshot_stats, util_latent_aug.py:620-633) without matplotlib: a valid greyscale PNG whose
    polyline rises where the values rise."""
    import struct
    import zlib
    import numpy as np
    from latentaugment_amd.latent_aug import write_curve_png
    path = tmp_path / 'losses_loss.png'
    write_curve_png(str(path), [0.0, 1.0, 4.0, 9.0])
    blob = open(path, 'rb').read()
    assert blob[:8] == b'\x89PNG\r\n\x1a\n'
    w, h = struct.unpack('>II', blob[16:24])
    n = struct.unpack('>I', blob[33:37])[0]
    img = np.frombuffer(zlib.decompress(blob[41:41 + n]), np.uint8).reshape(h, w + 1)[:, 1:]
    dark = np.argwhere(img[30:-30, 30:-30] == 0)                      # the markers (frame excluded)
    first, last = dark[dark[:, 1] < 40], dark[dark[:, 1] > dark[:, 1].max() - 10]
    assert first[:, 0].mean() > last[:, 0].mean() + 100           # image rows grow downwards: the last value sits far above the first
    write_curve_png(str(path), [3.0])                              # a single epoch still gives a picture
    write_curve_png(str(path), [])


def test_gather_pair_packs_an_empty_shard(monkeypatch):
    """LatentAug._gather_pair on a rank whose shard is empty (B = 5 on 4 ranks: the last rank has no rows): 0 rows are packed at the full
    width, so the rank reaches the collective like the others, and the unpacked pair has the batch's shapes.  With rows, pack / unpack
    return image and latent unchanged."""
    import types
    from latentaugment_amd import latent_aug
    from latentaugment_amd.latent_aug import LatentAug
    me = types.SimpleNamespace(engine=types.SimpleNamespace(img_channels=2), res=4, num_ws=3, w_dim=5, group=None)
    seen = []

    def fake_gather(local, per, batch, group=None):      # the other ranks' rows: zeros
        seen.append(tuple(local.shape))
        return torch.cat([local, torch.zeros([batch - local.shape[0], local.shape[1]])])

    monkeypatch.setattr(latent_aug, 'gather_shards', fake_gather)
    img, w_aug = LatentAug._gather_pair(me, torch.empty([0, 2, 4, 4]), torch.empty([0, 3, 5]), 2, 5)
    assert seen == [(0, 2 * 4 * 4 + 3 * 5)] and img.shape == (5, 2, 4, 4) and w_aug.shape == (5, 3, 5)
    a, b = torch.randn([2, 2, 4, 4]), torch.randn([2, 3, 5])
    img, w_aug = LatentAug._gather_pair(me, a, b, 2, 5)
    assert torch.equal(img[:2], a) and torch.equal(w_aug[:2], b) and not img[2:].any() and not w_aug[2:].any()


def test_stream_lane_rule():
    """LatentAug.lanes_eligible (host logic, no GPU): two lanes take the FULL, even local batch of >= 4; with the discriminator a multiple
    of 8 (MinibatchStd groups sample n with n + b/4, n + 2b/4, n + 3b/4: the even / odd halves keep them only then); 'auto' not with the
    perceptual criterion (the discriminator and the perceptual branch run side by side inside one loop instead); 1 never."""
    import types
    from latentaugment_amd.latent_aug import LatentAug

    def rule(b, max_local, lanes='auto', w_disc=0.0, w_lpips=0.0):
        me = types.SimpleNamespace(stream_lanes=lanes, _max_local=max_local, w_disc=w_disc, w_lpips=w_lpips)
        return LatentAug.lanes_eligible(me, b)

    assert rule(8, 8) and rule(4, 4) and rule(16, 16) and rule(6, 6)
    assert not rule(2, 2) and not rule(5, 5) and not rule(4, 8)            # too small, odd, not the full batch
    assert rule(8, 8, w_disc=0.01) and rule(16, 16, w_disc=0.01) and not rule(4, 4, w_disc=0.01) and not rule(12, 12, w_disc=0.01)
    assert not rule(8, 8, w_lpips=10.0) and rule(8, 8, lanes=2, w_lpips=10.0) and not rule(8, 8, lanes=1)
    # the MinibatchStd claim itself: groups of the reference's reshape(G, -1, ...) against the groups inside the even / odd halves
    for n in (8, 16, 24):
        g = min(4, n)
        groups = {frozenset(m + j * (n // g) for j in range(g)) for m in range(n // g)}
        for half in (range(0, n, 2), range(1, n, 2)):
            half = list(half)
            gh = min(4, len(half))
            for m in range(len(half) // gh):
                assert frozenset(half[m + j * (len(half) // gh)] for j in range(gh)) in groups


def test_bench_witness_accepts_the_reference_and_rejects_a_wrong_batch():
    """bench.py's correctness witness (the last timed batch against the reference's fixture of the workload) on the host: the reference's
    own float32 result passes its own bound, a result two Adam steps off in a handful of entries or with a scrambled image does not, a
    workload without a fixture yields no verdict."""
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'fullsize_B.npz'))
    args = types.SimpleNamespace(w_disc=0.0, preset='B', res=256, channel_base=32768, batch=8, latent_steps=20)

    def run(w, img_sub):
        w_aug = torch.tensor(w, dtype=torch.float32)[:, None, :].repeat(1, 14, 1)
        full = torch.zeros([8, 2, 256, 256])
        full[:, :, 2::4, 2::4] = torch.tensor(img_sub, dtype=torch.float32)
        return bench.witness(args, w_aug, {'A': full[:, :1], 'B': full[:, 1:]}, 0, 8)
    ok = run(fx['ref32_w'], fx['ref32_img_sub'])
    assert ok['ok'] is True and abs(ok['w_rms_vs_f64'] - ok['reference_f32_rms_vs_f64']) < 1e-9
    bad_w = fx['ref32_w'].copy()
    bad_w[:, :8] += 0.02
    assert run(bad_w, fx['ref32_img_sub'])['ok'] is False
    assert run(fx['ref32_w'], fx['ref32_img_sub'][::-1].copy())['ok'] is False
    args.batch = 4
    assert bench.witness(args, torch.zeros([4, 14, 512]), {}, 0, 4) is None


def test_bench_dump_outputs_float32_and_seeded_sample_over_budget(tmp_path):
    """bench.py --dump-outputs: every array as <name>.npy in float32, whole while the arrays fit the budget; above it, the same fraction
    of each array's entries at fixed positions, so that two runs write the same sample."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    big = np.arange(4000, dtype=np.float64).reshape(40, 100)
    small = np.linspace(-1, 1, 1000).astype(np.float32)
    info = bench.dump_outputs(str(tmp_path / 'whole'), {'big': big, 'small': small})
    assert info == {'big': ((40, 100), 4000), 'small': ((1000,), 1000)}
    got = np.load(tmp_path / 'whole' / 'big.npy')
    assert got.dtype == np.float32 and np.array_equal(got, big.astype(np.float32))
    budget = 2000 * 4
    info = bench.dump_outputs(str(tmp_path / 'a'), {'big': big, 'small': small}, budget=budget)
    bench.dump_outputs(str(tmp_path / 'b'), {'big': big, 'small': small}, budget=budget)
    a_big, a_small = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'a' / 'small.npy')
    assert a_big.dtype == a_small.dtype == np.float32 and (a_big.nbytes + a_small.nbytes) <= budget
    assert info['big'] == ((40, 100), a_big.size) and a_big.size == 1600 and a_small.size == 400
    assert np.all(np.diff(a_big) > 0) and np.isin(a_big, big).all()      # sorted positions of the flat array, values kept as they are
    assert np.array_equal(a_big, np.load(tmp_path / 'b' / 'big.npy')) and np.array_equal(a_small, np.load(tmp_path / 'b' / 'small.npy'))


def test_kernel_class_map_is_the_profilers():
    """One class map (latentaugment_amd/kernel_classes.py) for bench.py's brackets and the rocprofv3 post-processing: its order is the
    C enum's (csrc/la_common.h), every class is described, and the kernels of the contraction classes land where the library brackets them."""
    import re
    from latentaugment_amd import kernel_classes as kc
    src = open(os.path.join(ROOT, 'latentaugment_amd', 'csrc', 'la_common.h')).read()
    enum = re.search(r'enum \{ (LA_PC_CONV_HALO.*?)LA_PC_NCLASS \}', src, re.S).group(1)
    names = [n.strip() for n in enum.replace('= 0', '').split(',') if n.strip()]
    want = {'LA_PC_CONV_HALO': 'conv_halo', 'LA_PC_CONV_FLAT': 'conv_flat', 'LA_PC_CONV_SPLITK': 'conv_splitk', 'LA_PC_CONV_F32': 'conv_f32',
            'LA_PC_PRESPLIT': 'operand_prep', 'LA_PC_FIR': 'fir', 'LA_PC_SEAM': 'seam_bwd', 'LA_PC_TORGB': 'torgb_fwd', 'LA_PC_BANK': 'bank'}
    assert [want[n] for n in names] == kc.CLASSES and set(kc.CLASS_KERNELS) == set(kc.CLASSES)
    assert kc.class_of('void la_conv_bf16_halo_kernel<128, 16, 3, 5>(LaConvArgs)') == 'conv_halo'
    assert kc.class_of('void la_conv_bf16_kernel<128, true, 16, 3, 1>(LaConvArgs)') == 'conv_splitk'
    assert kc.class_of('void la_conv_bf16_kernel<128, false, 16, 3, 2>(LaConvArgs)') == 'conv_flat'
    assert kc.class_of('la_conv_splitk_finish_kernel<4>') == 'conv_splitk' and kc.class_of('la_xscale_bound_kernel') is None
    assert kc.class_of('la_imgrad_pyramid_kernel(PyrArgs)') == 'fir' and kc.class_of('la_step_tail_kernel') is None


def test_reductions_and_noise_stream_have_one_home():
    """The Philox stream is written once (csrc/la_rng.h) and the wave xor butterfly lives in csrc/la_common.h (la_wave_sum / _max / _min):
    a kernel file calls them and does not write its own.  `kept` counts the written-out butterflies that stay, per file: the ones whose
    result is read only under a following `if (lane == 0)`, where a call changes the unit's instruction schedule (la_common.h,
    scripts/device_code_hashes.py).  The list is exact: a new copy fails here, and so does a listed site that has gone."""
    import glob
    csrc = os.path.join(ROOT, 'latentaugment_amd', 'csrc')
    kept = {'la_common.h': 4,            # la_wave_sum, la_wave_max, la_wave_min, la_block_max_256
            'la_conv_device.h': 5, 'la_conv_operand.hip': 5, 'la_criteria.hip': 2, 'la_frechet.hip': 1, 'la_grid_sample.hip': 1,
            'la_metrics.hip': 2, 'la_ops.hip': 1, 'la_pairmetrics.hip': 1, 'la_pathpoints.hip': 1, 'la_style.hip': 2}
    found, philox = {}, []
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        text, name = open(path).read(), os.path.basename(path)
        n = len(re.findall(r'for \(int (\w+) = [^;]+; \1 > 0; \1 >>= 1\)[^;]*__shfl_xor', text))      # (a tree loop over LDS has none)
        if n:
            found[name] = n
        if '0xd2511f53' in text.lower():
            philox.append(name)
        assert not re.findall(r'\b(?:la_proj_philox4x32_10|la_geom_philox4x32_10|la_wave_sum_f64|fd_block_sum|kid_block_sum)\b', text), name
    assert philox == ['la_rng.h'] and found == kept


def test_workspace_contract_has_one_home():
    """A caller-owned workspace is laid out by LaCarver (csrc/la_common.h) in elements of each buffer's own type, refused by
    LA_CHECK_WORKSPACE when it is short and by la_aligned<N> when it is misaligned: no file carves with a lambda of its own, none casts
    what a take returns (a float-counted take seen as doubles is where a factor of two goes missing), none keeps private alignment
    helpers, and LA_ERR_WORKSPACE is returned by the macro alone -- and by the launch profiler's two overflow reports, which are no
    workspace refusals.  The lists are exact: a new copy fails here, and so does a listed site that has gone."""
    import glob
    csrc = os.path.join(ROOT, 'latentaugment_amd', 'csrc')
    returns, lambdas, casts, helpers = {}, [], [], []
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        text, name = open(path).read(), os.path.basename(path)
        n = len(re.findall(r'\breturn\b[^;]*\bLA_ERR_WORKSPACE\b', text))
        if n:
            returns[name] = n
        if re.search(r'auto\s+take\s*=', text):
            lambdas.append(name)
        if re.search(r'(?:\*\s*\)|_cast\s*<[^;()]*>\s*\()\s*\w+(?:\.|->)take\b', text):
            casts.append(name)
        if re.search(r'\w_al(?:4|8)\b', text):
            helpers.append(name)
    assert returns == {'la_common.h': 1, 'la_prof.hip': 2}
    assert lambdas == [] and casts == [] and helpers == []
    # the scan itself: the forms it replaced
    assert re.search(r'(?:\*\s*\)|_cast\s*<[^;()]*>\s*\()\s*\w+(?:\.|->)take\b', 's.tsum = (double*)c.take(2 * (size_t)P * g.ntile * g.nseg);')
    assert re.search(r'\w_al(?:4|8)\b', 'LA_CHECK_ARG(swd_al4(desc) && umap_al8(mean), "...");')


def test_exact_fp32_tile_loop_has_one_home():
    """The LDS-staged exact-fp32 MFMA step (v_mfma_f32_32x32x2_f32) is written once, in csrc/la_f32_tile.h (la_f32_tile_mma), beside the
    pipeline that feeds it.  `kept` counts the written-out steps that stay, per file: la_featconv_gemm_kernel, whose weight tile is
    [co][k + 1] and not [k][col], and la_conv_igemm_kernel, which the shared form costs 52 VGPRs and global loads turned flat (DESIGN.md,
    'One home for the exact-fp32 tile loop').  The vector type of the 32 x 32 fp32 accumulator is defined there and, for the 16-bit
    kernels, in la_conv_device.h.  The list is exact: a new copy fails here, and so does a listed site that has gone."""
    import glob
    csrc = os.path.join(ROOT, 'latentaugment_amd', 'csrc')
    kept = {'la_f32_tile.h': 1, 'la_feat_conv.hip': 1, 'la_conv.hip': 1}
    found, typedefs = {}, []
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        text, name = open(path).read(), os.path.basename(path)
        n = text.count('__builtin_amdgcn_mfma_f32_32x32x2f32')
        if n:
            found[name] = n
        if re.search(r'typedef\s+float\s+\w+\s+__attribute__\(\(ext_vector_type\(16\)\)\)', text):
            typedefs.append(name)
    assert found == kept and typedefs == ['la_conv_device.h', 'la_f32_tile.h']
