"""The restatements of tests/noise_cases.py against torch autograd, the argument refusals of the noise entries and of project(), and the
plan record of a synthesis pass, which the noise gradient must not have changed.  No GPU: the library's host side only."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_cases as nc  # noqa: E402
import projector_cases as pj  # noqa: E402
import synth_cases as sc  # noqa: E402
import test_synth_plan_cpu as tp  # noqa: E402

ENTRIES = ('la_synth_backward_noise', 'la_noise_grad_f32', 'la_noise_reg_scratch_bytes', 'la_noise_reg_f32', 'la_proj_noise_tail_scratch_bytes',
           'la_proj_noise_tail_f32')
# the cases test_hip_projector_noise.py runs the noise gradient on: R8-imgc1 is the smallest of the table with a conv0 layer; in f32 every
# seam is a kernel, in f16x2 the conv0 seam of block 8 is fused into its conv1's backward and the conv1 seam of block 4 into the up layer's
PLAN_CASES = [('R8-imgc1', 'f32'), ('R8-imgc1', 'f16x2'), ('R16-noise-mixed', 'f32'), ('R16-noise-mixed', 'f16x2')]


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('r', [4, 8, 16, 32, 64])
def test_regulariser_gradient_is_autograd_of_the_published_loop(r):
    n = torch.randn([3, r, r], generator=torch.Generator().manual_seed(r), dtype=torch.float64).requires_grad_(True)
    (want,) = torch.autograd.grad(nc.reg_loss(n).sum(), n)
    got = nc.reg_grad(n.detach())
    assert want.abs().max() > 0
    assert (got - want).abs().max() <= 1e-13 * want.abs().max()
    assert len(nc.reg_levels(n.detach())) == {4: 1, 8: 1, 16: 2, 32: 3, 64: 4}[r]


def test_channel_reduction_is_the_noise_gradient_of_a_modulated_layer():
    """z = conv * d + strength * n, y = act(z + bias): with gz = dL/dz * d (what the seams store, act' included) the reduction gives dL/dn"""
    g = torch.Generator().manual_seed(3)
    B, Cc, HW, strength = 2, 5, 12, 0.3
    conv, d = torch.randn([B, Cc, HW], generator=g, dtype=torch.float64), torch.rand([B, Cc], generator=g, dtype=torch.float64) + 0.5
    n = torch.randn([B, HW], generator=g, dtype=torch.float64).requires_grad_(True)
    z = (conv * d[:, :, None] + strength * n[:, None]).requires_grad_(True)
    y = torch.nn.functional.leaky_relu(z, 0.2) * 2 ** 0.5
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (gz_plain,) = torch.autograd.grad(y, z, gy, retain_graph=True)
    (want,) = torch.autograd.grad(y, n, gy)
    got = nc.noise_grad(gz_plain * d[:, :, None], d, strength)
    assert (got - want).abs().max() <= 1e-14 * want.abs().max()


@pytest.mark.parametrize('key', nc.STEP_CASES, ids=[f'{k[0]}-pix{k[1]}-k{k[2]}' for k in nc.STEP_CASES])
def test_step_restatement_equals_autograd_through_the_oracle(key):
    case = pj.make_case(*key)
    tgt = pj.targets()
    B = tgt.shape[0]
    avg, std = pj.w_stats()
    w = torch.from_numpy(avg).reshape(1, 1, -1).repeat(B, case.L, 1)
    sigma = pj.schedule(0, case.T, std)[1]
    n0 = pj.noise(B, case.L, w.shape[2], case.seed, 0)
    maps = [m.double() for m in nc.initial_maps(B, case.seed)]
    loss, dws, gns, _ = nc.terms(case, w + sigma * n0, maps, tgt, torch.float64)
    loss_a, gw_a, gn_a = nc.autograd_terms(case, w, sigma, n0, maps, tgt)
    gw = dws if case.L > 1 else dws.sum(1, keepdim=True)
    assert loss.shape == (B, 3) and (loss - loss_a).abs().max() <= 1e-11 * loss_a.abs().max()
    assert (gw - gw_a).abs().max() <= 1e-10 * gw_a.abs().max()
    for li, (a, b) in enumerate(zip(gns, gn_a)):
        assert b.abs().max() > 0 and (a - b).abs().max() <= 1e-10 * b.abs().max(), li


def test_noise_tail_restatement():
    g = torch.Generator().manual_seed(5)
    n, grad = torch.randn([3, 8, 8], generator=g, dtype=torch.float64), torch.randn([3, 8, 8], generator=g, dtype=torch.float64)
    out, m, v = nc.noise_tail(n, torch.zeros_like(n), torch.zeros_like(n), grad, 1, 0.05)
    assert out.mean((1, 2)).abs().max() < 1e-15 and (out.square().mean((1, 2)) - 1).abs().max() < 1e-14
    flat, _, _ = nc.noise_tail(torch.full([1, 4, 4], 0.75, dtype=torch.float64), torch.zeros([1, 4, 4], dtype=torch.float64), torch.zeros([1, 4, 4], dtype=torch.float64),
                               torch.full([1, 4, 4], 2.0, dtype=torch.float64), 1, 0.05)
    assert torch.equal(flat, torch.zeros_like(flat))


def test_entries_are_declared_and_exported(lib):
    from latentaugment_amd import _lib
    P, I, L, D, F_, Z = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_float, C.c_size_t
    want = {'la_synth_backward_noise': (I, [P] * 5),
            'la_noise_grad_f32': (I, [P, P, L, I, I, L, F_, P, P]),
            'la_noise_reg_scratch_bytes': (Z, [P, I, I]),
            'la_noise_reg_f32': (I, [P, P, I, I, D, F_, P, I, P, L, P, Z, P]),
            'la_proj_noise_tail_scratch_bytes': (Z, [P, I, I]),
            'la_proj_noise_tail_f32': (I, [P] * 5 + [I] * 3 + [F_] * 4 + [P, Z, P])}
    assert set(want) == set(ENTRIES)
    for name in ENTRIES:
        assert _lib.SIGNATURES[name] == want[name], name
        assert getattr(lib, name).argtypes == want[name][1]


def test_refusals_carry_a_message(lib):
    def err():
        return lib.la_last_error().decode()
    buf = (C.c_double * 4096)()
    f = C.cast(buf, C.c_void_p)
    ptrs = (C.c_void_p * 2)(f, f)

    def res(*r):
        return (C.c_int * len(r))(*r)
    # resolutions that are not 4 << k, empty or oversized tables
    for r in (0, 2, 6, 12, 24, 8192):
        assert lib.la_noise_reg_scratch_bytes(res(r), 1, 1) == 0 and '4 << k' in err(), r
        assert lib.la_proj_noise_tail_scratch_bytes(res(r), 1, 1) == 0 and '4 << k' in err(), r
        assert lib.la_noise_reg_f32(ptrs, res(r), 1, 1, 1.0, 1.0, ptrs, 0, f, 1, f, 1 << 15, None) == -1 and '4 << k' in err(), r
        assert lib.la_proj_noise_tail_f32(ptrs, ptrs, ptrs, ptrs, res(r), 1, 1, 1, 0.1, 0.9, 0.999, 1e-8, f, 1 << 15, None) == -1 and '4 << k' in err(), r
    for nmaps, B in ((0, 1), (33, 1), (1, 0)):
        assert lib.la_noise_reg_scratch_bytes(res(*([4] * 33)), nmaps, B) == 0 and 'nmaps' in err()
        assert lib.la_proj_noise_tail_scratch_bytes(res(*([4] * 33)), nmaps, B) == 0 and 'nmaps' in err()
    assert lib.la_noise_reg_f32(None, res(4), 1, 1, 1.0, 1.0, ptrs, 0, f, 1, f, 1 << 15, None) == -1 and 'null' in err()
    assert lib.la_noise_reg_f32(ptrs, res(4), 1, 1, 1.0, 1.0, ptrs, 0, None, 1, f, 1 << 15, None) == -1 and 'null' in err()
    assert lib.la_noise_reg_f32(ptrs, res(4), 1, 1, 1.0, 1.0, ptrs, 0, f, 0, f, 1 << 15, None) == -1 and 'reg_stride' in err()
    assert lib.la_noise_reg_f32((C.c_void_p * 2)(None, f), res(4, 4), 2, 1, 1.0, 1.0, ptrs, 0, f, 1, f, 1 << 15, None) == -1 and 'null or misaligned' in err()
    need = lib.la_noise_reg_scratch_bytes(res(4, 16), 2, 3)
    assert need > 0 and need % 64 == 0
    assert lib.la_noise_reg_f32(ptrs, res(4, 16), 2, 3, 1.0, 1.0, ptrs, 0, f, 1, f, need - 64, None) == -3 and 'workspace too small' in err()
    need = lib.la_proj_noise_tail_scratch_bytes(res(4, 16), 2, 3)
    assert need > 0
    assert lib.la_proj_noise_tail_f32(ptrs, ptrs, ptrs, ptrs, res(4, 16), 2, 3, 1, 0.1, 0.9, 0.999, 1e-8, f, need - 64, None) == -3 and 'workspace too small' in err()
    assert lib.la_proj_noise_tail_f32(ptrs, ptrs, ptrs, ptrs, res(4, 16), 2, 3, 0, 0.1, 0.9, 0.999, 1e-8, f, need, None) == -1 and '1-based' in err()
    assert lib.la_proj_noise_tail_f32(ptrs, None, ptrs, ptrs, res(4, 16), 2, 3, 1, 0.1, 0.9, 0.999, 1e-8, f, need, None) == -1 and 'null' in err()
    # the channel reduction
    assert lib.la_noise_grad_f32(None, f, 4, 1, 4, 16, 0.1, f, None) == -1 and 'null' in err()
    assert lib.la_noise_grad_f32(f, f, 4, 1, 4, 18, 0.1, f, None) == -1 and 'multiple of 4' in err()
    assert lib.la_noise_grad_f32(f, f, 4, 0, 4, 16, 0.1, f, None) == -1 and 'at least 1' in err()
    assert lib.la_noise_grad_f32(C.c_void_p(f.value + 4), f, 4, 1, 4, 16, 0.1, f, None) == -1 and '16-byte' in err()
    assert lib.la_synth_backward_noise(None, f, f, None, None) == -1 and 'null' in err()


def test_project_refuses_a_bad_regulariser_weight():
    from latentaugment_amd import _lib
    from latentaugment_amd.projector import NOISE_LAYER0, check_project_args
    assert NOISE_LAYER0 == nc.NOISE_LAYER0
    good = ((3, 2, 32, 32), 2, 32, 8, 32, 20, 'w', 0.0, None)
    assert check_project_args(*good) == 1 and check_project_args(*good, regularize_noise_weight=0.0) == 1
    assert check_project_args(*good, regularize_noise_weight=1e5) == 1
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(_lib.LatentAugHipError, match='regularize_noise_weight'):
            check_project_args(*good, regularize_noise_weight=bad)


@pytest.mark.parametrize('name,mode', PLAN_CASES)
def test_plan_record_is_unchanged(lib, name, mode):
    """la_synth_backward_noise is la_synth_backward's pass: the plan of a pass is what synth_cases.branch_plan says, as before"""
    case = sc.SYNTH_BY_NAME[name]
    tp.check_against_the_model(lib, case, mode, case.B)
    plan = tp.ask(lib, case, mode)
    want = sc.branch_plan(case, mode)
    assert [plan['layers'][2 * k]['seam'] for k in range(want['nblocks'])] == [b['seam'] for b in want['blocks']]
    if name == 'R8-imgc1':
        seams = [plan['layers'][ci]['seam'] for ci in range(3)]
        assert seams == (['kernel'] * 3 if mode == 'f32' else ['fused', 'fused', 'kernel'])
