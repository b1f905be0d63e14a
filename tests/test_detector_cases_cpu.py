"""No GPU: the restatements of tests/detector_cases.py equal torch's own ops in float64, the quantisation restatement equals torch's
expression bit for bit on the bin-edge set (and a fused multiply-add would not), the FC case list reaches both sides of every
predicate of the kernel's plan, and the host-only part of the detector loader (candidate enumeration on a saved scripted net) contains
the mapping that was built."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_cases as dc  # noqa: E402
import helpers_script_detector as hsd  # noqa: E402


@pytest.mark.parametrize('H,W,S', dc.PREP_SIZES)
def test_area_restatement_is_torchs_area_interpolation(H, W, S):
    x = dc.prep_inputs(3, H, W).double()
    got = dc.area_restate(x, S)
    assert dc.worst(got, F.adaptive_avg_pool2d(x, (S, S))) <= 1e-15
    assert dc.worst(got, F.interpolate(x, size=(S, S), mode='area')) <= 1e-15


@pytest.mark.parametrize('H,W,S', dc.PREP_SIZES)
def test_bilinear_restatement_is_torchs_bilinear_interpolation(H, W, S):
    x = dc.prep_inputs(3, H, W).double()
    got = dc.bilinear_restate(x, S)
    assert dc.worst(got, F.interpolate(x, size=(S, S), mode='bilinear', align_corners=False, antialias=False)) <= 1e-14


def test_area_bins_cover_the_input_and_stay_inside():
    for H, W, S in dc.PREP_SIZES:
        for n in (H, W):
            bins = dc.area_bins(n, S)
            assert bins[0][0] == 0 and bins[-1][1] == n and all(0 <= lo < hi <= n for lo, hi in bins)
    assert bool(dc.area_pow2_mask(16, 16, 8).all()) and not bool(dc.area_pow2_mask(10, 10, 7).all()) and bool(dc.area_pow2_mask(10, 10, 7).any())


def test_quantisation_restatement_is_torchs_expression_bit_for_bit():
    x = dc.bin_edge_inputs()
    assert x.numel() == 765
    want = dc.quant_torch(x)
    got = dc.quant_restate(x)
    assert torch.equal(got.to(torch.uint8), want) and torch.equal(got, want.float())
    # the set does its job: one fused multiply-add (a single rounding of x * 127.5 + 128) lands in another bin somewhere on it
    # (x * 127.5 + 128 is exact in float64: rounding it to float32 once is what a fused multiply-add returns)
    fused = np.floor(np.clip((x.numpy().astype(np.float64) * 127.5 + 128.0).astype(np.float32), 0, 255))
    assert int((fused != want.numpy()).sum()) > 0
    # values far outside clamp to the ends
    far = torch.tensor([-3.0, -1.0, 1.0, 3.0, 0.0])
    assert torch.equal(dc.quant_restate(far).to(torch.uint8), dc.quant_torch(far))


@pytest.mark.parametrize('relu', [False, True])
def test_fc_restatement_is_torchs_linear(relu):
    x, w, b = dc.fc_inputs(5, 100, 6)
    want = F.linear(x.double(), w.double(), b.double())
    want = F.relu(want) if relu else want
    assert dc.worst(dc.fc_restate(x, w, b, relu), want) <= 1e-14
    xi, wi, bi = dc.fc_inputs(5, 100, 6, integers=True)
    assert torch.equal(dc.fc_restate(xi, wi, bi, relu), F.relu(F.linear(xi.double(), wi.double(), bi.double())) if relu
                       else F.linear(xi.double(), wi.double(), bi.double()))


def test_fc_integer_inputs_stay_below_2_to_24():
    for N, K, O in dc.FC_SHAPES + [(dc.FC_REAL['N'], dc.FC_REAL['K'], dc.FC_REAL['O'])]:
        assert K * 1 * 2 + 8 < 2 ** 24


def test_fc_cases_reach_both_sides_of_every_plan_predicate():
    plans = [dc.fc_plan(*s) for s in dc.FC_SHAPES]
    for key, sides in [('nb', (1, 2)), ('vec', (True, False)), ('ragged_n', (True, False)), ('ragged_k', (True, False)),
                       ('ragged_o', (True, False)), ('ragged_slice', (True, False))]:
        for side in sides:
            assert any(p[key] == side for p in plans), (key, side)
    assert any(p['ks'] == 1 for p in plans) and any(p['ks'] > 1 for p in plans)
    assert any(p['ntiles'] == 1 for p in plans) and any(p['ntiles'] > 1 for p in plans)
    assert any(p['otiles'] == 1 for p in plans) and any(p['otiles'] > 1 for p in plans)
    assert any(p['ks'] > 1 and not p['vec'] for p in plans)
    # the real-size case: many slices, 32 feature tiles
    real = dc.fc_plan(dc.FC_REAL['N'], dc.FC_REAL['K'], dc.FC_REAL['O'])
    assert real['ks'] > 8 and real['otiles'] == 32 and real['nchunk'] == 784
    # every chunk belongs to exactly one slice, and a workspace sized for N serves every smaller N
    for p in plans + [real]:
        assert (p['ks'] - 1) * p['per'] < p['nchunk'] <= p['ks'] * p['per']
    for N, K, O in dc.FC_SHAPES:
        for n in range(1, N + 1):
            pn = dc.fc_plan(n, K, O)
            assert 256 + (pn['ks'] * n * O * 4 if pn['ks'] > 1 else 0) <= dc.fc_workspace_bytes(N, K, O)


def test_detector_restatement_is_torchs_own_ops():
    for case in dc.DET_CASES:
        ops, x = case.build()
        cur = x.double()
        for op in ops:
            if op[0] == 'conv':
                cur = F.relu(F.conv2d(cur, op[1].double(), op[2].double(), padding=1))
            elif op[0] == 'fc':
                cur = F.linear(cur.flatten(1), op[1].double(), op[2].double())
                cur = F.relu(cur) if op[3] else cur
            else:
                cur = F.max_pool2d(cur, 2) if op[0] == 'maxpool' else F.avg_pool2d(cur, 2)
        got = dc.detector_restate(ops, x)
        assert got.shape == (case.N, case.fcs[-1]) and dc.worst(got, cur) <= 1e-13


@pytest.mark.parametrize('resize', ['area', 'bilinear'])
@pytest.mark.parametrize('after', [1, 2])
def test_loader_candidates_contain_the_mapping_that_was_built(tmp_path, resize, after):
    """host only: among the enumerated readings of the saved module's tensors, the one that was built reproduces the module's own
    return_features output through the restatements, and no other reading does"""
    from latentaugment_amd.synthesis import detector_probe, run_scripted_detector, vgg16_detector_candidates
    path = tmp_path / 'det.pt'
    hsd.save_scripted_detector(path, resize=resize, features_after=after)
    cands = vgg16_detector_candidates(str(path))
    assert all(c.size == 32 for c in cands) and {(c.resize_mode, c.fc_depth) for c in cands} == {(m, d) for m in dc.PREP_MODES for d in (1, 2)}
    probe = detector_probe(32)
    assert probe.shape[1] == 3 and probe.shape[2] % 32 != 0 and not torch.equal(probe[:, 0], probe[:, 1])
    want = run_scripted_detector(cands[0].source, probe).double()
    hits = []
    for c in cands:
        x = dc.prep_restate(probe, c.size, c.resize_mode, False, c.pre_scale, c.pre_shift)
        got = dc.detector_restate(c.ops, x)
        if got.shape == want.shape and float((got - want).norm() / want.norm()) <= 2e-3:
            hits.append((c.resize_mode, c.fc_depth, c.pre_scale != (1.0, 1.0, 1.0)))
    assert hits == [(resize, after, True)]
