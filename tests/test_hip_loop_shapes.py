"""What the latent loop itself owns (la_latent_opt.hip: la_step_tail_kernel, la_wplus_step_tail_kernel, la_wplus_gate_kernel,
la_broadcast_mix_kernel, la_pix_grad_kernel, la_lpips_gfeat_kernel, the coefficients, signs and accumulation of make_run / part_*, and the
strided and modulo forms of la_bank_dot / rows_sqnorm / la_l2_mean_from_bank and la_bank_colsum that only the loop reaches) against the
float64 restatement of tests/loop_cases.py, step by step, at the shapes no whole-loop test runs.

THE RULE.  Traced eager runs (`run_local(..., want_losses=True, trace=...)`), teacher forcing: step k's dL/dw and latent scalar are judged
from the traced w_{k-1}, its pixel / discriminator / perceptual scalars from the traced image, its Adam update from w_{k-1} and the traced
gradients 1..k (moments rebuilt in float64), the gate from the last traced latent and w0.  No expected value needs a free-running
trajectory to stay close, and Adam's step-1 g / (|g| + eps) amplifies nothing.  Every element of every step:
    worst |hip - f64| <= K x worst |f32-CPU - f64| + 2^-23 x (largest term)
K = 4 for what the loop owns (Adam, gate, latent and pixel scalars, closed-form dw); 4 / 6.7 / 4.2 in f32 / bf16x3 / f16x2 for dw and the
scalars that pass through an engine.  The float32 CPU run is the same restatement from the same forced state; the code under test sets no
budget.  The largest terms are written out in loop_cases.py.  An inactive criterion's column must be exactly 0.  GUARDED cases recompute
engine_cases.guard_of at every traced w_{k-1} and FAIL (never skip) when a pre-activation of G, D or the feature net is inside the guard.
The final image is only required to be, bit for bit, a fresh SynthesisEngine's forward of w_aug in the same precision with const noise.
Cases with a two-workgroup tail run the same handle again without trace or losses (the captured step: graph_state 1, w_aug bit-identical),
then B = 1 on that handle: against float64, and bit for bit against a fresh handle (ticket and counter reset, cached column sums).
Two full groups of eight slots need R >= 512 (num_ws 16): test_hip_fullsize.py covers that against goldens, not this file.

Each loss column is judged over all steps of a run as one vector: a single scalar's float32 error is one draw, not a scale.  GUARDED cases
carry calibrated conv biases (loop_cases.KINK_Z): whole channels sit three standard deviations on either side of the lrelu kink.

Measured on an MI355X, largest err / budget per group (the case that had it):
    Adam 0.226 (all-R32)   gate 0.102 (all-W+-R32)   dw closed form 0.252 (W-R16-wd88-B3)
    dw through the engines: f32 0.307 (disc-R32), bf16x3 0.298 (pix-R16), f16x2 0.394 (disc-R32)
    loss latent 0.499 (pix-R16-imgc3-Mx9-B9)   loss pix 0.434 (pix-R16)
    loss disc: f32 0.250 (all-W+-R32), bf16x3 0.200 (all-R32), f16x2 0.254 (all-R32)
    loss lpips: f32 0.174 (all-R32), bf16x3 0.123 (all-R32), f16x2 0.173 (lpips-R32)
Every final image was the engine's forward of w_aug bit for bit, every replayed w_aug and every B = 1 rerun bit-identical; the guard held at
every traced latent (smallest margin / guard 3.5, all-W+-R32 step 2).  The sweep found no defect.  Wall time of the file on the MI355X: 5.5 s for
32 tests (the float64 and float32 CPU runs included; slowest test 0.85 s).

Which case reaches which form (generated: python tests/loop_cases.py --table; test_loop_cases_cpu.py compares):
    W tail, one partial workgroup: W-R16-wd24-B1, W-R64-wd32-B2, W-R16-wd24-B9, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R32-imgc2-Mx9, pix-R256-imgc3-Mx3-B1, pix-R32, disc-R32, lpips-R32, all-R32, pix-R16
    W+ tail, one partial workgroup: W+-R16-wd24-B1, all-W+-R32
    W tail, exactly one full workgroup: W-R32-wd64-B4
    W+ tail, exactly one full workgroup: W+-R32-wd32-B4
    W tail, two workgroups, the last partial (la_step_ticket counts): W-R16-wd88-B3
    W+ tail, two workgroups, the last partial (la_step_ticket counts): W+-R64-wd32-B4
    the captured step and then B = 1 on the same handle (ticket, counter, cached column sums): W-R16-wd88-B3, W+-R64-wd32-B4
    slot sum: remainder only (num_ws 6): W-R16-wd24-B1, W-R16-wd88-B3, W-R16-wd24-B9, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R16
    slot sum: one group of eight, no remainder (num_ws 8): W-R32-wd64-B4, pix-R32-imgc2-Mx9, pix-R32, disc-R32, lpips-R32, all-R32
    slot sum: a group of eight and a remainder (num_ws 10): W-R64-wd32-B2
    slot sum of a synthesis gradient (dws not null): pix-R32, disc-R32, lpips-R32, all-R32, pix-R16
    W+ tail with a synthesis gradient: all-W+-R32
    column sums of 1 bank row: W-R16-wd24-B1, W+-R16-wd24-steps0, pix-R16-imgc1-Mx1
    column sums of 4 bank rows: W-R32-wd64-B4, W-R16-wd24-steps0, pix-R16-imgc3-Mx9-B9, pix-R16
    column sums of 5 bank rows: W+-R16-wd24-B1, W-R16-wd24-B9, lpips-R32, all-R32, all-W+-R32
    column sums of 17 bank rows: W+-R32-wd32-B4, W-R16-wd88-B3
    column sums of 29 bank rows: W+-R64-wd32-B4, W-R64-wd32-B2
    column sums: no 16-row group: W-R16-wd24-B1, W+-R16-wd24-B1, W-R32-wd64-B4, W-R16-wd24-B9, W-R16-wd24-steps0, W+-R16-wd24-steps0, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R32-imgc2-Mx9, pix-R256-imgc3-Mx3-B1, pix-R32, lpips-R32, all-R32, all-W+-R32, pix-R16
    column sums: a 16-row group and a remainder in one wave: W+-R32-wd32-B4, W-R16-wd88-B3, W+-R64-wd32-B4, W-R64-wd32-B2
    column sums: two 16-row groups in one wave: W+-R64-wd32-B4, W-R64-wd32-B2
    0 steps: W-R16-wd24-steps0, W+-R16-wd24-steps0
    1 steps: W-R16-wd24-B1, W+-R32-wd32-B4, W-R16-wd24-B9, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9
    2 steps: W+-R16-wd24-B1, W-R32-wd64-B4, W-R64-wd32-B2, pix-R32-imgc2-Mx9, pix-R256-imgc3-Mx3-B1
    5 steps: W-R16-wd88-B3, W+-R64-wd32-B4
    norm_batch unset: W-R16-wd24-B1, W+-R16-wd24-B1, W+-R32-wd32-B4, W-R16-wd88-B3, W-R64-wd32-B2, W-R16-wd24-B9, W-R16-wd24-steps0, W+-R16-wd24-steps0, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R256-imgc3-Mx3-B1, pix-R32, disc-R32, lpips-R32, all-R32, all-W+-R32, pix-R16
    norm_batch = 2 B: W-R32-wd64-B4, W+-R64-wd32-B4, pix-R32-imgc2-Mx9
    soft gate, alpha 0.7, W: W-R16-wd88-B3, W-R16-wd24-steps0
    soft gate, alpha 0.7, W+: W+-R32-wd32-B4, all-W+-R32
    hard gate: W-R16-wd24-B1, W+-R16-wd24-B1, W-R32-wd64-B4, W+-R64-wd32-B4, W-R64-wd32-B2, W-R16-wd24-B9, W+-R16-wd24-steps0, pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R32-imgc2-Mx9, pix-R256-imgc3-Mx3-B1, pix-R32, disc-R32, lpips-R32, all-R32, pix-R16
    latent dot, W: ldx = w_dim, xmod = w_dim: W-R16-wd24-B1, W-R32-wd64-B4, W-R16-wd88-B3, W-R64-wd32-B2, W-R16-wd24-B9, W-R16-wd24-steps0, pix-R16-imgc3-Mx9-B9, all-R32, pix-R16
    latent dot, W+: ldx = num_ws w_dim: W+-R16-wd24-B1, W+-R32-wd32-B4, W+-R64-wd32-B4, W+-R16-wd24-steps0, all-W+-R32
    latent dot: two passes of query rows (B 9): W-R16-wd24-B9, pix-R16-imgc3-Mx9-B9
    pixel dot: scalar form (cc^2 = 121): pix-R16-imgc1-Mx1, pix-R16-imgc3-Mx9-B9, pix-R16
    pixel dot: scalar form at an unaligned channel base: pix-R16-imgc3-Mx9-B9, pix-R16
    pixel dot: float4 form (cc^2 = 484): pix-R32-imgc2-Mx9, pix-R32, all-R32, all-W+-R32
    pixel dot: 16 K slices (cc^2 = 32761): pix-R256-imgc3-Mx3-B1
    pixel dot: two row blocks (Mx 9): pix-R16-imgc3-Mx9-B9, pix-R32-imgc2-Mx9, pix-R16
    pixel dot: two passes of query rows (B 9): pix-R16-imgc3-Mx9-B9
    pixel criterion accumulated over 2 channels and more: pix-R16-imgc3-Mx9-B9, pix-R32-imgc2-Mx9, pix-R256-imgc3-Mx3-B1, pix-R32, all-R32, all-W+-R32, pix-R16
    pixel criterion, imgc 1: pix-R16-imgc1-Mx1
    pixel criterion, imgc 2: pix-R32-imgc2-Mx9, pix-R32, all-R32, all-W+-R32
    pixel criterion, imgc 3: pix-R16-imgc3-Mx9-B9, pix-R256-imgc3-Mx3-B1, pix-R16
    Mx 1: pix-R16-imgc1-Mx1
    discriminator column: disc-R32, all-R32, all-W+-R32
    perceptual column, window at x != y, both non-zero: lpips-R32, all-R32, all-W+-R32
    every criterion at once: all-R32, all-W+-R32
    gradient through the engines in f32, bf16x3 and f16x2: pix-R32, disc-R32, lpips-R32, all-R32, all-W+-R32, pix-R16
"""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
_RATIOS = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    yield torch.device('cuda:0')
    print('\nlargest err / budget per group: ' + ', '.join(f'{k} {v[0]:.3f} ({v[1]})' for k, v in sorted(_RATIOS.items())))


def _aug(case, b, mode):
    from latentaugment_amd.latent_aug import LatentAug
    opt = types.SimpleNamespace(
        img_resolution=case.R, batch_size=case.max_batch, modalities_aug=','.join('ABC'[:case.imgc]), opt_num_epochs=case.steps, opt_lr=lc.LR,
        truncation_psi=1.0, w_pix=case.w_pix, w_lpips=case.w_lpips, w_latent=case.w_latent, w_disc=case.w_disc, crop_size_aug=lc.FEAT_CROP,
        preprocess_aug='center_random_crop', soft_aug=case.soft, alpha=case.alpha, verbose_log=False, criterion_mode='gemm',
        final_noise_mode='const', precision=mode, latent_space=case.space, norm_batch=case.norm_batch, stream_lanes=1, lpips_preproc=lc.PREPROC)
    la = LatentAug('train', opt, None, [0], generator=b.G, discriminator=b.D, banks=b.banks(), feature_net=b.ops)
    assert la.num_ws == case.num_ws and la.latent_rows == case.rows and (la.center_crop, la.center_off) == lc.crop_geometry(case.R)
    return la


def _traced(la, case, b, dev, B):
    """one traced eager run -> (the run in loop_cases.simulate's form, on the CPU; the final image and w_aug on the device)"""
    w0 = b.w0[:B]
    tr = {'want': ('w', 'img', 'grad') if case.img_crit else ('w', 'grad')}
    img, w_aug, losses = la.run_local(w0.to(dev), want_losses=True, crop_pos=case.crop_pos, trace=tr)
    torch.cuda.synchronize()
    steps = case.steps
    shape = (steps, B, case.rows, case.w_dim)          # (W traces come as [steps][B][w_dim])
    run = dict(w0=w0, w=list(tr['w'].cpu().reshape(shape)) if steps else [], grad=list(tr['grad'].cpu().reshape(shape)) if steps else [],
               img=list(tr['img'].cpu()) if steps and case.img_crit else None, losses=list(losses.cpu())[:steps], w_aug=w_aug.cpu())
    assert len(run['w']) == len(run['grad']) == steps and run['w_aug'].shape == (B, case.num_ws, case.w_dim)
    return run, img, w_aug


def _judge(case, b, run, mode):
    v = lc.judge(case, b, run, mode)
    for k, r in v.ratios.items():
        if r > _RATIOS.get(k, (0.0, ''))[0]:
            _RATIOS[k] = (r, case.name)
    return v.bad


def _final_image_is_the_engines(case, b, dev, mode, img, w_aug):
    from latentaugment_amd.synthesis import SynthesisEngine
    eng = SynthesisEngine.from_generator(b.G, dev, w_aug.shape[0], precision=mode)
    return [] if torch.equal(eng.forward(w_aug, noise_mode='const'), img) else [f'loop {case.name}: the final image is not the engine\'s forward of w_aug']


def _sweep(case, dev, mode):
    b = case.build()
    la = _aug(case, b, mode)
    run, img, w_aug = _traced(la, case, b, dev, case.B)
    bad = _judge(case, b, run, mode) + _final_image_is_the_engines(case, b, dev, mode, img, w_aug)
    assert not bad, '\n'.join(bad)
    return b, la, run, w_aug


@pytest.mark.parametrize('case', lc.TAIL_CASES, ids=[c.name for c in lc.TAIL_CASES])
def test_tail_sweep(dev, case):
    """the latent criterion alone (dw closed form), W and W+, f32: tail sizes, slot remainders, bank rows, step counts, norm_batch, gates"""
    b, la, run, w_aug = _sweep(case, dev, 'f32')
    if not case.rerun:
        return
    assert lc.reach(case)['tail']['workgroups'] > 1 and case.steps >= 2
    # the captured step on the same handle
    _, w_again, _ = la.run_local(b.w0[:case.B].to(dev), crop_pos=case.crop_pos)
    assert la.graph_state == 1 and torch.equal(w_again, w_aug)
    # B = 1 on the handle that just ran B = max: replayed (captured again for the new size), then traced
    _, w_one, _ = la.run_local(b.w0[:1].to(dev), crop_pos=case.crop_pos)
    assert la.graph_state == 1
    used, img1, w1 = _traced(la, case, b, dev, 1)
    fresh, _, _ = _traced(_aug(case, b, 'f32'), case, b, dev, 1)
    bad = _judge(case, b, used, 'f32') + _final_image_is_the_engines(case, b, dev, 'f32', img1, w1)
    assert not bad, '\n'.join(bad)
    assert torch.equal(w_one, w1)
    for key in ('w', 'grad', 'losses'):
        assert all(torch.equal(x, y) for x, y in zip(used[key], fresh[key])), key
    assert torch.equal(used['w_aug'], fresh['w_aug'])


@pytest.mark.parametrize('case', lc.SCALAR_CASES, ids=[c.name for c in lc.SCALAR_CASES])
def test_loss_scalar_sweep(dev, case):
    """the pixel criterion's scalar from the traced image: scalar and float4 dot, unaligned channel bases, 16 K slices, two row blocks, two
    passes of query rows, imgc 1 / 2 / 3"""
    _sweep(case, dev, 'f32')


@pytest.mark.parametrize('mode', lc.MODES)
@pytest.mark.parametrize('case', lc.GUARDED_CASES, ids=[c.name for c in lc.GUARDED_CASES])
def test_gradient_through_the_engines(dev, case, mode):
    """dL/dw of every step against one float64 step composed of the engines' restatements, every scalar column, Adam and the gate"""
    _sweep(case, dev, mode)
