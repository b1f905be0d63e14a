"""TEST INFRASTRUCTURE -- the float64 / float32 restatement of the projector's noise-map optimisation (latentaugment_amd/projector.py,
la_noise.hip, la_projector.hip): the channel reduction that turns a layer's stored gradient into the gradient of its noise map, the
published regulariser written as the published loop, its gradient written out by hand as the gather the kernel runs, the noise tail
(Adam + re-normalisation), and a projector step with noise maps, composed with the oracle's generator (explicit `noises` under autograd)
and the restatements of projector_cases.py.

Shared by test_noise_cases_cpu.py and test_hip_projector_noise.py.  The error rule is the project's: integer-valued inputs whose float32
sums are exact must match float64 bit for bit; float inputs must lie within 4 x the error of the same restatement run in float32 on the
CPU + 2e-6 x the largest float64 magnitude (lpips_cases.bound).
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]
import lpips_cases as lc  # noqa: E402
import projector_cases as pj  # noqa: E402
from oracle import noise_ref  # noqa: E402

NOISE_LAYER0 = 0x40000000      # projector.NOISE_LAYER0: the layer slot of map li in the library's noise stream is NOISE_LAYER0 + li
REG_WEIGHT = 1e5


def layer_resolutions(G=None):
    """resolution of every SynthesisLayer in the engine's order: 4, 8, 8, 16, 16, ..."""
    G = pj.generator() if G is None else G
    return [r for r in G.synthesis.block_resolutions for _ in range(1 if r == 4 else 2)]


# ---- the channel reduction: gz [B, C, HW] holds dL/dz * act' * d[b, c]; the noise enters every channel alike in front of the activation
def noise_grad(gz, d, strength):
    """gn [B, HW] = strength * sum_c gz[b, c] / d[b, c], in the dtype of gz"""
    return strength * (gz / d.to(gz.dtype)[:, :, None]).sum(1)


# ---- the regulariser, as published (Karras et al. 2020, projector.py: reg_loss), per sample
def reg_loss(n):
    """n [B, r, r] -> [B]: the published loop; cyclic shifts; levels by avg_pool2d while the level is larger than 8 x 8"""
    x = n[:, None]
    reg = 0.0
    while True:
        reg = reg + (x * torch.roll(x, shifts=1, dims=3)).mean((1, 2, 3)) ** 2
        reg = reg + (x * torch.roll(x, shifts=1, dims=2)).mean((1, 2, 3)) ** 2
        if x.shape[2] <= 8:
            break
        x = F.avg_pool2d(x, kernel_size=2)
    return reg


def reg_levels(n):
    out = [n]
    while out[-1].shape[-1] > 8:
        out.append(F.avg_pool2d(out[-1][:, None], kernel_size=2)[:, 0])
    return out


def reg_grad(n):
    """d reg_loss(n).sum() / d n, written out: at a fine pixel the gather
    g[y][x] = sum_l 4^-l (2 a_l / N_l (n_l[y_l][x_l - 1] + n_l[y_l][x_l + 1]) + 2 c_l / N_l (n_l[y_l - 1][x_l] + n_l[y_l + 1][x_l])), (y_l, x_l) = (y >> l, x >> l)"""
    g = torch.zeros_like(n)
    for l, x in enumerate(reg_levels(n)):
        N = x.shape[1] * x.shape[2]
        a = (x * torch.roll(x, 1, 2)).mean((1, 2))
        c = (x * torch.roll(x, 1, 1)).mean((1, 2))
        gl = (2 * a / N)[:, None, None] * (torch.roll(x, 1, 2) + torch.roll(x, -1, 2)) + (2 * c / N)[:, None, None] * (torch.roll(x, 1, 1) + torch.roll(x, -1, 1))
        g = g + gl.repeat_interleave(1 << l, 1).repeat_interleave(1 << l, 2) / 4 ** l
    return g


def regulariser(maps, scale, weight):
    """The entry over a table of maps: (scale * sum over maps of reg_loss [B] float64, [weight * reg_grad(map)])"""
    reg = sum(reg_loss(n).double() for n in maps)
    return scale * reg, [weight * reg_grad(n) for n in maps]


# ---- the noise tail
def noise_tail(n, m, v, g, step, lr):
    """Adam (projector_cases.adam: the latent's constants), then n -= mean(n); n *= rsqrt(mean(n^2)) per map and sample; a map whose
    centred mean square is exactly 0 is left at zeros"""
    n, m, v = pj.adam(n, m, v, g.to(n.dtype), step, lr)
    n = n - n.mean((1, 2), keepdim=True)
    q = n.square().mean((1, 2), keepdim=True)
    return torch.where(q > 0, n * q.clamp_min(1e-300 if n.dtype == torch.float64 else 1e-38).rsqrt(), torch.zeros_like(n)), m, v


# ---- a projector step with noise maps
def synthesis(ws, maps, dtype, G=None):
    """The oracle generator with explicit noises: maps is one [B, r, r] per layer"""
    G = pj.generator_as(dtype) if G is None else G
    with pj._Dtype(dtype):
        return G.synthesis(ws.to(dtype), noise_mode='random', noises=[n.to(dtype)[:, None] for n in maps])


def synth_noise_grads(G, ws, maps, g_img, dtype):
    """(img, d<img, g_img> / d ws, [d<img, g_img> / d map]) by torch autograd through the oracle synthesis of G (any generator of
    oracle/sg2_networks.py; a copy in `dtype` is made) with explicit noises"""
    import copy
    Gd = copy.deepcopy(G).to(dtype)
    w = ws.detach().to(dtype).requires_grad_(True)
    nz = [n.detach().to(dtype).requires_grad_(True) for n in maps]
    img = synthesis(w, nz, dtype, Gd)
    grads = torch.autograd.grad(img, [w] + nz, g_img.to(dtype))
    return img.detach(), grads[0], list(grads[1:])


def initial_maps(B, seed, row0=0, G=None):
    """The maps project() starts from: unit normals of (seed, NOISE_LAYER0 + li, row0 + b) in the library's stream, float32 values"""
    return [torch.from_numpy(noise_ref.noise_normal(B, r * r, seed, NOISE_LAYER0 + li, row0)).reshape(B, r, r) for li, r in enumerate(layer_resolutions(G))]


def terms(case, ws, maps, tgt, dtype, reg_weight=REG_WEIGHT):
    """At ws [B, L, w_dim] and maps: (loss [B, 3] float64: perceptual, pixel, reg_weight * reg; d(sum of the three) / d(ws per style slot)
    [B, num_ws, w_dim]; d(sum) / d(map) per layer; img) by the chain the product runs -- distance gradients, preparation adjoint and the
    regulariser's gather written out, generator and feature net by their vector-Jacobian products."""
    G = pj.generator()
    B, C, R = tgt.shape[0], tgt.shape[1], tgt.shape[2]
    tgt = tgt.to(dtype)
    ws_full = ws.to(dtype).expand(B, G.num_ws, G.w_dim).clone().requires_grad_(True)
    nz = [n.to(dtype).clone().requires_grad_(True) for n in maps]
    img = synthesis(ws_full, nz, dtype)
    x = pj.prepare(img.detach(), case.k, case.pre_scale, case.pre_shift).requires_grad_(True)
    f = lc.feature_vector(lc.cast_ops(case.ops, dtype), x)
    with torch.no_grad():
        ft = pj.features(case, tgt, dtype)
    d, gfeat = pj.row_dist(f.detach(), ft, C, 1.0 / C, 2.0 / C)
    (gx,) = torch.autograd.grad(f, x, gfeat)
    g_img = pj.prepare_adjoint(gx, B, C, case.k, case.pre_scale)
    p = torch.zeros_like(d)
    if case.w_pix > 0:
        n_el = C * R * R
        p, gp = pj.row_dist(img.detach().reshape(B, n_el), tgt.reshape(B, n_el), 1, case.w_pix / n_el, 2.0 * case.w_pix / n_el)
        g_img = g_img + gp.reshape(B, C, R, R)
    grads = torch.autograd.grad(img, [ws_full] + nz, g_img)
    with torch.no_grad():
        reg, greg = regulariser([n.detach() for n in nz], reg_weight, float(np.float32(reg_weight)))
    return torch.stack([d, p, reg], dim=1), grads[0], [a + b for a, b in zip(grads[1:], greg)], img.detach()


def autograd_terms(case, w_opt, sigma, n, maps, tgt, reg_weight=REG_WEIGHT, dtype=torch.float64):
    """(loss [B, 3], d(sum) / d(w_opt), d(sum) / d(maps)) with the whole expression left to torch autograd, the regulariser as the published loop"""
    G = pj.generator()
    B, C = tgt.shape[0], tgt.shape[1]
    tgt = tgt.to(dtype)
    w = w_opt.to(dtype).clone().requires_grad_(True)
    nz = [t.to(dtype).clone().requires_grad_(True) for t in maps]
    img = synthesis((w + sigma * n.to(dtype)).expand(B, G.num_ws, G.w_dim), nz, dtype)
    ops = lc.cast_ops(case.ops, dtype)

    def feats(im):
        small = F.avg_pool2d(im, case.k) if case.k > 1 else im
        rows = torch.cat([small[:, c:c + 1].repeat(1, 3, 1, 1) for c in range(C)])
        return lc.feature_vector(ops, lc.affine(rows, case.pre_scale, case.pre_shift))
    d = (feats(img) - feats(tgt)).square().sum(1).reshape(C, B).mean(0)
    p = case.w_pix * (img - tgt).square().mean((1, 2, 3))
    reg = reg_weight * sum(reg_loss(t) for t in nz)
    grads = torch.autograd.grad((d + p + reg).sum(), [w] + nz)
    return torch.stack([d, p, reg], dim=1).detach(), grads[0], list(grads[1:])


def step(case, w, m, v, maps, nm, nv, ws, tgt, t, dtype, reg_weight=REG_WEIGHT, n_next=None):
    """One step of project(optimize_noise=True) from the given state (t 0-based): -> dict(loss, w, m, v, ws, maps, nm, nv)"""
    _, std = pj.w_stats()
    loss, dws, gns, _ = terms(case, ws, maps, tgt, dtype, reg_weight)
    lr = float(np.float32(pj.schedule(t, case.T, std)[0]))
    sigma = float(np.float32(pj.schedule(t + 1, case.T, std)[1])) if t + 1 < case.T else 0.0
    n_next = pj.noise(w.shape[0], case.L, w.shape[2], case.seed, t + 1) if n_next is None else n_next
    w, m, v, ws = pj.step_tail(dws, w, m, v, t + 1, lr, sigma, n_next)
    tails = [noise_tail(a, b, c, g, t + 1, lr) for a, b, c, g in zip(maps, nm, nv, gns)]
    return dict(loss=loss, w=w, m=m, v=v, ws=ws, maps=[x[0] for x in tails], nm=[x[1] for x in tails], nv=[x[2] for x in tails], lr=lr, sigma=sigma)


@functools.lru_cache(maxsize=None)
def noisy_targets(n=3, seed=11):
    """G(mapping(z), random noise maps) of n seeded z as float32 images: targets whose stochastic detail no latent explains"""
    G = pj.generator()
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn([n, pj.TINY['w_dim']], generator=gen, dtype=torch.float64)
    maps = [torch.randn([n, r, r], generator=gen, dtype=torch.float64) for r in layer_resolutions(G)]
    with pj._Dtype(torch.float64), torch.no_grad():
        ws = pj.generator_as(torch.float64).mapping(z, None, truncation_psi=1.0)
        return synthesis(ws, maps, torch.float64).float()


def simulate(case, tgt, steps, optimize_noise, dtype=torch.float64, reg_weight=REG_WEIGHT):
    """Free-running trajectory of `steps` steps: final (perceptual + pixel) per sample evaluated at the last w (sigma = 0 at the end)"""
    B = tgt.shape[0]
    avg, std = pj.w_stats()
    w = torch.from_numpy(avg).to(dtype).reshape(1, 1, -1).repeat(B, case.L, 1)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    ws = w + pj.schedule(0, case.T, std)[1] * pj.noise(B, case.L, w.shape[2], case.seed, 0).to(dtype)
    if optimize_noise:
        maps = [n.to(dtype) for n in initial_maps(B, case.seed)]
        nm, nv = [torch.zeros_like(n) for n in maps], [torch.zeros_like(n) for n in maps]
    losses = []
    for t in range(steps):
        if optimize_noise:
            s = step(case, w, m, v, maps, nm, nv, ws, tgt, t, dtype, reg_weight)
            w, m, v, ws, maps, nm, nv = s['w'], s['m'], s['v'], s['ws'], s['maps'], s['nm'], s['nv']
            losses.append(s['loss'])
        else:
            loss, dws, _ = pj.terms(case, ws, tgt, dtype)
            sigma = pj.schedule(t + 1, case.T, std)[1] if t + 1 < case.T else 0.0
            w, m, v, ws = pj.step_tail(dws, w, m, v, t + 1, pj.schedule(t, case.T, std)[0], sigma, pj.noise(B, case.L, w.shape[2], case.seed, t + 1))
            losses.append(loss)
    final = terms(case, w, maps, tgt, dtype, reg_weight)[0] if optimize_noise else pj.terms(case, w, tgt, dtype)[0]
    return dict(w=w, loss=torch.stack(losses), final=final[:, :2].sum(1))


# ---- case tables of the kernel tests
GRAD_SHAPES = [(HW, C, B) for HW in (16, 64, 1024) for C in (4, 16, 132, 512) for B in (1, 3)] + [(256, 16, 3), (65536, 4, 1)] + \
    [(1048576, 5, 1), (1048572, 5, 1)]      # B HW / 4 = 256 x 1024 float4 groups, where la_noise_grad_f32 stops slicing the channels (<1>), and one group fewer (<4>)
REG_SHAPES = [(r, B) for r in (4, 8, 16, 32, 64, 256) for B in (1, 3)]
TAIL_SHAPES = [(r, B) for r in (4, 8, 32, 256) for B in (1, 3)]
STEP_CASES = [('w', 0.0, 1, False), ('w+', 0.1, 1, False), ('w', 0.1, 2, True)]      # (space, w_pix, k, affine): both spaces, w_pix 0 and > 0, k 1 and 2
