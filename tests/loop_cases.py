"""Case table, seeded inputs and the float64 / float32 restatement of what the latent loop itself owns (la_latent_opt.hip): the step
tails (la_step_tail_kernel, la_wplus_step_tail_kernel), the gates (la_broadcast_mix_kernel, la_wplus_gate_kernel), the pixel gradient
(la_pix_grad_kernel), the perceptual feature gradient (la_lpips_gfeat_kernel), the coefficients, signs and accumulation of make_run /
part_*, and the strided and modulo forms of the bank kernels only the loop reaches.  Shared by test_loop_cases_cpu.py and
test_hip_loop_shapes.py.  No GPU and no ctypes here; every input is synthetic and seeded.  The helpers (`Pre`, `guard_of`, `worst`) are
those of tests/engine_cases.py; the networks are restated by synth_cases.synth_restate and engine_cases.disc_restate / feat_restate.

TEACHER FORCING.  A traced run hands back, per step, the latent after the step, the synthesised image, dL/dw and the four loss
scalars.  `judge` compares every step with a restatement that starts from the state the kernels themselves were in: step k's
gradient and latent loss from the traced w_{k-1}, its image scalars from the traced image, its Adam update from w_{k-1} and the traced
gradients 1..k, the gate from the last traced latent.  Nothing needs a free-running trajectory to stay close.  Every comparison is
    worst |got - f64| <= K x worst |f32-CPU - f64| + 2^-23 x (largest term)
with the float32 run of the same restatement from the same forced state; K = 4 for what the loop owns, 4 / 6.7 / 4.2 (f32 / bf16x3 /
f16x2, the convention of test_hip_synth_shapes.py and test_hip_engine_shapes.py) for what passes through an engine.  The largest
term: of a loss scalar in GEMM form coef x sum_mn (|Y_m|^2 + |X_n|^2), the positive sum its cancellation starts from; of the
discriminator scalar the scalar, or w / n x sum_b sigmoid(-l_b) |l_b| (one rounding of every logit through softplus' slope) if that is
larger; of a closed-form gradient |lat2| x num_ws x Mw x max|w| (W+: per slot, without num_ws); of a gradient
through the engines max|dw|, or the latent term if that is larger; of the Adam update and the gate max|w|.  dw, Adam and the gate are
judged step by step, element by element; each loss column over all steps of the run as one vector (the float32 error of a single
scalar is one draw, not a scale).

Three kinds of case.
CLOSED   the latent criterion alone: dw is a closed form, no network in it.
SCALARS  image criteria whose loss scalars are judged from the traced image; dw is not compared (Adam, gate and counter still are).
GUARDED  image criteria, dw through the engines: one float64 step composed of synth_restate (forward, then backward with the
         criteria's image gradient), disc_restate, feat_restate and the criteria formulas.  The seed is the first of 0..63 whose
         free-running float64 trajectory keeps every pre-activation of G, D and the feature net further than engine_cases' guard
         from a kink at every step (`first_seed`); the GPU test recomputes the guard at every traced w_{k-1} and fails below it.

`reach` restates on the host which launch form a case takes.  It only proves reach; no expected value comes from it.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_cases as ec  # noqa: E402
import synth_cases as sc  # noqa: E402
from engine_cases import EPS32, guard_of, worst  # noqa: E402,F401

MODES = sc.MODES
K_LOOP = 4.0
K_ENGINE = {'f32': 4.0, 'bf16x3': 6.7, 'f16x2': 4.2}
LR, BETA1, BETA2, ADAM_EPS = 0.01, 0.9, 0.999, 1e-8
NOISE = float(torch.tensor(0.1, dtype=torch.float32))
CLAMP = 256.0
FEAT_CROP, FEAT_SEED = 8, 5
PREPROC = ((0.9, 1.1, 0.8), (0.05, -0.1, 0.2))          # input affine of the feature net, per repeated channel
G_CHANNELS = {16: (8, 8, 8), 32: (8, 8, 4, 4), 64: (8, 8, 4, 4, 4), 256: (8, 8, 8, 8, 4, 4, 4)}
D_CHANNELS = {32: (8, 8, 4, 4)}
# GUARDED cases: B 2 over three steps puts 10^5 pre-activations of G, D and the feature net in front of a guard of 10^-5 of a layer's
# largest; with biases around zero no seed of 0..63 keeps them all outside it, and a seed that just does depends on the float32 rounding
# of the machine's CPU.  So the conv biases of those cases are calibrated (`Built.calibrate`): channel by channel, layer by layer, the
# pre-activations at w0 are centred at +/- KINK_Z standard deviations of the layer, signs alternating over the channels.  Both slopes of
# every lrelu / relu carry gradient, whole channels on either side, and few pre-activations crowd the kink.  (The engines' own sweeps
# run the natural distributions.)
KINK_Z = 3.0
# la_misc.hip / la_wplus.hip / la_criteria.hip
TAIL_WG, SLOT_UNROLL, RB, NCH, KSPLIT, KSPLIT_MIN_K, COLSUM_ROWS = 256, 8, 8, 8, 16, 16384, 16


def cdiv(a, b):
    return -(-a // b)


def num_ws_of(R):
    return 2 * (int(math.log2(R)) - 1)


def crop_geometry(R):
    """(side, offset) of the pixel criterion's centre crop: CenterCrop(int(sqrt(R^2 / 2))), torchvision's offset"""
    cc = int(math.sqrt(R * R / 2))
    return cc, int(round((R - cc) / 2.0))


class LoopCase:
    """space 'w' | 'w+'; B live samples of max_batch; Mw / Mx / Mf bank rows; crop_pos (x, y) of the perceptual window inside the
    centre crop; rerun: after the traced run, the captured step on the same handle and then B = 1 on it (multi-workgroup tails)."""

    def __init__(self, name, R, w_dim, B, space='w', steps=3, Mw=0, Mx=0, Mf=0, imgc=2, w_latent=0.0, w_pix=0.0, w_disc=0.0, w_lpips=0.0,
                 norm_batch=0, soft=False, alpha=1.0, crop_pos=(0, 0), seed=0, kind='closed', rerun=False, max_batch=None):
        self.name, self.R, self.w_dim, self.B, self.space, self.steps = name, R, w_dim, B, space, steps
        self.Mw, self.Mx, self.Mf, self.imgc = Mw, Mx, Mf, imgc
        self.w_latent, self.w_pix, self.w_disc, self.w_lpips = w_latent, w_pix, w_disc, w_lpips
        self.norm_batch, self.soft, self.alpha, self.crop_pos = norm_batch, soft, alpha, tuple(crop_pos)
        self.seed, self.kind, self.rerun = seed, kind, rerun
        self.max_batch = B if max_batch is None else max_batch
        assert (w_latent > 0) == (Mw > 0) and (w_pix > 0) == (Mx > 0) and (w_lpips > 0) == (Mf > 0) and w_dim % 4 == 0
        assert kind in ('closed', 'scalars', 'guarded') and (kind == 'closed') == (not self.img_crit)
        self._built = {}

    @property
    def wplus(self):
        return self.space == 'w+'

    @property
    def img_crit(self):
        return self.w_pix > 0 or self.w_disc > 0 or self.w_lpips > 0

    @property
    def num_ws(self):
        return num_ws_of(self.R)

    @property
    def rows(self):
        return self.num_ws if self.wplus else 1

    def nb(self, B):
        """the batch size the criteria's means divide by"""
        return self.norm_batch if self.norm_batch > 0 else B

    def window(self):
        """absolute (x, y) of the perceptual window"""
        off = crop_geometry(self.R)[1]
        return off + self.crop_pos[0], off + self.crop_pos[1]

    def build(self, seed=None):
        """networks, banks and w0 (float32) from the case's seed; memoised"""
        seed = self.seed if seed is None else seed
        if seed not in self._built:
            self._built[seed] = Built(self, seed)
        return self._built[seed]

    def runs(self, seed=None):
        """(built, float32 free-running trajectory, float64 free-running trajectory); each a dict with the `pre` of every step"""
        b = self.build(seed)
        return b, simulate(self, b, torch.float32), simulate(self, b, torch.float64)


class Built:
    def __init__(self, case, seed):
        from oracle import feature_net as fnets
        from oracle import sg2_networks as nets
        c = case
        self.seed = seed
        table = dict(zip(sc.block_resolutions(c.R), G_CHANNELS[c.R]))
        self.G = nets.make_generator(img_resolution=c.R, img_channels=c.imgc, seed=seed, noise_strength=0.1, w_dim=c.w_dim, mapping_layers=1,
                                     channels=table)
        g = torch.Generator().manual_seed(1000 * seed + 41)
        with torch.no_grad():
            for n, m in self.G.synthesis.named_modules():
                if isinstance(m, (nets.SynthesisLayer, nets.ToRGBLayer)):
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        assert self.G.num_ws == c.num_ws
        self.sd = self.G.synthesis.state_dict()
        self.noise = [NOISE] * (2 * len(table) - 1)
        self.D = self.fnet = self.ops = None
        if c.w_disc > 0:
            self.D = nets.make_discriminator(img_resolution=c.R, img_channels=c.imgc, seed=seed, channels=dict(zip(sc.block_resolutions(c.R), D_CHANNELS[c.R])))
            with torch.no_grad():
                for n, p in self.D.named_parameters():
                    if n.endswith('bias'):
                        p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if c.w_lpips > 0:
            self.fnet = fnets.TinyFeatureNet(seed=FEAT_SEED, crop=FEAT_CROP)
            self.ops = fnets.tiny_ops(self.fnet)
        self.w0 = torch.randn([c.max_batch, c.rows, c.w_dim], generator=g)
        self.W = torch.randn([c.Mw, c.num_ws, c.w_dim], generator=g) * 0.8 + 0.1 if c.Mw else None
        self.X = torch.rand([c.Mx, c.imgc, c.R, c.R], generator=g) * 2 - 1 if c.Mx else None
        if c.kind == 'guarded':
            self.calibrate(c)
        self.fea = None
        if c.Mf:
            with torch.no_grad():
                self.fea = [self.fnet(torch.rand([c.Mf, 3, FEAT_CROP, FEAT_CROP], generator=g) * 2 - 1).contiguous() for _ in range(c.imgc)]


    def calibrate(self, case):
        """see KINK_Z: one float64 forward pass at w0 per calibrated layer, in execution order"""
        d = torch.float64

        def centre(bias, pre, name):
            a = next(p.a for p in pre if p.name == name)
            mu = a.mean(dim=[0, 2, 3])
            sigma = float((a - mu.reshape(1, -1, 1, 1)).std())
            sign = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(mu.numel())], dtype=d)
            with torch.no_grad():
                bias.add_((sign * KINK_Z * sigma - mu).to(bias.dtype))

        def synth():
            return sc.synth_restate(self.sd, case.R, case.imgc, CLAMP, self.noise, broadcast(case, self.w0.to(d)), d)

        for res in sc.block_resolutions(case.R):
            for ln in (('conv1',) if res == 4 else ('conv0', 'conv1')):
                centre(getattr(getattr(self.G.synthesis, f'b{res}'), ln).bias, synth()['pre'], f'b{res}.{ln}')
        img = synth()['img']
        if self.D is not None:
            P = dict(self.D.named_parameters())
            names = [f'b{r}.{ln}' for r in reversed(sc.block_resolutions(case.R)[1:]) for ln in (('fromrgb',) if r == case.R else ()) + ('conv0', 'conv1')]
            for name in names + ['b4.conv']:
                centre(P[name + '.bias'], ec.disc_restate(self.D.state_dict(), case.R, CLAMP, 4, img, d)['pre'], name)
        if self.fnet is not None:
            for bias, name in ((self.fnet.b1, 'op0.conv'), (self.fnet.b2, 'op3.conv')):
                centre(bias, ec.feat_restate(self.ops, lpips_input(case, img, d).flatten(0, 1), d)['pre'], name)

    def banks(self):
        out = {}
        if self.W is not None:
            out['W'] = self.W
        if self.X is not None:
            out['X'] = self.X
        if self.fea is not None:
            out['fea'] = self.fea
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the criteria (make_run's coefficients; loss = -latent - pix - lpips + disc)

def coefs(case, B):
    nb = float(case.nb(B))
    cc = crop_geometry(case.R)[0]
    return dict(lat=case.w_latent / (case.Mw * nb * case.num_ws * case.w_dim) if case.Mw else 0.0,
                pix=case.w_pix / (case.imgc * case.Mx * nb * cc * cc) if case.Mx else 0.0,
                lp=case.w_lpips / (case.imgc * case.Mf * nb) if case.Mf else 0.0)


def l2_gemm(Y, X):
    """(sum_mn (|Y_m|^2 + |X_n|^2 - 2 <Y_m, X_n>), sum_mn (|Y_m|^2 + |X_n|^2)): l2_loss_vectorized's GEMM form in the dtype of Y, X"""
    YY, XX = (Y * Y).sum(1), (X * X).sum(1)
    top = YY[:, None] + XX[None, :]
    return (top - 2 * (Y @ X.t())).sum(), top.sum()


def broadcast(case, w):
    """ws [B][num_ws][w_dim] of the optimised latent [B][rows][w_dim]"""
    return w if case.wplus else w.repeat(1, case.num_ws, 1)


def slot_sum(case, t):
    """a per-slot quantity [.., num_ws, w_dim] as the gradient of the optimised latent: W sums the slots, W+ keeps them"""
    return t if case.wplus else t.sum(dim=-2, keepdim=True)


def latent_terms(case, b, w, dtype):
    """column 0 and the latent criterion's gradient, from the optimised latent w [B][rows][w_dim]"""
    w = w.detach().to(dtype)
    B = w.shape[0]
    co = coefs(case, B)['lat']
    W = b.W.to(dtype)
    s, top = l2_gemm(W.flatten(1), broadcast(case, w).flatten(1))
    lat2 = -2.0 * co
    if case.wplus:
        dw = lat2 * (case.Mw * w - W.sum(0))
        big = abs(lat2) * case.Mw * float(w.abs().max())
    else:
        dw = lat2 * (case.num_ws * case.Mw * w - slot_sum(case, W.sum(0)))
        big = abs(lat2) * case.num_ws * case.Mw * float(w.abs().max())
    return dict(loss=co * s, top=co * float(top), dw=dw, big=big)


def pix_bank(case, b, dtype):
    """the centre-cropped image bank [Mx][imgc][cc][cc]"""
    cc, off = crop_geometry(case.R)
    return b.X.to(dtype)[:, :, off:off + cc, off:off + cc]


def lpips_input(case, img, dtype):
    """[imgc][B][3][S][S]: the window of every modality, repeated to 3 channels, through the preproc affine"""
    x, y = case.window()
    S = FEAT_CROP
    win = img[:, :, y:y + S, x:x + S].permute(1, 0, 2, 3)
    scale, shift = (torch.tensor(v, dtype=torch.float32).to(dtype).reshape(1, 1, 3, 1, 1) for v in PREPROC)
    return win[:, :, None] * scale + shift


def image_terms(case, b, img, dtype, grad=False):
    """columns 1..3 from an image [B][imgc][R][R], the largest term of each, and with `grad` dL/d(image) and the pre-activations of
    the criterion networks"""
    img = img.detach().to(dtype)
    B = img.shape[0]
    co = coefs(case, B)
    cc, off = crop_geometry(case.R)
    loss, top, pre = [img.new_zeros([]) for _ in range(4)], [0.0] * 4, []
    g_img = torch.zeros_like(img) if grad else None
    if case.w_pix > 0:
        xc, Xc = img[:, :, off:off + cc, off:off + cc], pix_bank(case, b, dtype)
        for c in range(case.imgc):
            s, t = l2_gemm(Xc[:, c].flatten(1), xc[:, c].flatten(1))
            loss[1] = loss[1] + co['pix'] * s
            top[1] += co['pix'] * float(t)
        if grad:
            g_img[:, :, off:off + cc, off:off + cc] = -2.0 * co['pix'] * (case.Mx * xc - Xc.sum(0))
    if case.w_disc > 0:
        args = (b.D.state_dict(), case.R, CLAMP, 4, img, dtype)
        logits = ec.disc_restate(*args)['logits']
        loss[2] = F.softplus(-logits).sum() / case.nb(B) * case.w_disc
        # (the scalar, or one float32 rounding of every logit carried through softplus' slope if that is larger)
        top[2] = max(float(loss[2]), float((torch.sigmoid(-logits) * logits.abs()).sum()) / case.nb(B) * case.w_disc)
        if grad:
            r = ec.disc_restate(*args, dlogits=-torch.sigmoid(-logits) * (case.w_disc / case.nb(B)))
            g_img = g_img + r['gx']
            pre += r['pre']
    if case.w_lpips > 0:
        xin = lpips_input(case, img, dtype)
        f = ec.feat_restate(b.ops, xin.flatten(0, 1), dtype)
        feat = f['feat'].reshape(case.imgc, B, -1)
        gfeat = torch.zeros_like(feat)
        for c in range(case.imgc):
            bank = b.fea[c].to(dtype)
            s, t = l2_gemm(bank, feat[c])
            loss[3] = loss[3] + co['lp'] * s
            top[3] += co['lp'] * float(t)
            gfeat[c] = -2.0 * co['lp'] * (case.Mf * feat[c] - bank.sum(0))
        if grad:
            r = ec.feat_restate(b.ops, xin.flatten(0, 1), dtype, gfeat.flatten(0, 1))
            x, y = case.window()
            scale = torch.tensor(PREPROC[0], dtype=torch.float32).to(dtype).reshape(1, 1, 3, 1, 1)
            gwin = (r['gx'].reshape(case.imgc, B, 3, FEAT_CROP, FEAT_CROP) * scale).sum(2).permute(1, 0, 2, 3)
            g_img[:, :, y:y + FEAT_CROP, x:x + FEAT_CROP] += gwin
            pre += r['pre']
    return dict(loss=loss, top=top, g_img=g_img, pre=pre)


def step_restate(case, w_prev, dtype, built=None):
    """One step from the optimised latent w_prev [B][rows][w_dim], every operation in `dtype` -> dict(losses [4], top [4] (largest term of
    each scalar), dw (the shape of w_prev), big (largest term of dw), img, pre)."""
    b = case.build() if built is None else built
    w = w_prev.detach().to(dtype)
    losses, top, pre, img = [w.new_zeros([]) for _ in range(4)], [0.0] * 4, [], None
    dw, big = torch.zeros_like(w), 0.0
    if case.img_crit:
        syn = (b.sd, case.R, case.imgc, CLAMP, b.noise, broadcast(case, w), dtype)
        fwd = sc.synth_restate(*syn)
        img = fwd['img']
        t = image_terms(case, b, img, dtype, grad=True)
        losses, top = t['loss'], t['top']
        dw = slot_sum(case, sc.synth_restate(*syn, g_img=t['g_img'])['dws'])
        pre = fwd['pre'] + t['pre']
    if case.w_latent > 0:
        lt = latent_terms(case, b, w, dtype)
        losses[0], top[0], big = lt['loss'], lt['top'], lt['big']
        dw = dw + lt['dw']
    big = max(big, float(dw.abs().max())) if case.img_crit else big
    return dict(losses=torch.stack([v.to(dtype) for v in losses]), top=top, dw=dw, big=big, img=img, pre=pre)


def adam_restate(w_prev, grads, dtype, lr=LR):
    """w_k from w_{k-1} and the gradients of steps 1..k (moments rebuilt from them), oracle.latent_aug_ref.AdamState's arithmetic in `dtype`"""
    from oracle.latent_aug_ref import AdamState
    p = w_prev.detach().to(dtype)
    st = AdamState(p, lr, BETA1, BETA2, ADAM_EPS)
    out = None
    for g in grads:
        out = st.step(p, g.detach().to(dtype))
    return out


def gate_restate(case, w_last, w0, dtype):
    """w_aug [B][num_ws][w_dim]: hard w_last, soft alpha w_last + (1 - alpha) w0, broadcast to the slots in W"""
    a, z = w_last.detach().to(dtype), w0.detach().to(dtype)
    return broadcast(case, case.alpha * a + (1 - case.alpha) * z if case.soft else a)


def simulate(case, b, dtype, B=None):
    """a free-running run of the restatement in `dtype`, in the form of a traced run: dict(w0, w [steps], grad [steps], img [steps] or None,
    losses [steps][4], w_aug, pre)"""
    w0 = b.w0[:case.B if B is None else B]
    w, ws, gs, imgs, Ls, pre = w0.to(dtype), [], [], [], [], []
    for k in range(case.steps):
        r = step_restate(case, w, dtype, b)
        gs.append(r['dw'])
        w = adam_restate(w, gs, dtype)
        ws.append(w)
        imgs.append(r['img'])
        Ls.append(r['losses'])
        pre += r['pre']
    return dict(w0=w0, w=ws, grad=gs, img=imgs if case.img_crit else None, losses=Ls, w_aug=gate_restate(case, w, w0, dtype), pre=pre)


# ---------------------------------------------------------------------------------------------------------------------------------
# the judge

class Verdict:
    def __init__(self, say=print):
        self.bad, self.ratios, self.say = [], {}, say

    def check(self, group, name, got, r32, r64, k, top):
        got, r32, r64 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r32, r64))
        assert got.shape == r64.shape, f'{name}: shape {tuple(got.shape)} != {tuple(r64.shape)}'
        err, err32 = worst(got, r64), worst(r32, r64)
        bud = k * err32 + EPS32 * top
        ratio = err / bud if bud > 0 else (0.0 if err == 0 else float('inf'))
        self.say(f'{name}: err {err:.3e} / budget {bud:.3e} = ratio {ratio:.3f} (f32-CPU err {err32:.3e}, k {k}, largest term {top:.3e})')
        self.ratios[group] = max(self.ratios.get(group, 0.0), ratio)
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f'{name}: not finite')
        elif not err <= bud:
            self.bad.append(f'{name}: err {err:.3e} > budget {bud:.3e}')

    def exact_zero(self, name, got):
        if float(torch.as_tensor(got).abs().max()) != 0.0:
            self.bad.append(f'{name}: an inactive criterion wrote {float(torch.as_tensor(got).abs().max()):.3e}')


def judge(case, b, run, mode='f32', say=print, verdict=None):
    """Every element of every step of a traced run (`simulate`'s form, CPU tensors) against the teacher-forced float64 restatement.
    Returns the Verdict: .bad (failure texts), .ratios (largest err / budget per group)."""
    v = Verdict(say) if verdict is None else verdict
    ke = K_ENGINE[mode]
    w0 = run['w0']
    B = w0.shape[0]
    tag = f'loop {case.name} B{B} [{mode}]'
    cols = []
    for k in range(1, case.steps + 1):
        w_prev = w0 if k == 1 else run['w'][k - 2]
        L = run['losses'][k - 1]
        if case.kind == 'scalars':
            t64, t32 = (image_terms(case, b, run['img'][k - 1], d) for d in (torch.float64, torch.float32))
            l64, l32, top = t64['loss'], t32['loss'], t64['top']
            if case.w_latent > 0:
                a64, a32 = (latent_terms(case, b, w_prev, d) for d in (torch.float64, torch.float32))
                l64[0], l32[0], top[0] = a64['loss'], a32['loss'], a64['top']
        else:
            r64, r32 = (step_restate(case, w_prev, d, b) for d in (torch.float64, torch.float32))
            if case.kind == 'guarded':
                g, m, where = guard_of(r32['pre'], r64['pre'])
                say(f'{tag} step {k}: guard g {g:.3e}, smallest margin {m:.3e} ({where})')
                if m < g:
                    v.bad.append(f'{tag} step {k}: margin {m:.3e} ({where}) below the guard {g:.3e}')
            v.check('dw closed form' if case.kind == 'closed' else f'dw through the engines {mode}', f'{tag} step {k} dw', run['grad'][k - 1],
                    r32['dw'], r64['dw'], K_LOOP if case.kind == 'closed' else ke, r64['big'])
            l64, l32, top = list(r64['losses']), list(r32['losses']), list(r64['top'])
            if case.img_crit:          # columns 1..3 from the TRACED image
                t64, t32 = (image_terms(case, b, run['img'][k - 1], d) for d in (torch.float64, torch.float32))
                l64[1:], l32[1:], top[1:] = t64['loss'][1:], t32['loss'][1:], t64['top'][1:]
        cols.append((L, torch.stack([t.double() for t in l32]), torch.stack([t.double() for t in l64]), top))
        a64, a32 = (adam_restate(w_prev, run['grad'][:k], d) for d in (torch.float64, torch.float32))
        v.check('Adam', f'{tag} step {k} Adam', run['w'][k - 1], a32, a64, K_LOOP, float(w_prev.abs().max()))
    # the loss scalars: each column over all steps as one vector (a single scalar's float32 error is one draw, not a scale)
    for col, (wgt, name, kk) in enumerate(((case.w_latent, 'latent', K_LOOP), (case.w_pix, 'pix', K_LOOP), (case.w_disc, 'disc', ke),
                                           (case.w_lpips, 'lpips', ke))):
        if not cols:
            break
        got, c32, c64 = (torch.stack([torch.as_tensor(t[i][col]).double() for t in cols]) for i in range(3))
        if wgt > 0:
            v.check(f'loss {name}' + (f' {mode}' if col >= 2 else ''), f'{tag} loss_{name} of steps 1..{case.steps}', got, c32, c64, kk,
                    max(t[3][col] for t in cols))
        else:
            v.exact_zero(f'{tag} loss_{name}', got)
    w_last = run['w'][-1] if case.steps else w0
    g64, g32 = (gate_restate(case, w_last, w0, d) for d in (torch.float64, torch.float32))
    v.check('gate', f'{tag} gate', run['w_aug'], g32, g64, K_LOOP, max(float(w_last.abs().max()), float(w0.abs().max())))
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# the table

LAT = dict(w_latent=0.5)
TAIL_CASES = [
    # one partial workgroup; num_ws 6: remainder slots only
    LoopCase('W-R16-wd24-B1', 16, 24, 1, Mw=1, steps=1, **LAT),
    LoopCase('W+-R16-wd24-B1', 16, 24, 1, 'w+', Mw=5, steps=2, **LAT),
    # exactly 256 elements / float4; num_ws 8: one full group of slots
    LoopCase('W-R32-wd64-B4', 32, 64, 4, Mw=4, steps=2, norm_batch=8, **LAT),
    LoopCase('W+-R32-wd32-B4', 32, 32, 4, 'w+', Mw=17, steps=1, soft=True, alpha=0.7, **LAT),
    # two workgroups, the last one partial
    LoopCase('W-R16-wd88-B3', 16, 88, 3, Mw=17, steps=5, soft=True, alpha=0.7, rerun=True, **LAT),
    LoopCase('W+-R64-wd32-B4', 64, 32, 4, 'w+', Mw=29, steps=5, norm_batch=8, rerun=True, **LAT),
    # num_ws 10: a full group of slots and a remainder
    LoopCase('W-R64-wd32-B2', 64, 32, 2, Mw=29, steps=2, **LAT),
    # B 9: two passes of query rows
    LoopCase('W-R16-wd24-B9', 16, 24, 9, Mw=5, steps=1, **LAT),
    # no step at all: the gate of w0
    LoopCase('W-R16-wd24-steps0', 16, 24, 2, Mw=4, steps=0, soft=True, alpha=0.7, **LAT),
    LoopCase('W+-R16-wd24-steps0', 16, 24, 2, 'w+', Mw=1, steps=0, **LAT),
]
SCALAR_CASES = [
    LoopCase('pix-R16-imgc1-Mx1', 16, 24, 2, Mx=1, imgc=1, steps=1, w_pix=2.0, kind='scalars'),
    LoopCase('pix-R16-imgc3-Mx9-B9', 16, 24, 9, Mx=9, imgc=3, steps=1, w_pix=2.0, w_latent=0.3, Mw=4, kind='scalars'),
    LoopCase('pix-R32-imgc2-Mx9', 32, 32, 2, Mx=9, imgc=2, steps=2, w_pix=2.0, norm_batch=4, kind='scalars'),
    LoopCase('pix-R256-imgc3-Mx3-B1', 256, 32, 1, Mx=3, imgc=3, steps=2, w_pix=2.0, kind='scalars'),
]
ALL_MIX = dict(w_latent=0.3, Mw=5, w_pix=1.0, Mx=3, w_disc=0.5, w_lpips=2.0, Mf=5)
# (the seeds are the first of 0..63 that meet the guard at every step: `python tests/loop_cases.py` prints the search)
GUARDED_CASES = [
    LoopCase('pix-R32', 32, 32, 2, Mx=3, w_pix=2.0, kind='guarded', seed=0),
    LoopCase('disc-R32', 32, 32, 2, w_disc=1.0, kind='guarded', seed=1),
    LoopCase('lpips-R32', 32, 32, 2, w_lpips=3.0, Mf=5, crop_pos=(9, 4), kind='guarded', seed=0),
    LoopCase('all-R32', 32, 32, 2, crop_pos=(3, 11), kind='guarded', seed=0, **ALL_MIX),
    LoopCase('all-W+-R32', 32, 32, 2, 'w+', crop_pos=(3, 11), soft=True, alpha=0.7, kind='guarded', seed=0, **ALL_MIX),
    LoopCase('pix-R16', 16, 24, 2, Mx=9, imgc=3, w_pix=2.0, w_latent=0.3, Mw=4, kind='guarded', seed=0),
]
CASES = TAIL_CASES + SCALAR_CASES + GUARDED_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def first_seed(case):
    """first seed of 0..63 whose float32 and float64 free-running trajectories meet engine_cases' guard over every step, or None"""
    for s in range(ec.MAX_SEEDS):
        b = case.build(s)
        st = {d: dict(w=b.w0[:case.B].to(d), grads=[], pre=[]) for d in (torch.float32, torch.float64)}
        ok = True
        for _ in range(case.steps):          # (both trajectories step by step: g only grows and the margin only shrinks, so a miss is final)
            for d, t in st.items():
                r = step_restate(case, t['w'], d, b)
                t['grads'].append(r['dw'])
                t['w'] = adam_restate(t['w'], t['grads'], d)
                t['pre'] += r['pre']
            g, m, _ = guard_of(st[torch.float32]['pre'], st[torch.float64]['pre'])
            ok = m >= g
            if not ok:
                break
        if s != case.seed:
            case._built.pop(s, None)
        if ok:
            return s
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# reach: which launch form a case takes (la_step_tail / la_wplus_step_tail, la_bank_dot, la_bank_colsum)

def dot_plan(K, ldx, xmod, m, n, aligned=True):
    vec = K % 4 == 0 and ldx % 4 == 0 and xmod % 4 == 0 and aligned
    return dict(K=K, ldx=ldx, xmod=xmod, vec=vec, ksplit=KSPLIT if (K > KSPLIT_MIN_K and cdiv(m, RB) * 4 < 512) else 4, row_blocks=cdiv(m, RB),
                passes=cdiv(n, NCH))


def colsum_plan(m):
    """per wave (rows w, w + 4, ..): (16-row groups of four loads in flight, remainder rows)"""
    waves = []
    for w in range(4):
        r, groups = w, 0
        while r + 12 < m:
            groups, r = groups + 1, r + COLSUM_ROWS
        waves.append((groups, len(range(r, m, 4))))
    return dict(rows=m, groups=max(g for g, _ in waves), waves=waves)


def reach(case, B=None):
    B = case.B if B is None else B
    nws, wd = case.num_ws, case.w_dim
    cc = crop_geometry(case.R)[0]
    total = B * nws * wd // 4 if case.wplus else B * wd
    out = dict(tail=dict(kernel='wplus' if case.wplus else 'w', workgroups=cdiv(total, TAIL_WG), last_partial=total % TAIL_WG != 0),
               slots=dict(groups=0 if case.wplus else nws // SLOT_UNROLL, remainder=0 if case.wplus else nws % SLOT_UNROLL), dots={}, colsums={})
    if case.Mw:
        K = nws * wd
        out['dots']['latent'] = [dot_plan(K, K if case.wplus else wd, 0 if case.wplus else wd, case.Mw, B)]
        out['colsums']['latent'] = colsum_plan(case.Mw)
    if case.Mx:
        # channel c: bank rows at c * Mx * cc^2 floats, query rows at c * cc^2 floats of a row of imgc * cc^2 (16-byte aligned workspaces)
        out['dots']['pix'] = [dot_plan(cc * cc, case.imgc * cc * cc, 0, case.Mx, B, aligned=(c * case.Mx * cc * cc) % 4 == 0 and (c * cc * cc) % 4 == 0)
                              for c in range(case.imgc)]
        out['colsums']['pix'] = colsum_plan(case.Mx)
    if case.Mf:
        Fn = 8 * FEAT_CROP ** 2 + 16 * (FEAT_CROP // 2) ** 2
        out['dots']['lpips'] = [dot_plan(Fn, Fn, 0, case.Mf, B, aligned=(c * case.Mf * Fn) % 4 == 0 and (c * B * Fn) % 4 == 0) for c in range(case.imgc)]
        out['colsums']['lpips'] = colsum_plan(case.Mf)
    return out


def _tail(kernel, wgs, partial):
    return lambda c, r: r['tail'] == dict(kernel=kernel, workgroups=wgs, last_partial=partial) and c.steps > 0


def _dot(which, **want):
    return lambda c, r: any(all(p[k] == v for k, v in want.items()) for p in r['dots'].get(which, []))


def _colsum(pred):
    return lambda c, r: any(pred(p) for p in r['colsums'].values())


REACH = dict(
    [(f'{n} tail, one partial workgroup', _tail(k, 1, True)) for n, k in (('W', 'w'), ('W+', 'wplus'))] +
    [(f'{n} tail, exactly one full workgroup', _tail(k, 1, False)) for n, k in (('W', 'w'), ('W+', 'wplus'))] +
    [(f'{n} tail, two workgroups, the last partial (la_step_ticket counts)', _tail(k, 2, True)) for n, k in (('W', 'w'), ('W+', 'wplus'))] +
    [('the captured step and then B = 1 on the same handle (ticket, counter, cached column sums)', lambda c, r: c.rerun and r['tail']['workgroups'] > 1 and c.steps >= 2),
     ('slot sum: remainder only (num_ws 6)', lambda c, r: r['slots'] == dict(groups=0, remainder=6) and c.steps > 0),
     ('slot sum: one group of eight, no remainder (num_ws 8)', lambda c, r: r['slots'] == dict(groups=1, remainder=0) and c.steps > 0),
     ('slot sum: a group of eight and a remainder (num_ws 10)', lambda c, r: r['slots'] == dict(groups=1, remainder=2) and c.steps > 0),
     ('slot sum of a synthesis gradient (dws not null)', lambda c, r: c.kind == 'guarded' and not c.wplus),
     ('W+ tail with a synthesis gradient', lambda c, r: c.kind == 'guarded' and c.wplus)] +
    [(f'column sums of {m} bank row{"s" if m > 1 else ""}', _colsum(lambda p, m=m: p['rows'] == m)) for m in (1, 4, 5, 17, 29)] +
    [('column sums: no 16-row group', _colsum(lambda p: p['groups'] == 0)),
     ('column sums: a 16-row group and a remainder in one wave', _colsum(lambda p: any(g == 1 and rem >= 1 for g, rem in p['waves']))),
     ('column sums: two 16-row groups in one wave', _colsum(lambda p: p['groups'] == 2))] +
    [(f'{s} steps', lambda c, r, s=s: c.steps == s) for s in (0, 1, 2, 5)] +
    [('norm_batch unset', lambda c, r: c.norm_batch == 0),
     ('norm_batch = 2 B', lambda c, r: c.norm_batch == 2 * c.B),
     ('soft gate, alpha 0.7, W', lambda c, r: c.soft and c.alpha == 0.7 and not c.wplus),
     ('soft gate, alpha 0.7, W+', lambda c, r: c.soft and c.alpha == 0.7 and c.wplus),
     ('hard gate', lambda c, r: not c.soft),
     ('latent dot, W: ldx = w_dim, xmod = w_dim', lambda c, r: not c.wplus and _dot('latent', xmod=c.w_dim, ldx=c.w_dim, vec=True)(c, r)),
     ('latent dot, W+: ldx = num_ws w_dim', lambda c, r: c.wplus and _dot('latent', xmod=0, ldx=c.num_ws * c.w_dim, vec=True)(c, r)),
     ('latent dot: two passes of query rows (B 9)', _dot('latent', passes=2)),
     ('pixel dot: scalar form (cc^2 = 121)', _dot('pix', K=121, vec=False)),
     ('pixel dot: scalar form at an unaligned channel base', lambda c, r: any(not p['vec'] and k > 0 for k, p in enumerate(r['dots'].get('pix', [])) if p['K'] == 121)),
     ('pixel dot: float4 form (cc^2 = 484)', _dot('pix', K=484, vec=True)),
     ('pixel dot: 16 K slices (cc^2 = 32761)', _dot('pix', K=32761, ksplit=16)),
     ('pixel dot: two row blocks (Mx 9)', _dot('pix', row_blocks=2)),
     ('pixel dot: two passes of query rows (B 9)', _dot('pix', passes=2)),
     ('pixel criterion accumulated over 2 channels and more', lambda c, r: c.Mx > 0 and c.imgc >= 2)] +
    [(f'pixel criterion, imgc {k}', lambda c, r, k=k: c.Mx > 0 and c.imgc == k) for k in (1, 2, 3)] +
    [('Mx 1', lambda c, r: c.Mx == 1),
     ('discriminator column', lambda c, r: c.w_disc > 0),
     ('perceptual column, window at x != y, both non-zero', lambda c, r: c.w_lpips > 0 and 0 < c.crop_pos[0] != c.crop_pos[1] > 0),
     ('every criterion at once', lambda c, r: min(c.w_latent, c.w_pix, c.w_disc, c.w_lpips) > 0),
     ('gradient through the engines in f32, bf16x3 and f16x2', lambda c, r: c.kind == 'guarded')])


def reach_table():
    """{item: [case names]} over CASES"""
    return {name: [c.name for c in CASES if pred(c, reach(c))] for name, pred in REACH.items()}


def reach_text():
    """the table as it stands in the docstring of test_hip_loop_shapes.py"""
    return '\n'.join(f'    {name}: ' + (', '.join(rows) if rows else 'NO CASE') for name, rows in reach_table().items())


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if '--table' in sys.argv:
        print(reach_text())
    else:
        for case in GUARDED_CASES:
            print(f'{case.name}: recorded seed {case.seed}, first seed that meets the guard {first_seed(case)}', flush=True)
