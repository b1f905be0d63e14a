"""Case tables, seeded inputs and float64 / float32 restatements of the two criterion networks: the perceptual feature engine
(la_feat.hip, FeatureEngine) and the discriminator engine (la_disc.hip, DiscriminatorEngine).  Shared by test_engine_cases_cpu.py (which
proves, without a GPU, that the restatements equal float64 autograd of the oracle and that every case reaches what it claims) and by
test_hip_engine_shapes.py.  No GPU and no ctypes here; every input is synthetic and seeded.

The restatements are written in plain torch and expose every pre-activation: `feat_restate` (conv 3x3 pad 1 + bias, ReLU, 2x2 max / avg
pool with the gradient of a tie going to the FIRST maximum in scan order, the tap formula of oracle/feature_net._lpips_pack) and
`disc_restate` (the forward of oracle/sg2_networks.Discriminator: FromRGB, skip FIR-down + 1x1, conv0, conv1's pad-2 FIR + stride 2, the
gains sqrt2 / sqrt(1/2), the clamp, MinibatchStd with sqrt(var + 1e-8), the FC tail).  Both run in float64 (the answer) and in float32
(the budget: the code under test never sets one).

Three kinds of case.
EXACT    small-integer inputs: the pool cases.  The engine's result must equal, bit for bit, what exact routing gives.
GUARDED  float inputs whose float64 run has no pre-activation within g x max|a| of its layer of a kink (0, or the clamp), with
         g = 16 x the largest relative pre-activation error (over max|a| of the layer) of the float32 run against float64.  The seed is
         the first of 0..63 for which that holds (`search_seed`), recorded in the table.  Judged element by element:
             worst |hip - f64| <= k x worst |f32 - f64| + 2^-23 x max|f64|
BULK     too many pre-activations for a guard (R = 128): relative L2 against float64 <= 1.5 x that of the float32 run + 1e-6.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
TWO24 = float(2 ** 24)
GUARD_FACTOR = 16.0
MAX_SEEDS = 64
SQRT2, RSQRT2 = math.sqrt(2.0), math.sqrt(0.5)


class Pre:
    """One layer's pre-activations: `a` (before the activation; kink at 0) and, for a clamped layer, `v` = act(a) * gain (kink at
    |v| = clamp)."""

    def __init__(self, name, a, v=None, clamp=None):
        self.name, self.a, self.v, self.clamp = name, a.detach(), None if v is None else v.detach(), clamp

    def margin(self):
        """smallest distance of a pre-activation to a kink, relative to the layer's largest"""
        m = float(self.a.abs().min() / self.a.abs().max())
        if self.clamp is not None:
            m = min(m, float((self.v.abs() - self.clamp).abs().min() / self.v.abs().max()))
        return m

    def clamped_fraction(self):
        return float((self.v.abs() > self.clamp).double().mean())


def rel_err(p32, p64):
    """largest pre-activation error of the float32 run over max|a| of the layer (the clamped value counts too)"""
    e = float((p32.a.double() - p64.a).abs().max() / p64.a.abs().max())
    if p64.clamp is not None:
        e = max(e, float((p32.v.double() - p64.v).abs().max() / p64.v.abs().max()))
    return e


def guard_of(pre32, pre64):
    """(g, smallest margin, name of the layer that has it)"""
    if not pre64:
        return 0.0, float('inf'), '-'
    g = GUARD_FACTOR * max(rel_err(a, b) for a, b in zip(pre32, pre64))
    m, name = min((p.margin(), p.name) for p in pre64)
    return g, m, name


def worst(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def budget(k, ref32, ref64):
    """k x (worst float32-restatement error) + one float32 rounding of the largest value"""
    return k * worst(ref32, ref64) + EPS32 * float(torch.as_tensor(ref64).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# feature net

def pool_first_max(x):
    """2x2 max-pool whose gradient goes to the FIRST maximum in scan order (a, b / c, d), written out"""
    v = [x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]]
    m = torch.maximum(torch.maximum(v[0], v[1]), torch.maximum(v[2], v[3])).detach()
    taken = torch.zeros_like(m, dtype=torch.bool)
    y = 0
    for q in v:
        sel = (q.detach() == m) & ~taken
        taken = taken | sel
        y = y + torch.where(sel, q, torch.zeros_like(q))
    return y


def pool_avg(x):
    return 0.25 * ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]))


def tap_pack(f, lin):
    """f * rsqrt(sum_c f^2 + 1e-10) * sqrt(lin[c]) / sqrt(H * W), flattened"""
    r = torch.rsqrt((f * f).sum(dim=1, keepdim=True) + 1e-10)
    return (f * r * lin.sqrt().reshape(1, -1, 1, 1) / math.sqrt(f.shape[2] * f.shape[3])).flatten(1)


def feat_restate(ops, x, dtype, gfeat=None):
    """ops: ('conv', w, b) | ('tap', lin) | ('maxpool',) | ('avgpool',) with float32 tensors.  Returns dict(feat, gx, pre)."""
    x = x.detach().to(dtype).requires_grad_(True)
    cur, outs, pre = x, [], []
    for i, op in enumerate(ops):
        if op[0] == 'conv':
            a = F.conv2d(cur, op[1].to(dtype), op[2].to(dtype), padding=1)
            pre.append(Pre(f'op{i}.conv', a))
            cur = torch.where(a > 0, a, torch.zeros_like(a))
        elif op[0] == 'tap':
            outs.append(tap_pack(cur, op[1].to(dtype)))
        elif op[0] == 'maxpool':
            cur = pool_first_max(cur)
        elif op[0] == 'avgpool':
            cur = pool_avg(cur)
        else:
            raise ValueError(op[0])
    feat = torch.cat(outs, dim=1)
    gx = None
    if gfeat is not None:
        (gx,) = torch.autograd.grad(feat, [x], gfeat.to(dtype))
    return dict(feat=feat.detach(), gx=gx, pre=pre)


def feat_oracle(ops, x, gfeat):
    """the same network from stock torch ops and oracle/feature_net._lpips_pack, float64 autograd: what `feat_restate` must equal"""
    from oracle.feature_net import _lpips_pack
    x = x.detach().double().requires_grad_(True)
    cur, feats, lins = x, [], []
    for op in ops:
        if op[0] == 'conv':
            cur = F.relu(F.conv2d(cur, op[1].double(), op[2].double(), padding=1))
        elif op[0] == 'tap':
            feats.append(cur)
            lins.append(op[1].double())
        else:
            cur = F.max_pool2d(cur, 2) if op[0] == 'maxpool' else F.avg_pool2d(cur, 2)
    feat = _lpips_pack(feats, lins)
    (gx,) = torch.autograd.grad(feat, [x], gfeat.double())
    return feat.detach(), gx


class FeatCase:
    """kinds: list of op kinds; widths: cout of every conv in order.  N live samples of max_batch."""

    def __init__(self, name, kinds, in_ch, res, N, max_batch=None, widths=(), seed=0, scale=1.0, kind='guarded'):
        self.name, self.kinds, self.in_ch, self.res, self.N = name, kinds.split(','), in_ch, res, N
        self.max_batch = N if max_batch is None else max_batch
        self.widths, self.seed, self.scale, self.kind = list(widths), seed, scale, kind

    def build(self, seed=None):
        """(ops, x [N][in_ch][res][res], gfeat) float32 from the case's seed"""
        g = torch.Generator().manual_seed(1000 * (self.seed if seed is None else seed) + 17)
        ops, c, r, F_, wi = [], self.in_ch, self.res, 0, 0
        for k in self.kinds:
            if k == 'conv':
                co = self.widths[wi]
                wi += 1
                w = torch.randn([co, c, 3, 3], generator=g) * (2.0 / (c * 9)) ** 0.5
                b = torch.randn([co], generator=g) * 0.2 + 0.1          # a non-zero mean keeps fewer channels dead
                ops.append(('conv', w, b))
                c = co
            elif k == 'tap':
                ops.append(('tap', torch.rand([c], generator=g) + 0.1))
                F_ += c * r * r
            else:
                ops.append((k,))
                r //= 2
        x = (torch.randn([self.N, self.in_ch, self.res, self.res], generator=g) + 0.2) * self.scale
        gfeat = torch.randn([self.N, F_], generator=g)
        return ops, x, gfeat

    def runs(self, seed=None):
        ops, x, gfeat = self.build(seed)
        return ops, x, gfeat, feat_restate(ops, x, torch.float32, gfeat), feat_restate(ops, x, torch.float64, gfeat)


W16 = (16, 16, 16, 16)
TAP_ONLY = ([(C, 8) for C in (1, 3, 5, 28, 29, 32, 33, 36)] + [(C, 2) for C in (3, 64, 512, 513)] + [(8, r) for r in (3, 6, 10, 14)])

# (the seeds are the first of 0..63 that meet the guard: `python tests/engine_cases.py` prints the search)
FEAT_CASES = [FeatCase(f'tap-only-C{C}-res{r}', 'tap', C, r, 3, 4) for C, r in TAP_ONLY] + [
    FeatCase('cin4-in4-N1', 'conv,tap', 4, 8, 1, 8, (16,), seed=0),
    FeatCase('cin4-in4-N5', 'conv,tap', 4, 8, 5, 8, (16,), seed=0),
    FeatCase('cin4-in8-N1', 'conv,tap', 8, 8, 1, 8, (12,), seed=0),
    FeatCase('cin4-in8-N5', 'conv,tap', 8, 8, 5, 8, (12,), seed=0),
    FeatCase('cin-odd-in1', 'conv,tap', 1, 6, 3, 3, (8,), seed=0),
    FeatCase('cin-odd-in2', 'conv,tap', 2, 6, 3, 3, (8,), seed=0),
    FeatCase('cin-odd-in3', 'conv,tap', 3, 6, 3, 3, (8,), seed=0),
    FeatCase('conv-conv', 'conv,conv,tap', 3, 12, 3, 4, (8, 12), seed=0),
    FeatCase('conv-conv-conv-pool', 'conv,conv,conv,tap,maxpool,conv,tap', 3, 12, 3, 4, (8, 8, 12, 16), seed=1),
    FeatCase('tap-between', 'conv,tap,conv,tap', 3, 10, 2, 2, (8, 12), seed=0),
    FeatCase('tap-behind-maxpool', 'conv,maxpool,tap', 3, 12, 3, 4, (8,), seed=0),
    FeatCase('tap-behind-avgpool', 'conv,avgpool,tap,conv,tap', 3, 12, 3, 4, (8, 12), seed=0),
    FeatCase('odd-res-20', 'conv,tap,maxpool,conv,tap,maxpool,conv,tap', 3, 20, 2, 2, (8, 12, 16), seed=0),
    FeatCase('odd-res-28', 'conv,tap,maxpool,conv,tap,maxpool,conv,tap', 3, 28, 2, 2, (8, 12, 16), seed=0),
]
FEAT_BY_NAME = {c.name: c for c in FEAT_CASES}
FEAT_SHRINK = FeatCase('feat-shrinking-batch', 'conv,conv,tap', 3, 12, 3, 8, (8, 12), seed=0)          # N = 8 x 2^8 first, then these 3
FEAT_SHRINK_BIG = 2.0 ** 8

# refusals: (name, kinds, in_ch, res, widths, where it must be refused, fragment of the message)
FEAT_REFUSALS = [
    ('ends-in-conv', 'conv,tap,conv', 3, 8, (8, 8), 'backward', 'must end with a tap'),
    ('ends-in-pool', 'conv,tap,maxpool', 3, 8, (8,), 'backward', 'must end with a tap'),
    ('odd-res-into-pool', 'conv,maxpool,tap', 3, 7, (8,), 'create', 'even resolution'),
    ('cout-not-multiple-of-4', 'conv,tap', 3, 8, (6,), 'create', 'multiple of 4'),
    ('second-conv-cin3', 'maxpool,conv,tap', 3, 8, (8,), 'create', 'only the first conv may have cin % 4 != 0'),
    ('no-tap', 'conv,maxpool', 3, 8, (8,), 'create', 'no tap'),
]

TAP_ZERO = dict(C=8, res=4, N=2, zero_pixels=[(0, 0, 0), (0, 3, 3), (1, 2, 1)], zero_lin=[2, 5], seed=3)


def tap_zero_inputs():
    """(ops, x, gfeat): `tap` on C = 8 at 4x4 with planted all-zero channel vectors and two zero lin entries"""
    t = TAP_ZERO
    g = torch.Generator().manual_seed(t['seed'])
    x = torch.randn([t['N'], t['C'], t['res'], t['res']], generator=g) + 0.2
    for n, yy, xx in t['zero_pixels']:
        x[n, :, yy, xx] = 0.0
    lin = torch.rand([t['C']], generator=g) + 0.1
    lin[t['zero_lin']] = 0.0
    gfeat = torch.randn([t['N'], t['C'] * t['res'] ** 2], generator=g)
    return [('tap', lin)], x, gfeat


POOL_EXACT = [(pool, res) for pool in ('maxpool', 'avgpool') for res in (4, 6)]
POOL_C, POOL_N = 4, 2
TIE_PATTERNS = {'first=second': (0, 1), 'first=third': (0, 2), 'all-four': (0, 1, 2, 3)}


def pool_exact_inputs(res, C=POOL_C, seed=0):
    """x [2][C][res][res]: integers in -6..6 (multiples of 4 would make the average pool's quarter exact anyway: every integer below
    2^22 does), with the three tie patterns that scan order can distinguish planted as POSITIVE maxima: first = second, first = third,
    all four equal.  Returns (x, lin [C], gfeat for `pool, tap`)."""
    rs = np.random.RandomState([res, C, seed])
    x = rs.randint(-6, 7, size=[POOL_N, C, res, res]).astype(np.float32)
    spots = [(0, 0, 0, 0), (0, C - 1, res // 2 - 1, res // 2 - 1), (1, 0, 0, res // 2 - 1)]          # (n, c, window row, window column)
    for (n, c, wy, wx), (name, idx) in zip(spots, TIE_PATTERNS.items()):
        win = x[n, c, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2].reshape(4).copy()
        win[:] = rs.randint(-6, 5, size=4)
        win[list(idx)] = 7 + len(idx)
        x[n, c, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2] = win.reshape(2, 2)
    lin = (rs.randint(1, 5, size=[C]) / 4.0).astype(np.float32)
    gfeat = rs.randint(-4, 5, size=[POOL_N, C * (res // 2) ** 2]).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(lin), torch.from_numpy(gfeat)


def pool_exact_reference(pool, x):
    """(pooled [N][C][res/2][res/2] exact in float32, route(g): the pool's exact adjoint applied to a gradient of the pooled shape)"""
    x64 = x.double()
    y = (pool_first_max(x64) if pool == 'maxpool' else pool_avg(x64))

    def route(g):
        xr = x64.clone().requires_grad_(True)
        yy = pool_first_max(xr) if pool == 'maxpool' else pool_avg(xr)
        (gx,) = torch.autograd.grad(yy, [xr], g.double().reshape(yy.shape))
        return gx

    return y, route


def tie_windows(x):
    """which of the three tie patterns occur as a positive maximum of some 2x2 window"""
    v = torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]], dim=-1)
    m = v.max(dim=-1, keepdim=True).values
    at = (v == m) & (m > 0)
    found = {}
    for name, idx in TIE_PATTERNS.items():
        want = torch.zeros(4, dtype=torch.bool)
        want[list(idx)] = True
        found[name] = bool((at == want).all(dim=-1).any())
    return found


def pool_sign_inputs(res, seed=0):
    """C = 1, inputs +-k (k in 1..6, no zero): behind the pool the tap's normalised value is +-1 and its gradient is 0 by construction"""
    rs = np.random.RandomState([res, 1, seed, 9])
    x = (rs.randint(1, 7, size=[POOL_N, 1, res, res]) * rs.choice([-1, 1], size=[POOL_N, 1, res, res])).astype(np.float32)
    gfeat = rs.randint(-4, 5, size=[POOL_N, (res // 2) ** 2]).astype(np.float32)
    return torch.from_numpy(x), torch.ones([1]), torch.from_numpy(gfeat)


# ---------------------------------------------------------------------------------------------------------------------------------
# discriminator

def _fir(dtype):
    f1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float32)
    return (torch.outer(f1, f1) / 64.0).to(dtype)


def _fir_apply(x, pad, stride, dtype):
    c = x.shape[1]
    return F.conv2d(F.pad(x, [pad] * 4), _fir(dtype)[None, None].expand(c, 1, 4, 4), groups=c, stride=stride)


def disc_restate(sd, R, clamp, group, img, dtype, dlogits=None):
    """Forward of the 'resnet' discriminator from its state_dict (float32 tensors), every operation in `dtype`.
    clamp: float or None; group: MinibatchStd group size.  Returns dict(logits, gx, pre)."""
    P = {k: v.detach().to(dtype) for k, v in sd.items()}
    img = img.detach().to(dtype).requires_grad_(True)
    pre = []

    def lrelu(name, a, gain, cl):
        v = torch.where(a > 0, a, a * 0.2) * gain
        pre.append(Pre(name, a, v if cl is not None else None, cl))
        return v.clamp(-cl, cl) if cl is not None else v

    def wgt(name):
        w = P[name]
        return w * (1.0 / math.sqrt(w[0].numel()))

    x = None
    r = R
    while r > 4:
        b = f'b{r}'
        if r == R:
            x = lrelu(f'{b}.fromrgb', F.conv2d(img, wgt(f'{b}.fromrgb.weight'), P[f'{b}.fromrgb.bias']), SQRT2, clamp)
        y = F.conv2d(_fir_apply(x, 1, 2, dtype), wgt(f'{b}.skip.weight')) * RSQRT2
        x = lrelu(f'{b}.conv0', F.conv2d(x, wgt(f'{b}.conv0.weight'), P[f'{b}.conv0.bias'], padding=1), SQRT2, clamp)
        a = F.conv2d(_fir_apply(x, 2, 1, dtype), wgt(f'{b}.conv1.weight'), P[f'{b}.conv1.bias'], stride=2)
        x = y + lrelu(f'{b}.conv1', a, SQRT2 * RSQRT2, None if clamp is None else clamp * RSQRT2)
        r //= 2
    N, C, H, W = x.shape
    G = min(group, N)
    assert N % G == 0
    s = x.reshape(G, N // G, C, H, W)
    s = s - s.mean(dim=0)
    s = ((s * s).mean(dim=0) + 1e-8).sqrt().mean(dim=[1, 2, 3])          # [N / G]
    x = torch.cat([x, s.reshape(-1, 1, 1, 1).repeat(G, 1, H, W)], dim=1)
    x = lrelu('b4.conv', F.conv2d(x, wgt('b4.conv.weight'), P['b4.conv.bias'], padding=1), SQRT2, clamp)
    x = lrelu('b4.fc', x.flatten(1) @ wgt('b4.fc.weight').t() + P['b4.fc.bias'], SQRT2, None)
    logits = x @ wgt('b4.out.weight').t() + P['b4.out.bias']
    gx = None
    if dlogits is not None:
        (gx,) = torch.autograd.grad(logits, [img], dlogits.to(dtype).reshape(logits.shape))
    return dict(logits=logits.detach(), gx=gx, pre=pre)


def disc_oracle(D, img, dlogits):
    """float64 autograd of oracle/sg2_networks.Discriminator: what `disc_restate` must equal.  (Leaves D in float32.)"""
    from oracle import sg2_networks as nets
    old = nets.COMPUTE_DTYPE
    nets.COMPUTE_DTYPE = torch.float64
    try:
        D.double()
        x = img.detach().double().requires_grad_(True)
        logits = D(x, None)
        (gx,) = torch.autograd.grad(logits, [x], dlogits.double().reshape(logits.shape))
        return logits.detach(), gx
    finally:
        D.float()
        nets.COMPUTE_DTYPE = old


class DiscCase:
    """table: {resolution: channels} for 4..R.  B live samples of max_batch; clamp None = no clamp."""

    def __init__(self, name, R, table, B, imgc=2, group=4, clamp=256.0, max_batch=None, seed=0, scale=1.0, kind='guarded', wscale=1.0):
        self.wscale = wscale          # factor on the conv0 / conv1 / b4.conv weights (the clamp case: deeper layers must reach the clamp too)
        self.name, self.R, self.table, self.B, self.imgc, self.group, self.clamp = name, R, dict(table), B, imgc, group, clamp
        self.max_batch = B if max_batch is None else max_batch
        self.seed, self.scale, self.kind = seed, scale, kind

    def build(self, seed=None):
        """(D, img, dlogits): the oracle module with non-zero biases, and float32 inputs, from the case's seed"""
        from oracle import sg2_networks as nets
        seed = self.seed if seed is None else seed
        D = nets.make_discriminator(img_resolution=self.R, img_channels=self.imgc, seed=seed, conv_clamp=self.clamp,
                                    mbstd_group_size=self.group, channels=self.table)
        g = torch.Generator().manual_seed(1000 * seed + 29)
        with torch.no_grad():
            for n, p in D.named_parameters():
                if n.endswith('bias'):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
                elif self.wscale != 1.0 and n.split('.')[-2] in ('conv0', 'conv1', 'conv'):
                    p.mul_(self.wscale)
        img = torch.randn([self.B, self.imgc, self.R, self.R], generator=g) * self.scale
        dlogits = torch.randn([self.B, 1], generator=g)
        return D, img, dlogits

    def restate(self, D, img, dlogits, dtype):
        return disc_restate(D.state_dict(), self.R, self.clamp, self.group, img, dtype, dlogits)

    def runs(self, seed=None):
        D, img, dlogits = self.build(seed)
        return D, img, dlogits, self.restate(D, img, dlogits, torch.float32), self.restate(D, img, dlogits, torch.float64)


T8 = {4: 16, 8: 8}
CLAMP = 0.5
DISC_CASES = [
    DiscCase('R8', 8, T8, 4, seed=0),
    DiscCase('R128', 128, {4: 16, 8: 16, 16: 16, 32: 8, 64: 8, 128: 4}, 2, seed=0, kind='bulk'),
    # img_channels 1 / 3 / 4 above 64 x 64: the FromRGB backward runs la_torgb_fwd_kernel<imgc> there (la_torgb_fwd_small_kernel below)
    DiscCase('R128-imgc1', 128, {4: 16, 8: 16, 16: 16, 32: 8, 64: 8, 128: 4}, 1, imgc=1, seed=0, kind='bulk'),
    DiscCase('R128-imgc3', 128, {4: 16, 8: 16, 16: 16, 32: 8, 64: 8, 128: 4}, 1, imgc=3, seed=0, kind='bulk'),
    DiscCase('R128-imgc4', 128, {4: 16, 8: 16, 16: 16, 32: 8, 64: 8, 128: 4}, 1, imgc=4, seed=0, kind='bulk'),
    DiscCase('imgc1', 16, {4: 16, 8: 16, 16: 8}, 4, imgc=1, seed=2),
    DiscCase('imgc3', 16, {4: 16, 8: 16, 16: 8}, 4, imgc=3, seed=2),
    DiscCase('imgc4', 16, {4: 16, 8: 16, 16: 8}, 4, imgc=4, seed=5),
    DiscCase('group-B1', 8, T8, 1, seed=0),
    DiscCase('group-B3', 8, T8, 3, seed=0),
    DiscCase('group-B8-g4', 8, T8, 8, group=4, seed=0),
    DiscCase('group-B6-g3', 8, T8, 6, group=3, seed=0),
    DiscCase('group-B9-g9', 8, T8, 9, group=9, seed=0),
    DiscCase('group-B16-g16', 8, T8, 16, group=16, seed=1),
    DiscCase('clamp-0.5', 16, {4: 16, 8: 16, 16: 8}, 4, clamp=CLAMP, seed=0, wscale=2.0),
    DiscCase('clamp-none', 16, {4: 16, 8: 16, 16: 8}, 4, clamp=None, seed=1),
    DiscCase('channels-12-20-36', 32, {4: 36, 8: 20, 16: 12, 32: 20}, 1, seed=11)          # (B = 2 meets the guard at no seed below 64),
]
DISC_BY_NAME = {c.name: c for c in DISC_CASES}
DISC_CLAMP_CASES = ['clamp-0.5']
DISC_SHRINK = DiscCase('disc-shrinking-batch', 16, {4: 16, 8: 16, 16: 8}, 4, max_batch=8, seed=1)          # B = 8 x 2^8 first, then these 4
DISC_SHRINK_BIG = 2.0 ** 8
DISC_BAD_TABLE = {4: 16, 8: 6, 16: 8}          # an entry that is not a multiple of 4: refused at create
DISC_GROUP_REFUSAL = dict(B=5, group=4)

LOSS_LOGITS = [-100.0, -25.0, -20.5, -19.5, -1e-4, 1.0, 19.5, 100.0]          # both sides of softplus' threshold at 20, and saturation
LOSS_NORM_BATCH = [0, 16]
LOSS_W = 0.5


def disc_loss_restate(logits, w, norm_batch):
    """(softplus(-l).sum() / n * w, d(loss)/d(logits)) in float64"""
    l = np.asarray(logits, np.float64)
    n = float(norm_batch if norm_batch > 0 else l.size)
    sp = np.logaddexp(0.0, -l)
    return float(sp.sum() / n * w), -(1.0 / (1.0 + np.exp(l))) * w / n


# ---------------------------------------------------------------------------------------------------------------------------------

def search_seed(case):
    """first seed of 0..MAX_SEEDS-1 whose float64 run meets the guard, or None"""
    for s in range(MAX_SEEDS):
        r = case.runs(s)
        g, m, _ = guard_of(r[-2]['pre'], r[-1]['pre'])
        if m >= g:
            return s
    return None


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for case in FEAT_CASES + [FEAT_SHRINK] + DISC_CASES + [DISC_SHRINK]:
        if case.kind == 'guarded':
            print(f'{case.name}: recorded seed {case.seed}, first seed that meets the guard {search_seed(case)}', flush=True)
