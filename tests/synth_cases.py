"""Case table, seeded inputs and the float64 / float32 restatement of the synthesis engine (la_synth.hip, the affine / demod / ToRGB / seam /
style-finish kernels of la_style.hip, the ToRGB and the seams fused into the contraction epilogues; SynthesisEngine).  Shared by
test_synth_cases_cpu.py (which proves, without a GPU, that the restatement equals float64 autograd of the oracle and that every case
reaches what it claims) and by test_hip_synth_shapes.py.  No GPU and no ctypes here; every input is synthetic and seeded.  The helpers
(`Pre`, `guard_of`, `worst`, `rel_l2`, `budget`, `search_seed`) and the three kinds of case (GUARDED, BULK; no EXACT case here) are those
of tests/engine_cases.py.

`synth_restate` is the forward of oracle/sg2_networks.SynthesisNetwork (architecture 'skip', noise_mode 'const') written out in plain
torch from the state dict, in the engine's non-fused form: per layer styles = affine(w) (ToRGB: x 1 / sqrt(cin)), demodulation
rsqrt(sum (s W)^2 + 1e-8), x * s -> 3x3 conv (up layer: stride-2 transposed conv, then the 4x4 FIR with gain 4) -> * d + noise + bias,
lrelu x sqrt 2, clamp; ToRGB 1x1 without demodulation, bias, clamp; image = upsample2d(image of the block below) + ToRGB.  It exposes every
block image, every conv-layer output, every style row in the engine's order (conv layers first, then the ToRGB layers: `describe()` of
la_synth.hip), every kink as a `Pre` record (lrelu at 0 of each conv layer, |v| = clamp of conv and ToRGB layers) and, given g_img, dws
and the gradient with respect to every style row.

`branch_plan` restates on the host which form each block of a case takes in a mode.  It only proves reach (which case runs which kernel
form); no expected value comes from it.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_cases import Pre, SQRT2, budget, guard_of, rel_l2, search_seed, worst  # noqa: E402,F401

MODES = ['f32', 'bf16x3', 'f16x2']


class ClampPre(Pre):
    """a ToRGB layer: linear, so its only kink is |v| = clamp (`a` = `v` = the value in front of the clamp)"""

    def __init__(self, name, v, clamp):
        super().__init__(name, v, v, clamp)

    def margin(self):
        return float((self.v.abs() - self.clamp).abs().min() / self.v.abs().max())


def _fir(dtype):
    f1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float32)
    return (torch.outer(f1, f1) / 64.0 * 4.0).to(dtype)          # setup_filter([1, 3, 3, 1]) with the gain up^2 = 4 (symmetric: no flip)


def _fir_same(z, pad, dtype):
    c = z.shape[1]
    return F.conv2d(F.pad(z, pad), _fir(dtype)[None, None].expand(c, 1, 4, 4), groups=c)


def _upsample2d(img, dtype):
    """zero insertion, pad (2, 1, 2, 1), 4x4 FIR with gain 4"""
    n, c, h, w = img.shape
    z = img.new_zeros([n, c, 2 * h, 2 * w])
    z[:, :, ::2, ::2] = img
    return _fir_same(z, [2, 1, 2, 1], dtype)


def block_resolutions(R):
    return [2 ** i for i in range(2, int(math.log2(R)) + 1)]


def synth_restate(sd, R, imgc, clamp, noise_strengths, ws, dtype, g_img=None):
    """sd: state dict of the synthesis network (b4.const, b{r}.conv{0,1}.*, b{r}.torgb.*; float32 tensors), every operation in `dtype`.
    clamp: float or None; noise_strengths: one per conv layer in execution order; ws [B][num_ws][w_dim].
    Returns dict(img, imgs, layers, styles [B][S], pre, and with g_img: dws, dstyles [B][S])."""
    P = {k: v.detach().to(dtype) for k, v in sd.items() if torch.is_floating_point(v)}
    ws = ws.detach().to(dtype).requires_grad_(g_img is not None)
    B, _, w_dim = ws.shape

    def affine(pfx, w, post=1.0):
        return (w @ (P[pfx + '.affine.weight'] * (1.0 / math.sqrt(w_dim))).t() + P[pfx + '.affine.bias']) * post

    def cl(v):
        return v if clamp is None else v.clamp(-clamp, clamp)

    x = img = None
    conv_s, rgb_s, layers, imgs, pre = [], [], [], [], []
    li = wi = 0
    for res in block_resolutions(R):
        if res == 4:
            x = P['b4.const'][None].expand(B, -1, -1, -1)
        for ln in (('conv1',) if res == 4 else ('conv0', 'conv1')):
            pfx = f'b{res}.{ln}'
            W = P[pfx + '.weight']
            s = affine(pfx, ws[:, wi])
            wi += 1
            d = torch.rsqrt((s * s) @ (W * W).sum(dim=[2, 3]).t() + 1e-8)
            xs = x * s[:, :, None, None]
            if ln == 'conv0':
                z = _fir_same(F.conv_transpose2d(xs, W.transpose(0, 1), stride=2), [1, 1, 1, 1], dtype)
            else:
                z = F.conv2d(xs, W, padding=1)
            a = z * d[:, :, None, None]
            if noise_strengths[li] != 0.0:
                a = a + P[pfx + '.noise_const'] * noise_strengths[li]
            a = a + P[pfx + '.bias'][None, :, None, None]
            v = torch.where(a > 0, a, a * 0.2) * SQRT2
            pre.append(Pre(pfx, a, v if clamp is not None else None, clamp))
            x = cl(v)
            conv_s.append(s)
            layers.append(x)
            li += 1
        pfx = f'b{res}.torgb'
        s = affine(pfx, ws[:, wi], 1.0 / math.sqrt(x.shape[1]))          # (shares its w with the next block's conv0)
        y = F.conv2d(x * s[:, :, None, None], P[pfx + '.weight']) + P[pfx + '.bias'][None, :, None, None]
        if clamp is not None:
            pre.append(ClampPre(pfx, y, clamp))
        img = cl(y) if img is None else _upsample2d(img, dtype) + cl(y)
        rgb_s.append(s)
        imgs.append(img)
    assert li == len(noise_strengths) and wi + 1 == ws.shape[1] and img.shape[1] == imgc
    styles = conv_s + rgb_s
    out = dict(img=img.detach(), imgs=[t.detach() for t in imgs], layers=[t.detach() for t in layers],
               styles=torch.cat([t.detach() for t in styles], dim=1), pre=pre, dws=None, dstyles=None)
    if g_img is not None:
        grads = torch.autograd.grad(img, [ws] + styles, g_img.to(dtype))
        out['dws'], out['dstyles'] = grads[0], torch.cat(grads[1:], dim=1)
    return out


def synth_oracle(G, ws, g_img):
    """float64 autograd of oracle/sg2_networks.SynthesisNetwork: what `synth_restate` must equal.  Returns (img, the blocks' x, dws,
    gradients of the `affine` outputs in execution order: conv layers and ToRGB of block 4, of block 8, ...).  (Leaves G in float32.)"""
    from oracle import sg2_networks as nets
    old = nets.COMPUTE_DTYPE
    nets.COMPUTE_DTYPE = torch.float64
    kept, hooks = [], []
    try:
        G.double()
        for m in G.synthesis.modules():
            if isinstance(m, (nets.SynthesisLayer, nets.ToRGBLayer)):
                def hook(_mod, _inp, out, kept=kept):
                    out.retain_grad()
                    kept.append(out)
                hooks.append(m.affine.register_forward_hook(hook))
        w = ws.detach().double().requires_grad_(True)
        img, feats = G.synthesis(w, noise_mode='const', return_features=True)
        img.backward(g_img.double())
        return img.detach(), [f.detach() for f in feats], w.grad, [t.grad for t in kept]
    finally:
        for h in hooks:
            h.remove()
        G.float()
        nets.COMPUTE_DTYPE = old


class SynthCase:
    """channels: one per block 4..R.  B live samples of max_batch; clamp None = no clamp; noise: one strength per conv layer (a float:
    every layer); scale: factor on ws."""

    def __init__(self, name, R, channels, imgc, B, max_batch=None, w_dim=16, clamp=256.0, noise=0.1, seed=0, kind='guarded', scale=1.0):
        self.name, self.R, self.imgc, self.w_dim, self.B, self.clamp = name, R, imgc, w_dim, B, clamp
        self.table = dict(zip(block_resolutions(R), channels))
        assert len(self.table) == len(channels)
        self.max_batch = B if max_batch is None else max_batch
        nconv = 2 * len(channels) - 1
        # (as float32 numbers: the strengths are float32 parameters of the network, and the engine is handed their values)
        self.noise = [float(torch.tensor(v, dtype=torch.float32)) for v in ([noise] * nconv if isinstance(noise, (int, float)) else noise)]
        assert len(self.noise) == nconv
        self.seed, self.kind, self.scale = seed, kind, scale

    @property
    def channels(self):
        return [self.table[r] for r in sorted(self.table)]

    def build(self, seed=None):
        """(G, ws, g_img): the oracle generator (default init under the seed; conv and ToRGB biases randn x 0.1; the case's noise
        strengths) and float32 inputs from a seeded CPU generator"""
        from oracle import sg2_networks as nets
        seed = self.seed if seed is None else seed
        G = nets.make_generator(img_resolution=self.R, img_channels=self.imgc, seed=seed, conv_clamp=self.clamp, w_dim=self.w_dim,
                                mapping_layers=1, channels=self.table)
        g = torch.Generator().manual_seed(1000 * seed + 31)
        li = 0
        with torch.no_grad():
            for m in G.synthesis.modules():
                if isinstance(m, (nets.SynthesisLayer, nets.ToRGBLayer)):
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                if isinstance(m, nets.SynthesisLayer):
                    m.noise_strength.fill_(self.noise[li])
                    li += 1
        assert li == len(self.noise)
        ws = torch.randn([self.B, G.num_ws, self.w_dim], generator=g) * self.scale
        g_img = torch.randn([self.B, self.imgc, self.R, self.R], generator=g)
        return G, ws, g_img

    def restate(self, G, ws, g_img, dtype):
        return synth_restate(G.synthesis.state_dict(), self.R, self.imgc, self.clamp, self.noise, ws, dtype, g_img)

    def runs(self, seed=None):
        G, ws, g_img = self.build(seed)
        return G, ws, g_img, self.restate(G, ws, g_img, torch.float32), self.restate(G, ws, g_img, torch.float64)


C8 = (8, 8, 8)
CLAMP_BINDS = 1.0
RGBFUSE = (16, 16, 16, 16, 32)
R128 = (16, 16, 8, 8, 8, 8)
# (the seeds of the guarded cases are the first of 0..63 that meet the guard: `python tests/synth_cases.py` prints the search)
SYNTH_CASES = [
    SynthCase('R4-only', 4, (8,), 2, 3, seed=0),
    SynthCase('R8-imgc1', 8, (8, 8), 1, 2, seed=0),
    SynthCase('R16-imgc3-ch12-20-8', 16, (12, 20, 8), 3, 2, 4, w_dim=24, seed=0),
    SynthCase('R16-imgc4', 16, C8, 4, 3, seed=0),
    SynthCase('R16-clamp-binds', 16, C8, 2, 2, clamp=CLAMP_BINDS, seed=4),          # (the first guarded seed at which the clamp binds in every layer)
    SynthCase('R16-clamp-none', 16, C8, 2, 2, clamp=None, seed=2),
    SynthCase('R16-noise-mixed', 16, C8, 2, 2, noise=(0.3, 0.0, 0.1, 0.0, 0.2), seed=1),
    SynthCase('R32-imgc3-B1', 32, (8, 8, 4, 4), 3, 1, 2, seed=0),
] + [SynthCase(f'R64-rgbfuse-imgc{c}', 64, RGBFUSE, c, 2, kind='bulk') for c in (1, 3, 4)] + [
    # (imgc 1 and 4 beside the 3: the large ToRGB kernel has the four instantiations too, and the whole-network tests run the 2)
    SynthCase(f'R128-imgc{c}', 128, R128, c, 2, kind='bulk') for c in (1, 3, 4)] + [
    SynthCase('R256-imgc3-slabs', 256, (8, 8, 8, 8, 4, 4, 4), 3, 2, kind='bulk'),
]
SYNTH_BY_NAME = {c.name: c for c in SYNTH_CASES}
assert len(SYNTH_BY_NAME) == len(SYNTH_CASES)
SYNTH_GUARDED = [c for c in SYNTH_CASES if c.kind == 'guarded']
SYNTH_BULK = [c for c in SYNTH_CASES if c.kind == 'bulk']
SYNTH_CLAMP_CASE = 'R16-clamp-binds'
CLAMP_FRACTION = (0.01, 0.5)
SYNTH_SHRINK = SynthCase('synth-shrinking-batch', 16, C8, 3, 2, 4, seed=0)          # B = 4 with ws x 2^3, g_img x 2^8 first, then these 2
SHRINK_WS, SHRINK_G = 2.0 ** 3, 2.0 ** 8


def clamp_binds(pre64):
    """between 1 % and 50 % of the values of EVERY conv layer and EVERY ToRGB layer lie beyond the clamp"""
    return all(CLAMP_FRACTION[0] <= p.clamped_fraction() <= CLAMP_FRACTION[1] for p in pre64)


def first_seed(case):
    """`search_seed`; for the clamp case the first seed that meets the guard AND `clamp_binds`"""
    if case.name != SYNTH_CLAMP_CASE:
        return search_seed(case)
    for s in range(64):
        r = case.runs(s)
        g, m, _ = guard_of(r[-2]['pre'], r[-1]['pre'])
        if m >= g and clamp_binds(r[-1]['pre']):
            return s
    return None


def window_of(R):
    return R // 4 + 1, 3 * R // 4 - 2


# (case, columns too?): image rows (and columns) [R / 4 + 1, 3 R / 4 - 2), g_img zero outside
SYNTH_WINDOWED = [('R128-imgc3', False), ('R128-imgc3', True), ('R64-rgbfuse-imgc3', False)]


def windowed_g_img(case, g_img, cols):
    lo, hi = window_of(case.R)
    clo, chi = (lo, hi) if cols else (0, case.R)
    g = torch.zeros_like(g_img)
    g[:, :, lo:hi, clo:chi] = g_img[:, :, lo:hi, clo:chi]
    return g


# refusals: (name, R, channels, imgc, w_dim, where it must be refused, fragment of the message)
SYNTH_REFUSALS = [
    ('table-entry-6', 16, (8, 6, 8), 2, 16, 'create', 'multiples of 4'),
    ('imgc-0', 8, (8, 8), 0, 16, 'create', 'img_channels must be 1..4'),
    ('imgc-5', 8, (8, 8), 5, 16, 'create', 'img_channels must be 1..4'),
    ('w_dim-18', 8, (8, 8), 2, 18, 'forward', 'w_dim'),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# which form each block takes (la_synth_forward / la_synth_backward, la_torgb_forward, la_modconv3x3_fwd_fuses_rgb = the class la_conv_plan gives
# a dense 3x3 launch on the whole res x res grid, i.e. the conditions of its halo predicate, la_seam_slabs)

HALO_MIN_GRID = 1157
TORGB_SMALL_MAX_HW = 4096


def uses_halo(mode, cin, res):
    return mode != 'f32' and res % 32 == 0 and res % 4 == 0 and res * res >= HALO_MIN_GRID and cin * res * res < (1 << 28) and cin <= 4096


def seam_slabs(hw):
    return max(1, min(64, hw // 16384))


CONV_TILE_PIXELS = 128          # pixels per contraction tile (modconv_cases.NT): la_modconv_ds_tiles(res) = ceil(res^2 / 128)
PYRAMID_MAX_RES = 256


def ds_tiles(res):
    return -(-res * res // CONV_TILE_PIXELS)


def branch_plan(case, mode):
    """-> dict(nblocks, imgc, clamp, pyramid, pyramid_block, blocks=[dict(res, cin, cout, torgb='fused' | 'small' | 'large', up2_skip,
    seam='kernel' | 'fused', slabs, ...)]): per block the ToRGB forward form, whether its skip image is up-sampled inside the ToRGB kernel,
    where the seam of its conv1 output (with the ToRGB backward) runs, and the slabs of the seam kernel.  What la_synth_plan_query has
    beyond that (test_synth_plan_cpu.py holds the two against each other): skip_launch (the skip image is up-sampled by a launch of its own
    before conv1), seam0 (where the seam of the block's conv0 output runs: the seam kernel, or fused into conv1's backward; None in the
    first block), nseg1 / nseg0 (segments of the partials of conv1 / conv0: seam slabs where the seam is a kernel, contraction tiles where
    it is fused), tiles1 / tiles0 (tiles of the layers' style-gradient partials: the grid of their backward contraction), down_fir (the
    backward pass launches the image gradient's down-FIR at this block) and pyramid_block (the block whose launch makes every level below)."""
    ch, blocks = case.channels, []
    nb = len(ch)
    # the image-gradient pyramid: the first block from the top with k >= 2 whose level below is <= 256^2 hands every lower level to one launch
    pyramid_block = next((k for k in range(nb - 1, 0, -1) if k >= 2 and (4 << k) // 2 <= PYRAMID_MAX_RES), None)
    for k, co in enumerate(ch):
        res = 4 << k
        fused = co in (32, 64, 128) and uses_halo(mode, co, res)
        seam1 = 'kernel' if (mode == 'f32' or k == nb - 1) else 'fused'
        seam0 = None if k == 0 else ('kernel' if mode == 'f32' else 'fused')
        blocks.append(dict(res=res, cin=ch[k - 1] if k else 0, cout=co,
                           torgb='fused' if fused else ('small' if res * res <= TORGB_SMALL_MAX_HW else 'large'),
                           up2_skip=k > 0 and not fused,
                           seam=seam1, slabs=seam_slabs(res * res),
                           skip_launch=k > 0 and fused, seam0=seam0,
                           nseg1=ds_tiles(res) if seam1 == 'fused' else seam_slabs(res * res),
                           nseg0=None if k == 0 else (ds_tiles(res) if seam0 == 'fused' else seam_slabs(res * res)),
                           tiles1=ds_tiles(res), tiles0=None if k == 0 else ds_tiles(res // 2),
                           down_fir=k > 0 and (pyramid_block is None or k >= pyramid_block)))
    return dict(nblocks=nb, imgc=case.imgc, clamp=case.clamp, pyramid=pyramid_block is not None, pyramid_block=pyramid_block, blocks=blocks)


# what the sweep claims to reach: name -> predicate over (case, mode, plan)
def _any_block(plan, **want):
    return any(all(b[k] == v for k, v in want.items()) for b in plan['blocks'])


BRANCHES = dict(
    [(f'small ToRGB kernel, IMGC = {c}', (lambda cs, m, p, c=c: cs.imgc == c and _any_block(p, torgb='small'))) for c in (1, 2, 3, 4)] +
    [(f'large ToRGB kernel with the up-2 skip, IMGC = {c}', (lambda cs, m, p, c=c: cs.imgc == c and _any_block(p, torgb='large', up2_skip=True))) for c in (1, 3, 4)] +
    [(f'ToRGB fused into the halo forward, IMGC = {c}', (lambda cs, m, p, c=c: cs.imgc == c and _any_block(p, torgb='fused'))) for c in (1, 3, 4)] +
    [(f'seam kernel with ToRGB backward, IMGC = {c}', (lambda cs, m, p, c=c: cs.imgc == c and _any_block(p, seam='kernel'))) for c in (1, 2, 3, 4)] +
    [(f'ToRGB backward fused into the up layer\'s backward, imgc = {c}', (lambda cs, m, p, c=c: cs.imgc == c and _any_block(p, seam='fused'))) for c in (1, 2, 3, 4)] +
    [('seam kernel in 4 slabs', lambda cs, m, p: _any_block(p, seam='kernel', slabs=4)),
     ('one block (backward ends at k == 0)', lambda cs, m, p: p['nblocks'] == 1),
     ('image-gradient pyramid', lambda cs, m, p: p['pyramid']),
     ('no pyramid with two blocks', lambda cs, m, p: p['nblocks'] == 2 and not p['pyramid']),
     ('a clamp that binds', lambda cs, m, p: cs.clamp == CLAMP_BINDS),
     ('conv_clamp None', lambda cs, m, p: cs.clamp is None),
     ('channel counts that are no power of two', lambda cs, m, p: any(c & (c - 1) for c in cs.channels)),
     ('cin < cout in an up layer', lambda cs, m, p: any(b['cin'] and b['cin'] < b['cout'] for b in p['blocks'])),
     ('cin > cout in an up layer', lambda cs, m, p: any(b['cin'] > b['cout'] for b in p['blocks'])),
     ('4-channel layers', lambda cs, m, p: 4 in cs.channels),
     ('a layer without noise beside layers with noise', lambda cs, m, p: 0.0 in cs.noise and any(cs.noise)),
     ('B < max_batch', lambda cs, m, p: cs.B < cs.max_batch),
     ('B = 1', lambda cs, m, p: cs.B == 1),
     ('odd B', lambda cs, m, p: cs.B == 3),
     ('w_dim 24', lambda cs, m, p: cs.w_dim == 24)])


def reach_table():
    """{branch: [(case name, modes that reach it)]} over SYNTH_CASES + SYNTH_SHRINK"""
    table = {}
    for name, pred in BRANCHES.items():
        rows = []
        for cs in SYNTH_CASES + [SYNTH_SHRINK]:
            modes = [m for m in MODES if pred(cs, m, branch_plan(cs, m))]
            if modes:
                rows.append((cs.name, modes))
        table[name] = rows
    return table


def reach_text():
    """the table as it stands in the docstring of test_hip_synth_shapes.py"""
    lines = []
    for name, rows in reach_table().items():
        cells = [cn if len(ms) == len(MODES) else f'{cn} ({" ".join(ms)})' for cn, ms in rows]
        lines.append(f'    {name}: ' + (', '.join(cells) if cells else 'NO CASE'))
    return '\n'.join(lines)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if '--table' in sys.argv:
        print(reach_text())
    else:
        for case in SYNTH_GUARDED + [SYNTH_SHRINK]:
            print(f'{case.name}: recorded seed {case.seed}, first seed that meets the guard {first_seed(case)}', flush=True)
