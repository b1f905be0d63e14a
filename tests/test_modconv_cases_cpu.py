"""modconv_cases.py checked without a GPU: the float64 restatement of the four layer entries against float64 autograd through
oracle/sg2_ops.py, the exact cases' representability, and the coverage of the dispatch plan -- which kernel instantiations the table
reaches and that every edge it names is reached, asserted from each case's numbers.

Kernel forms that no call of the four public entries can reach (so the list below cannot hold them):
  * the halo kernel's plain tile order.  la_conv_halo.hip takes the XCD-contiguous order when `(nt & 7) == 0`; la_conv_bf16_uses_halo
    wants `(a.Gx & 31) == 0` and the entries are square, so a halo grid is (32 k)^2 and holds 8 k^2 tiles: always a multiple of 8
    (res 64: 32, res 96: 72, res 160: 200).  Only the engine's row / column windows give other counts.  The flat and the exact-fp32
    kernels have the same switch and are run on both sides of it (10, 11 and 18 tiles at res 35, 36 and 48; 32 at the 64x64 grids).
  * 32-row tiles of the flat kernel: LaConvPlan::mt is 32 only under la_conv_bf16_uses_halo (la_conv.hip, la_conv_plan).
  * a split exact-fp32 launch of merged phases: la_conv_plan refuses merged phases at LA_PREC_F32; la_conv_up2_launch merges for the 16-bit
    precisions only.
  * 16 slices from 17 chunks: choose_ksplit skips a slice count k with ceil(nck / ceil(nck / k)) != k, so C = 544 runs 9 slices of two
    chunks (the last of one); 16 slices need 16 chunks (C = 512) or 31 / 32.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modconv_cases as mc  # noqa: E402

from oracle import sg2_ops  # noqa: E402


def _index(c):
    return mc.CASES.index(c)


def test_table_is_small_and_well_formed():
    assert len(mc.CASES) <= 60
    for c in mc.CASES:
        assert c['why'] and c['entry'] in mc.ENTRIES
        rows = c['cout'] if c['entry'].endswith('fwd') else c['cin']
        assert rows % 4 == 0, c['name']
        if c['entry'].startswith('up2'):
            assert c['res'] % 2 == 0


def _oracle_forward(c, t, x, s):
    """y through sg2_ops in float64, the demodulation coefficients held fixed (they are an input of the entries)."""
    o = c['opts']
    up = c['entry'] == 'up2_fwd'
    f = sg2_ops.setup_filter([1, 3, 3, 1])
    z = sg2_ops.modulated_conv2d(x, t['w'].double(), s, noise=None, up=2 if up else 1, padding=1, resample_filter=f, demodulate=False,
                                 flip_weight=not up, fused_modconv=False)
    if t['d'] is not None:
        z = z * t['d'].double()[:, :, None, None]
    nz = t['noise'].double()
    z = z + (nz[:, None] if nz.ndim == 3 else nz[None, None]) * float(torch.tensor(o['noise_strength'], dtype=torch.float32))
    return sg2_ops.bias_act(z, t['bias'].double(), act=o['act'], alpha=float(torch.tensor(o['alpha'], dtype=torch.float32)),
                            gain=float(torch.tensor(o['gain'], dtype=torch.float32)), clamp=o['clamp'] if o['clamp'] >= 0 else None)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('name', mc.ORACLE_SUBSET)
def test_restatement_equals_oracle_autograd(name):
    """y of the forward cases; for a backward case the forward layer of the same shape is built around it: gz = dy * act' * d, then
    gx against dx and ds against the modulation term of the style gradient (demodulation coefficients detached)."""
    c = mc.BY_NAME[name]
    t = mc.make_tensors(c, _index(c))
    gen = torch.Generator().manual_seed(99)
    B, cin, cout, res = c['B'], c['cin'], c['cout'], c['res']
    if c['entry'] in ('fwd', 'up2_fwd'):
        x = t['x'].double().expand(B, -1, -1, -1)
        y = _oracle_forward(c, t, x, t['s'].double())
        assert _rel(mc.restate(c, t, torch.float64)['y'], y) <= 1e-12
        # the fused form with its own demodulation (what the reference runs) agrees to the rounding of d
        if t['d'] is not None and not c['opts']['noise_per_sample']:
            up = c['entry'] == 'up2_fwd'
            z = sg2_ops.modulated_conv2d(x, t['w'].double(), t['s'].double(), noise=t['noise'].double() * c['opts']['noise_strength'],
                                         up=2 if up else 1, padding=1, resample_filter=sg2_ops.setup_filter([1, 3, 3, 1]),
                                         flip_weight=not up, fused_modconv=True)
            yf = sg2_ops.bias_act(z, t['bias'].double(), act=c['opts']['act'], gain=c['opts']['gain'], clamp=c['opts']['clamp'])
            assert _rel(y, yf) <= 1e-6
        return
    # a forward layer around the backward case, both activations over the subset
    fwd = dict(c, entry='fwd' if c['entry'] == 'bwd' else 'up2_fwd',
               opts=dict(c['opts'], act='lrelu' if _index(c) % 2 else 'linear', clamp=1.5, gain=1.25))
    ft = dict(t)
    ft['x'] = t['xin']
    ft['noise'] = torch.randn([res, res], generator=gen)
    ft['bias'] = torch.randn([cout], generator=gen) * 0.1
    ft['d'] = torch.rand([B, cout], generator=gen) + 0.5
    fwd['opts']['x_bstride0'] = c['opts']['xin_bstride0']
    x = ft['x'].double().expand(B, -1, -1, -1).clone().requires_grad_(True)
    s = t['s'].double().clone().requires_grad_(True)
    y = _oracle_forward(fwd, ft, x, s)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    dx, ds = torch.autograd.grad(y, [x, s], dy)
    o = fwd['opts']
    slope = torch.ones_like(y)
    if o['act'] == 'lrelu':
        slope[y <= 0] = float(torch.tensor(o['alpha'], dtype=torch.float32))
    slope = slope * float(torch.tensor(o['gain'], dtype=torch.float32)) * (y.abs() < o['clamp'])
    gz = dy * slope * ft['d'].double()[:, :, None, None]
    # (restate() reads float32 tensors: hand it gz through a float64 side door)
    got = mc.restate(c, dict(t, gz=gz.detach(), xin=ft['x']), torch.float64)
    assert _rel(got['gx'], dx) <= 1e-12
    assert _rel(got['ds'], ds) <= 1e-12


@pytest.mark.parametrize('name', [c['name'] for c in mc.CASES if c['opts']['exact']])
def test_exact_cases_are_float32_numbers(name):
    c = mc.BY_NAME[name]
    t = mc.make_tensors(c, _index(c))
    for k, v in mc.restate(c, t, torch.float64).items():
        assert torch.equal(v.float().double(), v), k
        assert float(v.abs().max()) < 2 ** 22
        assert float(v.abs().max()) > 0


# every template instantiation that la_conv_halo_launch, la_conv_flat_launch and la_conv_launch can launch for a call of the public entries:
# (precision, class, row tile, MFMA form, merged phases)
EXPECTED_FORMS = (
    # la_conv_igemm_kernel<128 / 64, SPLIT>
    [(0, cls, mt, '32x32x2', False) for cls in ('conv_f32', 'conv_f32_split') for mt in (128, 64)]
    # la_conv_bf16_kernel<128 / 64, SPLIT, FMT, 2>: bf16 x3 and bf16 x2, one launch and merged phases
    + [(p, cls, mt, '32x32', mg) for p in (1, 2) for cls in ('conv_flat', 'conv_splitk') for mt in (128, 64) for mg in (False, True)]
    # la_conv_bf16_halo_kernel<128 / 64 / 32, FMT, WV, HALO_MF_BF16>
    + [(p, 'conv_halo', mt, '32x32', False) for p in (1, 2) for mt in (128, 64, 32)]
    # fp16 x2: <64, SPLIT, FMT, 2> and the three-wave 16x16x32 forms on 128 rows (FLAT_MF_16 split, FLAT_MF_16_3BUF direct)
    + [(3, cls, 64, '32x32', mg) for cls in ('conv_flat', 'conv_splitk') for mg in (False, True)]
    + [(3, cls, 128, '16x16x32', mg) for cls in ('conv_flat', 'conv_splitk') for mg in (False, True)]
    # fp16 x2 halo: HALO_MF_F16_16 on 128 rows with more than one chunk, HALO_MF_F16_32 otherwise
    + [(3, 'conv_halo', 128, '16x16x32', False)] + [(3, 'conv_halo', mt, '32x32', False) for mt in (128, 64, 32)]
)


def _all_plans():
    for c in mc.CASES:
        for p in mc.PRECISIONS:
            for ws in (True, False):
                if ws or mc.splits(c, p):
                    yield c, p, ws, mc.plan(c, p, ws)


def test_plan_reaches_every_kernel_form():
    assert len(set(EXPECTED_FORMS)) == len(EXPECTED_FORMS) == 38
    seen = {}
    for c, p, ws, pl in _all_plans():
        for l in pl['launches']:
            seen.setdefault(mc.form_key(p, l), c['name'])
    assert set(seen) == set(EXPECTED_FORMS), (set(seen) ^ set(EXPECTED_FORMS))
    # every form is also reached by an exact case
    exact = {mc.form_key(p, l) for c, p, ws, pl in _all_plans() if c['opts']['exact'] for l in pl['launches']}
    assert exact == set(EXPECTED_FORMS), set(EXPECTED_FORMS) - exact


def test_workspace_modes():
    """Without the room for the partials every launch is direct; the full workspace holds what the plan takes from it."""
    for c, p, ws, pl in _all_plans():
        if not ws:
            assert all(l.ksplit == 1 for l in pl['launches'])
            assert pl['ws_bytes'] < mc.plan(c, p, True)['ws_bytes']
        n = len(pl['launches'])
        assert n == (4 if c['entry'] == 'up2_fwd' and p == 0 else 1)
        assert sum(pl['counts'][k] for k in ('conv_halo', 'conv_flat', 'conv_splitk', 'conv_f32')) == n


def _k_slices(c, p):
    (l,) = mc.plan(c, p, True)['launches']
    C = c['cin'] if c['entry'].endswith('fwd') else c['cout']
    nck = mc.cdiv(C, mc.KCB if p else mc.KC)
    per = mc.cdiv(nck, l.ksplit)
    return l.ksplit, [min(per, nck - k * per) for k in range(l.ksplit)]


def test_named_edges_are_reached():
    B = mc.BY_NAME
    # one pixel tile holds every sample / a tile straddles two samples (tiles_flat = cdiv(B * G, 128))
    c = B['sk_r4_b3']
    assert c['B'] * c['res'] ** 2 <= mc.NT and c['B'] == 3
    for name in ('sk_r6_b5', 'sk_r6_b5_f'):
        c = B[name]
        G = c['res'] ** 2
        assert c['B'] * G == 180 and mc.NT % G != 0 and mc.NT // G < c['B'] - 1      # pixel 128 is inside sample 3
        assert all(mc.splits(c, p) for p in mc.PRECISIONS)
    # the split-K bound
    for p in mc.PRECISIONS:
        assert B['sk_r34']['res'] ** 2 == mc.SPLITK_MAX_G == 1156 and mc.splits(B['sk_r34'], p)
        assert B['fl_r35']['res'] ** 2 == 1225 and not mc.splits(B['fl_r35'], p) and B['fl_r35']['cin'] > 32
        assert mc.plan(B['fl_r35'], p, True)['launches'][0].cls == ('conv_flat' if p else 'conv_f32')
        assert mc.splits(B['sk_r33'], p) and B['sk_r33']['res'] % 2 == 1
    assert 1156 % mc.NT == 4
    # chunks: one channel in the last, for the 16-bit chunk of 32 and the fp32 chunk of 16
    assert B['sk_r4_b3']['cin'] % mc.KCB == 1 and B['sk_c17']['cin'] % mc.KC == 1 and B['sk_c15']['cin'] < mc.KC == B['sk_c16']['cout']
    assert mc.splits(B['sk_c17'], 0) and not mc.splits(B['sk_c16'], 0) and not mc.splits(B['sk_c15'], 0)
    for p in (1, 2, 3):
        assert not mc.splits(B['sk_c32'], p) and B['sk_c32']['cin'] == mc.KCB      # one chunk: nothing to slice
        assert _k_slices(B['sk_r4_b3'], p) == (2, [1, 1])
        assert _k_slices(B['sk_3p2'], p) == (2, [3, 2])
        assert _k_slices(B['sk_c512'], p) == (16, [1] * 16)
        assert _k_slices(B['sk_c544'], p) == (9, [2] * 8 + [1])                   # 17 chunks under the 16-slice cap
    assert _k_slices(B['sk_c544'], 0)[0] == 34                                     # (the exact-fp32 kernel has no cap)
    # row tiles
    rows = {(c['cout'] if c['entry'].endswith('fwd') else c['cin']) for c in mc.CASES if c['name'].startswith('sk_')}
    assert {4, 60, 64, 68, 124, 128, 132} <= rows
    rows = {(c['cout'] if c['entry'].endswith('fwd') else c['cin']) for c in mc.CASES if c['name'].startswith('ha_')}
    assert {28, 32, 36, 64, 128, 132} <= rows
    # halo grids: whole 4 x 32 tiles, and (square grids) always a multiple of eight of them -- see the module docstring
    for c in mc.CASES:
        if any(l.cls == 'conv_halo' for l in mc.plan(c, 1, True)['launches']):
            assert c['res'] % 32 == 0 and (c['res'] ** 2 // mc.NT) % 8 == 0
    assert {c['res'] for c in mc.CASES if c['name'].startswith('ha_')} == {64, 96, 160}
    assert all(c['cin' if c['entry'] == 'fwd' else 'cout'] <= 40 for c in mc.CASES if c['res'] == 160)
    # ... while the flat and fp32 direct kernels see both sides of the tile-order switch
    assert [mc.ds_tiles(r) % 8 for r in (35, 36, 48, 64)] == [2, 3, 2, 0]
    # up-sampling: phase grids at and past the bound, merged launch split and direct
    assert max(gy * gx for gy, gx, _ in mc.phase_grids(33)) == 1156 and B['uf_r66']['res'] % 4 == 2
    assert min(gy * gx for gy, gx, _ in mc.phase_grids(35)) == 1225
    for p in (1, 2, 3):
        assert mc.plan(B['uf_r66'], p, True)['launches'][0][:1] + mc.plan(B['uf_r66'], p, True)['launches'][0][5:] == ('conv_splitk', True)
        assert mc.plan(B['uf_r70'], p, True)['launches'][0].cls == 'conv_flat' and B['uf_r70']['cin'] > 32
        assert mc.plan(B['uf_r128'], p, True)['launches'] == [mc.Launch('conv_flat', 64, '32x32', 1, True, True)]
        assert mc.splits(B['ub_r66'], p) and not mc.splits(B['ub_r70'], p)
    assert {c['res'] for c in mc.CASES if c['name'].startswith('uf_')} == {4, 8, 34, 66, 70, 128}
    assert {c['res'] for c in mc.CASES if c['name'].startswith('ub_')} == {4, 8, 34, 66, 70, 128}
    assert any(c['cout'] % 32 for c in mc.CASES if c['name'].startswith('ub_'))


def test_workspace_bytes_is_monotone_in_what_it_must_hold():
    """The restated la_modconv_workspace_bytes holds the pre-split copy and the partials of every plan (the GPU test compares it with the
    library's value)."""
    for c in mc.CASES:
        up = c['entry'].startswith('up2')
        full = mc.workspace_bytes(c['B'], c['cin'], c['cout'], c['res'], 1 if up else 0)
        for p in mc.PRECISIONS:
            assert mc.plan(c, p, True)['ws_bytes'] == full


def test_refusals_in_the_plan():
    c = dict(mc.BY_NAME['sk_r4_b3'], cout=6)
    with pytest.raises(mc.Refused):
        mc._run_plan(c, 0, 1 << 20)
    with pytest.raises(mc.Refused):
        mc._run_plan(dict(mc.BY_NAME['uf_r4'], res=5), 1, 1 << 20)
    with pytest.raises(mc.Refused):
        mc._run_plan(mc.BY_NAME['sk_r4_b3'], 1, 0)
    with pytest.raises(mc.Refused):
        mc._run_plan(dict(mc.BY_NAME['sk_r4_b3'], B=65, cin=4), 3, 1 << 24)
