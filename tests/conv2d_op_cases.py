"""Case list of the conv2d_resample tests and `path_plan`, a host-side restatement of which kernel path each of a case's three
contractions takes (la_conv_op.hip: engine_ok, wgrad_slices).  It only picks shapes and proves that the case list reaches what it claims
to reach; it never produces an expected value.  Shared by test_conv2d_op_cpu.py (coverage proof, no GPU) and test_hip_conv2d_op.py."""

MAX_TAPS = 9          # LA_CONV_MAX_TAPS
WG_TILE = 128         # block tile of la_conv_wgrad_mfma_kernel (rows and columns)
WG_CHUNK = 16         # pixels of one grid row per K chunk


def _cdiv(a, b):
    return -(-a // b)


def _pad4(p):
    if isinstance(p, int):
        p = [p, p]
    p = list(p)
    if len(p) == 2:
        p = [p[0], p[0], p[1], p[1]]
    return p


def case(name, x, cout, k, up=1, down=1, padding=0, groups=1, flip_weight=True, f=(1, 3, 3, 1), flip_filter=False):
    kh, kw = (k, k) if isinstance(k, int) else k
    return dict(name=name, x=tuple(x), cout=cout, kh=kh, kw=kw, up=up, down=down, padding=padding, groups=groups, flip_weight=flip_weight,
                f=f, flip_filter=flip_filter)


# x = (N, Cin, H, W).  f: 1-D taps handed to setup_filter (fewer than 8: a dense 2-D filter), or None.
CASES = [
    case('same3x3', (2, 8, 8, 8), 8, 3, padding=1),
    case('same3x3_conv', (2, 8, 9, 8), 8, 3, padding=1, flip_weight=False),
    case('down2_3x3', (2, 8, 12, 12), 12, 3, down=2, padding=1),
    case('down2_3x3_conv', (2, 8, 12, 10), 12, 3, down=2, padding=1, flip_weight=False),
    case('up2_3x3', (2, 8, 8, 8), 8, 3, up=2, padding=1),
    case('up2_3x3_conv', (2, 8, 6, 9), 8, 3, up=2, padding=1, flip_weight=False),
    case('up2_g2', (2, 8, 8, 8), 16, 3, up=2, padding=1, groups=2),
    case('same_g2', (2, 8, 8, 8), 16, 3, padding=1, groups=2),
    case('down2_g2', (2, 8, 8, 8), 16, 3, down=2, padding=1, groups=2),
    case('same_g3', (2, 6, 8, 8), 9, 3, padding=1, groups=3),
    case('up2_g3', (2, 6, 5, 8), 9, 3, up=2, padding=1, groups=3),
    case('ragged_cout6', (2, 4, 8, 8), 6, 3, padding=1),
    case('ragged_cout6_up2', (2, 4, 8, 8), 6, 3, up=2, padding=1),
    case('ragged_cout6_down2', (2, 4, 8, 8), 6, 3, down=2, padding=1),
    case('k1', (2, 4, 8, 8), 8, 1),
    case('k1_up2', (2, 4, 8, 8), 8, 1, up=2),
    case('k1_down2', (2, 4, 8, 8), 8, 1, down=2),
    case('k1_down2_g2', (2, 8, 8, 8), 8, 1, down=2, groups=2),
    case('k1x3', (2, 4, 8, 8), 8, (1, 3), padding=[1, 1, 0, 0]),
    case('k1x3_up2', (2, 4, 8, 8), 8, (1, 3), up=2),
    case('k3x1_down2', (2, 4, 8, 8), 8, (3, 1), down=2),
    case('k5', (2, 3, 9, 9), 5, 5, padding=2),
    case('k5_conv', (2, 4, 9, 9), 4, 5, padding=2, flip_weight=False),
    case('k5_down2', (1, 3, 12, 12), 5, 5, down=2, padding=2),
    case('k7', (2, 3, 10, 10), 4, 7, padding=3),
    case('k7_up2', (1, 2, 6, 6), 4, 7, up=2, padding=3),
    case('up4', (2, 4, 5, 5), 8, 3, up=4, padding=1, f=(1, 3, 3, 1)),
    case('down4', (2, 4, 16, 16), 8, 3, down=4, padding=1),
    case('up2_down2', (2, 4, 8, 8), 8, 3, up=2, down=2, padding=1),
    case('rect', (2, 4, 10, 7), 8, 3, padding=1),
    case('rect_up2', (2, 4, 5, 11), 8, 3, up=2, padding=1),
    case('rect_down2', (2, 4, 14, 9), 8, 3, down=2, padding=1),
    case('pad_unequal', (2, 4, 8, 8), 8, 3, padding=[2, 0, 1, 3]),
    case('pad_negative', (2, 4, 10, 10), 8, 3, padding=[-1, 2, 1, -2]),
    case('pad_negative_conv', (2, 4, 10, 10), 8, 3, padding=[-1, 2, 1, -2], flip_weight=False),
    case('pad_unequal_up2', (2, 4, 6, 6), 8, 3, up=2, padding=[2, 0, 1, 3]),
    case('pad_unequal_down2', (2, 4, 12, 12), 8, 3, down=2, padding=[2, 0, 1, 3]),
    case('pad0', (2, 4, 8, 8), 8, 3),
    case('pad2_wide', (2, 4, 6, 6), 8, 3, padding=2),
    case('batch1', (1, 8, 8, 8), 8, 3, padding=1),
    case('batch1_up2', (1, 8, 8, 8), 8, 3, up=2, padding=1),
    case('chan1', (2, 1, 8, 8), 1, 3, padding=1),
    case('chan1_in', (2, 1, 8, 8), 8, 3, padding=1),
    case('chan1_out', (2, 8, 8, 8), 1, 3, padding=1),
    case('no_filter_up2', (2, 4, 6, 6), 8, 3, up=2, padding=1, f=None),
    case('flip_filter_down2', (2, 4, 12, 12), 8, 3, down=2, padding=1, f=(1, 2, 4, 1), flip_filter=True),
    case('tiles_132x144', (2, 16, 6, 6), 132, 3, padding=1),
    case('tiles_132x144_up2', (1, 16, 5, 5), 132, 3, up=2, padding=1),
    case('small_grid_splitk', (2, 64, 8, 8), 64, 3, padding=1),
    case('width40', (1, 8, 6, 40), 8, 3, padding=1),
    case('layer128_64', (4, 128, 64, 64), 128, 3, padding=1),
]
BY_NAME = {c['name']: c for c in CASES}
MANY_SLICES = 'layer128_64'
SECOND_ORDER = ('same3x3', 'k5')          # one per path
# ... and the branches that run through upfirdn2d (whose backward must itself be differentiable): up, down, both 1x1 forms, fallback
SECOND_ORDER_RESAMPLED = ('up2_3x3', 'down2_3x3', 'up2_down2', 'k1_up2', 'k1_down2', 'pad_negative', 'ragged_cout6_up2', 'k5_down2')
GRAPH_CASE = 'same3x3'


def _fir_out(size, up, down, p0, p1, taps):
    return (size * up + p0 + p1 - taps + down) // down


def conv_call(c):
    """Geometry of the ONE convolution a conv2d_resample call makes (branch structure of conv2d_resample.py:82-141): dict(branch,
    transpose, stride, cin, cout, h, w, oh, ow, kh, kw, groups, py, px)."""
    n, cin, h, w = c['x']
    cout, kh, kw, up, down, groups = c['cout'], c['kh'], c['kw'], c['up'], c['down'], c['groups']
    fw = fh = len(c['f']) if c['f'] is not None else 1
    px0, px1, py0, py1 = _pad4(c['padding'])
    if up > 1:
        px0 += (fw + up - 1) // 2; px1 += (fw - up) // 2; py0 += (fh + up - 1) // 2; py1 += (fh - up) // 2
    if down > 1:
        px0 += (fw - down + 1) // 2; px1 += (fw - down) // 2; py0 += (fh - down + 1) // 2; py1 += (fh - down) // 2
    r = dict(transpose=False, stride=1, cin=cin, cout=cout, kh=kh, kw=kw, groups=groups, n=n, py=0, px=0)
    if kw == 1 and kh == 1 and down > 1 and up == 1:
        r.update(branch='k1_down', h=_fir_out(h, 1, down, py0, py1, fh), w=_fir_out(w, 1, down, px0, px1, fw))
    elif kw == 1 and kh == 1 and up > 1 and down == 1:
        r.update(branch='k1_up', h=h, w=w)
    elif down > 1 and up == 1:
        r.update(branch='down', stride=down, h=_fir_out(h, 1, 1, py0, py1, fh), w=_fir_out(w, 1, 1, px0, px1, fw))
    elif up > 1:
        px0 -= kw - 1; px1 -= kw - up; py0 -= kh - 1; py1 -= kh - up
        r.update(branch='up', transpose=True, stride=up, h=h, w=w, px=max(min(-px0, -px1), 0), py=max(min(-py0, -py1), 0))
    elif px0 == px1 and py0 == py1 and px0 >= 0 and py0 >= 0:
        r.update(branch='plain', h=h, w=w, py=py0, px=px0)
    else:
        r.update(branch='fallback', h=h + py0 + py1, w=w + px0 + px1)
    if r['transpose']:
        r['oh'] = (r['h'] - 1) * r['stride'] - 2 * r['py'] + kh
        r['ow'] = (r['w'] - 1) * r['stride'] - 2 * r['px'] + kw
    else:
        r['oh'] = (r['h'] + 2 * r['py'] - kh) // r['stride'] + 1
        r['ow'] = (r['w'] + 2 * r['px'] - kw) // r['stride'] + 1
    return r


def engine_ok(op, cout, kh, kw, stride, groups):
    """op 'y': forward / data gradient (the engine writes whole 4-row groups of output channels); 'w': weight gradient."""
    if kh * kw > MAX_TAPS or stride > 2:
        return False
    return op == 'w' or (cout // groups) % 4 == 0


def wgrad_slices(nchunk, tiles):
    ks = min(_cdiv(1024, tiles), 64, max(nchunk // 8, 1))
    per = _cdiv(nchunk, ks)
    return _cdiv(nchunk, per)


def path_plan(c):
    """-> dict(call=conv_call(c), fwd=, dgrad=, wgrad= 'engine' | 'generic', slices=K slices of an engine weight gradient or 0)."""
    g = conv_call(c)
    k = (g['kh'], g['kw'], g['stride'], g['groups'])
    plan = dict(call=g, fwd='engine' if engine_ok('y', g['cout'], *k) else 'generic',
                dgrad='engine' if engine_ok('y', g['cin'], *k) else 'generic',
                wgrad='engine' if engine_ok('w', g['cout'], *k) else 'generic', slices=0)
    if plan['wgrad'] == 'engine':
        # rows = channels of the tensor on the strided grid (dy of a conv, x of a transposed conv), columns = the other's channels x taps
        a, e, gh, gw = (g['cin'], g['cout'], g['h'], g['w']) if g['transpose'] else (g['cout'], g['cin'], g['oh'], g['ow'])
        tiles = _cdiv(a // g['groups'], WG_TILE) * _cdiv(e // g['groups'] * g['kh'] * g['kw'], WG_TILE) * g['groups']
        plan['slices'] = wgrad_slices(g['n'] * gh * _cdiv(gw, WG_CHUNK), tiles)
    return plan
