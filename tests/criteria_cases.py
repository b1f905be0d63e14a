"""Case tables, seeded input generators and float64 restatements for the criteria, metric and loop-primitive kernels
(la_criteria.hip, la_metrics.hip, la_mapping.hip, la_crop_repeat_*, la_adam_step_f32).  Shared by test_criteria_cases_cpu.py (which
proves, without a GPU, that the tables reach what they claim and that the restatements are right) and by test_hip_criteria_shapes.py /
test_hip_metric_shapes.py.  Nothing here reads a file; every input is synthetic and seeded.

Two kinds of input per kernel.  EXACT: small integers, every float32 partial sum an integer below 2^24, so the result does not depend
on the summation order and the kernel must return exactly the float64 answer.  FLOAT: non-zero mean, mixed signs; the error budget is
`budget()` below: 4 x the error of the same restatement run in float32 on the CPU (worst element of the case) + one float32 rounding
of the largest term.  The float32 CPU run sets the budget, never the kernel."""
import numpy as np

TWO24 = float(2 ** 24)
EPS32 = 2.0 ** -23


def cdiv(a, b):
    return -(-a // b)


def budget(ref32, ref64, floor):
    """4 x (worst float32-restatement error) + floor"""
    return 4.0 * float(np.max(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)))) + float(floor)


# ---------------------------------------------------------------------------------------------------------------------------------
# pairwise squared L2 (la_pairwise_l2_f32)

L2_RB, L2_NCH, L2_KSPLIT = 8, 8, 16          # la_criteria.hip: RB, NCH, KSPLIT
L2_K = [1, 3, 4, 255, 256, 257, 1024, 1025, 1028, 4096, 4100, 16384, 16385, 16388, 32761]
L2_NM = [(1, 1), (7, 9), (8, 8), (9, 7), (17, 64)]
L2_PREDICATE_PAIR = [(3, 1016, 16388), (3, 1017, 16388)]          # (n, m, K): cdiv(m, 8) * 4 = 508 < 512 and = 512


def l2_plan(K, n, m, aligned=True):
    """Host-side restatement of la_bank_dot's launch: which kernel form, how many K slices, where they begin and end, how many passes
    over the query rows.  It only names cases and proves coverage; it never produces an expected value."""
    vec = K % 4 == 0 and aligned
    V = 4 if vec else 1
    ksplit = L2_KSPLIT if (K > 16384 and cdiv(m, L2_RB) * 4 < 512) else 4
    kper = cdiv(cdiv(K, ksplit), 256 * V) * 256 * V
    occ = ''
    for ks in range(ksplit):
        beg, end = ks * kper, min(ks * kper + kper, K)
        occ += 'E' if beg >= K else ('F' if end - beg == kper else 'P')
    return dict(vec=vec, ksplit=ksplit, kper=kper, occupancy=occ, passes=cdiv(n, L2_NCH), ragged_n=n % L2_NCH != 0, ragged_m=m % L2_RB != 0)


def _occ_words(occ):
    w = []
    if 'F' in occ:
        w.append('full')
    if 'P' in occ:
        w.append('partial')
    if 'E' in occ:
        w.append('empty')
    return '+'.join(w) + '-slice'


def l2_case_id(K, n, m, aligned=True):
    p = l2_plan(K, n, m, aligned)
    parts = [f'K{K}', 'vec' if p['vec'] else ('scalar' if aligned else 'scalar-unaligned'), f'ks{p["ksplit"]}', _occ_words(p['occupancy']),
             f'n{n}' + ('' if p['passes'] == 1 else f'-{p["passes"]}chunks') + ('-ragged' if p['ragged_n'] else ''),
             f'm{m}' + ('-ragged' if p['ragged_m'] else '')]
    return '-'.join(parts)


L2_CASES = [(K, n, m) for K in L2_K for (n, m) in L2_NM]


def l2_inputs(K, n, m, kind, seed=0):
    """(X [n][K], Y [m][K]) float32.  'exact': integers in -3..3 (every entry of D at most 36 K, every norm at most 9 K);
    'float': normal, X around +0.3 and Y around -0.2 (non-zero mean, mixed signs)."""
    rs = np.random.RandomState([K % 65536, n, m, seed, 0 if kind == 'exact' else 1])
    if kind == 'exact':
        return rs.randint(-3, 4, size=[n, K]).astype(np.float32), rs.randint(-3, 4, size=[m, K]).astype(np.float32)
    return (rs.standard_normal([n, K]) + 0.3).astype(np.float32), (rs.standard_normal([m, K]) * 1.5 - 0.2).astype(np.float32)


def l2_restate(X, Y, dtype):
    """l2_loss_vectorized in GEMM form, every operation in `dtype`: (D [m][n], mean, largest |Y_m|^2 + |X_n|^2)"""
    n, m = X.shape[0], Y.shape[0]
    Xf, Yf = X.reshape(n, -1).astype(dtype), Y.reshape(m, -1).astype(dtype)
    YY, XX = (Yf * Yf).sum(1, dtype=dtype), (Xf * Xf).sum(1, dtype=dtype)
    YX = Yf @ Xf.T
    D = (YY[:, None] + XX[None, :]) - dtype(2) * YX
    mean = D.sum(dtype=dtype) / dtype(m * n) / dtype(Xf.shape[1])
    return D, mean, float(YY.max()) + float(XX.max())


def l2_direct(X, Y):
    """sum_k (Y_mk - X_nk)^2 in float64: the definition the GEMM form restates"""
    n, m = X.shape[0], Y.shape[0]
    Xf, Yf = X.reshape(n, -1).astype(np.float64), Y.reshape(m, -1).astype(np.float64)
    return np.stack([((Yf - Xf[j]) ** 2).sum(1) for j in range(n)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# precision / recall kernels on float16 features (la_pr_kth_f16, la_pr_member_f16, la_cdist_f16)

PR_KMAX = 8
PR_D = [16, 48, 112]
PR_D_PADDED = 100                        # through metrics.py: padded to 112 on the host
PR_SHAPES = [(1, 9), (31, 33), (32, 32), (33, 127), (129, 128), (161, 130), (130, 257)]          # (rows, cols)
PR_NHOOD = [0, 1, 3, 7]
PR_CLAMP = float(np.float32(1e-30))      # the kernels clamp the squared distance here before the square root
PLANT_COLS = [0, 31, 32, 127, 128]       # and nc - 1


def pr_case_id(D, nr, nc):
    w = [f'D{D}', f'r{nr}', f'c{nc}']
    if nr < 32:
        w.append('lt32rows')
    if nr > 128:
        w.append('2blocks')
    if nc % 32 in (1, 2):          # the last one or two columns are alone in their 32- (and for 130, 257: 128-) column tile
        w.append('col-past-seam')
    return '-'.join(w)


def pr_features(n, D, seed, kind='exact'):
    """float16 [n][D].  'exact': integers in -2..2 (squared norms at most 4 D, squared distances integers at most 16 D);
    'float': detector-like, mostly positive with a negative tail, rounded to float16."""
    rs = np.random.RandomState([n, D, seed, 0 if kind == 'exact' else 1])
    if kind == 'exact':
        return rs.randint(-2, 3, size=[n, D]).astype(np.float16)
    return (np.abs(rs.standard_normal([n, D])) * 0.7 - 0.15 + 0.3 * rs.standard_normal([1, D])).astype(np.float16)


def pr_dist2(rows, cols, dtype=np.float64):
    """squared distances in torch.cdist's GEMM form |a|^2 + |b|^2 - 2 a.b from the float16 values, every operation in `dtype`"""
    a, b = rows.astype(dtype), cols.astype(dtype)
    na, nb = (a * a).sum(1, dtype=dtype), (b * b).sum(1, dtype=dtype)
    return (na[:, None] + nb[None, :]) - dtype(2) * (a @ b.T)


def pr_dist(rows, cols, dtype=np.float64):
    return np.sqrt(np.maximum(pr_dist2(rows, cols, dtype), dtype(PR_CLAMP)))


def pr_kth(manifold_rows, cols, k):
    """(k+1)-th smallest distance of every row, float64"""
    return np.sort(pr_dist(manifold_rows, cols), axis=1)[:, k]


def pr_member(probes, cols, radius):
    """any_j dist(i, j) <= radius[j] with the float64 distances"""
    return (pr_dist(probes, cols) <= np.asarray(radius, np.float64)[None, :]).any(axis=1)


def sqrt_expect32(d2):
    """float32(sqrt(float64(d2))) with the kernels' clamp: what an exact squared distance must turn into, to within 1 float32 ulp"""
    return np.sqrt(np.maximum(np.asarray(d2, np.float64), PR_CLAMP)).astype(np.float32)


def within_one_ulp(got32, want32):
    got32, want32 = np.asarray(got32, np.float32), np.asarray(want32, np.float32)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)


def member_pattern_a(probes, cols, seed):
    """Radii sqrt(q_j + 0.5), q_j = max(0, base + r_j) with r_j in -2..2: integer squared distances never lie on a boundary.  `base` is
    the integer that brings the member fraction of the float64 answer closest to one half.  With fewer than 5 probes no fraction can
    lie in a window, so two radius sets come back instead: ('admit') the nearest column of probe 0 admits it with q = d^2 exactly and
    every other column misses by one, and ('miss') every column misses every probe by one (q_j = min_i d2_ij - 1)."""
    d2 = np.rint(pr_dist2(probes, cols)).astype(np.int64)
    if probes.shape[0] < 5:
        miss = np.maximum(d2.min(axis=0) - 1, -1)          # q = -1: radius sqrt(-0.5) is not a number; use 0 radius below
        admit = miss.copy()
        j = int(np.argmin(d2[0]))
        admit[j] = d2[0, j]
        out = []
        for name, q in (('admit', admit), ('miss', miss)):
            rad = np.where(q >= 0, np.sqrt(np.maximum(q, 0) + 0.5), 0.0).astype(np.float32)
            out.append((name, rad, pr_member(probes, cols, rad)))
        return out
    r = np.random.RandomState([seed, 77]).randint(-2, 3, size=[cols.shape[0]])
    best = None
    for base in range(0, 16 * probes.shape[1] + 4):
        q = np.maximum(base + r, 0)
        frac = float((d2 <= q[None, :]).any(axis=1).mean())
        if best is None or abs(frac - 0.5) < abs(best[1] - 0.5):
            best = (q, frac)
        if frac >= 0.8:
            break
    rad = np.sqrt(best[0] + 0.5).astype(np.float32)
    return [('window', rad, pr_member(probes, cols, rad))]


def member_pattern_b(nr, cols, seed):
    """Planted: (probes, planted {probe row: column}).  The chosen probes are copies of columns nc - 1, 0, 31, 32, 127, 128 (those that
    exist, as many as there are probe rows), spread over the probe rows with the last row among them; every other probe is drawn afresh.
    With every radius sqrt(0.5) exactly the planted probes are members."""
    nc, D = cols.shape
    want = [c for c in [nc - 1] + PLANT_COLS if c < nc]
    want = list(dict.fromkeys(want))[:nr]
    probes = pr_features(nr, D, seed + 500)
    pos = sorted({int(round(i * (nr - 1) / max(len(want) - 1, 1))) for i in range(len(want))}) if nr > 1 else [0]
    planted = dict(zip(pos[::-1], want))          # the last probe row carries column nc - 1
    for i, c in planted.items():
        probes[i] = cols[c]
    return probes, planted


def member_pattern_c(nc):
    """only the last column admits anything, and it admits everything"""
    rad = np.zeros([nc], np.float32)
    rad[nc - 1] = 1e6
    return rad


# ---------------------------------------------------------------------------------------------------------------------------------
# feature moments (la_feature_moments_f64)

MOM_D = [1, 15, 16, 17, 33]
MOM_N = [1, 15, 16, 17, 50]


def mom_inputs(n, D, kind, seed=0):
    rs = np.random.RandomState([n, D, seed, 0 if kind == 'exact' else 1])
    if kind == 'exact':
        return rs.randint(-9, 10, size=[n, D]).astype(np.float32)
    return (rs.standard_normal([n, D]) * 0.8 + 0.3).astype(np.float32)          # non-zero mean, mixed signs


def mom_restate(x, mean0=None, cov0=None):
    """(raw_mean, raw_cov, sum |x|, sum |x_i x_j|) in float64; the products of two float32 values are exact in float64"""
    x64 = x.astype(np.float64)
    D = x.shape[1]
    mean = x64.sum(0) + (0 if mean0 is None else mean0)
    cov = x64.T @ x64 + (0 if cov0 is None else cov0)
    a = np.abs(x64)
    return mean.reshape(D), cov.reshape(D, D), a.sum(0), a.T @ a


# ---------------------------------------------------------------------------------------------------------------------------------
# fully connected layer and mapping network (la_fc_f32, la_mapping_forward_f32)

FC_IN = [1, 63, 64, 65, 512, 2044, 2047, 2048, 2052, 4100]
FC_OUT = [1, 4, 5]
FC_B = [1, 8, 9, 17]
FC_ACT = [(1, 'linear'), (3, 'lrelu')]          # LA_ACT_LINEAR, LA_ACT_LRELU
FC_LR_MUL = [1.0, 0.01]
FC_MB = 8                                       # la_mapping.hip: MB


def fc_plan(n_in, aligned=True):
    """which la_fc_f32 form a row length takes"""
    vec = n_in % 4 == 0 and aligned
    if vec and n_in >= 2048:
        n4 = n_in // 4
        per = cdiv(n4, 4)
        return dict(form='wide', ragged_quarter=n4 % 4 != 0, last_quarter=n4 - 3 * per)
    if vec:
        n4 = n_in // 4
        # per lane and step: does the second float4 (j + 64) exist?  'mixed' = the `two` guard is true for some loads, false for others
        two = {j + 64 < n4 for lane in range(64) for j in range(lane, n4, 128)}
        return dict(form='float4', two='mixed' if len(two) == 2 else ('all' if two == {True} else 'none'))
    return dict(form='scalar')


def fc_case_id(n_in, aligned=True):
    p = fc_plan(n_in, aligned)
    w = [f'in{n_in}', p['form']]
    if p['form'] == 'wide':
        w.append('ragged-quarter' if p['ragged_quarter'] else 'even-quarters')
    if p['form'] == 'float4':
        w.append(f'two-{p["two"]}')
    if not aligned:
        w.append('x-unaligned')
    return '-'.join(w)


def fc_inputs(B, n_in, n_out, lr_mul, seed=0):
    """x with a non-zero mean, W stored as the reference stores it (randn / lr_mul), a bias of order 1 / lr_mul"""
    rs = np.random.RandomState([B, n_in, n_out, seed])
    x = (rs.standard_normal([B, n_in]) + 0.25).astype(np.float32)
    W = (rs.standard_normal([n_out, n_in]) / lr_mul).astype(np.float32)
    b = (rs.standard_normal([n_out]) * 0.5 / lr_mul).astype(np.float32)
    return x, W, b


def fc_restate(x, W, b, lr_mul, act, alpha, gain, dtype):
    """act(x @ (W * lr_mul / sqrt(in))^T + b * lr_mul) * gain, every operation in `dtype`"""
    n_in = x.shape[1]
    w = W.astype(dtype) * dtype(dtype(lr_mul) / np.sqrt(dtype(n_in)))
    y = x.astype(dtype) @ w.T
    if b is not None:
        y = y + b.astype(dtype) * dtype(lr_mul)
    if act == 'lrelu':
        y = np.where(y > 0, y, y * dtype(alpha))
    return (y * dtype(gain)).astype(dtype)


MAP_DIMS = [(64, 64), (40, 72), (72, 40)]          # (z_dim, w_dim)
MAP_LAYERS = [0, 2, 8]
MAP_B = [1, 9]
MAP_PSI = [1.0, 0.7]
MAP_NUM_WS = [1, 6]
MAP_LR_MUL = 0.01


def map_inputs(B, z_dim, w_dim, num_layers, seed=0):
    rs = np.random.RandomState([B, z_dim, w_dim, num_layers, seed])
    z = (rs.standard_normal([B, z_dim]) + 0.1).astype(np.float32)
    dims = [z_dim] + [w_dim] * num_layers
    Ws = [(rs.standard_normal([dims[i + 1], dims[i]]) / MAP_LR_MUL).astype(np.float32) for i in range(num_layers)]
    bs = [(rs.standard_normal([dims[i + 1]]) * 0.3 / MAP_LR_MUL).astype(np.float32) for i in range(num_layers)]
    w_avg = (rs.standard_normal([dims[-1]]) * 0.5).astype(np.float32)
    return z, Ws, bs, w_avg


def map_restate(z, Ws, bs, w_avg, psi, num_ws, dtype):
    """x = z * rsqrt(mean(z^2) + 1e-8); per layer x = lrelu(fc(x)) * sqrt(2); broadcast to num_ws; psi != 1 and a w_avg given:
    w_avg + psi * (x - w_avg).  Without a w_avg there is nothing to truncate towards and the kernel leaves x as it is."""
    x = z.astype(dtype)
    x = x * (dtype(1) / np.sqrt((x * x).mean(1, keepdims=True, dtype=dtype) + dtype(1e-8)))
    for W, b in zip(Ws, bs):
        x = fc_restate(x, W, b, MAP_LR_MUL, 'lrelu', 0.2, np.sqrt(dtype(2)), dtype)
    x = np.repeat(x[:, None, :], num_ws, axis=1)
    if psi != 1 and w_avg is not None:
        wa = w_avg.astype(dtype)
        x = wa + dtype(psi) * (x - wa)
    return x.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# crops and Adam

CENTER_CROP = [(32, 23, 5), (33, 23, 5), (16, 16, 0), (16, 1, 15)]          # (R, cc, off)
CENTER_PLANES = [1, 6]
CROP_REP = [1, 3, 4]
CROP_IMGC = [1, 2]
CROP_B = [1, 3]
CROP_WINDOWS = [(13, 6, 3, 2), (13, 5, 8, 8), (8, 8, 0, 0)]          # (R, S, y0, x0); the second touches the last row and column
ADAM_N = [1, 256, 257, 1000]
ADAM_STEPS = 5


def center_crop_restate(src, cc, off):
    return src[:, off:off + cc, off:off + cc].copy()


def crop_repeat_restate(img, S, y0, x0, rep, scale, shift, dtype=np.float64):
    """xc[c * B + b][k][y][x] = img[b][c][y0 + y][x0 + x] * scale + shift"""
    B, imgc = img.shape[:2]
    win = img[:, :, y0:y0 + S, x0:x0 + S].astype(dtype) * dtype(scale) + dtype(shift)          # [B][imgc][S][S]
    rows = win.transpose(1, 0, 2, 3).reshape(imgc * B, 1, S, S)
    return np.repeat(rows, rep, axis=1)


def crop_repeat_grad_restate(gxc, g_img0, S, y0, x0, rep, scale, dtype=np.float64):
    """g_img[b][c][y0 + y][x0 + x] += scale * sum_k gxc[c * B + b][k][y][x]; everything else untouched"""
    B, imgc = g_img0.shape[:2]
    g = g_img0.astype(dtype).copy()
    acc = (gxc.astype(dtype) * dtype(scale)).sum(1).reshape(imgc, B, S, S).transpose(1, 0, 2, 3)
    g[:, :, y0:y0 + S, x0:x0 + S] += acc
    return g


def pr_from_features(real, gen, nhood_size):
    """compute_pr_from_features restated in float64: features rounded to float16, radii rounded to float16 as the reference keeps them
    (precision_recall.py:78), membership dist <= radius.  Also the smallest relative gap between a distance and a radius it is compared
    with and does not equal: a float32 kernel can only disagree where that gap is a few float32 ulps."""
    real, gen = np.asarray(real).astype(np.float16), np.asarray(gen).astype(np.float16)
    out, gap = {}, np.inf
    for name, manifold, probes in (('precision', real, gen), ('recall', gen, real)):
        kth = pr_kth(manifold, manifold, nhood_size).astype(np.float16)
        d = pr_dist(probes, manifold)
        r = kth.astype(np.float64)[None, :]
        rel = np.abs(d - r) / np.maximum(r, 1e-300)
        gap = min(gap, float(rel[rel > 0].min()))
        pred = (d <= r).any(axis=1)
        out[name], out[name + '_kth'], out[name + '_pred'] = float(pred.mean()), kth.astype(np.float32), pred
    out['gap'] = gap
    return out
