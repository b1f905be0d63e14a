"""Float64 restatement, analytic bounds and the case table of the Gram-matrix style / content distance (csrc/la_gram.hip,
la_gram_pair_dist_f32, la_feat_style_distance, metrics.compute_style_content).  No GPU, no library: numpy only.

The restatement is the D / S form the library uses.  f is float32 [2P][C][HW], rows p and p + P are a pair; D = f1 - f2 and
S = f1 + f2 are formed IN FLOAT32 (as the kernel forms them while loading), everything after that in `dtype`:
    E = D S^T + S D^T = 2 HW (G1 - G2),   style = sum_ij E_ij^2 / (4 HW^2 C^2),   content = sum D^2 / (C HW),
with G = F F^T / HW the reference's gram_matrix (augments/criteria/nst/nst.py:7-13), style its mse_loss(G1, G2) and content its
mse_loss(f1, f2).  `reference_form` is the reference's own expression in float64, for the fixture.

Bounds (derived, not measured; u = 2^-24):
  * every entry of E from a float32 computation in ANY summation order differs from the float64 value on the same D, S by at most
        dE_ij = (2 HW + 2) u A_ij,    A_ij = sum_k (|D_ik S_jk| + |S_ik D_jk|):
    the dot-product bound for 2 HW terms -- a product is rounded once and then passes through at most 2 HW + 1 further additions (the
    2 HW - 1 of its chain and, where K is split into ks slices, ks - 1 slice additions: 2 HW / ks + ks <= 2 HW + 2).
  * style: |sum E'^2 - sum E^2| <= sum (2 |E| dE + dE^2), divided by the same denominator, plus (C^2 + 2) 2^-53 style for the float64
    squares, sum and division.
  * content: D is the same float32 value on both sides, its square is exact in float64: (C HW + 2) 2^-53 content for the sum and division.
Integer inputs in -2 .. 2: |D|, |S| <= 4, so |E| <= 32 HW; with 32 HW < 2^24 every float32 partial sum is an exact integer and with
C^2 (32 HW)^2 < 2^53 the float64 sum of squares is exact in any order: the result is the restatement's bit for bit.
"""
import numpy as np

TILE, TILE_SMALL, KC = 128, 64, 16  # la_gram.hip: GRAM_T, GRAM_TS (the tile edge for C <= 64), GRAM_KC
SLICE_CHUNKS, PAIR_WGS = 32, 128    # GRAM_PER, GRAM_WGS
U32, U64 = 2.0 ** -24, 2.0 ** -53

HW_SPLIT = 1110                     # 70 chunks: 3 slices of 24, 24 and 22 chunks, the last chunk 6 k wide
CHANNELS = (4, 12, TILE_SMALL, TILE_SMALL + 1, TILE, TILE + 4, 2 * TILE + 4)
# ragged single small tile; exactly one small tile; the first C of the 128 tile (ragged, three active waves); exactly one tile; one
# plus 4 (two tile rows: an off-diagonal tile); three tile rows
PIXELS = (1, 4, 9, 33, HW_SPLIT)
PAIRS = (1, 3)
CASES = [(C, HW) for C in CHANNELS for HW in PIXELS]


def slices(C, HW):
    """(ks, chunks per slice, chunks) as la_gram.hip's gram_plan splits K = HW: a function of (C, HW) only."""
    edge = TILE_SMALL if C <= TILE_SMALL else TILE
    T = -(-C // edge)
    ntile = T * (T + 1) // 2
    nchunk = -(-HW // KC)
    want = min(-(-nchunk // SLICE_CHUNKS), max(1, PAIR_WGS // ntile))
    per = -(-nchunk // want)
    return -(-nchunk // per), per, nchunk


def split(f):
    """D, S [P][C][HW] in float32 from f float32 [2P][C][HW]."""
    f = np.asarray(f)
    assert f.dtype == np.float32 and f.ndim == 3 and f.shape[0] % 2 == 0
    P = f.shape[0] // 2
    return f[:P] - f[P:], f[:P] + f[P:]


def gram_diff(D, S, dtype):
    D, S = D.astype(dtype), S.astype(dtype)
    return np.matmul(D, S.transpose(0, 2, 1)) + np.matmul(S, D.transpose(0, 2, 1))


def restate(f, dtype=np.float64):
    """(style [P], content [P]) in `dtype` (the division in float64)."""
    D, S = split(f)
    C, HW = D.shape[1], D.shape[2]
    E = gram_diff(D, S, dtype)
    style = (E * E).sum(axis=(1, 2), dtype=dtype).astype(np.float64) / (4.0 * HW * HW * C * C)
    Dd = D.astype(dtype)
    content = (Dd * Dd).sum(axis=(1, 2), dtype=dtype).astype(np.float64) / float(C * HW)
    return style, content


def bounds(f):
    """(style bound [P], content bound [P]) of a float32 computation against restate(f, float64): see the module docstring."""
    D, S = split(f)
    C, HW = D.shape[1], D.shape[2]
    Dd, Sd = np.abs(D.astype(np.float64)), np.abs(S.astype(np.float64))
    A = np.matmul(Dd, Sd.transpose(0, 2, 1)) + np.matmul(Sd, Dd.transpose(0, 2, 1))
    dE = (2 * HW + 2) * U32 * A
    E = np.abs(gram_diff(D, S, np.float64))
    style, content = restate(f)
    sb = (2.0 * E * dE + dE * dE).sum(axis=(1, 2)) / (4.0 * HW * HW * C * C) + (C * C + 2) * U64 * style
    return sb, (C * HW + 2) * U64 * content


def restate_pair64(f1, f2):
    """The D / S form on float64 activations [C][HW] of one pair (D and S in float64 too): (style, content)."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    C, HW = f1.shape
    D, S = f1 - f2, f1 + f2
    E = D @ S.T + S @ D.T
    return float((E * E).sum() / (4.0 * HW * HW * C * C)), float((D * D).sum() / float(C * HW))


def reference_form(f1, f2):
    """The reference's own expressions on float64 activations [C][HW]: mse(G1, G2) with G = F F^T / HW, and mse(f1, f2)."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    HW = f1.shape[1]
    G1, G2 = f1 @ f1.T / HW, f2 @ f2.T / HW
    return float(((G1 - G2) ** 2).mean()), float(((f1 - f2) ** 2).mean())


def int_inputs(C, HW, P, seed=0):
    """float32 [2P][C][HW] of integers in -2 .. 2."""
    rng = np.random.default_rng([seed, C, HW, 1])
    return rng.integers(-2, 3, size=[2 * P, C, HW]).astype(np.float32)


def float_inputs(C, HW, seed=0):
    """float32 [6][C][HW], three pairs: pair 0 is close (y = x + 1e-3 noise), pair 1 independent, pair 2 identical (y = x)."""
    rng = np.random.default_rng([seed, C, HW, 2])
    x = rng.standard_normal([3, C, HW]).astype(np.float32)
    y = rng.standard_normal([3, C, HW]).astype(np.float32)
    y[0] = x[0] + np.float32(1e-3) * y[0]
    y[2] = x[2]
    return np.concatenate([x, y])


# ---- the narrow VGG19 of tests/golden/nst.npz on the host, for the fixture check of the restatement ----
CONV_IDS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
TAP_AFTER = (0, 5, 10, 19, 28)
POOL_AFTER = (2, 7, 16, 25)


def fixture_state_dict(fx):
    import torch
    return {k: torch.tensor(fx[k]) for k in fx.files if k.startswith('features.')}


def fixture_taps(fx, img, mode):
    """The five tapped activations (float64 torch, [C][HW] each) of modality `mode` of img [2][R][R] through the fixture's net:
    prepare_img(synthetic=True, normalize=True) of the reference, then conv + ReLU / max pool with a tap after the convs TAP_AFTER."""
    import torch
    import torch.nn.functional as F
    x = (torch.as_tensor(img, dtype=torch.float64)[mode] * 127.5 + 128).clamp(0, 255) / 255.0
    x = x[None, None].repeat(1, 3, 1, 1)
    taps = []
    for i in CONV_IDS:
        x = torch.relu(F.conv2d(x, torch.tensor(fx[f'features.{i}.weight'], dtype=torch.float64),
                                torch.tensor(fx[f'features.{i}.bias'], dtype=torch.float64), padding=1))
        if i in TAP_AFTER:
            taps.append(x[0].reshape(x.shape[1], -1))
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 2)
    return taps
