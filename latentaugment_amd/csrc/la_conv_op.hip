// conv2d / conv_transpose2d of the op layer (the pair under the reference's conv2d_resample: torch_utils/ops/conv2d_gradfix.py) with
// data and weight gradients, float32 NCHW.  Written for gfx950 only.
//
//   la_conv2d_f32        y = conv(x, w) or conv_transpose(x, w); the data gradient is the same entry with `transpose` toggled
//   la_conv2d_wgrad_f32  dW = sum over batch and output pixels of dy (x) shifted x -- a GEMM with a small result and a very long
//                        reduction: LDS-staged fp32 MFMA tiles, K split over workgroups, slices summed in a fixed order (no atomics)
//
// Two paths each, chosen on the host (la_conv2d_uses_engine):
//   engine   kh*kw <= 9 taps, stride 1 or 2 (forward / data gradient also: output channels per group a multiple of 4, because the
//            engine writes whole 4-row groups).  Forward / data gradient go through la_conv_launch (la_conv.h) as raw launches on the exact
//            fp32 MFMA with weights packed per call into the workspace; stride-2 transposed forms run as one launch per output phase.
//            The weight gradient runs la_conv_wgrad_mfma_kernel below.
//   generic  kernels up to 7x7, strides up to 8, any groups / channel counts: one thread per output (forward), one workgroup per
//            dW element with a fixed-order tree reduction (weight gradient); double accumulators.  Correct, not fast.
#include "la_conv.h"
#include "la_f32_tile.h"
#include <string.h>

#define LA_OP_MAX_K 7
#define LA_OP_MAX_STRIDE 8
#define LA_OP_FWD 0
#define LA_OP_WGRAD 1

namespace {

struct Geo {
    int B, Cin, H, W, Cout, kh, kw, Ho, Wo, s, py, px, groups, corr, transpose;
};

int check_geo(const Geo& g) {
    LA_CHECK_ARG(g.B > 0 && g.Cin > 0 && g.H > 0 && g.W > 0 && g.Cout > 0 && g.kh > 0 && g.kw > 0, "conv2d: empty shape");
    LA_CHECK_ARG(g.groups >= 1 && g.Cin % g.groups == 0 && g.Cout % g.groups == 0, "conv2d: groups must divide both channel counts");
    LA_CHECK_ARG(g.kh <= LA_OP_MAX_K && g.kw <= LA_OP_MAX_K, "conv2d: kernel larger than 7x7 (limit of the generic path)");
    LA_CHECK_ARG(g.s >= 1 && g.s <= LA_OP_MAX_STRIDE, "conv2d: stride must be 1..8 (limit of the generic path)");
    LA_CHECK_ARG(g.py >= 0 && g.px >= 0, "conv2d: negative padding");
    LA_CHECK_ARG(g.Ho >= 1 && g.Wo >= 1, "conv2d: output smaller than 1x1");
    if (!g.transpose) {
        LA_CHECK_ARG(g.H + 2 * g.py >= g.kh && g.W + 2 * g.px >= g.kw, "conv2d: output smaller than 1x1");
        LA_CHECK_ARG(g.Ho == (g.H + 2 * g.py - g.kh) / g.s + 1 && g.Wo == (g.W + 2 * g.px - g.kw) / g.s + 1,
                     "conv2d: output size must be (H + 2p - k) / stride + 1");
    } else {
        const int by = (g.H - 1) * g.s - 2 * g.py + g.kh, bx = (g.W - 1) * g.s - 2 * g.px + g.kw;
        LA_CHECK_ARG(by >= 1 && bx >= 1, "conv2d: output smaller than 1x1");
        LA_CHECK_ARG(g.Ho >= by && g.Ho < by + g.s && g.Wo >= bx && g.Wo < bx + g.s,
                     "conv2d: transposed output size must be (H - 1) * stride - 2p + k (+ less than one stride of output padding)");
    }
    LA_CHECK_ARG((long)g.H * g.W < (1L << 31) && (long)g.Ho * g.Wo < (1L << 31), "conv2d: plane too large");
    return LA_OK;
}

bool engine_ok(int op, int cout, int kh, int kw, int stride, int groups) {
    if (kh * kw > LA_CONV_MAX_TAPS || stride > 2) return false;
    return op == LA_OP_WGRAD || (cout / groups) % 4 == 0;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---------------------------------------------------------------------------------------------- generic forward
// non-transposed: y[b,m,oy,ox] = sum w[m,c,ky,kx] x[b,c,oy*s-py+ky,ox*s-px+kx];  transposed: the adjoint, w [Cin][Cout/groups][kh][kw]
__global__ __launch_bounds__(256) void la_conv_generic_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, Geo g) {
    const long total = (long)g.B * g.Cout * g.Ho * g.Wo;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % g.Wo);
    const int oy = (int)((idx / g.Wo) % g.Ho);
    const int m = (int)((idx / ((long)g.Wo * g.Ho)) % g.Cout);
    const int b = (int)(idx / ((long)g.Wo * g.Ho * g.Cout));
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const int grp = m / Mg, mm = m - grp * Mg;
    const int taps = g.kh * g.kw;
    double acc = 0.0;
    for (int c = 0; c < Cg; ++c) {
        const int cin = grp * Cg + c;
        const float* xp = x + ((long)b * g.Cin + cin) * g.H * g.W;
        const float* wp = g.transpose ? w + ((long)cin * Mg + mm) * taps : w + ((long)m * Cg + c) * taps;
        for (int ky = 0; ky < g.kh; ++ky) {
            int iy;
            if (!g.transpose) iy = oy * g.s - g.py + ky;
            else {
                const int t = oy + g.py - ky;
                if (t < 0 || t % g.s) continue;
                iy = t / g.s;
            }
            if (iy < 0 || iy >= g.H) continue;
            for (int kx = 0; kx < g.kw; ++kx) {
                int ix;
                if (!g.transpose) ix = ox * g.s - g.px + kx;
                else {
                    const int t = ox + g.px - kx;
                    if (t < 0 || t % g.s) continue;
                    ix = t / g.s;
                }
                if (ix < 0 || ix >= g.W) continue;
                const int wi = g.corr ? ky * g.kw + kx : taps - 1 - (ky * g.kw + kx);
                acc += (double)wp[wi] * (double)xp[(long)iy * g.W + ix];
            }
        }
    }
    y[idx] = (float)acc;
}

// ---------------------------------------------------------------------------------------------- weight gradient, both paths
// P [B][A][Gh][Gw] is the tensor on the convolution's strided grid (dy of a conv, x of a transposed conv), Q [B][E][Qh][Qw] the other one:
//   dW[a][e][ky][kx] = sum_{b,gy,gx} P[b,a,gy,gx] * Q[b, grp(a)*Eg + e, gy*s - py + ky, gx*s - px + kx]      (zero outside Q)
struct WgArgs {
    const float* P; const float* Q; float* dw; float* part;
    int B, A, E, Ag, Eg, Gh, Gw, Qh, Qw, kh, kw, s, py, px, groups, corr;
    int N;              // Eg * kh * kw: columns of one group's GEMM
    int xc;             // 16-pixel chunks per grid row
    long nchunk;        // B * Gh * xc
    int per, ks;        // chunks per K slice, slices
    int mtiles, ntiles;
};

__global__ __launch_bounds__(256) void la_conv_generic_wgrad_kernel(WgArgs a) {
    __shared__ double red[256];
    const int taps = a.kh * a.kw;
    const long el = blockIdx.x;                       // (a, e, ky, kx)
    const int t = (int)(el % taps);
    const int e = (int)((el / taps) % a.Eg);
    const int ch = (int)(el / ((long)taps * a.Eg));
    const int grp = ch / a.Ag;
    const int ky = t / a.kw, kx = t - ky * a.kw;
    const long K = (long)a.B * a.Gh * a.Gw;
    double acc = 0.0;
    for (long k = threadIdx.x; k < K; k += 256) {
        const int gx = (int)(k % a.Gw);
        const int gy = (int)((k / a.Gw) % a.Gh);
        const int b = (int)(k / ((long)a.Gw * a.Gh));
        const int iy = gy * a.s - a.py + ky, ix = gx * a.s - a.px + kx;
        if (iy < 0 || iy >= a.Qh || ix < 0 || ix >= a.Qw) continue;
        acc += (double)a.P[(((long)b * a.A + ch) * a.Gh + gy) * a.Gw + gx] *
               (double)a.Q[(((long)b * a.E + grp * a.Eg + e) * a.Qh + iy) * a.Qw + ix];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {               // fixed-order tree: the same bits every run
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.dw[((long)ch * a.Eg + e) * taps + (a.corr ? t : taps - 1 - t)] = (float)red[0];
}

// MFMA path.  Per group a GEMM  dW[Ag][N] = Pm[Ag][K] * Qm[K][N],  K = (b, gy, gx) flattened, N = (e, ky, kx).
// Workgroup = 256 threads = 4 waves (2 x 2), block tile 128 x 128, every wave 64 x 64 as 2 x 2 v_mfma_f32_32x32x2_f32 tiles.  K is walked in
// chunks of 16 consecutive pixels of ONE grid row (so a chunk's loads are 64-byte runs of P and, at stride 1, of Q, and the row / sample
// decode is once per chunk, not per element); chunks beyond the row's end, image edges and padding load zeros, ragged Ag / N tails are
// masked.  The next chunk's global loads are in flight while the current one feeds the MFMAs (register staging, two LDS buffers, one
// barrier per chunk: la_tile_pipeline of la_f32_tile.h).  LDS rows are [k][128 + 4] floats: the MFMA operand reads (32 consecutive floats per
// half-wave) and the loader's transposing writes (lane = k, 4-float row step) both spread over all banks.
// blockIdx = (n tile * mtiles + m tile, group, K slice); the slice's raw tile goes to part[slice][group][Ag][N].
#define WG_T 128
#define WG_KC 16
#define WG_LD (WG_T + 4)
#define WG_RPT (WG_T / 16)     // rows per thread of each operand tile

__global__ __launch_bounds__(256) void la_conv_wgrad_mfma_kernel(WgArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][WG_KC][WG_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][WG_KC][WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int mt = blockIdx.x % a.mtiles, nt = blockIdx.x / a.mtiles;
    const int grp = blockIdx.y;
    const int m0 = mt * WG_T, n0 = nt * WG_T;
    const int taps = a.kh * a.kw;
    const long GHW = (long)a.Gh * a.Gw, QHW = (long)a.Qh * a.Qw;

    // loader roles: lane = pixel of the chunk, 8 rows of each operand per thread
    const int kk = tid & (WG_KC - 1), r0 = tid >> 4;
    long poff[WG_RPT], qoff[WG_RPT];
    int qdy[WG_RPT], qdx[WG_RPT];
    bool pok[WG_RPT], qok[WG_RPT];
#pragma unroll
    for (int j = 0; j < WG_RPT; ++j) {
        const int m = m0 + r0 + 16 * j;
        pok[j] = m < a.Ag;
        poff[j] = (long)(grp * a.Ag + (pok[j] ? m : 0)) * GHW;
        const int n = n0 + r0 + 16 * j;
        qok[j] = n < a.N;
        const int nn = qok[j] ? n : 0;
        const int e = nn / taps, t = nn - e * taps;
        const int ky = t / a.kw, kx = t - ky * a.kw;
        qoff[j] = (long)(grp * a.Eg + e) * QHW;
        qdy[j] = ky - a.py; qdx[j] = kx - a.px;
    }

    long c_beg, c_end;
    la_slice_range<long>(blockIdx.z, a.per, a.nchunk, &c_beg, &c_end);

    float areg[WG_RPT], breg[WG_RPT];
    auto prefetch = [&](long ci) {
        const int xi = (int)(ci % a.xc);
        const long row = ci / a.xc;
        const int gy = (int)(row % a.Gh);
        const int b = (int)(row / a.Gh);
        const int gx = xi * WG_KC + kk;
        const bool pv = gx < a.Gw;
        const float* Pb = a.P + (long)b * a.A * GHW + (long)gy * a.Gw + gx;
        const float* Qb = a.Q + (long)b * a.E * QHW;
        const int iy0 = gy * a.s, ix0 = gx * a.s;
#pragma unroll
        for (int j = 0; j < WG_RPT; ++j) {
            float v = 0.f;
            if (pv && pok[j]) v = Pb[poff[j]];
            areg[j] = v;
        }
#pragma unroll
        for (int j = 0; j < WG_RPT; ++j) {
            const int iy = iy0 + qdy[j], ix = ix0 + qdx[j];
            float v = 0.f;
            if (pv && qok[j] && iy >= 0 && iy < a.Qh && ix >= 0 && ix < a.Qw) v = Qb[qoff[j] + (long)iy * a.Qw + ix];
            breg[j] = v;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < WG_RPT; ++j) {
            As[buf][kk][r0 + 16 * j] = areg[j];
            Bs[buf][kk][r0 + 16 * j] = breg[j];
        }
    };

    la_f32x16 acc[2][2];
    la_f32_tile_zero(acc);
    la_tile_pipeline(c_beg, c_end, prefetch, stage,
                     [&](int buf, long) { la_f32_tile_mma<WG_KC>(As, Bs, buf, wm * 64, wn * 64, l31, lh, acc); });

    float* part = a.part + ((long)blockIdx.z * a.groups + grp) * a.Ag * a.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + l31;
            if (n >= a.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + la_mfma32_row(r, lh);
                if (m < a.Ag) part[(long)m * a.N + n] = acc[i][j][r];
            }
        }
}

// second pass of the split: slices summed in slice order (bit-identical from run to run), result written in the weight's own layout
__global__ __launch_bounds__(256) void la_conv_wgrad_finish_kernel(WgArgs a) {
    const long total = (long)a.groups * a.Ag * a.N;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const float s = la_slices_sum(a.part, idx, total, a.ks);
    const int taps = a.kh * a.kw;
    const int n = (int)(idx % a.N);
    const long ch = idx / a.N;                        // grp * Ag + m
    const int e = n / taps, t = n - e * taps;
    a.dw[(ch * a.Eg + e) * taps + (a.corr ? t : taps - 1 - t)] = s;
}

// K slices of the MFMA weight gradient: enough workgroups for ~4 per CU of a 256-CU device, at most 64 slices (the partials are
// ks copies of dW) and at least 8 chunks (128 pixels) per slice.  `upper` = the bound used to size the workspace (monotone in nchunk).
int wgrad_slices(long nchunk, int tiles, bool upper) {
    long ks = la_cdiv(1024, tiles);
    if (ks > 64) ks = 64;
    const long by_len = nchunk / 8 > 1 ? nchunk / 8 : 1;
    if (ks > by_len) ks = by_len;
    if (ks < 1) ks = 1;
    if (upper) return (int)ks;
    const long per = (nchunk + ks - 1) / ks;
    return (int)((nchunk + per - 1) / per);
}

void wgrad_shape(const Geo& g, WgArgs& a) {
    memset(&a, 0, sizeof(a));
    a.B = g.B; a.kh = g.kh; a.kw = g.kw; a.s = g.s; a.py = g.py; a.px = g.px; a.groups = g.groups; a.corr = g.corr;
    if (!g.transpose) { a.A = g.Cout; a.Gh = g.Ho; a.Gw = g.Wo; a.E = g.Cin; a.Qh = g.H; a.Qw = g.W; }
    else { a.A = g.Cin; a.Gh = g.H; a.Gw = g.W; a.E = g.Cout; a.Qh = g.Ho; a.Qw = g.Wo; }
    a.Ag = a.A / g.groups; a.Eg = a.E / g.groups;
    a.N = a.Eg * g.kh * g.kw;
    a.xc = la_cdiv(a.Gw, WG_KC);
    a.nchunk = (long)a.B * a.Gh * a.xc;
    a.mtiles = la_cdiv(a.Ag, WG_T); a.ntiles = la_cdiv(a.N, WG_T);
    a.ks = wgrad_slices(a.nchunk, a.mtiles * a.ntiles * a.groups, false);
    a.per = (int)((a.nchunk + a.ks - 1) / a.ks);
}

// ---------------------------------------------------------------------------------------------- engine forward
// w -> [group][tap][Cg][Mg] (the engine's tap-major A operand), tap = ky * kw + kx of the correlation the launch runs
__global__ __launch_bounds__(256) void la_conv_op_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int groups, int Cg, int Mg, int taps, int corr,
                                                             int transpose) {
    const long total = (long)groups * taps * Cg * Mg;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int m = (int)(idx % Mg);
    const int c = (int)((idx / Mg) % Cg);
    const int t = (int)((idx / ((long)Mg * Cg)) % taps);
    const int grp = (int)(idx / ((long)Mg * Cg * taps));
    const int tt = corr ? t : taps - 1 - t;
    wp[idx] = transpose ? w[(((long)grp * Cg + c) * Mg + m) * taps + tt] : w[(((long)grp * Mg + m) * Cg + c) * taps + tt];
}

size_t engine_fwd_splitk_bytes(const Geo& g) {
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups;
    const bool phases = g.transpose && g.s == 2;
    const int Gy = phases ? (g.Ho + 1) / 2 : g.Ho, Gx = phases ? (g.Wo + 1) / 2 : g.Wo;
    const int Bl = g.groups > 1 ? 1 : g.B;
    long fl = 0;
    for (int b = 1; b <= Bl; ++b) {                   // (the slice count falls as the batch grows: size for the largest product)
        const long f = la_conv_splitk_floats(b, Mg, Cg, Gy, Gx, LA_PREC_F32);
        if (f > fl) fl = f;
    }
    return (size_t)fl * sizeof(float);
}

size_t workspace_bytes(int op, const Geo& g) {
    if (!engine_ok(op, g.Cout, g.kh, g.kw, g.s, g.groups)) return 16;
    if (op == LA_OP_FWD) return align16((size_t)g.Cin / g.groups * g.Cout * g.kh * g.kw * sizeof(float)) + engine_fwd_splitk_bytes(g) + 16;
    WgArgs a;
    wgrad_shape(g, a);
    const int ks = wgrad_slices(a.nchunk, a.mtiles * a.ntiles * a.groups, true);
    return (size_t)ks * a.groups * a.Ag * a.N * sizeof(float) + 16;
}

int engine_forward(const Geo& g, const float* x, const float* w, float* y, void* ws, size_t ws_bytes, hipStream_t stream) {
    const int Cg = g.Cin / g.groups, Mg = g.Cout / g.groups, taps = g.kh * g.kw;
    float* wp = static_cast<float*>(ws);
    const size_t pack_bytes = align16((size_t)g.groups * taps * Cg * Mg * sizeof(float));
    const long npack = (long)g.groups * taps * Cg * Mg;
    hipLaunchKernelGGL(la_conv_op_pack_kernel, dim3(la_cdiv(npack, 256)), dim3(256), 0, stream, w, wp, g.groups, Cg, Mg, taps, g.corr, g.transpose);
    LA_CHECK_LAUNCH();
    const bool phases = g.transpose && g.s == 2;
    // a 1-tap axis at stride 2 leaves output phases that no tap reaches: they are zeros
    if (phases && (g.kh == 1 || g.kw == 1)) LA_HIP(hipMemsetAsync(y, 0, (size_t)g.B * g.Cout * g.Ho * g.Wo * sizeof(float), stream));
    const long HWi = (long)g.H * g.W, HWo = (long)g.Ho * g.Wo;
    const int nb = g.groups > 1 ? g.B : 1;            // groups: one launch per (group, sample) on offset pointers
    for (int grp = 0; grp < g.groups; ++grp)
        for (int bs = 0; bs < nb; ++bs) {
            LaConvArgs a;
            la_conv_args_init(a);      // (epi = LA_EPI_RAW, precision = LA_PREC_F32: both zero)
            a.in = x + ((long)bs * g.Cin + (long)grp * Cg) * HWi;
            a.in_bstride = (long)g.Cin * HWi;
            a.wgt = wp + (long)grp * taps * Cg * Mg;
            a.out = y + ((long)bs * g.Cout + (long)grp * Mg) * HWo;
            a.B = g.groups > 1 ? 1 : g.B; a.C = Cg; a.M = Mg;
            a.Hin = g.H; a.Win = g.W; a.Hout = g.Ho; a.Wout = g.Wo;
            a.ws = static_cast<char*>(ws) + pack_bytes; a.ws_bytes = ws_bytes - pack_bytes;
            if (!phases) {
                a.Gy = g.Ho; a.Gx = g.Wo;
                if (!g.transpose) a.in_sy = a.in_sx = g.s;
                a.ntaps = taps;
                for (int t = 0; t < taps; ++t) {
                    const int ky = t / g.kw, kx = t % g.kw;
                    a.tap_dy[t] = g.transpose ? g.py - ky : ky - g.py;
                    a.tap_dx[t] = g.transpose ? g.px - kx : kx - g.px;
                    a.tap_w[t] = t;
                }
                const int rc = la_conv_launch(a, stream);
                if (rc) return rc;
                continue;
            }
            a.out_sy = a.out_sx = 2;
            for (int ry = 0; ry < 2; ++ry)
                for (int rx = 0; rx < 2; ++rx) {
                    a.Gy = (g.Ho - ry + 1) / 2; a.Gx = (g.Wo - rx + 1) / 2;
                    if (a.Gy <= 0 || a.Gx <= 0) continue;
                    a.out_oy = ry; a.out_ox = rx;
                    int nt = 0;
                    for (int ky = 0; ky < g.kh; ++ky) {
                        if ((ry + g.py - ky) & 1) continue;
                        for (int kx = 0; kx < g.kw; ++kx) {
                            if ((rx + g.px - kx) & 1) continue;
                            a.tap_dy[nt] = (ry + g.py - ky) / 2; a.tap_dx[nt] = (rx + g.px - kx) / 2; a.tap_w[nt] = ky * g.kw + kx;
                            ++nt;
                        }
                    }
                    if (nt == 0) continue;
                    a.ntaps = nt;
                    const int rc = la_conv_launch(a, stream);
                    if (rc) return rc;
                }
        }
    return LA_OK;
}

}  // namespace

extern "C" int la_conv2d_uses_engine(int op, int cout, int kh, int kw, int stride, int groups) {
    if (groups < 1 || cout < 1 || kh < 1 || kw < 1 || stride < 1) return 0;
    return engine_ok(op, cout, kh, kw, stride, groups) ? 1 : 0;
}

extern "C" size_t la_conv2d_workspace_bytes(int op, int B, int Cin, int H, int W, int Cout, int kh, int kw, int Hout, int Wout, int stride,
                                            int groups, int transpose) {
    Geo g = {B, Cin, H, W, Cout, kh, kw, Hout, Wout, stride, 0, 0, groups, 1, transpose};
    if (B < 1 || Cin < 1 || H < 1 || W < 1 || Cout < 1 || kh < 1 || kw < 1 || Hout < 1 || Wout < 1 || stride < 1 || groups < 1 ||
        Cin % groups || Cout % groups || (op != LA_OP_FWD && op != LA_OP_WGRAD))
        return 16;
    return workspace_bytes(op, g);
}

extern "C" int la_conv2d_wgrad_slices(int B, int Cin, int H, int W, int Cout, int kh, int kw, int Hout, int Wout, int stride, int groups,
                                      int transpose) {
    Geo g = {B, Cin, H, W, Cout, kh, kw, Hout, Wout, stride, 0, 0, groups, 1, transpose};
    if (B < 1 || Cin < 1 || H < 1 || W < 1 || Cout < 1 || kh < 1 || kw < 1 || Hout < 1 || Wout < 1 || stride < 1 || groups < 1 ||
        Cin % groups || Cout % groups || !engine_ok(LA_OP_WGRAD, Cout, kh, kw, stride, groups))
        return 0;
    WgArgs a;
    wgrad_shape(g, a);
    return a.ks;
}

extern "C" int la_conv2d_f32(const float* x, const float* w, float* y, void* ws, size_t ws_bytes, int B, int Cin, int H, int W, int Cout,
                             int kh, int kw, int Hout, int Wout, int stride, int pady, int padx, int groups, int flip_weight, int transpose,
                             hipStream_t stream) {
    LA_CHECK_ARG(x && w && y, "conv2d: null pointer");
    Geo g = {B, Cin, H, W, Cout, kh, kw, Hout, Wout, stride, pady, padx, groups, flip_weight ? 1 : 0, transpose ? 1 : 0};
    int rc = check_geo(g);
    if (rc) return rc;
    if (engine_ok(LA_OP_FWD, Cout, kh, kw, stride, groups)) {
        LA_CHECK_ARG(ws && ((size_t)ws & 15) == 0, "conv2d: the engine path needs a 16-byte aligned workspace (la_conv2d_workspace_bytes)");
        LA_CHECK_WORKSPACE(ws_bytes, workspace_bytes(LA_OP_FWD, g), "conv2d: workspace too small (la_conv2d_workspace_bytes)");
        return engine_forward(g, x, w, y, ws, ws_bytes, stream);
    }
    const long total = (long)B * Cout * Hout * Wout;
    LA_CHECK_ARG(total <= (1L << 32) - 256, "conv2d: more than 2^32 - 256 outputs (limit of the generic path: one thread per output)");
    hipLaunchKernelGGL(la_conv_generic_fwd_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, x, w, y, g);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int B, int Cin, int H, int W,
                                   int Cout, int kh, int kw, int Hout, int Wout, int stride, int pady, int padx, int groups, int flip_weight,
                                   int transpose, hipStream_t stream) {
    LA_CHECK_ARG(x && dy && dw, "conv2d_wgrad: null pointer");
    Geo g = {B, Cin, H, W, Cout, kh, kw, Hout, Wout, stride, pady, padx, groups, flip_weight ? 1 : 0, transpose ? 1 : 0};
    int rc = check_geo(g);
    if (rc) return rc;
    WgArgs a;
    wgrad_shape(g, a);
    a.P = g.transpose ? x : dy;
    a.Q = g.transpose ? dy : x;
    a.dw = dw;
    const long nel = (long)a.A * a.N;
    if (engine_ok(LA_OP_WGRAD, Cout, kh, kw, stride, groups)) {
        LA_CHECK_ARG(ws && ((size_t)ws & 15) == 0, "conv2d_wgrad: the MFMA path needs a 16-byte aligned workspace (la_conv2d_workspace_bytes)");
        LA_CHECK_WORKSPACE(ws_bytes, workspace_bytes(LA_OP_WGRAD, g), "conv2d_wgrad: workspace too small (la_conv2d_workspace_bytes)");
        a.part = static_cast<float*>(ws);
        hipLaunchKernelGGL(la_conv_wgrad_mfma_kernel, dim3(a.mtiles * a.ntiles, a.groups, a.ks), dim3(256), 0, stream, a);
        LA_CHECK_LAUNCH();
        hipLaunchKernelGGL(la_conv_wgrad_finish_kernel, dim3(la_cdiv(nel, 256)), dim3(256), 0, stream, a);
        LA_CHECK_LAUNCH();
        return LA_OK;
    }
    LA_CHECK_ARG(nel < (1L << 24), "conv2d_wgrad: more than 2^24 - 1 weight elements (limit of the generic path: one workgroup per element)");
    hipLaunchKernelGGL(la_conv_generic_wgrad_kernel, dim3((unsigned)nel), dim3(256), 0, stream, a);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
