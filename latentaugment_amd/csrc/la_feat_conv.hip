// General convolution + bias + ReLU (square kernel up to 11, stride 1 | 2 | 4, pad 0 .. 5) with its data gradient, and the 3x3
// stride-2 max pool (floor and ceil mode) with its gradient: the trunk ops of the AlexNet and SqueezeNet 1.1 LPIPS nets
// (augments/criteria/lpips/networks.py:52-84).  Exact fp32 in every precision mode of the feature engine, as the FC ops are: these
// layers are a twentieth of VGG16's multiply-adds and do not need the split-fp16 path.  No float atomics, no host sync, no allocation.
#include "la_feat_conv.h"
#include "la_f32_tile.h"

// ------------------------------------------------------------------------------------------------------------
// Forward: an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products), D[co][pixel] = sum_K W[co][K] * col[K][pixel],
//   M = N * Ro * Ro pixels, K = cin * k * k (K index = (ci * k + ky) * k + kx: a row of the weight tensor as it is stored).
// Workgroup = 256 threads = 4 waves (2 x 2), block tile 64 output channels x 64 pixels, every wave one 32 x 32 MFMA tile.  The weights are
// the A operand and the pixels the B operand, so an accumulator register row is an output channel and its 32 lanes are 32 consecutive
// pixels (coalesced NCHW stores).  K is walked in chunks of 32: the im2col gather of the next chunk (8 elements per thread, pixel along
// the lanes, zero outside the image, the batch and K) and its weight rows are in flight in registers while the current chunk feeds the
// MFMAs from LDS (two buffers, one barrier per chunk: la_tile_pipeline of la_f32_tile.h).  LDS: Ws[co][k + 1] is written along k and
// read along co, Xs[k][pixel + 4] is written and read along the pixel: both free of bank conflicts.
// Small M (the loop's 64 x 64 crop leaves 9 .. 225 pixels in the deep layers, with K in the thousands): K is split over gridDim.y
// workgroups (fcv_plan); a slice's raw tile goes to part[slice][tile][64][64] and la_featconv_finish_kernel sums the slices in slice
// order, adds the bias and applies the ReLU -- a fixed order, the same bits on every run.  With one slice the kernel applies them itself.
#define FCV_CT 64
#define FCV_PT 64
#define FCV_KC 32

// The same kernel is the data gradient of a stride-1 layer (BWD): a convolution of the masked gradient with the flipped kernel and pad
// k - 1 - pad, rows of the GEMM = input channels, K = cout * k * k.  In GEMM terms, for both directions: the gathered tensor x is
// [N][in_ctotal][R][R] of which channels [in_coff, in_coff + cin) are read, the output y is [N][c_total][Ro][Ro] of which channels
// [c_off, c_off + cout) are written; BWD reads x through the ReLU mask (mask > 0, same layout as x), looks the weight of
// (row ci', K index (co', ky, kx)) up at w[co'][ci'][k-1-ky][k-1-kx] (wcin = channels of the weight tensor's second axis), adds no
// bias, applies no ReLU and, with accumulate, adds onto y.
struct FcvArgs {
    const float *x, *w, *b, *mask;
    float *y, *part;
    int N, cin, cout, k, stride, pad, R, Ro, c_off, c_total, in_coff, in_ctotal, wcin, accumulate;
    int K, ptiles, ctiles, ks, per, nchunk;
    long M;
};

template <bool BWD>
__global__ __launch_bounds__(256) void la_featconv_gemm_kernel(FcvArgs a) {
    __shared__ float Ws[2][FCV_CT][FCV_KC + 1];
    __shared__ float Xs[2][FCV_KC][FCV_PT + 4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int pt = blockIdx.x % a.ptiles, ct = blockIdx.x / a.ptiles;
    const long m0 = (long)pt * FCV_PT;
    const int co0 = ct * FCV_CT;
    const int HWo = a.Ro * a.Ro, kk = a.k * a.k;

    // gather role: pixel gp of the tile, K rows gk0 + 4 j of the chunk
    const int gp = tid & 63, gk0 = tid >> 6;
    const long gm = m0 + gp;
    const bool gok = gm < a.M;
    const int gn = gok ? (int)(gm / HWo) : 0;
    const int grem = gok ? (int)(gm - (long)gn * HWo) : 0;
    const int iy0 = (grem / a.Ro) * a.stride - a.pad, ix0 = (grem % a.Ro) * a.stride - a.pad;
    const long xoff = ((long)gn * a.in_ctotal + a.in_coff) * a.R * a.R;
    const float* xn = a.x + xoff;
    const float* mn = BWD ? a.mask + xoff : nullptr;
    // weight role: K column wk of the chunk, channel rows wc0 + 8 j of the tile
    const int wk = tid & 31, wc0 = tid >> 5;

    int c_beg, c_end;
    la_slice_range(blockIdx.y, a.per, a.nchunk, &c_beg, &c_end);

    float xreg[8], wreg[8];
    auto prefetch = [&](int ci) {
        const int kb = ci * FCV_KC;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kidx = kb + gk0 + 4 * j;
            float v = 0.f;
            if (gok && kidx < a.K) {
                const int c = kidx / kk, t = kidx - c * kk;
                const int ky = t / a.k, kx = t - ky * a.k;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if ((unsigned)iy < (unsigned)a.R && (unsigned)ix < (unsigned)a.R) {
                    const long o = ((long)c * a.R + iy) * a.R + ix;
                    v = xn[o];
                    if (BWD && !(mn[o] > 0.f)) v = 0.f;
                }
            }
            xreg[j] = v;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int co = co0 + wc0 + 8 * j, kidx = kb + wk;
            float v = 0.f;
            if (co < a.cout && kidx < a.K) {
                if (BWD) {
                    const int c = kidx / kk, t = kk - 1 - (kidx - c * kk);      // (flipping both axes of a k x k tap is reversing its index)
                    v = a.w[((long)c * a.wcin + co) * kk + t];
                } else {
                    v = a.w[(long)co * a.K + kidx];
                }
            }
            wreg[j] = v;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) Xs[buf][gk0 + 4 * j][gp] = xreg[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Ws[buf][wc0 + 8 * j][wk] = wreg[j];
    };

    const int ch = wid & 1, ph = wid >> 1;      // this wave's 32 channels / 32 pixels of the tile
    la_f32x16 tile[1][1];
    la_f32_tile_zero(tile);
    la_f32x16& acc = tile[0][0];
    // (the header's la_f32_tile_mma reads both operands as [k][col]; Ws is [co][k + 1] here, so the inner product stays written out)
    la_tile_pipeline(c_beg, c_end, prefetch, stage, [&](int buf, int) {
#pragma unroll
        for (int kp = 0; kp < FCV_KC / 2; ++kp)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[buf][ch * 32 + l31][2 * kp + lh], Xs[buf][2 * kp + lh][ph * 32 + l31], acc, 0, 0, 0);
    });

    const int pl = ph * 32 + l31;
    if (a.ks > 1) {      // raw tile of this slice: every element of the 64 x 64 block, inside the output or not
        float* dst = a.part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (FCV_CT * FCV_PT);
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(ch * 32 + la_mfma32_row(r, lh)) * FCV_PT + pl] = acc[r];
        return;
    }
    const long m = m0 + pl;
    if (m >= a.M) return;
    const int n = (int)(m / HWo);
    const int rem = (int)(m - (long)n * HWo);
    float* yo = a.y + ((long)n * a.c_total + a.c_off) * HWo + rem;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + ch * 32 + la_mfma32_row(r, lh);
        if (co >= a.cout) continue;
        if (BWD) {
            yo[(long)co * HWo] = a.accumulate ? yo[(long)co * HWo] + acc[r] : acc[r];
        } else {
            const float v = acc[r] + a.b[co];
            yo[(long)co * HWo] = v > 0.f ? v : 0.f;
        }
    }
}

// second pass of the split: slices summed in slice order, then bias and ReLU (BWD: the optional accumulation).  One thread per output
// element, pixel along the lanes
template <bool BWD>
__global__ __launch_bounds__(256) void la_featconv_finish_kernel(FcvArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.M * a.cout) return;
    const int co = (int)(idx / a.M);
    const long m = idx - (long)co * a.M;
    const long tiles = (long)a.ptiles * a.ctiles;
    const long tile = (long)(co / FCV_CT) * a.ptiles + m / FCV_PT;
    const float* src = a.part + tile * (FCV_CT * FCV_PT) + (co % FCV_CT) * FCV_PT + m % FCV_PT;
    float s = la_slices_sum(src, 0, tiles * (FCV_CT * FCV_PT), a.ks);
    const int HWo = a.Ro * a.Ro;
    const int n = (int)(m / HWo);
    const int rem = (int)(m - (long)n * HWo);
    float* dst = a.y + ((long)n * a.c_total + a.c_off + co) * HWo + rem;
    if (BWD) {
        *dst = a.accumulate ? *dst + s : s;
    } else {
        s += a.b[co];
        *dst = s > 0.f ? s : 0.f;
    }
}

struct FcvPlan { int ptiles, ctiles, nchunk, ks, per; };
// K slices only where the tiles alone leave most of the chip idle and K is long: at most 256 workgroups in all, at least 4 chunks a slice
static FcvPlan fcv_plan(long M, int cout, int K) {
    FcvPlan p;
    p.ptiles = la_cdiv(M, FCV_PT); p.ctiles = la_cdiv(cout, FCV_CT); p.nchunk = la_cdiv(K, FCV_KC);
    const long tiles = (long)p.ptiles * p.ctiles;
    int ks = 1;
    if (tiles <= 64 && p.nchunk >= 8) {
        ks = (int)(256 / tiles);
        if (ks > p.nchunk / 4) ks = p.nchunk / 4;
        if (ks < 1) ks = 1;
    }
    p.per = la_cdiv(p.nchunk, ks);
    p.ks = la_cdiv(p.nchunk, p.per);
    return p;
}

// the data gradient of a stride-1 layer behind the first runs on the GEMM kernel; strided layers and the 3-channel first layer gather
static inline bool fcv_bwd_gemm(const LaFeatConvGeom& g) { return g.stride == 1 && g.cin % 4 == 0; }

int la_featconv_out_res(int cin, int cout, int k, int stride, int pad, int R) {
    if (k < 1 || k > LA_FCV_KMAX || !(stride == 1 || stride == 2 || stride == 4) || pad < 0 || pad > 5 || pad >= k) return 0;
    if (cout < 4 || cout % 4 || cin < 1 || !(cin == 3 || cin % 4 == 0) || R < 1 || R + 2 * pad < k) return 0;
    return (R + 2 * pad - k) / stride + 1;
}

size_t la_featconv_part_floats(int maxN, const LaFeatConvGeom& g) {
    size_t worst = 0;
    for (int n = 1; n <= maxN; ++n) {
        const FcvPlan p = fcv_plan((long)n * g.Ro * g.Ro, g.cout, g.cin * g.k * g.k);
        const size_t f = p.ks > 1 ? (size_t)p.ks * p.ptiles * p.ctiles * (FCV_CT * FCV_PT) : 0;
        if (f > worst) worst = f;
        if (fcv_bwd_gemm(g)) {
            const FcvPlan q = fcv_plan((long)n * g.R * g.R, g.cin, g.cout * g.k * g.k);
            const size_t fb = q.ks > 1 ? (size_t)q.ks * q.ptiles * q.ctiles * (FCV_CT * FCV_PT) : 0;
            if (fb > worst) worst = fb;
        }
    }
    return worst;
}

static int fcv_check(const LaFeatConvGeom& g, int N, int c_off, int c_total) {
    LA_CHECK_ARG(N >= 1 && la_featconv_out_res(g.cin, g.cout, g.k, g.stride, g.pad, g.R) == g.Ro && g.Ro >= 1, "featconv: geometry refused");
    LA_CHECK_ARG(c_off >= 0 && c_off + g.cout <= c_total, "featconv: channel slice outside the output");
    LA_CHECK_ARG((long)N * g.Ro * g.Ro * c_total < (1L << 31) && (long)N * g.R * g.R * g.cin < (1L << 31), "featconv: tensor too large");
    return LA_OK;
}

int la_featconv_forward(const float* x, const float* w, const float* b, float* y, int N, const LaFeatConvGeom& g, int c_off, int c_total,
                        float* part, size_t part_floats, hipStream_t stream) {
    LA_CHECK_ARG(x && w && b && y, "featconv: null pointer");
    int rc = fcv_check(g, N, c_off, c_total);
    if (rc) return rc;
    FcvArgs a;
    a.x = x; a.w = w; a.b = b; a.y = y; a.part = part;
    a.N = N; a.cin = g.cin; a.cout = g.cout; a.k = g.k; a.stride = g.stride; a.pad = g.pad; a.R = g.R; a.Ro = g.Ro;
    a.c_off = c_off; a.c_total = c_total; a.K = g.cin * g.k * g.k; a.M = (long)N * g.Ro * g.Ro;
    a.mask = nullptr; a.in_coff = 0; a.in_ctotal = g.cin; a.wcin = g.cin; a.accumulate = 0;
    const FcvPlan p = fcv_plan(a.M, g.cout, a.K);
    a.ptiles = p.ptiles; a.ctiles = p.ctiles; a.ks = p.ks; a.per = p.per; a.nchunk = p.nchunk;
    if (p.ks > 1) LA_CHECK_WORKSPACE(part ? part_floats : 0, (size_t)p.ks * p.ptiles * p.ctiles * (FCV_CT * FCV_PT), "featconv: split-K workspace too small");
    hipLaunchKernelGGL(la_featconv_gemm_kernel<false>, dim3((unsigned)(p.ptiles * p.ctiles), (unsigned)p.ks), dim3(256), 0, stream, a);
    if (p.ks > 1) hipLaunchKernelGGL(la_featconv_finish_kernel<false>, dim3(la_cdiv(a.M * g.cout, 256)), dim3(256), 0, stream, a);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Data gradient of the strided layers and of a 3-channel first layer (every other layer: la_featconv_gemm_kernel<true>; measured at the
// loop's crop, this form on every layer cost 3.8 ms against 0.66 ms per step of the AlexNet criterion), in gather form: one thread per
// input element (ix along the lanes), which walks the output channels and, per channel,
// the taps (ky, kx) congruent to (iy + pad, ix + pad) modulo the stride whose output pixel exists.  The incoming gradient is masked on
// load by the saved ReLU output (y > 0).  A fixed summation order (co, then ky, then kx ascending): the same bits on every run.
struct FcvBwdArgs {
    const float *gy, *y, *w;
    float* gx;
    int N, cin, cout, k, stride, pad, R, Ro, c_off, c_total, accumulate;
    long total;
};

__global__ __launch_bounds__(256) void la_featconv_bwd_kernel(FcvBwdArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int ix = (int)(idx % a.R), iy = (int)((idx / a.R) % a.R);
    const long pl = idx / ((long)a.R * a.R);
    const int ci = (int)(pl % a.cin);
    const long n = pl / a.cin;
    const int HWo = a.Ro * a.Ro, kk = a.k * a.k;
    // taps of one axis: ky = ky0, ky0 + stride, .. < k with oy = (iy + pad - ky) / stride inside [0, Ro)
    const int ty = iy + a.pad, tx = ix + a.pad;
    int ky_lo = ty % a.stride, kx_lo = tx % a.stride;
    while ((ty - ky_lo) / a.stride >= a.Ro) ky_lo += a.stride;
    while ((tx - kx_lo) / a.stride >= a.Ro) kx_lo += a.stride;
    const int ky_hi = ty < a.k - 1 ? ty : a.k - 1, kx_hi = tx < a.k - 1 ? tx : a.k - 1;      // inclusive: oy >= 0
    const long gbase = (n * a.c_total + a.c_off) * HWo;
    float acc = 0.f;
    for (int co = 0; co < a.cout; ++co) {
        const float* gp = a.gy + gbase + (long)co * HWo;
        const float* yp = a.y + gbase + (long)co * HWo;
        const float* wp = a.w + ((long)co * a.cin + ci) * kk;
        for (int ky = ky_lo; ky <= ky_hi; ky += a.stride) {
            const int oy = (ty - ky) / a.stride;
            for (int kx = kx_lo; kx <= kx_hi; kx += a.stride) {
                const int o = oy * a.Ro + (tx - kx) / a.stride;
                const float g = yp[o] > 0.f ? gp[o] : 0.f;
                acc += g * wp[ky * a.k + kx];
            }
        }
    }
    a.gx[idx] = a.accumulate ? a.gx[idx] + acc : acc;
}

int la_featconv_backward(const float* gy, const float* y, const float* w, float* gx, int N, const LaFeatConvGeom& g, int c_off, int c_total,
                         int accumulate, float* part, size_t part_floats, hipStream_t stream) {
    LA_CHECK_ARG(gy && y && w && gx, "featconv_backward: null pointer");
    int rc = fcv_check(g, N, c_off, c_total);
    if (rc) return rc;
    if (fcv_bwd_gemm(g)) {
        // a stride-1 convolution of the masked gradient [N][c_total][Ro][Ro] with the flipped kernel, pad k - 1 - pad: Ro -> R
        FcvArgs a;
        a.x = gy; a.mask = y; a.w = w; a.b = nullptr; a.y = gx; a.part = part;
        a.N = N; a.cin = g.cout; a.cout = g.cin; a.k = g.k; a.stride = 1; a.pad = g.k - 1 - g.pad; a.R = g.Ro; a.Ro = g.R;
        a.c_off = 0; a.c_total = g.cin; a.in_coff = c_off; a.in_ctotal = c_total; a.wcin = g.cin; a.accumulate = accumulate ? 1 : 0;
        a.K = g.cout * g.k * g.k; a.M = (long)N * g.R * g.R;
        const FcvPlan p = fcv_plan(a.M, a.cout, a.K);
        a.ptiles = p.ptiles; a.ctiles = p.ctiles; a.ks = p.ks; a.per = p.per; a.nchunk = p.nchunk;
        if (p.ks > 1) LA_CHECK_WORKSPACE(part ? part_floats : 0, (size_t)p.ks * p.ptiles * p.ctiles * (FCV_CT * FCV_PT), "featconv_backward: split-K workspace too small");
        hipLaunchKernelGGL(la_featconv_gemm_kernel<true>, dim3((unsigned)(p.ptiles * p.ctiles), (unsigned)p.ks), dim3(256), 0, stream, a);
        if (p.ks > 1) hipLaunchKernelGGL(la_featconv_finish_kernel<true>, dim3(la_cdiv(a.M * a.cout, 256)), dim3(256), 0, stream, a);
        LA_CHECK_LAUNCH();
        return LA_OK;
    }
    FcvBwdArgs a;
    a.gy = gy; a.y = y; a.w = w; a.gx = gx;
    a.N = N; a.cin = g.cin; a.cout = g.cout; a.k = g.k; a.stride = g.stride; a.pad = g.pad; a.R = g.R; a.Ro = g.Ro;
    a.c_off = c_off; a.c_total = c_total; a.accumulate = accumulate ? 1 : 0;
    a.total = (long)N * g.cin * g.R * g.R;
    hipLaunchKernelGGL(la_featconv_bwd_kernel, dim3(la_cdiv(a.total, 256)), dim3(256), 0, stream, a);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// 3x3 stride-2 max pool, no padding.  torch's output size: floor or ceil of (R - 3) / 2, plus 1; in ceil mode a last window that
// would start at or past the end of the input is dropped.  A ceil-mode window may hang over the edge: it is clipped to the input.
int la_pool3s2_out_res(int R, int ceil_mode) {
    if (R < 1) return 0;
    const int num = R - 3 + (ceil_mode ? 1 : 0);
    int out = (num >= 0 ? num / 2 : -((-num + 1) / 2)) + 1;      // floor division
    if (ceil_mode && out >= 1 && (out - 1) * 2 >= R) --out;
    return out < 1 ? 0 : out;
}

// first maximum of window (oy, ox) in row-major scan order (torch: a later element replaces the maximum only if it is greater)
__device__ __forceinline__ int pool3_argmax(const float* __restrict__ p, int R, int oy, int ox, float& best) {
    const int y0 = 2 * oy, x0 = 2 * ox;
    const int y1 = y0 + 3 < R ? y0 + 3 : R, x1 = x0 + 3 < R ? x0 + 3 : R;
    int am = y0 * R + x0;
    best = p[am];
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const float v = p[y * R + x];
            if (v > best) { best = v; am = y * R + x; }
        }
    return am;
}

__global__ void la_pool3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int Ro, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Ro), oy = (int)((i / Ro) % Ro);
    const long pl = i / ((long)Ro * Ro);
    float best;
    pool3_argmax(x + pl * R * R, R, oy, ox, best);
    y[i] = best;
}

// Gather form: an input pixel lies in at most two windows per axis, four in all; for each the window's argmax is recomputed and gy
// taken if the pixel is that argmax (windows in ascending (oy, ox) order).  Ties: the first maximum in scan order takes the gradient,
// as in torch.  Among the zeros a ReLU leaves, which of them is "first" cannot change the gradient of the net's input: the ReLU mask
// of the convolution below multiplies every one of them by zero.
__global__ void la_pool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, int R, int Ro,
                                      long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ix = (int)(i % R), iy = (int)((i / R) % R);
    const long pl = i / ((long)R * R);
    const float* xp = x + pl * R * R;
    const float* gp = gy + pl * Ro * Ro;
    const int oy_lo = iy >= 2 ? (iy - 1) / 2 : 0, ox_lo = ix >= 2 ? (ix - 1) / 2 : 0;      // ceil((i - 2) / 2)
    const int oy_hi = iy / 2 < Ro - 1 ? iy / 2 : Ro - 1, ox_hi = ix / 2 < Ro - 1 ? ix / 2 : Ro - 1;
    const int me = iy * R + ix;
    float acc = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            float best;
            if (pool3_argmax(xp, R, oy, ox, best) == me) acc += gp[oy * Ro + ox];
        }
    gx[i] = acc;
}

int la_pool3s2_forward(const float* x, float* y, long planes, int R, int Ro, hipStream_t stream) {
    LA_CHECK_ARG(x && y && planes >= 1 && Ro >= 1 && (Ro - 1) * 2 < R, "pool3s2: bad arguments");
    const long total = planes * Ro * Ro;
    LA_CHECK_ARG(total < (1L << 31) && planes * R * R < (1L << 31), "pool3s2: tensor too large");
    hipLaunchKernelGGL(la_pool3s2_fwd_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, x, y, R, Ro, total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

int la_pool3s2_backward(const float* x, const float* gy, float* gx, long planes, int R, int Ro, hipStream_t stream) {
    LA_CHECK_ARG(x && gy && gx && planes >= 1 && Ro >= 1 && (Ro - 1) * 2 < R, "pool3s2_backward: bad arguments");
    const long total = planes * R * R;
    LA_CHECK_ARG(total < (1L << 31), "pool3s2_backward: tensor too large");
    hipLaunchKernelGGL(la_pool3s2_bwd_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, x, gy, gx, R, Ro, total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
