// Detector features (the `return_features=True` branch of NVIDIA's scripted VGG16, metrics/metric_utils.py:264-328 and
// metrics/precision_recall.py:36-85): what the perceptual feature engine (la_feat.hip) lacks for it.
//   la_detector_prep_f32   generator image -> the net's input: quantise to the uint8 grid, repeat one channel three times, resample
//                          to S x S (area | bilinear), per-channel input affine; one launch.
//   la_fc_bias_act_f32     y = act(x W^T + b) for the two large fully connected layers: a weight stream on the fp32 MFMA.
// The index arithmetic of both is in la_detector_index.h (host and device).
#include "la_common.h"
#include "la_detector_index.h"
#include "la_f32_tile.h"

// ------------------------------------------------------------------------------------------------------------
struct LaDetAffine { float scale[3], shift[3]; };

// One thread per (n, input channel c, oy, ox): the resampled value is computed once and written to its `rep` output channels
// (channel r * C + c, torch's x.repeat([1, rep, 1, 1])).
// quantize: torch's (x * 127.5 + 128).clamp(0, 255).to(torch.uint8) -- the product and the sum are rounded separately, and the
// conversion truncates, which is floor on [0, 255].  Contraction is switched off for this function: a fused multiply-add lands in
// another bin at 95 of the 765 floats around the 255 bin edges.  (HIP's __fmul_rn / __fadd_rn are plain operators that the compiler
// contracts under its default -ffp-contract=fast, so they do not keep the two roundings apart; the pragma does.)
__device__ __forceinline__ float la_det_quant(float x) {
#pragma clang fp contract(off)
    const float p = x * 127.5f;
    const float v = p + 128.f;
    return floorf(fminf(fmaxf(v, 0.f), 255.f));
}

__global__ __launch_bounds__(256) void la_detector_prep_kernel(const float* __restrict__ img, float* __restrict__ out, int C, int H, int W,
                                                                int S, int rep, int mode, int quantize, LaDetAffine aff, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    const long pl = i / ((long)S * S);                  // n * C + c
    const int c = (int)(pl % C);
    const long n = pl / C;
    const float* p = img + pl * (long)H * W;
    float v;
    if (H == S && W == S) {
        v = p[(long)oy * W + ox];
        if (quantize) v = la_det_quant(v);
    } else if (mode == LA_DET_AREA) {
        const int y0 = la_det_area_lo(oy, H, S), y1 = la_det_area_hi(oy, H, S);
        const int x0 = la_det_area_lo(ox, W, S), x1 = la_det_area_hi(ox, W, S);
        float s = 0.f;
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                const float t = p[(long)y * W + x];
                s += quantize ? la_det_quant(t) : t;
            }
        v = s / (float)((y1 - y0) * (x1 - x0));
    } else {
        const LaDetLerp<float> ly = la_det_bilinear<float>(oy, H, S), lx = la_det_bilinear<float>(ox, W, S);
        float a = p[(long)ly.i0 * W + lx.i0], b = p[(long)ly.i0 * W + lx.i1];
        float cc = p[(long)ly.i1 * W + lx.i0], d = p[(long)ly.i1 * W + lx.i1];
        if (quantize) { a = la_det_quant(a); b = la_det_quant(b); cc = la_det_quant(cc); d = la_det_quant(d); }
        v = ly.w0 * (lx.w0 * a + lx.w1 * b) + ly.w1 * (lx.w0 * cc + lx.w1 * d);
    }
    for (int r = 0; r < rep; ++r) {
        const int k = r * C + c;
        out[((n * rep * C + k) * S + oy) * S + ox] = v * aff.scale[k] + aff.shift[k];
    }
}

extern "C" int la_detector_prep_f32(const float* img, float* out, int N, int C, int H, int W, int S, int rep, int mode, int quantize,
                                    const float* scale, const float* shift, hipStream_t stream) {
    LA_CHECK_ARG(img && out && scale && shift, "detector_prep: null pointer");
    LA_CHECK_ARG(N >= 1 && C >= 1 && rep >= 1 && C * rep == 3, "detector_prep: channels * rep must be 3");
    LA_CHECK_ARG(H >= 1 && W >= 1 && S >= 1 && H <= 32768 && W <= 32768 && S <= 32768, "detector_prep: sizes must lie in 1 .. 32768");
    LA_CHECK_ARG(mode == LA_DET_AREA || mode == LA_DET_BILINEAR, "detector_prep: mode must be 0 (area) or 1 (bilinear)");
    LaDetAffine aff;
    for (int k = 0; k < 3; ++k) { aff.scale[k] = scale[k]; aff.shift[k] = shift[k]; }
    const long total = (long)N * C * S * S;
    LA_CHECK_ARG(la_cdiv(total, 256) > 0 && total / 256 < (1L << 31) - 1, "detector_prep: too many output elements for one launch");
    hipLaunchKernelGGL(la_detector_prep_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, img, out, C, H, W, S, rep, mode, quantize ? 1 : 0,
                       aff, total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// y[N][O] = act(x[N][K] . W[O][K]^T + b[O]), exact fp32 products on v_mfma_f32_32x32x2_f32.
// The layer is a weight stream (fc1 of VGG16: 411 MB of weights against 13 GFLOP at N = 64), so the kernel is built around reading
// W once: a workgroup owns LA_FC_OT = 128 output features x a batch tile of 32 * NB rows (NB = 2: every N <= 64 is ONE batch tile and
// each weight element leaves HBM once per call; beyond 64 rows the batch tiles of one weight tile are neighbours in launch order and
// the repeats are served by the caches) x one K slice, and all rows of the batch tile share the staged weight chunk through LDS.
// 256 threads = 4 waves; wave w computes features [32w, 32w + 32) for all 32 * NB rows: x is the A operand (rows = batch), W the B
// operand (columns = features), so an accumulator register row is a batch row and its 32 lanes are 32 consecutive features (coalesced
// stores).  K is walked in chunks of LA_FC_KC = 32: loads of the next chunk (16 bytes per lane along K where K % 4 == 0 and the
// pointers allow, else scalar) are in flight while the current one feeds the MFMAs (register staging, two LDS buffers, one barrier per
// chunk: la_tile_pipeline of la_f32_tile.h).  LDS rows are [k][tile + 4]: the operand reads are 32 consecutive floats per half-wave.
// Parallelism at O = 4096 (32 feature tiles) comes from K slices (la_fc_plan): a slice's raw tile goes to part[slice][N][O] and
// la_fc_finish_kernel sums the slices in slice order and applies bias and activation -- no float atomics, the same bits on every run.
// With one slice the kernel applies them itself.  Ragged N, K and O: loads outside load zeros, stores outside are skipped.
#define FC_WLD (LA_FC_OT + 4)

struct FcArgs {
    const float *x, *w, *b;
    float *y, *part;
    long N, K, O;
    int ntiles, ks, act;
    long per, nchunk;
};

template <int NB, bool VEC>
__global__ __launch_bounds__(256) void la_fc_mfma_kernel(FcArgs a) {
    constexpr int XLD = 32 * NB + 4;
    __shared__ __attribute__((aligned(16))) float Ws[2][LA_FC_KC][FC_WLD];
    __shared__ __attribute__((aligned(16))) float Xs[2][LA_FC_KC][XLD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int nt = blockIdx.x % a.ntiles, ot = blockIdx.x / a.ntiles;
    const long n0 = (long)nt * (32 * NB), o0 = (long)ot * LA_FC_OT;

    // loader roles: 8 threads x 4 floats cover a row's chunk; 32 rows per pass, 4 passes for W, NB for x
    const int kq = (tid & 7) * 4, r0 = tid >> 3;
    long c_beg, c_end;
    la_slice_range(blockIdx.y, a.per, a.nchunk, &c_beg, &c_end);

    float wreg[4][4], xreg[NB][4];
    auto load4 = [&](const float* row, bool ok, long k, float* dst) {
        if (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && k < a.K) v = *reinterpret_cast<const float4*>(row + k);      // (K % 4 == 0: all four inside or none)
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = (ok && k + j < a.K) ? row[k + j] : 0.f;
        }
    };
    auto prefetch = [&](long ci) {
        const long k = ci * LA_FC_KC + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long o = o0 + r0 + 32 * j;
            load4(a.w + (o < a.O ? o : 0) * a.K, o < a.O, k, wreg[j]);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const long n = n0 + r0 + 32 * j;
            load4(a.x + (n < a.N ? n : 0) * a.K, n < a.N, k, xreg[j]);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) Ws[buf][kq + q][r0 + 32 * j] = wreg[j][q];
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) Xs[buf][kq + q][r0 + 32 * j] = xreg[j][q];
    };

    la_f32x16 acc[NB][1];
    la_f32_tile_zero(acc);
    la_tile_pipeline(c_beg, c_end, prefetch, stage,
                     [&](int buf, long) { la_f32_tile_mma<LA_FC_KC>(Xs, Ws, buf, 0, wid * 32, l31, lh, acc); });

    const long o = o0 + wid * 32 + l31;
    if (o >= a.O) return;
    const bool direct = a.ks == 1;
    float* dst = direct ? a.y : a.part + (long)blockIdx.y * a.N * a.O;
    const float bias = direct ? a.b[o] : 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long n = n0 + i * 32 + la_mfma32_row(r, lh);
            if (n >= a.N) continue;
            float v = acc[i][0][r];
            if (direct) { v += bias; if (a.act == LA_ACT_RELU) v = v > 0.f ? v : 0.f; }
            dst[n * a.O + o] = v;
        }
}

// second pass of the split: slices summed in slice order (bit-identical from run to run), then bias and activation
__global__ __launch_bounds__(256) void la_fc_finish_kernel(FcArgs a) {
    const long total = a.N * a.O;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float s = la_slices_sum(a.part, idx, total, a.ks) + a.b[idx % a.O];
    if (a.act == LA_ACT_RELU) s = s > 0.f ? s : 0.f;
    a.y[idx] = s;
}

static int fc_check_shape(long N, long K, long O) {
    LA_CHECK_ARG(N >= 1 && K >= 1 && O >= 1, "fc: N, K and O must be at least 1");
    LA_CHECK_ARG(N <= (1L << 24) && K < (1L << 31) && O < (1L << 31) && N * O < (1L << 40), "fc: shape too large");
    return LA_OK;
}

// bytes for any batch of up to N rows on one workspace: a smaller batch never takes more slices than a batch of one
extern "C" size_t la_fc_workspace_bytes(long N, long K, long O) {
    if (fc_check_shape(N, K, O)) return 0;
    const LaFcPlan p1 = la_fc_plan(1, K, O);
    return 256 + (p1.ks > 1 ? (size_t)p1.ks * (size_t)N * (size_t)O * sizeof(float) : 0);
}

extern "C" int la_fc_bias_act_f32(const float* x, const float* w, const float* b, float* y, long N, long K, long O, int act, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
    LA_CHECK_ARG(x && w && b && y && workspace, "fc: null pointer");
    int rc = fc_check_shape(N, K, O);
    if (rc) return rc;
    LA_CHECK_ARG(act == LA_ACT_LINEAR || act == LA_ACT_RELU, "fc: act must be linear or relu");
    LA_CHECK_WORKSPACE(workspace_bytes, la_fc_workspace_bytes(N, K, O), "fc: workspace too small");
    const LaFcPlan p = la_fc_plan(N, K, O);
    LA_CHECK_ARG((long)p.ntiles * p.otiles < (1L << 31) - 1, "fc: too many tiles for one launch");
    FcArgs a;
    a.x = x; a.w = w; a.b = b; a.y = y;
    a.part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    a.N = N; a.K = K; a.O = O; a.ntiles = p.ntiles; a.ks = p.ks; a.act = act; a.per = p.per; a.nchunk = p.nchunk;
    const bool vec = p.vec && ((uintptr_t)x % 16 == 0) && ((uintptr_t)w % 16 == 0);
    const dim3 grid((unsigned)(p.ntiles * p.otiles), (unsigned)p.ks);
    if (p.nb == 1) {
        if (vec) hipLaunchKernelGGL((la_fc_mfma_kernel<1, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((la_fc_mfma_kernel<1, false>), grid, dim3(256), 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((la_fc_mfma_kernel<2, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((la_fc_mfma_kernel<2, false>), grid, dim3(256), 0, stream, a);
    }
    if (p.ks > 1) hipLaunchKernelGGL(la_fc_finish_kernel, dim3(la_cdiv(N * O, 256)), dim3(256), 0, stream, a);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
