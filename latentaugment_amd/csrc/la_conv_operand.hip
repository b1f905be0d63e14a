// Implicit-GEMM convolution on the 16-bit MFMA path with fp32 operands split into 16-bit terms.
//
// fp32 MFMA runs at 1/16 of the 16-bit MFMA rate on gfx950 (MI355X_MICROARCH.md, Matrix cores), so an fp32 contraction is
// re-expressed as a few 16-bit x 16-bit products with fp32 accumulation (the products are exact in fp32, the MFMA
// accumulates in fp32, so the only approximation is the dropped low-order cross terms):
//     FMT_BF16X3:  x = h + m + l (each term the bf16 rounding of what the previous terms left), same for w;
//                  x.w ~= hh + (hm + mh) + (mm + hl + lh)     6 MFMAs, error ~1e-7 relative (fp32-class)
//     FMT_BF16X2:  x.w ~= hh + (hm + mh)                       3 MFMAs, error ~4e-6 relative (approximate mode)
//     FMT_F16X2:   x and w are first brought into fp16 range by exact power-of-two scales (one per weight tensor, one per
//                  sample of the modulated input, scaled max in [2^14, 2^15)), then x = h + l in fp16 (22 significand
//                  bits);  x.w ~= hh + hl + lh               3 MFMAs, error ~2e-7 relative (fp32-class); the accumulators
//                  are multiplied by the inverse scales before the epilogue (exact)
// One accumulator per output; within a K step the correction products are issued before the leading one.  Measured errors:
// tests/test_hip_ops.py against the oracle.
//
// Tiling: as la_conv.hip (256 threads = 2x2 waves, tile MT x 128 pixels, wave 64x64 = 2x2 MFMA tiles), K chunk =
// (one tap, 32 input channels) = two K=16 MFMA steps.  Weights are split at pack time into a FRAGMENT-ORDER pack
// (pack_slab_offset) that the waves read straight from global memory.  Pixels: the halo kernel reads the fp32 input and
// splits on the way into LDS; the flat kernel (whose gather re-reads every element once per tap) reads a pre-split copy
// made once per launch input (la_presplit_*: 8 bytes per element {h | m<<16, l} bf16, 4 bytes {h | l<<16} fp16).
// This unit: operand preparation (weight packs, fp16 operand scales, the pre-split copy); which of the two kernels (la_conv_halo.hip,
// la_conv_flat.hip) a launch runs is la_conv_plan's decision (la_conv.hip).
#include "la_conv_device.h"

#define PRESPLIT_HDR 512       // head of the workspace: [0,256) xscale[b] floats; the segment maxima follow the header

// ------------------------------------------------------------------------------------------------------------
// weight packing: W[o][i][t] (fp32) -> out[term][t][cc][m/32][k/16][lane][8] with (m,k) = (o,i) forward or (i,o) backward.
// Inside a (tap, 32-channel chunk) slab the 32-row x 16-channel blocks are stored in MFMA A-FRAGMENT order: lane
// (r = m%32, h = (k/8)%2) holds A[r][8h .. 8h+7] as 16 contiguous bytes, lanes contiguous -- so a wave fetches one
// fragment with a single fully coalesced 1 KB load, no LDS staging.  M is padded to a multiple of 32 with zero rows.
__device__ __forceinline__ long pack_slab_offset(int m, int k) {      // element offset of (row m, channel k) inside a slab
    return ((((long)(m >> 5) * 2 + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (m & 31)) << 3) + (k & 7);
}
__global__ void la_pack_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int cout, int cin, int ktaps,
                                    int transpose, int nterm, float scale, int m_pad) {
    const int Mreal = transpose ? cin : cout, C = transpose ? cout : cin;
    const int M = pack_mp(m_pad > Mreal ? m_pad : Mreal);
    const int nck = (C + KCB - 1) / KCB;
    const long per_term = (long)ktaps * nck * M * KCB;
    for (long lin = blockIdx.x * (long)blockDim.x + threadIdx.x; lin < per_term; lin += (long)gridDim.x * blockDim.x) {
        const int k = (int)(lin % KCB);
        const int m = (int)((lin / KCB) % M);
        const int cc = (int)((lin / ((long)KCB * M)) % nck);
        const int t = (int)(lin / ((long)KCB * M * nck));
        const long idx = ((long)t * nck + cc) * M * KCB + pack_slab_offset(m, k);
        const int c = cc * KCB + k;
        float v = 0.f;
        if (c < C && m < Mreal) {
            const int o = transpose ? c : m, i = transpose ? m : c;
            v = w[((long)o * cin + i) * ktaps + t] * scale;
        }
        for (int q = 0; q < nterm; ++q) {
            const __bf16 h = (__bf16)v;
            out[(long)q * per_term + idx] = h;
            v -= (float)h;
        }
    }
}

long la_conv_bf16_pack_elems(int M, int C, int ktaps) { return (long)ktaps * la_cdiv(C, KCB) * pack_mp(M) * KCB; }

size_t la_conv_split_pack_bytes(int M, int C, int ktaps) {
    return (size_t)5 * la_conv_bf16_pack_elems(M, C, ktaps) * 2 + 256;
}

// |w * scale| max over the tensor -> bit pattern via atomicMax (non-negative floats order like unsigned ints)
__global__ void la_absmax_kernel(const float* __restrict__ w, long n, float scale, unsigned* __restrict__ amax_bits) {
    __shared__ float red[4];
    float m = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(w[i] * scale));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

int la_absmax_bits(const float* w, long n, unsigned* amax_bits, hipStream_t stream) {
    long b2 = la_cdiv(n, 256); if (b2 > 1024) b2 = 1024;
    hipLaunchKernelGGL(la_absmax_kernel, dim3((unsigned)b2), dim3(256), 0, stream, w, n, 1.f, amax_bits);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

__global__ void la_pack_f16_kernel(const float* __restrict__ w, _Float16* __restrict__ out, const unsigned* __restrict__ amax_bits,
                                   float* __restrict__ wscale_out, int cout, int cin, int ktaps, int transpose, float scale,
                                   int m_pad) {
    const int Mreal = transpose ? cin : cout, C = transpose ? cout : cin;
    const int M = pack_mp(m_pad > Mreal ? m_pad : Mreal);
    const int nck = (C + KCB - 1) / KCB;
    const long per_term = (long)ktaps * nck * M * KCB;
    const float ws = la_pow2_scale(__uint_as_float(*amax_bits));
    if (blockIdx.x == 0 && threadIdx.x == 0) *wscale_out = ws;
    for (long lin = blockIdx.x * (long)blockDim.x + threadIdx.x; lin < per_term; lin += (long)gridDim.x * blockDim.x) {
        const int k = (int)(lin % KCB);
        const int m = (int)((lin / KCB) % M);
        const int cc = (int)((lin / ((long)KCB * M)) % nck);
        const int t = (int)(lin / ((long)KCB * M * nck));
        const long idx = ((long)t * nck + cc) * M * KCB + pack_slab_offset(m, k);
        const int c = cc * KCB + k;
        float v = 0.f;
        if (c < C && m < Mreal) {
            const int o = transpose ? c : m, i = transpose ? m : c;
            v = w[((long)o * cin + i) * ktaps + t] * scale * ws;
        }
        const _Float16 h = (_Float16)v;
        out[idx] = h;
        out[per_term + idx] = (_Float16)(v - (float)h);
    }
}

// packs EVERY split precision into `out` (la_conv_split_pack_bytes): bf16 x3 terms, fp16 x2 terms (+ their weight scale)
int la_pack_conv_weights_bf16(const float* w, void* out, int cout, int cin, int ktaps, int transpose, int nterm,
                              hipStream_t stream, float scale, int m_pad) {
    LA_CHECK_ARG(w && out && nterm >= 1 && nterm <= 3, "pack_bf16: bad args");
    LA_CHECK_ARG(((size_t)out & 15) == 0, "pack_bf16: output must be 16-byte aligned");
    const int Mreal = transpose ? cin : cout;
    const long n = la_conv_bf16_pack_elems(m_pad > Mreal ? m_pad : Mreal, transpose ? cout : cin, ktaps);
    long blocks = la_cdiv(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_pack_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, w, (__bf16*)out, cout, cin, ktaps,
                       transpose, 3, scale, m_pad);
    char* base = static_cast<char*>(out);
    float* wscale = reinterpret_cast<float*>(base + la_conv_pack_wscale_offset(n));
    unsigned* amax = reinterpret_cast<unsigned*>(wscale) + 1;
    LA_HIP(hipMemsetAsync(amax, 0, sizeof(unsigned), stream));
    const long nw = (long)cout * cin * ktaps;
    long b2 = la_cdiv(nw, 256); if (b2 > 1024) b2 = 1024;
    hipLaunchKernelGGL(la_absmax_kernel, dim3((unsigned)b2), dim3(256), 0, stream, w, nw, scale, amax);
    hipLaunchKernelGGL(la_pack_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, w, (_Float16*)(base + pack_f16_offset(n)), amax,
                       wscale, cout, cin, ktaps, transpose, scale, m_pad);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// fp16 operand scale, pass 1: max |x * scale| of every (b, c) plane in PM_NS segments, one workgroup per segment (no atomics)
#define PM_NS 8
__global__ __launch_bounds__(256) void la_plane_absmax_kernel(const float* __restrict__ in, long in_bstride,
                                                             const float* __restrict__ scale, int scale_stride,
                                                             float* __restrict__ pm, int C, long HW, int ns) {
    __shared__ float red[4];
    const int seg = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float* ip = in + (long)b * in_bstride + (long)c * HW;
    const long per = ((HW + ns - 1) / ns + 3) & ~3l;
    const long p0 = seg * per, p1 = p0 + per < HW ? p0 + per : HW;
    float m = 0.f;
    if ((((size_t)ip | (size_t)(HW * 4)) & 15) == 0) {          // 16-byte aligned plane: float4 stream, 4 loads in flight
        const float4* ip4 = reinterpret_cast<const float4*>(ip);
        long q = p0 / 4 + threadIdx.x;
        const long q1 = p1 / 4;
        for (; q + 768 < q1; q += 1024) {
            const float4 v0 = ip4[q], v1 = ip4[q + 256], v2 = ip4[q + 512], v3 = ip4[q + 768];
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w))),
                               fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w)))));
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(v2.x), fabsf(v2.y)), fmaxf(fabsf(v2.z), fabsf(v2.w))),
                               fmaxf(fmaxf(fabsf(v3.x), fabsf(v3.y)), fmaxf(fabsf(v3.z), fabsf(v3.w)))));
        }
        for (; q < q1; q += 256) {
            const float4 v = ip4[q];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
        for (long p = q1 * 4 + threadIdx.x; p < p1; p += 256) m = fmaxf(m, fabsf(ip[p]));
    } else {
        for (long p = p0 + threadIdx.x; p < p1; p += 256) m = fmaxf(m, fabsf(ip[p]));
    }
    m *= fabsf(scale ? scale[(long)b * scale_stride + c] : 1.f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) pm[((long)b * C + c) * ns + seg] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Activation backward of the layer that produced `yref`, fused with pass 1 of the fp16 operand scale of the contraction that consumes
// the result: dx = dy * act'(yref) and the segment maxima of |dx| in one sweep (the discriminator / feature-net backward passes ran
// la_bias_act_grad_f32, la_plane_absmax_kernel and la_xscale_kernel for every backward contraction; now this kernel and
// la_xscale_pmax_kernel).  Same grid and segment layout as la_plane_absmax_kernel; dx may alias dy.
__global__ __launch_bounds__(256) void la_act_grad_pmax_kernel(const float* dy, const float* __restrict__ yref, float* dx,
                                                              float* __restrict__ pm, int C, long HW, int ns, int act, float alpha,
                                                              float gain, float clamp) {
    __shared__ float red[4];
    const int seg = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const long base = ((long)b * C + c) * HW;
    const long per = ((HW + ns - 1) / ns + 3) & ~3l;
    const long p0 = seg * per, p1 = p0 + per < HW ? p0 + per : HW;
    float m = 0.f;
    auto one = [&](float g, float y) { const float v = g * la_act_bwd_from_y(y, act, alpha, gain, clamp); m = fmaxf(m, fabsf(v)); return v; };
    if (((((size_t)(dy + base)) | ((size_t)(yref + base)) | ((size_t)(dx + base)) | (size_t)(HW * 4)) & 15) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(dy + base);
        const float4* y4 = reinterpret_cast<const float4*>(yref + base);
        float4* d4 = reinterpret_cast<float4*>(dx + base);
        long q = p0 / 4 + threadIdx.x;
        const long q1 = p1 / 4;
        for (; q + 256 < q1; q += 512) {
            const float4 ga = g4[q], gb = g4[q + 256], ya = y4[q], yb = y4[q + 256];
            d4[q] = make_float4(one(ga.x, ya.x), one(ga.y, ya.y), one(ga.z, ya.z), one(ga.w, ya.w));
            d4[q + 256] = make_float4(one(gb.x, yb.x), one(gb.y, yb.y), one(gb.z, yb.z), one(gb.w, yb.w));
        }
        for (; q < q1; q += 256) {
            const float4 ga = g4[q], ya = y4[q];
            d4[q] = make_float4(one(ga.x, ya.x), one(ga.y, ya.y), one(ga.z, ya.z), one(ga.w, ya.w));
        }
        for (long p = q1 * 4 + threadIdx.x; p < p1; p += 256) dx[base + p] = one(dy[base + p], yref[base + p]);
    } else {
        for (long p = p0 + threadIdx.x; p < p1; p += 256) dx[base + p] = one(dy[base + p], yref[base + p]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) pm[((long)b * C + c) * ns + seg] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

int la_conv_act_grad_segments(long HW) {
    int ns = (int)(HW / 8192);
    return ns < 1 ? 1 : (ns > PM_NS ? PM_NS : ns);
}

// dx [B][C][HW] = dy * act'(yref); pm [B][C][la_conv_act_grad_segments(HW)] = segment maxima of |dx| (-> LaConvArgs::in_pmax)
int la_conv_act_grad_pmax(const float* dy, const float* yref, float* dx, float* pm, int B, int C, long HW, int act, float alpha, float gain,
                          float clamp, hipStream_t stream) {
    LA_CHECK_ARG(dy && yref && dx && pm && B >= 1 && C >= 1 && HW >= 1, "act_grad_pmax: bad arguments");
    LA_CHECK_ARG(B <= 65535 && C <= 65535, "act_grad_pmax: grid too large");
    const int ns = la_conv_act_grad_segments(HW);
    hipLaunchKernelGGL(la_act_grad_pmax_kernel, dim3(ns, C, B), dim3(256), 0, stream, dy, yref, dx, pm, C, HW, ns, act, alpha, gain, clamp);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// per-sample power-of-two scale from the segment maxima: xscale[b] = pow2(max over the sample)
__global__ __launch_bounds__(256) void la_xscale_kernel(const float* __restrict__ pm, float* __restrict__ xscale, int n) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    float m = 0.f;
    for (int k = threadIdx.x; k < n; k += blockDim.x) m = fmaxf(m, pm[(long)b * n + k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) xscale[b] = la_pow2_scale(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

__global__ __launch_bounds__(1024) void la_xscale_pmax_kernel(const float* __restrict__ pmax, int nseg, const float* __restrict__ scale,
                                                             int scale_stride, float* __restrict__ xscale, int C, float mult) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const float* pb = pmax + (long)b * C * nseg;
    const float* sb = scale ? scale + (long)b * scale_stride : nullptr;
    const int n = C * nseg;
    float m = 0.f;
    if (!sb && (n & 3) == 0 && (((size_t)pb) & 15) == 0) {      // plain maximum of a contiguous array: 16-byte loads
        const float4* p4 = reinterpret_cast<const float4*>(pb);
        for (int k = threadIdx.x; k < (n >> 2); k += 1024) {
            const float4 v = p4[k];
            m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        for (int k = threadIdx.x; k < n; k += 1024) m = fmaxf(m, pb[k] * fabsf(sb ? sb[k / nseg] : 1.f));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) t = fmaxf(t, red[w]);
        xscale[b] = la_pow2_scale(mult * t);
    }
}

// xscale[b] = power-of-two operand scale of a tensor bounded by mult * max_c(|scale[b][c]| * max_seg pmax[b][c][seg])
int la_conv_xscale_from_pmax(const float* pmax, int nseg, const float* scale, int scale_stride, float mult, float* xscale, int B, int C,
                             hipStream_t stream) {
    LA_CHECK_ARG(pmax && xscale && nseg >= 1 && B >= 1 && C >= 1, "xscale_from_pmax: bad arguments");
    hipLaunchKernelGGL(la_xscale_pmax_kernel, dim3(B), dim3(1024), 0, stream, pmax, nseg, scale, scale_stride, xscale, C, mult);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// Pre-split copy for the flat kernel, CHANNEL-INTERLEAVED: q[b][chunk][pixel][32 channels]; fp16: a 128-byte record per (chunk, pixel) =
// the h terms of the 32 channels (64 B) followed by their l terms (64 B), so that a 16-byte piece is one LDS slot of one term;
// bf16: 8 B per element {h | m<<16, l}.  Channels past C are zeros.  The flat kernel's gather thread (pixel, 16-channel half) then reads its
// operand as 64 / 128 contiguous bytes (4 / 8 dwordx4) instead of 16 strided dwords, and a stride-2 gather wastes no sectors.
// One workgroup = 32 channels x 64 pixels, transposed through LDS.
struct LaInMask { const float* y; int act; float alpha, gain, clamp, in_gain; long p_lo, p_hi; };      // LaConvArgs::in_mask_* / in_gain; pixel range that is read (in_row_lo), 0 / 0 = all
template <bool F16>
__global__ __launch_bounds__(256) void la_presplit_t_kernel(const float* __restrict__ in, long in_bstride,
                                                           const float* __restrict__ scale, int scale_stride,
                                                           const float* __restrict__ xscale, int xs_fan, unsigned* __restrict__ out, int C, long HW,
                                                           LaInMask mk) {
    constexpr int EW = F16 ? 1 : 2;                           // dwords per element
    __shared__ unsigned tile[EW][64][33];
    const int cc = blockIdx.y, b = blockIdx.z, nck = gridDim.y;
    const long p0 = (long)blockIdx.x * 64;
    if (mk.p_hi > 0 && (p0 + 64 <= mk.p_lo || p0 >= mk.p_hi)) return;      // rows the launch reads as zeros anyway (LaConvArgs::in_row_lo): not copied
    const float xs = F16 ? la_xs_get(xscale, b, xs_fan) : 1.f;
    {
        const int px = threadIdx.x & 63, cg = threadIdx.x >> 6;
        const long p = p0 + px;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = cg * 8 + i, c = cc * KCB + cl;
            float v = 0.f;
            if (c < C && p < HW) {
                const long o = (long)b * in_bstride + (long)c * HW + p;
                v = in[o] * ((scale ? scale[(long)b * scale_stride + c] : 1.f) * xs);
                if (mk.y) v *= la_act_bwd_from_y(mk.y[o], mk.act, mk.alpha, mk.gain, mk.clamp);
                v *= mk.in_gain;
            }
            if (F16) {
                const _Float16 h = (_Float16)v;
                const _Float16 l = (_Float16)(v - (float)h);
                tile[0][px][cl] = (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
            } else {
                unsigned short t[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const __bf16 h = (__bf16)v;
                    t[q] = __builtin_bit_cast(unsigned short, h);
                    v -= (float)h;
                }
                tile[0][px][cl] = (unsigned)t[0] | ((unsigned)t[1] << 16);
                tile[EW - 1][px][cl] = (unsigned)t[2];
            }
        }
    }
    __syncthreads();
    {
        const int px = threadIdx.x >> 2, qt = threadIdx.x & 3;         // 8 channels of one pixel per thread
        const long p = p0 + px;
        if (p < HW) {
            unsigned* op = out + (((long)b * nck + cc) * HW + p) * (KCB * EW) + qt * 8 * EW;
            if (F16) {      // record = [h of 32 channels | l of 32 channels]: this thread's 8 channels are slot qt of each half
                unsigned e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = tile[0][px][qt * 8 + k];
                uint4* rec = reinterpret_cast<uint4*>(out + (((long)b * nck + cc) * HW + p) * KCB);
                rec[qt] = make_uint4(__builtin_amdgcn_perm(e[1], e[0], 0x05040100u), __builtin_amdgcn_perm(e[3], e[2], 0x05040100u),
                                     __builtin_amdgcn_perm(e[5], e[4], 0x05040100u), __builtin_amdgcn_perm(e[7], e[6], 0x05040100u));
                rec[4 + qt] = make_uint4(__builtin_amdgcn_perm(e[1], e[0], 0x07060302u), __builtin_amdgcn_perm(e[3], e[2], 0x07060302u),
                                         __builtin_amdgcn_perm(e[5], e[4], 0x07060302u), __builtin_amdgcn_perm(e[7], e[6], 0x07060302u));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    reinterpret_cast<uint4*>(op)[k] = make_uint4(tile[0][px][qt * 8 + 2 * k], tile[EW - 1][px][qt * 8 + 2 * k],
                                                                 tile[0][px][qt * 8 + 2 * k + 1], tile[EW - 1][px][qt * 8 + 2 * k + 1]);
            }
        }
    }
}

size_t la_conv_presplit_hdr_bytes(int B, int C) { return (PRESPLIT_HDR + (size_t)B * C * PM_NS * 4 + 255) & ~(size_t)255; }
size_t la_conv_presplit_bytes(int B, int C, int Hin, int Win) {      // channel-interleaved copy, C padded to whole chunks, 8 B / element
    return (size_t)B * la_cdiv(C, KCB) * KCB * Hin * Win * 8 + 16 + la_conv_presplit_hdr_bytes(B, C);
}

// Operand preparation of a split-precision launch as la_conv_plan laid it out (it has checked the workspace): the fp16 per-sample
// operand scale (segment maxima -> xscale[b]) in the header, the pre-split copy at p.q_off
int la_conv_prepare_input(LaConvArgs& a, const LaConvPlan& p, hipStream_t stream) {
    if (p.prep == LA_PREP_NONE) return LA_OK;      // (nothing is launched, nothing is bracketed)
    const long HW = (long)a.Hin * a.Win;
    const bool copy = p.prep == LA_PREP_PRESPLIT;
    // launch profiler: operand preparation = its own class (read the fp32 input once; the pre-split copy is written once)
    struct Bracket { int slot; hipStream_t st; ~Bracket() { la_prof_close(slot, st); } };
    const double elems = 4.0 * a.B * (double)a.C * HW, in_reads = a.in_bstride ? 1.0 : 1.0 / a.B;
    Bracket br{la_prof_open(LA_PC_PRESPLIT, 0.0, copy ? elems * (in_reads + 1.0) : (a.in_pmax ? 0.0 : elems * in_reads), stream), stream};
    char* base = static_cast<char*>(a.ws);
    if (p.scale_pass) {
        float* xscale = reinterpret_cast<float*>(base);
        float* pm = reinterpret_cast<float*>(base + PRESPLIT_HDR);       // segment maxima [B][C][ns]
        const int ns = la_conv_act_grad_segments(HW);
        if (a.in_pmax)      // the producer of `in` already reduced every plane: max over the sample of |style| * plane max
            hipLaunchKernelGGL(la_xscale_pmax_kernel, dim3(a.B), dim3(1024), 0, stream, a.in_pmax, a.in_pmax_nseg > 0 ? a.in_pmax_nseg : 1, a.in_scale,
                               a.scale_stride, xscale, a.C, 1.f);
        else {
            hipLaunchKernelGGL(la_plane_absmax_kernel, dim3(ns, a.C, a.B), dim3(256), 0, stream, a.in, a.in_bstride, a.in_scale,
                               a.scale_stride, pm, a.C, HW, ns);
            hipLaunchKernelGGL(la_xscale_kernel, dim3(a.B), dim3(256), 0, stream, pm, xscale, a.C * ns);
        }
        LA_CHECK_LAUNCH();
        a.acc_scale_x = xscale; a.acc_scale_fan = 1;
    }
    if (copy) {
        const dim3 pgrid((unsigned)la_cdiv(HW, 64), (unsigned)la_cdiv(a.C, KCB), (unsigned)a.B);
        const LaInMask mk{a.in_mask_y, a.in_mask_act, a.in_mask_alpha, a.in_mask_gain, a.in_mask_clamp, a.in_gain != 0.f ? a.in_gain : 1.f,
                          a.in_row_hi > 0 ? (long)a.in_row_lo * a.Win : 0, a.in_row_hi > 0 ? (long)a.in_row_hi * a.Win : 0};
        unsigned* q = reinterpret_cast<unsigned*>(base + p.q_off);
        if (a.precision == LA_PREC_F16X2)
            hipLaunchKernelGGL(la_presplit_t_kernel<true>, pgrid, dim3(256), 0, stream, a.in, a.in_bstride, a.in_scale, a.scale_stride,
                               a.acc_scale_x, a.acc_scale_fan, q, a.C, HW, mk);
        else
            hipLaunchKernelGGL(la_presplit_t_kernel<false>, pgrid, dim3(256), 0, stream, a.in, a.in_bstride, a.in_scale, a.scale_stride,
                               (const float*)nullptr, 0, q, a.C, HW, mk);
        LA_CHECK_LAUNCH();
        a.in_q = q;
    }
    a.ws = a.ws_bytes > p.ws_head ? base + p.ws_head : nullptr;
    a.ws_bytes -= p.ws_head;
    return LA_OK;
}
