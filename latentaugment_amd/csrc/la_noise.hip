// Gradient with respect to a layer's noise map out of the synthesis backward pass (la_synth_backward_noise, la_synth.hip).
// The backward seams (la_style.hip, and the fused ones in the contraction epilogues) store gz = dL/dz * act' * d[b][c] per output
// channel, and the noise enters every channel of a layer alike, in front of the activation:
//   gn[b][p] = strength * sum_c gz[b][c][p] / d[b][c]
// A channel reduction that reads gz once: HBM-bound, no atomics, float32 sums in an order fixed by the shape alone.
#include "la_common.h"

// Planes of at least LA_NG_SMALL_HW pixels.  A workgroup is PG pixel groups (one float4 of 4 contiguous pixels each) x CSL channel slices,
// PG * CSL = 256, thread t = slice * PG + group: a thread walks the channels slice, slice + CSL, ... of its four pixels, the slices of a
// group are then added in slice order through LDS.  The host picks CSL so that a small plane count still fills the chip.
#define LA_NG_SMALL_HW 256

template <int CSL>
__global__ __launch_bounds__(256) void la_noise_grad_kernel(const float* __restrict__ gz, const float* __restrict__ d, long d_stride, int C, long HW,
                                                           long groups, float strength, float* __restrict__ gn) {
    constexpr int PG = 256 / CSL;
    __shared__ float4 red[CSL > 1 ? 256 : 1];
    const int pg = threadIdx.x % PG, cs = threadIdx.x / PG;
    const long g = (long)blockIdx.x * PG + pg;      // float4 group of the [B][HW] output
    const bool live = g < groups;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    long b = 0, p = 0;
    if (live) {
        const long per = HW >> 2;
        b = g / per; p = (g - b * per) << 2;
        const float* src = gz + (b * C) * HW + p;
        const float* dr = d + b * d_stride;
#pragma unroll 4
        for (int c = cs; c < C; c += CSL) {
            const float4 v = *reinterpret_cast<const float4*>(src + (long)c * HW);
            const float rinv = 1.f / dr[c];
            acc.x += v.x * rinv; acc.y += v.y * rinv; acc.z += v.z * rinv; acc.w += v.w * rinv;
        }
    }
    if (CSL > 1) {
        red[threadIdx.x] = acc;
        __syncthreads();
        if (cs != 0) return;
        for (int s = 1; s < CSL; ++s) {
            const float4 o = red[s * PG + pg];
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
    }
    if (live) *reinterpret_cast<float4*>(gn + b * HW + p) = make_float4(strength * acc.x, strength * acc.y, strength * acc.z, strength * acc.w);
}

// Small planes (4 x 4 and 8 x 8, where the channel count is at its largest): one wave per output pixel, lane l adds channels l, l + 64, ...,
// then the xor butterfly of la_common.h.
__global__ __launch_bounds__(256) void la_noise_grad_small_kernel(const float* __restrict__ gz, const float* __restrict__ d, long d_stride, int C, long HW,
                                                                 long outs, float strength, float* __restrict__ gn) {
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (uniform over a wave)
    if (o >= outs) return;
    const int lane = threadIdx.x & 63;
    const long b = o / HW, p = o - b * HW;
    const float* src = gz + (b * C) * HW + p;
    const float* dr = d + b * d_stride;
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc += src[(long)c * HW] / dr[c];
    acc = la_wave_sum(acc);
    if (lane == 0) gn[o] = strength * acc;
}

extern "C" int la_noise_grad_f32(const float* gz, const float* d, long d_stride, int B, int C, long HW, float strength, float* gn, hipStream_t stream) {
    LA_CHECK_ARG(gz && d && gn, "noise_grad: null pointer");
    LA_CHECK_ARG(B >= 1 && C >= 1 && HW >= 4 && HW % 4 == 0 && d_stride >= 0, "noise_grad: B, C at least 1, HW a multiple of 4");
    LA_CHECK_ARG(((uintptr_t)gz | (uintptr_t)gn) % 16 == 0 && (uintptr_t)d % sizeof(float) == 0, "noise_grad: gz and gn must be 16-byte aligned");
    LA_CHECK_ARG((long)B * HW <= 0x7fffffffl, "noise_grad: tensor too large");
    if (HW < LA_NG_SMALL_HW) {
        const long outs = (long)B * HW;
        hipLaunchKernelGGL(la_noise_grad_small_kernel, dim3((unsigned)la_cdiv(outs, 4)), dim3(256), 0, stream, gz, d, d_stride, C, HW, outs, strength, gn);
    } else {
        // channel slices: as few as give every CU a few workgroups (256 CUs; a slice count is a power of two that divides 256)
        const long groups = (long)B * HW / 4;
        const int csl = groups >= 256l * 1024 ? 1 : (groups >= 64l * 1024 || C < 16) ? 4 : 16;
#define LAUNCH(N) hipLaunchKernelGGL(la_noise_grad_kernel<N>, dim3((unsigned)la_cdiv(groups, 256 / N)), dim3(256), 0, stream, gz, d, d_stride, C, HW, groups, strength, gn)
        if (csl == 1) LAUNCH(1); else if (csl == 4) LAUNCH(4); else LAUNCH(16);
#undef LAUNCH
    }
    LA_CHECK_LAUNCH();
    return LA_OK;
}
