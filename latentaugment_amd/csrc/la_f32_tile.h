// The LDS-staged exact-fp32 tile loop (v_mfma_f32_32x32x2_f32) shared by la_conv_wgrad_mfma_kernel (la_conv_op.hip), la_kid_tile_kernel
// (la_metrics.hip), la_fc_mfma_kernel (la_detector.hip) and la_featconv_gemm_kernel (la_feat_conv.hip): operands go through registers
// into two LDS buffers, and the next chunk's global loads are in flight while the current chunk multiplies, one barrier per chunk.
// la_dc_tile_kernel (la_metrics.hip, fp16 operands) takes la_tile_pipeline alone.  Written out where it stays: la_conv_igemm_kernel
// (la_conv.hip: in this form its <128, false> instance goes from 184 to 236 VGPRs and <64, false> loads through flat instructions)
// and the inner product of la_featconv_gemm_kernel (weight tile [co][k + 1]); tests/test_host_cpu.py lists both.
// f32 C/D layout of a 32 x 32 tile: column = lane & 31, row = la_mfma32_row(reg, lane >> 5).
#pragma once
#include "la_common.h"

typedef float la_f32x16 __attribute__((ext_vector_type(16)));

template <int TM, int TN>
__device__ __forceinline__ void la_f32_tile_zero(la_f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// Chunks [c_beg, c_end) of a K walk.  prefetch(ci): global memory -> registers; stage(buf): registers -> LDS buffer buf;
// compute(buf, ci): multiplies the chunk staged in buffer buf.  Contract: every thread of the workgroup must reach it (an empty range
// included: it still meets one barrier); LDS is free on return; buffer buf ^ 1 is written only after the barrier that ends the last
// read of it (iteration ci - 1's), and read only after the barrier that follows the write.  The closures are taken by reference: a
// copy would hide the address space of the pointers they capture from the compiler (flat instead of global loads).
template <class Idx, class Prefetch, class Stage, class Compute>
__device__ __forceinline__ void la_tile_pipeline(Idx c_beg, Idx c_end, Prefetch&& prefetch, Stage&& stage, Compute&& compute) {
    if (c_beg < c_end) {
        prefetch(c_beg);
        stage(0);
    }
    __syncthreads();
    for (Idx ci = c_beg; ci < c_end; ++ci) {
        const int buf = (int)(ci - c_beg) & 1;
        if (ci + 1 < c_end) prefetch(ci + 1);
        compute(buf, ci);
        if (ci + 1 < c_end) stage(buf ^ 1);
        __syncthreads();
    }
}

// acc[i][j] += the chunk staged in buffer buf of As / Bs ([2][KC][cols + pad], whole arrays by reference so that they stay LDS to the
// compiler): KC / 2 steps, each reading TM fragments As[buf][2 kp + lh][a0 + 32 i + l31] and TN fragments of Bs (from b0), then
// TM x TN MFMAs in (i, j) order.  One k order whatever the tile: every accumulator is one k-ordered chain.
template <int KC, int TM, int TN, int LDA, int LDB>
__device__ __forceinline__ void la_f32_tile_mma(const float (&As)[2][KC][LDA], const float (&Bs)[2][KC][LDB], int buf, int a0, int b0, int l31,
                                                int lh, la_f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int kp = 0; kp < KC / 2; ++kp) {
        float av[TM], bv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) av[i] = As[buf][2 * kp + lh][a0 + i * 32 + l31];
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = Bs[buf][2 * kp + lh][b0 + j * 32 + l31];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
}

// chunks [*beg, *end) of K slice `slice`: `per` chunks each, the last slice takes what is left of nchunk
template <class Idx>
__device__ __forceinline__ void la_slice_range(unsigned slice, Idx per, Idx nchunk, Idx* beg, Idx* end) {
    *beg = (Idx)slice * per;
    *end = *beg + per < nchunk ? *beg + per : nchunk;
}

// element idx of the ks slice partials part[slice * stride + idx], summed in slice order: slice 0 first, then 1 .. ks - 1 (the same
// bits on every run)
__device__ __forceinline__ float la_slices_sum(const float* __restrict__ part, long idx, long stride, int ks) {
    float s = part[idx];
    for (int k = 1; k < ks; ++k) s += part[(long)k * stride + idx];
    return s;
}
