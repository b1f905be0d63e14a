// Index arithmetic of the detector's image preparation (la_detector.hip) and the tiling of its fully connected kernel, host and device:
// the kernels call it, and a host program can include it on its own (nothing here needs the HIP runtime).
//   area      torch's F.interpolate(mode='area') == adaptive_avg_pool2d: output i averages the input bin [lo, hi),
//             lo = floor(i * in / out), hi = ceil((i + 1) * in / out).  Bins of neighbouring outputs may overlap (non-integer ratios) and
//             an up-sampling bin is one pixel.  1 <= hi - lo, 0 <= lo, hi <= in for every 0 <= i < out.
//   bilinear  align_corners=False without antialiasing: src = (i + 0.5) * (in / out) - 0.5 clipped below at 0, neighbours floor(src) and
//             the next pixel (the last pixel is its own neighbour), weights (1 - t, t) with t = src - floor(src).
//   fc        la_fc_bias_act_f32's tile and K-slice count (la_fc_plan), so that workspace size, launch and tests agree on one statement.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LA_DET_HD __host__ __device__ inline
#else
#define LA_DET_HD inline
#endif

#ifndef LA_DET_AREA          /* (the public header defines the same two) */
#define LA_DET_AREA 0
#define LA_DET_BILINEAR 1
#endif

LA_DET_HD int la_det_area_lo(int i, int in, int out) { return (int)(((long)i * in) / out); }
LA_DET_HD int la_det_area_hi(int i, int in, int out) { return (int)(((long)(i + 1) * in + out - 1) / out); }

template <class A>
struct LaDetLerp { int i0, i1; A w0, w1; };

// (torch computes the scale and the position in the arithmetic type of the data: A = float in the kernel, double in a check)
template <class A>
LA_DET_HD LaDetLerp<A> la_det_bilinear(int i, int in, int out) {
    LaDetLerp<A> r;
    const A scale = (A)in / (A)out;
    A src = ((A)i + (A)0.5) * scale - (A)0.5;
    if (src < (A)0) src = (A)0;
    int i0 = (int)src;                      // src >= 0: truncation is floor
    if (i0 > in - 1) i0 = in - 1;
    r.i0 = i0;
    r.i1 = i0 < in - 1 ? i0 + 1 : i0;
    r.w1 = src - (A)i0;
    r.w0 = (A)1 - r.w1;
    return r;
}

// ---------------------------------------------------------------- fully connected kernel: tiles and K slices
#define LA_FC_OT 128          // output features per workgroup (4 waves x 32)
#define LA_FC_KC 32           // K elements per staged chunk
#define LA_FC_NB_MAX 2        // 32-row blocks of the batch per workgroup: N <= 32 -> 1, else 2 (a 64-row batch tile)
#define LA_FC_WG_TARGET 768   // resident workgroups aimed at: 3 per CU (LDS: 50 KB each) on 256 CUs
#define LA_FC_KS_MAX 64
#define LA_FC_MIN_CHUNKS 4    // at least 4 chunks (128 K elements) per slice

struct LaFcPlan {
    int nb;          // 32-row batch blocks per workgroup (1 | 2)
    int ntiles;      // batch tiles of 32 * nb rows
    int otiles;      // tiles of LA_FC_OT output features
    long nchunk;     // chunks of LA_FC_KC along K (the last one may be ragged)
    long per;        // chunks per K slice
    int ks;          // K slices (1: the kernel writes y itself; > 1: partials + a fixed-order finish pass)
    int vec;         // 16-byte loads along K (K % 4 == 0; the pointers' alignment is tested by the launch)
};

LA_DET_HD LaFcPlan la_fc_plan(long N, long K, long O) {
    LaFcPlan p;
    p.nb = N > 32 ? 2 : 1;
    p.ntiles = (int)((N + 32 * p.nb - 1) / (32 * p.nb));
    p.otiles = (int)((O + LA_FC_OT - 1) / LA_FC_OT);
    p.nchunk = (K + LA_FC_KC - 1) / LA_FC_KC;
    long ks = (LA_FC_WG_TARGET + (long)p.ntiles * p.otiles - 1) / ((long)p.ntiles * p.otiles);
    if (ks > LA_FC_KS_MAX) ks = LA_FC_KS_MAX;
    const long by_len = p.nchunk / LA_FC_MIN_CHUNKS > 1 ? p.nchunk / LA_FC_MIN_CHUNKS : 1;
    if (ks > by_len) ks = by_len;
    if (ks < 1) ks = 1;
    p.per = (p.nchunk + ks - 1) / ks;
    p.ks = (int)((p.nchunk + p.per - 1) / p.per);
    p.vec = K % 4 == 0;
    return p;
}
