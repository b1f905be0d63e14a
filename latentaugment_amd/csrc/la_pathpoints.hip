// Points on latent paths (no reference counterpart): the inputs of perceptual path length.
//   la_path_points_f32        out[k][p][r][:] = the point of path p (from a[p] to b[p]) at parameter t[p] + dt[k], r < reps copies:
//                             lerp (W space) or the slerp of the published PPL (Z space), in double, rounded once to float32.
// One workgroup per path; the slerp's sums are block reductions in a fixed order, no atomics: two runs give the same bits.
#include "la_common.h"

#define PP_MAXT 64
#define PP_THREADS 256

struct PpArgs {
    const float* a;        // [N][D]
    const float* b;
    const float* t;        // [N]
    float* out;            // [T][N][reps][D]
    long N;
    int D, reps, T;
    double dt[PP_MAXT];
};

// Sum over the 256 threads of the workgroup: xor butterfly inside a wave, then the four wave sums in wave order.  `red` is 4 doubles of
// LDS.  Every thread must reach it; all get the result.
__device__ __forceinline__ double pp_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ void pp_store(const PpArgs& g, int k, long p, int i, float v) {
    float* o = g.out + (((long)k * g.N + p) * g.reps) * g.D + i;
    for (int r = 0; r < g.reps; ++r) o[(long)r * g.D] = v;
}

// grid (N), 256 threads; thread i owns elements i, i + 256, .. of the row
template <int MODE>
__global__ __launch_bounds__(PP_THREADS) void la_path_points_kernel(PpArgs g) {
    // every double product and sum is rounded on its own, in the order written: the lerp equals its numpy float64 restatement bit for bit
#pragma clang fp contract(off)
    __shared__ double red[4];
    const long p = blockIdx.x;
    const int tid = threadIdx.x;
    const float* pa = g.a + p * g.D;
    const float* pb = g.b + p * g.D;
    const double t0 = (double)g.t[p];
    if (MODE == 0) {
        for (int i = tid; i < g.D; i += PP_THREADS) {
            const double av = (double)pa[i], dv = (double)pb[i] - av;
            for (int k = 0; k < g.T; ++k) pp_store(g, k, p, i, (float)(av + dv * (t0 + g.dt[k])));
        }
        return;
    }
    double saa = 0.0, sbb = 0.0;
    for (int i = tid; i < g.D; i += PP_THREADS) {
        const double av = (double)pa[i], bv = (double)pb[i];
        saa += av * av;
        sbb += bv * bv;
    }
    const double na = sqrt(pp_block_sum(saa, red)), nb = sqrt(pp_block_sum(sbb, red));
    double sab = 0.0;
    for (int i = tid; i < g.D; i += PP_THREADS) sab += ((double)pa[i] / na) * ((double)pb[i] / nb);
    const double d = pp_block_sum(sab, red);
    double scc = 0.0;
    for (int i = tid; i < g.D; i += PP_THREADS) {
        const double au = (double)pa[i] / na, cv = (double)pb[i] / nb - d * au;
        scc += cv * cv;
    }
    const double nc = sqrt(pp_block_sum(scc, red));
    if (nc == 0.0) {          // identical or opposite directions: every point is the normalised a (uniform over the workgroup)
        for (int i = tid; i < g.D; i += PP_THREADS) {
            const float v = (float)((double)pa[i] / na);
            for (int k = 0; k < g.T; ++k) pp_store(g, k, p, i, v);
        }
        return;
    }
    const double omega = atan2(nc, d);          // acos(d): |b' - d a'| is the sine of the angle; keeps its digits next to d = +-1
    for (int k = 0; k < g.T; ++k) {
        const double th = (t0 + g.dt[k]) * omega;
        const double cs = cos(th), sn = sin(th);
        double spp = 0.0;
        for (int i = tid; i < g.D; i += PP_THREADS) {
            const double au = (double)pa[i] / na, cu = ((double)pb[i] / nb - d * au) / nc;
            const double q = au * cs + cu * sn;
            spp += q * q;
        }
        const double np_ = sqrt(pp_block_sum(spp, red));
        for (int i = tid; i < g.D; i += PP_THREADS) {
            const double au = (double)pa[i] / na, cu = ((double)pb[i] / nb - d * au) / nc;
            pp_store(g, k, p, i, (float)((au * cs + cu * sn) / np_));
        }
    }
}

extern "C" int la_path_points_f32(const float* a, const float* b, const float* t, const double* dt_host, int T, int N, int D, int reps,
                                  int mode, float* out, hipStream_t stream) {
    LA_CHECK_ARG(a && b && t && dt_host && out, "path_points: null pointer");
    LA_CHECK_ARG(N >= 1 && D >= 1 && reps >= 1, "path_points: N, D and reps must be at least 1");
    LA_CHECK_ARG(T >= 1 && T <= PP_MAXT, "path_points: T must lie in 1 .. 64");
    LA_CHECK_ARG(mode == 0 || mode == 1, "path_points: mode must be 0 (lerp) or 1 (slerp)");
    PpArgs g;
    g.a = a; g.b = b; g.t = t; g.out = out;
    g.N = N; g.D = D; g.reps = reps; g.T = T;
    for (int k = 0; k < PP_MAXT; ++k) g.dt[k] = k < T ? dt_host[k] : 0.0;
    if (mode == 0) hipLaunchKernelGGL(la_path_points_kernel<0>, dim3(N), dim3(PP_THREADS), 0, stream, g);
    else hipLaunchKernelGGL(la_path_points_kernel<1>, dim3(N), dim3(PP_THREADS), 0, stream, g);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
