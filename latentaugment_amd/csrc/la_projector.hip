// Projector (inversion of images into W / W+, Karras et al. 2020, Appendix D, without the noise maps): the three kernels that are
// specific to it.  The optimisation itself is an eager sequence of launches over the synthesis and feature engines (projector.py).
//   la_row_dist_f32     loss[j] = scale * sum_c sum_k (a - t)^2 over rows c * (rows / fold) + j, and g (+)= gscale * (a - t)
//   la_box_down_f32     [planes][R][R] -> [planes][R / k][R / k], the mean of k x k boxes;  la_box_up_f32: its adjoint
//   la_proj_step_tail_f32   W-space row sum + Adam + the next step's noised latent in one launch
// No atomics anywhere: two runs give the same bits.
#include "la_common.h"
#include "la_rng.h"

#include <math.h>

// ------------------------------------------------------------------------------------------------------------
// Row-to-own-target distance.  A workgroup takes one chunk of LA_RD_CHUNK elements of one row: the difference is formed in float32,
// its square accumulated in float64 -- per thread in element order, then lanes by xor-shuffle, then the four waves in order -- and the
// chunk's sum stored as partial[row][chunk].  The finish launch adds the partials of an output's rows in (row, chunk) order: thread i
// takes partials i, i + 64, ..., then the same shuffle.  Every order is fixed by the shape alone.
#define LA_RD_CHUNK 8192      // elements per workgroup: 256 threads x 8 float4

template <bool VEC>
__global__ __launch_bounds__(256) void la_row_dist_kernel(const float* __restrict__ a, const float* __restrict__ t, float* __restrict__ g,
                                                         long K, int chunks, float gscale, int accumulate, double* __restrict__ partial) {
    __shared__ double red[4];
    const long row = blockIdx.y;
    const long k0 = (long)blockIdx.x * LA_RD_CHUNK;
    const long k1 = k0 + LA_RD_CHUNK < K ? k0 + LA_RD_CHUNK : K;
    const float* ar = a + row * K;
    const float* tr = t + row * K;
    float* gr = g ? g + row * K : nullptr;
    double acc = 0.0;
    if (VEC) {      // (all three rows 16-byte aligned and K % 4 == 0: checked by the host)
        for (long k = k0 + 4 * (long)threadIdx.x; k < k1; k += 4 * 256) {
            const float4 av = *reinterpret_cast<const float4*>(ar + k), tv = *reinterpret_cast<const float4*>(tr + k);
            const float d0 = av.x - tv.x, d1 = av.y - tv.y, d2 = av.z - tv.z, d3 = av.w - tv.w;
            acc += (double)d0 * (double)d0; acc += (double)d1 * (double)d1; acc += (double)d2 * (double)d2; acc += (double)d3 * (double)d3;
            if (gr) {
                float4 gv = make_float4(gscale * d0, gscale * d1, gscale * d2, gscale * d3);
                if (accumulate) {
                    const float4 old = *reinterpret_cast<const float4*>(gr + k);
                    gv.x += old.x; gv.y += old.y; gv.z += old.z; gv.w += old.w;
                }
                *reinterpret_cast<float4*>(gr + k) = gv;
            }
        }
    } else {
        for (long k = k0 + threadIdx.x; k < k1; k += 256) {
            const float d = ar[k] - tr[k];
            acc += (double)d * (double)d;
            if (gr) gr[k] = accumulate ? gr[k] + gscale * d : gscale * d;
        }
    }
    acc = la_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[row * chunks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void la_row_dist_finish_kernel(const double* __restrict__ partial, int chunks, int outs, int fold, double scale,
                                                               double* __restrict__ loss, long loss_stride) {
    const int j = blockIdx.x;
    double acc = 0.0;
    for (int c = 0; c < fold; ++c) {
        const double* p = partial + ((long)c * outs + j) * chunks;
        for (int i = threadIdx.x; i < chunks; i += 64) acc += p[i];
    }
    acc = la_wave_sum(acc);
    if (threadIdx.x == 0) loss[(long)j * loss_stride] = scale * acc;
}

static long la_row_dist_chunks(long K) { return (K + LA_RD_CHUNK - 1) / LA_RD_CHUNK; }

extern "C" size_t la_row_dist_workspace_bytes(int rows, long K) {
    if (rows < 1 || K < 1) return 0;
    return la_align64((size_t)rows * (size_t)la_row_dist_chunks(K) * sizeof(double));
}

extern "C" int la_row_dist_f32(const float* a, const float* t, int rows, long K, int fold, double scale, float gscale, float* g, int accumulate,
                               double* loss, long loss_stride, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(a && t && loss && ws, "row_dist: null pointer");
    LA_CHECK_ARG(rows >= 1 && rows <= 65535 && K >= 1, "row_dist: rows must be 1 .. 65535 and K at least 1");
    LA_CHECK_ARG(fold >= 1 && rows % fold == 0, "row_dist: fold must divide rows");
    LA_CHECK_ARG(loss_stride >= 1, "row_dist: loss_stride must be at least 1");
    LA_CHECK_ARG(((uintptr_t)a | (uintptr_t)t | (uintptr_t)g) % sizeof(float) == 0 && (uintptr_t)loss % sizeof(double) == 0 &&
                 (uintptr_t)ws % sizeof(double) == 0, "row_dist: pointer not aligned to its element type");
    const long chunks = la_row_dist_chunks(K);
    LA_CHECK_ARG(chunks <= 0x7fffffffl, "row_dist: K too large");
    if (ws_bytes < la_row_dist_workspace_bytes(rows, K)) {
        la_set_error("row_dist: workspace too small (la_row_dist_workspace_bytes)");
        return LA_ERR_WORKSPACE;
    }
    const bool vec = K % 4 == 0 && ((uintptr_t)a | (uintptr_t)t | (uintptr_t)g) % 16 == 0;
    double* partial = (double*)ws;
    if (vec)
        hipLaunchKernelGGL(la_row_dist_kernel<true>, dim3((unsigned)chunks, rows), dim3(256), 0, stream, a, t, g, K, (int)chunks, gscale, accumulate, partial);
    else
        hipLaunchKernelGGL(la_row_dist_kernel<false>, dim3((unsigned)chunks, rows), dim3(256), 0, stream, a, t, g, K, (int)chunks, gscale, accumulate, partial);
    LA_CHECK_LAUNCH();
    hipLaunchKernelGGL(la_row_dist_finish_kernel, dim3(rows / fold), dim3(64), 0, stream, (const double*)partial, (int)chunks, rows / fold, fold, scale, loss,
                       loss_stride);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Box down-sampling by an integer factor: y[p][oy][ox] = (1 / k^2) * sum_{dy, dx < k} x[p][k oy + dy][k ox + dx], added in (dy, dx) order
// and scaled once -- for k a power of two the factor is exact, so integer-valued planes come out exact.  The adjoint spreads
// gy / k^2 over the box.  One thread per output element of either kernel.
__global__ __launch_bounds__(256) void la_box_down_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int S, int k, float inv, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    const long p = i / ((long)S * S);
    const float* src = x + (p * R + (long)oy * k) * R + (long)ox * k;
    float acc = 0.f;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) acc += src[(long)dy * R + dx];
    y[i] = acc * inv;
}

__global__ __launch_bounds__(256) void la_box_up_kernel(const float* __restrict__ gy, float* __restrict__ gx, int R, int S, int k, float inv, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int X = (int)(i % R), Y = (int)((i / R) % R);
    const long p = i / ((long)R * R);
    gx[i] = gy[(p * S + Y / k) * S + X / k] * inv;
}

static int la_box_check(const void* a, const void* b, long planes, int R, int k) {
    LA_CHECK_ARG(a && b, "box_down / box_up: null pointer");
    LA_CHECK_ARG(k == 1 || k == 2 || k == 4 || k == 8, "box_down / box_up: the factor k must be 1, 2, 4 or 8");
    LA_CHECK_ARG(planes >= 1 && R >= k && R % k == 0, "box_down / box_up: planes at least 1 and R a multiple of k");
    LA_CHECK_ARG(planes * R * R <= 0x7fffffffl * 256l, "box_down / box_up: tensor too large");
    return LA_OK;
}

extern "C" int la_box_down_f32(const float* x, float* y, long planes, int R, int k, hipStream_t stream) {
    const int rc = la_box_check(x, y, planes, R, k);
    if (rc) return rc;
    const int S = R / k;
    const long total = planes * S * S;
    hipLaunchKernelGGL(la_box_down_kernel, dim3((unsigned)la_cdiv(total, 256)), dim3(256), 0, stream, x, y, R, S, k, 1.f / (float)(k * k), total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_box_up_f32(const float* gy, float* gx, long planes, int R, int k, hipStream_t stream) {
    const int rc = la_box_check(gy, gx, planes, R, k);
    if (rc) return rc;
    const int S = R / k;
    const long total = planes * R * R;
    hipLaunchKernelGGL(la_box_up_kernel, dim3((unsigned)la_cdiv(total, 256)), dim3(256), 0, stream, gy, gx, R, S, k, 1.f / (float)(k * k), total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Step tail.  The latent p is [B][L][wdim] with L = 1 (W) or num_ws (W+); a thread owns the four consecutive elements 4q .. 4q + 3 of
// one sample's row of L * wdim elements, i.e. one Philox counter of the noise stream.  Per element (slot l, column j):
//   gradient  W: dws[b][0][j] + dws[b][1][j] + ... in slot order (float32);  W+: dws[b][l][j]
//   Adam      la_adam_update with the bias corrections of the 1-based `step` (the powf / sqrtf of la_adam_step_f32, taken by the host)
//   ws        p + sigma * n, n the unit normal of (seed, layer, row0 + b, element): the stream of la_noise_normal_f32 (la_rng.h)
// dws null: no update, only ws is written (the start of a run).
__global__ __launch_bounds__(256) void la_proj_step_tail_kernel(const float* __restrict__ dws, float* __restrict__ p, float* __restrict__ m,
                                                               float* __restrict__ v, float* __restrict__ ws, int B, int num_ws, int wdim, int L,
                                                               float step_size, float bc2_sqrt, float b1, float b2, float eps, float sigma,
                                                               unsigned k0, unsigned k1, unsigned layer, long row0) {
    const long row_elems = (long)L * wdim;
    const long q4 = (row_elems + 3) >> 2;
    const long gidx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gidx >= (long)B * q4) return;
    const long b = gidx / q4, q = gidx - b * q4;
    unsigned x[4];
    la_noise_words(q, row0 + b, layer, k0, k1, x);
    float z[4];
    la_unit_normals4(x, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = 4 * q + k;
        if (e >= row_elems) break;
        const long i = b * row_elems + e;
        float pv = p[i];
        if (dws) {
            float gsum;
            if (L == 1) {
                gsum = 0.f;
                for (int l = 0; l < num_ws; ++l) gsum += dws[(b * num_ws + l) * wdim + e];
            } else {
                gsum = dws[i];
            }
            float mv = m[i], vv = v[i];
            la_adam_update(pv, mv, vv, gsum, step_size, bc2_sqrt, b1, b2, eps);
            p[i] = pv; m[i] = mv; v[i] = vv;
        }
        ws[i] = pv + sigma * z[k];
    }
}

extern "C" int la_proj_step_tail_f32(const float* dws, float* p, float* m, float* v, float* ws, int B, int num_ws, int wdim, int wplus, int step,
                                     float lr, float beta1, float beta2, float eps, float sigma, unsigned long long seed, unsigned layer, long row0,
                                     hipStream_t stream) {
    LA_CHECK_ARG(p && ws && (!dws || (m && v)), "proj_step_tail: null pointer");
    LA_CHECK_ARG(B >= 1 && num_ws >= 1 && wdim >= 1, "proj_step_tail: B, num_ws and wdim must be at least 1");
    LA_CHECK_ARG(!dws || step >= 1, "proj_step_tail: the Adam step is 1-based");
    LA_CHECK_ARG(row0 >= 0 && row0 + B <= 0xffffffffl, "proj_step_tail: row index exceeds 32 bits");
    const int L = wplus ? num_ws : 1;
    float step_size = 0.f, bc2s = 1.f;
    if (dws) {
        step_size = lr / (1.f - powf(beta1, (float)step));
        bc2s = sqrtf(1.f - powf(beta2, (float)step));
    }
    const long n = (long)B * (((long)L * wdim + 3) >> 2);
    hipLaunchKernelGGL(la_proj_step_tail_kernel, dim3((unsigned)la_cdiv(n, 256)), dim3(256), 0, stream, dws, p, m, v, ws, B, num_ws, wdim, L, step_size, bc2s,
                       beta1, beta2, eps, sigma, (unsigned)seed, (unsigned)(seed >> 32), layer, row0);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
