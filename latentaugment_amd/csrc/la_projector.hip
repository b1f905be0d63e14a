// Projector (inversion of images into W / W+, Karras et al. 2020, Appendix D): the kernels that are specific to it -- three for the
// latent, and the regulariser and step tail of the per-layer noise maps, which are optimised on request (second half of the file).  The optimisation itself is an eager sequence of launches over the synthesis and feature engines (projector.py).
//   la_row_dist_f32     loss[j] = scale * sum_c sum_k (a - t)^2 over rows c * (rows / fold) + j, and g (+)= gscale * (a - t)
//   la_box_down_f32     [planes][R][R] -> [planes][R / k][R / k], the mean of k x k boxes;  la_box_up_f32: its adjoint
//   la_proj_step_tail_f32   W-space row sum + Adam + the next step's noised latent in one launch
//   la_noise_reg_f32    the published noise regulariser over a table of maps, with its gradient as a gather
//   la_proj_noise_tail_f32  Adam + re-normalisation of every map
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
    LA_CHECK_ARG(la_aligned<4>(a, t, g) && la_aligned<8>(loss, ws), "row_dist: pointer not aligned to its element type");
    const long chunks = la_row_dist_chunks(K);
    LA_CHECK_ARG(chunks <= 0x7fffffffl, "row_dist: K too large");
    LA_CHECK_WORKSPACE(ws_bytes, la_row_dist_workspace_bytes(rows, K), "row_dist: workspace too small (la_row_dist_workspace_bytes)");
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

// ------------------------------------------------------------------------------------------------------------
// Noise maps.  The published projector optimises the per-layer noise maps beside the latent, keeps them noise-like with a regulariser,
// re-normalises them after every step and throws them away at the end.  A call takes the maps of ONE batch as a table: map i is
// [B][res[i]][res[i]], res[i] = 4 << k.  The launches are table-driven: one grid covers every (map, sample, chunk).
#define LA_NZ_MAXMAPS 32      // (an engine has at most 2 * 12 conv layers)
#define LA_NZ_MAXLEV 10       // pyramid levels of a 4096^2 map: 4096 .. 8

// A flat grid over (map, sample, chunk): the workgroups of map i are start[i] .. start[i + 1] - 1, sample-major, chunks[i] per sample
// (0: the map takes no part in the launch).
struct LaMapGrid { int nmaps, B; int chunks[LA_NZ_MAXMAPS]; int start[LA_NZ_MAXMAPS + 1]; };

static long la_map_grid(LaMapGrid& g, const int* chunks, int nmaps, int B) {
    g.nmaps = nmaps; g.B = B; g.start[0] = 0;
    long total = 0;
    for (int i = 0; i < nmaps; ++i) { g.chunks[i] = chunks[i]; total += (long)B * chunks[i]; g.start[i + 1] = (int)total; }
    return total;
}

__device__ __forceinline__ void la_map_locate(const LaMapGrid& g, int blk, int& m, int& b, int& chunk) {
    m = 0;
    while (m + 1 < g.nmaps && blk >= g.start[m + 1]) ++m;
    const int local = blk - g.start[m];
    b = local / g.chunks[m]; chunk = local - b * g.chunks[m];
}

// float64 sums over a 256-thread workgroup: lanes by the xor butterfly, then the four waves in order.  `red` is 4 (8) doubles of LDS; the
// leading barrier lets calls follow one another.  Every thread must reach them; all threads get the result.
__device__ __forceinline__ double la_block_sum_256_f64(double v, double* red) {
    v = la_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

static bool la_map_res_ok(int r) { return r >= 4 && r <= 4096 && (r & (r - 1)) == 0; }
static int la_map_table_check(const int* res, int nmaps, int B, const char* msg) {
    LA_CHECK_ARG(res && nmaps >= 1 && nmaps <= LA_NZ_MAXMAPS && B >= 1 && B <= 65535, msg);
    for (int i = 0; i < nmaps; ++i) LA_CHECK_ARG(la_map_res_ok(res[i]), "noise maps: a resolution must be 4 << k (4 .. 4096)");
    return LA_OK;
}

// ---- the regulariser.  Per map and sample:  reg = 0; loop: reg += mean(n * roll(n, 1, x))^2 + mean(n * roll(n, 1, y))^2; if r <= 8: break;
// n = avg_pool2d(n, 2); r /= 2  -- cyclic shifts; a 4 x 4 or 8 x 8 map has one level, a 256 x 256 map six.  With a_l, c_l the two means of
// level l and N_l = r_l^2 the gradient at a fine pixel is a gather (no scatter, no atomics):
//   g[y][x] = sum_l 4^-l * (2 a_l / N_l * (n_l[y_l][x_l - 1] + n_l[y_l][x_l + 1]) + 2 c_l / N_l * (n_l[y_l - 1][x_l] + n_l[y_l + 1][x_l])),  (y_l, x_l) = (y >> l, x >> l)
// Launch l (one per level index, over all maps that have level l): a workgroup takes 256 elements of level l of one (map, sample), adds
// up their two products in float64 -- the partial [map][level][sample][chunk] -- and, where the map has a level l + 1, writes its 2 x 2
// averages (float32, 0.25 * (((n00 + n01) + n10) + n11)).  The finish launch adds the partials in chunk order, thread i taking i, i + 64, ...,
// leaves the two coefficients of every (map, level, sample) and writes reg; the gather launch is one thread per fine pixel.
struct NregTab {
    int nmaps, B;
    const float* n[LA_NZ_MAXMAPS];
    float* g[LA_NZ_MAXMAPS];
    int r[LA_NZ_MAXMAPS], nlev[LA_NZ_MAXMAPS];
    long lev_off[LA_NZ_MAXMAPS], part_off[LA_NZ_MAXMAPS];      // floats into `levels` (levels 1 ..), doubles into `part`
    float* levels;
    double *part, *coef;
};

__host__ __device__ static inline int nreg_levels(int r) { int n = 1; while (r > 8) { r >>= 1; ++n; } return n; }
__host__ __device__ static inline int nreg_chunks(int r, int l) { const long n = (long)(r >> l) * (r >> l); return (int)((n + 255) / 256); }

__device__ __forceinline__ float* nreg_level(const NregTab& t, int m, int l, int b) {      // (l >= 1)
    const long r = t.r[m], rl = r >> l;
    long pre = 0;
    for (int q = 1; q < l; ++q) pre += (r >> q) * (r >> q);
    return t.levels + t.lev_off[m] + (long)t.B * pre + (long)b * rl * rl;
}
__device__ __forceinline__ const float* nreg_level_in(const NregTab& t, int m, int l, int b) {
    return l == 0 ? t.n[m] + (long)b * t.r[m] * t.r[m] : nreg_level(t, m, l, b);
}
__device__ __forceinline__ long nreg_part(const NregTab& t, int m, int l, int b) {      // first of the (x, y) pairs of (map, level, sample)
    long pre = 0;
    for (int q = 0; q < l; ++q) pre += nreg_chunks(t.r[m], q);
    return t.part_off[m] + 2 * ((long)t.B * pre + (long)b * nreg_chunks(t.r[m], l));
}

__global__ __launch_bounds__(256) void la_nreg_level_kernel(NregTab t, LaMapGrid g, int l) {
    __shared__ double red[4];
    int m, b, chunk;
    la_map_locate(g, blockIdx.x, m, b, chunk);
    const int r = t.r[m] >> l;
    const long N = (long)r * r, e = (long)chunk * 256 + threadIdx.x;
    const float* src = nreg_level_in(t, m, l, b);
    double sx = 0.0, sy = 0.0;
    if (e < N) {
        const int y = (int)(e / r), x = (int)(e - (long)y * r);
        const float v = src[e];
        sx = (double)v * (double)src[(long)y * r + (x == 0 ? r - 1 : x - 1)];
        sy = (double)v * (double)src[(long)(y == 0 ? r - 1 : y - 1) * r + x];
        if (l + 1 < t.nlev[m] && !(x & 1) && !(y & 1))
            nreg_level(t, m, l + 1, b)[(long)(y >> 1) * (r >> 1) + (x >> 1)] = 0.25f * (((v + src[e + 1]) + src[e + r]) + src[e + r + 1]);
    }
    sx = la_block_sum_256_f64(sx, red);
    sy = la_block_sum_256_f64(sy, red);
    if (threadIdx.x == 0) {
        double* p = t.part + nreg_part(t, m, l, b) + 2 * chunk;
        p[0] = sx; p[1] = sy;
    }
}

__global__ __launch_bounds__(64) void la_nreg_finish_kernel(NregTab t, double scale, double* __restrict__ reg, long reg_stride) {
    const int b = blockIdx.x;
    double total = 0.0;
    for (int m = 0; m < t.nmaps; ++m)
        for (int l = 0; l < t.nlev[m]; ++l) {
            const int chunks = nreg_chunks(t.r[m], l);
            const double* p = t.part + nreg_part(t, m, l, b);
            double ax = 0.0, ay = 0.0;
            for (int i = threadIdx.x; i < chunks; i += 64) { ax += p[2 * i]; ay += p[2 * i + 1]; }
            ax = la_wave_sum(ax); ay = la_wave_sum(ay);
            const double N = (double)(t.r[m] >> l) * (double)(t.r[m] >> l);
            const double a = ax / N, c = ay / N;
            total += a * a;
            total += c * c;
            if (threadIdx.x == 0) {
                double* cf = t.coef + (((long)m * LA_NZ_MAXLEV + l) * t.B + b) * 2;
                cf[0] = ldexp(2.0 * a / N, -2 * l); cf[1] = ldexp(2.0 * c / N, -2 * l);
            }
        }
    if (threadIdx.x == 0) reg[(long)b * reg_stride] = scale * total;
}

__global__ __launch_bounds__(256) void la_nreg_gather_kernel(NregTab t, LaMapGrid g, float weight, int accumulate) {
    int m, b, chunk;
    la_map_locate(g, blockIdx.x, m, b, chunk);
    const int r = t.r[m];
    const long e = (long)chunk * 256 + threadIdx.x;
    if (e >= (long)r * r) return;
    const int y = (int)(e / r), x = (int)(e - (long)y * r);
    double acc = 0.0;
    for (int l = 0; l < t.nlev[m]; ++l) {
        const int rl = r >> l, yl = y >> l, xl = x >> l;
        const int xm = xl == 0 ? rl - 1 : xl - 1, xp = xl == rl - 1 ? 0 : xl + 1, ym = yl == 0 ? rl - 1 : yl - 1, yp = yl == rl - 1 ? 0 : yl + 1;
        const float* src = nreg_level_in(t, m, l, b);
        const double* cf = t.coef + (((long)m * LA_NZ_MAXLEV + l) * t.B + b) * 2;
        acc += cf[0] * ((double)src[(long)yl * rl + xm] + (double)src[(long)yl * rl + xp]);
        acc += cf[1] * ((double)src[(long)ym * rl + xl] + (double)src[(long)yp * rl + xl]);
    }
    float* out = t.g[m] + (long)b * r * r + e;
    const float gv = weight * (float)acc;
    *out = accumulate ? *out + gv : gv;
}

// workspace: the levels 1 .. of every map [B][r_l][r_l] float32 | the partial pairs [map][level][B][chunks][2] float64 | the coefficient
// pairs [nmaps][LA_NZ_MAXLEV][B][2] float64
static size_t nreg_layout(NregTab& t, const int* res, int nmaps, int B, char* base) {
    LaCarver c; c.base = base;
    long lev = 0, part = 0;
    t.nmaps = nmaps; t.B = B;
    for (int i = 0; i < nmaps; ++i) {
        t.r[i] = res[i]; t.nlev[i] = nreg_levels(res[i]);
        t.lev_off[i] = lev; t.part_off[i] = part;
        for (int l = 0; l < t.nlev[i]; ++l) {
            if (l >= 1) lev += (long)B * (res[i] >> l) * (res[i] >> l);
            part += 2l * B * nreg_chunks(res[i], l);
        }
    }
    t.levels = c.take<float>((size_t)lev);
    t.part = c.take<double>((size_t)part);
    t.coef = c.take<double>((size_t)nmaps * LA_NZ_MAXLEV * B * 2);
    return c.off;
}

extern "C" size_t la_noise_reg_scratch_bytes(const int* res, int nmaps, int B) {
    if (la_map_table_check(res, nmaps, B, "noise_reg: nmaps must be 1 .. 32 and B 1 .. 65535")) return 0;
    NregTab t;
    return nreg_layout(t, res, nmaps, B, nullptr);
}

extern "C" int la_noise_reg_f32(const float* const* maps, const int* res, int nmaps, int B, double scale, float weight, float* const* gn, int accumulate,
                                double* reg, long reg_stride, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(maps && reg && ws, "noise_reg: null pointer");
    int rc = la_map_table_check(res, nmaps, B, "noise_reg: nmaps must be 1 .. 32 and B 1 .. 65535");
    if (rc) return rc;
    LA_CHECK_ARG(reg_stride >= 1, "noise_reg: reg_stride must be at least 1");
    LA_CHECK_ARG(la_aligned<8>(reg, ws), "noise_reg: pointer not aligned to its element type");
    NregTab t;
    LA_CHECK_WORKSPACE(ws_bytes, nreg_layout(t, res, nmaps, B, (char*)ws), "noise_reg: workspace too small (la_noise_reg_scratch_bytes)");
    int maxlev = 0;
    for (int i = 0; i < nmaps; ++i) {
        LA_CHECK_ARG(maps[i] && (!gn || gn[i]) && la_aligned<4>(maps[i], gn ? gn[i] : (float*)nullptr), "noise_reg: null or misaligned map");
        t.n[i] = maps[i]; t.g[i] = gn ? gn[i] : nullptr;
        maxlev = t.nlev[i] > maxlev ? t.nlev[i] : maxlev;
    }
    LaMapGrid g;
    int chunks[LA_NZ_MAXMAPS];
    for (int l = 0; l < maxlev; ++l) {
        for (int i = 0; i < nmaps; ++i) chunks[i] = l < t.nlev[i] ? nreg_chunks(res[i], l) : 0;
        const long total = la_map_grid(g, chunks, nmaps, B);
        LA_CHECK_ARG(total <= 0x7fffffffl, "noise_reg: tables too large");
        hipLaunchKernelGGL(la_nreg_level_kernel, dim3((unsigned)total), dim3(256), 0, stream, t, g, l);
        LA_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(la_nreg_finish_kernel, dim3(B), dim3(64), 0, stream, t, scale, reg, reg_stride);
    LA_CHECK_LAUNCH();
    if (gn) {
        for (int i = 0; i < nmaps; ++i) chunks[i] = nreg_chunks(res[i], 0);
        const long total = la_map_grid(g, chunks, nmaps, B);
        hipLaunchKernelGGL(la_nreg_gather_kernel, dim3((unsigned)total), dim3(256), 0, stream, t, g, weight, accumulate);
        LA_CHECK_LAUNCH();
    }
    return LA_OK;
}

// ---- the noise step tail.  Per (map, sample): Adam (la_adam_update, float32, the bias corrections of the 1-based `step` taken by the host
// as in la_proj_step_tail_f32), then the published re-normalisation n -= mean(n); n *= rsqrt(mean(n^2)).  Maps reach 1024^2 elements, so
// the moments span workgroups: a workgroup owns 1024 elements (thread t: t, t + 256, ...) of one (map, sample), and there are three launches
//   1  update, and the chunk's sum                         -> part[workgroup]
//   2  mean = (partials in chunk order) / N; the chunk's sum of (n - mean)^2   -> part2[workgroup]
//   3  the same mean, q = (partials of 2) / N, n = (n - mean) / sqrt(q)   (q == 0: zeros)
// all float64, thread i of a workgroup adding partials i, i + 256, ... before the workgroup sum: fixed by the shape alone.  Summing the
// CENTRED squares means E[n^2] - mean^2 is never formed; a map of equal values has the exact mean (N is a power of two) and q = 0.
#define LA_NT_CHUNK 1024
struct NtailTab {
    const float* gn[LA_NZ_MAXMAPS];
    float *n[LA_NZ_MAXMAPS], *m[LA_NZ_MAXMAPS], *v[LA_NZ_MAXMAPS];
    int r[LA_NZ_MAXMAPS];
    double *part, *part2;
};

__device__ __forceinline__ double ntail_total(const double* part, const LaMapGrid& g, int m, int b, double* red) {
    const double* p = part + g.start[m] + (long)b * g.chunks[m];
    double s = 0.0;
    for (int i = threadIdx.x; i < g.chunks[m]; i += 256) s += p[i];
    return la_block_sum_256_f64(s, red);
}

__global__ __launch_bounds__(256) void la_ntail_adam_kernel(NtailTab t, LaMapGrid g, float step_size, float bc2_sqrt, float b1, float b2, float eps) {
    __shared__ double red[4];
    int m, b, chunk;
    la_map_locate(g, blockIdx.x, m, b, chunk);
    const long N = (long)t.r[m] * t.r[m], base = (long)b * N;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_NT_CHUNK / 256; ++k) {
        const long e = (long)chunk * LA_NT_CHUNK + k * 256 + threadIdx.x;
        if (e < N) {
            const long i = base + e;
            float pv = t.n[m][i], mv = t.m[m][i], vv = t.v[m][i];
            la_adam_update(pv, mv, vv, t.gn[m][i], step_size, bc2_sqrt, b1, b2, eps);
            t.n[m][i] = pv; t.m[m][i] = mv; t.v[m][i] = vv;
            s += (double)pv;
        }
    }
    s = la_block_sum_256_f64(s, red);
    if (threadIdx.x == 0) t.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void la_ntail_centre_kernel(NtailTab t, LaMapGrid g) {
    __shared__ double red[4];
    int m, b, chunk;
    la_map_locate(g, blockIdx.x, m, b, chunk);
    const long N = (long)t.r[m] * t.r[m], base = (long)b * N;
    const double mean = ntail_total(t.part, g, m, b, red) / (double)N;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_NT_CHUNK / 256; ++k) {
        const long e = (long)chunk * LA_NT_CHUNK + k * 256 + threadIdx.x;
        if (e < N) { const double dv = (double)t.n[m][base + e] - mean; s += dv * dv; }
    }
    s = la_block_sum_256_f64(s, red);
    if (threadIdx.x == 0) t.part2[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void la_ntail_scale_kernel(NtailTab t, LaMapGrid g) {
    __shared__ double red[4];
    int m, b, chunk;
    la_map_locate(g, blockIdx.x, m, b, chunk);
    const long N = (long)t.r[m] * t.r[m], base = (long)b * N;
    const double mean = ntail_total(t.part, g, m, b, red) / (double)N;
    const double q = ntail_total(t.part2, g, m, b, red) / (double)N;
    const double sc = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
#pragma unroll
    for (int k = 0; k < LA_NT_CHUNK / 256; ++k) {
        const long e = (long)chunk * LA_NT_CHUNK + k * 256 + threadIdx.x;
        if (e < N) t.n[m][base + e] = (float)(((double)t.n[m][base + e] - mean) * sc);
    }
}

// scratch: the launch-1 partials [workgroups] float64, then the launch-2 partials
static size_t ntail_layout(NtailTab& t, long total, void* base) {
    LaCarver c{(char*)base};
    t.part = c.take<double>((size_t)total);
    t.part2 = c.take<double>((size_t)total);
    return c.off;
}

static long ntail_grid(LaMapGrid& g, const int* res, int nmaps, int B) {
    int chunks[LA_NZ_MAXMAPS];
    for (int i = 0; i < nmaps; ++i) chunks[i] = (int)(((long)res[i] * res[i] + LA_NT_CHUNK - 1) / LA_NT_CHUNK);
    return la_map_grid(g, chunks, nmaps, B);
}

extern "C" size_t la_proj_noise_tail_scratch_bytes(const int* res, int nmaps, int B) {
    if (la_map_table_check(res, nmaps, B, "proj_noise_tail: nmaps must be 1 .. 32 and B 1 .. 65535")) return 0;
    LaMapGrid g;
    NtailTab t;
    return ntail_layout(t, ntail_grid(g, res, nmaps, B), nullptr);
}

extern "C" int la_proj_noise_tail_f32(const float* const* gn, float* const* n, float* const* m, float* const* v, const int* res, int nmaps, int B, int step,
                                      float lr, float beta1, float beta2, float eps, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(gn && n && m && v && ws, "proj_noise_tail: null pointer");
    int rc = la_map_table_check(res, nmaps, B, "proj_noise_tail: nmaps must be 1 .. 32 and B 1 .. 65535");
    if (rc) return rc;
    LA_CHECK_ARG(step >= 1, "proj_noise_tail: the Adam step is 1-based");
    LA_CHECK_ARG(la_aligned<8>(ws), "proj_noise_tail: workspace not aligned to 8 bytes");
    LaMapGrid g;
    const long total = ntail_grid(g, res, nmaps, B);
    LA_CHECK_ARG(total <= 0x7fffffffl, "proj_noise_tail: tables too large");
    NtailTab t;
    LA_CHECK_WORKSPACE(ws_bytes, ntail_layout(t, total, ws), "proj_noise_tail: workspace too small (la_proj_noise_tail_scratch_bytes)");
    for (int i = 0; i < nmaps; ++i) {
        LA_CHECK_ARG(gn[i] && n[i] && m[i] && v[i] && la_aligned<4>(gn[i], n[i], m[i], v[i]),
                     "proj_noise_tail: null or misaligned map");
        t.gn[i] = gn[i]; t.n[i] = n[i]; t.m[i] = m[i]; t.v[i] = v[i]; t.r[i] = res[i];
    }
    const float step_size = lr / (1.f - powf(beta1, (float)step)), bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(la_ntail_adam_kernel, dim3((unsigned)total), dim3(256), 0, stream, t, g, step_size, bc2s, beta1, beta2, eps);
    LA_CHECK_LAUNCH();
    hipLaunchKernelGGL(la_ntail_centre_kernel, dim3((unsigned)total), dim3(256), 0, stream, t, g);
    LA_CHECK_LAUNCH();
    hipLaunchKernelGGL(la_ntail_scale_kernel, dim3((unsigned)total), dim3(256), 0, stream, t, g);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
