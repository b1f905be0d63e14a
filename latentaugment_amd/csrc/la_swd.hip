// Sliced Wasserstein distance of image and feature sets (gfx950 only): the Laplacian pyramid, the patch descriptors, their channel
// statistics and normalisation, the random unit directions, and the distance itself (project, sort the columns with
// la_sort_columns_f32, mean |a - b|).  The method and every contract are written down at the prototypes (include/latentaug_hip.h) and
// in DESIGN.md 'Sliced Wasserstein distance'; the counter convention of the draws is in la_rng.h.
//
// No float atomics, no host synchronisation, nothing allocated: every float64 sum has a fixed order and two runs give the same bits.
#include "la_f32_tile.h"
#include "la_rng.h"

#include <math.h>

// ------------------------------------------------------------------------------------------------------------ Laplacian pyramid
// index i of a line of n >= 2 samples mirrored about both ends without repeating the edge (d c b | a b c d | c b a), any distance
__device__ __forceinline__ int swd_mirror(int i, int n) {
    const int period = 2 * (n - 1);
    i %= period;
    i = i < 0 ? i + period : i;
    return i < n ? i : period - i;
}

// y [planes][H / 2][W / 2] = every second sample (from 0) of x [planes][H][W] under the 5 x 5 binomial filter; one thread per output
__global__ __launch_bounds__(256) void la_lap_pyr_down_kernel(const float* __restrict__ x, float* __restrict__ y, long planes, int H, int W) {
    const int h2 = H >> 1, w2 = W >> 1;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= planes * h2 * w2) return;
    const int ox = (int)(g % w2), oy = (int)(g / w2 % h2);
    const float* xp = x + g / ((long)w2 * h2) * ((long)H * W);
    const float k[5] = {1.f, 4.f, 6.f, 4.f, 1.f};
    int xs[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) xs[d] = swd_mirror(2 * ox + d - 2, W);
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float* row = xp + (long)swd_mirror(2 * oy + dy - 2, H) * W;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) acc = fmaf(k[dy] * k[dx] * (1.f / 256.f), row[xs[dx]], acc);
    }
    y[g] = acc;
}

// fine [planes][H][W] -= up(coarse [planes][H / 2][W / 2]).  up = the same filter times 4 on the zero-stuffed image (samples at even
// positions), mirrored like the filter's input; a mirror keeps the parity of a position (the period 2 (n - 1) is even), so an even
// output position sees the taps [1, 6, 1] / 8 at its even neighbours and an odd one [4, 4] / 8: the zeros are never multiplied.
__global__ __launch_bounds__(256) void la_lap_pyr_up_sub_kernel(float* __restrict__ fine, const float* __restrict__ coarse, long planes, int H,
                                                               int W) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= planes * H * W) return;
    const int x = (int)(g % W), y = (int)(g / W % H);
    const int w2 = W >> 1;
    const float* cp = coarse + g / ((long)W * H) * ((long)(H >> 1) * w2);
    int ys[3], xs[3], ny, nx;
    float wy[3], wx[3];
    if (y & 1) { ny = 2; ys[0] = swd_mirror(y - 1, H) >> 1; ys[1] = swd_mirror(y + 1, H) >> 1; ys[2] = 0; wy[0] = wy[1] = 0.5f; wy[2] = 0.f; }
    else { ny = 3; ys[0] = swd_mirror(y - 2, H) >> 1; ys[1] = y >> 1; ys[2] = swd_mirror(y + 2, H) >> 1; wy[0] = wy[2] = 0.125f; wy[1] = 0.75f; }
    if (x & 1) { nx = 2; xs[0] = swd_mirror(x - 1, W) >> 1; xs[1] = swd_mirror(x + 1, W) >> 1; xs[2] = 0; wx[0] = wx[1] = 0.5f; wx[2] = 0.f; }
    else { nx = 3; xs[0] = swd_mirror(x - 2, W) >> 1; xs[1] = x >> 1; xs[2] = swd_mirror(x + 2, W) >> 1; wx[0] = wx[2] = 0.125f; wx[1] = 0.75f; }
    float acc = 0.f;
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b) acc = fmaf(wy[a] * wx[b], cp[(long)ys[a] * w2 + xs[b]], acc);
    fine[g] -= acc;
}

// ------------------------------------------------------------------------------------------------------------ descriptors
// one thread per descriptor element; the patch corner from two Philox words of counter (patch, global image, stream, level)
__global__ __launch_bounds__(256) void la_swd_gather_kernel(const float* __restrict__ img, long n, int C, int H, int W, long img0, int level,
                                                           int nhood, int per_image, unsigned k0, unsigned k1, float* __restrict__ desc) {
    const int D = C * nhood * nhood;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * per_image * D) return;
    const int e = (int)(g % D);
    const long row = g / D;
    const int j = (int)(row % per_image);
    const long i = row / per_image;
    unsigned w[4];
    la_philox4x32_10((unsigned)j, (unsigned)(img0 + i), LA_RNG_STREAM_SWD_POS, (unsigned)level, k0, k1, w);
    const int x0 = (int)(((unsigned long long)w[0] * (unsigned long long)(W - nhood + 1)) >> 32);
    const int y0 = (int)(((unsigned long long)w[1] * (unsigned long long)(H - nhood + 1)) >> 32);
    const int c = e / (nhood * nhood), py = e / nhood % nhood, px = e % nhood;
    desc[g] = img[((i * C + c) * H + (y0 + py)) * W + (x0 + px)];
}

// ------------------------------------------------------------------------------------------------------------ channel statistics
// Channel c of desc [M][C * P] is columns [c P, (c + 1) P) of every row: M P values, element q = (row q / P, position q % P).
// Workgroup (b, c) sums a contiguous run of them in float64 -- the threads stride the run, then a fixed tree -- either x (mean NULL)
// or (x - mean[c])^2; the finish kernel adds the runs in order.
#define SWD_STATS_RUN 16384          // elements per workgroup at least: 64 per thread
static inline int swd_stats_blocks(long M, int P) {
    const long n = M * P;
    const long b = (n + SWD_STATS_RUN - 1) / SWD_STATS_RUN;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__global__ __launch_bounds__(256) void la_swd_stats_part_kernel(const float* __restrict__ desc, long M, int C, int P, const double* __restrict__ mean,
                                                               double* __restrict__ part) {
    __shared__ double red[256];
    const int c = blockIdx.y, nb = gridDim.x;
    const long n = M * P, run = (n + nb - 1) / nb;
    const long q0 = (long)blockIdx.x * run, q1 = q0 + run < n ? q0 + run : n;
    const double mu = mean ? mean[c] : 0.0;
    double s = 0.0;
    for (long q = q0 + threadIdx.x; q < q1; q += 256) {
        const double v = (double)desc[q / P * ((long)C * P) + (long)c * P + q % P] - mu;
        s += mean ? v * v : v;
    }
    s = la_block_tree_sum_256(s, red);
    if (threadIdx.x == 0) part[(long)c * nb + blockIdx.x] = s;
}

// thread c: out[c] = (sum of the nb runs of channel c in order) / count, or its square root
__global__ void la_swd_stats_finish_kernel(const double* __restrict__ part, int C, int nb, double count, int root, double* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(long)c * nb + b];
    s /= count;
    out[c] = root ? sqrt(s) : s;
}

// (x - mean) / std in float64, one rounding.  std == 0 (a constant channel has no descriptor: callers refuse it) writes NaN
__global__ __launch_bounds__(256) void la_swd_normalize_kernel(float* __restrict__ desc, long M, int C, int P, const double* __restrict__ mean,
                                                              const double* __restrict__ std) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= M * C * P) return;
    const int c = (int)(g % ((long)C * P)) / P;
    const double sd = std[c];
    desc[g] = sd > 0.0 ? (float)(((double)desc[g] - mean[c]) / sd) : NAN;
}

// ------------------------------------------------------------------------------------------------------------ directions
// one wave per direction: the lanes stride the 4-element groups of the row, write the normals, add their squares in float64 in
// element order and combine by the wave butterfly; then every lane divides what it wrote
__global__ __launch_bounds__(256) void la_swd_directions_kernel(float* __restrict__ dirs, long ndirs, int D, long dir0, unsigned k0, unsigned k1) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= ndirs) return;          // (the whole wave)
    float* row = dirs + j * D;
    const int groups = (D + 3) >> 2;
    double ss = 0.0;
    for (int q = lane; q < groups; q += 64) {
        unsigned w[4];
        float z[4];
        la_noise_words(q, dir0 + j, LA_RNG_STREAM_SWD_DIR, k0, k1, w);
        la_unit_normals4(w, z);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * q + u < D) { row[4 * q + u] = z[u]; ss += (double)z[u] * (double)z[u]; }
    }
    const double norm = sqrt(la_wave_sum(ss));
    for (int q = lane; q < groups; q += 64)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * q + u < D) row[4 * q + u] = (float)((double)row[4 * q + u] / norm);
}

// ------------------------------------------------------------------------------------------------------------ projection
// proj[(set * nd + j) * M + m] = desc_set[m] . dirs[j] for the nd directions of a chunk: the exact-fp32 tile loop of la_f32_tile.h on
// 128 directions x 128 rows per workgroup, 4 waves (2 x 2) of 64 x 64, K walked in chunks of 16.  The directions are the tile's rows
// and the descriptor rows its columns (column = lane & 31), so a wave stores 32 consecutive m of a column of proj.  Every projection
// is one k-ordered fp32 chain.  Rows past either end load zeros and are not stored.
#define SWD_T 128
#define SWD_KC 16
#define SWD_LD (SWD_T + 4)

__global__ __launch_bounds__(256) void la_swd_project_kernel(const float* __restrict__ descA, const float* __restrict__ descB, long M, int D,
                                                            const float* __restrict__ dirs, int nd, float* __restrict__ proj) {
    __shared__ __attribute__((aligned(16))) float As[2][SWD_KC][SWD_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][SWD_KC][SWD_LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const float* desc = blockIdx.z ? descB : descA;
    const long m0 = (long)blockIdx.x * SWD_T;
    const int j0 = (int)blockIdx.y * SWD_T;

    // loader roles: 4 threads per row (4 consecutive k each), rows tid / 4 and tid / 4 + 64 of both operands
    const int kq = (tid & 3) * 4, lr = tid >> 2;
    const float *pa[2], *pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = j0 + lr + 64 * h;
        const long m = m0 + lr + 64 * h;
        pa[h] = j < nd ? dirs + (long)j * D : nullptr;
        pb[h] = m < M ? desc + m * D : nullptr;
    }
    float areg[2][4], breg[2][4];
    auto fetch = [&](const float* p, int k, float (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (p && k + u < D) ? p[k + u] : 0.f;
    };
    auto prefetch = [&](int ci) {
        const int k = ci * SWD_KC + kq;
#pragma unroll
        for (int h = 0; h < 2; ++h) { fetch(pa[h], k, areg[h]); fetch(pb[h], k, breg[h]); }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int u = 0; u < 4; ++u) { As[buf][kq + u][lr + 64 * h] = areg[h][u]; Bs[buf][kq + u][lr + 64 * h] = breg[h][u]; }
    };

    la_f32x16 acc[2][2];
    la_f32_tile_zero(acc);
    const int nchunk = (D + SWD_KC - 1) / SWD_KC;
    la_tile_pipeline(0, nchunk, prefetch, stage, [&](int buf, int) { la_f32_tile_mma<SWD_KC>(As, Bs, buf, wm * 64, wn * 64, l31, lh, acc); });

    float* out = proj + (long)blockIdx.z * nd * M;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            const long m = m0 + wn * 64 + jt * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + wm * 64 + i * 32 + la_mfma32_row(r, lh);
                if (j < nd && m < M) out[(long)j * M + m] = acc[i][jt][r];
            }
        }
}

// w1[j] = (sum over m of |a[j][m] - b[j][m]| in float64) / M: one workgroup per column, the threads stride it, then a fixed tree
__global__ __launch_bounds__(256) void la_swd_w1_kernel(const float* __restrict__ proj, long M, int nd, double* __restrict__ w1) {
    __shared__ double red[256];
    const float* a = proj + (long)blockIdx.x * M;
    const float* b = a + (long)nd * M;
    double s = 0.0;
    for (long m = threadIdx.x; m < M; m += 256) s += fabs((double)a[m] - (double)b[m]);
    s = la_block_tree_sum_256(s, red);
    if (threadIdx.x == 0) w1[blockIdx.x] = s / (double)M;
}

// ------------------------------------------------------------------------------------------------------------ host side
#define SWD_MAX_ELEMS 0x7fffffffffffL          // (far beyond any memory: keeps the 64-bit products of the checks from overflowing)

extern "C" int la_lap_pyr_down_f32(const float* x, float* y, long planes, int H, int W, hipStream_t stream) {
    LA_CHECK_ARG(x && y && la_aligned<4>(x, y), "lap_pyr_down: null or misaligned pointer");
    LA_CHECK_ARG(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && H <= 32768 && W <= 32768, "lap_pyr_down: H and W must be even and lie in 2 .. 32768");
    LA_CHECK_ARG(planes >= 1 && planes <= 0x7fffffffL && planes * (long)H * W <= 0x3fffffffffL, "lap_pyr_down: planes out of range");
    LA_CHECK_ARG(x != y, "lap_pyr_down: y must not be x");
    hipLaunchKernelGGL(la_lap_pyr_down_kernel, dim3((unsigned)((planes * (H / 2) * (W / 2) + 255) / 256)), dim3(256), 0, stream, x, y, planes, H, W);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_lap_pyr_up_sub_f32(float* fine, const float* coarse, long planes, int H, int W, hipStream_t stream) {
    LA_CHECK_ARG(fine && coarse && la_aligned<4>(fine, coarse), "lap_pyr_up_sub: null or misaligned pointer");
    LA_CHECK_ARG(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && H <= 32768 && W <= 32768, "lap_pyr_up_sub: H and W must be even and lie in 2 .. 32768");
    LA_CHECK_ARG(planes >= 1 && planes <= 0x7fffffffL && planes * (long)H * W <= 0x3fffffffffL, "lap_pyr_up_sub: planes out of range");
    LA_CHECK_ARG(fine != coarse, "lap_pyr_up_sub: coarse must not be fine");
    hipLaunchKernelGGL(la_lap_pyr_up_sub_kernel, dim3((unsigned)((planes * H * W + 255) / 256)), dim3(256), 0, stream, fine, coarse, planes, H, W);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_swd_gather_f32(const float* img, long n, int C, int H, int W, long img0, int level, int nhood, int per_image,
                                 unsigned long long seed, float* desc, hipStream_t stream) {
    LA_CHECK_ARG(img && desc && la_aligned<4>(img, desc), "swd_gather: null or misaligned pointer");
    LA_CHECK_ARG(C >= 1 && C <= 64 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "swd_gather: C must lie in 1 .. 64, H and W in 1 .. 32768");
    LA_CHECK_ARG(nhood >= 1 && nhood <= 64 && nhood <= H && nhood <= W, "swd_gather: nhood must lie in 1 .. min(64, H, W)");
    LA_CHECK_ARG(per_image >= 1 && per_image <= 65536 && level >= 0, "swd_gather: per_image must lie in 1 .. 65536 and level be non-negative");
    LA_CHECK_ARG(n >= 1 && n <= 0x7fffffffL && img0 >= 0 && img0 + n <= 0xffffffffL, "swd_gather: image index exceeds 32 bits");
    const long total = n * per_image * ((long)C * nhood * nhood);
    LA_CHECK_ARG(total <= 0x3fffffffffL && n * C * (long)H * W <= 0x3fffffffffL, "swd_gather: too many elements");
    hipLaunchKernelGGL(la_swd_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, img, n, C, H, W, img0, level, nhood,
                       per_image, (unsigned)seed, (unsigned)(seed >> 32), desc);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

static inline bool swd_stats_sizes_ok(long M, int C, int P) {
    return M >= 1 && M <= 0x7fffffffL && C >= 1 && C <= 64 && P >= 1 && P <= 4096 && M * ((long)C * P) <= 0x3fffffffffL;
}

extern "C" size_t la_swd_stats_scratch_bytes(long M, int C, int P) {
    if (!swd_stats_sizes_ok(M, C, P)) return 0;
    return la_align64((size_t)C * swd_stats_blocks(M, P) * sizeof(double));
}

extern "C" int la_swd_channel_stats_f64(const float* desc, long M, int C, int P, double* mean, double* std, void* scratch, size_t scratch_bytes,
                                        hipStream_t stream) {
    LA_CHECK_ARG(desc && mean && std && scratch, "swd_channel_stats: null pointer");
    LA_CHECK_ARG(swd_stats_sizes_ok(M, C, P), "swd_channel_stats: M must be at least 1, C in 1 .. 64, P in 1 .. 4096");
    LA_CHECK_ARG(la_aligned<4>(desc) && la_aligned<8>(mean, std, scratch), "swd_channel_stats: float64 arrays and the scratch must be 8-byte aligned");
    LA_CHECK_WORKSPACE(scratch_bytes, la_swd_stats_scratch_bytes(M, C, P), "swd_channel_stats: scratch smaller than la_swd_stats_scratch_bytes(M, C, P)");
    const int nb = swd_stats_blocks(M, P);
    double* part = (double*)scratch;
    const double count = (double)M * (double)P;
    hipLaunchKernelGGL(la_swd_stats_part_kernel, dim3(nb, C), dim3(256), 0, stream, desc, M, C, P, (const double*)nullptr, part);
    hipLaunchKernelGGL(la_swd_stats_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)part, C, nb, count, 0, mean);
    hipLaunchKernelGGL(la_swd_stats_part_kernel, dim3(nb, C), dim3(256), 0, stream, desc, M, C, P, (const double*)mean, part);
    hipLaunchKernelGGL(la_swd_stats_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)part, C, nb, count, 1, std);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_swd_normalize_f32(float* desc, long M, int C, int P, const double* mean, const double* std, hipStream_t stream) {
    LA_CHECK_ARG(desc && mean && std, "swd_normalize: null pointer");
    LA_CHECK_ARG(swd_stats_sizes_ok(M, C, P), "swd_normalize: M must be at least 1, C in 1 .. 64, P in 1 .. 4096");
    LA_CHECK_ARG(la_aligned<4>(desc) && la_aligned<8>(mean, std), "swd_normalize: float64 arrays must be 8-byte aligned");
    hipLaunchKernelGGL(la_swd_normalize_kernel, dim3((unsigned)((M * C * P + 255) / 256)), dim3(256), 0, stream, desc, M, C, P, mean, std);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_swd_directions_f32(float* dirs, long ndirs, int D, long dir0, unsigned long long seed, hipStream_t stream) {
    LA_CHECK_ARG(dirs && la_aligned<4>(dirs), "swd_directions: null or misaligned pointer");
    LA_CHECK_ARG(ndirs >= 1 && ndirs <= 0x3fffffffL && D >= 1 && D <= (1 << 24), "swd_directions: ndirs must lie in 1 .. 2^30 - 1 and D in 1 .. 2^24");
    LA_CHECK_ARG(dir0 >= 0 && dir0 + ndirs <= 0xffffffffL, "swd_directions: direction index exceeds 32 bits");
    hipLaunchKernelGGL(la_swd_directions_kernel, dim3((unsigned)((ndirs + 3) / 4)), dim3(256), 0, stream, dirs, ndirs, D, dir0, (unsigned)seed,
                       (unsigned)(seed >> 32));
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// scratch of la_swd_f32 for a chunk of c directions: the projections of both sets [2 c][M], then the sort's image of them
#define SWD_MIN_CHUNK 32
#define SWD_MAX_CHUNK 32767          // 2 c columns are the sort's grid y
static inline bool swd_sizes_ok(long M, int D, long ndirs) {
    return M >= 1 && M <= 0x40000000L && D >= 1 && D <= (1 << 20) && ndirs >= 1 && ndirs <= 0x7fffffffL && M * (long)D <= 0x3fffffffffL;
}
struct SwdScratch { float* proj; char* sort; size_t sort_bytes, bytes; };
static inline SwdScratch swd_scratch(long M, long c, void* base) {
    LaCarver cv{(char*)base};
    SwdScratch s;
    s.proj = cv.take<float>((size_t)2 * c * M);
    s.sort_bytes = la_sort_columns_scratch_bytes(2 * c, M);
    s.sort = cv.take<char>(s.sort_bytes);
    s.bytes = cv.off;
    return s;
}

extern "C" size_t la_swd_scratch_bytes(long M, int D, long ndirs) {
    if (!swd_sizes_ok(M, D, ndirs)) return 0;
    return swd_scratch(M, ndirs < SWD_MIN_CHUNK ? ndirs : SWD_MIN_CHUNK, nullptr).bytes;
}

extern "C" int la_swd_f32(const float* descA, const float* descB, long M, int D, const float* dirs, long ndirs, double* w1, void* scratch,
                          size_t scratch_bytes, hipStream_t stream) {
    LA_CHECK_ARG(descA && descB && dirs && w1 && scratch, "swd: null pointer");
    LA_CHECK_ARG(swd_sizes_ok(M, D, ndirs), "swd: M must lie in 1 .. 2^30, D in 1 .. 2^20, ndirs be at least 1");
    LA_CHECK_ARG(la_aligned<4>(descA, descB, dirs) && la_aligned<8>(w1, scratch),
                 "swd: w1 and the scratch must be 8-byte aligned, float arrays 4-byte aligned");
    LA_CHECK_WORKSPACE(scratch_bytes, la_swd_scratch_bytes(M, D, ndirs), "swd: scratch smaller than la_swd_scratch_bytes(M, D, ndirs)");
    // the largest chunk that fits (at least the documented minimum's): a column's bits do not depend on its chunk
    long chunk = (long)(scratch_bytes / ((size_t)16 * M));
    chunk = chunk > ndirs ? ndirs : chunk;
    chunk = chunk > SWD_MAX_CHUNK ? SWD_MAX_CHUNK : chunk;
    const long floor_chunk = ndirs < SWD_MIN_CHUNK ? ndirs : SWD_MIN_CHUNK;
    chunk = chunk < floor_chunk ? floor_chunk : chunk;
    while (chunk > floor_chunk && swd_scratch(M, chunk, nullptr).bytes > scratch_bytes) --chunk;
    const SwdScratch s = swd_scratch(M, chunk, scratch);
    for (long j0 = 0; j0 < ndirs; j0 += chunk) {
        const int nd = (int)(ndirs - j0 < chunk ? ndirs - j0 : chunk);
        hipLaunchKernelGGL(la_swd_project_kernel, dim3((unsigned)((M + SWD_T - 1) / SWD_T), (unsigned)((nd + SWD_T - 1) / SWD_T), 2), dim3(256), 0,
                           stream, descA, descB, M, D, dirs + j0 * D, nd, s.proj);
        const int rc = la_sort_columns_f32(s.proj, 2 * nd, M, M, s.sort, s.sort_bytes, stream);
        if (rc != LA_OK) return rc;
        hipLaunchKernelGGL(la_swd_w1_kernel, dim3((unsigned)nd), dim3(256), 0, stream, (const float*)s.proj, M, nd, w1 + j0);
    }
    LA_CHECK_LAUNCH();
    return LA_OK;
}
