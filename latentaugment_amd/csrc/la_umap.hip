// UMAP embedding after the neighbour search (gfx950 only): smooth-kNN weights, the fuzzy union as a symmetric CSR, the initial
// layouts and the force layout, one synchronous epoch per launch.  The method and its four differences from umap-learn are written
// down at the prototypes (include/latentaug_hip.h) and in DESIGN.md 'UMAP embedding'; the counter convention of the draws is in la_rng.h.
//
// Everything is float64.  Nothing here uses a float atomic, a grid-wide barrier or a cooperative launch: the only atomics are integer
// counters of the graph build, whose arrival order a later rank sort removes from the result.  Row kernels give one wave to a row
// (four rows per workgroup): the lanes stride the row's entries and la_wave_sum combines them, so a row of any length goes through
// one loop and two runs give the same bits.
#include "la_rng.h"

#include <math.h>
#include <stdio.h>

#define UMAP_MAX_K 32
#define UMAP_MAX_C 8
#define UMAP_MAX_RATE 32
#define UMAP_ROWS_PER_WG 4

// ------------------------------------------------------------------------------------------------------------ smooth-kNN
// One wave per row; lane s < k owns slot s.  rho and the mean are selections / a sum in slot order that every lane repeats for
// itself (k <= 32 broadcast loads); the 64 bisection sums are the wave butterfly over the lanes' terms.
__global__ __launch_bounds__(256) void la_umap_smooth_knn_kernel(const double* __restrict__ dist2, const int* __restrict__ idx, long n, int k,
                                                                double target, double* __restrict__ rho_out, double* __restrict__ sigma_out,
                                                                double* __restrict__ w_out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * UMAP_ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= n) return;          // (the whole wave)
    const double* drow = dist2 + i * k;
    const int* irow = idx + i * k;
    double rho = INFINITY, sum = 0.0;
    int cnt = 0;
    for (int s = 0; s < k; ++s) {
        const double d2 = drow[s];
        if (irow[s] < 0 || !(d2 >= 0.0) || !(d2 < INFINITY)) continue;
        const double d = sqrt(d2);
        if (d > 0.0 && d < rho) rho = d;
        sum += d;
        ++cnt;
    }
    if (!(rho < INFINITY)) rho = 0.0;
    bool valid = false;
    double x = 0.0;
    if (lane < k) {
        const double d2 = drow[lane];
        valid = irow[lane] >= 0 && d2 >= 0.0 && d2 < INFINITY;
        if (valid) {
            const double d = sqrt(d2) - rho;
            x = d > 0.0 ? d : 0.0;
        }
    }
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        const double s = la_wave_sum(valid ? exp(-(x / mid)) : 0.0);
        if (s > target) {
            hi = mid;
            mid = (lo + hi) * 0.5;
        } else {
            lo = mid;
            mid = hi < INFINITY ? (lo + hi) * 0.5 : mid * 2.0;
        }
    }
    const double floor_sigma = cnt > 0 ? 1e-3 * (sum / (double)cnt) : 0.0;
    const double sigma = mid > floor_sigma ? mid : floor_sigma;
    if (lane == 0) { rho_out[i] = rho; sigma_out[i] = sigma; }
    if (lane < k) w_out[i * k + lane] = valid ? exp(-(x / sigma)) : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ fuzzy union
// scratch of the graph build: three int arrays [n] (one-sided in-degree, fill cursor, out-degree), then the unsorted columns and
// values (2 n k each)
struct UmapLayout {
    int *cnt, *cur, *outdeg, *ucol;
    double* uval;
    size_t bytes;
};

static inline bool umap_sizes_ok(long n, int k) { return n >= 2 && n <= 0x3fffffffL && k >= 1 && k <= UMAP_MAX_K && 2 * n * (long)k <= 0x7fffffffL; }

static inline UmapLayout umap_layout(long n, int k, void* base) {
    UmapLayout L;
    LaCarver c{(char*)base};
    L.cnt = c.take<int>((size_t)n);
    L.cur = c.take<int>((size_t)n);
    L.outdeg = c.take<int>((size_t)n);
    L.ucol = c.take<int>(2 * (size_t)n * k);
    L.uval = c.take<double>(2 * (size_t)n * k);
    L.bytes = c.off;
    return L;
}

extern "C" size_t la_umap_scratch_bytes(long n, int k) {
    if (!umap_sizes_ok(n, k)) return 0;
    return umap_layout(n, k, nullptr).bytes;
}

__device__ __forceinline__ bool umap_slot_ok(int j, long n) { return j >= 0 && (long)j < n; }
// the slot of row j that names i, or -1
__device__ __forceinline__ int umap_find(const int* __restrict__ idx, int k, int j, int i) {
    for (int t = 0; t < k; ++t)
        if (idx[(long)j * k + t] == i) return t;
    return -1;
}

__global__ __launch_bounds__(256) void la_umap_degree_kernel(const int* __restrict__ idx, long n, int k, int* __restrict__ cnt,
                                                            int* __restrict__ cur, int* __restrict__ outdeg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int d = 0;
    for (int s = 0; s < k; ++s) d += umap_slot_ok(idx[i * k + s], n) ? 1 : 0;
    cnt[i] = 0; cur[i] = 0; outdeg[i] = d;
}

// one thread per slot (i, s): an edge i -> j that j does not return adds one entry to row j
__global__ __launch_bounds__(256) void la_umap_count_kernel(const int* __restrict__ idx, long n, int k, int* __restrict__ cnt) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * k) return;
    const int i = (int)(g / k), j = idx[g];
    if (!umap_slot_ok(j, n)) return;
    if (umap_find(idx, k, j, i) < 0) atomicAdd(&cnt[j], 1);
}

// row_ptr = exclusive scan of outdeg + cnt.  One workgroup: every thread sums a contiguous run of rows, thread 0 scans the 256 run
// totals, every thread writes its run.
__global__ __launch_bounds__(256) void la_umap_scan_kernel(const int* __restrict__ outdeg, const int* __restrict__ cnt, long n,
                                                          int* __restrict__ row_ptr) {
    __shared__ int part[256];
    const long run = (n + 255) / 256;
    const long r0 = (long)threadIdx.x * run, r1 = r0 + run < n ? r0 + run : n;
    int s = 0;
    for (long r = r0; r < r1; ++r) s += outdeg[r] + cnt[r];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = acc; acc += v; }
        row_ptr[n] = acc;
    }
    __syncthreads();
    int acc = part[threadIdx.x];
    for (long r = r0; r < r1; ++r) { row_ptr[r] = acc; acc += outdeg[r] + cnt[r]; }
}

// one thread per slot (i, s): the row's own entries in slot order, then -- through the cursor -- the entries that one-sided edges add
// to their target's row, in arrival order (the sort below removes it).  val = a + b - a b with a the row's own weight of the pair.
__global__ __launch_bounds__(256) void la_umap_fill_kernel(const int* __restrict__ idx, const double* __restrict__ w, long n, int k,
                                                          const int* __restrict__ row_ptr, const int* __restrict__ outdeg,
                                                          int* __restrict__ cur, int* __restrict__ ucol, double* __restrict__ uval) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * k) return;
    const int i = (int)(g / k), s = (int)(g - (long)i * k), j = idx[g];
    if (!umap_slot_ok(j, n)) return;
    int before = 0;
    for (int t = 0; t < s; ++t) before += umap_slot_ok(idx[(long)i * k + t], n) ? 1 : 0;
    const double a = w[g];
    const int back = umap_find(idx, k, j, i);
    const double b = back >= 0 ? w[(long)j * k + back] : 0.0;
    const long at = (long)row_ptr[i] + before;
    ucol[at] = j;
    uval[at] = (a + b) - a * b;
    if (back < 0) {
        const long to = (long)row_ptr[j] + outdeg[j] + atomicAdd(&cur[j], 1);
        ucol[to] = i;
        uval[to] = (0.0 + a) - 0.0 * a;
    }
}

// one wave per row: every entry goes to its rank among the row's columns (distinct, so the ranks are a permutation)
__global__ __launch_bounds__(256) void la_umap_sort_kernel(const int* __restrict__ row_ptr, long n, const int* __restrict__ ucol,
                                                          const double* __restrict__ uval, int* __restrict__ col, double* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * UMAP_ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= n) return;
    const long beg = row_ptr[i];
    const int len = row_ptr[i + 1] - row_ptr[i];
    for (int t = lane; t < len; t += 64) {
        const int c = ucol[beg + t];
        int rank = 0;
        for (int u = 0; u < len; ++u) rank += ucol[beg + u] < c ? 1 : 0;
        col[beg + rank] = c;
        val[beg + rank] = uval[beg + t];
    }
}

// wmax = max(val[0 .. row_ptr[n])): one workgroup, a halving tree over LDS (a maximum does not depend on the order)
__global__ __launch_bounds__(256) void la_umap_wmax_kernel(const int* __restrict__ row_ptr, long n, const double* __restrict__ val,
                                                          double* __restrict__ wmax) {
    __shared__ double red[256];
    const long nnz = row_ptr[n];
    double m = 0.0;
    for (long t = threadIdx.x; t < nnz; t += 256) m = fmax(m, val[t]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) wmax[0] = red[0];
}

// ------------------------------------------------------------------------------------------------------------ initial layouts
__global__ __launch_bounds__(256) void la_umap_init_kernel(double* __restrict__ y, long n, int C, unsigned k0, unsigned k1, long row0) {
    const int groups = (C + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * groups) return;
    const long i = g / groups;
    const int q = (int)(g - i * groups);
    unsigned x[4];
    la_umap_init_words(q, row0 + i, k0, k1, x);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (4 * q + u < C) y[i * C + 4 * q + u] = 10.0 * (double)la_unit_uniform(x[u]);
}

// one thread per (row, coordinate): the weighted mean in slot order; thread (i, 0) writes row_ptr[i] = i k
__global__ __launch_bounds__(256) void la_umap_transform_init_kernel(const int* __restrict__ idx, const double* __restrict__ w, long n, int k,
                                                                    const double* __restrict__ bank_y, long n_bank, int C,
                                                                    double* __restrict__ y, int* __restrict__ row_ptr,
                                                                    double* __restrict__ wmax) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g == 0) { row_ptr[n] = (int)(n * k); wmax[0] = 1.0; }
    if (g >= n * C) return;
    const long i = g / C;
    const int c = (int)(g - i * C);
    double num = 0.0, den = 0.0;
    for (int s = 0; s < k; ++s) {
        const int j = idx[i * k + s];
        if (!umap_slot_ok(j, n_bank)) continue;
        const double ws = w[i * k + s];
        num += ws * bank_y[(long)j * C + c];
        den += ws;
    }
    y[g] = den > 0.0 ? num / den : 0.0;
    if (c == 0) row_ptr[i] = (int)(i * k);
}

// ------------------------------------------------------------------------------------------------------------ one epoch
struct UmapEpochArgs {
    const double* y_in;
    double* y_out;
    const double* y_tail;
    const int* row_ptr;
    const int* col;
    const double* val;
    const double* wmax;
    long n, n_tail, cap, row0;
    double a, b, alpha, e;
    int epoch, rate, skip_self;
    unsigned k0, k1;
};

__device__ __forceinline__ double umap_clip(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

template <int C>
__global__ __launch_bounds__(256) void la_umap_epoch_kernel(const UmapEpochArgs A) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * UMAP_ROWS_PER_WG + (threadIdx.x >> 6);
    if (i >= A.n) return;          // (the whole wave)
    double yi[C], acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { yi[c] = A.y_in[i * C + c]; acc[c] = 0.0; }
    const double wmax = A.wmax[0];
    long beg = A.row_ptr[i], end = A.row_ptr[i + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > A.cap ? A.cap : end;
    const int groups = (A.rate + 3) >> 2;
    for (long t = beg + lane; t < end; t += 64) {
        const int j = A.col[t];
        if (!umap_slot_ok(j, A.n_tail)) continue;
        const double p = A.val[t] / wmax;
        if (!(floor((A.e + 1.0) * p) > floor(A.e * p))) continue;
        {          // the attraction towards tail j
            double diff[C], d2 = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) { diff[c] = yi[c] - A.y_tail[(long)j * C + c]; d2 += diff[c] * diff[c]; }
            if (d2 > 0.0) {
                const double coef = (-2.0 * A.a * A.b * pow(d2, A.b - 1.0)) / (1.0 + A.a * pow(d2, A.b));
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += umap_clip(coef * diff[c]);
            }
        }
        for (int g = 0; g < groups; ++g) {
            unsigned x[4];
            la_umap_neg_words((int)(t - beg), A.row0 + i, A.epoch, g, A.k0, A.k1, x);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * g + u >= A.rate) break;
                const long r = (long)(((unsigned long long)x[u] * (unsigned long long)A.n_tail) >> 32);
                if (A.skip_self && r == i) continue;
                double diff[C], q2 = 0.0;
#pragma unroll
                for (int c = 0; c < C; ++c) { diff[c] = yi[c] - A.y_tail[r * C + c]; q2 += diff[c] * diff[c]; }
                if (!(q2 > 0.0)) continue;
                const double coef = (2.0 * A.b) / ((0.001 + q2) * (1.0 + A.a * pow(q2, A.b)));
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += umap_clip(coef * diff[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = la_wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) A.y_out[i * C + c] = yi[c] + A.alpha * acc[c];
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
static inline unsigned umap_row_blocks(long n) { return (unsigned)((n + UMAP_ROWS_PER_WG - 1) / UMAP_ROWS_PER_WG); }

extern "C" int la_umap_smooth_knn_f64(const double* dist2, const int* idx, long n, int k, double target, double* rho, double* sigma, double* w,
                                      hipStream_t stream) {
    LA_CHECK_ARG(dist2 && idx && rho && sigma && w, "umap_smooth_knn: null pointer");
    LA_CHECK_ARG(n >= 1 && n <= 0x3fffffffL, "umap_smooth_knn: n must lie in 1 .. 2^30 - 1");
    LA_CHECK_ARG(k >= 1 && k <= UMAP_MAX_K, "umap_smooth_knn: k must lie in 1 .. 32");
    LA_CHECK_ARG(target > 0.0 && target < INFINITY, "umap_smooth_knn: the target must be positive and finite");
    LA_CHECK_ARG(la_aligned<8>(dist2, rho, sigma, w) && la_aligned<4>(idx),
                 "umap_smooth_knn: float64 arrays must be 8-byte aligned, indices 4-byte aligned");
    hipLaunchKernelGGL(la_umap_smooth_knn_kernel, dim3(umap_row_blocks(n)), dim3(256), 0, stream, dist2, idx, n, k, target, rho, sigma, w);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_umap_graph_f64(const int* idx, const double* w, long n, int k, int* row_ptr, int* col, double* val, long cap, double* wmax,
                                 void* scratch, size_t scratch_bytes, hipStream_t stream) {
    LA_CHECK_ARG(idx && w && row_ptr && col && val && wmax && scratch, "umap_graph: null pointer");
    LA_CHECK_ARG(k >= 1 && k <= UMAP_MAX_K, "umap_graph: k must lie in 1 .. 32");
    LA_CHECK_ARG(umap_sizes_ok(n, k), "umap_graph: n must be at least 2 and 2 n k below 2^31");
    LA_CHECK_ARG(cap >= 2 * n * (long)k, "umap_graph: col and val need a capacity of 2 n k entries");
    LA_CHECK_ARG(la_aligned<8>(w, val, wmax, scratch) && la_aligned<4>(idx, row_ptr, col),
                 "umap_graph: float64 arrays and the scratch must be 8-byte aligned, int arrays 4-byte aligned");
    LA_CHECK_WORKSPACE(scratch_bytes, la_umap_scratch_bytes(n, k), "umap_graph: scratch smaller than la_umap_scratch_bytes(n, k)");
    const UmapLayout L = umap_layout(n, k, scratch);
    const unsigned slots = (unsigned)la_cdiv(n * k, 256);
    hipLaunchKernelGGL(la_umap_degree_kernel, dim3((unsigned)la_cdiv(n, 256)), dim3(256), 0, stream, idx, n, k, L.cnt, L.cur, L.outdeg);
    hipLaunchKernelGGL(la_umap_count_kernel, dim3(slots), dim3(256), 0, stream, idx, n, k, L.cnt);
    hipLaunchKernelGGL(la_umap_scan_kernel, dim3(1), dim3(256), 0, stream, (const int*)L.outdeg, (const int*)L.cnt, n, row_ptr);
    hipLaunchKernelGGL(la_umap_fill_kernel, dim3(slots), dim3(256), 0, stream, idx, w, n, k, (const int*)row_ptr, (const int*)L.outdeg, L.cur, L.ucol,
                       L.uval);
    hipLaunchKernelGGL(la_umap_sort_kernel, dim3(umap_row_blocks(n)), dim3(256), 0, stream, (const int*)row_ptr, n, (const int*)L.ucol,
                       (const double*)L.uval, col, val);
    hipLaunchKernelGGL(la_umap_wmax_kernel, dim3(1), dim3(256), 0, stream, (const int*)row_ptr, n, (const double*)val, wmax);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_umap_init_f64(double* y, long n, int C, unsigned long long seed, long row0, hipStream_t stream) {
    LA_CHECK_ARG(y && la_aligned<8>(y), "umap_init: null or misaligned pointer");
    LA_CHECK_ARG(n >= 1 && n <= 0x3fffffffL, "umap_init: n must lie in 1 .. 2^30 - 1");
    LA_CHECK_ARG(C >= 1 && C <= UMAP_MAX_C, "umap_init: C must lie in 1 .. 8");
    LA_CHECK_ARG(row0 >= 0 && row0 + n <= 0xffffffffL, "umap_init: row index exceeds 32 bits");
    hipLaunchKernelGGL(la_umap_init_kernel, dim3((unsigned)la_cdiv(n * ((C + 3) / 4), 256)), dim3(256), 0, stream, y, n, C, (unsigned)seed,
                       (unsigned)(seed >> 32), row0);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_umap_transform_init_f64(const int* idx, const double* w, long n, int k, const double* bank_y, long n_bank, int C, double* y,
                                          int* row_ptr, double* wmax, hipStream_t stream) {
    LA_CHECK_ARG(idx && w && bank_y && y && row_ptr && wmax, "umap_transform_init: null pointer");
    LA_CHECK_ARG(k >= 1 && k <= UMAP_MAX_K, "umap_transform_init: k must lie in 1 .. 32");
    LA_CHECK_ARG(n >= 1 && n * (long)k <= 0x7fffffffL && n_bank >= 1 && n_bank <= 0x7fffffffL, "umap_transform_init: sizes out of range");
    LA_CHECK_ARG(C >= 1 && C <= UMAP_MAX_C, "umap_transform_init: C must lie in 1 .. 8");
    LA_CHECK_ARG(la_aligned<8>(w, bank_y, y, wmax) && la_aligned<4>(idx, row_ptr),
                 "umap_transform_init: float64 arrays must be 8-byte aligned, int arrays 4-byte aligned");
    hipLaunchKernelGGL(la_umap_transform_init_kernel, dim3((unsigned)la_cdiv(n * C, 256)), dim3(256), 0, stream, idx, w, n, k, bank_y, n_bank, C,
                       y, row_ptr, wmax);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

struct UmapEpochCall {
    long n, n_tail, cap, row0;
    int C, E, rate, skip_self;
    double a, b, lr;
    unsigned long long seed;
    const int* row_ptr;
    const int* col;
    const double* val;
    const double* wmax;
};

// everything about an epoch launch but its buffers and its epoch number
static int umap_epoch_check(const char* who, const UmapEpochCall& c) {
    char msg[160];
    auto fail = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); la_set_error(msg); return LA_ERR_ARG; };
    if (!c.row_ptr || !c.col || !c.val || !c.wmax) return fail("null pointer");
    if (c.n < 1 || c.n > 0x3fffffffL || c.n_tail < 1 || c.n_tail > 0x7fffffffL) return fail("row counts out of range");
    if (c.C < 1 || c.C > UMAP_MAX_C) return fail("C must lie in 1 .. 8");
    if (c.E < 1 || c.E > LA_UMAP_MAX_EPOCHS) return fail("E must lie in 1 .. 2^28");
    if (c.rate < 0 || c.rate > UMAP_MAX_RATE) return fail("the negative sample rate must lie in 0 .. 32");
    if (!(c.a > 0.0) || !(c.b > 0.0) || !(c.a < INFINITY) || !(c.b < INFINITY)) return fail("a and b must be positive and finite");
    if (!(c.lr == c.lr) || c.lr == INFINITY || c.lr == -INFINITY) return fail("the learning rate must be finite");
    if (c.cap < 0 || c.cap > 0x7fffffffL) return fail("cap out of range");
    if (c.row0 < 0 || c.row0 + c.n > 0xffffffffL) return fail("row index exceeds 32 bits");
    if (!la_aligned<8>(c.val, c.wmax) || !la_aligned<4>(c.row_ptr, c.col))
        return fail("float64 arrays must be 8-byte aligned, int arrays 4-byte aligned");
    return LA_OK;
}

static void umap_epoch_enqueue(const UmapEpochCall& c, const double* y_in, double* y_out, const double* y_tail, int e, hipStream_t stream) {
    UmapEpochArgs A;
    A.y_in = y_in; A.y_out = y_out; A.y_tail = y_tail;
    A.row_ptr = c.row_ptr; A.col = c.col; A.val = c.val; A.wmax = c.wmax;
    A.n = c.n; A.n_tail = c.n_tail; A.cap = c.cap; A.row0 = c.row0;
    A.a = c.a; A.b = c.b; A.alpha = c.lr * (1.0 - (double)e / (double)c.E); A.e = (double)e;
    A.epoch = e; A.rate = c.rate; A.skip_self = c.skip_self;
    A.k0 = (unsigned)c.seed; A.k1 = (unsigned)(c.seed >> 32);
    const dim3 grid(umap_row_blocks(c.n)), block(256);
    switch (c.C) {
        case 1: hipLaunchKernelGGL(la_umap_epoch_kernel<1>, grid, block, 0, stream, A); break;
        case 2: hipLaunchKernelGGL(la_umap_epoch_kernel<2>, grid, block, 0, stream, A); break;
        case 3: hipLaunchKernelGGL(la_umap_epoch_kernel<3>, grid, block, 0, stream, A); break;
        case 4: hipLaunchKernelGGL(la_umap_epoch_kernel<4>, grid, block, 0, stream, A); break;
        case 5: hipLaunchKernelGGL(la_umap_epoch_kernel<5>, grid, block, 0, stream, A); break;
        case 6: hipLaunchKernelGGL(la_umap_epoch_kernel<6>, grid, block, 0, stream, A); break;
        case 7: hipLaunchKernelGGL(la_umap_epoch_kernel<7>, grid, block, 0, stream, A); break;
        default: hipLaunchKernelGGL(la_umap_epoch_kernel<8>, grid, block, 0, stream, A); break;
    }
}

extern "C" int la_umap_epoch_f64(const double* y_in, double* y_out, long n, const double* y_tail, long n_tail, int C, const int* row_ptr,
                                 const int* col, const double* val, long cap, const double* wmax, int e, int E, double a, double b, int rate,
                                 double lr, unsigned long long seed, long row0, int skip_self, hipStream_t stream) {
    const UmapEpochCall c = {n, n_tail, cap, row0, C, E, rate, skip_self, a, b, lr, seed, row_ptr, col, val, wmax};
    const int rc = umap_epoch_check("umap_epoch", c);
    if (rc != LA_OK) return rc;
    LA_CHECK_ARG(y_in && y_out && y_tail && la_aligned<8>(y_in, y_out, y_tail), "umap_epoch: null or misaligned positions");
    LA_CHECK_ARG(y_in != y_out && y_tail != y_out, "umap_epoch: an epoch is synchronous: y_out must not be y_in or y_tail");
    LA_CHECK_ARG(e >= 0 && e < E, "umap_epoch: e must lie in 0 .. E - 1");
    umap_epoch_enqueue(c, y_in, y_out, y_tail, e, stream);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_umap_layout_f64(double* ya, double* yb, long n, const double* y_tail, long n_tail, int C, const int* row_ptr, const int* col,
                                  const double* val, long cap, const double* wmax, int e0, int e1, int E, double a, double b, int rate, double lr,
                                  unsigned long long seed, long row0, int skip_self, int* which, hipStream_t stream) {
    const UmapEpochCall c = {n, n_tail, cap, row0, C, E, rate, skip_self, a, b, lr, seed, row_ptr, col, val, wmax};
    const int rc = umap_epoch_check("umap_layout", c);
    if (rc != LA_OK) return rc;
    LA_CHECK_ARG(ya && yb && which && la_aligned<8>(ya, yb, y_tail), "umap_layout: null or misaligned positions");
    LA_CHECK_ARG(ya != yb && y_tail != ya && y_tail != yb, "umap_layout: ya, yb and y_tail must be three buffers");
    LA_CHECK_ARG(e0 >= 0 && e0 <= e1 && e1 <= E, "umap_layout: the epochs must satisfy 0 <= e0 <= e1 <= E");
    LA_CHECK_ARG(y_tail || n_tail == n, "umap_layout: a fit (y_tail NULL) has n_tail == n");
    double* buf[2] = {ya, yb};
    for (int e = e0; e < e1; ++e) {
        const double* in = buf[(e - e0) & 1];
        umap_epoch_enqueue(c, in, buf[(e - e0 + 1) & 1], y_tail ? y_tail : in, e, stream);
    }
    LA_CHECK_LAUNCH();
    *which = (e1 - e0) & 1;
    return LA_OK;
}
