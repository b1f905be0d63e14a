// Per-sample neighbour queries on float32 features in float64 arithmetic (gfx950 only): the k nearest bank rows of every query row
// (la_knn_f32) and the realism score of Kynkaanniemi et al. 2019 (la_realism_f32).
//
// One definition of the squared distance of a pair, used by both entries:
//   d2(q, x) = max(0, (|q|^2 + |x|^2) - 2 q.x)
// with all three sums in float64 over the float32 inputs widened exactly (a product of two float32 values is exact in float64).  The
// dot products are the tile product of la_f64_tile.h (la_fd_gram_kernel's, without centring), whose k order does not depend on the
// tile; the norms of both sides come from one kernel (la_knn_rowsq_kernel) as the diagonal of the same product, i.e. in the same k
// order.  So the bits of d2(q, x) depend on the two rows and D only -- not on the tile, the column split, the row of the batch or the
// number of other rows -- equal rows have equal norms, and d2 of two equal rows is exactly 0 (n + n - 2 n), whatever their values: a
// copy of a bank row is found at distance 0, not at the rounding error of three sums.  For any summation order |d2 - d2_exact| <= (2 D + 4) 2^-53 (|q|^2 + |x|^2): three sums
// of D exact products each, then two roundings to combine them.
//
// Launch shape: grid (blocks of 64 query rows) x (la_knn_col_splits chunks of bank columns).  A workgroup walks its chunk in tiles of
// 64 columns; the finished 64 x 64 tile of d2 goes through LDS (over the staging buffers, which are free by then) and one thread per
// query row inserts from it into that row's sorted list of k (key, index) in LDS.  Columns arrive in index order, so inserting behind
// equal keys keeps the order (key, index).  The lists of the splits go to scratch; la_knn_finish_kernel gives every candidate its rank
// among the candidates of its row -- the number of (key, index) pairs below it -- and writes the first k.  A rank does not depend on
// any merge order.  No atomics, no host synchronisation, nothing allocated: two runs give the same bits.
// The realism entry is the same template with another key: -radius2[x] / d2 over the kept spheres, k = 1.
#include "la_f64_tile.h"

#include <math.h>
#include <stdio.h>

#define KNN_MAX_K 32
#define KNN_TARGET_WG 512        // workgroups a launch aims at: two per CU
#define KNN_MAX_SPLITS 64        // the finish kernel holds splits x k candidates of a row in LDS
#define KNN_TLD (FD_T + 1)       // doubles per row of the d2 tile in LDS

static_assert(FD_T * KNN_TLD <= 2 * FD_T * FD_LD, "the d2 tile lies over the two staging buffers");

// rowsq[i] = q_i . q_i (i < nq), rowsq[nq + i] = x_i . x_i, each as the diagonal of a tile of the row block with itself: the chain of
// MFMA steps of the tile kernel below for a pair of equal rows.  grid ceil(nq / 64) + ceil(nx / 64): the blocks of q, then of x
__global__ __launch_bounds__(256) void la_knn_rowsq_kernel(const float* __restrict__ q, long nq, const float* __restrict__ x, long nx, int D,
                                                          double* __restrict__ rowsq) {
    __shared__ double S[FD_T][FD_LD];
    const int tid = threadIdx.x;
    const FdLane t = fd_tile_lane();
    const int lk = tid & 31, lr = tid >> 5;
    const long qb = (nq + FD_T - 1) / FD_T;
    const bool isq = (long)blockIdx.x < qb;
    const float* m = isq ? q : x;
    const long n = isq ? nq : nx;
    const long i0 = (isq ? (long)blockIdx.x : (long)blockIdx.x - qb) * FD_T;
    fd_f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0;
    // both sides are these rows: staged once, into one buffer
    fd_tile_loop<false>(S, S, m, n, nullptr, i0, m, n, nullptr, i0, D, lk, lr,
                        [&](const double (*P)[FD_LD], const double (*)[FD_LD]) { fd_tile_mma_diag(P, acc, t); });
    const long row = i0 + (t.wm * 2 + t.wn) * 16 + t.l15;
    if (t.l4 == (t.l15 & 3) && row < n) rowsq[(isq ? 0 : nq) + row] = fd_tile_diag(acc, t);
}

// The tile loop.  grid (row blocks, splits); the workgroup's columns are [blockIdx.y * chunk, + chunk) cut at nx (chunk: a multiple
// of 64).  pkey / pidx [row block][split][k][64]: the sorted list of every row of the block, unused slots (+inf, -1).
// REALISM: key = -(radius2[x] / d2) (d2 == 0: -inf) over the columns with radius2 >= 0; otherwise key = d2.
template <bool REALISM>
__global__ __launch_bounds__(256) void la_knn_tile_kernel(const float* __restrict__ q, long nq, const float* __restrict__ x, long nx, int D,
                                                         const double* __restrict__ rowsq, long chunk, int k, int exclude_self,
                                                         const double* __restrict__ radius2, double* __restrict__ pkey,
                                                         int* __restrict__ pidx) {
    __shared__ double stage[2 * FD_T * FD_LD];
    extern __shared__ double lists[];          // k x 64 keys, then k x 64 indices: knn_list_bytes(k)
    double (*Lk)[FD_T] = reinterpret_cast<double (*)[FD_T]>(lists);
    int (*Li)[FD_T] = reinterpret_cast<int (*)[FD_T]>(lists + (size_t)k * FD_T);
    double (*Ps)[FD_LD] = reinterpret_cast<double (*)[FD_LD]>(stage);
    double (*Qs)[FD_LD] = reinterpret_cast<double (*)[FD_LD]>(stage + FD_T * FD_LD);
    double (*Ts)[KNN_TLD] = reinterpret_cast<double (*)[KNN_TLD]>(stage);
    const int tid = threadIdx.x;
    const FdLane t = fd_tile_lane();
    const int lk = tid & 31, lr = tid >> 5;          // loader roles
    const long i0 = (long)blockIdx.x * FD_T;
    const long c0 = (long)blockIdx.y * chunk;
    const long c1 = c0 + chunk < nx ? c0 + chunk : nx;
    if (tid < FD_T)
        for (int s = 0; s < k; ++s) { Lk[s][tid] = INFINITY; Li[s][tid] = -1; }
    // |q|^2 of the rows this lane's accumulators belong to
    double qn[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = i0 + fd_tile_row(t, i, r);
            qn[i][r] = rowsq[row < nq ? row : nq - 1];
        }
    const long grow = i0 + tid;          // the row whose list thread tid < 64 keeps
    for (long j0 = c0; j0 < c1; j0 += FD_T) {
        fd_f64x4 acc[2][2];
        fd_tile_zero(acc);
        fd_tile_loop<false>(Ps, Qs, q, nq, nullptr, i0, x, nx, nullptr, j0, D, lk, lr,
                            [&](const double (*P)[FD_LD], const double (*Q)[FD_LD]) { fd_tile_mma(P, Q, acc, t); });
        // d2 of the tile into LDS (the staging buffers are free: every wave is past the last fragment read)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tc = fd_tile_col(t, j);
            const long col = j0 + tc;
            const double xn = rowsq[nq + (col < nx ? col : nx - 1)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d2 = (qn[i][r] + xn) - 2.0 * acc[i][j][r];
                    Ts[fd_tile_row(t, i, r)][tc] = d2 > 0.0 ? d2 : 0.0;
                }
        }
        __syncthreads();
        if (tid < FD_T && grow < nq) {
            const int ncol = (int)(c1 - j0 < FD_T ? c1 - j0 : FD_T);
            double worst = Lk[k - 1][tid];
            for (int c = 0; c < ncol; ++c) {
                const long gx = j0 + c;
                if (exclude_self && gx == grow) continue;
                double v = Ts[tid][c];
                if (REALISM) {
                    const double r2 = radius2[gx];
                    if (r2 < 0.0) continue;
                    v = v == 0.0 ? -INFINITY : -(r2 / v);
                }
                if (!(v < worst)) continue;
                int s = k - 1;
                while (s > 0 && Lk[s - 1][tid] > v) {
                    Lk[s][tid] = Lk[s - 1][tid];
                    Li[s][tid] = Li[s - 1][tid];
                    --s;
                }
                Lk[s][tid] = v;
                Li[s][tid] = (int)gx;
                worst = Lk[k - 1][tid];
            }
        }
        __syncthreads();          // the next tile stages over Ts
    }
    if (tid < FD_T) {
        const size_t base = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (size_t)k * FD_T;
        for (int s = 0; s < k; ++s) {
            pkey[base + (size_t)s * FD_T + tid] = Lk[s][tid];
            pidx[base + (size_t)s * FD_T + tid] = Li[s][tid];
        }
    }
}

// One workgroup per query row: the splits x k candidates of the row into LDS, every one ranked by the number of candidates below
// it in (key, index) order, the first k written.  Slots past the number of candidates: (+inf, -1); REALISM (k = 1): score2 = -key,
// and (0, -1) without a candidate.
template <bool REALISM>
__global__ __launch_bounds__(256) void la_knn_finish_kernel(const double* __restrict__ pkey, const int* __restrict__ pidx, int splits, int k,
                                                           double* __restrict__ out_key, int* __restrict__ out_idx) {
    __shared__ double ck[KNN_MAX_SPLITS * KNN_MAX_K];
    __shared__ int ci[KNN_MAX_SPLITS * KNN_MAX_K];
    const long row = blockIdx.x;
    const size_t rb = (size_t)(row / FD_T);
    const int r = (int)(row % FD_T);
    const int n = splits * k;
    for (int c = threadIdx.x; c < n; c += 256) {
        const size_t at = ((rb * splits + (size_t)(c / k)) * k + (size_t)(c % k)) * FD_T + r;
        ck[c] = pkey[at];
        ci[c] = pidx[at];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += 256) {
        const int me = ci[c];
        if (me < 0) continue;
        const double key = ck[c];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int oi = ci[j];
            const double ok = ck[j];
            rank += (oi >= 0 && (ok < key || (ok == key && oi < me))) ? 1 : 0;
        }
        if (rank < k) {
            out_key[row * k + rank] = REALISM ? -key : key;
            out_idx[row * k + rank] = me;
        }
    }
    if ((int)threadIdx.x < k) {
        int valid = 0;
        for (int j = 0; j < n; ++j) valid += ci[j] >= 0 ? 1 : 0;
        if ((int)threadIdx.x >= valid) {
            out_key[row * k + threadIdx.x] = REALISM ? 0.0 : (double)INFINITY;
            out_idx[row * k + threadIdx.x] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// (an index is an int; the finish launch has one workgroup per query row)
static inline bool knn_sizes_ok(long nq, long nx) { return nq >= 1 && nx >= 1 && nq <= 0x7fffffffL && nx <= 0x7fffffffL && nq + nx <= 0x7fffffffL; }

// LDS of the k-lists of a workgroup's 64 rows (dynamic: a small k leaves room for more workgroups per CU)
static inline size_t knn_list_bytes(int k) { return (size_t)k * FD_T * (sizeof(double) + sizeof(int)); }

// tiles of 64 columns per chunk: enough chunks that row blocks x chunks reaches KNN_TARGET_WG workgroups (rounded towards more
// chunks: a tile stages both its sides whatever the chunk, so short chunks cost nothing in the tile loop), never more chunks than
// there are tiles or than the finish kernel holds.  chunks < 2 want: row blocks x chunks < 2 (KNN_TARGET_WG + row blocks)
static inline long knn_chunk_tiles(long nq, long nx) {
    const long rb = (nq + FD_T - 1) / FD_T, ct = (nx + FD_T - 1) / FD_T;
    long want = (KNN_TARGET_WG + rb - 1) / rb;
    if (want > ct) want = ct;
    long tiles = ct / want;
    const long least = (ct + KNN_MAX_SPLITS - 1) / KNN_MAX_SPLITS;
    return tiles > least ? tiles : least;
}

// number of column chunks of a launch (0 for sizes it refuses)
extern "C" int la_knn_col_splits(long nq, long nx) {
    if (!knn_sizes_ok(nq, nx)) return 0;
    const long ct = (nx + FD_T - 1) / FD_T, tiles = knn_chunk_tiles(nq, nx);
    return (int)((ct + tiles - 1) / tiles);
}

// The scratch: the squared norms of both sides, then the split lists' keys, then their indices.  The lists are sized by a bound on
// row blocks x splits that grows with nq and with nx (the product itself does not: more row blocks take fewer splits):
// min(2 (KNN_TARGET_WG + row blocks), row blocks x min(column tiles, KNN_MAX_SPLITS)).
struct KnnLayout {
    double *rowsq, *keys;
    int* idx;
    size_t bytes;
};

static inline KnnLayout knn_layout(long nq, long nx, int k, void* base) {
    const size_t rb = (size_t)((nq + FD_T - 1) / FD_T), ct = (size_t)((nx + FD_T - 1) / FD_T);
    const size_t a = 2 * (KNN_TARGET_WG + rb), b = rb * (ct < KNN_MAX_SPLITS ? ct : KNN_MAX_SPLITS);
    const size_t lists = (a < b ? a : b) * (size_t)k * FD_T;
    KnnLayout L;
    LaCarver c{(char*)base};
    L.rowsq = c.take<double>((size_t)nq + (size_t)nx);
    L.keys = c.take<double>(lists);
    L.idx = c.take<int>(lists);
    L.bytes = c.off;
    return L;
}

extern "C" size_t la_knn_scratch_bytes(long nq, long nx, int D, int k) {
    if (!knn_sizes_ok(nq, nx) || D < 1 || k < 1 || k > KNN_MAX_K) return 0;
    return knn_layout(nq, nx, k, nullptr).bytes;
}

template <bool REALISM>
static int knn_launch(const char* who, const float* q, long nq, const float* x, long nx, int D, int k, int exclude_self,
                      const double* radius2, double* out_key, int* out_idx, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    char msg[160];
    auto says = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return (const char*)msg; };
    LA_CHECK_ARG(q && x && out_key && out_idx && scratch && (!REALISM || radius2), says("null pointer"));
    LA_CHECK_ARG(nq >= 1 && nx >= 1, says("queries and bank need at least one row each"));
    LA_CHECK_ARG(D >= 1, says("the feature dimension must be positive"));
    LA_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, says("k must lie in 1 .. 32"));
    LA_CHECK_ARG(!exclude_self || nq == nx, says("exclude_self needs nq == nx (the queries are the bank)"));
    LA_CHECK_ARG(knn_sizes_ok(nq, nx), says("sizes exceed the grid"));
    LA_CHECK_WORKSPACE(scratch_bytes, la_knn_scratch_bytes(nq, nx, D, k), says("scratch smaller than la_knn_scratch_bytes(nq, nx, D, k)"));
    LA_CHECK_ARG(la_aligned<4>(q, x, out_idx) && la_aligned<8>(out_key, scratch, radius2),
                 says("features and indices must be 4-byte aligned, float64 arrays and the scratch 8-byte aligned"));
    const long tiles = knn_chunk_tiles(nq, nx);
    const int splits = la_knn_col_splits(nq, nx);
    const long rb = (nq + FD_T - 1) / FD_T;
    const KnnLayout L = knn_layout(nq, nx, k, scratch);
    hipLaunchKernelGGL(la_knn_rowsq_kernel, dim3((unsigned)(rb + (nx + FD_T - 1) / FD_T)), dim3(256), 0, stream, q, nq, x, nx, D, L.rowsq);
    hipLaunchKernelGGL(la_knn_tile_kernel<REALISM>, dim3((unsigned)rb, (unsigned)splits), dim3(256), knn_list_bytes(k), stream, q, nq, x, nx, D,
                       (const double*)L.rowsq, tiles * FD_T, k, exclude_self, radius2, L.keys, L.idx);
    hipLaunchKernelGGL(la_knn_finish_kernel<REALISM>, dim3((unsigned)nq), dim3(256), 0, stream, (const double*)L.keys, (const int*)L.idx, splits,
                       k, out_key, out_idx);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_knn_f32(const float* q, long nq, const float* x, long nx, int D, int k, int exclude_self, double* dist2, int* idx,
                          void* scratch, size_t scratch_bytes, hipStream_t stream) {
    return knn_launch<false>("knn", q, nq, x, nx, D, k, exclude_self, nullptr, dist2, idx, scratch, scratch_bytes, stream);
}

extern "C" int la_realism_f32(const float* q, long nq, const float* x, long nx, int D, const double* radius2, double* score2, int* arg,
                              void* scratch, size_t scratch_bytes, hipStream_t stream) {
    return knn_launch<true>("realism", q, nq, x, nx, D, 1, 0, radius2, score2, arg, scratch, scratch_bytes, stream);
}
