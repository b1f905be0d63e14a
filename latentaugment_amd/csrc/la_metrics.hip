// Quality-metric kernels: the numeric core of the reference's FID and Improved Precision/Recall,
// downstream of the detector features.
//   la_feature_moments_f64    metrics/metric_utils.py:104-118  raw_mean += sum_k x[k], raw_cov += x^T x, float64 accumulators
//   la_pr_kth_f16             metrics/precision_recall.py:75-79 k-th neighbour radius of every manifold point
//   la_pr_member_f16          metrics/precision_recall.py:80-84 is a probe inside any manifold point's radius
//   la_cdist_f16              metrics/precision_recall.py:19-32 the distance matrix itself (torch.cdist)
//   la_kid_poly3_f32          (no reference counterpart) Kernel Inception Distance: unbiased MMD^2, cubic polynomial kernel, per subset
//   la_dc_count_f16           (no reference counterpart) density and coverage: per generated row the number of real balls that hold it,
//                             per real sample the distance to its nearest generated row, one pass over the pair grid
// Distances follow torch.cdist's GEMM form |a|^2 + |b|^2 - 2 a.b, clamped at 1e-30, square root.  The reference hands
// cdist float16 features; their products are exact on the fp16 MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulate), so the dot
// products here are fp32 sums of exact terms.  The [rows, cols] matrix is never materialised for the radii / membership
// kernels: each wave keeps the k+1 smallest distances (or an OR) per row in registers while it streams over the columns.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "la_common.h"
#include "la_f32_tile.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define PR_KMAX 8

// The distance of two rows from their squared norms and their dot product: written once, so that la_pr_tile_kernel and
// la_dc_tile_kernel give a pair the same bits.
__device__ __forceinline__ float la_pr_dist(float na, float nb, float dot) { return sqrtf(fmaxf(na + nb - 2.f * dot, 1e-30f)); }

// squared norms of fp16 rows, fp32
__global__ __launch_bounds__(256) void la_rows_sqnorm_f16_kernel(const _Float16* __restrict__ x, long n, int D, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) { const float v = (float)x[r * D + k]; s += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[r] = s;
}

// MODE 0: kth radius (k+1-th smallest distance per row, the row's own zero included, as torch.kthvalue(k+1) over the full
//         row of the manifold-vs-manifold matrix);  MODE 1: membership (any column with dist <= radius[col]);
// MODE 2: write the distance tile.
// Workgroup = 4 waves x 32 rows; every wave walks all columns 128 at a time (4 MFMA column tiles share one row fragment).
// Fragments come straight from the row-major fp16 matrices: lane (r, h) of a 32x16 block is 16 contiguous bytes of row r.
template <int MODE>
__global__ __launch_bounds__(256) void la_pr_tile_kernel(const _Float16* __restrict__ rows, const float* __restrict__ rown, long nr,
                                                        const _Float16* __restrict__ cols, const float* __restrict__ coln, long nc,
                                                        int D, int kk, const float* __restrict__ radius, float* __restrict__ out_kth,
                                                        unsigned char* __restrict__ out_member, float* __restrict__ out_dist) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const long r0 = (long)blockIdx.x * 128 + wid * 32;
    if (r0 >= nr) return;                                      // whole wave out of range (no barriers in this kernel)
    const long arow = r0 + l31 < nr ? r0 + l31 : nr - 1;
    const _Float16* ap = rows + arow * D + lh * 8;
    // rows held by this lane: m(r) = (r&3) + 8*(r>>2) + 4*lh
    float na[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = r0 + la_mfma32_row(r, lh);
        na[r] = rown[m < nr ? m : nr - 1];
    }
    float best[MODE == 0 ? 16 : 1][PR_KMAX];
    unsigned member = 0u;
    if (MODE == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int q = 0; q < PR_KMAX; ++q) best[MODE == 0 ? r : 0][q] = __builtin_huge_valf();
    }
    for (long c0 = 0; c0 < nc; c0 += 128) {
        la_f32x16 acc[4];
        const _Float16* bp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            const long c = c0 + j * 32 + l31;
            bp[j] = cols + (c < nc ? c : nc - 1) * D + lh * 8;
        }
        for (int k = 0; k < D; k += 16) {
            const f16x8 af = *reinterpret_cast<const f16x8*>(ap + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16x8 bf = *reinterpret_cast<const f16x8*>(bp[j] + k);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long c = c0 + j * 32 + l31;
            const bool cok = c < nc;
            const float nb = coln[cok ? c : nc - 1];
            const float rad = (MODE == 1) ? radius[cok ? c : nc - 1] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = la_pr_dist(na[r], nb, acc[j][r]);
                if (MODE == 0) {
                    // sorted insert into the row's k+1 smallest (ascending), columns past the end never enter
                    float v = cok ? d : __builtin_huge_valf();
#pragma unroll
                    for (int q = 0; q < PR_KMAX; ++q) {
                        if (q < kk) {
                            const float lo = fminf(best[MODE == 0 ? r : 0][q], v);
                            v = fmaxf(best[MODE == 0 ? r : 0][q], v);
                            best[MODE == 0 ? r : 0][q] = lo;
                        }
                    }
                } else if (MODE == 1) {
                    if (cok && d <= rad) member |= 1u << r;
                } else {
                    const long m = r0 + la_mfma32_row(r, lh);
                    if (cok && m < nr) out_dist[m * nc + c] = d;
                }
            }
        }
    }
    if (MODE == 0) {
        // merge the 32 per-lane lists of every row: pop the global minimum kk times (ties: any owner, the value is what counts)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float kth = 0.f;
            for (int t = 0; t < kk; ++t) {
                float m = best[MODE == 0 ? r : 0][0];
                m = la_wave_min<32>(m);      // stays inside each 32-lane half
                kth = m;
                // the lowest lane holding m pops its head
                const unsigned long long has = __ballot(best[MODE == 0 ? r : 0][0] == m);
                const unsigned half = (unsigned)(lh ? (has >> 32) : (has & 0xffffffffull));
                const int owner = __builtin_ctz(half ? half : 1u);
                if (l31 == owner) {
#pragma unroll
                    for (int q = 0; q + 1 < PR_KMAX; ++q) best[MODE == 0 ? r : 0][q] = best[MODE == 0 ? r : 0][q + 1];
                    best[MODE == 0 ? r : 0][PR_KMAX - 1] = __builtin_huge_valf();
                }
            }
            const long mrow = r0 + la_mfma32_row(r, lh);
            if (l31 == 0 && mrow < nr) out_kth[mrow] = kth;
        }
    } else if (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long any = __ballot((member >> r) & 1u);
            const unsigned half = (unsigned)(lh ? (any >> 32) : (any & 0xffffffffull));
            const long mrow = r0 + la_mfma32_row(r, lh);
            if (l31 == 0 && mrow < nr) out_member[mrow] = half ? 1 : 0;
        }
    }
}

// squared norms of both feature sets into ws: [na] then [nb]
static void sqnorms_f16(const void* a, long na, const void* b, long nb, int D, float* ws, hipStream_t stream) {
    hipLaunchKernelGGL(la_rows_sqnorm_f16_kernel, dim3((unsigned)la_cdiv(na, 4)), dim3(256), 0, stream, (const _Float16*)a, na, D, ws);
    hipLaunchKernelGGL(la_rows_sqnorm_f16_kernel, dim3((unsigned)la_cdiv(nb, 4)), dim3(256), 0, stream, (const _Float16*)b, nb, D, ws + na);
}

// the three entries below: argument check, the norms of both sides, the tile launch of MODE (each entry passes the outputs it has)
template <int MODE>
static int pr_launch(const void* rows, long nr, const void* cols, long nc, int D, int kk, const float* radius, float* kth,
                     unsigned char* member, float* dist, float* ws, hipStream_t stream) {
    LA_CHECK_ARG(rows && cols && ws && nr >= 1 && nc >= 1, "pr: bad args");
    LA_CHECK_ARG(D >= 16 && D % 16 == 0, "pr: the feature dimension must be a multiple of 16 (pad with zeros)");
    LA_CHECK_ARG((((size_t)rows | (size_t)cols) & 15) == 0, "pr: feature matrices must be 16-byte aligned");
    sqnorms_f16(rows, nr, cols, nc, D, ws, stream);
    hipLaunchKernelGGL(la_pr_tile_kernel<MODE>, dim3((unsigned)la_cdiv(nr, 128)), dim3(256), 0, stream, (const _Float16*)rows, (const float*)ws,
                       nr, (const _Float16*)cols, (const float*)(ws + nr), nc, D, kk, radius, kth, member, dist);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" size_t la_pr_workspace_floats(long nr, long nc) { return (size_t)(nr + nc); }

// kth[i] = (k+1)-th smallest Euclidean distance from row i to the columns (k = nhood_size; i's own zero distance counts)
extern "C" int la_pr_kth_f16(const void* rows, long nr, const void* cols, long nc, int D, int nhood_size, float* kth, float* ws,
                             hipStream_t stream) {
    LA_CHECK_ARG(kth && nhood_size >= 0 && nhood_size + 1 <= PR_KMAX && nhood_size + 1 <= nc, "pr_kth: nhood_size out of range");
    return pr_launch<0>(rows, nr, cols, nc, D, nhood_size + 1, nullptr, kth, nullptr, nullptr, ws, stream);
}

// member[i] = 1 if dist(row i, col j) <= radius[j] for any j
extern "C" int la_pr_member_f16(const void* rows, long nr, const void* cols, long nc, int D, const float* radius,
                                unsigned char* member, float* ws, hipStream_t stream) {
    LA_CHECK_ARG(radius && member, "pr_member: bad args");
    return pr_launch<1>(rows, nr, cols, nc, D, 0, radius, nullptr, member, nullptr, ws, stream);
}

// dist[i][j] = Euclidean distance (the matrix torch.cdist returns), float32 [nr][nc]
extern "C" int la_cdist_f16(const void* rows, long nr, const void* cols, long nc, int D, float* dist, float* ws, hipStream_t stream) {
    LA_CHECK_ARG(dist, "cdist: bad args");
    return pr_launch<2>(rows, nr, cols, nc, D, 0, nullptr, nullptr, nullptr, dist, ws, stream);
}

// ------------------------------------------------------------------------------------------------------------
// FeatureStats.append: raw_mean[i] += sum_k x[k][i];  raw_cov[i][j] += sum_k x[k][i] * x[k][j]   (float64 accumulators,
// float32 features).  16x16 output tile per workgroup, the batch streamed through LDS 16 rows at a time.
__global__ __launch_bounds__(256) void la_feature_moments_kernel(const float* __restrict__ x, long n, int D, double* __restrict__ raw_mean,
                                                                double* __restrict__ raw_cov) {
    __shared__ float xi[16][17], xj[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    double acc = 0.0, msum = 0.0;
    for (long k0 = 0; k0 < n; k0 += 16) {
        const long k = k0 + ty;
        xi[ty][tx] = (k < n && i0 + tx < D) ? x[k * D + i0 + tx] : 0.f;
        xj[ty][tx] = (k < n && j0 + tx < D) ? x[k * D + j0 + tx] : 0.f;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            acc += (double)xi[q][ty] * (double)xj[q][tx];
            if (blockIdx.y == 0 && ty == 0) msum += (double)xj[q][tx];
        }
        __syncthreads();
    }
    if (i0 + ty < D && j0 + tx < D) raw_cov[(long)(i0 + ty) * D + j0 + tx] += acc;
    if (blockIdx.y == 0 && ty == 0 && j0 + tx < D) raw_mean[j0 + tx] += msum;
}

extern "C" int la_feature_moments_f64(const float* x, long n, int D, double* raw_mean, double* raw_cov, hipStream_t stream) {
    LA_CHECK_ARG(x && raw_mean && raw_cov && n >= 0 && D >= 1, "feature_moments: bad args");
    if (n == 0) return LA_OK;
    hipLaunchKernelGGL(la_feature_moments_kernel, dim3(la_cdiv(D, 16), la_cdiv(D, 16)), dim3(256), 0, stream, x, n, D, raw_mean, raw_cov);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Kernel Inception Distance: per subset s the three sums of k(a, b) = (a.b / D + 1)^3 that the unbiased MMD^2 estimator needs,
//   sxx = sum_{i != j} k(x_i, x_j),  syy = sum_{i != j} k(y_i, y_j),  sxy = sum_{i, j} k(x_i, y_j),
// over the rows x_i = X[ix[s][i]] (mx of them) and y_j = Y[iy[s][j]] (my).  The rows are gathered by index while the tiles are loaded;
// the m x m kernel matrices live in accumulator registers only: one float64 partial per 128 x 128 tile is all that reaches memory.
// Arithmetic: the exact fp32 MFMA (v_mfma_f32_32x32x2_f32) through the tile loop of la_f32_tile.h: 4 waves (2 x 2) of 64 x 64 = 2 x 2
// MFMA tiles, K walked in chunks of 16 through two LDS buffers [k][128 + 4] with the next chunk's global loads in flight, one barrier
// per chunk.
// An MFMA accumulator is one k-ordered fp32 fma chain, whose rounding error grows like sqrt(chain length); with m as small as 2 nothing
// averages it out, so a chain runs over KID_SEG chunks (128 k) only and is then added into a second fp32 accumulator (two-level
// summation: ~2.4e-7 relative on a D = 2048 dot product of non-negative features instead of ~9e-7).
// The xx and yy Grams are symmetric: only tiles with tj >= ti are computed; an off-diagonal tile counts twice, a diagonal tile sums
// both of its triangles and drops i == j.  Epilogue per element in fp32, (dot / D + 1)^3, summed in float64 per lane, then over the
// workgroup by a fixed tree.  A second launch adds the tile partials of each subset in index order: no atomics, the same bits every run.
#define KID_T 128
#define KID_KC 16
#define KID_LD (KID_T + 4)
#define KID_SEG 8

struct KidArgs {
    const float *x, *y;
    const int *ix, *iy;
    long nx, ny, mx, my;
    int D, vec;          // vec: rows are 16-byte aligned (D % 4 == 0 and aligned bases): float4 loads
    int tx, ty;          // 128-row tiles per side
    int nxx, nyy, tiles; // tiles per subset: xx upper triangle, yy upper triangle, then tx * ty of xy
    double* part;        // [S][tiles]
};

__global__ __launch_bounds__(256) void la_kid_tile_kernel(KidArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][KID_KC][KID_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KID_KC][KID_LD];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    // blockIdx.x = subset * tiles + tile (the x axis carries the subset: no 65 535 limit)
    const long s = blockIdx.x / (unsigned)a.tiles;
    int t = (int)(blockIdx.x - (unsigned)(s * a.tiles));
    const int kind = t < a.nxx ? 0 : (t < a.nxx + a.nyy ? 1 : 2);      // 0 xx, 1 yy, 2 xy
    t -= kind == 0 ? 0 : (kind == 1 ? a.nxx : a.nxx + a.nyy);
    const float* A = kind == 1 ? a.y : a.x;
    const float* B = kind == 0 ? a.x : a.y;
    const int* ia = kind == 1 ? a.iy + s * a.my : a.ix + s * a.mx;
    const int* ib = kind == 0 ? a.ix + s * a.mx : a.iy + s * a.my;
    const long ma = kind == 1 ? a.my : a.mx, mb = kind == 0 ? a.mx : a.my;
    const long na = kind == 1 ? a.ny : a.nx, nb = kind == 0 ? a.nx : a.ny;
    int ti, tj;
    if (kind == 2) {
        ti = t / a.ty;
        tj = t - ti * a.ty;
    } else {
        const int T = kind == 0 ? a.tx : a.ty;
        ti = 0;
        while (t >= T - ti) { t -= T - ti; ++ti; }
        tj = ti + t;
    }
    const long i0 = (long)ti * KID_T, j0 = (long)tj * KID_T;
    const int D = a.D;

    // loader roles: 4 threads per row (4 consecutive k each), rows tid / 4 and tid / 4 + 64 of both operands.  Rows past the end of
    // the subset load zeros; an index outside the matrix is clamped into it, so nothing is ever read out of bounds.
    const int kq = (tid & 3) * 4, lr = tid >> 2;
    const float *pa[2], *pb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long i = i0 + lr + 64 * j, c = j0 + lr + 64 * j;
        pa[j] = pb[j] = nullptr;
        if (i < ma) { long r = ia[i]; r = r < 0 ? 0 : (r >= na ? na - 1 : r); pa[j] = A + r * D; }
        if (c < mb) { long r = ib[c]; r = r < 0 ? 0 : (r >= nb ? nb - 1 : r); pb[j] = B + r * D; }
    }
    float4 areg[2], breg[2];
    auto fetch = [&](const float* p, int k) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p && k < D) {
            if (a.vec) {
                v = *reinterpret_cast<const float4*>(p + k);      // D % 4 == 0: k + 3 < D
            } else {
                v.x = p[k];
                if (k + 1 < D) v.y = p[k + 1];
                if (k + 2 < D) v.z = p[k + 2];
                if (k + 3 < D) v.w = p[k + 3];
            }
        }
        return v;
    };
    auto prefetch = [&](int ci) {
        const int k = ci * KID_KC + kq;
#pragma unroll
        for (int j = 0; j < 2; ++j) { areg[j] = fetch(pa[j], k); breg[j] = fetch(pb[j], k); }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = lr + 64 * j;
            As[buf][kq][r] = areg[j].x; As[buf][kq + 1][r] = areg[j].y; As[buf][kq + 2][r] = areg[j].z; As[buf][kq + 3][r] = areg[j].w;
            Bs[buf][kq][r] = breg[j].x; Bs[buf][kq + 1][r] = breg[j].y; Bs[buf][kq + 2][r] = breg[j].z; Bs[buf][kq + 3][r] = breg[j].w;
        }
    };

    la_f32x16 acc[2][2], tot[2][2];
    la_f32_tile_zero(acc);
    la_f32_tile_zero(tot);

    const int nchunk = (D + KID_KC - 1) / KID_KC;
    __builtin_assume(nchunk > 0);      // D >= 1 (la_kid_poly3_f32 refuses less): without it the compiler keeps a second copy of the loop
    la_tile_pipeline(0, nchunk, prefetch, stage, [&](int buf, int ci) {
        la_f32_tile_mma<KID_KC>(As, Bs, buf, wm * 64, wn * 64, l31, lh, acc);
        if ((ci & (KID_SEG - 1)) == KID_SEG - 1 || ci + 1 == nchunk) {      // end of a chain: fold it into the second level
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { tot[i][j][r] += acc[i][j][r]; acc[i][j][r] = 0.f; }
        }
    });

    const bool diag = kind != 2 && ti == tj;
    const float fD = (float)D;
    double dsum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long n = j0 + wn * 64 + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = i0 + wm * 64 + i * 32 + la_mfma32_row(r, lh);
                if (m < ma && n < mb && !(diag && m == n)) {
                    const float v = tot[i][j][r] / fD + 1.f;
                    dsum += (double)(v * v * v);
                }
            }
        }
    la_block_tree_sum_256(dsum, red);
    if (tid == 0) a.part[blockIdx.x] = (kind != 2 && ti != tj) ? 2.0 * red[0] : red[0];
}

// one workgroup per subset: the tile partials of each of the three sums in index order (thread-strided, then the fixed tree)
__global__ __launch_bounds__(256) void la_kid_finish_kernel(const double* __restrict__ part, int nxx, int nyy, int tiles, long mx, long my,
                                                           double* __restrict__ sums, double* __restrict__ mmd2) {
    __shared__ double red[256];
    const long s = blockIdx.x;
    const double* p = part + s * tiles;
    const int beg[4] = {0, nxx, nxx + nyy, tiles};
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double acc = 0.0;
        for (int t = beg[q] + (int)threadIdx.x; t < beg[q + 1]; t += 256) acc += p[t];
        la_block_tree_sum_256(acc, red);
        v[q] = red[0];
    }
    if (threadIdx.x == 0) {
        sums[s * 3 + 0] = v[0];
        sums[s * 3 + 1] = v[1];
        sums[s * 3 + 2] = v[2];
        mmd2[s] = v[0] / ((double)mx * (double)(mx - 1)) + v[1] / ((double)my * (double)(my - 1)) - 2.0 * v[2] / ((double)mx * (double)my);
    }
}

__global__ __launch_bounds__(256) void la_kid_mean_kernel(const double* __restrict__ mmd2, long S, double* __restrict__ kid) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long s = threadIdx.x; s < S; s += 256) acc += mmd2[s];
    la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) kid[0] = red[0] / (double)S;
}

static inline long kid_tiles(long mx, long my) {
    const long tx = (mx + KID_T - 1) / KID_T, ty = (my + KID_T - 1) / KID_T;
    return tx * (tx + 1) / 2 + ty * (ty + 1) / 2 + tx * ty;
}

// one float64 partial per tile and subset (0 for sizes the launch refuses)
extern "C" size_t la_kid_workspace_bytes(long S, long mx, long my) {
    if (S < 1 || mx < 2 || my < 2 || mx > 0x7fffffffL || my > 0x7fffffffL) return 0;
    return (size_t)S * (size_t)kid_tiles(mx, my) * sizeof(double);
}

extern "C" int la_kid_poly3_f32(const float* x, long nx, const float* y, long ny, int D, const int* ix, const int* iy, long S, long mx,
                                long my, double* sums, double* mmd2, double* kid, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(x && y && ix && iy && sums && mmd2 && kid && ws, "kid: null pointer");
    LA_CHECK_ARG(mx >= 2 && my >= 2, "kid: a subset needs at least 2 rows per side (the estimator divides by m (m - 1))");
    LA_CHECK_ARG(D >= 1 && S >= 1 && nx >= 1 && ny >= 1, "kid: D, the number of subsets and the row counts must be positive");
    LA_CHECK_ARG(mx <= 0x7fffffffL && my <= 0x7fffffffL && nx <= 0x7fffffffL && ny <= 0x7fffffffL, "kid: sizes beyond int32 indices");
    const long tiles = kid_tiles(mx, my);
    LA_CHECK_ARG(tiles <= 0x7fffffffL / S, "kid: num_subsets x tiles exceeds the grid");
    LA_CHECK_WORKSPACE(ws_bytes, la_kid_workspace_bytes(S, mx, my), "kid: workspace smaller than la_kid_workspace_bytes(S, mx, my)");
    LA_CHECK_ARG(la_aligned<8>(ws), "kid: the workspace must be 8-byte aligned");
    KidArgs a;
    a.x = x; a.y = y; a.ix = ix; a.iy = iy;
    a.nx = nx; a.ny = ny; a.mx = mx; a.my = my;
    a.D = D;
    a.vec = (D % 4 == 0 && (((size_t)x | (size_t)y) & 15) == 0) ? 1 : 0;
    a.tx = (int)((mx + KID_T - 1) / KID_T); a.ty = (int)((my + KID_T - 1) / KID_T);
    a.nxx = (int)((long)a.tx * (a.tx + 1) / 2); a.nyy = (int)((long)a.ty * (a.ty + 1) / 2); a.tiles = (int)tiles;
    a.part = (double*)ws;
    hipLaunchKernelGGL(la_kid_tile_kernel, dim3((unsigned)(S * tiles)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(la_kid_finish_kernel, dim3((unsigned)S), dim3(256), 0, stream, (const double*)a.part, a.nxx, a.nyy, a.tiles, mx, my,
                       sums, mmd2);
    hipLaunchKernelGGL(la_kid_mean_kernel, dim3(1), dim3(256), 0, stream, (const double*)mmd2, S, kid);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Density and coverage (Naeem et al., ICML 2020): one tiled pass over the ng x nr grid of (generated row j, real column i) pairs,
//   count[j]   = #{ i : dist(Y_j, X_i) <= radius[i] }      (int32; density = sum_j count[j] / (k ng))
//   nearest[i] = min_j dist(Y_j, X_i)                        (float32; covered[i] = nearest[i] <= radius[i])
// with dist and the fragments exactly as la_pr_tile_kernel has them.  Only the real samples' balls are used: radius[i] is the
// (k+1)-th smallest distance from real i to the reals (la_pr_kth_f16(real, real)), kept in float32.
// Grid: x = blocks of 128 generated rows (4 waves x 32), y = column chunks of `chunk` (a multiple of 128) real columns; the number
// of chunks is the host rule dc_col_splits.  A workgroup walks its chunk in steps of 128 columns, and each step's K range in chunks
// of DC_KC = 64: the 128 x 64 tiles of both operands go through LDS (two buffers each, the next chunk's global loads in flight during
// the MFMAs, one barrier per chunk: la_tile_pipeline of la_f32_tile.h).  Eight lanes load 128 contiguous bytes of a row, so every
// cache line that is touched is used whole, and the four waves share one copy of the column tile; rows of 64 + 8 halves (144 bytes) keep the 16-byte
// fragment reads of 16 consecutive rows on distinct banks.  K past D is filled with zeros (an exact no-op in the accumulator).
// Every accumulator is the same k-ordered chain as in la_pr_tile_kernel and both kernels form the distance with la_pr_dist, so a
// distance has the same bits here and in la_pr_kth_f16.
// Row side: every lane counts, for its 16 rows, the columns it sees (one per MFMA tile) in 16 integer registers over the whole chunk;
// the 32 lanes of a half are summed once at the end and one lane adds the row's total into count[] with an integer atomicAdd.
// Column side: per step of 128 columns a lane takes the minimum over its 16 rows, the two lane halves are combined by a shuffle, the
// four waves through LDS (two buffers, one barrier per step), and 128 threads fold the workgroup's minimum into nearest[] with
// atomicMin on the bit pattern (the distances are positive floats, whose order is the order of their bits as unsigned integers).
// Integer adds and minima do not depend on their order: two runs give the same bits.
// count[] and nearest[] are initialised by la_dc_init_kernel on the same stream.
#define DC_TARGET_WG 512      // about two workgroups per CU of a 256-CU device
#define DC_KC 64
#define DC_LD (DC_KC + 8)

__global__ __launch_bounds__(256) void la_dc_init_kernel(int* __restrict__ count, long ng, unsigned* __restrict__ nearest, long nr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < ng) count[i] = 0;
    if (i < nr) nearest[i] = 0x7f800000u;      // +inf
}

__global__ __launch_bounds__(256) void la_dc_tile_kernel(const _Float16* __restrict__ rows, const float* __restrict__ rown, long ng,
                                                        const _Float16* __restrict__ cols, const float* __restrict__ coln, long nr,
                                                        int D, long chunk, const float* __restrict__ radius, int* __restrict__ count,
                                                        unsigned* __restrict__ nearest) {
    __shared__ __attribute__((aligned(16))) _Float16 As[2][128][DC_LD];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[2][128][DC_LD];
    __shared__ float smin[2][4][128];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const long b0 = (long)blockIdx.x * 128;                     // b0 < ng: the grid has no empty row block
    const long r0 = b0 + wid * 32;                              // a wave past the end works on clamped rows and contributes nothing
    const long cbeg = (long)blockIdx.y * chunk;
    const long cend = cbeg + chunk < nr ? cbeg + chunk : nr;
    // rows held by this lane: m(r) = (r&3) + 8*(r>>2) + 4*lh
    float na[16];
    int cnt[16];
    unsigned rowok = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = r0 + la_mfma32_row(r, lh);
        na[r] = rown[m < ng ? m : ng - 1];
        cnt[r] = 0;
        if (m < ng) rowok |= 1u << r;
    }
    // loader roles: 8 threads per tile row (8 halves = 16 bytes each), tile rows tid / 8 + 32 p of both operands.  A row past the end
    // of its matrix is clamped into it, so nothing is read out of bounds; what it yields is masked in the epilogue.
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const _Float16 *pa[4], *pb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const long m = b0 + p * 32 + lrow;
        pa[p] = rows + (m < ng ? m : ng - 1) * D + lk;
    }
    f16x8 areg[4], breg[4];
    auto prefetch = [&](int kc) {
        const int k = kc * DC_KC;
        const bool in = k + lk < D;                             // D % 16 == 0: the 8 halves are inside or outside together
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = 0; q < 8; ++q) areg[p][q] = breg[p][q] = (_Float16)0.f;
            if (in) {
                areg[p] = *reinterpret_cast<const f16x8*>(pa[p] + k);
                breg[p] = *reinterpret_cast<const f16x8*>(pb[p] + k);
            }
        }
    };
    auto stage = [&](int b) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f16x8*>(&As[b][p * 32 + lrow][lk]) = areg[p];
            *reinterpret_cast<f16x8*>(&Bs[b][p * 32 + lrow][lk]) = breg[p];
        }
    };
    const int nkc = (D + DC_KC - 1) / DC_KC;
    int sbuf = 0;
    for (long c0 = cbeg; c0 < cend; c0 += 128, sbuf ^= 1) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long c = c0 + p * 32 + lrow;
            pb[p] = cols + (c < nr ? c : nr - 1) * D + lk;
        }
        la_f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        // the K loop of the step (la_f32_tile.h; LDS is free on its return, so the next step may stage into buffer 0 at once)
        la_tile_pipeline(0, nkc, prefetch, stage, [&](int b, int) {
#pragma unroll
            for (int ks = 0; ks < DC_KC / 16; ++ks) {
                const f16x8 af = *reinterpret_cast<const f16x8*>(&As[b][wid * 32 + l31][ks * 16 + lh * 8]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f16x8 bf = *reinterpret_cast<const f16x8*>(&Bs[b][j * 32 + l31][ks * 16 + lh * 8]);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[j], 0, 0, 0);
                }
            }
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long c = c0 + j * 32 + l31;
            const bool cok = c < cend;
            const float nb = coln[c < nr ? c : nr - 1];
            const float rad = radius[c < nr ? c : nr - 1];
            float cm = __builtin_huge_valf();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = la_pr_dist(na[r], nb, acc[j][r]);
                const bool ok = cok && ((rowok >> r) & 1u);
                if (ok && d <= rad) ++cnt[r];
                cm = fminf(cm, ok ? d : __builtin_huge_valf());
            }
            cm = fminf(cm, __shfl_xor(cm, 32, 64));          // the other 16 rows of the same column
            if (lh == 0) smin[sbuf][wid][j * 32 + l31] = cm;
        }
        // One barrier per step: buffer `sbuf` is next written two steps on, after the barriers of the step between, which its readers
        // below reach only when they have read it.
        __syncthreads();
        if (tid < 128 && c0 + tid < cend) {
            const float m = fminf(fminf(smin[sbuf][0][tid], smin[sbuf][1][tid]), fminf(smin[sbuf][2][tid], smin[sbuf][3][tid]));
            atomicMin(nearest + c0 + tid, __float_as_uint(m));
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int s = cnt[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);      // stays inside each 32-lane half
        const long mrow = r0 + la_mfma32_row(r, lh);
        if (l31 == 0 && mrow < ng && s) atomicAdd(count + mrow, s);
    }
}

// columns per chunk (a multiple of 128): enough chunks that row blocks x chunks reaches DC_TARGET_WG workgroups, never more chunks
// than there are 128-column steps
static inline long dc_chunk_cols(long ng, long nr) {
    const long rb = (ng + 127) / 128, ct = (nr + 127) / 128;
    long want = (DC_TARGET_WG + rb - 1) / rb;
    if (want > ct) want = ct;
    return (ct + want - 1) / want * 128;
}

// number of column chunks of the launch (0 for sizes it refuses)
extern "C" int la_dc_col_splits(long ng, long nr) {
    if (ng < 1 || nr < 1) return 0;
    const long chunk = dc_chunk_cols(ng, nr);
    return (int)((nr + chunk - 1) / chunk);
}

// the squared norms of both sides, fp32 (0 for sizes the launch refuses)
extern "C" size_t la_dc_workspace_bytes(long ng, long nr) {
    if (ng < 1 || nr < 1) return 0;
    return ((size_t)ng + (size_t)nr) * sizeof(float);
}

extern "C" int la_dc_count_f16(const void* gen, long ng, const void* real, long nr, int D, const float* radius, int* count,
                               float* nearest, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(gen && real && radius && count && nearest && ws, "dc: null pointer");
    LA_CHECK_ARG(ng >= 1 && nr >= 1, "dc: both feature sets need at least one row");
    LA_CHECK_ARG(D >= 16 && D % 16 == 0, "dc: the feature dimension must be a multiple of 16 (pad with zeros)");
    LA_CHECK_ARG((((size_t)gen | (size_t)real) & 15) == 0, "dc: feature matrices must be 16-byte aligned");
    LA_CHECK_ARG(la_aligned<4>(radius, count, nearest, ws), "dc: radius, count, nearest and ws must be 4-byte aligned");
    const long chunk = dc_chunk_cols(ng, nr);
    const long rb = (ng + 127) / 128, splits = (nr + chunk - 1) / chunk;
    LA_CHECK_ARG(rb <= 0x7fffffffL && splits <= 65535, "dc: sizes exceed the grid");
    LA_CHECK_WORKSPACE(ws_bytes, la_dc_workspace_bytes(ng, nr), "dc: workspace smaller than la_dc_workspace_bytes(ng, nr)");
    float* gn = (float*)ws;
    float* rn = gn + ng;
    const long nmax = ng > nr ? ng : nr;
    hipLaunchKernelGGL(la_dc_init_kernel, dim3((unsigned)la_cdiv(nmax, 256)), dim3(256), 0, stream, count, ng, (unsigned*)nearest, nr);
    sqnorms_f16(gen, ng, real, nr, D, gn, stream);
    hipLaunchKernelGGL(la_dc_tile_kernel, dim3((unsigned)rb, (unsigned)splits), dim3(256), 0, stream, (const _Float16*)gen, (const float*)gn,
                       ng, (const _Float16*)real, (const float*)rn, nr, D, chunk, radius, count, (unsigned*)nearest);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
