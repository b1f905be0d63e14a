// Frechet distance of two feature sets without a covariance matrix or a matrix square root (gfx950 only).
//
// With A [Ng][D], B [Nr][D] the generated and real features minus their column means and the reference's 1/N covariance
// (metric_utils.py:136-140):
//   FD = |mu_g - mu_r|^2 + |A|_F^2 / Ng + |B|_F^2 / Nr - 2 nuc(A B^T) / sqrt(Ng Nr)
// nuc = the sum of the singular values: the non-zero eigenvalues of Sigma_g Sigma_r are the squared singular values of
// A B^T / sqrt(Ng Nr).  A B^T is Ng x Nr -- small where the sets are small -- and its singular values are well conditioned where the
// square root of the singular D x D product is not.
//
// Three entries; the caller runs the sweep loop between them (the number of sweeps depends on the data):
//   la_fd_gram_f32          float64 column means (row chunks of FD_ROWS rows summed in row order, the chunk partials added in chunk
//                           order), then C = (x - mu_x)(y - mu_y)^T on v_mfma_f64_16x16x4_f64.  The float32 operands are widened and
//                           centred in float64 on their way into LDS: no centred copy exists in memory in any type.  A workgroup owns a
//                           64 x 64 tile of C (4 waves, 2 x 2 MFMA tiles each) and walks D in chunks of FD_KC; k past D is stored as 0.
//                           The side with FEWER rows is the MFMA's A operand, so C comes out as n = min(nx, ny) vectors of
//                           m = max(nx, ny) contiguous doubles whichever side is the smaller (the product of two doubles does not
//                           depend on the order of its factors and the k order is the same: C and C^T have the same bits); 16 lanes
//                           store 128 contiguous bytes.  An odd n gets one zero vector appended by the same launch.
//                           f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 map.
//   la_fd_jacobi_sweep_f64  one-sided Jacobi (Hestenes): n' - 1 rounds of the circle method, one launch per round, one workgroup per
//                           pair.  A PAIR LIVES IN REGISTERS: thread t holds elements t, t + 256, ... of both vectors (up to 32 each,
//                           m <= 8192; the kernel is instantiated for 1, 2, 4, 8, 16 and 32), so a vector is read once per round and
//                           written at most once.  Longer vectors take the streaming instantiation, which reads a rotated pair twice.
//   la_fd_finish_f64        the vector norms (= singular values) and their sum.
// Every float64 sum is thread-strided and then a fixed tree (la_block_tree_sum_256): no float atomics anywhere, two runs give the same bits.
// The only atomic is the integer count of rotations.
#include "la_f64_tile.h"      // FD_T, FD_KC and the tile product, shared with la_knn.hip

#include <math.h>

#define FD_ROWS 64           // rows per column-sum chunk
#define FD_MAX_N 8192

// pair k (0 .. n2/2 - 1) of round `round` (0 .. n2 - 2) of the round-robin tournament of n2 (even) players, circle method:
// player n2 - 1 stays, the others rotate.  p < q.
__host__ __device__ static inline void fd_round_pair(int n2, int round, int k, int* p, int* q) {
    const int r1 = n2 - 1;
    const int a = k == 0 ? r1 : (round + k) % r1;
    const int b = k == 0 ? round : (round - k + r1) % r1;
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

extern "C" int la_fd_round_pair(int n, int round, int k, int* p, int* q) {
    LA_CHECK_ARG(p && q, "fd_round_pair: null pointer");
    LA_CHECK_ARG(n >= 2 && n <= FD_MAX_N, "fd_round_pair: n must lie in 2 .. 8192");
    const int n2 = (n + 1) & ~1;
    LA_CHECK_ARG(round >= 0 && round < n2 - 1 && k >= 0 && k < n2 / 2, "fd_round_pair: round in 0 .. n' - 2 and k in 0 .. n'/2 - 1");
    fd_round_pair(n2, round, k, p, q);
    return LA_OK;
}

// three sums at once for the Jacobi round (one barrier): xor tree inside each wave, then the four waves in wave order.  Every thread
// gets the sums.  red: 12 doubles of LDS
__device__ __forceinline__ void fd_block_sum3(double& a, double& b, double& c, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid * 3 + 0] = a; red[wid * 3 + 1] = b; red[wid * 3 + 2] = c; }
    __syncthreads();
    a = ((red[0] + red[3]) + red[6]) + red[9];
    b = ((red[1] + red[4]) + red[7]) + red[10];
    c = ((red[2] + red[5]) + red[8]) + red[11];
}

// ------------------------------------------------------------------------------------------------------------ means and scalar terms
// part[chunk][d] = sum of x[r][d] over the chunk's rows in row order.  grid (ceil(D / 256), chunks)
__global__ __launch_bounds__(256) void la_fd_colsum_kernel(const float* __restrict__ x, long N, int D, double* __restrict__ part) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const long r0 = (long)blockIdx.y * FD_ROWS;
    const long r1 = r0 + FD_ROWS < N ? r0 + FD_ROWS : N;
    double acc = 0.0;
    for (long r = r0; r < r1; ++r) acc += (double)x[r * D + d];
    part[(long)blockIdx.y * D + d] = acc;
}

// mu[d] = (sum of the chunk partials in chunk order) / N.  grid (ceil(D / 256), 2): y = 0 the x side, 1 the y side
__global__ __launch_bounds__(256) void la_fd_mean_kernel(const double* __restrict__ partx, int chunksx, long nx, double* __restrict__ mux,
                                                        const double* __restrict__ party, int chunksy, long ny, double* __restrict__ muy,
                                                        int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const double* part = blockIdx.y ? party : partx;
    const int chunks = blockIdx.y ? chunksy : chunksx;
    double acc = 0.0;
    for (int c = 0; c < chunks; ++c) acc += part[(long)c * D + d];
    (blockIdx.y ? muy : mux)[d] = acc / (double)(blockIdx.y ? ny : nx);
}

// rowsq[i] = sum_d (x[i][d] - mu[d])^2; rows 0 .. nx - 1 are x's, nx .. nx + ny - 1 are y's.  grid nx + ny
__global__ __launch_bounds__(256) void la_fd_rowsq_kernel(const float* __restrict__ x, long nx, const double* __restrict__ mux,
                                                         const float* __restrict__ y, const double* __restrict__ muy, int D,
                                                         double* __restrict__ rowsq) {
    __shared__ double red[256];
    const long b = blockIdx.x;
    const float* row = b < nx ? x + b * D : y + (b - nx) * D;
    const double* mu = b < nx ? mux : muy;
    double acc = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double v = (double)row[d] - mu[d];
        acc += v * v;
    }
    acc = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) rowsq[b] = acc;
}

// terms[0..2] = |mu_x - mu_y|^2, |A|_F^2, |B|_F^2.  one workgroup
__global__ __launch_bounds__(256) void la_fd_terms_kernel(const double* __restrict__ mux, const double* __restrict__ muy, int D,
                                                         const double* __restrict__ rowsq, long nx, long ny, double* __restrict__ terms) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double v = mux[d] - muy[d];
        acc += v * v;
    }
    const double t0 = la_block_tree_sum_256(acc, red);
    acc = 0.0;
    for (long i = threadIdx.x; i < nx; i += 256) acc += rowsq[i];
    const double t1 = la_block_tree_sum_256(acc, red);
    acc = 0.0;
    for (long i = threadIdx.x; i < ny; i += 256) acc += rowsq[nx + i];
    const double t2 = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) { terms[0] = t0; terms[1] = t1; terms[2] = t2; }
}

// ------------------------------------------------------------------------------------------------------------ centred cross-Gram matrix
// V[i][j] = sum_k (p[i][k] - mup[k]) (q[j][k] - muq[k]), i < np (the vectors), j < nq (their elements, nq doubles per vector).
// grid (ceil(nq / 64), ceil(np / 64)).  A row past the end of its matrix is clamped into it (nothing is read out of bounds) and
// masked at the store.  pad: vector np is written as zeros by the workgroups of the first tile row.
__global__ __launch_bounds__(256) void la_fd_gram_kernel(const float* __restrict__ p, long np, const double* __restrict__ mup,
                                                        const float* __restrict__ q, long nq, const double* __restrict__ muq, int D,
                                                        double* __restrict__ V, int pad) {
    __shared__ double Ps[FD_T][FD_LD];
    __shared__ double Qs[FD_T][FD_LD];
    const int tid = threadIdx.x;
    const FdLane t = fd_tile_lane();
    const long i0 = (long)blockIdx.y * FD_T, j0 = (long)blockIdx.x * FD_T;
    const int lk = tid & 31, lr = tid >> 5;          // loader roles
    fd_f64x4 acc[2][2];
    fd_tile_zero(acc);
    // staging and fragments: la_f64_tile.h
    fd_tile_loop<true>(Ps, Qs, p, np, mup, i0, q, nq, muq, j0, D, lk, lr,
                       [&](const double (*P)[FD_LD], const double (*Q)[FD_LD]) { fd_tile_mma(P, Q, acc, t); });
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long col = j0 + fd_tile_col(t, j);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = i0 + fd_tile_row(t, i, r);
                if (row < np && col < nq) V[row * nq + col] = acc[i][j][r];
            }
        }
    if (pad && blockIdx.y == 0 && tid < FD_T && j0 + tid < nq) V[np * nq + j0 + tid] = 0.0;
}

// ------------------------------------------------------------------------------------------------------------ one Jacobi round
// E > 0: elements tid + 256 e (e < E) of both vectors in registers, m <= 256 E.  E == 0: streaming, any m.
template <int E>
__global__ __launch_bounds__(256) void la_fd_jacobi_round_kernel(double* __restrict__ v, int n2, long m, int round, double tol,
                                                                int* __restrict__ rotations) {
    __shared__ double red[12];
    int p, q;
    fd_round_pair(n2, round, (int)blockIdx.x, &p, &q);
    double* cp = v + (long)p * m;
    double* cq = v + (long)q * m;
    const int tid = threadIdx.x;
    constexpr int R = E > 0 ? E : 1;
    double a[R], b[R];
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
    if (E > 0) {
#pragma unroll
        for (int e = 0; e < R; ++e) {
            const long i = tid + 256L * e;
            a[e] = i < m ? cp[i] : 0.0;
            b[e] = i < m ? cq[i] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < R; ++e) {
            alpha += a[e] * a[e];
            beta += b[e] * b[e];
            gamma += a[e] * b[e];
        }
    } else {
        for (long i = tid; i < m; i += 256) {
            const double x = cp[i], y = cq[i];
            alpha += x * x;
            beta += y * y;
            gamma += x * y;
        }
    }
    fd_block_sum3(alpha, beta, gamma, red);
    const double ab = alpha * beta;
    if (!(ab > 0.0) || !(fabs(gamma) > tol * sqrt(ab))) return;      // (uniform over the workgroup)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = zeta == 0.0 ? 1.0 : copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    if (E > 0) {
#pragma unroll
        for (int e = 0; e < R; ++e) {
            const long i = tid + 256L * e;
            if (i < m) {
                cp[i] = c * a[e] - s * b[e];
                cq[i] = s * a[e] + c * b[e];
            }
        }
    } else {
        for (long i = tid; i < m; i += 256) {
            const double x = cp[i], y = cq[i];
            cp[i] = c * x - s * y;
            cq[i] = s * x + c * y;
        }
    }
    if (tid == 0) atomicAdd(rotations, 1);
}

// ------------------------------------------------------------------------------------------------------------ singular values
// norms[i] = |vector i|.  grid n
__global__ __launch_bounds__(256) void la_fd_norm_kernel(const double* __restrict__ v, long m, double* __restrict__ norms,
                                                        double* __restrict__ sv) {
    __shared__ double red[256];
    const double* c = v + (long)blockIdx.x * m;
    double acc = 0.0;
    for (long i = threadIdx.x; i < m; i += 256) acc += c[i] * c[i];
    acc = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) {
        const double s = sqrt(acc);
        norms[blockIdx.x] = s;
        if (sv) sv[blockIdx.x] = s;
    }
}

// nuc[0] = sum of the norms in index order (thread-strided, then the fixed tree).  one workgroup
__global__ __launch_bounds__(256) void la_fd_nuc_kernel(const double* __restrict__ norms, long n, double* __restrict__ nuc) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += norms[i];
    acc = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) nuc[0] = acc;
}

// ------------------------------------------------------------------------------------------------------------ host side
// The workspace: the n' vectors of m (first: la_fd_jacobi_sweep_f64 is handed the start of the workspace as its vectors), then what
// the Gram and finish entries need beside them.
struct FdLayout {
    long n, n2, m;
    int chunksx, chunksy;
    double *vec, *mux, *muy, *partx, *party, *rowsq, *norms;
    size_t bytes;
};

static inline bool fd_sizes_ok(long nx, long ny, int D) {
    const long n = nx < ny ? nx : ny, m = nx < ny ? ny : nx;
    return nx >= 2 && ny >= 2 && D >= 1 && n <= FD_MAX_N && m <= 65535L * FD_ROWS;      // (the row chunks are a grid's y axis)
}

static inline FdLayout fd_layout(long nx, long ny, int D, void* base) {
    FdLayout L;
    L.n = nx < ny ? nx : ny;
    L.m = nx < ny ? ny : nx;
    L.n2 = (L.n + 1) & ~1L;
    L.chunksx = la_cdiv(nx, FD_ROWS);
    L.chunksy = la_cdiv(ny, FD_ROWS);
    LaCarver c{(char*)base};
    L.vec = c.take<double>((size_t)L.n2 * (size_t)L.m);
    L.mux = c.take<double>((size_t)D);
    L.muy = c.take<double>((size_t)D);
    L.partx = c.take<double>((size_t)L.chunksx * (size_t)D);
    L.party = c.take<double>((size_t)L.chunksy * (size_t)D);
    L.rowsq = c.take<double>((size_t)nx + (size_t)ny);
    L.norms = c.take<double>((size_t)L.n2);
    L.bytes = c.off;
    return L;
}

// bytes of the workspace of one problem (0 for sizes the entries refuse)
extern "C" size_t la_fd_workspace_bytes(long nx, long ny, int D) {
    if (!fd_sizes_ok(nx, ny, D)) return 0;
    return fd_layout(nx, ny, D, nullptr).bytes;
}

static int fd_check_sizes(long nx, long ny, int D) {
    LA_CHECK_ARG(nx >= 2 && ny >= 2, "fd: each feature set needs at least 2 rows");
    LA_CHECK_ARG(D >= 1, "fd: the feature dimension must be positive");
    LA_CHECK_ARG((nx < ny ? nx : ny) <= FD_MAX_N,
                 "fd: min(nx, ny) > 8192 is the many-samples regime: use the moments route (compute_fid_from_stats)");
    LA_CHECK_ARG(fd_sizes_ok(nx, ny, D), "fd: sizes exceed the grid");
    return LA_OK;
}

extern "C" int la_fd_gram_f32(const float* x, long nx, const float* y, long ny, int D, double* terms, void* ws, size_t ws_bytes,
                              hipStream_t stream) {
    LA_CHECK_ARG(x && y && terms && ws, "fd_gram: null pointer");
    if (const int rc = fd_check_sizes(nx, ny, D)) return rc;
    LA_CHECK_WORKSPACE(ws_bytes, la_fd_workspace_bytes(nx, ny, D), "fd_gram: workspace smaller than la_fd_workspace_bytes(nx, ny, D)");
    LA_CHECK_ARG(la_aligned<4>(x, y) && la_aligned<8>(ws, terms),
                 "fd_gram: features must be 4-byte aligned, terms and the workspace 8-byte aligned");
    const FdLayout L = fd_layout(nx, ny, D, ws);
    const unsigned dblocks = (unsigned)la_cdiv(D, 256);
    hipLaunchKernelGGL(la_fd_colsum_kernel, dim3(dblocks, (unsigned)L.chunksx), dim3(256), 0, stream, x, nx, D, L.partx);
    hipLaunchKernelGGL(la_fd_colsum_kernel, dim3(dblocks, (unsigned)L.chunksy), dim3(256), 0, stream, y, ny, D, L.party);
    hipLaunchKernelGGL(la_fd_mean_kernel, dim3(dblocks, 2), dim3(256), 0, stream, (const double*)L.partx, L.chunksx, nx, L.mux,
                       (const double*)L.party, L.chunksy, ny, L.muy, D);
    hipLaunchKernelGGL(la_fd_rowsq_kernel, dim3((unsigned)(nx + ny)), dim3(256), 0, stream, x, nx, (const double*)L.mux, y,
                       (const double*)L.muy, D, L.rowsq);
    hipLaunchKernelGGL(la_fd_terms_kernel, dim3(1), dim3(256), 0, stream, (const double*)L.mux, (const double*)L.muy, D,
                       (const double*)L.rowsq, nx, ny, terms);
    // the side with fewer rows supplies the vectors: C for nx <= ny, C^T otherwise, by exchanging the operands
    const bool xs = nx <= ny;
    const float* p = xs ? x : y;
    const float* q = xs ? y : x;
    const double* mup = xs ? L.mux : L.muy;
    const double* muq = xs ? L.muy : L.mux;
    hipLaunchKernelGGL(la_fd_gram_kernel, dim3((unsigned)la_cdiv(L.m, FD_T), (unsigned)la_cdiv(L.n, FD_T)), dim3(256), 0, stream, p, L.n, mup,
                       q, L.m, muq, D, L.vec, (int)(L.n2 != L.n));
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_fd_jacobi_sweep_f64(double* v, long n, long m, int* rotations, hipStream_t stream) {
    LA_CHECK_ARG(v && rotations, "fd_jacobi_sweep: null pointer");
    LA_CHECK_ARG(n >= 2 && n <= FD_MAX_N, "fd_jacobi_sweep: the number of vectors must lie in 2 .. 8192");
    LA_CHECK_ARG(m >= 1 && m <= 0x7fffffffL, "fd_jacobi_sweep: the vector length must lie in 1 .. 2^31 - 1");
    LA_CHECK_ARG(la_aligned<8>(v) && la_aligned<4>(rotations), "fd_jacobi_sweep: v must be 8-byte and rotations 4-byte aligned");
    const int n2 = (int)((n + 1) & ~1L);
    const double tol = ldexp(sqrt((double)m), -52);      // LAPACK dgesvj's criterion: sqrt(m) eps
    LA_HIP(hipMemsetAsync(rotations, 0, sizeof(int), stream));
    void (*kern)(double*, int, long, int, double, int*) =
        m <= 256 ? la_fd_jacobi_round_kernel<1> : m <= 512 ? la_fd_jacobi_round_kernel<2> : m <= 1024 ? la_fd_jacobi_round_kernel<4>
        : m <= 2048 ? la_fd_jacobi_round_kernel<8> : m <= 4096 ? la_fd_jacobi_round_kernel<16>
        : m <= 8192 ? la_fd_jacobi_round_kernel<32> : la_fd_jacobi_round_kernel<0>;
    for (int round = 0; round < n2 - 1; ++round)
        hipLaunchKernelGGL(kern, dim3((unsigned)(n2 / 2)), dim3(256), 0, stream, v, n2, m, round, tol, rotations);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_fd_finish_f64(void* ws, size_t ws_bytes, long nx, long ny, int D, double* sv, double* terms, hipStream_t stream) {
    LA_CHECK_ARG(ws && terms, "fd_finish: null pointer");
    if (const int rc = fd_check_sizes(nx, ny, D)) return rc;
    LA_CHECK_WORKSPACE(ws_bytes, la_fd_workspace_bytes(nx, ny, D), "fd_finish: workspace smaller than la_fd_workspace_bytes(nx, ny, D)");
    LA_CHECK_ARG(la_aligned<8>(ws, terms, sv), "fd_finish: the workspace, terms and sv must be 8-byte aligned");
    const FdLayout L = fd_layout(nx, ny, D, ws);
    hipLaunchKernelGGL(la_fd_norm_kernel, dim3((unsigned)L.n), dim3(256), 0, stream, (const double*)L.vec, L.m, L.norms, sv);
    hipLaunchKernelGGL(la_fd_nuc_kernel, dim3(1), dim3(256), 0, stream, (const double*)L.norms, L.n, terms + 3);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
