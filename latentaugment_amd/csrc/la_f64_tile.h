// The float64 tile product shared by the cross-Gram kernel of the Frechet distance (la_frechet.hip) and the nearest-neighbour kernels
// (la_knn.hip): a workgroup of 256 threads (4 waves, 2 x 2 MFMA tiles each) forms a 64 x 64 tile of P Q^T on
// v_mfma_f64_16x16x4_f64, walking k in chunks of FD_KC.  The float32 operands are widened (and, for the Gram matrix, centred) in
// float64 on their way into LDS; k past D is stored as 0.  One k order whatever the tile: element (i, j) is the same chain of MFMA
// steps over k = 0, 4, 8, .. wherever the pair sits in the grid, so its bits depend on the two rows and D only.
// f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 map.
#pragma once
#include "la_common.h"

typedef double fd_f64x4 __attribute__((ext_vector_type(4)));

#define FD_T 64              // tile of C per workgroup
#define FD_KC 32             // k per LDS chunk
#define FD_LD (FD_KC + 1)    // doubles per LDS row: the 16 rows of a fragment read land on distinct banks

__device__ __forceinline__ void fd_tile_zero(fd_f64x4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
}

// Staging k chunk [k0, k0 + FD_KC) of tile rows i0 .. i0 + 63 of p and j0 .. j0 + 63 of q.  Loader roles: 32 threads per tile row
// (one k each: lk = tid & 31), tile rows lr + 8 pass (lr = tid >> 5).  A row past the end of its matrix is clamped into it (nothing
// is read out of bounds; the caller masks it).  CENTRE: the column means mup / muq are subtracted in float64; without it they are
// not read.  Two steps, so that a kernel can have the next chunk's loads in flight while it multiplies the current one:
// fd_tile_fetch (global memory -> registers) and fd_tile_store (registers -> LDS, widened and centred).
struct FdFetch {
    float p[FD_T / 8], q[FD_T / 8];
};

__device__ __forceinline__ void fd_tile_fetch(FdFetch& f, const float* __restrict__ p, long np, long i0, const float* __restrict__ q,
                                              long nq, long j0, int D, int k0, int lk, int lr) {
    const int k = k0 + lk;
    const bool in = k < D;
#pragma unroll
    for (int pass = 0; pass < FD_T / 8; ++pass) {
        const int r = lr + 8 * pass;
        const long gi = i0 + r < np ? i0 + r : np - 1;
        const long gj = j0 + r < nq ? j0 + r : nq - 1;
        f.p[pass] = in ? p[gi * D + k] : 0.f;
        f.q[pass] = in ? q[gj * D + k] : 0.f;
    }
}

template <bool CENTRE>
__device__ __forceinline__ void fd_tile_store(double (*Ps)[FD_LD], double (*Qs)[FD_LD], const FdFetch& f, const double* __restrict__ mup,
                                              const double* __restrict__ muq, int D, int k0, int lk, int lr) {
    const int k = k0 + lk;
    const bool in = k < D;
    const double mp = CENTRE && in ? mup[k] : 0.0, mq = CENTRE && in ? muq[k] : 0.0;
#pragma unroll
    for (int pass = 0; pass < FD_T / 8; ++pass) {
        const int r = lr + 8 * pass;
        if (CENTRE) {
            Ps[r][lk] = in ? (double)f.p[pass] - mp : 0.0;
            Qs[r][lk] = in ? (double)f.q[pass] - mq : 0.0;
        } else {
            Ps[r][lk] = (double)f.p[pass];          // (0 past D already)
            Qs[r][lk] = (double)f.q[pass];
        }
    }
}

// The k loop of a tile: acc += P[i0 .. i0 + 63] Q[j0 .. j0 + 63]^T over all of D, chunk k + 1 fetched while chunk k is multiplied.
// `mma(Ps, Qs)` multiplies one staged chunk (fd_tile_mma or fd_tile_mma_diag).  Every thread of the workgroup must reach it; LDS is
// free again on return.
template <bool CENTRE, class Mma>
__device__ __forceinline__ void fd_tile_loop(double (*Ps)[FD_LD], double (*Qs)[FD_LD], const float* __restrict__ p, long np,
                                             const double* __restrict__ mup, long i0, const float* __restrict__ q, long nq,
                                             const double* __restrict__ muq, long j0, int D, int lk, int lr, Mma mma) {
    FdFetch f;
    fd_tile_fetch(f, p, np, i0, q, nq, j0, D, 0, lk, lr);
    for (int k0 = 0; k0 < D; k0 += FD_KC) {
        fd_tile_store<CENTRE>(Ps, Qs, f, mup, muq, D, k0, lk, lr);
        __syncthreads();
        if (k0 + FD_KC < D) fd_tile_fetch(f, p, np, i0, q, nq, j0, D, k0 + FD_KC, lk, lr);
        mma(Ps, Qs);
        __syncthreads();
    }
}

// A thread's place in the tile product: wave (wm, wn) of the 2 x 2 waves, lane & 15 and lane >> 4 of the f64 MFMA layout
struct FdLane {
    int wm, wn, l15, l4;
};
__device__ __forceinline__ FdLane fd_tile_lane() {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    return FdLane{wid >> 1, wid & 1, lane & 15, lane >> 4};
}
// tile row and column of accumulator element acc[i][j][r]
__device__ __forceinline__ int fd_tile_row(const FdLane& t, int i, int r) { return t.wm * 32 + i * 16 + t.l4 + 4 * r; }
__device__ __forceinline__ int fd_tile_col(const FdLane& t, int j) { return t.wn * 32 + j * 16 + t.l15; }

// The diagonal of a tile whose two sides are the same 64 rows (staged once: Ps == Qs): wave w forms the 16 x 16 block (w, w) alone.
// Element (i, i) goes through the chain of MFMA steps that fd_tile_mma runs for a pair of equal rows, so a squared norm formed
// here has the bits of that pair's dot product.  The lanes with l4 == (l15 & 3) hold it: fd_tile_diag().
__device__ __forceinline__ void fd_tile_mma_diag(const double (*Ps)[FD_LD], fd_f64x4& acc, const FdLane& t) {
    const int w = t.wm * 2 + t.wn;
#pragma unroll
    for (int ks = 0; ks < FD_KC / 4; ++ks) {
        const double a = Ps[w * 16 + t.l15][ks * 4 + t.l4];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
    }
}
// element (row, row) of wave w's diagonal block, row = w * 16 + l15, in the lanes with l4 == (l15 & 3) (the others: any element)
__device__ __forceinline__ double fd_tile_diag(const fd_f64x4& acc, const FdLane& t) {
    const int r = t.l15 >> 2;
    return r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
}

// acc += the staged chunk's product: wave (wm, wn) owns rows wm * 32 .. + 31 and columns wn * 32 .. + 31 of the tile
__device__ __forceinline__ void fd_tile_mma(const double (*Ps)[FD_LD], const double (*Qs)[FD_LD], fd_f64x4 (&acc)[2][2], const FdLane& t) {
    const int wm = t.wm, wn = t.wn, l15 = t.l15, l4 = t.l4;
#pragma unroll
    for (int ks = 0; ks < FD_KC / 4; ++ks) {
        const int kk = ks * 4 + l4;
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Ps[wm * 32 + i * 16 + l15][kk];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Qs[wn * 32 + j * 16 + l15][kk];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

