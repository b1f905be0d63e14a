// Segmented key sort (gfx950 only): `ncols` independent columns of M float32 keys each, ascending, in place, keys only.  The contract
// is at the prototypes (include/latentaug_hip.h) and the measurements are in DESIGN.md 'Sliced Wasserstein distance'.
//
// A key is sorted as the unsigned image of its bit pattern (sign bit set: all bits flipped, else the sign bit flipped), which orders
// like the float: -inf < .. < -0.0 < +0.0 < .. < +inf.  The image 0xFFFFFFFF belongs to a NaN pattern, so it is free to pad with.
//   tile kernel    one 256-thread workgroup sorts SORT_TILE keys in LDS with a bitonic network (the last tile of a column padded with
//                  0xFFFFFFFF) and writes the images of its real keys
//   merge kernel   one pass merges runs of L keys into runs of 2 L.  A workgroup produces one SORT_TILE-key output tile: two threads
//                  find the ends of its segment on the merge path in global memory, the (at most SORT_TILE) input keys are staged in
//                  LDS, every thread finds its own diagonal there and merges SORT_KPT keys serially; the tile leaves through the same LDS
//                  so that the stores are contiguous.  The last pass writes floats again.
// The passes alternate between `keys` and the scratch (one image of the columns); the tile kernel starts on the side that makes the
// last pass end in `keys`.  Keys only: the sorted column is a unique bit pattern, whatever the network or the merge order.
#include "la_common.h"

#define SORT_TILE 4096
#define SORT_KPT (SORT_TILE / 256)
#define SORT_PAD 0xFFFFFFFFu

__device__ __forceinline__ unsigned sort_image(unsigned u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned sort_bits(unsigned v) { return v ^ ((v >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// src: floats (column stride src_ld); dst: images, or floats again when `unmap` (M <= SORT_TILE: the tile is the column)
__global__ __launch_bounds__(256) void la_sort_tile_kernel(const unsigned* __restrict__ src, long src_ld, unsigned* __restrict__ dst, long dst_ld,
                                                          long M, int unmap) {
    __shared__ unsigned s[SORT_TILE];
    const long t0 = (long)blockIdx.x * SORT_TILE;
    const long left = M - t0;
    const int cnt = left < SORT_TILE ? (int)left : SORT_TILE;
    const unsigned* in = src + (long)blockIdx.y * src_ld + t0;
    for (int i = threadIdx.x; i < SORT_TILE; i += 256) s[i] = i < cnt ? sort_image(in[i]) : SORT_PAD;
    __syncthreads();
    for (int k = 2; k <= SORT_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int r = 0; r < SORT_TILE / 512; ++r) {
                const int p = (int)threadIdx.x + 256 * r;
                const int i = 2 * p - (p & (j - 1)), l = i | j;          // (a zero bit put in at j's position, and its partner)
                const unsigned a = s[i], b = s[l];
                if ((a > b) == ((i & k) == 0)) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
    unsigned* out = dst + (long)blockIdx.y * dst_ld + t0;
    for (int i = threadIdx.x; i < cnt; i += 256) out[i] = unmap ? sort_bits(s[i]) : s[i];
}

// how many of the first d merged keys come from a (ties: a first); d <= na + nb
template <class P> __device__ __forceinline__ int sort_merge_path(P a, int na, P b, int nb, int d) {
    int lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// runs of L keys (the last of a column shorter, possibly unpaired) -> runs of 2 L; grid (tiles of the column, columns)
__global__ __launch_bounds__(256) void la_sort_merge_kernel(const unsigned* __restrict__ src, long src_ld, unsigned* __restrict__ dst, long dst_ld,
                                                           long M, long L, int unmap) {
    __shared__ unsigned sin[SORT_TILE];
    __shared__ int cut[2];
    const long o0 = (long)blockIdx.x * SORT_TILE;              // first output position of this tile
    const long pair0 = o0 / (2 * L) * (2 * L);                  // (L is a multiple of SORT_TILE: a tile lies inside one pair)
    const long a_end = pair0 + L < M ? pair0 + L : M, b_end = pair0 + 2 * L < M ? pair0 + 2 * L : M;
    const int na = (int)(a_end - pair0), nb = (int)(b_end - a_end);      // L <= 2^30
    const unsigned* a = src + (long)blockIdx.y * src_ld + pair0;
    const unsigned* b = a + na;
    const int d0 = (int)(o0 - pair0);
    const int d1 = d0 + SORT_TILE < na + nb ? d0 + SORT_TILE : na + nb;
    if (threadIdx.x < 2) cut[threadIdx.x] = sort_merge_path(a, na, b, nb, threadIdx.x == 0 ? d0 : d1);
    __syncthreads();
    const int a0 = cut[0], a1 = cut[1], b0 = d0 - a0, b1 = d1 - a1;
    const int ca = a1 - a0, cb = b1 - b0, n = ca + cb;             // n = d1 - d0 <= SORT_TILE
    for (int i = threadIdx.x; i < n; i += 256) sin[i] = i < ca ? a[a0 + i] : b[b0 + (i - ca)];
    __syncthreads();
    const unsigned* sa = sin;
    const unsigned* sb = sin + ca;
    const int d = (int)threadIdx.x * SORT_KPT < n ? (int)threadIdx.x * SORT_KPT : n;
    int ia = sort_merge_path(sa, ca, sb, cb, d), ib = d - ia;
    unsigned reg[SORT_KPT];
#pragma unroll
    for (int r = 0; r < SORT_KPT; ++r) {
        const bool live = d + r < n;
        const bool take_a = live && (ib >= cb || (ia < ca && sa[ia] <= sb[ib]));
        const bool take_b = live && !take_a;
        reg[r] = take_a ? sa[ia] : (take_b ? sb[ib] : SORT_PAD);
        ia += take_a ? 1 : 0;
        ib += take_b ? 1 : 0;
    }
    __syncthreads();          // every thread has read its inputs: the tile takes their place
#pragma unroll
    for (int r = 0; r < SORT_KPT; ++r)
        if (d + r < n) sin[d + r] = reg[r];
    __syncthreads();
    unsigned* out = dst + (long)blockIdx.y * dst_ld + o0;
    for (int i = threadIdx.x; i < n; i += 256) out[i] = unmap ? sort_bits(sin[i]) : sin[i];
}

// ------------------------------------------------------------------------------------------------------------ host side
static inline bool sort_sizes_ok(long ncols, long M) { return ncols >= 1 && ncols <= 65535 && M >= 1 && M <= 0x40000000L; }

extern "C" int la_sort_tile_keys(void) { return SORT_TILE; }

extern "C" size_t la_sort_columns_scratch_bytes(long ncols, long M) {
    if (!sort_sizes_ok(ncols, M)) return 0;
    return la_align64((size_t)ncols * (size_t)M * sizeof(unsigned));
}

extern "C" int la_sort_columns_f32(float* keys, long ncols, long M, long ld, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    LA_CHECK_ARG(keys && scratch, "sort_columns: null pointer");
    LA_CHECK_ARG(sort_sizes_ok(ncols, M), "sort_columns: ncols must lie in 1 .. 65535 and M in 1 .. 2^30");
    LA_CHECK_ARG(ld >= M, "sort_columns: the column stride ld must be at least M");
    LA_CHECK_ARG(la_aligned<4>(keys, scratch), "sort_columns: keys and scratch must be 4-byte aligned");
    LA_CHECK_WORKSPACE(scratch_bytes, la_sort_columns_scratch_bytes(ncols, M), "sort_columns: scratch smaller than la_sort_columns_scratch_bytes(ncols, M)");
    const long tiles = (M + SORT_TILE - 1) / SORT_TILE;
    int passes = 0;
    for (long runs = tiles; runs > 1; runs = (runs + 1) / 2) ++passes;
    unsigned* buf[2] = {(unsigned*)keys, (unsigned*)scratch};
    const long stride[2] = {ld, M};
    const dim3 grid((unsigned)tiles, (unsigned)ncols), block(256);
    int side = passes & 1;          // where the tiles go: an even number of passes from there ends in keys
    hipLaunchKernelGGL(la_sort_tile_kernel, grid, block, 0, stream, (const unsigned*)keys, ld, buf[side], stride[side], M, passes == 0 ? 1 : 0);
    long L = SORT_TILE;
    for (int p = 0; p < passes; ++p, L *= 2, side ^= 1)
        hipLaunchKernelGGL(la_sort_merge_kernel, grid, block, 0, stream, (const unsigned*)buf[side], stride[side], buf[side ^ 1], stride[side ^ 1],
                           M, L, p == passes - 1 ? 1 : 0);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
