// Gram-matrix style distance and content distance of activation pairs: NSTLoss of augments/criteria/nst/nst.py:7-35 on the taps of
// VGG19Net (networks.py:60-70), per pair and tap
//       G = F F^T / HW  with F [C][HW];   style = mean over the C^2 entries of (G1 - G2)^2;   content = mean over C HW of (f1 - f2)^2.
// Rows p and p + P of f [2P][C][HW] are a pair.  With D = f1 - f2 and S = f1 + f2, both formed in float32 while loading,
//       E = D S^T + S D^T = 2 HW (G1 - G2),     style = sum_ij E_ij^2 / (4 HW^2 C^2),     content = sum D^2 / (C HW).
// The images of a pair are close and the expanded G1 - G2 cancels (the reason la_tap_pair_dist_kernel takes differences); in this
// form d(x, x) is exactly 0 (D = 0), and d(x, y) = d(y, x) bit for bit: D changes sign, S does not, and an fma chain of negated
// products is the negated chain.
// la_gram_diff_kernel<T>: one workgroup per (K slice, T x T tile with I <= J, pair); E is symmetric, an off-diagonal tile counts
// twice in the finish.  Arithmetic: the exact fp32 MFMA through the tile loop of la_f32_tile.h, 4 waves (2 x 2) of T/2 x T/2; per
// chunk of 16 k two chains go into the one accumulator, D_I S_J^T then S_I D_J^T.  T = 128 (2 x 2 MFMA tiles per wave); T = 64 for
// C <= 64 (one MFMA tile per wave: with T = 128 three of the four waves would have nothing to multiply).  K = HW is contiguous in
// memory: 4 threads load 16 consecutive k of a row of both images (la_kid_tile_kernel's loader roles) and stage D and S transposed
// into [k][c + 4] LDS tiles.  A diagonal tile loads its rows once and stages them on both sides.  A wave whose block lies wholly
// beyond C loads and meets the barriers but issues no MFMA.
// Split-K: the number of slices is a function of (C, HW) only (gram_plan), never of P, so a pair alone gives the bits it gives in
// any batch.  Partials are float32 [pair][slice][tile][tw^2], tw = min(C, T); the finish adds them in slice order (la_slices_sum),
// squares in float64 and reduces in a fixed order, a tile's entries in nseg segments of one workgroup each (nseg from (C, HW) too).
// No float atomics: two runs give the same bits.
#include "la_gram.h"

#include "la_f32_tile.h"

#define GRAM_T 128
#define GRAM_TS 64         // tile edge for C <= GRAM_TS
#define GRAM_KC 16
#define GRAM_PER 32        // chunks of a K slice aimed at (512 k): a slice's partial tile is small beside what it reads
#define GRAM_WGS 128       // workgroups per pair aimed at
#define GRAM_CBLK 128      // most workgroups per pair of the content sum
#define GRAM_CELEMS 4096   // elements per workgroup of the content sum aimed at
#define GRAM_FLOADS 8192   // partial loads per workgroup of the finish aimed at (32 per thread), at least 256 entries each

struct GramPlan {
    int edge, T, ntile, tw;    // tile edge (GRAM_T | GRAM_TS), tiles per side, tiles with I <= J, edge of a stored tile
    int nseg;                  // workgroups of the finish per tile
    int nchunk, per, ks;       // chunks of GRAM_KC k, chunks per slice, slices
    int cblk;                  // workgroups per pair of the content sum
    long cper;                 // elements of each
};

// 0: refused.  Everything here depends on (C, HW) alone.
static bool gram_plan(int C, int HW, GramPlan& g) {
    if (C < 1 || HW < 1 || C > 8192 || HW > (1 << 26)) return false;
    g.edge = C <= GRAM_TS ? GRAM_TS : GRAM_T;
    g.T = (C + g.edge - 1) / g.edge;
    g.ntile = g.T * (g.T + 1) / 2;
    g.tw = C < g.edge ? C : g.edge;
    g.nchunk = (HW + GRAM_KC - 1) / GRAM_KC;
    int want = (g.nchunk + GRAM_PER - 1) / GRAM_PER;
    const int cap = GRAM_WGS / g.ntile > 1 ? GRAM_WGS / g.ntile : 1;
    if (want > cap) want = cap;
    g.per = (g.nchunk + want - 1) / want;
    g.ks = (g.nchunk + g.per - 1) / g.per;      // (every slice holds at least one chunk; the last one may be shorter)
    const long loads = (long)g.ks * g.tw * g.tw;
    const int by_entries = (g.tw * g.tw + 255) / 256, by_loads = (int)(loads / GRAM_FLOADS > 1 ? loads / GRAM_FLOADS : 1);
    g.nseg = by_entries < by_loads ? by_entries : by_loads;
    const long n = (long)C * HW;
    long cb = (n + GRAM_CELEMS - 1) / GRAM_CELEMS;
    if (cb > GRAM_CBLK) cb = GRAM_CBLK;
    g.cblk = (int)cb;
    g.cper = (n + cb - 1) / cb;
    return true;
}

struct GramArgs {
    const float* f;
    float* part;      // [P][ks][ntile][tw * tw]
    int P, C, HW, vec; // vec: rows are 16-byte aligned (HW % 4 == 0 and an aligned base): float4 loads
    GramPlan g;
};

// tile t of the upper triangle, rows first: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void gram_tile(int t, int T, int* ti, int* tj) {
    int i = 0;
    while (t >= T - i) { t -= T - i; ++i; }
    *ti = i; *tj = i + t;
}

template <int T>
__global__ __launch_bounds__(256) void la_gram_diff_kernel(GramArgs a) {
    constexpr int LD = T + 4, NP = T / 64, WT = T / 64;      // LDS row, loader passes of 64 rows, MFMA tiles per wave and side
    __shared__ __attribute__((aligned(16))) float Da[2][GRAM_KC][LD];
    __shared__ __attribute__((aligned(16))) float Sa[2][GRAM_KC][LD];
    __shared__ __attribute__((aligned(16))) float Db[2][GRAM_KC][LD];
    __shared__ __attribute__((aligned(16))) float Sb[2][GRAM_KC][LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int C = a.C, HW = a.HW;

    const int slice = blockIdx.x / (unsigned)a.g.ntile;
    const int t = blockIdx.x - slice * a.g.ntile;
    int ti, tj;
    gram_tile(t, a.g.T, &ti, &tj);
    const int i0 = ti * T, j0 = tj * T;
    const bool diag = ti == tj;      // (workgroup-uniform)
    const long p = blockIdx.y;
    const float* fx = a.f + p * C * HW;
    const float* fy = a.f + (p + a.P) * C * HW;

    // loader roles: 4 threads per row (4 consecutive k each), rows tid / 4 (+ 64) of both sides.  Rows past C and k past HW load
    // zeros: nothing is read outside the two images.
    const int kq = (tid & 3) * 4, lr = tid >> 2;
    long offa[NP], offb[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int ra = i0 + lr + 64 * j, rb = j0 + lr + 64 * j;
        offa[j] = ra < C ? (long)ra * HW : -1;
        offb[j] = rb < C ? (long)rb * HW : -1;
    }
    float4 ax[NP], ay[NP], bx[NP], by[NP];
    auto fetch = [&](const float* base, long off, int k) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (off >= 0 && k < HW) {
            const float* q = base + off + k;
            if (a.vec) {
                v = *reinterpret_cast<const float4*>(q);      // HW % 4 == 0: k + 3 < HW
            } else {
                v.x = q[0];
                if (k + 1 < HW) v.y = q[1];
                if (k + 2 < HW) v.z = q[2];
                if (k + 3 < HW) v.w = q[3];
            }
        }
        return v;
    };
    auto prefetch = [&](int ci) {
        const int k = ci * GRAM_KC + kq;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            ax[j] = fetch(fx, offa[j], k); ay[j] = fetch(fy, offa[j], k);
            if (diag) { bx[j] = ax[j]; by[j] = ay[j]; }      // (the same rows: no second load)
            else { bx[j] = fetch(fx, offb[j], k); by[j] = fetch(fy, offb[j], k); }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int r = lr + 64 * j;
            Da[buf][kq][r] = ax[j].x - ay[j].x; Da[buf][kq + 1][r] = ax[j].y - ay[j].y;
            Da[buf][kq + 2][r] = ax[j].z - ay[j].z; Da[buf][kq + 3][r] = ax[j].w - ay[j].w;
            Sa[buf][kq][r] = ax[j].x + ay[j].x; Sa[buf][kq + 1][r] = ax[j].y + ay[j].y;
            Sa[buf][kq + 2][r] = ax[j].z + ay[j].z; Sa[buf][kq + 3][r] = ax[j].w + ay[j].w;
            Db[buf][kq][r] = bx[j].x - by[j].x; Db[buf][kq + 1][r] = bx[j].y - by[j].y;
            Db[buf][kq + 2][r] = bx[j].z - by[j].z; Db[buf][kq + 3][r] = bx[j].w - by[j].w;
            Sb[buf][kq][r] = bx[j].x + by[j].x; Sb[buf][kq + 1][r] = bx[j].y + by[j].y;
            Sb[buf][kq + 2][r] = bx[j].z + by[j].z; Sb[buf][kq + 3][r] = bx[j].w + by[j].w;
        }
    };

    la_f32x16 acc[WT][WT];
    la_f32_tile_zero(acc);
    const int a0 = wm * (T / 2), b0 = wn * (T / 2);
    const bool active = i0 + a0 < C && j0 + b0 < C;      // (wave-uniform)

    int c_beg, c_end;
    la_slice_range(slice, a.g.per, a.g.nchunk, &c_beg, &c_end);
    la_tile_pipeline(c_beg, c_end, prefetch, stage, [&](int buf, int) {
        if (active) {
            la_f32_tile_mma<GRAM_KC>(Da, Sb, buf, a0, b0, l31, lh, acc);
            la_f32_tile_mma<GRAM_KC>(Sa, Db, buf, a0, b0, l31, lh, acc);
        }
    });
    if (!active) return;

    const int tw = a.g.tw;
    float* dst = a.part + ((p * a.g.ks + slice) * a.g.ntile + t) * (long)(tw * tw);
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const int nl = b0 + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = a0 + i * 32 + la_mfma32_row(r, lh);
                if (i0 + ml < C && j0 + nl < C) dst[ml * tw + nl] = acc[i][j][r];
            }
        }
}

// tsum[p][t][seg] = sum over segment seg of the tile's entries of E^2 (float64; E = the slices in order), twice that for an
// off-diagonal tile
__global__ __launch_bounds__(256) void la_gram_finish_kernel(const float* __restrict__ part, double* __restrict__ tsum, int C, GramPlan g) {
    __shared__ double red[256];
    const int t = blockIdx.x / (unsigned)g.nseg, seg = blockIdx.x - t * g.nseg;
    const long p = blockIdx.y;
    int ti, tj;
    gram_tile(t, g.T, &ti, &tj);
    const int rows = C - ti * g.edge < g.edge ? C - ti * g.edge : g.edge, cols = C - tj * g.edge < g.edge ? C - tj * g.edge : g.edge;
    const long tw2 = (long)g.tw * g.tw, stride = (long)g.ntile * tw2;
    const float* src = part + p * g.ks * stride + t * tw2;
    const int per = (rows * cols + g.nseg - 1) / g.nseg, e_end = (seg + 1) * per < rows * cols ? (seg + 1) * per : rows * cols;
    double acc = 0.0;
    for (int e = seg * per + threadIdx.x; e < e_end; e += 256) {
        const int m = e / cols, n = e - m * cols;
        const double v = (double)la_slices_sum(src, (long)m * g.tw + n, stride, g.ks);
        acc += v * v;
    }
    const double s = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) tsum[(p * g.ntile + t) * g.nseg + seg] = ti != tj ? 2.0 * s : s;
}

// csum[p][b] = sum of (f1 - f2)^2 over block b's elements: the difference in float32, its square (exact) and the sum in float64
__global__ __launch_bounds__(256) void la_gram_content_kernel(const float* __restrict__ f, double* __restrict__ csum, int P, long n, GramPlan g) {
    __shared__ double red[256];
    const long p = blockIdx.y;
    const float* fx = f + p * n;
    const float* fy = f + (p + P) * n;
    const long beg = blockIdx.x * g.cper, end = beg + g.cper < n ? beg + g.cper : n;
    double acc = 0.0;
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        const double d = (double)(fx[i] - fy[i]);
        acc += d * d;
    }
    const double s = la_block_tree_sum_256(acc, red);
    if (threadIdx.x == 0) csum[p * g.cblk + blockIdx.x] = s;
}

// style[p] = (tile segments in order) / (4 HW^2 C^2), content[p] = (blocks in order) / (C HW): one division each
__global__ __launch_bounds__(64) void la_gram_combine_kernel(const double* __restrict__ tsum, const double* __restrict__ csum, double* __restrict__ style,
                                                            double* __restrict__ content, int P, long ostride, double style_den, double content_den,
                                                            GramPlan g) {
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    const int nt = g.ntile * g.nseg;
    for (int t = 0; t < nt; ++t) s += tsum[p * nt + t];
    style[p * ostride] = s / style_den;
    if (content) {
        double c = 0.0;
        for (int b = 0; b < g.cblk; ++b) c += csum[p * g.cblk + b];
        content[p * ostride] = c / content_den;
    }
}

// scratch: the float32 slice partials, then the float64 tile sums and content partials
struct GramScratch { float* part; double *tsum, *csum; size_t bytes; };
static GramScratch gram_scratch(void* base, int P, const GramPlan& g) {
    LaCarver c{(char*)base};
    GramScratch s;
    s.part = c.take<float>((size_t)P * g.ks * g.ntile * g.tw * g.tw);
    s.tsum = c.take<double>((size_t)P * g.ntile * g.nseg);
    s.csum = c.take<double>((size_t)P * g.cblk);
    s.bytes = c.off;
    return s;
}

extern "C" int la_gram_pair_slices(int C, int HW) {
    GramPlan g;
    return gram_plan(C, HW, g) ? g.ks : 0;
}

extern "C" size_t la_gram_pair_scratch_bytes(int P, int C, int HW) {
    GramPlan g;
    if (P < 1 || P > 65535 || !gram_plan(C, HW, g)) return 0;
    return gram_scratch(nullptr, P, g).bytes;
}

int la_gram_pair_launch(const float* f, int P, int C, int HW, double* style, double* content, long ostride, void* scratch, hipStream_t stream) {
    GramArgs a;
    if (!gram_plan(C, HW, a.g)) { la_set_error("gram_pair: shape refused"); return LA_ERR_ARG; }
    const GramScratch s = gram_scratch(scratch, P, a.g);
    a.f = f; a.part = s.part; a.P = P; a.C = C; a.HW = HW;
    a.vec = (HW % 4 == 0 && ((size_t)f & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(a.g.edge == GRAM_TS ? la_gram_diff_kernel<GRAM_TS> : la_gram_diff_kernel<GRAM_T>, dim3((unsigned)(a.g.ks * a.g.ntile), P),
                       dim3(256), 0, stream, a);
    hipLaunchKernelGGL(la_gram_finish_kernel, dim3(a.g.ntile * a.g.nseg, P), dim3(256), 0, stream, (const float*)s.part, s.tsum, C, a.g);
    if (content) hipLaunchKernelGGL(la_gram_content_kernel, dim3(a.g.cblk, P), dim3(256), 0, stream, f, s.csum, P, (long)C * HW, a.g);
    hipLaunchKernelGGL(la_gram_combine_kernel, dim3(la_cdiv(P, 64)), dim3(64), 0, stream, (const double*)s.tsum, (const double*)s.csum, style, content,
                       P, ostride, 4.0 * (double)HW * (double)HW * (double)C * (double)C, (double)C * (double)HW, a.g);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_gram_pair_dist_f32(const float* f, int P, int C, int HW, double* style, double* content, void* scratch, size_t scratch_bytes,
                                     hipStream_t stream) {
    LA_CHECK_ARG(f && style && scratch, "gram_pair_dist: null pointer");
    const size_t need = la_gram_pair_scratch_bytes(P, C, HW);
    LA_CHECK_ARG(need > 0, "gram_pair_dist: P must lie in 1 .. 65535, C in 1 .. 8192, HW in 1 .. 2^26");
    LA_CHECK_WORKSPACE(scratch_bytes, need, "gram_pair_dist: scratch smaller than la_gram_pair_scratch_bytes(P, C, HW)");
    LA_CHECK_ARG(la_aligned<8>(scratch), "gram_pair_dist: the scratch must be 8-byte aligned");
    return la_gram_pair_launch(f, P, C, HW, style, content, 1, scratch, stream);
}
