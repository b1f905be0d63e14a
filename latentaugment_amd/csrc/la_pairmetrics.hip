// Paired image metrics (no reference counterpart): what describes a PAIR of images rather than two sets.
//   la_pair_metrics_f32       per plane of a pair: sum d^2 and sum |d| (float64), SSIM and contrast-structure means per pyramid level,
//                             MS-SSIM (Wang, Simoncelli, Bovik 2003).  One fused launch per level + a finish launch + a combine launch.
//   la_joint_hist_f32         joint histogram of two planes (uint32 counts): the input of mutual information.
// Everything is reproducible: float partials are added in a fixed order, the only atomics are integer ones.
#include "la_common.h"

#define PM_T 32            // a workgroup owns a PM_T x PM_T block of a plane
#define PM_MAXWIN 11
#define PM_MAXLEV 5
#define PM_HLD (PM_T + 1)  // leading dimension of the row-pass maps: 33, so rows r and r + 1 start one bank apart

struct PmLevelArgs {
    const float* x;        // level 0: the caller's images, gathered through ix / iy; deeper levels: the pyramid, plane-contiguous
    const float* y;
    const int* ix;         // null: pair p reads image p
    const int* iy;
    float* nx;             // next level's images [planes][h/2][w/2] (null on the last level)
    float* ny;
    double* part;          // [planes][tiles][2]: sum of ssim, sum of cs over the outputs whose window origin lies in the tile
    double* epart;         // level 0: [planes][tiles][2]: sum d^2, sum |d| over the tile's pixels
    long planes;
    int C, h, w;
    int ntx, tiles;
    int oh, ow;            // valid extent: h - win + 1, w - win + 1
    float c1, c2;
    float g[PM_MAXWIN];
};

// four double sums over the 256 threads of the workgroup, fixed tree; the results are in red[q * 256]
__device__ __forceinline__ void pm_block_sum4(double v0, double v1, double v2, double v3, double* red) {
    const int t = threadIdx.x;
    red[t] = v0; red[256 + t] = v1; red[512 + t] = v2; red[768 + t] = v3;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[t] += red[t + o]; red[256 + t] += red[256 + t + o];
            red[512 + t] += red[512 + t + o]; red[768 + t] += red[768 + t + o];
        }
        __syncthreads();
    }
}

// One pyramid level.  grid (tiles, min(planes, 65535)); the planes beyond the grid go through the loop.
// LDS at WIN = 11: two staged images 2 x 42 x 43 floats (14.4 KB), five row-pass maps 5 x 42 x 33 floats (27.7 KB), 8 KB of sums.
template <int WIN, bool L0>
__global__ __launch_bounds__(256) void la_pm_level_kernel(PmLevelArgs a) {
    // every float32 product and sum below is rounded on its own, in the order written (taps ascending): the maps are those of the plain
    // separable definition evaluated in float32, bit for bit, which is what the tests' error budget is derived from
#pragma clang fp contract(off)
    constexpr int TS = PM_T + WIN - 1;          // staged rows / columns: the block plus the halo to the right and below
    constexpr int SLD = TS | 1;                 // odd leading dimension
    __shared__ float sx[TS * SLD];
    __shared__ float sy[TS * SLD];
    __shared__ float hm[5][TS * PM_HLD];
    __shared__ double red[4 * 256];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / a.ntx, tx = (int)blockIdx.x - ty * a.ntx;
    const int y0 = ty * PM_T, x0 = tx * PM_T;
    const long hw = (long)a.h * a.w;
    for (long pl = blockIdx.y; pl < a.planes; pl += gridDim.y) {
        const float *px, *py;
        if (L0) {
            const long p = pl / a.C;
            const int c = (int)(pl - p * a.C);
            px = a.x + ((a.ix ? (long)a.ix[p] : p) * a.C + c) * hw;
            py = a.y + ((a.iy ? (long)a.iy[p] : p) * a.C + c) * hw;
        } else {
            px = a.x + pl * hw;
            py = a.y + pl * hw;
        }
        // stage: pixels outside the image are 0; they only reach outputs outside the valid extent, which are not evaluated
        for (int i = tid; i < TS * TS; i += 256) {
            const int r = i / TS, c = i - r * TS;
            const int gy = y0 + r, gx = x0 + c;
            const bool in = gy < a.h && gx < a.w;
            const int off = in ? gy * a.w + gx : 0;
            const float vx = px[off], vy = py[off];
            sx[r * SLD + c] = in ? vx : 0.f;
            sy[r * SLD + c] = in ? vy : 0.f;
        }
        __syncthreads();
        // row pass: the five moment maps, TS rows x 32 columns
        for (int i = tid; i < TS * PM_T; i += 256) {
            const int r = i >> 5, c = i & 31;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float u = sx[r * SLD + c + k], v = sy[r * SLD + c + k];
                const float uu = u * u, vv = v * v, uv = u * v;
                m0 += a.g[k] * u;
                m1 += a.g[k] * v;
                m2 += a.g[k] * uu;
                m3 += a.g[k] * vv;
                m4 += a.g[k] * uv;
            }
            hm[0][r * PM_HLD + c] = m0; hm[1][r * PM_HLD + c] = m1; hm[2][r * PM_HLD + c] = m2;
            hm[3][r * PM_HLD + c] = m3; hm[4][r * PM_HLD + c] = m4;
        }
        // the block's 2 x 2 means are the next level's images (the staged block starts at row 0, column 0)
        if (a.nx) {
            const int qy = tid >> 4, qx = tid & 15;
            const int oy = (y0 >> 1) + qy, ox = (x0 >> 1) + qx;
            const int h2 = a.h >> 1, w2 = a.w >> 1;
            if (oy < h2 && ox < w2) {
                const float* s0 = sx + (2 * qy) * SLD + 2 * qx;
                const float* s1 = sy + (2 * qy) * SLD + 2 * qx;
                const long o = (pl * h2 + oy) * w2 + ox;
                a.nx[o] = ((s0[0] + s0[1]) + (s0[SLD] + s0[SLD + 1])) * 0.25f;
                a.ny[o] = ((s1[0] + s1[1]) + (s1[SLD] + s1[SLD + 1])) * 0.25f;
            }
        }
        __syncthreads();
        // column pass from LDS and the two quotients: thread (lx, ly0) owns outputs (ly0 + 8 j, lx)
        const int lx = tid & 31, ly0 = tid >> 5;
        double ss = 0.0, sc = 0.0, e2 = 0.0, e1 = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ly0 + 8 * j;
            if (L0) {
                const float d = sx[ly * SLD + lx] - sy[ly * SLD + lx];          // 0 outside the image
                e2 += (double)d * (double)d;
                e1 += (double)fabsf(d);
            }
            if (y0 + ly < a.oh && x0 + lx < a.ow) {
                float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
                for (int k = 0; k < WIN; ++k) {
                    const int o = (ly + k) * PM_HLD + lx;
                    mx += a.g[k] * hm[0][o];
                    my += a.g[k] * hm[1][o];
                    exx += a.g[k] * hm[2][o];
                    eyy += a.g[k] * hm[3][o];
                    exy += a.g[k] * hm[4][o];
                }
                const float sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
                const float cs = (2.f * sxy + a.c2) / (sxx + syy + a.c2);
                const float lum = (2.f * mx * my + a.c1) / (mx * mx + my * my + a.c1);
                ss += (double)(lum * cs);
                sc += (double)cs;
            }
        }
        pm_block_sum4(ss, sc, e2, e1, red);
        if (tid == 0) {
            const long o = (pl * a.tiles + blockIdx.x) * 2;
            a.part[o] = red[0];
            a.part[o + 1] = red[256];
            if (L0) {
                a.epart[o] = red[512];
                a.epart[o + 1] = red[768];
            }
        }
        __syncthreads();          // the next plane restages
    }
}

struct PmFinishArgs {
    const double* part[PM_MAXLEV + 1];          // per level, then the error partials
    int tiles[PM_MAXLEV + 1];
    double count[PM_MAXLEV];
    long planes;
    int levels;
    double* means;        // [planes][levels][2]
    float* ssim;          // [planes][levels]
    float* cs;
    double* err;          // [planes][2]
};

// grid (levels + 1, min(planes, 65535)), one wave: the tile partials of a plane in tile order (lane-strided, then the shuffle tree)
__global__ __launch_bounds__(64) void la_pm_finish_kernel(PmFinishArgs a) {
    const int q = blockIdx.x;
    const int nt = a.tiles[q];
    for (long pl = blockIdx.y; pl < a.planes; pl += gridDim.y) {
        const double* p = a.part[q] + pl * nt * 2;
        double v0 = 0.0, v1 = 0.0;
        for (int t = threadIdx.x; t < nt; t += 64) { v0 += p[2 * t]; v1 += p[2 * t + 1]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_xor(v0, o, 64); v1 += __shfl_xor(v1, o, 64); }
        if (threadIdx.x == 0) {
            if (q < a.levels) {
                const double s = v0 / a.count[q], c = v1 / a.count[q];
                a.means[(pl * a.levels + q) * 2] = s;
                a.means[(pl * a.levels + q) * 2 + 1] = c;
                a.ssim[pl * a.levels + q] = (float)s;
                a.cs[pl * a.levels + q] = (float)c;
            } else {
                a.err[pl * 2] = v0;
                a.err[pl * 2 + 1] = v1;
            }
        }
    }
}

struct PmCombineArgs {
    const double* means;
    float* ms;
    long planes;
    int levels;
    double w[PM_MAXLEV];
};

// ms = prod_{l < levels - 1} max(cs_l, 0)^w_l * max(ssim_last, 0)^w_last from the float64 means; a negative factor is exactly 0
__global__ __launch_bounds__(256) void la_pm_combine_kernel(PmCombineArgs a) {
    for (long pl = (long)blockIdx.x * 256 + threadIdx.x; pl < a.planes; pl += (long)gridDim.x * 256) {
        double v = 1.0;
        for (int l = 0; l < a.levels; ++l) {
            const double f = a.means[(pl * a.levels + l) * 2 + (l == a.levels - 1 ? 0 : 1)];
            v *= f > 0.0 ? pow(f, a.w[l]) : (a.w[l] == 0.0 ? 1.0 : 0.0);
        }
        a.ms[pl] = (float)v;
    }
}

struct PmPlan {
    long planes;
    int h[PM_MAXLEV], w[PM_MAXLEV], ntx[PM_MAXLEV], tiles[PM_MAXLEV];
    double *part[PM_MAXLEV], *epart, *means;
    float *px[PM_MAXLEV], *py[PM_MAXLEV];          // pyramid images of levels 1 ..
};

// the shape rules of the launch (false: refused) and the workspace layout over `base` (null: measuring)
static bool pm_plan(PmPlan* pp, long P, int C, int H, int W, int win, int levels, char* base, size_t* bytes) {
    if (P < 1 || C < 1 || H < 1 || W < 1 || win < 1 || win > PM_MAXWIN || !(win & 1) || levels < 1 || levels > PM_MAXLEV) return false;
    const int m = 1 << (levels - 1);
    if (H % m || W % m || H / m < win || W / m < win) return false;
    if ((long)H * W > 0x7fffffffL || P > 0x7fffffffL / C) return false;
    if ((double)P * C * H * W > 1e13) return false;          // the pyramid stays far inside size_t
    LaCarver cv;
    cv.base = base;
    pp->planes = P * C;
    for (int l = 0; l < levels; ++l) {
        pp->h[l] = H >> l; pp->w[l] = W >> l;
        pp->ntx[l] = la_cdiv(pp->w[l], PM_T);
        pp->tiles[l] = pp->ntx[l] * la_cdiv(pp->h[l], PM_T);
        pp->part[l] = cv.take<double>((size_t)pp->planes * pp->tiles[l] * 2);          // 2 doubles per tile
    }
    pp->epart = cv.take<double>((size_t)pp->planes * pp->tiles[0] * 2);
    pp->means = cv.take<double>((size_t)pp->planes * levels * 2);
    pp->px[0] = pp->py[0] = nullptr;
    for (int l = 1; l < levels; ++l) {
        pp->px[l] = cv.take<float>((size_t)pp->planes * pp->h[l] * pp->w[l]);
        pp->py[l] = cv.take<float>((size_t)pp->planes * pp->h[l] * pp->w[l]);
    }
    *bytes = cv.off;
    return true;
}

extern "C" size_t la_pair_metrics_workspace_bytes(long P, int C, int H, int W, int win, int levels) {
    PmPlan pp;
    size_t bytes = 0;
    return pm_plan(&pp, P, C, H, W, win, levels, nullptr, &bytes) ? bytes : 0;
}

template <int WIN>
static void pm_launch_level(const PmLevelArgs& a, bool l0, dim3 grid, hipStream_t stream) {
    if (l0) hipLaunchKernelGGL((la_pm_level_kernel<WIN, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((la_pm_level_kernel<WIN, false>), grid, dim3(256), 0, stream, a);
}

extern "C" int la_pair_metrics_f32(const float* x, const float* y, const int* ix, const int* iy, long P, int C, int H, int W,
                                   const float* taps_host, int win, int levels, const float* weights_host, float c1, float c2,
                                   double* err, float* ssim, float* cs, float* ms, void* workspace, size_t workspace_bytes,
                                   hipStream_t stream) {
    LA_CHECK_ARG(x && y && taps_host && weights_host && err && ssim && cs && ms && workspace, "pair_metrics: null pointer");
    LA_CHECK_ARG(win >= 1 && win <= PM_MAXWIN && (win & 1), "pair_metrics: win must be odd and lie in 1 .. 11");
    LA_CHECK_ARG(levels >= 1 && levels <= PM_MAXLEV, "pair_metrics: levels must lie in 1 .. 5");
    LA_CHECK_ARG(P >= 1 && C >= 1 && H >= 1 && W >= 1, "pair_metrics: P, C, H and W must be positive");
    LA_CHECK_ARG(H % (1 << (levels - 1)) == 0 && W % (1 << (levels - 1)) == 0, "pair_metrics: H and W must be multiples of 2^(levels-1)");
    LA_CHECK_ARG((H >> (levels - 1)) >= win && (W >> (levels - 1)) >= win, "pair_metrics: the last level is smaller than the window");
    PmPlan pp;
    size_t need = 0;
    LA_CHECK_ARG(pm_plan(&pp, P, C, H, W, win, levels, nullptr, &need), "pair_metrics: sizes beyond the launch limits");
    LA_CHECK_WORKSPACE(workspace_bytes, need, "pair_metrics: workspace smaller than la_pair_metrics_workspace_bytes(P, C, H, W, win, levels)");
    LA_CHECK_ARG(la_aligned<8>(workspace), "pair_metrics: the workspace must be 8-byte aligned");
    LA_CHECK_ARG(la_aligned<4>(x, y), "pair_metrics: image pointers must be 4-byte aligned");
    for (int l = 0; l < levels; ++l) LA_CHECK_ARG(weights_host[l] >= 0.f, "pair_metrics: weights must be non-negative");
    pm_plan(&pp, P, C, H, W, win, levels, (char*)workspace, &need);

    const unsigned gy = (unsigned)(pp.planes < 65535 ? pp.planes : 65535);
    for (int l = 0; l < levels; ++l) {
        PmLevelArgs a;
        a.x = l ? pp.px[l] : x; a.y = l ? pp.py[l] : y;
        a.ix = ix; a.iy = iy;
        a.nx = l + 1 < levels ? pp.px[l + 1] : nullptr; a.ny = l + 1 < levels ? pp.py[l + 1] : nullptr;
        a.part = pp.part[l]; a.epart = pp.epart;
        a.planes = pp.planes; a.C = C; a.h = pp.h[l]; a.w = pp.w[l];
        a.ntx = pp.ntx[l]; a.tiles = pp.tiles[l];
        a.oh = pp.h[l] - win + 1; a.ow = pp.w[l] - win + 1;
        a.c1 = c1; a.c2 = c2;
        for (int k = 0; k < PM_MAXWIN; ++k) a.g[k] = k < win ? taps_host[k] : 0.f;
        const dim3 grid((unsigned)pp.tiles[l], gy);
        switch (win) {
            case 1: pm_launch_level<1>(a, l == 0, grid, stream); break;
            case 3: pm_launch_level<3>(a, l == 0, grid, stream); break;
            case 5: pm_launch_level<5>(a, l == 0, grid, stream); break;
            case 7: pm_launch_level<7>(a, l == 0, grid, stream); break;
            case 9: pm_launch_level<9>(a, l == 0, grid, stream); break;
            default: pm_launch_level<11>(a, l == 0, grid, stream); break;
        }
    }
    PmFinishArgs f;
    for (int l = 0; l < levels; ++l) {
        f.part[l] = pp.part[l]; f.tiles[l] = pp.tiles[l];
        f.count[l] = (double)(pp.h[l] - win + 1) * (double)(pp.w[l] - win + 1);
    }
    f.part[levels] = pp.epart; f.tiles[levels] = pp.tiles[0];
    f.planes = pp.planes; f.levels = levels;
    f.means = pp.means; f.ssim = ssim; f.cs = cs; f.err = err;
    hipLaunchKernelGGL(la_pm_finish_kernel, dim3((unsigned)(levels + 1), gy), dim3(64), 0, stream, f);
    PmCombineArgs c;
    c.means = pp.means; c.ms = ms; c.planes = pp.planes; c.levels = levels;
    for (int l = 0; l < PM_MAXLEV; ++l) c.w[l] = l < levels ? (double)weights_host[l] : 0.0;
    const long cb = (pp.planes + 255) / 256;
    hipLaunchKernelGGL(la_pm_combine_kernel, dim3((unsigned)(cb < 1024 ? cb : 1024)), dim3(256), 0, stream, c);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Joint histogram.  grid (pixel chunks, min(planes, 65535)): a workgroup counts JH_CHUNK pixels of one plane pair into a bins x bins
// uint32 table in LDS and adds its non-zero bins to the plane's table in memory with integer atomics (order-independent).
// A thread walks JH_PT consecutive pixels and issues one LDS add per RUN of equal bin pairs: a constant background (most of a medical
// slice) costs one add per thread instead of JH_PT adds that all serialise on one LDS address.
#define JH_PT 8
#define JH_CHUNK (256 * JH_PT)
#define JH_MAXBINS 64

__device__ __forceinline__ int jh_bin(float v, float lo, float scale, int bins) {
    const float f = floorf((v - lo) * scale);
    return (int)fminf(fmaxf(f, 0.f), (float)(bins - 1));          // NaN counts in bin 0
}

__global__ __launch_bounds__(256) void la_joint_hist_kernel(const float* __restrict__ a, long a_stride, const float* __restrict__ b,
                                                            long b_stride, long planes, long npix, int bins, float lo, float scale,
                                                            int vec, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[JH_MAXBINS * JH_MAXBINS];
    const int nb = bins * bins;
    const long i0 = (long)blockIdx.x * JH_CHUNK + (long)threadIdx.x * JH_PT;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        for (int i = threadIdx.x; i < nb; i += 256) sh[i] = 0u;
        __syncthreads();
        const float* pa = a + pl * a_stride;
        const float* pb = b + pl * b_stride;
        if (i0 < npix) {
            float va[JH_PT], vb[JH_PT];
            const int n = npix - i0 < JH_PT ? (int)(npix - i0) : JH_PT;
            if (vec && n == JH_PT) {          // both planes 16-byte aligned at every chunk offset
                const float4 a0 = *(const float4*)(pa + i0), a1 = *(const float4*)(pa + i0 + 4);
                const float4 b0 = *(const float4*)(pb + i0), b1 = *(const float4*)(pb + i0 + 4);
                va[0] = a0.x; va[1] = a0.y; va[2] = a0.z; va[3] = a0.w; va[4] = a1.x; va[5] = a1.y; va[6] = a1.z; va[7] = a1.w;
                vb[0] = b0.x; vb[1] = b0.y; vb[2] = b0.z; vb[3] = b0.w; vb[4] = b1.x; vb[5] = b1.y; vb[6] = b1.z; vb[7] = b1.w;
            } else {
#pragma unroll
                for (int j = 0; j < JH_PT; ++j) {
                    va[j] = j < n ? pa[i0 + j] : 0.f;
                    vb[j] = j < n ? pb[i0 + j] : 0.f;
                }
            }
            int cur = jh_bin(va[0], lo, scale, bins) * bins + jh_bin(vb[0], lo, scale, bins);
            unsigned run = 1u;
#pragma unroll
            for (int j = 1; j < JH_PT; ++j) {
                if (j < n) {
                    const int k = jh_bin(va[j], lo, scale, bins) * bins + jh_bin(vb[j], lo, scale, bins);
                    if (k != cur) {
                        atomicAdd(&sh[cur], run);
                        cur = k;
                        run = 0u;
                    }
                    ++run;
                }
            }
            atomicAdd(&sh[cur], run);
        }
        __syncthreads();
        unsigned* h = hist + pl * nb;
        for (int i = threadIdx.x; i < nb; i += 256) {
            const unsigned v = sh[i];
            if (v) atomicAdd(&h[i], v);
        }
        __syncthreads();
    }
}

extern "C" int la_joint_hist_f32(const float* a, long a_plane_stride, const float* b, long b_plane_stride, long planes, long npix,
                                 int bins, float lo, float scale, unsigned* hist, hipStream_t stream) {
    LA_CHECK_ARG(a && b && hist, "joint_hist: null pointer");
    LA_CHECK_ARG(bins >= 1 && bins <= JH_MAXBINS, "joint_hist: bins must lie in 1 .. 64");
    LA_CHECK_ARG(planes >= 1 && npix >= 1, "joint_hist: planes and npix must be positive");
    LA_CHECK_ARG(npix <= 0xffffffffL, "joint_hist: a plane of more pixels than a uint32 count holds");
    LA_CHECK_ARG(planes <= 0x7fffffffL, "joint_hist: too many planes");
    LA_CHECK_ARG(a_plane_stride >= 0 && b_plane_stride >= 0, "joint_hist: negative plane stride");
    LA_CHECK_ARG(scale > 0.f && scale == scale && lo == lo, "joint_hist: scale must be positive and lo a number");
    LA_CHECK_ARG(la_aligned<4>(a, b, hist), "joint_hist: pointers must be 4-byte aligned");
    LA_HIP(hipMemsetAsync(hist, 0, (size_t)planes * bins * bins * sizeof(unsigned), stream));
    const int vec = ((((size_t)a | (size_t)b) & 15) == 0 && a_plane_stride % 4 == 0 && b_plane_stride % 4 == 0) ? 1 : 0;
    const long chunks = (npix + JH_CHUNK - 1) / JH_CHUNK;
    hipLaunchKernelGGL(la_joint_hist_kernel, dim3((unsigned)chunks, (unsigned)(planes < 65535 ? planes : 65535)), dim3(256), 0, stream,
                       a, a_plane_stride, b, b_plane_stride, planes, npix, bins, lo, scale, vec, hist);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
