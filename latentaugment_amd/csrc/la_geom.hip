// The kernels of the GeometricAugment plugin (the reference's augments/geometric_aug.py builds the same pipeline from kornia):
// horizontal flip and a small rotation / shift as ONE affine resampling, an elastic deformation as a second one, the smoothed noise field
// that drives it, and the counter-based uniform noise that field is made of.  float32 NCHW, x the column index, y the row index, pixel
// centres at integer coordinates.  Sampling is bilinear under padding 'zeros', 'border' or 'reflection' (la_geom_index.h: the range
// test happens in floating point, before any int exists).  Nothing here uses atomics: every output element is written by one thread
// from sums taken in a fixed order, so two runs give the same bits.
//
//   la_noise_uniform_f32   the noise stream of la_rng.h: four words -> four values in (-1, 1)
//   la_elastic_field_f32   separable zero-border blur of both noise planes, ONE launch: a workgroup stages its 16 x 64 output tile with a
//                          halo of (ntaps - 1) / 2 on every side in LDS, filters the rows into a second LDS image, then the columns
//   la_warp_affine_f32     out[b,c,y,x] = S(in[b,c], Minv[b] (x, y, 1))
//   la_warp_elastic_f32    out[b,c,y,x] = S(in[b,c], position of the displaced normalised grid)
#include "la_common.h"
#include "la_rng.h"
#include "la_geom_index.h"

#include <limits.h>

#define LA_GEOM_BLOCK 256
#define LA_GEOM_MAXTAPS 63
#define LA_EF_TW 64      // output tile of the field kernel: one wave along x ...
#define LA_EF_TH 16      // ... 16 rows; LDS at the largest halo (31): (78 x 126 + 78 x 64) floats = 59 280 bytes, two workgroups per CU

// ------------------------------------------------------------------------------------------------------------ uniform noise
// word j of the block of counter e / 4 (la_noise_words) is element 4 (e / 4) + j, mapped into (-1, 1) by la_unit_uniform
__global__ __launch_bounds__(LA_GEOM_BLOCK) void la_noise_uniform_kernel(float* __restrict__ out, long rows, long row_elems, unsigned k0, unsigned k1,
                                                                         unsigned stream_id, long row0) {
    const long q4 = (row_elems + 3) >> 2;
    const long g = (long)blockIdx.x * LA_GEOM_BLOCK + threadIdx.x;
    if (g >= rows * q4) return;
    const long r = g / q4, q = g - r * q4;
    unsigned x[4];
    la_noise_words(q, row0 + r, stream_id, k0, k1, x);
    float* o = out + r * row_elems + 4 * q;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * q + k < row_elems) o[k] = la_unit_uniform(x[k]);
}

extern "C" int la_noise_uniform_f32(float* out, long rows, long row_elems, unsigned long long seed, unsigned stream_id, long row0, hipStream_t stream) {
    LA_CHECK_ARG((out || rows == 0) && rows >= 0 && row_elems >= 1 && row0 >= 0, "noise_uniform: bad arguments");
    LA_CHECK_ARG(row0 + rows <= 0xffffffffl, "noise_uniform: row index exceeds 32 bits");
    if (rows == 0) return LA_OK;
    const long q4 = (row_elems + 3) >> 2;
    LA_CHECK_ARG((double)rows * (double)q4 <= (double)INT_MAX * LA_GEOM_BLOCK, "noise_uniform: more than INT_MAX workgroups: refused");
    hipLaunchKernelGGL(la_noise_uniform_kernel, dim3((unsigned)la_cdiv(rows * q4, LA_GEOM_BLOCK)), dim3(LA_GEOM_BLOCK), 0, stream, out, rows,
                       row_elems, (unsigned)seed, (unsigned)(seed >> 32), stream_id, row0);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------ elastic field
struct LaGeomTaps {
    float t[LA_GEOM_MAXTAPS];      // kernel argument: the tap index is wave-uniform, so every read is a scalar load
};

// disp[b][p][y][x] = alpha_p * sum_i taps[i] * ( sum_j taps[j] * noise[b][p][y + i - R][x + j - R] ), noise outside the image = 0
// (a correlation, as F.conv2d; the plugin's Gaussian is symmetric).  One workgroup per 16 x 64 output tile of one plane:
//   1. tile [16 + 2R][64 + 2R]  <- noise, zero outside the image: the one read of the noise from memory (the halo from L2);
//   2. rows [16 + 2R][64]       <- the row pass, taps in ascending order with fmaf;
//   3. disp                     <- the column pass over `rows`, the same way, times alpha: the one write.
// In both passes the 64 lanes of a wave hold 64 consecutive x of one row, so every LDS read and write of a wave covers 64 consecutive
// dwords: conflict-free under the 32-bank rule of ds_read_b32 / ds_write_b32 whatever the pitch, and the pitch needs no padding.
__global__ __launch_bounds__(LA_GEOM_BLOCK) void la_elastic_field_kernel(const float* __restrict__ noise, float* __restrict__ disp, LaGeomTaps taps,
                                                                        int ntaps, float alpha_x, float alpha_y, int H, int W) {
    extern __shared__ float la_ef_lds[];
    const int R = ntaps >> 1;
    const int TWH = LA_EF_TW + 2 * R, THH = LA_EF_TH + 2 * R;
    float* tile = la_ef_lds;                   // [THH][TWH]
    float* rows = la_ef_lds + THH * TWH;       // [THH][LA_EF_TW]
    const int x0 = blockIdx.x * LA_EF_TW, y0 = blockIdx.y * LA_EF_TH;
    const long plane = (long)blockIdx.z * H * W;
    const float* src = noise + plane;
    for (int i = threadIdx.x; i < THH * TWH; i += LA_GEOM_BLOCK) {
        const int ty = i / TWH, tx = i - ty * TWH;
        const int gy = y0 + ty - R, gx = x0 + tx - R;
        tile[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(long)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int lx = threadIdx.x & (LA_EF_TW - 1), ly = threadIdx.x / LA_EF_TW;      // 4 waves: wave ly takes rows ly, ly + 4, ...
    for (int ty = ly; ty < THH; ty += LA_GEOM_BLOCK / LA_EF_TW) {
        const float* t = tile + ty * TWH + lx;
        float acc = 0.f;
        for (int k = 0; k < ntaps; ++k) acc = fmaf(taps.t[k], t[k], acc);
        rows[ty * LA_EF_TW + lx] = acc;
    }
    __syncthreads();
    const float alpha = (blockIdx.z & 1) ? alpha_y : alpha_x;
    const int gx = x0 + lx;
    for (int ty = ly; ty < LA_EF_TH; ty += LA_GEOM_BLOCK / LA_EF_TW) {
        const int gy = y0 + ty;
        if (gx >= W || gy >= H) continue;
        const float* t = rows + ty * LA_EF_TW + lx;
        float acc = 0.f;
        for (int k = 0; k < ntaps; ++k) acc = fmaf(taps.t[k], t[k * LA_EF_TW], acc);
        disp[plane + (long)gy * W + gx] = alpha * acc;
    }
}

extern "C" int la_elastic_field_f32(const float* noise, const float* taps_host, int ntaps, float alpha_x, float alpha_y, float* disp, float* ws, int B,
                                    int H, int W, hipStream_t stream) {
    (void)ws;      // the one-launch form keeps the row pass in LDS
    LA_CHECK_ARG(noise && taps_host && disp, "elastic_field: null pointer");
    LA_CHECK_ARG(noise != disp, "elastic_field: noise and disp must not alias");
    LA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "elastic_field: empty or negative shape");
    LA_CHECK_ARG(ntaps >= 1 && ntaps <= LA_GEOM_MAXTAPS && (ntaps & 1), "elastic_field: ntaps must be odd and at most 63");
    LA_CHECK_ARG((double)B * 2 * H * W <= (double)INT_MAX, "elastic_field: more than INT_MAX elements: refused");
    LA_CHECK_ARG(2 * B <= 65535 && la_cdiv(H, LA_EF_TH) <= 65535, "elastic_field: more than 65535 planes or row tiles: refused");
    LaGeomTaps taps;
    for (int k = 0; k < LA_GEOM_MAXTAPS; ++k) taps.t[k] = k < ntaps ? taps_host[k] : 0.f;
    const int R = ntaps >> 1;
    const size_t lds = (size_t)(LA_EF_TH + 2 * R) * (LA_EF_TW + 2 * R + LA_EF_TW) * sizeof(float);
    hipLaunchKernelGGL(la_elastic_field_kernel, dim3((unsigned)la_cdiv(W, LA_EF_TW), (unsigned)la_cdiv(H, LA_EF_TH), (unsigned)(2 * B)),
                       dim3(LA_GEOM_BLOCK), lds, stream, noise, disp, taps, ntaps, alpha_x, alpha_y, H, W);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------ the two warps
struct LaGeomTaps4 {
    float w[4];       // nw, ne, sw, se
    int off[4];       // offset inside one H x W plane (0 where the corner is not addressable)
    bool in[4];
};

__device__ __forceinline__ LaGeomTaps4 la_geom_taps(float px, float py, int H, int W, int mode) {
    const LaGsAxis<float> ax = la_geom_axis<float>(px, W, mode), ay = la_geom_axis<float>(py, H, mode);
    LaGeomTaps4 t;
    t.w[0] = ax.w0 * ay.w0; t.w[1] = ax.w1 * ay.w0; t.w[2] = ax.w0 * ay.w1; t.w[3] = ax.w1 * ay.w1;
    t.in[0] = ax.in0 && ay.in0; t.in[1] = ax.in1 && ay.in0; t.in[2] = ax.in0 && ay.in1; t.in[3] = ax.in1 && ay.in1;
    const int o = ay.i0 * W + ax.i0;
    t.off[0] = t.in[0] ? o : 0; t.off[1] = t.in[1] ? o + 1 : 0; t.off[2] = t.in[2] ? o + W : 0; t.off[3] = t.in[3] ? o + W + 1 : 0;
    return t;
}

// corners and weights once, then the channels: y = sum over the addressable corners, nw, ne, sw, se in this order
__device__ __forceinline__ void la_geom_gather(const float* __restrict__ xp, float* __restrict__ yp, const LaGeomTaps4& t, int C, long HW) {
    for (int c = 0; c < C; ++c, xp += HW, yp += HW) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.in[k]) v += t.w[k] * xp[t.off[k]];
        *yp = v;
    }
}

__device__ __forceinline__ void la_geom_copy(const float* __restrict__ xp, float* __restrict__ yp, int C, long HW) {
    for (int c = 0; c < C; ++c, xp += HW, yp += HW) *yp = *xp;
}

// One thread per output pixel, consecutive lanes along x; blockIdx.y is the sample, so apply[b] and Minv[b] are wave-uniform loads.
__global__ __launch_bounds__(LA_GEOM_BLOCK) void la_warp_affine_kernel(const float* __restrict__ x, const float* __restrict__ minv,
                                                                      const unsigned char* __restrict__ apply, float* __restrict__ y, int C, int H,
                                                                      int W, int mode) {
    const int HW = H * W;
    const long il = (long)blockIdx.x * LA_GEOM_BLOCK + threadIdx.x;
    if (il >= HW) return;
    const int i = (int)il;
    const int b = blockIdx.y;
    const float* xp = x + (long)b * C * HW;
    float* yp = y + (long)b * C * HW + i;
    if (!apply[b]) {
        la_geom_copy(xp + i, yp, C, HW);
        return;
    }
    const float* m = minv + 6 * b;
    const int oy = i / W, ox = i - oy * W;
    const float fx = (float)ox, fy = (float)oy;
    const float px = fmaf(m[0], fx, fmaf(m[1], fy, m[2]));
    const float py = fmaf(m[3], fx, fmaf(m[4], fy, m[5]));
    la_geom_gather(xp, yp, la_geom_taps(px, py, H, W, mode), C, HW);
}

// a clamp that lets NaN through (fminf / fmaxf would turn it into a bound): the position is then refused by la_geom_axis
__device__ __forceinline__ float la_geom_clamp1(float g) { return g < -1.f ? -1.f : (g > 1.f ? 1.f : g); }

// g = clamp(-1 + 2 i / (size - 1) + d, -1, 1) (0 on a one-pixel axis), position ((g + 1) size - 1) / 2
__device__ __forceinline__ float la_geom_elastic_pos(int i, int size, float d) {
    const float g = size == 1 ? 0.f : la_geom_clamp1((-1.f + (2.f * (float)i) / (float)(size - 1)) + d);
    return la_geom_unnormalize<float>(g, size);
}

__global__ __launch_bounds__(LA_GEOM_BLOCK) void la_warp_elastic_kernel(const float* __restrict__ x, const float* __restrict__ disp,
                                                                       const unsigned char* __restrict__ apply, float* __restrict__ y, int C, int H,
                                                                       int W, int mode) {
    const int HW = H * W;
    const long il = (long)blockIdx.x * LA_GEOM_BLOCK + threadIdx.x;
    if (il >= HW) return;
    const int i = (int)il;
    const int b = blockIdx.y;
    const float* xp = x + (long)b * C * HW;
    float* yp = y + (long)b * C * HW + i;
    if (!apply[b]) {
        la_geom_copy(xp + i, yp, C, HW);
        return;
    }
    const int oy = i / W, ox = i - oy * W;
    const float* d = disp + (long)b * 2 * HW + i;
    const float px = la_geom_elastic_pos(ox, W, d[0]);
    const float py = la_geom_elastic_pos(oy, H, d[HW]);
    la_geom_gather(xp, yp, la_geom_taps(px, py, H, W, mode), C, HW);
}

static int warp_check(const char* who, const void* x, const void* par, const void* apply, const void* y, int B, int C, int H, int W, int mode) {
    static thread_local char msg[160];
    const char* what = nullptr;
    if (!x || !par || !apply || !y) what = "null pointer";
    else if (x == y) what = "x and y must not alias";
    else if (B < 1 || C < 1 || H < 1 || W < 1) what = "empty or negative shape";
    else if (mode != LA_GEOM_ZEROS && mode != LA_GEOM_BORDER && mode != LA_GEOM_REFLECTION) what = "unknown padding mode";
    else if ((double)B * C * H * W > (double)INT_MAX) what = "more than INT_MAX elements: refused";
    else if (B > 65535) what = "more than 65535 samples: refused";
    if (!what) return LA_OK;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    la_set_error(msg);
    return LA_ERR_ARG;
}

extern "C" int la_warp_affine_f32(const float* x, const float* minv, const unsigned char* apply, float* y, int B, int C, int H, int W, int mode,
                                  hipStream_t stream) {
    const int rc = warp_check("warp_affine", x, minv, apply, y, B, C, H, W, mode);
    if (rc) return rc;
    hipLaunchKernelGGL(la_warp_affine_kernel, dim3((unsigned)la_cdiv((long)H * W, LA_GEOM_BLOCK), (unsigned)B), dim3(LA_GEOM_BLOCK), 0, stream, x, minv,
                       apply, y, C, H, W, mode);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_warp_elastic_f32(const float* x, const float* disp, const unsigned char* apply, float* y, int B, int C, int H, int W, int mode,
                                   hipStream_t stream) {
    const int rc = warp_check("warp_elastic", x, disp, apply, y, B, C, H, W, mode);
    if (rc) return rc;
    hipLaunchKernelGGL(la_warp_elastic_kernel, dim3((unsigned)la_cdiv((long)H * W, LA_GEOM_BLOCK), (unsigned)B), dim3(LA_GEOM_BLOCK), 0, stream, x, disp,
                       apply, y, C, H, W, mode);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
