// filtered_lrelu: bias -> zero-insert up -> pad / crop -> FIR fu (gain up^2) -> * gain -> leaky ReLU -> clamp -> FIR fd -> keep every
// down-th sample, per (n, c) plane (the nine steps of the reference's filtered_lrelu.py:59-108; plugin entry filtered_lrelu.cpp:16-18).
//
// Two paths, chosen on the host:
//   fused    la_flrelu_fused_kernel<UP, DOWN>: one workgroup = one output tile of one plane.  The input tile + halo is staged in LDS with
//            the bias added, the up-FIR runs polyphase (only the taps that land on non-zero samples; a 1-D filter as two 1-D passes, a
//            2-D filter as one 2-D pass), the activation runs in place in LDS (evaluating lrelu, or multiplying by the derivative read
//            from a sign buffer), then the down-FIR + decimation writes the tile.  The up-sampled intermediate never reaches HBM.
//            Envelope: up, down in {1, 2, 4}, at most 8 * up taps of fu and 8 * down taps of fd per axis, LDS <= 64 KB.
//   generic  la_flrelu_generic_kernel: one thread per output, direct FIR that recomputes each intermediate sample it needs from the
//            input and the taps in device memory (any up, down >= 1, filters up to 64 x 64); la_flrelu_generic_signs_kernel writes the
//            sign buffer of that path.  Correct, not fast.
// Both share the activation / sign stage (flr_act) with la_flrelu_act_kernel, the in-place activation of la_filtered_lrelu_act_f32.
//
// Sign buffer (include/latentaug_hip.h): 2 bits per intermediate sample, bit 0 = "negative" (the value times gain was < 0), bit 1 =
// "clamped" (|lrelu| > clamp); 4 samples per byte, sample t of a row at bits 2 * (t % 4) of byte t / 4; rows of row_bytes (a multiple
// of 4), planes of `rows` rows.  A call reads sample (ty + sy, tx + sx) for intermediate sample (ty, tx); outside the buffer it reads 0.
#include "la_common.h"

#include <math.h>

#include <algorithm>

#define FLR_THREADS 256
#define FLR_MAX_TAPS 64
#define FLR_LDS_BYTES 65536

struct FlrArgs {
    const float* x; const float* fu; const float* fd; const float* b;
    const unsigned char* si; unsigned char* so; float* y;
    int C, H, W, OH, OW;
    int fuh, fuw, fdh, fdw;        // taps per axis (a 1-D filter: fuh == fuw)
    int fu2d, fd2d;                // 1 = 2-D filter, 0 = the same 1-D filter along both axes
    int up, down, px0, py0;
    int ah, aw;                    // active intermediate extent (the samples some output reads): (O - 1) * down + fd taps
    int sx, sy, srows, swid, spitch;   // sign buffer: offsets, rows per plane, samples per row, bytes per row
    float gain, slope, clamp;      // clamp: +inf = none
    float upgain;                  // up^2, the gain of the up-FIR
    int flip;
    int mode;                      // 0 = plain, 1 = write signs, 2 = read signs
    // fused path only
    int tow, toh, mw, mh, iw, ih, pin, pmid, pdh;
};

static __device__ __forceinline__ int flr_floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
static __device__ __forceinline__ int flr_posmod(int a, int b) { const int r = a % b; return r < 0 ? r + b : r; }

// activation of one intermediate sample `v` (already times up^2): evaluated (mode 0 / 1, *bits = its two sign bits) or taken from the
// stored derivative (mode 2: gain, gain * slope or 0)
static __device__ __forceinline__ float flr_act(float v, int mode, unsigned rbits, float gain, float slope, float clamp, unsigned* bits) {
    float a = v * gain;
    if (mode == 2) {
        if (rbits & 2u) return 0.f;
        return (rbits & 1u) ? a * slope : a;
    }
    unsigned s = 0;
    if (a < 0.f) { a *= slope; s = 1u; }
    if (fabsf(a) > clamp) { a = a > 0.f ? clamp : -clamp; s |= 2u; }
    *bits = s;
    return a;
}

static __device__ __forceinline__ unsigned flr_read_bits(const unsigned char* si, long plane, int srows, int swid, int spitch, int ry, int rx) {
    if (ry < 0 || ry >= srows || rx < 0 || rx >= swid) return 0u;
    return (si[(plane * srows + ry) * (long)spitch + (rx >> 2)] >> (2 * (rx & 3))) & 3u;
}

// correlation tap k of an axis of K taps: flip = correlation with the filter as given, else convolution (the filter reversed)
static __device__ __forceinline__ int flr_tap(int k, int K, int flip) { return flip ? k : K - 1 - k; }

// ------------------------------------------------------------------------------------------------------------ fused path
template <int UP, int DOWN>
__global__ void __launch_bounds__(FLR_THREADS) la_flrelu_fused_kernel(FlrArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x;      // (planes on x: the grid's only axis without a 65535 limit)
    const int c = plane % a.C;
    const int o0x = blockIdx.y * a.tow, o0y = blockIdx.z * a.toh;
    const int mx0 = o0x * DOWN, my0 = o0y * DOWN;
    const int ix0 = flr_floordiv(mx0 - a.px0 + UP - 1, UP), iy0 = flr_floordiv(my0 - a.py0 + UP - 1, UP);

    // LDS: taps | region 1 (input tile [ih][pin], then (1-D fu) the horizontal pass [ih][pmid]; later (1-D fd) [mh][pdh]) | mid [mh][pmid]
    const int nfu = a.fu2d ? a.fuh * a.fuw : a.fuw, nfd = a.fd2d ? a.fdh * a.fdw : a.fdw;
    float* sfu = lds;
    float* sfd = sfu + nfu;
    float* sin = sfd + nfd;
    float* shp = sin + a.ih * a.pin;
    float* sdh = sin;
    const int r1 = max(a.ih * a.pin + (a.fu2d ? 0 : a.ih * a.pmid), a.fd2d ? 0 : a.mh * a.pdh);
    float* smid = sin + r1;

    // taps in correlation order, the up-FIR gain folded in (up^2 for a 2-D filter, up per axis for a 1-D one)
    const float gu = a.fu2d ? a.upgain : (float)UP;
    for (int i = tid; i < nfu; i += FLR_THREADS) {
        int src;
        if (a.fu2d) { const int ky = i / a.fuw, kx = i - ky * a.fuw; src = flr_tap(ky, a.fuh, a.flip) * a.fuw + flr_tap(kx, a.fuw, a.flip); }
        else src = flr_tap(i, a.fuw, a.flip);
        sfu[i] = a.fu ? a.fu[src] * gu : gu;
    }
    for (int i = tid; i < nfd; i += FLR_THREADS) {
        int src;
        if (a.fd2d) { const int ky = i / a.fdw, kx = i - ky * a.fdw; src = flr_tap(ky, a.fdh, a.flip) * a.fdw + flr_tap(kx, a.fdw, a.flip); }
        else src = flr_tap(i, a.fdw, a.flip);
        sfd[i] = a.fd ? a.fd[src] : 1.f;
    }
    // input tile + halo, bias added to the samples of the image only (the padding is zeros)
    {
        const float bias = a.b ? a.b[c] : 0.f;
        const float* xp = a.x + (long)plane * a.H * a.W;
        const int n = a.ih * a.iw;
        for (int e = tid; e < n; e += FLR_THREADS) {
            const int r = e / a.iw, q = e - r * a.iw;
            const int gy = iy0 + r, gx = ix0 + q;
            float v = 0.f;
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = xp[(long)gy * a.W + gx] + bias;
            sin[r * a.pin + q] = v;
        }
    }
    __syncthreads();

    // up-FIR, polyphase: intermediate sample t reads upsampled position u = t - pad + k; only k with u % UP == 0 hit an input sample
    if (a.fu2d) {
        const int n = a.mh * a.mw;
        for (int e = tid; e < n; e += FLR_THREADS) {
            const int j = e / a.mw, i = e - j * a.mw;
            const int uy = my0 + j - a.py0, ux = mx0 + i - a.px0;
            const int ky0 = flr_posmod(-uy, UP), kx0 = flr_posmod(-ux, UP);
            const int ly0 = (uy + ky0) / UP - iy0, lx0 = (ux + kx0) / UP - ix0;
            float acc = 0.f;
            for (int ky = ky0, ly = ly0; ky < a.fuh; ky += UP, ++ly) {
                const float* fr = sfu + ky * a.fuw;
                const float* ir = sin + ly * a.pin;
                for (int kx = kx0, lx = lx0; kx < a.fuw; kx += UP, ++lx) acc = fmaf(fr[kx], ir[lx], acc);
            }
            smid[j * a.pmid + i] = acc;
        }
    } else {
        const int n = a.ih * a.mw;
        for (int e = tid; e < n; e += FLR_THREADS) {
            const int r = e / a.mw, i = e - r * a.mw;
            const int ux = mx0 + i - a.px0;
            const int kx0 = flr_posmod(-ux, UP);
            const float* ir = sin + r * a.pin + ((ux + kx0) / UP - ix0);
            float acc = 0.f;
            for (int kx = kx0, lx = 0; kx < a.fuw; kx += UP, ++lx) acc = fmaf(sfu[kx], ir[lx], acc);
            shp[r * a.pmid + i] = acc;
        }
        __syncthreads();
        const int m = a.mh * a.mw;
        for (int e = tid; e < m; e += FLR_THREADS) {
            const int j = e / a.mw, i = e - j * a.mw;
            const int uy = my0 + j - a.py0;
            const int ky0 = flr_posmod(-uy, UP);
            const float* hc = shp + ((uy + ky0) / UP - iy0) * a.pmid + i;
            float acc = 0.f;
            for (int ky = ky0, ly = 0; ky < a.fuw; ky += UP, ++ly) acc = fmaf(sfu[ky], hc[ly * a.pmid], acc);
            smid[j * a.pmid + i] = acc;
        }
    }
    __syncthreads();

    // activation in place, 4 consecutive samples (one sign byte) per item; in write mode a tile stores the bytes of the samples it owns:
    // [m0, m0 + tile * DOWN) per axis, the last tile of a row / column up to the active extent (mx0 is a multiple of 4: tow is)
    {
        const int gw = a.mw >> 2;
        const int n = a.mh * gw;
        const bool lastx = o0x + a.tow >= a.OW, lasty = o0y + a.toh >= a.OH;
        const int ownx1 = lastx ? a.aw : mx0 + a.tow * DOWN, owny1 = lasty ? a.ah : my0 + a.toh * DOWN;
        for (int e = tid; e < n; e += FLR_THREADS) {
            const int j = e / gw, g = e - j * gw;
            float* p = smid + j * a.pmid + 4 * g;
            const int ty = my0 + j, tx = mx0 + 4 * g;
            unsigned byte = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned rb = 0, wb = 0;
                if (a.mode == 2) rb = flr_read_bits(a.si, plane, a.srows, a.swid, a.spitch, ty + a.sy, tx + q + a.sx);
                p[q] = flr_act(p[q], a.mode, rb, a.gain, a.slope, a.clamp, &wb);
                if (tx + q < ownx1) byte |= wb << (2 * q);
            }
            if (a.mode == 1 && ty < owny1 && tx < ownx1) a.so[((long)plane * a.srows + ty) * a.spitch + (tx >> 2)] = (unsigned char)byte;
        }
    }
    __syncthreads();

    // down-FIR + decimation
    float* yp = a.y + (long)plane * a.OH * a.OW;
    const int nout = a.toh * a.tow;
    if (a.fd2d) {
        for (int e = tid; e < nout; e += FLR_THREADS) {
            const int p = e / a.tow, o = e - p * a.tow;
            if (o0y + p >= a.OH || o0x + o >= a.OW) continue;
            float acc = 0.f;
            for (int ky = 0; ky < a.fdh; ++ky) {
                const float* fr = sfd + ky * a.fdw;
                const float* mr = smid + (p * DOWN + ky) * a.pmid + o * DOWN;
                for (int kx = 0; kx < a.fdw; ++kx) acc = fmaf(fr[kx], mr[kx], acc);
            }
            yp[(long)(o0y + p) * a.OW + o0x + o] = acc;
        }
    } else {
        const int n = a.mh * a.tow;
        for (int e = tid; e < n; e += FLR_THREADS) {
            const int j = e / a.tow, o = e - j * a.tow;
            const float* mr = smid + j * a.pmid + o * DOWN;
            float acc = 0.f;
            for (int kx = 0; kx < a.fdw; ++kx) acc = fmaf(sfd[kx], mr[kx], acc);
            sdh[j * a.pdh + o] = acc;
        }
        __syncthreads();
        for (int e = tid; e < nout; e += FLR_THREADS) {
            const int p = e / a.tow, o = e - p * a.tow;
            if (o0y + p >= a.OH || o0x + o >= a.OW) continue;
            const float* dc = sdh + p * DOWN * a.pdh + o;
            float acc = 0.f;
            for (int ky = 0; ky < a.fdw; ++ky) acc = fmaf(sfd[ky], dc[ky * a.pdh], acc);
            yp[(long)(o0y + p) * a.OW + o0x + o] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ generic path
// one intermediate sample (ty, tx) of plane `plane`, times up^2, straight from x and the taps in device memory
static __device__ float flr_mid_direct(const FlrArgs& a, long plane, float bias, int ty, int tx) {
    const float* xp = a.x + plane * a.H * a.W;
    const int uy = ty - a.py0, ux = tx - a.px0;
    const int ky0 = flr_posmod(-uy, a.up), kx0 = flr_posmod(-ux, a.up);
    float acc = 0.f;
    for (int ky = ky0; ky < a.fuh; ky += a.up) {
        const int iy = (uy + ky) / a.up;
        if (iy < 0 || iy >= a.H) continue;
        const int fy = flr_tap(ky, a.fuh, a.flip);
        const float wy = a.fu2d ? 1.f : a.fu[fy];      // (a NULL filter is a 2-D 1 x 1 identity)
        for (int kx = kx0; kx < a.fuw; kx += a.up) {
            const int ix = (ux + kx) / a.up;
            if (ix < 0 || ix >= a.W) continue;
            const int fx = flr_tap(kx, a.fuw, a.flip);
            const float w = a.fu2d ? (a.fu ? a.fu[fy * a.fuw + fx] : 1.f) : wy * a.fu[fx];
            acc = fmaf(w, xp[(long)iy * a.W + ix] + bias, acc);
        }
    }
    return acc * a.upgain;
}

__global__ void __launch_bounds__(FLR_THREADS) la_flrelu_generic_kernel(FlrArgs a, long total) {
    const long e = (long)blockIdx.x * FLR_THREADS + threadIdx.x;
    if (e >= total) return;
    const int ox = (int)(e % a.OW);
    const long r = e / a.OW;
    const int oy = (int)(r % a.OH);
    const long plane = r / a.OH;
    const float bias = a.b ? a.b[plane % a.C] : 0.f;
    float acc = 0.f;
    for (int ky = 0; ky < a.fdh; ++ky) {
        const int fy = flr_tap(ky, a.fdh, a.flip);
        const float wy = a.fd2d ? 1.f : a.fd[fy];
        const int ty = oy * a.down + ky;
        for (int kx = 0; kx < a.fdw; ++kx) {
            const int fx = flr_tap(kx, a.fdw, a.flip);
            const float w = a.fd2d ? (a.fd ? a.fd[fy * a.fdw + fx] : 1.f) : wy * a.fd[fx];
            const int tx = ox * a.down + kx;
            unsigned rb = 0, wb = 0;
            if (a.mode == 2) rb = flr_read_bits(a.si, plane, a.srows, a.swid, a.spitch, ty + a.sy, tx + a.sx);
            const float v = flr_act(flr_mid_direct(a, plane, bias, ty, tx), a.mode, rb, a.gain, a.slope, a.clamp, &wb);
            acc = fmaf(w, v, acc);
        }
    }
    a.y[e] = acc;
}

// sign bytes of the generic path: one byte (4 samples) of the active intermediate per thread
__global__ void __launch_bounds__(FLR_THREADS) la_flrelu_generic_signs_kernel(FlrArgs a, long total) {
    const long e = (long)blockIdx.x * FLR_THREADS + threadIdx.x;
    if (e >= total) return;
    const int gw = (a.aw + 3) >> 2;
    const int g = (int)(e % gw);
    const long r = e / gw;
    const int ty = (int)(r % a.ah);
    const long plane = r / a.ah;
    const float bias = a.b ? a.b[plane % a.C] : 0.f;
    unsigned byte = 0;
    for (int q = 0; q < 4; ++q) {
        const int tx = 4 * g + q;
        if (tx >= a.aw) break;
        unsigned wb = 0;
        flr_act(flr_mid_direct(a, plane, bias, ty, tx), 1, 0u, a.gain, a.slope, a.clamp, &wb);
        byte |= wb << (2 * q);
    }
    a.so[(plane * a.srows + ty) * a.spitch + g] = (unsigned char)byte;
}

// ------------------------------------------------------------------------------------------------------------ in-place activation
// (the plugin's filtered_lrelu_act_): x [planes][H][W] in place, 4 samples (one sign byte) per thread; sign buffer [planes][H][row_bytes]
__global__ void __launch_bounds__(FLR_THREADS) la_flrelu_act_kernel(float* x, const unsigned char* si, unsigned char* so, int H, int W,
                                                                    int spitch, int sx, int sy, float gain, float slope, float clamp,
                                                                    int mode, long total) {
    const long e = (long)blockIdx.x * FLR_THREADS + threadIdx.x;
    if (e >= total) return;
    const int gw = (W + 3) >> 2;
    const int g = (int)(e % gw);
    const long r = e / gw;
    const int h = (int)(r % H);
    const long plane = r / H;
    float* p = x + (plane * H + h) * W;
    unsigned byte = 0;
    for (int q = 0; q < 4; ++q) {
        const int w = 4 * g + q;
        if (w >= W) break;
        unsigned rb = 0, wb = 0;
        if (mode == 2) rb = flr_read_bits(si, plane, H, W, spitch, h + sy, w + sx);
        p[w] = flr_act(p[w], mode, rb, gain, slope, clamp, &wb);
        byte |= wb << (2 * q);
    }
    if (mode == 1) so[(plane * H + h) * spitch + g] = (unsigned char)byte;
}

// ------------------------------------------------------------------------------------------------------------ host side
static long flr_floordiv_h(long a, long b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

extern "C" int la_filtered_lrelu_out_size(int in_size, int up, int down, int pad0, int pad1, int fu_taps, int fd_taps) {
    if (up < 1 || down < 1) return 0;
    return (int)flr_floordiv_h((long)in_size * up + pad0 + pad1 - (fu_taps - 1) - (fd_taps - 1) + (down - 1), down);
}

// rows / samples per row of the sign buffer: the larger of the active extents seen from the output side, (O - 1) * down + fd taps, and
// from the input side, (I - 1) * up + fu taps.  The backward call (up <-> down, fu <-> fd, x <-> y) swaps the two, so the forward, the
// backward and every higher-order call of one op agree on the layout.
static void flr_sign_extent(int I, int O, int up, int down, int fut, int fdt, int* active, int* extent) {
    *active = (O - 1) * down + fdt;
    const int inside = (I - 1) * up + fut;
    *extent = *active > inside ? *active : inside;
}

extern "C" int la_filtered_lrelu_sign_shape(int H, int W, int fu_h, int fu_w, int fd_h, int fd_w, int up, int down, int px0, int px1, int py0,
                                            int py1, int* rows, int* row_bytes) {
    LA_CHECK_ARG(rows && row_bytes, "filtered_lrelu_sign_shape: rows / row_bytes must not be NULL");
    LA_CHECK_ARG(H >= 1 && W >= 1 && up >= 1 && down >= 1 && fu_w >= 1 && fd_w >= 1 && fu_h >= 0 && fd_h >= 0,
                 "filtered_lrelu_sign_shape: bad sizes");
    const int fuy = fu_h ? fu_h : fu_w, fdy = fd_h ? fd_h : fd_w;
    const int OW = la_filtered_lrelu_out_size(W, up, down, px0, px1, fu_w, fd_w), OH = la_filtered_lrelu_out_size(H, up, down, py0, py1, fuy, fdy);
    LA_CHECK_ARG(OW >= 1 && OH >= 1, "filtered_lrelu_sign_shape: output must be at least 1x1");
    int aw, ah, ew, eh;
    flr_sign_extent(W, OW, up, down, fu_w, fd_w, &aw, &ew);
    flr_sign_extent(H, OH, up, down, fuy, fdy, &ah, &eh);
    *rows = eh;
    *row_bytes = 4 * ((ew + 15) / 16);
    return LA_OK;
}

// fused tile: the largest candidate whose LDS fits (0 = none)
static int flr_fused_lds(FlrArgs& a, int tow, int toh) {
    a.tow = tow; a.toh = toh;
    const int mw = std::max((tow - 1) * a.down + a.fdw, tow * a.down), mh = std::max((toh - 1) * a.down + a.fdh, toh * a.down);
    a.mw = (mw + 3) & ~3; a.mh = mh;
    a.iw = (a.mw + a.fuw - 2) / a.up + 1; a.ih = (a.mh + a.fuh - 2) / a.up + 1;
    a.pin = a.iw | 1; a.pmid = a.mw | 1; a.pdh = tow | 1;
    const long nfu = a.fu2d ? a.fuh * a.fuw : a.fuw, nfd = a.fd2d ? a.fdh * a.fdw : a.fdw;
    const long r1 = std::max((long)a.ih * a.pin + (a.fu2d ? 0 : (long)a.ih * a.pmid), a.fd2d ? 0L : (long)a.mh * a.pdh);
    return (int)std::min(4L * (nfu + nfd + r1 + (long)a.mh * a.pmid), (long)INT32_MAX);
}

static bool flr_fused_ok(int up, int down, int fut, int fdt) {
    return (up == 1 || up == 2 || up == 4) && (down == 1 || down == 2 || down == 4) && fut <= 8 * up && fdt <= 8 * down;
}

template <int UP, int DOWN>
static void flr_launch_fused(const FlrArgs& a, int lds, int planes, hipStream_t s) {
    const dim3 grid((unsigned)planes, (unsigned)la_cdiv(a.OW, a.tow), (unsigned)la_cdiv(a.OH, a.toh));
    hipLaunchKernelGGL((la_flrelu_fused_kernel<UP, DOWN>), grid, dim3(FLR_THREADS), lds, s, a);
}

template <int UP>
static void flr_launch_fused_up(const FlrArgs& a, int lds, int planes, hipStream_t s) {
    if (a.down == 1) flr_launch_fused<UP, 1>(a, lds, planes, s);
    else if (a.down == 2) flr_launch_fused<UP, 2>(a, lds, planes, s);
    else flr_launch_fused<UP, 4>(a, lds, planes, s);
}

extern "C" int la_filtered_lrelu_f32(const float* x, const float* fu, const float* fd, const float* b, const unsigned char* si, unsigned char* so,
                                     float* y, int N, int C, int H, int W, int fu_h, int fu_w, int fd_h, int fd_w, int up, int down, int px0,
                                     int px1, int py0, int py1, int sx, int sy, float gain, float slope, float clamp, int flip, int write_signs,
                                     hipStream_t stream) {
    // (the checks of filtered_lrelu.cpp:21-79, host side, before any launch)
    LA_CHECK_ARG(x && y, "filtered_lrelu: x and y must not be NULL");
    LA_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "filtered_lrelu: x is empty");
    LA_CHECK_ARG((long)N * C <= INT32_MAX && (long)N * C * H * W <= (1L << 40), "filtered_lrelu: x is too large");
    if (!fu) { fu_h = 1; fu_w = 1; }
    if (!fd) { fd_h = 1; fd_w = 1; }
    LA_CHECK_ARG(fu_w >= 1 && fu_h >= 0, "filtered_lrelu: fu is empty");
    LA_CHECK_ARG(fd_w >= 1 && fd_h >= 0, "filtered_lrelu: fd is empty");
    LA_CHECK_ARG(fu_w <= FLR_MAX_TAPS && fu_h <= FLR_MAX_TAPS && fd_w <= FLR_MAX_TAPS && fd_h <= FLR_MAX_TAPS,
                 "filtered_lrelu: filters are limited to 64 x 64 taps");
    LA_CHECK_ARG(up >= 1 && down >= 1, "filtered_lrelu: up and down must be at least 1");
    LA_CHECK_ARG(gain > 0.f && slope >= 0.f && clamp >= 0.f, "filtered_lrelu: need gain > 0, slope >= 0, clamp >= 0 (+inf = no clamp)");
    LA_CHECK_ARG(!(write_signs && si), "filtered_lrelu: signs are either written or read, not both");
    LA_CHECK_ARG(!write_signs || so, "filtered_lrelu: write_signs needs a sign buffer (so)");
    LA_CHECK_ARG(!write_signs || (sx == 0 && sy == 0), "filtered_lrelu: sign offsets must be 0 when writing signs");
    const int fuy = fu_h ? fu_h : fu_w, fdy = fd_h ? fd_h : fd_w;
    const long cw = (long)W * up + px0 + px1 - (fu_w - 1), ch = (long)H * up + py0 + py1 - (fuy - 1);
    LA_CHECK_ARG(cw > fd_w - 1 && ch > fdy - 1, "filtered_lrelu: upsampled buffer must be at least the size of downsampling filter");
    LA_CHECK_ARG(cw <= INT32_MAX / 2 && ch <= INT32_MAX / 2, "filtered_lrelu: upsampled buffer is too large");
    const int OW = la_filtered_lrelu_out_size(W, up, down, px0, px1, fu_w, fd_w), OH = la_filtered_lrelu_out_size(H, up, down, py0, py1, fuy, fdy);
    LA_CHECK_ARG(OW >= 1 && OH >= 1, "filtered_lrelu: output must be at least 1x1");

    FlrArgs a{};
    a.x = x; a.fu = fu; a.fd = fd; a.b = b; a.y = y;
    a.mode = write_signs ? 1 : (si ? 2 : 0);
    a.si = si; a.so = so;
    a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    a.fu2d = (fu && fu_h > 0) ? 1 : 0; a.fd2d = (fd && fd_h > 0) ? 1 : 0;
    if (!fu) a.fu2d = 1;
    if (!fd) a.fd2d = 1;
    a.fuh = fuy; a.fuw = fu_w; a.fdh = fdy; a.fdw = fd_w;
    a.up = up; a.down = down; a.px0 = px0; a.py0 = py0;
    int ew, eh;
    flr_sign_extent(W, OW, up, down, fu_w, fd_w, &a.aw, &ew);
    flr_sign_extent(H, OH, up, down, fuy, fdy, &a.ah, &eh);
    a.sx = sx; a.sy = sy; a.srows = eh; a.swid = ew; a.spitch = 4 * ((ew + 15) / 16);
    a.gain = gain; a.slope = slope; a.clamp = clamp;
    a.upgain = (float)up * (float)up;
    a.flip = flip ? 1 : 0;
    const int planes = N * C;

    int lds = 0;
    if (flr_fused_ok(up, down, std::max(fu_w, fuy), std::max(fd_w, fdy))) {
        static const int cand[][2] = {{32, 32}, {32, 16}, {16, 16}, {16, 8}, {8, 8}, {4, 4}};
        for (const auto& t : cand) {
            // (the same number of tiles as the candidate, spread evenly: 36 outputs -> 2 tiles of 20, not 32 + 4)
            const int tow = (la_cdiv(OW, la_cdiv(OW, t[0])) + 3) & ~3, toh = la_cdiv(OH, la_cdiv(OH, t[1]));
            const int need = flr_fused_lds(a, tow, toh);
            if (need <= FLR_LDS_BYTES) { lds = need; break; }
        }
    }
    if (lds > 0) {
        if (up == 1) flr_launch_fused_up<1>(a, lds, planes, stream);
        else if (up == 2) flr_launch_fused_up<2>(a, lds, planes, stream);
        else flr_launch_fused_up<4>(a, lds, planes, stream);
        LA_CHECK_LAUNCH();
        return LA_OK;
    }
    if (a.mode == 1) {
        const long ns = (long)planes * a.ah * ((a.aw + 3) / 4);
        hipLaunchKernelGGL(la_flrelu_generic_signs_kernel, dim3((unsigned)((ns + FLR_THREADS - 1) / FLR_THREADS)), dim3(FLR_THREADS), 0, stream, a, ns);
        LA_CHECK_LAUNCH();
        a.mode = 0;      // (the output itself needs no signs)
    }
    const long total = (long)planes * OH * OW;
    hipLaunchKernelGGL(la_flrelu_generic_kernel, dim3((unsigned)((total + FLR_THREADS - 1) / FLR_THREADS)), dim3(FLR_THREADS), 0, stream, a, total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_filtered_lrelu_act_f32(float* x, const unsigned char* si, unsigned char* so, int N, int C, int H, int W, int sx, int sy,
                                         float gain, float slope, float clamp, int write_signs, hipStream_t stream) {
    LA_CHECK_ARG(x, "filtered_lrelu_act: x must not be NULL");
    LA_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "filtered_lrelu_act: x is empty");
    LA_CHECK_ARG((long)N * C <= INT32_MAX && (long)N * C * H * W <= (1L << 40), "filtered_lrelu_act: x is too large");
    LA_CHECK_ARG(gain > 0.f && slope >= 0.f && clamp >= 0.f, "filtered_lrelu_act: need gain > 0, slope >= 0, clamp >= 0 (+inf = no clamp)");
    LA_CHECK_ARG(!(write_signs && si), "filtered_lrelu_act: signs are either written or read, not both");
    LA_CHECK_ARG(!write_signs || so, "filtered_lrelu_act: write_signs needs a sign buffer (so)");
    LA_CHECK_ARG(!write_signs || (sx == 0 && sy == 0), "filtered_lrelu_act: sign offsets must be 0 when writing signs");
    const int mode = write_signs ? 1 : (si ? 2 : 0);
    const long total = (long)N * C * H * ((W + 3) / 4);
    hipLaunchKernelGGL(la_flrelu_act_kernel, dim3((unsigned)((total + FLR_THREADS - 1) / FLR_THREADS)), dim3(FLR_THREADS), 0, stream, x, si, so, H,
                       W, 4 * ((W + 15) / 16), sx, sy, gain, slope, clamp, mode, total);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
