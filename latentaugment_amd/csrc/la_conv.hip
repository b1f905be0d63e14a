// Implicit-GEMM convolution, fp32 MFMA 32x32x2 (see la_conv.h).  Written for gfx950 only.
//
// Tiling: workgroup = 256 threads = 4 waves in a 2(m) x 2(n) grid; block tile MT(out channels) x 128(pixels);
// each wave owns (MT/2) x 64 as TM x 2 MFMA tiles of 32x32.  K is walked in chunks of (one tap, 16 input
// channels): the A slab [16][MT] comes straight from the tap-major packed weights (float4, coalesced), the B
// slab [16][128] is gathered from the NCHW input (lanes = consecutive pixels, coalesced) with the per-(b,c)
// modulation multiplied in on the way to LDS.  The next chunk's global loads are issued before the current
// chunk's MFMAs (register-staged prefetch); fp32 MFMA takes 64 cycles per instruction so the loader has slack.
#include "la_conv.h"
#include <stdlib.h>
#include "la_conv_device.h"
#include <type_traits>

#define KC 16

int la_conv_tiles_per_sample(int Gy, int Gx) { return la_cdiv((long)Gy * Gx, NT); }

#define SPLITK_MAX_G 1156     // up to 34x34 grids (covers the 33x33 phases of the 32 -> 64 up-sampling layer)
// K chunks and row tile of a launch, for la_conv_plan and the workspace sizes alike; 32-row tiles only exist for the halo kernel (the
// 32-channel layers of the 1024^2 generators)
static inline int conv_nck(int C, bool bf) { return la_cdiv(C, bf ? KCB : KC); }
static inline int conv_mt(int M, bool halo) { return M >= 128 ? 128 : (M <= 32 && halo ? 32 : 64); }
// K slices of a split-K launch over `tiles` (flattened-pixel tiles x row tiles) workgroups, each walking nck chunks x `taps`
// (chunk, tap) steps.  The 16-bit kernels keep 2 workgroups per CU = 512 resident slots.  Cost model in microseconds, fitted to
// the kernel trace of the config-f generator (profiles/): a step costs ~1.7 us of a resident slot, a workgroup ~10 us of
// prologue + epilogue, and slicing adds a finish pass that reads ks partial copies of the output and writes it once at
// ~3.5 TB/s (+5 us of launch).  E.g. 256 tiles x 144 steps -> 2 slices; the 4 merged 33x33 phases of the 32 -> 64 layer
// (1060 tiles x 36 steps, 69 MB of output) -> no slices: their finish pass would cost more than the tail it removes.
// (The fp32 kernel keeps 3 workgroups per CU: 768 slots, rounded up as before.)
static int choose_ksplit(bool bf, long tiles, int nck, float taps, double out_bytes) {
    int ks;
    if (bf) {
        float best = 1e30f;
        ks = 1;
        for (int k = 1; k <= nck && k <= 16; ++k) {
            const int per = la_cdiv(nck, k);
            const int kk = la_cdiv(nck, per);                       // slices actually launched
            if (kk != k) continue;
            const float slots = (float)(tiles * kk) / 512.f;
            const float rounds = slots <= 1.f ? 1.f : slots;          // (dynamic dispatch: beyond one round, work / slots)
            float cost = rounds * ((float)per * taps * 1.7f + 10.f);
            if (kk > 1) cost += 5.f + (float)((kk + 1) * out_bytes / 3.5e6);
            if (cost < best - 1e-3f) { best = cost; ks = kk; }
        }
        return ks;
    }
    ks = la_cdiv(768, tiles);
    if (ks > nck) ks = nck;
    if (ks < 2) return 1;
    const int per = la_cdiv(nck, ks);
    return la_cdiv(nck, per);
}

// scratch floats of the split-K form of a launch whose nphase (>= 1) output phases have the grids Gy[p] x Gx[p]; 0 if the launch
// would not be split
long la_conv_splitk_floats_phases(int B, int M, int C, int nphase, const int* Gy, const int* Gx, int precision) {
    const bool bf = precision != LA_PREC_F32;
    const int nck = conv_nck(C, bf);
    if (nck < 2 || nphase < 1 || (nphase > 1 && !bf)) return 0;
    const int mtiles = la_cdiv(M, conv_mt(M, false));      // (a launch that splits is no halo launch)
    long tiles = 0, Gsum = 0;
    for (int p = 0; p < nphase; ++p) {
        const long G = (long)Gy[p] * Gx[p];
        if (G > SPLITK_MAX_G) return 0;
        tiles += la_cdiv((long)B * G, NT);
        Gsum += G;
    }
    // (upper bound over the tap counts a launch of these grids may have: fewer taps never ask for more slices ... except that
    //  cheaper steps favour fewer slices; size for the densest case, 9 taps, and for the 9/4 of transposed-conv phases)
    int ks = choose_ksplit(bf, tiles * mtiles, nck, nphase > 1 ? 2.25f : 9.f, 4.0 * B * M * (double)Gsum);
    const int ks1 = choose_ksplit(bf, tiles * mtiles, nck, 1.f, 4.0 * B * M * (double)Gsum);
    if (ks1 > ks) ks = ks1;
    return ks >= 2 ? (long)ks * B * M * Gsum : 0;
}

// SPLIT = false: one workgroup owns a (sample, 128-pixel tile, MT-channel tile) and runs the whole K loop, epilogue fused.
// SPLIT = true : pixels of all samples are flattened (tiles may straddle samples), blockIdx.z walks K slices, raw
//                accumulators go to ws[slice][b][m][g]; la_conv_splitk_finish_kernel sums the slices and applies the epilogue.
//                Used for the <= 32x32 layers, whose K loop (up to 4608 deep) would otherwise serialise on a handful of CUs.
template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void la_conv_igemm_kernel(LaConvArgs a) {
    constexpr int TM = MT / 64;            // 32-row MFMA tiles per wave along m
    constexpr int A_F4 = (KC * MT / 4) / 256;  // float4 loads of the A slab per thread (2 for MT=128, 1 for MT=64)
    __shared__ __attribute__((aligned(16))) float As[2][KC][MT];
    __shared__ __attribute__((aligned(16))) float Bs[2][KC][NT];
    __shared__ float red[4][MT];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    // XCD-aware tile order (direct mode): workgroups are dealt round-robin over the 8 XCDs, so give each XCD a contiguous
    // run of pixel tiles -- vertically adjacent tiles (which share the +-1 row halos of the 3x3 taps) then hit the same L2.
    int ntile = blockIdx.x;
    if (!SPLIT && (gridDim.x & 7) == 0) ntile = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int m0 = blockIdx.y * MT;
    const int G = a.Gy * a.Gx;
    const int Ntot = SPLIT ? a.B * G : G;

    // ---- loader roles
    const int n_l = tid & (NT - 1);
    const int khalf = tid >> 7;
    const int nidx_l = ntile * NT + n_l;
    const bool nvalid = nidx_l < Ntot;
    int b_l = SPLIT ? (nvalid ? nidx_l / G : 0) : (int)blockIdx.z;
    const int g_l = SPLIT ? nidx_l - b_l * G : nidx_l;
    const int gy_l = nvalid ? g_l / a.Gx : 0;
    const int gx_l = nvalid ? g_l - gy_l * a.Gx : 0;
    const int iy0 = gy_l * a.in_sy, ix0 = gx_l * a.in_sx;
    const long HWin = (long)a.Hin * a.Win;
    const float* in_b = a.in + (long)b_l * a.in_bstride;
    const float* sc_b = a.in_scale ? a.in_scale + (long)b_l * a.scale_stride : nullptr;

    const int nck = (a.C + KC - 1) / KC;
    int ck_beg = 0, ck_end = nck;
    if (SPLIT) {
        const int per = (nck + a.ksplit - 1) / a.ksplit;
        ck_beg = blockIdx.z * per;
        ck_end = ck_beg + per < nck ? ck_beg + per : nck;
    }
    const int ci_beg = ck_beg * a.ntaps, ci_end = ck_end * a.ntaps;

    float breg[KC / 2];
    float4 areg[A_F4];

    auto prefetch = [&](int ci) {
        const int cc = ci / a.ntaps;
        const int t = ci - cc * a.ntaps;
        const int c0 = cc * KC;
        const int iy = iy0 + a.tap_dy[t], ix = ix0 + a.tap_dx[t];
        const bool ok = nvalid && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
        const long off = (long)iy * a.Win + ix;
#pragma unroll
        for (int j = 0; j < KC / 2; ++j) {
            const int c = c0 + khalf + 2 * j;
            float v = 0.f;
            if (ok && c < a.C) {
                v = in_b[(long)c * HWin + off];
                if (sc_b) v *= sc_b[c];
            }
            breg[j] = v;
        }
        const float* wslab = a.wgt + (long)a.tap_w[t] * a.C * a.M;
#pragma unroll
        for (int j = 0; j < A_F4; ++j) {
            const int idx = tid + 256 * j;
            const int row = idx / (MT / 4), col = (idx - row * (MT / 4)) * 4;
            const int c = c0 + row, m = m0 + col;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < a.C && m < a.M) v = *reinterpret_cast<const float4*>(wslab + (long)c * a.M + m);
            areg[j] = v;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < KC / 2; ++j) Bs[buf][khalf + 2 * j][n_l] = breg[j];
#pragma unroll
        for (int j = 0; j < A_F4; ++j) {
            const int idx = tid + 256 * j;
            const int row = idx / (MT / 4), col = (idx - row * (MT / 4)) * 4;
            *reinterpret_cast<float4*>(&As[buf][row][col]) = areg[j];
        }
    };

    f32x16 acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;
    if (ci_beg < ci_end) {
        prefetch(ci_beg);
        stage(0);
    }
    __syncthreads();
    // double-buffered LDS, one barrier per chunk: loads for chunk i+1 are in flight while chunk i feeds the MFMAs.  This is the loop of
    // la_f32_tile.h (la_tile_pipeline + la_f32_tile_mma) written out: taken from there it costs this kernel registers (see that header)
    for (int ci = ci_beg; ci < ci_end; ++ci) {
        const int buf = (ci - ci_beg) & 1;
        if (ci + 1 < ci_end) prefetch(ci + 1);
#pragma unroll
        for (int kp = 0; kp < KC / 2; ++kp) {
            float av[TM], bv[2];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[buf][2 * kp + lh][wm * (MT / 2) + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[buf][2 * kp + lh][wn * 64 + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (ci + 1 < ci_end) stage(buf ^ 1);
        __syncthreads();
    }

    la_conv_epilogue<MT, SPLIT>(a, acc, red, ntile, m0, G, Ntot);
}

// Split-K finisher: sums the K slices in a fixed order and applies the same epilogue as the direct kernel (deterministic).
// One wave per (b, m) plane, four planes per workgroup (the kernel is pure latency; with 16-byte loads a wave covers a 32x32 plane
// in four steps).
template <int PPB>      // planes per workgroup: 4 (one wave each) or 1
__global__ __launch_bounds__(256) void la_conv_splitk_finish_kernel(LaConvArgs a_in) {
    __shared__ float wpart[4];
    LaConvArgs a = a_in;
    if (a_in.nphase > 0) {        // merged phases: blockIdx.z = phase (grid, output offset and partials of that phase)
        const LaConvArgs::Phase& P = a_in.ph[blockIdx.z];
        a.Gy = P.Gy; a.Gx = P.Gx; a.out_oy = P.out_oy; a.out_ox = P.out_ox;
        a.splitk_ws = a_in.splitk_ws + P.ws_off;
    }
    constexpr int T = 256 / PPB;                    // threads per plane
    const int lane = threadIdx.x & 63;
    const int tp = threadIdx.x % T;
    const int m = blockIdx.x * PPB + threadIdx.x / T;
    const int b = blockIdx.y;
    const bool live = m < a.M;
    if (!live && PPB > 1) return;
    const int G = a.Gy * a.Gx;
    const int wpitch = (a.epi == LA_EPI_RAW && a.out_pitch > 0) ? a.out_pitch : a.Wout;
    const long HWout = (a.epi == LA_EPI_RAW && a.out_plane > 0) ? a.out_plane : (long)a.Hout * a.Wout;
    const long slice = (long)a.B * a.M * G;
    const float* wsp = a.splitk_ws + ((long)b * a.M + m) * G;
    float* out_p = a.out + ((long)b * a.M + m) * HWout;
    const float dmv = (a.epi == LA_EPI_FWD && a.demod) ? a.demod[(long)b * a.demod_stride + m] : 1.f;
    const float bv = (a.epi == LA_EPI_FWD && a.bias) ? a.bias[m] : 0.f;
    const float sc = (a.epi == LA_EPI_BWD && a.out_scale) ? a.out_scale[(long)b * a.oscale_stride + m] : 1.f;
    const float* xin_p = (a.epi == LA_EPI_BWD && a.xin) ? a.xin + (long)b * a.xin_bstride + (long)m * HWout : nullptr;
    // fused seam of the layer that produced xin (LaConvArgs::seam): same arithmetic as the direct kernels' epilogue
    const bool seam = a.epi == LA_EPI_BWD && a.seam.ddn_part != nullptr && xin_p != nullptr;
    const float dm0 = (seam && a.seam.demod) ? a.seam.demod[(long)b * a.seam.demod_stride + m] : 1.f;
    const float b0 = (seam && a.seam.bias) ? a.seam.bias[m] : 0.f;
    float part = 0.f, dd = 0.f, mx = 0.f;
    // (the sub-slot of the consumer's scale row this plane lowers, read early: the round trip hides under the slice loads)
    float* xs_row = (seam && a.seam.xs_out && lane == 0 && (PPB > 1 || threadIdx.x == 0)) ? a.seam.xs_out + (long)b * LA_XS_FAN + la_xs_sub((int)(threadIdx.x >> 6) * 5) : nullptr;
    // (forward epilogue: the same for LaConvArgs::fwd_xs_out, one atomic per wave)
    float ymax = 0.f;
    if (a.epi == LA_EPI_FWD && a.fwd_xs_out && lane == 0) xs_row = a.fwd_xs_out + (long)b * LA_XS_FAN + la_xs_sub((int)(threadIdx.x >> 6) * 5);
    const float xs_seen = xs_row ? la_xs_peek(xs_row) : 0.f;
    const int imgc = seam ? (a.seam.imgc < 4 ? a.seam.imgc : 4) : 0;
    float we[4] = {0.f, 0.f, 0.f, 0.f}, dwe[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < imgc; ++c) we[c] = a.seam.wrgb[(long)c * a.M + m] * a.seam.s_rgb[(long)b * a.seam.s_rgb_stride + m];
    // VEC consecutive grid positions per thread and step (4: 16-byte loads / stores when the rows allow it, else 1)
    auto run = [&](auto vec_tag) {
        constexpr int VEC = decltype(vec_tag)::value;
        typedef float vf __attribute__((ext_vector_type(VEC)));
        auto ld = [](const float* p) { return *reinterpret_cast<const vf*>(p); };
        for (int g = tp * VEC; g < G; g += T * VEC) {
            // (the slices' loads in flight eight at a time, added in slice order: with one load and one add per trip the pass was an
            //  exposed L2 latency per slice -- up to 16 of them at the 4x4 and 8x8 layers)
            // (sums written element by element: a vector add is v_pk_add_f32 -- no packed-FP32 arithmetic anywhere, Makefile)
            auto add = [](vf& s, const vf& p) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) s[e] += p[e];
            };
            vf acc = ld(wsp + g);
            int k = 1;
            for (; k + 7 < a.ksplit; k += 8) {
                vf p[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) p[u] = ld(wsp + (long)(k + u) * slice + g);
#pragma unroll
                for (int u = 0; u < 8; ++u) add(acc, p[u]);
            }
            if (k + 3 < a.ksplit) {
                vf p[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) p[u] = ld(wsp + (long)(k + u) * slice + g);
#pragma unroll
                for (int u = 0; u < 4; ++u) add(acc, p[u]);
                k += 4;
            }
            for (; k < a.ksplit; ++k) { const vf p = ld(wsp + (long)k * slice + g); add(acc, p); }
            const int gy = g / a.Gx, gx = g - gy * a.Gx;
            const long pos = (long)(gy * a.out_sy + a.out_oy) * wpitch + gx * a.out_sx + a.out_ox;
            float v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = VEC == 1 ? acc[0] : acc[e];
            if (a.epi == LA_EPI_FWD) {
                vf nz = 0.f;
                if (a.noise) nz = ld(a.noise + (long)b * a.noise_bstride + pos);
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = la_conv_epi_fwd(a, v[e], dmv, nz[e] * a.noise_strength, bv);
                if (a.out2) {
                    const long o2 = ((long)b * a.M + m) * HWout + pos;
                    vf ad = 0.f;
                    if (a.addend) ad = ld(a.addend + o2);
                    vf w;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) { w[e] = v[e] + ad[e]; ymax = fmaxf(ymax, fabsf(w[e])); }
                    *reinterpret_cast<vf*>(a.out2 + o2) = w;
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) ymax = fmaxf(ymax, fabsf(v[e]));
                }
            } else if (a.epi == LA_EPI_BWD) {
                vf y = 0.f;
                if (xin_p) y = ld(xin_p + pos);
                vf gv[4], nz0 = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    gv[c] = 0.f;
                    if (c < imgc) {
                        const long o = ((long)b * imgc + c) * HWout + pos;
                        gv[c] = ld(a.seam.g_img + o);
                        if (a.seam.rgb_clamp >= 0.f) {
                            const vf pre = ld(a.seam.rgb_pre + o);
#pragma unroll
                            for (int e = 0; e < VEC; ++e) if (fabsf(pre[e]) > a.seam.rgb_clamp) gv[c][e] = 0.f;
                        }
                    }
                }
                if (seam && a.seam.noise) {
                    nz0 = ld(a.seam.noise + (long)b * a.seam.noise_bstride + pos);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) nz0[e] *= a.seam.noise_strength;
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    part += v[e] * y[e];
                    v[e] *= sc;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < imgc) { v[e] += we[c] * gv[c][e]; dwe[c] += gv[c][e] * y[e]; }
                    if (seam) {
                        const float g1 = v[e] * la_act_bwd_from_y(y[e], a.seam.act, a.seam.alpha, a.seam.gain, a.seam.clamp);
                        dd += g1 * (la_act_inv(y[e], a.seam.act, a.seam.alpha, a.seam.gain) - b0 - nz0[e]);
                        v[e] = g1 * dm0;
                        mx = fmaxf(mx, fabsf(v[e]));
                    }
                }
            }
            vf w;
#pragma unroll
            for (int e = 0; e < VEC; ++e) w[e] = v[e];
            *reinterpret_cast<vf*>(out_p + pos) = w;
        }
    };
    {
        size_t al = (size_t)a.splitk_ws | (size_t)a.out | (size_t)a.out2 | (size_t)a.addend | (size_t)a.noise | (size_t)a.xin;
        if (seam) al |= (size_t)a.seam.noise | (size_t)(imgc ? a.seam.g_img : nullptr) | (size_t)(imgc ? a.seam.rgb_pre : nullptr);
        const bool vec4 = a.out_sx == 1 && ((a.Gx | wpitch | a.out_ox) & 3) == 0 && ((HWout | a.noise_bstride | a.seam.noise_bstride | a.xin_bstride) & 3) == 0 &&
                          (al & 15) == 0 && (a_in.nphase == 0 || (a_in.ph[blockIdx.z].ws_off & 3) == 0);
        if (vec4) run(std::integral_constant<int, 4>{});
        else run(std::integral_constant<int, 1>{});
    }
    if (a.epi == LA_EPI_FWD && a.fwd_xs_out) {      // (uniform; PPB == 1: every wave of the plane lowers its own sub-slot)
        ymax = la_wave_max(ymax);
        if (xs_row) la_xs_lower(xs_row, xs_seen, a.fwd_xs_mult ? a.fwd_xs_mult[b] : 1.f, ymax);
    }
    if (a.epi == LA_EPI_BWD && (a.ds_part || seam)) {
        part = la_wave_sum(part);
        dd = la_wave_sum(dd);
#pragma unroll
        for (int c = 0; c < 4; ++c) dwe[c] = la_wave_sum(dwe[c]);
        mx = la_wave_max(mx);
        if (PPB == 1) {
            __shared__ float wdd[4], wmx[4], wdw[4][4];
            if (lane == 0) {
                const int w = threadIdx.x >> 6;
                wpart[w] = part; wdd[w] = dd; wmx[w] = mx;
#pragma unroll
                for (int c = 0; c < 4; ++c) wdw[c][w] = dwe[c];
            }
            __syncthreads();
            part = (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
            dd = (wdd[0] + wdd[1]) + (wdd[2] + wdd[3]);
            mx = fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3]));
#pragma unroll
            for (int c = 0; c < 4; ++c) dwe[c] = (wdw[c][0] + wdw[c][1]) + (wdw[c][2] + wdw[c][3]);
        }
        // operand scale of the output for its consumer: one atomic per plane (wave) on a sub-slot of the sample's row
        if (xs_row) la_xs_lower(xs_row, xs_seen, a.seam.xs_mult, mx);
        if (tp < a.tiles_per_sample) {
            const long slot = ((long)b * a.M + m) * a.tiles_per_sample + tp;
            for (int c = 0; c < imgc; ++c)
                a.seam.dweff_part[(((long)b * imgc + c) * a.M + m) * a.tiles_per_sample + tp] = tp == 0 ? dwe[c] : 0.f;
            if (a.ds_part) a.ds_part[slot] = tp == 0 ? part : 0.f;
            if (seam) {
                a.seam.ddn_part[slot] = tp == 0 ? dd : 0.f;
                if (a.seam.pmax) a.seam.pmax[slot] = tp == 0 ? mx : 0.f;
            }
        }
    }
}

// can this launch use the halo kernel?  dense stride-1 3x3 taps within +-1, grid = whole 4x32 tiles, above the split-K sizes
static bool la_conv_bf16_uses_halo(const LaConvArgs& a) {
    if (a.precision == LA_PREC_F32 || a.in_q) return false;
    if (a.in_mask_y || (a.in_gain != 0.f && a.in_gain != 1.f)) return false;      // (an input mask is applied by the pre-split copy)
    if (a.in_sy != 1 || a.in_sx != 1 || a.out_sy != 1 || a.out_sx != 1 || a.out_oy != 0 || a.out_ox != 0) return false;
    if ((a.Gx & 31) != 0 || (a.Gy & 3) != 0 || a.Gy != a.Hout || a.Gx != a.Wout || a.ntaps != 9) return false;
    // Grids up to 34x34 stay on the split-K path (SPLITK_MAX_G).  Round 3 measured the 32x32 layers (512 -> 512, K = 4608) on
    // this kernel: 114 us against 135 us for slices + finish pass + pre-split copy in isolation, no difference inside a batch -- and
    // the first-step gradient of the 1024^2 loop 12x further from float64 (rms 4.4e-6 against 3.7e-7 of max |g| 0.4; the reference's
    // float32: 1.5e-6): K slices summed afterwards are a blocked summation, one accumulator walking all 4608 terms is not.  Dev knob
    // LA_KNOB_HALO_MING: grids of at least that many points run here.
    if ((long)a.Gy * a.Gx < (la_dev_knob(LA_KNOB_HALO_MING) ? la_dev_knob(LA_KNOB_HALO_MING) : SPLITK_MAX_G + 1)) return false;
    if ((long)a.C * a.Hin * a.Win >= (1l << 28) || a.C > 4096) return false;   // 32-bit byte offsets inside one sample, below the
                                                                             // out-of-range sentinel of the pixel-stationary loader
    for (int t = 0; t < a.ntaps; ++t)
        if (a.tap_dy[t] < -1 || a.tap_dy[t] > 1 || a.tap_dx[t] < -1 || a.tap_dx[t] > 1) return false;
    return true;
}

// The one place that decides which kernel a launch runs, in which form and on what grid (LaConvPlan, la_conv.h); the dev-build knobs
// that bend the decision are read here (and in the predicate above) only.
int la_conv_plan(const LaConvArgs& a, LaConvPlan& p) {
    LA_CHECK_ARG(a.in && a.wgt && a.out, "conv: null pointer");
    LA_CHECK_ARG(a.B > 0 && a.C > 0 && a.M > 0 && a.Gy > 0 && a.Gx > 0, "conv: empty shape");
    LA_CHECK_ARG(a.M % 4 == 0, "conv: M must be a multiple of 4");
    LA_CHECK_ARG(a.ntaps >= 1 && a.ntaps <= LA_CONV_MAX_TAPS, "conv: bad tap count");
    LA_CHECK_ARG(a.in_sy >= 1 && a.in_sx >= 1 && a.out_sy >= 1 && a.out_sx >= 1, "conv: bad strides");
    // last grid point must land inside the output
    LA_CHECK_ARG((a.Gy - 1) * a.out_sy + a.out_oy < a.Hout && (a.Gx - 1) * a.out_sx + a.out_ox < a.Wout && a.out_oy >= 0 && a.out_ox >= 0,
                 "conv: output grid exceeds output tensor");
    LA_CHECK_ARG((long)a.Hout * a.Wout < (1L << 31) && (long)a.Hin * a.Win < (1L << 31), "conv: plane too large");
    if (a.epi == LA_EPI_BWD && a.ds_part) {
        LA_CHECK_ARG(a.tiles_per_sample == la_conv_tiles_per_sample(a.Gy, a.Gx), "conv: tiles_per_sample mismatch");
        LA_CHECK_ARG(a.out_sy == 1 && a.out_sx == 1 && a.out_oy == 0 && a.out_ox == 0, "conv: bwd epilogue needs dense output");
    }
    LA_CHECK_ARG(a.col_hi == 0 || (a.row_hi > 0 && a.col_lo >= 0 && a.col_hi > a.col_lo), "conv: a column window needs a row window");
    LA_CHECK_ARG(a.col_hi == 0 || a.epi != LA_EPI_BWD || (a.Gy == a.Hout && a.Gx == a.Wout && a.out_sy == 1 && a.out_sx == 1 && a.out_oy == 0 && a.out_ox == 0),
                 "conv: a backward launch with a column window needs a dense output (it zero-fills the columns it leaves out)");
    const int nphase = a.nphase, np = nphase > 0 ? nphase : 1;
    LA_CHECK_ARG(nphase >= 0 && nphase <= LA_CONV_MAX_PHASES, "conv: bad phase count");
    if (nphase > 0) LA_CHECK_ARG(a.precision != LA_PREC_F32 && a.epi == LA_EPI_RAW && a.in_q, "conv: merged phases need a pre-split 16-bit launch without epilogue");
    for (int q = 0; q < nphase; ++q) {
        const LaConvArgs::Phase& P = a.ph[q];
        LA_CHECK_ARG(P.Gy > 0 && P.Gx > 0 && P.ntaps >= 1 && P.ntaps <= LA_CONV_PHASE_TAPS, "conv: bad phase");
        LA_CHECK_ARG((P.Gy - 1) * a.out_sy + P.out_oy < a.Hout && (P.Gx - 1) * a.out_sx + P.out_ox < a.Wout && P.out_oy >= 0 && P.out_ox >= 0,
                     "conv: phase grid exceeds output tensor");
    }
    const bool bf = a.precision != LA_PREC_F32;
    LA_CHECK_ARG(!bf || (a.wgt_bf16 && a.wgt_bf16_term_elems > 0), "conv: split-bf16 precision needs packed bf16 weights");
    const bool halo = la_conv_bf16_uses_halo(a);      // (never a merged launch: those arrive pre-split)
    p = LaConvPlan{}; p.ksplit = 1;
    // dev knob (kernel experiments only): LA_FORCE_MT=64 runs the >= 128-row layers on 64-row tiles
    static const int force_mt = []() { const char* e = la_dev_env("LA_FORCE_MT"); return e ? atoi(e) : 0; }();
    p.mt = (force_mt == 64 && a.M >= 128) ? 64 : conv_mt(a.M, halo);
    p.mtiles = la_cdiv(a.M, p.mt);
    // Operand preparation, from the head of the workspace.  Halo launches read the fp32 input directly (modulation, scaling and the split
    // happen on the way into LDS) and only need the fp16 scale; every other 16-bit launch gets a pre-split copy, [header | copy].
    if (bf && !a.in_q) {
        const size_t hb = la_conv_presplit_hdr_bytes(a.B, a.C), qb = la_conv_presplit_bytes(a.B, a.C, a.Hin, a.Win);
        p.scale_pass = a.precision == LA_PREC_F16X2 && !a.acc_scale_x;      // (a preset scale: e.g. from the clamp bound of the producer)
        p.prep = !halo ? LA_PREP_PRESPLIT : (p.scale_pass ? LA_PREP_SCALE : LA_PREP_NONE);
        if (p.prep != LA_PREP_NONE) {
            LA_CHECK_ARG(a.ws && a.ws_bytes >= (halo ? hb : qb), "conv: split precisions need a workspace (la_modconv_workspace_bytes)");
            LA_CHECK_ARG(((size_t)a.ws & 15) == 0, "conv: workspace must be 16-byte aligned");
            LA_CHECK_ARG(a.B <= 64, "conv: split precisions support at most 64 samples per launch");
        }
        if (p.prep == LA_PREP_PRESPLIT) {
            LA_CHECK_ARG(qb < 0x7ff00000u, "conv: pre-split operand too large for 32-bit buffer offsets");
            LA_CHECK_ARG((!a.in_mask_y && (a.in_gain == 0.f || a.in_gain == 1.f)) || !p.scale_pass, "conv: an input mask needs a preset operand scale");
            p.q_off = (a.precision == LA_PREC_F16X2 && !p.scale_pass) ? 0 : hb;
            const size_t off = (qb + 255) & ~(size_t)255; p.ws_head = a.ws_bytes > off ? off : a.ws_bytes;
        } else if (p.prep == LA_PREP_SCALE) p.ws_head = hb;
    }
    // Split-K for the small-resolution layers (see kernel comment), where the rest of the workspace holds the slice partials.  Merged
    // phases: blockIdx.x walks the phases' flattened-pixel tiles back to back.  (The halo kernel claims what it can run directly.)
    const long splitk_floats = a.ws ? (long)((a.ws_bytes - p.ws_head) / sizeof(float)) : 0;
    const int nck = conv_nck(a.C, bf);
    auto grid_of = [&](int q, int& Gy, int& Gx) { Gy = nphase > 0 ? a.ph[q].Gy : a.Gy; Gx = nphase > 0 ? a.ph[q].Gx : a.Gx; return nphase > 0 ? a.ph[q].ntaps : a.ntaps; };
    bool small = !halo;
    long Gsum = 0, tiles_flat = 0; int tiles = 0, Gy, Gx;
    for (int q = 0; q < np; ++q) {
        grid_of(q, Gy, Gx);
        const long Gq = (long)Gy * Gx;
        small = small && Gq <= SPLITK_MAX_G; Gsum += Gq;
        p.tile0[q] = (int)tiles_flat; tiles_flat += la_cdiv((long)a.B * Gq, NT);
        if (la_conv_tiles_per_sample(Gy, Gx) > tiles) tiles = la_conv_tiles_per_sample(Gy, Gx);
    }
    if (splitk_floats >= 1 && small && nck >= 2) {
        float taps = 0.f;      // per step of the K loop, weighted by the phases' share of the pixels
        for (int q = 0; q < np; ++q) { const int nt = grid_of(q, Gy, Gx); taps += (float)nt * ((float)Gy * Gx / (float)Gsum); }
        int ks = choose_ksplit(bf, tiles_flat * p.mtiles, nck, taps, 4.0 * a.B * a.M * (double)Gsum);
        if (la_dev_knob(LA_KNOB_KSPLIT) > 0 && la_dev_knob(LA_KNOB_KSPLIT) <= nck) { const int per = la_cdiv(nck, la_dev_knob(LA_KNOB_KSPLIT)); ks = la_cdiv(nck, per); }
        if (ks >= 2 && (long)ks * a.B * a.M * Gsum <= splitk_floats) p.ksplit = ks;
    }
    if (p.ksplit > 1) {
        long off = 0;
        for (int q = 0; q < np; ++q) { grid_of(q, Gy, Gx); p.ws_off[q] = off; off += (long)p.ksplit * a.B * a.M * Gy * Gx; }
        p.form = bf ? LA_FORM_FLAT_SPLIT : LA_FORM_F32_SPLIT; p.cls = bf ? LA_PC_CONV_SPLITK : LA_PC_CONV_F32;
        p.grid = dim3((unsigned)tiles_flat, p.mtiles, p.ksplit);
    } else {
        // a windowed 16-bit launch holds the window's tiles only (rounded up to a multiple of 8: one run of tiles per XCD); the kernels
        // derive the same counts from row_lo / row_hi / col_lo / col_hi
        if (bf && a.row_hi > 0) {
            int nt = 0;
            if (halo) {
                const int r0 = a.row_lo >> 2, r1 = ((a.row_hi < a.Gy ? a.row_hi : a.Gy) + 3) >> 2;
                const int cw = a.col_hi > 0 ? (((a.col_hi < a.Gx ? a.col_hi : a.Gx) + 31) >> 5) - (a.col_lo >> 5) : a.Gx >> 5;
                nt = (r1 - r0) * cw;
            } else {
                for (int q = 0; q < np; ++q) {
                    grid_of(q, Gy, Gx);
                    const int r1 = a.row_hi < Gy ? a.row_hi : Gy;
                    if (a.col_hi > 0) {      // the tiles of the rectangle, flattened over its own rows
                        const int c1 = a.col_hi < Gx ? a.col_hi : Gx;
                        const int ntq = (r1 > a.row_lo && c1 > a.col_lo) ? la_cdiv((r1 - a.row_lo) * (c1 - a.col_lo), NT) : 0;
                        if (ntq > nt) nt = ntq;
                        continue;
                    }
                    const int t0 = (a.row_lo * Gx) / NT, t1 = la_cdiv(r1 * Gx, NT);
                    if (t1 - t0 > nt) nt = t1 - t0;
                }
            }
            if (nt > 0 && ((nt + 7) & ~7) < tiles) tiles = (nt + 7) & ~7;
        }
        p.form = !bf ? LA_FORM_F32 : (halo ? LA_FORM_HALO : LA_FORM_FLAT); p.cls = !bf ? LA_PC_CONV_F32 : (halo ? LA_PC_CONV_HALO : LA_PC_CONV_FLAT);
        p.grid = dim3(tiles, p.mtiles, a.B * np);
    }
    // the MFMA form of that kernel: fp16 x2 has three-wave 16x16x32 forms on 128-row tiles (la_conv_flat.hip; la_conv_halo.hip: with more
    // than one chunk), every other 16-bit launch runs 32x32 MFMAs
    p.mfma = !bf ? LA_CONV_MFMA_F32_32X32X2 : (a.precision == LA_PREC_F16X2 && p.mt == 128 && (!halo || a.C > KCB) ? LA_CONV_MFMA_16X16X32 : LA_CONV_MFMA_32X32);
    return LA_OK;
}

// launch profiler: algorithmic work of a launch = 2*MACs; bytes = input read once + output written once (+ weights once)
static void conv_prof_work(const LaConvArgs& a, const LaConvPlan& p, double& flops, double& bytes) {
    double gt = (double)a.Gy * a.Gx * a.ntaps, gout = (double)a.Gy * a.Gx, ntw = a.ntaps;
    if (a.nphase > 0) gt = gout = ntw = 0.0;
    for (int q = 0; q < a.nphase; ++q) { gt += (double)a.ph[q].Gy * a.ph[q].Gx * a.ph[q].ntaps; gout += (double)a.ph[q].Gy * a.ph[q].Gx; ntw += a.ph[q].ntaps; }
    if (a.row_hi > 0 && a.Gy > 0) {      // row window: only the wanted rows are work (tiles hold 4 rows / 128 flattened pixels: counted as wanted)
        int lo = a.row_lo > 0 ? a.row_lo : 0, hi = a.row_hi < a.Gy ? a.row_hi : a.Gy;
        const bool rect = a.col_hi > 0 && a.Gx > 0 && p.form == LA_FORM_FLAT;      // flat kernel: exactly the rectangle
        if (!rect) { lo &= ~3; hi = (hi + 3) & ~3; if (hi > a.Gy) hi = a.Gy; }
        double f = hi > lo ? (double)(hi - lo) / a.Gy : 0.0;
        if (a.col_hi > 0 && a.Gx > 0 && p.form == LA_FORM_HALO) f *= (double)((((a.col_hi < a.Gx ? a.col_hi : a.Gx) + 31) & ~31) - (a.col_lo & ~31)) / a.Gx;
        if (rect) f *= (double)((a.col_hi < a.Gx ? a.col_hi : a.Gx) - a.col_lo) / a.Gx;
        gt *= f; gout *= f;
    }
    flops = 2.0 * a.B * gt * a.M * (double)a.C;
    bytes = 4.0 * ((double)a.B * a.C * a.Hin * a.Win * (a.in_bstride ? 1.0 : 1.0 / a.B) + (double)a.B * a.M * gout + ntw * a.C * a.M);
}

// plan, operand preparation as planned, the kernel-parameter fields the plan determines, one launch by the plan's form (+ the finish pass)
int la_conv_launch(const LaConvArgs& a, hipStream_t stream) {
    LaConvPlan p;
    int rc = la_conv_plan(a, p); if (rc) return rc;
    LaConvArgs as = a;
    if ((rc = la_conv_prepare_input(as, p, stream))) return rc;      // scratch: operand first, split-K partials after it
    as.ksplit = p.ksplit;
    as.splitk_ws = (as.ws && as.ws_bytes >= sizeof(float)) ? reinterpret_cast<float*>(as.ws) : nullptr;
    for (int q = 0; q < a.nphase; ++q) { as.ph[q].tile0 = p.tile0[q]; as.ph[q].ws_off = p.ws_off[q]; }
    if (a.precision == LA_PREC_F16X2)      // the fp16 weight scale lives behind the terms of the pack
        as.acc_scale_w = reinterpret_cast<const float*>(static_cast<const char*>(a.wgt_bf16) + la_conv_pack_wscale_offset(a.wgt_bf16_term_elems));
    if (as.seam.xs_out) as.seam.pmax = nullptr;      // every kernel form lowers the consumer's slot row itself: no plane maxima
#ifdef LA_DEV
    if (p.ksplit == 1) as.dbg_stamp = la_dev_knob(LA_KNOB_HALO_STAMP);
#endif
    double pflops = 0, pbytes = 0; if (la_prof_enabled()) conv_prof_work(a, p, pflops, pbytes);
    const int pslot = la_prof_open(p.cls, pflops, pbytes, stream);
    if (p.ksplit > 1) {
        if (p.form == LA_FORM_FLAT_SPLIT) rc = la_conv_flat_launch(as, p, stream);
        else if (p.mt == 128) hipLaunchKernelGGL((la_conv_igemm_kernel<128, true>), p.grid, dim3(256), 0, stream, as);
        else hipLaunchKernelGGL((la_conv_igemm_kernel<64, true>), p.grid, dim3(256), 0, stream, as);
        // the finish pass (it also lowers the consumer's operand scale, LaConvArgs::seam.xs_out): one wave per (b, m) plane, four planes per workgroup,
        // at every split-K size (<= 34x34): a whole workgroup per plane (the <1> form) measured 21 against 13 us on the 8 x 512 x 32^2 launches
        if (!rc) hipLaunchKernelGGL(la_conv_splitk_finish_kernel<4>, dim3(la_cdiv(a.M, 4), a.B, a.nphase > 0 ? a.nphase : 1), dim3(256), 0, stream, as);
    } else if (p.form == LA_FORM_HALO) rc = la_conv_halo_launch(as, p, stream);
    else if (p.form == LA_FORM_FLAT) rc = la_conv_flat_launch(as, p, stream);
    else if (p.mt == 128) hipLaunchKernelGGL((la_conv_igemm_kernel<128, false>), p.grid, dim3(256), 0, stream, as);
    else hipLaunchKernelGGL((la_conv_igemm_kernel<64, false>), p.grid, dim3(256), 0, stream, as);
    if (rc) return rc;
    LA_CHECK_LAUNCH();
    la_prof_close(pslot, stream);
    return LA_OK;
}

// Host-only query of the plan (include/latentaug_hip.h): an LaConvArgs of that geometry from the builders of la_conv.h, through la_conv_plan
extern "C" int la_conv_plan_query(int precision, int B, int C, int M, int geom, int res, int have_in_q, size_t ws_bytes, long* info) {
    LA_CHECK_ARG(info && precision >= LA_PREC_F32 && precision <= LA_PREC_F16X2 && geom >= 0 && geom <= LA_CONV_GEOM_UP2_MERGED && res >= 1 &&
                     (geom < LA_CONV_GEOM_DOWN2 || res % 2 == 0), "conv_plan_query: bad arguments (the stride-2 geometries need an even resolution)");
    alignas(16) static float never_read[4]; LaConvArgs a; la_conv_args_init(a);
    a.in = a.wgt = never_read; a.out = never_read; a.wgt_bf16 = never_read; a.wgt_bf16_term_elems = la_conv_bf16_pack_elems(M, C, 9);
    a.precision = precision; a.B = B; a.C = C; a.M = M;
    a.ws = ws_bytes ? never_read : nullptr; a.ws_bytes = ws_bytes; a.in_q = have_in_q ? never_read : nullptr;
    if (geom >= LA_CONV_GEOM_UP2_PHASE) la_conv_geom_up2(a, res / 2, 0, 0);
    if (geom <= LA_CONV_GEOM_SAME_BWD) la_conv_geom_same(a, res, 3, geom == LA_CONV_GEOM_SAME_BWD);
    else if (geom == LA_CONV_GEOM_DOWN2) la_conv_geom_down2(a, res);
    else if (geom == LA_CONV_GEOM_UP2_MERGED) la_conv_up2_merged(a, res / 2, 1);
    else la_conv_up2_phase(a, res / 2, (geom - LA_CONV_GEOM_UP2_PHASE) >> 1, (geom - LA_CONV_GEOM_UP2_PHASE) & 1, 1, false);
    LaConvPlan p;
    const int rc = la_conv_plan(a, p); if (rc) return rc;
    const long out[LA_CONV_PLAN_NINFO] = {p.cls, p.mt, p.mfma, p.ksplit, precision != LA_PREC_F32 && (have_in_q || p.prep == LA_PREP_PRESPLIT), a.nphase > 0, p.prep != LA_PREP_NONE,
                                          (long)p.grid.x, (long)p.grid.y, (long)p.grid.z, (long)p.ws_head};
    memcpy(info, out, sizeof(out));
    return LA_OK;
}
