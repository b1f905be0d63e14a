// Flat variant of the 16-bit split contraction (formats, tiling and weight pack: la_conv_operand.hip; shared pieces:
// la_conv_device.h): 128 consecutive grid positions per tile, any stride / tap table / ragged grid, optional split-K.
//   * B (pixels): thread (pixel, 16-channel half) gathers the tap-shifted inputs of one (chunk, tap) step with 16
//     unconditional buffer loads (clamped addresses; out-of-image pixels are zeroed on the way to LDS), one step ahead,
//     into the other of two swizzled LDS buffers (64-byte rows, slots XOR (row >> 2) & 3): ONE barrier per step.
//   * A (weights): MFMA fragments straight from the fragment-order pack, re-loaded for the next step right after the
//     MFMAs that read them have issued.  Never in LDS.
#include "la_conv_device.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define BPITCH 64
// WV = waves per SIMD the kernel is compiled for.  MF = form of the step (FLAT_MF_*, la_conv_device.h):
//   0 (FLAT_MF_32): v_mfma_f32_32x32x16 on two waves per SIMD, two sets of B fragments (K-step 1 read under the MFMAs of K-step 0), the weights of
//      the next step loaded a full step ahead -- every format, 128- and 64-row tiles.
//   1 (FLAT_MF_16): the fp16 x2 split-K launches on 128-row tiles, three waves per SIMD: the step on v_mfma_f32_16x16x32_f16, as in the halo kernel
//      (2 x 8 tiles of 16 x 16 per wave, every pixel fragment read once per step, LDS slots swizzled by 2 * ((pixel >> 2) & 1),
//      accumulators brought into the 32x32 layout through LDS before the shared epilogue).
//   2 (FLAT_MF_16_3BUF): MF 1 on THREE pixel buffers, for the direct launches.  The barrier at the end of step s then publishes the buffer of step s + 2,
//      so the buffer of step s + 1 is already complete while step s computes: its first fragments are read under the last MFMAs of
//      step s, and no LDS read latency is left exposed behind the barrier (two buffers: every step began with eight fragment reads
//      nothing could cover).
template <int MT, bool SPLIT, int FMT, int WV, int MF = FLAT_MF_32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WV))) void la_conv_bf16_kernel(LaConvArgs a_in) {
    static_assert(MF == FLAT_MF_32 ? WV == 2 : ((MF == FLAT_MF_16 || MF == FLAT_MF_16_3BUF) && WV == 3 && FMT == FMT_F16X2 && MT == 128),
                  "the 16x16x32 forms exist for the three-wave fp16 x2 kernel on 128-row tiles, the 32x32x16 form for two waves");
    // merged output phases: blockIdx.z = phase * B + sample; the phase's grid, output offset and taps replace the launch-wide ones
    LaConvArgs a = a_in;
    int bz = blockIdx.z;
    int bx = blockIdx.x;
    if (a_in.nphase > 0) {
        int ph;
        if (SPLIT) {      // split-K form: blockIdx.x walks the phases' tiles back to back, blockIdx.z stays the K slice
            ph = 0;
#pragma unroll
            for (int q = 1; q < LA_CONV_MAX_PHASES; ++q)
                if (q < a_in.nphase && bx >= a_in.ph[q].tile0) ph = q;
            bx -= a_in.ph[ph].tile0;
            a.splitk_ws = a_in.splitk_ws + a_in.ph[ph].ws_off;
        } else {
            ph = bz / a_in.B;
            bz -= ph * a_in.B;
        }
        a.Gy = a_in.ph[ph].Gy; a.Gx = a_in.ph[ph].Gx; a.out_oy = a_in.ph[ph].out_oy; a.out_ox = a_in.ph[ph].out_ox; a.ntaps = a_in.ph[ph].ntaps;
#pragma unroll
        for (int t = 0; t < LA_CONV_PHASE_TAPS; ++t) { a.tap_dy[t] = a_in.ph[ph].tap_dy[t]; a.tap_dx[t] = a_in.ph[ph].tap_dx[t]; a.tap_w[t] = a_in.ph[ph].tap_w[t]; }
    }
    constexpr int NTERM = FMT == FMT_BF16X3 ? 3 : 2;
    constexpr bool F16 = FMT == FMT_F16X2;
    constexpr int WM_ = MT == 128 ? 4 : 2;         // wave grid WM_ x WN_ over the MT x 128 tile: every wave owns 32 rows
    constexpr int WN_ = 4 / WM_;                   // (128-row tiles: 4 x 1, no weight fragment is loaded by two waves)
    constexpr int TM = 1;
    constexpr int NJ = 4 / WN_;                    // 32-pixel MFMA tiles per wave
    constexpr int EB = F16 ? 4 : 8;                // bytes per pre-split element
    constexpr int BPLANE = NT * BPITCH;            // one term of one pixel buffer
    constexpr int BBUF = NTERM * BPLANE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [2][NTERM][NT][BPITCH]
    float (*red)[MT] = reinterpret_cast<float (*)[MT]>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN_, wn = wid % WN_;
    // XCD-aware tile order (direct mode): workgroups are dealt round-robin over the 8 XCDs, so give each XCD a contiguous
    // run of pixel tiles -- vertically adjacent tiles (which share the +-1 row halos of the 3x3 taps) then hit the same L2.
    int ntile = bx;
    const int m0 = blockIdx.y * MT;
    int G = a.Gy * a.Gx;
    int goy = 0, gox = 0;      // origin of the part of the grid that the tiles are flattened over (column window: the wanted rectangle)
    if (!SPLIT) {
        // row window (LaConvArgs::row_lo): the tiles that hold a wanted row are a contiguous run [t0, t0 + nt) of the flattened tiles; the
        // first nt workgroups of the launch take them (in the XCD-aware order below, so the run is spread over all XCDs), the rest return
        int t0 = 0, nt = (int)gridDim.x;
        if (a.row_hi > 0 && a.col_hi > 0) {
            // row and column window (LaConvArgs::col_lo): the launch's grid IS the rectangle rows [row_lo, row_hi) x columns [col_lo, col_hi) of
            // this phase's grid -- its tiles 0 .. nt - 1 are flattened over the rectangle's own rows, so a tile holds wanted pixels only (at
            // 128 columns every 128-pixel tile of whole rows would touch the wanted columns).  From here on a.Gy / a.Gx / a.out_oy / a.out_ox
            // describe the rectangle: the epilogue needs nothing else, the loader adds the origin to its input coordinates.
            const int tall = (G + NT - 1) / NT;
            const int r1 = a.row_hi < a.Gy ? a.row_hi : a.Gy, c1 = a.col_hi < a.Gx ? a.col_hi : a.Gx;
            const int nr = r1 > a.row_lo ? r1 - a.row_lo : 0, wc = c1 > a.col_lo ? c1 - a.col_lo : 0;
            nt = (nr * wc + NT - 1) / NT;
            // the partials of the tile slots past the rectangle's (the style finish sums every slot of the whole grid) ...
            for (int j = nt + (int)blockIdx.x; j < tall; j += (int)gridDim.x) la_conv_zero_partials<MT>(a, bz, m0, j);
            // ... and, backward, the gradient in the columns left out: exact zeros for the contraction that reads these rows next (its loader
            // masks rows, not columns; the buffer holds another layer's gradient there).  Dense output, grid = output plane.
            if (a.epi == LA_EPI_BWD && wc < a.Gx) {
                const int ns = a.Gx - wc, per_m = nr * ns, mrows = a.M - m0 < MT ? a.M - m0 : MT;
                float* ob = a.out + ((long)bz * a.M + m0) * a.Hout * a.Wout + (long)a.row_lo * a.Wout;
                for (int e = (int)blockIdx.x * 256 + (int)threadIdx.x; e < mrows * per_m; e += (int)gridDim.x * 256) {
                    const int m = e / per_m, rem = e - m * per_m, r = rem / ns, c = rem - r * ns;
                    ob[(long)m * a.Hout * a.Wout + (long)r * a.Wout + (c < a.col_lo ? c : c + wc)] = 0.f;
                }
            }
            const int n8 = (int)gridDim.x;
            if ((n8 & 7) == 0) ntile = (blockIdx.x & 7) * (n8 >> 3) + (blockIdx.x >> 3);
            if (ntile >= nt) return;
            goy = a.row_lo; gox = a.col_lo;
            a.out_oy += goy * a.out_sy; a.out_ox += gox * a.out_sx;
            a.Gy = nr; a.Gx = wc; G = nr * wc;
        } else if (a.row_hi > 0) {
            // (round 5, as the halo kernel: the launch holds the window's tiles only, rounded up to a multiple of eight -- for merged phases
            //  those of the phase with the most -- and its workgroups zero the partials of the tiles outside the window in turn)
            const int tall = (G + NT - 1) / NT;
            t0 = (a.row_lo * a.Gx) / NT;
            int t1 = ((a.row_hi < a.Gy ? a.row_hi : a.Gy) * a.Gx + NT - 1) / NT;
            t1 = t1 < tall ? t1 : tall;
            nt = t1 - t0;
            for (int j = (int)blockIdx.x; j < tall - nt; j += (int)gridDim.x) la_conv_zero_partials<MT>(a, bz, m0, j < t0 ? j : j + nt);
            const int n8 = (int)gridDim.x;
            if ((n8 & 7) == 0) ntile = (blockIdx.x & 7) * (n8 >> 3) + (blockIdx.x >> 3);
            if (ntile >= nt) return;
        } else if ((nt & 7) == 0) ntile = (blockIdx.x & 7) * (nt >> 3) + (blockIdx.x >> 3);
        ntile += t0;
    }
    const int Ntot = SPLIT ? a.B * G : G;
    if (!SPLIT && (long)ntile * NT >= G) return;          // merged phases: the launch is sized for the largest phase
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- loader role: thread = (pixel n_l, 16-channel half khalf)
    const int n_l = tid & (NT - 1);
    const int khalf = tid >> 7;
    const int nidx_l = ntile * NT + n_l;
    const bool nvalid = nidx_l < Ntot;
    const int b_l = SPLIT ? (nvalid ? nidx_l / G : 0) : bz;
    const int g_l = SPLIT ? nidx_l - b_l * G : nidx_l;
    const int gy_l = nvalid ? g_l / a.Gx : 0;
    const int gx_l = nvalid ? g_l - gy_l * a.Gx : 0;
    const int iy0 = (gy_l + goy) * a.in_sy, ix0 = (gx_l + gox) * a.in_sx;
    const unsigned HWin = (unsigned)(a.Hin * a.Win);
    const int vy0 = a.in_row_hi > 0 ? a.in_row_lo : 0, vy1 = a.in_row_hi > 0 ? a.in_row_hi : a.Hin;      // valid input rows (LaConvArgs::in_row_lo)
    // fp16 pieces: load k of a thread is the 16-byte piece tid & 7 of the 128-byte record of pixel k * 32 + (tid >> 3) -- pieces 0-3 are
    // the h terms of channels 0-7 / 8-15 / 16-23 / 24-31 of the chunk, pieces 4-7 their l terms (la_presplit_t_kernel, la_fir4x4_adj_pack) --
    // so that the 8 lanes of a pixel read its whole record (a wave instruction touches 8 lines instead of 64) and a piece IS one 16-byte
    // LDS slot of one term: no unpacking between the load and the LDS write.
    // Pixel-stationary addressing (as the halo kernel's loader): the record offset of the un-shifted pixel and the set of taps that fall
    // outside the image are computed ONCE per piece; per step the tap adds a scalar to the offset and an out-of-image tap turns it
    // into an out-of-range buffer offset, which the hardware reads as zeros -- 3 vector instructions per piece and step (was ~25:
    // clamps, comparisons, a 64-bit multiply-add and a select per value).
    constexpr bool PIECES = FMT == FMT_F16X2;
    constexpr unsigned OOB = 0x7ff00000u;          // >= every operand size (checked by la_conv_prepare_input)
    unsigned plin[4] = {0u, 0u, 0u, 0u}, pinv[4] = {0u, 0u, 0u, 0u};
    if constexpr (PIECES) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int n_k = k * 32 + (tid >> 3);
            const int nidx = ntile * NT + n_k;
            const bool pv = nidx < Ntot;
            const int bb = SPLIT ? (pv ? nidx / G : 0) : bz;
            const int g = SPLIT ? nidx - bb * G : nidx;
            const int gy = pv ? g / a.Gx : 0, gx = pv ? g - gy * a.Gx : 0;
            const int py = (gy + goy) * a.in_sy, px = (gx + gox) * a.in_sx;
            const unsigned base = (SPLIT ? (unsigned)bb * ((unsigned)((a.C + KCB - 1) / KCB) * KCB * HWin * 4u) : 0u) + (unsigned)(tid & 7) * 16u;
            plin[k] = base + (unsigned)(py * a.Win + px) * (unsigned)(KCB * EB);
            unsigned m = 0u;
#pragma unroll
            for (int t = 0; t < LA_CONV_MAX_TAPS; ++t) {
                const int iy = py + a.tap_dy[t], ix = px + a.tap_dx[t];
                const bool bad = !pv || iy < vy0 || iy >= vy1 || ix < 0 || ix >= a.Win;
                m |= (bad ? 1u : 0u) << t;
            }
            pinv[k] = m;
        }
    }

    const int nck = (a.C + KCB - 1) / KCB;
    int ck_beg = 0, ck_end = nck;
    if (SPLIT) {
        const int per = (nck + a.ksplit - 1) / a.ksplit;
        ck_beg = blockIdx.z * per;
        ck_end = ck_beg + per < nck ? ck_beg + per : nck;
    }
    const int ntaps = a.ntaps;
    const int nstep = ck_end > ck_beg ? (ck_end - ck_beg) * ntaps : 0;
    const long term_elems = a.wgt_bf16_term_elems;
    // buffer descriptors (wave-uniform).  Direct mode: this sample's pre-split input; split-K: the whole batch.
    // pre-split layout: [b][chunk][pixel][32 channels] -> a gather thread reads 16 contiguous channels of its pixel
    const unsigned samp_bytes = (unsigned)nck * KCB * HWin * EB;
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(static_cast<const char*>(a.in_q)) + (SPLIT ? (size_t)0 : (size_t)bz * samp_bytes), 0,
        (int)(SPLIT ? samp_bytes * (unsigned)a.B : samp_bytes), 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(static_cast<const char*>(a.wgt_bf16)) + (F16 ? pack_f16_offset(term_elems) : 0), 0, (int)(NTERM * term_elems * 2),
        0x00020000);
    const unsigned lane_base = (SPLIT ? (unsigned)b_l * samp_bytes : 0u) + (unsigned)(khalf * 16) * EB;

    // tap table -> packed scalars (offsets are within +-7), so the step loop needs no indexed kernarg reads
    unsigned long long dypack = 0ull, dxpack = 0ull, wpack = 0ull;
#pragma unroll
    for (int t = 0; t < LA_CONV_MAX_TAPS; ++t) {
        dypack |= (unsigned long long)((a.tap_dy[t] + 8) & 15) << (4 * t);
        dxpack |= (unsigned long long)((a.tap_dx[t] + 8) & 15) << (4 * t);
        wpack |= (unsigned long long)(a.tap_w[t] & 15) << (4 * t);
    }

    // ---- B gather of one step: 16 channels of this thread's pixel = 64 / 128 contiguous bytes
    unsigned ex[16], ey[NTERM == 3 ? 16 : 1];
    bool ok_r = false;
    auto load_b = [&](int cc, int t) {
        if constexpr (PIECES) {
            const int dy = (int)((dypack >> (4 * t)) & 15u) - 8, dx = (int)((dxpack >> (4 * t)) & 15u) - 8;
            const unsigned delta = (unsigned)((dy * a.Win + dx) * (KCB * EB));      // (scalar)
            const unsigned so = (unsigned)cc * HWin * (KCB * EB);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int bad = __builtin_amdgcn_sbfe((int)pinv[k], (unsigned)t, 1u);      // -1: the tap is outside the image for this piece
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (plin[k] + delta) | ((unsigned)bad & OOB), so, 0);
                ex[4 * k] = v.x; ex[4 * k + 1] = v.y; ex[4 * k + 2] = v.z; ex[4 * k + 3] = v.w;
            }
            return;
        }
        const int iy = iy0 + (int)((dypack >> (4 * t)) & 15u) - 8, ix = ix0 + (int)((dxpack >> (4 * t)) & 15u) - 8;
        ok_r = nvalid && iy >= vy0 && iy < vy1 && ix >= 0 && ix < a.Win;
        const int iyc = iy < 0 ? 0 : (iy >= a.Hin ? a.Hin - 1 : iy), ixc = ix < 0 ? 0 : (ix >= a.Win ? a.Win - 1 : ix);
        const unsigned vo = lane_base + (unsigned)(iyc * a.Win + ixc) * (KCB * EB);
        const unsigned so = (unsigned)cc * HWin * (KCB * EB);
        if (NTERM == 3) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_in, vo, so + 16 * k, 0);
                ex[2 * k] = v.x; ey[NTERM == 3 ? 2 * k : 0] = v.y; ex[2 * k + 1] = v.z; ey[NTERM == 3 ? 2 * k + 1 : 0] = v.w;
            }
        } else if (F16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_in, vo, so + 16 * k, 0);
                ex[4 * k] = v.x; ex[4 * k + 1] = v.y; ex[4 * k + 2] = v.z; ex[4 * k + 3] = v.w;
            }
        } else {      // 2 bf16 terms: the {h | m} words of the 8-byte elements
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_in, vo, so + 16 * k, 0);
                ex[2 * k] = v.x; ex[2 * k + 1] = v.z;
            }
        }
    };
    const int wrow = n_l * BPITCH, wsw = (n_l >> 2) & 3;
    auto write_b = [&](unsigned char* buf) {
        if constexpr (PIECES) {      // piece (tid & 7) = slot (tid & 3) of term (tid >> 2 & 1); the tile row only adds k * 32 rows
            const int wsw = MF != FLAT_MF_32 ? ((tid >> 5) & 1) << 1 : (tid >> 5);      // slot swizzle of pixel k * 32 + (tid >> 3): by (pixel >> 2) & 3, MF: 2 * ((pixel >> 2) & 1)
            unsigned char* p0 = buf + ((tid >> 2) & 1) * BPLANE + (tid >> 3) * BPITCH + ((((tid & 3) ^ wsw) & 3) << 4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                *reinterpret_cast<uint4*>(p0 + k * 32 * BPITCH) = make_uint4(ex[4 * k], ex[4 * k + 1], ex[4 * k + 2], ex[4 * k + 3]);
            return;
        }
#pragma unroll
        for (int q = 0; q < NTERM; ++q) {
            const unsigned sel = q == 1 ? 0x07060302u : 0x05040100u;
            unsigned w[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const unsigned e0 = q == 2 ? ey[NTERM == 3 ? 2 * d : 0] : ex[2 * d];
                const unsigned e1 = q == 2 ? ey[NTERM == 3 ? 2 * d + 1 : 0] : ex[2 * d + 1];
                const unsigned v = __builtin_amdgcn_perm(e1, e0, sel);
                w[d] = ok_r ? v : 0u;
            }
            unsigned char* p = buf + q * BPLANE + wrow;
            *reinterpret_cast<uint4*>(p + ((((khalf * 2) ^ wsw) & 3) << 4)) = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint4*>(p + ((((khalf * 2 + 1) ^ wsw) & 3) << 4)) = make_uint4(w[4], w[5], w[6], w[7]);
        }
    };
    // B fragments: lane (l31, lh) of N-subtile j reads slot ks*2 + lh of row (wn*NJ + j)*32 + l31
    const int rsw = (l31 >> 2) & 3;
    const int rbase = (wn * NJ * 32 + l31) * BPITCH;
    auto read_b = [&](const unsigned char* buf, int ks, bf16x8 (&dst)[NTERM][NJ]) {
        const int o = rbase + ((((ks * 2 + lh) ^ rsw) & 3) << 4);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < NTERM; ++q) dst[q][j] = *reinterpret_cast<const bf16x8*>(buf + q * BPLANE + j * 32 * BPITCH + o);
    };

    // ---- A fragments straight from the fragment-order pack (blocks past M are clamped: their rows are never stored)
    const int Mp = pack_mp(a.M);
    unsigned a_off[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int mblk = (m0 + wm * (MT / WM_) + i * 32) >> 5;
        mblk = mblk < (Mp >> 5) ? mblk : (Mp >> 5) - 1;
        a_off[i] = (unsigned)mblk * 2048u + (unsigned)lane * 16u;
    }
    const unsigned slab_bytes = (unsigned)Mp * KCB * 2u;         // one (tap, chunk) slab of one term
    const unsigned term_bytes = (unsigned)term_elems * 2u;
    auto load_a = [&](int cc, int t, int ks, bf16x8 (&dst)[NTERM][TM]) {
        const unsigned tw = (unsigned)((wpack >> (4 * t)) & 15u);
        const unsigned so = (tw * nck + cc) * slab_bytes + ks * 1024;
#pragma unroll
        for (int q = 0; q < NTERM; ++q)
#pragma unroll
            for (int i = 0; i < TM; ++i)
                dst[q][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, a_off[i], so + q * term_bytes, 0));
    };

    f32x16 acc[TM][NJ];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto mma_step = [&](bf16x8 (&af)[NTERM][TM], bf16x8 (&bf)[NTERM][NJ]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // smallest products first, so they are not swamped by the leading term inside the accumulator
                if constexpr (NTERM == 3) {
                    acc[i][j] = la_mma<F16>(af[2][i], bf[0][j], acc[i][j]);   // lh
                    acc[i][j] = la_mma<F16>(af[0][i], bf[2][j], acc[i][j]);   // hl
                    acc[i][j] = la_mma<F16>(af[1][i], bf[1][j], acc[i][j]);   // mm
                }
                acc[i][j] = la_mma<F16>(af[1][i], bf[0][j], acc[i][j]);   // mh
                acc[i][j] = la_mma<F16>(af[0][i], bf[1][j], acc[i][j]);   // hm
                acc[i][j] = la_mma<F16>(af[0][i], bf[0][j], acc[i][j]);   // hh
            }
    };

    if constexpr (MF != FLAT_MF_32) {
      const int c16 = lane & 15, kq = lane >> 4;
      f32x4 acc16[2][8];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int n = 0; n < 8; ++n) acc16[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (nstep > 0) {
        int c1 = ck_beg, t1 = 0;
        auto adv = [&](int& c, int& t) { la_step_adv(c, t, ntaps, ck_end); };
        int mblk16 = (m0 + wm * 32) >> 5;
        mblk16 = mblk16 < (Mp >> 5) ? mblk16 : (Mp >> 5) - 1;
        const unsigned a16_off = (unsigned)mblk16 * 2048u + (unsigned)(kq * 32 + c16) * 16u;
        auto load_a16 = [&](int cc, int t, int mi, f16x8 (&dst)[2]) {
            const unsigned tw = (unsigned)((wpack >> (4 * t)) & 15u);
            const unsigned so = (tw * nck + cc) * slab_bytes;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                dst[q] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, a16_off + (unsigned)mi * 256u, so + q * term_bytes, 0));
        };
        const int rb16 = c16 * BPITCH + (((kq ^ (((c16 >> 2) & 1) << 1)) & 3) << 4);      // tile n adds n * 16 rows
        auto read_b16 = [&](const unsigned char* buf, int n, f16x8 (&dst)[2]) {
#pragma unroll
            for (int q = 0; q < 2; ++q) dst[q] = *reinterpret_cast<const f16x8*>(buf + q * BPLANE + n * 16 * BPITCH + rb16);
        };
        f16x8 a16[2][2], b16[4][2];
        // Prologue in the loop's own issue order -- [pieces of the step furthest ahead | weights of rows 0-15 | weights of rows 16-31] are
        // the youngest loads when an iteration starts, on the first entry as on the back edge -- so that the counted waits of the loop hold
        // for both and never fall back to vmcnt(0): with the weights requested first, every step began by waiting for the weight
        // fragments issued just before its barrier.
        const int c0 = c1, t0 = t1;
      if constexpr (MF == FLAT_MF_16_3BUF) {
        load_b(c0, t0);
        adv(c1, t1);                                   // (c1, t1) = step 1
        int c2 = c1, t2 = t1;
        write_b(smem);                                 // step 0 -> buffer 0
        __builtin_amdgcn_sched_barrier(0);
        load_b(c1, t1);
        adv(c2, t2);                                   // (c2, t2) = step 2
        write_b(smem + BBUF);                          // step 1 -> buffer 1
        __builtin_amdgcn_sched_barrier(0);
        load_b(c2, t2);                                // step 2: written by iteration 0
        __builtin_amdgcn_sched_barrier(0);
        load_a16(c0, t0, 0, a16[0]);
        __builtin_amdgcn_sched_barrier(0);
        load_a16(c0, t0, 1, a16[1]);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        adv(c2, t2);                                   // (c2, t2) = step 3
#pragma unroll
        for (int n = 0; n < 4; ++n) read_b16(smem, n, b16[n]);
        int ib = 0;                                    // buffer of step s
#pragma unroll 1
        for (int s = 0; s < nstep; ++s) {
            const int ib1 = ib == 2 ? 0 : ib + 1, ib2 = ib1 == 2 ? 0 : ib1 + 1;
            const unsigned char* cur = smem + ib * BBUF;
            const unsigned char* nx1 = smem + ib1 * BBUF;
            write_b(smem + ib2 * BBUF);                // step s+2 (loaded during step s-1)
            load_b(c2, t2);                            // step s+3
            __builtin_amdgcn_sched_barrier(0);
            const bool more = s + 1 < nstep;
            // a slot is re-filled with tile k + 4 of this step, then tile k of step s+1 (published by the PREVIOUS barrier); the next step's
            // weights get a quarter step to land.  Round 4 walked all eight tiles per 16-row half and read every fragment twice
            la_quarter_walk(a16, b16, acc16,
                            [&](int hf, int k, f16x8 (&bs)[2]) {
                                if (hf == 0) read_b16(cur, 4 + k, bs);
                                else if (more) read_b16(nx1, k, bs);
                            },
                            [&](int q4) { if (q4 >= 2) load_a16(c1, t1, q4 & 1, a16[q4 & 1]); });      // this half's weights of step s+1
            adv(c1, t1);           // weights run one step ahead, pieces three
            adv(c2, t2);
            ib = ib1;
            __syncthreads();
        }
      } else {
        load_b(c0, t0);
        adv(c1, t1);                                   // (c1, t1) = step 1
        int c2 = c1, t2 = t1;
        write_b(smem);
        __builtin_amdgcn_sched_barrier(0);
        load_b(c1, t1);
        __builtin_amdgcn_sched_barrier(0);
        load_a16(c0, t0, 0, a16[0]);
        __builtin_amdgcn_sched_barrier(0);
        load_a16(c0, t0, 1, a16[1]);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        adv(c2, t2);                                   // (c2, t2) = step 2
#pragma unroll 1
        for (int s = 0; s < nstep; ++s) {
            const unsigned char* cur = smem + (s & 1) * BBUF;
            unsigned char* nxt = smem + ((s + 1) & 1) * BBUF;
#pragma unroll
            for (int n = 0; n < 4; ++n) read_b16(cur, n, b16[n]);
            write_b(nxt);                              // step s+1 (loaded during step s-1)
            load_b(c2, t2);                            // step s+2
            __builtin_amdgcn_sched_barrier(0);
            la_quarter_walk(a16, b16, acc16,
                            [&](int hf, int k, f16x8 (&bs)[2]) { if (hf == 0) read_b16(cur, 4 + k, bs); },
                            [&](int q4) { if (q4 >= 2) load_a16(c1, t1, q4 & 1, a16[q4 & 1]); });      // this half's weights of step s+1
            c1 = c2; t1 = t2;
            adv(c2, t2);
            __syncthreads();
        }
      }
      }
      // 16x16 tiles -> the 32x32 accumulator layout of the epilogue through LDS (free after the last barrier), two 32-pixel blocks at a time
      {
        float* tb = reinterpret_cast<float*>(smem) + wid * (64 * 36);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            if (hf) __syncthreads();
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int n4 = 0; n4 < 4; ++n4) {
                    const int n = hf * 4 + n4;
                    *reinterpret_cast<f32x4*>(tb + (n4 * 16 + c16) * 36 + mi * 16 + kq * 4) = acc16[mi][n];
                }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(tb + (jj * 32 + l31) * 36 + 8 * g + 4 * lh);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][hf * 2 + jj][4 * g + r] = v[r];
                }
        }
        __syncthreads();
      }
    } else
    if (nstep > 0) {
        // (chunk, tap) of steps s, s+1, s+2; past the end they stay on the last valid step (harmless re-loads)
        int c1 = ck_beg, t1 = 0;
        auto adv = [&](int& c, int& t) { la_step_adv(c, t, ntaps, ck_end); };
        bf16x8 acur[2][NTERM][TM], anxt[2][NTERM][TM], bf0[NTERM][NJ], bf1[NTERM][NJ];
        // (prologue in the loop's issue order -- pixel loads of the step after next, then the weight loads -- so that the loop's
        //  waits are exact counts on both of its entries: see the 16x16x32 forms above)
        const int c0 = c1, t0 = t1;
        load_b(c0, t0);
        adv(c1, t1);                                   // (c1, t1) = step 1
        int c2 = c1, t2 = t1;
        write_b(smem);
        __builtin_amdgcn_sched_barrier(0);
        load_b(c1, t1);
        __builtin_amdgcn_sched_barrier(0);
        load_a(c0, t0, 0, acur[0]);
        load_a(c0, t0, 1, acur[1]);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        adv(c2, t2);                                   // (c2, t2) = step 2
#pragma unroll 1
        for (int s = 0; s < nstep; ++s) {
            const unsigned char* cur = smem + (s & 1) * BBUF;
            unsigned char* nxt = smem + ((s + 1) & 1) * BBUF;
            // (the fences pin the issue order: left alone, the scheduler sinks every load to just before its first use)
            read_b(cur, 0, bf0);
            read_b(cur, 1, bf1);
            write_b(nxt);                              // step s+1 (loaded during step s-1)
            load_b(c2, t2);                            // step s+2
            load_a(c1, t1, 0, anxt[0]);                // weights of step s+1: a full step ahead (they may come from beyond L2)
            load_a(c1, t1, 1, anxt[1]);
            __builtin_amdgcn_sched_barrier(0);
            mma_step(acur[0], bf0);
            mma_step(acur[1], bf1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int q = 0; q < NTERM; ++q)
#pragma unroll
                    for (int i = 0; i < TM; ++i) acur[ks][q][i] = anxt[ks][q][i];
            c1 = c2; t1 = t2;
            adv(c2, t2);
            __syncthreads();
        }
    }
    if (F16) {
        // undo the power-of-two operand scales (exact)
        const float iw = 1.f / a.acc_scale_w[0];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            int bb = bz;
            if (SPLIT) { const int nidx = ntile * NT + (wn * NJ + j) * 32 + l31; bb = nidx < Ntot ? nidx / G : 0; }
            const float inv = iw / la_xs_get(a.acc_scale_x, bb, a.acc_scale_fan);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] *= inv;
        }
    }
    la_conv_epilogue<MT, SPLIT, false, WM_>(a, acc, red, ntile, m0, G, Ntot, SPLIT ? -1 : bz);
}

template <int FMT>
static int launch_flat(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream) {
    constexpr int NTERM = FMT == FMT_BF16X3 ? 3 : 2;
    const size_t lds = (size_t)2 * NTERM * NT * BPITCH;      // two pixel buffers (>= the epilogue's 4 * MT floats)
    const bool split = p.form == LA_FORM_FLAT_SPLIT;
    if constexpr (FMT == FMT_F16X2) {
        if (p.mfma == LA_CONV_MFMA_16X16X32) {
            // the three-wave 16x16x32 forms (128-row tiles): split-K slices on two pixel buffers (the accumulator hand-over needs 36 KB of
            // LDS), direct launches on three
            const size_t lds_mf = lds > (size_t)4 * 64 * 36 * 4 ? lds : (size_t)4 * 64 * 36 * 4;
            if (split) hipLaunchKernelGGL((la_conv_bf16_kernel<128, true, FMT, 3, FLAT_MF_16>), p.grid, dim3(256), lds_mf, stream, as);
            else hipLaunchKernelGGL((la_conv_bf16_kernel<128, false, FMT, 3, FLAT_MF_16_3BUF>), p.grid, dim3(256), (size_t)3 * NTERM * NT * BPITCH, stream, as);
            return LA_OK;
        }
    } else if (p.mt == 128) {
        if (split) hipLaunchKernelGGL((la_conv_bf16_kernel<128, true, FMT, 2>), p.grid, dim3(256), lds, stream, as);
        else hipLaunchKernelGGL((la_conv_bf16_kernel<128, false, FMT, 2>), p.grid, dim3(256), lds, stream, as);
        return LA_OK;
    }
    if (split) hipLaunchKernelGGL((la_conv_bf16_kernel<64, true, FMT, 2>), p.grid, dim3(256), lds, stream, as);
    else hipLaunchKernelGGL((la_conv_bf16_kernel<64, false, FMT, 2>), p.grid, dim3(256), lds, stream, as);
    return LA_OK;
}

int la_conv_flat_launch(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream) {
    if (as.precision == LA_PREC_BF16X3) return launch_flat<FMT_BF16X3>(as, p, stream);
    if (as.precision == LA_PREC_F16X2) return launch_flat<FMT_F16X2>(as, p, stream);
    return launch_flat<FMT_BF16X2>(as, p, stream);
}
