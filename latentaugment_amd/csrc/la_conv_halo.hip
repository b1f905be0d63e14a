// Halo variant of the 16-bit split contraction (formats, tiling and weight pack: la_conv_operand.hip; shared fragments:
// la_conv_device.h) for dense stride-1 3x3 launches on grids that tile exactly into 4 x 32 pixel tiles (the >= 64x64 layers,
// i.e. the bulk of the FLOPs).  The flat kernel (la_conv_flat.hip) re-gathers every input element once per tap (9x) from L2; here the
// (4+2) x (32+2) halo of a 32-channel chunk is staged in LDS ONCE and the 9 taps read shifted fragments from it.
//   * B (pixels): two halo buffers.  While chunk cc computes, chunk cc+1 streams in, one ninth per tap: each thread loads a
//     4-channel unit, holds it for one tap (4 / 8 registers) and writes it to the other buffer during the next tap, so an
//     HBM miss has a whole tap of MFMAs to land and no wait ever covers more than one tap's loads.  ONE barrier per chunk.
//     Rows are 64 B (32 channels of one term) with the 16-byte slots XOR-swizzled by (pixel >> 2) & 3: conflict-free
//     ds_read_b128 fragments at any tap shift, no padding.
//   * A (weights): never touches LDS.  The pack stores every 32-row x 16-channel block in MFMA fragment order, so a wave
//     loads a fragment with one coalesced 1 KB buffer load; each fragment register is re-loaded for the next tap right
//     after the MFMAs that read it have issued.
// LDS: 2 x 204 px x 64 B x NTERM = 51 / 76.5 KB; registers <= 168 (NTERM = 2: three waves per SIMD) / <= 256.
#include "la_conv_device.h"
#include <atomic>
#include <type_traits>

#define HALO_W 34
#define HALO_PX (6 * HALO_W)
#define HPITCH 64
#define H_UNITS (8 * HALO_PX)          // (4-channel group, halo pixel) load units per chunk
#define H_UPT 182                      // units per tap (9 x 182 >= 1632)
// WV = waves per SIMD the kernel is compiled for.  2: two sets of B fragments (K-step 1 is read under the MFMAs of K-step 0), the chunk
// loop in a with-next and a last instance.  3 (<= 168 registers, three workgroups per CU -- the partner workgroups cover a
// workgroup's prologue and store bursts): ONE set of B fragments, every 32-pixel sub-tile re-loaded for the following K-step right
// after its own three MFMAs, and ONE instance of the chunk loop (the last chunk issues dummy loads): the merge of two instances
// cost a second set of 64 accumulator registers and 64 moves per chunk.  Measured per 154.6-GFLOP launch (WV 3 against 2):
// 128->128 @256^2 fwd -9.5 %, bwd -7 %; 256->256 @128^2 fwd -8 %, bwd -8 %; 512->512 @64^2 +-0 (two rounds of workgroups only) --
// select_halo uses WV 3 for every 128-row launch of the two-term formats.
// MF bits (HALO_MF_*, la_conv_device.h): 4 = pixel-stationary halo loader (PSL, below); 1 = v_mfma_f32_16x16x32_f16 (M16).  Bit 16 is
// part of the value 21 and of the kernel's name, and selects nothing: no code tests it (the 16x16x32 tap loop has one form, which reads
// every pixel fragment once per tap).
// The forms: MF 0 (HALO_MF_BF16) for the bf16 formats; for fp16 x2, MF 21 (HALO_MF_F16_16) on 128-row tiles of launches with more than
// one chunk and MF 4 (HALO_MF_F16_32: the loader on the 32x32x16 form) for the others.  MF 21: the same wave tile (32 rows x 128
// pixels) on v_mfma_f32_16x16x32_f16 -- 2 x 8 tiles of 16 x 16, one MFMA per (tile, term pair) over the whole 32-channel chunk; the tap
// is walked in quarters (tap loop below).  Same weight pack (a 16-row fragment is four 256-byte pieces of the 32-row block), LDS slots
// swizzled by 2 * ((column >> 2) & 1) (conflict-free for this lane map at every tap shift).  The accumulators are brought into the
// 32x32 layout through LDS before the shared epilogue.
#ifdef LA_DEV
// Development build, dev knob LA_KNOB_HALO_STAMP = 1: every wave of the MF 21 halo kernel accumulates s_memtime differences per segment
// (prologue issue / prologue wait + first stage / tap loops / chunk barriers / accumulator hand-over / epilogue) in scalar registers and
// leaves them in la_dbg_buf[wave][16] (la_dev_dbg_read); segments 6-8 are stamped inside the epilogue (la_conv_device.h, LA_ESTAMP).  scripts/halo_wave_timeline.py
__device__ unsigned long long la_dbg_buf[1 << 18];
#define LA_STAMP_DECL LaStamp stv; stv.on = a.dbg_stamp != 0; stv.last = 0ull; for (int i_ = 0; i_ < 12; ++i_) stv.seg[i_] = 0ull; if (stv.on) stv.last = __builtin_amdgcn_s_memtime();
#define LA_STAMP(i) do { if (stv.on) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); stv.seg[i] += t_ - stv.last; stv.last = t_; } } while (0)
#define LA_STAMP_ARG , -1, &stv
#define LA_STAMP_OUT do { if (stv.on && (threadIdx.x & 63) == 0) { const long wv_ = ((long)blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z)) * 4 + (threadIdx.x >> 6); \
    if (wv_ * 16 + 16 <= (1 << 18)) { for (int i_ = 0; i_ < 12; ++i_) la_dbg_buf[wv_ * 16 + i_] = stv.seg[i_]; la_dbg_buf[wv_ * 16 + 12] = stv.last; \
    unsigned hw_, xcc_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_)); \
    la_dbg_buf[wv_ * 16 + 13] = hw_; la_dbg_buf[wv_ * 16 + 14] = xcc_; } } } while (0)
extern "C" int la_dev_dbg_read(unsigned long long* dst, long n) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(la_dbg_buf), (size_t)n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#else
#define LA_STAMP_DECL
#define LA_STAMP(i)
#define LA_STAMP_ARG
#define LA_STAMP_OUT
#endif
template <int MT, int FMT, int WV, int MF = HALO_MF_BF16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WV))) void la_conv_bf16_halo_kernel(LaConvArgs a) {
    constexpr bool SB = WV == 3;
    constexpr bool M16 = (MF & HALO_MF_M16) != 0, PSL = (MF & HALO_MF_PSL) != 0;
    static_assert(MF == HALO_MF_BF16 ? FMT != FMT_F16X2 : (MF == HALO_MF_F16_32 || MF == HALO_MF_F16_16) && FMT == FMT_F16X2,
                  "MF 0 for the bf16 formats, MF 4 / 21 for fp16 x2");
    static_assert(!M16 || (MF == HALO_MF_F16_16 && WV == 3 && MT == 128), "the 16x16x32 form (M16) is MF 21: pixel-stationary loader, three waves, 128-row tiles");
    constexpr int NTERM = FMT == FMT_BF16X3 ? 3 : 2;
    constexpr bool F16 = FMT == FMT_F16X2;
    constexpr int WM_ = MT / 32;                   // wave grid WM_ x WN_ over the MT x 128 tile: every wave owns 32 rows
    constexpr int WN_ = 4 / WM_;                   // (128-row tiles: 4 x 1, no weight fragment is loaded by two waves; 32-row tiles
                                                   //  for the 32-channel layers of the 1024^2 generators: 1 x 4)
    constexpr int NJ = 4 / WN_;                    // 32-pixel MFMA tiles (= tile rows) per wave
    constexpr int EB = 4;                          // the halo kernel reads the fp32 input itself
    constexpr int HPLANE = HALO_PX * HPITCH;       // one term of one halo buffer
    constexpr int HBUF = NTERM * HPLANE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [2][NTERM][HALO_PX][HPITCH] + scl[nck*32]
    float (*red)[MT] = reinterpret_cast<float (*)[MT]>(smem);
    // per-channel factor (style modulation x fp16 sample scale) behind the halo buffers; a single-chunk launch (<= 32 input channels: the
    // top layers of the 1024^2 generators) never stages a second chunk and gets ONE buffer, i.e. twice the workgroups per CU
    float* scl = reinterpret_cast<float*>(smem + (a.C > KCB ? 2 : 1) * HBUF);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN_, wn = wid % WN_;
    const int tpr = a.Gx >> 5;
    // row window (LaConvArgs::row_lo): the 4-row tiles that hold a wanted row are the run [t0, t0 + nt) of the row-major tile order; the
    // first nt workgroups of the launch take them -- in the XCD-aware order, so that the run is spread over all eight XCDs (a test on the
    // tile row alone left the XCDs that own the top and the bottom of the frame idle and the launch as long as before) -- the rest return
    // Round 5: the launch holds the window's tiles ONLY, rounded up to a multiple of eight workgroups (la_conv_window_tiles; round 4 launched
    // a workgroup per tile of the whole frame and let those outside the window return: a launch with 1 104 wanted tiles of 2 048 took
    // ~30 us longer than the wanted tiles alone).  Workgroup x of the launch takes tile (x & 7) * (n8 / 8) + (x >> 3) of the window's
    // row-major run -- a contiguous run of tiles per XCD whatever the tile count (round 4 fell back to the plain order whenever the
    // count was not a multiple of eight: the 256^2 and 64^2 windows of config B) -- and the per-tile partials of the tiles outside
    // the window, which the one-pass style finish sums, are zeroed by the launch's workgroups in turn.
    int nt = (int)gridDim.x;
    int r0 = 0, c0 = 0, cw = tpr;                 // window rectangle in tiles: rows [r0, r1), columns [c0, c0 + cw)
    int ntile = blockIdx.x;
    if (a.row_hi > 0) {
        const int r1 = ((a.row_hi < a.Gy ? a.row_hi : a.Gy) + 3) >> 2;
        r0 = a.row_lo >> 2;
        if (a.col_hi > 0) { c0 = a.col_lo >> 5; cw = (((a.col_hi < a.Gx ? a.col_hi : a.Gx) + 31) >> 5) - c0; }
        nt = (r1 - r0) * cw;
        const int tall = (a.Gy >> 2) * tpr, n_out = tall - nt;
        for (int j = (int)blockIdx.x; j < n_out; j += (int)gridDim.x) {      // tiles outside the window, in row-major order
            int otile, k = j;
            const int per = tpr - cw;             // outside tiles per window row
            if (k < r0 * tpr) otile = k;
            else if ((k -= r0 * tpr) < (r1 - r0) * per) { const int rr = k / per, kk = k - rr * per; otile = (r0 + rr) * tpr + (kk < c0 ? kk : kk + cw); }
            else otile = r1 * tpr + (k - (r1 - r0) * per);
            la_conv_zero_partials<MT>(a, (int)blockIdx.z, (int)blockIdx.y * MT, otile);
        }
        const int n8 = (int)gridDim.x;            // (host: the window's tile count rounded up to a multiple of 8, or the whole frame's)
        if ((n8 & 7) == 0) {
            // eight runs of tiles, one per XCD, as even as the count allows (nt = 8 q + r: the first r runs hold q + 1 tiles); the run an
            // XCD takes rotates with the sample, so that over the samples of a launch every XCD sees long and short runs alike (the
            // 28-tile window at 64^2 with one fixed run per XCD: 4 4 4 4 4 4 4 0 tiles per sample; rotated: 28 per XCD over 8 samples)
            const int q = nt >> 3, r = nt & 7, rot = gridDim.z >= 8 ? 1 : (gridDim.z >= 4 ? 2 : (gridDim.z >= 2 ? 4 : 0));
            const int kv = (int)((blockIdx.x + blockIdx.z * rot) & 7), idx = (int)(blockIdx.x >> 3);
            if (idx >= q + (kv < r ? 1 : 0)) return;
            ntile = kv * q + (kv < r ? kv : r) + idx;
        } else if (ntile >= nt) return;
        const int rr = ntile / cw;
        ntile = (r0 + rr) * tpr + c0 + (ntile - rr * cw);
    } else if ((nt & 7) == 0) ntile = (blockIdx.x & 7) * (nt >> 3) + (blockIdx.x >> 3);   // XCD-contiguous tile runs
    const int m0 = blockIdx.y * MT;
    const int b = blockIdx.z;
    const int G = a.Gy * a.Gx;
    const int tyb = ntile / tpr, txb = ntile - tyb * tpr;
    const int y0 = tyb * 4 - 1, x0 = txb * 32 - 1;              // grid coordinates of halo pixel (0, 0)
    const unsigned HWin = (unsigned)(a.Hin * a.Win);
    const int vy0 = a.in_row_hi > 0 ? a.in_row_lo : 0, vy1 = a.in_row_hi > 0 ? a.in_row_hi : a.Hin;      // valid input rows (LaConvArgs::in_row_lo)
    const int nck = (a.C + KCB - 1) / KCB;
    const int l31 = lane & 31, lh = lane >> 5;
    // buffer descriptor (wave-uniform): this sample's fp32 input
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.in) + (size_t)b * a.in_bstride, 0, (int)((unsigned)a.C * HWin * EB), 0x00020000);

    // tap table -> packed scalars, so the tap loop needs no indexed kernarg reads
    unsigned long long shpack = 0ull, wpack = 0ull;
    unsigned xpack = 0u;                       // 1 + dx of every tap (PSL: the LDS slot swizzle follows the halo COLUMN)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        shpack |= (unsigned long long)((1 + a.tap_dy[t]) * HALO_W + (1 + a.tap_dx[t])) << (7 * t);
        wpack |= (unsigned long long)a.tap_w[t] << (4 * t);
        xpack |= (unsigned)(1 + a.tap_dx[t]) << (2 * t);
    }

    // ---- halo slices (the loader of MF 0, i.e. of the bf16 formats).  Every load is unconditional (clamped address; out-of-image
    // pixels are zeroed on the way to LDS, channels past C meet zero weights), so the compiler can count them: no wait in the tap
    // loop is a vmcnt(0).
    struct Slice { float x[4]; int wr, c0; bool ok; };
    auto slice_load = [&](int cc, int t, Slice& sl, bool live = true) {      // !live (uniform): one dword of traffic per wave, nothing written
        const int lt = (tid + 64 * t) & 255;                      // the idle lanes rotate over the waves
        int u = t * H_UPT + (lt < H_UPT ? lt : H_UPT - 1);
        const bool valid = live && lt < H_UPT && u < H_UNITS;
        u = u < H_UNITS ? u : H_UNITS - 1;
        const int c4 = u / HALO_PX, hp = u - c4 * HALO_PX;
        const int hy = hp / HALO_W, hx = hp - hy * HALO_W;
        const int iy = y0 + hy, ix = x0 + hx;
        sl.ok = iy >= vy0 && iy < vy1 && ix >= 0 && ix < a.Win;
        const int iyc = iy < 0 ? 0 : (iy >= a.Hin ? a.Hin - 1 : iy), ixc = ix < 0 ? 0 : (ix >= a.Win ? a.Win - 1 : ix);
        const unsigned off = (unsigned)(iyc * a.Win + ixc) * EB;
        const int swz = hp >> 2;
        sl.wr = valid ? hp * HPITCH + ((((c4 >> 1) ^ swz) & 3) << 4) + (c4 & 1) * 8 : -1;
        sl.c0 = cc * KCB + c4 * 4;
        const bool fast = cc * KCB + KCB <= a.C;                  // uniform: only a ragged last chunk clamps channels
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned vo, so;
            if (fast) { vo = live ? (unsigned)(c4 * 4) * HWin * EB + off : 0u; so = live ? (unsigned)(cc * KCB + j) * HWin * EB : 0u; }
            else {
                const int c = cc * KCB + c4 * 4 + j;
                vo = (unsigned)(c < a.C ? c : a.C - 1) * HWin * EB + off;
                so = 0u;
            }
            sl.x[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_in, vo, so, 0));
        }
    };
    // modulate (+ scale), split into NTERM 16-bit terms (each the rounding of the remainder), 8 bytes per term
    auto slice_write = [&](unsigned char* buf, const Slice& sl) {
        if (sl.wr >= 0) {
            // (2-wide vector types so that the packed v_cvt_pk_* / v_pk_* instructions are selected)
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            const float4 f = *reinterpret_cast<const float4*>(scl + sl.c0);
            // (scalar fp32 arithmetic, only the conversions are packed: no v_pk_*_f32, Makefile)
            float p[4] = {sl.x[0] * f.x, sl.x[1] * f.y, sl.x[2] * f.z, sl.x[3] * f.w};
#pragma unroll
            for (int q = 0; q < NTERM; ++q) {
                const bf16x2_t h0 = __builtin_convertvector(f32x2{p[0], p[1]}, bf16x2_t), h1 = __builtin_convertvector(f32x2{p[2], p[3]}, bf16x2_t);
                const uint2 w = make_uint2(__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1));
                if (q + 1 < NTERM) { p[0] -= (float)h0[0]; p[1] -= (float)h0[1]; p[2] -= (float)h1[0]; p[3] -= (float)h1[1]; }
                *reinterpret_cast<uint2*>(buf + q * HPLANE + sl.wr) = sl.ok ? w : make_uint2(0u, 0u);
            }
        }
    };

    // ---- pixel-stationary form of the halo loader (PSL: the fp16 x2 forms).  The slices above give every thread a different (channel
    // group, halo pixel) unit in every tap and recompute its image position, clamps and LDS slot from scratch: ~45 integer instructions
    // per tap and thread (five of them quarter-rate 32-bit multiplies) beside the MFMAs.  Here thread hp < 204 owns halo pixel hp for the whole
    // kernel -- image offset, validity and LDS row are computed ONCE -- and tap t (0..7) stages channel group t of the next chunk
    // for it (tap 8 repeats the loads of tap 0 and drops them, so that every wait in the tap loop stays a counted vmcnt): the channel is
    // wave-uniform, i.e. scalar arithmetic, and what is left per tap are the four loads, the split and one XOR for the LDS slot.
    // With it the 16-byte slots of a pixel row are XOR-swizzled by the halo COLUMN (hx >> 2) instead of the linear pixel index: equally
    // conflict-free (a fragment read covers consecutive columns of one halo row), but the swizzle of a fragment read then depends on
    // the lane and the tap's dx only -- not on the tile row or dy -- so ONE lane address per tap serves every fragment read of the tap
    // through immediate offsets (was: five instructions per read).  Out-of-image pixels are loaded with an out-of-range buffer
    // offset, which the hardware returns as zeros (no select per value).
    const bool ps_act = tid < HALO_PX;
    unsigned ps_off = 0u; int ps_row = 0, ps_swz = 0; bool ps_ok = false;
    if constexpr (PSL) {
        const int hp = ps_act ? tid : 0;
        const int hy = hp / HALO_W, hx = hp - hy * HALO_W;
        const int iy = y0 + hy, ix = x0 + hx;
        ps_ok = ps_act && iy >= vy0 && iy < vy1 && ix >= 0 && ix < a.Win;
        const int iyc = iy < 0 ? 0 : (iy >= a.Hin ? a.Hin - 1 : iy), ixc = ix < 0 ? 0 : (ix >= a.Win ? a.Win - 1 : ix);
        ps_off = ps_ok ? (unsigned)(iyc * a.Win + ixc) * EB : 0x7ffffff0u;      // (raw buffer: voffset >= num_records reads as 0)
        ps_row = hp * HPITCH;
        ps_swz = M16 ? ((hx >> 2) & 1) << 1 : (hx >> 2) & 3;
    }
    auto ps_load = [&](int cc, int t, float (&x)[4]) {      // cc, t: wave-uniform.  Tap 8 (and the last chunk, which passes its own
        // cc) re-loads data that is already on its way / in L2 instead of branching around the loads: a uniform condition here is
        // turned into scalar branches with one load form per path, and the waits of the tap loop stop being exact counts
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = cc * KCB + (t & 7) * 4 + j;
            c = c < a.C ? c : a.C - 1;                                 // (ragged last chunk: the channel meets zero weights)
            x[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_in, ps_off, (unsigned)c * HWin * EB, 0));
        }
    };
    // per-channel factors of a slice (style x fp16 sample scale): requested at the START of the tap that writes the slice, half a tap
    // before they are used, so that the LDS read is long complete and its wait does not drain the fragment reads in flight
    auto ps_factors = [&](int cc, int t) -> float4 {
        return *reinterpret_cast<const float4*>(scl + cc * KCB + (t & 7) * 4);
    };
    auto ps_write = [&](unsigned char* buf, int t, const float (&x)[4], const float4 f) {      // the slice loaded with the same t
        if (t < 8 && ps_act) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            unsigned char* dst = buf + ps_row + ((((t >> 1) ^ ps_swz) & 3) << 4) + (t & 1) * 8;
            // scalar fp32 arithmetic on purpose: v_pk_mul_f32 / v_pk_fma_f32 beside MFMAs cost ~20 cycles each (MI355X_MICROARCH.md,
            // 'price of one filler beside MFMAs'); only the two conversions are packed
            const float p0 = x[0] * f.x, p1 = x[1] * f.y, p2 = x[2] * f.z, p3 = x[3] * f.w;
            const f16x2 h0 = __builtin_convertvector(f32x2{p0, p1}, f16x2), h1 = __builtin_convertvector(f32x2{p2, p3}, f16x2);
            const float r0 = __builtin_fmaf(x[0], f.x, -(float)h0[0]), r1 = __builtin_fmaf(x[1], f.y, -(float)h0[1]);
            const float r2 = __builtin_fmaf(x[2], f.z, -(float)h1[0]), r3 = __builtin_fmaf(x[3], f.w, -(float)h1[1]);
            const f16x2 l0 = __builtin_convertvector(f32x2{r0, r1}, f16x2), l1 = __builtin_convertvector(f32x2{r2, r3}, f16x2);
            const uint2 wh = make_uint2(__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1));
            const uint2 wl = make_uint2(__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1));
            *reinterpret_cast<uint2*>(dst) = wh;
            *reinterpret_cast<uint2*>(dst + HPLANE) = wl;
        }
    };

    // ---- A fragments straight from the fragment-order pack
    const LaWgt wg = la_wgt_setup<FMT>(a, m0 + wm * 32, wpack);
    const unsigned a_off = wg.off + (unsigned)lane * 16u;
    auto load_a = [&](int cc, int t, int ks, bf16x8 (&dst)[NTERM]) { la_wgt_load(wg, cc, t, a_off, ks * 1024, dst); };
    // B fragments: lane (l31, lh) of N-subtile j reads slot ks*2 + lh of halo pixel (wn*NJ + j) * 34 + shift + l31
    // PSL (column swizzle): byte offset of this lane's K-step 0 fragment of tile row 0 for a tap; K-step 1 = ^ 32, tile row j = + j * 34 * 64
    auto lane_b = [&](int shift, int dxp) -> int {
        return (shift + l31) * HPITCH + (((lh ^ ((l31 + dxp) >> 2)) & 3) << 4);
    };
    auto read_b = [&](const unsigned char* buf, int shift, int ks, bf16x8 (&dst)[NTERM][NJ], int lb = 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            int o;
            if constexpr (PSL) o = (lb ^ (ks << 5)) + (wn * NJ + j) * HALO_W * HPITCH;
            else {
                const int p = (wn * NJ + j) * HALO_W + shift + l31;
                o = p * HPITCH + ((((ks * 2 + lh) ^ (p >> 2)) & 3) << 4);
            }
#pragma unroll
            for (int q = 0; q < NTERM; ++q) dst[q][j] = *reinterpret_cast<const bf16x8*>(buf + q * HPLANE + o);
        }
    };

    f32x16 acc[1][NJ];
    la_acc_zero(acc);
    auto mma_step = [&](bf16x8 (&af)[NTERM], bf16x8 (&bf)[NTERM][NJ]) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[0][j] = la_mma_terms<F16>(af, bf, j, acc[0][j]);
    };

    // ---- prologue: chunk 0's halo (all nine slices in flight at once) and the first tap's weights
    bf16x8 acur[2][NTERM];
    LA_STAMP_DECL
    if constexpr (PSL) {
        float pre[8][4];
#pragma unroll
        for (int t = 0; t < 8; ++t) ps_load(0, t, pre[t]);
        if constexpr (!M16) { load_a(0, 0, 0, acur[0]); load_a(0, 0, 1, acur[1]); }
        {
            const float xs = F16 ? la_xs_get(a.acc_scale_x, b, a.acc_scale_fan) : 1.f;
            for (int k = tid; k < nck * KCB; k += 256)
                scl[k] = k < a.C ? (a.in_scale ? a.in_scale[(long)b * a.scale_stride + k] : 1.f) * xs : 0.f;
        }
        LA_STAMP(0);
        __syncthreads();                           // scl is complete before any slice is scaled with it
#pragma unroll
        for (int t = 0; t < 8; ++t) ps_write(smem, t, pre[t], ps_factors(0, t));
    } else {
        Slice pre[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) slice_load(0, t, pre[t]);
        load_a(0, 0, 0, acur[0]);
        load_a(0, 0, 1, acur[1]);
        {      // per-channel factors: filled after the halo / weight loads were issued, so that the latencies overlap
            const float xs = F16 ? la_xs_get(a.acc_scale_x, b, a.acc_scale_fan) : 1.f;
            for (int k = tid; k < nck * KCB; k += 256)
                scl[k] = k < a.C ? (a.in_scale ? a.in_scale[(long)b * a.scale_stride + k] : 1.f) * xs : 0.f;
        }
        __syncthreads();                           // scl is complete before any slice is scaled with it
#pragma unroll
        for (int t = 0; t < 9; ++t) slice_write(smem, pre[t]);
    }
    __syncthreads();
    LA_STAMP(1);

  if constexpr (M16) {
    const int c16 = lane & 15, kq = lane >> 4;
    f32x4 acc16[2][8];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int n = 0; n < 8; ++n) acc16[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // weight fragments of a 16-row half: lane (c16, kq) holds rows mi*16 + c16, channels 8 kq .. 8 kq + 7 of the chunk
    const unsigned a16_off = wg.off + (unsigned)(kq * 32 + c16) * 16u;
    auto load_a16 = [&](int cc, int t, int mi, f16x8 (&dst)[2]) { la_wgt_load(wg, cc, t, a16_off + (unsigned)mi * 256u, 0u, dst); };
    // pixel fragment of tile n (tile row n >> 1, x half n & 1): lane (c16, kq) reads slot kq of its pixel's 64-byte row (column swizzle:
    // lb16 = this lane's offset for the tap, the tile adds an immediate)
    auto lane_b16 = [&](int shift, int dxp) -> int {
        return (shift + c16) * HPITCH + (((kq ^ ((((c16 + dxp) >> 2) & 1) << 1)) & 3) << 4);
    };
    auto read_b16 = [&](const unsigned char* buf, int n, f16x8 (&dst)[2], int lb16) {
        const int o = lb16 + ((n >> 1) * HALO_W + (n & 1) * 16) * HPITCH;
#pragma unroll
        for (int q = 0; q < 2; ++q) dst[q] = *reinterpret_cast<const f16x8*>(buf + q * HPLANE + o);
    };
    f16x8 a16[2][2], b16[4][2];
    // (issue order pinned: the tap loop's first wait is counted for "everything but the two youngest loads" on both of its entries)
    __builtin_amdgcn_sched_barrier(0);
    load_a16(0, 0, 0, a16[0]);
    __builtin_amdgcn_sched_barrier(0);
    load_a16(0, 0, 1, a16[1]);
    __builtin_amdgcn_sched_barrier(0);
    for (int cc = 0; cc < nck; ++cc) {
        const unsigned char* cur = smem + (cc & 1) * HBUF;
        unsigned char* nxt = smem + ((cc + 1) & 1) * HBUF;
        const bool has_next = cc + 1 < nck;
        float psx[4] = {0.f, 0.f, 0.f, 0.f};
        int lb_cur = lane_b16((int)(shpack & 127u), (int)(xpack & 3u));
#pragma unroll
        for (int n = 0; n < 4; ++n) read_b16(cur, n, b16[n], lb_cur);
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int tn = t + 1 < 9 ? t + 1 : 0;
            const int ccn = t + 1 < 9 ? cc : (has_next ? cc + 1 : 0);
            const int shift_n = (int)((shpack >> (7 * (t + 1 < 9 ? t + 1 : 8))) & 127u);
            const int lb_nxt = lane_b16(shift_n, (int)((xpack >> (2 * (t + 1 < 9 ? t + 1 : 8))) & 3u));
            float4 psf = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has_next && t >= 1) psf = ps_factors(cc + 1, t - 1);
            // every pixel fragment read ONCE per tap: four quarters (tiles 0-3 x rows 0-15, tiles 0-3 x rows 16-31, tiles 4-7 x rows 0-15,
            // tiles 4-7 x rows 16-31); a slot is re-filled after its second use with the tile four steps ahead (tile k + 4 of this tap, then
            // tile k of the next tap).  Half the LDS fragment traffic of walking all eight tiles per 16-row half (the LDS pipe of a CU is
            // busy 54-90 % under three workgroups, profiles/r05_pmc_halo_waits.txt) -- at the price of a QUARTER tap instead of half a tap
            // for the next weights to land
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int hf = q4 >> 1, mi = q4 & 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int n = hf * 4 + k;
                    f16x8 (&bs)[2] = b16[k];
                    acc16[mi][n] = la_mma16_terms(a16[mi], bs, acc16[mi][n]);
                    if (mi == 1) {
                        if (hf == 0) read_b16(cur, 4 + k, bs, lb_cur);
                        else if (t + 1 < 9) read_b16(cur, k, bs, lb_nxt);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (q4 == 2) load_a16(ccn, tn, 0, a16[0]);      // rows 0-15 are done with this tap's weights: the next tap's, a quarter tap to land
                if (q4 == 3) load_a16(ccn, tn, 1, a16[1]);
                if (q4 == 1) {
                    if (has_next && t >= 1) ps_write(nxt, t - 1, psx, psf);      // the slice loaded one tap ago
                    ps_load(has_next ? cc + 1 : cc, t, psx);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            lb_cur = lb_nxt;
        }
        LA_STAMP(2);
        __syncthreads();
        LA_STAMP(3);
    }
    // 16x16 tiles -> the 32x32 accumulator layout of the epilogue, through LDS (free after the loop's last barrier), two tile rows
    // at a time: image [wave][64 pixels][36 floats] (32 rows + 4 of padding), 16-byte writes and reads
    {
        const float inv = 1.f / (a.acc_scale_w[0] * la_xs_get(a.acc_scale_x, b, a.acc_scale_fan));
        float* tb = reinterpret_cast<float*>(smem) + wid * (64 * 36);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            if (hf) __syncthreads();
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int n4 = 0; n4 < 4; ++n4) {
                    const int n = hf * 4 + n4;
                    const int px = (n4 >> 1) * 32 + (n & 1) * 16 + c16;
                    // (element by element: a vector multiply here is two v_pk_mul_f32 -- no packed-FP32 arithmetic anywhere, Makefile)
                    const f32x4 v = acc16[mi][n];
                    *reinterpret_cast<f32x4*>(tb + px * 36 + mi * 16 + kq * 4) = f32x4{v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv};
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
    LA_STAMP(4);
    la_conv_epilogue<MT, false, true, WM_>(a, acc, red, ntile, m0, G, G LA_STAMP_ARG);
    LA_STAMP(5);
    LA_STAMP_OUT;
    return;
  } else
  if constexpr (SB) {
    // single-buffer form: bf holds the fragments of ONE K-step; sub-tile j is re-loaded for the following K-step right after its own
    // three MFMAs have issued, so its LDS latency runs under the MFMAs of the other sub-tiles and no second fragment set is live
    bf16x8 bf[NTERM][NJ];
    auto mma_refill = [&](bf16x8 (&af)[NTERM], const unsigned char* buf, int shift, int ks, bool refill, int lb = 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            acc[0][j] = la_mma_terms<F16>(af, bf, j, acc[0][j]);
            if (refill) {
                int o;
                if constexpr (PSL) o = (lb ^ (ks << 5)) + (wn * NJ + j) * HALO_W * HPITCH;
                else {
                    const int p = (wn * NJ + j) * HALO_W + shift + l31;
                    o = p * HPITCH + ((((ks * 2 + lh) ^ (p >> 2)) & 3) << 4);
                }
#pragma unroll
                for (int q = 0; q < NTERM; ++q) bf[q][j] = *reinterpret_cast<const bf16x8*>(buf + q * HPLANE + o);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int cc = 0; cc < nck; ++cc) {
        const unsigned char* cur = smem + (cc & 1) * HBUF;
        unsigned char* nxt = smem + ((cc + 1) & 1) * HBUF;
        const bool has_next = cc + 1 < nck;
        Slice sl;
        sl.wr = -1;
        sl.ok = false;
        float psx[4] = {0.f, 0.f, 0.f, 0.f};
        int lb = PSL ? lane_b((int)(shpack & 127u), (int)(xpack & 3u)) : 0;      // lane address of the current tap (PSL)
        read_b(cur, (int)(shpack & 127u), 0, bf, lb);
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int shift = (int)((shpack >> (7 * t)) & 127u);
            const int tn = t + 1 < 9 ? t + 1 : 0;
            const int ccn = t + 1 < 9 ? cc : (has_next ? cc + 1 : 0);
            const int shift_n = (int)((shpack >> (7 * (t + 1 < 9 ? t + 1 : 8))) & 127u);
            float4 psf = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (PSL) { if (has_next && t >= 1) psf = ps_factors(cc + 1, t - 1); }
            mma_refill(acur[0], cur, shift, 1, true, lb);      // K-step 0; refilled with this tap's K-step 1
            if constexpr (PSL) lb = lane_b(shift_n, (int)((xpack >> (2 * (t + 1 < 9 ? t + 1 : 8))) & 3u));
            load_a(ccn, tn, 0, acur[0]);
            if constexpr (PSL) {
                if (has_next && t >= 1) ps_write(nxt, t - 1, psx, psf);      // the slice loaded one tap ago
                ps_load(has_next ? cc + 1 : cc, t, psx);
            } else {
                slice_write(nxt, sl);
                slice_load(has_next ? cc + 1 : cc, t, sl, has_next);      // (last chunk: dummy loads, nothing staged)
            }
            __builtin_amdgcn_sched_barrier(0);
            mma_refill(acur[1], cur, shift_n, 0, t + 1 < 9, lb);   // K-step 1; refilled with the next tap's K-step 0 (not across the barrier)
            load_a(ccn, tn, 1, acur[1]);
        }
        if constexpr (!PSL) slice_write(nxt, sl);      // (PSL: tap 8 loads nothing)
        __syncthreads();       // next halo complete, everyone done with this one (and, at the end, LDS free for the epilogue)
    }
  } else {
    bf16x8 bf0[NTERM][NJ], bf1[NTERM][NJ];
    auto chunk = [&](int cc, auto has_next) {
        constexpr bool NEXT = decltype(has_next)::value;
        const unsigned char* cur = smem + (cc & 1) * HBUF;
        unsigned char* nxt = smem + ((cc + 1) & 1) * HBUF;
        Slice sl;
        sl.wr = -1;
        sl.ok = false;
        float psx[4] = {0.f, 0.f, 0.f, 0.f};
        int lb = PSL ? lane_b((int)(shpack & 127u), (int)(xpack & 3u)) : 0;      // lane address of the current tap (PSL)
        read_b(cur, (int)(shpack & 127u), 0, bf0, lb);
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int shift = (int)((shpack >> (7 * t)) & 127u);
            // the tap after this one: next tap, else first tap of the next chunk (the final one re-reads a valid slab)
            const int tn = t + 1 < 9 ? t + 1 : 0;
            const int ccn = t + 1 < 9 ? cc : (NEXT ? cc + 1 : 0);
            const int shift_n = (int)((shpack >> (7 * (t + 1 < 9 ? t + 1 : 8))) & 127u);   // (last tap: harmless re-read)
            // (the fences pin the issue order: left alone, the scheduler sinks every load to just before its first use)
            float4 psf = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (PSL) { if (NEXT && t >= 1) psf = ps_factors(cc + 1, t - 1); }
            read_b(cur, shift, 1, bf1, lb);        // B of K-step 1 flies under the MFMAs of K-step 0
            mma_step(acur[0], bf0);
            __builtin_amdgcn_sched_barrier(0);
            load_a(ccn, tn, 0, acur[0]);           // re-loaded as soon as its MFMAs have issued
            if constexpr (PSL) lb = lane_b(shift_n, (int)((xpack >> (2 * (t + 1 < 9 ? t + 1 : 8))) & 3u));
            read_b(cur, shift_n, 0, bf0, lb);      // B of the next tap's K-step 0
            if (NEXT) {
                if constexpr (PSL) {
                    if (t >= 1) ps_write(nxt, t - 1, psx, psf);      // the slice loaded one tap ago
                    ps_load(cc + 1, t, psx);
                } else {
                    slice_write(nxt, sl);
                    slice_load(cc + 1, t, sl);
                }
            }
            mma_step(acur[1], bf1);
            __builtin_amdgcn_sched_barrier(0);
            load_a(ccn, tn, 1, acur[1]);
        }
        if (NEXT && !PSL) slice_write(nxt, sl);      // (PSL: tap 8 loads nothing new)
    };
    for (int cc = 0; cc < nck; ++cc) {
        if (cc + 1 < nck) chunk(cc, std::true_type{});
        else chunk(cc, std::false_type{});
        __syncthreads();       // next halo complete, everyone done with this one (and, at the end, LDS free for the epilogue)
    }
  }
    if (F16) {
        const float inv = 1.f / (a.acc_scale_w[0] * la_xs_get(a.acc_scale_x, b, a.acc_scale_fan));
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][j][r] *= inv;
    }
    la_conv_epilogue<MT, false, true, WM_>(a, acc, red, ntile, m0, G, G);
}

// > 64 KB of dynamic LDS needs the opt-in, and the attribute is per DEVICE: it is set once per (kernel, device) before the kernel's first
// launch (atomic flags: the entry points may be entered from several host threads, one per device)
#ifdef LA_DEV
#define HALO_LDS_CAP (160 * 1024)      // (room for LA_KNOB_HALO_LDSPAD)
#else
#define HALO_LDS_CAP (2 * 3 * HALO_PX * HPITCH + 4096 * (int)sizeof(float))
#endif
template <int MT, int FMT, int WV, int MF>
static int launch_halo(const LaConvArgs& as, dim3 grid, size_t lds, hipStream_t stream) {
    static std::atomic<bool> cap_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!cap_set[dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&la_conv_bf16_halo_kernel<MT, FMT, WV, MF>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, HALO_LDS_CAP);
        if (e != hipSuccess) { la_set_error(hipGetErrorString(e)); return LA_ERR_HIP; }
        cap_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL((la_conv_bf16_halo_kernel<MT, FMT, WV, MF>), grid, dim3(256), lds, stream, as);
    return LA_OK;
}

template <int FMT>
static int select_halo(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream) {
    constexpr int NTERM = FMT == FMT_BF16X3 ? 3 : 2;
    // two halo buffers (>= the epilogue's 4 * MT floats) + the per-channel factor table
    size_t lds = (size_t)(as.C > KCB ? 2 : 1) * NTERM * HALO_PX * HPITCH + (size_t)la_cdiv(as.C, KCB) * KCB * sizeof(float);
    const size_t epi = (size_t)160 * p.mt + (size_t)2048 * (p.mt / 32);      // what the epilogue addresses (row tables + fused-ToRGB partials)
    if (lds < epi) lds = epi;
    if constexpr (FMT == FMT_F16X2) {
        // the pixel-stationary loader; on 128-row tiles with more than one chunk its 16x16x32 form.  Dev knob LA_KNOB_HALO_LDSPAD:
        // extra KB of dynamic LDS per workgroup of that form -- fewer workgroups per CU, for scripts/halo_wave_timeline.py
        if (p.mfma == LA_CONV_MFMA_16X16X32)
            return launch_halo<128, FMT, 3, HALO_MF_F16_16>(as, p.grid, lds + (size_t)la_dev_knob(LA_KNOB_HALO_LDSPAD) * 1024, stream);
        if (p.mt == 128) return launch_halo<128, FMT, 3, HALO_MF_F16_32>(as, p.grid, lds, stream);
        if (p.mt == 64) return launch_halo<64, FMT, 2, HALO_MF_F16_32>(as, p.grid, lds, stream);
        return launch_halo<32, FMT, 2, HALO_MF_F16_32>(as, p.grid, lds, stream);
    } else {
        // three waves per SIMD on 128-row tiles for the two-term format (the three-term one does not fit them)
        if (p.mt == 128) return launch_halo<128, FMT, NTERM == 2 ? 3 : 2, HALO_MF_BF16>(as, p.grid, lds, stream);
        if (p.mt == 64) return launch_halo<64, FMT, 2, HALO_MF_BF16>(as, p.grid, lds, stream);
        return launch_halo<32, FMT, 2, HALO_MF_BF16>(as, p.grid, lds, stream);
    }
}

int la_conv_halo_launch(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream) {
    if (as.precision == LA_PREC_BF16X3) return select_halo<FMT_BF16X3>(as, p, stream);
    if (as.precision == LA_PREC_F16X2) return select_halo<FMT_F16X2>(as, p, stream);
    return select_halo<FMT_BF16X2>(as, p, stream);
}
