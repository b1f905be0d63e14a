// Implicit-GEMM convolution on the fp32 MFMA path (v_mfma_f32_32x32x2_f32), gfx950.
//
// One kernel family serves every dense contraction of the synthesis pass (DESIGN.md "conv_igemm"):
//   F1  forward 3x3 same-resolution conv          (conv2d_resample.py:132-134)
//   F2  forward transposed stride-2 conv, one launch per output phase (conv2d_resample.py:112-125)
//   B1  backward-data of F1 (flipped taps, transposed weight slab)
//   B2  backward-data of F2 (stride-2 gather over the (2h+1)^2 gradient)
// expressed as  out[b, m, g*os+oo] = sum_{t, c} wgt[tap_w[t]][c][m] * scale[b][c] * in[b, c, g*is + tap_d[t]]
#pragma once
#include <stddef.h>
#include <string.h>

#include "la_common.h"
#include "la_launch_args.h"

#define LA_EPI_RAW 0
#define LA_EPI_FWD 1
#define LA_EPI_BWD 2
#define LA_CONV_MAX_TAPS 9
#define LA_CONV_MAX_PHASES 4
#define LA_CONV_PHASE_TAPS 4

// Fused ToRGB of a block inside the epilogue of its conv1 (LaConvArgs::rgb): possible where one row tile of the halo kernel holds every
// output channel (la_modconv3x3_fwd_fuses_rgb); weights [imgc][cout], styles [B][s_stride] (already * weight_gain), bias [imgc],
// skip [B][imgc][res^2] or null, outputs rgb_pre / img [B][imgc][res^2]
struct LaRgbFuse {
    int imgc;                // 0: none
    const float* w; const float* s; int s_stride; const float* bias; const float* skip;
    float* rgb_pre; float* img; float clamp;
};
// Backward seam of the layer that produced `xin`, applied inside the backward contraction's epilogue (LaConvArgs::seam): its demod /
// bias / noise / activation (la_seam_set_epi), and where its demod-gradient partials and plane maxima go ([B][cin][la_modconv_ds_tiles(res)]).
struct LaSeamFuse {
    const float* demod; int demod_stride;
    const float* bias;
    const float* noise; long noise_bstride; float noise_strength;
    int act; float alpha, gain, clamp;
    float* ddn_part;         // [B][M][tiles_per_sample]
    float* pmax;             // [B][M][tiles_per_sample] or null
    float* xs_out;           // [B][LA_XS_FAN] or null: slot rows of the fp16 operand scale of `out` for its consumer = pow2 scale of
    float xs_mult;           //   xs_mult * max|out| over the sample, final when the launch has run: every kernel form (direct epilogues,
                             //   split-K finish pass) lowers the row itself (la_xs_lower, la_common.h; it must hold LA_XS_INIT before)
    // ToRGB backward of that block (imgc > 0): image gradient, ToRGB pre-clamp output, weights [imgc][C], styles, partial outputs
    int imgc;
    const float* g_img; const float* rgb_pre; float rgb_clamp;
    const float* wrgb; const float* s_rgb; int s_rgb_stride;
    float* dweff_part;       // [B][imgc][M][tiles_per_sample]
};

struct LaConvArgs {
    const float* in;         // [B][C][Hin][Win]; in_bstride == 0 broadcasts one sample over the batch
    const float* wgt;        // [slabs][C][M]
    float* out;              // [B][M][Hout][Wout]
    const float* in_scale;   // [B][scale_stride] or null: modulate-on-load  x * s[b][c]
    long in_bstride;
    int scale_stride;
    // Launch input = in * act'(in_mask_y) * in_gain, applied while the pre-split copy is made (16-bit flat / split-K launches only: the
    // activation backward in front of a backward contraction without a sweep of its own, bias_act.py:170 with grad = 1).  in_mask_y:
    // saved output of the activation, same shape as `in`, or null (factor in_gain only; 0 is read as 1).  The operand scale must then
    // be preset (acc_scale_x) from a bound of the product, e.g. max |in| * max slope.
    const float* in_mask_y;
    int in_mask_act; float in_mask_alpha, in_mask_gain, in_mask_clamp;
    float in_gain;
    int B, C, M, Hin, Win, Hout, Wout;
    int Gy, Gx;              // output grid per sample handled by this launch
    int in_sy, in_sx;
    int out_sy, out_sx, out_oy, out_ox;
    int out_pitch; long out_plane;   // LA_EPI_RAW only, 0 = dense: row pitch / plane stride of `out` in floats (padded scratch rows, 16-byte aligned)
    int ntaps;
    int tap_dy[LA_CONV_MAX_TAPS], tap_dx[LA_CONV_MAX_TAPS], tap_w[LA_CONV_MAX_TAPS];
    int epi;
    // LA_EPI_FWD:  y = clamp(act(acc*demod[b][m] + noise*strength + bias[m]) * gain)
    const float* demod;
    int demod_stride;
    const float* noise;      // [Hout][Wout] (noise_bstride 0) or [B][Hout][Wout]
    long noise_bstride;
    float noise_strength;
    const float* bias;
    int act;
    float alpha, gain, clamp;
    const float* addend;     // optional [B][M][Hout][Wout]: out2 = y + addend (residual sum), y itself still goes to `out`
    float* out2;
    // LA_EPI_FWD, optional: the fp16 operand scale of this launch's output for the contraction that consumes it -- slot rows
    // [B][LA_XS_FAN] (holding LA_XS_INIT before) that every producing workgroup lowers to pow2(mult[b] * its max |y|) (la_xs_lower,
    // la_common.h; y = out2 where there is one); fwd_xs_mult [B] or null (1): e.g. max_c |style| of the consuming layer
    float* fwd_xs_out;
    const float* fwd_xs_mult;
    // LA_EPI_BWD:  out = acc * out_scale[b][m];  ds_part[b][m][tile] = sum_pixels acc * xin[b][m][pixel]
    const float* out_scale;
    int oscale_stride;
    const float* xin;
    long xin_bstride;
    float* ds_part;          // [B][M][tiles_per_sample]
    int tiles_per_sample;
    // LA_EPI_BWD with seam.ddn_part != null (16-bit kernels and the split-K finish pass only): the backward "seam" of the layer
    // that PRODUCED xin is applied to the outgoing gradient in the same epilogue -- xin is that layer's saved output y, which the
    // epilogue loads anyway for ds_part -- instead of a separate pass over y and the gradient (la_seam_bwd_kernel<0>):
    //   g = acc * out_scale;  g1 = g * act'(y);  seam.ddn_part[b][m][tile] = sum_px g1 * (act^-1(y) - seam.bias[m] - noise*strength);
    //   out = g1 * seam.demod[b][m];  seam.pmax[b][m][tile] = max_px |out|   (plane maxima for the next contraction's operand scale)
    LaSeamFuse seam;
    // Fused ToRGB of the block (LA_EPI_FWD, 16-bit halo launches whose ONE row tile holds every output channel, M == tile rows):
    //   rgb.rgb_pre[b][c][px] = sum_m rgb.w[c][m] * rgb.s[b][m] * out[b][m][px] + rgb.bias[c];  rgb.img = clamp(rgb.rgb_pre) + rgb.skip
    // (la_torgb_fwd_kernel's arithmetic on the epilogue's registers: the block's conv1 output is not streamed a second time)
    LaRgbFuse rgb;
    // optional caller-provided scratch (la_conv_workspace_bytes): [fp16 scale header | pre-split input | split-K slice partials]
    void* ws;
    size_t ws_bytes;
    // filled in by la_conv_launch
    float* splitk_ws;
    int ksplit;
    const float* in_pmax;          // optional [B][C][in_pmax_nseg]: partial max |in| of every plane, left by the kernel that produced `in`
    int in_pmax_nseg;              //   (the fp16 operand scale then needs no absmax pass)
    const void* in_q;              // split paths: input already split by la_conv_prepare_input (flat / split-K kernels), or NULL
    // split-bf16 path (precision != LA_PREC_F32): weights pre-split by la_pack_conv_weights_bf16
    int precision;
    const void* wgt_bf16;          // split pack (la_conv_split_pack_bytes): 3 bf16 terms, 2 fp16 terms, fp16 weight scale
    long wgt_bf16_term_elems;      // elements per term: slabs * ceil(C/32) * M * 32
    // LA_PREC_F16X2: acc is divided by xscale[b] * wscale (exact powers of two) before the epilogue; set by la_conv_prepare_input
    const float* acc_scale_x;      // [B] (acc_scale_fan <= 1), or slot rows [B][LA_XS_FAN] left by the producer of `in` (acc_scale_fan = LA_XS_FAN)
    int acc_scale_fan;
    const float* acc_scale_w;      // [1]
    // Merged output phases (transposed stride-2 conv, 16-bit direct kernel only): nphase > 0 runs all phases in ONE launch,
    // blockIdx.z = phase * B + sample, each phase with its own grid / output offset / tap table (<= 4 taps).  One launch of
    // ~4x the workgroups instead of four launches that each end in a nearly empty last round.  Phase grids at the split-K sizes
    // (<= 34x34) run the same way through the split-K kernel: blockIdx.x walks the phases' flattened-pixel tiles back to back,
    // one finish launch serves all phases (blockIdx.z = phase).
    // Row window (16-bit direct kernels; a hint, 0 / 0 = all rows): only output-grid rows [row_lo, row_hi) are wanted -- pixel tiles that
    // hold none of them return at once and write nothing (merged phases: the window counts rows of every phase's own grid).  The
    // caller guarantees that nobody reads the rows left out (la_synth.hip: the loop steps of a criterion that sees a crop only).
    int row_lo, row_hi;
    // ... and a column window on top of it (0 / 0 = all columns; needs a row window).  Halo kernel: the wanted tiles are the rectangle of
    // 4 x 32 tiles that holds rows [row_lo, row_hi) x columns [col_lo, col_hi).  Direct flat kernel: the 128-pixel tiles are flattened over
    // exactly that rectangle of the grid (merged phases: of every phase's own grid), nothing outside it is computed or read; a backward
    // launch zero-fills the columns it leaves out in rows [row_lo, row_hi) of `out` (its readers have no column mask) and the partials of
    // the tile slots past the rectangle's.  The split-K forms compute every column.
    int col_lo, col_hi;
    // Valid rows of the INPUT (16-bit direct kernels; 0 / 0 = all): rows outside [in_row_lo, in_row_hi) read as zeros, as rows outside the
    // image do -- the backward contractions behind a windowed producer, whose other rows hold older contents of a shared buffer while the
    // gradient there is exactly zero.  (Flat kernel: rows of the pre-split operand's grid.)
    int in_row_lo, in_row_hi;
#ifdef LA_DEV
    int dbg_stamp;                 // development build: per-wave segment clocks of the MF 21 halo kernel (la_conv_halo.hip, LA_STAMP)
#endif
    int nphase;
    struct Phase {
        int Gy, Gx, out_oy, out_ox, ntaps; int tap_dy[LA_CONV_PHASE_TAPS], tap_dx[LA_CONV_PHASE_TAPS], tap_w[LA_CONV_PHASE_TAPS];
        int tile0;           // split-K form (filled by la_conv_launch): first flattened-pixel tile of the phase on blockIdx.x ...
        long ws_off;         // ... and the float offset of its slice partials inside splitk_ws
    } ph[LA_CONV_MAX_PHASES];
};
// Kernel parameter: the byte layout is pinned (numbers of the flat struct before the seam / ToRGB records became members).
static_assert(sizeof(LaConvArgs) == 1096 && offsetof(LaConvArgs, seam) == 416 && offsetof(LaConvArgs, rgb) == 568 && offsetof(LaConvArgs, ws) == 640,
              "LaConvArgs: an embedded record moved a kernel-parameter field");

// every launch starts from this: zeros, unit strides, a linear epilogue without clamp
static inline void la_conv_args_init(LaConvArgs& a) {
    memset(&a, 0, sizeof(a));
    a.in_sy = a.in_sx = a.out_sy = a.out_sx = 1;
    a.clamp = -1.f; a.gain = 1.f; a.act = LA_ACT_LINEAR;
}
// k x k taps around the centre (pad k / 2); backward: the flipped taps of the backward-data contraction
static inline void la_conv_taps_kxk(LaConvArgs& a, int k, bool backward) {
    a.ntaps = k * k;
    for (int t = 0; t < a.ntaps; ++t) {
        const int dy = t / k - k / 2, dx = t % k - k / 2;
        a.tap_dy[t] = backward ? -dy : dy; a.tap_dx[t] = backward ? -dx : dx; a.tap_w[t] = t;
    }
}
// Launch geometries on top of a.C (la_conv_weights_select).  k x k conv (pad k / 2) at one resolution, or its backward-data contraction ...
static inline void la_conv_geom_same(LaConvArgs& a, int res, int k, bool backward) {
    a.Hin = a.Win = a.Hout = a.Wout = a.Gy = a.Gx = res;
    a.in_bstride = (long)a.C * res * res;
    la_conv_taps_kxk(a, k, backward);
}
// ... and the stride-2 3x3 gather over a (res+1)^2 input onto a (res/2)^2 grid (D's down-sampling conv; backward-data of an up layer)
static inline void la_conv_geom_down2(LaConvArgs& a, int res) {
    a.Hin = a.Win = res + 1; a.Hout = a.Wout = a.Gy = a.Gx = res / 2;
    a.in_sy = a.in_sx = 2;
    a.in_bstride = (long)a.C * (res + 1) * (res + 1);
    a.ntaps = 9;      // 3 x 3 taps from the corner (offsets 0 .. 2)
    for (int t = 0; t < 9; ++t) { a.tap_dy[t] = t / 3; a.tap_dx[t] = t % 3; a.tap_w[t] = t; }
}
// the forward epilogue of a layer (demod and noise null: a plain bias / activation epilogue)
static inline void la_conv_set_epi(LaConvArgs& a, const LaLayerEpi& e) {
    a.epi = LA_EPI_FWD;
    a.demod = e.demod; a.demod_stride = e.demod_stride;
    a.noise = e.noise; a.noise_bstride = e.noise_bstride; a.noise_strength = e.noise_strength;
    a.bias = e.bias; a.act = e.act; a.alpha = e.alpha; a.gain = e.gain; a.clamp = e.clamp;
}
// Output phase (py, px) of the transposed stride-2 3x3 conv over an hin^2 input: row Y = 2 * qy + py receives the taps ky with
// (Y - ky) even.  Sets the launch-wide grid, offset (column phase px at out_ox = px * ox_step) and taps; merged: also appends them
// as the next phase of a one-launch form (LaConvArgs::nphase).
static inline void la_conv_up2_phase(LaConvArgs& a, int hin, int py, int px, int ox_step, bool merged) {
    a.out_oy = py; a.out_ox = px * ox_step;
    a.Gy = py ? hin : hin + 1; a.Gx = px ? hin : hin + 1;
    int nt = 0;
    for (int ky = py; ky < 3; ky += 2)
        for (int kx = px; kx < 3; kx += 2) { a.tap_dy[nt] = -(ky / 2); a.tap_dx[nt] = -(kx / 2); a.tap_w[nt] = ky * 3 + kx; ++nt; }
    a.ntaps = nt;
    if (!merged) return;
    LaConvArgs::Phase& P = a.ph[a.nphase++];
    P.Gy = a.Gy; P.Gx = a.Gx; P.out_oy = py; P.out_ox = a.out_ox; P.ntaps = nt;
    for (int t = 0; t < nt; ++t) { P.tap_dy[t] = a.tap_dy[t]; P.tap_dx[t] = a.tap_dx[t]; P.tap_w[t] = a.tap_w[t]; }
}
// ... the raw (2 hin + 1)-row intermediate those phases write: dense rows (pitch = xhalf = 0) or column-planar ones (la_conv_up2_launch) ...
static inline void la_conv_geom_up2(LaConvArgs& a, int hin, int pitch, int xhalf) {
    const int res = 2 * hin;
    a.Hin = a.Win = hin; a.Hout = a.Wout = res + 1;
    a.out_sy = a.out_sx = 2; a.epi = LA_EPI_RAW;
    if (pitch > 0) { a.out_pitch = pitch; a.out_plane = (long)pitch * (res + 1); }      // padded (2h+1)-wide rows
    if (xhalf > 0) { a.out_sx = 1; a.Wout = pitch; }      // phase px writes the contiguous run from px * xhalf
}
// ... and the four phases as one launch
static inline void la_conv_up2_merged(LaConvArgs& a, int hin, int ox_step) {
    for (int k = 0; k < 4; ++k) la_conv_up2_phase(a, hin, k >> 1, k & 1, ox_step, true);
    a.out_oy = a.out_ox = 0; a.Gy = a.Gx = hin + 1; a.ntaps = 4;      // launch-wide fields = the largest phase (checks only)
}

// The kernel form of one launch, decided once by la_conv_plan (host only: no HIP call) and read by everything that prepares, launches or
// accounts for it.  Not a kernel parameter.
enum { LA_FORM_F32 = 0, LA_FORM_F32_SPLIT, LA_FORM_FLAT, LA_FORM_FLAT_SPLIT, LA_FORM_HALO };
enum { LA_PREP_NONE = 0, LA_PREP_SCALE, LA_PREP_PRESPLIT };      // operand preparation: nothing, the fp16 scale pass only, a pre-split copy
struct LaConvPlan {
    int form, cls;           // LA_FORM_*, profiler class (LA_PC_CONV_*)
    int mt, mtiles, mfma, ksplit;      // row tile (128 / 64 / 32), row tiles, LA_CONV_MFMA_*, K slices (1: direct)
    dim3 grid;               // of the contraction launch; a windowed 16-bit launch holds the window's tiles only
    int prep; bool scale_pass;      // LA_PREP_*; with the per-sample fp16 operand scale computed into the workspace header
    size_t q_off, ws_head;   // byte offset of the pre-split copy in the workspace; bytes taken from its head, in front of the split-K partials
    int tile0[LA_CONV_MAX_PHASES]; long ws_off[LA_CONV_MAX_PHASES];      // split-K form, per phase: LaConvArgs::Phase::tile0 / ws_off
};
// LA_OK and the plan, or the refusal (error code + la_set_error text) of a launch with these arguments
int la_conv_plan(const LaConvArgs& a, LaConvPlan& p);

// ---- 16-bit split path, three units: la_conv_operand.hip (weight packs, operand scales, pre-split copy), la_conv_flat.hip
// (la_conv_bf16_kernel) and la_conv_halo.hip (la_conv_bf16_halo_kernel): the launches of the two kernels in the form p (LA_FORM_FLAT* / LA_FORM_HALO)
int la_conv_flat_launch(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream);
int la_conv_halo_launch(const LaConvArgs& as, const LaConvPlan& p, hipStream_t stream);

long la_conv_bf16_pack_elems(int M, int C, int ktaps);   // elements per term
int la_pack_conv_weights_bf16(const float* w, void* out, int cout, int cin, int ktaps, int transpose, int nterm,
                              hipStream_t stream, float scale = 1.f, int m_pad = 0);
// bytes of one weight pack serving every split precision: [3 bf16 terms][2 fp16 terms][pad to 16 B][wscale float] (term offsets: la_conv_device.h)
size_t la_conv_split_pack_bytes(int M, int C, int ktaps);
static inline size_t la_conv_pack_wscale_offset(long term_elems) { return ((size_t)5 * term_elems * 2 + 15) & ~(size_t)15; }
// fp32 slabs wf [ktaps][cin][cout], wb [ktaps][cout][wb_ld] and wsq [cin][cout] = sum over taps of w^2 (each optional) of w * scale (la_style.hip)
int la_pack_conv_weights(const float* w, float* wf, float* wb, float* wsq, int cout, int cin, int ktaps, hipStream_t,
                         float scale = 1.f, int wb_ld = 0);   // wb_ld > cin: backward slab rows padded with zero columns

// The weights of one conv layer as the contraction reads them, both directions, every precision.
struct LaConvWeights {
    int cin, cout, k;
    int cin_pad;             // output channels of the backward contraction: cin padded to a multiple of 4 (the padded ones come out as zeros)
    const float* w;          // the layer's parameter [cout][cin][k][k]
    float *wf, *wb, *wsq;    // fp32 slabs, forward / backward; wsq: optional (demodulation)
    void *wqf, *wqb;         // split packs, forward / backward
};
static inline void la_conv_weights_shape(LaConvWeights& L, int cin, int cout, int k) {
    L.cin = cin; L.cout = cout; L.k = k; L.cin_pad = (cin + 3) & ~3;
}
static inline void la_conv_weights_layout(LaCarver& c, LaConvWeights& L, bool with_wsq = false) {
    const size_t kk = (size_t)L.k * L.k;
    L.wf = c.take((size_t)L.cin * L.cout * kk); L.wb = c.take((size_t)L.cin_pad * L.cout * kk);
    L.wsq = with_wsq ? c.take((size_t)L.cin * L.cout) : nullptr;
    L.wqf = c.take((la_conv_split_pack_bytes(L.cout, L.cin, (int)kk) + 3) / 4);
    L.wqb = c.take((la_conv_split_pack_bytes(L.cin_pad, L.cout, (int)kk) + 3) / 4);
}
// packs L.w * gain (stream-ordered)
static inline int la_conv_weights_pack(const LaConvWeights& L, float gain, hipStream_t stream) {
    int rc = la_pack_conv_weights(L.w, L.wf, L.wb, L.wsq, L.cout, L.cin, L.k * L.k, stream, gain, L.cin_pad);
    if (!rc) rc = la_pack_conv_weights_bf16(L.w, L.wqf, L.cout, L.cin, L.k * L.k, 0, 3, stream, gain);
    if (!rc) rc = la_pack_conv_weights_bf16(L.w, L.wqb, L.cout, L.cin, L.k * L.k, 1, 3, stream, gain, L.cin_pad);
    return rc;
}
// the weights and channel counts of a launch in one direction (backward: the transposed contraction, cout -> cin_pad)
static inline void la_conv_weights_select(LaConvArgs& a, const LaConvWeights& L, bool backward) {
    a.wgt = backward ? L.wb : L.wf; a.wgt_bf16 = backward ? L.wqb : L.wqf;
    a.C = backward ? L.cout : L.cin; a.M = backward ? L.cin_pad : L.cout;
    a.wgt_bf16_term_elems = la_conv_bf16_pack_elems(a.M, a.C, L.k * L.k);
}

// scratch floats that let every <= 32x32 launch of a (B, M) problem use split-K: slices * B * M * G, G <= 1024
long la_conv_splitk_floats_phases(int B, int M, int C, int nphase, const int* Gy, const int* Gx, int precision);
static inline long la_conv_splitk_floats(int B, int M, int C, int Gy, int Gx, int precision) { return la_conv_splitk_floats_phases(B, M, C, 1, &Gy, &Gx, precision); }
// bytes of the pre-split copy of an input [B][C][Hin][Win] (split paths; sized for the larger, 8 B/element format)
size_t la_conv_presplit_bytes(int B, int C, int Hin, int Win);
size_t la_conv_presplit_hdr_bytes(int B, int C);      // ... and of its header alone (fp16 operand scales and their segment maxima)
// Operand preparation as the plan says (p.prep): split a.in (* a.in_scale) into the head of a.ws and / or compute the fp16 operand scale there,
// point a.in_q / a.acc_scale_x at them and advance a.ws / a.ws_bytes past p.ws_head.  bf16: {hi | mid << 16, lo} (8 B / element);  fp16:
// per-sample power-of-two scale, {hi | lo << 16} (4 B).  Without a plan: that of a launch of `a` as it stands -- callers that launch several
// phases over one input call this once, up front; the launch that then arrives with in_q set plans no preparation.
int la_conv_prepare_input(LaConvArgs& a, const LaConvPlan& p, hipStream_t stream);
static inline int la_conv_prepare_input(LaConvArgs& a, hipStream_t stream) {
    LaConvPlan p; const int rc = la_conv_plan(a, p); return rc ? rc : la_conv_prepare_input(a, p, stream);
}
// Activation backward fused with the plane maxima of its result (pass 1 of the fp16 operand scale of the consuming contraction):
// dx [B][C][HW] = dy * act'(yref) (dx may alias dy), pm [B][C][la_conv_act_grad_segments(HW)] -> LaConvArgs::in_pmax / in_pmax_nseg.
// Replaces la_bias_act_grad_f32 (bias_act.py:170, grad = 1) where the result feeds a contraction.
int la_conv_act_grad_segments(long HW);
int la_conv_act_grad_pmax(const float* dy, const float* yref, float* dx, float* pm, int B, int C, long HW, int act, float alpha, float gain,
                          float clamp, hipStream_t stream);
int la_conv_xscale_from_pmax(const float* pmax, int nseg, const float* scale, int scale_stride, float mult, float* xscale, int B, int C,
                             hipStream_t stream);
int la_absmax_bits(const float* w, long n, unsigned* amax_bits, hipStream_t stream);      // max |w| as a float bit pattern (zero it first)

// number of pixel tiles per sample for a launch (the ds_part leading dimension)
int la_conv_tiles_per_sample(int Gy, int Gx);
int la_conv_launch(const LaConvArgs& a, hipStream_t stream);

// Transposed stride-2 3x3 conv of an [B][C][hin][hin] input into a raw (2 hin + 1)-row intermediate: dense rows (pitch = xhalf = 0), or
// COLUMN-PLANAR rows of `pitch` floats -- even output columns from 0, odd ones from xhalf on -- so that every output phase stores
// contiguous runs.  The caller has set input, weights, operand scale, mask and windows.  16-bit precisions: the input is split once
// and the four phases run in ONE launch -- above the split-K sizes each phase launch would end in a nearly empty round, at the
// split-K sizes (<= 34x34 phase grids) four launches + four finish passes become one of each; fp32: a launch per phase.
static inline int la_conv_up2_launch(LaConvArgs& a, int hin, int pitch, int xhalf, hipStream_t stream) {
    la_conv_geom_up2(a, hin, pitch, xhalf);
    const int ox_step = xhalf > 0 ? xhalf : 1;
    int rc;
    if (a.precision != LA_PREC_F32) {
        la_conv_up2_phase(a, hin, 0, 0, ox_step, false);      // (the preparation is planned on the largest phase)
        if ((rc = la_conv_prepare_input(a, stream))) return rc;
        la_conv_up2_merged(a, hin, ox_step);
        return la_conv_launch(a, stream);
    }
    for (int k = 0; k < 4; ++k) {
        la_conv_up2_phase(a, hin, k >> 1, k & 1, ox_step, false);
        if ((rc = la_conv_launch(a, stream))) return rc;
    }
    return LA_OK;
}
