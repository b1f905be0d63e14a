// Modulated 3x3 convolution of a SynthesisLayer, forward and backward-to-(input, style), composed from the
// implicit-GEMM contraction (la_conv.hip) and the FIR kernels (la_upfirdn2d.hip).
// Reference semantics: SG2 `modulated_conv2d` + `bias_act` inside SynthesisLayer.forward, with the
// resampling algebra of models/stylegan3/torch_utils/ops/conv2d_resample.py:82-86,112-134 (Appendix B).
#include "la_modconv.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "la_conv.h"
#include "la_upfirdn2d.h"

extern "C" int la_pack_conv_weights_f32(const float* w, float* wf, float* wb, float* wsq, int cout, int cin, int ktaps,
                                        hipStream_t stream) {
    return la_pack_conv_weights(w, wf, wb, wsq, cout, cin, ktaps, stream);
}

// what every launch of a layer starts from: weights, arithmetic, scratch, channel counts (backward: the transposed contraction)
static void start_args(LaConvArgs& a, const LaModconv& m, bool backward) {
    la_conv_args_init(a);
    a.wgt = m.w; a.ws = m.ws; a.ws_bytes = m.ws_bytes;
    a.precision = m.precision; a.wgt_bf16 = m.wq;
    a.B = m.B; a.C = backward ? m.cout : m.cin; a.M = backward ? m.cin : m.cout;
    a.wgt_bf16_term_elems = la_conv_bf16_pack_elems(a.M, a.C, 9);
}
static void set_bwd(LaConvArgs& a, const LaModconv& m, const float* xin, long xin_bstride, float* ds_part, int grid_res, const LaSeamFuse* seam) {
    a.epi = LA_EPI_BWD;
    a.out_scale = m.s; a.oscale_stride = m.s_stride;
    a.xin = xin; a.xin_bstride = xin_bstride;
    a.ds_part = ds_part; a.tiles_per_sample = la_conv_tiles_per_sample(grid_res, grid_res);
    if (seam) a.seam = *seam;
}

// one row tile of the halo kernel = all output channels (tiles of 128, 64 or -- for <= 32 channels -- 32 rows): what la_conv_plan says of
// the forward launch, with a workspace that holds whatever it asks for
bool la_modconv3x3_fwd_fuses_rgb(int precision, int B, int cin, int cout, int res) {
    static const bool off = la_dev_env("LA_NO_RGB_FUSE") != nullptr;      // dev knob
    long info[LA_CONV_PLAN_NINFO];
    return !off && la_conv_plan_query(precision, B, cin, cout, LA_CONV_GEOM_SAME_FWD, res, 0, (size_t)1 << 40, info) == LA_OK &&
           info[LA_CONV_PLAN_CLS] == LA_PC_CONV_HALO && info[LA_CONV_PLAN_MT] == cout;
}

int la_modconv3x3_fwd_ex(const float* x, long x_bstride, const LaModconv& m, const LaLayerEpi& epi, float* y, hipStream_t stream,
                         const LaModconvFwdOpts& o) {
    const int res = m.res;
    const LaWindow& w = o.win;
    LA_CHECK_ARG(x && m.w && y, "modconv_fwd: null pointer");
    LA_CHECK_ARG(w.col_lo >= 0 && (w.col_hi == 0 || (w.row_hi > 0 && w.col_hi > w.col_lo && w.col_hi <= res)), "modconv_fwd: bad column window");
    LA_CHECK_ARG(w.row_lo >= 0 && (w.row_hi == 0 || (w.row_hi > w.row_lo && w.row_hi <= res)), "modconv_fwd: bad row window");
    LaConvArgs a; start_args(a, m, false);
    a.row_lo = w.row_lo; a.row_hi = w.row_hi; a.col_lo = w.col_lo; a.col_hi = w.col_hi;
    a.fwd_xs_out = o.xs_out; a.fwd_xs_mult = o.xs_mult;
    if (o.rgb) {
        const LaRgbFuse& r = *o.rgb;
        LA_CHECK_ARG(r.imgc >= 1 && r.imgc <= 4 && r.w && r.s && r.rgb_pre && r.img && la_modconv3x3_fwd_fuses_rgb(m.precision, m.B, m.cin, m.cout, res),
                     "modconv_fwd: this launch cannot carry the fused ToRGB (la_modconv3x3_fwd_fuses_rgb)");
        a.rgb = r;
    }
    if (m.precision == LA_PREC_F16X2 && o.xscale) { a.acc_scale_x = o.xscale; a.acc_scale_fan = LA_XS_FAN; }      // preset operand scale (slot rows of the caller): no absmax / plane-maxima pass
    la_conv_geom_same(a, res, 3, false);
    a.in = x; a.in_bstride = x_bstride; a.out = y; a.in_pmax = o.in_pmax; a.in_pmax_nseg = o.in_nseg;
    a.in_scale = m.s; a.scale_stride = m.s_stride;
    la_conv_set_epi(a, epi);
    return la_conv_launch(a, stream);
}

extern "C" int la_modconv3x3_fwd_f32(const float* x, long x_bstride, const float* wf, const void* wq, int precision, const float* s, int s_stride, const float* d,
                                     int d_stride, const float* noise, long noise_bstride, float noise_strength, const float* bias,
                                     int act, float alpha, float gain, float clamp, float* y, void* ws, size_t ws_bytes, int B, int cin, int cout, int res,
                                     hipStream_t stream) {
    return la_modconv3x3_fwd_ex(x, x_bstride, LaModconv{wf, wq, precision, s, s_stride, B, cin, cout, res, ws, ws_bytes},
                                LaLayerEpi{d, d_stride, noise, noise_bstride, noise_strength, bias, act, alpha, gain, clamp}, y, stream);
}

int la_modconv3x3_up2_fwd_ex(const float* x, long x_bstride, const LaModconv& m, const LaLayerEpi& epi, const float* fir_host, float* scratch,
                             float* y, hipStream_t stream, const LaModconvFwdOpts& o) {
    const int res = m.res, scratch_pitch = o.scratch_pitch, scratch_xhalf = o.scratch_xhalf;
    LaWindow w = o.win;
    LA_CHECK_ARG(x && m.w && y && scratch && fir_host, "modconv_up2_fwd: null pointer");
    LA_CHECK_ARG(w.row_lo >= 0 && (w.row_hi == 0 || (w.row_hi > w.row_lo && w.row_hi <= res)), "modconv_up2_fwd: bad row window");
    if (scratch_xhalf == 0) w.row_lo = w.row_hi = 0;      // (only the planar FIR kernel honours a window)
    if (w.row_hi == 0) w.col_lo = w.col_hi = 0;
    LA_CHECK_ARG(w.col_lo >= 0 && (w.col_hi == 0 || (w.col_hi > w.col_lo && w.col_hi <= res)), "modconv_up2_fwd: bad column window");
    LA_CHECK_ARG(scratch_pitch == 0 || scratch_pitch >= res + 1, "modconv_up2_fwd: scratch pitch smaller than a row");
    LA_CHECK_ARG((scratch_xhalf == 0 && scratch_pitch == 0) || (scratch_xhalf >= res / 2 + 1 && scratch_pitch >= scratch_xhalf + res / 2),
                 "modconv_up2_fwd: bad column-planar scratch layout");
    LA_CHECK_ARG(res >= 2 && res % 2 == 0, "modconv_up2_fwd: output resolution must be even");
    const int hin = res / 2;
    LaConvArgs a; start_args(a, m, false);
    a.in = x; a.in_bstride = x_bstride; a.out = scratch;
    a.in_scale = m.s; a.scale_stride = m.s_stride;
    if (m.precision == LA_PREC_F16X2 && o.xscale) { a.acc_scale_x = o.xscale; a.acc_scale_fan = LA_XS_FAN; }      // preset operand scale (slot rows of the caller): no absmax pass
    if (w.row_hi > 0) {
        // FIR output row y reads intermediate rows y - 1 .. y + 2; intermediate row Y = 2 q + py belongs to row q of phase py
        int zlo = w.row_lo, zhi = w.row_hi;
        la_span_grow(zlo, zhi, 1, 2, res + 1);
        a.row_lo = zlo >> 1; a.row_hi = ((zhi - 1) >> 1) + 1;
        // the input rows those phase rows read: nothing else is copied into the pre-split operand, and the contraction reads the rest as zeros
        la_modconv3x3_up2_fwd_rows(res, w.row_lo, w.row_hi, &a.in_row_lo, &a.in_row_hi);
        if (w.col_hi > 0) {
            // columns likewise; the FIR computes the whole 4-column groups that hold a wanted column (la_fir4x4_s1p_kernel), so the phase
            // columns are those of the groups: everything the FIR reads is computed, what lies outside is neither written nor read
            int zc0 = w.col_lo, zc1 = w.col_hi;
            la_span_tiles(zc0, zc1, 4, res);
            la_span_grow(zc0, zc1, 1, 2, res + 1);
            const int q0 = zc0 >> 1, q1 = ((zc1 - 1) >> 1) + 1;
            if (q0 > 0 || q1 < res / 2 + 1) { a.col_lo = q0; a.col_hi = q1; }
        }
    }
    // transposed stride-2 conv of the (modulated) input into the scratch
    int rc = la_conv_up2_launch(a, hin, scratch_pitch, scratch_xhalf, stream);
    if (rc) return rc;
    // FIR with pad (1,1,1,1) and gain up^2 = 4, then the layer epilogue
    LaFirTail t;
    t.pmax = o.y_pmax; t.xs_out = o.xs_out; t.xs_mult = o.xs_mult; t.win = w;
    t.in_pitch = scratch_pitch; t.in_plane = (long)scratch_pitch * (res + 1); t.in_xhalf = scratch_xhalf;
    return la_upfirdn2d_modconv_epilogue(scratch, y, m.B, m.cout, res + 1, res + 1, fir_host, la_fir_same_pad1(), epi, stream, t);
}

// input rows [in_lo, in_hi) (of the res/2-row input) that la_modconv3x3_up2_fwd_ex reads for the row window [row_lo, row_hi) of y: the phase
// rows of the window (above) plus the tap row above
void la_modconv3x3_up2_fwd_rows(int res, int row_lo, int row_hi, int* in_lo, int* in_hi) {
    int zlo = row_lo, zhi = row_hi;
    la_span_grow(zlo, zhi, 1, 2, res + 1);
    // (the flattened 128-pixel tiles at the ends of the window reach into phase rows outside it; what they compute there from rows the
    //  producer did not deliver lands in intermediate rows that the FIR never reads)
    *in_lo = zlo >> 1; *in_hi = ((zhi - 1) >> 1) + 1;
    la_span_grow(*in_lo, *in_hi, 1, 0, res / 2);
}

extern "C" int la_modconv3x3_up2_fwd_f32(const float* x, long x_bstride, const float* wf, const void* wq, int precision, const float* s, int s_stride,
                                         const float* d, int d_stride, const float* noise, long noise_bstride,
                                         float noise_strength, const float* bias, int act, float alpha, float gain,
                                         float clamp, const float* fir_host, float* scratch, float* y, void* ws, size_t ws_bytes, int B, int cin,
                                         int cout, int res, hipStream_t stream) {
    return la_modconv3x3_up2_fwd_ex(x, x_bstride, LaModconv{wf, wq, precision, s, s_stride, B, cin, cout, res, ws, ws_bytes},
                                    LaLayerEpi{d, d_stride, noise, noise_bstride, noise_strength, bias, act, alpha, gain, clamp}, fir_host, scratch, y, stream);
}

int la_modconv3x3_bwd_ex(const float* gz, const LaModconv& m, const float* xin, long xin_bstride, float* gx, float* ds_part, hipStream_t stream,
                         const LaModconvBwdOpts& o) {
    const int res = m.res;
    LA_CHECK_ARG(gz && m.w && gx, "modconv_bwd: null pointer");
    LA_CHECK_ARG(!o.seam || (m.precision != LA_PREC_F32 && xin && o.seam->ddn_part), "modconv_bwd: the fused seam needs a 16-bit contraction and xin");
    LaConvArgs a; start_args(a, m, true);
    a.in = gz; a.out = gx; a.in_pmax = o.in_pmax; a.in_pmax_nseg = o.in_nseg;
    la_conv_geom_same(a, res, 3, true);
    if (m.precision == LA_PREC_F16X2 && o.xscale) { a.acc_scale_x = o.xscale; a.acc_scale_fan = LA_XS_FAN; a.in_pmax = nullptr; }      // preset operand scale (slot rows)
    set_bwd(a, m, xin, xin_bstride, ds_part, res, o.seam);
    if (o.rows && m.precision != LA_PREC_F32) {
        const LaWindow &in = o.rows->in, &out = o.rows->out;
        LA_CHECK_ARG(in.row_lo >= 0 && in.row_hi <= res && out.row_lo >= 0 && out.row_hi <= res, "modconv_bwd: bad row windows");
        a.in_row_lo = in.row_lo; a.in_row_hi = in.row_hi; a.row_lo = out.row_lo; a.row_hi = out.row_hi;
        if (out.row_hi > 0) { a.col_lo = out.col_lo; a.col_hi = out.col_hi; }      // (gz is valid in every column here: no input column mask)
    }
    return la_conv_launch(a, stream);
}

extern "C" int la_modconv3x3_bwd_f32(const float* gz, const float* wb, const void* wq, int precision, const float* s, int s_stride, const float* xin,
                                     long xin_bstride, float* gx, float* ds_part, void* ws, size_t ws_bytes, int B, int cin, int cout, int res,
                                     hipStream_t stream) {
    return la_modconv3x3_bwd_ex(gz, LaModconv{wb, wq, precision, s, s_stride, B, cin, cout, res, ws, ws_bytes}, xin, xin_bstride, gx, ds_part, stream);
}

int la_modconv3x3_up2_bwd_ex(const float* gz, const LaModconv& m, const float* xin, long xin_bstride, const float* fir_host, float* scratch,
                             float* gx, float* ds_part, hipStream_t stream, const LaModconvBwdOpts& o) {
    const int res = m.res, B = m.B, cout = m.cout;
    const LaSeamFuse* seam = o.seam;
    const LaBwdRows* rows = o.rows;
    void* ws = m.ws;
    size_t ws_bytes = m.ws_bytes;
    LA_CHECK_ARG(gz && m.w && gx && scratch && fir_host, "modconv_up2_bwd: null pointer");
    LA_CHECK_ARG(res >= 2 && res % 2 == 0, "modconv_up2_bwd: output resolution must be even");
    LA_CHECK_ARG(!seam || (m.precision != LA_PREC_F32 && xin && seam->ddn_part && (seam->imgc == 0 || (seam->g_img && seam->wrgb && seam->s_rgb && seam->dweff_part))),
                 "modconv_up2_bwd: the fused seam needs a 16-bit contraction, xin and its output buffers");
    const int hin = res / 2;
    LaConvArgs a; start_args(a, m, true);
    a.out = gx;
    la_conv_geom_down2(a, res);
    set_bwd(a, m, xin, xin_bstride, ds_part, hin, seam);
    const size_t fused_need = 512 + ((la_fir4x4_adjoint_pack_bytes(B, cout, res, res) + 255) & ~(size_t)255);
    if (m.precision == LA_PREC_F16X2 && (o.xscale || (o.in_pmax && o.in_nseg >= 1)) && res % 4 == 0 && ws && ws_bytes > fused_need && (((size_t)ws | (size_t)gz) & 15) == 0) {
        // fp16 mode with the plane maxima of gz at hand (left by the seam kernel): ONE pass turns gz into the contraction's
        // operand -- FIR adjoint (pad 2, flipped taps, gain 4; upfirdn2d.py:255-266) + operand scale + fp16 split + channel
        // interleave.  The scale comes from the bound |adjoint(gz)| <= 4 * sum(f) * max|gz| = 4 * max|gz| (see la_upfirdn2d.hip).
        const float* xscale = o.xscale;      // (slot rows, already final: the producer of gz lowered them with the same bound, la_modconv_up2_bwd_xs_mult)
        int xs_fan = LA_XS_FAN;
        unsigned* q = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + 512);
        int rc;
        if (!xscale) {
            float* xs = static_cast<float*>(ws);
            if ((rc = la_conv_xscale_from_pmax(o.in_pmax, o.in_nseg, nullptr, 0, la_modconv_up2_bwd_xs_mult(fir_host), xs, B, cout, stream))) return rc;
            xscale = xs; xs_fan = 1;
        }
        LaWindow in_win = {}, z = {};
        if (rows) in_win = rows->in;
        if (rows && in_win.row_hi > 0) {      // rows of the adjoint that can be non-zero: 4 taps, pad 2
            LA_CHECK_ARG(in_win.row_lo >= 0 && in_win.row_hi <= res && rows->out.row_lo >= 0 && rows->out.row_hi <= hin, "modconv_up2_bwd: bad row windows");
            z.row_lo = in_win.row_lo; z.row_hi = in_win.row_hi;
            la_span_grow(z.row_lo, z.row_hi, 2, 2, res + 1);
            a.in_row_lo = z.row_lo; a.in_row_hi = z.row_hi;
        }
        if (rows) { a.row_lo = rows->out.row_lo; a.row_hi = rows->out.row_hi; }
        a.in = gz;                       // (not read: the launch takes its operand from in_q)
        a.in_q = q; a.acc_scale_x = xscale; a.acc_scale_fan = xs_fan;
        a.ws = static_cast<char*>(ws) + fused_need; a.ws_bytes = ws_bytes - fused_need;
        if (a.row_hi > 0 && in_win.row_hi > 0 && in_win.col_hi > 0) {
            // Column cone, as the rows: gz is non-zero in columns [col_lo, col_hi) only, the adjoint (4 taps, pad 2) two columns further,
            // and output column X gathers operand columns 2 X .. 2 X + 2 -- outside [x0, x1) the contraction sums zeros.  The fused seam
            // adds the ToRGB share of the image gradient one level down: the caller keeps that inside the same columns (la_synth.hip: the
            // window's tile columns hold the image columns with one to spare, which halves to less than the two taken here).  The launch
            // then computes the rectangle only and zero-fills the other columns of its rows (LaConvArgs::col_lo); the operand is packed in
            // the 64-column groups it reads.  Only the direct flat kernel follows columns: where the plan runs another form, all stay.
            int zc0 = in_win.col_lo, zc1 = in_win.col_hi;
            la_span_grow(zc0, zc1, 2, 2, res + 1);
            const int x0 = zc0 > 2 ? (zc0 - 1) >> 1 : 0, x1 = ((zc1 - 1) >> 1) + 1 < hin ? ((zc1 - 1) >> 1) + 1 : hin;
            if (x0 > 0 || x1 < hin) {
                a.col_lo = x0; a.col_hi = x1;
                LaConvPlan p;
                if ((rc = la_conv_plan(a, p))) return rc;
                if (p.form == LA_FORM_FLAT) { z.col_lo = 2 * x0; z.col_hi = 2 * x1 + 1; }
                else a.col_lo = a.col_hi = 0;
            }
        }
        if ((rc = la_fir4x4_adjoint_pack_f16(gz, q, xscale, xs_fan, B, cout, res, res, fir_host, 4.f, stream, 0, in_win, z))) return rc;
        return la_conv_launch(a, stream);
    }
    // adjoint of [pad (1,1,1,1) -> FIR] (la_fir_same_pad2, flipped)
    // (fp16 mode: the FIR kernel also leaves the plane maxima of the scratch at the head of ws, so the contraction below
    //  needs no absmax pass)
    LaFirTail t;
    const int nseg = la_fir4x4_segments(res + 1, res + 1);
    const size_t pm_bytes = ((size_t)B * cout * nseg * sizeof(float) + 255) & ~(size_t)255;
    if (m.precision == LA_PREC_F16X2 && ws && ws_bytes > pm_bytes) {
        t.pmax = static_cast<float*>(ws);
        ws = static_cast<char*>(ws) + pm_bytes;
        ws_bytes -= pm_bytes;
    }
    int rc = la_upfirdn2d_ex(gz, scratch, B, cout, res, res, fir_host, la_fir_same_pad2(1, 4.f), stream, t);
    if (rc) return rc;
    a.in = scratch; a.in_pmax = t.pmax; a.in_pmax_nseg = nseg;
    a.ws = ws; a.ws_bytes = ws_bytes;
    return la_conv_launch(a, stream);
}

// bound factor of the fused FIR-adjoint operand: |adjoint(gz)| <= 4 * sum|f| * max|gz|
float la_modconv_up2_bwd_xs_mult(const float* fir_host) {
    float fsum = 0.f;
    for (int i = 0; i < 16; ++i) fsum += fabsf(fir_host[i]);
    return 4.f * fsum;
}

extern "C" int la_modconv3x3_up2_bwd_f32(const float* gz, const float* wb, const void* wq, int precision, const float* s, int s_stride, const float* xin,
                                         long xin_bstride, const float* fir_host, float* scratch, float* gx,
                                         float* ds_part, void* ws, size_t ws_bytes, int B, int cin, int cout,
                                         int res, hipStream_t stream) {
    return la_modconv3x3_up2_bwd_ex(gz, LaModconv{wb, wq, precision, s, s_stride, B, cin, cout, res, ws, ws_bytes}, xin, xin_bstride, fir_host, scratch,
                                    gx, ds_part, stream);
}

extern "C" int la_modconv_ds_tiles(int grid_res) { return la_conv_tiles_per_sample(grid_res, grid_res); }

// scratch bytes for a layer's forward and backward launches at any contraction precision:
// pre-split bf16 copy of the launch input (split-bf16 only) + split-K slice partials (<= 34x34 grids).
extern "C" size_t la_modconv_workspace_bytes(int B, int cin, int cout, int res, int up) {
    size_t need = 0;
    const int hin = up ? res / 2 : res, rb = up ? res + 1 : res;      // input resolution of the forward / of the backward contraction
    // forward grids: the layer's own, or the phases of the transposed conv -- fp32: one phase per launch, 16-bit: four phases' partials side by side
    const int gy[4] = {hin + up, hin + 1, hin, hin}, gx[4] = {hin + up, hin, hin + 1, hin};
    for (int prec = 0; prec <= 3; ++prec) {
        const long f = la_conv_splitk_floats_phases(B, cout, cin, up && prec ? 4 : 1, gy, gx, prec), b = la_conv_splitk_floats(B, cin, cout, hin, hin, prec);
        const size_t qf = prec ? la_conv_presplit_bytes(B, cin, hin, hin) : 0, qb = prec ? la_conv_presplit_bytes(B, cout, rb, rb) : 0;
        const size_t nf = ((qf + 255) & ~(size_t)255) + (size_t)f * 4, nb = ((qb + 255) & ~(size_t)255) + (size_t)b * 4;
        if (nf > need) need = nf;
        if (nb > need) need = nb;
    }
    // head of the workspace in la_modconv3x3_up2_bwd (fp16 mode): plane maxima of the FIR-adjoint scratch
    need += ((size_t)B * (cin > cout ? cin : cout) * la_fir4x4_segments(res + 1, res + 1) * sizeof(float) + 255) & ~(size_t)255;
    return need;
}

// split-bf16 weight packs: bytes for one direction (forward: transpose = 0, backward: transpose = 1), nterm terms
extern "C" size_t la_modconv_bf16_pack_bytes(int cin, int cout, int transpose, int /*nterm*/) {      // one pack serves every split precision (3 bf16 terms + 2 fp16 terms + the fp16 weight scale)
    return la_conv_split_pack_bytes(transpose ? cin : cout, transpose ? cout : cin, 9);
}

extern "C" int la_pack_conv_weights_bf16_f32(const float* w, void* out, int cout, int cin, int ktaps, int transpose,
                                             int nterm, hipStream_t stream) {
    return la_pack_conv_weights_bf16(w, out, cout, cin, ktaps, transpose, nterm, stream);
}
