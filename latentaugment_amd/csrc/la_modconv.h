// Modulated 3x3 conv: the internal (C++) variants of the entry points of include/latentaug_hip.h.
#pragma once
#include "la_common.h"
#include "la_conv.h"
#include "la_style.h"

// The contraction of one launch: which weights, which arithmetic, the styles, the layer's shape and the caller's scratch.
struct LaModconv {
    const float* w;          // packed fp32 slabs of the direction of the call: forward (wf) or backward (wb)
    const void* wq;          // 16-bit split pack of the same direction
    int precision;
    const float* s; int s_stride;      // styles [B][s_stride]
    int B, cin, cout, res;   // res: resolution of the layer's output
    void* ws; size_t ws_bytes;
};
// Options of the forward calls, all off by default:
//   in_pmax [B][cin][in_nseg]: partial max |input| per plane, written by the kernel that produced the input (same-resolution call)
//   xscale  [B][LA_XS_FAN] slot rows: preset power-of-two fp16 operand scale of the input -- no absmax / plane-maxima pass
//   rgb     ToRGB of the block fused into the epilogue (LaConvArgs::rgb; same-resolution call, la_modconv3x3_fwd_fuses_rgb)
//   xs_out / xs_mult  the operand scale of y for the contraction that consumes it (LaConvArgs::fwd_xs_out / fwd_xs_mult)
//   win     window of y, a hint: rows (columns) outside it may or may not be written.  Up-sampling call (column-planar scratch only): the FIR
//           writes exactly these rows and the 4-column groups of these columns, the transposed conv (direct flat kernel) the rectangle of
//           every phase of its intermediate that they read -- the rest of the scratch is neither written nor read
//           (la_modconv3x3_up2_fwd_rows: the input rows such a call reads)
//   y_pmax  (up-sampling call) [B][cout][la_fir4x4_segments(res, res)]: partial max |y| per plane, written by the FIR epilogue
//   scratch_pitch / scratch_xhalf (up-sampling call; floats; both 0 = dense (res+1)-wide rows, or both set): COLUMN-PLANAR rows of the
//           transposed-conv intermediate -- the even output columns of a row at [0, res/2 + 1), the odd ones from scratch_xhalf on (a
//           multiple of 4, scratch_pitch >= scratch_xhalf + res/2) -- so that every output phase of the transposed conv stores contiguous
//           runs and the FIR runs its vector kernel (the scratch then holds B * cout * (res+1) * scratch_pitch floats)
struct LaModconvFwdOpts {
    const float* in_pmax = nullptr; int in_nseg = 0;
    const float* xscale = nullptr;
    const LaRgbFuse* rgb = nullptr;
    float* xs_out = nullptr; const float* xs_mult = nullptr;
    LaWindow win = {};
    float* y_pmax = nullptr;
    int scratch_pitch = 0, scratch_xhalf = 0;
};
bool la_modconv3x3_fwd_fuses_rgb(int precision, int B, int cin, int cout, int res);
int la_modconv3x3_fwd_ex(const float* x, long x_bstride, const LaModconv& m, const LaLayerEpi& epi, float* y, hipStream_t stream,
                         const LaModconvFwdOpts& o = LaModconvFwdOpts());
int la_modconv3x3_up2_fwd_ex(const float* x, long x_bstride, const LaModconv& m, const LaLayerEpi& epi, const float* fir_host, float* scratch,
                             float* y, hipStream_t stream, const LaModconvFwdOpts& o = LaModconvFwdOpts());
void la_modconv3x3_up2_fwd_rows(int res, int row_lo, int row_hi, int* in_lo, int* in_hi);

// Windows of a backward launch (la_synth.hip): `in` = the valid part of gz -- the rest holds older contents of a shared buffer where the
// gradient is exactly zero, and reads as zeros -- and `out` = the wanted part of gx (tiles outside write nothing but zero their
// style-gradient partials).  16-bit direct kernels; other forms ignore them.
struct LaBwdRows { LaWindow in, out; };
// Options of the backward calls, all off by default:
//   in_pmax [B][cout][in_nseg]: partial max |gz| per plane (left by the seam kernel); with it the up-sampling call in fp16 mode builds the
//           contraction's operand in one fused pass (FIR adjoint + scale + split + interleave)
//   seam    backward seam of the layer whose saved output is xin, applied in the epilogue (LaConvArgs::seam); up-sampling call: the seam of
//           the block BELOW, incl. its ToRGB backward
//   xscale  [B][LA_XS_FAN] slot rows: the fp16 operand scale of gz, already final when this launch starts (left by the producer of gz through
//           LaSeamFuse::xs_out / LaSeamArgs::xs_out) -- no plane-maxima reduction launch
//   rows    up-sampling call (fused fp16 path only): in = valid part of gz (res rows), out = window of gx (res/2 rows); the FIR adjoint then
//           writes the rows of its (res+1)-row result that can be non-zero, [in.row_lo - 2, in.row_hi + 2), and the contraction reads the others as zeros.
//           With in.col_* (gz, and the image gradient behind a fused ToRGB seam, are zero outside those columns) the contraction computes only
//           the columns of gx where the gradient can be non-zero and writes exact zeros into the others of its rows
struct LaModconvBwdOpts {
    const float* in_pmax = nullptr; int in_nseg = 0;
    const LaSeamFuse* seam = nullptr;
    const float* xscale = nullptr;
    const LaBwdRows* rows = nullptr;
};
int la_modconv3x3_bwd_ex(const float* gz, const LaModconv& m, const float* xin, long xin_bstride, float* gx, float* ds_part, hipStream_t stream,
                         const LaModconvBwdOpts& o = LaModconvBwdOpts());
int la_modconv3x3_up2_bwd_ex(const float* gz, const LaModconv& m, const float* xin, long xin_bstride, const float* fir_host, float* scratch,
                             float* gx, float* ds_part, hipStream_t stream, const LaModconvBwdOpts& o = LaModconvBwdOpts());

float la_modconv_up2_bwd_xs_mult(const float* fir_host);      // the `mult` of the operand scale an up layer's backward expects (LaSeamFuse::xs_mult)
