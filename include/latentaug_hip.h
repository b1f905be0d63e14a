/* latentaug_hip.h -- C ABI of liblatentaug_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the latent-optimisation hot path of ltronchin/LatentAugment.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repository root).
 *
 * This file is the only copy of the ABI: the library's sources are compiled against it (a definition that disagrees does not build)
 * and the Python binding (latentaugment_amd/_lib.py) reads its prototypes and structs from it.  Keep the style it parses: C comments
 * only, one `ret name(type name, ...);` per entry with every parameter named, scalars of int / long / float / double / size_t /
 * unsigned / unsigned long long.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is DEVICE memory (fp32, contiguous NCHW) unless its name ends
 *     in `_host`; the caller has selected the device and owns every buffer; nothing here allocates device memory.
 *   - workspaces (`ws`, `workspace`, `scratch`, the sign buffer `so`, the mapping's `tmp`): a workspace may hold ANY bytes when it is
 *     handed over -- no entry relies on zeros or on what an earlier call left, except where an entry says that it continues another
 *     on the same workspace (la_fd_gram_f32 -> la_fd_jacobi_sweep_f64 -> la_fd_finish_f64; the passes of one engine handle) -- and
 *     nothing outside [base, base + bytes) is written, `bytes` being what the entry's la_*_workspace_bytes / _floats reports (or the
 *     `workspace_bytes` passed, where that is smaller and still accepted).  Outputs are written in full and nowhere else.
 *     An engine whose create clears its workspace (la_synth_create) meets the first half that way; the others re-arm what a pass
 *     accumulates into before the pass does ("Workspace contract"; tests/test_hip_workspace_guard.py).
 *   - History contract (engine and loop handles: la_synth, la_disc, la_feat, la_latent_opt).  The results of a pass depend on its inputs and
 *     on the handle's CURRENT settings only, bit for bit: not on the batch sizes, windows, precisions, schedules, traces, captured graphs or
 *     values of earlier passes on the handle.  A backward pass uses the settings its forward pass ran with (precision, window, ToRGB
 *     schedule): a setter takes effect at the next forward pass.  A refused call (LA_ERR_ARG before any launch) changes nothing.  A setter
 *     of an engine attached to a loop handle takes effect at the loop's next run: a captured step of the old settings is never replayed.
 *     ("Handle history"; tests/test_hip_history.py.)
 *   - all work is enqueued on `stream` (a hipStream_t, passed as void* from foreign code); no host<->device sync.
 *   - return 0 on success, negative on failure (LA_ERR_*); la_last_error() gives the thread's last message.
 *     This replaces the TORCH_CHECKs of the reference bindings (bias_act.cpp:35-51, upfirdn2d.cpp:19-40).
 *   - re-entrant: the only global mutable state is the thread-local error string (cf. bias_act.cpp:54,88), a once-per-device
 *     "kernel attribute set" flag (atomic) and the opt-in launch profiler la_prof_* (off by default; ONE process-wide instance
 *     that is not thread-safe: measurement runs only).  No kernel-variant switches, no environment variables (see la_prof_*).
 */
#ifndef LATENTAUG_HIP_H
#define LATENTAUG_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef LA_STREAM_T
#define LA_STREAM_T
typedef struct ihipStream_t* la_stream_t; /* == hipStream_t */
#endif

#define LA_OK 0
#define LA_ERR_ARG (-1)       /* bad argument / unsupported configuration */
#define LA_ERR_HIP (-2)       /* a HIP runtime call failed (see la_last_error) */
#define LA_ERR_WORKSPACE (-3) /* caller-provided workspace too small */

/* activation ids = the reference's cuda_idx (torch_utils/ops/bias_act.py:20-30) */
#define LA_ACT_LINEAR 1
#define LA_ACT_RELU 2
#define LA_ACT_LRELU 3

const char* la_last_error(void);
int la_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * L0 ops -- replace the pybind plugins of models/stylegan3/torch_utils/ops/
 * ------------------------------------------------------------------------------------------------------------- */

/* bias_act forward.  Replaces bias_act_plugin.bias_act(x,b,xref,yref,dy,grad=0,dim,act,alpha,gain,clamp)
 * (bias_act.cpp:32-90, kernel bias_act.cu:23-147).  Element i takes b[(i / stepb) % nb]; for NCHW and dim=1:
 * stepb = H*W, nb = C.  b may be NULL.  clamp < 0 disables clamping. */
int la_bias_act_f32(const float* x, const float* b, float* y, long n, long stepb, int nb, int act, float alpha,
                    float gain, float clamp, la_stream_t stream);

/* bias_act first-order backward (grad=1 of the same plugin; python side bias_act.py:155-177):
 * dx = dy * act'(.) taken from the saved OUTPUT yref (sign for lrelu, zero where |yref| >= clamp), db[c] = sum dx. */
int la_bias_act_grad_f32(const float* dy, const float* yref, float* dx, float* db, long n, long stepb, int nb, int act,
                         float alpha, float gain, float clamp, la_stream_t stream);

/* The general form of the same plugin entry point (bias_act.cpp:32 `bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)`):
 * every activation of bias_act.py:20-30 (act = its cuda_idx 1..9: linear relu lrelu tanh sigmoid elu selu softplus swish) and grad = 0
 * (forward), 1 (x = incoming gradient: x * f' * gain * dy) or 2 (x = gradient of the gradient: x * f'' * gain * dy); f', f'' are formed
 * from yref / gain (swish: from xref + b), results are zero where |yref| >= clamp.  b / xref / yref / dy may be NULL ("absent", the
 * reference's empty tensors); dim enters as (stepb, nb): element i belongs to bias entry (i / stepb) % nb. */
int la_bias_act_ex_f32(const float* x, const float* b, const float* xref, const float* yref, const float* dy, float* out, long n,
                       long stepb, int nb, int grad, int act, float alpha, float gain, float clamp, la_stream_t stream);
/* db [nb] = sum of dx over every axis but the bias axis (what bias_act.py:187,206 forms with Tensor.sum): element i -> (i / stepb) % nb. */
int la_bias_sum_f32(const float* dx, float* db, long n, long stepb, int nb, la_stream_t stream);
/* The same two entries for the reference plugin's other storage types (AT_DISPATCH_FLOATING_TYPES_AND_HALF, bias_act.cpp:77): argument
 * order, (stepb, nb), grad, activation ids, NULL conventions and checks as la_bias_act_ex_f32 / la_bias_sum_f32.
 *   _f16: IEEE binary16 storage (x, b, xref, yref, dy, out, db), fp32 arithmetic with one rounding on store (the plugin's
 *         InternalType<half> = float), float scalars; db is summed in fp32 and rounded once.  With grad >= 1 the clamp test compares
 *         yref with the clamp rounded to binary16, the value a clamped output holds.
 *   _f64: double storage and arithmetic with DOUBLE alpha / gain / clamp (the reference's impl='ref' path applies them as doubles). */
int la_bias_act_ex_f16(const unsigned short* x, const unsigned short* b, const unsigned short* xref, const unsigned short* yref,
                       const unsigned short* dy, unsigned short* out, long n, long stepb, int nb, int grad, int act, float alpha, float gain,
                       float clamp, la_stream_t stream);
int la_bias_sum_f16(const unsigned short* dx, unsigned short* db, long n, long stepb, int nb, la_stream_t stream);
int la_bias_act_ex_f64(const double* x, const double* b, const double* xref, const double* yref, const double* dy, double* out, long n,
                       long stepb, int nb, int grad, int act, double alpha, double gain, double clamp, la_stream_t stream);
int la_bias_sum_f64(const double* dx, double* db, long n, long stepb, int nb, la_stream_t stream);

/* upfirdn2d.  Replaces upfirdn2d_plugin.upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)
 * (upfirdn2d.cpp:16-98, kernels upfirdn2d.cu:29-200).  f_host: fh*fw taps in HOST memory (<= 8x8), as produced by
 * setup_filter (upfirdn2d.py:70-114).  Output size per axis: la_upfirdn2d_out_size (upfirdn2d.cpp:35-36).
 * The backward of the op is the same op with up<->down swapped, flip negated and the pads of upfirdn2d.py:255-266. */
int la_upfirdn2d_out_size(int in_size, int up, int down, int pad0, int pad1, int taps);
int la_upfirdn2d_f32(const float* x, const float* f_host, float* y, int N, int C, int H, int W, int fh, int fw, int upx,
                     int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                     la_stream_t stream);
/* upfirdn2d for the plugin's other storage types (upfirdn2d.cpp:63); arguments, limits (<= 8x8 taps, or one separable pass of
 * <= 32) and error messages as la_upfirdn2d_f32.  The taps stay float32 host values for every type (upfirdn2d.cpp:21).
 *   _f16: binary16 x / y, fp32 accumulation, one rounding on store.
 *   _f64: double x / y, the taps widened exactly, double arithmetic and a DOUBLE gain. */
int la_upfirdn2d_f16(const unsigned short* x, const float* f_host, unsigned short* y, int N, int C, int H, int W, int fh, int fw,
                     int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                     la_stream_t stream);
int la_upfirdn2d_f64(const double* x, const float* f_host, double* y, int N, int C, int H, int W, int fh, int fw, int upx, int upy,
                     int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, double gain, la_stream_t stream);

/* filtered_lrelu.  Replaces filtered_lrelu_plugin.filtered_lrelu(x,fu,fd,b,si,up,down,px0,px1,py0,py1,sx,sy,gain,slope,clamp,
 * flip_filters,writeSigns) (filtered_lrelu.cpp:16-18; the nine steps of filtered_lrelu.py:59-108): per (n, c) plane
 *   y = down-FIR fd + decimate by `down` ( clamp( lrelu( gain * up-FIR fu with gain up^2 ( pad ( zero-insert up ( x + b[c] ))))))
 * x [N][C][H][W] -> y [N][C][OH][OW], OW = la_filtered_lrelu_out_size(W, up, down, px0, px1, fu_w, fd_w) (same for OH).
 *   fu [fu_h][fu_w], fd [fd_h][fd_w]: taps in DEVICE memory (so the call needs no host copy and can be captured in a graph).  fu_h == 0
 *     (fd_h == 0) passes a 1-D filter of fu_w taps, applied along both axes (the plugin's fuShape.y == 0).  NULL = the 1 x 1 identity
 *     (its sizes are then ignored).  At most 64 taps per axis.
 *   b [C] (device) or NULL; clamp = +INFINITY disables the clamp; flip = 1: correlation, 0: convolution.
 *   Up, down, taps in the envelope of the fused kernel (up, down in {1, 2, 4}, <= 8 * up taps of fu and <= 8 * down taps of fd per
 *   axis) run as one launch that keeps the up-sampled intermediate on chip; any other valid call runs on a direct (slow) kernel.
 * Signs.  The intermediate after the up-FIR ("mid", active extent ah x aw = ((OH - 1) * down + fd rows) x ((OW - 1) * down + fd_w))
 * can be recorded in a sign buffer of 2 bits per sample: bit 0 = negative (gain * value < 0), bit 1 = clamped (|lrelu| > clamp).
 * Layout: per plane `rows` rows of `row_bytes` bytes (la_filtered_lrelu_sign_shape; the buffer is N * C * rows * row_bytes bytes);
 * sample t of a row sits in bits 2 * (t % 4) .. 2 * (t % 4) + 1 of byte t / 4.  The layout is the same for the forward call and for
 * the backward call below (and every higher order), so one buffer serves them all.
 *   write_signs = 1: the samples of the active extent are written to `so` (si must be NULL, sx = sy = 0); the bytes past it are not.
 *   si != NULL: read mode -- the activation stage multiplies mid sample (ty, tx) by the stored derivative of sample (ty + sy, tx + sx):
 *     gain, gain * slope, or 0 where it was clamped (and gain outside the buffer), instead of evaluating lrelu and the clamp.
 * Backward (filtered_lrelu.py:239-268): dx = the same call on dy in read mode with fu <-> fd, up <-> down, padding
 *   [fu_w - 1 + fd_w - 1 - px0, W * up - OW * down + px0 - (up - 1), (same for y)], gain * up^2 / down^2, flip negated, no clamp,
 *   sx - (fu_w - 1) + px0, sy - (fu rows - 1) + py0.  That call is linear in dy, so the same recipe gives every higher order.
 * Arguments are checked on the host before any launch (the TORCH_CHECKs of filtered_lrelu.cpp:21-79; LA_ERR_ARG + la_last_error). */
int la_filtered_lrelu_f32(const float* x, const float* fu, const float* fd, const float* b, const unsigned char* si, unsigned char* so,
                          float* y, int N, int C, int H, int W, int fu_h, int fu_w, int fd_h, int fd_w, int up, int down, int px0, int px1,
                          int py0, int py1, int sx, int sy, float gain, float slope, float clamp, int flip, int write_signs,
                          la_stream_t stream);
/* filtered_lrelu_act_ of the plugin (filtered_lrelu.cpp:213): x [N][C][H][W] IN PLACE = clamp(lrelu(gain * x)), or gain * x times the
 * derivative read from si at (h + sy, w + sx) (read mode).  Sign buffer: per plane H rows of 4 * ceil(W / 16) bytes, same bit layout. */
int la_filtered_lrelu_act_f32(float* x, const unsigned char* si, unsigned char* so, int N, int C, int H, int W, int sx, int sy, float gain,
                              float slope, float clamp, int write_signs, la_stream_t stream);
/* pure host queries: output size per axis, (in * up + pad0 + pad1 - (fu_taps - 1) - (fd_taps - 1) + (down - 1)) // down (floor; the
 * formula of filtered_lrelu.py:141-142), and the sign buffer of a call: *rows rows per plane of *row_bytes bytes (LA_ERR_ARG if the
 * call is invalid).  fu_h / fd_h == 0: 1-D filters. */
int la_filtered_lrelu_out_size(int in_size, int up, int down, int pad0, int pad1, int fu_taps, int fd_taps);
int la_filtered_lrelu_sign_shape(int H, int W, int fu_h, int fu_w, int fd_h, int fd_w, int up, int down, int px0, int px1, int py0, int py1,
                                 int* rows, int* row_bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * conv2d / conv_transpose2d with data and weight gradients: the pair under conv2d_resample
 * (torch_utils/ops/conv2d_gradfix.py:24-33, conv2d_resample.py:26-40).  float32, dense NCHW.
 * ------------------------------------------------------------------------------------------------------------- */

/* y = conv(x, w).  x [B][Cin][H][W], y [B][Cout][Hout][Wout], the same stride on both axes, padding pady / padx >= 0.
 *   transpose == 0: w [Cout][Cin/groups][kh][kw], Hout = (H + 2 pady - kh) / stride + 1 (torch.nn.functional.conv2d)
 *   transpose != 0: w [Cin][Cout/groups][kh][kw], (H-1) stride - 2 pady + kh <= Hout < that + stride: the excess is the output
 *                   padding (torch.nn.functional.conv_transpose2d)
 *   flip_weight != 0: correlation, w used as it is (what torch computes; the reference's flip_weight=True); 0: w flipped on both axes.
 * The data gradient of a call is the same entry with `transpose` toggled, x := dy, the same w and the two shapes exchanged.
 * Limits: kh, kw <= 7, stride <= 8; anything beyond is refused.  kh*kw <= 9, stride <= 2 and Cout/groups % 4 == 0 run on the MFMA
 * contraction engine (la_conv2d_uses_engine), everything else on a direct-form kernel.
 * ws: la_conv2d_workspace_bytes(0, ...) bytes of 16-byte aligned scratch (packed weights, split-K partials). */
int la_conv2d_f32(const float* x, const float* w, float* y, void* ws, size_t ws_bytes, int B, int Cin, int H, int W, int Cout, int kh, int kw,
                  int Hout, int Wout, int stride, int pady, int padx, int groups, int flip_weight, int transpose, la_stream_t stream);
/* dw (the shape of w) = gradient of <dy, conv(x, w)> with respect to w; every argument means what it means in la_conv2d_f32, x and
 * dy [B][Cout][Hout][Wout] being that call's input and output.  kh*kw <= 9 and stride <= 2: split-K fp32-MFMA kernel whose slices
 * are summed in a fixed order; otherwise one workgroup per element with a fixed-order tree.  Bit-identical from run to run.
 * ws: la_conv2d_workspace_bytes(1, ...) bytes. */
int la_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int B, int Cin, int H, int W, int Cout,
                        int kh, int kw, int Hout, int Wout, int stride, int pady, int padx, int groups, int flip_weight, int transpose,
                        la_stream_t stream);
/* pure host queries.  op: 0 = la_conv2d_f32, 1 = la_conv2d_wgrad_f32.  Scratch bytes of a call (never 0, non-decreasing in B);
 * whether a call runs on the engine / MFMA path (1) or the direct-form one (0); K slices of an MFMA weight gradient (0: direct form). */
size_t la_conv2d_workspace_bytes(int op, int B, int Cin, int H, int W, int Cout, int kh, int kw, int Hout, int Wout, int stride, int groups,
                                 int transpose);
int la_conv2d_uses_engine(int op, int cout, int kh, int kw, int stride, int groups);
int la_conv2d_wgrad_slices(int B, int Cin, int H, int W, int Cout, int kh, int kw, int Hout, int Wout, int stride, int groups, int transpose);

/* ---------------------------------------------------------------------------------------------------------------
 * grid_sample and fma: the last two modules of torch_utils/ops/ (grid_sample_gradfix.py, fma.py).
 * ------------------------------------------------------------------------------------------------------------- */

/* torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False) in 2-D, the only form
 * grid_sample_gradfix.py:28-31 provides.  x [N][C][H][W], grid [N][Ho][Wo][2] = (x, y) in [-1, 1], y [N][C][Ho][Wo], contiguous.
 * Pixel position of a grid value g along an axis of `size` pixels: ((g + 1) * size - 1) / 2; the four neighbouring pixels are read, one
 * outside the image contributes nothing.  A position outside [-1, size) -- huge, infinite or NaN included -- is tested in floating
 * point before any integer is formed from it: it reads and writes no memory, y = 0 and dgrid = 0 there.
 * Every tensor of a call must have at most INT_MAX elements; a larger shape is LA_ERR_ARG, never truncated.
 *   _f16: binary16 storage, fp32 arithmetic, one rounding on store.   _f64: double throughout. */
int la_grid_sample_f32(const float* x, const float* grid, float* y, int N, int C, int H, int W, int Ho, int Wo, la_stream_t stream);
int la_grid_sample_f16(const unsigned short* x, const unsigned short* grid, unsigned short* y, int N, int C, int H, int W, int Ho, int Wo,
                       la_stream_t stream);
int la_grid_sample_f64(const double* x, const double* grid, double* y, int N, int C, int H, int W, int Ho, int Wo, la_stream_t stream);
/* aten::grid_sampler_2d_backward(dy, x, grid, 0, 0, False, output_mask) (grid_sample_gradfix.py:60-63) as one launch.  dx (the shape of
 * x) and dgrid (the shape of grid) may each be NULL: that output is then not computed (torch's output_mask); x may be NULL when dgrid
 * is.  dgrid is summed over the channels in registers: bit-identical from run to run.  dx is zeroed by the entry and then summed with
 * global float atomic adds, so its last bits can depend on arrival order (no other sum of this library does).  The gradient of dx with
 * respect to dy is la_grid_sample_* applied to the incoming gradient; nothing is defined for second derivatives that involve grid
 * (grid_sample_gradfix.py:70-81).
 *   _f16: dx is accumulated in ws, la_grid_sample_grad_workspace_floats(N, C, H, W) = N*C*H*W floats of device memory (0: the shape
 *   is refused), and rounded to binary16 once by a second launch; ws may be NULL when dx is. */
int la_grid_sample_grad_f32(const float* dy, const float* x, const float* grid, float* dx, float* dgrid, int N, int C, int H, int W, int Ho,
                            int Wo, la_stream_t stream);
int la_grid_sample_grad_f16(const unsigned short* dy, const unsigned short* x, const unsigned short* grid, unsigned short* dx,
                            unsigned short* dgrid, float* ws, int N, int C, int H, int W, int Ho, int Wo, la_stream_t stream);
int la_grid_sample_grad_f64(const double* dy, const double* x, const double* grid, double* dx, double* dgrid, int N, int C, int H, int W,
                            int Ho, int Wo, la_stream_t stream);
long la_grid_sample_grad_workspace_floats(int N, int C, int H, int W);

/* fma.py:15 `fma(a, b, c)`: y = a * b + c (one fused multiply-add per element) over the broadcast shape shape_host[4] (HOST memory,
 * operands of lower rank left-padded with 1s).  astride_host / bstride_host / cstride_host [4] (HOST): element strides of each operand,
 * 0 along an axis it broadcasts; y is contiguous.  c NULL = 0 (cstride_host is then ignored).  At most INT_MAX elements. */
int la_fma_f32(const float* a, const float* b, const float* c, float* y, const long* shape_host, const long* astride_host,
               const long* bstride_host, const long* cstride_host, la_stream_t stream);
/* _unbroadcast of fma.py:49-58: x contiguous of shape_host[4] -> out contiguous of out_shape_host[4] (both HOST), every axis of which is
 * either the input's (kept) or 1 (summed).  Terms are added in double, in an order that depends on the shapes alone, and rounded once:
 * bit-identical from run to run.  At most INT_MAX elements. */
int la_unbroadcast_sum_f32(const float* x, float* out, const long* shape_host, const long* out_shape_host, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Modulated 3x3 convolution of a SynthesisLayer (the SG2 `modulated_conv2d` + `bias_act` pair that the reference
 * reaches through G.synthesis, util_latent_aug.py:227; resampling algebra conv2d_resample.py:82-134).
 * Non-fused formulation: y = act((W * (x.s)) . d + noise + bias); never materialises per-sample weights.
 * ------------------------------------------------------------------------------------------------------------- */

/* W[cout][cin][ktaps] -> wf[t][cin][cout] (forward A-operand), wb[t][cout][cin] (backward), wsq[cout][cin] = sum_t W^2.
 * Any of wf/wb/wsq may be NULL. */
int la_pack_conv_weights_f32(const float* w, float* wf, float* wb, float* wsq, int cout, int cin, int ktaps,
                             la_stream_t stream);

/* same-resolution layer (conv1): x [B][cin][res][res] (x_bstride = 0 broadcasts one sample), s [B][s_stride] styles,
 * d [B][d_stride] demodulation coefficients (NULL = no demod), noise [res][res] (noise_bstride 0) or per sample. */
int la_modconv3x3_fwd_f32(const float* x, long x_bstride, const float* wf, const void* wq, int precision, const float* s, int s_stride, const float* d,
                          int d_stride, const float* noise, long noise_bstride, float noise_strength, const float* bias,
                          int act, float alpha, float gain, float clamp, float* y, void* ws, size_t ws_bytes, int B, int cin, int cout, int res,
                          la_stream_t stream);

/* up-sampling layer (conv0): x [B][cin][res/2][res/2] -> y [B][cout][res][res];
 * scratch: B*cout*(res+1)^2 floats (the transposed-conv intermediate of conv2d_resample.py:125).
 * All four entries: square images of any resolution >= 1 for the same-resolution calls, of any EVEN resolution >= 2 for the two
 * up-sampling calls (an odd one is LA_ERR_ARG); cout (forward) / cin (backward), the row count of the contraction, must be a multiple of 4. */
int la_modconv3x3_up2_fwd_f32(const float* x, long x_bstride, const float* wf, const void* wq, int precision, const float* s, int s_stride,
                              const float* d, int d_stride, const float* noise, long noise_bstride, float noise_strength,
                              const float* bias, int act, float alpha, float gain, float clamp, const float* fir_host,
                              float* scratch, float* y, void* ws, size_t ws_bytes, int B, int cin, int cout, int res, la_stream_t stream);

/* backward-data + style-gradient partials.  gz [B][cout][res][res] = gradient w.r.t. the raw contraction (already
 * multiplied by d and by act').  gx = (W^T * gz) . s ;  ds_part[b][i][tile] = partial sums of sum_p (W^T*gz) . xin.
 * ds_part [B][cin][la_modconv_ds_tiles(grid)] (grid = res, up-sampling call: res / 2) needs no initialisation: every kernel form writes
 * every slot (the split-K finish pass puts the sum into tile 0 and zeros into the others). */
int la_modconv3x3_bwd_f32(const float* gz, const float* wb, const void* wq, int precision, const float* s, int s_stride, const float* xin,
                          long xin_bstride, float* gx, float* ds_part, void* ws, size_t ws_bytes, int B, int cin, int cout, int res,
                          la_stream_t stream);
int la_modconv3x3_up2_bwd_f32(const float* gz, const float* wb, const void* wq, int precision, const float* s, int s_stride, const float* xin,
                              long xin_bstride, const float* fir_host, float* scratch, float* gx, float* ds_part, void* ws, size_t ws_bytes, int B,
                              int cin, int cout, int res, la_stream_t stream);
int la_modconv_ds_tiles(int grid_res); /* leading dimension of ds_part for a backward over a grid_res^2 grid */
/* ws (may be NULL for precision 0): scratch of la_modconv_workspace_bytes() bytes, 16-byte aligned.  With it, layers of <= 34x34 split
 * their K loop over workgroups (deterministic slice sum) instead of serialising it on a few CUs; the split-bf16
 * precisions also park the pre-split copy of the launch input there.  Precisions 1-3 REQUIRE it wherever that copy is made -- every
 * call except the same-resolution ones at res % 32 == 0, res >= 64 (precision 3 keeps its operand scales there even then) -- and take
 * at most 64 samples per call: a NULL or too small ws, or B > 64, is LA_ERR_ARG.  A ws that holds the copy but not the slice partials
 * is valid: the call then runs its direct kernels. */
size_t la_modconv_workspace_bytes(int B, int cin, int cout, int res, int up);
/* Contraction precision (the `precision` argument of the la_modconv3x3_* calls; `wq` = weights packed for it or NULL):
 *   0 LA_PREC_F32     exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *   1 LA_PREC_BF16X3  fp32 operands split into 3 bf16 terms, 6 bf16 MFMAs per product, fp32 accumulate (fp32-class error)
 *   2 LA_PREC_BF16X2  2 bf16 terms, 3 bf16 MFMAs (~4e-6 relative error per layer)
 *   3 LA_PREC_F16X2   operands scaled by per-sample / per-layer powers of two and split into 2 fp16 terms, 3 fp16 MFMAs per
 *                     product, fp32 accumulate (fp32-class error: 2 x 11 mantissa bits)
 * Magnitude range of LA_PREC_F16X2.  Every scale is 2^s with s = 15 - e, e the binary exponent of the largest magnitude max = f * 2^e
 * (f in [0.5, 1)) of the weight tensor, or of ONE SAMPLE of the (modulated) launch input, so that the scaled maximum lies in
 * [2^14, 2^15); s is clamped to [-100, 100], and a maximum that is zero, NaN or infinite gives the scale 1.  The fp32-class claim
 * therefore holds while 2^-86 <= max < 2^115 for the weights and for every sample, and while products and sums stay normal float32
 * numbers: inside that range multiplying x, gz, xin or W by a power of two (one per sample for the inputs) multiplies y, gx and
 * ds_part by the same power of two BIT FOR BIT, at every precision (tests/test_hip_operand_range.py).  Below 2^-86 the clamp leaves
 * the scaled maximum under 2^14 and bits are lost in proportion; from 2^115 on fp16 overflows.  An element far below its sample's
 * maximum keeps 22 significand bits down to about 2^-16 of that maximum and loses one bit per further halving (fp16 subnormals), as
 * in any block-scaled format.  A sample (or a weight tensor) that is entirely zero is exact: the products are zero, the scale 1 is
 * never divided by, and the forward calls return act(noise * noise_strength + bias), the backward calls 0 in gx and ds_part.
 * wq is produced by la_pack_conv_weights_bf16_f32 (transpose = 0 for the forward calls, 1 for the backward calls). */
#define LA_PREC_F32 0
#define LA_PREC_BF16X3 1
#define LA_PREC_BF16X2 2
#define LA_PREC_F16X2 3
size_t la_modconv_bf16_pack_bytes(int cin, int cout, int transpose, int nterm);
int la_pack_conv_weights_bf16_f32(const float* w, void* out, int cout, int cin, int ktaps, int transpose, int nterm,
                                  la_stream_t stream);
/* Host only, no launch, usable without a GPU.  The kernel form that ONE contraction launch of these calls takes: C = contraction depth,
 * M = rows (a multiple of 4), geom = the launch geometry at output resolution res, have_in_q != 0 = the launch input was split up
 * front (the merged up-sampling launch), ws_bytes = what the caller hands to the launch.  The library decides with the same function
 * when it launches.  info[LA_CONV_PLAN_NINFO]: profiler class (the index of la_prof_end_classes), row tile, LA_CONV_MFMA_*, K slices
 * (1 = direct), a pre-split copy of the input is read (0 / 1), merged phases (0 / 1), operand-preparation brackets of the launch
 * (0 / 1), the grid x / y / z of the contraction launch, and the workspace bytes taken in front of the split-K partials.  A launch that
 * would be refused is refused here with the same code and message. */
#define LA_CONV_GEOM_SAME_FWD 0   /* 3x3 conv at res^2 ... */
#define LA_CONV_GEOM_SAME_BWD 1   /* ... and its backward-data contraction */
#define LA_CONV_GEOM_DOWN2 2      /* stride-2 3x3 gather over (res+1)^2 onto (res/2)^2: backward of the up-sampling layer */
#define LA_CONV_GEOM_UP2_PHASE 3  /* + 2 * py + px: one output phase of the transposed stride-2 conv of a (res/2)^2 input ... */
#define LA_CONV_GEOM_UP2_MERGED 7 /* ... and the four phases in one launch */
#define LA_CONV_MFMA_F32_32X32X2 0
#define LA_CONV_MFMA_32X32 1      /* the 16-bit formats' 32x32 forms */
#define LA_CONV_MFMA_16X16X32 2
#define LA_CONV_PLAN_CLS 0
#define LA_CONV_PLAN_MT 1
#define LA_CONV_PLAN_MFMA 2
#define LA_CONV_PLAN_KSPLIT 3
#define LA_CONV_PLAN_PRESPLIT 4
#define LA_CONV_PLAN_MERGED 5
#define LA_CONV_PLAN_PREP 6
#define LA_CONV_PLAN_GRID 7       /* .. 9 */
#define LA_CONV_PLAN_WS_HEAD 10
#define LA_CONV_PLAN_NINFO 11
int la_conv_plan_query(int precision, int B, int C, int M, int geom, int res, int have_in_q, size_t ws_bytes, long* info);

/* ---------------------------------------------------------------------------------------------------------------
 * Criteria and optimiser
 * ------------------------------------------------------------------------------------------------------------- */

/* l2_loss_vectorized (augments/utils/util_latent_aug.py:315-361) on flattened rows: X [n][K], Y [m][K] ->
 * D [m][n] = |Y_m|^2 + |X_n|^2 - 2<Y_m,X_n> (compute_mean=False); mean_out (may be NULL) = sum(D)/(m*n)/K.
 * workspace: la_pairwise_l2_workspace_floats(n, m) floats (K-slice partials of the bank scan). */
long la_pairwise_l2_workspace_floats(int n, long m);
int la_pairwise_l2_f32(const float* X, int n, const float* Y, long m, long K, float* D, float* mean_out,
                       float* workspace, la_stream_t stream);

/* get_center_crop (augments/utils/util_dataset.py:317-323) on [planes][R][R] -> [planes][cc][cc]. */
int la_center_crop_f32(const float* src, float* dst, long planes, int R, int cc, int off, la_stream_t stream);

/* torch.optim.Adam step as used at util_latent_aug.py:213,274-276 (step is 1-based). */
int la_adam_step_f32(float* p, const float* g, float* m, float* v, long n, int step, float lr, float beta1, float beta2,
                     float eps, la_stream_t stream);

/* Unit normals for the explicit per-layer noise tensors of noise_mode='random' (the reference's SynthesisLayer draws torch.randn inside
 * G.synthesis, call site augments/utils/util_latent_aug.py:308): out [rows][row_elems]; element e of GLOBAL sample row row0 + r of
 * `layer` is a pure function of (seed, layer, row0 + r, e) -- Philox4x32-10 + Box-Muller -- so a rank generates only the rows of its
 * shard and the gathered batch does not depend on the sharding. */
int la_noise_normal_f32(float* out, long rows, long row_elems, unsigned long long seed, unsigned layer, long row0, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GeometricAugment (augments/geometric_aug.py): flip, affine and elastic warps of a float32 [B][C][H][W] batch.  x is the column index,
 * y the row index, pixel centres sit at integer coordinates.  S(img, px, py, mode) is bilinear sampling at pixel position (px, py),
 * per axis: a position that is not finite or beyond 2^23 in magnitude is refused in floating point (the output element is 0, nothing
 * is addressed); mode 0 'zeros' = the rule of la_grid_sample_* applied to the position; 1 'border' = the position clipped to
 * [0, size - 1]; 2 'reflection' = torch's for align_corners=False: reflected about -0.5 and size - 0.5 as often as needed, then
 * clipped.  No atomics anywhere: bit-identical from run to run.  Every tensor of a call has at most INT_MAX elements, B at most 65535.
 * ------------------------------------------------------------------------------------------------------------- */

/* Uniform noise of the elastic field (geometric_aug.py:122, kornia's RandomElasticTransform draws torch.rand * 2 - 1): out
 * [rows][row_elems]; element e of GLOBAL row row0 + r of `stream_id` is a pure function of (seed, stream_id, row0 + r, e) --
 * Philox4x32-10 with the counter and key layout of la_noise_normal_f32 -- so a shard draws only its rows.  The value is
 * (k + 0.5) * 2^-22 - 1 with k the top 23 bits of the word: exact in float32 and strictly inside (-1, 1). */
int la_noise_uniform_f32(float* out, long rows, long row_elems, unsigned long long seed, unsigned stream_id, long row0, la_stream_t stream);

/* Displacement field of the elastic warp (geometric_aug.py:122, kornia's elastic_transform2d): noise [B][2][H][W] -> disp [B][2][H][W],
 * disp[b][p][y][x] = alpha_p * sum_i sum_j taps[i] taps[j] noise[b][p][y + i - r][x + j - r] with r = (ntaps - 1) / 2 and noise outside
 * the image = 0; plane 0 (alpha_x) is the x displacement, plane 1 (alpha_y) the y displacement, in normalised units.  taps_host: ntaps
 * floats in HOST memory, ntaps odd and at most 63, applied in ascending order.  One launch, the row pass kept in LDS: ws is not used and
 * may be NULL.  noise and disp must not alias. */
int la_elastic_field_f32(const float* noise, const float* taps_host, int ntaps, float alpha_x, float alpha_y, float* disp, float* ws, int B, int H,
                         int W, la_stream_t stream);

/* Flip and affine as one resampling (geometric_aug.py:112,117): y[b][c][oy][ox] = S(x[b][c], Minv[b] (ox, oy, 1), mode) with minv [B][6]
 * float32 in device memory, the rows (m0 m1 m2), (m3 m4 m5) of the inverse map in pixel coordinates: px = m0 ox + m1 oy + m2,
 * py = m3 ox + m4 oy + m5.  apply [B] bytes in device memory: a sample whose byte is 0 is copied bit for bit.  x and y must not alias. */
int la_warp_affine_f32(const float* x, const float* minv, const unsigned char* apply, float* y, int B, int C, int H, int W, int mode,
                       la_stream_t stream);

/* The elastic resampling (geometric_aug.py:122): gx = clamp(-1 + 2 ox / (W - 1) + disp[b][0][oy][ox], -1, 1), gy likewise with H and plane 1
 * (0 along a one-pixel axis), position ((g + 1) * size - 1) / 2, y[b][c][oy][ox] = S(x[b][c], px, py, mode).  A NaN displacement passes
 * the clamp and is refused by S.  apply as above.  x and y must not alias. */
int la_warp_elastic_f32(const float* x, const float* disp, const unsigned char* apply, float* y, int B, int C, int H, int W, int mode,
                        la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Synthesis network engine: replaces  G.synthesis(ws, noise_mode=...)  (call sites util_latent_aug.py:227,488) and the
 * autograd backward to ws that loss.backward() (:275) runs through it.  Architecture 'skip', fp32
 * (models/stylegan3/legacy.py:122-144).
 *
 * params: flat list of device tensors in execution order (names as in legacy.py:171-203):
 *   b4:            const | conv1.{affine.weight, affine.bias, weight, bias, noise_const} | torgb.{affine.weight, affine.bias, weight, bias}
 *   b8 .. bR each: conv0.{5 tensors as above} | conv1.{5} | torgb.{4}
 * noise_strength_host: one float per SynthesisLayer in the same order.  channels[k] = channels at resolution 4<<k.
 * fir_host: the 4x4 resample filter (setup_filter([1,3,3,1])).  workspace: la_synth_workspace_bytes() of device memory,
 * owned by the caller and alive as long as the handle.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct la_synth la_synth;
int la_synth_num_ws(int img_resolution);
int la_synth_num_params(int img_resolution);
size_t la_synth_workspace_bytes(int img_resolution, int img_channels, int w_dim, const int* channels, int max_batch);
int la_synth_create(int img_resolution, int img_channels, int w_dim, const int* channels, float conv_clamp,
                    const float* const* params, int nparams, const float* noise_strength_host, int nlayers,
                    const float* fir_host, int fir_h, int fir_w, int max_batch, void* workspace, size_t workspace_bytes,
                    la_stream_t stream, la_synth** out);
void la_synth_destroy(la_synth* h);
/* contraction precision of every modulated conv of the engine (LA_PREC_*, default LA_PREC_F32).  History contract: takes effect at the
 * next la_synth_forward; a backward pass runs in the precision, window and ToRGB schedule of the forward pass it differentiates.  (Noise
 * gradients are the exception on the safe side: la_synth_backward_noise refuses them while a window is set, whatever the forward ran with.) */
int la_synth_set_precision(la_synth* h, int precision);
/* Kept for ABI compatibility, no effect since round 4 (rounds 2-3: 0 = fp16 operand scale of the forward contractions from the a-priori
 * bound conv_clamp * max|style|, 1 = from data maxima).  Every fp16 operand scale is now derived from the data of each pass by the
 * kernel that produces the tensor (slot rows lowered with atomicMin, csrc/la_common.h): no bound, no calibration, nothing to select. */
int la_synth_set_operand_scale(la_synth* h, int from_data);
/* Row window of the image for the forward passes that follow (rows [row_lo, row_hi) of img_resolution; 0, 0 = whole frames): the 16-bit
 * forward kernels of the blocks at >= 64^2 compute the rows that window depends on -- 3x3 / FIR taps and the up-sampling geometry of
 * SynthesisBlock / SynthesisLayer geometry (conv2d_resample.py:112-134, upfirdn2d.py:342-348) followed down the blocks -- and leave the other rows of every buffer as they were.  la_synth_backward is
 * unchanged and expects an image gradient that is zero outside the window. */
int la_synth_set_row_window(la_synth* h, int row_lo, int row_hi);
/* Column window on top of the row window (0, 0 = all): the top block's conv1, the FIR in front of it and the FIR adjoint behind it follow it in
 * whole 32-column tiles; every other kernel computes whole rows. */
int la_synth_set_col_window(la_synth* h, int col_lo, int col_hi);
int la_synth_get_precision(const la_synth* h);
/* per_block 0 (default): the ToRGB layers that are kernels of their own run deferred, two launches for all of them (la_synth_plan_query:
 * LA_SYNTH_SKIP_CHAIN); 1: one launch behind every block's conv1 and an up-FIR launch per skip image.  Every buffer holds the same bits. */
int la_synth_set_torgb_schedule(la_synth* h, int per_block);
/* Host only, no launch.  The backward pass of a windowed forward pass follows the CONE of the image window: window[0..1] = the rows of
 * the gradient of conv output conv_index (engine layer order) that can be non-zero for image rows [row_lo, row_hi) -- the forward windows
 * without their tile rounding; the launch that writes them rounds them outward to its own 4-row tiles -- and window[2..3] = the tile
 * columns that launch writes for image columns [col_lo, col_hi) (top block's up-sampling layer only).  0, 0 on an axis = all of it. */
int la_synth_plan_bwd_window(int img_resolution, int row_lo, int row_hi, int col_lo, int col_hi, int conv_index, int* window);
/* the rows the last la_synth_forward of a handle planned for its backward pass */
int la_synth_bwd_rows(const la_synth* h, int conv_index, int* row_lo, int* row_hi);
/* Host only, no launch, no handle, usable without a GPU.  Everything a la_synth_forward of B samples and the la_synth_backward behind it
 * decide before they launch, for an engine of this shape (channels[k] at resolution 4 << k), this precision and this image window (0, 0 on an
 * axis = all): the record both passes execute.  info[LA_SYNTH_PLAN_NINFO] holds three kinds of record.
 *   pass, info[LA_SYNTH_PLAN_*]: blocks, conv layers, B, precision; F16 = the forward contractions take their fp16 operand scales from slot
 *     rows; XS_HANDOFF = the backward ones too (else plane maxima and a reduction launch); ZT_DENSE = dense transposed-conv scratch rows (else
 *     column-planar); CONE = the backward launches follow the gradient cone of the image window.
 *   conv layer ci (engine order), info[LA_SYNTH_PLAN_LAYER(ci) + LA_SYNTH_PLAN_L_*]: FWD = row_lo, row_hi, col_lo, col_hi its forward launch
 *     computes; CONE = the rows in which the gradient of its output can be non-zero (la_synth_plan_bwd_window); WIN (0 / 1), ROWS_IN, ROWS_OUT =
 *     the tile-rounded windows (four numbers each, as FWD) its backward launch reads of that gradient and writes of the gradient of its input;
 *     SEAM = where the backward seam of its output runs: LA_SYNTH_SEAM_KERNEL, a launch of its own (a conv1's with the ToRGB backward), or
 *     LA_SYNTH_SEAM_FUSED, the epilogue of the backward contraction above it (a conv0's: conv1's of the block; a conv1's: the up-sampling layer's
 *     one block up); SEAM_PMAX / PMAX_IN = the plane-maxima buffer that seam writes / its backward contraction reads (LA_SYNTH_PMAX_*: none, the
 *     shared one, the up-sampling layers' fused seams', the conv1 layers' fused seams'); NSEG = segments of its demod-gradient, plane-maxima and
 *     (conv1) ToRGB weight-gradient partials: seam slabs or contraction tiles; NTILES = tiles of its style-gradient partials.
 *   block k, info[LA_SYNTH_PLAN_BLOCK(k) + LA_SYNTH_PLAN_B_*]: FUSE_RGB = ToRGB runs in the epilogue of conv1's launch (else the ToRGB kernel,
 *     which up-samples the skip image itself and is handed the image rows IMG_ROWS lo, hi); SKIP_UP = where the skip image of a fused ToRGB
 *     comes from, before conv1: LA_SYNTH_SKIP_LAUNCH, an up-FIR launch of its own, or LA_SYNTH_SKIP_CHAIN, the image-chain launch -- the
 *     block is then the DEFERRAL POINT of the ToRGB kernels of the blocks below it: none of them launches behind its conv1, one launch in
 *     front of this block makes rgb_pre of all of them and one their images and this skip image (skip images up to 256^2; a larger one keeps
 *     its launch behind those two.  No fused block above a ToRGB kernel: its run ends the pass); DOWN_FIR = the backward pass launches the down-FIR of the image gradient at this block; PYRAMID = and one more launch
 *     for every level below.
 * Bad arguments are refused with a message. */
#define LA_SYNTH_PLAN_NBLOCKS 0
#define LA_SYNTH_PLAN_NCONV 1
#define LA_SYNTH_PLAN_B 2
#define LA_SYNTH_PLAN_PRECISION 3
#define LA_SYNTH_PLAN_F16 4
#define LA_SYNTH_PLAN_XS_HANDOFF 5
#define LA_SYNTH_PLAN_ZT_DENSE 6
#define LA_SYNTH_PLAN_CONE 7
#define LA_SYNTH_PLAN_PASS_N 8
#define LA_SYNTH_PLAN_L_FWD 0        /* .. 3 */
#define LA_SYNTH_PLAN_L_CONE 4       /* .. 5 */
#define LA_SYNTH_PLAN_L_WIN 6
#define LA_SYNTH_PLAN_L_ROWS_IN 7    /* .. 10 */
#define LA_SYNTH_PLAN_L_ROWS_OUT 11  /* .. 14 */
#define LA_SYNTH_PLAN_L_SEAM 15
#define LA_SYNTH_PLAN_L_SEAM_PMAX 16
#define LA_SYNTH_PLAN_L_PMAX_IN 17
#define LA_SYNTH_PLAN_L_NSEG 18
#define LA_SYNTH_PLAN_L_NTILES 19
#define LA_SYNTH_PLAN_LAYER_N 20
#define LA_SYNTH_PLAN_B_FUSE_RGB 0
#define LA_SYNTH_PLAN_B_SKIP_UP 1
#define LA_SYNTH_PLAN_B_IMG_ROWS 2   /* .. 3 */
#define LA_SYNTH_PLAN_B_DOWN_FIR 4
#define LA_SYNTH_PLAN_B_PYRAMID 5
#define LA_SYNTH_PLAN_BLOCK_N 6
#define LA_SYNTH_PLAN_LAYER(ci) (LA_SYNTH_PLAN_PASS_N + LA_SYNTH_PLAN_LAYER_N * (ci))        /* ci < 24 */
#define LA_SYNTH_PLAN_BLOCK(k) (LA_SYNTH_PLAN_LAYER(24) + LA_SYNTH_PLAN_BLOCK_N * (k))       /* k < 12 */
#define LA_SYNTH_PLAN_NINFO LA_SYNTH_PLAN_BLOCK(12)
#define LA_SYNTH_SEAM_KERNEL 0
#define LA_SYNTH_SEAM_FUSED 1
#define LA_SYNTH_PMAX_NONE 0         /* 1, 2, 3: the three buffers in the order above */
#define LA_SYNTH_SKIP_LAUNCH 1       /* (0: the block has no skip image of its own) */
#define LA_SYNTH_SKIP_CHAIN 2
int la_synth_plan_query(int img_resolution, int img_channels, const int* channels, int B, int precision, int row_lo, int row_hi, int col_lo,
                        int col_hi, long* info);
/* ws element (b,l,j) = ws[b*ws_bstride + l*ws_lstride + j] (ws_lstride = 0: W space, one w per sample).
 * noise_mode 0 'none', 1 'const', 2 explicit unit-variance tensors noises[layer] [B][res][res] ('random' drawn by the caller).
 * img_out NULL: the image stays in the engine (la_synth_image). */
int la_synth_forward(la_synth* h, const float* ws, long ws_bstride, long ws_lstride, int B, int noise_mode,
                     const float* const* noises, float* img_out, la_stream_t stream);
/* d(loss)/d(ws) [B][num_ws][w_dim] from d(loss)/d(img) [B][C][R][R]; differentiates the last la_synth_forward. */
int la_synth_backward(la_synth* h, const float* g_img, float* dws, la_stream_t stream);
/* The same pass (la_synth_backward is this entry with gnoises NULL: the same launches, the same bits in dws) that also delivers the gradient
 * with respect to the per-layer noise: gnoises[layer] [B][res][res] in the engine's layer order, the gradient with respect to a unit noise
 * added to sample b of that layer, whatever noise_mode the forward pass used.  A NULL entry skips its layer; a layer whose
 * noise_strength is 0 gets zeros.  Per layer one launch of la_noise_grad_f32's kernel behind the seam that wrote the gradient of the
 * layer's raw output.  Refused (LA_ERR_ARG) while a row or column window is set (windowed passes leave rows of those buffers stale) and
 * before the first forward pass. */
int la_synth_backward_noise(la_synth* h, const float* g_img, float* dws, float* const* gnoises, la_stream_t stream);
/* gn[b][p] = strength * sum_c gz[b][c][p] / d[b * d_stride + c]: gz [B][C][HW] holds the gradient of a modulated layer's raw output times
 * the demodulation coefficient d > 0 (what the backward seams store).  float32, channels added in an order fixed by the shape (no
 * atomics: two runs give the same bits); HW a multiple of 4, gz and gn 16-byte aligned. */
int la_noise_grad_f32(const float* gz, const float* d, long d_stride, int B, int C, long HW, float strength, float* gn, la_stream_t stream);
const float* la_synth_image(const la_synth* h);
const float* la_synth_block_image(const la_synth* h, int block);
const float* la_synth_layer_output(const la_synth* h, int layer);
const float* la_synth_styles(const la_synth* h);
const float* la_synth_style_grads(const la_synth* h);
int la_synth_style_rows(const la_synth* h);

/* ---------------------------------------------------------------------------------------------------------------
 * Mapping network (rand_aug mode): replaces G.mapping(z, c=None, truncation_psi=...) at util_latent_aug.py:203,460.
 * weights[i] = mapping.fc{i}.weight [w_dim][in], biases[i] = mapping.fc{i}.bias (legacy.py:175-176), lr_mul 0.01
 * (legacy.py:141), w_avg = mapping.w_avg (legacy.py:172).  tmp: 2*B*max(z_dim,w_dim) floats.
 * la_fc_f32: FullyConnectedLayer forward y = act(x @ (W*lr_mul/sqrt(in))^T + b*lr_mul) * gain.
 * ------------------------------------------------------------------------------------------------------------- */
int la_fc_f32(const float* x, const float* W, const float* bias, float* y, int B, int in, int out, float lr_mul, int act,
              float alpha, float gain, la_stream_t stream);
int la_mapping_forward_f32(const float* z, int B, int z_dim, int w_dim, int num_layers, const float* const* weights,
                           const float* const* biases, float lr_mul, const float* w_avg, float truncation_psi,
                           int num_ws, float* tmp, float* ws_out, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Discriminator engine: replaces  D(x, c=None)  and its backward to x inside calc_loss_disc (util_latent_aug.py:363-371).
 * Architecture 'resnet' + MinibatchStd epilogue (legacy.py:220-247).  params: device tensors in this order (names of
 * legacy.py:271-288), resolution R first:
 *   bR: fromrgb.weight, fromrgb.bias, conv0.weight, conv0.bias, conv1.weight, conv1.bias, skip.weight
 *   b(R/2) .. b8: conv0.weight, conv0.bias, conv1.weight, conv1.bias, skip.weight
 *   b4: conv.weight, conv.bias, fc.weight, fc.bias, out.weight, out.bias
 * channels[k] = channels at resolution 4 << k (same table as the generator).  mbstd_group_size: 4 in every SG2 config;
 * the batch of a forward must be divisible by min(group, batch) exactly as in the reference.
 * la_disc_loss: loss_out[0] = softplus(-logits).mean() * w_disc and keeps d(loss)/d(logits) for la_disc_backward.
 * la_disc_backward: g_img [B][C][R][R] (accumulate != 0: added to what g_img holds).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct la_disc la_disc;
int la_disc_num_params(int img_resolution);
size_t la_disc_workspace_bytes(int img_resolution, int img_channels, const int* channels, int max_batch);
int la_disc_create(int img_resolution, int img_channels, const int* channels, float conv_clamp, const float* const* params,
                   int nparams, const float* fir_host, int mbstd_group_size, int max_batch, void* workspace,
                   size_t workspace_bytes, la_stream_t stream, la_disc** out);
void la_disc_destroy(la_disc* h);
/* History contract: takes effect at the next la_disc_forward; la_disc_backward runs in the precision of the forward pass it differentiates,
 * so forward(P1), set_precision(P2), backward gives the bits of forward(P1), backward. */
int la_disc_set_precision(la_disc* h, int precision);
int la_disc_forward(la_disc* h, const float* img, int B, la_stream_t stream);
int la_disc_loss(la_disc* h, float w_disc, int norm_batch, float* loss_out, la_stream_t stream);
int la_disc_backward(la_disc* h, const float* dlogits, float* g_img, int accumulate, la_stream_t stream);
const float* la_disc_logits(const la_disc* h);

/* ---------------------------------------------------------------------------------------------------------------
 * Perceptual feature engine: replaces  self.vgg16(x, resize_images=False, return_lpips=True)  and its backward inside
 * calc_loss_lpips_torchscript (util_latent_aug.py:387-409).  The network is described by the caller as a list of ops
 * (VGG16 = 13 x conv3x3+ReLU, 4 x max-pool, 5 taps); a tap emits f * rsqrt(sum_c f^2 + 1e-10) * sqrt(lin[c]) / sqrt(H*W),
 * so squared L2 between two outputs is their LPIPS distance.  params: per op in order -- conv: weight [cout][cin][3][3],
 * bias [cout]; tap: lin [C]; pools: none.  Every conv needs cout % 4 == 0, and cin % 4 == 0 unless it is the first op of
 * the list; a pool needs an even resolution; the list must hold a tap (or end in an FC op, below).  A list that breaks one of these is refused by
 * la_feat_workspace_bytes (0) and la_feat_create (LA_ERR_ARG), before any launch.  la_crop_repeat_f32: the crop + `.repeat([1,3,1,1])` of :394 for every modality
 * (rows ordered modality-major: row = c*B + b) with an affine preprocess; la_crop_repeat_grad_f32: its adjoint, ADDED to
 * g_img.
 * Detector lists: LA_FEAT_FC_RELU / LA_FEAT_FC are fully connected layers, y = act(flatten(x) W^T + b), for the
 * `return_features=True` branch of the same net (metrics/metric_utils.py:264-328).  cin is the flattened C*res*res of what
 * precedes (NCHW order, torch's flatten), cout the number of outputs; params: weight [cout][cin], bias [cout].  A list that
 * ends in an FC op is a detector list: forward only (la_feat_backward refuses it), its feature vector is the last FC's output,
 * it holds no tap (a list with both is refused), and only FC ops may follow the first FC.  Its convolutions run in the engine's
 * precision mode; the FC ops are always exact fp32 (la_fc_bias_act_f32).
 * Pair distance (tap lists only): la_feat_pair_distance runs the trunk once on xy [2P][in_ch][in_res^2] and writes, per tap,
 * the LPIPS distance of rows p and p + P -- dist [P][ntaps] float64, dist[p][t] = mean over pixels of
 * sum_c lin[c] (fx rx - fy ry)^2 with the tap's r = rsqrt(sum_c f^2 + 1e-10) -- without writing a feature vector.  lin enters
 * as it is (no sqrt), so its sign does not matter here.  ws: la_feat_pair_workspace_bytes(h, P) bytes (0: detector list or
 * 2P > max_batch, which la_feat_pair_distance refuses with LA_ERR_ARG before any launch).  No atomics: two runs give the same
 * bits; no host sync, no allocation.  It overwrites the activations of an earlier la_feat_forward (la_feat_backward then refuses
 * until the next forward).  la_feat_num_taps: taps of the list = columns of dist.  la_crop_repeat_affine_f32: la_crop_repeat_f32
 * with one scale / shift per repeated channel (host arrays of `rep` floats), e.g. the (x - mean_k) / std_k of an input layer.
 * General ops (the AlexNet and SqueezeNet 1.1 trunks of augments/criteria/lpips/networks.py:52-84): la_feat_op cannot grow, and the
 * two entries below stay the only ones that take a list, so a general op is its {kind, cin, cout} record FOLLOWED by argument
 * records {LA_FEAT_OP_ARGS, a, b} that carry the rest:
 *       LA_FEAT_CONV_RELU_EX  {k, stride}, {pad, 0}        LA_FEAT_MAXPOOL3S2  {ceil_mode, 0}        LA_FEAT_FIRE  {squeeze, expand1}, {expand3, 0}
 * nops counts records (at most 144, at most 48 ops); a list of the six first kinds is what it was.  The new kinds:
 *   LA_FEAT_CONV_RELU_EX  y = relu(conv(x, w, stride, pad) + b): square kernel k 1 .. 11, stride 1 | 2 | 4, pad 0 .. 5 and < k, output
 *                         size floor((res + 2 pad - k) / stride) + 1; cout % 4 == 0; cin % 4 == 0, or cin == 3 as the first op of the
 *                         list.  params: weight [cout][cin][k][k], bias [cout], used in place.
 *   LA_FEAT_MAXPOOL3S2    3x3 stride-2 max pool without padding, ceil_mode 0 | 1, output size by torch's rule (in ceil mode the last
 *                         window must start inside the input; a window that hangs over the edge is clipped).  The gradient goes to
 *                         the first maximum of a window in row-major scan order, as in torch.  No params.
 *   LA_FEAT_FIRE          SqueezeNet's Fire module as one op, so that the list stays a chain: s = relu(conv1x1(x, squeeze)), then
 *                         y[:, :expand1] = relu(conv1x1(s)) and y[:, expand1:] = relu(conv3x3(s), pad 1), written into the two
 *                         channel slices of one output; cout = expand1 + expand3; cin, squeeze, expand1, expand3 multiples of 4.
 *                         params: six tensors -- squeeze weight [squeeze][cin][1][1], bias, expand1x1 weight [expand1][squeeze][1][1],
 *                         bias, expand3x3 weight [expand3][squeeze][3][3], bias.
 * The resolution is tracked per op and stays square.  A list in which a geometry above is broken, a resolution would fall below 1
 * or a pool would have no window, or whose argument records are missing, is refused by la_feat_workspace_bytes (0) and la_feat_create
 * (LA_ERR_ARG) before any launch, and la_last_error names the index of the op (ops counted, not records).  A detector list holds none
 * of the new conv / fire kinds.  The input of a list with a general op may be one pixel (in_res >= 1; other lists: >= 2).
 * The new ops compute in exact fp32 (fp32 MFMA products) in EVERY precision mode, as the FC ops do; la_feat_set_precision governs the
 * LA_FEAT_CONV_RELU ops of a list only.  Where the K = cin * k * k sum of a small layer is split over workgroups the slices are
 * added in a fixed order: no float atomics, two runs give the same bits; no host sync, no allocation.  Taps, la_feat_forward,
 * la_feat_backward and la_feat_pair_distance work over them unchanged.  Lists of the six first kinds take the workspace bytes and
 * give the bits they did before these kinds existed.
 * ------------------------------------------------------------------------------------------------------------- */
#define LA_FEAT_CONV_RELU 0
#define LA_FEAT_TAP 1
#define LA_FEAT_MAXPOOL2 2
#define LA_FEAT_AVGPOOL2 3
#define LA_FEAT_FC_RELU 4
#define LA_FEAT_FC 5
#define LA_FEAT_CONV_RELU_EX 6
#define LA_FEAT_MAXPOOL3S2 7
#define LA_FEAT_FIRE 8
#define LA_FEAT_OP_ARGS 9
typedef struct la_feat_op { int kind, cin, cout; } la_feat_op;
typedef struct la_feat la_feat;
size_t la_feat_workspace_bytes(int nops, const la_feat_op* ops, int in_ch, int in_res, int max_batch);
int la_feat_create(int nops, const la_feat_op* ops, const float* const* params, int nparams, int in_ch, int in_res,
                   int max_batch, void* workspace, size_t workspace_bytes, la_stream_t stream, la_feat** out);
void la_feat_destroy(la_feat* h);
int la_feat_num_features(const la_feat* h);
/* History contract: takes effect at the next la_feat_forward / la_feat_pair_distance; la_feat_backward runs in the precision of the forward
 * pass it differentiates. */
int la_feat_set_precision(la_feat* h, int precision);
int la_feat_forward(la_feat* h, const float* x, int N, float* feat_out, la_stream_t stream);
int la_feat_backward(la_feat* h, const float* gfeat, float* gx, la_stream_t stream);
int la_feat_num_taps(const la_feat* h);
size_t la_feat_pair_workspace_bytes(const la_feat* h, int P);
int la_feat_pair_distance(la_feat* h, const float* xy, int P, double* dist, void* ws, size_t ws_bytes, la_stream_t stream);
int la_crop_repeat_f32(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, int rep, float scale,
                       float shift, la_stream_t stream);
int la_crop_repeat_affine_f32(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, int rep,
                              const float* scale, const float* shift, la_stream_t stream);
int la_crop_repeat_grad_f32(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, int rep,
                            float scale, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Detector features: the steps of the reference's image -> VGG16 feature path (metrics/metric_utils.py:314-318 and the scripted
 * module's own resize and fully connected layers) that the feature engine does not hold.
 *   la_detector_prep_f32  img [N][C][H][W] -> out [N][rep*C][S][S] in one launch, rep * C == 3 (rep = 3: x.repeat([1,3,1,1]),
 *                         output channel r*C + c).  In this order: quantize != 0: q = floor(clamp(x*127.5 + 128, 0, 255)), the
 *                         bits of torch's (x * 127.5 + 128).clamp(0, 255).to(torch.uint8) (product and sum rounded separately);
 *                         resampling (H, W) -> (S, S), mode LA_DET_AREA: F.interpolate(mode='area') == adaptive_avg_pool2d
 *                         (bins floor(i*H/S) .. ceil((i+1)*H/S); non-integer ratios, up-sampling and H != W allowed), mode
 *                         LA_DET_BILINEAR: align_corners=False, no antialiasing; H == S && W == S is a copy; then the
 *                         per-channel affine v * scale[k] + shift[k], k < 3 (scale / shift: host arrays of 3).
 *   la_fc_bias_act_f32    y [N][O] = act(x [N][K] . W [O][K]^T + b [O]), act LA_ACT_LINEAR | LA_ACT_RELU, float32 with exact
 *                         fp32 products (fp32 MFMA).  A weight stream: every batch of up to 64 rows reads each weight element
 *                         from memory once.  K is split over workgroups; the partial sums are added in a fixed order (no float
 *                         atomics), so two runs give the same bits.  workspace: la_fc_workspace_bytes(N, K, O) bytes, which also
 *                         serve every smaller N; 0 means the shape was refused.  Bad arguments: LA_ERR_ARG, a workspace that is
 *                         too small: LA_ERR_WORKSPACE, both before any launch.
 * ------------------------------------------------------------------------------------------------------------- */
#define LA_DET_AREA 0
#define LA_DET_BILINEAR 1
int la_detector_prep_f32(const float* img, float* out, int N, int C, int H, int W, int S, int rep, int mode, int quantize,
                         const float* scale, const float* shift, la_stream_t stream);
size_t la_fc_workspace_bytes(long N, long K, long O);
int la_fc_bias_act_f32(const float* x, const float* w, const float* b, float* y, long N, long K, long O, int act,
                       void* workspace, size_t workspace_bytes, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The loop: replaces LatentAug.forward(w, fname) (augments/utils/util_latent_aug.py:207-310) for 3-D w input.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct la_opt_config {
    int steps;              /* opt_num_epochs (latent_aug.py:81) */
    float lr;               /* opt_lr (latent_aug.py:82) */
    float beta1, beta2, eps; /* Adam (0.9, 0.999, 1e-8) (util_latent_aug.py:213) */
    float w_latent, w_pix, w_disc, w_lpips; /* latent_aug.py:88-91 */
    int criterion_mode;     /* 0 | 1, kept for ABI stability: both use bank column sums reduced once per handle for the gradient;
                               loss scalars (only when losses_out is given) always use the reference's GEMM form over the banks */
    int soft_aug;           /* latent_aug.py:94 */
    float alpha;            /* latent_aug.py:95 */
    int loop_noise_mode;    /* 1 = 'const' (util_latent_aug.py:227) */
    int final_noise_mode;   /* 0 none / 1 const / 2 explicit tensors; util_latent_aug.py:488 uses the generator default ('random'):
                               pass 2 + tensors */
    int norm_batch;         /* n of the criteria's 1/(m*n); 0 = local batch (what a DataParallel replica sees) */
    int crop, crop_off;     /* util_dataset.py:317-323: int(sqrt(R*R/2)), round((R-crop)/2) */
} la_opt_config;
typedef struct la_latent_opt la_latent_opt;
size_t la_latent_opt_workspace_bytes(int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg, long Mw,
                                     long Mx, int max_batch);
/* bankW [Mw][num_ws][w_dim] (register_buffer 'W', :148); bankXc [C][Mx][crop*crop] = centre-cropped 'X' (:158, :253),
 * modality-major. */
int la_latent_opt_create(la_synth* g, int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                         const float* bankW, long Mw, const float* bankXc, long Mx, int max_batch, void* workspace,
                         size_t workspace_bytes, la_latent_opt** out);
/* The latent space the loop optimises in.  latent_space 0 = W: one w_dim row per sample, broadcast to every style slot (the reference's
 * broadcasting(), util_latent_aug.py:493-494); the two entries above are these with 0.  1 = W+: one row per sample AND slot, w_opt
 * [B][num_ws][w_dim] -- the reference's LatentAug.forward (:207-310) with broadcasting() the identity, hard_aug(w, w_tilde) = w_tilde,
 * smooth_aug(w, w_tilde) = alpha * w_tilde + (1 - alpha) * w row by row; Adam, the criteria and the loss signs unchanged.  For a W+
 * handle la_latent_opt_run's w0 is [B][num_ws][w_dim] (16-byte aligned), and the buffers of la_latent_opt_set_trace (w_trace) and
 * la_latent_opt_set_grad_trace (dw_trace) are [steps][B][num_ws][w_dim].  W+ needs w_dim % 4 == 0.  Any other latent_space is
 * LA_ERR_ARG (create_ex: before anything is allocated or launched; workspace_bytes_ex: 0 bytes). */
size_t la_latent_opt_workspace_bytes_ex(int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg, long Mw,
                                        long Mx, int max_batch, int latent_space);
int la_latent_opt_create_ex(la_synth* g, int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                            const float* bankW, long Mw, const float* bankXc, long Mx, int max_batch, int latent_space,
                            void* workspace, size_t workspace_bytes, la_latent_opt** out);
void la_latent_opt_destroy(la_latent_opt* h);
/* attach the discriminator used when cfg.w_disc != 0 (must outlive the loop handle) */
int la_latent_opt_set_disc(la_latent_opt* h, la_disc* d);
/* attach the LPIPS criterion used when cfg.w_lpips != 0: feature engine, real-feature banks [C][Mf][F] (register_buffer
 * 'fea_<mode>', util_latent_aug.py:171; modality-major), crop size S (crop_size_aug), input preprocess x*scale+shift.
 * la_latent_opt_set_crop_pos: absolute (x, y) of the S x S window, drawn by the host once per forward
 * (util_dataset.py:284-296 + the centre-crop offset).  A ws_bytes below la_latent_opt_lpips_workspace_bytes is LA_ERR_WORKSPACE. */
size_t la_latent_opt_lpips_workspace_bytes(int img_channels, int F, int S, long Mf, int max_batch);
int la_latent_opt_set_lpips(la_latent_opt* h, la_feat* f, const float* bankF, long Mf, int S, float pre_scale,
                            float pre_shift, void* ws, size_t ws_bytes);
/* Per-channel input affine of the feature net, x_k * scale[k] + shift[k] for the n (<= 3) repeated channels of :394 -- the
 * (x - mean_k) / std_k input layer inside NVIDIA's TorchScript vgg16.pt (util_latent_aug.py:35-43).  Overrides the scalar pair. */
int la_latent_opt_set_lpips_preproc(la_latent_opt* h, const float* scale, const float* shift, int n);
int la_latent_opt_set_crop_pos(la_latent_opt* h, int x, int y);
/* Launch mode of the step loop (util_latent_aug.py:219-276).  1 (default): one optimisation step is captured as a hipGraph
 * after its first eager execution and replayed for every further step and batch of the same size -- the loop is ~230 short
 * launches per step and otherwise host-launch-bound at small batches.  0: every launch eager.  Results are identical. */
int la_latent_opt_set_graph(la_latent_opt* h, int enable);
/* 1: a captured step is being replayed; 0: eager launches (as asked / nothing run yet); -1: eager because the runtime refused the
   capture of the step.  (No reference counterpart: the reference loop is eager PyTorch, util_latent_aug.py:240-300.) */
int la_latent_opt_graph_state(const la_latent_opt* h);
/* Per-step snapshots for the reference's verbose_log (util_latent_aug.py:292-295 snap_w / snap_img): device buffers (or NULL)
 * w_trace [steps][B][w_dim] = the optimised latent after every step, img_trace [steps][B][C][R][R] = the image synthesised in
 * every step (W+ handle: w_trace [steps][B][num_ws][w_dim]).  While either is set the loop launches eagerly. */
int la_latent_opt_set_trace(la_latent_opt* h, float* w_trace, float* img_trace);
/* dw_trace [steps][B][w_dim] (device, or NULL) = dL/dw of every step, L = -latent - pix - lpips + disc (util_latent_aug.py:270):
 * the tensor `loss.backward()` leaves in w_opt.grad (:275) before Adam consumes it (W+ handle: [steps][B][num_ws][w_dim]).  While set
 * the loop launches eagerly. */
int la_latent_opt_set_grad_trace(la_latent_opt* h, float* dw_trace);
/* How a step places its discriminator branch and its perceptual branch (crop + feature net forward / backward) when both criteria are
 * active; `enable` is a mode, values outside 0 .. 2 are clamped.
 *   0: one after the other on the launch stream.
 *   1: split replay -- the step is captured as four graphs and the perceptual one is replayed on a stream of the handle's own beside
 *      the discriminator's on the launch stream.  The branches overlap only while the step is replayed: launched steps (the first of a
 *      batch size, a run with loss scalars or traces, graph mode off) run them one after the other.
 *   2 (the handle's default): fork / join inside the step -- the perceptual branch on the handle's own stream, forked after the synthesis
 *      forward and joined before its crop gradient is added to the image gradient; launched that way, and captured as two parallel
 *      branches of one graph.  A run that asks for loss scalars keeps both branches on the launch stream.
 * Bit-identical results in every mode (same launches, same accumulation order).  Drops the captured graphs. */
int la_latent_opt_set_overlap(la_latent_opt* h, int enable);
/* Image rows [row_lo, row_hi) that the loop's image criteria read (0, 0 = not known, the default).  The reference synthesises a whole
 * frame in every epoch and hands the pixel criterion its centre crop and the perceptual criterion a window inside it
 * (util_latent_aug.py:216, :246-262; util_dataset.py:284-323): no output of the loop depends on the other rows.  With a window given, the
 * synthesis passes of the loop steps compute only what those rows depend on (la_synth_set_row_window); the final synthesis of the
 * augmented latent (:303) is a whole frame.  Ignored while the discriminator (whole frame, :233-242) is active or per-step images are
 * traced.  Drops a captured step when the window changes. */
int la_latent_opt_set_row_window(la_latent_opt* h, int row_lo, int row_hi);
/* ... and the image columns [col_lo, col_hi) they read (the centre crop is a square: util_dataset.py:317-323); 0, 0 = all.  Used with the row window. */
int la_latent_opt_set_col_window(la_latent_opt* h, int col_lo, int col_hi);
/* verbose_log timers of the reference's first batch (time_latent / time_disc / time_pix / time_lpips / time_epoch,
 * util_latent_aug.py:221-272): with the time trace on, a run that asks for the loss scalars brackets the criteria of every step with
 * HIP events on the launch stream; la_latent_opt_get_times (after the stream has drained, or blocking) fills ms [steps][5] =
 * {latent, disc, pix, lpips, epoch} in milliseconds.  A criterion's bracket holds its loss scalar and its gradient launches. */
int la_latent_opt_set_time_trace(la_latent_opt* h, int enable);
int la_latent_opt_get_times(la_latent_opt* h, float* ms);
/* The banks handed to la_latent_opt_create / _set_lpips (register_buffer('W'/'X'/'fea_*'), util_latent_aug.py:137-171) must stay
 * IMMUTABLE for the life of the handle: their column sums are reduced once (both criterion modes) and every later gradient uses
 * them.  A caller that does rewrite bank contents in place calls this before the next la_latent_opt_run: all three sets of column sums (W,
 * the pixel crops, the perceptual features) are reduced again by that run, and the handle then equals, bit for bit, one created on the new
 * banks (History contract; a captured step reads the sums from the same buffers and stays valid). */
int la_latent_opt_invalidate_banks(la_latent_opt* h);
/* w0 [B][w_dim] (W+ handle: [B][num_ws][w_dim]) -> img_out [B][C][R][R], w_aug_out [B][num_ws][w_dim]; losses_out (may be NULL) [steps][4] =
 * weighted {latent, pix, disc, lpips} per step. */
int la_latent_opt_run(la_latent_opt* h, const float* w0, int B, const float* const* final_noises, float* img_out,
                      float* w_aug_out, float* losses_out, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Quality metrics on the augmented outputs: the numeric core of the reference's FID and Improved
 * Precision/Recall downstream of the detector features (the detectors are NVIDIA-hosted pickles, metric_utils.py:46-60).
 *   la_feature_moments_f64  FeatureStats.append, metrics/metric_utils.py:104-118: raw_mean[D] += sum_k x[k];
 *                           raw_cov[D][D] += x^T x with float64 accumulators; x float32 [n][D].
 *   la_cdist_f16            compute_distances, metrics/precision_recall.py:19-32 (torch.cdist of float16 features):
 *                           dist float32 [nr][nc].  rows/cols: float16 [n][D] row-major, D % 16 == 0, 16-byte aligned.
 *   la_pr_kth_f16           precision_recall.py:75-79: kth[i] = (nhood_size+1)-th smallest distance of row i.
 *   la_pr_member_f16        precision_recall.py:80-84: member[i] = any_j dist(i, j) <= radius[j].
 *   la_kid_poly3_f32        Kernel Inception Distance of two feature sets (described at its prototype below).
 *   la_dc_count_f16         density and coverage of two feature sets (described at its prototype below).
 *   la_fd_*                 Frechet distance of two feature sets from their cross-Gram matrix (described at the prototypes below).
 *   la_knn_f32, la_realism_f32   nearest bank rows and realism score of single samples (described at the prototypes below).
 * ws: la_pr_workspace_floats(nr, nc) floats.  The [nr][nc] matrix is not materialised by the last two.
 * ------------------------------------------------------------------------------------------------------------- */
int la_feature_moments_f64(const float* x, long n, int D, double* raw_mean, double* raw_cov, la_stream_t stream);
size_t la_pr_workspace_floats(long nr, long nc);
int la_cdist_f16(const void* rows, long nr, const void* cols, long nc, int D, float* dist, float* ws, la_stream_t stream);
int la_pr_kth_f16(const void* rows, long nr, const void* cols, long nc, int D, int nhood_size, float* kth, float* ws,
                  la_stream_t stream);
int la_pr_member_f16(const void* rows, long nr, const void* cols, long nc, int D, const float* radius, unsigned char* member,
                     float* ws, la_stream_t stream);

/* Kernel Inception Distance (no reference counterpart; the community's kid50k_full recipe): the unbiased MMD^2 estimator with the
 * cubic polynomial kernel k(a, b) = (a.b / D + 1)^3 over detector features, averaged over S subsets.  For subset s, with
 * x_i = x[ix[s][i]] (i < mx, the generated side) and y_j = y[iy[s][j]] (j < my, the real side):
 *   sums[s] = { sum_{i != j} k(x_i, x_j),  sum_{i != j} k(y_i, y_j),  sum_{i, j} k(x_i, y_j) }
 *   mmd2[s] = sums[s][0] / (mx (mx - 1)) + sums[s][1] / (my (my - 1)) - 2 sums[s][2] / (mx my);    kid[0] = mean_s mmd2[s]
 * x float32 [nx][D], y float32 [ny][D], row-major, any D >= 1 (no padding; float4 loads when D % 4 == 0 and both are 16-byte
 * aligned).  ix int32 [S][mx], iy int32 [S][my]: row numbers, gathered while loading (no gathered copy is made); the caller
 * draws them, and a value outside [0, n) is clamped into it rather than read out of bounds.  mx, my >= 2; they differ only for the
 * full-set estimator (S = 1, ix = 0..nx-1, iy = 0..ny-1).  sums float64 [S][3], mmd2 float64 [S], kid float64 [1]: device memory.
 * Dot products on the exact fp32 MFMA, in fp32 chains of 128 terms added in fp32; (dot / D + 1)^3 in fp32 per element; every sum
 * of kernel values in float64.  The kernel matrices are never written out: ws holds one float64 partial per 128 x 128 tile and
 * subset, la_kid_workspace_bytes(S, mx, my) bytes (8-byte aligned; 0 for sizes the launch refuses), about 109 KB at S = 100,
 * mx = my = 1000.  A smaller ws_bytes is LA_ERR_WORKSPACE, checked with the other arguments before anything is launched.
 * Deterministic: partials are added in index order by a second launch, no atomics; two runs give the same bits. */
size_t la_kid_workspace_bytes(long S, long mx, long my);
int la_kid_poly3_f32(const float* x, long nx, const float* y, long ny, int D, const int* ix, const int* iy, long S, long mx, long my,
                     double* sums, double* mmd2, double* kid, void* ws, size_t ws_bytes, la_stream_t stream);

/* Density and coverage (no reference counterpart; Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models",
 * ICML 2020, the `prdc` package).  Both use the balls of the REAL samples only.  With real features X [nr][D], generated features
 * Y [ng][D] (float16, row-major, D % 16 == 0, D >= 16, 16-byte aligned, as the entries above), k = nhood_size,
 * dist(a, b) = sqrt(max(|a|^2 + |b|^2 - 2 a.b, 1e-30)) with fp32 accumulation (the torch.cdist form of the entries above) and
 * radius[i] = the (k+1)-th smallest distance from real i to all reals, its own zero included -- la_pr_kth_f16(real, real), kept in
 * float32 (not rounded to float16: no reference keeps these radii in float16):
 *   count[j]   = #{ i : dist(Y_j, X_i) <= radius[i] }      int32 [ng];     density  = sum_j count[j] / (k ng)
 *   nearest[i] = min_j dist(Y_j, X_i)                       float32 [nr];   coverage = mean_i (nearest[i] <= radius[i])
 * The comparison is <=, as the library's precision (precision_recall.py:83); prdc uses <.  They differ at exact ties only.
 * la_dc_count_f16 makes one tiled pass over the ng x nr pairs (exact float16 products on v_mfma_f32_32x32x16_f16) for both outputs;
 * the distance matrix is never written.  The grid is blocks of 128 generated rows x la_dc_col_splits(ng, nr) chunks of real
 * columns (a host rule that brings the launch to about 512 workgroups; 0 for sizes the launch refuses).  Row counts stay in
 * registers over a chunk; column minima are reduced in the wave and the workgroup first.  Chunks and row blocks are combined with
 * integer atomics only (atomicAdd on count, atomicMin on the bit pattern of the positive distances): order-independent, two runs give
 * the same bits.  count and nearest are initialised by a kernel on `stream` inside the entry, which can be captured in a graph.
 * ws: la_dc_workspace_bytes(ng, nr) bytes (the squared norms of both sides; 0 for sizes the launch refuses).  A smaller ws_bytes
 * is LA_ERR_WORKSPACE, checked with the other arguments before anything is launched. */
size_t la_dc_workspace_bytes(long ng, long nr);
int la_dc_col_splits(long ng, long nr);
int la_dc_count_f16(const void* gen, long ng, const void* real, long nr, int D, const float* radius, int* count, float* nearest,
                    void* ws, size_t ws_bytes, la_stream_t stream);

/* Frechet distance of two feature sets (metrics/frechet_inception_distance.py:41-45) without a covariance matrix or a matrix square
 * root.  x float32 [nx][D] (generated), y float32 [ny][D] (real), row-major, any D >= 1, 4-byte aligned.  With A, B the two sets minus
 * their column means and the reference's 1/N covariance (metric_utils.py:136-140):
 *   FD = |mu_x - mu_y|^2 + |A|_F^2 / nx + |B|_F^2 / ny - 2 nuc(A B^T) / sqrt(nx ny),   nuc = the sum of the singular values
 * (the non-zero eigenvalues of Sigma_x Sigma_y are the squared singular values of A B^T / sqrt(nx ny)).  It is meant for the
 * few-samples regime, n = min(nx, ny) <= 8192; nx, ny >= 2.  m = max(nx, ny), n' = n rounded up to even.
 *   la_fd_gram_f32          column means in float64 (fixed order); C = A B^T in float64 on v_mfma_f64_16x16x4_f64, the float32 operands
 *                           centred in float64 while they are loaded (no centred copy exists); C is stored at the START of ws as n
 *                           vectors of m contiguous doubles (C for nx <= ny, C^T otherwise, same bits; no transposing pass), one
 *                           zero vector appended when n is odd.  terms float64 [4] (device): |mu_x - mu_y|^2, |A|_F^2, |B|_F^2, and a
 *                           slot for nuc(C) that la_fd_finish_f64 fills.
 *   la_fd_jacobi_sweep_f64  one sweep of one-sided Jacobi (Hestenes) over v = n' vectors of m doubles (an odd n: the caller's zero
 *                           vector last), in place: n' - 1 rounds of n'/2 disjoint pairs, la_fd_round_pair's order, one launch per
 *                           round and one workgroup per pair.  With alpha = |c_p|^2, beta = |c_q|^2, gamma = c_p . c_q the pair is
 *                           rotated when alpha beta > 0 and |gamma| > sqrt(m) 2^-52 sqrt(alpha beta) (LAPACK dgesvj's criterion):
 *                           zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (1 at zeta = 0),
 *                           c = 1 / sqrt(1 + t^2), s = c t, c_p' = c c_p - s c_q, c_q' = s c_p + c c_q.  rotations int32 [1]
 *                           (device): zeroed by the entry on `stream`, then the number of rotations of the sweep (integer atomic
 *                           adds).  The caller repeats the entry until a sweep leaves 0 there.  Up to m = 8192 a pair is held in
 *                           registers: read once per round, written at most once.
 *   la_fd_finish_f64        sv float64 [n] (device, may be NULL): the norms of the vectors at the start of ws, in vector order -- the
 *                           singular values once the sweeps have converged; terms[3] = their sum in index order.
 *   la_fd_round_pair        pure host: pair k (0 .. n'/2 - 1) of round `round` (0 .. n' - 2) of the circle method for n vectors, *p < *q
 *                           (index n of an odd n is the zero vector); the kernels use the same arithmetic.  LA_ERR_ARG outside
 *                           those ranges or n outside 2 .. 8192.
 * ws: la_fd_workspace_bytes(nx, ny, D) bytes, 8-byte aligned (the n' x m doubles, the means, the reduction partials; 0 for sizes the
 * entries refuse).  nx < 2, ny < 2, min(nx, ny) > 8192 and null pointers are LA_ERR_ARG, a smaller ws_bytes is LA_ERR_WORKSPACE, all
 * before anything is launched.  Every float64 sum has a fixed order and there are no float atomics: two runs give the same bits. */
size_t la_fd_workspace_bytes(long nx, long ny, int D);
int la_fd_round_pair(int n, int round, int k, int* p, int* q);
int la_fd_gram_f32(const float* x, long nx, const float* y, long ny, int D, double* terms, void* ws, size_t ws_bytes, la_stream_t stream);
int la_fd_jacobi_sweep_f64(double* v, long n, long m, int* rotations, la_stream_t stream);
int la_fd_finish_f64(void* ws, size_t ws_bytes, long nx, long ny, int D, double* sv, double* terms, la_stream_t stream);

/* Per-sample neighbour queries (no reference counterpart as entries): the k nearest bank rows of every query row, and the realism
 * score of the Improved Precision / Recall paper (Kynkaanniemi et al. 2019, whose pr50k3 is metrics/precision_recall.py).  Where the
 * entries above keep the reference's float16 distances, these two are float64 arithmetic on the float32 features: float16 in
 * |a|^2 + |b|^2 - 2 a.b form has no digits left at the small distances of a near-copy.
 * q float32 [nq][D] (queries), x float32 [nx][D] (the bank), row-major, any D >= 1, 4-byte aligned.  One definition of the squared
 * distance of a pair for both entries:
 *   d2(q, x) = max(0, (|q|^2 + |x|^2) - 2 q.x)
 * all three sums in float64 over the inputs widened exactly (a product of two float32 values is exact in float64), the dot products
 * on v_mfma_f64_16x16x4_f64 in the tile form of la_fd_gram_f32 without centring, the norms of both sides by one kernel as the
 * diagonal of the same product (the same k order).  The bits of d2(q, x) depend on the two rows and D only: not on the tile, the
 * column split, the row of the batch or the number of other rows.  Equal rows have equal norms and d2 of two equal rows is exactly
 * 0: a copy of a bank row is found at distance 0.  For any summation order |d2 - d2_exact| <= (2 D + 4) 2^-53 (|q|^2 + |x|^2): three sums of D exact
 * products each, then two roundings to combine them.
 *   la_knn_f32      dist2 float64 [nq][k] ascending, idx int32 [nq][k] (device), 1 <= k <= 32.  The order is (d2, index): of two equal
 *                   d2 the lower index comes first, so the result does not depend on any merge order.  exclude_self != 0 needs
 *                   nq == nx and skips bank row i for query i (the queries are the bank).  Slots beyond the number of candidates
 *                   hold idx = -1 and dist2 = +inf.  A d2 that is not finite (inf or NaN in a row) is never listed.
 *   la_realism_f32  radius2 float64 [nx] (device): the squared radius of the sphere around bank row i; a negative value drops the
 *                   sphere.  score2[j] = max over the kept i of radius2[i] / d2(q_j, x_i), the quotient in float64; d2 == 0 on a kept
 *                   sphere gives +inf; arg int32 [nq] is the maximising i, ties to the lower i.  No kept sphere: score2 = 0, arg = -1.
 *                   The same tile loop as la_knn_f32 with another selection key, k = 1.
 * The grid is blocks of 64 query rows x la_knn_col_splits(nq, nx) chunks of bank columns (a host rule that brings the launch to
 * 512 workgroups or somewhat more, at most 64 chunks; 0 for sizes the launch refuses), so a batch of 8 queries against a bank of thousands
 * still fills the chip.  A workgroup walks its chunk tile by tile and keeps the sorted k-list of each of its rows in LDS; a finish
 * launch ranks the candidates of the chunks.  No atomics, no host synchronisation, nothing allocated: the entries can be captured in
 * a graph and two runs give the same bits.
 * scratch: la_knn_scratch_bytes(nq, nx, D, k) bytes, 8-byte aligned, any contents (the float64 norms of both sides and the chunks'
 * lists; non-decreasing in every argument; 0 for sizes the entries refuse); la_realism_f32 needs the size for k = 1.
 * k outside 1 .. 32, nq or nx < 1, D < 1, null pointers and exclude_self with nq != nx are LA_ERR_ARG, a smaller scratch_bytes is
 * LA_ERR_WORKSPACE, all before anything is launched. */
int la_knn_col_splits(long nq, long nx);
size_t la_knn_scratch_bytes(long nq, long nx, int D, int k);
int la_knn_f32(const float* q, long nq, const float* x, long nx, int D, int k, int exclude_self, double* dist2, int* idx, void* scratch,
               size_t scratch_bytes, la_stream_t stream);
int la_realism_f32(const float* q, long nq, const float* x, long nx, int D, const double* radius2, double* score2, int* arg,
                   void* scratch, size_t scratch_bytes, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * UMAP embedding (McInnes, Healy, Melville 2018; the reference's analysis/umap_analysis.py calls the umap-learn library): the stages
 * after the neighbour search, all float64, no float atomics, no host synchronisation, nothing allocated, capturable in a graph; two
 * runs give the same bits.  Four deliberate differences from umap-learn: (1) an epoch is synchronous -- all forces come from the
 * positions at the start of the epoch; (2) the randomness is the library's Philox stream (counter convention: csrc/la_rng.h);
 * (3) the initial layout is random or the caller's, never spectral; (4) the sigma bisection always runs its 64 iterations.
 * Empty neighbour slots (idx = -1, dist2 = +inf, as la_knn_f32 leaves them) are skipped everywhere.
 *
 *   la_umap_smooth_knn_f64   dist2 float64 / idx int32 [n][k] as la_knn_f32 wrote them, 1 <= k <= 32; target = log2(n_neighbors).  Per
 *       row, d_s = sqrt(dist2_s); rho = the smallest non-zero d_s (0: none); sigma = the root of sum_s exp(-max(0, d_s - rho) / sigma)
 *       = target by bisection from lo = 0, hi = inf, mid = 1 (mid doubles while hi is infinite, else the bracket's midpoint), 64
 *       iterations without an early exit; then sigma = max(sigma, 1e-3 * mean of the row's finite d_s); w_s = exp(-max(0, d_s - rho)
 *       / sigma), 0 in an empty slot.  Out: rho [n], sigma [n], w [n][k].  One wave per row, the sum by the wave butterfly.
 *   la_umap_graph_f64        the fuzzy union S = A + A^T - A o A^T of the directed weights A[i][idx[i][s]] = w[i][s] as a symmetric
 *       CSR: row_ptr int32 [n + 1], col int32 ascending within a row, val float64, both of capacity cap >= 2 n k (entries past
 *       row_ptr[n] are not written); wmax float64 [1] = max(val).  The columns of a row of idx must be distinct (la_knn_f32's are);
 *       an index outside 0 .. n - 1 counts as an empty slot.  In-degrees by integer atomics, a scan, a fill through integer cursors,
 *       a rank sort of every row by column: the arrays do not depend on the arrival order.  A row is not bounded by 2 k.
 *       scratch: la_umap_scratch_bytes(n, k) bytes, 8-byte aligned, any contents (non-decreasing; 0 for refused sizes).
 *   la_umap_init_f64         y [n][C] = 10 * (the noise stream's exact unit uniform of one Philox word) per coordinate of global
 *       row row0 + i under `seed`: every value is exact.
 *   la_umap_transform_init_f64   new rows against a fitted bank: y [n][C] = the w-weighted mean of bank_y [n_bank][C] over the row's
 *       neighbours (idx, w [n][k]; 0 without a neighbour), and the rows' CSR for the epochs: row_ptr[i] = i k (col = idx and val = w
 *       are the arrays themselves), wmax = 1 -- the nearest neighbour of every row has weight exactly 1, whatever the batch.
 *   la_umap_epoch_f64        epoch e of E, alpha = lr (1 - e / E), one wave per head row i.  Entry t of the row (column j, value v,
 *       skipped if j is outside 0 .. n_tail - 1) is active iff floor((e + 1) p) > floor(e p), p = v / wmax.  An active entry pulls i
 *       towards tail j with coefficient -2 a b d2^(b-1) / (1 + a d2^b) (0 at d2 = 0), d2 = |y_i - y_j|^2, and draws `rate` (0 .. 32)
 *       tail rows r = (word n_tail) >> 32, each pushing i with 2 b / ((0.001 + q2) (1 + a q2^b)) (0 at q2 = 0, or at r == i when
 *       skip_self != 0).  Every component of coefficient (y_i - y_other) is clipped to [-4, 4]; y_out[i] = y_i + alpha (sum of the
 *       clipped terms), the lanes' sums combined by the wave butterfly; a row without an active entry is copied bit for bit.  Only
 *       the head moves.  y_in [n][C], y_out [n][C] (not y_in), y_tail [n_tail][C] (a fit: y_in itself), 1 <= C <= 8; col / val hold
 *       cap entries and row_ptr is clamped to that.  row0: the global index of head row 0 (the Philox counter's; row0 + n < 2^32).
 *   la_umap_layout_f64       epochs e0 .. e1 - 1 of that launch over the two buffers ya, yb: epoch e0 reads ya.  y_tail NULL: a fit
 *       (the tails are the buffer being read).  *which (host int) = 0 if ya holds the result, 1 if yb.
 * Null pointers, n < 1 (graph and fit: n < 2), k outside 1 .. 32, C outside 1 .. 8, e outside 0 .. E - 1, E > 2^28, a, b <= 0 or
 * not finite, rate outside 0 .. 32, misaligned arrays, cap < what is needed are LA_ERR_ARG, a smaller scratch_bytes is
 * LA_ERR_WORKSPACE, all before anything is launched.
 * ------------------------------------------------------------------------------------------------------------- */
size_t la_umap_scratch_bytes(long n, int k);
int la_umap_smooth_knn_f64(const double* dist2, const int* idx, long n, int k, double target, double* rho, double* sigma, double* w,
                           la_stream_t stream);
int la_umap_graph_f64(const int* idx, const double* w, long n, int k, int* row_ptr, int* col, double* val, long cap, double* wmax,
                      void* scratch, size_t scratch_bytes, la_stream_t stream);
int la_umap_init_f64(double* y, long n, int C, unsigned long long seed, long row0, la_stream_t stream);
int la_umap_transform_init_f64(const int* idx, const double* w, long n, int k, const double* bank_y, long n_bank, int C, double* y,
                               int* row_ptr, double* wmax, la_stream_t stream);
int la_umap_epoch_f64(const double* y_in, double* y_out, long n, const double* y_tail, long n_tail, int C, const int* row_ptr,
                      const int* col, const double* val, long cap, const double* wmax, int e, int E, double a, double b, int rate,
                      double lr, unsigned long long seed, long row0, int skip_self, la_stream_t stream);
int la_umap_layout_f64(double* ya, double* yb, long n, const double* y_tail, long n_tail, int C, const int* row_ptr, const int* col,
                       const double* val, long cap, const double* wmax, int e0, int e1, int E, double a, double b, int rate, double lr,
                       unsigned long long seed, long row0, int skip_self, int* which, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Segmented key sort: `ncols` independent columns of float32 keys, ascending, in place.  Column c is keys[c ld .. c ld + M), ld >= M;
 * elements [M, ld) of a column's stride are neither read nor written.  The order is that of the bit pattern under the sign-flip map
 * to unsigned (sign set: all bits flipped, else the sign bit flipped): -inf < .. < -0.0 < +0.0 < .. < +inf.  Keys must not be NaN
 * (not checked; a NaN is placed by its bit pattern, and the pattern 0x7FFFFFFF may change places with the padding).  Keys only, no
 * payload: the sorted column is a unique bit pattern whatever the algorithm, and two runs agree by construction.
 * One 256-thread workgroup sorts a tile of la_sort_tile_keys() keys in LDS with a bitonic network, then ceil(log2(tiles)) merge passes
 * alternate between `keys` and the scratch: a workgroup produces one tile of output, its segment found by a merge-path search, staged
 * in LDS and merged serially by each thread; grid (tiles, columns).  The first launch starts on the side that makes the last pass end
 * in `keys`.  No atomics, no host synchronisation, nothing allocated.
 * scratch: la_sort_columns_scratch_bytes(ncols, M) bytes, 4-byte aligned, any contents (non-decreasing; 0 for refused sizes).
 * ncols outside 1 .. 65535, M outside 1 .. 2^30, ld < M and null pointers are LA_ERR_ARG, a smaller scratch_bytes is LA_ERR_WORKSPACE,
 * all before anything is launched.
 * ------------------------------------------------------------------------------------------------------------- */
int la_sort_tile_keys(void);
size_t la_sort_columns_scratch_bytes(long ncols, long M);
int la_sort_columns_f32(float* keys, long ncols, long M, long ld, void* scratch, size_t scratch_bytes, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance on a Laplacian pyramid (Karras, Aila, Laine, Lehtinen, ICLR 2018, section 5; the slicing: Rabin, Peyre,
 * Delon, Bernot 2011).  No reference counterpart and no network: the stages below, each an entry, restated here as their definition.
 * No float atomics, no host synchronisation, nothing allocated; every float64 sum has a fixed order: two runs give the same bits.
 *
 *   la_lap_pyr_down_f32      y [planes][H/2][W/2] = every second row and column (from 0) of x [planes][H][W] under the 5 x 5 binomial
 *       filter outer([1,4,6,4,1], [1,4,6,4,1]) / 256; borders mirrored without repeating the edge (d c b | a b c d | c b a).
 *   la_lap_pyr_up_sub_f32    fine [planes][H][W] -= up(coarse [planes][H/2][W/2]) in place: up = the same filter times 4 on the
 *       zero-stuffed 2x image (samples at even positions), mirrored the same way on the zero-stuffed image.  Polyphase: an even
 *       position takes [1,6,1] / 8 of its even neighbours, an odd one [4,4] / 8; the zeros are never multiplied.
 *       Both: H and W even, 2 .. 32768.  A pyramid is G_0 = x, G_{l+1} = down(G_l), L_l = G_l - up(G_{l+1}), the last level G itself.
 *   la_swd_gather_f32        rows [0, n per_image) of desc [.][D], D = C nhood^2: patch j of GLOBAL image img0 + i is the nhood x nhood
 *       window of all C channels of img [n][C][H][W] in (channel, y, x) order with corner x0 = (word 0 * (W - nhood + 1)) >> 32,
 *       y0 = (word 1 * (H - nhood + 1)) >> 32, the words those of the library's Philox stream with counter (j, img0 + i,
 *       LA_RNG_STREAM_SWD_POS, level) and key seed (csrc/la_rng.h): integers only, and a set gives the same rows in any batches.
 *   la_swd_channel_stats_f64 mean, std float64 [C] of desc [M][C P] per channel (columns [c P, (c + 1) P) of every row, M P values):
 *       two passes, the mean first, then sum (x - mean)^2 / (M P) and its root (ddof 0); float64 sums over at most 1024 contiguous
 *       runs, added in order.  scratch: la_swd_stats_scratch_bytes(M, C, P) bytes, 8-byte aligned, any contents.
 *   la_swd_normalize_f32     desc = (desc - mean[c]) / std[c] in float64, one rounding to float32.  std[c] == 0 (a constant channel has
 *       no descriptor; callers refuse it) is not divided by: the channel becomes NaN.
 *   la_swd_directions_f32    dirs [ndirs][D]: row j is GLOBAL direction dir0 + j: the unit normals of the noise entries' map for row
 *       dir0 + j of stream LA_RNG_STREAM_SWD_DIR under `seed`, divided by their norm -- sum of squares and quotient in float64, one
 *       rounding.  Directions can be made in chunks.
 *   la_swd_f32               w1 float64 [ndirs]: w1[j] = mean over i of |sort(A d_j)_i - sort(B d_j)_i| for descA, descB [M][D] and
 *       dirs [ndirs][D] (an argument: any vectors will do).  Projections: exact-fp32 MFMA products, each one k-ordered chain,
 *       written as [direction][M] columns; both sets' columns sorted by la_sort_columns_f32; per column sum |a - b| in float64 in a
 *       fixed order, divided once by M.  Directions go through in chunks that fit the scratch; a column's bits do not depend on its
 *       chunk, so any scratch_bytes >= la_swd_scratch_bytes(M, D, ndirs) (chunks of 32 directions; every further 16 M bytes let one
 *       more direction join a chunk) gives the same bits.  scratch 8-byte aligned, any contents.
 * Null pointers, odd or out-of-range H / W, nhood > min(H, W), M, n, ndirs or per_image < 1, C outside 1 .. 64 are LA_ERR_ARG, a
 * smaller scratch_bytes is LA_ERR_WORKSPACE, all before anything is launched; the size queries are non-decreasing and 0 for what the
 * entries refuse.
 * ------------------------------------------------------------------------------------------------------------- */
int la_lap_pyr_down_f32(const float* x, float* y, long planes, int H, int W, la_stream_t stream);
int la_lap_pyr_up_sub_f32(float* fine, const float* coarse, long planes, int H, int W, la_stream_t stream);
int la_swd_gather_f32(const float* img, long n, int C, int H, int W, long img0, int level, int nhood, int per_image,
                      unsigned long long seed, float* desc, la_stream_t stream);
size_t la_swd_stats_scratch_bytes(long M, int C, int P);
int la_swd_channel_stats_f64(const float* desc, long M, int C, int P, double* mean, double* std, void* scratch, size_t scratch_bytes,
                             la_stream_t stream);
int la_swd_normalize_f32(float* desc, long M, int C, int P, const double* mean, const double* std, la_stream_t stream);
int la_swd_directions_f32(float* dirs, long ndirs, int D, long dir0, unsigned long long seed, la_stream_t stream);
size_t la_swd_scratch_bytes(long M, int D, long ndirs);
int la_swd_f32(const float* descA, const float* descB, long M, int D, const float* dirs, long ndirs, double* w1, void* scratch,
               size_t scratch_bytes, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Gram-matrix style distance and content distance of activation pairs: NSTLoss of augments/criteria/nst/nst.py:7-35 on the taps
 * of VGG19Net (networks.py:60-70).  f float32 [2P][C][HW]; rows p and p + P are a pair.  With G = F F^T / HW for F [C][HW]:
 *   style[p]   = mean over the C^2 entries of (G1 - G2)^2
 *   content[p] = mean over the C HW entries of (f1 - f2)^2          (content may be NULL)
 * computed from D = f1 - f2 and S = f1 + f2, both formed in float32 while loading: E = D S^T + S D^T = 2 HW (G1 - G2),
 * style = sum E^2 / (4 HW^2 C^2), content = sum D^2 / (C HW).  d(f, f) is exactly 0 and swapping the halves gives the same bits.
 * E: exact fp32 MFMA products in k-ordered chains over 128 x 128 tiles with I <= J; K = HW is split into la_gram_pair_slices(C, HW)
 * slices, a function of (C, HW) only, whose partials are added in slice order: a pair gives the same bits alone and at any
 * position of a batch.  Squares and sums in float64 in a fixed order, one division: no float atomics, two runs give the same bits;
 * no host sync, no allocation.  scratch: la_gram_pair_scratch_bytes(P, C, HW) bytes, 8-byte aligned, any contents (written before it
 * is read; non-decreasing in P; 0 for what the entry refuses: P outside 1 .. 65535, C outside 1 .. 8192, HW outside 1 .. 2^26).
 * Bad shapes and null pointers are LA_ERR_ARG, a smaller scratch_bytes is LA_ERR_WORKSPACE, all before anything is launched.
 * la_feat_style_distance (tap lists only): the trunk once on xy [2P][in_ch][in_res^2] with the entry above as its tap step, on the
 * raw activation each LA_FEAT_TAP sees (lin is not read): style, content float64 [P][ntaps].  Same contract as
 * la_feat_pair_distance: it overwrites the activations of an earlier la_feat_forward (la_feat_backward then refuses until the next
 * forward); la_feat_style_scratch_bytes is 0 for a detector list or 2P > max_batch, which the entry refuses with LA_ERR_ARG.
 * ------------------------------------------------------------------------------------------------------------- */
size_t la_gram_pair_scratch_bytes(int P, int C, int HW);
int la_gram_pair_slices(int C, int HW);
int la_gram_pair_dist_f32(const float* f, int P, int C, int HW, double* style, double* content, void* scratch, size_t scratch_bytes,
                          la_stream_t stream);
size_t la_feat_style_scratch_bytes(const la_feat* h, int P);
int la_feat_style_distance(la_feat* h, const float* xy, int P, double* style, double* content, void* scratch, size_t scratch_bytes,
                           la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Paired image metrics (no reference counterpart): what describes a PAIR of images.  Images are float32 [N][C][H][W]; pair p is
 * (x[ix[p]], y[iy[p]]), ix / iy int32 device arrays of length P (NULL: p itself; the caller vouches for the range of the indices).
 *
 * la_pair_metrics_f32, per plane (p, c):
 *   err [P][C][2]        sum d^2 and sum |d| over the H W pixels, d = x - y formed in float32, accumulated in float64 in a fixed order.
 *   ssim, cs [P][C][levels]   means over the 'valid' extent (h - win + 1) x (w - win + 1) of a level of
 *                          cs   = (2 s_xy + c2) / (s_xx + s_yy + c2)
 *                          ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * cs
 *                        with mu_x = g * x, s_xx = g * (x x) - mu_x^2 (likewise s_yy, s_xy) and g the separable window taps_host[win]
 *                        (win odd, 1 .. 11).  The next level is the 2 x 2 mean with stride 2 of both images: H and W must be multiples
 *                        of 2^(levels-1), the last level at least win x win, 1 <= levels <= 5.
 *   ms [P][C]            prod_{l < levels-1} max(cs_l, 0)^w_l * max(ssim_{levels-1}, 0)^w_{levels-1}, w = weights_host[levels] (>= 0),
 *                        from the float64 means; a negative factor gives exactly 0.  levels = 1 with w = {1} is SSIM clamped at 0.
 * One fused launch per level (a workgroup owns a 32 x 32 block: both images with their halo in LDS, row pass, column pass, the two
 * quotients, one float64 partial pair per tile; the same launch writes the next level's images and, on level 0, the error partials),
 * one launch that adds the tile partials per plane in tile order, one that combines the levels.  No float atomics: two runs give the
 * same bits.  workspace: la_pair_metrics_workspace_bytes bytes, 8-byte aligned (partials and the pyramid; 0: the shape is refused).
 * A refused shape is LA_ERR_ARG and a short workspace LA_ERR_WORKSPACE, both before any launch.
 *
 * la_joint_hist_f32: hist[p][bin(a_i)][bin(b_i)] += 1 (uint32) over the npix values of plane p of a (at a + p * a_plane_stride floats)
 * and of b, bin(v) = min(bins - 1, max(0, (int)floorf((v - lo) * scale))) in float32, 1 <= bins <= 64; the caller passes
 * scale = float32(bins / (hi - lo)).  The entry zeroes hist on `stream`.  Workgroups count in LDS and add their non-zero bins with
 * integer atomics: order-independent, two runs give the same counts.  The plane strides let two channels of one [N][2][H][W] tensor be
 * read in place.
 * ------------------------------------------------------------------------------------------------------------- */
size_t la_pair_metrics_workspace_bytes(long P, int C, int H, int W, int win, int levels);
int la_pair_metrics_f32(const float* x, const float* y, const int* ix, const int* iy, long P, int C, int H, int W,
                        const float* taps_host, int win, int levels, const float* weights_host, float c1, float c2, double* err,
                        float* ssim, float* cs, float* ms, void* workspace, size_t workspace_bytes, la_stream_t stream);
int la_joint_hist_f32(const float* a, long a_plane_stride, const float* b, long b_plane_stride, long planes, long npix, int bins,
                      float lo, float scale, unsigned* hist, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Points on latent paths (no reference counterpart): the inputs of perceptual path length (Karras et al. 2019 / 2020).
 *
 * la_path_points_f32: a, b float32 [N][D] and t float32 [N] on the device, dt_host double [T] on the host, 1 <= T <= 64.
 *   out [T][N][reps][D] = the point of path p, from a[p] to b[p], at parameter s = (double)t[p] + dt_host[k], written reps times
 *   (reps = num_ws broadcasts a W point to the layers; reps = 1 for Z, or for W+ rows with D = num_ws * w_dim).
 *   mode 0, lerp:   a + (b - a) * s.
 *   mode 1, slerp of the published PPL: with a' = a / |a|, b' = b / |b|, d = <a', b'>, c = (b' - d a') / |b' - d a'|, omega = acos(d):
 *                   normalise(a' cos(s omega) + c sin(s omega)).  omega is evaluated as atan2(|b' - d a'|, d), the same angle without
 *                   acos's loss of digits next to d = +-1 (a rounded d above 1 would make acos NaN), so a == b gives a'.
 *                   Where |b' - d a'| == 0 (identical or opposite directions) every point is a'; the published form gives NaN there.
 *                   Nearly opposite rows have no stable geodesic: c is then rounding noise.  A zero row has no direction and
 *                   gives NaN, as the published form does.
 *   s outside [0, 1] extrapolates (t + eps next to 1).  Every operation is in double, in the order written and unfused, and the result is
 *   rounded once to float32: t + dt is never formed in float32, and the lerp equals its float64 restatement bit for bit.
 *   One workgroup per path; the norms and the dot product are block reductions in a fixed order, no atomics: two runs give the same bits.
 *   Null pointers, N, D, reps < 1, T outside 1 .. 64 and an unknown mode are LA_ERR_ARG before any launch; a failed launch is LA_ERR_HIP.
 * ------------------------------------------------------------------------------------------------------------- */
int la_path_points_f32(const float* a, const float* b, const float* t, const double* dt_host, int T, int N, int D, int reps, int mode,
                       float* out, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Projector: inversion of images into W / W+ (Karras et al. 2020, Appendix D; the per-layer noise maps are optimised on request, with the
 * published regulariser and re-normalisation, and then discarded).  The reference reads inverted
 * latents (augments/latent_aug.py:310-324) and has no code that makes them.  The optimisation is an eager sequence of launches over
 * the synthesis and feature engines (latentaugment_amd/projector.py); these are the kernels that only it needs.  No atomics: two runs
 * give the same bits.  Bad arguments are LA_ERR_ARG before any launch.
 *   la_row_dist_f32   a, t [rows][K]: loss[j * loss_stride] = scale * sum_{c < fold} sum_k (a - t)^2 over row c * (rows / fold) + j, for
 *                     j < rows / fold (fold = 1: one value per row; fold = C: the modality-major rows of la_crop_repeat_f32 folded per
 *                     sample), and, g not null, g = gscale * (a - t) -- accumulate != 0: added to g.  The difference is formed in
 *                     float32 and its square summed in float64 in an order fixed by the shape.  ws: la_row_dist_workspace_bytes(rows, K)
 *                     bytes, 8-byte aligned (LA_ERR_WORKSPACE when short).  rows at most 65535.  Any 4-byte aligned a, t, g.
 *   la_box_down_f32   x [planes][R][R] -> y [planes][R / k][R / k], the mean of each k x k box; k in 1, 2, 4, 8 and R a multiple of k.
 *                     Exact on integer-valued planes.  la_box_up_f32: its adjoint, gx [planes][R][R] = gy[..][Y / k][X / k] / k^2 (written).
 *   la_proj_step_tail_f32   one launch for the end of a step.  p, m, v, ws are [B][L][wdim] with L = 1 (wplus = 0) or num_ws; dws is
 *                     [B][num_ws][wdim], in W space summed over its num_ws rows in index order.  p, m, v take the Adam step of
 *                     la_adam_step_f32 (`step` 1-based, lr of this step), then ws = p + sigma * n with n the unit normal of
 *                     (seed, layer, row0 + b, element l * wdim + j): the stream of la_noise_normal_f32 with rows of L * wdim elements.
 *                     dws null: no update, ws alone is written (m, v may be null).
 *   The noise maps: a table of nmaps maps for one batch, map i being [B][res[i]][res[i]] with res[i] = 4 << k (anything else is refused).
 *   la_noise_reg_f32  the published regulariser of every map and sample -- per pyramid level (the map, then 2 x 2 averages of it while
 *                     the level above is larger than 8 x 8) the squared means of n * roll(n, 1, x) and n * roll(n, 1, y), shifts cyclic --
 *                     reg[b * reg_stride] = scale * (sum over maps, levels), and its gradient gn[i] = weight * g (accumulate != 0: added).
 *                     Levels are float32, every sum float64 in an order fixed by the shapes.  One launch per pyramid level over all maps
 *                     (it adds up level l and builds level l + 1), one that finishes the sums, one that gathers the gradient.
 *                     ws: la_noise_reg_scratch_bytes(res, nmaps, B) bytes, 8-byte aligned, any contents (LA_ERR_WORKSPACE when short).
 *   la_proj_noise_tail_f32   the end of a step for the maps: Adam as above (one optimiser over latent and maps: the same lr, betas,
 *                     eps, step) on n, m, v from gn, then n -= mean(n); n *= rsqrt(mean(n^2)) per map and sample, moments in float64 in a
 *                     fixed order (the squares are those of the centred values).  A map whose centred mean square is exactly 0 is left
 *                     at zeros.  Three launches over all maps.  ws: la_proj_noise_tail_scratch_bytes(res, nmaps, B) bytes.
 * ------------------------------------------------------------------------------------------------------------- */
size_t la_row_dist_workspace_bytes(int rows, long K);
int la_row_dist_f32(const float* a, const float* t, int rows, long K, int fold, double scale, float gscale, float* g, int accumulate,
                    double* loss, long loss_stride, void* ws, size_t ws_bytes, la_stream_t stream);
int la_box_down_f32(const float* x, float* y, long planes, int R, int k, la_stream_t stream);
int la_box_up_f32(const float* gy, float* gx, long planes, int R, int k, la_stream_t stream);
int la_proj_step_tail_f32(const float* dws, float* p, float* m, float* v, float* ws, int B, int num_ws, int wdim, int wplus, int step,
                          float lr, float beta1, float beta2, float eps, float sigma, unsigned long long seed, unsigned layer, long row0,
                          la_stream_t stream);
size_t la_noise_reg_scratch_bytes(const int* res, int nmaps, int B);
int la_noise_reg_f32(const float* const* maps, const int* res, int nmaps, int B, double scale, float weight, float* const* gn, int accumulate,
                     double* reg, long reg_stride, void* ws, size_t ws_bytes, la_stream_t stream);
size_t la_proj_noise_tail_scratch_bytes(const int* res, int nmaps, int B);
int la_proj_noise_tail_f32(const float* const* gn, float* const* n, float* const* m, float* const* v, const int* res, int nmaps, int B, int step,
                           float lr, float beta1, float beta2, float eps, void* ws, size_t ws_bytes, la_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Opt-in profiler for the contraction launches (HIP events on the launch stream).  No reference counterpart: the
 * reference's only timing hook is wall-clock stats_time (augments/latent_aug.py:276).
 * la_prof_end: summed device ms, launch count, algorithmic FLOPs (2*MACs) and algorithmic bytes (input + output +
 * weights, each once) of every la_conv launch since la_prof_begin.
 * ------------------------------------------------------------------------------------------------------------- */
int la_prof_begin(void);
int la_prof_end(double* total_ms, long* launches, double* flops, double* bytes);
/* la_prof_set_stride(k): bracket a hashed 1-in-k sample of the launches instead of all of them (an event pair costs ~3 us on
 * the stream); la_prof_end then reports the sampled launches' ms / count / FLOPs / bytes, la_prof_total_launches() all of them. */
int la_prof_set_stride(int stride);
/* (The development build, `make dev` -> liblatentaug_hip_dev.so, additionally exports `la_dev_knob_set` (int id, int value -> int): it
 *  selects kernel variants for in-process A/B timing by scripts/bench_layer.py --ab.  The product library has no such symbol, no
 *  kernel-variant state and reads no LA_* environment variable.) */
long la_prof_total_launches(void);
/* Per kernel class (la_prof_num_classes() entries per array): 0 contraction / halo, 1 contraction / flat, 2 contraction /
 * split-K incl. its finish pass, 3 contraction / exact-fp32 MFMA, 4 operand preparation (plane maxima, pre-split copy),
 * 5 FIR (upfirdn2d family), 6 backward seam (bias_act backward + ToRGB backward), 7 ToRGB forward, 8 bank scans.
 * Bytes are the algorithmic ones (each operand once).  While the profiler is on, the step loop launches eagerly. */
int la_prof_num_classes(void);
int la_prof_end_classes(double* ms, long* launches, double* flops, double* bytes, int nclass);

#ifdef __cplusplus
}
#endif
#endif /* LATENTAUG_HIP_H */
