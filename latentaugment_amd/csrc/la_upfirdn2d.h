// Internal (C++) entry points of the FIR resampling kernels; the public C ABI is in include/latentaug_hip.h.
#pragma once
#include "la_common.h"
#include "la_launch_args.h"

// What every upfirdn2d entry (float16 / float32 / float64) derives from its arguments: the argument checks, the output size
// (upfirdn2d.cpp:35-36) and the correlation taps in float32 -- up to 8 x 8, or one separable pass of up to 32 (1 x fw / fh x 1, the
// two-pass form of upfirdn2d.py:188-201 for 1-D filters); the op is a true convolution unless flip_filter, so the taps are the flipped
// filter (upfirdn2d.py:198-199).  The gain goes onto the float32 taps IN float32 whatever the dtype of x: upfirdn2d.py:196-197
// multiplies the float32 filter tensor by the gain before converting it to the dtype of x, so a float64 call sees a non-power-of-two
// gain rounded to float32 and widens the product exactly.
#define LA_FIR_MAX 8
struct LaFirSetup {
    int Hout, Wout;
    float f[LA_FIR_MAX * LA_FIR_MAX];
};
int la_fir_setup(LaFirSetup& s, const void* in, const void* out, int B, int C, int Hin, int Win, const float* f_host, const LaFirGeom& g);

// The generic kernels' gather of output (x, y) of one input plane `ip` (storage T, sum in A): the contributing input rows are
// iy * upy = y * dny + ta - pady0 with ta in [0, fh), columns likewise; taps in ascending row, then column order.
// Args: FirArgs (la_upfirdn2d.hip) or LaFirOpArgs<T> (la_ops.hip).
template <class A, class T, class Args>
__device__ __forceinline__ A la_fir_gather(const Args& a, const T* ip, int x, int y) {
    const int by = y * a.dny - a.pady0, bx = x * a.dnx - a.padx0;
    // smallest iy with iy * upy >= by  (floor division that is safe for negatives)
    const int iy_lo = (by >= 0) ? (by + a.upy - 1) / a.upy : -((-by) / a.upy);
    const int ix_lo = (bx >= 0) ? (bx + a.upx - 1) / a.upx : -((-bx) / a.upx);
    A v = 0;
    for (int iy = iy_lo; iy * a.upy - by < a.fh; ++iy) {
        if (iy < 0 || iy >= a.Hin) continue;
        const int ta = iy * a.upy - by;
        for (int ix = ix_lo; ix * a.upx - bx < a.fw; ++ix) {
            if (ix < 0 || ix >= a.Win) continue;
            v += (A)ip[(long)iy * a.Win + ix] * a.f[ta * a.fw + (ix * a.upx - bx)];
        }
    }
    return v;
}

// The options of a FIR launch, all off by default:
//   addend   same-shape tensor added to the result (skip connection add fused into the store); plain launches only
//   pmax     [B*C][la_fir4x4_segments(Hout, Wout)]: partial max |out| of every plane, one per workgroup (4x4 stride-1 scalar kernel) -- lets
//            the contraction that consumes `out` skip its own absmax pass (fp16 operand scale)
//   yref ..  activation backward of the layer whose saved output `yref` has the shape of `out` (4x4 stride-1 kernels: out = fir(in) *
//            act'(yref), bias_act.py:170 with grad = 1)
//   xs_out / xs_mult  slot rows [B][LA_XS_FAN] of the fp16 operand scale of `out` for the contraction that consumes it (la_common.h),
//            lowered by the producing workgroups to pow2(xs_mult[b] * max |out|), xs_mult null = 1 (4x4 stride-1 and up-2 kernels)
//   in_pitch / in_plane  (floats, 0 = dense; 4x4 stride-1 only) padded row pitch / plane stride of `in` (multiples of 4 select the vector kernel)
//   in_xhalf (> 0, needs in_pitch) column-planar rows -- even columns of the image at [0, ceil(Win/2)), odd columns from in_xhalf on
//   win      (column-planar input only) only these output rows / 4-column groups are computed and written
struct LaFirTail {
    const float* yref = nullptr; int act = LA_ACT_LINEAR; float alpha = 0.f, gain = 1.f, clamp = -1.f;
    float* xs_out = nullptr; const float* xs_mult = nullptr;
    int in_pitch = 0; long in_plane = 0; int in_xhalf = 0;
    const float* addend = nullptr;
    float* pmax = nullptr;
    LaWindow win = {};
};
int la_upfirdn2d_ex(const float* in, float* out, int B, int C, int Hin, int Win, const float* f_host, const LaFirGeom& g, hipStream_t stream,
                    const LaFirTail& opts = LaFirTail());
int la_fir4x4_segments(int Hout, int Wout);

// FIR (up=down=1) followed by the modulated-conv epilogue: *demod[b][c] + noise*strength + bias[c] -> act -> clamp.
// Used after the transposed stride-2 conv of an up-sampling SynthesisLayer (conv2d_resample.py:126).  opts: pmax, xs_out / xs_mult, the
// input layout and the window (yref and addend do not apply).
int la_upfirdn2d_modconv_epilogue(const float* in, float* out, int B, int C, int Hin, int Win, const float* f_host, const LaFirGeom& g,
                                  const LaLayerEpi& epi, hipStream_t stream, const LaFirTail& opts = LaFirTail());

// FIR adjoint of an up-sampling layer written straight into the stride-2 backward contraction's operand format (fp16 mode):
// q [B][ceil(C/32)][(H+1)*(W+1)][32 channels] = {h | l << 16} of xscale[b] * adjoint(in); see la_upfirdn2d.hip
// in_win: valid rows / columns of `in` (the others read as zeros); out_win: rows / columns of the (H+1) x (W+1) output
// that the contraction reads (8-row x 64-column tiles outside it are not written)
// flip_taps = 1: the forward 4x4 FIR with pad 2 (same geometry: (H+1) x (W+1) outputs) instead of the adjoint of the pad-1 FIR
int la_fir4x4_adjoint_pack_f16(const float* in, unsigned* q, const float* xscale, int xs_fan, int B, int C, int H, int W, const float* f_host,
                               float gain, hipStream_t stream, int flip_taps = 0, const LaWindow& in_win = LaWindow{},
                               const LaWindow& out_win = LaWindow{});
static inline size_t la_fir4x4_adjoint_pack_bytes(int B, int C, int H, int W) { return (size_t)B * la_cdiv(C, 32) * 32 * (H + 1) * (W + 1) * 4; }      // bytes of q

// The image-gradient pyramid of a synthesis backward pass in one launch: outs[l] [planes][R0 >> (l+1)]^2 = adjoint of upsample2d applied l + 1
// times to g_top [planes][R0]^2 (per level exactly la_upfirdn2d_ex(.., la_fir_down2_adjoint())); R0 <= 256: the kernel keeps two levels in LDS,
// ((R0/2)^2 + (R0/4)^2) * 4 bytes = 80 KB at R0 = 256, and raises its dynamic-LDS limit to 96 KB for that.
int la_image_grad_pyramid(const float* g_top, float* const* outs, int nlev, int planes, int R0, const float* f_host, hipStream_t stream);
