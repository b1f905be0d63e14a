// Internal (C++) forms of the feature engine's general convolution and 3x3 stride-2 max pool (la_feat_conv.hip): the trunk ops of the
// AlexNet and SqueezeNet 1.1 LPIPS nets that la_conv*.hip (3x3, pad 1) and the 2x2 pools of la_feat.hip cannot describe.
// Everything here is exact fp32 in every precision mode of the engine, uses no float atomics (two runs give the same bits), does not
// synchronise with the host and allocates nothing: a captured step replays it.
#pragma once
#include "la_common.h"

#define LA_FCV_KMAX 11      // largest square kernel

// y[n][c_off + co][oy][ox] = relu(b[co] + sum_{ci,ky,kx} x[n][ci][oy*stride - pad + ky][ox*stride - pad + kx] * w[co][ci][ky][kx])
// x [N][cin][R][R]; y has c_total channels of Ro x Ro, Ro = (R + 2 pad - k) / stride + 1 (floor); the launch writes channels
// [c_off, c_off + cout) of it and no other (a Fire module's two expand branches share one output).
struct LaFeatConvGeom { int cin, cout, k, stride, pad, R, Ro; };

// Ro of the geometry, or 0 where it is refused: k 1 .. 11, stride 1 | 2 | 4, pad 0 .. 5, pad < k, cout % 4 == 0, cin % 4 == 0 or cin == 3,
// R + 2 pad >= k
int la_featconv_out_res(int cin, int cout, int k, int stride, int pad, int R);
// floats of the split-K partials la_featconv_forward may need for any batch 1 .. maxN
size_t la_featconv_part_floats(int maxN, const LaFeatConvGeom& g);
int la_featconv_forward(const float* x, const float* w, const float* b, float* y, int N, const LaFeatConvGeom& g, int c_off, int c_total,
                        float* part, size_t part_floats, hipStream_t stream);
// gx[n][ci][iy][ix] (+)= sum_{co,ky,kx} [y > 0] gy[n][c_off + co][(iy + pad - ky) / stride][(ix + pad - kx) / stride] * w[co][ci][ky][kx]
// over the taps whose division is exact and in range; gy and the saved output y share the [N][c_total][Ro][Ro] layout.
// accumulate != 0: added onto gx (the second expand branch of a Fire module).  A stride-1 layer with cin % 4 == 0 runs on the forward's
// GEMM kernel (flipped kernel, pad k - 1 - pad; part: the same split-K partials), every other layer as a gather per input element.
int la_featconv_backward(const float* gy, const float* y, const float* w, float* gx, int N, const LaFeatConvGeom& g, int c_off, int c_total,
                         int accumulate, float* part, size_t part_floats, hipStream_t stream);

// 3x3 stride-2 max pool without padding: output size by torch's rule (ceil mode: the last window must start inside the input); 0: refused
int la_pool3s2_out_res(int R, int ceil_mode);
int la_pool3s2_forward(const float* x, float* y, long planes, int R, int Ro, hipStream_t stream);
int la_pool3s2_backward(const float* x, const float* gy, float* gx, long planes, int R, int Ro, hipStream_t stream);
