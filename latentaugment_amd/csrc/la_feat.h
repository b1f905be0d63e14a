// Internal (C++) forms of the perceptual feature engine's crop + repeat (la_feat.hip); the engine's C ABI is in include/latentaug_hip.h.
#pragma once
#include "la_common.h"

// window position read from device memory {y0, x0} when pos_dev != null (captured launches)
int la_crop_repeat_ex(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep, float scale,
                      float shift, hipStream_t stream);
int la_crop_repeat_grad_ex(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                           float scale, hipStream_t stream);
// per-repeated-channel affine ([rep] values each, rep <= 4): the input layer of an ImageNet-style net, (x - mean_k) / std_k
int la_crop_repeat_ex3(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                       const float* scale, const float* shift, hipStream_t stream);
int la_crop_repeat_grad_ex3(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                            const float* scale, hipStream_t stream);
