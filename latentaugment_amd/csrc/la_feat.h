// Internal (C++) forms of the perceptual feature engine's crop + repeat (la_feat.hip); the engine's C ABI is in include/latentaug_hip.h.
#pragma once
#include "la_common.h"

// The public la_crop_repeat_f32 / _grad_f32 with a per-repeated-channel affine ([rep] values each, rep <= 4: the input layer of an
// ImageNet-style net, (x - mean_k) / std_k) and the window position read from device memory {y0, x0} when pos_dev != null (captured launches)
int la_crop_repeat(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                   const float* scale, const float* shift, hipStream_t stream);
int la_crop_repeat_grad(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                        const float* scale, hipStream_t stream);
