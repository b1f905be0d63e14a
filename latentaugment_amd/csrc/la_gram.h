// Internal (C++) form of the Gram-matrix style and content distance of activation pairs (la_gram.hip); the C ABI is in
// include/latentaug_hip.h.
#pragma once
#include "la_common.h"

// la_gram_pair_dist_f32 with an output stride: style[p * ostride], content[p * ostride] (the trunk entry la_feat_style_distance writes
// column `tap` of [P][ntaps]).  Checks nothing: the callers have refused bad shapes and short scratch before their first launch.
int la_gram_pair_launch(const float* f, int P, int C, int HW, double* style, double* content, long ostride, void* scratch, hipStream_t stream);
