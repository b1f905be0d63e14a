// Internal (C++) interface of la_style.hip.
#pragma once
#include "la_common.h"
#include "la_conv.h"

#define LA_MAX_STYLE_LAYERS 40

// One row block per affine layer (conv layers first, then ToRGB layers); rows = that layer's in_channels.
struct LaStyleTable {
    int nlayers;
    int total_rows;
    int row_start[LA_MAX_STYLE_LAYERS + 1];   // row_start[nlayers] == total_rows
    int widx[LA_MAX_STYLE_LAYERS];            // which w of ws[b][.] feeds the layer
    float post_gain[LA_MAX_STYLE_LAYERS];     // 1 for conv layers, 1/sqrt(cin) for ToRGB (weight_gain folded into the style)
    const float* aw[LA_MAX_STYLE_LAYERS];     // affine.weight [cin][wdim]
    const float* ab[LA_MAX_STYLE_LAYERS];     // affine.bias   [cin]
};

struct LaDemodTable {
    int nlayers;
    int total_rows;
    int row_start[LA_MAX_STYLE_LAYERS + 1];
    int cin[LA_MAX_STYLE_LAYERS];
    int s_off[LA_MAX_STYLE_LAYERS];           // offset of the layer's styles inside a row of s_all
    const float* wsq[LA_MAX_STYLE_LAYERS];    // [cout][cin]
};

struct LaSeamArgs {
    const float* y;          // [B][C][HW] saved post-activation output of the layer
    const float* gx_next;    // [B][C][HW] or null
    float* gz;               // [B][C][HW] (may alias gx_next)
    long HW;
    int C;
    const float* demod; int demod_stride;      // the layer's epilogue, in the seam order (la_seam_set_epi)
    const float* bias;
    const float* noise; long noise_bstride; float noise_strength;
    int act; float alpha, gain, clamp;
    float* ddn_part;         // [B][C][slabs]
    // ToRGB part (imgc > 0)
    const float* g_img;      // [B][imgc][HW] gradient w.r.t. the image at this resolution
    const float* rgb_pre;    // [B][imgc][HW] ToRGB output before its clamp
    float rgb_clamp;
    const float* wrgb;       // [imgc][C]
    const float* s_rgb; int s_stride;   // styles of the ToRGB layer (already * weight_gain)
    float* dweff_part;       // [B][imgc][C][slabs]
    float* pmax_out;         // optional [B][C][slabs]: partial max |gz| per plane (one per workgroup)
    float* xs_out; float xs_mult;      // optional slot rows [B][LA_XS_FAN] (la_common.h): fp16 operand scale of gz for its consumer, pow2 scale of xs_mult * max|gz|
    long p_lo, p_hi;         // pixel window, not a LaWindow: a range of flattened pixels (multiples of 4; 0 / 0 = the whole plane): only pixels [p_lo, p_hi) of every plane are read and written --
                             // the incoming gradient is zero outside them (la_synth.hip: row windows); the slabs share the window
};

int la_affine_forward(const LaStyleTable& t, const float* ws, long ws_bstride, long ws_lstride, int B, int wdim,
                      float* s_all, hipStream_t);
// xscale (optional, fp16 x2 mode), in the same launch, the start of a pass for the fp16 operand scales: resets the slot rows xs
// [nlayers][B][LA_XS_FAN] (layer 0: the scale of the constant input `cst`, cst_n floats) and xs_bwd (optional) and writes xs_mult
// [nlayers][B] = max_i |style| of every layer (la_style.hip)
struct LaXscaleBounds { const float* cst; int cst_n; float* xs; float* xs_mult; float* xs_bwd; };
int la_demod_forward(const LaDemodTable& t, const float* s_all, int s_stride, int B, float* d_all, hipStream_t, const LaXscaleBounds* xscale = nullptr);
// mask (optional, planes above 64x64): x is a gradient still to be taken through an activation -- x[b][i][p] * act'(mask.y[b][i][p]) is what
// the 1x1 reads (the discriminator's FromRGB backward: one stream of the gradient and the saved output instead of a sweep + a stream)
struct LaTorgbMask { const float* y; int act; float alpha, gain, clamp; };
// r: the ToRGB layer as LaRgbFuse describes it (la_conv.h; s null = no modulation, rgb_pre null = not kept)
int la_torgb_forward(const float* x, const LaRgbFuse& r, int B, int C, int H, int W, hipStream_t, const LaTorgbMask* mask = nullptr, int row_lo = 0,
                     int row_hi = 0, const float* skip_lo = nullptr, const float* fir_host = nullptr);      // skip_lo + fir_host: the block below's image, up-sampled inside the kernel
// row_lo / row_hi (planes above 64x64; 0 / 0 = all): only these rows of rgb_pre / img are computed and written
// la_torgb_forward's kernel choice: planes up to 64x64 take the small kernel (whole planes: no row window, no mask), larger ones the large
static inline bool la_torgb_small(long HW) { return HW <= 4096; }
// The ToRGB layers of several blocks whose images nobody reads before the last of them has run, in two launches instead of one per block
// (la_synth.hip: the blocks below the first fused ToRGB).  Tables by value, lowest level first.
//   la_torgb_forward_levels  rgb_pre of every level: per level la_torgb_forward's channel sum (same kernel form per plane size, same order:
//                            the same bits), rows [row_lo, row_hi) of a plane above 64x64 (0 / 0 = all)
//   la_image_chain_forward   img_k = clamp(rgb_pre_k) + upsample2d(img_{k-1}) level by level (base: the image below the first level, or null),
//                            each level's rows [row_lo, row_hi) (they must lie inside what the level below delivers); skip (optional): the
//                            up-sampled image of the LAST level [B][imgc][2H][2W], whole planes -- what a fused
//                            ToRGB one block up reads (LaRgbFuse::skip), equal to la_upfirdn2d_ex(.., la_fir_up2()) of that image; it needs
//                            the levels below the last within 64x64 and the last within 128x128 (the kernel's LDS strips), else refused
#define LA_TORGB_MAX_LEVELS 12
struct LaTorgbLevels {
    int n, imgc, s_stride;
    struct Level { const float* x; int C, H, W; const float* wrgb; const float* s; const float* bias; float* rgb_pre; int row_lo, row_hi; } lv[LA_TORGB_MAX_LEVELS];
};
struct LaImageChain {
    int n, imgc; float clamp;
    const float* base;
    struct Level { const float* rgb_pre; float* img; int H, W, row_lo, row_hi; } lv[LA_TORGB_MAX_LEVELS];
    float* skip;
};
int la_torgb_forward_levels(const LaTorgbLevels& t, int B, hipStream_t);
int la_image_chain_forward(const LaImageChain& t, int B, const float* fir_host, hipStream_t);
int la_seam_slabs(long HW);
int la_seam_backward(const LaSeamArgs& a, int B, int imgc, hipStream_t);
// Style-gradient finish of ALL layers of one backward pass in three launches (row sums of every partial buffer, conv layers,
// ToRGB layers) instead of three small launches per layer: the per-layer partial buffers are kept until the end of the pass.
#define LA_FIN_MAX_CONV 24
#define LA_FIN_MAX_RGB 12
struct LaStyleFinish {
    int nconv, nrgb, imgc, d_stride, s_stride, ds_stride;
    struct Conv { float* ds_part; float* ddn_part; const float* d; const float* s; const float* wsq; float* ds_out; int ntiles, nslabs, cin, cout, blk0; } conv[LA_FIN_MAX_CONV];
    struct Rgb { float* dweff_part; const float* wrgb; float* ds_out; int nslabs, C, blk0; } rgb[LA_FIN_MAX_RGB];
};
int la_style_backward_all(const LaStyleFinish& f, int B, hipStream_t stream);
int la_affine_bwd_chunks(const LaStyleTable& t);   // part scratch = chunks * B * wdim floats
int la_affine_backward(const LaStyleTable& t, const float* ds_all, int B, int wdim, float* dws, int num_ws, float* part,
                       hipStream_t);
