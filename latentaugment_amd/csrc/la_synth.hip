// StyleGAN2 synthesis network (architecture 'skip') forward + backward-to-latent as a sequence of HIP launches.
// Mirrors the call  G.synthesis(ws, noise_mode=...)  at augments/utils/util_latent_aug.py:227,488 and the autograd
// backward of it that loss.backward() at :275 performs, restricted to d/d(ws) (G is frozen: :480).
// Formulation: non-fused modulated conv (x*s -> shared-weight contraction -> *demod), see DESIGN.md.
#include "la_common.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "la_conv.h"
#include "la_modconv.h"
#include "la_style.h"
#include "la_upfirdn2d.h"

#define MAX_BLOCKS 12

struct ConvLayer : LaConvWeights {      // (channel counts are multiples of 4: cin_pad = cin; wsq feeds the demodulation)
    int res, up, widx;
    const float *affine_w, *affine_b, *bias, *noise_const;
    float noise_strength;
    float* y;               // saved output [maxB][cout][res*res]
    float *dsp, *ddnp;      // style-gradient partials of this layer (kept until the one-pass finish at the end of a backward pass)
    int s_off, d_off, style_idx;
    const float* noise_used;   // set by forward (null when the term vanishes)
    long noise_bstride;
};

struct RgbLayer {
    int cin, res, widx;
    const float *affine_w, *affine_b, *weight, *bias;
    int s_off, style_idx;
    float *rgb_pre, *img, *g_img;
    float* dwep;            // ToRGB weight-gradient partials [maxB][imgc][cin][slabs]
};

// What a forward pass and the backward pass that differentiates it decide before they launch anything.  plan_pass builds the record on the
// host (no handle memory, no stream, no launch), la_synth_forward stores it in the handle, both passes execute it, la_synth_plan_query shows
// it: every member is an int, in the order of the LA_SYNTH_PLAN_* constants of include/latentaug_hip.h, which describes each of them.
struct SynthPlan {
    struct Pass { int nblocks, nconv, B, precision, f16, xs_hand, zt_dense, cone; } pass;      // (B = 0: no pass planned)
    // per conv layer; rows: what its backward launch reads (in) of the gradient of its output and writes (out) of the gradient of its input
    struct Layer { LaWindow fwd; int cone_lo, cone_hi, win; LaBwdRows rows; int seam, seam_pmax, pmax_in, nseg, ntiles; } conv[2 * MAX_BLOCKS];
    struct Block { int fuse_rgb, skip_up, img_lo, img_hi, down_fir, pyramid; } blk[MAX_BLOCKS];
};
static_assert(sizeof(SynthPlan::Pass) == LA_SYNTH_PLAN_PASS_N * sizeof(int) && sizeof(SynthPlan::Layer) == LA_SYNTH_PLAN_LAYER_N * sizeof(int) &&
              sizeof(SynthPlan::Block) == LA_SYNTH_PLAN_BLOCK_N * sizeof(int) && sizeof(SynthPlan) == LA_SYNTH_PLAN_NINFO * sizeof(int), "SynthPlan and its query disagree");

struct la_synth {
    int R, imgc, wdim, nblocks, num_ws, maxB;
    int channels[MAX_BLOCKS];
    float clamp;
    const float* cst;   // b4.const [C4][4][4]
    int nconv;
    ConvLayer conv[2 * MAX_BLOCKS];
    RgbLayer rgb[MAX_BLOCKS];
    float fir[16];
    LaStyleTable st;
    LaDemodTable dt;
    int S, Dt;
    float *s_all, *d_all, *ds_all;
    float *zT, *G0, *G1, *aff_part;
    void* cws;
    size_t cws_bytes;
    float* pmax;             // [maxB][max channels]: plane maxima handed from a producing kernel to the next contraction (fp16 mode)
    float* pmax3;            // the same for a block's conv1 output when ITS seam (incl. ToRGB backward) is fused into the epilogue of the
                             // up-sampling layer's backward contraction of the block above
    float* pmax2;            // [maxB][cout][tiles]: plane maxima of an up-sampling layer's gz when its seam is fused into the epilogue of
                             // the conv1 backward contraction above it
    float* xs_fwd;           // [nconv][B][LA_XS_FAN] slot rows: fp16 operand scales of the forward contractions (from the clamp bound, one launch per pass)
    float* xs_bwd;           // [nconv][B][LA_XS_FAN] slot rows: running fp16 operand scales of the backward contractions' inputs, lowered by the producing kernels
    float* xs_mult;          // [nconv][B]: max_i |style| of every conv layer = what the producer of its input multiplies its max |x| with
    int precision;
    float* final_img;   // where the last forward put the full-resolution image
    LaWindow win;       // window of the image the next forward passes are asked for (la_synth_set_row_window / _col_window; 0 / 0 on an axis = all)
    SynthPlan plan;     // of the LAST forward pass: what it ran and what its backward pass runs
    const float* g_top; // image gradient the running backward pass was handed (top block)
    float up_mult;      // la_modconv_up2_bwd_xs_mult of the filter
    int rgb_per_block;  // la_synth_set_torgb_schedule: a ToRGB launch behind every block's conv1 (else deferred, see plan_pass)
    int settings_gen;   // la_synth_settings_gen: raised when precision or ToRGB schedule change
};

enum { SEAM_KERNEL = LA_SYNTH_SEAM_KERNEL, SEAM_FUSED = LA_SYNTH_SEAM_FUSED, PMAX_NONE = LA_SYNTH_PMAX_NONE, PMAX_1, PMAX_2, PMAX_3 };
enum { SKIP_NONE = 0, SKIP_LAUNCH = LA_SYNTH_SKIP_LAUNCH, SKIP_CHAIN = LA_SYNTH_SKIP_CHAIN };

// Windows of a pass (P.pass.nblocks / nconv set, the rest zero) for the image window `img`, top block downwards until a row window is the
// whole plane.
//   fwd rows   what the FORWARD pass computes of every conv output: conv1 in 4-row tiles around what the image / the block above need, conv0
//              (FIR output) one row more on either side, the block below what conv0's transposed conv reads (la_modconv3x3_up2_fwd_rows)
//              and what the image up-sampling reads.  Everything a consumer reads must be exact, so the tile rounding of one level is part
//              of the next level's need.
//   img_lo/hi  image rows a block has to deliver (kept where the large ToRGB kernel runs: la_torgb_small)
//   cone       where the GRADIENT of a conv output can be non-zero: the same recursion WITHOUT the tile rounding (a row that was computed
//              only because a tile had to be whole feeds nothing that is read, its gradient is an exact zero) -- need of conv1, conv0 one
//              row more, the block below what those conv0 rows read united with its image rows.  Inside the fwd rows by construction; set
//              for exactly the layers that have a forward window.  The backward launches round them to their own tiles, once.
//   fwd cols   top block only, where its conv1 has a row window: conv1 in the 32-column tiles that hold the image columns with a tile column
//              to spare on both sides (the gradient of conv1's input reaches one column beyond the image window: it must stay inside the
//              tiles), the FIR in front of it (conv0) one column more on either side.  The two flat launches of the top up-sampling layer
//              derive their columns from these in their builders (la_modconv.hip): the transposed conv the phase columns that FIR reads, the
//              stride-2 backward the columns where the gradient at res / 2 can be non-zero (it zero-fills the others of its rows).  That
//              cone must hold the image gradient one level down (ToRGB share of the fused seam): image columns start one inside the tiles
//              at least, so they reach column lo / 2 .. hi / 2 there, the cone (lo - 3) / 2 .. hi / 2 + 1.
static void plan_windows(SynthPlan& P, const LaWindow& img) {
    const int nblocks = P.pass.nblocks, nconv = P.pass.nconv, R = 4 << (nblocks - 1);
    if (img.row_hi <= 0) return;
    int img_lo = img.row_lo, img_hi = img.row_hi, up_lo = 0, up_hi = 0;      // needs of block k: image rows, rows read by block k + 1
    int gup_lo = 0, gup_hi = 0;                                               // (gradient cone: rows read by the NEEDED conv0 rows of block k + 1)
    for (int k = nblocks - 1, c1 = nconv - 1; k >= 1; --k, c1 -= 2) {
        const int res = 4 << k;
        if (res < 64) break;
        int lo = img_lo, hi = img_hi, glo = img_lo, ghi = img_hi;
        if (up_hi > 0) { lo = up_lo < lo ? up_lo : lo; hi = up_hi > hi ? up_hi : hi; }
        if (gup_hi > 0) { glo = gup_lo < glo ? gup_lo : glo; ghi = gup_hi > ghi ? gup_hi : ghi; }
        la_span_tiles(lo, hi, 4, res);
        if (lo <= 0 && hi >= res) break;                      // everything is needed from here down
        SynthPlan::Layer &L1 = P.conv[c1], &L0 = P.conv[c1 - 1];
        L1.fwd.row_lo = lo; L1.fwd.row_hi = hi;
        L1.cone_lo = glo; L1.cone_hi = ghi;
        if (!la_torgb_small((long)res * res)) { P.blk[k].img_lo = img_lo; P.blk[k].img_hi = img_hi; }
        la_span_grow(lo, hi, 1, 1, res);
        L0.fwd.row_lo = lo; L0.fwd.row_hi = hi;
        la_modconv3x3_up2_fwd_rows(res, lo, hi, &up_lo, &up_hi);
        la_span_grow(glo, ghi, 1, 1, res);
        L0.cone_lo = glo; L0.cone_hi = ghi;
        la_modconv3x3_up2_fwd_rows(res, glo, ghi, &gup_lo, &gup_hi);
        img_lo = (img_lo - 2) >> 1; if (img_lo < 0) img_lo = 0;
        img_hi = (img_hi >> 1) + 1; if (img_hi > res / 2) img_hi = res / 2;
    }
    LaWindow& c1w = P.conv[nconv - 1].fwd;
    if (c1w.row_hi <= 0 || img.col_hi <= 0 || R < 64) return;
    int lo = img.col_lo, hi = img.col_hi;
    la_span_tiles(lo, hi, 32, R);
    if (!(img.col_lo - 1 >= lo && img.col_hi + 1 <= hi && (lo > 0 || hi < R))) return;
    c1w.col_lo = lo; c1w.col_hi = hi;
    la_span_grow(lo, hi, 1, 1, R);
    P.conv[nconv - 2].fwd.col_lo = lo; P.conv[nconv - 2].fwd.col_hi = hi;
}

// The plan of a pass of `nblocks` blocks with the channel table, B samples, the contraction precision and the image window.  The development
// switches are read here and nowhere else, once per process.
static void plan_pass(int nblocks, const int* channels, int B, int precision, const LaWindow& img, bool rgb_per_block, SynthPlan& P) {
    static const bool zt_dense = la_dev_env("LA_NO_ZT_PITCH") != nullptr;      // dense interleaved scratch rows + the scalar FIR kernel
    static const bool no_fuse = la_dev_env("LA_NO_SEAM_FUSE") != nullptr, no_fuse2 = la_dev_env("LA_NO_SEAM2_FUSE") != nullptr;      // A/B of the fused seams on one box
    static const bool no_xs = la_dev_env("LA_NO_XS_HANDOFF") != nullptr;       // plane maxima + la_xscale_pmax at the consumer
    memset(&P, 0, sizeof(P));
    const int top = nblocks - 1;
    const bool b16 = precision != LA_PREC_F32, f16 = precision == LA_PREC_F16X2, xs_hand = f16 && !no_xs;
    // 16-bit modes: a conv0 seam runs in the epilogue of conv1's backward contraction (its saved output is that contraction's xin: no pass
    // of its own over y0 and the gradient), a conv1 seam incl. its ToRGB backward in the epilogue of the up layer's backward one block up
    const bool fuse0 = b16 && !no_fuse, fuse1 = b16 && !no_fuse2;
    // the cone needs the default path (fused seams, slot rows) and an image gradient that is zero outside the image window
    P.pass = {nblocks, 2 * nblocks - 1, B, precision, f16, xs_hand, zt_dense, xs_hand && fuse0 && fuse1};
    // row / column windows: 16-bit kernels with the column-planar scratch only
    if (b16 && !zt_dense) plan_windows(P, img);
    auto seam = [&](SynthPlan::Layer& L, bool fused, int fused_buf, int tiles, int slabs) {
        L.seam = fused ? SEAM_FUSED : SEAM_KERNEL;
        L.nseg = fused ? tiles : slabs;      // granularity of the layer's ddn / dweff / plane-maxima partials
        L.pmax_in = !f16 ? PMAX_NONE : fused ? fused_buf : PMAX_1;
        L.seam_pmax = (fused || !xs_hand) ? L.pmax_in : PMAX_NONE;      // (a seam kernel lowers the slot row instead where rows are handed on)
    };
    auto cone_tiles = [](const SynthPlan::Layer& of, int res, LaWindow& w) {      // the 4-row tiles around the gradient rows of a conv output
        w.row_lo = of.cone_lo; w.row_hi = of.cone_hi;
        la_span_tiles(w.row_lo, w.row_hi, 4, res);
    };
    bool pyramid_done = false;
    for (int k = top; k >= 0; --k) {
        const int res = 4 << k, slabs = la_seam_slabs((long)res * res), tiles1 = la_modconv_ds_tiles(res);
        SynthPlan::Block& Bk = P.blk[k];
        SynthPlan::Layer& L1 = P.conv[2 * k];
        // ToRGB inside the epilogue of the block's conv1 where one row tile of the halo kernel holds all its channels (the top blocks:
        // <= 128 channels at >= 64^2) -- conv1's output is then not streamed a second time; the skip image has to exist before conv1 runs
        Bk.fuse_rgb = la_modconv3x3_fwd_fuses_rgb(precision, B, channels[k], channels[k], res);
        Bk.skip_up = k > 0 && Bk.fuse_rgb ? SKIP_LAUNCH : SKIP_NONE;
        seam(L1, k < top && fuse1, PMAX_3, tiles1, slabs);
        L1.ntiles = tiles1;
        if (k == 0) break;
        SynthPlan::Layer& L0 = P.conv[2 * k - 1];
        seam(L0, fuse0, PMAX_2, tiles1, slabs);
        L0.ntiles = la_modconv_ds_tiles(res / 2);
        // image-gradient levels: a down-FIR per block until one launch makes every level below (la_image_grad_pyramid, from <= 256^2 inputs)
        Bk.down_fir = !pyramid_done;
        Bk.pyramid = Bk.down_fir && k >= 2 && res / 2 <= 256;
        pyramid_done |= Bk.pyramid != 0;
        // cone: conv1's backward contraction reads the tiles around the gradient rows of conv1's output (what the seam kernel or the block
        // above wrote into G0) and writes those of conv0's output into G1 -- top block: in the window's tile columns, the FIR adjoint reads
        // the others as zeros; the up layer's backward reads these and writes the tiles around the gradient rows of the block below's conv1 output
        if (!(P.pass.cone && L1.cone_hi > 0)) continue;
        L1.win = L0.win = 1;
        cone_tiles(L1, res, L1.rows.in);
        cone_tiles(L0, res, L1.rows.out);
        if (k == top) { L1.rows.out.col_lo = L1.fwd.col_lo; L1.rows.out.col_hi = L1.fwd.col_hi; }
        L0.rows.in = L1.rows.out;
        if (P.conv[2 * k - 2].cone_hi > 0) cone_tiles(P.conv[2 * k - 2], res / 2, L0.rows.out);
    }
    // Deferred ToRGBs: nothing reads the image of a block whose ToRGB is a kernel of its own before the next fused ToRGB does (its skip
    // image), so those blocks run no ToRGB launch of their own.  A run of them ends in front of the first fused block above it
    // (SKIP_CHAIN: two launches there make rgb_pre and the images of the whole run and that block's skip image, which takes over its
    // up-FIR launch; la_image_chain_forward makes skip images up to 256^2, a larger one keeps its launch behind the two) or, where no
    // block above fuses, at the end of the pass.
    for (int k = 1; k <= top && !rgb_per_block; ++k)
        if (P.blk[k].skip_up && !P.blk[k - 1].fuse_rgb && (4 << k) <= 256) P.blk[k].skip_up = SKIP_CHAIN;
}

// a layer's epilogue (SynthesisLayer.forward: lrelu, gain sqrt(2), conv_clamp) with the noise the last forward pass used ...
static LaLayerEpi layer_epi(const la_synth* h, const ConvLayer& L) {
    return LaLayerEpi{h->d_all + L.d_off, h->Dt, L.noise_used, L.noise_bstride, L.noise_strength, L.bias, LA_ACT_LRELU, 0.2f, sqrtf(2.f), h->clamp};
}
// ... and its contraction, forward or backward, in the arithmetic the pass was planned for
static LaModconv layer_conv(const la_synth* h, const ConvLayer& L, int B, bool backward) {
    return LaModconv{backward ? L.wb : L.wf, backward ? L.wqb : L.wqf, h->plan.pass.precision, h->s_all + L.s_off, h->S, B, L.cin, L.cout, L.res, h->cws, h->cws_bytes};
}
// the block's ToRGB layer writing its image to `img`
static LaRgbFuse layer_rgb(const la_synth* h, const RgbLayer& T, const float* skip, float* img) {
    return LaRgbFuse{h->imgc, T.weight, h->s_all + T.s_off, h->S, T.bias, skip, T.rgb_pre, img, h->clamp};
}

// column-planar intermediate of an up layer (la_modconv3x3_up2_fwd_ex): floats from the start of a row to its odd-column run
static inline int zt_xhalf(int res) { return (res / 2 + 1 + 3) & ~3; }
static int layout(la_synth* h, void* workspace, size_t cap, size_t* need) {
    LaCarver c{(char*)workspace, 0, cap};
    const size_t mb = h->maxB;
    size_t gmax = 0, ztmax = 0, skf = 0;
    for (int k = 0; k < h->nconv; ++k) {
        ConvLayer& L = h->conv[k];
        la_conv_weights_layout(c, L, true);
        const size_t hw = (size_t)L.res * L.res;
        L.y = c.take(mb * L.cout * hw);
        if (mb * L.cout * hw > gmax) gmax = mb * L.cout * hw;
        if (mb * L.cin * hw > gmax && !L.up) gmax = mb * L.cin * hw;
        if (L.up) {      // transposed-conv intermediate, column-planar rows (zt_xhalf)
            const size_t z = mb * L.cout * (size_t)(L.res + 1) * (size_t)(2 * zt_xhalf(L.res));
            if (z > ztmax) ztmax = z;
        }
        const int gin = L.up ? L.res / 2 : L.res;   // grid of the backward-data conv
        {
            const size_t sl0 = (size_t)la_seam_slabs((long)hw), t1 = (size_t)la_conv_tiles_per_sample(L.res, L.res);
            L.dsp = c.take(mb * L.cin * (size_t)la_conv_tiles_per_sample(gin, gin));
            L.ddnp = c.take(mb * L.cout * (sl0 > t1 ? sl0 : t1));
        }
        const size_t sk = la_modconv_workspace_bytes((int)mb, L.cin, L.cout, L.res, L.up);
        if (sk > skf) skf = sk;
    }
    for (int k = 0; k < h->nblocks; ++k) {
        RgbLayer& T = h->rgb[k];
        const size_t hw = (size_t)T.res * T.res;
        T.rgb_pre = c.take(mb * h->imgc * hw);
        T.img = c.take(mb * h->imgc * hw);
        T.g_img = c.take(mb * h->imgc * hw);
        {
            const size_t sl0 = (size_t)la_seam_slabs((long)hw), t1 = (size_t)la_conv_tiles_per_sample(T.res, T.res);
            T.dwep = c.take(mb * h->imgc * T.cin * (sl0 > t1 ? sl0 : t1));
        }
    }
    h->s_all = c.take(mb * h->S);
    h->ds_all = c.take(mb * h->S);
    h->d_all = c.take(mb * h->Dt);
    h->zT = c.take(ztmax);
    h->G0 = c.take(gmax);
    h->G1 = c.take(gmax);
    h->aff_part = c.take((size_t)la_affine_bwd_chunks(h->st) * mb * h->wdim);
    h->cws = c.take((skf + 3) / 4);
    h->cws_bytes = skf;
    // plane-maxima buffers, each [B][C][segments] of its largest producer: pmax the FIR epilogue of an up layer and the seam kernel, pmax2 /
    // pmax3 the fused seams of the up layers / of the conv1 layers (contraction tiles)
    auto largest = [&](auto per_layer) {
        size_t m = 0;
        for (int k = 0; k < h->nconv; ++k) { const size_t n = per_layer(h->conv[k]); if (n > m) m = n; }
        return m;
    };
    auto tiles_of = [&](const ConvLayer& L) { return mb * L.cout * (size_t)la_conv_tiles_per_sample(L.res, L.res); };
    h->pmax = c.take(mb * largest([](const ConvLayer& L) {
        const size_t a = (size_t)L.cout * (L.up ? la_fir4x4_segments(L.res, L.res) : 1), b2 = (size_t)L.cout * la_seam_slabs((long)L.res * L.res);
        return a > b2 ? a : b2;
    }));
    const size_t f2 = largest([&](const ConvLayer& L) { return L.up ? tiles_of(L) : 0; }), f3 = largest([&](const ConvLayer& L) { return L.up ? 0 : tiles_of(L); });
    h->pmax2 = c.take(f2 ? f2 : 16);
    h->pmax3 = c.take(f3 ? f3 : 16);
    h->xs_fwd = c.take((size_t)h->nconv * mb * LA_XS_FAN);
    h->xs_bwd = c.take((size_t)h->nconv * mb * LA_XS_FAN);
    h->xs_mult = c.take((size_t)h->nconv * mb + 16);
    *need = c.off;
    return LA_OK;
}

static int describe(la_synth* h, int R, int imgc, int wdim, const int* channels, int maxB) {
    LA_CHECK_ARG(R >= 4 && (R & (R - 1)) == 0 && R <= 4096, "synth: resolution must be a power of two >= 4");
    LA_CHECK_ARG(imgc >= 1 && imgc <= 4, "synth: img_channels must be 1..4");
    LA_CHECK_ARG(wdim >= 1 && maxB >= 1, "synth: bad w_dim / batch");
    memset(h, 0, sizeof(*h));
    h->R = R; h->imgc = imgc; h->wdim = wdim; h->maxB = maxB;
    int nb = 0;
    for (int r = 4; r <= R; r *= 2) ++nb;
    LA_CHECK_ARG(nb <= MAX_BLOCKS, "synth: too many blocks");
    h->nblocks = nb;
    int nconv = 0, widx = 0, S = 0, Dt = 0, nst = 0;
    for (int k = 0; k < nb; ++k) {
        const int res = 4 << k;
        const int co = channels[k];
        LA_CHECK_ARG(co >= 4 && co % 4 == 0, "synth: channel counts must be multiples of 4");
        h->channels[k] = co;
        if (k > 0) {
            ConvLayer& L = h->conv[nconv++];
            la_conv_weights_shape(L, channels[k - 1], co, 3); L.res = res; L.up = 1; L.widx = widx++;
        }
        ConvLayer& L1 = h->conv[nconv++];
        la_conv_weights_shape(L1, co, co, 3); L1.res = res; L1.up = 0; L1.widx = widx++;
        RgbLayer& T = h->rgb[k];
        T.cin = co; T.res = res; T.widx = widx;   // shares its w with the next block's conv0
    }
    h->nconv = nconv;
    h->num_ws = widx + 1;
    LA_CHECK_ARG(nconv + nb <= LA_MAX_STYLE_LAYERS, "synth: too many style layers");
    // style rows: conv layers then rgb layers
    for (int k = 0; k < nconv; ++k) {
        ConvLayer& L = h->conv[k];
        L.s_off = S; L.d_off = Dt; L.style_idx = nst;
        h->st.row_start[nst] = S; h->st.widx[nst] = L.widx; h->st.post_gain[nst] = 1.f;
        h->dt.row_start[k] = Dt; h->dt.cin[k] = L.cin; h->dt.s_off[k] = S;
        S += L.cin; Dt += L.cout; ++nst;
    }
    for (int k = 0; k < nb; ++k) {
        RgbLayer& T = h->rgb[k];
        T.s_off = S; T.style_idx = nst;
        h->st.row_start[nst] = S; h->st.widx[nst] = T.widx; h->st.post_gain[nst] = 1.f / sqrtf((float)T.cin);
        S += T.cin; ++nst;
    }
    h->st.nlayers = nst; h->st.total_rows = S; h->st.row_start[nst] = S;
    h->dt.nlayers = nconv; h->dt.total_rows = Dt; h->dt.row_start[nconv] = Dt;
    h->S = S; h->Dt = Dt;
    return LA_OK;
}

extern "C" int la_synth_num_ws(int img_resolution) {
    int nb = 0;
    for (int r = 4; r <= img_resolution; r *= 2) ++nb;
    return 2 * nb;   // 2*log2(R) - 2
}

extern "C" int la_synth_num_params(int img_resolution) {
    int nb = 0;
    for (int r = 4; r <= img_resolution; r *= 2) ++nb;
    return 1 + 5 + 4 + (nb - 1) * 14;
}

extern "C" size_t la_synth_workspace_bytes(int img_resolution, int img_channels, int w_dim, const int* channels,
                                           int max_batch) {
    return la_measure_workspace<la_synth>([&](la_synth* h) {
        size_t need = 0;
        if (describe(h, img_resolution, img_channels, w_dim, channels, max_batch) == LA_OK) layout(h, nullptr, 0, &need);
        return need;
    });
}

extern "C" int la_synth_create(int img_resolution, int img_channels, int w_dim, const int* channels, float conv_clamp,
                               const float* const* params, int nparams, const float* noise_strength, int nlayers,
                               const float* fir_host, int fir_h, int fir_w, int max_batch, void* workspace,
                               size_t workspace_bytes, hipStream_t stream, la_synth** out) {
    LA_CHECK_ARG(params && noise_strength && fir_host && workspace && out, "synth_create: null pointer");
    LA_CHECK_ARG(fir_h == 4 && fir_w == 4, "synth_create: resample filter must be 4x4 (setup_filter([1,3,3,1]))");
    auto own = la_host_handle<la_synth>();
    la_synth* h = own.get();
    LA_CHECK_ARG(h, "synth_create: out of host memory");
    int rc = describe(h, img_resolution, img_channels, w_dim, channels, max_batch);
    if (rc) return rc;
    LA_CHECK_ARG(nparams == la_synth_num_params(img_resolution) && nlayers == h->nconv, "synth_create: parameter list length mismatch");
    for (int i = 0; i < nparams; ++i) LA_CHECK_ARG(params[i], "synth_create: null parameter tensor");
    size_t need = 0;
    layout(h, workspace, workspace_bytes, &need);
    LA_CHECK_WORKSPACE(workspace_bytes, need, "synth_create: workspace too small");
    h->clamp = conv_clamp;
    // every buffer starts as zeros: a forward pass restricted to a row window (la_synth_set_row_window) leaves the other rows of its saved
    // activations as they were, and the backward pass multiplies them with gradients that are exactly zero there -- they must be finite
    if (hipMemsetAsync(workspace, 0, need, stream) != hipSuccess) { la_set_error("synth_create: clearing the workspace failed"); return LA_ERR_HIP; }
    memcpy(h->fir, fir_host, sizeof(float) * 16);
    h->up_mult = la_modconv_up2_bwd_xs_mult(h->fir);
    int p = 0, ci = 0;
    for (int k = 0; k < h->nblocks; ++k) {
        if (k == 0) h->cst = params[p++];
        const int nl = (k == 0) ? 1 : 2;
        for (int q = 0; q < nl; ++q) {
            ConvLayer& L = h->conv[ci];
            L.affine_w = params[p++]; L.affine_b = params[p++]; L.w = params[p++]; L.bias = params[p++];
            L.noise_const = params[p++];
            L.noise_strength = noise_strength[ci];
            h->st.aw[L.style_idx] = L.affine_w; h->st.ab[L.style_idx] = L.affine_b;
            h->dt.wsq[ci] = L.wsq;
            if ((rc = la_conv_weights_pack(L, 1.f, stream))) return rc;
            ++ci;
        }
        RgbLayer& T = h->rgb[k];
        T.affine_w = params[p++]; T.affine_b = params[p++]; T.weight = params[p++]; T.bias = params[p++];
        h->st.aw[T.style_idx] = T.affine_w; h->st.ab[T.style_idx] = T.affine_b;
    }
    *out = own.release();
    return LA_OK;
}

extern "C" void la_synth_destroy(la_synth* h) { free(h); }

// contraction arithmetic of every modulated conv of the engine: 0 fp32 MFMA, 1 split-bf16 x3 (fp32-class), 2 split-bf16 x2
extern "C" int la_synth_set_precision(la_synth* h, int precision) {
    LA_CHECK_ARG(h && precision >= 0 && precision <= 3, "synth_set_precision: precision must be 0..3");
    if (precision != h->precision) ++h->settings_gen;
    h->precision = precision;
    return LA_OK;
}
int la_synth_settings_gen(const la_synth* h) { return h->settings_gen; }
extern "C" int la_synth_get_precision(const la_synth* h) { return h ? h->precision : -1; }
// Kept for ABI compatibility (rounds 1-3 selected between an a-priori bound and data maxima for the fp16 operand scale of the forward
// contractions): since round 4 every forward scale is derived from the data of the pass by the kernel that produces the tensor
// (la_xscale_bound_block, la_style.hip) -- there is nothing to select, the launch sequence does not depend on this call.
extern "C" int la_synth_set_operand_scale(la_synth* h, int from_data) {
    LA_CHECK_ARG(h && (from_data == 0 || from_data == 1), "synth_set_operand_scale: 0 or 1");
    return LA_OK;
}

// Where the ToRGB layers that are kernels of their own run in the following forward passes: 0 (default) deferred -- one launch for rgb_pre of
// all of them and one for their images in front of the first fused ToRGB / at the end of the pass (plan_pass) --, 1 a launch behind
// every block's conv1 (la_torgb_forward, and an up-FIR launch for every skip image).  Same buffers, same bits: the per-block schedule is
// what tests/test_hip_image_chain.py holds the deferred one against.
extern "C" int la_synth_set_torgb_schedule(la_synth* h, int per_block) {
    LA_CHECK_ARG(h && (per_block == 0 || per_block == 1), "synth_set_torgb_schedule: 0 or 1");
    if (per_block != h->rgb_per_block) ++h->settings_gen;
    h->rgb_per_block = per_block;
    return LA_OK;
}

// Row window of the IMAGE that the following forward passes must deliver (rows [row_lo, row_hi) of the img_resolution rows; 0, 0 = all):
// the latent-optimisation loop whose criteria read a centre crop only (la_latent_opt.hip).  The 16-bit forward kernels of the blocks at
// >= 64^2 then compute only the rows that window depends on (3x3 taps, FIR taps and the up-sampling geometry followed down the
// blocks, tile granularities included: everything that IS computed is exact); the rest of every buffer keeps older contents.  The
// backward pass is unchanged: image-gradient rows outside the window must be zero (they are for a criterion that reads the window only).
extern "C" int la_synth_set_row_window(la_synth* h, int row_lo, int row_hi) {
    LA_CHECK_ARG(h && row_lo >= 0 && (row_hi == 0 ? row_lo == 0 : (row_hi > row_lo && row_hi <= h->R)), "synth_set_row_window: bad window");
    h->win.row_lo = row_lo; h->win.row_hi = row_hi;
    return LA_OK;
}

// Column window of the image on top of the row window (0, 0 = all columns).  Only the TOP block follows it -- its conv1 (forward: the 32-column
// tiles that hold the window; backward: the same tiles, the gradient of its input is non-zero one column further at most), the FIR that
// feeds it, the FIR adjoint behind it (which reads the other columns as zeros) and the two contractions of its up-sampling layer (forward: the
// phase columns the FIR reads; backward: the columns of the gradient at half the resolution that can be non-zero); every other kernel
// computes whole rows.
extern "C" int la_synth_set_col_window(la_synth* h, int col_lo, int col_hi) {
    LA_CHECK_ARG(h && col_lo >= 0 && (col_hi == 0 ? col_lo == 0 : (col_hi > col_lo && col_hi <= h->R)), "synth_set_col_window: bad window");
    h->win.col_lo = col_lo; h->win.col_hi = col_hi;
    return LA_OK;
}

// Host only, no launch: the window of the gradient of conv output `conv_index` (0 .. 2 log2(R) - 2, the engine's layer order) that a backward pass
// computes for the image window rows [row_lo, row_hi) x columns [col_lo, col_hi) (0, 0 = all) of a 16-bit engine at img_resolution --
// window[0..1]: the rows in which that gradient can be non-zero (the cone of the image window; the launch that writes them rounds
// them outward to its 4-row tiles, once), window[2..3]: the tile columns the launch writes; 0, 0 on an axis = all of it.
extern "C" int la_synth_plan_bwd_window(int img_resolution, int row_lo, int row_hi, int col_lo, int col_hi, int conv_index, int* window) {
    const int R = img_resolution;
    LA_CHECK_ARG(R >= 4 && (R & (R - 1)) == 0 && R <= 4096 && window, "synth_plan_bwd_window: resolution must be a power of two >= 4");
    LA_CHECK_ARG(row_lo >= 0 && (row_hi == 0 ? row_lo == 0 : (row_hi > row_lo && row_hi <= R)), "synth_plan_bwd_window: bad row window");
    LA_CHECK_ARG(col_lo >= 0 && (col_hi == 0 ? col_lo == 0 : (col_hi > col_lo && col_hi <= R)), "synth_plan_bwd_window: bad column window");
    SynthPlan P; memset(&P, 0, sizeof(P));
    P.pass.nblocks = la_synth_num_ws(R) / 2; P.pass.nconv = 2 * P.pass.nblocks - 1;
    LA_CHECK_ARG(conv_index >= 0 && conv_index < P.pass.nconv, "synth_plan_bwd_window: no such conv layer");
    plan_windows(P, LaWindow{row_lo, row_hi, col_lo, col_hi});
    const LaWindow none = {}, &c1w = conv_index == P.pass.nconv - 2 ? P.conv[conv_index + 1].fwd : none;      // (written by the top conv1's backward)
    window[0] = P.conv[conv_index].cone_lo; window[1] = P.conv[conv_index].cone_hi; window[2] = c1w.col_lo; window[3] = c1w.col_hi;
    return LA_OK;
}
// ... and what the LAST forward pass of a handle planned for its backward pass (rows only)
extern "C" int la_synth_bwd_rows(const la_synth* h, int conv_index, int* row_lo, int* row_hi) {
    LA_CHECK_ARG(h && row_lo && row_hi && conv_index >= 0 && conv_index < h->nconv, "synth_bwd_rows: no such conv layer");
    *row_lo = h->plan.conv[conv_index].cone_lo; *row_hi = h->plan.conv[conv_index].cone_hi;
    return LA_OK;
}
// Host only, no launch, no handle: the whole plan of a pass as info[LA_SYNTH_PLAN_NINFO] (include/latentaug_hip.h)
extern "C" int la_synth_plan_query(int img_resolution, int img_channels, const int* channels, int B, int precision, int row_lo, int row_hi, int col_lo,
                                   int col_hi, long* info) {
    const int R = img_resolution;
    LA_CHECK_ARG(R >= 4 && (R & (R - 1)) == 0 && R <= 4096 && channels && info, "synth_plan_query: resolution must be a power of two >= 4");
    LA_CHECK_ARG(img_channels >= 1 && img_channels <= 4 && B >= 1 && precision >= 0 && precision <= 3, "synth_plan_query: bad img_channels / batch / precision");
    LA_CHECK_ARG(row_lo >= 0 && (row_hi == 0 ? row_lo == 0 : (row_hi > row_lo && row_hi <= R)), "synth_plan_query: bad row window");
    LA_CHECK_ARG(col_lo >= 0 && (col_hi == 0 ? col_lo == 0 : (col_hi > col_lo && col_hi <= R)), "synth_plan_query: bad column window");
    const int nblocks = la_synth_num_ws(R) / 2;
    for (int k = 0; k < nblocks; ++k) LA_CHECK_ARG(channels[k] >= 4 && channels[k] % 4 == 0, "synth_plan_query: channel counts must be multiples of 4");
    SynthPlan P;
    plan_pass(nblocks, channels, B, precision, LaWindow{row_lo, row_hi, col_lo, col_hi}, false, P);
    const int* src = reinterpret_cast<const int*>(&P);      // (ints throughout, in the order of the constants: the static_assert above)
    for (int i = 0; i < LA_SYNTH_PLAN_NINFO; ++i) info[i] = src[i];
    return LA_OK;
}

#ifdef LA_DEV
// development build: the transposed-conv intermediate of the LAST up-sampling layer that ran (column-planar rows; scripts/exp_overlap_*.py)
extern "C" const float* la_synth_dev_zt(const la_synth* h) { return h ? h->zT : nullptr; }
#endif
extern "C" const float* la_synth_image(const la_synth* h) { return h ? h->final_img : nullptr; }
extern "C" const float* la_synth_block_image(const la_synth* h, int k) { return (h && k >= 0 && k < h->nblocks) ? h->rgb[k].img : nullptr; }
extern "C" const float* la_synth_layer_output(const la_synth* h, int k) { return (h && k >= 0 && k < h->nconv) ? h->conv[k].y : nullptr; }
extern "C" const float* la_synth_styles(const la_synth* h) { return h ? h->s_all : nullptr; }
extern "C" const float* la_synth_style_grads(const la_synth* h) { return h ? h->ds_all : nullptr; }
extern "C" int la_synth_style_rows(const la_synth* h) { return h ? h->S : 0; }

// The deferred ToRGBs of blocks k0 .. k1 (plan_pass) from their saved conv1 outputs, two launches: rgb_pre of every level, then the images
// level by level (block k1's into top_img where given) and, where a fused block follows, its skip image.  Windowed blocks: the rows the
// plan asks of them, as the per-block launch computed.
static int deferred_images(la_synth* h, const SynthPlan& P, int k0, int k1, int B, float* skip, float* top_img, hipStream_t stream) {
    LaTorgbLevels lv; memset(&lv, 0, sizeof(lv));
    LaImageChain ch; memset(&ch, 0, sizeof(ch));
    lv.imgc = ch.imgc = h->imgc; lv.s_stride = h->S; ch.clamp = h->clamp;
    ch.base = k0 > 0 ? h->rgb[k0 - 1].img : nullptr; ch.skip = skip;
    for (int k = k0; k <= k1; ++k) {
        const RgbLayer& T = h->rgb[k];
        const int lo = P.blk[k].img_lo, hi = P.blk[k].img_hi;
        lv.lv[lv.n++] = {h->conv[2 * k].y, T.cin, T.res, T.res, T.weight, h->s_all + T.s_off, T.bias, T.rgb_pre, lo, hi};
        ch.lv[ch.n++] = {T.rgb_pre, (k == k1 && top_img) ? top_img : T.img, T.res, T.res, lo, hi};
    }
    int rc = la_torgb_forward_levels(lv, B, stream);
    return rc ? rc : la_image_chain_forward(ch, B, h->fir, stream);
}

extern "C" int la_synth_forward(la_synth* h, const float* ws, long ws_bstride, long ws_lstride, int B, int noise_mode,
                                const float* const* noises, float* img_out, hipStream_t stream) {
    LA_CHECK_ARG(h && ws, "synth_forward: null pointer");
    LA_CHECK_ARG(B >= 1 && B <= h->maxB, "synth_forward: batch exceeds the max_batch the workspace was sized for");
    LA_CHECK_ARG(noise_mode >= 0 && noise_mode <= 2, "synth_forward: noise_mode must be 0 (none), 1 (const), 2 (explicit)");
    LA_CHECK_ARG(noise_mode != 2 || noises, "synth_forward: explicit noise requested but no noise tensors given");
    for (int ci = 0; ci < h->nconv && noise_mode == 2; ++ci) LA_CHECK_ARG(h->conv[ci].noise_strength == 0.f || noises[ci], "synth_forward: missing noise tensor");
    plan_pass(h->nblocks, h->channels, B, h->precision, h->win, h->rgb_per_block != 0, h->plan);
    const SynthPlan& P = h->plan;
    int rc;
    if ((rc = la_affine_forward(h->st, ws, ws_bstride, ws_lstride, B, h->wdim, h->s_all, stream))) return rc;
    // fp16 operand scales: the slot rows of every layer start the pass at LA_XS_INIT (in the demod launch); the kernel that PRODUCES a
    // layer's input lowers that layer's row (forward: xs_fwd, la_xs_lower with max|style| of the consuming layer; backward: xs_bwd)
    const LaXscaleBounds xb = {h->cst, h->channels[0] * 16, h->xs_fwd, h->xs_mult, h->xs_bwd};
    if ((rc = la_demod_forward(h->dt, h->s_all, h->S, B, h->d_all, stream, P.pass.f16 ? &xb : nullptr))) return rc;
    auto fwd_row = [&](int conv_index) { return (P.pass.f16 && conv_index < h->nconv) ? h->xs_fwd + (long)conv_index * B * LA_XS_FAN : nullptr; };
    auto fwd_mult = [&](int conv_index) { return (P.pass.f16 && conv_index < h->nconv) ? h->xs_mult + (long)conv_index * B : nullptr; };
    int ci = 0, pending = -1;      // pending: the first block whose deferred ToRGB has not run yet
    const float* x = h->cst;
    long x_bstride = 0;
    for (int k = 0; k < h->nblocks; ++k) {
        const int res = 4 << k;
        RgbLayer& T = h->rgb[k];
        float* const rgb_dst = (k == h->nblocks - 1 && img_out) ? img_out : T.img;
        const float* skip = nullptr;
        if (P.blk[k].fuse_rgb && pending >= 0) {      // the deferred blocks below: rgb_pre, images and (SKIP_CHAIN) this block's skip image
            if ((rc = deferred_images(h, P, pending, k - 1, B, P.blk[k].skip_up == SKIP_CHAIN ? T.g_img : nullptr, nullptr, stream))) return rc;
            pending = -1;
        }
        if (P.blk[k].skip_up == SKIP_CHAIN) skip = T.g_img;
        else if (P.blk[k].skip_up) {
            if ((rc = la_upfirdn2d_ex(h->rgb[k - 1].img, T.g_img, B, h->imgc, res / 2, res / 2, h->fir, la_fir_up2(), stream))) return rc;
            skip = T.g_img;
        }
        for (int q = k == 0; q < 2; ++q, ++ci) {      // conv0 (up-sampling; none in the first block), conv1
            ConvLayer& L = h->conv[ci];
            L.noise_used = nullptr; L.noise_bstride = 0;
            if (L.noise_strength != 0.f) {
                if (noise_mode == 1) L.noise_used = L.noise_const;
                else if (noise_mode == 2) { L.noise_used = noises[ci]; L.noise_bstride = (long)res * res; }
            }
            const LaRgbFuse rf = layer_rgb(h, T, skip, rgb_dst);
            LaModconvFwdOpts o;
            o.xscale = fwd_row(ci); o.xs_out = fwd_row(ci + 1); o.xs_mult = fwd_mult(ci + 1);
            o.win = P.conv[ci].fwd;
            if (!L.up) {
                if (P.blk[k].fuse_rgb) o.rgb = &rf;
                rc = la_modconv3x3_fwd_ex(x, x_bstride, layer_conv(h, L, B, false), layer_epi(h, L), L.y, stream, o);
            } else {
                if (!P.pass.zt_dense) { o.scratch_pitch = 2 * zt_xhalf(res); o.scratch_xhalf = zt_xhalf(res); }
                rc = la_modconv3x3_up2_fwd_ex(x, x_bstride, layer_conv(h, L, B, false), layer_epi(h, L), h->fir, h->zT, L.y, stream, o);
            }
            if (rc) return rc;
            x = L.y; x_bstride = (long)L.cout * res * res;
        }
        // img = upsample2d(img_prev, f) + torgb(x): up 2, pad (2,1,2,1), gain 4 (upfirdn2d.py:342-348) -- the up-sampled image of the block
        // below is computed inside the ToRGB kernel (la_up2_quad); a windowed block: only the image rows somebody reads.  Deferred unless the
        // handle asks for a launch per block: the block joins the run that deferred_images makes in front of the next fused block / at the end
        if (!P.blk[k].fuse_rgb && !h->rgb_per_block) { if (pending < 0) pending = k; }
        else if (!P.blk[k].fuse_rgb && (rc = la_torgb_forward(x, layer_rgb(h, T, nullptr, rgb_dst), B, T.cin, res, res, stream, nullptr, P.blk[k].img_lo, P.blk[k].img_hi,
                                                              k > 0 ? h->rgb[k - 1].img : nullptr, h->fir)))
            return rc;
        if (k == h->nblocks - 1) h->final_img = rgb_dst;
    }
    if (pending >= 0 && (rc = deferred_images(h, P, pending, h->nblocks - 1, B, nullptr, h->final_img, stream))) return rc;
    return LA_OK;
}

// ---- backward pass: the parts of one block, each a function of (handle, plan, block, B, stream); la_synth_backward orders them by the plan.
// Buffers: G0 holds the gradient of a block's conv1 output, G1 that of its conv0 output; every layer leaves its style-gradient partials in
// buffers of its own until the finish.  fp16 operand scales: the kernels whose epilogues produce a contraction's input (direct contraction
// kernels, split-K finish pass, seam kernel) lower the consumer's slot row themselves (la_xs_lower; la_synth_forward reset the rows) where
// the plan hands rows on; else they leave plane maxima for la_xscale_pmax at the consumer.
static float* pmax_buf(const la_synth* h, int which) { return which == PMAX_1 ? h->pmax : which == PMAX_2 ? h->pmax2 : which == PMAX_3 ? h->pmax3 : nullptr; }
static float* bwd_slot(const la_synth* h, int ci) { return h->plan.pass.xs_hand ? h->xs_bwd + (long)ci * h->plan.pass.B * LA_XS_FAN : nullptr; }
static const float* image_grad(const la_synth* h, int k) { return k == h->nblocks - 1 ? h->g_top : h->rgb[k].g_img; }
// what the seam of conv layer ci's output needs wherever it runs (LaSeamArgs / LaSeamFuse): the layer's epilogue, its partials, the slot row
// of the backward contraction that follows (xs_mult: 1, an up layer's la_modconv_up2_bwd_xs_mult)
template <class S>
static void seam_common(const la_synth* h, S& s, int ci) {
    memset(&s, 0, sizeof(s));
    la_seam_set_epi(s, layer_epi(h, h->conv[ci]));
    s.ddn_part = h->conv[ci].ddnp;
    if (h->plan.pass.xs_hand) { s.xs_out = bwd_slot(h, ci); s.xs_mult = h->conv[ci].up ? h->up_mult : 1.f; }
}
// a seam kernel's launch: conv layer ci's saved output, gz = (gx_next +) its ToRGB's share, through the activation backward
static LaSeamArgs seam_kernel(const la_synth* h, int ci, const float* gx_next, float* gz) {
    const ConvLayer& L = h->conv[ci];
    LaSeamArgs s; seam_common(h, s, ci);
    s.y = L.y; s.gx_next = gx_next; s.gz = gz; s.HW = (long)L.res * L.res; s.C = L.cout;
    s.pmax_out = pmax_buf(h, h->plan.conv[ci].seam_pmax);
    return s;
}
static LaModconvBwdOpts bwd_opts(const la_synth* h, int ci, const LaSeamFuse* seam) {
    const SynthPlan::Layer& pl = h->plan.conv[ci];
    LaModconvBwdOpts o;
    o.in_pmax = pmax_buf(h, pl.pmax_in); o.in_nseg = pl.nseg; o.seam = seam; o.xscale = bwd_slot(h, ci); o.rows = pl.win ? &pl.rows : nullptr;
    return o;
}

// conv1 seam as a kernel (top block, or where it was not fused above): ToRGB backward + activation backward at conv1's output
static int bwd_conv1_seam(la_synth* h, const SynthPlan& P, int k, int B, hipStream_t stream) {
    const RgbLayer& T = h->rgb[k];
    const SynthPlan::Layer& pl = P.conv[2 * k];
    LaSeamArgs s = seam_kernel(h, 2 * k, k == h->nblocks - 1 ? nullptr : h->G0, h->G0);
    s.g_img = image_grad(h, k); s.rgb_pre = T.rgb_pre; s.rgb_clamp = h->clamp; s.wrgb = T.weight;
    s.s_rgb = h->s_all + T.s_off; s.s_stride = h->S; s.dweff_part = T.dwep;
    if (pl.win) { s.p_lo = (long)pl.rows.in.row_lo * T.res; s.p_hi = (long)pl.rows.in.row_hi * T.res; }
    return la_seam_backward(s, B, h->imgc, stream);
}
// conv1 backward-data (+ style-gradient partials); where the plan fuses conv0's seam, this contraction's epilogue applies it (conv0's saved
// output is its xin): its demod-gradient partials and plane maxima come out per pixel tile
static int bwd_conv1_data(la_synth* h, const SynthPlan& P, int k, int B, hipStream_t stream) {
    const ConvLayer& L1 = h->conv[2 * k];
    LaSeamFuse sf;
    const bool fused = k > 0 && P.conv[2 * k - 1].seam == SEAM_FUSED;
    if (fused) { seam_common(h, sf, 2 * k - 1); sf.pmax = pmax_buf(h, P.conv[2 * k - 1].seam_pmax); }
    return la_modconv3x3_bwd_ex(h->G0, layer_conv(h, L1, B, true), k == 0 ? h->cst : h->conv[2 * k - 1].y, k == 0 ? 0 : (long)L1.cin * L1.res * L1.res, h->G1,
                                L1.dsp, stream, bwd_opts(h, 2 * k, fused ? &sf : nullptr));
}
// conv0 seam as a kernel: activation backward at the up-sampling layer's output, in place in G1
static int bwd_conv0_seam(la_synth* h, const SynthPlan&, int k, int B, hipStream_t stream) {
    return la_seam_backward(seam_kernel(h, 2 * k - 1, h->G1, h->G1), B, 0, stream);
}
// image gradient one level down: adjoint of upsample2d = FIR (flipped) + decimate 2, pad (1,1,1,1), gain 4; with the pyramid every level
// below in ONE more launch (the levels depend on the image gradient only)
static int bwd_image_grad(la_synth* h, const SynthPlan& P, int k, int B, hipStream_t stream) {
    const int res = 4 << k;
    int rc = la_upfirdn2d_ex(image_grad(h, k), h->rgb[k - 1].g_img, B, h->imgc, res, res, h->fir, la_fir_down2_adjoint(), stream);
    if (rc || !P.blk[k].pyramid) return rc;
    float* outs[MAX_BLOCKS];
    for (int q = k - 2; q >= 0; --q) outs[k - 2 - q] = h->rgb[q].g_img;
    return la_image_grad_pyramid(h->rgb[k - 1].g_img, outs, k - 1, B * h->imgc, res / 2, h->fir, stream);
}
// up layer's backward-data: FIR adjoint -> stride-2 backward-data; where the plan fuses it, the epilogue applies the conv1 seam of the block
// BELOW (its saved output is this contraction's xin), incl. its ToRGB backward
static int bwd_up_data(la_synth* h, const SynthPlan& P, int k, int B, hipStream_t stream) {
    const ConvLayer &L0 = h->conv[2 * k - 1], &Lb = h->conv[2 * k - 2];
    const RgbLayer& Tb = h->rgb[k - 1];
    LaSeamFuse sf;
    const bool fused = P.conv[2 * k - 2].seam == SEAM_FUSED;
    if (fused) {
        seam_common(h, sf, 2 * k - 2);
        sf.pmax = pmax_buf(h, P.conv[2 * k - 2].seam_pmax);
        sf.imgc = h->imgc; sf.g_img = Tb.g_img; sf.rgb_pre = Tb.rgb_pre; sf.rgb_clamp = h->clamp;
        sf.wrgb = Tb.weight; sf.s_rgb = h->s_all + Tb.s_off; sf.s_rgb_stride = h->S; sf.dweff_part = Tb.dwep;
    }
    return la_modconv3x3_up2_bwd_ex(h->G1, layer_conv(h, L0, B, true), Lb.y, (long)L0.cin * Lb.res * Lb.res, h->fir, h->zT, h->G0, L0.dsp, stream,
                                    bwd_opts(h, 2 * k - 1, fused ? &sf : nullptr));
}
// the style finish: ONE pass (3 launches) turns the partials of every layer into ds_all, segment counts from the plan
static int bwd_style_finish(la_synth* h, const SynthPlan& P, int, int B, hipStream_t stream) {
    LaStyleFinish fin; memset(&fin, 0, sizeof(fin));
    fin.imgc = h->imgc; fin.d_stride = h->Dt; fin.s_stride = h->S; fin.ds_stride = h->S;
    for (int k = h->nblocks - 1; k >= 0; --k) {
        const RgbLayer& T = h->rgb[k];
        LaStyleFinish::Rgb& r = fin.rgb[fin.nrgb++];
        r.dweff_part = T.dwep; r.wrgb = T.weight; r.ds_out = h->ds_all + T.s_off; r.nslabs = P.conv[2 * k].nseg; r.C = T.cin;
        for (int ci = 2 * k; ci >= 2 * k - 1 && ci >= 0; --ci) {
            const ConvLayer& L = h->conv[ci];
            LaStyleFinish::Conv& c = fin.conv[fin.nconv++];
            c.ds_part = L.dsp; c.ddn_part = L.ddnp; c.d = h->d_all + L.d_off; c.s = h->s_all + L.s_off; c.wsq = L.wsq;
            c.ds_out = h->ds_all + L.s_off; c.ntiles = P.conv[ci].ntiles; c.nslabs = P.conv[ci].nseg; c.cin = L.cin; c.cout = L.cout;
        }
    }
    return la_style_backward_all(fin, B, stream);
}

// noise gradient of conv layer ci from the gz its seam (a kernel, or the epilogue of the contraction above) has just left in `gz`: what is
// stored there carries the demodulation coefficient, gn[b][p] = strength * sum_c gz[b][c][p] / d[b][c] (la_noise.hip).  A launch of its
// own between the seam and the layer's backward contraction, which reads the same buffer; a layer without noise gets zeros.
static int bwd_noise_grad(la_synth* h, int ci, const float* gz, float* const* gnoises, int B, hipStream_t stream) {
    if (!gnoises || !gnoises[ci]) return LA_OK;
    const ConvLayer& L = h->conv[ci];
    const long HW = (long)L.res * L.res;
    if (L.noise_strength == 0.f) {
        LA_HIP(hipMemsetAsync(gnoises[ci], 0, (size_t)B * HW * sizeof(float), stream));
        return LA_OK;
    }
    return la_noise_grad_f32(gz, h->d_all + L.d_off, h->Dt, B, L.cout, HW, L.noise_strength, gnoises[ci], stream);
}

static int synth_backward(la_synth* h, const float* g_img, float* dws, float* const* gnoises, hipStream_t stream) {
    const SynthPlan& P = h->plan;
    const int B = P.pass.B;
    h->g_top = g_img;
    int rc;
    for (int k = h->nblocks - 1; k >= 0; --k) {
        if (P.conv[2 * k].seam == SEAM_KERNEL && (rc = bwd_conv1_seam(h, P, k, B, stream))) return rc;
        if ((rc = bwd_noise_grad(h, 2 * k, h->G0, gnoises, B, stream))) return rc;
        if ((rc = bwd_conv1_data(h, P, k, B, stream))) return rc;
        if (k == 0) break;
        if (P.conv[2 * k - 1].seam == SEAM_KERNEL && (rc = bwd_conv0_seam(h, P, k, B, stream))) return rc;
        if ((rc = bwd_noise_grad(h, 2 * k - 1, h->G1, gnoises, B, stream))) return rc;
        // (before the up layer's backward contraction: its epilogue may apply the block below's ToRGB backward)
        if (P.blk[k].down_fir && (rc = bwd_image_grad(h, P, k, B, stream))) return rc;
        if ((rc = bwd_up_data(h, P, k, B, stream))) return rc;
    }
    if ((rc = bwd_style_finish(h, P, 0, B, stream))) return rc;
    return la_affine_backward(h->st, h->ds_all, B, h->wdim, dws, h->num_ws, h->aff_part, stream);
}

extern "C" int la_synth_backward(la_synth* h, const float* g_img, float* dws, hipStream_t stream) {
    LA_CHECK_ARG(h && g_img && dws, "synth_backward: null pointer");
    LA_CHECK_ARG(h->plan.pass.B >= 1, "synth_backward: no forward pass to differentiate");
    return synth_backward(h, g_img, dws, nullptr, stream);
}

extern "C" int la_synth_backward_noise(la_synth* h, const float* g_img, float* dws, float* const* gnoises, hipStream_t stream) {
    LA_CHECK_ARG(h && g_img && dws, "synth_backward_noise: null pointer");
    LA_CHECK_ARG(h->plan.pass.B >= 1, "synth_backward_noise: no forward pass to differentiate");
    // a windowed pass leaves rows of the gradient buffers stale: the channel reduction reads whole planes
    bool windowed = h->win.row_hi > 0 || h->win.col_hi > 0;
    for (int ci = 0; ci < h->nconv; ++ci) windowed = windowed || h->plan.conv[ci].fwd.row_hi > 0 || h->plan.conv[ci].fwd.col_hi > 0 || h->plan.conv[ci].win;
    LA_CHECK_ARG(!gnoises || !windowed, "synth_backward_noise: noise gradients need whole planes; clear the row / column window (and run the forward pass again)");
    return synth_backward(h, g_img, dws, gnoises, stream);
}
