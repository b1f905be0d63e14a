// The latent-optimisation loop: LatentAug.forward (augments/utils/util_latent_aug.py:207-310) as one host-driven
// launch sequence with no host<->device synchronisation inside the loop (the reference syncs 5x per step through
// `.item()`, :234-271).  W-space optimisation: ws = w repeated num_ws times (:226, :493-494); a W+ handle (la_latent_opt_create_ex,
// latent_space 1) optimises one row per slot instead (la_wplus.hip).
#include "la_common.h"

#include <string.h>

#include "la_conv.h"
#include "la_criteria.h"
#include "la_feat.h"

#define LA_TEV 7      // step start | after synthesis | after latent | after pix | after disc | after lpips | step end
struct LaGraphPart { hipGraph_t graph; hipGraphExec_t exec; };
enum { LA_PART_A, LA_PART_P, LA_PART_D, LA_PART_Z };      // the parts of a step (run_step)

struct la_latent_opt {
    la_synth* g; la_disc* d;
    la_opt_config cfg;
    int R, imgc, wdim, num_ws, maxB;
    int wplus;              // latent space: 0 W (w_opt [B][w_dim], broadcast to the slots), 1 W+ (w_opt [B][num_ws][w_dim], la_wplus.hip)
    const float* bankW; long Mw;
    const float* bankX; long Mx;     // [imgc][Mx][cc*cc]
    float *w_opt, *m, *v, *dw, *dws, *g_img, *colsumW, *colsumX, *yx, *yy, *xx, *xc, *losses;
    int colsums_valid;
    float* adam_tab;        // device [steps][2]: the Adam bias corrections of every step
    float* adam_tab_host;   // host copy (malloc), uploaded ONCE (first run; constant afterwards)
    int adam_tab_valid;
    int* step_ctr;          // device (16 ints: [0] counter, [4..5] crop_dev, [8] ticket of la_step_tail)
    int* crop_dev;          // device {y0, x0} of the perceptual window
    int win_lo, win_hi;     // image rows the criteria read (la_latent_opt_set_row_window; 0 / 0 = unknown: whole frames in every step)
    int wcol_lo, wcol_hi;   // ... and image columns (la_latent_opt_set_col_window; 0 / 0 = all)
    int overlap;            // la_latent_opt_set_overlap: 0 criteria one after the other, 1 split replay, 2 (default) fork / join inside the step
    struct Lpips {          // the perceptual criterion (la_latent_opt_set_lpips)
        la_feat* f;
        const float* bankF; long Mf;          // [imgc][Mf][F] (modality-major)
        int F, S;                             // features per image; side of the window the features are taken of
        int crop_x, crop_y;                   // absolute position of the window (la_latent_opt_set_crop_pos)
        float pre_scale[4], pre_shift[4];     // input affine of the feature net, per repeated channel
        float *xc, *feat, *gfeat, *gxc, *colsum, *yx, *yy, *xx;
        int colsum_valid;
    } lp;
    struct Trace {          // what a logging run leaves behind, all optional; any of the three traces keeps the launches eager
        float* w;           // [steps][B][w_dim] (W+: [steps][B][num_ws][w_dim]): the latent after every step (la_latent_opt_set_trace)
        float* img;         // [steps][B][C][R][R]: the image synthesised in every step; keeps the steps on whole frames too
        float* dw;          // the shape of w: dL/dw of every step (la_latent_opt_set_grad_trace)
        int time_trace;     // la_latent_opt_set_time_trace: a run that returns loss scalars records LA_TEV events per step on the launch stream
        hipEvent_t* tev; int tev_steps;      // [tev_steps][LA_TEV]
    } tr;
    // The side branch: the perceptual part of a step beside the discriminator part.  It needs the image only, and its crop gradient is added
    // into g_img on the launch stream after the discriminator's: same arithmetic, same summation order.  Possible since no kernel of the
    // library contains packed-FP32 arithmetic ('Two streams').  Made by the first run with both criteria and overlap != 0.
    struct Side { hipStream_t stream; hipEvent_t ev_fork, ev_join; } side;
    // The captured step: what a step launches is independent of the step number (step counter, Adam bias corrections and window position
    // are read from device memory), so ONE capture is replayed for every step of every batch of the same size.
    struct Graphs {
        LaGraphPart part[4];
        int count;              // 0: none; 1: the whole step, in part[0]; 4: the parts A, P, D, Z (overlap mode 1)
        int B, windowed;        // batch size of the capture, and whether its synthesis passes were windowed
        int gen[3];             // settings generations of the attached engines (synthesis, discriminator, features) at the capture
        int mode;               // 0 eager, 1 replay a captured step (default; la_latent_opt_set_graph)
        int refused;            // 1: stream capture / instantiation of the step failed once; the handle launches eagerly since
        hipStream_t cap_stream; // capture needs a non-default stream; the replay goes to the caller's stream
    } graphs;
};

static size_t carve(la_latent_opt* h, char* base) {
    LaCarver c{base};
    const size_t B = h->maxB, wd = h->wdim, cc2 = (size_t)h->cfg.crop * h->cfg.crop;
    const size_t wl = h->wplus ? (size_t)h->num_ws * wd : wd;      // floats of one sample's optimised latent
    h->w_opt = c.take(B * wl); h->m = c.take(B * wl); h->v = c.take(B * wl); h->dw = c.take(B * wl);
    h->dws = c.take(B * h->num_ws * wd);
    h->g_img = c.take(B * h->imgc * (size_t)h->R * h->R);
    h->colsumW = c.take((size_t)h->num_ws * wd);
    h->colsumX = c.take((size_t)h->imgc * cc2);
    const size_t mm = (size_t)(h->Mw > h->Mx ? h->Mw : h->Mx);
    h->yx = c.take(LA_YX_FLOATS(mm ? mm : 1, B)); h->yy = c.take(LA_YY_FLOATS(mm ? mm : 1)); h->xx = c.take(LA_XX_FLOATS(B));
    h->xc = c.take(B * h->imgc * cc2);
    h->losses = c.take((size_t)(h->cfg.steps > 0 ? h->cfg.steps : 1) * 4);
    h->adam_tab = c.take((size_t)(h->cfg.steps > 0 ? h->cfg.steps : 1) * 2);
    h->step_ctr = c.take<int>(16);
    h->crop_dev = h->step_ctr + 4;
    return c.off;
}

// the perceptual criterion's buffers (la_latent_opt_set_lpips): from imgc, maxB, F, S, Mf of the handle
static size_t carve_lpips(la_latent_opt* h, char* base) {
    LaCarver c{base};
    const size_t n = (size_t)h->imgc * h->maxB;
    auto& p = h->lp;
    p.xc = c.take(n * 3 * p.S * p.S); p.gxc = c.take(n * 3 * p.S * p.S);
    p.feat = c.take(n * p.F); p.gfeat = c.take(n * p.F);
    p.colsum = c.take((size_t)h->imgc * p.F);
    p.yx = c.take(LA_YX_FLOATS(p.Mf, h->maxB)); p.yy = c.take(LA_YY_FLOATS(p.Mf)); p.xx = c.take(LA_XX_FLOATS(h->maxB));
    return c.off;
}

// latent_space: 0 W, 1 W+ (anything else: 0 bytes, and la_latent_opt_create_ex refuses it)
extern "C" size_t la_latent_opt_workspace_bytes_ex(int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                                                   long Mw, long Mx, int max_batch, int latent_space) {
    if (!cfg || (latent_space != 0 && latent_space != 1)) return 0;
    la_latent_opt h; memset(&h, 0, sizeof(h));
    h.cfg = *cfg; h.R = img_resolution; h.imgc = img_channels; h.wdim = w_dim; h.num_ws = la_synth_num_ws(img_resolution);
    h.maxB = max_batch; h.Mw = Mw; h.Mx = Mx; h.wplus = latent_space;
    return carve(&h, nullptr);
}

extern "C" size_t la_latent_opt_workspace_bytes(int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                                                long Mw, long Mx, int max_batch) {
    return la_latent_opt_workspace_bytes_ex(img_resolution, img_channels, w_dim, cfg, Mw, Mx, max_batch, 0);
}

extern "C" int la_latent_opt_create(la_synth* g, int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                                    const float* bankW, long Mw, const float* bankXc, long Mx, int max_batch,
                                    void* workspace, size_t workspace_bytes, la_latent_opt** out) {
    return la_latent_opt_create_ex(g, img_resolution, img_channels, w_dim, cfg, bankW, Mw, bankXc, Mx, max_batch, 0, workspace,
                                   workspace_bytes, out);
}

extern "C" int la_latent_opt_create_ex(la_synth* g, int img_resolution, int img_channels, int w_dim, const la_opt_config* cfg,
                                       const float* bankW, long Mw, const float* bankXc, long Mx, int max_batch, int latent_space,
                                       void* workspace, size_t workspace_bytes, la_latent_opt** out) {
    LA_CHECK_ARG(latent_space == 0 || latent_space == 1, "latent_opt_create: latent_space must be 0 (W) or 1 (W+)");
    LA_CHECK_ARG(latent_space == 0 || w_dim % 4 == 0, "latent_opt_create: W+ needs w_dim % 4 == 0");
    LA_CHECK_ARG(g && cfg && workspace && out, "latent_opt_create: null pointer");
    LA_CHECK_ARG(cfg->steps >= 0, "latent_opt_create: negative step count");
    LA_CHECK_ARG(cfg->w_latent == 0.f || (bankW && Mw >= 1), "latent_opt_create: w_latent > 0 needs the latent bank W");
    LA_CHECK_ARG(cfg->w_pix == 0.f || (bankXc && Mx >= 1), "latent_opt_create: w_pix > 0 needs the cropped image bank X");
    LA_CHECK_ARG(cfg->crop >= 1 && cfg->crop_off >= 0 && cfg->crop + cfg->crop_off <= img_resolution,
                 "latent_opt_create: centre crop does not fit the image");
    LA_CHECK_ARG(cfg->criterion_mode == 0 || cfg->criterion_mode == 1, "latent_opt_create: criterion_mode must be 0 or 1");
    auto own = la_host_handle<la_latent_opt>();
    la_latent_opt* h = own.get();
    LA_CHECK_ARG(h, "latent_opt_create: out of host memory");
    memset(h, 0, sizeof(*h));
    h->g = g; h->cfg = *cfg; h->R = img_resolution; h->imgc = img_channels; h->wdim = w_dim;
    h->num_ws = la_synth_num_ws(img_resolution); h->maxB = max_batch; h->wplus = latent_space;
    h->bankW = bankW; h->Mw = cfg->w_latent != 0.f ? Mw : 0; h->bankX = bankXc; h->Mx = cfg->w_pix != 0.f ? Mx : 0;
    const size_t need = carve(h, (char*)workspace);
    LA_CHECK_WORKSPACE(workspace_bytes, need, "latent_opt_create: workspace too small");
    h->adam_tab_host = (float*)malloc(sizeof(float) * 2 * (size_t)(cfg->steps > 0 ? cfg->steps : 1));
    LA_CHECK_ARG(h->adam_tab_host, "latent_opt_create: out of host memory");
    la_adam_fill_table(h->adam_tab_host, cfg->steps, cfg->beta1, cfg->beta2);
    h->graphs.mode = 1;
    h->overlap = 2;
    *out = own.release();
    return LA_OK;
}

static void drop_graph(la_latent_opt* h) {
    for (auto& p : h->graphs.part) {      // (all four: a capture that failed half way leaves parts behind with count still 0)
        if (p.exec) { (void)hipGraphExecDestroy(p.exec); p.exec = nullptr; }
        if (p.graph) { (void)hipGraphDestroy(p.graph); p.graph = nullptr; }
    }
    h->graphs.count = 0; h->graphs.B = 0; h->graphs.windowed = 0;
}

extern "C" void la_latent_opt_destroy(la_latent_opt* h) {
    if (!h) return;
    drop_graph(h);
    if (h->tr.tev) { for (int i = 0; i < h->tr.tev_steps * LA_TEV; ++i) (void)hipEventDestroy(h->tr.tev[i]); free(h->tr.tev); }
    if (h->side.ev_fork) (void)hipEventDestroy(h->side.ev_fork);
    if (h->side.ev_join) (void)hipEventDestroy(h->side.ev_join);
    if (h->side.stream) (void)hipStreamDestroy(h->side.stream);
    if (h->graphs.cap_stream) (void)hipStreamDestroy(h->graphs.cap_stream);
    free(h->adam_tab_host);
    free(h);
}

// the three modes: include/latentaug_hip.h and plan_schedule below; bit-identical results in every one
extern "C" int la_latent_opt_set_overlap(la_latent_opt* h, int enable) {
    LA_CHECK_ARG(h, "latent_opt_set_overlap: null handle");
    h->overlap = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    drop_graph(h);
    return LA_OK;
}

// Image rows [row_lo, row_hi) that the IMAGE criteria of the loop read (0, 0 = not known): with the pixel criterion on its centre crop and
// the perceptual criterion on a window inside it, nothing in a loop step depends on the other rows of the synthesised image, and the
// synthesis passes of the steps deliver that window only (la_synth_set_row_window: the top blocks compute the rows it depends on).  The
// final synthesis of the augmented latent is always a whole frame.  Ignored while the discriminator (whole frame) is active or
// per-step images are traced.
extern "C" int la_latent_opt_set_row_window(la_latent_opt* h, int row_lo, int row_hi) {
    LA_CHECK_ARG(h && row_lo >= 0 && (row_hi == 0 ? row_lo == 0 : (row_hi > row_lo && row_hi <= h->R)), "latent_opt_set_row_window: bad window");
    if (row_lo != h->win_lo || row_hi != h->win_hi) drop_graph(h);
    h->win_lo = row_lo; h->win_hi = row_hi;
    return LA_OK;
}

// ... and the image columns [col_lo, col_hi) they read (0, 0 = all): used together with the row window (la_synth_set_col_window)
extern "C" int la_latent_opt_set_col_window(la_latent_opt* h, int col_lo, int col_hi) {
    LA_CHECK_ARG(h && col_lo >= 0 && (col_hi == 0 ? col_lo == 0 : (col_hi > col_lo && col_hi <= h->R)), "latent_opt_set_col_window: bad window");
    if (col_lo != h->wcol_lo || col_hi != h->wcol_hi) drop_graph(h);
    h->wcol_lo = col_lo; h->wcol_hi = col_hi;
    return LA_OK;
}

extern "C" int la_latent_opt_set_trace(la_latent_opt* h, float* w_trace, float* img_trace) {
    LA_CHECK_ARG(h, "latent_opt_set_trace: null handle");
    h->tr.w = w_trace; h->tr.img = img_trace;
    return LA_OK;
}

// Per-criterion times of a run that asks for the loss scalars (the reference's verbose_log timers time_latent / time_disc / time_pix /
// time_lpips / time_epoch, util_latent_aug.py:221-272): HIP events on the launch stream around the criteria of every step.  Here a
// criterion's bracket holds its loss scalar AND its gradient launches (the reference's holds the forward only; its backward is inside
// the untimed loss.backward()), time_epoch the whole step.  Read back with la_latent_opt_get_times after the stream has drained.
extern "C" int la_latent_opt_set_time_trace(la_latent_opt* h, int enable) {
    LA_CHECK_ARG(h, "latent_opt_set_time_trace: null handle");
    if (enable && !h->tr.tev && h->cfg.steps > 0) {
        h->tr.tev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * (size_t)h->cfg.steps * LA_TEV);
        LA_CHECK_ARG(h->tr.tev, "latent_opt_set_time_trace: out of host memory");
        for (int i = 0; i < h->cfg.steps * LA_TEV; ++i) LA_HIP(hipEventCreate(&h->tr.tev[i]));
        h->tr.tev_steps = h->cfg.steps;
    }
    h->tr.time_trace = enable ? 1 : 0;
    return LA_OK;
}

// ms [steps][5] = {time_latent, time_disc, time_pix, time_lpips, time_epoch} in milliseconds of the last run that recorded them
// (waits for the events: call after the run's stream work is complete or let it block)
extern "C" int la_latent_opt_get_times(la_latent_opt* h, float* ms) {
    LA_CHECK_ARG(h && ms && h->tr.tev, "latent_opt_get_times: no time trace recorded");
    for (int s = 0; s < h->tr.tev_steps; ++s) {
        hipEvent_t* e = h->tr.tev + (size_t)s * LA_TEV;
        LA_HIP(hipEventSynchronize(e[LA_TEV - 1]));
        float t[LA_TEV - 1];
        for (int k = 0; k + 1 < LA_TEV; ++k) LA_HIP(hipEventElapsedTime(&t[k], e[k], e[k + 1]));
        float* o = ms + (size_t)s * 5;
        o[0] = t[1]; o[2] = t[2]; o[1] = t[3]; o[3] = t[4];
        LA_HIP(hipEventElapsedTime(&o[4], e[0], e[LA_TEV - 1]));
    }
    return LA_OK;
}

// dL/dw [steps][B][w_dim] of every step (L = -latent - pix - lpips + disc, util_latent_aug.py:270): what Adam consumes, before
// its sign-like normalisation hides magnitudes.  Parity tests compare step 1 with a float64 gradient at full size.
extern "C" int la_latent_opt_set_grad_trace(la_latent_opt* h, float* dw_trace) {
    LA_CHECK_ARG(h, "latent_opt_set_grad_trace: null handle");
    h->tr.dw = dw_trace;
    return LA_OK;
}

// The banks (W, X crops, LPIPS features) are CONSTANTS of the handle: their column sums are reduced once and reused by every later
// step and batch.  A caller that rewrites bank contents in place must call this before the next run (the loss scalars are always
// computed from the live banks; without this call the gradient would keep using the old sums).
extern "C" int la_latent_opt_invalidate_banks(la_latent_opt* h) {
    LA_CHECK_ARG(h, "latent_opt_invalidate_banks: null handle");
    h->colsums_valid = 0;
    h->lp.colsum_valid = 0;
    return LA_OK;
}

// 1: a captured step is instantiated and being replayed; 0: eager launches (as asked, or no batch has run yet); -1: eager because the
// capture of the step was refused by the runtime (la_latent_opt_set_graph(h, 1) re-arms it)
extern "C" int la_latent_opt_graph_state(const la_latent_opt* h) {
    if (!h) return 0;
    return h->graphs.count ? 1 : (h->graphs.refused ? -1 : 0);
}

// 1 (default): steps 2..N of the first batch and every step of later batches replay ONE captured step; 0: every launch eager
extern "C" int la_latent_opt_set_graph(la_latent_opt* h, int enable) {
    LA_CHECK_ARG(h, "latent_opt_set_graph: null handle");
    h->graphs.mode = enable ? 1 : 0;
    h->graphs.refused = 0;
    if (!enable) drop_graph(h);
    return LA_OK;
}

// attach the discriminator engine used by the w_disc criterion (required before la_latent_opt_run when w_disc != 0)
extern "C" int la_latent_opt_set_disc(la_latent_opt* h, la_disc* d) {
    LA_CHECK_ARG(h, "latent_opt_set_disc: null handle");
    h->d = d;
    drop_graph(h);
    return LA_OK;
}

// LPIPS criterion: feature engine, real-feature banks [imgc][Mf][F] (modality-major), crop size S (crop_size_aug) and the
// affine input preprocess x*scale + shift.  ws: la_latent_opt_lpips_workspace_bytes() of device memory.
extern "C" size_t la_latent_opt_lpips_workspace_bytes(int img_channels, int F, int S, long Mf, int max_batch) {
    la_latent_opt h; memset(&h, 0, sizeof(h));
    h.imgc = img_channels; h.lp.F = F; h.lp.S = S; h.lp.Mf = Mf; h.maxB = max_batch;
    return carve_lpips(&h, nullptr);
}

extern "C" int la_latent_opt_set_lpips(la_latent_opt* h, la_feat* f, const float* bankF, long Mf, int S, float pre_scale,
                                       float pre_shift, void* ws, size_t ws_bytes) {
    LA_CHECK_ARG(h && f && bankF && Mf >= 1 && S >= 1 && ws, "latent_opt_set_lpips: bad arguments");
    const int F = la_feat_num_features(f);
    LA_CHECK_WORKSPACE(ws_bytes, la_latent_opt_lpips_workspace_bytes(h->imgc, F, S, Mf, h->maxB), "latent_opt_set_lpips: workspace too small");
    h->lp.f = f; h->lp.bankF = bankF; h->lp.Mf = Mf; h->lp.F = F; h->lp.S = S; for (int k = 0; k < 4; ++k) { h->lp.pre_scale[k] = pre_scale; h->lp.pre_shift[k] = pre_shift; }
    carve_lpips(h, (char*)ws);
    h->lp.colsum_valid = 0;
    drop_graph(h);
    return LA_OK;
}

// per-channel input affine of the feature net (the three repeated channels of :394): x_k * scale[k] + shift[k], e.g. the
// (x - mean_k) / std_k input layer of NVIDIA's vgg16.pt.  Overrides the scalar pair of la_latent_opt_set_lpips.
extern "C" int la_latent_opt_set_lpips_preproc(la_latent_opt* h, const float* scale, const float* shift, int n) {
    LA_CHECK_ARG(h && scale && shift && n >= 1 && n <= 4, "latent_opt_set_lpips_preproc: bad arguments");
    for (int k = 0; k < 4; ++k) { h->lp.pre_scale[k] = scale[k < n ? k : n - 1]; h->lp.pre_shift[k] = shift[k < n ? k : n - 1]; }
    drop_graph(h);
    return LA_OK;
}

// position of the crop_size_aug window inside the image, drawn by the host once per forward (util_dataset.py:284-296);
// (x, y) are absolute pixel coordinates (centre-crop offset already added)
extern "C" int la_latent_opt_set_crop_pos(la_latent_opt* h, int x, int y) {
    LA_CHECK_ARG(h && x >= 0 && y >= 0, "latent_opt_set_crop_pos: bad arguments");
    h->lp.crop_x = x; h->lp.crop_y = y;
    return LA_OK;
}

__global__ void la_lpips_gfeat_kernel(const float* __restrict__ feat, const float* __restrict__ colsum, float* __restrict__ g, int B,
                                      int F, float coef2, float mrows, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / F; const int k = (int)(i - n * F);
    const int c = (int)(n / B);
    g[i] = coef2 * (mrows * feat[i] - colsum[(long)c * F + k]);
}

// crop window position by value (no host buffer that a later call could overwrite while a copy is still in flight)
__global__ void la_set_int2_kernel(int* __restrict__ dst, int a, int b) { dst[0] = a; dst[1] = b; }

#define LA_RC(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)      // a library call's status, as LA_HIP a runtime call's

// What la_latent_opt_run derives from the handle and the batch: constant for every step of the run
struct LaRun {
    int B; long nw;         // batch; floats of the optimised latents (and of one trace step)
    float nb;               // batch size the criteria's means divide by
    bool use_disc, use_lpips, img_crit;      // img_crit: some criterion reads the image, so the step has an image gradient and a synthesis backward
    bool windowed;          // the synthesis passes of the steps deliver the handle's window only
    float lat_coef, pix_coef, lp_coef;      // loss = -loss_latent - loss_pix - loss_lpips + loss_disc  (:270): the diversity terms enter with a minus sign
    long wb, wl;            // w_opt strides per sample, per slot.  W: one row per sample read by every slot (ws = broadcasting(w_opt)); W+: a row per slot
};

static LaRun make_run(const la_latent_opt* h, int B) {
    const la_opt_config& c = h->cfg; const auto& p = h->lp;
    const int wd = h->wdim, cc = c.crop, off = c.crop_off;
    LaRun r;
    r.B = B; r.nw = (long)B * wd * (h->wplus ? h->num_ws : 1); r.nb = (float)(c.norm_batch > 0 ? c.norm_batch : B);
    r.use_disc = c.w_disc != 0.f; r.use_lpips = c.w_lpips != 0.f; r.img_crit = c.w_pix != 0.f || r.use_disc || r.use_lpips;
    r.lat_coef = h->Mw ? c.w_latent / ((float)h->Mw * r.nb * (float)h->num_ws * (float)wd) : 0.f;
    r.pix_coef = h->Mx ? c.w_pix / ((float)h->imgc * (float)h->Mx * r.nb * (float)((long)cc * cc)) : 0.f;
    r.lp_coef = r.use_lpips ? c.w_lpips / ((float)h->imgc * (float)p.Mf * r.nb) : 0.f;
    r.wb = h->wplus ? (long)h->num_ws * wd : wd; r.wl = h->wplus ? wd : 0;
    // Loop steps: the synthesis delivers the rows the criteria read; whole frames with the discriminator, with per-step image snapshots, or
    // with no window given.  The window is a caller-supplied hint (la_latent_opt_set_row_window / _col_window): it is honoured only while
    // every row and column the criteria of THIS run read lies inside it -- the pixel criterion's centre crop, the perceptual criterion's
    // crop_size window at the position of la_latent_opt_set_crop_pos.  A window that does not contain them would optimise against stale
    // rows of an earlier pass; such a run synthesises whole frames instead.
    auto inside = [&](int y0, int y1, int x0, int x1) { return y0 >= h->win_lo && y1 <= h->win_hi && (h->wcol_hi <= 0 || (x0 >= h->wcol_lo && x1 <= h->wcol_hi)); };
    const bool win_covers = (c.w_pix == 0.f || inside(off, off + cc, off, off + cc)) &&
                            (!r.use_lpips || inside(p.crop_y, p.crop_y + p.S, p.crop_x, p.crop_x + p.S));
    r.windowed = h->win_hi > 0 && !r.use_disc && !h->tr.img && win_covers;
    return r;
}

// the run's starting state: latent, Adam moments, step counter, window position
static int reset_state(la_latent_opt* h, const LaRun& r, const float* w0, hipStream_t stream) {
    LA_HIP(hipMemcpyAsync(h->w_opt, w0, r.nw * sizeof(float), hipMemcpyDeviceToDevice, stream));
    LA_HIP(hipMemsetAsync(h->m, 0, r.nw * sizeof(float), stream)); LA_HIP(hipMemsetAsync(h->v, 0, r.nw * sizeof(float), stream));
    LA_HIP(hipMemsetAsync(h->step_ctr, 0, 16 * sizeof(int), stream));      // step counter [0], crop position [4..5] (set below), ticket of la_step_tail [8]
    if (h->cfg.steps > 0 && !h->adam_tab_valid) {      // constant after create: one (host-blocking, pageable) upload per handle, not per batch
        LA_HIP(hipMemcpyAsync(h->adam_tab, h->adam_tab_host, sizeof(float) * 2 * (size_t)h->cfg.steps, hipMemcpyHostToDevice, stream));
        LA_HIP(hipStreamSynchronize(stream));
        h->adam_tab_valid = 1;
    }
    hipLaunchKernelGGL(la_set_int2_kernel, dim3(1), dim3(1), 0, stream, h->crop_dev, h->lp.crop_y, h->lp.crop_x);
    return LA_OK;
}

// The gradient needs the bank column sums only, and the banks are constants of the handle: reduced once (deterministic summation order, so
// this is bit-identical to re-reducing them every step).
static int refresh_colsums(la_latent_opt* h, const LaRun& r, hipStream_t stream) {
    const auto& p = h->lp;
    const long cc2 = (long)h->cfg.crop * h->cfg.crop;
    if (!h->colsums_valid) {
        if (h->Mw) LA_RC(la_bank_colsum(h->bankW, h->Mw, (long)h->num_ws * h->wdim, h->colsumW, stream));
        if (h->Mx)
            for (int c = 0; c < h->imgc; ++c) LA_RC(la_bank_colsum(h->bankX + (long)c * h->Mx * cc2, h->Mx, cc2, h->colsumX + (long)c * cc2, stream));
        h->colsums_valid = 1;
    }
    if (r.use_lpips && !p.colsum_valid) {
        for (int c = 0; c < h->imgc; ++c) LA_RC(la_bank_colsum(p.bankF + (long)c * p.Mf * p.F, p.Mf, p.F, p.colsum + (long)c * p.F, stream));
        h->lp.colsum_valid = 1;
    }
    return LA_OK;
}

// One optimisation step is four parts -- A | D and P | Z -- each a function of (handle, run, L, tev, stream).  L: this step's row of loss scalars
// or null (they only feed the reference's log lines, :234-271: computed when the caller asks for them, i.e. verbose_log).  tev: this step's
// LA_TEV timer events or null.  Their brackets (la_latent_opt_get_times): [1,2) latent loss scalar, [2,3) pixel loss scalar + gradient, [3,4)
// discriminator, [4,5) perceptual; the latent criterion's GRADIENT is fused with the step tail and sits in the epoch bracket [0,6) only.
static void mark(hipEvent_t* tev, int k, hipStream_t st) { if (tev) (void)hipEventRecord(tev[k], st); }

// A: synthesis forward, loss scalars of the latent and pixel criteria, pixel gradient
static int part_synth(la_latent_opt* h, const LaRun& r, float* L, hipEvent_t* tev, hipStream_t st) {
    const la_opt_config& c = h->cfg;
    const int B = r.B, wd = h->wdim, cc = c.crop, off = c.crop_off;
    const long cc2 = (long)cc * cc;
    mark(tev, 0, st);
    LA_RC(la_synth_forward(h->g, h->w_opt, r.wb, r.wl, B, c.loop_noise_mode, nullptr, nullptr, st));
    const float* img = la_synth_image(h->g);
    mark(tev, 1, st);
    if (L && h->Mw) LA_RC(la_l2_mean_from_bank(h->bankW, h->Mw, (long)h->num_ws * wd, h->w_opt, B, r.wb, h->wplus ? 0 : wd, h->yx, h->yy, h->xx, r.lat_coef, L + 0, 0, st));
    mark(tev, 2, st);
    if (L && h->Mx) {
        LA_RC(la_center_crop_f32(img, h->xc, (long)B * h->imgc, h->R, cc, off, st));
        for (int ch = 0; ch < h->imgc; ++ch)
            LA_RC(la_l2_mean_from_bank(h->bankX + (long)ch * h->Mx * cc2, h->Mx, cc2, h->xc + (long)ch * cc2, B, (long)h->imgc * cc2, 0, h->yx, h->yy,
                                       h->xx, r.pix_coef, L + 1, ch > 0, st));
    }
    if (!r.img_crit) return LA_OK;
    if (c.w_pix != 0.f) LA_RC(la_pix_grad(img, h->colsumX, h->g_img, B, h->imgc, h->R, cc, off, -2.f * r.pix_coef, (float)h->Mx, st));
    mark(tev, 3, st);
    return LA_OK;
}

// P: the perceptual branch up to the gradient of its window; of the step's results it reads the image only.
// loss_lpips = mean_modes( sum_{m,n} |f_n - F_m|^2 / (n*m) ) * w_lpips, entering the total with a minus sign (:270)
static int part_lpips(la_latent_opt* h, const LaRun& r, float* L, hipEvent_t*, hipStream_t st) {
    const auto& p = h->lp;
    const float* img = la_synth_image(h->g);      // (the loop's image buffer: fixed per handle)
    const int B = r.B, N = h->imgc * B;
    const long FF = p.F, total = (long)N * FF;
    // (g_img is overwritten by its first writer: the pixel gradient, else the discriminator's; with neither the crop gradient is added to zeros)
    if (h->cfg.w_pix == 0.f && !r.use_disc) LA_HIP(hipMemsetAsync(h->g_img, 0, sizeof(float) * (size_t)B * h->imgc * h->R * h->R, st));
    LA_RC(la_crop_repeat(img, p.xc, B, h->imgc, h->R, p.S, p.crop_y, p.crop_x, h->crop_dev, 3, p.pre_scale, p.pre_shift, st));
    LA_RC(la_feat_forward(p.f, p.xc, N, p.feat, st));
    if (L)
        for (int ch = 0; ch < h->imgc; ++ch)
            LA_RC(la_l2_mean_from_bank(p.bankF + (long)ch * p.Mf * FF, p.Mf, FF, p.feat + (long)ch * B * FF, B, FF, 0, p.yx, p.yy, p.xx, r.lp_coef, L + 3, ch > 0, st));
    hipLaunchKernelGGL(la_lpips_gfeat_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, st, p.feat, p.colsum, p.gfeat, B, (int)FF,
                       -2.f * r.lp_coef, (float)p.Mf, total);
    return la_feat_backward(p.f, p.gfeat, p.gxc, st);
}

// D: the discriminator branch.  loss_disc = softplus(-D(x)).mean() * w_disc enters the total with a plus sign (:270)
static int part_disc(la_latent_opt* h, const LaRun& r, float* L, hipEvent_t* tev, hipStream_t st) {
    if (r.use_disc) {
        LA_RC(la_disc_forward(h->d, la_synth_image(h->g), r.B, st));
        LA_RC(la_disc_loss(h->d, h->cfg.w_disc, h->cfg.norm_batch, L ? L + 2 : nullptr, st));
        LA_RC(la_disc_backward(h->d, nullptr, h->g_img, h->cfg.w_pix != 0.f, st));
    }
    mark(tev, 4, st);
    return LA_OK;
}

// Z: the window's gradient added into g_img, synthesis backward, step tail
static int part_tail(la_latent_opt* h, const LaRun& r, float*, hipEvent_t* tev, hipStream_t st) {
    const la_opt_config& c = h->cfg; const auto& p = h->lp;
    if (r.img_crit) {
        if (r.use_lpips) LA_RC(la_crop_repeat_grad(p.gxc, h->g_img, r.B, h->imgc, h->R, p.S, p.crop_y, p.crop_x, h->crop_dev, 3, p.pre_scale, st));
        mark(tev, 5, st);
        LA_RC(la_synth_backward(h->g, h->g_img, h->dws, st));
    } else { mark(tev, 3, st); mark(tev, 4, st); mark(tev, 5, st); }
    // dw = sum_ws dws + latent gradient, Adam, step counter: one launch (la_step_tail; W+: la_wplus_step_tail, no sum over the slots)
    LA_RC((h->wplus ? la_wplus_step_tail : la_step_tail)(r.img_crit ? h->dws : nullptr, h->Mw ? h->colsumW : nullptr, h->dw, h->w_opt, h->m, h->v, r.B,
                                                         h->num_ws, h->wdim, -2.f * r.lat_coef, (float)h->Mw, c.lr, c.beta1, c.beta2, c.eps,
                                                         h->adam_tab, h->step_ctr, h->step_ctr + 8, st));
    mark(tev, 6, st);
    return LA_OK;
}

typedef int (*LaPartFn)(la_latent_opt*, const LaRun&, float*, hipEvent_t*, hipStream_t);
static const LaPartFn la_parts[4] = {part_synth, part_lpips, part_disc, part_tail};      // indexed by LA_PART_*

// fork: the side stream goes on from what has been issued to `st`.  The join comes in two halves, so that work can be issued to `st` between
// them: the end of the side branch, and `st` waiting for it.
static int fork_side(la_latent_opt* h, hipStream_t st) {
    LA_HIP(hipEventRecord(h->side.ev_fork, st));
    LA_HIP(hipStreamWaitEvent(h->side.stream, h->side.ev_fork, 0));
    return LA_OK;
}
static int side_done(la_latent_opt* h) { LA_HIP(hipEventRecord(h->side.ev_join, h->side.stream)); return LA_OK; }
static int join_side(la_latent_opt* h, hipStream_t st) { LA_HIP(hipStreamWaitEvent(st, h->side.ev_join, 0)); return LA_OK; }

// part k of a step: its launches, or with `g` the replay of its captured graph
static int issue(la_latent_opt* h, const LaRun& r, const LaGraphPart* g, int k, float* L, hipEvent_t* tev, hipStream_t st) {
    if (!g) return la_parts[k](h, r, L, tev, st);
    LA_HIP(hipGraphLaunch(g[k].exec, st));
    return LA_OK;
}

// One step on `st`, the only place that orders the parts: A | D and P | Z.  g: null, or the four captured parts to replay instead of
// launching.  side: P goes to the side stream, forked after A and joined before Z (the crop gradient is added into g_img on the launch
// stream, after the discriminator's).  p_first: P is issued before D -- the order of the split replay -- instead of after it.
static int run_step(la_latent_opt* h, const LaRun& r, const LaGraphPart* g, bool side, bool p_first, float* L, hipEvent_t* tev, hipStream_t st) {
    LA_RC(issue(h, r, g, LA_PART_A, L, tev, st));
    if (r.img_crit) {
        if (side) LA_RC(fork_side(h, st));
        if (!p_first) LA_RC(issue(h, r, g, LA_PART_D, L, tev, st));
        if (r.use_lpips) LA_RC(issue(h, r, g, LA_PART_P, L, tev, side ? h->side.stream : st));
        if (side) LA_RC(side_done(h));
        if (p_first) LA_RC(issue(h, r, g, LA_PART_D, L, tev, st));
        if (side) LA_RC(join_side(h, st));
    }
    return issue(h, r, g, LA_PART_Z, L, tev, st);
}

// The schedule of a run, decided here and nowhere else
struct LaPlan {
    bool replay;            // after one launched step, the steps replay captured graphs (false: every step is launched)
    int parts;              // ... 1: the whole step as one graph; 4: A, P, D, Z as graphs of their own, P replayed on the side stream
    bool side;              // a whole step -- launched or captured -- forks P to the side stream
};
static LaPlan plan_schedule(const la_latent_opt* h, const LaRun& r, bool want_losses) {
    // The launch profiler (la_prof_begin .. la_prof_end) needs eager launches on one stream for its event brackets, and so do the loss scalars
    // with their timers.  The traces are copied out between steps: eager, but the fork does not disturb them.
    const bool prof = la_prof_enabled(), tracing = h->tr.w || h->tr.img || h->tr.dw;
    const bool branches = r.use_disc && r.use_lpips && h->side.stream && h->side.ev_fork && h->side.ev_join;      // two parts, and somewhere to put one
    const bool replay = h->graphs.mode == 1 && !want_losses && !tracing && h->cfg.steps > 0 && !prof;
    // (overlap mode 1 overlaps only while it replays: its launched steps stay one after the other)
    return LaPlan{replay, replay && h->overlap == 1 && branches ? 4 : 1, h->overlap == 2 && branches && !want_losses && !prof};
}

// part k of the plan -- the whole step when it has one part -- captured into the graph table
static bool capture(la_latent_opt* h, const LaRun& r, const LaPlan& plan, int k) {
    auto& G = h->graphs;
    bool ok = hipStreamBeginCapture(G.cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
        const int rcs = plan.parts == 4 ? la_parts[k](h, r, nullptr, nullptr, G.cap_stream)
                                        : run_step(h, r, nullptr, plan.side, false, nullptr, nullptr, G.cap_stream);
        const hipError_t er = hipStreamEndCapture(G.cap_stream, &G.part[k].graph);
        ok = rcs == LA_OK && er == hipSuccess && G.part[k].graph;
    }
    return ok && hipGraphInstantiate(&G.part[k].exec, G.part[k].graph, nullptr, nullptr, 0) == hipSuccess;
}

// The steps of a run.  A replaying run whose graphs do not fit (none yet, another batch size or window flag, an attached engine set to
// another precision or ToRGB schedule since) launches step 1 eagerly -- module
// loading, per-device attribute opt-ins and every other first-use effect happen outside the capture -- captures the same sequencer and
// replays it from step 2 on.  If capture is refused the handle falls back to eager launches of the same kernels.
// the settings generations of the engines a step of this run launches (an engine the run does not use: 0)
static void engine_gens(const la_latent_opt* h, const LaRun& r, int gen[3]) {
    gen[0] = la_synth_settings_gen(h->g);
    gen[1] = r.use_disc ? la_disc_settings_gen(h->d) : 0;
    gen[2] = r.use_lpips ? la_feat_settings_gen(h->lp.f) : 0;
}

static int run_steps(la_latent_opt* h, const LaRun& r, const LaPlan& plan, bool want_losses, hipStream_t stream) {
    const la_opt_config& c = h->cfg; const auto& t = h->tr;
    auto& G = h->graphs;
    int first = 1;
    int gen[3]; engine_gens(h, r, gen);
    const bool engines_set = gen[0] != G.gen[0] || gen[1] != G.gen[1] || gen[2] != G.gen[2];      // a setter of an attached engine since the capture
    if (plan.replay && (G.count != plan.parts || G.B != r.B || G.windowed != (int)r.windowed || engines_set)) {
        drop_graph(h);
        LA_RC(run_step(h, r, nullptr, plan.side, false, nullptr, nullptr, stream));
        first = 2;
        bool ok = c.steps >= 2;
        if (ok && !G.cap_stream) ok = hipStreamCreateWithFlags(&G.cap_stream, hipStreamNonBlocking) == hipSuccess;
        for (int k = 0; k < plan.parts && ok; ++k) ok = capture(h, r, plan, k);
        if (ok) { G.count = plan.parts; G.B = r.B; G.windowed = (int)r.windowed; memcpy(G.gen, gen, sizeof(gen)); }
        else { drop_graph(h); (void)hipGetLastError(); if (c.steps >= 2) { G.mode = 0; G.refused = 1; } }
    }
    const size_t img_floats = (size_t)r.B * h->imgc * h->R * h->R;
    for (int step = first; step <= c.steps; ++step) {
        if (plan.replay && G.count == 4) LA_RC(run_step(h, r, G.part, true, true, nullptr, nullptr, stream));      // A | fork | P beside D | join | Z
        else if (plan.replay && G.count == 1) LA_HIP(hipGraphLaunch(G.part[0].exec, stream));
        else {
            float* L = want_losses ? h->losses + (size_t)(step - 1) * 4 : nullptr;
            hipEvent_t* tev = (L && t.time_trace && t.tev && step - 1 < t.tev_steps) ? t.tev + (size_t)(step - 1) * LA_TEV : nullptr;
            LA_RC(run_step(h, r, nullptr, plan.side, false, L, tev, stream));
            // verbose_log snapshots (util_latent_aug.py:292-295): the image synthesised in this step, the latent after its update
            if (t.img) LA_HIP(hipMemcpyAsync(t.img + (step - 1) * img_floats, la_synth_image(h->g), sizeof(float) * img_floats, hipMemcpyDeviceToDevice, stream));
            if (t.w) LA_HIP(hipMemcpyAsync(t.w + (size_t)(step - 1) * r.nw, h->w_opt, sizeof(float) * r.nw, hipMemcpyDeviceToDevice, stream));
            if (t.dw) LA_HIP(hipMemcpyAsync(t.dw + (size_t)(step - 1) * r.nw, h->dw, sizeof(float) * r.nw, hipMemcpyDeviceToDevice, stream));
        }
    }
    return LA_OK;
}

struct LaWinGuard { la_synth* g; ~LaWinGuard() { (void)la_synth_set_row_window(g, 0, 0); (void)la_synth_set_col_window(g, 0, 0); } };      // whole frames on every way out

extern "C" int la_latent_opt_run(la_latent_opt* h, const float* w0, int B, const float* const* final_noises,
                                 float* img_out, float* w_aug_out, float* losses_out, hipStream_t stream) {
    LA_CHECK_ARG(h && w0 && img_out && w_aug_out, "latent_opt_run: null pointer");
    LA_CHECK_ARG(B >= 1 && B <= h->maxB, "latent_opt_run: batch exceeds max_batch");
    const la_opt_config& c = h->cfg;
    LA_CHECK_ARG(c.final_noise_mode != 2 || final_noises, "latent_opt_run: explicit final noise requested but not given");
    const LaRun r = make_run(h, B);
    LA_CHECK_ARG(!r.use_disc || h->d, "latent_opt_run: w_disc != 0 but no discriminator attached (la_latent_opt_set_disc)");
    LA_CHECK_ARG(!r.use_lpips || h->lp.f, "latent_opt_run: w_lpips != 0 but no feature engine attached (la_latent_opt_set_lpips)");
    LA_CHECK_ARG(!r.use_lpips || (h->lp.crop_x + h->lp.S <= h->R && h->lp.crop_y + h->lp.S <= h->R), "latent_opt_run: LPIPS crop outside the image");
    const bool want_losses = losses_out != nullptr;
    LA_RC(reset_state(h, r, w0, stream));
    if (r.use_disc && r.use_lpips && h->overlap && !h->side.stream) {      // once per handle: the side stream and the fork / join events
        LA_HIP(hipStreamCreateWithFlags(&h->side.stream, hipStreamNonBlocking));
        LA_HIP(hipEventCreateWithFlags(&h->side.ev_fork, hipEventDisableTiming));
        LA_HIP(hipEventCreateWithFlags(&h->side.ev_join, hipEventDisableTiming));
    }
    LA_RC(refresh_colsums(h, r, stream));
    LaWinGuard win_guard{h->g};
    LA_RC(la_synth_set_row_window(h->g, r.windowed ? h->win_lo : 0, r.windowed ? h->win_hi : 0));
    LA_RC(la_synth_set_col_window(h->g, r.windowed ? h->wcol_lo : 0, r.windowed ? h->wcol_hi : 0));
    if (want_losses && c.steps > 0) LA_HIP(hipMemsetAsync(h->losses, 0, (size_t)c.steps * 4 * sizeof(float), stream));
    LA_RC(run_steps(h, r, plan_schedule(h, r, want_losses), want_losses, stream));
    LA_RC((h->wplus ? la_wplus_gate : la_broadcast_mix)(h->w_opt, w0, w_aug_out, B, h->num_ws, h->wdim, c.alpha, c.soft_aug, stream));
    LA_RC(la_synth_set_row_window(h->g, 0, 0)); LA_RC(la_synth_set_col_window(h->g, 0, 0));      // the augmented image: a whole frame
    LA_RC(la_synth_forward(h->g, w_aug_out, (long)h->num_ws * h->wdim, h->wdim, B, c.final_noise_mode, final_noises, img_out, stream));
    if (want_losses && c.steps > 0) LA_HIP(hipMemcpyAsync(losses_out, h->losses, (size_t)c.steps * 4 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return LA_OK;
}
