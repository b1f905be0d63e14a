// LPIPS-style perceptual feature extractor, forward + backward-to-input, for the criterion
//   calc_loss_lpips_torchscript (augments/utils/util_latent_aug.py:387-409):
//       x = crop[:, mode].repeat(1, 3, 1, 1);  f = vgg16(x, resize_images=False, return_lpips=True);
//       loss_mode = l2_loss_vectorized(f, bank_mode, compute_mean=False).sum() / (n * m) * w_lpips
// The network is a caller-described sequence of { conv3x3 + bias + ReLU | 2x2 max-pool | 2x2 avg-pool | LPIPS tap } ops
// (VGG16: 13 convs, 4 max-pools, taps after conv1_2 / 2_2 / 3_3 / 4_3 / 5_3).  A tap contributes
//       f[n][c][p] * rsqrt(sum_c f^2 + 1e-10) * sqrt(lin[c]) / sqrt(H*W)
// to the output vector, so that squared L2 distance of two vectors is their LPIPS distance.
// Contractions reuse la_conv*.hip (shared weights); pools / taps are small HBM-bound kernels.
// General ops (the AlexNet and SqueezeNet 1.1 trunks of augments/criteria/lpips/networks.py:52-84): a convolution + ReLU with any square
// kernel, stride and padding, a 3x3 stride-2 max pool (floor / ceil mode) and SqueezeNet's Fire module as ONE op -- squeeze, then the
// two expand branches written into the channel slices of one output -- so that the list stays the chain f_trunk and la_feat_backward
// walk.  They run on la_feat_conv.hip in exact fp32 in every precision mode and lower no slot rows: a 3x3 op behind one takes its fp16
// operand scale the way a first conv does.  The resolution is tracked per op (res_in / res_out).
// Detector lists (the `return_features=True` branch of the same net, metrics/metric_utils.py:264-328) end in fully connected ops
// instead of taps: forward only, the feature vector is the last FC's output (la_fc_bias_act_f32, la_detector.hip).
#include "la_feat.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "la_conv.h"
#include "la_feat_conv.h"
#include "la_gram.h"
#include "la_modconv.h"
#include "la_style.h"

#define FEAT_MAX_OPS 48

// One op as the caller describes it: its la_feat_op record with the values of its LA_FEAT_OP_ARGS records (f_parse)
struct FOpDesc { int kind, cin, cout, k, stride, pad, ceil_mode, squeeze, expand1, expand3; };

struct FOp {
    int kind, cin, cout, res_in, res_out;
    const float *w, *bias, *lin;      // w: fc ops and general convs, used in place ([cout][cin], [cout][cin][k][k])
    // general conv: k, stride, pad; 3x3 stride-2 pool: ceil_mode; fire: squeeze / expand channels, cout = expand1 + expand3
    int k, stride, pad, ceil_mode, squeeze, expand1, expand3;
    const float *sq_w, *sq_b, *e1_w, *e1_b, *e3_w, *e3_b;      // fire: the six tensors, used in place
    float* sq_y;       // fire: the squeeze activation [maxN][squeeze][res^2]
    LaConvWeights cw;  // conv ops
    float* y;          // output activation [maxN][cout][res_out^2] (conv, pools, fc: res_out = 1); taps have none
    long feat_off;     // taps: offset of the slice inside the feature vector
};

struct la_feat {
    int nops, in_ch, in_res, maxN, F, precision;
    FOp op[FEAT_MAX_OPS];
    float *gA, *gB;
    float* pm;           // plane maxima of the gradient entering a backward contraction (la_conv_act_grad_pmax: exact-fp32 / fallback path)
    // fp16 operand scales as slot rows lowered by the producing kernels (la_common.h): xs_f [nops][maxN][LA_XS_FAN] for the input of every
    // forward conv but the first, xs_b for the (masked) gradient entering every backward conv; seam_scr: scratch for the demod-gradient
    // partials the fused activation backward of the contraction epilogues writes (unused here: these convs have no demodulation)
    float *xs_f, *xs_b, *seam_scr;
    void* cws; size_t cws_bytes;
    const float* x_in;   // input of the last forward
    int lastN;
    int settings_gen;    // la_feat_settings_gen: raised when the precision changes
    int pass_precision;  // precision of the last forward: what its backward runs in (a setter takes effect at the next forward)
    int detector;        // the list ends in an FC op: forward only, F = the last FC's outputs
    void* fcws; size_t fcws_bytes;      // la_fc_bias_act_f32's workspace (detector lists only)
    // lists with a general conv or a fire op only: the split-K partials of la_featconv_forward, the gradient of a fire's squeeze activation
    float* fcv_part; size_t fcv_part_floats;
    float* fire_g;
};

static inline bool f_is_fc(int kind) { return kind == LA_FEAT_FC_RELU || kind == LA_FEAT_FC; }
// the three convolutions of a fire op and a general conv as la_feat_conv.hip takes them
static inline LaFeatConvGeom f_geom(int cin, int cout, int k, int stride, int pad, int R, int Ro) { return LaFeatConvGeom{cin, cout, k, stride, pad, R, Ro}; }
static inline LaFeatConvGeom f_geom(const FOp& o) { return f_geom(o.cin, o.cout, o.k, o.stride, o.pad, o.res_in, o.res_out); }
static inline LaFeatConvGeom f_fire_sq(const FOp& o) { return f_geom(o.cin, o.squeeze, 1, 1, 0, o.res_in, o.res_in); }
static inline LaFeatConvGeom f_fire_e1(const FOp& o) { return f_geom(o.squeeze, o.expand1, 1, 1, 0, o.res_in, o.res_in); }
static inline LaFeatConvGeom f_fire_e3(const FOp& o) { return f_geom(o.squeeze, o.expand3, 3, 1, 1, o.res_in, o.res_in); }

// refusal with the index of the op that causes it
static int f_refuse(int k, const char* why) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "feat: op %d: %s", k, why);
    la_set_error(msg);
    return LA_ERR_ARG;
}

// min_res: 2 for a list of the six first kinds (as ever), 1 for a list with a general op (a one-pixel input of a general conv)
static int f_describe(la_feat* h, int nops, const FOpDesc* ops, int in_ch, int in_res, int maxN, int min_res) {
    LA_CHECK_ARG(nops >= 1 && nops <= FEAT_MAX_OPS && ops, "feat: bad op list");
    LA_CHECK_ARG(in_ch >= 1 && in_res >= min_res && maxN >= 1, "feat: bad input shape");
    memset(h, 0, sizeof(*h));
    h->nops = nops; h->in_ch = in_ch; h->in_res = in_res; h->maxN = maxN;
    int c = in_ch, r = in_res;
    long F = 0;
    int ntap = 0, nfc = 0, nex = 0;
    for (int k = 0; k < nops; ++k) {
        FOp& o = h->op[k];
        o.kind = ops[k].kind; o.cin = c; o.res_in = r;
        if (nfc) LA_CHECK_ARG(f_is_fc(o.kind), "feat: only fc ops may follow an fc op");
        switch (o.kind) {
            case LA_FEAT_CONV_RELU:
                LA_CHECK_ARG(ops[k].cin == c && ops[k].cout >= 4 && ops[k].cout % 4 == 0, "feat: conv channels mismatch / not a multiple of 4");
                // (the backward pads the gradient of a conv's input to a multiple of 4 channels and copies the real ones out: only into gx)
                LA_CHECK_ARG(c % 4 == 0 || k == 0, "feat: only the first conv may have cin % 4 != 0");
                o.cout = ops[k].cout; o.res_out = r; c = o.cout;
                la_conv_weights_shape(o.cw, o.cin, o.cout, 3); break;
            case LA_FEAT_MAXPOOL2: case LA_FEAT_AVGPOOL2:
                LA_CHECK_ARG(r % 2 == 0, "feat: pooling needs an even resolution");
                o.cout = c; o.res_out = r / 2; r /= 2; break;
            case LA_FEAT_TAP:
                o.cout = c; o.res_out = r; o.feat_off = F; F += (long)c * r * r; ++ntap; break;
            case LA_FEAT_CONV_RELU_EX: {
                const FOpDesc& d = ops[k];
                if (d.cin != c) return f_refuse(k, "conv cin does not match the channels in front of it");
                if (c == 3 && k != 0) return f_refuse(k, "only the first op may have cin = 3");
                const int ro = la_featconv_out_res(c, d.cout, d.k, d.stride, d.pad, r);
                if (ro < 1) return f_refuse(k, "conv refused: k 1..11, stride 1|2|4, pad 0..5 and < k, cout % 4 == 0, cin % 4 == 0 (a first op: 3), resolution >= 1");
                o.cout = d.cout; o.k = d.k; o.stride = d.stride; o.pad = d.pad; o.res_out = ro; c = o.cout; r = ro; ++nex; break;
            }
            case LA_FEAT_MAXPOOL3S2: {
                const int ro = la_pool3s2_out_res(r, ops[k].ceil_mode);
                if (ro < 1) return f_refuse(k, "3x3 stride-2 pool: the resolution in front of it is too small");
                o.cout = c; o.ceil_mode = ops[k].ceil_mode ? 1 : 0; o.res_out = ro; r = ro; break;
            }
            case LA_FEAT_FIRE: {
                const FOpDesc& d = ops[k];
                if (d.cin != c || d.cout != d.expand1 + d.expand3) return f_refuse(k, "fire: cin must match what precedes it and cout = expand1 + expand3");
                if (la_featconv_out_res(c, d.squeeze, 1, 1, 0, r) != r || la_featconv_out_res(d.squeeze, d.expand1, 1, 1, 0, r) != r ||
                    la_featconv_out_res(d.squeeze, d.expand3, 3, 1, 1, r) != r || c == 3)
                    return f_refuse(k, "fire: cin, squeeze, expand1 and expand3 must be positive multiples of 4");
                o.cout = d.cout; o.squeeze = d.squeeze; o.expand1 = d.expand1; o.expand3 = d.expand3; o.res_out = r; c = o.cout; ++nex; break;
            }
            case LA_FEAT_FC_RELU: case LA_FEAT_FC:
                LA_CHECK_ARG(ntap == 0, "feat: taps and fc ops cannot be mixed in one list");
                LA_CHECK_ARG((long)ops[k].cin == (long)c * r * r, "feat: fc cin must be C*res*res of what precedes it");
                LA_CHECK_ARG(ops[k].cout >= 1, "feat: fc needs at least one output");
                o.cin = ops[k].cin; o.cout = ops[k].cout; o.res_out = 1; c = o.cout; r = 1; ++nfc; break;
            default:
                la_set_error("feat: unknown op kind"); return LA_ERR_ARG;
        }
    }
    LA_CHECK_ARG(!(nfc && nex), "feat: a detector list (fc ops) holds no general conv or fire op");
    if (nfc) { h->detector = 1; F = c; }
    LA_CHECK_ARG(F > 0 && F < (1L << 31), "feat: no tap op / feature vector too long");
    h->F = (int)F;
    return LA_OK;
}

static size_t f_layout(la_feat* h, void* ws) {
    LaCarver c{(char*)ws};
    const size_t mn = h->maxN;
    size_t gmax = mn * h->in_ch * (size_t)h->in_res * h->in_res, cw = 0, pmax = 0, part = 0, fire = 0;
    for (int k = 0; k < h->nops; ++k) {
        FOp& o = h->op[k];
        const size_t n_out = mn * o.cout * (size_t)o.res_out * o.res_out;
        if (o.kind == LA_FEAT_CONV_RELU) {
            la_conv_weights_layout(c, o.cw);
            const int cmax = o.cw.cin_pad > o.cout ? o.cw.cin_pad : o.cout;
            size_t w = la_modconv_workspace_bytes((int)mn, cmax, cmax, o.res_in, 0);
            if (w > cw) cw = w;
            const size_t gin = mn * o.cw.cin_pad * (size_t)o.res_in * o.res_in;
            if (gin > gmax) gmax = gin;
            const size_t pmn = mn * o.cout * (size_t)la_conv_act_grad_segments((long)o.res_out * o.res_out);
            if (pmn > pmax) pmax = pmn;
        }
        if (o.kind != LA_FEAT_TAP) { o.y = c.take(n_out); if (n_out > gmax) gmax = n_out; }
        if (o.kind == LA_FEAT_CONV_RELU_EX) { const size_t f = la_featconv_part_floats((int)mn, f_geom(o)); if (f > part) part = f; }
        if (o.kind == LA_FEAT_FIRE) {
            const size_t n_sq = mn * o.squeeze * (size_t)o.res_in * o.res_in;
            o.sq_y = c.take(n_sq);
            if (n_sq > fire) fire = n_sq;
            for (const LaFeatConvGeom& g : {f_fire_sq(o), f_fire_e1(o), f_fire_e3(o)}) { const size_t f = la_featconv_part_floats((int)mn, g); if (f > part) part = f; }
        }
    }
    // (carved only for a list that holds one of the new ops: every other list keeps the bytes it had)
    if (part) { h->fcv_part = c.take(part); h->fcv_part_floats = part; }
    if (fire) h->fire_g = c.take(fire);
    if (h->detector) {      // forward only: no gradient buffers; the FC kernel's K-slice partials instead
        gmax = 0; pmax = 0;
        size_t fb = 0;
        for (int k = 0; k < h->nops; ++k)
            if (f_is_fc(h->op[k].kind)) {
                const size_t b = la_fc_workspace_bytes((long)mn, h->op[k].cin, h->op[k].cout);
                if (b > fb) fb = b;
            }
        h->fcws = c.take((fb + 3) / 4); h->fcws_bytes = fb;
    }
    h->gA = c.take(gmax); h->gB = c.take(gmax);
    h->pm = c.take(pmax);
    h->xs_f = c.take((size_t)h->nops * mn * LA_XS_FAN); h->xs_b = c.take((size_t)h->nops * mn * LA_XS_FAN);
    {
        size_t sc = 16;
        for (int k = 0; k < h->nops; ++k)
            if (h->op[k].kind == LA_FEAT_CONV_RELU) {
                const size_t n = mn * (size_t)h->op[k].cout * la_conv_tiles_per_sample(h->op[k].res_in, h->op[k].res_in);
                if (n > sc) sc = n;
            }
        h->seam_scr = c.take(sc);
    }
    h->cws = c.take((cw + 3) / 4); h->cws_bytes = cw;
    return c.off;
}

static size_t f_workspace_bytes(int nops, const FOpDesc* ops, int in_ch, int in_res, int max_batch, int min_res) {
    return la_measure_workspace<la_feat>([&](la_feat* h) { return f_describe(h, nops, ops, in_ch, in_res, max_batch, min_res) == LA_OK ? f_layout(h, nullptr) : 0; });
}

// params: for each op in order: conv -> weight [cout][cin][k][k], bias [cout]; tap -> lin [C]; pools -> nothing;
// fire -> squeeze weight, bias, expand1x1 weight, bias, expand3x3 weight, bias
static int f_create(int nops, const FOpDesc* ops, const float* const* params, int nparams, int in_ch, int in_res,
                    int max_batch, void* workspace, size_t workspace_bytes, hipStream_t stream, la_feat** out, int min_res) {
    LA_CHECK_ARG(params && workspace && out, "feat_create: null pointer");
    auto own = la_host_handle<la_feat>();
    la_feat* h = own.get();
    LA_CHECK_ARG(h, "feat_create: out of host memory");
    int rc = f_describe(h, nops, ops, in_ch, in_res, max_batch, min_res);
    if (rc) return rc;
    LA_CHECK_WORKSPACE(workspace_bytes, f_layout(h, workspace), "feat_create: workspace too small");
    int p = 0;
    for (int k = 0; k < nops && !rc; ++k) {
        FOp& o = h->op[k];
        if (o.kind == LA_FEAT_CONV_RELU) {
            if (p + 2 > nparams || !params[p] || !params[p + 1]) { rc = LA_ERR_ARG; la_set_error("feat_create: missing conv tensors"); break; }
            o.cw.w = params[p++]; o.bias = params[p++];
            rc = la_conv_weights_pack(o.cw, 1.f, stream);
        } else if (o.kind == LA_FEAT_TAP) {
            if (p + 1 > nparams || !params[p]) { rc = LA_ERR_ARG; la_set_error("feat_create: missing tap weights"); break; }
            o.lin = params[p++];
        } else if (f_is_fc(o.kind)) {      // used in place: weight [cout][cin], bias [cout]
            if (p + 2 > nparams || !params[p] || !params[p + 1]) { rc = LA_ERR_ARG; la_set_error("feat_create: missing fc tensors"); break; }
            o.w = params[p++]; o.bias = params[p++];
        } else if (o.kind == LA_FEAT_CONV_RELU_EX) {      // used in place: weight [cout][cin][k][k], bias [cout]
            if (p + 2 > nparams || !params[p] || !params[p + 1]) { rc = LA_ERR_ARG; la_set_error("feat_create: missing conv tensors"); break; }
            o.w = params[p++]; o.bias = params[p++];
        } else if (o.kind == LA_FEAT_FIRE) {
            bool ok = p + 6 <= nparams;
            for (int q = 0; ok && q < 6; ++q) ok = params[p + q] != nullptr;
            if (!ok) { rc = LA_ERR_ARG; la_set_error("feat_create: missing fire tensors"); break; }
            o.sq_w = params[p]; o.sq_b = params[p + 1]; o.e1_w = params[p + 2]; o.e1_b = params[p + 3]; o.e3_w = params[p + 4]; o.e3_b = params[p + 5];
            p += 6;
        }
    }
    if (!rc && p != nparams) { rc = LA_ERR_ARG; la_set_error("feat_create: parameter list length mismatch"); }
    if (rc) return rc;
    *out = own.release();
    return LA_OK;
}

// The caller's records -> ops.  A record of one of the six first kinds is an op; a general op is its record followed by the
// LA_FEAT_OP_ARGS records that carry what {kind, cin, cout} cannot (include/latentaug_hip.h): conv {k, stride}, {pad, 0}; 3x3 pool
// {ceil_mode, 0}; fire {squeeze, expand1}, {expand3, 0}.  A list without general ops parses to itself.
static int f_parse(int nrec, const la_feat_op* rec, FOpDesc* wide, int* nops, int* min_res) {
    LA_CHECK_ARG(nrec >= 1 && nrec <= 3 * FEAT_MAX_OPS && rec, "feat: bad op list");
    memset(wide, 0, sizeof(FOpDesc) * FEAT_MAX_OPS);
    int n = 0;
    *min_res = 2;      // (a one-pixel input only in front of a general op)
    for (int r = 0; r < nrec; ++n) {
        LA_CHECK_ARG(n < FEAT_MAX_OPS, "feat: bad op list");
        FOpDesc& d = wide[n];
        d.kind = rec[r].kind; d.cin = rec[r].cin; d.cout = rec[r].cout;
        ++r;
        const int nargs = d.kind == LA_FEAT_CONV_RELU_EX || d.kind == LA_FEAT_FIRE ? 2 : d.kind == LA_FEAT_MAXPOOL3S2 ? 1 : 0;
        if (nargs == 0) {
            LA_CHECK_ARG(d.kind >= LA_FEAT_CONV_RELU && d.kind <= LA_FEAT_FC, d.kind == LA_FEAT_OP_ARGS ? "feat: argument record without its op" : "feat: unknown op kind");
            continue;
        }
        *min_res = 1;
        int v[4] = {0, 0, 0, 0};
        for (int q = 0; q < nargs; ++q, ++r) {
            if (r >= nrec || rec[r].kind != LA_FEAT_OP_ARGS) return f_refuse(n, "the op's argument records are missing");
            v[2 * q] = rec[r].cin; v[2 * q + 1] = rec[r].cout;
        }
        if (d.kind == LA_FEAT_CONV_RELU_EX) { d.k = v[0]; d.stride = v[1]; d.pad = v[2]; }
        else if (d.kind == LA_FEAT_MAXPOOL3S2) d.ceil_mode = v[0];
        else { d.squeeze = v[0]; d.expand1 = v[1]; d.expand3 = v[2]; }
    }
    *nops = n;
    return LA_OK;
}
extern "C" size_t la_feat_workspace_bytes(int nops, const la_feat_op* ops, int in_ch, int in_res, int max_batch) {
    FOpDesc wide[FEAT_MAX_OPS];
    int n, min_res;
    return f_parse(nops, ops, wide, &n, &min_res) == LA_OK ? f_workspace_bytes(n, wide, in_ch, in_res, max_batch, min_res) : 0;
}
extern "C" int la_feat_create(int nops, const la_feat_op* ops, const float* const* params, int nparams, int in_ch, int in_res,
                              int max_batch, void* workspace, size_t workspace_bytes, hipStream_t stream, la_feat** out) {
    FOpDesc wide[FEAT_MAX_OPS];
    int n, min_res;
    const int rc = f_parse(nops, ops, wide, &n, &min_res);
    return rc ? rc : f_create(n, wide, params, nparams, in_ch, in_res, max_batch, workspace, workspace_bytes, stream, out, min_res);
}

extern "C" void la_feat_destroy(la_feat* h) { free(h); }
extern "C" int la_feat_num_features(const la_feat* h) { return h ? h->F : 0; }
extern "C" int la_feat_set_precision(la_feat* h, int precision) {
    LA_CHECK_ARG(h && precision >= 0 && precision <= 3, "feat_set_precision: precision must be 0..3");
    if (precision != h->precision) ++h->settings_gen;
    h->precision = precision;
    return LA_OK;
}
int la_feat_settings_gen(const la_feat* h) { return h->settings_gen; }

// ------------------------------------------------------------------------------------------------------------
__global__ void la_pool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int R, long planes, int is_max) {
    const int Ro = R / 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= planes * Ro * Ro) return;
    const int ox = (int)(i % Ro), oy = (int)((i / Ro) % Ro);
    const long pl = i / ((long)Ro * Ro);
    const float* p = x + (pl * R + 2 * oy) * R + 2 * ox;
    const float a = p[0], b = p[1], c = p[R], d = p[R + 1];
    y[i] = is_max ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : 0.25f * ((a + b) + (c + d));
}

// max: the gradient goes to the first maximum in scan order (torch semantics); avg: a quarter to each
__global__ void la_pool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, int R,
                                    long planes, int is_max) {
    const int Ro = R / 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= planes * Ro * Ro) return;
    const int ox = (int)(i % Ro), oy = (int)((i / Ro) % Ro);
    const long pl = i / ((long)Ro * Ro);
    const long base = (pl * R + 2 * oy) * R + 2 * ox;
    const float g = gy[i];
    if (!is_max) {
        const float q = 0.25f * g;
        gx[base] = q; gx[base + 1] = q; gx[base + R] = q; gx[base + R + 1] = q;
        return;
    }
    const float v[4] = {x[base], x[base + 1], x[base + R], x[base + R + 1]};
    int am = 0;
    for (int k = 1; k < 4; ++k) if (v[k] > v[am]) am = k;
    gx[base] = am == 0 ? g : 0.f; gx[base + 1] = am == 1 ? g : 0.f; gx[base + R] = am == 2 ? g : 0.f; gx[base + R + 1] = am == 3 ? g : 0.f;
}

// tap forward: feat[n][off + c*HW + p] = f * rsqrt(sum_c f^2 + 1e-10) * sqrt(lin[c]) / sqrt(HW)
// Workgroup = PL pixel lanes (consecutive pixels: coalesced) x 256 / PL channel groups of one image; every thread walks C / groups
// channels, the channel sums are combined through LDS in a fixed order.  (Round 1 ran one thread per pixel over all C channels:
// 16 threads walking 512 channels three times at the 4x4 tap of VGG16, 555 us.)
__global__ __launch_bounds__(256) void la_tap_fwd_kernel(const float* __restrict__ f, const float* __restrict__ lin, float* __restrict__ feat, int C,
                                                          int HW, long F, long off, int PL) {
    __shared__ float red[256];
    const int pl = threadIdx.x % PL, cg = threadIdx.x / PL, CG = 256 / PL;
    const int p = blockIdx.x * PL + pl;
    const long n = blockIdx.y;
    const bool ok = p < HW;
    const float* fp = f + n * C * HW + p;
    // (eight channel loads in flight per thread, summed in the channel order of the plain loop: at the 4x4 / 8x8 taps a thread walks
    //  32 - 128 channels and the loop was one exposed load latency per channel, 40 - 60 us for 16 workgroups)
    float s = 0.f;
    if (ok) {
        int c = cg;
        for (; c + 7 * CG < C; c += 8 * CG) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fp[(long)(c + k * CG) * HW];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k] * v[k];
        }
        for (; c < C; c += CG) { const float v = fp[(long)c * HW]; s += v * v; }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    float tot = 0.f;
    for (int g = 0; g < CG; ++g) tot += red[g * PL + pl];
    const float r = rsqrtf(tot + 1e-10f) * rsqrtf((float)HW);
    if (!ok) return;
    float* o = feat + n * F + off + p;
    int c = cg;
    for (; c + 7 * CG < C; c += 8 * CG) {
        float v[8], w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = fp[(long)(c + k * CG) * HW]; w[k] = lin[c + k * CG]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) o[(long)(c + k * CG) * HW] = v[k] * r * sqrtf(w[k]);
    }
    for (; c < C; c += CG) o[(long)c * HW] = fp[(long)c * HW] * r * sqrtf(lin[c]);
}

// tap backward: gf[k] (+)= r * (u_k - y_k * sum_c u_c y_c),  u_c = g_c * sqrt(lin_c)/sqrt(HW),  y_c = f_c * r   (same thread layout)
// mask != 0: the tapped activation is the ReLU output of the conv in front of the tap, and the result is the gradient entering that
// conv's backward contraction: the ReLU mask (f > 0) is applied to the SUM (incoming gradient + this tap's) here, and xs_row (slot rows
// [N][LA_XS_FAN], la_common.h) receives the fp16 operand scale of the result -- no separate activation-backward / plane-maxima sweep.
__global__ __launch_bounds__(256) void la_tap_bwd_kernel(const float* __restrict__ f, const float* __restrict__ lin, const float* __restrict__ gfeat,
                                                          float* __restrict__ gf, int C, int HW, long F, long off, int PL, int accumulate, int mask,
                                                          float* __restrict__ xs_row) {
    __shared__ float red[2][256];
    const int pl = threadIdx.x % PL, cg = threadIdx.x / PL, CG = 256 / PL;
    const int p = blockIdx.x * PL + pl;
    const long n = blockIdx.y;
    const bool ok = p < HW;
    const float* fp = f + n * C * HW + p;
    const float* gp = gfeat + n * F + off + p;
    const float a = rsqrtf((float)HW);
    float s = 0.f, d = 0.f;                       // sum f^2 and sum u_c f_c of this thread's channels
    if (ok) {
        int c = cg;
        for (; c + 7 * CG < C; c += 8 * CG) {      // (eight channels' loads in flight, summed in channel order: see la_tap_fwd_kernel)
            float v[8], g[8], w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] = fp[(long)(c + k * CG) * HW]; g[k] = gp[(long)(c + k * CG) * HW]; w[k] = lin[c + k * CG]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s += v[k] * v[k]; d += g[k] * sqrtf(w[k]) * a * v[k]; }
        }
        for (; c < C; c += CG) {
            const float v = fp[(long)c * HW];
            s += v * v;
            d += gp[(long)c * HW] * sqrtf(lin[c]) * a * v;
        }
    }
    red[0][threadIdx.x] = s; red[1][threadIdx.x] = d;
    __syncthreads();
    float st = 0.f, dt = 0.f;
    for (int g = 0; g < CG; ++g) { st += red[0][g * PL + pl]; dt += red[1][g * PL + pl]; }
    const float r = rsqrtf(st + 1e-10f);
    const float dot = dt * r;                      // sum_c u_c y_c
    float omax = 0.f;
    if (ok) {
        float* op = gf + n * C * HW + p;
        int c = cg;
        for (; c + 7 * CG < C; c += 8 * CG) {
            float fv[8], g[8], w[8], prev[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                fv[k] = fp[(long)(c + k * CG) * HW]; g[k] = gp[(long)(c + k * CG) * HW]; w[k] = lin[c + k * CG];
                prev[k] = accumulate ? op[(long)(c + k * CG) * HW] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float u = g[k] * sqrtf(w[k]) * a, y = fv[k] * r;
                float v = r * (u - y * dot);
                if (accumulate) v += prev[k];
                if (mask && !(fv[k] > 0.f)) v = 0.f;
                op[(long)(c + k * CG) * HW] = v;
                omax = fmaxf(omax, fabsf(v));
            }
        }
        for (; c < C; c += CG) {
            const float fv = fp[(long)c * HW];
            const float u = gp[(long)c * HW] * sqrtf(lin[c]) * a, y = fv * r;
            float v = r * (u - y * dot);
            if (accumulate) v += op[(long)c * HW];
            if (mask && !(fv > 0.f)) v = 0.f;
            op[(long)c * HW] = v;
            omax = fmaxf(omax, fabsf(v));
        }
    }
    // (uniform) this workgroup's maximum lowers a sub-slot of sample n's row
    if (xs_row) la_xs_lower_wg(xs_row, n, 1.f, la_block_max_256(omax, red[0]));
}

// pixel lanes of a tap workgroup: the largest power of two <= min(64, HW)
static inline int tap_lanes(int HW) { int pl = 1; while (pl * 2 <= HW && pl < 64) pl *= 2; return pl; }

// What the launch of a conv op starts from: its weights of the direction, arithmetic, scratch, the 3x3 geometry at its resolution and
// the bias + ReLU epilogue (backward: plain).  The callers name the tensors and the slot-row hand-over of the fp16 operand scales
// (f16x2 mode): acc_scale_x = rows of the launch's input (none: absmax / plane-maxima passes), fwd_xs_out = rows the epilogue lowers
// for the next conv.
static void f_conv(LaConvArgs& a, const la_feat* h, const FOp& o, bool backward, int N) {
    la_conv_args_init(a);
    la_conv_weights_select(a, o.cw, backward);
    a.precision = backward ? h->pass_precision : h->precision; a.ws = h->cws; a.ws_bytes = h->cws_bytes; a.B = N;
    la_conv_geom_same(a, o.res_in, 3, backward);
    if (backward) a.epi = LA_EPI_BWD;
    else la_conv_set_epi(a, LaLayerEpi{nullptr, 0, nullptr, 0, 0.f, o.bias, LA_ACT_RELU, 0.f, 1.f, -1.f});
}
// Backward launch: the activation backward of the conv below, fused -- its saved ReLU output mask_y is the epilogue's xin, the
// epilogue applies that ReLU's mask to the outgoing gradient and lowers the slot rows xs_out of that conv's contraction (LaConvArgs::seam)
static void f_relu_seam(LaConvArgs& a, const la_feat* h, const float* mask_y, float* xs_out) {
    a.xin = mask_y; a.xin_bstride = (long)a.M * a.Gy * a.Gx; a.tiles_per_sample = la_conv_tiles_per_sample(a.Gy, a.Gx);
    a.seam.ddn_part = h->seam_scr; a.seam.act = LA_ACT_RELU; a.seam.alpha = 0.f; a.seam.gain = 1.f; a.seam.clamp = -1.f;
    a.seam.xs_out = xs_out; a.seam.xs_mult = 1.f;
}

// fp16 x2 mode: operand scales as slot rows lowered by the producing kernels; decided once per call (dev knob LA_NO_FEAT_SLOTS: the round-3 passes)
static bool f_slots(const la_feat* h, bool backward) { return (backward ? h->pass_precision : h->precision) == LA_PREC_F16X2 && !la_dev_env("LA_NO_FEAT_SLOTS"); }
static float* f_rows(const la_feat* h, float* base, int op) { return base + (size_t)op * h->maxN * LA_XS_FAN; }

// The trunk on N rows of x: resets the forward slot rows, walks the op list with the conv, pool and fc launches and hands every tap op, with
// the activation it taps and its pixel count, to `tap`.  fc_out: where the last fc op of a detector list writes (no other caller has fc ops).
// fp16 x2 mode: every conv's epilogue lowers the slot rows of the NEXT conv's operand scale (a pool in between only shrinks the maximum;
// taps do not touch the activation), so only the first conv -- whose input no kernel of this engine produces -- runs the absmax / scale passes
template <class Tap>
static int f_trunk(la_feat* h, const float* x, int N, float* fc_out, hipStream_t stream, Tap tap) {
    const float* cur = x;
    int rc;
    const bool slots = f_slots(h, false);
    if (slots) LA_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->xs_f), (int)LA_XS_INIT, (size_t)h->nops * h->maxN * LA_XS_FAN, stream));
    bool first_conv = true;
    for (int k = 0; k < h->nops; ++k) {
        FOp& o = h->op[k];
        const int HWo = o.res_out * o.res_out;
        if (o.kind == LA_FEAT_CONV_RELU) {
            int nxt = -1;
            for (int q = k + 1; q < h->nops; ++q) if (h->op[q].kind == LA_FEAT_CONV_RELU) { nxt = q; break; }
            LaConvArgs a; f_conv(a, h, o, false, N);
            a.in = cur; a.out = o.y;
            if (slots && !first_conv) { a.acc_scale_x = f_rows(h, h->xs_f, k); a.acc_scale_fan = LA_XS_FAN; }
            if (slots && nxt >= 0) a.fwd_xs_out = f_rows(h, h->xs_f, nxt);
            if ((rc = la_conv_launch(a, stream))) return rc;
            first_conv = false;
            cur = o.y;
        } else if (o.kind == LA_FEAT_TAP) {
            tap(o, cur, HWo);
        } else if (f_is_fc(o.kind)) {
            // the activation in front is [N][C][res][res] contiguous: torch's flatten is a reinterpretation; the last FC writes the features
            float* dst = k == h->nops - 1 ? fc_out : o.y;
            if ((rc = la_fc_bias_act_f32(cur, o.w, o.bias, dst, N, o.cin, o.cout, o.kind == LA_FEAT_FC_RELU ? LA_ACT_RELU : LA_ACT_LINEAR, h->fcws,
                                         h->fcws_bytes, stream)))
                return rc;
            cur = dst;
        } else if (o.kind == LA_FEAT_CONV_RELU_EX) {
            if ((rc = la_featconv_forward(cur, o.w, o.bias, o.y, N, f_geom(o), 0, o.cout, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            cur = o.y;
            first_conv = true;      // (no slot rows from this producer: a 3x3 op behind it takes its operand scale as a first conv does)
        } else if (o.kind == LA_FEAT_FIRE) {
            // squeeze, then the two expand branches into the channel slices [0, expand1) and [expand1, cout) of one output: torch.cat without a copy
            if ((rc = la_featconv_forward(cur, o.sq_w, o.sq_b, o.sq_y, N, f_fire_sq(o), 0, o.squeeze, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            if ((rc = la_featconv_forward(o.sq_y, o.e1_w, o.e1_b, o.y, N, f_fire_e1(o), 0, o.cout, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            if ((rc = la_featconv_forward(o.sq_y, o.e3_w, o.e3_b, o.y, N, f_fire_e3(o), o.expand1, o.cout, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            cur = o.y;
            first_conv = true;
        } else if (o.kind == LA_FEAT_MAXPOOL3S2) {
            if ((rc = la_pool3s2_forward(cur, o.y, (long)N * o.cout, o.res_in, o.res_out, stream))) return rc;
            cur = o.y;
        } else {
            const long planes = (long)N * o.cout;
            hipLaunchKernelGGL(la_pool2_fwd_kernel, dim3(la_cdiv(planes * HWo, 256)), dim3(256), 0, stream, cur, o.y, o.res_in, planes,
                               o.kind == LA_FEAT_MAXPOOL2);
            cur = o.y;
        }
    }
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_feat_forward(la_feat* h, const float* x, int N, float* feat_out, hipStream_t stream) {
    LA_CHECK_ARG(h && x && feat_out, "feat_forward: null pointer");
    LA_CHECK_ARG(N >= 1 && N <= h->maxN, "feat_forward: batch exceeds max_batch");
    const int rc = f_trunk(h, x, N, feat_out, stream, [&](const FOp& o, const float* cur, int HWo) {
        const int pl = tap_lanes(HWo);
        hipLaunchKernelGGL(la_tap_fwd_kernel, dim3(la_cdiv(HWo, pl), N), dim3(256), 0, stream, cur, o.lin, feat_out, o.cout, HWo, (long)h->F, o.feat_off, pl);
    });
    if (rc) return rc;
    h->x_in = x; h->lastN = N; h->pass_precision = h->precision;
    return LA_OK;
}

// gx [N][in_ch][in_res^2] = d(sum gfeat . feat)/dx for the last forward (x must still hold the forward's input)
extern "C" int la_feat_backward(la_feat* h, const float* gfeat, float* gx, hipStream_t stream) {
    LA_CHECK_ARG(h && gfeat && gx && h->lastN >= 1, "feat_backward: null pointer / no forward pass");
    LA_CHECK_ARG(!h->detector, "feat_backward: a detector list (fc ops) is forward only");
    const int N = h->lastN;
    float* g = h->gA;       // gradient w.r.t. the activation that op k produced / tapped
    float* other = h->gB;
    bool have = false;
    int rc;
    // fp16 x2 mode: the ReLU mask of conv k and the operand scale of the masked gradient come from the kernel that WRITES that gradient
    // last -- the tap behind conv k (la_tap_bwd_kernel, mask fused), or the backward contraction of conv k+1 when it follows directly
    // (its epilogue applies the mask of its xin = y_k, LaConvArgs::seam) -- instead of an activation-backward sweep with plane maxima
    // and a scale-reduction launch per conv.  `masked`: g already carries op k's mask and its slot rows are final.
    const bool slots = f_slots(h, true);
    if (slots) LA_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->xs_b), (int)LA_XS_INIT, (size_t)h->nops * h->maxN * LA_XS_FAN, stream));
    auto rows = [&](float* base, int op) { return f_rows(h, base, op); };
    bool masked = false;
    for (int k = h->nops - 1; k >= 0; --k) {
        FOp& o = h->op[k];
        // activation feeding op k
        const float* act_in = h->x_in;
        for (int q = k - 1; q >= 0; --q) if (h->op[q].kind != LA_FEAT_TAP) { act_in = h->op[q].y; break; }
        const int HWo = o.res_out * o.res_out;
        if (o.kind == LA_FEAT_TAP) {
            const int pl = tap_lanes(HWo);
            // (the tap's input is the output of the conv right in front of it: this launch is the last writer of that conv's gradient)
            const bool fuse = slots && k > 0 && h->op[k - 1].kind == LA_FEAT_CONV_RELU;
            hipLaunchKernelGGL(la_tap_bwd_kernel, dim3(la_cdiv(HWo, pl), N), dim3(256), 0, stream, act_in, o.lin, gfeat, g, o.cout, HWo,
                               (long)h->F, o.feat_off, pl, have ? 1 : 0, fuse ? 1 : 0, fuse ? rows(h->xs_b, k - 1) : (float*)nullptr);
            have = true;
            masked = fuse;
        } else if (o.kind == LA_FEAT_CONV_RELU) {
            LA_CHECK_ARG(have, "feat_backward: the op list must end with a tap");
            float* dst = (k == 0 && o.cw.cin_pad == o.cin) ? gx : other;
            // the conv below, if it feeds this one directly: this contraction's epilogue masks its gradient and lowers its slot rows
            const bool below = slots && k > 0 && h->op[k - 1].kind == LA_FEAT_CONV_RELU && o.cw.cin_pad == o.cin && dst != gx;
            LaConvArgs a; f_conv(a, h, o, true, N);
            a.in = g; a.out = dst;
            if (masked) { a.acc_scale_x = rows(h->xs_b, k); a.acc_scale_fan = LA_XS_FAN; }
            else {
                // ReLU mask of this layer on the incoming gradient, with the plane maxima the fp16 operand scale of its backward
                // contraction needs (one sweep instead of a mask pass + an absmax pass): exact-fp32 / bf16 modes, op lists without
                // a tap or a conv right behind this conv
                if ((rc = la_conv_act_grad_pmax(g, o.y, g, h->pm, N, o.cout, HWo, LA_ACT_RELU, 0.f, 1.f, -1.f, stream))) return rc;
                a.in_pmax = h->pm; a.in_pmax_nseg = la_conv_act_grad_segments(HWo);
            }
            if (below) f_relu_seam(a, h, h->op[k - 1].y, rows(h->xs_b, k - 1));
            if ((rc = la_conv_launch(a, stream))) return rc;
            masked = below;
            if (k == 0 && dst != gx) {
                // padded backward channels (cin not a multiple of 4): copy the real ones out
                const long HWi = (long)o.res_in * o.res_in;
                // (one strided copy: a copy per sample was 16 launches of 5 us each in every step of preset E)
                LA_HIP(hipMemcpy2DAsync(gx, sizeof(float) * o.cin * HWi, dst, sizeof(float) * o.cw.cin_pad * HWi, sizeof(float) * o.cin * HWi, (size_t)N,
                                        hipMemcpyDeviceToDevice, stream));
            }
            float* t = g; g = other; other = t;
        } else if (o.kind == LA_FEAT_CONV_RELU_EX || o.kind == LA_FEAT_FIRE || o.kind == LA_FEAT_MAXPOOL3S2) {
            LA_CHECK_ARG(have, "feat_backward: the op list must end with a tap");
            float* dst = k == 0 ? gx : other;      // (a first op writes gx [N][in_ch][in_res^2] itself)
            if (o.kind == LA_FEAT_CONV_RELU_EX) {
                // (the ReLU mask of this layer is applied to g on load, from its saved output)
                if ((rc = la_featconv_backward(g, o.y, o.w, dst, N, f_geom(o), 0, o.cout, 0, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            } else if (o.kind == LA_FEAT_FIRE) {
                // expand3x3 gradient, expand1x1 gradient added to it (both masked by their slice of y), then the squeeze mask and gradient
                if ((rc = la_featconv_backward(g, o.y, o.e3_w, h->fire_g, N, f_fire_e3(o), o.expand1, o.cout, 0, h->fcv_part, h->fcv_part_floats, stream))) return rc;
                if ((rc = la_featconv_backward(g, o.y, o.e1_w, h->fire_g, N, f_fire_e1(o), 0, o.cout, 1, h->fcv_part, h->fcv_part_floats, stream))) return rc;
                if ((rc = la_featconv_backward(h->fire_g, o.sq_y, o.sq_w, dst, N, f_fire_sq(o), 0, o.squeeze, 0, h->fcv_part, h->fcv_part_floats, stream))) return rc;
            } else {
                if ((rc = la_pool3s2_backward(act_in, g, dst, (long)N * o.cout, o.res_in, o.res_out, stream))) return rc;
            }
            float* t = g; g = other; other = t;
            masked = false;
        } else {
            LA_CHECK_ARG(have, "feat_backward: the op list must end with a tap");
            const long planes = (long)N * o.cout;
            hipLaunchKernelGGL(la_pool2_bwd_kernel, dim3(la_cdiv(planes * HWo, 256)), dim3(256), 0, stream, act_in, g, other, o.res_in,
                               planes, o.kind == LA_FEAT_MAXPOOL2);
            float* t = g; g = other; other = t;
            masked = false;
        }
    }
    LA_CHECK_LAUNCH();
    if (h->op[0].kind == LA_FEAT_TAP || h->op[0].kind == LA_FEAT_MAXPOOL2 || h->op[0].kind == LA_FEAT_AVGPOOL2) {
        // the gradient ended in g (no first conv, fire or 3x3 pool wrote gx)
        const long n_in = (long)N * h->in_ch * h->in_res * h->in_res;
        LA_HIP(hipMemcpyAsync(gx, g, sizeof(float) * n_in, hipMemcpyDeviceToDevice, stream));
    }
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// LPIPS distance of image pairs: rows p and p + P of one 2P batch, one launch per tap and no feature vector in memory.
//       part[p][tap][tile] = sum over the tile's pixels and all channels of lin[c] * (fx * rx - fy * ry)^2,   r = rsqrt(sum_c f^2 + 1e-10)
// Thread layout of la_tap_fwd_kernel (PL pixel lanes x 256 / PL channel groups; pass 1 sums each thread's channels in the same order,
// so r is the tap's).  Pass 2 takes DIFFERENCES of the normalised values -- the images of a pair are close, the expanded form
// |x|^2 + |y|^2 - 2 x.y cancels -- with contraction off: a fused fx * rx - (fy * ry) would round one product and not the other, and
// d(x, x) = 0, d(x, y) = d(y, x) would no longer hold bit for bit.  lin enters as it is (no sqrt: a negative weight is legal here).
// KEEP > 0: a thread's ceil(C / groups) <= KEEP channels of both images stay in registers between the passes; KEEP = 0 reads them again.
// One float64 partial per workgroup, combined in a fixed order: no atomics, two runs give the same bits.
template <int KEEP>
__global__ __launch_bounds__(256) void la_tap_pair_dist_kernel(const float* __restrict__ f, const float* __restrict__ lin, double* __restrict__ part,
                                                                int C, int HW, int P, int PL, long part_stride, long part_off) {
    __shared__ float red[2][256];
    __shared__ double dred[256];
    const int pl = threadIdx.x % PL, cg = threadIdx.x / PL, CG = 256 / PL;
    const int p = blockIdx.x * PL + pl;
    const long n = blockIdx.y;
    const bool ok = p < HW;
    const float* fx = f + n * C * HW + p;
    const float* fy = f + (n + P) * C * HW + p;
    float vx[KEEP ? KEEP : 1], vy[KEEP ? KEEP : 1];
    float sx = 0.f, sy = 0.f;
    if (ok) {
        if constexpr (KEEP > 0) {
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                const int c = cg + k * CG;
                vx[k] = c < C ? fx[(long)c * HW] : 0.f;
                vy[k] = c < C ? fy[(long)c * HW] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < KEEP; ++k) { sx += vx[k] * vx[k]; sy += vy[k] * vy[k]; }
        } else {
            int c = cg;
            for (; c + 7 * CG < C; c += 8 * CG) {      // (eight channels' loads of each image in flight: see la_tap_fwd_kernel)
                float a[8], b[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { a[k] = fx[(long)(c + k * CG) * HW]; b[k] = fy[(long)(c + k * CG) * HW]; }
#pragma unroll
                for (int k = 0; k < 8; ++k) { sx += a[k] * a[k]; sy += b[k] * b[k]; }
            }
            for (; c < C; c += CG) { const float a = fx[(long)c * HW], b = fy[(long)c * HW]; sx += a * a; sy += b * b; }
        }
    }
    red[0][threadIdx.x] = sx; red[1][threadIdx.x] = sy;
    __syncthreads();
    float tx = 0.f, ty = 0.f;
    for (int g = 0; g < CG; ++g) { tx += red[0][g * PL + pl]; ty += red[1][g * PL + pl]; }
    const float rx = rsqrtf(tx + 1e-10f), ry = rsqrtf(ty + 1e-10f);
    double acc = 0.0;
    if (ok) {
#pragma clang fp contract(off)
        if constexpr (KEEP > 0) {
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                const int c = cg + k * CG;
                const float w = c < C ? lin[c] : 0.f;
                const float ax = vx[k] * rx, ay = vy[k] * ry;
                const float d = ax - ay;
                acc += (double)(w * (d * d));
            }
        } else {
            int c = cg;
            for (; c + 7 * CG < C; c += 8 * CG) {
                float a[8], b[8], w[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { a[k] = fx[(long)(c + k * CG) * HW]; b[k] = fy[(long)(c + k * CG) * HW]; w[k] = lin[c + k * CG]; }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float ax = a[k] * rx, ay = b[k] * ry;
                    const float d = ax - ay;
                    acc += (double)(w[k] * (d * d));
                }
            }
            for (; c < C; c += CG) {
                const float ax = fx[(long)c * HW] * rx, ay = fy[(long)c * HW] * ry;
                const float d = ax - ay;
                acc += (double)(lin[c] * (d * d));
            }
        }
    }
    dred[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) dred[threadIdx.x] += dred[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[n * part_stride + part_off + blockIdx.x] = dred[0];
}

// dist[p][tap] = (sum of the tap's tiles, in order) / HW.  One 64-thread workgroup per (tap, pair): thread i adds tiles i, i + 64, ..
struct LaPairTaps { int n, tiles_max; int tiles[FEAT_MAX_OPS], hw[FEAT_MAX_OPS]; };
__global__ __launch_bounds__(64) void la_pair_dist_finish_kernel(const double* __restrict__ part, double* __restrict__ dist, LaPairTaps t) {
    __shared__ double red[64];
    const int tap = blockIdx.x;
    const long p = blockIdx.y;
    const double* src = part + (p * t.n + tap) * t.tiles_max;
    double s = 0.0;
    for (int i = threadIdx.x; i < t.tiles[tap]; i += 64) s += src[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int g = 0; g < 64; ++g) tot += red[g];
        dist[p * t.n + tap] = tot / (double)t.hw[tap];
    }
}

// channels of BOTH images a thread of the pair kernel keeps in registers: 32 or 64 each where its share of the tap fits, else none
static inline int pair_keep(int C, int HW) {
    const int per = la_cdiv(C, 256 / tap_lanes(HW));
    return per <= 32 ? 32 : per <= 64 ? 64 : 0;
}

static void pair_taps(const la_feat* h, LaPairTaps& t) {
    t.n = 0; t.tiles_max = 1;
    for (int k = 0; k < h->nops; ++k)
        if (h->op[k].kind == LA_FEAT_TAP) {
            const int HW = h->op[k].res_out * h->op[k].res_out;
            t.hw[t.n] = HW; t.tiles[t.n] = la_cdiv(HW, tap_lanes(HW));
            if (t.tiles[t.n] > t.tiles_max) t.tiles_max = t.tiles[t.n];
            ++t.n;
        }
}

extern "C" int la_feat_num_taps(const la_feat* h) {
    if (!h || h->detector) return 0;
    LaPairTaps t; pair_taps(h, t);
    return t.n;
}

// the float64 partials [P][ntaps][tiles of the largest tap]; 0: no handle, a detector list, or 2P outside 2 .. max_batch
extern "C" size_t la_feat_pair_workspace_bytes(const la_feat* h, int P) {
    if (!h || h->detector || P < 1 || 2L * P > h->maxN) return 0;
    LaPairTaps t; pair_taps(h, t);
    return la_align64(sizeof(double) * (size_t)P * t.n * t.tiles_max);
}

// dist [P][ntaps] (float64) = per tap, the LPIPS distance of rows p and p + P of xy [2P][in_ch][in_res^2]: the trunk (f_trunk) once on the
// 2P rows, the pair kernel as its tap step.  No host sync, no allocation.  The activations of an earlier la_feat_forward are overwritten:
// la_feat_backward refuses until the next forward.
extern "C" int la_feat_pair_distance(la_feat* h, const float* xy, int P, double* dist, void* ws, size_t ws_bytes, hipStream_t stream) {
    LA_CHECK_ARG(h && xy && dist && ws, "feat_pair_distance: null pointer");
    LA_CHECK_ARG(!h->detector, "feat_pair_distance: a detector list (fc ops) has no taps");
    LA_CHECK_ARG(P >= 1 && 2L * P <= h->maxN, "feat_pair_distance: 2 * pairs exceeds max_batch");
    LA_CHECK_WORKSPACE(ws_bytes, la_feat_pair_workspace_bytes(h, P), "feat_pair_distance: workspace too small");
    LaPairTaps t; pair_taps(h, t);
    int tap = 0;
    h->lastN = 0;
    const int rc = f_trunk(h, xy, 2 * P, nullptr, stream, [&](const FOp& o, const float* cur, int HWo) {
        const int pl = tap_lanes(HWo), keep = pair_keep(o.cout, HWo);
        auto kern = keep == 32 ? la_tap_pair_dist_kernel<32> : keep == 64 ? la_tap_pair_dist_kernel<64> : la_tap_pair_dist_kernel<0>;
        hipLaunchKernelGGL(kern, dim3(t.tiles[tap], P), dim3(256), 0, stream, cur, o.lin, (double*)ws, o.cout, HWo, P, pl,
                           (long)t.n * t.tiles_max, (long)tap * t.tiles_max);
        ++tap;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(la_pair_dist_finish_kernel, dim3(t.n, P), dim3(64), 0, stream, (const double*)ws, dist, t);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Gram-matrix style and content distance of image pairs (NSTLoss on the taps of VGG19Net, augments/criteria/nst): the trunk once on the
// 2P rows, la_gram_pair_launch (la_gram.hip) as its tap step on the raw activation each tap sees; `lin` is not read.  The scratch is
// the largest tap's, used by one tap after the other on the one stream.
extern "C" size_t la_feat_style_scratch_bytes(const la_feat* h, int P) {
    if (!h || h->detector || P < 1 || 2L * P > h->maxN) return 0;
    size_t need = 0;
    for (int k = 0; k < h->nops; ++k)
        if (h->op[k].kind == LA_FEAT_TAP) {
            const size_t b = la_gram_pair_scratch_bytes(P, h->op[k].cout, h->op[k].res_out * h->op[k].res_out);
            if (b == 0) return 0;
            if (b > need) need = b;
        }
    return need;
}

// style, content [P][ntaps] (float64): per tap, the distances of rows p and p + P of xy [2P][in_ch][in_res^2].  No host sync, no
// allocation.  The activations of an earlier la_feat_forward are overwritten: la_feat_backward refuses until the next forward.
extern "C" int la_feat_style_distance(la_feat* h, const float* xy, int P, double* style, double* content, void* scratch, size_t scratch_bytes,
                                      hipStream_t stream) {
    LA_CHECK_ARG(h && xy && style && content && scratch, "feat_style_distance: null pointer");
    LA_CHECK_ARG(!h->detector, "feat_style_distance: a detector list (fc ops) has no taps");
    LA_CHECK_ARG(P >= 1 && 2L * P <= h->maxN, "feat_style_distance: 2 * pairs exceeds max_batch");
    const size_t need = la_feat_style_scratch_bytes(h, P);
    LA_CHECK_ARG(need > 0, "feat_style_distance: a tap's shape is refused by la_gram_pair_scratch_bytes");
    LA_CHECK_WORKSPACE(scratch_bytes, need, "feat_style_distance: scratch smaller than la_feat_style_scratch_bytes(h, P)");
    LA_CHECK_ARG(la_aligned<8>(scratch), "feat_style_distance: the scratch must be 8-byte aligned");
    const int ntaps = la_feat_num_taps(h);
    int tap = 0, trc = LA_OK;
    h->lastN = 0;
    const int rc = f_trunk(h, xy, 2 * P, nullptr, stream, [&](const FOp& o, const float* cur, int HWo) {
        if (!trc) trc = la_gram_pair_launch(cur, P, o.cout, HWo, style + tap, content + tap, ntaps, scratch, stream);
        ++tap;
    });
    return rc ? rc : trc;
}

// ------------------------------------------------------------------------------------------------------------
// criterion glue: crop (+ repeat to 3 channels, affine preprocess) and its adjoint
//   xc[(c*B + b)][k][y][x] = img[b][c][y0+y][x0+x] * scale + shift      k = 0..rep-1
// (pos != null: the window position {y0, x0} is read from device memory, so that a captured launch follows the position the
//  host draws per forward)
struct LaPreAffine { float scale[4], shift[4]; };      // per repeated channel k (k < rep <= 4)
__global__ void la_crop_repeat_kernel(const float* __restrict__ img, float* __restrict__ xc, int B, int imgc, int R, int S, int y0,
                                      int x0, int rep, LaPreAffine pre, long total, const int* __restrict__ pos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (pos) { y0 = pos[0]; x0 = pos[1]; }
    const int x = (int)(i % S), y = (int)((i / S) % S);
    const long rest = i / ((long)S * S);
    const long n = rest / rep;
    const int k = (int)(rest - n * rep);
    const int c = (int)(n / B), b = (int)(n - (long)c * B);
    xc[i] = img[(((long)b * imgc + c) * R + y0 + y) * R + x0 + x] * pre.scale[k] + pre.shift[k];
}

// g_img[b][c][y0+y][x0+x] += sum_k scale[k] * gxc[(c*B+b)][k][y][x]
__global__ void la_crop_repeat_bwd_kernel(const float* __restrict__ gxc, float* __restrict__ g_img, int B, int imgc, int R, int S,
                                          int y0, int x0, int rep, LaPreAffine pre, long total, const int* __restrict__ pos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (pos) { y0 = pos[0]; x0 = pos[1]; }
    const int x = (int)(i % S), y = (int)((i / S) % S);
    const long n = i / ((long)S * S);
    const int c = (int)(n / B), b = (int)(n - (long)c * B);
    float acc = 0.f;
    for (int k = 0; k < rep; ++k) acc += gxc[((n * rep + k) * S + y) * S + x] * pre.scale[k];
    g_img[(((long)b * imgc + c) * R + y0 + y) * R + x0 + x] += acc;
}

// scale / shift: one value per repeated channel ([rep], rep <= 4) -- e.g. the (x - mean_k) / std_k of an ImageNet-style input layer
int la_crop_repeat(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                   const float* scale, const float* shift, hipStream_t stream) {
    LA_CHECK_ARG(rep >= 1 && rep <= 4, "crop_repeat: rep must be 1..4");
    LA_CHECK_ARG(img && xc && y0 >= 0 && x0 >= 0 && y0 + S <= R && x0 + S <= R && scale && shift, "crop_repeat: bad arguments");
    LaPreAffine pre;
    for (int k = 0; k < 4; ++k) { pre.scale[k] = scale[k < rep ? k : rep - 1]; pre.shift[k] = shift[k < rep ? k : rep - 1]; }
    const long total = (long)B * imgc * rep * S * S;
    hipLaunchKernelGGL(la_crop_repeat_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, img, xc, B, imgc, R, S, y0, x0, rep, pre,
                       total, pos_dev);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
extern "C" int la_crop_repeat_f32(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, int rep, float scale,
                                  float shift, hipStream_t stream) {
    const float sc[4] = {scale, scale, scale, scale}, sh[4] = {shift, shift, shift, shift};
    return la_crop_repeat(img, xc, B, imgc, R, S, y0, x0, nullptr, rep, sc, sh, stream);
}

extern "C" int la_crop_repeat_affine_f32(const float* img, float* xc, int B, int imgc, int R, int S, int y0, int x0, int rep,
                                         const float* scale, const float* shift, hipStream_t stream) {
    return la_crop_repeat(img, xc, B, imgc, R, S, y0, x0, nullptr, rep, scale, shift, stream);
}

int la_crop_repeat_grad(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, const int* pos_dev, int rep,
                        const float* scale, hipStream_t stream) {
    LA_CHECK_ARG(rep >= 1 && rep <= 4, "crop_repeat_grad: rep must be 1..4");
    LA_CHECK_ARG(gxc && g_img && y0 >= 0 && x0 >= 0 && y0 + S <= R && x0 + S <= R && scale, "crop_repeat_grad: bad arguments");
    LaPreAffine pre;
    for (int k = 0; k < 4; ++k) { pre.scale[k] = scale[k < rep ? k : rep - 1]; pre.shift[k] = 0.f; }
    const long total = (long)B * imgc * S * S;
    hipLaunchKernelGGL(la_crop_repeat_bwd_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, gxc, g_img, B, imgc, R, S, y0, x0, rep,
                       pre, total, pos_dev);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
extern "C" int la_crop_repeat_grad_f32(const float* gxc, float* g_img, int B, int imgc, int R, int S, int y0, int x0, int rep,
                                       float scale, hipStream_t stream) {
    const float sc[4] = {scale, scale, scale, scale};
    return la_crop_repeat_grad(gxc, g_img, B, imgc, R, S, y0, x0, nullptr, rep, sc, stream);
}
