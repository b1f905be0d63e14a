// W+ latent optimisation (la_latent_opt_create_ex with latent_space = 1): the loop optimises one latent row per style slot,
// w_opt [B][num_ws][w_dim], instead of one 512-vector broadcast to every slot.  It is the reference's LatentAug.forward
// (augments/utils/util_latent_aug.py:207-310) with broadcasting() the identity, hard_aug(w, w_tilde) = w_tilde and
// smooth_aug(w, w_tilde) = alpha * w_tilde + (1 - alpha) * w row by row.  The synthesis, the criteria and their gradients are the
// W loop's launches with a per-slot latent stride; only the step tail and the gate differ, and they live here.
#include "la_criteria.h"

// Tail of a W+ optimisation step in ONE launch, the W+ counterpart of la_step_tail_kernel (la_misc.hip): per element (b, l, j)
//   g = dws[b][l][j] + lat2 * (Mw * p[b][l][j] - colsumW[l][j])
// (no sum over the slots: each slot is a parameter of its own; the latent criterion's term is added to the slot's gradient), then
// the Adam update (la_adam_update, component by component) with the bias corrections of step *ctr + 1 from the device table
// tab[t - 1] = {1 - b1^t, sqrt(1 - b2^t)}, and the step counter (la_step_ticket).  Four elements per thread: w_dim % 4 == 0 and
// 16-byte aligned buffers (checked by the caller).  dws / colsumW may be null (no image criterion / no latent criterion).
__global__ __launch_bounds__(256) void la_wplus_step_tail_kernel(const float4* __restrict__ dws, const float4* __restrict__ colsumW,
                                                                float4* __restrict__ dw, float4* __restrict__ p, float4* __restrict__ m,
                                                                float4* __restrict__ v, long row4, float lat2, float mrows, long total4,
                                                                float lr, float b1, float b2, float eps, const float2* __restrict__ tab,
                                                                int* __restrict__ ctr, int* __restrict__ ticket) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const float2 bc = tab[*ctr];
    if (i < total4) {
        float4 g = dws ? dws[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 pv = p[i];
        if (colsumW) {
            const float4 cs = colsumW[i % row4];
            g.x += lat2 * (mrows * pv.x - cs.x);
            g.y += lat2 * (mrows * pv.y - cs.y);
            g.z += lat2 * (mrows * pv.z - cs.z);
            g.w += lat2 * (mrows * pv.w - cs.w);
        }
        dw[i] = g;
        float4 mv = m[i], vv = v[i], pn = pv;
        const float step = lr / bc.x;
        la_adam_update(pn.x, mv.x, vv.x, g.x, step, bc.y, b1, b2, eps);
        la_adam_update(pn.y, mv.y, vv.y, g.y, step, bc.y, b1, b2, eps);
        la_adam_update(pn.z, mv.z, vv.z, g.z, step, bc.y, b1, b2, eps);
        la_adam_update(pn.w, mv.w, vv.w, g.w, step, bc.y, b1, b2, eps);
        m[i] = mv; v[i] = vv; p[i] = pn;
    }
    la_step_ticket(ctr, ticket);
}

static bool al16(const void* p) { return ((size_t)p & 15) == 0; }

int la_wplus_step_tail(const float* dws, const float* colsumW, float* dw, float* p, float* m, float* v, int B, int num_ws, int wdim,
                       float lat2, float mrows, float lr, float beta1, float beta2, float eps, const float* tab, int* ctr, int* ticket,
                       hipStream_t stream) {
    LA_CHECK_ARG(wdim % 4 == 0, "wplus_step_tail: w_dim must be a multiple of 4");
    LA_CHECK_ARG(al16(dws) && al16(colsumW) && al16(dw) && al16(p) && al16(m) && al16(v), "wplus_step_tail: buffers must be 16-byte aligned");
    const long row4 = (long)num_ws * wdim / 4;
    const long total4 = (long)B * row4;
    if (total4 == 0) return LA_OK;
    hipLaunchKernelGGL(la_wplus_step_tail_kernel, dim3(la_cdiv(total4, 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(dws),
                       reinterpret_cast<const float4*>(colsumW), reinterpret_cast<float4*>(dw), reinterpret_cast<float4*>(p),
                       reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), row4, lat2, mrows, total4, lr, beta1, beta2, eps,
                       reinterpret_cast<const float2*>(tab), ctr, ticket);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// The W+ gate (hard_aug / smooth_aug with the identity broadcast): w_aug = soft ? alpha * w_opt + (1 - alpha) * w0 : w_opt,
// element-wise over [B][num_ws][w_dim] (la_broadcast_mix_kernel's arithmetic without the broadcast).
__global__ void la_wplus_gate_kernel(const float4* __restrict__ w_opt, const float4* __restrict__ w0, float4* __restrict__ w_aug,
                                     float alpha, int soft, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 a = w_opt[i];
    if (soft) {
        const float4 b = w0[i];
        a.x = (alpha * a.x) + ((1.f - alpha) * b.x);
        a.y = (alpha * a.y) + ((1.f - alpha) * b.y);
        a.z = (alpha * a.z) + ((1.f - alpha) * b.z);
        a.w = (alpha * a.w) + ((1.f - alpha) * b.w);
    }
    w_aug[i] = a;
}

int la_wplus_gate(const float* w_opt, const float* w0, float* w_aug, int B, int num_ws, int wdim, float alpha, int soft,
                  hipStream_t stream) {
    LA_CHECK_ARG(wdim % 4 == 0, "wplus_gate: w_dim must be a multiple of 4");
    LA_CHECK_ARG(al16(w_opt) && al16(w0) && al16(w_aug), "wplus_gate: buffers must be 16-byte aligned");
    const long total4 = (long)B * num_ws * wdim / 4;
    if (total4 == 0) return LA_OK;
    hipLaunchKernelGGL(la_wplus_gate_kernel, dim3(la_cdiv(total4, 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(w_opt),
                       reinterpret_cast<const float4*>(w0), reinterpret_cast<float4*>(w_aug), alpha, soft, total4);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
