// Error reporting + the standalone elementwise ops of the C ABI (the SG2 forms of bias_act, Adam, small vector helpers).
#include "la_common.h"
#include "la_rng.h"

#include <string.h>

static thread_local char g_err[256] = "";
void la_set_error(const char* msg) {
    strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
}
extern "C" const char* la_last_error(void) { return g_err; }
extern "C" int la_abi_version(void) { return 1; }

// ------------------------------------------------------------------------------------------------------------
// bias_act forward:  y = clamp(act(x + b[(i / stepb) % nb]) * gain)            (bias_act.cu:23-147, grad = 0)
// bias_act backward: dx = dy * act'(y-referenced) ; db[c] = sum dx              (bias_act.cu grad = 1; bias_act.py:155-177)
// linear / relu / lrelu, first order: all the SG2 path needs; the general op (every activation, grad 0 / 1 / 2, three dtypes) is in la_ops.hip
__global__ __launch_bounds__(256) void la_bias_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ b,
                                                             float* __restrict__ y, long n, long stepb, int nb, int act,
                                                             float alpha, float gain, float clamp) {
    const long stride = (long)gridDim.x * blockDim.x * 4;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n && (stepb % 4 == 0 || !b)) {
            float4 v = *reinterpret_cast<const float4*>(x + i);
            const float bv = b ? b[(i / stepb) % nb] : 0.f;
            v.x = la_act_fwd(v.x + bv, act, alpha, gain, clamp); v.y = la_act_fwd(v.y + bv, act, alpha, gain, clamp);
            v.z = la_act_fwd(v.z + bv, act, alpha, gain, clamp); v.w = la_act_fwd(v.w + bv, act, alpha, gain, clamp);
            *reinterpret_cast<float4*>(y + i) = v;
        } else {
            for (long k = i; k < n && k < i + 4; ++k) {
                const float bv = b ? b[(k / stepb) % nb] : 0.f;
                y[k] = la_act_fwd(x[k] + bv, act, alpha, gain, clamp);
            }
        }
    }
}

__global__ __launch_bounds__(256) void la_bias_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ yref,
                                                             float* __restrict__ dx, long n, int act, float alpha,
                                                             float gain, float clamp) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dx[i] = dy[i] * la_act_bwd_from_y(yref[i], act, alpha, gain, clamp);
}

static int act_ok(int act) { return act == LA_ACT_LINEAR || act == LA_ACT_RELU || act == LA_ACT_LRELU; }

extern "C" int la_bias_act_f32(const float* x, const float* b, float* y, long n, long stepb, int nb, int act, float alpha,
                               float gain, float clamp, hipStream_t stream) {
    if (n == 0) return LA_OK;   // empty tensors are legal (and have null data pointers)
    LA_CHECK_ARG(x && y && n > 0, "bias_act: null pointer");
    LA_CHECK_ARG(act_ok(act), "bias_act: only linear(1)/relu(2)/lrelu(3) are implemented on this path");
    LA_CHECK_ARG(!b || (stepb >= 1 && nb >= 1 && n % (stepb * nb) == 0), "bias_act: bias does not tile the tensor");
    if (!b) { stepb = 4; nb = 1; }
    long blocks = la_cdiv(la_cdiv(n, 4), 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_bias_act_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, b, y, n, stepb, nb, act,
                       alpha, gain, clamp);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_bias_act_grad_f32(const float* dy, const float* yref, float* dx, float* db, long n, long stepb, int nb,
                                    int act, float alpha, float gain, float clamp, hipStream_t stream) {
    if (n == 0) return LA_OK;
    LA_CHECK_ARG(dy && yref && dx && n > 0, "bias_act_grad: null pointer");
    LA_CHECK_ARG(act_ok(act), "bias_act_grad: only linear(1)/relu(2)/lrelu(3) are implemented on this path");
    long blocks = la_cdiv(n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_bias_act_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dy, yref, dx, n, act, alpha,
                       gain, clamp);
    LA_CHECK_LAUNCH();
    if (db) {
        LA_CHECK_ARG(stepb >= 1 && nb >= 1 && n % (stepb * nb) == 0, "bias_act_grad: bias does not tile the tensor");
        return la_bias_sum_f32(dx, db, n, stepb, nb, stream);      // (la_ops.hip)
    }
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam semantics as used at util_latent_aug.py:213,276): one fused elementwise update.
__global__ void la_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                               float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float bc1,
                               float bc2_sqrt, float gscale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    la_adam_update(p[i], m[i], v[i], g[i] * gscale, lr / bc1, bc2_sqrt, b1, b2, eps);
}

// Tail of an optimisation step in ONE launch (three separate ones were each a 5 us link of the step's serial chain).  Per element
// (b, j) of the W-space latent (ws = w repeated num_ws times, util_latent_aug.py:493-494):
//   dw[b][j] = sum_l dws[b][l][j]  +  lat2 * (num_ws * mrows * p[b][j] - sum_l colsumW[l][j])
// both sums over the ws slots l in ascending order (eight loads in flight at a time, added in slot order), the latent criterion's
// term added last; lat2 = sign * 2 * w_latent / (m * n * num_ws * wdim), mrows = rows of the latent bank; dws / colsumW may be null
// (no image criterion / no latent criterion).  Then the Adam update (la_adam_update) with the bias corrections of step *ctr + 1 from
// the device table tab[t - 1] = {1 - b1^t, sqrt(1 - b2^t)} (la_adam_fill_table: the same powf as la_adam_step_f32), so that one
// captured launch serves every step, and the step counter (la_step_ticket).
__global__ __launch_bounds__(256) void la_step_tail_kernel(const float* __restrict__ dws, const float* __restrict__ colsumW, float* __restrict__ dw,
                                                          float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int num_ws,
                                                          int wdim, float lat2, float mrows, long total, float lr, float b1, float b2,
                                                          float eps, const float2* __restrict__ tab, int* __restrict__ ctr,
                                                          int* __restrict__ ticket) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const float2 bc = tab[*ctr];
    if (i < total) {
        const long b = i / wdim;
        const int j = (int)(i - b * wdim);
        float acc = 0.f, cs = 0.f;
        int l = 0;
        for (; l + 7 < num_ws; l += 8) {      // (eight slots' loads in flight, added in slot order)
            float a[8], c[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a[k] = dws ? dws[(b * num_ws + l + k) * wdim + j] : 0.f;
                c[k] = colsumW ? colsumW[(long)(l + k) * wdim + j] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) { if (dws) acc += a[k]; if (colsumW) cs += c[k]; }
        }
        for (; l < num_ws; ++l) {
            if (dws) acc += dws[(b * num_ws + l) * wdim + j];
            if (colsumW) cs += colsumW[(long)l * wdim + j];
        }
        const float pv = p[i];
        if (colsumW) acc += lat2 * ((float)num_ws * mrows * pv - cs);
        dw[i] = acc;
        float pn = pv;
        la_adam_update(pn, m[i], v[i], acc, lr / bc.x, bc.y, b1, b2, eps);
        p[i] = pn;
    }
    la_step_ticket(ctr, ticket);
}

int la_step_tail(const float* dws, const float* colsumW, float* dw, float* p, float* m, float* v, int B, int num_ws, int wdim, float lat2,
                 float mrows, float lr, float beta1, float beta2, float eps, const float* tab, int* ctr, int* ticket, hipStream_t stream) {
    const long total = (long)B * wdim;
    if (total == 0) return LA_OK;
    hipLaunchKernelGGL(la_step_tail_kernel, dim3(la_cdiv(total, 256)), dim3(256), 0, stream, dws, colsumW, dw, p, m, v, num_ws, wdim, lat2,
                       mrows, total, lr, beta1, beta2, eps, reinterpret_cast<const float2*>(tab), ctr, ticket);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

void la_adam_fill_table(float* tab_host, int steps, float beta1, float beta2) {
    for (int t = 1; t <= steps; ++t) {
        tab_host[2 * (t - 1)] = 1.f - powf(beta1, (float)t);
        tab_host[2 * (t - 1) + 1] = sqrtf(1.f - powf(beta2, (float)t));
    }
}

extern "C" int la_adam_step_f32(float* p, const float* g, float* m, float* v, long n, int step, float lr, float beta1,
                                float beta2, float eps, hipStream_t stream) {
    LA_CHECK_ARG(p && g && m && v && n >= 0 && step >= 1, "adam: bad arguments");
    if (n == 0) return LA_OK;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(la_adam_kernel, dim3(la_cdiv(n, 256)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       bc1, bc2s, 1.f);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// The counter-based unit normals of noise_mode='random': one thread per 4-element group of a row (the stream: la_rng.h).
__global__ __launch_bounds__(256) void la_noise_normal_kernel(float* __restrict__ out, long rows, long row_elems, unsigned k0, unsigned k1,
                                                             unsigned layer, long row0) {
    const long q4 = (row_elems + 3) >> 2;                      // 4-element groups per row
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows * q4) return;
    const long r = g / q4, q = g - r * q4;
    unsigned x[4];
    la_noise_words(q, row0 + r, layer, k0, k1, x);
    float z[4];
    la_unit_normals4(x, z);
    float* o = out + r * row_elems + 4 * q;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * q + k < row_elems) o[k] = z[k];
}

extern "C" int la_noise_normal_f32(float* out, long rows, long row_elems, unsigned long long seed, unsigned layer, long row0, hipStream_t stream) {
    LA_CHECK_ARG((out || rows == 0) && rows >= 0 && row_elems >= 1 && row0 >= 0, "noise_normal: bad arguments");
    LA_CHECK_ARG(row0 + rows <= 0xffffffffl, "noise_normal: row index exceeds 32 bits");
    if (rows == 0) return LA_OK;
    const long n = rows * ((row_elems + 3) >> 2);
    hipLaunchKernelGGL(la_noise_normal_kernel, dim3((unsigned)la_cdiv(n, 256)), dim3(256), 0, stream, out, rows, row_elems, (unsigned)seed,
                       (unsigned)(seed >> 32), layer, row0);
    LA_CHECK_LAUNCH();
    return LA_OK;
}
