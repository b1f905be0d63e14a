// Internal (C++) interface of la_criteria.hip.
#pragma once
#include "la_common.h"

int la_bank_dot(const float* Y, long m, long K, const float* X, int n, long ldx, long xmod, float* yx, float* yy,
                hipStream_t stream);
int la_bank_colsum(const float* Y, long m, long K, float* colsum, hipStream_t stream);
// scratch sizes of the bank kernels (floats): yx 5*m*n, yy 5*m, xx 33*n
#define LA_YX_FLOATS(m, n) (17L * (m) * (n))      // result + up to 16 K-slice partials (la_criteria.hip KSPLIT)
#define LA_YY_FLOATS(m) (17L * (m))
#define LA_XX_FLOATS(n) (33L * (n))
// out[0] (+)= scale * sum_{m,n} (|Y_m|^2 + |X_n|^2 - 2<Y_m,X_n>); workspaces: yx_ws LA_YX_FLOATS, yy_ws LA_YY_FLOATS, xx_ws LA_XX_FLOATS
int la_l2_mean_from_bank(const float* Y, long m, long K, const float* X, int n, long ldx, long xmod, float* yx_ws,
                         float* yy_ws, float* xx_ws, float scale, float* out, int accumulate, hipStream_t stream);
int la_pix_grad(const float* img, const float* colsum, float* g, int B, int imgc, int R, int cc, int off, float coef2,
                float mrows, hipStream_t stream);
int la_broadcast_mix(const float* w_opt, const float* w0, float* w_aug, int B, int num_ws, int wdim, float alpha,
                     int soft, hipStream_t stream);
// Tail of a W-space loop step in one launch (la_misc.hip): dw = sum of dws over the ws slots + the latent criterion's gradient, the
// Adam update with the bias corrections of step *ctr + 1 from the device table `tab` (la_adam_fill_table), and *ctr += 1;
// ticket: a zeroed device int of the handle
int la_step_tail(const float* dws, const float* colsumW, float* dw, float* p, float* m, float* v, int B, int num_ws, int wdim, float lat2,
                 float mrows, float lr, float beta1, float beta2, float eps, const float* tab, int* ctr, int* ticket, hipStream_t stream);
void la_adam_fill_table(float* tab_host, int steps, float beta1, float beta2);
// W+ loop (la_wplus.hip): the step tail without the sum over the slots, and the gate without the broadcast; all of
// [B][num_ws][w_dim], w_dim % 4 == 0, 16-byte aligned buffers
int la_wplus_step_tail(const float* dws, const float* colsumW, float* dw, float* p, float* m, float* v, int B, int num_ws, int wdim,
                       float lat2, float mrows, float lr, float beta1, float beta2, float eps, const float* tab, int* ctr, int* ticket,
                       hipStream_t stream);
int la_wplus_gate(const float* w_opt, const float* w0, float* w_aug, int B, int num_ws, int wdim, float alpha, int soft,
                  hipStream_t stream);
