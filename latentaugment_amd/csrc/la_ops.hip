// The op layer's bias_act, bias_sum and upfirdn2d over a storage type T and an arithmetic type A, instantiated for the three dtypes the
// reference's plugins dispatch with AT_DISPATCH_FLOATING_TYPES_AND_HALF (bias_act.cpp:77, upfirdn2d.cpp:63):
//   float16: half storage, fp32 arithmetic, one rounding on store (the plugin's InternalType<half> = float); scalar fp32 math with
//            conversions to and from half only (no packed arithmetic, see the Makefile)
//   float32: float storage and arithmetic (bias_act and bias_sum here; la_upfirdn2d_f32 is la_upfirdn2d.hip's, with the product path's
//            4x4 kernels)
//   float64: double storage and arithmetic, double scalars (the parity target, the reference's impl='ref' path, applies gain / alpha /
//            clamp of bias_act as Python doubles; upfirdn2d's gain is folded into the float32 taps first, see la_fir_setup)
// The SG2 path's own linear / relu / lrelu forms of bias_act (la_bias_act_f32, la_bias_act_grad_f32) are in la_misc.hip.
#include "la_op_types.h"
#include "la_upfirdn2d.h"

#include <hip/hip_fp16.h>
#include <type_traits>

__device__ __forceinline__ float la_op_exp(float v) { return expf(v); }
__device__ __forceinline__ double la_op_exp(double v) { return exp(v); }
__device__ __forceinline__ float la_op_expm1(float v) { return expm1f(v); }
__device__ __forceinline__ double la_op_expm1(double v) { return expm1(v); }
__device__ __forceinline__ float la_op_log1p(float v) { return log1pf(v); }
__device__ __forceinline__ double la_op_log1p(double v) { return log1p(v); }
__device__ __forceinline__ float la_op_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ double la_op_tanh(double v) { return tanh(v); }

// ------------------------------------------------------------------------------------------------------------
// The general bias_act op: the plugin entry point  bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)  of the reference
// (bias_act.cpp:32; activation table bias_act.py:20-30: linear, relu, lrelu, tanh, sigmoid, elu, selu, softplus, swish = ids 1..9) with
// all three values of `grad`:
//   grad 0:  out = clamp(f(x + b) * gain)                         (dy, if given, multiplies before the clamp, as the plugin does)
//   grad 1:  out = x * f'  * gain * dy,  zero where |yref| >= clamp      (x = the incoming gradient, f' from yref / gain or xref + b)
//   grad 2:  out = x * f'' * gain * dy,  zero where |yref| >= clamp      (x = the gradient of the gradient)
// Value, first and second derivative of each activation, the derivatives written in what the reference saves for it -- the OUTPUT
// (bias_act.py `ref='y'`) or, for swish, the INPUT (`ref='x'`).
#define LA_OP_SELU_SCALE 1.0507009873554804934193349852946
#define LA_OP_SELU_ALPHA 1.6732632423543772848170429916717
template <class A>
__device__ __forceinline__ A la_op_act_value(int act, A v, A alpha) {
    const A zero = 0, one = 1;
    switch (act) {
        case 2: return v > zero ? v : zero;
        case 3: return v > zero ? v : v * alpha;
        case 4: return la_op_tanh(v);
        case 5: return one / (one + la_op_exp(-v));
        case 6: return v >= zero ? v : la_op_expm1(v);
        case 7: return v >= zero ? (A)LA_OP_SELU_SCALE * v : (A)(LA_OP_SELU_SCALE * LA_OP_SELU_ALPHA) * la_op_expm1(v);
        case 8: return v > (A)80 ? v : la_op_log1p(la_op_exp(v));
        case 9: return v / (one + la_op_exp(-v));
        default: return v;
    }
}
template <class A>
__device__ __forceinline__ void la_op_act_derivs(int act, A r, A alpha, A& d1, A& d2) {
    const A zero = 0, one = 1, two = 2, sa = (A)(LA_OP_SELU_SCALE * LA_OP_SELU_ALPHA);
    d2 = zero;
    switch (act) {
        case 2: d1 = r > zero ? one : zero; break;
        case 3: d1 = r > zero ? one : alpha; break;
        case 4: d1 = one - r * r; d2 = d1 * (-two * r); break;
        case 5: d1 = r * (one - r); d2 = d1 * (one - two * r); break;
        case 6: d1 = r >= zero ? one : r + one; d2 = r >= zero ? zero : r + one; break;
        case 7: d1 = r >= zero ? (A)LA_OP_SELU_SCALE : r + sa; d2 = r >= zero ? zero : r + sa; break;
        case 8: { const A e = la_op_exp(-r); d1 = one - e; d2 = e * (one - e); break; }
        case 9: {      // r = the pre-activation: sigma = 1 / (1 + e^-r);  f' = sigma (1 + r (1 - sigma));  f'' = sigma (1 - sigma) (2 + r (1 - 2 sigma))
            const A sg = one / (one + la_op_exp(-r));
            d1 = sg * (one + r * (one - sg));
            d2 = sg * (one - sg) * (two + r * (one - two * sg));
            break;
        }
        default: d1 = one; break;
    }
}

template <class T>
struct LaBiasActArgs {
    typedef typename LaOpType<T>::A A;
    const T *x, *b, *xref, *yref, *dy;
    T* out;
    long n, stepb;
    int nb, grad, act;
    int vec;              // every pointer 16-byte aligned: whole groups move as one 16-byte load / store
    A alpha, gain, clamp;
    A clamp_s;            // the clamp as the storage type holds it: a clamped output reads back as exactly this value (grad >= 1)
};

// one element: xv = x[i], bv = its bias entry, xr / yr / g = xref[i] / yref[i] / dy[i] (0, 0, 1 where absent)
template <class T>
__device__ __forceinline__ typename LaOpType<T>::A la_op_bias_act_one(const LaBiasActArgs<T>& p, typename LaOpType<T>::A xv,
                                                                      typename LaOpType<T>::A bv, typename LaOpType<T>::A xr,
                                                                      typename LaOpType<T>::A yr, typename LaOpType<T>::A g) {
    typedef typename LaOpType<T>::A A;
    A v;
    if (p.grad == 0) {
        v = la_op_act_value<A>(p.act, xv + bv, p.alpha) * p.gain * g;
        if (p.clamp >= (A)0) v = fmin(fmax(v, -p.clamp), p.clamp);
    } else {
        A r = p.gain != (A)0 ? yr / p.gain : (A)0;
        A cl = p.clamp_s;
        if (p.act == 9) {      // swish re-derives the reference value (unrounded) from its saved input: compared with the clamp itself
            r = xr + bv;
            yr = la_op_act_value<A>(9, r, p.alpha) * p.gain;
            cl = p.clamp;
        }
        A d1, d2;
        la_op_act_derivs<A>(p.act, r, p.alpha, d1, d2);
        v = xv * (p.grad == 1 ? d1 : d2) * p.gain * g;
        if (p.clamp >= (A)0 && !(yr > -cl && yr < cl)) v = (A)0;
    }
    return v;
}

// one work item = V = 16 / sizeof(T) consecutive elements (8 halves / 4 floats / 2 doubles): one 16-byte load per operand and one 16-byte store
template <class T, int V>
struct alignas(16) LaOpVec { T v[V]; };

template <class T>
__global__ __launch_bounds__(256) void la_bias_act_op_kernel(LaBiasActArgs<T> p) {
    typedef typename LaOpType<T>::A A;
    constexpr int V = 16 / sizeof(T);
    typedef LaOpVec<T, V> Vec;
    const long groups = (p.n + V - 1) / V;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += stride) {
        const long i0 = gi * V;
        A bv[V];
        if (!p.b) {
#pragma unroll
            for (int k = 0; k < V; ++k) bv[k] = (A)0;
        } else if (p.stepb % V == 0) {      // the group lies inside one bias entry
            const A b0 = la_op_load(p.b[(i0 / p.stepb) % p.nb]);
#pragma unroll
            for (int k = 0; k < V; ++k) bv[k] = b0;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) bv[k] = i0 + k < p.n ? la_op_load(p.b[((i0 + k) / p.stepb) % p.nb]) : (A)0;
        }
        if (p.vec && i0 + V <= p.n) {
            Vec xs, xr, yr, g, o;
            xs = *reinterpret_cast<const Vec*>(p.x + i0);
            if (p.xref) xr = *reinterpret_cast<const Vec*>(p.xref + i0);
            if (p.yref) yr = *reinterpret_cast<const Vec*>(p.yref + i0);
            if (p.dy) g = *reinterpret_cast<const Vec*>(p.dy + i0);
#pragma unroll
            for (int k = 0; k < V; ++k)
                o.v[k] = la_op_store<T>(la_op_bias_act_one<T>(p, la_op_load(xs.v[k]), bv[k], p.xref ? la_op_load(xr.v[k]) : (A)0,
                                                              p.yref ? la_op_load(yr.v[k]) : (A)0, p.dy ? la_op_load(g.v[k]) : (A)1));
            *reinterpret_cast<Vec*>(p.out + i0) = o;
        } else {
            for (int k = 0; k < V && i0 + k < p.n; ++k) {
                const long i = i0 + k;
                p.out[i] = la_op_store<T>(la_op_bias_act_one<T>(p, la_op_load(p.x[i]), bv[k], p.xref ? la_op_load(p.xref[i]) : (A)0,
                                                                p.yref ? la_op_load(p.yref[i]) : (A)0, p.dy ? la_op_load(p.dy[i]) : (A)1));
            }
        }
    }
}

template <class T>
__device__ __forceinline__ typename LaOpType<T>::A la_op_block_sum_256(typename LaOpType<T>::A v, typename LaOpType<T>::A* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// db[c] = sum of dx over every axis but the bias axis (bias_act.py:187, :206), accumulated in A, one rounding into db: element i belongs
// to channel (i / stepb) % nb, one block per channel
template <class T>
__global__ __launch_bounds__(256) void la_bias_sum_op_kernel(const T* __restrict__ dx, T* __restrict__ db, long n, long stepb, int nb) {
    typedef typename LaOpType<T>::A A;
    __shared__ A red[4];
    const int c = blockIdx.x;
    const long outer = n / (stepb * nb);
    A acc = 0;
    for (long o = 0; o < outer; ++o) {
        const T* q = dx + (o * nb + c) * stepb;
        for (long k = threadIdx.x; k < stepb; k += blockDim.x) acc += la_op_load(q[k]);
    }
    const A t = la_op_block_sum_256<T>(acc, red);
    if (threadIdx.x == 0) db[c] = la_op_store<T>(t);
}

template <class T> static typename LaOpType<T>::A la_op_round(typename LaOpType<T>::A v) { return v; }      // (host) v as storage type T holds it
template <> float la_op_round<__half>(float v) { return __half2float(__float2half(v)); }

template <class T>
static int bias_act_op(const T* x, const T* b, const T* xref, const T* yref, const T* dy, T* out, long n, long stepb, int nb, int grad,
                       int act, typename LaOpType<T>::A alpha, typename LaOpType<T>::A gain, typename LaOpType<T>::A clamp, hipStream_t stream) {
    typedef typename LaOpType<T>::A A;
    if (n == 0) return LA_OK;
    LA_CHECK_ARG(x && out && n > 0, "bias_act_ex: null pointer");
    LA_CHECK_ARG(act >= 1 && act <= 9, "bias_act_ex: activation id must be 1..9 (bias_act.py:20-30)");
    LA_CHECK_ARG(grad >= 0 && grad <= 2, "bias_act_ex: grad must be 0, 1 or 2");
    LA_CHECK_ARG(grad == 0 || act == 9 || act == 1 || yref, "bias_act_ex: grad >= 1 needs the saved output yref");
    LA_CHECK_ARG(grad == 0 || act != 9 || xref, "bias_act_ex: swish derives its gradients from the saved input xref");
    LA_CHECK_ARG(!b || (stepb >= 1 && nb >= 1 && n % (stepb * nb) == 0), "bias_act_ex: bias does not tile the tensor");
    if (!b) { stepb = 1; nb = 1; }
    LaBiasActArgs<T> p;
    p.x = x; p.b = b; p.xref = xref; p.yref = yref; p.dy = dy; p.out = out;
    p.n = n; p.stepb = stepb; p.nb = nb; p.grad = grad; p.act = act;
    p.vec = ((((size_t)x | (size_t)xref | (size_t)yref | (size_t)dy | (size_t)out) & 15) == 0);
    p.alpha = alpha; p.gain = gain; p.clamp = clamp;
    p.clamp_s = clamp >= (A)0 ? la_op_round<T>(clamp) : clamp;
    constexpr int V = 16 / sizeof(T);
    long blocks = la_cdiv(la_cdiv(n, V), 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_bias_act_op_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

template <class T>
static int bias_sum_op(const T* dx, T* db, long n, long stepb, int nb, hipStream_t stream) {
    LA_CHECK_ARG(dx && db && n > 0 && stepb >= 1 && nb >= 1 && n % (stepb * nb) == 0, "bias_sum: bad arguments");
    hipLaunchKernelGGL(la_bias_sum_op_kernel<T>, dim3(nb), dim3(256), 0, stream, dx, db, n, stepb, nb);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_bias_act_ex_f16(const unsigned short* x, const unsigned short* b, const unsigned short* xref, const unsigned short* yref,
                                  const unsigned short* dy, unsigned short* out, long n, long stepb, int nb, int grad, int act, float alpha,
                                  float gain, float clamp, hipStream_t stream) {
    typedef const __half* H;
    return bias_act_op<__half>(H(x), H(b), H(xref), H(yref), H(dy), (__half*)out, n, stepb, nb, grad, act, alpha, gain, clamp, stream);
}
extern "C" int la_bias_act_ex_f32(const float* x, const float* b, const float* xref, const float* yref, const float* dy, float* out, long n,
                                  long stepb, int nb, int grad, int act, float alpha, float gain, float clamp, hipStream_t stream) {
    return bias_act_op<float>(x, b, xref, yref, dy, out, n, stepb, nb, grad, act, alpha, gain, clamp, stream);
}
extern "C" int la_bias_act_ex_f64(const double* x, const double* b, const double* xref, const double* yref, const double* dy, double* out,
                                  long n, long stepb, int nb, int grad, int act, double alpha, double gain, double clamp, hipStream_t stream) {
    return bias_act_op<double>(x, b, xref, yref, dy, out, n, stepb, nb, grad, act, alpha, gain, clamp, stream);
}
extern "C" int la_bias_sum_f16(const unsigned short* dx, unsigned short* db, long n, long stepb, int nb, hipStream_t stream) {
    return bias_sum_op<__half>((const __half*)dx, (__half*)db, n, stepb, nb, stream);
}
extern "C" int la_bias_sum_f32(const float* dx, float* db, long n, long stepb, int nb, hipStream_t stream) {
    return bias_sum_op<float>(dx, db, n, stepb, nb, stream);
}
extern "C" int la_bias_sum_f64(const double* dx, double* db, long n, long stepb, int nb, hipStream_t stream) {
    return bias_sum_op<double>(dx, db, n, stepb, nb, stream);
}

// ------------------------------------------------------------------------------------------------------------
// upfirdn2d in float16 / float64: the generic gather (la_fir_gather, as la_upfirdn2d_kernel) over storage T with the taps in A, plus a float16 form of the 4x4 filter at
// stride 1, up 2 and down 2 (setup_filter([1,3,3,1]) through filter2d / upsample2d / downsample2d and their adjoints)
template <class T>
struct LaFirOpArgs {
    const T* in;
    T* out;
    int P;
    int Hin, Win, Hout, Wout;
    int upx, upy, dnx, dny, padx0, pady0;
    int fw, fh;
    typename LaOpType<T>::A f[LA_FIR_MAX * LA_FIR_MAX];      // correlation taps (flipped as needed, gain folded in)
};

template <class T>
__global__ __launch_bounds__(256) void la_upfirdn2d_op_kernel(LaFirOpArgs<T> a) {
    typedef typename LaOpType<T>::A A;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wout || y >= a.Hout) return;
    const long HWin = (long)a.Hin * a.Win, HWout = (long)a.Hout * a.Wout;
    for (int p = blockIdx.z; p < a.P; p += gridDim.z) {
        const A v = la_fir_gather<A>(a, a.in + (long)p * HWin, x, y);
        a.out[(long)p * HWout + (long)y * a.Wout + x] = la_op_store<T>(v);
    }
}

// columns base + LO .. base + LO + N - 1 of one half row into fp32 (base % 8 == 0, W % 8 == 0, row 16-byte aligned): the 8-column
// chunks that lie wholly inside the span as one 16-byte load each, the columns at its ends as 2-byte loads; zeros outside [0, W)
__device__ __forceinline__ float la_op_h2f(unsigned u, int hi) { return __half2float(__ushort_as_half((unsigned short)(hi ? u >> 16 : u))); }
template <int LO, int N>
__device__ __forceinline__ void la_op_hrow(const __half* rp, int base, int W, bool rok, float (&w)[N]) {
    constexpr int C0 = LO >= 0 ? LO / 8 : -((7 - LO) / 8), C1 = (LO + N - 1) >= 0 ? (LO + N - 1) / 8 : -((8 - LO - N) / 8);
#pragma unroll
    for (int c = C0; c <= C1; ++c) {
        const int c0 = base + 8 * c;
        if (8 * c >= LO && 8 * c + 8 <= LO + N) {
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (rok && c0 >= 0 && c0 < W) u = *reinterpret_cast<const uint4*>(rp + c0);
            const unsigned d[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) w[8 * c + k - LO] = la_op_h2f(d[k >> 1], k & 1);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = 8 * c + k - LO;
                if (j >= 0 && j < N) w[j] = (rok && c0 + k >= 0 && c0 + k < W) ? __half2float(rp[c0 + k]) : 0.f;
            }
        }
    }
}
__device__ __forceinline__ uint4 la_op_pack8(const float* o) {
    unsigned d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        d[k] = (unsigned)__half_as_ushort(__float2half(o[2 * k])) | ((unsigned)__half_as_ushort(__float2half(o[2 * k + 1])) << 16);
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// float16, 4x4 taps (any), fp32 accumulation in the taps' ascending row, column order (that of the float32 kernels), one rounding:
//   MODE 0  up = down = 1, pad x PADX (1 or 2): work item = 8 columns of LA_OP_S1_ROWS output rows, from the rolling input rows
//           (one load of each input row per work item: 1 row per item measured 131 us at [8,128,256,256], no faster than float32)
//   MODE 1  up 2, pad 2: work item = 16 columns of output rows 2i and 2i + 1, from input rows i - 1 .. i + 1 (la_fir4x4_up2_kernel's taps)
//   MODE 2  down 2, pad 1: work item = 8 outputs of one row, from input rows 2y - 1 .. 2y + 2
// Needs W % 8 == 0 of the input and the output rows and 16-byte aligned planes (fir_op_launch checks); every load and store is in bounds.
#define LA_OP_S1_ROWS 4
template <int MODE, int PADX>
__global__ __launch_bounds__(256) void la_fir4x4_h_kernel(LaFirOpArgs<__half> a) {
    const int gw = MODE == 1 ? a.Wout / 16 : a.Wout / 8;
    const int rows = MODE == 1 ? a.Hin : MODE == 0 ? (a.Hout + LA_OP_S1_ROWS - 1) / LA_OP_S1_ROWS : a.Hout;
    const long per_plane = (long)rows * gw;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int p = (int)(gid / per_plane);
    if (p >= a.P) return;
    const int within = (int)(gid - (long)p * per_plane);
    const int y = within / gw, q = within - y * gw;
    const __half* ip = a.in + (long)p * a.Hin * a.Win;
    __half* op = a.out + (long)p * a.Hout * a.Wout;
    float f[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = a.f[i];
    if (MODE == 0) {
        const int x0 = 8 * q, y0 = y * LA_OP_S1_ROWS;
        float acc[LA_OP_S1_ROWS][8];
#pragma unroll
        for (int r = 0; r < LA_OP_S1_ROWS; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[r][k] = 0.f;
#pragma unroll
        for (int wr = 0; wr < LA_OP_S1_ROWS + 3; ++wr) {
            const int iy = y0 + wr - a.pady0;
            const bool rok = iy >= 0 && iy < a.Hin;
            float w[11];
            la_op_hrow<-PADX, 11>(ip + (long)(rok ? iy : 0) * a.Win, x0, a.Win, rok, w);
#pragma unroll
            for (int r = 0; r < LA_OP_S1_ROWS; ++r) {
                const int ta = wr - r;      // filter row of output row y0 + r (ascending for each r, as in the float32 kernels)
                if (ta >= 0 && ta < 4) {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
#pragma unroll
                        for (int tb = 0; tb < 4; ++tb) acc[r][k] += w[k + tb] * f[ta * 4 + tb];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < LA_OP_S1_ROWS; ++r)
            if (y0 + r < a.Hout) *reinterpret_cast<uint4*>(op + (long)(y0 + r) * a.Wout + x0) = la_op_pack8(acc[r]);
    } else if (MODE == 1) {
        const int i = y, j0 = 8 * q;
        float w[3][10];                                              // in[i-1 .. i+1][j0-1 .. j0+8]
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int iy = i - 1 + r;
            const bool rok = iy >= 0 && iy < a.Hin;
            la_op_hrow<-1, 10>(ip + (long)(rok ? iy : 0) * a.Win, j0, a.Win, rok, w[r]);
        }
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            float o[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {                           // output column 16q + k = 2 (j0 + k/2) + (k & 1)
                const int px = k & 1, jj = k >> 1;
                float s = 0.f;
#pragma unroll
                for (int ua = 0; ua < 2; ++ua)
#pragma unroll
                    for (int ub = 0; ub < 2; ++ub) s += w[py + ua][jj + px + ub] * f[(py + 2 * ua) * 4 + px + 2 * ub];
                o[k] = s;
            }
            __half* rp = op + (long)(2 * i + py) * a.Wout + 16 * q;
            *reinterpret_cast<uint4*>(rp) = la_op_pack8(o);
            *reinterpret_cast<uint4*>(rp + 8) = la_op_pack8(o + 8);
        }
    } else {
        const int x0 = 8 * q;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            const int iy = 2 * y - 1 + ta;
            const bool rok = iy >= 0 && iy < a.Hin;
            float w[18];                                             // columns 2 x0 - 1 .. 2 x0 + 16
            la_op_hrow<-1, 18>(ip + (long)(rok ? iy : 0) * a.Win, 2 * x0, a.Win, rok, w);
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int tb = 0; tb < 4; ++tb) acc[k] += w[2 * k + tb] * f[ta * 4 + tb];
        }
        *reinterpret_cast<uint4*>(op + (long)y * a.Wout + x0) = la_op_pack8(acc);
    }
}

template <class T>
static int fir_op_fill(LaFirOpArgs<T>& a, const T* in, T* out, int B, int C, int Hin, int Win, const float* f_host, int fh, int fw, int upx,
                       int upy, int dnx, int dny, int padx0, int padx1, int pady0, int pady1, int flip_filter, typename LaOpType<T>::A gain) {
    LaFirSetup s;
    const int rc = la_fir_setup(s, in, out, B, C, Hin, Win, f_host, LaFirGeom{fh, fw, upx, upy, dnx, dny, padx0, padx1, pady0, pady1, flip_filter, (float)gain});
    if (rc) return rc;
    a.in = in; a.out = out; a.P = B * C;
    a.Hin = Hin; a.Win = Win; a.Wout = s.Wout; a.Hout = s.Hout;
    a.upx = upx; a.upy = upy; a.dnx = dnx; a.dny = dny; a.padx0 = padx0; a.pady0 = pady0;
    a.fw = fw; a.fh = fh;
    for (int k = 0; k < fh * fw; ++k) a.f[k] = (typename LaOpType<T>::A)s.f[k];
    return LA_OK;
}

// the float16 4x4 forms: which one, if any, takes this call (-1 = the generic kernel)
static int fir_h_mode(const LaFirOpArgs<__half>& a) {
    if (a.fw != 4 || a.fh != 4 || (((size_t)a.in | (size_t)a.out) & 15) != 0 || a.Win % 8 != 0) return -1;
    if (a.upx == 1 && a.upy == 1 && a.dnx == 1 && a.dny == 1 && (a.padx0 == 1 || a.padx0 == 2) && a.Wout % 8 == 0) return 0;
    if (a.upx == 2 && a.upy == 2 && a.dnx == 1 && a.dny == 1 && a.padx0 == 2 && a.pady0 == 2 && a.Wout == 2 * a.Win && a.Hout == 2 * a.Hin)
        return 1;
    if (a.upx == 1 && a.upy == 1 && a.dnx == 2 && a.dny == 2 && a.padx0 == 1 && a.pady0 == 1 && a.Win == 2 * a.Wout && a.Hin == 2 * a.Hout &&
        a.Wout % 8 == 0)
        return 2;
    return -1;
}

template <class T>
static int fir_op_launch(const LaFirOpArgs<T>& a, hipStream_t stream) {
    if constexpr (std::is_same<T, __half>::value) {
        const int mode = fir_h_mode(a);
        if (mode >= 0) {
            const long rows = mode == 1 ? a.Hin : mode == 0 ? la_cdiv(a.Hout, LA_OP_S1_ROWS) : a.Hout;
            const long items = (long)a.P * rows * (a.Wout / (mode == 1 ? 16 : 8));
            LA_CHECK_ARG(items < (1l << 38), "upfirdn2d: too many planes");
            const dim3 g((unsigned)((items + 255) / 256));
            if (mode == 0 && a.padx0 == 1) hipLaunchKernelGGL((la_fir4x4_h_kernel<0, 1>), g, dim3(256), 0, stream, a);
            else if (mode == 0) hipLaunchKernelGGL((la_fir4x4_h_kernel<0, 2>), g, dim3(256), 0, stream, a);
            else if (mode == 1) hipLaunchKernelGGL((la_fir4x4_h_kernel<1, 2>), g, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((la_fir4x4_h_kernel<2, 1>), g, dim3(256), 0, stream, a);
            LA_CHECK_LAUNCH();
            return LA_OK;
        }
    }
    dim3 grid(la_cdiv(a.Wout, 64), la_cdiv(a.Hout, 4), a.P < 1024 ? a.P : 1024);
    LA_CHECK_ARG(grid.y <= 65535, "upfirdn2d: output too tall");
    hipLaunchKernelGGL(la_upfirdn2d_op_kernel<T>, grid, dim3(256), 0, stream, a);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_upfirdn2d_f16(const unsigned short* x, const float* f_host, unsigned short* y, int N, int C, int H, int W, int fh, int fw,
                                int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                                hipStream_t stream) {
    LaFirOpArgs<__half> a;
    const int rc = fir_op_fill<__half>(a, (const __half*)x, (__half*)y, N, C, H, W, f_host, fh, fw, upx, upy, downx, downy, padx0, padx1,
                                       pady0, pady1, flip, gain);
    return rc ? rc : fir_op_launch<__half>(a, stream);
}
extern "C" int la_upfirdn2d_f64(const double* x, const float* f_host, double* y, int N, int C, int H, int W, int fh, int fw, int upx,
                                int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, double gain,
                                hipStream_t stream) {
    LaFirOpArgs<double> a;
    const int rc = fir_op_fill<double>(a, x, y, N, C, H, W, f_host, fh, fw, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain);
    return rc ? rc : fir_op_launch<double>(a, stream);
}
