// The op layer's last two modules of the reference's torch_utils/ops/: grid_sample (grid_sample_gradfix.py) and fma (fma.py).
//
// grid_sample: 2-D, mode='bilinear', padding_mode='zeros', align_corners=False.  x [N][C][H][W], grid [N][Ho][Wo][2] = (x, y) in
// [-1, 1], y [N][C][Ho][Wo], everything contiguous.  One thread per (n, ho, wo), consecutive lanes along wo: it turns its grid entry
// into corners and weights once (la_grid_sample_index.h: the range test happens in floating point, before any int exists) and loops
// over the channels, so the loads of a near-identity grid and every store coalesce.
//   forward   y = sum over the four corners of weight * x, a corner outside the image contributing nothing
//   backward  ONE launch: dgrid[n][ho][wo][:] summed over the channels in the thread's registers (deterministic); dx = scatter of
//             dy * weight to up to four corners with global atomic adds into a dx (float16: an fp32 workspace) that the entry zeroes
//             first -- the one sum of this library whose last bits depend on arrival order (DESIGN 'grid_sample' prices it).
//             Either output may be NULL (torch's output_mask).
//   The gradient of dx with respect to dy is the forward on the incoming gradient: no third kernel.
// float16 computes in fp32 and rounds once (dx: the fp32 workspace is rounded by a second small launch); float64 in double throughout.
//
// fma: y = a * b + c with a, b, c broadcast against each other (rank <= 4, strides 0 along broadcast axes), and the un-broadcast sum
// its gradients need: a reduction with a fixed summation order (bit-identical from run to run), double accumulators, one rounding.
#include "la_grid_sample_index.h"
#include "la_op_types.h"

#include <limits.h>

#define LA_GS_BLOCK 256

template <class A>
struct LaGsTaps {
    A w[4];          // nw, ne, sw, se
    int off[4];      // offset inside one H x W plane (0 where the corner is outside)
    bool in[4];
    A wx0, wx1, wy0, wy1;
};

template <class T>
__device__ __forceinline__ LaGsTaps<typename LaOpType<T>::A> la_gs_taps(const T* __restrict__ grid, long i, int H, int W) {
    typedef typename LaOpType<T>::A A;
    const LaGsAxis<A> ax = la_gs_axis<A>(la_op_load(grid[2 * i]), W), ay = la_gs_axis<A>(la_op_load(grid[2 * i + 1]), H);
    LaGsTaps<A> t;
    t.wx0 = ax.w0; t.wx1 = ax.w1; t.wy0 = ay.w0; t.wy1 = ay.w1;
    t.w[0] = ax.w0 * ay.w0; t.w[1] = ax.w1 * ay.w0; t.w[2] = ax.w0 * ay.w1; t.w[3] = ax.w1 * ay.w1;
    t.in[0] = ax.in0 && ay.in0; t.in[1] = ax.in1 && ay.in0; t.in[2] = ax.in0 && ay.in1; t.in[3] = ax.in1 && ay.in1;
    const int o = ay.i0 * W + ax.i0;
    t.off[0] = t.in[0] ? o : 0; t.off[1] = t.in[1] ? o + 1 : 0; t.off[2] = t.in[2] ? o + W : 0; t.off[3] = t.in[3] ? o + W + 1 : 0;
    return t;
}

template <class T>
__global__ __launch_bounds__(LA_GS_BLOCK) void la_grid_sample_fwd_kernel(const T* __restrict__ x, const T* __restrict__ grid, T* __restrict__ y,
                                                                         int C, int H, int W, int HoWo, long total) {
    typedef typename LaOpType<T>::A A;
    const long i = (long)blockIdx.x * LA_GS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const long n = i / HoWo;
    const LaGsTaps<A> t = la_gs_taps<T>(grid, i, H, W);
    const long HW = (long)H * W;
    const T* xp = x + n * C * HW;
    T* yp = y + n * C * HoWo + (i - n * HoWo);
    for (int c = 0; c < C; ++c, xp += HW, yp += HoWo) {
        A v = (A)0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.in[k]) v += t.w[k] * la_op_load(xp[t.off[k]]);
        *yp = la_op_store<T>(v);
    }
}

// ACC: what dx is accumulated in -- T itself for float32 / float64, the fp32 workspace for float16
template <class T, class ACC>
__global__ __launch_bounds__(LA_GS_BLOCK) void la_grid_sample_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ grid,
                                                                         ACC* __restrict__ dx, T* __restrict__ dgrid, int C, int H, int W, int HoWo,
                                                                         long total) {
    typedef typename LaOpType<T>::A A;
    const long i = (long)blockIdx.x * LA_GS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const long n = i / HoWo;
    const LaGsTaps<A> t = la_gs_taps<T>(grid, i, H, W);
    const long HW = (long)H * W;
    const T* gp = dy + n * C * HoWo + (i - n * HoWo);
    const long plane0 = n * C * HW;
    A gix = (A)0, giy = (A)0;
    for (int c = 0; c < C; ++c, gp += HoWo) {
        const A g = la_op_load(*gp);
        const long plane = plane0 + c * HW;
        if (dx) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.in[k]) atomicAdd(dx + plane + t.off[k], (ACC)(t.w[k] * g));
        }
        if (dgrid) {      // the terms and their order are torch's grid_sampler_2d_backward
            A v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = t.in[k] ? la_op_load(x[plane + t.off[k]]) : (A)0;
            gix -= v[0] * t.wy0 * g; giy -= v[0] * t.wx0 * g;
            gix += v[1] * t.wy0 * g; giy -= v[1] * t.wx1 * g;
            gix -= v[2] * t.wy1 * g; giy += v[2] * t.wx0 * g;
            gix += v[3] * t.wy1 * g; giy += v[3] * t.wx1 * g;
        }
    }
    if (dgrid) {
        dgrid[2 * i] = la_op_store<T>(gix * ((A)W / (A)2));
        dgrid[2 * i + 1] = la_op_store<T>(giy * ((A)H / (A)2));
    }
}

__global__ __launch_bounds__(256) void la_gs_round_f16_kernel(const float* __restrict__ ws, __half* __restrict__ out, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = __float2half(ws[i]);
}

// element counts of a call, each of which must fit an int: refused, never truncated
static int gs_check(const char* who, int N, int C, int H, int W, int Ho, int Wo, long* nx, long* ny, long* npos) {
    static thread_local char msg[160];
    if (N < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) {
        snprintf(msg, sizeof msg, "%s: empty or negative shape", who);
        la_set_error(msg);
        return LA_ERR_ARG;
    }
    const double lim = (double)INT_MAX;
    const double dx = (double)N * C * H * W, dy = (double)N * C * Ho * Wo, dg = (double)N * Ho * Wo * 2;
    if (dx > lim || dy > lim || dg > lim) {
        snprintf(msg, sizeof msg, "%s: a tensor of this call has more than INT_MAX elements (x %.0f, y %.0f, grid %.0f): refused", who, dx, dy, dg);
        la_set_error(msg);
        return LA_ERR_ARG;
    }
    *nx = (long)N * C * H * W; *ny = (long)N * C * Ho * Wo; *npos = (long)N * Ho * Wo;
    return LA_OK;
}

template <class T>
static int grid_sample_fwd(const T* x, const T* grid, T* y, int N, int C, int H, int W, int Ho, int Wo, hipStream_t stream) {
    long nx, ny, npos;
    const int rc = gs_check("grid_sample", N, C, H, W, Ho, Wo, &nx, &ny, &npos);
    if (rc) return rc;
    LA_CHECK_ARG(x && grid && y, "grid_sample: null pointer");
    hipLaunchKernelGGL(la_grid_sample_fwd_kernel<T>, dim3((unsigned)la_cdiv(npos, LA_GS_BLOCK)), dim3(LA_GS_BLOCK), 0, stream, x, grid, y, C, H, W,
                       Ho * Wo, npos);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

template <class T, class ACC>
static int grid_sample_bwd(const T* dy, const T* x, const T* grid, T* dx, T* dgrid, ACC* acc, int N, int C, int H, int W, int Ho, int Wo,
                           hipStream_t stream) {
    long nx, ny, npos;
    const int rc = gs_check("grid_sample_grad", N, C, H, W, Ho, Wo, &nx, &ny, &npos);
    if (rc) return rc;
    LA_CHECK_ARG(dy && grid, "grid_sample_grad: null pointer");
    LA_CHECK_ARG(dx || dgrid, "grid_sample_grad: neither dx nor dgrid asked for");
    LA_CHECK_ARG(!dgrid || x, "grid_sample_grad: dgrid needs x");
    LA_CHECK_ARG(!dx || acc, "grid_sample_grad: the float16 dx needs the fp32 workspace (la_grid_sample_grad_workspace_floats)");
    if (dx) LA_HIP(hipMemsetAsync(acc, 0, (size_t)nx * sizeof(ACC), stream));
    hipLaunchKernelGGL((la_grid_sample_bwd_kernel<T, ACC>), dim3((unsigned)la_cdiv(npos, LA_GS_BLOCK)), dim3(LA_GS_BLOCK), 0, stream, dy, x, grid,
                       dx ? acc : (ACC*)nullptr, dgrid, C, H, W, Ho * Wo, npos);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

extern "C" int la_grid_sample_f32(const float* x, const float* grid, float* y, int N, int C, int H, int W, int Ho, int Wo, hipStream_t stream) {
    return grid_sample_fwd<float>(x, grid, y, N, C, H, W, Ho, Wo, stream);
}
extern "C" int la_grid_sample_f16(const unsigned short* x, const unsigned short* grid, unsigned short* y, int N, int C, int H, int W, int Ho, int Wo,
                                  hipStream_t stream) {
    return grid_sample_fwd<__half>((const __half*)x, (const __half*)grid, (__half*)y, N, C, H, W, Ho, Wo, stream);
}
extern "C" int la_grid_sample_f64(const double* x, const double* grid, double* y, int N, int C, int H, int W, int Ho, int Wo, hipStream_t stream) {
    return grid_sample_fwd<double>(x, grid, y, N, C, H, W, Ho, Wo, stream);
}
extern "C" int la_grid_sample_grad_f32(const float* dy, const float* x, const float* grid, float* dx, float* dgrid, int N, int C, int H, int W,
                                       int Ho, int Wo, hipStream_t stream) {
    return grid_sample_bwd<float, float>(dy, x, grid, dx, dgrid, dx, N, C, H, W, Ho, Wo, stream);
}
extern "C" int la_grid_sample_grad_f64(const double* dy, const double* x, const double* grid, double* dx, double* dgrid, int N, int C, int H, int W,
                                       int Ho, int Wo, hipStream_t stream) {
    return grid_sample_bwd<double, double>(dy, x, grid, dx, dgrid, dx, N, C, H, W, Ho, Wo, stream);
}
extern "C" long la_grid_sample_grad_workspace_floats(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || (double)N * C * H * W > (double)INT_MAX) return 0;
    return (long)N * C * H * W;
}
extern "C" int la_grid_sample_grad_f16(const unsigned short* dy, const unsigned short* x, const unsigned short* grid, unsigned short* dx,
                                       unsigned short* dgrid, float* ws, int N, int C, int H, int W, int Ho, int Wo, hipStream_t stream) {
    const int rc = grid_sample_bwd<__half, float>((const __half*)dy, (const __half*)x, (const __half*)grid, (__half*)dx, (__half*)dgrid, ws, N, C, H,
                                                  W, Ho, Wo, stream);
    if (rc || !dx) return rc;
    const long nx = (long)N * C * H * W;
    long blocks = la_cdiv(nx, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_gs_round_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ws, (__half*)dx, nx);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// ------------------------------------------------------------------------------------------------------------
// fma (fma.py): y = a * b + c over the broadcast shape (rank 4, operands left-padded with 1s by the caller, stride 0 along an axis an
// operand broadcasts); c NULL = 0.  One fused multiply-add per element: a single rounding.
struct LaFmaArgs {
    const float *a, *b, *c;
    float* y;
    unsigned n, d1, d2, d3;      // elements; sizes of axes 1..3
    long as[4], bs[4], cs[4];
};

__global__ __launch_bounds__(256) void la_fma_kernel(LaFmaArgs p) {
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
        unsigned r = i;
        const unsigned i3 = r % p.d3; r /= p.d3;
        const unsigned i2 = r % p.d2; r /= p.d2;
        const unsigned i1 = r % p.d1; r /= p.d1;
        const float a = p.a[r * p.as[0] + i1 * p.as[1] + i2 * p.as[2] + i3 * p.as[3]];
        const float b = p.b[r * p.bs[0] + i1 * p.bs[1] + i2 * p.bs[2] + i3 * p.bs[3]];
        const float c = p.c ? p.c[r * p.cs[0] + i1 * p.cs[1] + i2 * p.cs[2] + i3 * p.cs[3]] : 0.f;
        p.y[i] = fmaf(a, b, c);
        if (stride > ~0u - i) break;      // (the next index would wrap)
    }
}

extern "C" int la_fma_f32(const float* a, const float* b, const float* c, float* y, const long* shape_host, const long* astride_host,
                          const long* bstride_host, const long* cstride_host, hipStream_t stream) {
    LA_CHECK_ARG(a && b && y && shape_host && astride_host && bstride_host && (!c || cstride_host), "fma: null pointer");
    double n = 1;
    for (int k = 0; k < 4; ++k) {
        LA_CHECK_ARG(shape_host[k] >= 1, "fma: empty or negative shape");
        LA_CHECK_ARG(astride_host[k] >= 0 && bstride_host[k] >= 0 && (!c || cstride_host[k] >= 0), "fma: negative stride");
        n *= (double)shape_host[k];
    }
    LA_CHECK_ARG(n <= (double)INT_MAX, "fma: more than INT_MAX elements: refused");
    LaFmaArgs p;
    p.a = a; p.b = b; p.c = c; p.y = y;
    p.n = (unsigned)n; p.d1 = (unsigned)shape_host[1]; p.d2 = (unsigned)shape_host[2]; p.d3 = (unsigned)shape_host[3];
    for (int k = 0; k < 4; ++k) { p.as[k] = astride_host[k]; p.bs[k] = bstride_host[k]; p.cs[k] = c ? cstride_host[k] : 0; }
    long blocks = la_cdiv((long)p.n, 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(la_fma_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    LA_CHECK_LAUNCH();
    return LA_OK;
}

// Un-broadcast sum (fma.py:49-58 _unbroadcast): x contiguous [s0][s1][s2][s3] -> out contiguous [o0][o1][o2][o3], o_k = s_k (axis kept)
// or 1 (axis summed).  Every output element adds its terms in double and rounds once; which thread adds what, and in which order, depends
// on the shapes alone, so two runs give the same bits.
struct LaUnbArgs {
    const float* x;
    float* out;
    long nout, nred;
    long o[4];         // output shape
    long r[4];         // summed extent per axis (1 where the axis is kept)
    long xs[4];        // strides of x
};

__device__ __forceinline__ long la_unb_base(const LaUnbArgs& p, long j) {
    long base = 0;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        base += (j % p.o[k]) * p.xs[k];
        j /= p.o[k];
    }
    return base;
}

// the innermost axis is kept: one thread per output element, consecutive lanes along that axis, the summed axes walked serially
__global__ __launch_bounds__(256) void la_unbroadcast_rows_kernel(LaUnbArgs p) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= p.nout) return;
    const float* q = p.x + la_unb_base(p, j);
    double acc = 0.0;
    for (long k0 = 0; k0 < p.r[0]; ++k0)
        for (long k1 = 0; k1 < p.r[1]; ++k1)
            for (long k2 = 0; k2 < p.r[2]; ++k2) acc += (double)q[k0 * p.xs[0] + k1 * p.xs[1] + k2 * p.xs[2]];
    p.out[j] = (float)acc;
}

// anything else: one workgroup per output element, thread t takes terms t, t + 256, ...; wave shuffles and four LDS slots in a fixed order
__global__ __launch_bounds__(256) void la_unbroadcast_block_kernel(LaUnbArgs p) {
    __shared__ double red[4];
    const float* q = p.x + la_unb_base(p, blockIdx.x);
    double acc = 0.0;
    for (long t = threadIdx.x; t < p.nred; t += 256) {
        long r = t, off = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            off += (r % p.r[k]) * p.xs[k];
            r /= p.r[k];
        }
        acc += (double)q[off];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.out[blockIdx.x] = (float)(red[0] + red[1] + red[2] + red[3]);
}

#define LA_UNB_ROWS_MIN 256      // outputs from which the one-thread-per-output form is used (when the innermost axis is kept)

extern "C" int la_unbroadcast_sum_f32(const float* x, float* out, const long* shape_host, const long* out_shape_host, hipStream_t stream) {
    LA_CHECK_ARG(x && out && shape_host && out_shape_host, "unbroadcast_sum: null pointer");
    LaUnbArgs p;
    p.x = x; p.out = out;
    double n = 1;
    p.nout = 1; p.nred = 1;
    for (int k = 0; k < 4; ++k) {
        const long s = shape_host[k], o = out_shape_host[k];
        LA_CHECK_ARG(s >= 1, "unbroadcast_sum: empty or negative shape");
        LA_CHECK_ARG(o == s || o == 1, "unbroadcast_sum: an output axis is neither the input's nor 1");
        n *= (double)s;
        p.o[k] = o; p.r[k] = s / o;
        p.nout *= o;
    }
    LA_CHECK_ARG(n <= (double)INT_MAX, "unbroadcast_sum: more than INT_MAX elements: refused");
    p.nred = (long)n / p.nout;
    p.xs[3] = 1; p.xs[2] = shape_host[3]; p.xs[1] = shape_host[2] * shape_host[3]; p.xs[0] = shape_host[1] * shape_host[2] * shape_host[3];
    if (p.r[3] == 1 && p.nout >= LA_UNB_ROWS_MIN) {
        hipLaunchKernelGGL(la_unbroadcast_rows_kernel, dim3((unsigned)la_cdiv(p.nout, 256)), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(la_unbroadcast_block_kernel, dim3((unsigned)p.nout), dim3(256), 0, stream, p);
    }
    LA_CHECK_LAUNCH();
    return LA_OK;
}
