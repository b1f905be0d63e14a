// Shared definitions for the latentaug HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <memory>

// The public C ABI: every translation unit sees the prototypes, structs and LA_* constants it defines or calls from the one header
// that callers get, so a definition that disagrees with it does not compile.  (la_stream_t there is hipStream_t.)
#include "latentaug_hip.h"

#define LA_WAVE 64

void la_set_error(const char* msg);

#define LA_CHECK_ARG(cond, msg)            \
    do {                                   \
        if (!(cond)) {                     \
            la_set_error(msg);             \
            return LA_ERR_ARG;             \
        }                                  \
    } while (0)

// the one refusal of a caller-owned workspace or scratch that is smaller than its size entry reports
#define LA_CHECK_WORKSPACE(have, need, msg) \
    do {                                   \
        if ((have) < (need)) {             \
            la_set_error(msg);             \
            return LA_ERR_WORKSPACE;       \
        }                                  \
    } while (0)

#define LA_CHECK_LAUNCH()                              \
    do {                                               \
        hipError_t e__ = hipGetLastError();            \
        if (e__ != hipSuccess) {                       \
            la_set_error(hipGetErrorString(e__));      \
            return LA_ERR_HIP;                         \
        }                                              \
    } while (0)

#define LA_HIP(call)                                   \
    do {                                               \
        hipError_t e__ = (call);                       \
        if (e__ != hipSuccess) {                       \
            la_set_error(hipGetErrorString(e__));      \
            return LA_ERR_HIP;                         \
        }                                              \
    } while (0)

// kernel classes of the launch profiler (la_prof.hip); the first four are the contraction classes
enum { LA_PC_CONV_HALO = 0, LA_PC_CONV_FLAT, LA_PC_CONV_SPLITK, LA_PC_CONV_F32, LA_PC_PRESPLIT, LA_PC_FIR, LA_PC_SEAM, LA_PC_TORGB,
       LA_PC_BANK, LA_PC_NCLASS };
bool la_prof_enabled();      // profiler active: callers keep their launches eager
// Settings generation of an engine handle: raised by every setter that changes what the engine's following passes launch (precision,
// ToRGB schedule).  The latent loop records the three at capture and drops a captured step whose engines have been set since.
int la_synth_settings_gen(const la_synth* h);
int la_disc_settings_gen(const la_disc* h);
int la_feat_settings_gen(const la_feat* h);
// Development switches -- kernel-variant selectors for in-process A/B measurements (la_dev_knob_set) and LA_* environment switches --
// exist in the DEVELOPMENT build only (make dev: -DLA_DEV, liblatentaug_hip_dev.so, used by scripts/).  The product library has
// neither: every knob reads 0, no LA_* variable is looked at, la_dev_knob_set is not exported.
#ifdef LA_DEV
int la_dev_knob(int id);
const char* la_dev_env(const char* name);      // getenv
#else
static inline int la_dev_knob(int) { return 0; }
static inline const char* la_dev_env(const char*) { return nullptr; }
#endif
#define LA_KNOB_HALO_MING 1   // dev: grids of fewer points than this go to split-K instead of the halo kernel (0 = 1157: up to 34x34)
#define LA_KNOB_KSPLIT 3       // dev: force this many K slices on the split-K launches (0 = the cost model's choice)
#define LA_KNOB_HALO_STAMP 5   // dev: 1 = the MF 21 halo kernel records per-wave segment clocks (la_dev_dbg_read)
#define LA_KNOB_HALO_LDSPAD 6  // dev: extra KB of LDS per workgroup of the MF 21 halo kernel (occupancy experiments)
#define LA_NKNOB 16
int la_prof_open(int cls, double flops, double bytes, hipStream_t stream);     // -> slot or -1
void la_prof_close(int slot, hipStream_t stream);

static inline int la_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Workspace carving: every buffer of a caller-supplied region starts on a 64-byte boundary.  A layout function is written once
// and run twice -- with a null base to measure (take returns null, `off` ends as the bytes needed), then over the region.  A size
// is counted in elements of the buffer's own type (take<double>(n), take<int>(n)): a count converted by hand to another unit is
// where a layout goes wrong by a factor.
static inline size_t la_align64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
struct LaCarver {
    char* base = nullptr;
    size_t off = 0;
    size_t cap = 0;      // bytes behind `base` where the caller knows them (0: not given)
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += la_align64(count * sizeof(T));
        return p;
    }
    float* take(size_t nfloats) { return take<float>(nfloats); }
};
// every pointer on a multiple of N bytes (a null pointer counts as aligned: optional arguments are tested with the rest)
template <size_t N, class... P> static inline bool la_aligned(const P*... p) { return (((uintptr_t)p | ... | (uintptr_t)0) & (N - 1)) == 0; }

// A host handle (plain data, malloc'ed: the destroy entries free() it), owned by its create entry until that releases it into *out
struct LaFree { void operator()(void* p) const { free(p); } };
template <class H> using LaHostHandle = std::unique_ptr<H, LaFree>;
template <class H> static inline LaHostHandle<H> la_host_handle() { return LaHostHandle<H>((H*)malloc(sizeof(H))); }
// the *_workspace_bytes entries: `measure` describes a scratch handle and lays it out on a null base (0: bad description)
template <class H, class F> static inline size_t la_measure_workspace(F measure) {
    const LaHostHandle<H> h = la_host_handle<H>();
    return h ? measure(h.get()) : 0;
}

// ---------------------------------------------------------------- device helpers
// Reductions live here (and the noise stream in la_rng.h): a kernel file does not write its own, so that "in a fixed order" has one
// definition.  The xor butterfly over the W = 64 lanes of a wave, or inside each 32-lane half (W = 32), starting at distance W / 2:
// every lane ends with the result.  T: float, double or int.
// (Where a butterfly's result is read only under a following `if (lane == 0)`, the written-out loop and a call compile to different
// instruction schedules -- the last step is sunk into that block at another moment.  The sites of that shape which were written out
// when these helpers arrived stay written out -- la_block_max_256 below, la_op_block_sum_256 (la_ops.hip) and pp_block_sum
// (la_pathpoints.hip) among them; tests/test_host_cpu.py lists them.)
template <int W = 64, class T> __device__ __forceinline__ T la_wave_sum(T v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int W = 64> __device__ __forceinline__ float la_wave_max(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int W = 64> __device__ __forceinline__ float la_wave_min(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves).  `red` is >= 4 floats of LDS.  All threads get the result.
__device__ __forceinline__ float la_block_sum_256(float v, float* red) {
    v = la_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// Block-wide float64 sum for blockDim.x == 256 as a halving tree over 256 LDS doubles (`red`); the leading barrier lets calls follow
// one another on the same `red`.  All threads get the result, which also stays in red[0].
__device__ __forceinline__ double la_block_tree_sum_256(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// Block-wide maximum, same shape: wave shuffle, then 4 LDS floats.  Every thread of the workgroup must reach it (lanes with nothing
// to contribute pass their neutral value); all threads get the result.
__device__ __forceinline__ float la_block_max_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// output row of accumulator register r (0..15) of a 32x32 MFMA tile in the lane half lh (lane >> 5); the column is lane & 31
__device__ __host__ constexpr int la_mfma32_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// One Adam update (torch.optim.Adam, no weight decay / amsgrad) of parameter p with moments m, v and gradient g:
// step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t).  The expression shapes are fixed: results are compared bit for bit.
__device__ __forceinline__ void la_adam_update(float& p, float& m, float& v, float g, float step_size, float bc2_sqrt, float b1, float b2,
                                               float eps) {
    const float mv = b1 * m + (1.f - b1) * g;
    const float vv = b2 * v + (1.f - b2) * g * g;
    m = mv; v = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p = p - step_size * (mv / denom);
}

// Step counter of a one-launch step tail whose threads have all read *ctr (the index of this step's bias corrections): every
// workgroup draws a ticket AFTER the barrier, i.e. after its threads' reads; the one that draws the last ticket resets the ticket
// and bumps the counter -- nobody is left to read the old value.  Every thread of the workgroup must reach it.
__device__ __forceinline__ void la_step_ticket(int* ctr, int* ticket) {
    __syncthreads();      // every thread of the workgroup has read *ctr
    if (threadIdx.x == 0) {
        if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) { *ticket = 0; *ctr += 1; }
    }
}

// power-of-two operand scale of the fp16 split (la_conv_operand.hip): brings a tensor's max magnitude into [2^14, 2^15)
__device__ __forceinline__ float la_pow2_scale(float amax) {
    if (!(amax > 0.f) || !isfinite(amax)) return 1.f;
    int e;
    frexpf(amax, &e);                    // amax = f * 2^e, f in [0.5, 1)
    int s = 15 - e;                      // scaled max in [2^14, 2^15): fp16 never overflows, 3 more bits above the subnormals
    s = s > 100 ? 100 : (s < -100 ? -100 : s);
    return ldexpf(1.f, s);
}

// Running per-sample fp16 operand scale handed from a producing kernel to the contraction that consumes its output: the slot
// starts a pass at LA_XS_INIT (2^100, the largest scale la_pow2_scale returns); every producing workgroup lowers it to
// la_pow2_scale(mult * its own max) -- positive floats order like unsigned ints, so an atomicMin on the bit pattern does it, the
// result is the scale of the overall maximum whatever the arrival order, and the consumer just reads a float.  `seen` is an
// earlier (possibly stale, i.e. larger) read of the slot: workgroups that cannot lower it skip the atomic.
// A slot is a ROW of LA_XS_SUBS sub-slots per sample, each in a 128-byte line of its own (LA_XS_FAN floats per row): a producing
// workgroup lowers the sub-slot picked by its id, the consumer takes the minimum of the row (la_xs_get) -- so that a launch of thousands
// of short workgroups finishing together (the split-K finish pass, the seam kernel) spreads its atomics over 32 LINES per sample
// instead of serialising on one (device-scope atomics execute at the memory side, one line at a time: round 2 measured the
// single-address form at 21 -> 65 us and 158 -> 281 us for those two and kept a reduction launch for them; round 4 measured 32
// sub-slots inside ONE line no better, +13 us / +40 us).  The minimum of the row is the scale of the overall maximum either way.
#define LA_XS_INIT 0x71800000u
#define LA_XS_SUBS 32
#define LA_XS_LINE 32                          // floats per 128-byte line
#define LA_XS_FAN (LA_XS_SUBS * LA_XS_LINE)    // floats per slot row
__device__ __forceinline__ float la_xs_peek(const float* slot) {
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void la_xs_lower(float* slot, float seen, float mult, float wg_max) {
    if (!(wg_max > 0.f)) return;
    const float s = la_pow2_scale(mult * wg_max);
    if (s < seen) atomicMin(reinterpret_cast<unsigned*>(slot), __float_as_uint(s));
}
// sub-slot of the calling workgroup inside a row (any spread will do; the multipliers keep neighbouring workgroups of every grid apart)
// (returned as the float offset of the sub-slot inside the row)
__device__ __forceinline__ int la_xs_sub(int salt = 0) { return (int)((blockIdx.x + 7u * blockIdx.y + 13u * blockIdx.z + (unsigned)salt) & (LA_XS_SUBS - 1)) * LA_XS_LINE; }
// thread 0 of the calling workgroup lowers sub-slot la_xs_sub(salt) of sample b's row in `rows` [B][LA_XS_FAN] to the scale of wg_max
__device__ __forceinline__ void la_xs_lower_wg(float* rows, long b, float mult, float wg_max, int salt = 0) {
    if (threadIdx.x != 0) return;
    float* row = rows + b * LA_XS_FAN + la_xs_sub(salt);
    la_xs_lower(row, la_xs_peek(row), mult, wg_max);
}
// Lowering for 256-thread workgroups whose work items are consecutive planes, i.e. a handful of consecutive samples starting at b0:
// thread (sample b, maximum omax; `live` false: nothing) -- the per-sample maxima of the workgroup are collected in LDS, then one
// thread per sample lowers a sub-slot of that sample's row: one atomic per (workgroup, sample) instead of one per thread.  The LDS
// maxima are bit patterns: non-negative floats order like unsigned ints, so atomicMax on the pattern is the float maximum.  The
// table holds 64 samples; a thread whose sample lies further from b0 lowers its row directly (sub-slot spread by its thread id).
// xs_mult: per-sample multipliers (null: 1); C planes per sample, P planes in all.  Every thread of the workgroup must reach it.
__device__ __forceinline__ void la_xs_lower_by_sample(float* rows, const float* xs_mult, int b, int b0, int C, int P, bool live, float omax) {
    __shared__ unsigned smx[64];
    if (threadIdx.x < 64) smx[threadIdx.x] = 0u;
    __syncthreads();
    if (live && omax > 0.f) {
        if (b - b0 < 64) atomicMax(&smx[b - b0], __float_as_uint(omax));
        else { float* row = rows + (long)b * LA_XS_FAN + la_xs_sub(threadIdx.x); la_xs_lower(row, la_xs_peek(row), xs_mult ? xs_mult[b] : 1.f, omax); }
    }
    __syncthreads();
    const int bt = b0 + (int)threadIdx.x;
    if (threadIdx.x < 64 && smx[threadIdx.x] != 0u && bt * C < P) {
        float* row = rows + (long)bt * LA_XS_FAN + la_xs_sub();
        la_xs_lower(row, la_xs_peek(row), xs_mult ? xs_mult[bt] : 1.f, __uint_as_float(smx[threadIdx.x]));
    }
}
// final per-sample scale: plain arrays [B] (fan <= 1: scales computed by a reduction launch or known a priori) or slot rows [B][LA_XS_FAN]
__device__ __forceinline__ float la_xs_get(const float* p, int b, int fan) {
    if (fan <= 1) return p[b];
    const float* q = p + (long)b * LA_XS_FAN;
    float v[LA_XS_SUBS];
#pragma unroll
    for (int i = 0; i < LA_XS_SUBS; ++i) v[i] = q[i * LA_XS_LINE];      // (all in flight: one round trip)
    float m = v[0];
#pragma unroll
    for (int i = 1; i < LA_XS_SUBS; ++i) m = fminf(m, v[i]);
    return m;
}

// y = clamp(act(v) * gain)  (bias_act.cu:23-147 semantics, grad=0)
__device__ __forceinline__ float la_act_fwd(float v, int act, float alpha, float gain, float clamp) {
    if (act == LA_ACT_LRELU) v = v > 0.f ? v : v * alpha;
    else if (act == LA_ACT_RELU) v = v > 0.f ? v : 0.f;
    v *= gain;
    if (clamp >= 0.f) v = fminf(fmaxf(v, -clamp), clamp);
    return v;
}

// d(y)/d(v) expressed through the saved OUTPUT y, as the reference's kernel does (bias_act.cu:46-48,71-72,141):
// slope from the sign of y, zero where the clamp is active.
__device__ __forceinline__ float la_act_bwd_from_y(float y, int act, float alpha, float gain, float clamp) {
    float s = gain;
    if (act == LA_ACT_LRELU) s = y > 0.f ? gain : gain * alpha;
    else if (act == LA_ACT_RELU) s = y > 0.f ? gain : 0.f;
    if (clamp >= 0.f && fabsf(y) >= clamp) s = 0.f;
    return s;
}

// pre-activation value (x + b) recovered from the saved output (only meaningful where the clamp is inactive)
__device__ __forceinline__ float la_act_inv(float y, int act, float alpha, float gain) {
    float v = y / gain;
    if (act == LA_ACT_LRELU && v < 0.f) v = v / alpha;
    return v;
}
