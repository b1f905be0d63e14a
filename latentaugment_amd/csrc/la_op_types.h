// Storage type T and arithmetic type A of the op layer's typed kernels (la_ops.hip, la_grid_sample.hip): float16 is stored as half and
// computed in fp32 with one rounding on store, float32 and float64 are computed as they are stored.
#pragma once
#include "la_common.h"

#include <hip/hip_fp16.h>

template <class T> struct LaOpType;
template <> struct LaOpType<__half> { typedef float A; };
template <> struct LaOpType<float> { typedef float A; };
template <> struct LaOpType<double> { typedef double A; };

__device__ __forceinline__ float la_op_load(__half v) { return __half2float(v); }
__device__ __forceinline__ float la_op_load(float v) { return v; }
__device__ __forceinline__ double la_op_load(double v) { return v; }
template <class T> __device__ __forceinline__ T la_op_store(typename LaOpType<T>::A v);
template <> __device__ __forceinline__ __half la_op_store<__half>(float v) { return __float2half(v); }      // (round to nearest even)
template <> __device__ __forceinline__ float la_op_store<float>(float v) { return v; }
template <> __device__ __forceinline__ double la_op_store<double>(double v) { return v; }
