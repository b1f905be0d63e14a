// Position-to-corner arithmetic of grid_sample (2-D, bilinear, padding_mode='zeros', align_corners=False), one axis at a time.
// Host and device: la_grid_sample.hip's kernels call it, and tests/test_grid_sample_cpu.py compiles it into a stand-alone host program
// under the sanitizers.  Nothing but <math.h> is needed, so a plain C++ compiler takes it as well as hipcc.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LA_GS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LA_GS_HD inline
#endif

LA_GS_HD float la_gs_floor(float v) { return floorf(v); }
LA_GS_HD double la_gs_floor(double v) { return floor(v); }

// One axis of one sample position: the two neighbouring pixels i0 and i0 + 1, their weights and whether each lies inside [0, size).
template <class A>
struct LaGsAxis {
    int i0;           // lower neighbour, in [-1, size - 1] (0 when the position is refused)
    A w0, w1;         // weights of i0 and i0 + 1; 0 for a neighbour outside the image (both when the position is refused)
    bool in0, in1;    // i0 / i0 + 1 addresses a pixel; a refused position has neither
};

// g in [-1, 1] spans the image edge to edge: pixel position p = ((g + 1) * size - 1) / 2, in exactly this form (positions that are
// dyadic in g then come out exact).  The range test is done on p in floating point, BEFORE any conversion to int: a position outside
// [-1, size) -- huge, infinite or NaN included (every comparison with NaN is false) -- has no neighbour inside the image and is refused
// with zero weights, so no int is ever formed from a value it cannot hold and no address from such an int.  Inside the range
// floor(p) is in [-1, size - 1].  The weights are torch's (GridSampler: ix_se - ix, ix - ix_nw), both differences formed from p;
// a neighbour outside the image gets weight 0 (its pixel value is 0 in every term of y, dx and dgrid, so nothing changes by that).
template <class A>
LA_GS_HD LaGsAxis<A> la_gs_axis(A g, int size) {
    LaGsAxis<A> r;
    const A p = ((g + (A)1) * (A)size - (A)1) / (A)2;
    if (!(p >= (A)-1 && p < (A)size)) {
        r.i0 = 0; r.w0 = (A)0; r.w1 = (A)0; r.in0 = false; r.in1 = false;
        return r;
    }
    const A f = la_gs_floor(p);
    r.i0 = (int)f;
    r.in0 = r.i0 >= 0;
    r.in1 = r.i0 + 1 < size;
    r.w0 = r.in0 ? (f + (A)1) - p : (A)0;
    r.w1 = r.in1 ? p - f : (A)0;
    return r;
}
