// Position-to-corner arithmetic of the geometric warps (la_geom.hip), one axis at a time: bilinear sampling at a PIXEL position p (pixel
// centres at integer coordinates) under padding 'zeros', 'border' or 'reflection', align_corners=False.  Host and device, like
// la_grid_sample_index.h, whose result record (LaGsAxis), floor and qualifiers it reuses: la_geom.hip's kernels call it, and
// tests/test_geometric_cpu.py compiles it into a stand-alone host program under the sanitizers.
#pragma once
#include "la_grid_sample_index.h"

#define LA_GEOM_ZEROS 0
#define LA_GEOM_BORDER 1
#define LA_GEOM_REFLECTION 2
#define LA_GEOM_PMAX 8388608      // 2^23: positions beyond it (in magnitude) are refused

LA_GS_HD float la_geom_abs(float v) { return fabsf(v); }
LA_GS_HD double la_geom_abs(double v) { return fabs(v); }
LA_GS_HD float la_geom_mod(float a, float b) { return fmodf(a, b); }
LA_GS_HD double la_geom_mod(double a, double b) { return fmod(a, b); }

// torch's reflect_coordinates for align_corners=False: reflect p about -0.5 and size - 0.5 as often as needed (period 2 * size).
// d = |p + 0.5| is the distance from the lower mirror; r = fmod(d, size) is exact, and so is the number of whole spans (d - r) / size
// (d - r is an integer multiple of size below 2^24), which torch forms as floor(d / size): the two agree except where d / size rounds
// up to an integer, and there this form stays continuous.  An even count keeps the direction, an odd one turns it round.
template <class A>
LA_GS_HD A la_geom_reflect(A p, int size) {
    const A span = (A)size;
    const A d = la_geom_abs(p + (A)0.5);
    const A r = la_geom_mod(d, span);
    const int flips = (int)((d - r) / span);      // <= 2^23 + 1: |p| <= 2^23 was tested by the caller
    return (flips & 1) ? (span - r) - (A)0.5 : r - (A)0.5;
}

// The two neighbours of position p along an axis of `size` pixels, with their weights (LaGsAxis: i0, w0, w1, in0, in1).
//   before anything else: a position that is not finite, or beyond 2^23 in magnitude, is refused in floating point (every comparison
//     with NaN is false) -- zero weights, neither neighbour addressable, no int formed from it;
//   zeros: la_gs_axis's rule applied to p itself -- outside [-1, size) nothing, inside floor(p) in [-1, size - 1], a neighbour outside
//     the image has weight 0 and is not addressable;
//   border: p clipped to [0, size - 1];  reflection: p reflected (la_geom_reflect), then clipped the same way.  A one-pixel axis puts
//     every position on that pixel (torch: the position becomes 0).  After the clip floor(p) is in [0, size - 1] and the lower neighbour
//     is always a pixel; the upper one is i0 + 1 == size only where p == size - 1, with weight 0, and is then not addressable.
// The weights are torch's (ix_se - ix, ix - ix_nw): (floor(p) + 1) - p and p - floor(p).
template <class A>
LA_GS_HD LaGsAxis<A> la_geom_axis(A p, int size, int mode) {
    LaGsAxis<A> r;
    r.i0 = 0; r.w0 = (A)0; r.w1 = (A)0; r.in0 = false; r.in1 = false;
    if (!(la_geom_abs(p) <= (A)LA_GEOM_PMAX)) return r;
    if (mode == LA_GEOM_ZEROS) {
        if (!(p >= (A)-1 && p < (A)size)) return r;
        const A f = la_gs_floor(p);
        r.i0 = (int)f;
        r.in0 = r.i0 >= 0;
        r.in1 = r.i0 + 1 < size;
        r.w0 = r.in0 ? (f + (A)1) - p : (A)0;
        r.w1 = r.in1 ? p - f : (A)0;
        return r;
    }
    if (size == 1) {
        p = (A)0;
    } else {
        if (mode == LA_GEOM_REFLECTION) p = la_geom_reflect<A>(p, size);
        const A hi = (A)(size - 1);
        p = p < (A)0 ? (A)0 : (p > hi ? hi : p);
    }
    const A f = la_gs_floor(p);
    r.i0 = (int)f;
    r.in0 = true;
    r.in1 = r.i0 + 1 < size;
    r.w0 = (f + (A)1) - p;
    r.w1 = r.in1 ? p - f : (A)0;
    return r;
}

// Normalised coordinate g in [-1, 1] -> pixel position, in the form la_gs_axis uses (dyadic g come out exact).
template <class A>
LA_GS_HD A la_geom_unnormalize(A g, int size) { return ((g + (A)1) * (A)size - (A)1) / (A)2; }
