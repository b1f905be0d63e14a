// Stand-alone host check of the geometric warps' position-to-corner arithmetic (latentaugment_amd/csrc/la_geom_index.h), built by
// tests/test_geometric_cpu.py with -fsanitize=undefined,address: a float-to-int conversion of a value an int cannot hold, or a signed
// overflow in the fold or corner arithmetic, stops the program.  Feeds la_geom_axis<float> and <double>, in the three padding modes, NaN,
// +-inf, +-1e30, the largest finite values, +-2^23 and its neighbours, and every quarter-pixel position from -4.5 periods to +4.5 periods
// (a period = 2 * size) for several sizes; reads a pixel through every corner reported as addressable from an array of exactly `size`
// elements (so that a wrong index is an address error), fails if a corner with a non-zero weight or an addressable mark lies outside
// [0, size), and prints one line per input for the test to compare with numpy:
//   <type> <mode> <size> <p as a hex float> <i0> <w0 hex> <w1 hex> <in0> <in1>
#include <limits>
#include <math.h>
#include <stdio.h>
#include <vector>

#include "la_geom_index.h"

template <class A>
static int run(const char* type, int mode, int size) {
    std::vector<A> ps;
    const A inf = std::numeric_limits<A>::infinity(), big = std::numeric_limits<A>::max(), lim = (A)LA_GEOM_PMAX;
    for (A v : {std::numeric_limits<A>::quiet_NaN(), inf, -inf, (A)1e30, (A)-1e30, big, -big, (A)3e9, (A)-3e9, lim, -lim, lim + (A)1, -lim - (A)1,
                (A)nextafter((double)lim, 0.0), (A)-nextafter((double)lim, 0.0), lim * (A)2, -lim * (A)2})
        ps.push_back(v);
    for (int q = -4 * 9 * size; q <= 4 * 9 * size; ++q) ps.push_back((A)q / (A)4);
    std::vector<A> pixels(size, (A)1);
    int bad = 0;
    for (A p : ps) {
        const LaGsAxis<A> r = la_geom_axis<A>(p, size, mode);
        A touched = 0;
        if (r.in0) touched += pixels[r.i0];
        if (r.in1) touched += pixels[r.i0 + 1];
        if (r.w0 != (A)0 && !(r.in0 && r.i0 >= 0 && r.i0 < size)) ++bad;
        if (r.w1 != (A)0 && !(r.in1 && r.i0 + 1 >= 0 && r.i0 + 1 < size)) ++bad;
        if ((r.in0 && (r.i0 < 0 || r.i0 >= size)) || (r.in1 && (r.i0 + 1 < 0 || r.i0 + 1 >= size))) ++bad;
        printf("%s %d %d %a %d %a %a %d %d %g\n", type, mode, size, (double)p, r.i0, (double)r.w0, (double)r.w1, (int)r.in0, (int)r.in1, (double)touched);
    }
    return bad;
}

int main() {
    int bad = 0;
    for (int mode : {LA_GEOM_ZEROS, LA_GEOM_BORDER, LA_GEOM_REFLECTION})
        for (int size : {1, 2, 5, 8}) bad += run<float>("f32", mode, size) + run<double>("f64", mode, size);
    if (bad) fprintf(stderr, "%d corners with a weight or marked addressable lie outside the image\n", bad);
    return bad ? 1 : 0;
}
