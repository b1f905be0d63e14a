// Stand-alone host check of grid_sample's position-to-corner arithmetic (latentaugment_amd/csrc/la_grid_sample_index.h), built by
// tests/test_grid_sample_cpu.py with -fsanitize=undefined,address: a float-to-int conversion of a value an int cannot hold, or a signed
// overflow in the corner arithmetic, stops the program.  Feeds la_gs_axis<float> and <double> +-1e30, +-inf, NaN, the largest finite
// values and every quarter-pixel position from -2 to size + 2 (sent as g = (2 pos + 1) / size - 1) for several sizes, reads a pixel
// through every corner it reports as inside from an array of exactly `size` elements (so that a wrong index is an address error), fails
// if a corner with a non-zero weight lies outside [0, size), and prints one line per input for the test to compare with numpy:
//   <type> <size> <g as a hex float> <i0> <w0 hex> <w1 hex> <in0> <in1>
#include <float.h>
#include <limits>
#include <stdio.h>
#include <vector>

#include "la_grid_sample_index.h"

template <class A>
static int run(const char* type, int size) {
    std::vector<A> g;
    const A inf = std::numeric_limits<A>::infinity(), big = std::numeric_limits<A>::max();
    for (A v : {(A)1e30, (A)-1e30, inf, -inf, std::numeric_limits<A>::quiet_NaN(), big, -big, (A)3e9, (A)-3e9, (A)3, (A)-3}) g.push_back(v);
    for (int q = -8; q <= 4 * (size + 2); ++q) g.push_back((A)(2 * (q / (A)4) + 1) / (A)size - (A)1);
    std::vector<A> pixels(size, (A)1);
    int bad = 0;
    for (A v : g) {
        const LaGsAxis<A> r = la_gs_axis<A>(v, size);
        A touched = 0;
        if (r.in0) touched += pixels[r.i0];
        if (r.in1) touched += pixels[r.i0 + 1];
        if (r.w0 != (A)0 && !(r.in0 && r.i0 >= 0 && r.i0 < size)) ++bad;
        if (r.w1 != (A)0 && !(r.in1 && r.i0 + 1 >= 0 && r.i0 + 1 < size)) ++bad;
        if ((r.in0 && (r.i0 < 0 || r.i0 >= size)) || (r.in1 && (r.i0 + 1 < 0 || r.i0 + 1 >= size))) ++bad;
        printf("%s %d %a %d %a %a %d %d %g\n", type, size, (double)v, r.i0, (double)r.w0, (double)r.w1, (int)r.in0, (int)r.in1, (double)touched);
    }
    return bad;
}

int main() {
    int bad = 0;
    for (int size : {1, 2, 4, 7, 8, 256}) bad += run<float>("f32", size) + run<double>("f64", size);
    if (bad) fprintf(stderr, "%d corners with a weight or marked inside lie outside the image\n", bad);
    return bad ? 1 : 0;
}
