// Host-side records that the engines (la_synth.hip, la_disc.hip, la_feat.hip) hand to the launchers (la_modconv.hip, la_upfirdn2d.hip,
// la_conv.hip): the three groups of values that used to travel as runs of positional arguments.
#pragma once

// Epilogue of a SynthesisLayer: y = clamp(act(acc * demod[b][m] + noise * noise_strength + bias[m]) * gain).  The field order is the
// forward run of LaConvArgs and FirArgs (the seam records order bias before noise: la_seam_set_epi fills those).
struct LaLayerEpi {
    const float* demod; int demod_stride;      // [B][demod_stride] or null
    const float* noise; long noise_bstride;    // [H][W] (noise_bstride 0) or [B][H][W], or null
    float noise_strength;
    const float* bias;                         // [M] or null
    int act; float alpha, gain, clamp;         // clamp < 0: none
};
// S: LaSeamFuse (la_conv.h) or LaSeamArgs (la_style.h)
template <class S>
static inline void la_seam_set_epi(S& s, const LaLayerEpi& e) {
    s.demod = e.demod; s.demod_stride = e.demod_stride; s.bias = e.bias;
    s.noise = e.noise; s.noise_bstride = e.noise_bstride; s.noise_strength = e.noise_strength;
    s.act = e.act; s.alpha = e.alpha; s.gain = e.gain; s.clamp = e.clamp;
}

// Rows [row_lo, row_hi) x columns [col_lo, col_hi) of a plane.  On either axis hi == 0 (with lo == 0) means all of it; a column window
// needs a row window.
struct LaWindow { int row_lo, row_hi, col_lo, col_hi; };
// one axis of a window: [lo, hi) grown by `below` / `above` and clipped to [0, size) ...
static inline void la_span_grow(int& lo, int& hi, int below, int above, int size) {
    lo = lo - below > 0 ? lo - below : 0;
    hi = hi + above < size ? hi + above : size;
}
// ... and widened to whole tiles of t (a power of two)
static inline void la_span_tiles(int& lo, int& hi, int t, int size) {
    lo &= ~(t - 1);
    hi = (hi + t - 1) & ~(t - 1);
    if (hi > size) hi = size;
}

// Geometry of one upfirdn2d call (upfirdn2d.py:167-211).
struct LaFirGeom {
    int fh, fw, upx, upy, dnx, dny, padx0, padx1, pady0, pady1, flip_filter;
    float gain;
};
static inline LaFirGeom la_fir_geom4(int up, int dn, int pad0, int pad1, int flip, float gain) {
    return LaFirGeom{4, 4, up, up, dn, dn, pad0, pad1, pad0, pad1, flip, gain};
}
// The five 4x4 geometries of the engines; gain and flip are arguments where the generator and the discriminator differ.
// upsample2d: up 2, pad (2,1,2,1), gain up^2 (upfirdn2d.py:342-348); its adjoint in the discriminator's skip branch flips, with gain 1
static inline LaFirGeom la_fir_up2(int flip = 0, float gain = 4.f) { return la_fir_geom4(2, 1, 2, 1, flip, gain); }
// adjoint of upsample2d: flipped taps, decimate 2, pad (1,1,1,1), same gain (upfirdn2d.py:255-266 via :342-348)
static inline LaFirGeom la_fir_down2_adjoint() { return la_fir_geom4(1, 2, 1, 1, 1, 4.f); }
// FIR after a transposed stride-2 conv: pad (1,1,1,1), gain up^2 (conv2d_resample.py:119-126); the discriminator's backward runs it
// flipped with gain 1 as the adjoint of same_pad2
static inline LaFirGeom la_fir_same_pad1(int flip = 0, float gain = 4.f) { return la_fir_geom4(1, 1, 1, 1, flip, gain); }
// adjoint of same_pad1: pad fw - 1 - pad = 2 per side, flipped, same gain (upfirdn2d.py:255-266); without the flip and with gain 1 the
// pre-filter of the discriminator's stride-2 conv (conv2d_resample.py:106-109)
static inline LaFirGeom la_fir_same_pad2(int flip, float gain) { return la_fir_geom4(1, 1, 2, 2, flip, gain); }
// the discriminator's skip branch: FIR pad (1,1,1,1) + decimate 2 (conv2d_resample.py:94-97)
static inline LaFirGeom la_fir_down2() { return la_fir_geom4(1, 2, 1, 1, 0, 1.f); }
