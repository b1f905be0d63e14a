// The library's counter-based noise stream (device code; gfx950 / CDNA4 only): the one definition of the generator, of its counter
// convention and of the two maps from words to values.  A kernel file does not write its own.
#pragma once
#include "la_common.h"

// Counter-based unit normals for the explicit noise tensors of noise_mode='random' (the reference draws torch.randn per layer inside
// G.synthesis, util_latent_aug.py:308 / SURVEY 3.4 defect g; a draw cannot be bit-equal to another library's stream, it only has to
// be N(0, 1) and reproducible).  Element e of GLOBAL sample row r of stream (layer) l under `seed` is a pure function of (seed, l, r, e):
// Philox4x32-10 (Salmon et al., SC'11) with counter (e / 4, r, l, high word of e / 4) and key (seed low, seed high) gives four 32-bit
// words, two Box-Muller pairs turn them into elements 4 (e / 4) .. 4 (e / 4) + 3.  A rank that holds rows [row0, row0 + rows) of a
// batch therefore generates exactly its rows -- nothing of the other ranks' -- and the gathered batch does not depend on the sharding.
__device__ __forceinline__ void la_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// the four words of 4-element group q of global row `row` of stream `stream`: counter (q, row, stream, high word of q), key (k0, k1)
__device__ __forceinline__ void la_noise_words(long q, long row, unsigned stream, unsigned k0, unsigned k1, unsigned (&x)[4]) {
    la_philox4x32_10((unsigned)q, (unsigned)row, stream, (unsigned)((unsigned long long)q >> 32), k0, k1, x);
}

// Four words -> four unit normals: two Box-Muller pairs, u = (k + 0.5) * 2^-24 with k the word's top 24 bits.  In float32 k + 0.5
// needs 25 bits once k >= 2^23 and rounds to even there: the upper half of the range loses the offset, and u1 can be exactly 1
// (radius 0, both values of the pair 0).  It can never be 0, so no logarithm is infinite and no value is NaN.
// oracle/noise_ref.py copies this float32 rounding; the formula is pinned bit for bit and does not change.
__device__ __forceinline__ void la_unit_normals4(const unsigned (&x)[4], float (&z)[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(x[2 * h] >> 8) + 0.5f) * (1.f / 16777216.f);
        const float u2 = ((float)(x[2 * h + 1] >> 8) + 0.5f) * (1.f / 16777216.f);
        const float rad = sqrtf(-2.f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
    }
}

// One word -> one value in (-1, 1): (k + 0.5) * 2^-22 - 1 with k the top 23 bits, i.e. (2k + 1 - 2^23) * 2^-23, an odd numerator
// below 2^23 -- exact in float32, never -1, 0 or 1.
__device__ __forceinline__ float la_unit_uniform(unsigned word) { return ((float)(word >> 9) + 0.5f) * (1.f / 4194304.f) - 1.f; }

// The UMAP embedding's draws (la_umap.hip) use the same generator under two stream constants that no layer or caller-chosen stream
// id of the noise entries reaches, and their own counter convention -- again a pure function of GLOBAL indices, so that a row gives
// the same bits in any batch:
//   negative samples   counter (position t of the entry in its CSR row, global head row, LA_RNG_STREAM_UMAP_NEG, epoch * 8 + group),
//                      key (seed low, seed high): word u of group g is draw 4 g + u of that entry in that epoch (at most 32 draws,
//                      8 groups; epoch < 2^28); the sampled row is (word * n_tail) >> 32
//   initial layout     counter (c / 4, global row, LA_RNG_STREAM_UMAP_INIT, 0): word c % 4 is coordinate c, 10 * la_unit_uniform(word)
#define LA_RNG_STREAM_UMAP_NEG 0x554D4150u       // 'UMAP'
#define LA_RNG_STREAM_UMAP_INIT 0x554D4149u
#define LA_UMAP_MAX_EPOCHS (1 << 28)
__device__ __forceinline__ void la_umap_neg_words(int t, long head_row, int epoch, int group, unsigned k0, unsigned k1, unsigned (&x)[4]) {
    la_philox4x32_10((unsigned)t, (unsigned)head_row, LA_RNG_STREAM_UMAP_NEG, ((unsigned)epoch << 3) | (unsigned)group, k0, k1, x);
}
__device__ __forceinline__ void la_umap_init_words(int group, long row, unsigned k0, unsigned k1, unsigned (&x)[4]) {
    la_philox4x32_10((unsigned)group, (unsigned)row, LA_RNG_STREAM_UMAP_INIT, 0u, k0, k1, x);
}

// The sliced Wasserstein distance's draws (la_swd.hip), under two more constants that nothing else reaches:
//   patch positions    counter (patch j of the image, global image, LA_RNG_STREAM_SWD_POS, pyramid level), key (seed low, seed high):
//                      the corner is x0 = (word 0 * (W - nhood + 1)) >> 32, y0 = (word 1 * (H - nhood + 1)) >> 32 -- integers only
//   directions         la_noise_words(q, global direction, LA_RNG_STREAM_SWD_DIR) -> la_unit_normals4: elements 4 q .. 4 q + 3 of the
//                      direction before it is divided by its norm, i.e. the noise entries' map with the direction as the row
#define LA_RNG_STREAM_SWD_POS 0x53574450u        // 'SWDP'
#define LA_RNG_STREAM_SWD_DIR 0x53574444u        // 'SWDD'
