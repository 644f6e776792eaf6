// The sampled problem source (bsx_run_attract_sampled, bsx_sample_problems; include/bsx.h has the normative
// definition): sample j of a seed is a problem of the current space, a pure function of (seed, j).  Plain C++ with
// optional __host__ __device__ (as bsx_walk.h, bsx_wtrans.h and bsx_ranks.h), so that tests/sample_check.cpp drives
// exactly this code with the host compiler and no HIP include path.
//
// All arithmetic is mod 2^64.
//     G      = 0x9E3779B97F4A7C15
//     mix(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
//     k0     = mix(seed + G)
//     kb(b)  = mix(k0 + G * (b + 1))                     b = j >> 6   (a block of 64 samples)
//     A(b,a) = mix(kb(b) + G * (a + 1))                  a = 0 .. n_any-1, the order of any_nodes
//     U(j)   = mix(kb(j >> 6) + G * (n_any + 1 + (j & 63)))
// The a-th 'any' node of sample j has bit (j & 63) of A(j >> 6, a); its variant number is (U(j) * V) >> 64 with V the
// space's variant count.  That draw is one 64 x 64 -> high multiply: variant v is drawn for floor or ceil of 2^64 / V
// of the 2^64 values of U, so the probability of a variant differs from 1 / V by less than 2^-64, a relative bias below
// V / 2^64.
//
// One word A(b, a) serves 64 samples, two columns of the bit-sliced matrix of bsx_wide.h: the generator is evaluated
// per (row, column) of a group, never per trajectory (sample_column_word below).
#pragma once
#include <stdint.h>

#if !defined(BSX_HD)
#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#endif

namespace bsx {

constexpr uint64_t kSampleG = 0x9E3779B97F4A7C15ull;

BSX_HD uint64_t sample_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

BSX_HD uint64_t sample_k0(uint64_t seed) { return sample_mix(seed + kSampleG); }
// key of block b (samples 64 b .. 64 b + 63)
BSX_HD uint64_t sample_block_key(uint64_t k0, uint64_t b) { return sample_mix(k0 + kSampleG * (b + 1)); }
// A(b, a): bit i = state of the a-th 'any' node in sample 64 b + i
BSX_HD uint64_t sample_any_word(uint64_t kb, uint32_t a) { return sample_mix(kb + kSampleG * ((uint64_t)a + 1)); }
// U(j) of the sample with lane = j & 63 in the block of key kb
BSX_HD uint64_t sample_u(uint64_t kb, uint32_t n_any, uint32_t lane) {
    return sample_mix(kb + kSampleG * ((uint64_t)n_any + 1 + lane));
}

// (u * v) >> 64
BSX_HD uint64_t sample_mulhi(uint64_t u, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(u, v);
#else
    return (uint64_t)(((unsigned __int128)u * v) >> 64);
#endif
}
BSX_HD uint64_t sample_variant(uint64_t u, uint64_t variant_count) { return sample_mulhi(u, variant_count); }

// The block keys a column of 32 consecutive samples j0 .. j0 + 31 needs: the block of j0 and the one behind it (read
// only where the column straddles the two).  Computed once per column of a group, not once per row.
struct SampleColumn {
    uint64_t kb0, kb1;
    uint32_t shift;         // j0 & 63
};
BSX_HD SampleColumn sample_column(uint64_t k0, uint64_t j0) {
    const uint64_t b = j0 >> 6;
    return SampleColumn{sample_block_key(k0, b), sample_block_key(k0, b + 1), (uint32_t)(j0 & 63u)};
}

// The word the kernel stores into row any_nodes[a] of a column: bit i = the a-th 'any' node of sample j0 + i for
// i < n_bits (<= 32), 0 above.  j0 need not be aligned: bits that lie past the block of j0 come from the next one.
BSX_HD uint32_t sample_column_word(const SampleColumn& col, uint32_t a, uint32_t n_bits) {
    if (n_bits == 0) return 0u;
    uint64_t w = sample_any_word(col.kb0, a) >> col.shift;
    if (col.shift + n_bits > 64u) w |= sample_any_word(col.kb1, a) << (64u - col.shift);      // (shift > 32 here)
    const uint32_t valid = n_bits >= 32u ? 0xFFFFFFFFu : (1u << n_bits) - 1u;
    return (uint32_t)w & valid;
}

// Key of the block of sample j0 + i (i < 32) of a column, and that sample's lane in it
BSX_HD uint64_t sample_column_key(const SampleColumn& col, uint32_t i) { return col.shift + i >= 64u ? col.kb1 : col.kb0; }
BSX_HD uint32_t sample_column_lane(const SampleColumn& col, uint32_t i) { return (col.shift + i) & 63u; }

// One sample on its own (bsx_sample_problems): the state bit of its a-th 'any' node, its variant number
BSX_HD uint32_t sample_any_bit(uint64_t kb, uint32_t a, uint64_t j) { return (uint32_t)((sample_any_word(kb, a) >> (j & 63u)) & 1ull); }
BSX_HD uint64_t sample_variant_of(uint64_t kb, uint32_t n_any, uint64_t j, uint64_t variant_count) {
    return sample_variant(sample_u(kb, n_any, (uint32_t)(j & 63u)), variant_count);
}

// ---- damage spreading (bsx_run_damage_sampled; include/bsx.h has the normative definition) ----
// Sample j's partner y(0) is its x(0) with h distinct free nodes inverted (`free`: the ascending nodes the origin does not fix,
// n_free of them).  Flip i = 0 .. h-1 draws
//     D(j, i) = mix(kb(j >> 6) + G * (n_any + 65 + 64 i + lane))          lane = j & 63
//     p       = (D(j, i) * (n_free - i)) >> 64
// and then, for every position c chosen earlier in ascending order, p += 1 if p >= c: p is the position of the p-th free
// node not chosen yet.  That is how it is computed here: `chosen` is a bit mask over the positions (bit c & 31 of word
// c >> 5, the words `stride` apart so that a kernel can interleave the masks of its trajectories), and the p-th zero bit
// is found word by word.  The arguments of D lie past those of A (1 .. n_any) and U (n_any + 1 .. n_any + 64).
BSX_HD uint64_t damage_draw(uint64_t kb, uint32_t n_any, uint32_t lane, uint32_t i) {
    return sample_mix(kb + kSampleG * ((uint64_t)n_any + 65u + 64ull * i + lane));
}

// Position of flip i (i positions are set in `chosen`, i < n_free) for the draw d; sets its bit and returns it.
BSX_HD uint32_t damage_choose(uint64_t d, uint32_t n_free, uint32_t i, uint32_t* chosen, uint32_t stride) {
    uint32_t p = (uint32_t)sample_mulhi(d, (uint64_t)(n_free - i));        // < n_free - i: the zero bits below n_free
    const uint32_t n_words = (n_free + 31u) >> 5;
    for (uint32_t w = 0; w < n_words; ++w) {
        uint32_t open = ~chosen[w * stride];
        const uint32_t zeros = (uint32_t)__builtin_popcount(open);
        if (p >= zeros) { p -= zeros; continue; }
        for (; p; --p) open &= open - 1u;                                   // drop the p lowest zero positions
        const uint32_t bit = (uint32_t)__builtin_ctz(open);
        chosen[w * stride] |= 1u << bit;
        return 32u * w + bit;
    }
    return n_free;      // not reached: p < n_free - i
}

}  // namespace bsx
