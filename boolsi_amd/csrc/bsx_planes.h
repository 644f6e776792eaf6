// Vertical counters ("bit planes") of the attractor-profile kernels (bsx_profile.hip, k_wide_profile in
// bsx_wide.hip): how often was each bit of a word set over a run of words?
//
// P planes of NW words: bit i of plane j is bit j of the count of bit i.  Adding a word is a ripple carry over the
// planes -- `up = plane & carry`, `plane ^= carry`, `carry = up` -- 3 P operations per word for all its 32 bits at
// once, instead of 32 integer adds.  P planes hold counts up to 2^P - 1, so the owner flushes them into 32-bit integer counters
// every kFlushEvery adds (and at the end) and starts them from zero: any run length is exact.
//
// Plain C++ with optional __host__ __device__: tests/profile_check.cpp compiles this header with the host compiler
// and no HIP include path, and drives exactly the functions the kernels call.  Every index into the planes is a
// compile-time constant after unrolling (a dynamically indexed register array goes to scratch): bit
// positions are runtime values, words and planes never are.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#if defined(__clang__)
#define BSX_UNROLL _Pragma("unroll")
#else
#define BSX_UNROLL
#endif

namespace bsx {

template <int NW, int P>
struct Planes {
    static constexpr uint32_t kFlushEvery = (1u << P) - 1u;     // adds the planes hold without overflow
    uint32_t p[P][NW];
};

template <int NW, int P>
BSX_HD void planes_clear(Planes<NW, P>& pl) {
BSX_UNROLL
    for (int j = 0; j < P; ++j)
BSX_UNROLL
        for (int w = 0; w < NW; ++w) pl.p[j][w] = 0u;
}

// counts += bits of s (at most kFlushEvery adds between two clears)
template <int NW, int P>
BSX_HD void planes_add(Planes<NW, P>& pl, const uint32_t (&s)[NW]) {
BSX_UNROLL
    for (int w = 0; w < NW; ++w) {
        uint32_t carry = s[w];
BSX_UNROLL
        for (int j = 0; j < P; ++j) {
            const uint32_t up = pl.p[j][w] & carry;
            pl.p[j][w] ^= carry;
            carry = up;
        }
    }
}

// count of bit `bit` (0 .. 31, runtime) of word W (compile-time)
template <int W, int NW, int P>
BSX_HD uint32_t planes_count_at(const Planes<NW, P>& pl, uint32_t bit) {
    static_assert(W >= 0 && W < NW, "word index");
    uint32_t c = 0;
BSX_UNROLL
    for (int j = 0; j < P; ++j) c |= ((pl.p[j][W] >> bit) & 1u) << j;
    return c;
}

// count of bit `pos` of the NW-word string (runtime position): mask arithmetic over all words, as get_bit does
template <int NW, int P>
BSX_HD uint32_t planes_count(const Planes<NW, P>& pl, uint32_t pos) {
    uint32_t c = 0;
BSX_UNROLL
    for (int j = 0; j < P; ++j) {
        uint32_t word = 0;
BSX_UNROLL
        for (int w = 0; w < NW; ++w) word |= ((pos >> 5) == (uint32_t)w) ? pl.p[j][w] : 0u;
        c |= ((word >> (pos & 31u)) & 1u) << j;
    }
    return c;
}

template <int W, int NW, int P>
BSX_HD void planes_flush_word(const Planes<NW, P>& pl, uint32_t* row, uint32_t n_bits) {
    for (uint32_t b = 0; b < 32u && 32u * W + b < n_bits; ++b) {
        const uint32_t c = planes_count_at<W>(pl, b);
        if (c) row[32u * W + b] += c;
    }
    if constexpr (W + 1 < NW) planes_flush_word<W + 1>(pl, row, n_bits);
}

// row[i] += count of bit i for i < n_bits (<= 32 NW); the planes start from zero again.  A plain read-modify-write:
// the row has one owner.
template <int NW, int P>
BSX_HD void planes_flush(Planes<NW, P>& pl, uint32_t* row, uint32_t n_bits) {
    planes_flush_word<0>(pl, row, n_bits);
    planes_clear(pl);
}

constexpr int kProfilePlanes = 8;       // per-lane kernel: 8 NW registers, a flush every 255 states
constexpr int kWideProfilePlanes = 4;   // wide kernel: one set per owned row (up to kWideProfileRows), a flush every 15 steps

}  // namespace bsx
