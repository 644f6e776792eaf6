// Rank arithmetic of the node correlations (bsx_run_node_correlations; kernels in bsx_corr.hip): frequency-weighted
// average ranks of one column of observations, kept as exact 64-bit integers.
//
// A column is sorted by observation.  Position p of the sorted column carries the frequency f[p] of its attractor;
// P[p] = f[0] + ... + f[p - 1] is the exclusive prefix sum, P[n] = T the total frequency.  The tie group of p is the
// range [lb, ub) of positions with an equal observation.  Then W_less = P[lb], W_equal = P[ub] - P[lb] and
//     rank2 = 2 W_less + W_equal + 1 = P[lb] + P[ub] + 1          (twice the average rank)
//     d2    = rank2 - (T + 1)                                      (twice the centred rank: the weighted mean of rank2
//                                                                   is T + 1 in every column, exactly)
// With T < 2^62 rank2 <= 2 T + 1 fits 64 bits unsigned and |d2| <= T fits 64 bits signed.
//
// P[lb] and P[ub] reach every member of a tie group through two scans, which is how both the kernels and
// column_ranks() below do it: forwards, the heads of the groups put P[p] in and everybody keeps the last value put in
// (P never decreases: a running maximum); backwards, the tails put P[p + 1] in and everybody keeps the nearest one
// (a running minimum).
//
// Plain C++ with optional __host__ __device__, as bsx_planes.h: tests/corr_check.cpp compiles this header with the
// host compiler and no HIP include path and drives the functions the kernels call.
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

constexpr uint64_t kCorrTotalLimit = 1ull << 62;    // T must stay below it
constexpr uint64_t kRankNoTail = ~0ull;             // identity of the backward (minimum) scan

// what corr_total found
enum CorrTotalStatus { kCorrTotalOk = 0, kCorrTotalZeroFrequency = 1, kCorrTotalHighWord = 2, kCorrTotalTooLarge = 3 };

// T = sum of n 128-bit frequencies, given as (lo, hi) word pairs: every frequency at least 1 with its high word 0,
// and T < 2^62.  The first offence in index order decides the status; *total is written only with kCorrTotalOk.
inline CorrTotalStatus corr_total(const uint64_t* lo_hi_pairs, uint64_t n, uint64_t* total) {
    uint64_t t = 0;
    for (uint64_t q = 0; q < n; ++q) {
        const uint64_t lo = lo_hi_pairs[2 * q], hi = lo_hi_pairs[2 * q + 1];
        if (hi != 0) return kCorrTotalHighWord;
        if (lo == 0) return kCorrTotalZeroFrequency;
        if (lo >= kCorrTotalLimit || t + lo >= kCorrTotalLimit) return kCorrTotalTooLarge;     // (t < 2^62: no wrap)
        t += lo;
    }
    *total = t;
    return kCorrTotalOk;
}

// position p is the first / the last of its tie group (prev_key / next_key are not looked at at the column's ends)
BSX_HD bool tie_head(uint64_t p, uint64_t prev_key, uint64_t key) { return p == 0 || prev_key != key; }
BSX_HD bool tie_tail(uint64_t p, uint64_t n, uint64_t key, uint64_t next_key) { return p + 1 == n || next_key != key; }

// what a position puts into the two scans, and how two neighbours combine
BSX_HD uint64_t head_value(bool head, uint64_t p_excl) { return head ? p_excl : 0ull; }
BSX_HD uint64_t tail_value(bool tail, uint64_t p_incl) { return tail ? p_incl : kRankNoTail; }
BSX_HD uint64_t keep_last_head(uint64_t earlier, uint64_t later) { return earlier > later ? earlier : later; }
BSX_HD uint64_t keep_nearest_tail(uint64_t a, uint64_t b) { return a < b ? a : b; }

BSX_HD uint64_t rank2_of(uint64_t p_lb, uint64_t p_ub) { return p_lb + p_ub + 1ull; }
BSX_HD int64_t centred2_of(uint64_t rank2, uint64_t total) { return (int64_t)rank2 - (int64_t)(total + 1ull); }
// the average rank as the nearest double: one rounding of the integer, the halving is exact
BSX_HD double average_rank_of(uint64_t rank2) { return (double)rank2 * 0.5; }

// One sorted column, serially, with the two scans of the kernels.  sorted_keys ascending; freq[p] the frequency at
// sorted position p.  lo / rank2 / d2: n entries each (lo is scratch).
inline void column_ranks(const uint64_t* sorted_keys, const uint64_t* freq, uint64_t n, uint64_t total, uint64_t* lo,
                         uint64_t* rank2, int64_t* d2) {
    uint64_t p_excl = 0, carry = 0;
    for (uint64_t p = 0; p < n; ++p) {
        const bool head = tie_head(p, p ? sorted_keys[p - 1] : 0ull, sorted_keys[p]);
        carry = keep_last_head(carry, head_value(head, p_excl));
        lo[p] = carry;
        p_excl += freq[p];
    }
    uint64_t p_incl = p_excl, near = kRankNoTail;       // p_excl is T now
    for (uint64_t p = n; p-- > 0;) {
        const bool tail = tie_tail(p, n, sorted_keys[p], p + 1 < n ? sorted_keys[p + 1] : 0ull);
        near = keep_nearest_tail(near, tail_value(tail, p_incl));
        rank2[p] = rank2_of(lo[p], near);
        d2[p] = centred2_of(rank2[p], total);
        p_incl -= freq[p];
    }
}

}  // namespace bsx
