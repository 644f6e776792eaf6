// Attractor transitions on the wide-state family (bsx_run_attractor_transitions_wide, kernels in bsx_wide.hip): what
// is decided per flip once the lock-step walk of its group has ended, and the row-key table that decision looks into.
// Plain C++ with optional __host__ __device__ (as bsx_walk.h and bsx_ranks.h), so that tests/wtrans_check.cpp drives
// exactly this code with the host compiler and no HIP include path.
//
// A flip's walk (Brent in lock step, the mu pass, the key lap: k_wide's attract phases) ends in one of two states:
// found, with lambda' = the length of the cycle C the flip ends on, mu = the steps until it is on C and the canonical
// key of C (its minimum state); or not found, which under a finite max_t means mu + lambda' > max_t.  Rows are
// identified by their canonical keys too, so "C is row d" is one lookup of the flip's key among the n rows' keys:
//     row-key table   a power of two >= 2 n owners (row + 1, 0 = free), linear probing from wtrans_hash(key)
// The walk treats a max_t at or beyond a quarter of the step limit as unbounded; the rule below therefore compares
// mu + lambda' with max_t once more, which makes it exact for every max_t.
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

constexpr uint64_t kWtransInf = ~0ull;              // max_t: no cap (BSX_T_INF)
constexpr uint32_t kWtransNoRow = 0xFFFFFFFFu;      // lookup: the key is no row's
constexpr uint32_t kWtransOutside = 0xFFFFFFFEu;    // BSX_TRANS_OUTSIDE
constexpr uint32_t kWtransUnresolved = 0xFFFFFFFFu; // BSX_TRANS_UNRESOLVED

// Hash of a key of w64 64-bit words (every word counts, so two keys that differ only above bit 256 spread too).  The
// key is given by an accessor key_at(w) -> word w: the kernel gathers a flip's words out of the bit-sliced matrix one
// at a time and keeps no array of them.
template <typename KeyAt>
BSX_HD uint64_t wtrans_hash_of(KeyAt key_at, uint32_t w64) {
    uint64_t h = 0;
    for (uint32_t w = 0; w < w64; ++w) {
        // (the 64-bit finalizer of MurmurHash3, a bijection with full avalanche, chained over the words: the table
        // index takes the LOW bits of the result, which a multiplication alone leaves as weak as the key's low bits)
        h = (h ^ key_at(w)) + 0x9E3779B97F4A7C15ull;
        h ^= h >> 33;
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
        h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
    }
    return h;
}

BSX_HD uint64_t wtrans_hash(const uint64_t* key, uint32_t w64) {
    return wtrans_hash_of([key](uint32_t w) { return key[w]; }, w64);
}

BSX_HD bool wtrans_key_equal(const uint64_t* a, const uint64_t* b, uint32_t w64) {
    uint64_t d = 0;
    for (uint32_t w = 0; w < w64; ++w) d |= a[w] ^ b[w];
    return d == 0;
}

// -> the row whose canonical key (row_keys[row * w64 ..]) equals the key, or kWtransNoRow.  At most one round of the table.
template <typename KeyAt>
BSX_HD uint32_t wtrans_find_of(const uint32_t* owners, uint64_t slot_mask, const uint64_t* row_keys, uint32_t w64, KeyAt key_at) {
    uint64_t at = wtrans_hash_of(key_at, w64) & slot_mask;
    for (uint64_t probe = 0; probe <= slot_mask; ++probe, at = (at + 1) & slot_mask) {
        const uint32_t owner = owners[at];
        if (owner == 0) return kWtransNoRow;
        const uint64_t* theirs = row_keys + (uint64_t)(owner - 1) * w64;
        uint64_t d = 0;
        for (uint32_t w = 0; w < w64; ++w) d |= theirs[w] ^ key_at(w);
        if (d == 0) return owner - 1;
    }
    return kWtransNoRow;
}

BSX_HD uint32_t wtrans_find(const uint32_t* owners, uint64_t slot_mask, const uint64_t* row_keys, uint32_t w64, const uint64_t* key) {
    return wtrans_find_of(owners, slot_mask, row_keys, w64, [key](uint32_t w) { return key[w]; });
}

struct WtransEdge {
    uint32_t dst;       // a row, kWtransOutside or kWtransUnresolved
    uint64_t mu;        // what the flip adds to the edge's sum of recovery times: mu for a real row, else 0
};

// found / lam / mu: the walk's result (lam and mu are read only when found); row: wtrans_find of the walk's key (read
// only when found).
BSX_HD WtransEdge wtrans_classify(bool found, uint64_t lam, uint64_t mu, uint32_t row, uint64_t max_t) {
    const bool resolved = found && (max_t == kWtransInf || (mu <= max_t && lam <= max_t - mu));
    if (!resolved) return WtransEdge{kWtransUnresolved, 0};
    if (row == kWtransNoRow) return WtransEdge{kWtransOutside, 0};
    return WtransEdge{row, mu};
}

}  // namespace bsx
