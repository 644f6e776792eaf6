// The count of the depth-1 level per parent (bsx_device.h: LeafProgram; kernel: the `P.leaf` branch of the lower build,
// bsx_pool_kernel.h): of the 2^kb children of a parent -- the assignments of the kb digits the level adds -- how many have
// the cycle state c as their first update?  The nodes whose rule reads no added digit are compared by the caller; this
// is about the dependent rules.
//
// Brute force over the children evaluates every dependent rule for every child.  But a rule with ONE added digit among
// its inputs constrains that digit alone once the parent's bits are fixed.  A digit is ENTANGLED if some dependent rule
// reads it together with another added digit, else FREE; the program numbers the m entangled digits 0 .. m - 1 and
// lists the rules that read one of them first (the enumerated rules), then the rules of the free digits, grouped by
// digit.  Every rule constrains either entangled digits only or one free digit only, so the count factorises:
//     hits = N_E x product over the free digits q of |{v in {0, 1}: every rule of q gives c's bit at q = v}|
// N_E = the assignments of the entangled digits that satisfy the enumerated rules: the bit-sliced loop, 32 children to a
// word, 512 to a piece, over 2^m children instead of 2^kb.  A free digit's factor is 0 (no child hits), 1 or 2 (a digit
// no rule reads: 2), so the free digits together are a shift, or a zero.  m = kb: no free digit, everything enumerated.
//
// A parent's children may be shared out over `parts` work items, in units of one word of the ENUMERATED children; each
// part stands for its enumerated children times all 2^(kb - m) assignments of the free digits.
//
// Plain C++ with optional __host__ __device__, as bsx_walk.h and bsx_ranks.h: tests/leaf_check.cpp compiles this header
// with the host compiler and no HIP include path and drives the functions the kernel calls.  The rules are read as
// four 32-bit words each (the kernel keeps them in LDS); on the device every such read is made wave-uniform.
#pragma once
#include <stdint.h>

#include "bsx_device.h"

#if !defined(BSX_HD)
#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#endif
#if !defined(BSX_UNROLL)
#if defined(__clang__)
#define BSX_UNROLL _Pragma("unroll")
#else
#define BSX_UNROLL
#endif
#endif

namespace bsx {

BSX_HD uint32_t leaf_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}
BSX_HD uint32_t leaf_bfi(uint32_t sel, uint32_t a, uint32_t b) { return (sel & a) | (~sel & b); }      // (one v_bfi_b32)
BSX_HD uint32_t leaf_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
template <int NW>
BSX_HD uint32_t leaf_bit(const uint32_t (&s)[NW], uint32_t node) {
    uint32_t acc = 0;
BSX_UNROLL
    for (int w = 0; w < NW; ++w) acc |= s[w] & (((node >> 5) == (uint32_t)w) ? 1u << (node & 31u) : 0u);
    return acc ? 1u : 0u;
}

// bit `node` of a state that lies in memory (the cycle state: one word read, the same for every lane)
BSX_HD uint32_t leaf_bit_at(const uint32_t* s, uint32_t node) { return (s[node >> 5] >> (node & 31u)) & 1u; }

// rule i of a list of LeafDep, as words
BSX_HD LeafDep leaf_rule(const uint32_t* rules, uint32_t i) {
    const uint32_t* const dw = rules + 4u * i;
    const uint32_t d0 = leaf_uniform(dw[0]), d1 = leaf_uniform(dw[1]), d2 = leaf_uniform(dw[2]);
    LeafDep dep;
    dep.in[0] = (uint16_t)d0; dep.in[1] = (uint16_t)(d0 >> 16); dep.in[2] = (uint16_t)d1; dep.in[3] = (uint16_t)(d1 >> 16);
    dep.node = (uint16_t)d2; dep.k = (uint16_t)(d2 >> 16);
    dep.tt = leaf_uniform(dw[3]);
    return dep;
}

// 32-children words of the enumerated children
BSX_HD uint32_t leaf_units(uint32_t m) { return m > 5u ? 1u << (m - 5u) : 1u; }

// A batch of 64 parents with all their children is a long piece of serial work for one wave while most waves of a launch
// have nothing to do, so the enumerated children -- in units of one word -- are shared out over a power of two of work
// items per batch, enough for two per wave.
BSX_HD uint32_t leaf_parts(uint32_t m, unsigned long long listed, uint64_t n_waves) {
    const uint32_t units = leaf_units(m);
    const uint64_t batches = (listed + 63ull) / 64ull;
    uint32_t parts = 1;
    while (parts < units && batches * parts < 2ull * n_waves) parts <<= 1;
    return parts;
}

// the children one of `parts` parts stands for (its enumerated children x the free digits' assignments), at most 2^14
BSX_HD uint32_t leaf_children_per_part(uint32_t kb, uint32_t m, uint32_t parts) {
    return (m > 5u ? (leaf_units(m) / parts) * 32u : 1u << m) << (kb - m);
}

// N_E of part `part`: the enumerated children of that part whose enumerated rules all give c's bits.  Sp = the parent's
// state (per lane), C = the cycle state's NW words (uniform).  The children are taken 512 at a time: 16 words of 32; digits 9.. of
// the enumerated index number the pieces.
template <int NW>
BSX_HD uint32_t leaf_enum_hits(const uint32_t (&Sp)[NW], const uint32_t* C, const uint32_t* rules, uint32_t n_enum, uint32_t m,
                               uint32_t part, uint32_t parts) {
    const uint32_t m_in = m < 9u ? m : 9u;
    const uint32_t n_words = m_in > 5u ? 1u << (m_in - 5u) : 1u;                       // <= 16
    const uint32_t word_mask = m_in >= 5u ? 0xFFFFFFFFu : (1u << (1u << m_in)) - 1u;    // children in a word
    const uint32_t units_per_part = leaf_units(m) / parts;
    // this part's children: pieces [piece0, piece0 + n_pieces_here), of each the words [w0, w_end)
    const uint32_t unit0 = part * units_per_part;
    const uint32_t piece0 = unit0 >> 4, w0 = units_per_part >= 16u ? 0u : unit0 & 15u;
    const uint32_t n_pieces_here = units_per_part >= 16u ? units_per_part >> 4 : 1u;
    const uint32_t w_end = units_per_part >= 16u ? n_words : w0 + units_per_part;
    uint32_t n_hit = 0;
    for (uint32_t piece = piece0; piece < piece0 + n_pieces_here; ++piece) {
        uint32_t match[16];
BSX_UNROLL
        for (int w = 0; w < 16; ++w) match[w] = ((uint32_t)w >= w0 && (uint32_t)w < w_end) ? word_mask : 0u;
        for (uint32_t di = 0; di < n_enum; ++di) {
            const LeafDep dep = leaf_rule(rules, di);                   // uniform
            const uint32_t k = dep.k & 0xFFu;
            const uint32_t want = 0u - leaf_bit_at(C, dep.node);       // this cycle state's value of the node (uniform)
            uint32_t selp[kLeafMaxK];                                   // inputs that are parent bits: one broadcast per lane
BSX_UNROLL
            for (int j = 0; j < (int)kLeafMaxK; ++j)
                selp[j] = ((uint32_t)j < k && !(dep.in[j] & 0x8000u)) ? 0u - leaf_bit<NW>(Sp, dep.in[j]) : 0u;
BSX_UNROLL
            for (int w = 0; w < 16; ++w) {
                if ((uint32_t)w >= w0 && (uint32_t)w < w_end) {         // uniform
                    const uint32_t wg = piece * 16u + (uint32_t)w;      // the word's number among all enumerated children's
                    uint32_t sel[kLeafMaxK];
BSX_UNROLL
                    for (int j = 0; j < (int)kLeafMaxK; ++j) {
                        const uint32_t q_digit = dep.in[j] & 0x7FFFu;
                        const uint32_t pat = q_digit == 0u ? 0xAAAAAAAAu : q_digit == 1u ? 0xCCCCCCCCu : q_digit == 2u ? 0xF0F0F0F0u :
                                             q_digit == 3u ? 0xFF00FF00u : q_digit == 4u ? 0xFFFF0000u :
                                             (((wg >> ((q_digit - 5u) & 31u)) & 1u) ? 0xFFFFFFFFu : 0u);     // (a node's number: not used)
                        sel[j] = (dep.in[j] & 0x8000u) ? pat : selp[j];
                    }
                    // mux tree over the table bits (inputs beyond k select the low half: their selector is 0)
                    uint32_t v[1 << (kLeafMaxK - 1)];
BSX_UNROLL
                    for (int i = 0; i < (1 << (kLeafMaxK - 1)); ++i) {
                        const uint32_t lo = 0u - ((dep.tt >> (2 * i)) & 1u), hi = 0u - ((dep.tt >> (2 * i + 1)) & 1u);
                        v[i] = (sel[0] & hi) | (~sel[0] & lo);
                    }
BSX_UNROLL
                    for (int j = 1; j < (int)kLeafMaxK; ++j)
BSX_UNROLL
                        for (int i = 0; i < (1 << (kLeafMaxK - 1 - j)); ++i) v[i] = leaf_bfi(sel[j], v[2 * i + 1], v[2 * i]);
                    match[w] &= ~(v[0] ^ want);
                }
            }
        }
BSX_UNROLL
        for (int w = 0; w < 16; ++w) n_hit += leaf_popc(match[w]);
    }
    return n_hit;
}

constexpr uint32_t kLeafNoChild = 0xFFFFFFFFu;
// The free digits' factor for the parent Sp and the cycle state C as a shift (its log2), or kLeafNoChild: some free
// digit has no allowed value.  A free rule's value with its digit at 0 and at 1 comes from the parent's bits (a table
// lookup per lane); the digit's value v is allowed if every rule of its group gives c's bit of the rule's node at v.
// Starts from "every free digit may take both values" and takes one off per digit that is pinned.  (The values depend on
// the parent alone, but kept across the cycle states as two 64-bit masks per lane they cost the lower builds registers
// they do not have; they are formed again for every cycle state that agrees with the parent on the independent nodes.)
template <int NW>
BSX_HD uint32_t leaf_free_shift(const uint32_t (&Sp)[NW], const uint32_t* C, const uint32_t* rules, uint32_t n_enum, uint32_t n_free, uint32_t kb,
                                uint32_t m) {
    uint32_t shift = kb - m;
    bool none = false, at0 = true, at1 = true;
    for (uint32_t i = 0; i < n_free; ++i) {
        const LeafDep dep = leaf_rule(rules, n_enum + i);   // uniform
        const uint32_t k = dep.k & 0xFFu, q = dep.k >> 8;
        uint32_t idx = 0, digit_slots = 0;
BSX_UNROLL
        for (int j = 0; j < (int)kLeafMaxK; ++j) {
            if ((uint32_t)j < k) {                          // uniform
                if (dep.in[j] & 0x8000u) digit_slots |= 1u << j;
                else idx |= leaf_bit<NW>(Sp, dep.in[j]) << j;
            }
        }
        const uint32_t want = leaf_bit_at(C, dep.node);
        at0 = at0 && ((dep.tt >> idx) & 1u) == want;
        at1 = at1 && ((dep.tt >> (idx | digit_slots)) & 1u) == want;
        const bool last = i + 1u == n_free || (leaf_uniform(rules[4u * (n_enum + i + 1u) + 2u]) >> 24) != q;
        if (last) {                                         // uniform: the digit's group ends here
            none = none || !(at0 || at1);
            shift -= (at0 && at1) ? 0u : 1u;
            at0 = true; at1 = true;
        }
    }
    return none ? kLeafNoChild : shift;
}

// The whole count for one (parent, cycle state, part).
template <int NW>
BSX_HD uint32_t leaf_count(const uint32_t (&Sp)[NW], const uint32_t* C, const uint32_t* rules, uint32_t kb, uint32_t m, uint32_t n_enum,
                           uint32_t n_free, uint32_t part, uint32_t parts) {
    const uint32_t shift = leaf_free_shift<NW>(Sp, C, rules, n_enum, n_free, kb, m);
    if (shift == kLeafNoChild) return 0u;
    return leaf_enum_hits<NW>(Sp, C, rules, n_enum, m, part, parts) << shift;
}

}  // namespace bsx
