// The exact host arithmetic behind attract's results: wide integers for the counts and sums of sweeps beyond 2^64
// problems, the merge of device records by attractor key, and the unit accounting of cube passes (counts in units of
// 2^unit_shift problems plus signed absolute corrections).  No HIP and no handle here: tests/plan_check.cpp checks
// these against plain big integers on any CPU.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <unordered_map>

#include "bsx.h"
#include "bsx_device.h"

namespace bsx {

typedef unsigned __int128 u128;

// ---- wide unsigned integers: counts and sums of sweeps over more than 2^64 problems ------------------------------
struct U256 {
    uint64_t w[4] = {0, 0, 0, 0};
    void add_at(uint64_t v, int word) {                     // += v << (64 * word)
        for (int i = word; i < 4 && v; ++i) { const uint64_t s = w[i] + v; v = s < v ? 1 : 0; w[i] = s; }
    }
    void add(const U256& o) {
        uint64_t carry = 0;
        for (int i = 0; i < 4; ++i) {
            const u128 s = (u128)w[i] + o.w[i] + carry;
            w[i] = (uint64_t)s; carry = (uint64_t)(s >> 64);
        }
    }
    void add128(u128 v) { U256 t; t.w[0] = (uint64_t)v; t.w[1] = (uint64_t)(v >> 64); add(t); }
    // += (hi:lo) << shift, shift < 128
    void add_shifted(uint64_t lo, uint64_t hi, uint32_t shift) {
        U256 t;
        t.w[0] = lo; t.w[1] = hi;
        const uint32_t ws = shift >> 6, bs = shift & 63;
        U256 r;
        for (int i = 3; i >= 0; --i) {
            const int src = i - (int)ws;
            uint64_t v = 0;
            if (src >= 0) v = t.w[src] << bs;
            if (bs && src - 1 >= 0) v |= t.w[src - 1] >> (64 - bs);
            r.w[i] = v;
        }
        add(r);
    }
    // += sign-extended v (two's complement): the result is known to be non-negative
    void add_signed(int64_t v) {
        U256 t;
        t.w[0] = (uint64_t)v;
        t.w[1] = t.w[2] = t.w[3] = v < 0 ? ~0ull : 0ull;
        add(t);
    }
    // += a * b
    void add_mul(u128 a, uint64_t b) {
        const u128 p0 = (u128)(uint64_t)a * b, p1 = (u128)(uint64_t)(a >> 64) * b;
        U256 t;
        t.w[0] = (uint64_t)p0;
        const u128 mid = (p0 >> 64) + (uint64_t)p1;
        t.w[1] = (uint64_t)mid;
        t.w[2] = (uint64_t)((mid >> 64) + (uint64_t)(p1 >> 64));
        add(t);
    }
    bool fits(int words) const { for (int i = words; i < 4; ++i) if (w[i]) return false; return true; }
};

// One aggregated attractor inside the library (every sum wide; narrowed to the caller's record at the boundary).
struct WideRec {
    uint64_t key[BSX_MAX_WORDS] = {0, 0, 0, 0};
    uint64_t length = 0;
    u128 count = 0;
    U256 sum_l, sum_l2;
};

// attractor key as the table key of the host-side merge (zero padded to the longest state)
using Key8 = std::array<uint32_t, kMaxW32>;
struct Key8Hash {
    size_t operator()(const Key8& k) const {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (uint32_t w : k) h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
        return (size_t)(h ^ (h >> 29));
    }
};
inline Key8 key8(const uint32_t* words) { Key8 k; std::copy(words, words + kMaxW32, k.begin()); return k; }

using MergedTable = std::unordered_map<Key8, WideRec, Key8Hash>;

inline WideRec& slot_for(MergedTable& merged, const uint32_t* key32, uint32_t nw, uint64_t length) {
    const Key8 key = key8(key32);
    auto it = merged.find(key);
    if (it == merged.end()) {
        WideRec a;
        for (uint32_t w = 0; w < nw; ++w) a.key[w >> 1] |= (uint64_t)key32[w] << (32 * (w & 1));
        a.length = length;
        it = merged.emplace(key, a).first;
    }
    return it->second;
}

// merge by key (attract.py:405-455 write_aggregated_attractors_to_db, exact integers)
inline void merge_records(MergedTable& merged, const LogRec* recs, size_t n, uint32_t nw) {
    for (size_t i = 0; i < n; ++i) {
        const LogRec& r = recs[i];
        WideRec& a = slot_for(merged, r.key, nw, r.length);
        a.count += r.count;
        a.sum_l.add_at(r.sum_l, 0);
        a.sum_l2.add_shifted(r.sum_l2_lo, r.sum_l2_hi, 0);
    }
}

inline void fold_table(MergedTable& into, const MergedTable& from) {
    for (const auto& kv : from) {
        auto it = into.find(kv.first);
        if (it == into.end()) { into.emplace(kv.first, kv.second); continue; }
        WideRec& a = it->second;
        a.count += kv.second.count;
        a.sum_l.add(kv.second.sum_l);
        a.sum_l2.add(kv.second.sum_l2);
    }
}

// The sums a cube pass left in its Counters block (units of 2^shift problems + the absolute corrections of the
// members that are cycle states themselves, bsx_device.h) -> merged, exact.
inline void merge_cube_counters(MergedTable& merged, const Counters& c, uint32_t shift, uint32_t nw) {
    for (uint32_t a = 0; a < 64; ++a) {
        if (!c.acc_cnt[a] && !c.fix_cnt[a]) continue;
        WideRec& r = slot_for(merged, c.acc_key[a], nw, c.acc_len[a]);
        r.count += ((u128)c.acc_cnt[a] << shift) + (u128)(__int128)(int64_t)c.fix_cnt[a];
        r.sum_l.add_shifted(c.acc_sl[a], 0, shift);
        r.sum_l.add_signed((int64_t)c.fix_sl[a]);
        r.sum_l2.add_shifted(c.acc_sl2_lo[a], c.acc_sl2_hi[a], shift);
        r.sum_l2.add_signed((int64_t)c.fix_sl2[a]);
    }
}

// ... and its problems without attractor / reference steps -> pass_none / pass_ref (a member that failed only the time
// cap counts max_t reference steps: fix_capfail of them).
inline void fold_cube_level(const Counters& c, uint32_t shift, uint64_t max_t, u128& pass_none, u128& pass_ref) {
    pass_none += ((u128)c.n_none << shift) + (u128)(__int128)(int64_t)c.fix_none;
    pass_ref += ((u128)c.steps_ref << shift) + (u128)(__int128)(int64_t)c.fix_ref +
                (max_t == BSX_T_INF ? (u128)0 : (u128)((__int128)(int64_t)c.fix_capfail * (__int128)max_t));
}

// One unresolved class of a cube level, after the detector has run from its listed state.  rec = the level's record
// (state, class time, member count in units of 2^shift problems), pr = the detector's result from that state; tp / cap_rel:
// the warm-up and the time cap counted from s(T_p) (CascadeShape).  False: the class sat on a cycle, so its members' mu
// are unknown and nothing was booked (the pass is repeated with the richer cache).
inline bool book_unresolved_class(MergedTable& pass_table, u128& pass_none, u128& pass_ref, const uint32_t* rec, const ProblemRec32& pr,
                                  uint32_t nw, uint32_t shift, uint64_t tp, uint64_t cap_rel, uint64_t max_t, uint64_t max_len) {
    const uint64_t t_class = rec[nw];
    const u128 m = (u128)(((uint64_t)rec[nw + 2] << 32) | rec[nw + 1]) << shift;
    if (!pr.found) { pass_none += m; pass_ref += m * max_t; return true; }          // (finite cap, or the step limit was hit)
    if (pr.trajectory_l == 0) return false;
    const uint64_t mu = t_class + pr.trajectory_l, lam = pr.length, traj = tp + mu;
    const bool found = cap_rel == BSX_T_INF || mu + lam <= cap_rel;
    pass_ref += found ? m * (traj + lam) : m * max_t;
    if (!found || lam > max_len) { pass_none += m; return true; }
    WideRec& e = slot_for(pass_table, pr.key, nw, lam);
    e.count += m;
    e.sum_l.add_mul(m, traj);
    e.sum_l2.add_mul(m, traj * traj);               // traj < 2^31 here (32-bit device counters)
    return true;
}

}  // namespace bsx
