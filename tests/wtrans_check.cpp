// Stand-alone check of what the wide attractor transitions decide per flip (boolsi_amd/csrc/bsx_wtrans.h): the hash
// of a W-word key, the row-key table and the classification rule.  Compiled by the host C++ compiler with no HIP include
// path: these are the functions k_wide_trans and k_wide_trans_build call.
// Rho-shaped functional graphs: a tail of mu states that leads into a cycle of lambda states; two more cycles that
// the walk never reaches.  A state s is the W-word key (s * A, s * B, ..) so that keys differ in every word, or only in
// the last one.  Brute force (every state of the walk stored) gives mu, lambda' and the canonical key, the cycle's
// minimum in the order of the keys (highest word first).  For mu 0..24, lambda 1..24, W = 1, 5, 16, with the reached
// cycle listed and unlisted, under max_t on both sides of mu + lambda', 0, huge and none, and with the walk's own
// `found` both as a capped walk reports it and as a walk reports it that took max_t for unbounded, the edge must be what
// the definition says.  The table is built as k_wide_trans_build builds it (first free slot of the probe sequence).
//   wtrans_check           -> prints "ok <number of classifications>" and exits 0, or "FAIL ..." and exits 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bsx_wtrans.h"

namespace {

uint64_t checks = 0;

struct Graph {
    uint32_t mu, lambda, w64;
    bool last_word_only;
    // states 0 .. mu + lambda - 1: the rho (the cycle is mu .. mu + lambda - 1); 1000 .. 1004 and 2000: other cycles
    uint32_t step(uint32_t x) const {
        if (x >= 2000) return x;
        if (x >= 1000) return x == 1004 ? 1000 : x + 1;
        return x + 1 == mu + lambda ? mu : x + 1;
    }
    // the state's key; the order of keys (highest word first) is NOT the order of the state numbers
    void key_of(uint32_t x, uint64_t* key) const {
        const uint64_t v = ((uint64_t)x + 1) * 0x9E3779B97F4A7C15ull;
        for (uint32_t w = 0; w < w64; ++w) key[w] = last_word_only ? 0 : v * (2 * w + 1);
        key[w64 - 1] = v ^ (v >> 29);
    }
    bool key_less(uint32_t a, uint32_t b) const {
        std::vector<uint64_t> ka(w64), kb(w64);
        key_of(a, ka.data());
        key_of(b, kb.data());
        for (uint32_t w = w64; w-- > 0;)
            if (ka[w] != kb[w]) return ka[w] < kb[w];
        return false;
    }
    // the minimum state, in key order, of the cycle through x (x on a cycle)
    uint32_t canonical(uint32_t x) const {
        uint32_t best = x;
        for (uint32_t y = step(x); y != x; y = step(y))
            if (key_less(y, best)) best = y;
        return best;
    }
};

struct Table {
    std::vector<uint32_t> owners;
    std::vector<uint64_t> row_keys;
    uint64_t mask;
};

// rows: a state on each listed cycle
Table build(const Graph& g, const std::vector<uint32_t>& rows) {
    Table t;
    uint64_t slots = 2;
    while (slots < 2 * rows.size()) slots <<= 1;
    t.mask = slots - 1;
    t.owners.assign(slots, 0);
    t.row_keys.assign(rows.size() * g.w64, 0);
    for (size_t q = 0; q < rows.size(); ++q) {
        uint64_t* mine = &t.row_keys[q * g.w64];
        g.key_of(g.canonical(rows[q]), mine);
        uint64_t at = bsx::wtrans_hash(mine, g.w64) & t.mask;
        while (t.owners[at]) at = (at + 1) & t.mask;
        t.owners[at] = (uint32_t)q + 1;
    }
    return t;
}

bool run(const Graph& g, bool listed, uint64_t max_t) {
    // brute force: the walk from state 0
    std::vector<uint32_t> seen;
    uint32_t x = 0, mu = 0, lam = 0;
    for (;;) {
        size_t at = 0;
        while (at < seen.size() && seen[at] != x) ++at;
        if (at < seen.size()) { mu = (uint32_t)at; lam = (uint32_t)(seen.size() - at); break; }
        seen.push_back(x);
        x = g.step(x);
    }
    bool ok = mu == g.mu && lam == g.lambda;
    std::vector<uint32_t> rows = {1002, 2000};
    if (listed) rows.insert(rows.begin() + 1, g.mu + g.lambda / 2);        // row 1, listed from some state of the cycle
    const Table t = build(g, rows);
    std::vector<uint64_t> key(g.w64);
    g.key_of(g.canonical(g.mu), key.data());
    const uint32_t row = bsx::wtrans_find(t.owners.data(), t.mask, t.row_keys.data(), g.w64, key.data());
    ok = ok && row == (listed ? 1u : bsx::kWtransNoRow);
    // the accessor form the kernel uses must agree with the pointer form
    ok = ok && bsx::wtrans_hash_of([&](uint32_t w) { return key[w]; }, g.w64) == bsx::wtrans_hash(key.data(), g.w64);
    ok = ok && bsx::wtrans_find_of(t.owners.data(), t.mask, t.row_keys.data(), g.w64, [&](uint32_t w) { return key[w]; }) == row;
    // every row finds itself, whatever state of its cycle it was listed from
    for (size_t q = 0; q < rows.size(); ++q) {
        std::vector<uint64_t> k(g.w64);
        g.key_of(g.canonical(g.step(rows[q])), k.data());
        ok = ok && bsx::wtrans_find(t.owners.data(), t.mask, t.row_keys.data(), g.w64, k.data()) == q;
    }
    const bool resolved = max_t == bsx::kWtransInf || (uint64_t)mu + lam <= max_t;
    const uint32_t want_dst = !resolved ? bsx::kWtransUnresolved : listed ? 1u : bsx::kWtransOutside;
    const uint64_t want_mu = resolved && listed ? mu : 0;
    // `found` of a walk under the cap itself, and of a walk that took the cap for unbounded (always found)
    for (int unbounded = 0; unbounded < 2; ++unbounded) {
        const bool found = unbounded ? true : resolved;
        const bsx::WtransEdge e = bsx::wtrans_classify(found, lam, mu, found ? row : 12345u, max_t);
        ++checks;
        if (e.dst != want_dst || e.mu != want_mu) ok = false;
    }
    if (!ok)
        std::printf("FAIL mu %u lambda %u W %u listed %d max_t %llu: row %u, want dst %u mu %llu\n", g.mu, g.lambda, g.w64, (int)listed,
                    (unsigned long long)max_t, row, want_dst, (unsigned long long)want_mu);
    return ok;
}

}  // namespace

int main() {
    bool ok = true;
    for (uint32_t w64 : {1u, 5u, 16u})
        for (int last_only = 0; last_only < 2; ++last_only)
            for (uint32_t mu = 0; mu <= 24 && ok; ++mu)
                for (uint32_t lambda = 1; lambda <= 24 && ok; ++lambda) {
                    const Graph g{mu, lambda, w64, last_only != 0};
                    const uint64_t sum = mu + lambda;
                    for (int listed = 0; listed < 2; ++listed)
                        for (uint64_t max_t : std::vector<uint64_t>{0, 1, sum - 1, sum, sum + 1, 2 * sum, (uint64_t)1 << 40, bsx::kWtransInf - 1, bsx::kWtransInf})
                            ok = run(g, listed != 0, max_t) && ok;
                }
    // keys that differ in one bit of one word must not share a hash systematically: 64 x 16 single-bit keys, at most a few equal low bytes
    {
        uint32_t buckets[256] = {};
        for (uint32_t w = 0; w < 16; ++w)
            for (uint32_t b = 0; b < 64; ++b) {
                uint64_t key[16] = {};
                key[w] = 1ull << b;
                ++buckets[bsx::wtrans_hash(key, 16) & 255u];
            }
        for (uint32_t c : buckets)
            if (c > 16) { std::printf("FAIL hash: %u of 1024 single-bit keys in one of 256 buckets\n", c); ok = false; }
    }
    if (!ok) return 1;
    std::printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
