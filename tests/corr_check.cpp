// Stand-alone check of the rank arithmetic of the node correlations (boolsi_amd/csrc/bsx_ranks.h).  Compiled by the
// host C++ compiler with no HIP include path: the functions driven here are the ones the kernels call.
// Sorted columns with frequencies go through column_ranks (tie-group bounds by the two scans -> rank2 -> d2); every
// position is compared with brute-force pair counting, rank2 = 2 W_less + W_equal + 1 in 128-bit integers, and the
// weighted sum of d2 must be zero.  Columns: all ties, no ties, random tie groups, totals up to 2^62 - 1; and
// corr_total's refusals (a zero frequency, a high word, T >= 2^62).
//   corr_check            -> prints "ok <number of compared ranks>" and exits 0, or "FAIL ..." and exits 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bsx_ranks.h"

namespace {

typedef unsigned __int128 u128;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {                                   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

uint64_t compared = 0;

bool check_column(const char* what, const std::vector<uint64_t>& keys, const std::vector<uint64_t>& freq) {
    const uint64_t n = keys.size();
    std::vector<uint64_t> pairs(2 * n, 0ull);
    for (uint64_t q = 0; q < n; ++q) pairs[2 * q] = freq[q];
    uint64_t total = 0;
    if (bsx::corr_total(pairs.data(), n, &total) != bsx::kCorrTotalOk) { std::printf("FAIL %s: total refused\n", what); return false; }
    std::vector<uint64_t> lo(n), rank2(n);
    std::vector<int64_t> d2(n);
    bsx::column_ranks(keys.data(), freq.data(), n, total, lo.data(), rank2.data(), d2.data());
    __int128 weighted = 0;
    for (uint64_t p = 0; p < n; ++p, ++compared) {
        u128 less = 0, equal = 0;
        for (uint64_t o = 0; o < n; ++o) {
            if (keys[o] < keys[p]) less += freq[o];
            if (keys[o] == keys[p]) equal += freq[o];
        }
        const u128 want = 2 * less + equal + 1;
        if ((u128)rank2[p] != want) { std::printf("FAIL %s: position %llu rank2 %llu\n", what, (unsigned long long)p, (unsigned long long)rank2[p]); return false; }
        const __int128 centred = (__int128)want - (__int128)total - 1;
        if ((__int128)d2[p] != centred) { std::printf("FAIL %s: position %llu d2\n", what, (unsigned long long)p); return false; }
        if (bsx::average_rank_of(rank2[p]) != (double)rank2[p] / 2.0) { std::printf("FAIL %s: average rank\n", what); return false; }
        weighted += (__int128)freq[p] * d2[p];
    }
    if (weighted != 0) { std::printf("FAIL %s: the weighted mean of rank2 is not T + 1\n", what); return false; }
    return true;
}

// n sorted keys in tie groups of about `group` positions (1: no ties, n: all ties)
std::vector<uint64_t> sorted_keys(uint64_t n, uint64_t group) {
    std::vector<uint64_t> keys(n);
    uint64_t value = rnd() & 0xFFFF;
    for (uint64_t p = 0; p < n; ++p) {
        if (p && (group == 1 || (group < n && rnd() % group == 0))) value += 1 + (rnd() & 0xFF);
        keys[p] = value;
    }
    return keys;
}

bool families() {
    const uint64_t sizes[] = {1, 2, 3, 5, 64, 257};
    const uint64_t groups[] = {1, 2, 7, ~0ull};
    for (uint64_t n : sizes)
        for (uint64_t group : groups)
            for (int weights = 0; weights < 3; ++weights) {
                std::vector<uint64_t> keys = sorted_keys(n, group == ~0ull ? n : group), freq(n);
                for (uint64_t q = 0; q < n; ++q) freq[q] = weights == 0 ? 1ull : weights == 1 ? 1 + rnd() % 1000 : 1 + rnd() % (1ull << 40);
                if (!check_column("family", keys, freq)) return false;
            }
    return true;
}

// T = 2^62 - 1 exactly: the top of the range, with ties at both ends of the column
bool top_of_range() {
    const uint64_t n = 9, top = bsx::kCorrTotalLimit - 1;
    std::vector<uint64_t> freq(n, top / n);
    freq[n - 1] += top - (top / n) * n;
    const std::vector<uint64_t> keys = {3, 3, 5, 6, 6, 6, 8, 9, 9};
    if (!check_column("T = 2^62 - 1", keys, freq)) return false;
    if (!check_column("T = 2^62 - 1, all ties", std::vector<uint64_t>(n, 4), freq)) return false;
    if (!check_column("T = 2^62 - 1, one attractor", {1}, {top})) return false;
    return true;
}

bool refusals() {
    uint64_t total = 77;
    const uint64_t limit = bsx::kCorrTotalLimit;
    const uint64_t at_limit[] = {limit - 5, 0, 5, 0};
    const uint64_t below[] = {limit - 5, 0, 4, 0};
    const uint64_t single[] = {limit, 0};
    const uint64_t wraps[] = {~0ull, 0, ~0ull, 0, 2, 0};        // would wrap 64 bits if it were added up blindly
    const uint64_t zero[] = {3, 0, 0, 0};
    const uint64_t high[] = {3, 0, 1, 1};
    bool ok = bsx::corr_total(at_limit, 2, &total) == bsx::kCorrTotalTooLarge && total == 77;
    ok = ok && bsx::corr_total(single, 1, &total) == bsx::kCorrTotalTooLarge && total == 77;
    ok = ok && bsx::corr_total(wraps, 3, &total) == bsx::kCorrTotalTooLarge && total == 77;
    ok = ok && bsx::corr_total(zero, 2, &total) == bsx::kCorrTotalZeroFrequency && total == 77;
    ok = ok && bsx::corr_total(high, 2, &total) == bsx::kCorrTotalHighWord && total == 77;
    ok = ok && bsx::corr_total(below, 2, &total) == bsx::kCorrTotalOk && total == limit - 1;
    ok = ok && bsx::corr_total(below, 0, &total) == bsx::kCorrTotalOk && total == 0;
    if (!ok) std::printf("FAIL corr_total\n");
    return ok;
}

}  // namespace

int main() {
    if (!(families() && top_of_range() && refusals())) return 1;
    std::printf("ok %llu\n", (unsigned long long)compared);
    return 0;
}
