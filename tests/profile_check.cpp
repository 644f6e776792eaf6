// Stand-alone check of the vertical counters (boolsi_amd/csrc/bsx_planes.h) that the attractor-profile kernels keep
// their on-counts in.  Compiled by the host C++ compiler with no HIP include path: the functions driven here are the
// ones the kernels call.  Random words are added one by one; after every add the planes plus what has been flushed
// so far must equal a per-bit integer count.  Run lengths sit on both sides of a flush and span several.
//   profile_check            -> prints "ok <number of compared counts>" and exits 0, or "FAIL ..." and exits 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bsx_planes.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {                                   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

uint64_t compared = 0;

// density: 0 all bits set, 1 random, 2 sparse (and of three draws)
template <int NW, int P>
bool run(uint32_t n_bits, uint32_t length, int density) {
    typedef bsx::Planes<NW, P> Pl;
    Pl pl;
    bsx::planes_clear(pl);
    std::vector<uint32_t> row(32 * NW, 0u), want(32 * NW, 0u);
    uint32_t pending = 0, flushes = 0;
    for (uint32_t t = 0; t < length; ++t) {
        uint32_t s[NW];
        for (int w = 0; w < NW; ++w) {
            s[w] = density == 0 ? 0xFFFFFFFFu : density == 1 ? rnd() : (rnd() & rnd() & rnd());
            for (uint32_t b = 0; b < 32; ++b)
                if (32u * w + b >= n_bits) s[w] &= ~(1u << b);                  // (a state has no bits at or above n)
            for (uint32_t b = 0; b < 32; ++b) want[32 * w + b] += (s[w] >> b) & 1u;
        }
        bsx::planes_add(pl, s);
        ++pending;
        for (uint32_t i = 0; i < 32u * NW; ++i, ++compared) {                   // before the flush: planes + row
            const uint32_t got = row[i] + bsx::planes_count(pl, i);
            if (got != want[i]) { std::printf("FAIL NW %d P %d length %u t %u bit %u: %u != %u\n", NW, P, length, t, i, got, want[i]); return false; }
        }
        if (pending == Pl::kFlushEvery) { bsx::planes_flush(pl, row.data(), n_bits); pending = 0; ++flushes; }
    }
    if (pending) bsx::planes_flush(pl, row.data(), n_bits);
    for (uint32_t i = 0; i < 32u * NW; ++i, ++compared) {
        if (row[i] != want[i]) { std::printf("FAIL NW %d P %d length %u end bit %u: %u != %u\n", NW, P, length, i, row[i], want[i]); return false; }
        if (bsx::planes_count(pl, i) != 0) { std::printf("FAIL NW %d P %d: planes not cleared by the flush\n", NW, P); return false; }
    }
    if (flushes != length / Pl::kFlushEvery) { std::printf("FAIL NW %d P %d length %u: %u flushes\n", NW, P, length, flushes); return false; }
    return true;
}

template <int NW, int P>
bool family() {
    const uint32_t full = (1u << P) - 1u;
    const uint32_t lengths[] = {1, 2, full - 1, full, full + 1, 3 * full + 1};
    const uint32_t widths[] = {32u * NW, 32u * NW - 7u, 32u * (NW - 1) + 1u};   // full, ragged last word, one bit in it
    for (uint32_t length : lengths)
        for (uint32_t n_bits : widths)
            for (int density = 0; density < 3; ++density)
                if (!run<NW, P>(n_bits, length, density)) return false;
    return true;
}

}  // namespace

int main() {
    constexpr int P = bsx::kProfilePlanes, PW = bsx::kWideProfilePlanes;
    bool ok = family<1, P>() && family<2, P>() && family<4, P>() && family<8, P>();
    ok = ok && family<1, PW>() && family<2, PW>() && family<4, PW>() && family<8, PW>();     // the wide kernel's plane count
    ok = ok && family<1, 2>() && family<2, 3>();                                             // small P: many flushes
    if (!ok) return 1;
    std::printf("ok %llu\n", (unsigned long long)compared);
    return 0;
}
