// TEST INFRASTRUCTURE -- the flip selection of boolsi_amd/csrc/bsx_sample.h (damage_draw, damage_choose) with the host
// compiler alone (no HIP include path), so that the functions k_wide_damage calls are the ones printed here;
// tests/test_damage_host.py compares every position with tests/damage_ref.py.
//
//   damage_check SEED FIRST COUNT N_ANY N_FREE H L  ->  "F sample p0 p1 ... p(H-1)": the positions of samples
//        [FIRST, FIRST + COUNT) in the order they are chosen, by the kernel's own path: groups of 32 L samples, one
//        SampleColumn per column, the column's key and lane per sample, the chosen-position masks of a group interleaved
//        (word w of sample k at mask[w * G + k]) in a buffer of exactly the words the kernel uses.
// Numbers are decimal on the command line and in the output.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bsx_sample.h"

using namespace bsx;

static uint64_t num(const char* s) { return std::strtoull(s, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: damage_check SEED FIRST COUNT N_ANY N_FREE H L\n");
        return 2;
    }
    const uint64_t k0 = sample_k0(num(argv[1])), first = num(argv[2]), count = num(argv[3]);
    const uint32_t n_any = (uint32_t)num(argv[4]), n_free = (uint32_t)num(argv[5]), h = (uint32_t)num(argv[6]);
    const uint32_t L = (uint32_t)num(argv[7]), G = 32 * L;
    if (h == 0 || h > n_free) return 2;
    const uint32_t mask_words = (n_free + 31u) >> 5;
    for (uint64_t group = 0; group * G < count; ++group) {
        const uint64_t base = group * G;
        const uint32_t n_valid = (uint32_t)(count - base < G ? count - base : G);
        std::vector<uint32_t> mask((size_t)mask_words * G, 0u);     // (heap: the sanitized build checks its bounds)
        for (uint32_t k = 0; k < n_valid; ++k) {
            const uint32_t cw = k >> 5;
            const SampleColumn sc = sample_column(k0, first + base + 32ull * cw);
            const uint64_t kb = sample_column_key(sc, k & 31u);
            const uint32_t lane = sample_column_lane(sc, k & 31u);
            std::printf("F %" PRIu64, first + base + k);
            for (uint32_t i = 0; i < h; ++i)
                std::printf(" %u", damage_choose(damage_draw(kb, n_any, lane, i), n_free, i, mask.data() + k, G));
            std::printf("\n");
        }
    }
    return 0;
}
