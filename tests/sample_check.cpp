// TEST INFRASTRUCTURE -- boolsi_amd/csrc/bsx_sample.h with the host compiler alone (no HIP include path), so that the
// functions the kernels call are the ones printed here; tests/test_sample_host.py compares every word with
// tests/sample_ref.py.
//
//   sample_check words   SEED FIRST_BLOCK N_BLOCKS N_ANY        ->  "A b a word" for every (block, 'any' ordinal)
//   sample_check columns SEED FIRST COUNT N_ANY V L             ->  what a k_wide<K, KW, true> launch over samples
//        [FIRST, FIRST + COUNT) in groups of 32 L derives: "C group column a word" (the word stored into row
//        any_nodes[a]) and "V k variant" (the variant number of the launch's k-th sample), by the kernel's own path:
//        one SampleColumn per column, the column's key and lane per trajectory.
// Numbers are decimal on the command line and hexadecimal in the output.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bsx_sample.h"

using namespace bsx;

static uint64_t num(const char* s) { return std::strtoull(s, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "words")) {
        const uint64_t k0 = sample_k0(num(argv[2])), b0 = num(argv[3]), nb = num(argv[4]);
        const uint32_t n_any = (uint32_t)num(argv[5]);
        for (uint64_t b = b0; b < b0 + nb; ++b) {
            const uint64_t kb = sample_block_key(k0, b);
            for (uint32_t a = 0; a < n_any; ++a) std::printf("A %" PRIx64 " %x %" PRIx64 "\n", b, a, sample_any_word(kb, a));
        }
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "columns")) {
        const uint64_t k0 = sample_k0(num(argv[2])), first = num(argv[3]), count = num(argv[4]);
        const uint32_t n_any = (uint32_t)num(argv[5]);
        const uint64_t V = num(argv[6]);
        const uint32_t L = (uint32_t)num(argv[7]), G = 32 * L;
        for (uint64_t group = 0; group * G < count; ++group) {
            const uint64_t base = group * G;
            const uint32_t n_valid = (uint32_t)(count - base < G ? count - base : G);
            for (uint32_t c = 0; c < L; ++c) {
                const SampleColumn sc = sample_column(k0, first + base + 32ull * c);
                const uint32_t n_bits = n_valid > 32 * c ? (n_valid - 32 * c < 32u ? n_valid - 32 * c : 32u) : 0u;
                for (uint32_t a = 0; a < n_any; ++a)
                    std::printf("C %" PRIx64 " %x %x %x\n", group, c, a, sample_column_word(sc, a, n_bits));
                for (uint32_t i = 0; i < n_bits; ++i) {
                    const uint64_t u = sample_u(sample_column_key(sc, i), n_any, sample_column_lane(sc, i));
                    std::printf("V %" PRIx64 " %" PRIx64 "\n", (uint64_t)(base + 32ull * c + i), sample_variant(u, V));
                }
            }
        }
        return 0;
    }
    if (argc >= 6 && !std::strcmp(argv[1], "problems")) {     // SEED N_ANY V J...: k_sample_problems' path, one sample on its own
        const uint64_t k0 = sample_k0(num(argv[2])), V = num(argv[4]);
        const uint32_t n_any = (uint32_t)num(argv[3]);
        for (int q = 5; q < argc; ++q) {
            const uint64_t j = num(argv[q]), kb = sample_block_key(k0, j >> 6);
            std::printf("P %" PRIx64 " %" PRIx64 " ", j, sample_variant_of(kb, n_any, j, V));
            for (uint32_t a = 0; a < n_any; ++a) std::printf("%u", sample_any_bit(kb, a, j));
            std::printf("\n");
        }
        return 0;
    }
    std::fprintf(stderr, "usage: sample_check words SEED FIRST_BLOCK N_BLOCKS N_ANY | columns SEED FIRST COUNT N_ANY V L | problems SEED N_ANY V J...\n");
    return 2;
}
