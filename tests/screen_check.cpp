// TEST INFRASTRUCTURE -- drives boolsi_amd/csrc/bsx_screen.h (the HIP-free part of bsx_run_screen_sampled) with the host
// compiler alone: the validation of a mutant list, and the (mutant, group) layout with the pair range of every launch, as
// bsx_screen_api.cpp walks it.  tests/test_screen_host.py compares the output with a Python model.
//
//   screen_check check N_NODES FIXED OFFSETS NODES N_MUTANTS     lists are comma-separated, "-" = empty, "null" = NULL;
//                                                                NODES entries are node:value
//       -> "status S" and "msg TEXT"
//   screen_check layout N_SAMPLES N_MUTANTS L CHUNK
//       -> "layout G G_PER PAIRS CHUNK_PAIRS", then per launch "launch P0 N_PAIRS" and per pair of it
//          "pair P MUTANT GROUP N_VALID RECORD0"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bsx_screen.h"
#include "bsx_table_lower.h"

using namespace bsx;

static std::vector<std::string> split(const char* text) {
    std::vector<std::string> out;
    if (!std::strcmp(text, "-") || !std::strcmp(text, "null")) return out;
    std::string cur;
    for (const char* p = text;; ++p) {
        if (*p == ',' || *p == 0) { out.push_back(cur); cur.clear(); if (*p == 0) break; }
        else cur.push_back(*p);
    }
    return out;
}

static int run_check(char** a) {
    const uint32_t n_nodes = (uint32_t)std::strtoul(a[0], nullptr, 10);
    std::vector<uint32_t> fixmask((n_nodes + 31) / 32 + 1, 0u);
    for (const std::string& s : split(a[1])) {
        const uint32_t v = (uint32_t)std::strtoul(s.c_str(), nullptr, 10);
        fixmask[v >> 5] |= 1u << (v & 31u);
    }
    std::vector<uint32_t> offsets;
    for (const std::string& s : split(a[2])) offsets.push_back((uint32_t)std::strtoul(s.c_str(), nullptr, 10));
    std::vector<bsx_fixed> nodes;
    for (const std::string& s : split(a[3])) {
        const size_t colon = s.find(':');
        bsx_fixed f;
        f.node = (uint32_t)std::strtoul(s.substr(0, colon).c_str(), nullptr, 10);
        f.value = (uint32_t)std::strtoul(s.substr(colon + 1).c_str(), nullptr, 10);
        nodes.push_back(f);
    }
    const uint32_t n_mutants = (uint32_t)std::strtoul(a[4], nullptr, 10);
    // exactly-sized heap copies, so that a read past an end is the sanitizer's
    uint32_t* offs = std::strcmp(a[2], "null") ? new uint32_t[offsets.size()] : nullptr;
    for (size_t i = 0; i < offsets.size(); ++i) offs[i] = offsets[i];
    bsx_fixed* nds = std::strcmp(a[3], "null") ? new bsx_fixed[nodes.size()] : nullptr;
    for (size_t i = 0; i < nodes.size(); ++i) nds[i] = nodes[i];
    const ScreenStatus s = screen_check_mutants(n_nodes, fixmask.data(), offs, nds, n_mutants);
    std::printf("status %d\nmsg %s\n", s.status, s.msg.c_str());
    delete[] offs;
    delete[] nds;
    return 0;
}

static int run_layout(char** a) {
    const uint64_t n_samples = std::strtoull(a[0], nullptr, 10);
    const uint32_t n_mutants = (uint32_t)std::strtoul(a[1], nullptr, 10);
    const uint32_t L = (uint32_t)std::strtoul(a[2], nullptr, 10);
    const uint64_t chunk = std::strtoull(a[3], nullptr, 10);
    const ScreenLayout lay = screen_layout(n_samples, n_mutants, L, chunk);
    std::printf("layout %u %llu %llu %llu\n", lay.G, (unsigned long long)lay.g_per, (unsigned long long)lay.pairs,
                (unsigned long long)lay.chunk_pairs);
    for (const Chunk c : chunks(lay.pairs, lay.chunk_pairs)) {
        std::printf("launch %llu %llu\n", (unsigned long long)c.first, (unsigned long long)c.count);
        for (uint64_t i = 0; i < c.count; ++i) {
            const ScreenPair p = screen_pair_of(c.first + i, lay.g_per, n_samples, lay.G);
            std::printf("pair %llu %u %llu %u %llu\n", (unsigned long long)(c.first + i), p.mutant, (unsigned long long)p.group, p.n_valid,
                        (unsigned long long)(i * lay.G));
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && !std::strcmp(argv[1], "check")) return run_check(argv + 2);
    if (argc == 6 && !std::strcmp(argv[1], "layout")) return run_layout(argv + 2);
    std::fprintf(stderr, "usage: screen_check check N_NODES FIXED OFFSETS NODES N_MUTANTS | layout N_SAMPLES N_MUTANTS L CHUNK\n");
    return 2;
}
