// TEST INFRASTRUCTURE -- drives boolsi_amd/csrc/bsx_influence.h (the HIP-free part of bsx_run_influence_sampled) with the
// host compiler alone: the checks of the arguments, of the source list and of the sizes in the order of
// bsx_influence_api.cpp, and the (source, group) layout with the item range of every launch, as that file walks it.
// tests/test_influence_host.py compares the output with a Python model.
//
//   influence_check check N_NODES FIXED SOURCES N_SOURCES N_STEPS FIRST N_SAMPLES HAVE_TABLE
//                                  lists are comma-separated, "-" = empty, "null" = NULL; HAVE_TABLE 0 = influence is NULL
//       -> "status S", "msg TEXT" and "cells C"
//   influence_check layout N_SAMPLES N_SOURCES L CHUNK
//       -> "layout G G_PER ITEMS CHUNK_ITEMS", then per launch "launch P0 N_ITEMS" and per item of it
//          "item P SOURCE GROUP FIRST N_VALID"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bsx_influence.h"
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

static InfluenceStatus check_call(uint32_t n_nodes, const uint32_t* fixmask, const uint32_t* sources, uint32_t n_sources, uint32_t n_steps,
                                  uint64_t first, uint64_t n_samples, bool have_table) {
    if (const InfluenceStatus s = influence_check_args(have_table, sources != nullptr, n_sources, n_steps, first, n_samples)) return s;
    if (const InfluenceStatus s = influence_check_sources(n_nodes, fixmask, sources, n_sources)) return s;
    return influence_check_sizes(n_samples, n_sources, n_steps, n_nodes);
}

static int run_check(char** a) {
    const uint32_t n_nodes = (uint32_t)std::strtoul(a[0], nullptr, 10);
    std::vector<uint32_t> fixmask((n_nodes + 31) / 32 + 1, 0u);
    for (const std::string& s : split(a[1])) {
        const uint32_t v = (uint32_t)std::strtoul(s.c_str(), nullptr, 10);
        fixmask[v >> 5] |= 1u << (v & 31u);
    }
    std::vector<uint32_t> listed;
    for (const std::string& s : split(a[2])) listed.push_back((uint32_t)std::strtoul(s.c_str(), nullptr, 10));
    const uint32_t n_sources = (uint32_t)std::strtoul(a[3], nullptr, 10);
    const uint32_t n_steps = (uint32_t)std::strtoul(a[4], nullptr, 10);
    const uint64_t first = std::strtoull(a[5], nullptr, 10), n_samples = std::strtoull(a[6], nullptr, 10);
    // an exactly-sized heap copy, so that a read past its end is the sanitizer's
    uint32_t* src = std::strcmp(a[2], "null") ? new uint32_t[listed.size()] : nullptr;
    for (size_t i = 0; i < listed.size(); ++i) src[i] = listed[i];
    const InfluenceStatus s = check_call(n_nodes, fixmask.data(), src, n_sources, n_steps, first, n_samples, std::strcmp(a[7], "0") != 0);
    std::printf("status %d\nmsg %s\ncells %llu\n", s.status, s.msg.c_str(), (unsigned long long)influence_cells(n_sources, n_steps, n_nodes));
    delete[] src;
    return 0;
}

static int run_layout(char** a) {
    const uint64_t n_samples = std::strtoull(a[0], nullptr, 10);
    const uint32_t n_sources = (uint32_t)std::strtoul(a[1], nullptr, 10);
    const uint32_t L = (uint32_t)std::strtoul(a[2], nullptr, 10);
    const uint64_t chunk = std::strtoull(a[3], nullptr, 10);
    const InfluenceLayout lay = influence_layout(n_samples, n_sources, L, chunk);
    std::printf("layout %u %llu %llu %llu\n", lay.G, (unsigned long long)lay.g_per, (unsigned long long)lay.items,
                (unsigned long long)lay.chunk_items);
    for (const Chunk c : chunks(lay.items, lay.chunk_items)) {
        std::printf("launch %llu %llu\n", (unsigned long long)c.first, (unsigned long long)c.count);
        for (uint64_t i = 0; i < c.count; ++i) {
            const InfluenceItem it = influence_item_of(c.first + i, lay.g_per, n_samples, lay.G);
            std::printf("item %llu %u %llu %llu %u\n", (unsigned long long)(c.first + i), it.source, (unsigned long long)it.group,
                        (unsigned long long)it.first, it.n_valid);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 10 && !std::strcmp(argv[1], "check")) return run_check(argv + 2);
    if (argc == 6 && !std::strcmp(argv[1], "layout")) return run_layout(argv + 2);
    std::fprintf(stderr, "usage: influence_check check N_NODES FIXED SOURCES N_SOURCES N_STEPS FIRST N_SAMPLES HAVE_TABLE | "
                         "layout N_SAMPLES N_SOURCES L CHUNK\n");
    return 2;
}
