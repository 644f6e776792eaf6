// Mutant screens over samples (bsx_run_screen_sampled; include/bsx.h has the normative definition): what needs no device.
// The validation of a mutant list, the (mutant, group) layout of a call and the pair range of a launch.  Plain C++ with
// optional __host__ __device__ (as bsx_sample.h), so that tests/screen_check.cpp drives exactly this code with the host
// compiler and no HIP include path; k_wide_screen and the reduction decode a pair with screen_pair_of below.
//
// Layout: a group is 32 * L samples (one workgroup's matrix).  G_per = ceil(n_samples / 32 L) groups cover the range; the
// work items of a call are the pairs p = m * G_per + g, mutant m over group g, so that no group mixes mutants.  Group g
// holds samples first_sample + 32 L g + k, k < n_valid(g); only the last group of a mutant is ragged.  A launch carries the
// pairs [p0, p0 + n_pairs) and has room for 32 L records per pair, record q of the launch belonging to pair p0 + q / 32 L
// and to trajectory q % 32 L of its group: a record at or behind the group's n_valid does not exist and is never read.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>

#include "bsx.h"

#if !defined(BSX_HD)
#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#endif

namespace bsx {

struct ScreenPair {
    uint32_t mutant;
    uint32_t n_valid;       // samples of the group, 1 .. 32 L
    uint64_t group;         // its first sample is first_sample + 32 L * group
};
// pair p of a call over n_samples samples in groups of G = 32 L, g_per = ceil(n_samples / G) groups per mutant
BSX_HD ScreenPair screen_pair_of(uint64_t p, uint64_t g_per, uint64_t n_samples, uint32_t G) {
    const uint64_t m = p / g_per, g = p - m * g_per;
    const uint64_t left = n_samples - g * G;
    return ScreenPair{(uint32_t)m, (uint32_t)(left < G ? left : G), g};
}

struct ScreenLayout {
    uint32_t G = 0;             // samples per group
    uint64_t g_per = 0;         // groups per mutant
    uint64_t pairs = 0;         // n_mutants * g_per
    uint64_t chunk_pairs = 0;   // pairs per launch: the chunk in trajectories rounded down to whole groups, at least one
};
inline ScreenLayout screen_layout(uint64_t n_samples, uint32_t n_mutants, uint32_t L, uint64_t chunk_trajectories) {
    ScreenLayout S;
    S.G = 32u * L;
    S.g_per = (n_samples + S.G - 1) / S.G;
    S.pairs = S.g_per * n_mutants;
    S.chunk_pairs = chunk_trajectories / S.G ? chunk_trajectories / S.G : 1;
    if (S.chunk_pairs > S.pairs && S.pairs) S.chunk_pairs = S.pairs;
    return S;
}

// BSX_OK, or the status and the text for bsx_last_error (the text names the mutant and the node)
struct ScreenStatus {
    int status = BSX_OK;
    std::string msg;
    explicit operator bool() const { return status != BSX_OK; }
};

// fixmask: bit v of word v >> 5 = the origin fixes node v (WideSpace::fixmask)
inline ScreenStatus screen_check_mutants(uint32_t n_nodes, const uint32_t* fixmask, const uint32_t* mut_offsets, const bsx_fixed* mut_nodes,
                                         uint32_t n_mutants) {
    char buf[160];
    if (n_mutants == 0) return {BSX_ERR_INVALID, "screen: n_mutants is 0"};
    if (n_mutants > BSX_SCREEN_MAX_MUTANTS) return {BSX_ERR_INVALID, "screen: more than BSX_SCREEN_MAX_MUTANTS mutants"};
    if (!mut_offsets) return {BSX_ERR_INVALID, "screen: mut_offsets is null"};
    if (mut_offsets[0] != 0) return {BSX_ERR_INVALID, "screen: mut_offsets does not start at 0"};
    for (uint32_t m = 0; m < n_mutants; ++m) {
        if (mut_offsets[m + 1] < mut_offsets[m]) {
            std::snprintf(buf, sizeof buf, "screen: the offsets do not ascend at mutant %u", m);
            return {BSX_ERR_INVALID, buf};
        }
        if (mut_offsets[m + 1] - mut_offsets[m] > BSX_SCREEN_MAX_NODES) {
            std::snprintf(buf, sizeof buf, "screen: mutant %u lists %u nodes, more than BSX_SCREEN_MAX_NODES", m,
                          mut_offsets[m + 1] - mut_offsets[m]);
            return {BSX_ERR_INVALID, buf};
        }
    }
    if (mut_offsets[n_mutants] && !mut_nodes) return {BSX_ERR_INVALID, "screen: mut_nodes is null"};
    for (uint32_t m = 0; m < n_mutants; ++m) {
        for (uint32_t i = mut_offsets[m]; i < mut_offsets[m + 1]; ++i) {
            const uint32_t v = mut_nodes[i].node;
            const char* what = nullptr;
            if (v >= n_nodes) what = "is not a node of the network";
            else if ((fixmask[v >> 5] >> (v & 31u)) & 1u) what = "is fixed by the origin";
            else if (mut_nodes[i].value > 1) what = "has a value above 1";
            else
                for (uint32_t j = mut_offsets[m]; j < i; ++j)
                    if (mut_nodes[j].node == v) what = "is listed twice";
            if (what) {
                std::snprintf(buf, sizeof buf, "screen: mutant %u: node %u %s", m, v, what);
                return {BSX_ERR_INVALID, buf};
            }
        }
    }
    return {};
}

// n_mutants * n_samples <= 2^40
inline bool screen_range_ok(uint64_t n_samples, uint32_t n_mutants) {
    return n_samples <= (1ull << 40) / n_mutants;
}

}  // namespace bsx
