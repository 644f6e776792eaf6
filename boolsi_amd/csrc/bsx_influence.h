// Node influence over samples (bsx_run_influence_sampled; include/bsx.h has the normative definition): what needs no device.
// The (source, group) layout of a call with the item range of a launch, the validation of the arguments and of the source
// list, and the cell-count arithmetic.  Plain C++ with optional __host__ __device__ (as bsx_sample.h and bsx_screen.h), so
// that tests/influence_check.cpp drives exactly this code with the host compiler and no HIP include path; k_wide_influence
// decodes an item with influence_item_of below.
//
// Layout: a group is 32 * L samples (one workgroup's matrix).  G_per = ceil(n_samples / 32 L) groups cover the range; the
// work items of a call are p = s * G_per + g, source s over group g, so that no group mixes sources.  Group g holds samples
// first_sample + 32 L g + k, k < n_valid(g); only the last group of a source is ragged.  A launch carries the items
// [p0, p0 + n_items), and every launch adds to the one table of the call.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

#include "bsx.h"

#if !defined(BSX_HD)
#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#endif

namespace bsx {

struct InfluenceItem {
    uint32_t source;        // index into the call's source list
    uint32_t n_valid;       // samples of the group, 1 .. 32 L
    uint64_t group;
    uint64_t first;         // the group's first sample, counted from first_sample: 32 L * group
};
// item p of a call over n_samples samples in groups of G = 32 L, g_per = ceil(n_samples / G) groups per source
BSX_HD InfluenceItem influence_item_of(uint64_t p, uint64_t g_per, uint64_t n_samples, uint32_t G) {
    const uint64_t s = p / g_per, g = p - s * g_per;
    const uint64_t left = n_samples - g * G;
    return InfluenceItem{(uint32_t)s, (uint32_t)(left < G ? left : G), g, g * G};
}

struct InfluenceLayout {
    uint32_t G = 0;             // samples per group
    uint64_t g_per = 0;         // groups per source
    uint64_t items = 0;         // n_sources * g_per
    uint64_t chunk_items = 0;   // items per launch: the chunk in trajectories rounded down to whole groups, at least one
};
inline InfluenceLayout influence_layout(uint64_t n_samples, uint32_t n_sources, uint32_t L, uint64_t chunk_trajectories) {
    InfluenceLayout S;
    S.G = 32u * L;
    S.g_per = (n_samples + S.G - 1) / S.G;
    S.items = S.g_per * n_sources;
    S.chunk_items = chunk_trajectories / S.G ? chunk_trajectories / S.G : 1;
    if (S.chunk_items > S.items && S.items) S.chunk_items = S.items;
    return S;
}

// BSX_OK, or the status and the text for bsx_last_error
struct InfluenceStatus {
    int status = BSX_OK;
    std::string msg;
    explicit operator bool() const { return status != BSX_OK; }
};

// The checks that need neither the network nor the space: BSX_ERR_INVALID
inline InfluenceStatus influence_check_args(bool have_influence, bool have_sources, uint32_t n_sources, uint32_t n_steps,
                                            uint64_t first_sample, uint64_t n_samples) {
    if (!have_influence) return {BSX_ERR_INVALID, "influence: influence is null"};
    if (!have_sources) return {BSX_ERR_INVALID, "influence: sources is null"};
    if (n_sources == 0) return {BSX_ERR_INVALID, "influence: n_sources is 0"};
    if (n_steps == 0) return {BSX_ERR_INVALID, "influence: n_steps is 0"};
    if (first_sample + n_samples < first_sample) return {BSX_ERR_INVALID, "influence: first_sample + n_samples wraps"};
    return {};
}

// The source list: distinct nodes of the network that the origin does not fix; the text names the entry and the node.
// fixmask: bit v of word v >> 5 = the origin fixes node v (WideSpace::fixmask).  Reads at most n_nodes + 1 entries: a list
// that long repeats a node or leaves the network.
inline InfluenceStatus influence_check_sources(uint32_t n_nodes, const uint32_t* fixmask, const uint32_t* sources, uint32_t n_sources) {
    char buf[160];
    std::vector<uint32_t> seen((n_nodes + 31u) / 32u, 0u);
    for (uint32_t s = 0; s < n_sources; ++s) {
        const uint32_t v = sources[s];
        const char* what = nullptr;
        if (v >= n_nodes) what = "is not a node of the network";
        else if ((fixmask[v >> 5] >> (v & 31u)) & 1u) what = "is fixed by the origin";
        else if ((seen[v >> 5] >> (v & 31u)) & 1u) what = "is listed twice";
        if (what) {
            std::snprintf(buf, sizeof buf, "influence: sources[%u]: node %u %s", s, v, what);
            return {BSX_ERR_INVALID, buf};
        }
        seen[v >> 5] |= 1u << (v & 31u);
    }
    return {};
}

// cells of the table: n_sources * n_steps * n_nodes, saturated at 2^64 - 1
inline uint64_t influence_cells(uint32_t n_sources, uint32_t n_steps, uint32_t n_nodes) {
    const uint64_t rows = (uint64_t)n_sources * n_steps;        // < 2^64
    if (n_nodes && rows > ~0ull / n_nodes) return ~0ull;
    return rows * n_nodes;
}

// The sizes: BSX_ERR_RANGE_TOO_LARGE for n_samples > 2^31 (a cell is 32 bits wide) or n_sources * n_samples > 2^40, then
// BSX_ERR_UNSUPPORTED for more than BSX_INFLUENCE_MAX_CELLS cells.  n_sources >= 1.
inline InfluenceStatus influence_check_sizes(uint64_t n_samples, uint32_t n_sources, uint32_t n_steps, uint32_t n_nodes) {
    if (n_samples > (1ull << 31)) return {BSX_ERR_RANGE_TOO_LARGE, "influence: more than 2^31 samples per call"};
    if (n_samples > (1ull << 40) / n_sources) return {BSX_ERR_RANGE_TOO_LARGE, "influence: n_sources * n_samples exceeds 2^40"};
    if (influence_cells(n_sources, n_steps, n_nodes) > BSX_INFLUENCE_MAX_CELLS)
        return {BSX_ERR_UNSUPPORTED, "influence: n_sources * n_steps * n_nodes is more than BSX_INFLUENCE_MAX_CELLS (2^26) cells"};
    return {};
}

}  // namespace bsx
