// Lowering of the wide-state family without HIP: validation of the network arrays (shared with the per-lane family's
// bsx_set_network), a network and a problem space lowered to the arrays of bsx_wide.h, the target substate, the
// flat-index split and the grid rule.  Plain C++ over include/bsx.h and bsx_wide.h: tests/wide_lower_check.cpp builds
// this unit with the host compiler alone.  The wide host files (bsx_wide_host.h) upload what it returns.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bsx.h"
#include "bsx_lower_status.h"
#include "bsx_wide.h"

namespace bsx {

// bsx_set_network's arrays: monotone offsets, at most BSX_MAX_PREDECESSORS ascending predecessors, ceil(2^k / 64) table words
LowerStatus check_network_arrays(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets);
inline LowerStatus wide_check_size(uint32_t n_nodes) {
    return n_nodes > BSX_MAX_NODES_WIDE ? LowerStatus{BSX_ERR_UNSUPPORTED, "more than BSX_MAX_NODES_WIDE nodes"} : LowerStatus{};
}

struct WideNet {
    uint32_t n = 0, rows = 0, w64 = 0, K = 1;       // K: the most predecessors among the nodes with at most 6
    std::vector<uint32_t> pred_offsets, pred_idx, tt_offsets;
    std::vector<uint64_t> tt;
    std::vector<uint32_t> wdesc, wpreds, wtt;       // nodes with more than 6 predecessors, in node order (WideParams)
};
void wide_lower_network(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets,
                        const uint64_t* tt_words, WideNet& net);        // (the arrays have passed check_network_arrays)

struct WideSpace {
    uint32_t origin[kWideMaxW32] = {};      // origin state, 'any' nodes cleared
    uint32_t fixmask[kWideMaxW32] = {};     // nodes the origin fixes (constant rules in the descriptors)
    std::vector<uint32_t> any, fv, pv, sched, desc;     // as WideParams lays them out; desc: [rows][kWideDescWords]
    uint32_t n_any = 0, n_fv = 0, n_pv = 0, n_sched = 0, n_fslots = 0, tp_origin = 0, tp_max = 0;
    uint64_t variant_count = 1;             // product of the variation radices, UINT64_MAX when it saturates
    bool variant_count_saturated = false;
    uint32_t L = 0;                         // columns per group: the largest power of two <= 64 that fits the LDS
    size_t shmem = 0;
};
LowerStatus wide_lower_space(const WideNet& net, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                             const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                             const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var, WideSpace& sp);

// mask_words / code_words of a target call -> WideParams::tmask / tcode (kWideMaxW32 words each)
void wide_target_words(uint32_t n_nodes, const uint64_t* mask_words, const uint64_t* code_words, uint32_t* tmask, uint32_t* tcode);
// flat index -> bsx_index: the low n_any bits are the initial-state digits, the rest is the variant
LowerStatus wide_split_flat(bsx_u128 flat, uint32_t n_any, bsx_index& first);
// Workgroups of a launch over `count` trajectories in groups of 32 * L: as many as fit the device at once, at least one.
uint64_t wide_grid_blocks(uint64_t count, uint32_t L, size_t shmem, uint32_t compute_units);

}  // namespace bsx
