// Lowering of the per-lane family (n <= 256) without HIP: a network and a problem space lowered to the tables of
// bsx_device.h (DevNet, DevSpace), the LDS budget that picks the LUT mode, the problem-index arithmetic, the counting
// plan of bsx_run_target_summary and the shapes of the simulate launches.  Plain C++ over include/bsx.h, bsx_device.h,
// bsx_model.h, bsx_merge.h and bsx_cube_plan.h: tests/lane_lower_check.cpp builds this unit with the host compiler
// alone.  bsx_api.cpp, bsx_target_api.cpp and bsx_simulate_api.cpp upload and launch what it returns.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bsx.h"
#include "bsx_cube_plan.h"
#include "bsx_device.h"
#include "bsx_lower_status.h"
#include "bsx_merge.h"
#include "bsx_model.h"

namespace bsx {

// ---- network
struct LaneNet {
    uint32_t nw = 0, k_mux = 1, n_chunks = 0, n_wide = 0;
    int lut_mode = 0;                   // kLutGlobal / kLutLdsByte / kLutLdsNibble (bsx_kernels_common.h)
    uint32_t cache_lds_slots = 1;       // slots of the LDS cycle-cache mirror (a power of two)
    size_t cache_stride = 0, cache_bytes = 0;
    size_t shmem = 0, shmem_attract = 0;        // masks (+ LUT in LDS); + the cache mirror and the lean kernel's tables
    std::vector<uint32_t> masks, lut;           // DevNet::masks, DevNet::lut (byte, nibble or 6-word planar layout)
    std::vector<uint32_t> wdesc, wpreds, wtt;   // the nodes with more than kMaxMuxK predecessors
};
// The arrays have passed check_network_arrays.  cache_lds_kb: 0 = kCycleCacheLdsBytes; want_lut_mode: -1 = by the
// 144 KiB rule, 0 or 2 = that mode if it is available.  Fills the network fields of `model` as well.
void lane_lower_network(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets,
                        const uint64_t* tt_words, uint64_t cache_lds_kb, int want_lut_mode, LaneNet& net, HostModel& model);

// ---- problem space
struct LaneSpace {
    DevSpace sp{};                      // everything but the device pointers and the first index
    std::vector<uint32_t> any, fv, pv, set, clr;
    std::vector<uint32_t> sched;        // HostModel::sched: (t, node, value) stably sorted by t
    uint64_t variant_count = 1;         // product of the variation radices, UINT64_MAX when it saturates
    bool variant_count_saturated = false;
    uint32_t tp_max = 0;                // last perturbation time over origin schedule and variations
};
LowerStatus lane_lower_space(uint32_t n, uint32_t nw, uint32_t w64, const uint64_t* origin_state_words, const uint32_t* any_nodes,
                             uint32_t n_any, const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var,
                             uint32_t n_fixed_var, const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var,
                             uint32_t n_pert_var, LaneSpace& out);

// ---- problem indices
// [first, first + count) must lie inside the problem space (2^n_any initial states x variants): the fast
// enumeration paths add the offset to the digits without looking, so an over-long range would otherwise
// spill into nodes that are not 'any' and return plausible but wrong counts.
LowerStatus range_check(const bsx_index* first, u128 count, uint32_t n_any, uint64_t variant_count, bool saturated);
// first + delta as a problem index: the digits at or above n_any carry into the variant number (batching.py:212-255)
bsx_index index_plus(const bsx_index& first, u128 delta, uint32_t n_any);

// ---- target
// LDS of a k_target launch that counts into `hist_bins` bins (0: no histogram)
inline size_t target_shmem(size_t net_shmem, uint32_t hist_bins) { return net_shmem + (hist_bins ? 16 + (size_t)hist_bins * 8 : 0); }
// mask_words / code_words of a target call -> TargetParams::tmask / tcode (kMaxW32 words each; those above w64 stay as they are)
void target_words(uint32_t w64, const uint64_t* mask_words, const uint64_t* code_words, uint32_t* tmask, uint32_t* tcode);
// The nodes that variant number `variant` fixes (fv: HostModel::fv; batching.py:171-175, 212-229), on top of fixmask / fixval
void variant_fixed_nodes(const std::vector<uint32_t>& fv, uint64_t variant, uint32_t* fixmask, uint32_t* fixval);
// The cube words of a pass over c's classes: count, cube, cube_shift, and rep_mask, rep_code, cube_t0_shift from P.tmask / P.tcode
void target_cube_words(const Cube& c, TargetParams& P);
// ... and its work shares over the `n_waves` waves of the grid: even fixed shares below 2^28 classes, else the cursor with `chunk`
void target_cube_shares(uint64_t n_waves, uint32_t chunk, TargetParams& P);
// Problems of the next listing pass: what is left, at least a cube unit's worth and four times the hits still wanted
uint64_t target_listing_piece(uint64_t left, uint64_t hits_wanted);
// Whether the counted part of a summary call may run as cube passes over this space (BSX_CUBES aside)
bool target_cubes_ok(const DevSpace& sp, bool variant_count_saturated);

// The counted part of bsx_run_target_summary, piece by piece: the piece that begins `done` problems into a call over
// [first, first + count).  Without cubes: plain pieces of at most 2^32.  With them (n_any <= 64), inside every variant:
// a plain head up to the first multiple of 2^kCubeMinBits, aligned blocks of 2^a_bits -- each the largest that its
// alignment and the end of the body allow, at most 2^kCubeMaxBits -- and a plain tail.
struct CountPiece {
    uint64_t n = 0;             // problems (the piece is [done, done + n) of the call's range)
    bool block = false;         // an aligned block of one variant: a cube pass if build_cube admits it
    uint64_t digit = 0;         // block: its first digit value (a multiple of n = 2^a_bits)
    uint32_t a_bits = 0;
    uint64_t variant = 0;       // the variant number the piece begins in
};
CountPiece count_piece(const bsx_index& first, uint64_t done, uint64_t count, uint32_t n_any, bool cubes_ok);

// ---- simulate
// Workgroups of the per-lane simulate kernel
uint64_t lane_sim_blocks(uint64_t count, uint32_t compute_units);
// Bit-sliced kernels.  knob_sliced: BSX_SLICED (1 keeps the first generation, 0 turns the family off)
inline uint32_t sliced_rows(uint32_t n_nodes) { return (n_nodes + 15) & ~15u; }     // node batch (4) x waves per workgroup (4)
bool sliced_gen2(uint32_t n_nodes, uint32_t k_mux, int knob_sliced);
// Whether a bsx_run_simulate call goes through them: long fixed-length runs that only want final states (digests: gen 2 only)
bool sliced_ok(uint32_t n_nodes, const DevNet& net, const DevSpace& sp, int knob_sliced, bool want_trajectories, bool want_final,
               bool want_digests, uint64_t max_t, uint64_t count);
struct SlicedShape {
    bool gen2;
    uint32_t rows;
    size_t shmem;
    uint64_t groups, per_cu, blocks;
};
SlicedShape sliced_shape(uint32_t n_nodes, uint32_t k_mux, int knob_sliced, uint64_t count, uint32_t compute_units);
// SlicedParams::desc: per row 6 predecessors and the truth table replicated to 2^k_mux (an origin-fixed node: a constant table)
void sliced_row_desc(const HostModel& m, const DevSpace& sp, uint32_t k_mux, std::vector<uint32_t>& desc);

}  // namespace bsx
