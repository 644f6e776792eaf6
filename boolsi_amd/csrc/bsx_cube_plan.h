// Cube analysis and planning (DESIGN.md "cube collapse", "deeper collapse", "sub-blocks"): which digits of an aligned
// block F^d can depend on, what a cascade over them is estimated to cost, which top level and which split of the
// block that estimate prefers.  Plain host arithmetic over the truth tables -- no HIP, no handle: everything here takes
// the planner's inputs as data (bsx_model.h), and tests/plan_check.cpp checks it against brute force on any CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "bsx_device.h"
#include "bsx_model.h"

namespace bsx {

constexpr uint32_t kCubeMinBits = 16;           // cube collapse: smallest aligned block handled as a cube
constexpr uint32_t kCubeMaxBits = 63;           // ... and the largest (member counts are 64-bit; a 2^64 space is two blocks)
constexpr uint32_t kSplitMinBits = 52;          // smaller blocks finish in less time than the extra launches of their sub-blocks take
constexpr double kLevelOverheadUs = 22.0;       // cascade: what one more level costs whatever its size (cost estimates)

// ---- cube collapse: which of the `a` lowest initial-state digits can the FIRST update of the
// block starting at digit value d_lo depend on?  (attract's cascade and target's summary passes)
struct Cube {
    uint64_t d_lo;              // first digit value (multiple of 2^a)
    uint32_t a;                 // log2 of the problems in the block
    // A SUB-BLOCK fixes some of the block's a lowest digits as well (fix_mask / fix_vals over the digit index): the block is the
    // disjoint union of the sub-blocks of a split, and fixing a well-chosen digit makes many others irrelevant
    // (plan_split).  free_digits = the digits that vary, n_free of them: the sub-block has 2^n_free problems.
    uint64_t fix_mask = 0, fix_vals = 0, free_digits = 0;
    uint32_t n_free = 0;
    std::vector<uint32_t> rel;  // relevant digits: ascending from build_cube, then in class-index bit order
    uint32_t base[kMaxW32];     // the block's fixed bits, free bits zero
    DevSpace sp;                // enumeration of the relevant digits' assignments (plan_cube)
    uint32_t umask[kMaxW32];    // node bits of the irrelevant free digits
    uint32_t free_mask[kMaxW32];
    bool ok = false;            // false: more deposit runs than the kernels take
};
// fixmask: the fixed nodes that count (null: sp.fixmask; target passes: those of the block's fixed-node variant)
void build_cube(const HostModel& m, const DevSpace& sp, uint64_t d_lo, uint32_t a, Cube& c, const uint32_t* fixmask = nullptr,
                uint64_t fix_mask = 0, uint64_t fix_vals = 0);
void plan_cube(const HostModel& m, const DevSpace& sp, Cube& c);
// out[d - 1] = the digits of the block F^d may depend on, d = 1 .. max_depth (masks over the digit index)
void cube_levels(const HostModel& m, const DevSpace& sp, const Cube& c, uint32_t max_depth, std::vector<uint64_t>& out);
bool build_leaf_program(const HostModel& m, const DevSpace& sp, const std::vector<uint32_t>& added_digits, LeafProgram& L);

// What every cascade of a call shares: the time caps in the units the kernels count in, the FAST length, the deepest level.
struct CascadeShape {
    uint64_t tp, cap_rel;
    uint32_t cap_rel32, fast_steps, max_depth;
    bool forced_depth;
};

double near_fraction(const PlanState& ps, uint32_t d, bool is_top);
double chain_cost_us(const PlanState& ps, const std::vector<uint64_t>& rel_mask, uint32_t top);
// -> the top level (depth) that minimises the estimate, and the estimate
uint32_t choose_top(const PlanState& ps, const CascadeShape& sh, const std::vector<uint64_t>& rel_mask, uint32_t max_depth, double* est_out = nullptr);
// the estimate for the (sub-)block with the digits `mask` fixed at `vals`; top_rel = the digits its top level enumerates
double cube_cost_us(const HostModel& m, const DevSpace& sp, const PlanState& ps, const CascadeShape& sh, uint64_t d_lo, uint32_t a_bits,
                    uint64_t mask, uint64_t vals, uint64_t* top_rel = nullptr);

struct SplitLeaf { uint64_t mask, vals; };
void plan_split(const HostModel& m, const DevSpace& sp, const PlanState& ps, const CascadeShape& sh, uint64_t d_lo, uint32_t a_bits, bool forced,
                std::vector<SplitLeaf>& leaves);

}  // namespace bsx
