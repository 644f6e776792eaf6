// What the cube planner reads, as plain data: the host copies of the network and the problem space (HostModel) and
// what a handle has learned about its problem so far (PlanState).  No HIP and no handle here: bsx_cube_plan.cpp and
// tests/plan_check.cpp build with the host compiler alone.  bsx_engine owns one of each.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "bsx_device.h"

namespace bsx {

struct HostModel {
    uint32_t n_nodes = 0, nw = 0;       // nodes, 32-bit words per state
    std::vector<uint32_t> pred_offsets, pred_idx;
    std::vector<uint64_t> tt0;          // first table word of every node (all of it when k <= 6)
    std::vector<uint32_t> sched;        // origin perturbations (t, node, value), sorted by t
    std::vector<uint32_t> any;          // 'any' nodes in digit order (cube collapse: relevant-digit analysis)
    std::vector<uint32_t> fv;           // fixed-node variations (node, range) in digit order
};

// Experience of the cascade with the current problem space (bsx_set_problem_space starts it afresh).  Only speed
// depends on it: which top level a chain gets, how a block is split.
struct PlanState {
    double near_seen[2][kMaxCubeLevels + 1][2] = {};    // [top level / below][depth] -> classes seen, of them near a cycle
    uint32_t cube_depth_cap = 0;        // 0 = no experience yet; else the deepest level that paid off on this problem
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> split_cache;    // block size -> leaves (fix mask, values) of its split tree
    std::map<uint32_t, double> split_learned;           // ... how many classes' listing the handle had seen when it was grown (near_seen)
    std::map<uint32_t, uint32_t> split_regrown;         // ... and how often it was regrown because it did not fit a block
};

}  // namespace bsx
