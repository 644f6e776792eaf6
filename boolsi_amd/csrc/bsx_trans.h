// Single-node flip transitions of an attractor table (bsx_run_attractor_transitions, include/bsx.h): structures
// shared by bsx_trans_api.cpp and the kernels (bsx_trans.hip, bsx_trans_kernel.h), and the launch prototypes.  The
// records without HIP (TransEdge, TransCtr, the limits) are in bsx_trans_records.h.
#pragma once
#include <hip/hip_runtime.h>

#include "bsx_device.h"
#include "bsx_trans_records.h"

namespace bsx {

constexpr uint32_t kTransLdsEdges = 256;            // entries of a workgroup's LDS edge table (power of two)
constexpr uint32_t kTransLdsProbes = 4;             // ... probes before a record goes to the HBM table directly

// One slot of the edge tables (LDS and HBM).  key = ((src << 32) | dst) + 1, 0 = free: src <= 2^32 - 4, so the sum
// does not wrap.  The key is one word: whoever sees it sees all of it; count and sum_mu only ever take atomic adds.
struct TransEdgeSlot {
    unsigned long long key;
    unsigned long long count;
    unsigned long long sum_mu;
};
static_assert(sizeof(TransEdgeSlot) == 24, "edge slot layout");

// Cycle-state table in HBM: slot = owner, the index of a state in `states` plus one (0 = free), found by linear
// probing from the state's hash.  n_slots is a power of two >= 2 * n_states, at least 2.
struct TransTable {
    const uint64_t* states;     // [n_states][w64]: row q's states from index first(q) on, the key first
    uint32_t* slots;            // [1 << (32 - slot_shift)]
    uint32_t* state_row;        // [n_states]
    uint32_t slot_shift;        // slot of hash h: (h * golden) >> slot_shift
    uint32_t w64;
    uint64_t n_states;
};

struct TransParams {
    DevNet net;
    uint32_t fixmask[kMaxW32];
    uint32_t fixval[kMaxW32];
    TransTable tab;
    const uint64_t* lengths;        // [n]
    const uint32_t* free_nodes;     // [n_free] ascending
    uint32_t n_free;
    uint32_t step_limit;
    uint64_t flip0, flip_count;     // this launch walks flips [flip0, flip0 + flip_count); flip = state * n_free + j
    uint64_t max_t;                 // kWalkInf: none
    TransEdgeSlot* edges;           // HBM edge table
    uint64_t edge_mask;             // its slots - 1
    uint32_t* node_exits;           // nullable: [n][n_nodes]
    TransCtr* ctr;
};

hipError_t launch_trans_build(const TransTable& tab, const uint8_t* closed, uint64_t n_rows, const uint64_t* row_first, TransCtr* ctr,
                              hipStream_t st);
hipError_t launch_trans_walk(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P);
hipError_t launch_trans_drain(const TransEdgeSlot* edges, uint64_t slots, TransEdge* out, uint64_t cap, TransCtr* ctr, hipStream_t st);
size_t trans_lds_bytes();

}  // namespace bsx
