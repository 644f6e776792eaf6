// Attractor transitions: the plain records and limits that the host arithmetic (bsx_table_lower.h) shares with the
// kernels and their launch prototypes (bsx_trans.h, which includes this).  No HIP here.
#pragma once
#include <stdint.h>

namespace bsx {

constexpr uint64_t kTransMaxStates = 1ull << 28;    // BSX_TRANS_MAX_STATES
constexpr uint64_t kTransFlipChunk = 1ull << 28;    // flips per launch of the walk kernel
constexpr uint32_t kTransOutside = 0xFFFFFFFEu;     // BSX_TRANS_OUTSIDE
constexpr uint32_t kTransUnresolved = 0xFFFFFFFFu;  // BSX_TRANS_UNRESOLVED
constexpr uint32_t kTransNoRow = 0xFFFFFFFFu;

struct TransEdge {          // bsx_trans_edge
    uint32_t src, dst;
    uint64_t count, sum_mu;
};
static_assert(sizeof(TransEdge) == 24, "edge record layout");

struct alignas(8) TransCtr {            // zeroed (open_row / dup_row: all ones) before the build
    unsigned int open_row;              // least row whose walk did not close (kTransNoRow: none)
    unsigned int dup_row;               // least of the later rows of two equal states (kTransNoRow: none)
    unsigned int probe_full;            // k_trans_build: a probe went round the whole table (cannot happen at load <= 1/2)
    unsigned int step_limit_hits;       // walks undecided at the step limit
    unsigned int edge_overflow;         // the HBM edge table was full
    unsigned int rows_undecided;        // wide family: closed rows whose own walk ran into the step limit (else unused)
    unsigned long long n_edges;         // k_trans_drain's cursor
    unsigned long long steps_exec;      // network updates of the walk kernel
};
inline TransCtr trans_ctr_initial() {
    TransCtr c{};
    c.open_row = c.dup_row = kTransNoRow;
    return c;
}

}  // namespace bsx
