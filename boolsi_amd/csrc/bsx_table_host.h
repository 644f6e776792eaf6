// Private to the host files of the calls that take a caller's attractor table (bsx_profile_api.cpp, bsx_corr_api.cpp,
// bsx_trans_api.cpp, bsx_wide_trans_api.cpp): the profile stage both families share and the edge sink both transition
// calls share.  What they allocate, the chunks they launch and the statuses they answer come from bsx_table_lower.h.
//
// The profile stage in steps, each on the handle's stream:
//   table_check_args   every check of the table, before any device work
//   profile_stage      uploads keys and lengths, allocates what the want-set names (and clears the on-counts)
//   profile_enqueue    zeroes the family's counters, records ev0, one launch per chunk; never waits
//   profile_collect    records ev1, the call's one wait, copies back what the caller's non-null pointers ask for, stats
// bsx_run_attractor_profile and bsx_run_node_correlations run all four; the transition calls stop behind
// profile_enqueue and go on enqueueing on the states and the closure the profile leaves in HBM.
#pragma once
#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_table_lower.h"
#include "bsx_trans.h"

namespace bsx {

inline TableFamily table_family(const bsx_engine* h) { return h->wide ? kTableWide : kTableLanes; }

// table_check of bsx_table_lower.h with the handle's network and the family's step limit; `who` names the entry point
// in the error text.  On the wide family also: the profile kernel holds the rows a thread owns.
int table_check_args(bsx_handle h, const char* who, const TableView& t, bool want_states, const uint64_t* state_offsets, TableSizes& out);

struct ProfileWant {        // what a call wants on the device, whether or not the caller takes it on the host
    bool on_counts = false;
    bool states = false;    // states, with their offsets
    bool closed = false;
};
struct ProfileDev {         // a call's device side: freed when it goes out of scope
    ProfileWant want;
    DevBuf<uint64_t> keys, lengths, offsets, states;
    DevBuf<uint32_t> on_counts;     // [n][n_nodes]
    DevBuf<uint8_t> closed;
    uint64_t state_words = 0;
    uint32_t launches = 0;
};
struct ProfileOut {         // the caller's host buffers, each nullable
    uint32_t* on_counts;
    uint64_t* states;
    uint8_t* closed;
};
inline ProfileWant profile_want(const ProfileOut& out) { return ProfileWant{out.on_counts != nullptr, out.states != nullptr, out.closed != nullptr}; }

int profile_stage(bsx_handle h, const TableView& t, ProfileWant want, const uint64_t* state_offsets, uint64_t state_words, ProfileDev& dev);
int profile_enqueue(bsx_handle h, const TableView& t, ProfileDev& dev);
int profile_collect(bsx_handle h, const TableView& t, const ProfileDev& dev, const ProfileOut& out, uint64_t sum_len, bsx_stats* stats,
                    double t_begin);

// The end of a timed run of per-lane launches (the caller has zeroed d_ctr and recorded ev0 in front of it): records ev1,
// brings the counters back (and `bytes` of a caller's own counter block with them), waits, reads the device time.
// (The wide family's: wide_timed_wait, bsx_wide_host.h.)
inline int lane_timed_wait(bsx_handle h, Counters& ctr, float& ms, void* also = nullptr, const void* d_also = nullptr, size_t bytes = 0) {
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(&ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    if (bytes) HIPCHK(h, hipMemcpyAsync(also, d_also, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    return BSX_OK;
}

// ---- the transition calls ----
struct TransOut {           // the caller's host buffers: edges[edge_cap] and n_edges required, the rest nullable
    bsx_trans_edge* edges;
    uint64_t edge_cap;
    uint64_t* n_edges;
    uint32_t* node_exits;
    uint8_t* closed;
};

// Where both transition calls collect their edges: the HBM edge table the walk kernels add to, the records
// k_trans_drain packs out of it, the device's flags and counters (TransCtr), the exits per node, and the two lists every
// walk kernel reads (free nodes, first state of a row).
struct EdgeSink {
    DevBuf<uint64_t> d_row_first;
    DevBuf<uint32_t> d_free, d_exits;
    DevBuf<TransEdgeSlot> d_edges;
    DevBuf<TransEdge> d_out;
    DevBuf<TransCtr> d_tc;
    TransCtr tc{};          // what the device starts from; after the caller's wait, what it left (the wait reads d_tc into it)

    // allocates for `plan`, uploads the lists, enqueues TransCtr's initial value and the clears
    int prepare(bsx_handle h, const TransPlan& plan, bool want_exits);
    // enqueues k_trans_drain: edge table -> records, their number into TransCtr
    int drain(bsx_handle h, const TransPlan& plan);
    // after the wait: the status of `tc`; on BSX_OK the sorted edges, n_edges, the exits and the profile's closure go to
    // `out` and the sum of all sum_mu to *sum_mu.  On a refusal nothing is written but the error text.
    int finish(bsx_handle h, const std::string& who, const ProfileDev& prof, const TransOut& out, uint64_t* sum_mu);
};

}  // namespace bsx
