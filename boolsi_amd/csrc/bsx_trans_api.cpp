// bsx_run_attractor_transitions (include/bsx.h): where every single-node flip of every cycle state of a listed
// attractor table ends.  Host side: the checks and the plan (bsx_table_lower.h), then the enqueue chain
//     profile (states and closure stay in HBM) -> k_trans_build -> k_trans_walk per chunk of flips -> k_trans_drain,
// one wait, and the edge sink's finish (bsx_table_host.h): flags -> status, the sorted edge list.  This file keeps what
// is the per-lane family's own: the cycle-state table, TransParams and the walk launches.  What only the device can
// know before the walk (a row that does not close, two rows that share a state) is left in TransCtr by k_trans_build;
// k_trans_walk looks at it first and walks nothing, so such a table is refused with nothing written although the host
// waits only once.  The handle's problem space, cycle journal and mirror image are not touched.
// Networks on the wide-state family are refused here; bsx_run_attractor_transitions_wide (bsx_wide_trans_api.cpp) serves them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bsx_table_host.h"
#include "bsx_walk.h"

using namespace bsx;

static_assert(kWalkInf == BSX_T_INF, "no cap");

extern "C" int bsx_run_attractor_transitions(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                             uint64_t n, uint64_t max_t, bsx_trans_edge* edges, uint64_t edge_cap, uint64_t* n_edges,
                                             uint32_t* node_exits, uint8_t* closed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    const std::string who = "bsx_run_attractor_transitions";
    if (h->wide)
        return fail(h, BSX_ERR_UNSUPPORTED, who + ": the network runs on the wide-state family (more than 256 nodes, or BSX_WIDE=1), "
                                                  "which this call does not support");
    const TableView table{keys, key_stride, lengths, n};
    TableSizes sizes;
    if (int rc = table_check_args(h, who.c_str(), table, false, nullptr, sizes)) return rc;
    if (const LowerStatus s = trans_limits(n, sizes.sum_len, edges, n_edges)) return fail(h, s.status, who + ": " + s.msg);
    HIPCHK(h, hipSetDevice(h->device));

    const uint32_t W = h->w64;
    const TransPlan plan = trans_plan(kTableLanes, lengths, n, W, h->sp.fixmask, h->n_nodes, edge_cap);
    const TransSizes& sz = plan.sz;

    // the profile: states (row after row, the key first) and closure stay on the device; enqueued, not waited for
    ProfileDev prof;
    if (int rc = profile_stage(h, table, ProfileWant{false, true, true}, plan.offsets.data(), plan.sum_len * W, prof)) return rc;
    if (int rc = profile_enqueue(h, table, prof)) return rc;

    EdgeSink sink;
    if (int rc = sink.prepare(h, plan, node_exits != nullptr)) return rc;
    DevBuf<uint32_t> d_slots, d_state_row;                              // the cycle-state table
    HIPCHK(h, d_slots.alloc(sz.n_slots));
    HIPCHK(h, d_state_row.alloc(plan.sum_len));
    HIPCHK(h, hipMemsetAsync(d_slots.p, 0, sz.n_slots * sizeof(uint32_t), h->stream));

    TransParams P{};
    P.net = h->net;
    for (int w = 0; w < kMaxW32; ++w) { P.fixmask[w] = h->sp.fixmask[w]; P.fixval[w] = h->sp.fixval[w]; }
    P.tab.states = prof.states.p;
    P.tab.slots = d_slots.p;
    P.tab.state_row = d_state_row.p;
    P.tab.slot_shift = 32 - sz.slot_bits;
    P.tab.w64 = W;
    P.tab.n_states = plan.sum_len;
    P.lengths = prof.lengths.p;
    P.free_nodes = sink.d_free.p;
    P.n_free = (uint32_t)plan.free_nodes.size();
    P.step_limit = std::min<uint32_t>(kStepLimit, h->knobs.trans_step_limit);
    P.max_t = max_t;
    P.edges = sink.d_edges.p;
    P.edge_mask = sz.edge_slots - 1;
    P.node_exits = node_exits ? sink.d_exits.p : nullptr;
    P.ctr = sink.d_tc.p;

    HIPCHK(h, launch_trans_build(P.tab, prof.closed.p, n, sink.d_row_first.p, sink.d_tc.p, h->stream));
    const size_t shmem = h->shmem + trans_lds_bytes();
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    const uint64_t block = (uint64_t)profile_block((int)h->net.nw);
    for (const Chunk c : chunks(sz.flips, trans_flip_chunk(kTableLanes, 0))) {
        P.flip0 = c.first;
        P.flip_count = c.count;
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 4, (c.count + block - 1) / block));
        HIPCHK(h, launch_trans_walk((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), shmem, h->stream, P));
    }
    if (int rc = sink.drain(h, plan)) return rc;
    // the call's one wait (ev0: profile_enqueue, in front of its first launch)
    Counters ctr{};
    float ms = 0.f;
    if (int rc = lane_timed_wait(h, ctr, ms, &sink.tc, sink.d_tc.p, sizeof(TransCtr))) return rc;

    uint64_t sum_mu = 0;
    if (int rc = sink.finish(h, who, prof, TransOut{edges, edge_cap, n_edges, node_exits, closed}, &sum_mu)) return rc;
    put_stats(stats, sz.flips, sum_mu, ctr.steps_exec + sink.tc.steps_exec, ms, trans_launches(kTableLanes, n, sz.flips, 0), t_begin);
    return BSX_OK;
}
