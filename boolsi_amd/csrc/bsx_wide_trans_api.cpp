// Attractor transitions on the wide-state family: host side of bsx_run_attractor_transitions_wide.  The checks and the
// plan (bsx_table_lower.h), then the enqueue chain
//     profile (states and closure stay in HBM) -> k_wide_trans over the rows -> k_wide_trans_build ->
//     k_wide_trans over the flips, BSX_WTRANS_CHUNK per launch -> k_trans_drain,
// one wait, and the edge sink's finish (bsx_table_host.h), as bsx_trans_api.cpp does for the <= 256 family.  This file
// keeps what is the wide family's own: the LDS fit, the row keys and their owner table, the x_0 spill, WideTransParams
// and the two-stage launches.
#include <algorithm>
#include <cstring>
#include <string>

#include "bsx_table_host.h"
#include "bsx_wide_host.h"
#include "bsx_wtrans.h"

using namespace bsx;

static_assert(kWtransOutside == kTransOutside && kWtransUnresolved == kTransUnresolved, "the pseudo-destinations");
static_assert(kWtransInf == BSX_T_INF, "no cap");

extern "C" int bsx_run_attractor_transitions_wide(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                                  uint64_t n, uint64_t max_t, bsx_trans_edge* edges, uint64_t edge_cap,
                                                  uint64_t* n_edges, uint32_t* node_exits, uint8_t* closed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!h->wide) return bsx_run_attractor_transitions(h, keys, key_stride, lengths, n, max_t, edges, edge_cap, n_edges, node_exits, closed, stats);
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    const std::string who = "bsx_run_attractor_transitions_wide";
    const TableView table{keys, key_stride, lengths, n};
    TableSizes sizes;
    if (int rc = table_check_args(h, who.c_str(), table, false, nullptr, sizes)) return rc;
    if (const LowerStatus s = trans_limits(n, sizes.sum_len, edges, n_edges)) return fail(h, s.status, who + ": " + s.msg);
    WideHost& W = *h->wide;
    const uint32_t rows = W.net.rows, L = W.space.L;
    const size_t shmem = (size_t)wide_trans_lds_words(rows, L, W.space.n_fslots) * 4;
    if (shmem > W.space.shmem || (size_t)rows * L * 4 < kTransLdsEdges * sizeof(TransEdgeSlot))
        return fail(h, BSX_ERR_UNSUPPORTED, who + ": the group's tables do not fit the LDS");
    HIPCHK(h, hipSetDevice(h->device));

    const uint32_t w64 = W.net.w64;
    const TransPlan plan = trans_plan(kTableWide, lengths, n, w64, W.space.fixmask, W.net.n, edge_cap);
    const TransSizes& sz = plan.sz;
    const uint64_t flip_chunk = trans_flip_chunk(kTableWide, h->knobs.wtrans_chunk);

    // the profile: states (row after row, the key first) and closure stay on the device; enqueued, not waited for
    ProfileDev prof;
    if (int rc = profile_stage(h, table, ProfileWant{false, true, true}, plan.offsets.data(), plan.sum_len * w64, prof)) return rc;
    if (int rc = profile_enqueue(h, table, prof)) return rc;

    EdgeSink sink;
    if (int rc = sink.prepare(h, plan, node_exits != nullptr)) return rc;
    // row keys and their owner table (sz.n_slots); the x_0 spill takes rows * L words per workgroup
    const uint64_t most_blocks = std::max(wide_blocks(h, W, std::min(n, kWideTransRowChunk), shmem),
                                          wide_blocks(h, W, std::min(std::max<uint64_t>(sz.flips, 1), flip_chunk), shmem));
    DevBuf<uint64_t> d_row_keys;
    DevBuf<uint32_t> d_owners, d_row_info, d_x0;
    HIPCHK(h, d_row_keys.alloc(n * w64));
    HIPCHK(h, d_row_info.alloc(2 * n));
    HIPCHK(h, d_owners.alloc(sz.n_slots));
    HIPCHK(h, d_x0.alloc((size_t)most_blocks * rows * L));
    HIPCHK(h, hipMemsetAsync(d_owners.p, 0, sz.n_slots * sizeof(uint32_t), h->stream));

    WideTransParams Q{};
    WideParams& P = Q.net;
    wide_fill_net(W, P);
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;
    P.x0 = d_x0.p;
    Q.key_stride = key_stride; Q.n_rows = n;
    Q.keys = prof.keys.p; Q.lengths = prof.lengths.p; Q.closed = prof.closed.p; Q.states = prof.states.p;
    Q.row_first = sink.d_row_first.p;
    Q.free_nodes = sink.d_free.p; Q.n_free = (uint32_t)plan.free_nodes.size();
    Q.row_info = d_row_info.p; Q.row_keys = d_row_keys.p;
    Q.owners = d_owners.p; Q.slot_mask = sz.n_slots - 1;
    Q.edges = sink.d_edges.p; Q.edge_mask = sz.edge_slots - 1;
    Q.node_exits = node_exits ? sink.d_exits.p : nullptr;
    Q.ctr = sink.d_tc.p;

    auto walk = [&](WideTransStage stage, uint64_t count, uint64_t chunk) -> int {
        Q.stage = stage;
        for (const Chunk c : chunks(count, chunk)) {
            Q.first = c.first;
            Q.count = c.count;
            HIPCHK(h, launch_wide_trans((int)W.net.K, dim3((uint32_t)wide_blocks(h, W, c.count, shmem)), shmem, h->stream, Q));
        }
        return BSX_OK;
    };
    if (int rc = walk(kWideTransRows, n, kWideTransRowChunk)) return rc;
    HIPCHK(h, launch_wide_trans_build(Q, h->stream));
    if (int rc = walk(kWideTransFlips, sz.flips, flip_chunk)) return rc;
    if (int rc = sink.drain(h, plan)) return rc;
    // the call's one wait (ev0: profile_enqueue, in front of its first launch)
    unsigned long long ctr[4] = {0, 0, 0, 0};
    float ms = 0.f;
    if (int rc = wide_timed_wait(h, W, ctr, ms, &sink.tc, sink.d_tc.p, sizeof(TransCtr))) return rc;

    uint64_t sum_mu = 0;
    if (int rc = sink.finish(h, who, prof, TransOut{edges, edge_cap, n_edges, node_exits, closed}, &sum_mu)) return rc;
    put_stats(stats, sz.flips, sum_mu, ctr[1] + sink.tc.steps_exec, ms, trans_launches(kTableWide, n, sz.flips, h->knobs.wtrans_chunk), t_begin);
    return BSX_OK;
}
