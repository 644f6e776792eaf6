// bsx_run_attractor_transitions (include/bsx.h): where every single-node flip of every cycle state of a listed
// attractor table ends.  Host side: argument checks, allocation, the enqueue chain
//     profile (states and closure stay in HBM) -> k_trans_build -> k_trans_walk per chunk of flips -> k_trans_drain,
// one wait, the flags -> status mapping, the sort of the edge list.  What only the device can know before the walk
// (a row that does not close, two rows that share a state) is left in TransCtr by k_trans_build; k_trans_walk looks
// at it first and walks nothing, so such a table is refused with nothing written although the host waits only once.
// The handle's problem space, cycle journal and mirror image are not touched.
// Networks on the wide-state family are refused here; bsx_run_attractor_transitions_wide (bsx_wide_trans_api.cpp) serves them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_trans.h"
#include "bsx_walk.h"

using namespace bsx;

static_assert(kTransMaxStates == BSX_TRANS_MAX_STATES, "the header states the limit");
static_assert(kTransOutside == BSX_TRANS_OUTSIDE && kTransUnresolved == BSX_TRANS_UNRESOLVED, "the header states the pseudo-destinations");
static_assert(sizeof(TransEdge) == sizeof(bsx_trans_edge), "edge record layout");
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
    uint64_t sum_len = 0, unused = 0;
    if (int rc = profile_check_args(h, who.c_str(), keys, key_stride, lengths, n, nullptr, nullptr, &sum_len, &unused)) return rc;
    if (!edges || !n_edges) return fail(h, BSX_ERR_INVALID, who + ": edges or n_edges is null");
    if (n > 0xFFFFFFFDull) return fail(h, BSX_ERR_INVALID, who + ": more than 2^32 - 3 attractors");
    if (sum_len > kTransMaxStates) return fail(h, BSX_ERR_UNSUPPORTED, who + ": more than 2^28 cycle states (BSX_TRANS_MAX_STATES)");
    HIPCHK(h, hipSetDevice(h->device));

    const uint32_t W = h->w64, n_nodes = h->n_nodes;
    std::vector<uint32_t> free_nodes;
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (!((h->sp.fixmask[i >> 5] >> (i & 31)) & 1u)) free_nodes.push_back(i);
    const uint32_t n_free = (uint32_t)free_nodes.size();
    const uint64_t flips = sum_len * n_free;                            // (< 2^28 * 2^8)

    // the profile: states (row after row, the key first) and closure stay on the device; enqueued, not waited for
    std::vector<uint64_t> offsets(n), row_first(n);
    for (uint64_t q = 0, at = 0; q < n; at += lengths[q], ++q) { row_first[q] = at; offsets[q] = at * W; }
    ProfileKeep kept;
    if (int rc = profile_lanes(h, keys, key_stride, lengths, n, nullptr, nullptr, offsets.data(), sum_len * W, nullptr, sum_len, nullptr,
                               t_begin, nullptr, &kept))
        return rc;

    // cycle-state table: a power of two >= 2 * sum_len slots (at least 2); edge table: a power of two >= twice the
    // distinct edges there can be or the caller takes, whichever is less
    uint32_t slot_bits = 1;
    while ((1ull << slot_bits) < 2 * sum_len) ++slot_bits;
    const uint64_t n_slots = 1ull << slot_bits;
    const uint64_t most_edges = n >= (1ull << 31) ? ~0ull : n * (n + 2);
    const uint64_t out_cap = std::min({edge_cap, flips, most_edges});
    uint64_t edge_slots = 2;
    while (edge_slots < 2 * (out_cap + 1)) edge_slots <<= 1;           // (+ 1: one edge too many must still find a slot)

    DevBuf<uint64_t> d_row_first;
    DevBuf<uint32_t> d_slots, d_state_row, d_free, d_exits;
    DevBuf<TransEdgeSlot> d_edges;
    DevBuf<TransEdge> d_out;
    DevBuf<TransCtr> d_tc;
    HIPCHK(h, d_row_first.upload(row_first));
    HIPCHK(h, d_free.upload(free_nodes));
    HIPCHK(h, d_slots.alloc(n_slots));
    HIPCHK(h, d_state_row.alloc(sum_len));
    HIPCHK(h, d_edges.alloc(edge_slots));
    HIPCHK(h, d_out.alloc(out_cap));
    HIPCHK(h, d_tc.alloc(1));
    if (node_exits) HIPCHK(h, d_exits.alloc(n * n_nodes));
    TransCtr tc{};
    tc.open_row = tc.dup_row = kTransNoRow;
    HIPCHK(h, hipMemcpyAsync(d_tc.p, &tc, sizeof(tc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_slots.p, 0, n_slots * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d_edges.p, 0, edge_slots * sizeof(TransEdgeSlot), h->stream));
    if (node_exits) HIPCHK(h, hipMemsetAsync(d_exits.p, 0, n * n_nodes * sizeof(uint32_t), h->stream));

    TransParams P{};
    P.net = h->net;
    for (int w = 0; w < kMaxW32; ++w) { P.fixmask[w] = h->sp.fixmask[w]; P.fixval[w] = h->sp.fixval[w]; }
    P.tab.states = kept.states.p;
    P.tab.slots = d_slots.p;
    P.tab.state_row = d_state_row.p;
    P.tab.slot_shift = 32 - slot_bits;
    P.tab.w64 = W;
    P.tab.n_states = sum_len;
    P.lengths = kept.lengths.p;
    P.free_nodes = d_free.p;
    P.n_free = n_free;
    P.step_limit = std::min<uint32_t>(kStepLimit, h->knobs.trans_step_limit);
    P.max_t = max_t;
    P.edges = d_edges.p;
    P.edge_mask = edge_slots - 1;
    P.node_exits = node_exits ? d_exits.p : nullptr;
    P.ctr = d_tc.p;

    uint32_t launches = kept.launches;
    HIPCHK(h, launch_trans_build(P.tab, kept.closed.p, n, d_row_first.p, d_tc.p, h->stream));
    ++launches;
    const size_t shmem = h->shmem + trans_lds_bytes();
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    const uint64_t block = (uint64_t)profile_block((int)h->net.nw);
    for (uint64_t at = 0; at < flips; at += kTransFlipChunk, ++launches) {
        P.flip0 = at;
        P.flip_count = std::min<uint64_t>(kTransFlipChunk, flips - at);
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 4, (P.flip_count + block - 1) / block));
        HIPCHK(h, launch_trans_walk((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), shmem, h->stream, P));
    }
    HIPCHK(h, launch_trans_drain(d_edges.p, edge_slots, d_out.p, out_cap, d_tc.p, h->stream));
    ++launches;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));                       // (ev0: profile_lanes, in front of its first launch)
    Counters ctr{};
    HIPCHK(h, hipMemcpyAsync(&ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&tc, d_tc.p, sizeof(tc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                         // the call's one wait

    if (tc.open_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.open_row) + " is not closed: its key does not return after its length");
    if (tc.dup_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.dup_row) + " shares a state with another row or repeats one of its own "
                                              "(a duplicate row, or a length that is a multiple of the period)");
    if (tc.probe_full) return fail(h, BSX_ERR_HIP, who + ": the cycle-state table overflowed");
    if (tc.step_limit_hits) return fail(h, BSX_ERR_STEP_LIMIT, who + ": a walk ran into the internal step limit");
    if (tc.edge_overflow || tc.n_edges > edge_cap)
        return fail(h, BSX_ERR_TABLE_FULL, who + ": more distinct edges than edge_cap");
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    std::vector<TransEdge> got(tc.n_edges);
    if (tc.n_edges) HIPCHK(h, hipMemcpy(got.data(), d_out.p, tc.n_edges * sizeof(TransEdge), hipMemcpyDeviceToHost));
    std::sort(got.begin(), got.end(), [](const TransEdge& a, const TransEdge& b) { return a.src != b.src ? a.src < b.src : a.dst < b.dst; });
    uint64_t sum_mu = 0;
    for (uint64_t e = 0; e < tc.n_edges; ++e) {
        edges[e] = bsx_trans_edge{got[e].src, got[e].dst, got[e].count, got[e].sum_mu};
        sum_mu += got[e].sum_mu;
    }
    *n_edges = tc.n_edges;
    if (node_exits) HIPCHK(h, hipMemcpy(node_exits, d_exits.p, n * n_nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (closed) HIPCHK(h, hipMemcpy(closed, kept.closed.p, n, hipMemcpyDeviceToHost));
    if (stats) {
        stats->problems = flips;
        stats->state_steps = sum_mu;
        stats->executed_steps = ctr.steps_exec + tc.steps_exec;
        stats->kernel_ms = ms;
        stats->kernel_launches = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}
