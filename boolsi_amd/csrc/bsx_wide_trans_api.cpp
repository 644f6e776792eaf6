// Attractor transitions on the wide-state family: host side of bsx_run_attractor_transitions_wide.  Argument checks,
// allocation, the enqueue chain
//     profile (states and closure stay in HBM) -> k_wide_trans over the rows -> k_wide_trans_build ->
//     k_wide_trans over the flips, BSX_WTRANS_CHUNK per launch -> k_trans_drain,
// one wait, the flags -> status mapping and the sort of the edge list, as bsx_trans_api.cpp does for the <= 256 family.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bsx_trans.h"
#include "bsx_wide_host.h"
#include "bsx_wtrans.h"

using namespace bsx;

static_assert(kWtransOutside == kTransOutside && kWtransUnresolved == kTransUnresolved, "the pseudo-destinations");
static_assert(kWtransInf == BSX_T_INF, "no cap");
constexpr uint64_t kWideTransRowChunk = 1ull << 18;     // rows per launch of the rows' walks
constexpr uint64_t kWideTransFlipChunk = 1ull << 22;    // flips per launch (BSX_WTRANS_CHUNK)

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
    uint64_t sum_len = 0, unused = 0;
    if (int rc = profile_check_args(h, who.c_str(), keys, key_stride, lengths, n, nullptr, nullptr, &sum_len, &unused)) return rc;
    if (!edges || !n_edges) return fail(h, BSX_ERR_INVALID, who + ": edges or n_edges is null");
    if (n > 0xFFFFFFFDull) return fail(h, BSX_ERR_INVALID, who + ": more than 2^32 - 3 attractors");
    if (sum_len > kTransMaxStates) return fail(h, BSX_ERR_UNSUPPORTED, who + ": more than 2^28 cycle states (BSX_TRANS_MAX_STATES)");
    WideHost& W = *h->wide;
    const uint32_t rows = W.net.rows, L = W.space.L;
    const size_t shmem = (size_t)wide_trans_lds_words(rows, L, W.space.n_fslots) * 4;
    if (shmem > W.space.shmem || (size_t)rows * L * 4 < kTransLdsEdges * sizeof(TransEdgeSlot))
        return fail(h, BSX_ERR_UNSUPPORTED, who + ": the group's tables do not fit the LDS");
    HIPCHK(h, hipSetDevice(h->device));

    const uint32_t w64 = W.net.w64, n_nodes = W.net.n;
    std::vector<uint32_t> free_nodes;
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (!((W.space.fixmask[i >> 5] >> (i & 31)) & 1u)) free_nodes.push_back(i);
    const uint32_t n_free = (uint32_t)free_nodes.size();
    const uint64_t flips = sum_len * n_free;                            // (< 2^28 * 2^10)

    // the profile: states (row after row, the key first) and closure stay on the device; enqueued, not waited for
    std::vector<uint64_t> offsets(n), row_first(n);
    for (uint64_t q = 0, at = 0; q < n; at += lengths[q], ++q) { row_first[q] = at; offsets[q] = at * w64; }
    ProfileKeep kept;
    if (int rc = wide_run_profile(h, keys, key_stride, lengths, n, nullptr, nullptr, offsets.data(), sum_len * w64, nullptr, sum_len,
                                  nullptr, nullptr, &kept))
        return rc;

    // row-key table: a power of two >= 2 n owners (at least 2); edge table as in bsx_trans_api.cpp
    uint64_t n_slots = 2;
    while (n_slots < 2 * n) n_slots <<= 1;
    const uint64_t most_edges = n >= (1ull << 31) ? ~0ull : n * (n + 2);
    const uint64_t out_cap = std::min({edge_cap, flips, most_edges});
    uint64_t edge_slots = 2;
    while (edge_slots < 2 * (out_cap + 1)) edge_slots <<= 1;           // (+ 1: one edge too many must still find a slot)
    const uint64_t flip_chunk = h->knobs.wtrans_chunk ? std::min<uint64_t>(h->knobs.wtrans_chunk, 1ull << 28) : kWideTransFlipChunk;
    // the x_0 spill takes rows * L words per workgroup
    const uint64_t most_blocks = std::max(wide_blocks(h, W, std::min(n, kWideTransRowChunk), shmem),
                                          wide_blocks(h, W, std::min(std::max<uint64_t>(flips, 1), flip_chunk), shmem));

    DevBuf<uint64_t> d_row_first, d_row_keys;
    DevBuf<uint32_t> d_owners, d_row_info, d_free, d_exits, d_x0;
    DevBuf<TransEdgeSlot> d_edges;
    DevBuf<TransEdge> d_out;
    DevBuf<TransCtr> d_tc;
    HIPCHK(h, d_row_first.upload(row_first));
    HIPCHK(h, d_free.upload(free_nodes));
    HIPCHK(h, d_row_keys.alloc(n * w64));
    HIPCHK(h, d_row_info.alloc(2 * n));
    HIPCHK(h, d_owners.alloc(n_slots));
    HIPCHK(h, d_x0.alloc((size_t)most_blocks * rows * L));
    HIPCHK(h, d_edges.alloc(edge_slots));
    HIPCHK(h, d_out.alloc(out_cap));
    HIPCHK(h, d_tc.alloc(1));
    if (node_exits) HIPCHK(h, d_exits.alloc(n * n_nodes));
    TransCtr tc{};
    tc.open_row = tc.dup_row = kTransNoRow;
    HIPCHK(h, hipMemcpyAsync(d_tc.p, &tc, sizeof(tc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_owners.p, 0, n_slots * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d_edges.p, 0, edge_slots * sizeof(TransEdgeSlot), h->stream));
    if (node_exits) HIPCHK(h, hipMemsetAsync(d_exits.p, 0, n * n_nodes * sizeof(uint32_t), h->stream));

    WideTransParams Q{};
    WideParams& P = Q.net;
    wide_fill_net(W, P);
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;
    P.x0 = d_x0.p;
    Q.key_stride = key_stride; Q.n_rows = n;
    Q.keys = kept.keys.p; Q.lengths = kept.lengths.p; Q.closed = kept.closed.p; Q.states = kept.states.p;
    Q.row_first = d_row_first.p;
    Q.free_nodes = d_free.p; Q.n_free = n_free;
    Q.row_info = d_row_info.p; Q.row_keys = d_row_keys.p;
    Q.owners = d_owners.p; Q.slot_mask = n_slots - 1;
    Q.edges = d_edges.p; Q.edge_mask = edge_slots - 1;
    Q.node_exits = node_exits ? d_exits.p : nullptr;
    Q.ctr = d_tc.p;

    uint32_t launches = kept.launches;
    Q.stage = kWideTransRows;
    for (uint64_t at = 0; at < n; at += kWideTransRowChunk, ++launches) {
        Q.first = at;
        Q.count = std::min<uint64_t>(kWideTransRowChunk, n - at);
        HIPCHK(h, launch_wide_trans((int)W.net.K, dim3((uint32_t)wide_blocks(h, W, Q.count, shmem)), shmem, h->stream, Q));
    }
    HIPCHK(h, launch_wide_trans_build(Q, h->stream));
    ++launches;
    Q.stage = kWideTransFlips;
    for (uint64_t at = 0; at < flips; at += flip_chunk, ++launches) {
        Q.first = at;
        Q.count = std::min<uint64_t>(flip_chunk, flips - at);
        HIPCHK(h, launch_wide_trans((int)W.net.K, dim3((uint32_t)wide_blocks(h, W, Q.count, shmem)), shmem, h->stream, Q));
    }
    HIPCHK(h, launch_trans_drain(d_edges.p, edge_slots, d_out.p, out_cap, d_tc.p, h->stream));
    ++launches;
    // the call's one wait (ev0: wide_run_profile, in front of its first launch)
    unsigned long long ctr[4] = {0, 0, 0, 0};
    float ms = 0.f;
    if (int rc = wide_timed_wait(h, W, ctr, ms, &tc, d_tc.p, sizeof(tc))) return rc;

    if (tc.open_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.open_row) + " is not closed: its key does not return after its length");
    if (tc.dup_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.dup_row) + " lies on the cycle of another row or repeats its own "
                                              "(a duplicate row, or a length that is a multiple of the period)");
    if (tc.probe_full) return fail(h, BSX_ERR_HIP, who + ": the row-key table overflowed");
    if (tc.step_limit_hits || tc.rows_undecided) return fail(h, BSX_ERR_STEP_LIMIT, who + ": a walk ran into the internal step limit");
    if (tc.edge_overflow || tc.n_edges > edge_cap)
        return fail(h, BSX_ERR_TABLE_FULL, who + ": more distinct edges than edge_cap");
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
    put_stats(stats, flips, sum_mu, ctr[1] + tc.steps_exec, ms, launches, t_begin);
    return BSX_OK;
}
