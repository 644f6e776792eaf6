// bsx_table_lower.h: the host arithmetic of the attractor-table calls.  No HIP.
#include "bsx_table_lower.h"

#include <numeric>

namespace bsx {

static_assert(kTransMaxStates == BSX_TRANS_MAX_STATES, "the header states the limit");
static_assert(kTransOutside == BSX_TRANS_OUTSIDE && kTransUnresolved == BSX_TRANS_UNRESOLVED, "the header states the pseudo-destinations");
static_assert(sizeof(TransEdge) == sizeof(bsx_trans_edge), "edge record layout");

LowerStatus table_check(const TableView& t, bool want_states, const uint64_t* state_offsets, uint32_t w64, uint32_t n_nodes,
                        uint64_t step_limit, TableSizes& out) {
    if (!t.keys || !t.lengths) return {BSX_ERR_INVALID, "keys or lengths is null"};
    if (want_states && !state_offsets) return {BSX_ERR_INVALID, "states without state_offsets"};
    if (t.key_stride < w64) return {BSX_ERR_INVALID, "key_stride is below the words per state"};
    if (t.n > (1ull << 32)) return {BSX_ERR_INVALID, "at most 2^32 attractors per call"};
    // lengths: 1 <= length, and no walk beyond the family's step limit
    uint64_t sum_len = 0;
    bool too_long = false;
    for (uint64_t q = 0; q < t.n; ++q) {
        if (t.lengths[q] == 0) return {BSX_ERR_INVALID, "an attractor of length 0"};
        too_long = too_long || t.lengths[q] >= step_limit;
        if (!too_long) sum_len += t.lengths[q];
    }
    if (too_long) return {BSX_ERR_STEP_LIMIT, "a walk would exceed the internal step limit"};
    // keys: no bit at or above n_nodes in the words the kernels read
    if (n_nodes & 63u) {
        const uint64_t above = ~0ull << (n_nodes & 63u);
        for (uint64_t q = 0; q < t.n; ++q)
            if (t.keys[q * t.key_stride + (w64 - 1)] & above) return {BSX_ERR_INVALID, "a key has bits at or above n_nodes"};
    }
    // states: the ranges [offset, offset + length * w64) must not overlap; their end is the size of the output
    uint64_t state_words = 0;
    if (want_states) {
        std::vector<uint64_t> order(t.n);
        std::iota(order.begin(), order.end(), 0ull);
        std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return state_offsets[a] < state_offsets[b]; });
        for (uint64_t i = 0; i < t.n; ++i) {
            const uint64_t off = state_offsets[order[i]], need = t.lengths[order[i]] * w64;     // (< 2^30 * 16)
            if (off < state_words) return {BSX_ERR_INVALID, "state ranges overlap"};
            if (off > (1ull << 56)) return {BSX_ERR_INVALID, "state offset out of range"};
            state_words = off + need;
        }
    }
    out.sum_len = sum_len;
    out.state_words = state_words;
    return {};
}

LowerStatus trans_limits(uint64_t n, uint64_t sum_len, const void* edges, const void* n_edges) {
    if (!edges || !n_edges) return {BSX_ERR_INVALID, "edges or n_edges is null"};
    if (n > 0xFFFFFFFDull) return {BSX_ERR_INVALID, "more than 2^32 - 3 attractors"};
    if (sum_len > kTransMaxStates) return {BSX_ERR_UNSUPPORTED, "more than 2^28 cycle states (BSX_TRANS_MAX_STATES)"};
    return {};
}

TransSizes trans_sizes(TableFamily family, uint64_t n, uint64_t sum_len, uint32_t n_free, uint64_t edge_cap) {
    TransSizes s;
    s.flips = sum_len * n_free;                                         // (< 2^28 * 2^10)
    const uint64_t entries = family == kTableWide ? n : sum_len;
    while ((1ull << s.slot_bits) < 2 * entries) ++s.slot_bits;
    s.n_slots = 1ull << s.slot_bits;
    s.most_edges = n >= (1ull << 31) ? ~0ull : n * (n + 2);
    s.out_cap = std::min({edge_cap, s.flips, s.most_edges});
    while (s.edge_slots < 2 * (s.out_cap + 1)) s.edge_slots <<= 1;
    return s;
}

TransPlan trans_plan(TableFamily family, const uint64_t* lengths, uint64_t n, uint32_t w64, const uint32_t* fixmask, uint32_t n_nodes,
                     uint64_t edge_cap) {
    TransPlan p;
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (!((fixmask[i >> 5] >> (i & 31)) & 1u)) p.free_nodes.push_back(i);
    p.row_first.resize(n);
    p.offsets.resize(n);
    for (uint64_t q = 0; q < n; p.sum_len += lengths[q], ++q) {
        p.row_first[q] = p.sum_len;
        p.offsets[q] = p.sum_len * w64;
    }
    p.sz = trans_sizes(family, n, p.sum_len, (uint32_t)p.free_nodes.size(), edge_cap);
    return p;
}

int trans_status(TableFamily family, const TransCtr& tc, uint64_t edge_cap, std::string& text) {
    const bool wide = family == kTableWide;
    const unsigned int open = tc.open_row, dup = tc.dup_row;
    if (open != kTransNoRow) {
        text = "row " + std::to_string(open) + " is not closed: its key does not return after its length";
        return BSX_ERR_INVALID;
    }
    if (dup != kTransNoRow) {
        text = "row " + std::to_string(dup) +
               (wide ? " lies on the cycle of another row or repeats its own " : " shares a state with another row or repeats one of its own ") +
               "(a duplicate row, or a length that is a multiple of the period)";
        return BSX_ERR_INVALID;
    }
    if (tc.probe_full) {
        text = wide ? "the row-key table overflowed" : "the cycle-state table overflowed";
        return BSX_ERR_HIP;
    }
    if (tc.step_limit_hits || (wide && tc.rows_undecided)) {
        text = "a walk ran into the internal step limit";
        return BSX_ERR_STEP_LIMIT;
    }
    if (tc.edge_overflow || tc.n_edges > edge_cap) {
        text = "more distinct edges than edge_cap";
        return BSX_ERR_TABLE_FULL;
    }
    return BSX_OK;
}

uint64_t trans_finish_edges(std::vector<TransEdge>& got, bsx_trans_edge* edges) {
    std::sort(got.begin(), got.end(), [](const TransEdge& a, const TransEdge& b) { return a.src != b.src ? a.src < b.src : a.dst < b.dst; });
    uint64_t sum_mu = 0;
    for (size_t e = 0; e < got.size(); ++e) {
        edges[e] = bsx_trans_edge{got[e].src, got[e].dst, got[e].count, got[e].sum_mu};
        sum_mu += got[e].sum_mu;
    }
    return sum_mu;
}

}  // namespace bsx
