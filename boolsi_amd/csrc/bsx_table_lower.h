// Host arithmetic of the calls that take a caller's attractor table (keys, lengths) -- bsx_run_attractor_profile,
// bsx_run_node_correlations, bsx_run_attractor_transitions and its _wide twin -- without HIP: the checks of the table,
// the limits and the sizes of the transition calls, the chunks of every launch loop, the device flags -> status
// mapping and the finish of the edge list.  Plain C++ over include/bsx.h: tests/table_lower_check.cpp builds this unit
// with the host compiler alone.  bsx_table_host.h allocates, uploads and launches what it returns.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "bsx.h"
#include "bsx_device.h"
#include "bsx_lower_status.h"
#include "bsx_trans_records.h"

namespace bsx {

enum TableFamily : uint32_t { kTableLanes = 0, kTableWide = 1 };     // n <= BSX_MAX_NODES per lane; the wide-state family

// A caller's table: n rows of key_stride words (the first w64 of each used) and their lengths.
struct TableView {
    const uint64_t* keys = nullptr;
    uint32_t key_stride = 0;
    const uint64_t* lengths = nullptr;
    uint64_t n = 0;
};

// ---- the table check ----
// A walk's length limit: kStepLimit, on the wide family lock steps of a group, which BSX_WIDE_STEP_LIMIT lowers.
inline uint64_t table_step_limit(TableFamily family, uint32_t wide_step_limit) {
    return family == kTableWide ? std::min<uint64_t>(kStepLimit, wide_step_limit) : kStepLimit;
}
struct TableSizes {
    uint64_t sum_len = 0;       // sum of the lengths
    uint64_t state_words = 0;   // end of the last state range: the size of `states` in words (0 without states)
};
// Everything bsx_run_attractor_profile checks before it launches (include/bsx.h), n > 0; the text lacks the entry
// point's name.  want_states: the caller passed `states` (state_offsets may still be null: refused).
LowerStatus table_check(const TableView& t, bool want_states, const uint64_t* state_offsets, uint32_t w64, uint32_t n_nodes,
                        uint64_t step_limit, TableSizes& out);

// ---- chunks: [0, count) in launches of `chunk`, as (first, count) pairs ----
struct Chunk {
    uint64_t first, count;
};
struct Chunks {
    uint64_t total, chunk;
    struct Iter {
        uint64_t at, total, chunk;
        Chunk operator*() const { return Chunk{at, std::min(chunk, total - at)}; }
        Iter& operator++() { at += std::min(chunk, total - at); return *this; }
        bool operator!=(const Iter& o) const { return at != o.at; }
    };
    Iter begin() const { return Iter{0, total, chunk}; }
    Iter end() const { return Iter{total, total, chunk}; }
    uint64_t size() const { return total / chunk + (total % chunk != 0); }
};
inline Chunks chunks(uint64_t count, uint64_t chunk) { return Chunks{count, chunk}; }

constexpr uint64_t kWideTransRowChunk = 1ull << 18;     // rows per launch of the wide rows' walks
constexpr uint64_t kWideTransFlipChunk = 1ull << 22;    // flips per launch on the wide family (BSX_WTRANS_CHUNK)
// attractors per profile launch: BSX_PROFILE_CHUNK / BSX_PROFILE_CHUNK_WIDE
inline uint64_t profile_chunk(TableFamily family) { return family == kTableWide ? BSX_PROFILE_CHUNK_WIDE : BSX_PROFILE_CHUNK; }
// flips per walk launch; wtrans_chunk: the BSX_WTRANS_CHUNK knob (0 = not set), which only the wide family reads
inline uint64_t trans_flip_chunk(TableFamily family, uint64_t wtrans_chunk) {
    if (family == kTableLanes) return kTransFlipChunk;
    return wtrans_chunk ? std::min<uint64_t>(wtrans_chunk, 1ull << 28) : kWideTransFlipChunk;
}
inline uint32_t profile_launches(TableFamily family, uint64_t n) { return (uint32_t)chunks(n, profile_chunk(family)).size(); }
// kernel_launches of a transition call: profile, (wide: the rows' walks,) build, the flips' walks, drain
inline uint32_t trans_launches(TableFamily family, uint64_t n, uint64_t flips, uint64_t wtrans_chunk) {
    const uint64_t rows = family == kTableWide ? chunks(n, kWideTransRowChunk).size() : 0;
    return (uint32_t)(profile_launches(family, n) + rows + 1 + chunks(flips, trans_flip_chunk(family, wtrans_chunk)).size() + 1);
}

// ---- the transition calls: limits and plan ----
// edges / n_edges non-null, n <= 2^32 - 3 (row numbers and the two pseudo-destinations are u32), sum_len <= kTransMaxStates
LowerStatus trans_limits(uint64_t n, uint64_t sum_len, const void* edges, const void* n_edges);

// The sizes of a call from its counts alone.  Hash table (per lane: of the sum_len cycle states; wide: of the n row
// keys): a power of two >= twice the entries, at least 2.  Edge table: a power of two >= twice the distinct edges there
// can be or the caller takes, whichever is less, plus one: one edge too many must still find a slot.
struct TransSizes {
    uint64_t flips = 0;         // sum_len * n_free
    uint32_t slot_bits = 1;
    uint64_t n_slots = 2;       // 1 << slot_bits
    uint64_t most_edges = 0;    // n * (n + 2): every row to every row and the two pseudo-destinations (saturates from n = 2^31)
    uint64_t out_cap = 0;       // min(edge_cap, flips, most_edges)
    uint64_t edge_slots = 2;
};
TransSizes trans_sizes(TableFamily family, uint64_t n, uint64_t sum_len, uint32_t n_free, uint64_t edge_cap);

struct TransPlan {
    TransSizes sz;
    std::vector<uint32_t> free_nodes;       // the nodes the fix mask leaves free, ascending
    std::vector<uint64_t> row_first;        // index of a row's first state: the states lie row after row
    std::vector<uint64_t> offsets;          // ... in words: the profile's state_offsets
    uint64_t sum_len = 0;
};
// lengths[n] have passed table_check and trans_limits; fixmask: bit i of word i / 32 set = node i is fixed
TransPlan trans_plan(TableFamily family, const uint64_t* lengths, uint64_t n, uint32_t w64, const uint32_t* fixmask, uint32_t n_nodes,
                     uint64_t edge_cap);

// ---- after the wait ----
// What the device left in TransCtr -> BSX_OK, or the status and the text (without the entry point's name).
// Precedence: open row, duplicate row, probe overflow, step limit (rows_undecided counts on the wide family only),
// edge overflow or more edges than edge_cap.
int trans_status(TableFamily family, const TransCtr& tc, uint64_t edge_cap, std::string& text);
// The drained records sorted by (src, dst) into edges[got.size()] -> the sum of their sum_mu
uint64_t trans_finish_edges(std::vector<TransEdge>& got, bsx_trans_edge* edges);

}  // namespace bsx
