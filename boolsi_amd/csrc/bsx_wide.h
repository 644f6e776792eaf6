// Wide-state family (257 <= n <= BSX_MAX_NODES_WIDE, or any n with BSX_WIDE=1): kernel parameters shared by
// bsx_wide.hip, bsx_wide_lower.cpp and the host files behind bsx_wide_host.h.  See DESIGN.md "Wide networks".
//
// Bit-sliced like k_simulate_sliced: a group of 32 * L trajectories is a rows x L matrix of 32-bit words in LDS,
// row i = node i, column c = trajectories 32c .. 32c + 31, bit b of a word = trajectory 32c + b.  The 256 threads
// of a workgroup are (slice, column) pairs: column c = tid % L, slice s = tid / L owns the contiguous rows
// [s * rows_ps, (s + 1) * rows_ps).  A step costs the same per trajectory update whatever n is; L shrinks with n
// so that four such matrices fit the LDS.
#pragma once
#include <stdint.h>

namespace bsx {

constexpr uint32_t kWideThreads = 256;
constexpr uint32_t kWideMaxW32 = 32;            // 32-bit words of a state (n <= 1024)
constexpr uint32_t kWideNone = 0xFFFFFFFFu;
constexpr uint32_t kWideDescWords = 8;          // per row: preds (u16 x 6) in words 0..2, table bits 3..4, fixed slot 5, K>6 index 6
constexpr uint32_t kWideBuffers = 4;            // state matrices a workgroup holds in LDS
// Internal step limit, in lock steps of a group (BSX_ERR_STEP_LIMIT beyond it).  A lock step costs microseconds, not
// one lane's nanoseconds, so this is 2^24 rather than the per-lane kernels' 2^30: a chaotic network with max_t = inf
// gives up after minutes.  (BSX_WIDE_STEP_LIMIT lowers it, for tests.)
constexpr uint32_t kWideStepLimit = 1u << 24;

enum WideMode : uint32_t { kWideSimulate = 0, kWideTarget = 1, kWideAttract = 2 };

struct WideParams {
    uint32_t mode;
    uint32_t n_nodes, rows, L, lshift, rows_ps, w64, pad0;
    const uint32_t* desc;       // [rows][8]
    const uint32_t* wdesc;      // per node with more than 6 predecessors: k, first pred, first table word (u32 words); null: none
    const uint32_t* wpreds;
    const uint32_t* wtt;
    // problem space (bsx_index first + offset, batching.py:212-229)
    uint64_t first_digits[4];
    uint64_t first_variant;
    uint32_t origin[kWideMaxW32];   // origin state ('any' nodes cleared)
    uint32_t tmask[kWideMaxW32];    // target substate (target mode)
    uint32_t tcode[kWideMaxW32];
    uint32_t n_any, n_fv, n_pv, n_sched, n_fslots, tp_origin;
    const uint32_t* any_nodes;  // [n_any]
    const uint32_t* fv;         // [n_fv][3] node, range, fixed slot
    const uint32_t* pv;         // [n_pv][3] t, node, range
    const uint32_t* sched;      // [n_sched][3] t, node, value, sorted by t
    uint64_t count;
    uint64_t max_t;
    uint32_t cap_inf;           // max_t is BSX_T_INF
    uint32_t step_limit;        // kWideStepLimit (or BSX_WIDE_STEP_LIMIT)
    // simulate / trajectories
    const uint64_t* offsets;    // nullable: problem q = first + offsets[q]
    const uint64_t* t_len;      // nullable: per-problem length (else max_t)
    const uint64_t* out_offsets;
    uint64_t* traj;
    uint64_t* final_states;
    uint64_t* digests;
    // target: first hit time per problem, kWideNone = none
    uint32_t* t_hit;
    // attract: per problem (found-and-kept, lambda, trajectory_l lo, hi) and the key
    uint32_t* info;
    uint64_t* keys;
    uint64_t max_len;
    uint32_t* x0;               // scratch: [gridDim.x][rows * L] s(T_p) of the group
    unsigned long long* ctr;    // [0] reference steps, [1] executed trajectory updates, [2] step-limit hits
    // sampled source (the k_wide<K, KW, true, ...> instantiations only; behind every field the other kernels read, so that
    // their offsets stay)
    uint64_t sample_k0;         // sample_k0(seed)
    uint64_t sample_first;      // first sample of this launch
    uint64_t sample_variants;   // V, the space's variant count (not saturated)
    const uint64_t* sample_list;    // nullable, k_wide<K, KW, true, kWideSimulate> only: trajectory q is sample sample_list[q]
};

// ---- sampled problem source (k_wide<K, KW, true, MODE> / k_sample_problems in bsx_wide.hip, bsx_sample.h has the
// definition) ----
// k_wide<K, KW, true> is k_wide's attract branch over samples [sample_first, sample_first + count) of a seed: trajectory k
// of a group is sample sample_first + base + k.  Only a group's set-up differs (s(0) and the variant number come from the
// generator, word by word, not from a decoded index); first_digits / first_variant / offsets are not read.
// k_wide<K, KW, true, MODE> is the target or the simulate branch behind the same set-up; each sampled instantiation
// carries the one branch of its mode.  With sample_list the simulate instantiation sets a group up per trajectory
// (sample sample_list[base + k], with t_len / out_offsets of its own): lists are short, and that path is not tuned.
// k_sample_problems: s(0) and the variant number of listed samples, one thread per sample
struct WideSampleListParams {
    uint32_t n_nodes, w64, n_any, pad;
    uint32_t origin[kWideMaxW32];   // origin state ('any' nodes cleared)
    const uint32_t* any_nodes;      // [n_any]
    uint64_t k0, variant_count;
    const uint64_t* samples;        // [n]
    uint64_t n;
    uint64_t* states;               // [n][w64]
    uint64_t* variants;             // nullable: [n]
};

// ---- attractor profile (k_wide_profile in bsx_wide.hip, bsx_run_attractor_profile) ----
// A group of 32 * L attractors walks in lock step from its key states, bit b live while t < length_b and frozen after
// (so the matrix ends at f^length(key) for every bit); `net` carries the network part of WideParams (layout, row
// descriptors, n_fslots) and nothing of a problem space: origin fixed nodes are constant rules in the descriptors.
// Rows a thread owns: rows * L / kWideThreads, at most 36 for the L that wide_lds_words admits.
constexpr uint32_t kWideProfileRows = 36;
struct WideProfileParams {
    WideParams net;
    uint64_t count;
    uint32_t key_stride;            // uint64 words per row of `keys` (>= w64)
    uint32_t pad;
    const uint64_t* keys;           // [count][key_stride]
    const uint64_t* lengths;        // [count], checked by the host
    const uint64_t* state_offsets;  // [count] (with `states`)
    uint32_t* on_counts;            // nullable: [count][n_nodes], zeroed by the host
    uint64_t* states;               // nullable
    uint8_t* closed;                // nullable: [count]
    unsigned long long* ctr;        // [1] executed trajectory updates
};
// LDS words of k_wide_profile: two matrices, the (zero) fixed-variation masks, partials, live masks, lengths.
inline uint32_t wide_profile_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots) {
    return 2 * rows * L + 2 * n_fslots * L + kWideThreads + 2 * L + 32 * L + 8;
}

// ---- damage spreading (k_wide_damage in bsx_wide.hip, bsx_run_damage_sampled; include/bsx.h has the definition) ----
// A group of 32 * L samples holds two trajectories per sample: X (matrices 0 / 1) from the sampled source, Y (matrices
// 2 / 3) = X with n_flips free nodes inverted.  Both step under the network part of `net` (origin fixed nodes are constant
// rules; the space has no variations and no schedule, the host refuses the others).  d(t) of a sample is the column sum of
// X ^ Y over all rows: 6-plane vertical counters over the rows a thread owns, combined across the slices through LDS.
constexpr uint32_t kWideDamagePlanes = 6;       // rows a thread owns: at most kWideProfileRows = 36 < 2^6
struct WideDamageParams {
    WideParams net;                 // network part, origin, any_nodes / n_any, sample_k0, sample_first, count
    uint32_t n_flips, n_steps;
    uint32_t n_free, acc_lds;       // acc_lds: the (n_steps + 1) * 3 sums of a workgroup stay in LDS until it ends
    const uint32_t* free_nodes;     // [n_free] ascending
    unsigned long long* sums;       // [n_steps + 1][3] sum d, sum d^2, merged; zeroed by the host
    unsigned long long* hist;       // nullable: [n_steps + 1][n_nodes + 1], zeroed by the host
};
// LDS words of k_wide_damage: four matrices, the (zero) fixed-variation masks, the planes of every thread, the block keys
// of the columns, the sums of a step, the step's histogram (with hist) and the 64-bit accumulators (with acc_lds).
inline uint32_t wide_damage_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots, uint32_t n_nodes, bool hist, uint32_t acc_steps) {
    return kWideBuffers * rows * L + 2 * n_fslots * L + kWideDamagePlanes * kWideThreads + 4 * L + 8 + (hist ? ((n_nodes + 2) & ~1u) : 0) +
           6 * acc_steps;
}

// ---- node influence (k_wide_influence in bsx_wide.hip, bsx_run_influence_sampled; include/bsx.h has the definition,
// bsx_influence.h the layout) ----
// The work items of a launch are (source, group) pairs p = p0 + i, i < n_items: group p % g_per of source p / g_per, its
// samples first_sample + 32 L * group + k of the sampled source.  X (matrices 0 / 1) and Y (matrices 2 / 3) as in damage,
// Y = X with row sources[source] inverted under the columns' valid-bits masks.  After a lock step the count of row i is the
// popcount of X[i] ^ Y[i] over the L columns: one LDS counter per row, touched only for a nonzero word, and flushed with
// one 32-bit global add per nonzero (source, t, row).  `net` carries the network part, origin, any_nodes /
// n_any, sample_k0 and ctr; the space has no variations and no schedule (the host refuses the others).
struct WideInfluenceParams {
    WideParams net;
    uint64_t first_sample, n_samples;
    uint64_t p0, n_items, g_per;
    uint32_t n_steps, pad;
    const uint32_t* sources;        // [n_sources]
    uint32_t* influence;            // [n_sources][n_steps][n_nodes], zeroed by the host
    unsigned long long* n_merged;   // nullable: [n_sources][n_steps], zeroed by the host
};
// LDS words of k_wide_influence: four matrices, the (zero) fixed-variation masks, the row counters and the per-column ORs
// of a step (both in two halves, by the step's parity), the block keys of the columns.
inline uint32_t wide_influence_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots) {
    return kWideBuffers * rows * L + 2 * n_fslots * L + 2 * rows + 2 * L + 4 * L + 8;
}

// ---- attractor transitions (k_wide_trans / k_wide_trans_build in bsx_wide.hip, bsx_run_attractor_transitions_wide) ----
// A group of 32 * L trajectories runs k_wide's attract phases (Brent in lock step, the mu pass, the key lap) with
// T_p = 0 and the origin's fixed nodes only.  Two kinds of source:
//   rows   trajectory k starts at the key of row first + k (rows whose profile `closed` flag is 0 are not walked);
//          per row the true period, mu and the canonical key (the cycle's minimum state) are written;
//   flips  flip f = first + k is (listed state f / n_free, free node f % n_free): that state with one bit inverted;
//          the flip's canonical key is looked up in the table of the rows' keys (bsx_wtrans.h) and the edge
//          accumulated, per group in LDS first and then in the HBM edge table of bsx_trans.h.
// `net` carries the network part of WideParams and max_t / cap_inf / step_limit / x0; nothing of a problem space.
struct TransEdgeSlot;
struct TransCtr;
enum WideTransStage : uint32_t { kWideTransRows = 0, kWideTransFlips = 1 };
struct WideTransParams {
    WideParams net;
    uint32_t stage;
    uint32_t key_stride;            // uint64 words per row of `keys` (>= w64)
    uint64_t first, count;          // this launch: rows / flips [first, first + count)
    uint64_t n_rows;
    const uint64_t* keys;           // [n_rows][key_stride]
    const uint64_t* lengths;        // [n_rows]
    const uint8_t* closed;          // [n_rows], from the profile
    const uint64_t* states;         // [sum of the lengths][w64], row after row, from the profile
    const uint64_t* row_first;      // [n_rows] index of a row's first state
    const uint32_t* free_nodes;     // [n_free] ascending
    uint32_t n_free, pad;
    uint32_t* row_info;             // [n_rows][2] true period (0: not walked or undecided), mu
    uint64_t* row_keys;             // [n_rows][w64] canonical keys
    uint32_t* owners;               // row-key table: [slot_mask + 1], row + 1, 0 = free
    uint64_t slot_mask;
    TransEdgeSlot* edges;           // HBM edge table
    uint64_t edge_mask;             // its slots - 1
    uint32_t* node_exits;           // nullable: [n_rows][n_nodes]
    TransCtr* ctr;
};
// LDS words of k_wide_trans: k_wide's layout without perturbation variations (never more than wide_lds_words gives
// for the L that wide_lower_space chose); the group's edge table lies in the first matrix, dead by then.
inline uint32_t wide_trans_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots) {
    return kWideBuffers * rows * L + 2 * n_fslots * L + 2 * kWideThreads + 8 * L + 4 * 32 * L + 8;
}

// ---- mutant screens over samples (k_wide_screen in bsx_wide.hip, bsx_run_screen_sampled; include/bsx.h has the
// definition, bsx_screen.h the layout) ----
// The work items of a launch are (mutant, group) pairs p = p0 + i, i < n_pairs: group p % g_per of mutant p / g_per, its
// trajectories the samples first_sample + 32 L * group + k of the sampled source.  A workgroup runs k_wide's attract
// phases with T_p = 0 (as k_wide_trans) and, after every step, rewrites the rows of its mutant's nodes under the step's
// freeze mask.  Record (i * 32 L + k) of the launch goes to info / keys of `net`; records behind the end of a ragged
// group are not written (the reduction knows a record's pair, and so its validity, from its position).
// `net` carries the network part, origin, any_nodes / n_any, sample_k0, max_t / cap_inf / step_limit, max_len, info /
// keys, x0 and ctr; the space has no variations and no schedule (the host refuses the others).
struct WideScreenParams {
    WideParams net;
    uint64_t first_sample, n_samples;
    uint64_t p0, n_pairs, g_per;
    const uint32_t* mut_offsets;    // [n_mutants + 1]
    const uint32_t* mut_nodes;      // [mut_offsets[n_mutants]][2] node, value (bsx_fixed)
};
// LDS words of k_wide_screen: k_wide's layout without perturbation variations and without T_p (never more than
// wide_lds_words gives for the L that wide_lower_space chose)
inline uint32_t wide_screen_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots) {
    return kWideBuffers * rows * L + 2 * n_fslots * L + 2 * kWideThreads + 8 * L + 3 * 32 * L + 8;
}

// ---- device-side reduction of the kernel's per-problem records (bsx_wide_reduce.hip) ----
// Attract: an open-addressing HBM table keyed by the whole w64-word key, linear probing.
// Widths of the sums, for at most 2^64 - 1 problems per call (bsx_run_attract_wide refuses more) and
// l = T_p + mu < 2^33:  count < 2^64 (1 word),  sum l < 2^97 (2 words),  sum l^2 < 2^130 (3 words).  The adds carry
// across the words, so no field wraps and the result equals sums taken in unbounded integers.
struct WideSlot {
    uint32_t state;             // 0 empty, 1 key being written, 2 ready
    uint32_t length;
    unsigned long long count;
    unsigned long long sum_l[2];
    unsigned long long sum_l2[3];
    unsigned long long key[kWideMaxW32 / 2];    // words past w64 stay 0
};
// A drained record: the layout of bsx_attr_rec2w (include/bsx.h).
struct WideAttrRec {
    uint64_t key[kWideMaxW32 / 2];
    uint64_t length;
    uint64_t count[2];
    uint64_t sum_l[3];
    uint64_t sum_l2[4];
};
// Header words in front of the drained records; one device-to-host copy brings header and records back.
enum WideHdr : uint32_t {
    kHdrNone = 0,               // records without an attractor
    kHdrCursor = 1,             // ready slots seen by the drain (may exceed the capacity it packs)
    kHdrOverflow = 2,           // bit 0: table full (a probe went round all slots), bit 1: a bounded spin gave up
    kHdrHits = 3,               // target: problems that hit
    kHdrCtr = 4,                // copy of WideParams::ctr[0..3]
    kHdrWords = 8
};
constexpr uint32_t kWideReduceTile = 1024;      // records a workgroup of k_wide_reduce_attract combines in LDS
constexpr uint32_t kWideReduceLdsSlots = 128;   // entries of that LDS table
constexpr uint32_t kWideReduceMinSlots = 1024;  // smallest HBM table
// Largest min(cap, count) reduced on the device: 2^21 slots of 184 bytes and 2^20 records of 208 bytes, 0.6 GB.
constexpr uint64_t kWideReduceMaxCap = 1ull << 20;
// The screen's table slot and drained record (bsx_screen_reduce.hip): WideSlot / WideAttrRec with the mutant in the key.
struct ScreenSlot {
    uint32_t state;             // 0 empty, 1 key being written, 2 ready
    uint32_t length;
    unsigned long long mutant;
    unsigned long long count;
    unsigned long long sum_l[2];
    unsigned long long sum_l2[3];
    unsigned long long key[kWideMaxW32 / 2];    // words past w64 stay 0
};
struct ScreenRec {              // the layout of bsx_screen_rec (include/bsx.h)
    uint64_t mutant;
    WideAttrRec rec;
};
constexpr uint32_t kScreenInlineRecs = 256;     // records that come back with the header in the call's one copy

// LDS words of a workgroup for L columns (bsx_wide.hip lays them out in this order).
inline uint32_t wide_lds_words(uint32_t rows, uint32_t L, uint32_t n_fslots, uint32_t n_pv) {
    return kWideBuffers * rows * L + 2 * (n_fslots + n_pv) * L + 2 * kWideThreads + 8 * L + 4 * 32 * L + 8;
}

}  // namespace bsx
