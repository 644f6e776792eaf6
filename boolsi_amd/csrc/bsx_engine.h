// Host-side internals shared by the translation units behind include/bsx.h (bsx_api.cpp, bsx_target_api.cpp,
// bsx_simulate_api.cpp, bsx_attract_api.cpp, bsx_cascade.cpp, bsx_fgraph_api.cpp, bsx_wide_api.cpp, bsx_wide_attract_api.cpp, bsx_wide_trans_api.cpp,
// bsx_sample_api.cpp, bsx_comm.cpp, and behind bsx_table_host.h the attractor-table calls): the engine handle, device
// buffers, error plumbing.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "bsx.h"
#include "bsx_device.h"
#include "bsx_knobs.h"
#include "bsx_model.h"

namespace bsx {

struct WideHost;        // bsx_wide_host.h

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t reserve(size_t count) { return n >= count ? hipSuccess : alloc(count); }     // grow-only scratch
    hipError_t upload(const std::vector<T>& v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// host copies of the arguments of bsx_set_network / bsx_set_problem_space (HostModel holds only the first table word)
struct SampleInputs {
    std::vector<uint32_t> pred_offsets, pred_idx, tt_word_offsets, any_nodes;
    std::vector<uint64_t> tt_words, origin;
    std::vector<bsx_fixed> fixed;
    std::vector<bsx_fixed_var> fixed_var;
    std::vector<bsx_pert> sched;
    std::vector<bsx_pert_var> pert_var;
};

}  // namespace bsx

struct bsx_engine {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop{};
    double wall_clock_khz = 1e5;        // device clock behind wall_clock64()
    std::string error;
    bsx::Knobs knobs;           // the environment as the current ABI call found it (bsx_knobs.h)

    // network
    bool have_net = false;
    uint32_t n_nodes = 0, w64 = 0;
    bsx::DevNet net{};
    int lut_mode = 0;           // kLutGlobal / kLutLdsByte / kLutLdsNibble (bsx_kernels_common.h)
    size_t shmem = 0;           // masks (+ LUT) : target / simulate kernels
    size_t shmem_attract = 0;   // + LDS mirror of the cycle-state cache

    // cycle-state cache (valid for the current network + origin fixed nodes)
    bool cache_enabled = true;
    int lean_blocks_per_cu = 0;  // occupancy of the lean attract kernel for the current network
    bool fast_ok = true;        // cleared when the lean kernel's straggler list overflowed for this space
    bool pool_ok = false;       // the class-pool kernel fits the LDS for this network
    size_t cache_stride = 0;    // bytes per slot of the LDS cache mirror
    std::vector<bsx::CycleRecord> h_journal;
    bool journal_stale = true;  // a general-kernel pass (the only writer of the journal) ran since h_journal was read
    uint32_t mirror_slots = 64;
    uint64_t journal_states = 0;    // cycle states of the journal records the lean / pool mirror takes
    bool cube_mirror = false;       // the next pool pass is a cube pass (mirror sized for representative entries)
    uint32_t fast_steps = 0;    // lean kernel: steps without a cached cycle state before a problem is handed over (0 = default)
    bool fast_calibrated = false;
    uint32_t cache_lds_slots = 0;
    bsx::DevBuf<bsx::CycleRecord> d_cc_journal;
    bsx::DevBuf<unsigned int> d_cc_claims;
    bsx::DevBuf<unsigned int> d_cc_count;

    // scratch kept across calls (grow-only): hipMalloc / hipFree per call cost ~1 ms of a 16 ms step
    bsx::DevBuf<bsx::LogRec> d_log;
    bsx::DevBuf<bsx::LogRec> d_table;   // HBM attractor table behind the log (all slots zero between calls)
    uint64_t table_slots = 0;
    bool table_dirty = false;
    bsx::DevBuf<uint32_t> d_strag;
    bsx::DevBuf<uint32_t> d_mirror;     // pool kernel: image of the LDS cache mirror, valid for (image_n journal records, image_slots slots)
    size_t image_n = ~size_t(0);
    uint32_t image_slots = 0;
    // deep cube passes, one set per side stream (the lower levels of up to kSideStreams chains run side by side):
    bsx::DevBuf<uint32_t> d_near_seg[bsx::kSideStreams];        // classes listed for the level below, one segment per workgroup,
    bsx::DevBuf<uint32_t> d_near_list[bsx::kSideStreams][2];    // and the packed lists, alternated by level (one is read, one written)
    hipStream_t side[bsx::kSideStreams] = {};
    hipStream_t top2 = nullptr;         // BSX_CUBE_TOP_STREAMS=2: the tops of a batch's odd chains (created on first use)
    hipEvent_t ev_top2 = nullptr;       // ... fork (behind the fill and the image) and join
    bsx::DevBuf<uint32_t> d_unres;      // cascade: unresolved classes per level (state, t, member count)
    bsx::DevBuf<bsx::LeafProgram> d_leaf;   // cascade: the depth-1 level's per-parent program (bsx_device.h)
    bsx::LeafProgram* h_leaf = nullptr;     // ... its pinned staging copy
    uint32_t life_cache[64] = {};       // cube passes: k_digit_lifetimes per digit, measured on the first block that needed it
    uint64_t life_valid = 0;            // (an ordering heuristic: later blocks of the problem reuse it)
    bsx::PlanState plan;                // cascade: what the planner has learned about this problem space (bsx_model.h)
    bsx::DevBuf<uint32_t> d_life;       // cube collapse: per-digit influence lifetimes (ordering heuristic)
    bsx::DevBuf<uint32_t> d_lut, d_masks, d_wide_desc, d_wide_preds, d_wide_tt;

    // host copies of the network and the space (filled by bsx_lane_lower.cpp): the cube planner's input, the sliced simulate kernel's node descriptors
    bsx::HostModel model;

    // problem space
    bool have_space = false;
    uint64_t variant_count = 1;         // product of the variation radices ...
    bool variant_count_saturated = false;   // ... unless it does not fit 64 bits
    uint32_t tp_max = 0;                // last perturbation time over origin schedule and variations
    bsx::DevSpace sp{};
    bsx::DevBuf<uint32_t> d_any, d_fv, d_pv, d_set, d_clr;

    // counters: one block for a single pass, one per level for a cube cascade, which is enqueued as a whole and read
    // back once.  The hand-over descriptors of the levels (level above -> next launch) sit right in front of block 0
    // so that one fill clears both.  h_ctr: pinned host buffer of the same shape; a cascade's last kernel (k_publish)
    // stores the blocks there and then the sequence number of the call into h_flag, which the host spins on -- the
    // wake-up of a blocking wait was a third of a 0.3 ms call.
    bsx::DevBuf<unsigned char> d_ctr_raw;
    bsx::LevelDesc* d_level = nullptr;      // [kMaxCubeLevels + 1]
    bsx::Counters* d_ctr = nullptr;         // [kMaxCubeLevels]
    bsx::Counters* h_ctr = nullptr;
    volatile uint32_t* h_flag = nullptr;    // (behind h_ctr in the same pinned allocation)
    uint32_t flag_seq = 0;
    hipEvent_t ev_top0 = nullptr, ev_top1 = nullptr;
    std::vector<bsx::Counters> ctr_seen;                // the counter blocks of the last batch of chains, as fetched
    std::vector<hipEvent_t> ev_chain;                   // pairs around the top-level (dominant) launch of every chain of a batch
    // independent launches of one call side by side (target's cube passes): auxiliary streams, one counter block per launch
    hipStream_t aux[8] = {};
    hipEvent_t aux_done[8] = {};
    bsx::DevBuf<bsx::Counters> d_ctr_multi;
    bsx::Counters* h_ctr_multi = nullptr;

    // functional-graph mode (bsx_fgraph.hip): N-sized arrays, kept between calls (grow-only)
    bsx::DevBuf<uint32_t> d_fg_a, d_fg_b, d_fg_c, d_fg_warm;
    bsx::DevBuf<unsigned long long> d_fg_pair;

    // wide-state family (bsx_wide_host.h, bsx_wide_*api.cpp): set when the network has more than BSX_MAX_NODES nodes or BSX_WIDE=1
    bsx::WideHost* wide = nullptr;
    // sampled calls on a handle of the <= BSX_MAX_NODES family (bsx_sample_api.cpp): what bsx_set_network and
    // bsx_set_problem_space received, and their second lowering onto the wide family, built on the first sampled call and
    // dropped by the next bsx_set_network / bsx_set_problem_space
    bsx::SampleInputs inputs;
    bsx::WideHost* sample_wide = nullptr;

    // RCCL communicator of this handle's rank (bsx_comm.cpp); librccl is loaded on first use
    void* comm = nullptr;       // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    bsx::DevBuf<unsigned char> d_comm_send, d_comm_recv;
};

#define HIPCHK(h, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (h)->error = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return BSX_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

namespace bsx {
void wide_release(bsx_handle h);
void wide_release_sample(bsx_handle h);
int wide_set_network(bsx_handle h, uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx,
                     const uint32_t* tt_word_offsets, const uint64_t* tt_words);
int wide_set_problem_space(bsx_handle h, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                           const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                           const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var);
int wide_run_simulate(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, uint64_t* trajectories,
                      uint64_t* final_states, uint64_t* digests, bsx_stats* stats);
int wide_run_trajectories(bsx_handle h, const bsx_index* first, const uint64_t* offsets, const uint64_t* t_len, uint64_t n,
                          uint64_t* out, const uint64_t* out_offsets, bsx_stats* stats);
int wide_run_target(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                    const uint64_t* code_words, bsx_hit* hits, uint64_t cap, uint64_t* n_hits, bsx_stats* stats, double t_begin);
int wide_run_target_summary(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                            const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                            uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats, double t_call);
}  // namespace bsx

static inline int fail(bsx_handle h, int status, const std::string& msg) {
    if (h) h->error = msg;
    return status;
}

