// Private to the host files of the wide-state family (bsx_wide_api.cpp: network, space, simulate, target;
// bsx_wide_attract_api.cpp: bsx_run_attract_wide; bsx_wide_trans_api.cpp: bsx_run_attractor_transitions_wide;
// bsx_profile_api.cpp: the wide half of the profile stage): the family's part of a handle, the kernel launch prototypes
// and the one launch setup they share.
#pragma once
#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_wide.h"
#include "bsx_wide_lower.h"

namespace bsx {

hipError_t launch_wide(int k, dim3 grid, size_t shmem, hipStream_t st, const WideParams& P);
hipError_t launch_wide_sampled(int k, dim3 grid, size_t shmem, hipStream_t st, const WideParams& P);
hipError_t launch_sample_problems(const WideSampleListParams& Q, hipStream_t st);
hipError_t launch_wide_profile(int k, dim3 grid, size_t shmem, hipStream_t st, const WideProfileParams& Q);
hipError_t launch_wide_damage(int k, dim3 grid, size_t shmem, hipStream_t st, const WideDamageParams& Q);
hipError_t launch_wide_influence(int k, dim3 grid, size_t shmem, hipStream_t st, const WideInfluenceParams& Q);
hipError_t launch_wide_trans(int k, dim3 grid, size_t shmem, hipStream_t st, const WideTransParams& Q);
hipError_t launch_wide_trans_build(const WideTransParams& Q, hipStream_t st);
hipError_t launch_wide_screen(int k, dim3 grid, size_t shmem, hipStream_t st, const WideScreenParams& Q);
hipError_t launch_screen_reduce(const uint32_t* info, const uint64_t* keys, uint64_t n_pairs, uint64_t p0, uint64_t g_per, uint64_t n_samples,
                                uint32_t G, uint32_t w64, ScreenSlot* table, uint64_t slots, unsigned long long* hdr, hipStream_t st);
hipError_t launch_screen_drain(const ScreenSlot* table, uint64_t slots, ScreenRec* out, uint64_t cap, unsigned long long* hdr,
                               const unsigned long long* ctr, hipStream_t st);
hipError_t launch_wide_reduce_attract(const uint32_t* info, const uint64_t* keys, uint64_t m, uint32_t w64, WideSlot* table,
                                      uint64_t slots, unsigned long long* hdr, hipStream_t st);
hipError_t launch_wide_reduce_drain(const WideSlot* table, uint64_t slots, WideAttrRec* out, uint64_t cap, unsigned long long* hdr,
                                    const unsigned long long* ctr, hipStream_t st);
hipError_t launch_wide_reduce_target(const uint32_t* t_hit, uint64_t m, unsigned long long* hist, uint32_t bins,
                                     unsigned long long* hdr, hipStream_t st);

struct WideHost {
    WideNet net;                // what bsx_wide_lower.cpp made of the network ...
    WideSpace space;            // ... and of the problem space (valid while have_space)
    bool have_space = false;
    DevBuf<uint32_t> d_desc, d_wdesc, d_wpreds, d_wtt, d_any, d_fv, d_pv, d_sched, d_x0;
    DevBuf<unsigned long long> d_ctr;
    // device-side reduction (bsx_wide_reduce.hip): grow-only, reused from call to call
    DevBuf<uint32_t> d_info, d_thit;
    DevBuf<uint64_t> d_keys;
    DevBuf<WideSlot> d_table;
    DevBuf<ScreenSlot> d_screen;                // the screen's table (bsx_screen_reduce.hip)
    DevBuf<unsigned long long> d_out, d_hist;   // d_out: kHdrWords header words, then the drained records
};

// The network part of a WideParams: layout, row descriptors, the tables of the nodes with more than 6 predecessors.
inline void wide_fill_net(const WideHost& W, WideParams& P) {
    const uint32_t rows = W.net.rows, L = W.space.L;
    P.n_nodes = W.net.n; P.rows = rows; P.L = L;
    P.lshift = (uint32_t)__builtin_ctz(L); P.w64 = W.net.w64;
    P.rows_ps = rows / (kWideThreads / L);
    P.desc = W.d_desc.p; P.wdesc = W.net.wdesc.empty() ? nullptr : W.d_wdesc.p; P.wpreds = W.d_wpreds.p; P.wtt = W.d_wtt.p;
    P.n_fslots = W.space.n_fslots;
}

// Workgroups of a launch over `count` trajectories with `shmem` bytes of LDS each.
inline uint64_t wide_blocks(const bsx_engine* h, const WideHost& W, uint64_t count, size_t shmem) {
    return wide_grid_blocks(count, W.space.L, shmem, (uint32_t)h->prop.multiProcessorCount);
}

// The end of a timed run of launches (the caller has zeroed d_ctr and recorded ev0 in front of it): records ev1, brings the
// four counters back (and `bytes` of a caller's own counter block with them), waits, reads the device time.
inline int wide_timed_wait(bsx_handle h, WideHost& W, unsigned long long (&ctr)[4], float& ms, void* also = nullptr, const void* d_also = nullptr,
                           size_t bytes = 0) {
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    if (bytes) HIPCHK(h, hipMemcpyAsync(also, d_also, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    return BSX_OK;
}

// Problems per k_wide launch of a chunked run: BSX_WIDE_CHUNK clamped to [32 * L, 2^18], else `dflt`.
inline uint64_t wide_chunk(const bsx_engine* h, const WideHost& W, uint64_t dflt) {
    if (!h->knobs.wide_chunk_set) return dflt;
    return std::max<uint64_t>(32ull * W.space.L, std::min<uint64_t>(h->knobs.wide_chunk, 1ull << 18));
}

// The helpers below take the WideHost they work on: a wide handle's own (h->wide), or the second lowering that the sampled
// calls keep on a handle of the <= BSX_MAX_NODES family (h->sample_wide, bsx_sample_api.cpp).

// bsx_wide_api.cpp: a network / a problem space lowered into W and uploaded (the arrays have passed the callers' checks)
int wide_upload_network(bsx_handle h, WideHost& W, uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx,
                        const uint32_t* tt_word_offsets, const uint64_t* tt_words);
int wide_upload_space(bsx_handle h, WideHost& W, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                      const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                      const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var);
// bsx_wide_api.cpp: one k_wide launch enqueued; one launch waited for; one launch over samples enqueued
int wide_enqueue(bsx_handle h, WideHost& W, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t);
int wide_launch(bsx_handle h, WideHost& W, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t,
                unsigned long long (&ctr)[4], float& ms);
// (the sampled launch carries the branch of P.mode; with `list` -- device memory, `count` sample numbers -- trajectory q is
// sample list[q]: simulate only)
int wide_enqueue_sampled(bsx_handle h, WideHost& W, WideParams& P, uint64_t k0, uint64_t first_sample, uint64_t count, uint64_t max_t,
                         const uint64_t* list = nullptr);
// An enumerating call on a space with more 'any' nodes than a bsx_index holds (only the sampled calls reach such a space).
// The calls that take a bsx_index are refused by check_range (bsx_host.h); this is the same refusal for the flat index
// of bsx_run_attract_wide, in front of its split.
inline int wide_check_enumerable(bsx_handle h, const WideHost& W) {
    if (W.space.n_any > 64 * BSX_MAX_WORDS)
        return fail(h, BSX_ERR_UNSUPPORTED, "more 'any' nodes than a bsx_index holds (64 * BSX_MAX_WORDS)");
    return BSX_OK;
}

// The source of a call's launches: it enqueues the launch over problems [done, done + m) of the call (consecutive indices,
// or samples of a seed); everything behind the launch is the same for both.
struct WideSource {
    virtual int enqueue(WideParams& P, uint64_t done, uint64_t m) = 0;
    virtual ~WideSource() = default;
};
// bsx_wide_api.cpp: simulate / trajectories as one launch of `src` (t_len / out_offsets: listed trajectories; offsets: their
// problems where the source enumerates), and the target summary's chain over its launches (bsx_run_target_summary on a wide
// network, bsx_run_target_sampled); the callers have checked the arguments and zeroed the outputs
int wide_sim(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t max_t, const uint64_t* offsets, const uint64_t* t_len,
             const uint64_t* out_offsets, uint64_t traj_words, uint64_t* trajectories, uint64_t* final_states, uint64_t* digests,
             bsx_stats* stats);
int wide_target_summary(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, const uint64_t* mask_words,
                        const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                        uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats, double t_call);
// bsx_sample_api.cpp: the WideHost a call over samples works on (bsx_damage_api.cpp takes it from there too)
int sample_host(bsx_handle h, WideHost** out);
// bsx_wide_attract_api.cpp: the two legs of an attract call over `count` problems in launches of `chunk`, behind
// bsx_run_attract_wide and bsx_run_attract_sampled.
int attract_wide_device(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t chunk, uint64_t max_len,
                        bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor, bsx_stats2* stats, double t_begin);
int attract_wide_host(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t chunk, uint64_t max_len,
                      bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor, bsx_stats2* stats, double t_begin);

}  // namespace bsx
