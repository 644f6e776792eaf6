// Host side of the wide-state family (bsx_wide.hip): upload of what bsx_wide_lower.cpp makes of a network of up to
// BSX_MAX_NODES_WIDE nodes and its problem space, and the run entry points of include/bsx.h for such networks --
// simulate, trajectories, target.  (Attract: bsx_wide_attract_api.cpp; profile: bsx_profile_api.cpp; transitions:
// bsx_wide_trans_api.cpp.)
// bsx_api.cpp hands a handle over here when its network has more than BSX_MAX_NODES nodes (or BSX_WIDE=1).
#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_wide_host.h"

namespace bsx {

void wide_release(bsx_handle h) {
    delete h->wide;
    h->wide = nullptr;
}

// The second lowering of a handle of the <= BSX_MAX_NODES family (bsx_sample_api.cpp builds it on the first sampled call)
void wide_release_sample(bsx_handle h) {
    delete h->sample_wide;
    h->sample_wide = nullptr;
}

int wide_upload_network(bsx_handle h, WideHost& W, uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx,
                        const uint32_t* tt_word_offsets, const uint64_t* tt_words) {
    wide_lower_network(n_nodes, pred_offsets, pred_idx, tt_word_offsets, tt_words, W.net);
    HIPCHK(h, W.d_wdesc.upload(W.net.wdesc));
    HIPCHK(h, W.d_wpreds.upload(W.net.wpreds));
    HIPCHK(h, W.d_wtt.upload(W.net.wtt));
    HIPCHK(h, W.d_ctr.alloc(4));
    W.have_space = false;
    return BSX_OK;
}

int wide_upload_space(bsx_handle h, WideHost& W, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                      const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                      const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var) {
    W.have_space = false;
    WideSpace& S = W.space;
    if (const LowerStatus s = wide_lower_space(W.net, origin_state_words, any_nodes, n_any, fixed, n_fixed, fixed_var, n_fixed_var,
                                               sched, n_sched, pert_var, n_pert_var, S))
        return fail(h, s.status, s.msg);
    HIPCHK(h, W.d_desc.upload(S.desc));
    HIPCHK(h, W.d_any.upload(S.any));
    HIPCHK(h, W.d_fv.upload(S.fv));
    HIPCHK(h, W.d_pv.upload(S.pv));
    HIPCHK(h, W.d_sched.upload(S.sched));
    W.have_space = true;
    return BSX_OK;
}

int wide_set_network(bsx_handle h, uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx,
                     const uint32_t* tt_word_offsets, const uint64_t* tt_words) {
    if (const LowerStatus s = wide_check_size(n_nodes)) return fail(h, s.status, s.msg);
    HIPCHK(h, hipSetDevice(h->device));
    h->have_net = h->have_space = false;
    if (const LowerStatus s = check_network_arrays(n_nodes, pred_offsets, pred_idx, tt_word_offsets)) return fail(h, s.status, s.msg);
    if (!h->wide) h->wide = new WideHost();
    WideHost& W = *h->wide;
    if (int rc = wide_upload_network(h, W, n_nodes, pred_offsets, pred_idx, tt_word_offsets, tt_words)) return rc;
    h->n_nodes = n_nodes; h->w64 = W.net.w64;
    h->net = DevNet{};
    h->net.n_nodes = n_nodes; h->net.nw = (n_nodes + 31) / 32; h->net.k_mux = W.net.K;
    h->lut_mode = BSX_LUT_WIDE;
    h->have_net = true;
    return BSX_OK;
}

int wide_set_problem_space(bsx_handle h, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                           const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                           const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var) {
    WideHost& W = *h->wide;
    // (up to n 'any' nodes: a space with more than a bsx_index holds, 64 * BSX_MAX_WORDS, is reached by the sampled calls
    // alone; the enumerating calls refuse it: check_range of bsx_host.h, wide_check_enumerable)
    HIPCHK(h, hipSetDevice(h->device));
    h->have_space = false;
    if (int rc = wide_upload_space(h, W, origin_state_words, any_nodes, n_any, fixed, n_fixed, fixed_var, n_fixed_var, sched, n_sched,
                                   pert_var, n_pert_var))
        return rc;
    const WideSpace& S = W.space;
    // the fields of the handle that the range checks of bsx_host.h read
    h->sp = DevSpace{};
    h->sp.n_any = n_any;
    h->variant_count_saturated = S.variant_count_saturated; h->variant_count = S.variant_count; h->tp_max = S.tp_max;
    h->have_space = true;
    return BSX_OK;
}

// Everything of a k_wide launch over `count` problems but their source: network, space, caps, counters, the attract scratch.
// -> the launch's workgroups in *blocks_out.
static int wide_fill_launch(bsx_handle h, WideHost& W, WideParams& P, uint64_t count, uint64_t max_t, uint64_t* blocks_out) {
    const WideSpace& S = W.space;
    wide_fill_net(W, P);
    std::memcpy(P.origin, S.origin, sizeof(P.origin));
    P.n_any = S.n_any; P.n_fv = S.n_fv; P.n_pv = S.n_pv; P.n_sched = S.n_sched;
    P.tp_origin = S.tp_origin;
    P.any_nodes = W.d_any.p; P.fv = W.d_fv.p; P.pv = W.d_pv.p; P.sched = W.d_sched.p;
    P.count = count;
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;        // kWideStepLimit unless BSX_WIDE_STEP_LIMIT says less
    P.ctr = W.d_ctr.p;
    const uint64_t blocks = wide_blocks(h, W, count, S.shmem);
    if (P.mode == kWideAttract) {
        // (grow-only: a chunked run's first launch is its largest, so the buffer never moves under a queued launch)
        HIPCHK(h, W.d_x0.reserve((size_t)blocks * W.net.rows * S.L));
        P.x0 = W.d_x0.p;
    }
    *blocks_out = blocks;
    return BSX_OK;
}

// Enqueues one k_wide launch over [first, first + count) (count problems, or the listed offsets) on the engine's
// stream and returns without waiting; the caller fills the parameter fields of the mode's sinks before.  The kernel
// ADDS to the counters in W.d_ctr: the caller zeroes them once, in front of its first launch.
int wide_enqueue(bsx_handle h, WideHost& W, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t) {
    uint64_t blocks = 0;
    if (int rc = wide_fill_launch(h, W, P, count, max_t, &blocks)) return rc;
    for (int w = 0; w < 4; ++w) P.first_digits[w] = first->init_digits[w];
    P.first_variant = first->variant;
    HIPCHK(h, launch_wide((int)W.net.K, dim3((uint32_t)blocks), W.space.shmem, h->stream, P));
    return BSX_OK;
}

// The same over samples [first_sample, first_sample + count) of the seed behind k0, or over the `count` listed ones
// (bsx_sample.h); the kernel is the sampled instantiation of P.mode
int wide_enqueue_sampled(bsx_handle h, WideHost& W, WideParams& P, uint64_t k0, uint64_t first_sample, uint64_t count, uint64_t max_t,
                         const uint64_t* list) {
    uint64_t blocks = 0;
    if (list && P.mode != kWideSimulate) return fail(h, BSX_ERR_INVALID, "listed samples are a source of simulate launches only");
    if (int rc = wide_fill_launch(h, W, P, count, max_t, &blocks)) return rc;
    P.sample_k0 = k0;
    P.sample_first = first_sample;
    P.sample_variants = W.space.variant_count;
    P.sample_list = list;
    HIPCHK(h, launch_wide_sampled((int)W.net.K, dim3((uint32_t)blocks), W.space.shmem, h->stream, P));
    return BSX_OK;
}

// One launch, waited for: its counters and its device time.
int wide_launch(bsx_handle h, WideHost& W, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t,
                unsigned long long (&ctr)[4], float& ms) {
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = wide_enqueue(h, W, P, first, count, max_t)) return rc;
    return wide_timed_wait(h, W, ctr, ms);
}

namespace {

// consecutive problem indices from `first` (the enumerating calls)
struct IndexRange : WideSource {
    bsx_handle h; WideHost& W; const bsx_index* first; uint64_t max_t;
    IndexRange(bsx_handle h_, WideHost& W_, const bsx_index* f, uint64_t t) : h(h_), W(W_), first(f), max_t(t) {}
    int enqueue(WideParams& P, uint64_t done, uint64_t m) override {
        const bsx_index at = index_plus(*first, done, h->sp.n_any);
        return wide_enqueue(h, W, P, &at, m, max_t);
    }
};

}  // namespace

// simulate / trajectories over the `count` problems of one launch of `src` (listed: with offsets, lengths and places of
// their own; `offsets` is null where the source has its own list)
int wide_sim(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t max_t, const uint64_t* offsets, const uint64_t* t_len,
             const uint64_t* out_offsets, uint64_t traj_words, uint64_t* trajectories, uint64_t* final_states, uint64_t* digests,
             bsx_stats* stats) {
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (max_t >= kStepLimit) return fail(h, BSX_ERR_UNSUPPORTED, "simulation length above the engine's step limit");
    HIPCHK(h, hipSetDevice(h->device));
    const uint32_t w64 = W.net.w64;
    DevBuf<uint64_t> d_traj, d_final, d_dig, d_off, d_tlen, d_ooff;
    WideParams P{};
    P.mode = kWideSimulate;
    if (trajectories) { HIPCHK(h, d_traj.alloc(traj_words)); P.traj = d_traj.p; }
    // scattered trajectories: the whole buffer comes back in one copy, so the words between them make the round trip
    // (a caller's buffer keeps what no trajectory covers, as in bsx_simulate_api.cpp)
    if (trajectories && out_offsets) HIPCHK(h, hipMemcpy(d_traj.p, trajectories, traj_words * 8, hipMemcpyHostToDevice));
    if (final_states) { HIPCHK(h, d_final.alloc(count * w64)); P.final_states = d_final.p; }
    if (digests) { HIPCHK(h, d_dig.alloc(count)); P.digests = d_dig.p; }
    if (offsets) { HIPCHK(h, d_off.upload(std::vector<uint64_t>(offsets, offsets + count))); P.offsets = d_off.p; }
    if (t_len) {
        HIPCHK(h, d_tlen.upload(std::vector<uint64_t>(t_len, t_len + count))); P.t_len = d_tlen.p;
        HIPCHK(h, d_ooff.upload(std::vector<uint64_t>(out_offsets, out_offsets + count))); P.out_offsets = d_ooff.p;
    }
    unsigned long long ctr[4];
    float ms = 0.f;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = src.enqueue(P, 0, count)) return rc;
    if (int rc = wide_timed_wait(h, W, ctr, ms)) return rc;
    if (trajectories) HIPCHK(h, hipMemcpy(trajectories, d_traj.p, traj_words * 8, hipMemcpyDeviceToHost));
    if (final_states) HIPCHK(h, hipMemcpy(final_states, d_final.p, count * w64 * 8, hipMemcpyDeviceToHost));
    if (digests) HIPCHK(h, hipMemcpy(digests, d_dig.p, count * 8, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr[0], ctr[1], ms, 1, t_begin);
    return BSX_OK;
}

int wide_run_simulate(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, uint64_t* trajectories,
                      uint64_t* final_states, uint64_t* digests, bsx_stats* stats) {
    IndexRange src(h, *h->wide, first, max_t);
    return wide_sim(h, *h->wide, src, count, max_t, nullptr, nullptr, nullptr, trajectories ? count * (max_t + 1) * h->w64 : 0,
                    trajectories, final_states, digests, stats);
}

int wide_run_trajectories(bsx_handle h, const bsx_index* first, const uint64_t* offsets, const uint64_t* t_len, uint64_t n,
                          uint64_t* out, const uint64_t* out_offsets, bsx_stats* stats) {
    uint64_t words = 0, tmax = 0;
    for (uint64_t q = 0; q < n; ++q) {
        words = std::max(words, out_offsets[q] + (t_len[q] + 1) * h->w64);
        tmax = std::max(tmax, t_len[q]);
    }
    IndexRange src(h, *h->wide, first, tmax);
    return wide_sim(h, *h->wide, src, n, tmax, offsets, t_len, out_offsets, words, out, nullptr, nullptr, stats);
}

// target: first hit time per problem of one launch of `src` over [done, done + count) into t_hit (kWideNone = none)
static int wide_target_times(bsx_handle h, WideHost& W, WideSource& src, uint64_t done, uint64_t count, const uint64_t* mask_words,
                             const uint64_t* code_words, std::vector<uint32_t>& t_hit, bsx_stats* stats) {
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    t_hit.assign(count, kWideNone);
    if (count == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    WideParams P{};
    P.mode = kWideTarget;
    wide_target_words(W.net.n, mask_words, code_words, P.tmask, P.tcode);
    DevBuf<uint32_t> d_thit;
    HIPCHK(h, d_thit.alloc(count));
    HIPCHK(h, hipMemset(d_thit.p, 0xFF, count * 4));
    P.t_hit = d_thit.p;
    unsigned long long ctr[4];
    float ms = 0.f;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = src.enqueue(P, done, count)) return rc;
    if (int rc = wide_timed_wait(h, W, ctr, ms)) return rc;
    HIPCHK(h, hipMemcpy(t_hit.data(), d_thit.p, count * 4, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr[0], ctr[1], ms, 1, t_begin);
    if (ctr[2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    return BSX_OK;
}

// bsx_run_target, and the summary calls under BSX_WIDE_HOST_REDUCE=1 (the caller has checked the arguments and zeroed the
// outputs; count > 0): the per-problem first-hit times come to the host in chunks of 2^24 problems (not BSX_WIDE_CHUNK)
// and are counted, binned and listed here.  list_all: a hit beyond `cap` is an error.  The caller's arrays are written
// only when the whole call succeeds.
static int wide_target_host(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, const uint64_t* mask_words,
                            const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap, bool list_all,
                            uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats, double t_begin) {
    uint64_t total = 0, listed = 0;
    bsx_stats part{};
    if (stats) stats->problems = count;
    std::vector<uint64_t> bins(hist_bins, 0);
    std::vector<bsx_hit> list;
    for (uint64_t done = 0; done < count; done += 1ull << 24) {
        const uint64_t m = std::min<uint64_t>(1ull << 24, count - done);
        std::vector<uint32_t> t_hit;
        if (int rc = wide_target_times(h, W, src, done, m, mask_words, code_words, t_hit, &part)) return rc;
        for (uint64_t p = 0; p < m; ++p) {
            if (t_hit[p] == kWideNone) continue;
            ++total;
            if (hist_bins) ++bins[std::min<uint64_t>(t_hit[p], hist_bins - 1)];
            if (listed < cap) { list.push_back(bsx_hit{done + p, t_hit[p]}); ++listed; }
            else if (list_all) return fail(h, BSX_ERR_TABLE_FULL, "more hits than the caller's capacity (bsx_run_target_summary counts without listing)");
        }
        if (stats) {
            stats->state_steps += part.state_steps; stats->executed_steps += part.executed_steps;
            stats->kernel_ms += part.kernel_ms; stats->kernel_launches += part.kernel_launches;
        }
    }
    for (uint32_t b = 0; b < hist_bins; ++b) hist[b] = bins[b];
    std::copy(list.begin(), list.end(), hits);
    *n_hits = total;
    if (n_listed) *n_listed = listed;
    if (stats) stats->total_ms = now_ms() - t_begin;
    return BSX_OK;
}

int wide_run_target(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                    const uint64_t* code_words, bsx_hit* hits, uint64_t cap, uint64_t* n_hits, bsx_stats* stats, double t_begin) {
    IndexRange src(h, *h->wide, first, max_t);
    return wide_target_host(h, *h->wide, src, count, mask_words, code_words, nullptr, 0, hits, cap, true, n_hits, nullptr, stats, t_begin);
}

// bsx_run_target_summary on a wide network and bsx_run_target_sampled (the caller has checked the arguments and zeroed the
// outputs; count > 0), over the launches of `src`.  On the device: k_wide_reduce_target counts and bins every chunk's t_hit
// right behind the k_wide launch that wrote it.  A chunk's t_hit is copied to the host only while the caller's hit list
// has room; with cap == 0, or once the list is full, the host waits once, at the end.  Chunks are 2^24 problems, or
// BSX_WIDE_CHUNK.
int wide_target_summary(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, const uint64_t* mask_words,
                        const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                        uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats, double t_call) {
    if (h->knobs.wide_host_reduce)
        return wide_target_host(h, W, src, count, mask_words, code_words, hist, hist_bins, hits, cap, false, n_hits, n_listed, stats, t_call);
    const double t_begin = now_ms();
    WideParams P0{};
    P0.mode = kWideTarget;
    wide_target_words(W.net.n, mask_words, code_words, P0.tmask, P0.tcode);
    const uint64_t chunk = std::min<uint64_t>(count, wide_chunk(h, W, 1ull << 24));
    const uint32_t bins_alloc = std::max<uint32_t>(hist_bins, 1);
    HIPCHK(h, W.d_thit.reserve(chunk));
    HIPCHK(h, W.d_hist.reserve(bins_alloc));
    HIPCHK(h, W.d_out.reserve(kHdrWords));
    HIPCHK(h, hipMemsetAsync(W.d_hist.p, 0, bins_alloc * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(W.d_out.p, 0, kHdrWords * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    uint64_t listed = 0;
    uint32_t launches = 0;
    double kms = 0;
    bool timing = false;        // ev0 recorded, ev1 not yet: a run of launches the host has not waited for
    std::vector<uint32_t> t_hit;
    std::vector<bsx_hit> list;      // handed to the caller only when the call succeeds
    auto wait = [&]() -> int {
        float ms = 0.f;
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        kms += ms;
        timing = false;
        return BSX_OK;
    };
    for (uint64_t done = 0; done < count; done += chunk) {
        const uint64_t m = std::min(chunk, count - done);
        HIPCHK(h, hipMemsetAsync(W.d_thit.p, 0xFF, m * 4, h->stream));
        if (!timing) { HIPCHK(h, hipEventRecord(h->ev0, h->stream)); timing = true; }
        WideParams P = P0;
        P.t_hit = W.d_thit.p;
        if (int rc = src.enqueue(P, done, m)) return rc;
        HIPCHK(h, launch_wide_reduce_target(W.d_thit.p, m, W.d_hist.p, hist_bins, W.d_out.p, h->stream));
        launches += 2;
        if (listed < cap) {                     // the list still has room: this chunk's hit times, in index order
            if (int rc = wait()) return rc;
            t_hit.resize(m);
            HIPCHK(h, hipMemcpy(t_hit.data(), W.d_thit.p, m * 4, hipMemcpyDeviceToHost));
            for (uint64_t p = 0; p < m && listed < cap; ++p)
                if (t_hit[p] != kWideNone) { list.push_back(bsx_hit{done + p, t_hit[p]}); ++listed; }
        }
    }
    if (timing) if (int rc = wait()) return rc;
    unsigned long long hdr[kHdrWords], ctr[4];
    std::vector<unsigned long long> bins(bins_alloc);
    HIPCHK(h, hipMemcpyAsync(hdr, W.d_out.p, sizeof(hdr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bins.data(), W.d_hist.p, bins_alloc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    put_stats(stats, count, ctr[0], ctr[1], kms, launches, t_begin);     // (kms: HIP events around each run of launches waited for)
    if (ctr[2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    for (uint32_t b = 0; b < hist_bins; ++b) hist[b] = bins[b];
    *n_hits = hdr[kHdrHits];
    std::copy(list.begin(), list.end(), hits);
    if (n_listed) *n_listed = listed;
    return BSX_OK;
}

int wide_run_target_summary(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                            const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                            uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats, double t_call) {
    IndexRange src(h, *h->wide, first, max_t);
    return wide_target_summary(h, *h->wide, src, count, mask_words, code_words, hist, hist_bins, hits, cap, n_hits, n_listed, stats, t_call);
}

}  // namespace bsx
