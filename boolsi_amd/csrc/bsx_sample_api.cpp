// The calls over samples of a seed instead of consecutive problem indices (include/bsx.h and bsx_sample.h have the
// definition of sample j): bsx_run_attract_sampled, bsx_run_target_sampled, bsx_run_simulate_sampled,
// bsx_run_trajectories_sampled and bsx_sample_problems.  The chain behind a sampled call is the one of its enumerating
// counterpart on the wide family (bsx_wide_attract_api.cpp, bsx_wide_api.cpp) with another source of launches: the sampled
// instantiation of the call's mode in place of k_wide<K, KW>.
//
// Handles of the <= BSX_MAX_NODES family have no wide lowering of their own: the first sampled call lowers the arguments
// that bsx_set_network / bsx_set_problem_space received (bsx_engine::inputs) a second time, into a WideHost the handle
// owns (bsx_engine::sample_wide), and every later sampled call on the same network and space reuses it.  The per-lane
// kernels and their host state are not touched.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_wide_host.h"
// (behind the HIP runtime, which defines what BSX_HD expands to)
#include "bsx_sample.h"

using namespace bsx;

// The WideHost a sampled call works on: the handle's own, or the second lowering (built here on first use).
int bsx::sample_host(bsx_handle h, WideHost** out) {
    if (h->wide) { *out = h->wide; return BSX_OK; }
    if (!h->sample_wide) {
        const SampleInputs& in = h->inputs;
        WideHost* W = new WideHost();
        int rc = wide_upload_network(h, *W, h->n_nodes, in.pred_offsets.data(), in.pred_idx.data(), in.tt_word_offsets.data(),
                                     in.tt_words.data());
        if (rc == BSX_OK)
            rc = wide_upload_space(h, *W, in.origin.data(), in.any_nodes.data(), (uint32_t)in.any_nodes.size(), in.fixed.data(),
                                   (uint32_t)in.fixed.size(), in.fixed_var.data(), (uint32_t)in.fixed_var.size(), in.sched.data(),
                                   (uint32_t)in.sched.size(), in.pert_var.data(), (uint32_t)in.pert_var.size());
        if (rc != BSX_OK) { delete W; return rc; }
        h->sample_wide = W;
    }
    *out = h->sample_wide;
    return BSX_OK;
}

namespace {

// Launches over samples [first + done, first + done + m) of the seed behind k0 ...
struct SampleRange : WideSource {
    bsx_handle h; WideHost& W; uint64_t k0, first, max_t;
    SampleRange(bsx_handle h_, WideHost& W_, uint64_t k, uint64_t f, uint64_t t) : h(h_), W(W_), k0(k), first(f), max_t(t) {}
    int enqueue(WideParams& P, uint64_t done, uint64_t m) override { return wide_enqueue_sampled(h, W, P, k0, first + done, m, max_t); }
};
// ... and one launch over the listed samples (device memory)
struct SampleList : WideSource {
    bsx_handle h; WideHost& W; uint64_t k0, max_t; const uint64_t* d_list;
    SampleList(bsx_handle h_, WideHost& W_, uint64_t k, uint64_t t, const uint64_t* l) : h(h_), W(W_), k0(k), max_t(t), d_list(l) {}
    int enqueue(WideParams& P, uint64_t done, uint64_t m) override { return wide_enqueue_sampled(h, W, P, k0, 0, m, max_t, d_list + done); }
};

// What every call over a range of samples checks behind its own arguments
int check_sample_range(bsx_handle h, uint64_t first_sample, uint64_t n_samples) {
    if (first_sample + n_samples < first_sample) return fail(h, BSX_ERR_INVALID, "first_sample + n_samples wraps");
    if (h->variant_count_saturated) return fail(h, BSX_ERR_UNSUPPORTED, "the problem space has 2^64 variants or more");
    return BSX_OK;
}

}  // namespace

extern "C" int bsx_run_attract_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint64_t max_t,
                                       uint64_t max_len, bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out,
                                       uint64_t* n_no_attractor, bsx_stats2* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    *n_out = 0;
    if (n_no_attractor) *n_no_attractor = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (int rc = check_sample_range(h, first_sample, n_samples)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    if (n_samples == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    WideHost& W = *Wp;
    const uint64_t chunk = std::min<uint64_t>(n_samples, wide_chunk(h, W, 1ull << 18));
    // (the host-reduce path under the conditions of bsx_run_attract_wide)
    const bool on_device = !h->knobs.wide_host_reduce && std::min<uint64_t>(cap, n_samples) <= kWideReduceMaxCap;
    SampleRange src(h, W, sample_k0(seed), first_sample, max_t);
    bsx_u128 none{0, 0};
    const int rc = (on_device ? attract_wide_device : attract_wide_host)(h, W, src, n_samples, chunk, max_len, table, cap, n_out, &none,
                                                                         stats, t_begin);
    if (rc == BSX_OK && n_no_attractor) *n_no_attractor = none.lo;
    return rc;
}

extern "C" int bsx_sample_problems(bsx_handle h, uint64_t seed, const uint64_t* samples, uint64_t n, uint64_t* states,
                                   uint64_t* variants) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (n && (!samples || !states)) return fail(h, BSX_ERR_INVALID, "samples / states is null");
    if (h->variant_count_saturated) return fail(h, BSX_ERR_UNSUPPORTED, "the problem space has 2^64 variants or more");
    if (n == 0) return BSX_OK;
    if (n > (1ull << 31)) return fail(h, BSX_ERR_UNSUPPORTED, "more than 2^31 samples listed in one call");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    const WideHost& W = *Wp;
    DevBuf<uint64_t> d_samples, d_states, d_variants;
    HIPCHK(h, d_samples.alloc(n));
    HIPCHK(h, hipMemcpy(d_samples.p, samples, n * 8, hipMemcpyHostToDevice));
    HIPCHK(h, d_states.alloc(n * W.net.w64));
    if (variants) HIPCHK(h, d_variants.alloc(n));
    WideSampleListParams Q{};
    Q.n_nodes = W.net.n; Q.w64 = W.net.w64; Q.n_any = W.space.n_any;
    std::memcpy(Q.origin, W.space.origin, sizeof(Q.origin));
    Q.any_nodes = W.d_any.p;
    Q.k0 = sample_k0(seed);
    Q.variant_count = W.space.variant_count;
    Q.samples = d_samples.p; Q.n = n;
    Q.states = d_states.p;
    Q.variants = variants ? d_variants.p : nullptr;
    HIPCHK(h, launch_sample_problems(Q, h->stream));
    HIPCHK(h, hipMemcpyAsync(states, d_states.p, n * W.net.w64 * 8, hipMemcpyDeviceToHost, h->stream));
    if (variants) HIPCHK(h, hipMemcpyAsync(variants, d_variants.p, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BSX_OK;
}

// target over samples: the chain of bsx_run_target_summary on a wide network (wide_target_summary), offsets counted from
// first_sample.  The caller's arrays are written only when the call succeeds.
extern "C" int bsx_run_target_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint64_t max_t,
                                      const uint64_t* mask_words, const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins,
                                      bsx_hit* hits, uint64_t cap, uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!mask_words || !code_words || !n_hits || (cap && (!hits || !n_listed)) || (hist_bins && !hist))
        return fail(h, BSX_ERR_INVALID, "null argument");
    if (hist_bins > kTargetHistBins) return fail(h, BSX_ERR_INVALID, "at most 2048 histogram bins");
    if (int rc = check_sample_range(h, first_sample, n_samples)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    const double t_begin = now_ms();
    *n_hits = 0;
    if (n_listed) *n_listed = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_samples == 0) {
        for (uint32_t b = 0; b < hist_bins; ++b) hist[b] = 0;
        return BSX_OK;
    }
    if (n_samples > (1ull << 40)) return fail(h, BSX_ERR_INVALID, "at most 2^40 samples per call");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    SampleRange src(h, *Wp, sample_k0(seed), first_sample, max_t);
    return wide_target_summary(h, *Wp, src, n_samples, mask_words, code_words, hist, hist_bins, hits, cap, n_hits, n_listed, stats, t_begin);
}

extern "C" int bsx_run_simulate_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint64_t max_t,
                                        uint64_t* trajectories, uint64_t* final_states, uint64_t* digests, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (int rc = check_sample_range(h, first_sample, n_samples)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_samples == 0) return BSX_OK;
    if (max_t >= kStepLimit) return fail(h, BSX_ERR_UNSUPPORTED, "simulation length above the engine's step limit");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    SampleRange src(h, *Wp, sample_k0(seed), first_sample, max_t);
    return wide_sim(h, *Wp, src, n_samples, max_t, nullptr, nullptr, nullptr, trajectories ? n_samples * (max_t + 1) * Wp->net.w64 : 0,
                    trajectories, final_states, digests, stats);
}

extern "C" int bsx_run_trajectories_sampled(bsx_handle h, uint64_t seed, const uint64_t* samples, const uint64_t* t_len, uint64_t n,
                                            uint64_t* out, const uint64_t* out_offsets, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (n && (!samples || !t_len || !out || !out_offsets)) return fail(h, BSX_ERR_INVALID, "null argument");
    if (h->variant_count_saturated) return fail(h, BSX_ERR_UNSUPPORTED, "the problem space has 2^64 variants or more");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    if (n > (1ull << 31)) return fail(h, BSX_ERR_UNSUPPORTED, "more than 2^31 samples listed in one call");
    uint64_t words = 0, tmax = 0;
    for (uint64_t q = 0; q < n; ++q) {
        words = std::max(words, out_offsets[q] + (t_len[q] + 1) * h->w64);
        tmax = std::max(tmax, t_len[q]);
    }
    if (tmax >= kStepLimit) return fail(h, BSX_ERR_UNSUPPORTED, "simulation length above the engine's step limit");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    DevBuf<uint64_t> d_samples;
    HIPCHK(h, d_samples.upload(std::vector<uint64_t>(samples, samples + n)));
    SampleList src(h, *Wp, sample_k0(seed), tmax, d_samples.p);
    return wide_sim(h, *Wp, src, n, tmax, nullptr, t_len, out_offsets, words, out, nullptr, nullptr, stats);
}
