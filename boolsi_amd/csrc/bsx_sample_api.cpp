// bsx_run_attract_sampled and bsx_sample_problems: attract over samples of a seed instead of consecutive problem indices
// (include/bsx.h and bsx_sample.h have the definition of sample j).  The chain behind a sampled call is the one of
// bsx_run_attract_wide (bsx_wide_attract_api.cpp) with k_wide<K, KW, true> in place of k_wide<K, KW>.
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
static int sample_host(bsx_handle h, WideHost** out) {
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
    if (first_sample + n_samples < first_sample) return fail(h, BSX_ERR_INVALID, "first_sample + n_samples wraps");
    if (h->variant_count_saturated) return fail(h, BSX_ERR_UNSUPPORTED, "the problem space has 2^64 variants or more");
    if (int rc = check_max_t(h, max_t)) return rc;
    if (n_samples == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    WideHost& W = *Wp;
    const uint64_t chunk = std::min<uint64_t>(n_samples, wide_chunk(h, W, 1ull << 18));
    // (the host-reduce path under the conditions of bsx_run_attract_wide)
    const bool on_device = !h->knobs.wide_host_reduce && std::min<uint64_t>(cap, n_samples) <= kWideReduceMaxCap;
    struct Samples : WideAttractSource {
        bsx_handle h; WideHost& W; uint64_t k0, first, max_t;
        Samples(bsx_handle h_, WideHost& W_, uint64_t k, uint64_t f, uint64_t t) : h(h_), W(W_), k0(k), first(f), max_t(t) {}
        int enqueue(WideParams& P, uint64_t done, uint64_t m) override { return wide_enqueue_sampled(h, W, P, k0, first + done, m, max_t); }
    } src(h, W, sample_k0(seed), first_sample, max_t);
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
