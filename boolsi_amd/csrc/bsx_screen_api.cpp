// bsx_run_screen_sampled (include/bsx.h has the definition): knockout / overexpression screens over samples, every mutant
// on the wild type's initial states, in one device call.  Host side of k_wide_screen (bsx_wide.hip) and the reduction of
// bsx_screen_reduce.hip over the WideHost the sampled calls work on: the handle's own, or the second lowering of a handle of
// the <= BSX_MAX_NODES family (sample_host, bsx_sample_api.cpp).  Every check comes before the first launch (bsx_screen.h
// has those that need no device); per chunk of (mutant, group) pairs the kernel and the reduction are enqueued back to
// back, then one drain, and the host waits once.  The caller's arrays are written only when the call succeeds.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_table_lower.h"
#include "bsx_wide_host.h"
// (behind the HIP runtime, which defines what BSX_HD expands to)
#include "bsx_sample.h"
#include "bsx_screen.h"

using namespace bsx;

static_assert(sizeof(ScreenRec) == sizeof(bsx_screen_rec), "drained records have the layout of bsx_screen_rec");
static_assert(sizeof(bsx_fixed) == 8, "mut_nodes is uploaded as (node, value) word pairs");

extern "C" int bsx_run_screen_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, const uint32_t* mut_offsets,
                                      const bsx_fixed* mut_nodes, uint32_t n_mutants, uint64_t max_t, uint64_t max_len,
                                      bsx_screen_rec* table, uint64_t cap, uint64_t* n_out, uint64_t* n_no_attractor, bsx_stats2* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (first_sample + n_samples < first_sample) return fail(h, BSX_ERR_INVALID, "first_sample + n_samples wraps");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    WideHost& W = *Wp;
    const WideSpace& S = W.space;
    if (const ScreenStatus s = screen_check_mutants(W.net.n, S.fixmask, mut_offsets, mut_nodes, n_mutants))
        return fail(h, s.status, s.msg.c_str());
    if (S.n_fv) return fail(h, BSX_ERR_UNSUPPORTED, "screen: the problem space has fixed-node variations");
    if (S.n_pv) return fail(h, BSX_ERR_UNSUPPORTED, "screen: the problem space has perturbation variations");
    if (S.n_sched) return fail(h, BSX_ERR_UNSUPPORTED, "screen: the origin has a perturbation schedule");
    if (!screen_range_ok(n_samples, n_mutants)) return fail(h, BSX_ERR_RANGE_TOO_LARGE, "screen: n_mutants * n_samples exceeds 2^40");
    if (int rc = check_max_t(h, max_t)) return rc;

    if (n_samples == 0) {
        *n_out = 0;
        if (n_no_attractor) std::fill(n_no_attractor, n_no_attractor + n_mutants, 0ull);
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return BSX_OK;
    }

    const uint32_t rows = W.net.rows, L = S.L, w64 = W.net.w64;
    const ScreenLayout lay = screen_layout(n_samples, n_mutants, L, wide_chunk(h, W, 1ull << 18));
    const uint32_t G = lay.G;
    const size_t shmem = (size_t)wide_screen_lds_words(rows, L, S.n_fslots) * 4;
    // at most one record per trajectory: the device structures follow the smaller of the caller's cap and that
    const uint64_t dcap = std::min<uint64_t>(std::min<uint64_t>(cap, kWideReduceMaxCap), (uint64_t)n_mutants * n_samples);
    uint64_t slots = kWideReduceMinSlots;
    while (slots < 2 * dcap) slots <<= 1;
    constexpr size_t kRecWords = sizeof(ScreenRec) / 8;

    const uint32_t n_listed = mut_offsets[n_mutants];
    std::vector<uint32_t> offs(mut_offsets, mut_offsets + n_mutants + 1), nodes(2 * (size_t)std::max(n_listed, 1u), 0u);
    for (uint32_t i = 0; i < n_listed; ++i) { nodes[2 * i] = mut_nodes[i].node; nodes[2 * i + 1] = mut_nodes[i].value; }
    DevBuf<uint32_t> d_offs, d_nodes;
    HIPCHK(h, d_offs.upload(offs));
    HIPCHK(h, d_nodes.upload(nodes));
    HIPCHK(h, W.d_screen.reserve(slots));
    HIPCHK(h, W.d_info.reserve(lay.chunk_pairs * G * 4));
    HIPCHK(h, W.d_keys.reserve(lay.chunk_pairs * G * w64));
    HIPCHK(h, W.d_out.reserve(kHdrWords + (size_t)std::max<uint64_t>(dcap, 1) * kRecWords));
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(lay.chunk_pairs, wide_blocks(h, W, lay.chunk_pairs * G, shmem)));
    HIPCHK(h, W.d_x0.reserve((size_t)blocks * rows * L));
    unsigned long long* d_hdr = W.d_out.p;
    ScreenRec* d_recs = reinterpret_cast<ScreenRec*>(W.d_out.p + kHdrWords);

    WideScreenParams Q{};
    WideParams& P = Q.net;
    wide_fill_net(W, P);
    P.mode = kWideAttract;
    std::memcpy(P.origin, S.origin, sizeof(P.origin));
    P.n_any = S.n_any;
    P.any_nodes = W.d_any.p;
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;
    P.max_len = max_len;
    P.info = W.d_info.p;
    P.keys = W.d_keys.p;
    P.x0 = W.d_x0.p;
    P.ctr = W.d_ctr.p;
    P.sample_k0 = sample_k0(seed);
    Q.first_sample = first_sample; Q.n_samples = n_samples;
    Q.g_per = lay.g_per;
    Q.mut_offsets = d_offs.p; Q.mut_nodes = d_nodes.p;

    HIPCHK(h, hipMemsetAsync(W.d_screen.p, 0, slots * sizeof(ScreenSlot), h->stream));
    HIPCHK(h, hipMemsetAsync(d_hdr, 0, kHdrWords * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    uint32_t launches = 0;
    for (const Chunk c : chunks(lay.pairs, lay.chunk_pairs)) {
        Q.p0 = c.first; Q.n_pairs = c.count;
        const uint64_t grid = std::min<uint64_t>(c.count, blocks);
        HIPCHK(h, launch_wide_screen((int)W.net.K, dim3((uint32_t)grid), shmem, h->stream, Q));
        HIPCHK(h, launch_screen_reduce(W.d_info.p, W.d_keys.p, c.count, c.first, lay.g_per, n_samples, G, w64, W.d_screen.p, slots, d_hdr, h->stream));
        ++launches;
    }
    HIPCHK(h, launch_screen_drain(W.d_screen.p, slots, d_recs, dcap, d_hdr, W.d_ctr.p, h->stream));
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    // the call's one wait: header and the first kScreenInlineRecs records in one copy
    const uint32_t inl = (uint32_t)std::min<uint64_t>(dcap, kScreenInlineRecs);
    std::vector<unsigned long long> back(kHdrWords + (size_t)inl * kRecWords);
    HIPCHK(h, hipMemcpyAsync(back.data(), W.d_out.p, back.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    uint32_t syncs = 1;
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    const unsigned long long* hdr = back.data();
    if (hdr[kHdrCtr + 2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    if (hdr[kHdrOverflow] & 2) return fail(h, BSX_ERR_HIP, "screen reduction: a table slot stayed half-written");
    if ((hdr[kHdrOverflow] & 1) || hdr[kHdrCursor] > dcap)
        return fail(h, BSX_ERR_TABLE_FULL, "more distinct (mutant, attractor) pairs than the caller's capacity");
    const uint64_t n = hdr[kHdrCursor];
    std::vector<bsx_screen_rec> recs(n);
    const uint64_t n_inl = std::min<uint64_t>(n, inl);
    if (n_inl) std::memcpy(recs.data(), back.data() + kHdrWords, (size_t)n_inl * sizeof(ScreenRec));
    if (n > n_inl) {
        HIPCHK(h, hipMemcpy(recs.data() + n_inl, d_recs + n_inl, (size_t)(n - n_inl) * sizeof(ScreenRec), hipMemcpyDeviceToHost));
        ++syncs;
    }
    std::sort(recs.begin(), recs.end(), [](const bsx_screen_rec& a, const bsx_screen_rec& b) {
        if (a.mutant != b.mutant) return a.mutant < b.mutant;
        return std::lexicographical_compare(a.rec.key, a.rec.key + BSX_MAX_STATE_WORDS, b.rec.key, b.rec.key + BSX_MAX_STATE_WORDS);
    });
    std::copy(recs.begin(), recs.end(), table);
    *n_out = n;
    if (n_no_attractor) {
        std::fill(n_no_attractor, n_no_attractor + n_mutants, n_samples);
        for (const bsx_screen_rec& r : recs) n_no_attractor[r.mutant] -= r.rec.count.lo;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->problems = bsx_u128{(uint64_t)n_mutants * n_samples, 0};
        stats->state_steps = bsx_u128{hdr[kHdrCtr + 0], 0};
        stats->executed_steps = hdr[kHdrCtr + 1];
        stats->kernel_ms = ms;
        stats->dominant_ms = ms;
        stats->dominant_executed_steps = hdr[kHdrCtr + 1];
        stats->dominant_launches = launches;
        stats->kernel_launches = 2 * launches + 1;
        stats->host_syncs = syncs;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}
