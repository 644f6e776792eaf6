// bsx_run_attract_wide: attract over the wide-state family's per-problem records, aggregated by key -- on the device
// (bsx_wide_reduce.hip) or, with BSX_WIDE_HOST_REDUCE=1 or a table beyond kWideReduceMaxCap, chunk by chunk on the host
// (the path before bsx_wide_reduce.hip; kept for A/B runs and tests).  Both legs take the source of their launches as
// an argument (WideSource, bsx_wide_host.h): bsx_run_attract_sampled (bsx_sample_api.cpp) runs them over samples.
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "bsx_wide_host.h"

using namespace bsx;

static_assert(sizeof(WideAttrRec) == sizeof(bsx_attr_rec2w), "drained records have the layout of bsx_attr_rec2w");
static_assert(kWideMaxW32 / 2 == BSX_MAX_STATE_WORDS, "key words");

// The statistics of either leg: they differ in what they launched and how often the host waited.
static void put_stats2(bsx_stats2* stats, uint64_t count, u128 state_steps, uint64_t exec, double ms, uint32_t wide_launches,
                       uint32_t kernel_launches, uint32_t syncs, double t_begin) {
    if (!stats) return;
    stats->problems = bsx_u128{count, 0};
    stats->state_steps = bsx_u128{(uint64_t)state_steps, (uint64_t)(state_steps >> 64)};
    stats->executed_steps = exec;
    stats->kernel_ms = ms;                  // HIP events around every chain of launches the host waited for
    stats->dominant_ms = ms;
    stats->dominant_executed_steps = exec;
    stats->dominant_launches = wide_launches;
    stats->kernel_launches = kernel_launches;
    stats->host_syncs = syncs;
    stats->total_ms = now_ms() - t_begin;
}

static WideParams attract_params(uint32_t* d_info, uint64_t* d_keys, uint64_t max_len) {
    WideParams P{};
    P.mode = kWideAttract;
    P.info = d_info;
    P.keys = d_keys;
    P.max_len = max_len;
    return P;
}

// Device path: k_wide and k_wide_reduce_attract are enqueued for every chunk back to back (one info / keys buffer:
// the stream orders them), k_wide_reduce_drain packs the table, and the host waits once.  The first
// kInlineRecs records come back with the header in that one copy; a table with more costs a second copy.
static constexpr uint32_t kInlineRecs = 256;

int bsx::attract_wide_device(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t chunk, uint64_t max_len,
                             bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor, bsx_stats2* stats,
                             double t_begin) {
    const uint32_t w64 = W.net.w64;
    // a range of `count` problems has at most `count` attractors: the device structures follow the smaller of the two,
    // so a caller's very large cap ("no limit") costs nothing
    const uint64_t dcap = std::min<uint64_t>(cap, count);
    uint64_t slots = kWideReduceMinSlots;
    while (slots < 2 * dcap) slots <<= 1;
    constexpr size_t kRecWords = sizeof(WideAttrRec) / 8;
    HIPCHK(h, W.d_info.reserve(chunk * 4));
    HIPCHK(h, W.d_keys.reserve(chunk * w64));
    HIPCHK(h, W.d_table.reserve(slots));
    HIPCHK(h, W.d_out.reserve(kHdrWords + (size_t)std::max<uint64_t>(dcap, 1) * kRecWords));
    unsigned long long* d_hdr = W.d_out.p;
    WideAttrRec* d_recs = reinterpret_cast<WideAttrRec*>(W.d_out.p + kHdrWords);
    HIPCHK(h, hipMemsetAsync(W.d_table.p, 0, slots * sizeof(WideSlot), h->stream));
    HIPCHK(h, hipMemsetAsync(d_hdr, 0, kHdrWords * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    uint32_t wide_launches = 0;
    for (uint64_t done = 0; done < count; done += chunk, ++wide_launches) {
        const uint64_t m = std::min(chunk, count - done);
        WideParams P = attract_params(W.d_info.p, W.d_keys.p, max_len);
        if (int rc = src.enqueue(P, done, m)) return rc;
        HIPCHK(h, launch_wide_reduce_attract(W.d_info.p, W.d_keys.p, m, w64, W.d_table.p, slots, d_hdr, h->stream));
    }
    HIPCHK(h, launch_wide_reduce_drain(W.d_table.p, slots, d_recs, dcap, d_hdr, W.d_ctr.p, h->stream));
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    const uint32_t inl = (uint32_t)std::min<uint64_t>(dcap, kInlineRecs);
    std::vector<unsigned long long> back(kHdrWords + (size_t)inl * kRecWords);
    HIPCHK(h, hipMemcpyAsync(back.data(), W.d_out.p, back.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    uint32_t syncs = 1;
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    const unsigned long long* hdr = back.data();
    if (hdr[kHdrCtr + 2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    if (hdr[kHdrOverflow] & 2) return fail(h, BSX_ERR_HIP, "wide attract reduction: a table slot stayed half-written");
    if ((hdr[kHdrOverflow] & 1) || hdr[kHdrCursor] > cap)
        return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's capacity");
    const uint32_t n = (uint32_t)hdr[kHdrCursor];
    std::vector<bsx_attr_rec2w> recs(n);
    const uint32_t n_inl = std::min(n, inl);
    if (n_inl) std::memcpy(recs.data(), back.data() + kHdrWords, (size_t)n_inl * sizeof(WideAttrRec));
    if (n > n_inl) {
        HIPCHK(h, hipMemcpy(recs.data() + n_inl, d_recs + n_inl, (size_t)(n - n_inl) * sizeof(WideAttrRec), hipMemcpyDeviceToHost));
        ++syncs;
    }
    // the order of the host path's std::map over key arrays: lexicographic from word 0
    std::sort(recs.begin(), recs.end(), [](const bsx_attr_rec2w& a, const bsx_attr_rec2w& b) {
        return std::lexicographical_compare(a.key, a.key + BSX_MAX_STATE_WORDS, b.key, b.key + BSX_MAX_STATE_WORDS);
    });
    std::copy(recs.begin(), recs.end(), table);
    *n_out = n;
    if (n_no_attractor) *n_no_attractor = bsx_u128{hdr[kHdrNone], 0};
    put_stats2(stats, count, hdr[kHdrCtr + 0], hdr[kHdrCtr + 1], ms, wide_launches, 2 * wide_launches + 1, syncs, t_begin);
    return BSX_OK;
}

// Host path: every chunk's records come back and are aggregated here by key; one launch and one wait per chunk.
int bsx::attract_wide_host(bsx_handle h, WideHost& W, WideSource& src, uint64_t count, uint64_t chunk, uint64_t max_len,
                           bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor, bsx_stats2* stats,
                           double t_begin) {
    const uint32_t w64 = W.net.w64;
    DevBuf<uint32_t> d_info;
    DevBuf<uint64_t> d_keys;
    HIPCHK(h, d_info.alloc(chunk * 4));
    HIPCHK(h, d_keys.alloc(chunk * w64));
    std::vector<uint32_t> info(chunk * 4);
    std::vector<uint64_t> keys(chunk * w64);
    struct Agg { uint64_t length = 0; u128 count = 0, sl = 0, sl2 = 0; };
    std::map<std::array<uint64_t, BSX_MAX_STATE_WORDS>, Agg> agg;
    u128 none = 0, ref_steps = 0;
    uint64_t exec = 0;
    double kms = 0;
    uint32_t launches = 0;
    bool limit = false;
    for (uint64_t done = 0; done < count; done += chunk) {
        const uint64_t m = std::min(chunk, count - done);
        WideParams P = attract_params(d_info.p, d_keys.p, max_len);
        unsigned long long ctr[4];
        float ms = 0.f;
        HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));     // (one launch, waited for: wide_launch)
        HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        if (int rc = src.enqueue(P, done, m)) return rc;
        if (int rc = wide_timed_wait(h, W, ctr, ms)) return rc;
        HIPCHK(h, hipMemcpy(info.data(), d_info.p, m * 16, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(keys.data(), d_keys.p, m * w64 * 8, hipMemcpyDeviceToHost));
        kms += ms; ++launches; exec += ctr[1]; ref_steps += ctr[0];
        limit = limit || ctr[2];
        for (uint64_t q = 0; q < m; ++q) {
            if (!info[4 * q]) { ++none; continue; }
            std::array<uint64_t, BSX_MAX_STATE_WORDS> k{};
            for (uint32_t w = 0; w < w64; ++w) k[w] = keys[q * w64 + w];
            Agg& a = agg[k];
            const uint64_t l = (uint64_t)info[4 * q + 2] | ((uint64_t)info[4 * q + 3] << 32);
            a.length = info[4 * q + 1];
            a.count += 1; a.sl += l; a.sl2 += (u128)l * l;
        }
    }
    if (limit) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    if (agg.size() > cap) return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's capacity");
    uint32_t i = 0;
    for (const auto& e : agg) {
        bsx_attr_rec2w r{};
        std::memcpy(r.key, e.first.data(), sizeof(r.key));
        r.length = e.second.length;
        r.count = bsx_u128{(uint64_t)e.second.count, (uint64_t)(e.second.count >> 64)};
        r.sum_l[0] = (uint64_t)e.second.sl; r.sum_l[1] = (uint64_t)(e.second.sl >> 64);
        r.sum_l2[0] = (uint64_t)e.second.sl2; r.sum_l2[1] = (uint64_t)(e.second.sl2 >> 64);
        table[i++] = r;
    }
    *n_out = i;
    if (n_no_attractor) *n_no_attractor = bsx_u128{(uint64_t)none, (uint64_t)(none >> 64)};
    put_stats2(stats, count, ref_steps, exec, kms, launches, launches, launches, t_begin);
    return BSX_OK;
}

extern "C" int bsx_run_attract_wide(bsx_handle h, bsx_u128 first_flat, bsx_u128 count_flat, uint64_t max_t, uint64_t max_len,
                                    bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor,
                                    bsx_stats2* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!h->wide) {
        // networks of the <= 256-node family: bsx_run_attract2, keys zero-extended
        std::vector<bsx_attr_rec2> t2(cap ? cap : 1);
        const int rc = bsx_run_attract2(h, first_flat, count_flat, max_t, max_len, t2.data(), cap, n_out, n_no_attractor, stats);
        if (rc != BSX_OK) return rc;
        for (uint32_t i = 0; i < *n_out; ++i) {
            bsx_attr_rec2w r{};
            std::memcpy(r.key, t2[i].key, sizeof(t2[i].key));
            r.length = t2[i].length; r.count = t2[i].count;
            std::memcpy(r.sum_l, t2[i].sum_l, sizeof(r.sum_l));
            std::memcpy(r.sum_l2, t2[i].sum_l2, sizeof(r.sum_l2));
            table[i] = r;
        }
        return BSX_OK;
    }
    const double t_begin = now_ms();
    *n_out = 0;
    if (n_no_attractor) *n_no_attractor = bsx_u128{0, 0};
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count_flat.hi) return fail(h, BSX_ERR_UNSUPPORTED, "wide networks: at most 2^64 - 1 problems per call");
    const uint64_t count = count_flat.lo;
    WideHost& W = *h->wide;
    if (int rc = wide_check_enumerable(h, W)) return rc;
    bsx_index first{};
    if (const LowerStatus s = wide_split_flat(first_flat, h->sp.n_any, first)) return fail(h, s.status, s.msg);
    if (int rc = check_range(h, &first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    if (count == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t chunk = std::min<uint64_t>(count, wide_chunk(h, W, 1ull << 18));
    // (more than kWideReduceMaxCap possible attractors: the device table would take gigabytes; such a call is reduced
    // on the host, which allocates per attractor found)
    const bool on_device = !h->knobs.wide_host_reduce && std::min<uint64_t>(cap, count) <= kWideReduceMaxCap;
    struct Range : WideSource {      // consecutive problem indices from `first`
        bsx_handle h; WideHost& W; const bsx_index& first; uint64_t max_t;
        Range(bsx_handle h_, WideHost& W_, const bsx_index& f, uint64_t t) : h(h_), W(W_), first(f), max_t(t) {}
        int enqueue(WideParams& P, uint64_t done, uint64_t m) override {
            const bsx_index at = index_plus(first, done, h->sp.n_any);
            return wide_enqueue(h, W, P, &at, m, max_t);
        }
    } src(h, W, first, max_t);
    return (on_device ? attract_wide_device : attract_wide_host)(h, W, src, count, chunk, max_len, table, cap, n_out, n_no_attractor, stats, t_begin);
}
