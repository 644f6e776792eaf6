// Target mode of the per-lane family (n <= 256): bsx_run_target and bsx_run_target_summary.  The passes of a call --
// which pieces, which blocks, which words -- come from bsx_lane_lower.h; this file launches them (bsx_target.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bsx_cube_plan.h"
#include "bsx_lane_host.h"

using namespace bsx;

constexpr size_t kAuxStreams = 8, kMultiCtr = 64;

// Auxiliary streams of the handle (created on first use): independent launches of one call run side by side on them.
static int ensure_aux(bsx_handle h) {
    if (h->aux[0]) return BSX_OK;
    for (size_t i = 0; i < kAuxStreams; ++i) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->aux[i], hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->aux_done[i], hipEventDisableTiming));
    }
    HIPCHK(h, h->d_ctr_multi.alloc(kMultiCtr));
    HIPCHK(h, hipHostMalloc((void**)&h->h_ctr_multi, sizeof(Counters) * kMultiCtr, hipHostMallocDefault));
    return BSX_OK;
}

namespace {

// What every pass of a target call shares, and the sums over the passes it has run
struct TargetCall {
    bsx_handle h;
    const bsx_index* first;
    uint64_t max_t;
    const uint64_t *mask_words, *code_words;
    unsigned long long* d_hist = nullptr;       // summary sink: the histogram all passes count into ...
    uint32_t hist_bins = 0;                     // ... and its bins (at least one)
    uint64_t total = 0, steps_ref = 0, steps_exec = 0;
    double kernel_ms = 0.0;
    uint32_t launches = 0, limit_hits = 0;

    void book(const Counters& ctr) {
        total += ctr.log_cursor; steps_ref += ctr.steps_ref; steps_exec += ctr.steps_exec;
        ++launches; limit_hits += ctr.step_limit_hits;
    }
    TargetParams params() const {
        TargetParams P{};
        P.net = h->net;
        P.cap_rel_inf = max_t == BSX_T_INF ? 1 : 0;
        P.max_t = max_t;
        target_words(h->w64, mask_words, code_words, P.tmask, P.tcode);
        P.hist = d_hist;
        P.hist_bins = d_hist ? hist_bins : 1;
        return P;
    }
};

}  // namespace

// One k_target launch over [first + skip, first + skip + count): optional dense t_hit, the call's histogram if it has one.
static int plain_pass(TargetCall& c, uint64_t skip, uint64_t count, uint32_t* d_thit, Counters& ctr) {
    bsx_handle h = c.h;
    const size_t shmem = target_shmem(h->shmem, c.d_hist ? c.hist_bins : 0);
    const Launch L = plan_persistent(h, count, shmem);
    TargetParams P = c.params();
    P.sp = h->sp;
    const bsx_index at = index_plus(*c.first, skip, h->sp.n_any);     // (init_problem adds the offset the same way)
    set_first(P.sp, &at);
    P.count = count;
    P.chunk = L.chunk;
    P.ctr = h->d_ctr;
    P.t_hit = d_thit;
    float ms = 0.f;
    if (int rc = lane_timed_launch(h, ctr, ms, [&]() -> int {
            HIPCHK(h, launch_target((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, L.grid, shmem, h->stream, P));
            return BSX_OK;
        })) return rc;
    c.book(ctr);
    c.kernel_ms += ms;
    return BSX_OK;
}

// Ordered compaction of t_hit[0..count) -> up to `want` hit records (index order), offsets shifted by `skip`.
static int compact_hits(bsx_handle h, const uint32_t* d_thit, uint64_t count, uint64_t total_hits, uint64_t skip,
                        bsx_hit* hits, uint64_t want) {
    if (!total_hits || !want) return BSX_OK;
    const uint32_t segs = (uint32_t)((count + 4095) / 4096);
    DevBuf<uint32_t> d_cnt;
    DevBuf<uint64_t> d_base;
    DevBuf<HitRec> d_hits;
    const uint64_t n_write = std::min(total_hits, want);
    HIPCHK(h, d_cnt.alloc(segs));
    HIPCHK(h, d_base.alloc(segs));
    HIPCHK(h, d_hits.alloc(n_write));
    HIPCHK(h, launch_compact(d_thit, count, d_cnt.p, nullptr, nullptr, 0, false, h->stream));
    std::vector<uint32_t> cnt(segs);
    HIPCHK(h, hipMemcpyAsync(cnt.data(), d_cnt.p, segs * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<uint64_t> base(segs);
    uint64_t run = 0;
    for (uint32_t i = 0; i < segs; ++i) { base[i] = run; run += cnt[i]; }
    if (run != total_hits) return fail(h, BSX_ERR_HIP, "hit compaction count mismatch");
    HIPCHK(h, hipMemcpyAsync(d_base.p, base.data(), segs * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_compact(d_thit, count, nullptr, d_base.p, d_hits.p, n_write, true, h->stream));    // hits past n_write are dropped
    static_assert(sizeof(HitRec) == sizeof(bsx_hit), "hit layout");
    HIPCHK(h, hipMemcpyAsync(hits, d_hits.p, n_write * sizeof(HitRec), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (skip) for (uint64_t i = 0; i < n_write; ++i) hits[i].offset += skip;
    return BSX_OK;
}

extern "C" int bsx_run_target(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                              const uint64_t* mask_words, const uint64_t* code_words, bsx_hit* hits,
                              uint64_t cap, uint64_t* n_hits, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!mask_words || !code_words || !n_hits || (cap && !hits)) return fail(h, BSX_ERR_INVALID, "null argument");
    if (int rc = check_range(h, first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    const double t_begin = now_ms();
    HIPCHK(h, hipSetDevice(h->device));
    *n_hits = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (count > (1ull << 32)) return fail(h, BSX_ERR_INVALID, "at most 2^32 problems per call");
    if (h->wide) return wide_run_target(h, first, count, max_t, mask_words, code_words, hits, cap, n_hits, stats, t_begin);
    DevBuf<uint32_t> d_thit;
    HIPCHK(h, d_thit.alloc(count));
    TargetCall call{h, first, max_t, mask_words, code_words};
    Counters ctr{};
    if (int rc = plain_pass(call, 0, count, d_thit.p, ctr)) return rc;
    if (call.total > cap) return fail(h, BSX_ERR_TABLE_FULL, "more hits than the caller's capacity (bsx_run_target_summary counts without listing)");
    if (int rc = compact_hits(h, d_thit.p, count, call.total, 0, hits, cap)) return rc;
    *n_hits = call.total;
    put_stats(stats, count, call.steps_ref, call.steps_exec, call.kernel_ms, 1, t_begin);
    if (call.limit_hits) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    return BSX_OK;
}

// The cube passes of a call are independent of each other -- one per aligned block and fixed-node variant, each a
// short launch of one-class-per-lane searches that mostly waits (profiles/r03_pmc_config4.json: 90 % of the wave
// cycles) -- so they are enqueued side by side on the handle's auxiliary streams, every launch with its own counter
// block, and the host waits once for all of them (config 4: eight launches of 0.34 ms each back to back before).
struct PendingCube { TargetParams P; dim3 grid; size_t shmem; uint32_t a_bits; uint64_t variant; uint32_t rel; };

static int flush_cubes(TargetCall& c, std::vector<PendingCube>& pending) {
    if (pending.empty()) return BSX_OK;
    bsx_handle h = c.h;
    const size_t n = pending.size();
    if (int rc = ensure_aux(h)) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_ctr_multi.p, 0, n * sizeof(Counters), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    const size_t used = std::min<size_t>(n, kAuxStreams);
    for (size_t i = 0; i < used; ++i) HIPCHK(h, hipStreamWaitEvent(h->aux[i], h->ev0, 0));
    for (size_t i = 0; i < n; ++i) {
        pending[i].P.ctr = h->d_ctr_multi.p + i;
        HIPCHK(h, launch_target((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, pending[i].grid, pending[i].shmem, h->aux[i % kAuxStreams], pending[i].P));
    }
    for (size_t i = 0; i < used; ++i) {
        HIPCHK(h, hipEventRecord(h->aux_done[i], h->aux[i]));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->aux_done[i], 0));
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_ctr_multi, h->d_ctr_multi.p, n * sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    c.kernel_ms += ms;
    for (size_t i = 0; i < n; ++i) {
        c.book(h->h_ctr_multi[i]);
        if (h->knobs.debug) std::fprintf(stderr, "[bsx] target cube 2^%u, variant %llu: %u relevant digits (%zu launches side by side, %.3f ms together)\n", pending[i].a_bits, (unsigned long long)pending[i].variant, pending[i].rel, n, ms);
    }
    pending.clear();
    return BSX_OK;
}

// The block `p` of the counting plan as a cube pass over the digits its first update depends on (build_cube), appended to
// `pending`.  *admitted = false: the block does not collapse far enough (or has too many deposit runs), nothing is appended.
static int enqueue_cube(TargetCall& c, const CountPiece& p, std::vector<PendingCube>& pending, bool* admitted) {
    bsx_handle h = c.h;
    uint32_t vfm[kMaxW32], vfv[kMaxW32];
    for (int w = 0; w < kMaxW32; ++w) { vfm[w] = h->sp.fixmask[w]; vfv[w] = h->sp.fixval[w]; }
    variant_fixed_nodes(h->model.fv, p.variant, vfm, vfv);
    Cube cube;
    build_cube(h->model, h->sp, p.digit, p.a_bits, cube, vfm);
    *admitted = cube.ok && cube.rel.size() + 2 <= p.a_bits;
    if (!*admitted) return BSX_OK;
    plan_cube(h->model, h->sp, cube);
    TargetParams P = c.params();
    P.sp = cube.sp;
    P.sp.n_fv = 0;                              // the variant is baked into the masks
    for (int w = 0; w < kMaxW32; ++w) { P.sp.fixmask[w] = vfm[w]; P.sp.fixval[w] = vfv[w]; }
    target_cube_words(cube, P);
    P.ctr = h->d_ctr;
    P.t_hit = nullptr;
    const size_t shmem = target_shmem(h->shmem, P.hist_bins);
    const Launch L = plan_persistent(h, P.count, shmem);
    target_cube_shares((uint64_t)L.grid.x * kWavesPerBlock, L.chunk, P);
    pending.push_back(PendingCube{P, L.grid, shmem, p.a_bits, p.variant, (uint32_t)cube.rel.size()});
    if (pending.size() == kMultiCtr) return flush_cubes(c, pending);
    return BSX_OK;
}

extern "C" int bsx_run_target_summary(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                                      const uint64_t* mask_words, const uint64_t* code_words,
                                      uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                                      uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!mask_words || !code_words || !n_hits || (cap && (!hits || !n_listed)) || (hist_bins && !hist))
        return fail(h, BSX_ERR_INVALID, "null argument");
    if (hist_bins > kTargetHistBins) return fail(h, BSX_ERR_INVALID, "at most 2048 histogram bins");
    if (int rc = check_range(h, first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    const double t_begin = now_ms();
    HIPCHK(h, hipSetDevice(h->device));
    *n_hits = 0;
    if (n_listed) *n_listed = 0;
    for (uint32_t b = 0; b < hist_bins; ++b) hist[b] = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (count > (1ull << 40)) return fail(h, BSX_ERR_INVALID, "at most 2^40 problems per call");
    if (h->wide) return wide_run_target_summary(h, first, count, max_t, mask_words, code_words, hist, hist_bins, hits, cap, n_hits, n_listed, stats, t_begin);

    DevBuf<unsigned long long> d_hist;              // (one bin even if the caller wants none: the kernels count into it)
    HIPCHK(h, d_hist.alloc(std::max<uint32_t>(hist_bins, 1)));
    HIPCHK(h, hipMemsetAsync(d_hist.p, 0, std::max<uint32_t>(hist_bins, 1) * sizeof(unsigned long long), h->stream));
    TargetCall call{h, first, max_t, mask_words, code_words, d_hist.p, std::max<uint32_t>(hist_bins, 1)};
    // The hit list is the first `cap` hits in index order (what -n keeps, simulate.py:163-164): problems are
    // scanned in pieces with a dense t_hit array until the list is full, the rest of the range is only counted.
    uint64_t done = 0, listed = 0;
    DevBuf<uint32_t> d_thit;
    while (done < count && listed < cap) {
        const uint64_t piece = target_listing_piece(count - done, cap - listed);
        HIPCHK(h, d_thit.reserve(std::min<uint64_t>(piece, 1ull << 32)));
        const uint64_t n = std::min<uint64_t>(piece, d_thit.n);
        Counters ctr{};
        if (int rc = plain_pass(call, done, n, d_thit.p, ctr)) return rc;
        if (int rc = compact_hits(h, d_thit.p, n, ctr.log_cursor, done, hits + listed, cap - listed)) return rc;
        listed += std::min<uint64_t>(ctr.log_cursor, cap - listed);
        done += n;
    }
    // the rest is only counted: cube passes over the aligned blocks of every fixed-node variant (the first update
    // of a block depends on its relevant digits only, build_cube), plain passes over what is left
    const bool cubes_ok = h->knobs.cubes && target_cubes_ok(h->sp, h->variant_count_saturated);
    std::vector<PendingCube> pending;
    while (done < count) {
        const CountPiece p = count_piece(*first, done, count, h->sp.n_any, cubes_ok);
        bool as_cube = false;
        if (p.block) if (int rc = enqueue_cube(call, p, pending, &as_cube)) return rc;
        if (!as_cube) {
            Counters ctr{};
            if (int rc = plain_pass(call, done, p.n, nullptr, ctr)) return rc;
        }
        done += p.n;
    }
    if (int rc = flush_cubes(call, pending)) return rc;
    if (hist_bins) HIPCHK(h, hipMemcpy(hist, d_hist.p, hist_bins * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_hits = call.total;
    if (n_listed) *n_listed = listed;
    put_stats(stats, count, call.steps_ref, call.steps_exec, call.kernel_ms, call.launches, t_begin);
    if (call.limit_hits) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    return BSX_OK;
}
