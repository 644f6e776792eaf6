// Host side of the wide-state family (bsx_wide.hip): lowering of networks of up to BSX_MAX_NODES_WIDE nodes to
// per-row descriptors, the run entry points of include/bsx.h for such networks, and bsx_run_attract_wide.
// bsx_api.cpp hands a handle over here when its network has more than BSX_MAX_NODES nodes (or BSX_WIDE=1).
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_trans.h"
#include "bsx_wide.h"
#include "bsx_wtrans.h"

namespace bsx {

hipError_t launch_wide(int k, dim3 grid, size_t shmem, hipStream_t st, const WideParams& P);
hipError_t launch_wide_profile(int k, dim3 grid, size_t shmem, hipStream_t st, const WideProfileParams& Q);
hipError_t launch_wide_trans(int k, dim3 grid, size_t shmem, hipStream_t st, const WideTransParams& Q);
hipError_t launch_wide_trans_build(const WideTransParams& Q, hipStream_t st);
hipError_t launch_wide_reduce_attract(const uint32_t* info, const uint64_t* keys, uint64_t m, uint32_t w64, WideSlot* table,
                                      uint64_t slots, unsigned long long* hdr, hipStream_t st);
hipError_t launch_wide_reduce_drain(const WideSlot* table, uint64_t slots, WideAttrRec* out, uint64_t cap, unsigned long long* hdr,
                                    const unsigned long long* ctr, hipStream_t st);
hipError_t launch_wide_reduce_target(const uint32_t* t_hit, uint64_t m, unsigned long long* hist, uint32_t bins,
                                     unsigned long long* hdr, hipStream_t st);

static_assert(sizeof(WideAttrRec) == sizeof(bsx_attr_rec2w), "drained records have the layout of bsx_attr_rec2w");
static_assert(kWideMaxW32 / 2 == BSX_MAX_STATE_WORDS, "key words");

struct WideHost {
    uint32_t n = 0, rows = 0, K = 1, w64 = 0;
    std::vector<uint32_t> pred_offsets, pred_idx, tt_offsets;
    std::vector<uint64_t> tt;
    std::vector<uint32_t> wdesc, wpreds, wtt;
    DevBuf<uint32_t> d_desc, d_wdesc, d_wpreds, d_wtt, d_any, d_fv, d_pv, d_sched, d_x0;
    DevBuf<unsigned long long> d_ctr;
    // device-side reduction (bsx_wide_reduce.hip): grow-only, reused from call to call
    DevBuf<uint32_t> d_info, d_thit;
    DevBuf<uint64_t> d_keys;
    DevBuf<WideSlot> d_table;
    DevBuf<unsigned long long> d_out, d_hist;   // d_out: kHdrWords header words, then the drained records
    // problem space
    bool have_space = false;
    uint32_t origin[kWideMaxW32] = {};
    uint32_t fixmask[kWideMaxW32] = {};     // nodes the origin fixes (constant rules in the descriptors)
    uint32_t n_any = 0, n_fv = 0, n_pv = 0, n_sched = 0, n_fslots = 0, tp_origin = 0;
    uint32_t L = 0;
    size_t shmem = 0;
};

// (BSX_WIDE_HOST_REDUCE=1: per-problem records and hit times are copied back and reduced on the host, chunk by chunk --
// the path before bsx_wide_reduce.hip; kept for A/B runs and tests.)

// Problems per k_wide launch of a chunked run: BSX_WIDE_CHUNK clamped to [32 * L, 2^18], else `dflt`.
static uint64_t wide_chunk(const bsx_engine* h, uint64_t dflt) {
    if (!h->knobs.wide_chunk_set) return dflt;
    return std::max<uint64_t>(32ull * h->wide->L, std::min<uint64_t>(h->knobs.wide_chunk, 1ull << 18));
}

void wide_release(bsx_handle h) {
    delete h->wide;
    h->wide = nullptr;
}

int wide_set_network(bsx_handle h, uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx,
                     const uint32_t* tt_word_offsets, const uint64_t* tt_words) {
    if (n_nodes > BSX_MAX_NODES_WIDE) return fail(h, BSX_ERR_UNSUPPORTED, "more than BSX_MAX_NODES_WIDE nodes");
    HIPCHK(h, hipSetDevice(h->device));
    h->have_net = false;
    h->have_space = false;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        if (pred_offsets[i + 1] < pred_offsets[i]) return fail(h, BSX_ERR_INVALID, "pred_offsets not monotone");
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k > BSX_MAX_PREDECESSORS) return fail(h, BSX_ERR_UNSUPPORTED, "node with more than BSX_MAX_PREDECESSORS predecessors");
        if (k && !pred_idx) return fail(h, BSX_ERR_INVALID, "pred_idx is null");
        for (uint32_t j = pred_offsets[i]; j < pred_offsets[i + 1]; ++j) {
            if (pred_idx[j] >= n_nodes) return fail(h, BSX_ERR_INVALID, "predecessor index out of range");
            if (j > pred_offsets[i] && pred_idx[j] <= pred_idx[j - 1])
                return fail(h, BSX_ERR_INVALID, "predecessors must be strictly ascending");
        }
        const uint32_t need_words = k <= 6 ? 1u : (1u << (k - 6));
        if (tt_word_offsets[i + 1] - tt_word_offsets[i] != need_words)
            return fail(h, BSX_ERR_INVALID, "truth table of a node must have ceil(2^k / 64) words");
    }
    if (!h->wide) h->wide = new WideHost();
    WideHost& W = *h->wide;
    W.n = n_nodes;
    W.rows = (n_nodes + 63) & ~63u;
    W.w64 = (n_nodes + 63) / 64;
    W.pred_offsets.assign(pred_offsets, pred_offsets + n_nodes + 1);
    W.pred_idx.assign(pred_idx, pred_idx + pred_offsets[n_nodes]);
    W.tt_offsets.assign(tt_word_offsets, tt_word_offsets + n_nodes + 1);
    W.tt.assign(tt_words, tt_words + tt_word_offsets[n_nodes]);
    W.wdesc.clear(); W.wpreds.clear(); W.wtt.clear();
    uint32_t K = 1;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k <= 6) { K = std::max(K, k); continue; }
        W.wdesc.push_back(k); W.wdesc.push_back((uint32_t)W.wpreds.size()); W.wdesc.push_back((uint32_t)W.wtt.size());
        for (uint32_t j = pred_offsets[i]; j < pred_offsets[i + 1]; ++j) W.wpreds.push_back(pred_idx[j]);
        for (uint32_t w = tt_word_offsets[i]; w < tt_word_offsets[i + 1]; ++w) {
            W.wtt.push_back((uint32_t)tt_words[w]);
            W.wtt.push_back((uint32_t)(tt_words[w] >> 32));
        }
    }
    W.K = K;
    HIPCHK(h, W.d_wdesc.upload(W.wdesc));
    HIPCHK(h, W.d_wpreds.upload(W.wpreds));
    HIPCHK(h, W.d_wtt.upload(W.wtt));
    HIPCHK(h, W.d_ctr.alloc(4));
    W.have_space = false;
    h->n_nodes = n_nodes;
    h->w64 = W.w64;
    h->net = DevNet{};
    h->net.n_nodes = n_nodes;
    h->net.nw = (n_nodes + 31) / 32;
    h->net.k_mux = K;
    h->lut_mode = BSX_LUT_WIDE;
    h->have_net = true;
    return BSX_OK;
}

int wide_set_problem_space(bsx_handle h, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                           const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                           const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var) {
    WideHost& W = *h->wide;
    const uint32_t n = W.n;
    if (n_any > 64 * BSX_MAX_WORDS)
        return fail(h, BSX_ERR_UNSUPPORTED, "more 'any' nodes than a bsx_index holds (64 * BSX_MAX_WORDS)");
    HIPCHK(h, hipSetDevice(h->device));
    h->have_space = false;
    W.have_space = false;
    std::memset(W.origin, 0, sizeof(W.origin));
    for (uint32_t i = 0; i < n; ++i)
        if ((origin_state_words[i >> 6] >> (i & 63)) & 1ull) W.origin[i >> 5] |= 1u << (i & 31);
    std::vector<uint32_t> any(n_any);
    for (uint32_t j = 0; j < n_any; ++j) {
        if (any_nodes[j] >= n || (j && any_nodes[j] <= any_nodes[j - 1]))
            return fail(h, BSX_ERR_INVALID, "'any' nodes must be ascending node indices");
        any[j] = any_nodes[j];
        W.origin[any[j] >> 5] &= ~(1u << (any[j] & 31));
    }
    std::vector<int> fixed_val(n, -1), slot_of(n, -1);
    for (uint32_t j = 0; j < n_fixed; ++j) {
        if (fixed[j].node >= n || fixed[j].value > 1) return fail(h, BSX_ERR_INVALID, "bad fixed node entry");
        fixed_val[fixed[j].node] = (int)fixed[j].value;
    }
    std::memset(W.fixmask, 0, sizeof(W.fixmask));
    for (uint32_t i = 0; i < n; ++i)
        if (fixed_val[i] >= 0) W.fixmask[i >> 5] |= 1u << (i & 31);
    std::vector<uint32_t> fv, pv;
    uint32_t n_slots = 0;
    for (uint32_t j = 0; j < n_fixed_var; ++j) {
        const uint32_t node = fixed_var[j].node;
        if (node >= n || fixed_var[j].range > 3) return fail(h, BSX_ERR_INVALID, "bad fixed-node variation");
        if (slot_of[node] < 0) slot_of[node] = (int)n_slots++;
        fv.push_back(node); fv.push_back(fixed_var[j].range); fv.push_back((uint32_t)slot_of[node]);
    }
    uint32_t tp_origin = 0, tp_max = 0;
    std::vector<std::array<uint32_t, 3>> ordered;
    for (uint32_t j = 0; j < n_sched; ++j) {
        if (sched[j].node >= n || sched[j].value > 1 || sched[j].t == 0) return fail(h, BSX_ERR_INVALID, "bad perturbation entry");
        tp_origin = std::max(tp_origin, sched[j].t);
        ordered.push_back({sched[j].t, sched[j].node, sched[j].value});
    }
    std::stable_sort(ordered.begin(), ordered.end(), [](const auto& a, const auto& b) { return a[0] < b[0]; });
    std::vector<uint32_t> sch;
    for (const auto& e : ordered) { sch.push_back(e[0]); sch.push_back(e[1]); sch.push_back(e[2]); }
    tp_max = tp_origin;
    for (uint32_t j = 0; j < n_pert_var; ++j) {
        if (pert_var[j].node >= n || pert_var[j].range > 3 || pert_var[j].t == 0) return fail(h, BSX_ERR_INVALID, "bad perturbation variation");
        pv.push_back(pert_var[j].t); pv.push_back(pert_var[j].node); pv.push_back(pert_var[j].range);
        tp_max = std::max(tp_max, pert_var[j].t);
    }
    // row descriptors: K-input mux (tables replicated over unused inputs; origin fixed nodes are constant rules),
    // fixed-variation slot, index of the per-trajectory path for nodes with more than 6 predecessors
    std::vector<uint32_t> desc((size_t)W.rows * kWideDescWords, 0);
    uint32_t wide_at = 0;
    for (uint32_t i = 0; i < W.rows; ++i) {
        uint32_t* d = &desc[(size_t)i * kWideDescWords];
        d[5] = kWideNone;
        d[6] = kWideNone;
        if (i >= n) continue;                   // padding rows: constant 0
        d[5] = slot_of[i] >= 0 ? (uint32_t)slot_of[i] : kWideNone;
        const uint32_t k = W.pred_offsets[i + 1] - W.pred_offsets[i];
        if (k > 6) {
            const uint32_t at = wide_at++;
            if (fixed_val[i] < 0) { d[6] = at; continue; }
        }
        uint64_t bits = 0;
        if (fixed_val[i] >= 0) {
            bits = fixed_val[i] ? ~0ull : 0ull;
        } else {
            const uint64_t t = W.tt[W.tt_offsets[i]];
            for (uint32_t idx = 0; idx < 64; ++idx)
                if ((t >> (idx & ((1u << k) - 1))) & 1ull) bits |= 1ull << idx;
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t p = W.pred_idx[W.pred_offsets[i] + j];
                d[j >> 1] |= p << (16 * (j & 1));
            }
        }
        d[3] = (uint32_t)bits;
        d[4] = (uint32_t)(bits >> 32);
    }
    HIPCHK(h, W.d_desc.upload(desc));
    HIPCHK(h, W.d_any.upload(any));
    HIPCHK(h, W.d_fv.upload(fv));
    HIPCHK(h, W.d_pv.upload(pv));
    HIPCHK(h, W.d_sched.upload(sch));
    W.n_any = n_any; W.n_fv = n_fixed_var; W.n_pv = n_pert_var; W.n_sched = (uint32_t)ordered.size();
    W.n_fslots = n_slots; W.tp_origin = tp_origin;
    // columns per group: the largest power of two <= 64 whose four matrices and tables fit the LDS
    W.L = 0;
    for (uint32_t L = 64; L >= 4; L >>= 1) {
        const size_t bytes = (size_t)wide_lds_words(W.rows, L, W.n_fslots, W.n_pv) * 4;
        if (bytes <= 159 * 1024) { W.L = L; W.shmem = bytes; break; }
    }
    if (!W.L) return fail(h, BSX_ERR_UNSUPPORTED, "wide network: state matrices do not fit the LDS");
    // the fields of the handle that the range checks of bsx_host.h read
    h->sp = DevSpace{};
    h->sp.n_any = n_any;
    {
        unsigned __int128 v = 1;
        auto times = [&](uint32_t range) { if (v <= UINT64_MAX) v *= (range == BSX_RANGE_MAYBE_TRUE_OR_FALSE ? 3u : 2u); };
        for (uint32_t j = 0; j < n_fixed_var; ++j) times(fixed_var[j].range);
        for (uint32_t j = 0; j < n_pert_var; ++j) times(pert_var[j].range);
        h->variant_count_saturated = v > UINT64_MAX;
        h->variant_count = h->variant_count_saturated ? UINT64_MAX : (uint64_t)v;
    }
    h->tp_max = tp_max;
    W.have_space = true;
    h->have_space = true;
    return BSX_OK;
}

// Enqueues one k_wide launch over [first, first + count) (count problems, or the listed offsets) on the engine's
// stream and returns without waiting; the caller fills the parameter fields of the mode's sinks before.  The kernel
// ADDS to the counters in W.d_ctr: the caller zeroes them once, in front of its first launch.
static int wide_enqueue(bsx_handle h, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t) {
    WideHost& W = *h->wide;
    P.n_nodes = W.n; P.rows = W.rows; P.L = W.L;
    P.lshift = (uint32_t)__builtin_ctz(W.L);
    P.rows_ps = W.rows / (kWideThreads / W.L);
    P.w64 = W.w64;
    P.desc = W.d_desc.p; P.wdesc = W.d_wdesc.p; P.wpreds = W.d_wpreds.p; P.wtt = W.d_wtt.p;
    for (int w = 0; w < 4; ++w) P.first_digits[w] = first->init_digits[w];
    P.first_variant = first->variant;
    std::memcpy(P.origin, W.origin, sizeof(P.origin));
    P.n_any = W.n_any; P.n_fv = W.n_fv; P.n_pv = W.n_pv; P.n_sched = W.n_sched; P.n_fslots = W.n_fslots;
    P.tp_origin = W.tp_origin;
    P.any_nodes = W.d_any.p; P.fv = W.d_fv.p; P.pv = W.d_pv.p; P.sched = W.d_sched.p;
    P.count = count;
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;        // kWideStepLimit unless BSX_WIDE_STEP_LIMIT says less
    if (W.wdesc.empty()) P.wdesc = nullptr;
    P.ctr = W.d_ctr.p;
    const uint32_t G = 32 * W.L;
    const uint64_t groups = (count + G - 1) / G;
    const uint32_t per_cu = std::max<uint32_t>(1, (uint32_t)((160 * 1024) / W.shmem));
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(groups, (uint64_t)h->prop.multiProcessorCount * per_cu));
    if (P.mode == kWideAttract) {
        // (grow-only: a chunked run's first launch is its largest, so the buffer never moves under a queued launch)
        HIPCHK(h, W.d_x0.reserve((size_t)blocks * W.rows * W.L));
        P.x0 = W.d_x0.p;
    }
    HIPCHK(h, launch_wide((int)W.K, dim3((uint32_t)blocks), W.shmem, h->stream, P));
    return BSX_OK;
}

// One launch, waited for: its counters and its device time.
static int wide_launch(bsx_handle h, WideParams& P, const bsx_index* first, uint64_t count, uint64_t max_t,
                       unsigned long long (&ctr)[4], float& ms) {
    WideHost& W = *h->wide;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = wide_enqueue(h, P, first, count, max_t)) return rc;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    return BSX_OK;
}

static void put_stats(bsx_stats* stats, uint64_t problems, const unsigned long long (&ctr)[4], float ms, uint32_t launches,
                      double t_begin) {
    if (!stats) return;
    stats->problems = problems;
    stats->state_steps = ctr[0];
    stats->executed_steps = ctr[1];
    stats->kernel_ms = ms;
    stats->kernel_launches = launches;
    stats->total_ms = now_ms() - t_begin;
}

static int wide_sim(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* offsets,
                    const uint64_t* t_len, const uint64_t* out_offsets, uint64_t traj_words, uint64_t* trajectories,
                    uint64_t* final_states, uint64_t* digests, bsx_stats* stats) {
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (max_t >= kStepLimit) return fail(h, BSX_ERR_UNSUPPORTED, "simulation length above the engine's step limit");
    HIPCHK(h, hipSetDevice(h->device));
    const uint32_t w64 = h->wide->w64;
    DevBuf<uint64_t> d_traj, d_final, d_dig, d_off, d_tlen, d_ooff;
    WideParams P{};
    P.mode = kWideSimulate;
    if (trajectories) { HIPCHK(h, d_traj.alloc(traj_words)); P.traj = d_traj.p; }
    if (final_states) { HIPCHK(h, d_final.alloc(count * w64)); P.final_states = d_final.p; }
    if (digests) { HIPCHK(h, d_dig.alloc(count)); P.digests = d_dig.p; }
    if (offsets) {
        HIPCHK(h, d_off.upload(std::vector<uint64_t>(offsets, offsets + count))); P.offsets = d_off.p;
        HIPCHK(h, d_tlen.upload(std::vector<uint64_t>(t_len, t_len + count))); P.t_len = d_tlen.p;
        HIPCHK(h, d_ooff.upload(std::vector<uint64_t>(out_offsets, out_offsets + count))); P.out_offsets = d_ooff.p;
    }
    unsigned long long ctr[4];
    float ms = 0.f;
    if (int rc = wide_launch(h, P, first, count, max_t, ctr, ms)) return rc;
    if (trajectories) HIPCHK(h, hipMemcpy(trajectories, d_traj.p, traj_words * 8, hipMemcpyDeviceToHost));
    if (final_states) HIPCHK(h, hipMemcpy(final_states, d_final.p, count * w64 * 8, hipMemcpyDeviceToHost));
    if (digests) HIPCHK(h, hipMemcpy(digests, d_dig.p, count * 8, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr, ms, 1, t_begin);
    return BSX_OK;
}

int wide_run_simulate(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, uint64_t* trajectories,
                      uint64_t* final_states, uint64_t* digests, bsx_stats* stats) {
    return wide_sim(h, first, count, max_t, nullptr, nullptr, nullptr, trajectories ? count * (max_t + 1) * h->w64 : 0,
                    trajectories, final_states, digests, stats);
}

int wide_run_trajectories(bsx_handle h, const bsx_index* first, const uint64_t* offsets, const uint64_t* t_len, uint64_t n,
                          uint64_t* out, const uint64_t* out_offsets, bsx_stats* stats) {
    uint64_t words = 0, tmax = 0;
    for (uint64_t q = 0; q < n; ++q) {
        words = std::max(words, out_offsets[q] + (t_len[q] + 1) * h->w64);
        tmax = std::max(tmax, t_len[q]);
    }
    return wide_sim(h, first, n, tmax, offsets, t_len, out_offsets, words, out, nullptr, nullptr, stats);
}

// bsx_run_attractor_profile on the wide family (bsx_profile_api.cpp has checked every argument): one k_wide_profile
// launch per BSX_PROFILE_CHUNK_WIDE attractors, all enqueued before the one wait.
// keep_states (as profile_lanes): states and closure are written whether or not the caller wants them on the host and
// every device buffer of the call stays in *keep_states; the launches are enqueued and NOT waited for, nothing is
// copied back and `stats` is not written (the wide attractor transitions go on enqueueing behind them).
int wide_run_profile(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths, uint64_t n,
                     uint32_t* on_counts, uint64_t* states, const uint64_t* state_offsets, uint64_t state_words, uint8_t* closed,
                     uint64_t sum_len, bsx_stats* stats, DevBuf<uint32_t>* keep_on, ProfileKeep* keep_states) {
    static_assert(BSX_PROFILE_CHUNK_WIDE % (32 * 64) == 0, "a chunk is whole groups for every L");
    const double t_begin = now_ms();
    WideHost& W = *h->wide;
    if (W.rows / (kWideThreads / W.L) > kWideProfileRows)      // (before any device work, as every check of this call)
        return fail(h, BSX_ERR_UNSUPPORTED, "wide profile: more rows per thread than the kernel holds");
    ProfileKeep here;
    ProfileKeep& kept = keep_states ? *keep_states : here;
    DevBuf<uint64_t>&d_keys = kept.keys, &d_len = kept.lengths, &d_off = kept.offsets, &d_states = kept.states;
    DevBuf<uint32_t> d_on_here;
    DevBuf<uint32_t>& d_on = keep_on ? *keep_on : d_on_here;   // (keep_on: counted in any case, and left there)
    const bool count_on = on_counts || keep_on;
    DevBuf<uint8_t>& d_closed = kept.closed;
    const bool want_states = states || keep_states, want_closed = closed || keep_states;
    HIPCHK(h, d_keys.alloc(n * key_stride));
    HIPCHK(h, hipMemcpy(d_keys.p, keys, n * key_stride * 8, hipMemcpyHostToDevice));
    HIPCHK(h, d_len.alloc(n));
    HIPCHK(h, hipMemcpy(d_len.p, lengths, n * 8, hipMemcpyHostToDevice));
    if (want_states) {
        HIPCHK(h, d_off.alloc(n));
        HIPCHK(h, hipMemcpy(d_off.p, state_offsets, n * 8, hipMemcpyHostToDevice));
        HIPCHK(h, d_states.alloc(state_words));
    }
    if (count_on) {
        HIPCHK(h, d_on.alloc(n * W.n));
        HIPCHK(h, hipMemsetAsync(d_on.p, 0, n * W.n * sizeof(uint32_t), h->stream));
    }
    if (want_closed) HIPCHK(h, d_closed.alloc(n));

    WideProfileParams Q{};
    WideParams& P = Q.net;
    P.n_nodes = W.n; P.rows = W.rows; P.L = W.L;
    P.lshift = (uint32_t)__builtin_ctz(W.L);
    P.rows_ps = W.rows / (kWideThreads / W.L);
    P.w64 = W.w64;
    P.desc = W.d_desc.p; P.wdesc = W.wdesc.empty() ? nullptr : W.d_wdesc.p; P.wpreds = W.d_wpreds.p; P.wtt = W.d_wtt.p;
    P.n_fslots = W.n_fslots;
    Q.key_stride = key_stride;
    Q.states = want_states ? d_states.p : nullptr;
    Q.ctr = W.d_ctr.p;
    const size_t shmem = (size_t)wide_profile_lds_words(W.rows, W.L, W.n_fslots) * 4;
    const uint32_t G = 32 * W.L;
    const uint32_t per_cu = std::max<uint32_t>(1, (uint32_t)((160 * 1024) / shmem));
    uint32_t launches = 0;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (uint64_t at = 0; at < n; at += BSX_PROFILE_CHUNK_WIDE, ++launches) {
        const uint64_t m = std::min<uint64_t>(BSX_PROFILE_CHUNK_WIDE, n - at);
        Q.count = m;
        Q.keys = d_keys.p + at * key_stride;
        Q.lengths = d_len.p + at;
        Q.state_offsets = want_states ? d_off.p + at : nullptr;
        Q.on_counts = count_on ? d_on.p + at * W.n : nullptr;
        Q.closed = want_closed ? d_closed.p + at : nullptr;
        const uint64_t groups = (m + G - 1) / G;
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(groups, (uint64_t)h->prop.multiProcessorCount * per_cu));
        HIPCHK(h, launch_wide_profile((int)W.K, dim3((uint32_t)blocks), shmem, h->stream, Q));
    }
    if (keep_states) {
        keep_states->launches = launches;
        return BSX_OK;
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    unsigned long long ctr[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (on_counts) HIPCHK(h, hipMemcpy(on_counts, d_on.p, n * W.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (states && state_words) HIPCHK(h, hipMemcpy(states, d_states.p, state_words * 8, hipMemcpyDeviceToHost));
    if (closed) HIPCHK(h, hipMemcpy(closed, d_closed.p, n, hipMemcpyDeviceToHost));
    ctr[0] = sum_len;
    put_stats(stats, n, ctr, ms, launches, t_begin);
    return BSX_OK;
}

// target: first hit time per problem into t_hit (kWideNone = none)
int wide_target_times(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                      const uint64_t* code_words, std::vector<uint32_t>& t_hit, bsx_stats* stats) {
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    t_hit.assign(count, kWideNone);
    if (count == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    WideParams P{};
    P.mode = kWideTarget;
    for (uint32_t i = 0; i < h->wide->n; ++i) {
        if ((mask_words[i >> 6] >> (i & 63)) & 1ull) P.tmask[i >> 5] |= 1u << (i & 31);
        if ((code_words[i >> 6] >> (i & 63)) & 1ull) P.tcode[i >> 5] |= 1u << (i & 31);
    }
    DevBuf<uint32_t> d_thit;
    HIPCHK(h, d_thit.alloc(count));
    HIPCHK(h, hipMemset(d_thit.p, 0xFF, count * 4));
    P.t_hit = d_thit.p;
    unsigned long long ctr[4];
    float ms = 0.f;
    if (int rc = wide_launch(h, P, first, count, max_t, ctr, ms)) return rc;
    HIPCHK(h, hipMemcpy(t_hit.data(), d_thit.p, count * 4, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr, ms, 1, t_begin);
    if (ctr[2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    return BSX_OK;
}

// target summary on the device: k_wide_reduce_target counts and bins every chunk's t_hit right behind the k_wide
// launch that wrote it.  A chunk's t_hit is copied to the host only while the caller's hit list has room; with
// cap == 0, or once the list is full, the host waits once, at the end.  (The caller, bsx_run_target_summary, has
// checked the arguments and zeroed the outputs; count > 0.)  Chunks are 2^24 problems, or BSX_WIDE_CHUNK.
int wide_target_summary(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t, const uint64_t* mask_words,
                        const uint64_t* code_words, uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                        uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats) {
    const double t_begin = now_ms();
    WideHost& W = *h->wide;
    WideParams P0{};
    P0.mode = kWideTarget;
    for (uint32_t i = 0; i < W.n; ++i) {
        if ((mask_words[i >> 6] >> (i & 63)) & 1ull) P0.tmask[i >> 5] |= 1u << (i & 31);
        if ((code_words[i >> 6] >> (i & 63)) & 1ull) P0.tcode[i >> 5] |= 1u << (i & 31);
    }
    const uint64_t chunk = std::min<uint64_t>(count, wide_chunk(h, 1ull << 24));
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
        const bsx_index at = index_plus(*first, done, h->sp.n_any);
        HIPCHK(h, hipMemsetAsync(W.d_thit.p, 0xFF, m * 4, h->stream));
        if (!timing) { HIPCHK(h, hipEventRecord(h->ev0, h->stream)); timing = true; }
        WideParams P = P0;
        P.t_hit = W.d_thit.p;
        if (int rc = wide_enqueue(h, P, &at, m, max_t)) return rc;
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
    if (stats) {
        stats->problems = count;
        stats->state_steps = ctr[0];
        stats->executed_steps = ctr[1];
        stats->kernel_ms = kms;                 // HIP events around each run of launches the host waited for
        stats->kernel_launches = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    if (ctr[2]) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit");
    for (uint32_t b = 0; b < hist_bins; ++b) hist[b] = bins[b];
    *n_hits = hdr[kHdrHits];
    std::copy(list.begin(), list.end(), hits);
    if (n_listed) *n_listed = listed;
    return BSX_OK;
}

}  // namespace bsx

using namespace bsx;

// ---- attract over wide records: the kernel's per-problem results, aggregated by key
// Device path: k_wide and k_wide_reduce_attract are enqueued for every chunk back to back (one info / keys buffer:
// the stream orders them), k_wide_reduce_drain packs the table, and the host waits once.  The first
// kInlineRecs records come back with the header in that one copy; a table with more costs a second copy.
static constexpr uint32_t kInlineRecs = 256;

static int attract_wide_device(bsx_handle h, const bsx_index& first, uint64_t count, uint64_t chunk, uint64_t max_t,
                               uint64_t max_len, bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out,
                               bsx_u128* n_no_attractor, bsx_stats2* stats, double t_begin) {
    WideHost& W = *h->wide;
    const uint32_t n_any = h->sp.n_any;
    // a range of `count` problems has at most `count` attractors: the device structures follow the smaller of the two,
    // so a caller's very large cap ("no limit") costs nothing
    const uint64_t dcap = std::min<uint64_t>(cap, count);
    uint64_t slots = kWideReduceMinSlots;
    while (slots < 2 * dcap) slots <<= 1;
    constexpr size_t kRecWords = sizeof(WideAttrRec) / 8;
    HIPCHK(h, W.d_info.reserve(chunk * 4));
    HIPCHK(h, W.d_keys.reserve(chunk * W.w64));
    HIPCHK(h, W.d_table.reserve(slots));
    HIPCHK(h, W.d_out.reserve(kHdrWords + (size_t)std::max<uint64_t>(dcap, 1) * kRecWords));
    unsigned long long* d_hdr = W.d_out.p;
    WideAttrRec* d_recs = reinterpret_cast<WideAttrRec*>(W.d_out.p + kHdrWords);
    HIPCHK(h, hipMemsetAsync(W.d_table.p, 0, slots * sizeof(WideSlot), h->stream));
    HIPCHK(h, hipMemsetAsync(d_hdr, 0, kHdrWords * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    uint32_t wide_launches = 0;
    for (uint64_t done = 0; done < count; done += chunk) {
        const uint64_t m = std::min(chunk, count - done);
        const bsx_index at = index_plus(first, done, n_any);
        WideParams P{};
        P.mode = kWideAttract;
        P.info = W.d_info.p;
        P.keys = W.d_keys.p;
        P.max_len = max_len;
        if (int rc = wide_enqueue(h, P, &at, m, max_t)) return rc;
        HIPCHK(h, launch_wide_reduce_attract(W.d_info.p, W.d_keys.p, m, W.w64, W.d_table.p, slots, d_hdr, h->stream));
        ++wide_launches;
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
    if (stats) {
        stats->problems = bsx_u128{count, 0};
        stats->state_steps = bsx_u128{hdr[kHdrCtr + 0], 0};
        stats->executed_steps = hdr[kHdrCtr + 1];
        stats->kernel_ms = ms;                  // HIP events around the whole chain of launches
        stats->dominant_ms = ms;
        stats->dominant_executed_steps = hdr[kHdrCtr + 1];
        stats->dominant_launches = wide_launches;
        stats->kernel_launches = 2 * wide_launches + 1;
        stats->host_syncs = syncs;
        stats->total_ms = now_ms() - t_begin;
    }
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
    // flat index -> bsx_index: the low n_any bits are the initial-state digits, the rest is the variant
    const uint32_t n_any = h->sp.n_any;
    bsx_index first{};
    const u128 flat = ((u128)first_flat.hi << 64) | first_flat.lo;
    if (n_any >= 128) {
        first.init_digits[0] = first_flat.lo; first.init_digits[1] = first_flat.hi;
    } else {
        const u128 digits = n_any ? (flat & ((((u128)1) << n_any) - 1)) : 0;
        const u128 variant = flat >> n_any;
        if (variant >> 64) return fail(h, BSX_ERR_INVALID, "first lies beyond the problem space");
        first.init_digits[0] = (uint64_t)digits; first.init_digits[1] = (uint64_t)(digits >> 64);
        first.variant = (uint64_t)variant;
    }
    if (int rc = check_range(h, &first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    if (count == 0) return BSX_OK;
    HIPCHK(h, hipSetDevice(h->device));
    WideHost& W = *h->wide;
    const uint64_t chunk = std::min<uint64_t>(count, wide_chunk(h, 1ull << 18));
    // (more than kWideReduceMaxCap possible attractors: the device table would take gigabytes; such a call is reduced
    // on the host, which allocates per attractor found)
    if (!h->knobs.wide_host_reduce && std::min<uint64_t>(cap, count) <= kWideReduceMaxCap) return attract_wide_device(h, first, count, chunk, max_t, max_len, table, cap, n_out, n_no_attractor, stats, t_begin);
    // BSX_WIDE_HOST_REDUCE=1 (or a table beyond kWideReduceMaxCap): every chunk's records come back and are aggregated here by key
    DevBuf<uint32_t> d_info;
    DevBuf<uint64_t> d_keys;
    HIPCHK(h, d_info.alloc(chunk * 4));
    HIPCHK(h, d_keys.alloc(chunk * W.w64));
    std::vector<uint32_t> info(chunk * 4);
    std::vector<uint64_t> keys(chunk * W.w64);
    struct Agg { uint64_t length = 0; u128 count = 0, sl = 0, sl2 = 0; };
    std::map<std::array<uint64_t, BSX_MAX_STATE_WORDS>, Agg> agg;
    u128 none = 0, ref_steps = 0;
    uint64_t exec = 0;
    double kms = 0;
    uint32_t launches = 0;
    bool limit = false;
    for (uint64_t done = 0; done < count; done += chunk) {
        const uint64_t m = std::min(chunk, count - done);
        const bsx_index at = index_plus(first, done, n_any);
        WideParams P{};
        P.mode = kWideAttract;
        P.info = d_info.p;
        P.keys = d_keys.p;
        P.max_len = max_len;
        unsigned long long ctr[4];
        float ms = 0.f;
        if (int rc = wide_launch(h, P, &at, m, max_t, ctr, ms)) return rc;
        HIPCHK(h, hipMemcpy(info.data(), d_info.p, m * 16, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(keys.data(), d_keys.p, m * W.w64 * 8, hipMemcpyDeviceToHost));
        kms += ms; ++launches; exec += ctr[1]; ref_steps += ctr[0];
        limit = limit || ctr[2];
        for (uint64_t q = 0; q < m; ++q) {
            if (!info[4 * q]) { ++none; continue; }
            std::array<uint64_t, BSX_MAX_STATE_WORDS> k{};
            for (uint32_t w = 0; w < W.w64; ++w) k[w] = keys[q * W.w64 + w];
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
    if (stats) {
        stats->problems = bsx_u128{count, 0};
        stats->state_steps = bsx_u128{(uint64_t)ref_steps, (uint64_t)(ref_steps >> 64)};
        stats->executed_steps = exec;
        stats->kernel_ms = kms;
        stats->dominant_ms = kms;
        stats->dominant_executed_steps = exec;
        stats->dominant_launches = launches;
        stats->kernel_launches = launches;
        stats->host_syncs = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}

// ---- attractor transitions on the wide family -----------------------------------------------------------------------
// Host side of bsx_run_attractor_transitions_wide: argument checks, allocation, the enqueue chain
//     profile (states and closure stay in HBM) -> k_wide_trans over the rows -> k_wide_trans_build ->
//     k_wide_trans over the flips, BSX_WTRANS_CHUNK per launch -> k_trans_drain,
// one wait, the flags -> status mapping and the sort of the edge list, as bsx_trans_api.cpp does for the <= 256 family.
static_assert(kWtransOutside == kTransOutside && kWtransUnresolved == kTransUnresolved, "the pseudo-destinations");
static_assert(kWtransInf == BSX_T_INF, "no cap");
constexpr uint64_t kWideTransRowChunk = 1ull << 18;     // rows per launch of the rows' walks
constexpr uint64_t kWideTransFlipChunk = 1ull << 22;    // flips per launch (BSX_WTRANS_CHUNK)

extern "C" int bsx_run_attractor_transitions_wide(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                                  uint64_t n, uint64_t max_t, bsx_trans_edge* edges, uint64_t edge_cap,
                                                  uint64_t* n_edges, uint32_t* node_exits, uint8_t* closed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!h->wide) return bsx_run_attractor_transitions(h, keys, key_stride, lengths, n, max_t, edges, edge_cap, n_edges, node_exits, closed, stats);
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    const std::string who = "bsx_run_attractor_transitions_wide";
    uint64_t sum_len = 0, unused = 0;
    if (int rc = profile_check_args(h, who.c_str(), keys, key_stride, lengths, n, nullptr, nullptr, &sum_len, &unused)) return rc;
    if (!edges || !n_edges) return fail(h, BSX_ERR_INVALID, who + ": edges or n_edges is null");
    if (n > 0xFFFFFFFDull) return fail(h, BSX_ERR_INVALID, who + ": more than 2^32 - 3 attractors");
    if (sum_len > kTransMaxStates) return fail(h, BSX_ERR_UNSUPPORTED, who + ": more than 2^28 cycle states (BSX_TRANS_MAX_STATES)");
    WideHost& W = *h->wide;
    const size_t shmem = (size_t)wide_trans_lds_words(W.rows, W.L, W.n_fslots) * 4;
    if (shmem > W.shmem || (size_t)W.rows * W.L * 4 < kTransLdsEdges * sizeof(TransEdgeSlot))
        return fail(h, BSX_ERR_UNSUPPORTED, who + ": the group's tables do not fit the LDS");
    HIPCHK(h, hipSetDevice(h->device));

    const uint32_t w64 = W.w64, n_nodes = W.n;
    std::vector<uint32_t> free_nodes;
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (!((W.fixmask[i >> 5] >> (i & 31)) & 1u)) free_nodes.push_back(i);
    const uint32_t n_free = (uint32_t)free_nodes.size();
    const uint64_t flips = sum_len * n_free;                            // (< 2^28 * 2^10)

    // the profile: states (row after row, the key first) and closure stay on the device; enqueued, not waited for
    std::vector<uint64_t> offsets(n), row_first(n);
    for (uint64_t q = 0, at = 0; q < n; at += lengths[q], ++q) { row_first[q] = at; offsets[q] = at * w64; }
    ProfileKeep kept;
    if (int rc = wide_run_profile(h, keys, key_stride, lengths, n, nullptr, nullptr, offsets.data(), sum_len * w64, nullptr, sum_len,
                                  nullptr, nullptr, &kept))
        return rc;

    // row-key table: a power of two >= 2 n owners (at least 2); edge table as in bsx_trans_api.cpp
    uint64_t n_slots = 2;
    while (n_slots < 2 * n) n_slots <<= 1;
    const uint64_t most_edges = n >= (1ull << 31) ? ~0ull : n * (n + 2);
    const uint64_t out_cap = std::min({edge_cap, flips, most_edges});
    uint64_t edge_slots = 2;
    while (edge_slots < 2 * (out_cap + 1)) edge_slots <<= 1;           // (+ 1: one edge too many must still find a slot)
    const uint64_t flip_chunk = h->knobs.wtrans_chunk ? std::min<uint64_t>(h->knobs.wtrans_chunk, 1ull << 28) : kWideTransFlipChunk;

    // workgroups of a launch over `count` trajectories; the x_0 spill takes rows * L words per workgroup
    const uint32_t G = 32 * W.L;
    const uint32_t per_cu = std::max<uint32_t>(1, (uint32_t)((160 * 1024) / shmem));
    auto blocks_for = [&](uint64_t count) {
        return std::max<uint64_t>(1, std::min<uint64_t>((count + G - 1) / G, (uint64_t)h->prop.multiProcessorCount * per_cu));
    };
    const uint64_t most_blocks = std::max(blocks_for(std::min(n, kWideTransRowChunk)), blocks_for(std::min(std::max<uint64_t>(flips, 1), flip_chunk)));

    DevBuf<uint64_t> d_row_first, d_row_keys;
    DevBuf<uint32_t> d_owners, d_row_info, d_free, d_exits, d_x0;
    DevBuf<TransEdgeSlot> d_edges;
    DevBuf<TransEdge> d_out;
    DevBuf<TransCtr> d_tc;
    HIPCHK(h, d_row_first.upload(row_first));
    HIPCHK(h, d_free.upload(free_nodes));
    HIPCHK(h, d_row_keys.alloc(n * w64));
    HIPCHK(h, d_row_info.alloc(2 * n));
    HIPCHK(h, d_owners.alloc(n_slots));
    HIPCHK(h, d_x0.alloc((size_t)most_blocks * W.rows * W.L));
    HIPCHK(h, d_edges.alloc(edge_slots));
    HIPCHK(h, d_out.alloc(out_cap));
    HIPCHK(h, d_tc.alloc(1));
    if (node_exits) HIPCHK(h, d_exits.alloc(n * n_nodes));
    TransCtr tc{};
    tc.open_row = tc.dup_row = kTransNoRow;
    HIPCHK(h, hipMemcpyAsync(d_tc.p, &tc, sizeof(tc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_owners.p, 0, n_slots * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d_edges.p, 0, edge_slots * sizeof(TransEdgeSlot), h->stream));
    if (node_exits) HIPCHK(h, hipMemsetAsync(d_exits.p, 0, n * n_nodes * sizeof(uint32_t), h->stream));

    WideTransParams Q{};
    WideParams& P = Q.net;
    P.n_nodes = W.n; P.rows = W.rows; P.L = W.L;
    P.lshift = (uint32_t)__builtin_ctz(W.L);
    P.rows_ps = W.rows / (kWideThreads / W.L);
    P.w64 = w64;
    P.desc = W.d_desc.p; P.wdesc = W.wdesc.empty() ? nullptr : W.d_wdesc.p; P.wpreds = W.d_wpreds.p; P.wtt = W.d_wtt.p;
    P.n_fslots = W.n_fslots;
    P.max_t = max_t;
    P.cap_inf = max_t == BSX_T_INF ? 1u : 0u;
    P.step_limit = h->knobs.wide_step_limit;
    P.x0 = d_x0.p;
    Q.key_stride = key_stride;
    Q.n_rows = n;
    Q.keys = kept.keys.p;
    Q.lengths = kept.lengths.p;
    Q.closed = kept.closed.p;
    Q.states = kept.states.p;
    Q.row_first = d_row_first.p;
    Q.free_nodes = d_free.p;
    Q.n_free = n_free;
    Q.row_info = d_row_info.p;
    Q.row_keys = d_row_keys.p;
    Q.owners = d_owners.p;
    Q.slot_mask = n_slots - 1;
    Q.edges = d_edges.p;
    Q.edge_mask = edge_slots - 1;
    Q.node_exits = node_exits ? d_exits.p : nullptr;
    Q.ctr = d_tc.p;

    uint32_t launches = kept.launches;
    Q.stage = kWideTransRows;
    for (uint64_t at = 0; at < n; at += kWideTransRowChunk, ++launches) {
        Q.first = at;
        Q.count = std::min<uint64_t>(kWideTransRowChunk, n - at);
        HIPCHK(h, launch_wide_trans((int)W.K, dim3((uint32_t)blocks_for(Q.count)), shmem, h->stream, Q));
    }
    HIPCHK(h, launch_wide_trans_build(Q, h->stream));
    ++launches;
    Q.stage = kWideTransFlips;
    for (uint64_t at = 0; at < flips; at += flip_chunk, ++launches) {
        Q.first = at;
        Q.count = std::min<uint64_t>(flip_chunk, flips - at);
        HIPCHK(h, launch_wide_trans((int)W.K, dim3((uint32_t)blocks_for(Q.count)), shmem, h->stream, Q));
    }
    HIPCHK(h, launch_trans_drain(d_edges.p, edge_slots, d_out.p, out_cap, d_tc.p, h->stream));
    ++launches;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));                       // (ev0: wide_run_profile, in front of its first launch)
    unsigned long long ctr[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&tc, d_tc.p, sizeof(tc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                         // the call's one wait

    if (tc.open_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.open_row) + " is not closed: its key does not return after its length");
    if (tc.dup_row != kTransNoRow)
        return fail(h, BSX_ERR_INVALID, who + ": row " + std::to_string(tc.dup_row) + " lies on the cycle of another row or repeats its own "
                                              "(a duplicate row, or a length that is a multiple of the period)");
    if (tc.probe_full) return fail(h, BSX_ERR_HIP, who + ": the row-key table overflowed");
    if (tc.step_limit_hits || tc.rows_undecided) return fail(h, BSX_ERR_STEP_LIMIT, who + ": a walk ran into the internal step limit");
    if (tc.edge_overflow || tc.n_edges > edge_cap)
        return fail(h, BSX_ERR_TABLE_FULL, who + ": more distinct edges than edge_cap");
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    std::vector<TransEdge> got(tc.n_edges);
    if (tc.n_edges) HIPCHK(h, hipMemcpy(got.data(), d_out.p, tc.n_edges * sizeof(TransEdge), hipMemcpyDeviceToHost));
    std::sort(got.begin(), got.end(), [](const TransEdge& a, const TransEdge& b) { return a.src != b.src ? a.src < b.src : a.dst < b.dst; });
    uint64_t sum_mu = 0;
    for (uint64_t e = 0; e < tc.n_edges; ++e) {
        edges[e] = bsx_trans_edge{got[e].src, got[e].dst, got[e].count, got[e].sum_mu};
        sum_mu += got[e].sum_mu;
    }
    *n_edges = tc.n_edges;
    if (node_exits) HIPCHK(h, hipMemcpy(node_exits, d_exits.p, n * n_nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (closed) HIPCHK(h, hipMemcpy(closed, kept.closed.p, n, hipMemcpyDeviceToHost));
    if (stats) {
        stats->problems = flips;
        stats->state_steps = sum_mu;
        stats->executed_steps = ctr[1] + tc.steps_exec;
        stats->kernel_ms = ms;
        stats->kernel_launches = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}
