// bsx_run_attractor_profile (include/bsx.h): states, per-node on-counts and closure of listed attractors in one
// batched call.  Everything the kernels index with is checked here, before anything is launched; the handle's problem
// space and cycle journal are not touched.  Kernels: bsx_profile.hip (n <= 256), k_wide_profile in bsx_wide.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "bsx_engine.h"
#include "bsx_host.h"

using namespace bsx;

namespace {

// attractors per launch of the per-lane kernel (BSX_PROFILE_CHUNK in include/bsx.h): below it a call is one launch
constexpr uint64_t kProfileChunk = 1ull << 22;
static_assert(kProfileChunk == BSX_PROFILE_CHUNK, "the header states the chunk size");

}  // namespace

namespace bsx {

// keep_on: the on-counts are counted whether or not the caller wants them on the host, and stay in *keep_on
// keep_states: states and closure are written whether or not the caller wants them on the host, and every device
// buffer of the call stays in *keep_states; the launches are enqueued on the handle's stream and NOT waited for, nothing
// is copied back and `stats` is not written (bsx_trans_api.cpp goes on enqueueing behind them)
int profile_lanes(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths, uint64_t n,
                  uint32_t* on_counts, uint64_t* states, const uint64_t* state_offsets, uint64_t state_words,
                  uint8_t* closed, uint64_t sum_len, bsx_stats* stats, double t_begin, DevBuf<uint32_t>* keep_on,
                  ProfileKeep* keep_states) {
    const uint32_t W = h->w64, n_nodes = h->n_nodes;
    ProfileKeep here;
    ProfileKeep& kept = keep_states ? *keep_states : here;
    DevBuf<uint64_t>&d_keys = kept.keys, &d_len = kept.lengths, &d_off = kept.offsets, &d_states = kept.states;
    DevBuf<uint32_t> d_on_here;
    DevBuf<uint32_t>& d_on = keep_on ? *keep_on : d_on_here;
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
        HIPCHK(h, d_on.alloc(n * n_nodes));
        HIPCHK(h, hipMemsetAsync(d_on.p, 0, n * n_nodes * sizeof(uint32_t), h->stream));
    }
    if (want_closed) HIPCHK(h, d_closed.alloc(n));

    ProfileParams P{};
    P.net = h->net;
    for (int w = 0; w < kMaxW32; ++w) { P.fixmask[w] = h->sp.fixmask[w]; P.fixval[w] = h->sp.fixval[w]; }
    P.w64 = W;
    P.key_stride = key_stride;
    P.states = want_states ? d_states.p : nullptr;      // (offsets are relative to the whole buffer in every chunk)
    P.ctr = h->d_ctr;
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    uint32_t launches = 0;
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));    // the launches add to it
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (uint64_t at = 0; at < n; at += kProfileChunk, ++launches) {
        const uint64_t m = std::min<uint64_t>(kProfileChunk, n - at);
        P.count = m;
        P.keys = d_keys.p + at * key_stride;
        P.lengths = d_len.p + at;
        P.state_offsets = want_states ? d_off.p + at : nullptr;
        P.on_counts = count_on ? d_on.p + at * n_nodes : nullptr;
        P.closed = want_closed ? d_closed.p + at : nullptr;
        const uint64_t block = (uint64_t)profile_block((int)h->net.nw);
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 4, (m + block - 1) / block));
        HIPCHK(h, launch_profile((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), h->shmem, h->stream, P));
    }
    if (keep_states) {
        keep_states->launches = launches;
        return BSX_OK;
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    Counters ctr{};
    HIPCHK(h, hipMemcpyAsync(&ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (on_counts) HIPCHK(h, hipMemcpy(on_counts, d_on.p, n * n_nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (states && state_words) HIPCHK(h, hipMemcpy(states, d_states.p, state_words * 8, hipMemcpyDeviceToHost));
    if (closed) HIPCHK(h, hipMemcpy(closed, d_closed.p, n, hipMemcpyDeviceToHost));
    if (stats) {
        stats->problems = n;
        stats->state_steps = sum_len;
        stats->executed_steps = ctr.steps_exec;
        stats->kernel_ms = ms;
        stats->kernel_launches = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}

// Everything bsx_run_attractor_profile checks before it launches (include/bsx.h); `who` names the entry point in the
// error text.  n > 0.  -> sum of the lengths, size of `states` in words.
int profile_check_args(bsx_handle h, const char* who, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                       uint64_t n, const uint64_t* states, const uint64_t* state_offsets, uint64_t* sum_len_out,
                       uint64_t* state_words_out) {
    const std::string name(who);
    if (!keys || !lengths) return fail(h, BSX_ERR_INVALID, name + ": keys or lengths is null");
    if (states && !state_offsets) return fail(h, BSX_ERR_INVALID, name + ": states without state_offsets");
    const uint32_t W = h->w64, n_nodes = h->n_nodes;
    if (key_stride < W) return fail(h, BSX_ERR_INVALID, name + ": key_stride is below the words per state");
    if (n > (1ull << 32)) return fail(h, BSX_ERR_INVALID, "at most 2^32 attractors per call");
    // lengths: 1 <= length, and no walk beyond the family's step limit (the wide family counts lock steps of a group,
    // which makes as many as its longest walk; BSX_WIDE_STEP_LIMIT lowers that limit)
    const uint64_t limit = h->wide ? std::min<uint64_t>(kStepLimit, h->knobs.wide_step_limit) : kStepLimit;
    uint64_t sum_len = 0;
    bool too_long = false;
    for (uint64_t q = 0; q < n; ++q) {
        if (lengths[q] == 0) return fail(h, BSX_ERR_INVALID, name + ": an attractor of length 0");
        too_long = too_long || lengths[q] >= limit;
        if (!too_long) sum_len += lengths[q];
    }
    if (too_long) return fail(h, BSX_ERR_STEP_LIMIT, name + ": a walk would exceed the internal step limit");
    // keys: no bit at or above n_nodes in the words the kernels read
    if (n_nodes & 63u) {
        const uint64_t above = ~0ull << (n_nodes & 63u);
        for (uint64_t q = 0; q < n; ++q)
            if (keys[q * key_stride + (W - 1)] & above)
                return fail(h, BSX_ERR_INVALID, name + ": a key has bits at or above n_nodes");
    }
    // states: the ranges [offset, offset + length * W) must not overlap; their end is the size of the output
    uint64_t state_words = 0;
    if (states) {
        std::vector<uint64_t> order(n);
        std::iota(order.begin(), order.end(), 0ull);
        std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return state_offsets[a] < state_offsets[b]; });
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t off = state_offsets[order[i]], need = lengths[order[i]] * W;     // (< 2^30 * 16)
            if (off < state_words) return fail(h, BSX_ERR_INVALID, name + ": state ranges overlap");
            if (off > (1ull << 56)) return fail(h, BSX_ERR_INVALID, name + ": state offset out of range");
            state_words = off + need;
        }
    }
    *sum_len_out = sum_len;
    *state_words_out = state_words;
    return BSX_OK;
}

}  // namespace bsx

extern "C" int bsx_run_attractor_profile(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                         uint64_t n, uint32_t* on_counts, uint64_t* states, const uint64_t* state_offsets,
                                         uint8_t* closed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    uint64_t sum_len = 0, state_words = 0;
    if (int rc = profile_check_args(h, "bsx_run_attractor_profile", keys, key_stride, lengths, n, states, state_offsets, &sum_len,
                                    &state_words))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->wide)
        return wide_run_profile(h, keys, key_stride, lengths, n, on_counts, states, state_offsets, state_words, closed, sum_len,
                                stats, nullptr);
    return profile_lanes(h, keys, key_stride, lengths, n, on_counts, states, state_offsets, state_words, closed, sum_len, stats,
                         t_begin, nullptr, nullptr);
}
