// bsx_run_attractor_profile (include/bsx.h): states, per-node on-counts and closure of listed attractors in one
// batched call, and the profile stage (bsx_table_host.h) it shares with bsx_run_node_correlations and the transition
// calls.  Everything the kernels index with is checked before anything is launched (bsx_table_lower.h); the handle's
// problem space and cycle journal are not touched.  Kernels: bsx_profile.hip (n <= 256), k_wide_profile in bsx_wide.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bsx_table_host.h"
#include "bsx_wide_host.h"

using namespace bsx;

namespace bsx {

int table_check_args(bsx_handle h, const char* who, const TableView& t, bool want_states, const uint64_t* state_offsets, TableSizes& out) {
    const uint64_t limit = table_step_limit(table_family(h), h->knobs.wide_step_limit);
    if (const LowerStatus s = table_check(t, want_states, state_offsets, h->w64, h->n_nodes, limit, out))
        return fail(h, s.status, std::string(who) + ": " + s.msg);
    if (h->wide && h->wide->net.rows / (kWideThreads / h->wide->space.L) > kWideProfileRows)
        return fail(h, BSX_ERR_UNSUPPORTED, "wide profile: more rows per thread than the kernel holds");
    return BSX_OK;
}

int profile_stage(bsx_handle h, const TableView& t, ProfileWant want, const uint64_t* state_offsets, uint64_t state_words, ProfileDev& dev) {
    dev.want = want;
    dev.state_words = state_words;
    HIPCHK(h, dev.keys.alloc(t.n * t.key_stride));
    HIPCHK(h, hipMemcpy(dev.keys.p, t.keys, t.n * t.key_stride * 8, hipMemcpyHostToDevice));
    HIPCHK(h, dev.lengths.alloc(t.n));
    HIPCHK(h, hipMemcpy(dev.lengths.p, t.lengths, t.n * 8, hipMemcpyHostToDevice));
    if (want.states) {
        HIPCHK(h, dev.offsets.alloc(t.n));
        HIPCHK(h, hipMemcpy(dev.offsets.p, state_offsets, t.n * 8, hipMemcpyHostToDevice));
        HIPCHK(h, dev.states.alloc(state_words));
    }
    if (want.on_counts) {
        HIPCHK(h, dev.on_counts.alloc(t.n * h->n_nodes));
        HIPCHK(h, hipMemsetAsync(dev.on_counts.p, 0, t.n * h->n_nodes * sizeof(uint32_t), h->stream));
    }
    if (want.closed) HIPCHK(h, dev.closed.alloc(t.n));
    return BSX_OK;
}

// The fields of a launch over chunk c that both families' parameter blocks name alike
template <typename Params>
static void profile_fill_chunk(Params& P, const Chunk& c, const TableView& t, const ProfileDev& dev, uint32_t n_nodes) {
    P.count = c.count;
    P.keys = dev.keys.p + c.first * t.key_stride;
    P.lengths = dev.lengths.p + c.first;
    P.state_offsets = dev.want.states ? dev.offsets.p + c.first : nullptr;
    P.on_counts = dev.want.on_counts ? dev.on_counts.p + c.first * n_nodes : nullptr;
    P.closed = dev.want.closed ? dev.closed.p + c.first : nullptr;
}

static int profile_enqueue_lanes(bsx_handle h, const TableView& t, ProfileDev& dev) {
    ProfileParams P{};
    P.net = h->net;
    for (int w = 0; w < kMaxW32; ++w) { P.fixmask[w] = h->sp.fixmask[w]; P.fixval[w] = h->sp.fixval[w]; }
    P.w64 = h->w64;
    P.key_stride = t.key_stride;
    P.states = dev.want.states ? dev.states.p : nullptr;    // (offsets are relative to the whole buffer in every chunk)
    P.ctr = h->d_ctr;
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    const uint64_t block = (uint64_t)profile_block((int)h->net.nw);
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));    // the launches add to it
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (const Chunk c : chunks(t.n, profile_chunk(kTableLanes))) {
        profile_fill_chunk(P, c, t, dev, h->n_nodes);
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 4, (c.count + block - 1) / block));
        HIPCHK(h, launch_profile((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), h->shmem, h->stream, P));
    }
    return BSX_OK;
}

static int profile_enqueue_wide(bsx_handle h, const TableView& t, ProfileDev& dev) {
    static_assert(BSX_PROFILE_CHUNK_WIDE % (32 * 64) == 0, "a chunk is whole groups for every L");
    WideHost& W = *h->wide;
    WideProfileParams Q{};
    wide_fill_net(W, Q.net);
    Q.key_stride = t.key_stride;
    Q.states = dev.want.states ? dev.states.p : nullptr;
    Q.ctr = W.d_ctr.p;
    const size_t shmem = (size_t)wide_profile_lds_words(W.net.rows, W.space.L, W.space.n_fslots) * 4;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (const Chunk c : chunks(t.n, profile_chunk(kTableWide))) {
        profile_fill_chunk(Q, c, t, dev, W.net.n);
        HIPCHK(h, launch_wide_profile((int)W.net.K, dim3((uint32_t)wide_blocks(h, W, c.count, shmem)), shmem, h->stream, Q));
    }
    return BSX_OK;
}

int profile_enqueue(bsx_handle h, const TableView& t, ProfileDev& dev) {
    dev.launches = profile_launches(table_family(h), t.n);
    return h->wide ? profile_enqueue_wide(h, t, dev) : profile_enqueue_lanes(h, t, dev);
}

int profile_collect(bsx_handle h, const TableView& t, const ProfileDev& dev, const ProfileOut& out, uint64_t sum_len, bsx_stats* stats,
                    double t_begin) {
    uint64_t executed = 0;
    float ms = 0.f;
    if (h->wide) {
        unsigned long long ctr[4] = {0, 0, 0, 0};
        if (int rc = wide_timed_wait(h, *h->wide, ctr, ms)) return rc;
        executed = ctr[1];
    } else {
        Counters ctr{};
        if (int rc = lane_timed_wait(h, ctr, ms)) return rc;
        executed = ctr.steps_exec;
    }
    if (out.on_counts) HIPCHK(h, hipMemcpy(out.on_counts, dev.on_counts.p, t.n * h->n_nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out.states && dev.state_words) HIPCHK(h, hipMemcpy(out.states, dev.states.p, dev.state_words * 8, hipMemcpyDeviceToHost));
    if (out.closed) HIPCHK(h, hipMemcpy(out.closed, dev.closed.p, t.n, hipMemcpyDeviceToHost));
    put_stats(stats, t.n, sum_len, executed, ms, dev.launches, t_begin);
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
    const TableView table{keys, key_stride, lengths, n};
    const ProfileOut out{on_counts, states, closed};
    TableSizes sizes;
    if (int rc = table_check_args(h, "bsx_run_attractor_profile", table, states != nullptr, state_offsets, sizes)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    ProfileDev dev;
    if (int rc = profile_stage(h, table, profile_want(out), state_offsets, sizes.state_words, dev)) return rc;
    if (int rc = profile_enqueue(h, table, dev)) return rc;
    return profile_collect(h, table, dev, out, sizes.sum_len, stats, t_begin);
}
