// Simulate mode of the per-lane family (n <= 256): bsx_run_simulate and bsx_run_trajectories.  Which kernel a call
// takes, its launch shape and the bit-sliced kernels' row descriptors come from bsx_lane_lower.h; this file uploads and
// launches (bsx_simulate.hip, bsx_sliced.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bsx_lane_host.h"

using namespace bsx;

static int run_sim_common(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                          const uint64_t* offsets, const uint64_t* t_len, const uint64_t* out_offsets,
                          uint64_t traj_words, uint64_t* trajectories, uint64_t* final_states,
                          uint64_t* digests, bsx_stats* stats) {
    const double t_begin = now_ms();
    HIPCHK(h, hipSetDevice(h->device));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (max_t >= kStepLimit) return fail(h, BSX_ERR_UNSUPPORTED, "simulation length above the engine's step limit");
    const uint32_t W = h->w64;
    DevBuf<uint64_t> d_traj, d_final, d_dig, d_off, d_tlen, d_ooff;
    if (trajectories) HIPCHK(h, d_traj.alloc(traj_words));
    // scattered trajectories: the whole buffer comes back in one copy, so the words between them make the round trip
    // (a caller's buffer keeps what no trajectory covers)
    if (trajectories && out_offsets) HIPCHK(h, hipMemcpy(d_traj.p, trajectories, traj_words * 8, hipMemcpyHostToDevice));
    if (final_states) HIPCHK(h, d_final.alloc(count * W));
    if (digests) HIPCHK(h, d_dig.alloc(count));
    if (offsets) { HIPCHK(h, d_off.alloc(count)); HIPCHK(h, hipMemcpy(d_off.p, offsets, count * 8, hipMemcpyHostToDevice)); }
    if (t_len) { HIPCHK(h, d_tlen.alloc(count)); HIPCHK(h, hipMemcpy(d_tlen.p, t_len, count * 8, hipMemcpyHostToDevice)); }
    if (out_offsets) { HIPCHK(h, d_ooff.alloc(count)); HIPCHK(h, hipMemcpy(d_ooff.p, out_offsets, count * 8, hipMemcpyHostToDevice)); }

    SimParams P{};
    P.net = h->net;
    P.sp = h->sp;
    set_first(P.sp, first);
    P.count = count;
    P.max_t = max_t;
    P.w64 = W;
    P.offsets = offsets ? d_off.p : nullptr;
    P.t_len = t_len ? d_tlen.p : nullptr;
    P.out_offsets = out_offsets ? d_ooff.p : nullptr;
    P.traj = trajectories ? d_traj.p : nullptr;
    P.final_states = final_states ? d_final.p : nullptr;
    P.digests = digests ? d_dig.p : nullptr;
    P.ctr = h->d_ctr;

    const uint64_t blocks = lane_sim_blocks(count, (uint32_t)h->prop.multiProcessorCount);
    if (h->knobs.debug && !offsets) std::fprintf(stderr, "[bsx] simulate: per-lane, %llu blocks\n", (unsigned long long)blocks);
    Counters ctr{};
    float ms = 0.f;
    if (int rc = lane_timed_launch(h, ctr, ms, [&]() -> int {
            HIPCHK(h, launch_simulate((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), h->shmem, h->stream, P));
            return BSX_OK;
        })) return rc;
    if (trajectories) HIPCHK(h, hipMemcpy(trajectories, d_traj.p, traj_words * 8, hipMemcpyDeviceToHost));
    if (final_states) HIPCHK(h, hipMemcpy(final_states, d_final.p, count * W * 8, hipMemcpyDeviceToHost));
    if (digests) HIPCHK(h, hipMemcpy(digests, d_dig.p, count * 8, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr.steps_ref, ctr.steps_exec, ms, 1, t_begin);
    return BSX_OK;
}

// Final states of a fixed-length run through the bit-sliced kernel (no variations, no wide rules).
static int run_sim_sliced(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                          uint64_t* final_states, uint64_t* digests, bsx_stats* stats) {
    const double t_begin = now_ms();
    HIPCHK(h, hipSetDevice(h->device));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const uint32_t K = h->net.k_mux, W = h->w64;
    const SlicedShape S = sliced_shape(h->n_nodes, K, h->knobs.sliced, count, (uint32_t)h->prop.multiProcessorCount);
    std::vector<uint32_t> desc;
    sliced_row_desc(h->model, h->sp, K, desc);
    DevBuf<uint32_t> d_desc, d_sched;
    DevBuf<uint64_t> d_final, d_dig;
    HIPCHK(h, d_desc.upload(desc));
    HIPCHK(h, d_sched.upload(h->model.sched));
    if (final_states) HIPCHK(h, d_final.alloc(count * W));
    if (digests) HIPCHK(h, d_dig.alloc(count));

    SlicedParams P{};
    P.sp = h->sp;
    set_first(P.sp, first);
    P.n_nodes = h->n_nodes;
    P.n_rows = S.rows;
    P.n_sched = (uint32_t)(h->model.sched.size() / 3);
    P.w64 = W;
    P.desc = d_desc.p;
    P.sched = d_sched.p;
    P.count = count;
    P.max_t = max_t;
    P.final_states = final_states ? d_final.p : nullptr;
    P.digests = digests ? d_dig.p : nullptr;
    P.ctr = h->d_ctr;

    if (h->knobs.debug) std::fprintf(stderr, "[bsx] simulate: %s, %llu blocks, %llu groups\n", S.gen2 ? "sliced64" : "sliced", (unsigned long long)S.blocks, (unsigned long long)S.groups);
    Counters ctr{};
    float ms = 0.f;
    if (int rc = lane_timed_launch(h, ctr, ms, [&]() -> int {
            if (S.gen2) HIPCHK(h, launch_simulate_sliced64((int)h->net.nw, (int)K, dim3((uint32_t)S.blocks), S.shmem, h->stream, P));
            else HIPCHK(h, launch_simulate_sliced((int)h->net.nw, (int)K, dim3((uint32_t)S.blocks), S.shmem, h->stream, P));
            return BSX_OK;
        })) return rc;
    if (final_states) HIPCHK(h, hipMemcpy(final_states, d_final.p, count * W * 8, hipMemcpyDeviceToHost));
    if (digests) HIPCHK(h, hipMemcpy(digests, d_dig.p, count * 8, hipMemcpyDeviceToHost));
    put_stats(stats, count, ctr.steps_ref, ctr.steps_exec, ms, 1, t_begin);
    return BSX_OK;
}

extern "C" int bsx_run_simulate(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                                uint64_t* trajectories, uint64_t* final_states, uint64_t* digests,
                                bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (int rc = check_range(h, first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    if (h->wide) return wide_run_simulate(h, first, count, max_t, trajectories, final_states, digests, stats);
    // Long fixed-length runs that only want final states go through the bit-sliced kernel
    // (BSX_SLICED=0 forces the per-lane kernel, for A/B runs and tests).
    if (sliced_ok(h->n_nodes, h->net, h->sp, h->knobs.sliced, trajectories != nullptr, final_states != nullptr, digests != nullptr, max_t, count))
        return run_sim_sliced(h, first, count, max_t, final_states, digests, stats);
    const uint64_t words = trajectories ? count * (max_t + 1) * h->w64 : 0;
    return run_sim_common(h, first, count, max_t, nullptr, nullptr, nullptr, words, trajectories, final_states,
                          digests, stats);
}

extern "C" int bsx_run_trajectories(bsx_handle h, const bsx_index* first, const uint64_t* offsets,
                                    const uint64_t* t_len, uint64_t n, uint64_t* out,
                                    const uint64_t* out_offsets, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (n && (!offsets || !t_len || !out || !out_offsets)) return fail(h, BSX_ERR_INVALID, "null argument");
    uint64_t words = 0, tmax = 0, off_max = 0;
    for (uint64_t q = 0; q < n; ++q) off_max = std::max(off_max, offsets[q]);
    if (int rc = check_range(h, first, n ? off_max + 1 : 0)) return rc;
    for (uint64_t q = 0; q < n; ++q) {
        words = std::max(words, out_offsets[q] + (t_len[q] + 1) * h->w64);
        tmax = std::max(tmax, t_len[q]);
    }
    if (h->wide) return wide_run_trajectories(h, first, offsets, t_len, n, out, out_offsets, stats);
    return run_sim_common(h, first, n, tmax, offsets, t_len, out_offsets, words, out, nullptr, nullptr, stats);
}
