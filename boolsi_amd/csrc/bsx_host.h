// Host-side helpers shared by the translation units behind include/bsx.h (bsx_api.cpp: handle, network, problem
// space; bsx_lane_host.h: target, simulate; bsx_attract_host.h: attract; bsx_wide_host.h: the wide family): kernel launch
// prototypes, range checks.  Not part of the ABI.  (Wide integers and the merge: bsx_merge.h; the cube analysis:
// bsx_cube_plan.h; the index arithmetic: bsx_lane_lower.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "bsx_engine.h"
#include "bsx_lane_lower.h"
#include "bsx_merge.h"

namespace bsx {
hipError_t launch_attract(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const AttractParams& P);
hipError_t launch_attract_fast(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const AttractParams& P);
hipError_t launch_target(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TargetParams& P);
hipError_t launch_simulate(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const SimParams& P);
hipError_t launch_simulate_sliced(int nw, int k, dim3 grid, size_t shmem, hipStream_t st, const SlicedParams& P);
hipError_t launch_simulate_sliced64(int nw, int k, dim3 grid, size_t shmem, hipStream_t st, const SlicedParams& P);
hipError_t launch_compact(const uint32_t* t_hit, uint64_t count, uint32_t* seg_counts, const uint64_t* seg_base,
                          HitRec* hits, uint64_t hits_cap, bool write_pass, hipStream_t st);
hipError_t configure_attract(int nw, int k, int lut_mode, size_t shmem);
hipError_t configure_attract_fast(int nw, int k, int lut_mode, size_t shmem, int* blocks_per_cu);
hipError_t launch_attract_pool(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const AttractParams& P);
hipError_t configure_attract_pool(int nw, int k, int lut_mode, size_t shmem, int* blocks_per_cu);
size_t pool_extra_bytes(uint32_t nw);
size_t pool_lower_extra_bytes(uint32_t nw);
hipError_t launch_digit_lifetimes(int nw, int k, int lut_mode, size_t shmem, hipStream_t st, const LifetimeParams& P);
hipError_t launch_publish(const uint32_t* src, uint32_t* host_dst, uint32_t words, uint32_t* host_flag, uint32_t seq, unsigned int* ticket,
                          hipStream_t stream);
hipError_t launch_fg_succ(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const DevNet& net, const DevSpace& sp,
                          uint64_t n_states, uint32_t* succ, uint32_t warm_steps);
hipError_t launch_fg_double(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t cus, hipStream_t st);
hipError_t launch_fg_mark(const uint32_t* land, uint64_t n, uint32_t* bits, uint32_t cus, hipStream_t st);
hipError_t launch_fg_collect(uint32_t* bits, uint64_t n_words, uint32_t* cand, uint32_t cand_cap, unsigned int* cursor, uint32_t cus, hipStream_t st);
hipError_t launch_fg_cycles(const uint32_t* succ, const uint32_t* cand, uint32_t n_cand, uint64_t walk_cap, void* cyc, uint32_t cyc_mask,
                            unsigned int* n_cyclic, unsigned int* n_open, hipStream_t st);
hipError_t launch_fg_pair_init(const uint32_t* succ, const void* cyc, uint32_t cyc_mask, unsigned long long* pair, uint64_t n, uint32_t cus, hipStream_t st);
hipError_t launch_fg_pair_jump(unsigned long long* pair, uint64_t n, uint32_t d_cap, unsigned int* changed, uint32_t cus, hipStream_t st);
hipError_t launch_fg_aggregate(const unsigned long long* pair, const void* cyc, uint32_t cyc_mask, const uint32_t* warm, uint32_t tp,
                               uint64_t first, uint64_t count,
                               uint64_t cap_rel, uint64_t max_len, uint64_t max_t, const AttractParams& P, uint32_t cus, hipStream_t st);
size_t fg_cyc_entry_bytes();
hipError_t launch_table_drain(LogRec* tab, uint64_t slots, LogRec* out, uint64_t out_cap, unsigned long long* cursor, hipStream_t st);
hipError_t configure_target(int nw, int k, int lut_mode, size_t shmem);
hipError_t configure_simulate(int nw, int k, int lut_mode, size_t shmem);
hipError_t launch_profile(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const ProfileParams& P);
hipError_t configure_profile(int nw, int k, int lut_mode, size_t shmem);
}  // namespace bsx

namespace bsx {

struct Launch {
    dim3 grid;
    uint32_t chunk;
};

inline Launch plan_persistent(const bsx_engine* h, uint64_t count, size_t shmem) {
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    uint32_t per_cu = (uint32_t)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(shmem, 1));
    per_cu = std::max(1u, std::min(per_cu, 4u));
    uint64_t blocks = (uint64_t)cus * per_cu;
    const uint64_t need = (count + kBlock - 1) / kBlock;
    blocks = std::max<uint64_t>(1, std::min(blocks, need));
    const uint64_t waves = blocks * kWavesPerBlock;
    uint64_t chunk = count / (waves * 8);
    chunk = std::min<uint64_t>(4096, std::max<uint64_t>(64, chunk));
    chunk = (chunk / 64) * 64;
    return Launch{dim3((uint32_t)blocks), (uint32_t)chunk};
}

// bsx_lane_lower.h's range_check against the handle's problem space
inline int check_range(bsx_handle h, const bsx_index* first, u128 count) {
    // (a wide space with more 'any' nodes than a bsx_index holds is for the sampled calls alone: whatever the index says,
    // a call that enumerates is refused before the index is looked at)
    if (h->wide && h->sp.n_any > 64 * BSX_MAX_WORDS)
        return fail(h, BSX_ERR_UNSUPPORTED, "more 'any' nodes than a bsx_index holds (64 * BSX_MAX_WORDS)");
    const LowerStatus s = range_check(first, count, h->sp.n_any, h->variant_count, h->variant_count_saturated);
    return s ? fail(h, s.status, s.msg) : BSX_OK;
}

inline int check_max_t(bsx_handle h, uint64_t max_t) {
    if (max_t != BSX_T_INF && max_t < h->tp_max)
        return fail(h, BSX_ERR_INVALID, "max_t is below the last perturbation time (origin schedule or a variation)");
    return BSX_OK;
}

inline void set_first(DevSpace& sp, const bsx_index* first) {
    for (int w = 0; w < 4; ++w) sp.first_digits[w] = first->init_digits[w];
    sp.first_variant = first->variant;
}

inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The statistics of a finished call that began at t_begin (now_ms)
inline void put_stats(bsx_stats* stats, uint64_t problems, uint64_t state_steps, uint64_t executed_steps, double kernel_ms,
                      uint32_t launches, double t_begin) {
    if (!stats) return;
    stats->problems = problems;
    stats->state_steps = state_steps;
    stats->executed_steps = executed_steps;
    stats->kernel_ms = kernel_ms;
    stats->kernel_launches = launches;
    stats->total_ms = now_ms() - t_begin;
}

}  // namespace bsx
