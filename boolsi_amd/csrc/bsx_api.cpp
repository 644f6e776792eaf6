// Host side of the C-ABI (include/bsx.h): handle management, and the per-lane family's bsx_set_network and
// bsx_set_problem_space: validate, lower (bsx_lane_lower.h: gather LUT, bit-packed truth-table masks, dense perturbation
// schedule), upload, configure.  The modes: bsx_target_api.cpp, bsx_simulate_api.cpp, bsx_attract_api.cpp.  No CPU compute
// path exists: every bsx_run_* ends in gfx950 kernel launches (bsx_attract.hip, bsx_target.hip, bsx_simulate.hip, bsx_sliced.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_lane_lower.h"
#include "bsx_wide_lower.h"

using namespace bsx;

namespace {
thread_local std::string g_create_error;
}  // namespace

extern "C" const char* bsx_status_string(int status) {
    switch (status) {
        case BSX_OK: return "ok";
        case BSX_ERR_INVALID: return "invalid argument";
        case BSX_ERR_NO_DEVICE: return "no gfx950 device";
        case BSX_ERR_HIP: return "HIP error";
        case BSX_ERR_UNSUPPORTED: return "unsupported network size";
        case BSX_ERR_TABLE_FULL: return "result table full";
        case BSX_ERR_STEP_LIMIT: return "internal step limit reached";
        case BSX_ERR_STATE: return "network / problem space not set";
        case BSX_ERR_COMM: return "RCCL communicator error";
        default: return "unknown status";
    }
}

extern "C" const char* bsx_last_error(bsx_handle h) {
    return h ? h->error.c_str() : g_create_error.c_str();
}

extern "C" int bsx_create(bsx_handle* out, int device) {
    if (!out) return BSX_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return BSX_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        g_create_error = "device index out of range";
        return BSX_ERR_INVALID;
    }
    bsx_engine* h = new bsx_engine();
    h->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&h->prop, device)) != hipSuccess) {
        g_create_error = std::string("hipSetDevice/hipGetDeviceProperties: ") + hipGetErrorString(e);
        delete h;
        return BSX_ERR_NO_DEVICE;
    }
    {
        int khz = 0;        // rate of wall_clock64() on the device (100 MHz on gfx9)
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_clock_khz = (double)khz;
    }
    if (std::strncmp(h->prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + h->prop.gcnArchName + ", this engine is built for gfx950 only";
        delete h;
        return BSX_ERR_NO_DEVICE;
    }
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&h->ev0)) != hipSuccess || (e = hipEventCreate(&h->ev1)) != hipSuccess ||
        (e = hipEventCreate(&h->ev_top0)) != hipSuccess || (e = hipEventCreate(&h->ev_top1)) != hipSuccess ||
        (e = h->d_ctr_raw.alloc(kLevelDescBytes + sizeof(Counters) * kMaxChainBlocks)) != hipSuccess ||
        (e = hipHostMalloc((void**)&h->h_ctr, sizeof(Counters) * kMaxChainBlocks + 256, hipHostMallocDefault)) != hipSuccess) {
        g_create_error = std::string("stream/event creation: ") + hipGetErrorString(e);
        if (h->h_ctr) (void)hipHostFree(h->h_ctr);
        delete h;
        return BSX_ERR_HIP;
    }
    h->d_level = reinterpret_cast<LevelDesc*>(h->d_ctr_raw.p);
    h->d_ctr = reinterpret_cast<Counters*>(h->d_ctr_raw.p + kLevelDescBytes);
    h->h_flag = reinterpret_cast<volatile uint32_t*>(h->h_ctr + kMaxChainBlocks);
    *h->h_flag = 0;
    h->knobs = Knobs::from_env();
    h->cache_enabled = h->knobs.cycle_cache;        // BSX_CYCLE_CACHE=0 disables the cycle-state cache (A/B runs, tests)
    if ((e = h->d_cc_journal.alloc(kCycleJournalCap)) != hipSuccess ||
        (e = h->d_cc_claims.alloc(kCycleClaimSlots)) != hipSuccess || (e = h->d_cc_count.alloc(1)) != hipSuccess) {
        g_create_error = std::string("cycle cache allocation: ") + hipGetErrorString(e);
        if (h->h_ctr) (void)hipHostFree(h->h_ctr);
        delete h;
        return BSX_ERR_HIP;
    }
    *out = h;
    return BSX_OK;
}

extern "C" int bsx_destroy(bsx_handle h) {
    if (!h) return BSX_OK;
    (void)hipSetDevice(h->device);
    if (h->comm) (void)bsx_comm_destroy(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (int i = 0; i < 8; ++i) {
        if (h->aux_done[i]) (void)hipEventDestroy(h->aux_done[i]);
        if (h->aux[i]) { (void)hipStreamSynchronize(h->aux[i]); (void)hipStreamDestroy(h->aux[i]); }
    }
    if (h->h_ctr_multi) (void)hipHostFree(h->h_ctr_multi);
    if (h->h_leaf) (void)hipHostFree(h->h_leaf);
    for (hipEvent_t e : h->ev_chain) (void)hipEventDestroy(e);
    for (hipStream_t st : h->side) if (st) (void)hipStreamDestroy(st);
    if (h->top2) (void)hipStreamDestroy(h->top2);
    if (h->ev_top2) (void)hipEventDestroy(h->ev_top2);
    if (h->ev_top0) (void)hipEventDestroy(h->ev_top0);
    if (h->ev_top1) (void)hipEventDestroy(h->ev_top1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->h_ctr) (void)hipHostFree(h->h_ctr);
    wide_release(h);
    wide_release_sample(h);
    delete h;
    return BSX_OK;
}

extern "C" int bsx_device_info(bsx_handle h, char* name, uint32_t name_cap, uint32_t* compute_units,
                               uint64_t* global_mem_bytes) {
    if (!h) return BSX_ERR_INVALID;
    if (name && name_cap) std::snprintf(name, name_cap, "%s (%s)", h->prop.name, h->prop.gcnArchName);
    if (compute_units) *compute_units = (uint32_t)h->prop.multiProcessorCount;
    if (global_mem_bytes) *global_mem_bytes = (uint64_t)h->prop.totalGlobalMem;
    return BSX_OK;
}

extern "C" int bsx_network_info(bsx_handle h, uint32_t* state_words32, uint32_t* mux_slots, uint32_t* lut_mode) {
    if (!h) return BSX_ERR_INVALID;
    if (!h->have_net) return fail(h, BSX_ERR_STATE, "network not set");
    if (state_words32) *state_words32 = h->net.nw;
    if (mux_slots) *mux_slots = h->net.k_mux;
    if (lut_mode) *lut_mode = (uint32_t)h->lut_mode;
    return BSX_OK;
}

extern "C" int bsx_synchronize(bsx_handle h) {
    if (!h) return BSX_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BSX_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int bsx_set_network(bsx_handle h, uint32_t n_nodes, const uint32_t* pred_offsets,
                               const uint32_t* pred_idx, const uint32_t* tt_word_offsets,
                               const uint64_t* tt_words) {
    if (!h) return BSX_ERR_INVALID;
    if (n_nodes == 0 || !pred_offsets || !tt_word_offsets || !tt_words)
        return fail(h, BSX_ERR_INVALID, "bsx_set_network: null table or zero nodes");
    h->knobs = Knobs::from_env();
    wide_release_sample(h);
    if (n_nodes > BSX_MAX_NODES || h->knobs.wide)          // the wide-state family (bsx_wide_host.h)
        return wide_set_network(h, n_nodes, pred_offsets, pred_idx, tt_word_offsets, tt_words);
    wide_release(h);
    HIPCHK(h, hipSetDevice(h->device));
    h->have_net = false;
    h->have_space = false;

    if (const LowerStatus s = check_network_arrays(n_nodes, pred_offsets, pred_idx, tt_word_offsets)) return fail(h, s.status, s.msg);
    {   // the arrays as received: the sampled calls lower them onto the wide family (bsx_sample_api.cpp)
        SampleInputs& in = h->inputs;
        in.pred_offsets.assign(pred_offsets, pred_offsets + n_nodes + 1);
        in.pred_idx.assign(pred_idx, pred_idx + pred_offsets[n_nodes]);
        in.tt_word_offsets.assign(tt_word_offsets, tt_word_offsets + n_nodes + 1);
        in.tt_words.assign(tt_words, tt_words + tt_word_offsets[n_nodes]);
    }
    LaneNet L;
    lane_lower_network(n_nodes, pred_offsets, pred_idx, tt_word_offsets, tt_words, h->knobs.cache_lds_kb, h->knobs.lut_mode, L, h->model);
    const uint32_t nw = L.nw, k_mux = L.k_mux;

    HIPCHK(h, h->d_lut.upload(L.lut));
    HIPCHK(h, h->d_masks.upload(L.masks));
    HIPCHK(h, h->d_wide_desc.upload(L.wdesc));
    HIPCHK(h, h->d_wide_preds.upload(L.wpreds));
    HIPCHK(h, h->d_wide_tt.upload(L.wtt));

    h->n_nodes = n_nodes;
    h->w64 = (n_nodes + 63) / 64;
    h->net.n_nodes = n_nodes;
    h->net.nw = nw;
    h->net.k_mux = k_mux;
    h->net.n_chunks = L.n_chunks;
    h->net.lut_words = (uint32_t)L.lut.size();
    h->net.n_wide = L.n_wide;
    h->net.lut = h->d_lut.p;
    h->net.masks = h->d_masks.p;
    h->net.wide_desc = h->d_wide_desc.p;
    h->net.wide_preds = h->d_wide_preds.p;
    h->net.wide_tt = h->d_wide_tt.p;

    h->cache_lds_slots = L.cache_lds_slots;
    h->lut_mode = L.lut_mode;
    h->shmem = L.shmem;
    h->shmem_attract = L.shmem_attract;
    HIPCHK(h, configure_attract((int)nw, (int)k_mux, h->lut_mode, h->shmem_attract));
    HIPCHK(h, configure_attract_fast((int)nw, (int)k_mux, h->lut_mode, h->shmem_attract, &h->lean_blocks_per_cu));
    h->cache_stride = L.cache_stride;
    {   // class-pool kernel: available when it fits next to the smallest useful mirror (64 slots)
        const size_t pool_max = h->shmem + (size_t)L.cache_lds_slots * L.cache_stride + 32 + pool_extra_bytes(nw);
        const size_t pool_min = h->shmem + (size_t)64 * L.cache_stride + 32 + pool_extra_bytes(nw);
        h->pool_ok = pool_min <= 160 * 1024 - 1024;
        int blocks = 0;
        if (h->pool_ok) HIPCHK(h, configure_attract_pool((int)nw, (int)k_mux, h->lut_mode, std::min<size_t>(pool_max, 160 * 1024 - 1024), &blocks));
    }
    if (h->knobs.debug) std::fprintf(stderr, "[bsx] network: nw %u k_mux %u lut mode %d (0 L2 bytes, 1 LDS bytes, 2 LDS nibbles) shmem %zu attract shmem %zu lean blocks/CU %d\n", nw, k_mux, (int)h->lut_mode, h->shmem, h->shmem_attract, h->lean_blocks_per_cu);
    HIPCHK(h, configure_target((int)nw, (int)k_mux, h->lut_mode, target_shmem(h->shmem, kTargetHistBins)));
    HIPCHK(h, configure_simulate((int)nw, (int)k_mux, h->lut_mode, h->shmem));
    HIPCHK(h, configure_profile((int)nw, (int)k_mux, h->lut_mode, h->shmem));
    h->have_net = true;
    return BSX_OK;
}

extern "C" int bsx_set_problem_space(bsx_handle h, const uint64_t* origin_state_words,
                                     const uint32_t* any_nodes, uint32_t n_any,
                                     const bsx_fixed* fixed, uint32_t n_fixed,
                                     const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                                     const bsx_pert* sched, uint32_t n_sched,
                                     const bsx_pert_var* pert_var, uint32_t n_pert_var) {
    if (!h) return BSX_ERR_INVALID;
    if (!h->have_net) return fail(h, BSX_ERR_STATE, "bsx_set_problem_space before bsx_set_network");
    if (!origin_state_words) return fail(h, BSX_ERR_INVALID, "origin state is null");
    if (n_pert_var > BSX_MAX_PERT_VARIATIONS) return fail(h, BSX_ERR_UNSUPPORTED, "more than BSX_MAX_PERT_VARIATIONS perturbation variations");
    if (n_any > h->n_nodes) return fail(h, BSX_ERR_INVALID, "more 'any' nodes than nodes");
    wide_release_sample(h);
    if (h->wide)
        return wide_set_problem_space(h, origin_state_words, any_nodes, n_any, fixed, n_fixed, fixed_var, n_fixed_var,
                                      sched, n_sched, pert_var, n_pert_var);
    HIPCHK(h, hipSetDevice(h->device));
    h->have_space = false;
    LaneSpace S;
    if (const LowerStatus s = lane_lower_space(h->n_nodes, h->net.nw, h->w64, origin_state_words, any_nodes, n_any, fixed, n_fixed,
                                               fixed_var, n_fixed_var, sched, n_sched, pert_var, n_pert_var, S))
        return fail(h, s.status, s.msg);
    {   // the arguments as received, for the sampled calls' second lowering
        SampleInputs& in = h->inputs;
        in.origin.assign(origin_state_words, origin_state_words + h->w64);
        in.any_nodes.assign(any_nodes, any_nodes + n_any);
        in.fixed.assign(fixed, fixed + n_fixed);
        in.fixed_var.assign(fixed_var, fixed_var + n_fixed_var);
        in.sched.assign(sched, sched + n_sched);
        in.pert_var.assign(pert_var, pert_var + n_pert_var);
    }
    h->model.sched = S.sched;
    h->model.any = S.any;
    h->model.fv = S.fv;
    HIPCHK(h, h->d_any.upload(S.any));
    HIPCHK(h, h->d_fv.upload(S.fv));
    HIPCHK(h, h->d_pv.upload(S.pv));
    HIPCHK(h, h->d_set.upload(S.set));
    HIPCHK(h, h->d_clr.upload(S.clr));
    // cycles depend on the network and the origin fixed nodes: start the cache empty
    HIPCHK(h, hipMemset(h->d_cc_journal.p, 0, sizeof(CycleRecord) * kCycleJournalCap));
    HIPCHK(h, hipMemset(h->d_cc_claims.p, 0, sizeof(unsigned int) * kCycleClaimSlots));
    HIPCHK(h, hipMemset(h->d_cc_count.p, 0, sizeof(unsigned int)));
    h->fast_ok = true;
    h->plan = PlanState();
    h->life_valid = 0;
    h->image_n = ~size_t(0);
    h->h_journal.clear();
    h->journal_stale = true;
    h->fast_steps = 0;
    h->fast_calibrated = false;
    h->variant_count = S.variant_count;
    h->variant_count_saturated = S.variant_count_saturated;
    h->tp_max = S.tp_max;
    DevSpace sp = S.sp;
    sp.any_nodes = h->d_any.p;
    sp.fv = h->d_fv.p;
    sp.pv = h->d_pv.p;
    sp.sched_set = h->d_set.p;
    sp.sched_clr = h->d_clr.p;
    h->sp = sp;
    h->have_space = true;
    return BSX_OK;
}
