// Internals shared by the translation units of attract (bsx_attract_api.cpp: tile ladder and entry points;
// bsx_cascade.cpp: cube cascade; bsx_fgraph_api.cpp: functional-graph mode).  Not part of the ABI.
#pragma once
#include "bsx_cube_plan.h"
#include "bsx_host.h"
#include "bsx_merge.h"

namespace bsx {

constexpr uint32_t kFastStepsMax = 3072;        // FAST phase length (steps without a cached cycle state), upper end

struct AttractRun {
    Counters ctr{};
    float ms = 0.f;
};

// What a call adds up (wide: a call may cover 2^128 problems).
struct Totals {
    MergedTable merged;
    u128 n_none = 0, steps_ref = 0;
    uint64_t steps_exec = 0;
    double kernel_ms = 0.0, dominant_ms = 0.0;
    uint64_t dominant_exec = 0;
    uint32_t launches = 0, dominant_launches = 0, limit_hits = 0, syncs = 0;
    double lower_ms = 0;                // cascades: the launches of the lower levels that had anything to do (device clock)
    uint64_t lower_exec = 0;
    uint32_t lower_launches = 0;
    // BSX_PROFILE: host time per section, ms: pass setup, enqueue, wait, kernels, split estimates, reading the counters
    double prof[6] = {};

    // One waited-for pass: its device time and work; with `results` also what it found (none / reference steps).
    // (`limits` = false: the discovery pass, whose results are discarded, does not report step-limit hits either)
    void book(const AttractRun& r, bool results, bool limits = true) {
        kernel_ms += r.ms; ++launches; steps_exec += r.ctr.steps_exec;
        if (limits) limit_hits += r.ctr.step_limit_hits;
        if (results) { n_none += r.ctr.n_none; steps_ref += r.ctr.steps_ref; }
    }
};

enum PassKind { kPassGeneral = 0, kPassLean = 1, kPassPool = 2 };

struct CascadeEnv {
    const AttractParams& P;         // the call's template (network, caps, cache)
    uint64_t max_t, max_len;
    Totals& tot;
    DevBuf<LogRec>& d_log;
};

// bsx_attract_api.cpp
int launch_attract_pass(bsx_handle h, AttractParams& P, int kind, DevBuf<LogRec>& d_log, MergedTable* merged, AttractRun& run, Totals& tot);
int drain_attractor_table(bsx_handle h, MergedTable& merged);
int ensure_attractor_table(bsx_handle h, uint32_t cap);

// bsx_cascade.cpp
int lean_mirror_slots(bsx_handle h, uint32_t* slots_out, Totals* tot = nullptr);
int ensure_mirror_image(bsx_handle h, AttractParams& P, size_t shmem);
int run_block(bsx_handle h, const CascadeEnv& env, uint64_t d_lo, uint32_t a_bits, bool& collapsed);

}  // namespace bsx
