// What one lane of bsx_run_attractor_transitions decides per step (kernel: k_trans_walk, bsx_trans_kernel.h): a
// trajectory x_0, x_1 = F(x_0), ... is followed until it is known whether it ends on a LISTED cycle (a row of the
// caller's attractor table), on an unlisted one, or cannot be resolved within max_t.  Written against three functors
//     step(x)            -> F(x)
//     lookup(x, d, len)  -> true iff x is a state of a listed cycle; then d = its row and len = its length
//     eq(a, b)           -> a == b
// so that tests/trans_check.cpp drives exactly this code on small functional graphs with the host compiler and no HIP
// include path (plain C++ with optional __host__ __device__, as bsx_planes.h and bsx_ranks.h).
//
// Semantics (include/bsx.h): mu = least t with x_t on a cycle C, lambda' = |C|; resolved iff mu + lambda' <= max_t.
//
// Listed C.  Every state of C is in the table and no state before x_mu is on any cycle, so the first t whose lookup
// succeeds is mu, with lambda' = len: kWalkHit iff t + len <= max_t, kWalkUnresolved otherwise.  A lookup at
// t >= max_t cannot resolve anything (len >= 1) and is not made.
//
// Unlisted C.  Brent's detector with power-of-two checkpoints runs beside the lookups.  The checkpoint rule: the
// checkpoint is x_c with c = 0 at first; at time t, before the step, t - c == power moves it (c = t, power *= 2), power
// = 1 at first.  So c takes the values 2^k - 1 and while c = 2^k - 1 the states x_t, c < t <= c + 2^k are compared with
// x_c ("window k").  x_t == x_c needs x_c on C and lambda' | t - c: window k closes the detector iff 2^k - 1 >= mu and
// 2^k >= lambda', and then at t = 2^k - 1 + lambda' with lambda' = t - c exactly.  mu comes from the usual two-pointer
// pass (a = x_0, b = F^lambda'(x_0), both stepped until they meet after mu steps): kWalkOutside iff
// mu + lambda' <= max_t.  The pass gives up as soon as mu + lambda' > max_t is certain.
//
// The early stop, finite max_t >= 1.  No hit at any t < max_t already means kWalkUnresolved if C is listed.  If C is
// unlisted and resolvable, mu + lambda' <= max_t with lambda' >= 1 gives mu <= max_t - 1 and lambda' <= max_t.  Let
// k* be the least k with 2^k >= max_t.  Then 2^k* - 1 >= mu and 2^k* >= lambda', so the detector closes in window k*
// at the latest, that is at a time
//     t <= 2^k* - 1 + lambda' <= 2^k* - 1 + max_t =: walk_stop_time(max_t)        (< 3 max_t, as 2^k* < 2 max_t).
// A detector still open at t = walk_stop_time(max_t) therefore means kWalkUnresolved, and the walk stops there: the
// detector phase makes at most walk_stop_time(max_t) steps.  The mu pass makes lambda' <= max_t steps for b and then at
// most 2 (max_t - lambda') for the pair, so the whole walk makes at most walk_stop_time(max_t) + 2 max_t steps.
// max_t == 0 resolves nothing (mu + lambda' >= 1) and takes no step.
//
// The step limit.  Times are 32-bit; `step_limit` (at most 2^30) bounds the detector phase's t and the mu pass's mu.
// A walk that reaches it undecided is kWalkStepLimit; under finite max_t that can happen only when walk_stop_time
// exceeds the limit.
#pragma once
#include <stdint.h>

#if !defined(BSX_HD)
#if defined(__HIPCC__)
#define BSX_HD __host__ __device__ __forceinline__
#else
#define BSX_HD inline
#endif
#endif

namespace bsx {

constexpr uint64_t kWalkInf = ~0ull;            // max_t: no cap (BSX_T_INF)
constexpr uint64_t kWalkNoStop = ~0ull;

enum WalkOutcome : uint32_t {
    kWalkHit = 0,           // resolved on listed row `dst` after `mu` steps
    kWalkOutside = 1,       // resolved on a cycle that is in no row
    kWalkUnresolved = 2,    // mu + lambda' > max_t
    kWalkStepLimit = 3,     // undecided at the step limit
};

struct WalkResult {
    uint32_t outcome;
    uint32_t dst;           // kWalkHit: the row
    uint32_t mu;            // kWalkHit, kWalkOutside
    uint32_t lambda;        // kWalkHit, kWalkOutside
    uint32_t detect_steps;  // steps of the detector phase
    uint32_t steps;         // all steps taken
};

// The time after which an open detector means "unresolved" (derivation above); kWalkNoStop without a cap or where
// the bound lies beyond every step limit anyway.
BSX_HD uint64_t walk_stop_time(uint64_t max_t) {
    if (max_t == kWalkInf || max_t > (1ull << 31)) return kWalkNoStop;
    uint64_t p = 1;
    while (p < max_t) p <<= 1;
    return p - 1 + max_t;
}

// The upper bound on all steps of one walk under a finite cap that walk_stop_time knows.
BSX_HD uint64_t walk_step_bound(uint64_t max_t) { return max_t == 0 ? 0 : walk_stop_time(max_t) + 2 * max_t; }

template <typename S, typename Step, typename Lookup, typename Eq>
BSX_HD WalkResult walk_flip(const S& x0, uint64_t max_t, uint32_t step_limit, Step step, Lookup lookup, Eq eq) {
    WalkResult r{kWalkUnresolved, 0u, 0u, 0u, 0u, 0u};
    const bool inf = max_t == kWalkInf;
    if (max_t == 0) return r;
    const uint64_t stop = walk_stop_time(max_t);
    // one loop, one call of `step` for x whatever the phase (the kernel inlines a network update per call):
    //   phase 0  detector: x = x_t, cp = x_c
    //   phase 1  x = F^i(x_0), i < lambda'  (the mu pass's far pointer gets its head start)
    //   phase 2  x = F^(lambda' + mu)(x_0), a = F^mu(x_0)
    S x = x0, cp = x0, a = x0;
    uint32_t phase = 0, t = 0, c = 0, power = 1, lam = 0, i = 0, mu = 0;
    for (;;) {
        if (phase == 0) {
            if (inf || t < max_t) {
                uint32_t d = 0, len = 0;
                if (lookup(x, d, len)) {
                    r.detect_steps = t;
                    if (!inf && (uint64_t)t + len > max_t) return r;
                    r.outcome = kWalkHit; r.dst = d; r.mu = t; r.lambda = len;
                    return r;
                }
            }
            if ((uint64_t)t >= stop) { r.detect_steps = t; return r; }
            if (t >= step_limit) { r.detect_steps = t; r.outcome = kWalkStepLimit; return r; }
            if (t - c == power) { cp = x; c = t; power <<= 1; }
        } else if (phase == 2) {
            if (eq(a, x)) { r.outcome = kWalkOutside; r.mu = mu; r.lambda = lam; return r; }
            if (!inf && (uint64_t)mu + 1 + lam > max_t) return r;
            if (mu >= step_limit) { r.outcome = kWalkStepLimit; return r; }
            a = step(a);
            ++mu;
            ++r.steps;
        }
        x = step(x);
        ++r.steps;
        if (phase == 0) {
            ++t;
            if (eq(x, cp)) {
                lam = t - c;
                r.detect_steps = t;
                if (!inf && (uint64_t)lam > max_t) return r;
                phase = 1; x = x0; i = 0;
            }
        } else if (phase == 1) {
            ++i;
        }
        if (phase == 1 && i == lam) phase = 2;
    }
}

}  // namespace bsx
