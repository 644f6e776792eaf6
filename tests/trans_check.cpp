// Stand-alone check of the walking lane's decision logic (boolsi_amd/csrc/bsx_walk.h).  Compiled by the host C++
// compiler with no HIP include path: walk_flip driven here is what k_trans_walk calls.
// Rho-shaped functional graphs: a tail of mu states 0 .. mu-1 that leads into a cycle of lambda states, plus a
// second, listed cycle that the walk never reaches.  For mu 0..40 and lambda 1..40, with the reached cycle listed and
// unlisted, under max_t on both sides of mu + lambda, small caps, a huge cap and no cap, the outcome, the row, mu
// and lambda must be what the definition says, the detector phase must take no more than walk_stop_time(max_t) steps
// and the whole walk no more than walk_step_bound(max_t).  Without a cap and with a lowered step limit L the walk must
// be decided iff the hit comes at t <= L (listed) or the detector closes at t <= L (unlisted: at 2^k - 1 + lambda
// for the least k with 2^k - 1 >= mu and 2^k >= lambda, as the header's comment derives).
//   trans_check            -> prints "ok <number of walks>" and exits 0, or "FAIL ..." and exits 1
#include <cstdint>
#include <cstdio>

#include "bsx_walk.h"

namespace {

uint64_t walks = 0;

struct Graph {
    uint32_t mu, lambda;
    bool listed;
    // states 0 .. mu + lambda - 1: the rho; 1000 .. 1004: another listed cycle (row 3, length 5)
    uint32_t step(uint32_t x) const {
        if (x >= 1000) return x == 1004 ? 1000 : x + 1;
        return x + 1 == mu + lambda ? mu : x + 1;
    }
    bool lookup(uint32_t x, uint32_t& d, uint32_t& len) const {
        if (x >= 1000) { d = 3; len = 5; return true; }
        if (listed && x >= mu) { d = 7; len = lambda; return true; }
        return false;
    }
};

bool run(const Graph& g, uint64_t max_t, uint32_t step_limit, uint32_t want_outcome) {
    const bsx::WalkResult r = bsx::walk_flip<uint32_t>(
        0u, max_t, step_limit, [&](uint32_t x) { return g.step(x); },
        [&](uint32_t x, uint32_t& d, uint32_t& len) { return g.lookup(x, d, len); }, [](uint32_t a, uint32_t b) { return a == b; });
    ++walks;
    bool ok = r.outcome == want_outcome;
    if (ok && r.outcome == bsx::kWalkHit) ok = r.dst == 7 && r.mu == g.mu && r.lambda == g.lambda;
    if (ok && r.outcome == bsx::kWalkOutside) ok = r.mu == g.mu && r.lambda == g.lambda;
    ok = ok && r.detect_steps <= r.steps;
    if (max_t <= (1ull << 20) && step_limit >= (1u << 30)) {
        ok = ok && bsx::walk_stop_time(max_t) != bsx::kWalkNoStop;
        ok = ok && r.detect_steps <= bsx::walk_stop_time(max_t) && r.steps <= bsx::walk_step_bound(max_t);
        ok = ok && bsx::walk_stop_time(max_t) <= 3 * max_t;
    }
    if (!ok)
        std::printf("FAIL mu %u lambda %u listed %d max_t %llu limit %u: outcome %u (want %u) dst %u mu %u lambda %u steps %u / %u\n",
                    g.mu, g.lambda, (int)g.listed, (unsigned long long)max_t, step_limit, r.outcome, want_outcome, r.dst, r.mu,
                    r.lambda, r.detect_steps, r.steps);
    return ok;
}

}  // namespace

int main() {
    const uint32_t kNoLimit = 1u << 30;
    bool ok = true;
    for (uint32_t mu = 0; mu <= 40; ++mu)
        for (uint32_t lambda = 1; lambda <= 40; ++lambda)
            for (int listed = 0; listed < 2; ++listed) {
                const Graph g{mu, lambda, listed != 0};
                const uint32_t resolved = listed ? bsx::kWalkHit : bsx::kWalkOutside;
                const uint64_t need = (uint64_t)mu + lambda;
                const uint64_t caps[] = {0, 1, 2, need / 2, need - 1, need, need + 1, 2 * need + 3, 1000, 1ull << 20};
                for (uint64_t cap : caps) ok = run(g, cap, kNoLimit, cap >= need ? resolved : (uint32_t)bsx::kWalkUnresolved) && ok;
                ok = run(g, bsx::kWalkInf, kNoLimit, resolved) && ok;
                // a cap so large that walk_stop_time does not apply behaves as no cap
                ok = run(g, 1ull << 40, kNoLimit, resolved) && ok;
                // lowered step limits, no cap
                uint32_t k = 0;
                while ((1u << k) - 1 < mu || (1u << k) < lambda) ++k;
                const uint32_t decided_at = listed ? mu : (1u << k) - 1 + lambda;
                const uint32_t limits[] = {0, 1, mu, mu + 1, decided_at - 1, decided_at, decided_at + 1, 16, 64, 200};
                for (uint32_t limit : limits) {
                    if (limit == 0 && decided_at == 0) { ok = run(g, bsx::kWalkInf, 0, resolved) && ok; continue; }
                    if (limit + 1 == 0) continue;
                    ok = run(g, bsx::kWalkInf, limit, limit >= decided_at ? resolved : (uint32_t)bsx::kWalkStepLimit) && ok;
                }
            }
    // the stop time is what the comment says: least power of two >= max_t, minus one, plus max_t
    ok = ok && bsx::walk_stop_time(1) == 1 && bsx::walk_stop_time(2) == 3 && bsx::walk_stop_time(3) == 6 && bsx::walk_stop_time(4) == 7 &&
         bsx::walk_stop_time(5) == 12 && bsx::walk_stop_time(bsx::kWalkInf) == bsx::kWalkNoStop && bsx::walk_step_bound(0) == 0;
    if (!ok) { std::printf("FAIL\n"); return 1; }
    std::printf("ok %llu\n", (unsigned long long)walks);
    return 0;
}
