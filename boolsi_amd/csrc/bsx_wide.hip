// Wide-state kernel family: simulate / trajectories, target and attract for networks of up to 1024 nodes
// (bsx_wide.h has the layout).  One workgroup steps a group of 32 * L trajectories in lock step; problems with
// different perturbation times, fixed-node variations and perturbation variations share a group through
// per-trajectory masks, so the mode of the group's control flow is uniform:
//   * warm-up (attract): trajectory b is frozen (its column bit keeps its value) after its own T_p, so that the
//     matrix ends at s(T_p) for every b; from there all trajectories are autonomous;
//   * Brent's detector: power-of-two checkpoints at the same relative time for every bit, "back at the
//     checkpoint" = no row differs in that bit (OR over rows of cur ^ saved, reduced over the slices);
//   * mu: a second lock-step pass, y = s(T_p + lambda_b) (bit b frozen after lambda_b steps) against x = s(T_p);
//   * key: the minimum state over one lap of the cycle, by a bit-sliced lexicographic compare from the highest
//     row down (per-slice lt / eq masks, combined across slices from the top).
// k_wide<K, KW, true> (attract) and k_wide<K, KW, true, MODE> (target, simulate) run over samples of a seed instead of
// consecutive problem indices (bsx_sample.h): the same body, with the group's set-up and the one branch an instantiation
// carries chosen at compile time.  k_wide_screen (at the end of the file) runs the attract phases per (mutant, group)
// pair of a knockout / overexpression screen over samples; k_wide_influence (behind k_wide_damage) counts, per (source,
// group) pair, which rows differ after a single node was inverted.
#include <hip/hip_runtime.h>

#include "bsx_device.h"
#include "bsx_influence.h"
#include "bsx_planes.h"
#include "bsx_sample.h"
#include "bsx_screen.h"
#include "bsx_trans.h"
#include "bsx_wide.h"
#include "bsx_wtrans.h"

namespace bsx {

namespace {

__device__ __forceinline__ uint32_t wbfi(uint32_t sel, uint32_t a, uint32_t b) { return (a & sel) | (b & ~sel); }

__device__ __forceinline__ int wide_digit_state(uint32_t range, uint32_t digit) {     // batching.py:171-175; -1 = absent
    if (range == 0) return digit ? 0 : -1;
    if (range == 1) return digit ? 1 : -1;
    if (range == 2) return digit ? 1 : 0;
    return digit == 0 ? -1 : (digit == 1 ? 0 : 1);
}

struct WideCtx {
    uint32_t L, c, slice, r0, r1, RL, tid;
};

// One synchronous update of rows [r0, r1) of column c: rules, fixed-node variations, freeze mask (bits not in
// `act` keep their value).  Origin fixed nodes are constant rules in the descriptors (model.py:31-49).
template <int K, bool KW>
__device__ __forceinline__ void wide_step(const WideParams& P, const WideCtx& X, const uint32_t* cur, uint32_t* nxt,
                                          const uint32_t* fmv, uint32_t act) {
    const uint32_t L = X.L, c = X.c;
    for (uint32_t r = X.r0; r < X.r1; ++r) {
        const uint4 d0 = *reinterpret_cast<const uint4*>(P.desc + (size_t)r * kWideDescWords);
        const uint4 d1 = *reinterpret_cast<const uint4*>(P.desc + (size_t)r * kWideDescWords + 4);
        uint32_t v;
        if (KW && d1.z != kWideNone) {
            // more than 6 predecessors: per-trajectory table lookups (32 indices built bit by bit)
            const uint32_t* wd = P.wdesc + 3 * d1.z;
            const uint32_t k = wd[0], poff = wd[1], toff = wd[2];
            uint32_t idx[32];
#pragma unroll
            for (int b = 0; b < 32; ++b) idx[b] = 0;
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t g = cur[P.wpreds[poff + j] * L + c];
#pragma unroll
                for (int b = 0; b < 32; ++b) idx[b] |= ((g >> b) & 1u) << j;
            }
            v = 0;
#pragma unroll
            for (int b = 0; b < 32; ++b) v |= ((P.wtt[toff + (idx[b] >> 5)] >> (idx[b] & 31u)) & 1u) << b;
        } else {
            const uint32_t pw[3] = {d0.x, d0.y, d0.z};
            const uint64_t tbits = ((uint64_t)d1.x << 32) | d0.w;
            uint32_t g[K];
#pragma unroll
            for (int j = 0; j < K; ++j) g[j] = cur[((pw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) * L + c];
            uint32_t m[1 << (K - 1)];
#pragma unroll
            for (int i = 0; i < (1 << (K - 1)); ++i) {
                const uint32_t hi = 0u - (uint32_t)((tbits >> (2 * i + 1)) & 1u);
                const uint32_t lo = 0u - (uint32_t)((tbits >> (2 * i)) & 1u);
                m[i] = wbfi(g[0], hi, lo);
            }
#pragma unroll
            for (int j = 1; j < K; ++j)
#pragma unroll
                for (int i = 0; i < (1 << (K - 1 - j)); ++i) m[i] = wbfi(g[j], m[2 * i + 1], m[2 * i]);
            v = m[0];
        }
        if (d1.y != kWideNone) v = (v & ~fmv[(2 * d1.y) * L + c]) | fmv[(2 * d1.y + 1) * L + c];
        nxt[r * L + c] = wbfi(act, v, cur[r * L + c]);
    }
}

// Perturbation override at time t (model.py:68-71) on the matrix just written: origin schedule, then the
// variations in list order (which win over an origin entry of the same (t, node), batching.py:198-207).
// Uniform: returns whether anything was written (then the caller's barrier is needed before the next read).
__device__ __forceinline__ bool wide_perturb(const WideParams& P, const WideCtx& X, uint64_t t, uint32_t* buf,
                                             const uint32_t* pmv, uint32_t& sched_at) {
    bool any = false;
    while (sched_at < P.n_sched && P.sched[3 * sched_at] < t) ++sched_at;
    for (uint32_t q = sched_at; q < P.n_sched && P.sched[3 * q] == t; ++q) {
        if (X.tid < X.L) buf[P.sched[3 * q + 1] * X.L + X.tid] = P.sched[3 * q + 2] ? 0xFFFFFFFFu : 0u;
        any = true;
    }
    for (uint32_t j = 0; j < P.n_pv; ++j) {
        if (P.pv[3 * j] != t) continue;
        if (X.tid < X.L) {
            uint32_t& w = buf[P.pv[3 * j + 1] * X.L + X.tid];
            w = (w & ~pmv[(2 * j) * X.L + X.tid]) | pmv[(2 * j + 1) * X.L + X.tid];
        }
        any = true;
    }
    return any;
}

// Bits of trajectory k: the 64 nodes of 64-bit state word w.
__device__ __forceinline__ uint64_t wide_gather64(const WideParams& P, const uint32_t* buf, uint32_t L, uint32_t k, uint32_t w) {
    uint64_t word = 0;
    const uint32_t col = k >> 5, bit = k & 31u;
    for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t node = w * 64 + i;
        if (node >= P.n_nodes) break;
        word |= (uint64_t)((buf[node * L + col] >> bit) & 1u) << i;
    }
    return word;
}

// Sampled source: the block keys of column cw (first sample j0), as the group's set-up left them in `keys` (4 words per column)
__device__ __forceinline__ SampleColumn wide_sample_column(const uint32_t* keys, uint32_t cw, uint64_t j0) {
    return SampleColumn{(uint64_t)keys[4 * cw] | ((uint64_t)keys[4 * cw + 1] << 32),
                        (uint64_t)keys[4 * cw + 2] | ((uint64_t)keys[4 * cw + 3] << 32), (uint32_t)(j0 & 63u)};
}

}  // namespace

// KW: the network has nodes with more than 6 predecessors (their path's 32 table indices cost registers)
// SAMPLED: trajectory k of a group is sample P.sample_first + base + k of the seed behind P.sample_k0 (bsx_sample.h), not
// problem first + base + k.  A compile-time choice: it changes a group's set-up and nothing behind it.
// MODE: the WideMode whose branch the instantiation carries, or -1 for all three, chosen by P.mode at run time (the
// enumerating kernels).  A sampled instantiation carries one branch: k_wide<K, KW, true> is attract over samples, as it
// was, k_wide<K, KW, true, kWideTarget / kWideSimulate> are target and simulate.  In the sampled simulate instantiation a
// non-null P.sample_list makes trajectory q sample P.sample_list[q] (bsx_run_trajectories_sampled): set up per trajectory,
// in the shape of the enumerating source, since a column's 32 samples are not consecutive there.
// (One kernel template, not a shared body behind several: behind a forwarding kernel the enumerating instantiations came
// out with other register and scratch figures.)
template <int K, bool KW, bool SAMPLED = false, int MODE = SAMPLED ? (int)kWideAttract : -1>
__global__ __launch_bounds__(kWideThreads) void k_wide(const WideParams P) {
    static_assert(SAMPLED ? MODE >= 0 : MODE == -1, "a sampled instantiation carries one branch, an enumerating one all three");
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    constexpr bool kListable = SAMPLED && MODE == (int)kWideSimulate;
    const bool listed = kListable && P.sample_list != nullptr;
    const uint32_t mode = MODE < 0 ? P.mode : (uint32_t)MODE;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t nslices = kWideThreads / L;
    uint32_t* B[4] = {sm, sm + RL, sm + 2 * RL, sm + 3 * RL};
    uint32_t* fmv = sm + 4 * RL;                    // [n_fslots][2][L]  fixed-node variations: mask, value
    uint32_t* pmv = fmv + 2 * P.n_fslots * L;       // [n_pv][2][L]      perturbation variations: mask, value
    uint32_t* red = pmv + 2 * P.n_pv * L;           // [2][256]          per-thread partials
    uint32_t* col = red + 2 * kWideThreads;         // [8][L]            per-column masks
    uint32_t* tpa = col + 8 * L;                    // [G] T_p
    uint32_t* lam = tpa + G;                        // [G] lambda
    uint32_t* mua = lam + G;                        // [G] mu
    uint32_t* sta = mua + G;                        // [G] state of the trajectory's search (below)
    uint32_t* misc = sta + G;                       // [8]
    enum : uint32_t { ST_ACTIVE = 0, ST_CAND = 1, ST_FOUND = 2, ST_NONE = 3, ST_INVALID = 4 };
    unsigned long long steps_ref = 0, steps_exec = 0, limit_hits = 0;

    const uint64_t n_groups = (P.count + G - 1) / G;
    for (uint64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
        const uint64_t base = group * G;
        const uint32_t n_valid = (uint32_t)((P.count - base) < G ? (P.count - base) : G);
        // ---- s(0) = origin | 'any' digits; per-trajectory fixed-node / perturbation masks and T_p
        for (uint32_t i = tid; i < RL; i += kWideThreads) {
            const uint32_t r = i >> P.lshift;
            B[0][i] = (r < P.n_nodes && ((P.origin[r >> 5] >> (r & 31u)) & 1u)) ? 0xFFFFFFFFu : 0u;
        }
        for (uint32_t i = tid; i < 2 * (P.n_fslots + P.n_pv) * L; i += kWideThreads) fmv[i] = 0;
        if (tid < 8) misc[tid] = 0;
        if constexpr (SAMPLED) {
            // the block keys of column tid's 32 samples (at most two blocks), once per group: col[4 tid ..], free until the warm-up
            if (tid < L && !listed) {
                const SampleColumn sc = sample_column(P.sample_k0, P.sample_first + base + 32ull * tid);
                col[4 * tid + 0] = (uint32_t)sc.kb0; col[4 * tid + 1] = (uint32_t)(sc.kb0 >> 32);
                col[4 * tid + 2] = (uint32_t)sc.kb1; col[4 * tid + 3] = (uint32_t)(sc.kb1 >> 32);
            }
        }
        __syncthreads();
        if constexpr (SAMPLED) {
            // s(0): one word per ('any' ordinal, column), one plain store each (the origin has these rows cleared and
            // 'any' rows are distinct)
            for (uint32_t i = tid; i < (listed ? 0u : P.n_any * L); i += kWideThreads) {
                const uint32_t a = i >> P.lshift, cw = i & (L - 1);
                const SampleColumn sc = wide_sample_column(col, cw, P.sample_first + base + 32ull * cw);
                const uint32_t n_bits = n_valid > 32 * cw ? (n_valid - 32 * cw < 32u ? n_valid - 32 * cw : 32u) : 0u;
                B[0][P.any_nodes[a] * L + cw] = sample_column_word(sc, a, n_bits);
            }
        }
        for (uint32_t k = tid; k < G; k += kWideThreads) {
            uint32_t tp = P.tp_origin, st = ST_ACTIVE;
            if (k >= n_valid) {
                st = ST_INVALID;
            } else {
                uint64_t variant;
                uint32_t bit, cw;
                if (listed) {
                    // sample P.sample_list[base + k]: its own block key, one mix per 'any' ordinal, one atomicOr per set bit
                    bit = 1u << (k & 31u); cw = k >> 5;
                    const uint64_t j = P.sample_list[base + k];
                    const uint64_t kb = sample_block_key(P.sample_k0, j >> 6);
                    for (uint32_t a = 0; a < P.n_any; ++a)
                        if (sample_any_bit(kb, a, j)) atomicOr(&B[0][P.any_nodes[a] * L + cw], bit);
                    variant = sample_variant_of(kb, P.n_any, j, P.sample_variants);
                } else if constexpr (SAMPLED) {
                    // sample first + base + k: the variant number is one draw of its own (the state bits are stored above)
                    bit = 1u << (k & 31u); cw = k >> 5;
                    const SampleColumn sc = wide_sample_column(col, cw, P.sample_first + base + 32ull * cw);
                    variant = sample_variant(sample_u(sample_column_key(sc, k & 31u), P.n_any, sample_column_lane(sc, k & 31u)),
                                             P.sample_variants);
                } else {
                    uint64_t p = base + k;
                    if (P.offsets) p = P.offsets[p];
                    // digits = first_digits + p; what spills over bit n_any goes to the variant number
                    uint64_t d[5];
                    unsigned long long carry = p;
                    for (int w = 0; w < 4; ++w) {
                        const unsigned long long a = P.first_digits[w], sum = a + carry;
                        carry = (sum < a) ? 1ull : 0ull;
                        d[w] = sum;
                    }
                    d[4] = carry;
                    const uint32_t sw = P.n_any >> 6, sb = P.n_any & 63;
                    uint64_t lo = d[0], hi = d[1];      // words sw, sw + 1 (selects: the array stays in registers)
#pragma unroll
                    for (int w = 1; w < 5; ++w) {
                        lo = (sw == (uint32_t)w) ? d[w] : lo;
                        hi = (sw + 1 == (uint32_t)w) ? d[w] : hi;
                    }
                    if (sw >= 4) hi = 0;
                    const uint64_t over = sb ? ((lo >> sb) | (hi << (64 - sb))) : lo;
                    variant = P.first_variant + over;
                    bit = 1u << (k & 31u); cw = k >> 5;
                    uint64_t sh[4] = {d[0], d[1], d[2], d[3]};
                    for (uint32_t j = 0; j < P.n_any; ++j) {
                        if (sh[0] & 1u) atomicOr(&B[0][P.any_nodes[j] * L + cw], bit);
                        sh[0] = (sh[0] >> 1) | (sh[1] << 63);
                        sh[1] = (sh[1] >> 1) | (sh[2] << 63);
                        sh[2] = (sh[2] >> 1) | (sh[3] << 63);
                        sh[3] >>= 1;
                    }
                }
                for (uint32_t j = 0; j < P.n_fv; ++j) {
                    const uint32_t range = P.fv[3 * j + 1], slot = P.fv[3 * j + 2];
                    uint32_t digit;
                    if (range == 3) { digit = (uint32_t)(variant % 3); variant /= 3; }
                    else { digit = (uint32_t)(variant & 1); variant >>= 1; }
                    const int s = wide_digit_state(range, digit);
                    if (s < 0) continue;
                    atomicOr(&fmv[(2 * slot) * L + cw], bit);
                    if (s) atomicOr(&fmv[(2 * slot + 1) * L + cw], bit);
                    else atomicAnd(&fmv[(2 * slot + 1) * L + cw], ~bit);
                }
                for (uint32_t j = 0; j < P.n_pv; ++j) {
                    const uint32_t t = P.pv[3 * j], range = P.pv[3 * j + 2];
                    uint32_t digit;
                    if (range == 3) { digit = (uint32_t)(variant % 3); variant /= 3; }
                    else { digit = (uint32_t)(variant & 1); variant >>= 1; }
                    const int s = wide_digit_state(range, digit);
                    if (s < 0) continue;
                    atomicOr(&pmv[(2 * j) * L + cw], bit);
                    if (s) atomicOr(&pmv[(2 * j + 1) * L + cw], bit);
                    if (t > tp) tp = t;                             // model.py:125
                }
                atomicMax(&misc[0], tp);
            }
            tpa[k] = tp; sta[k] = st; lam[k] = 0; mua[k] = 0;
        }
        __syncthreads();
        const uint32_t tp_max = misc[0];
        uint32_t sched_at = 0;
        uint32_t* cur = B[0];
        uint32_t* nxt = B[1];
        uint64_t group_steps = 0;

        if (mode == kWideSimulate) {
            // ---- s(0 .. T): trajectories as they pass, digest accumulators X / Y per row in B[2] / B[3]
            uint64_t T = P.max_t;
            if (P.t_len) {
                if (tid == 0) misc[1] = 0;
                __syncthreads();
                for (uint32_t k = tid; k < n_valid; k += kWideThreads) atomicMax(&misc[1], (uint32_t)P.t_len[base + k]);
                __syncthreads();
                T = misc[1];
            }
            if (P.digests)
                for (uint32_t i = tid; i < 2 * RL; i += kWideThreads) B[2][i] = 0;
            __syncthreads();
            for (uint64_t t = 0;; ++t) {
                if (P.traj) {
                    for (uint32_t i = tid; i < n_valid * P.w64; i += kWideThreads) {
                        const uint32_t k = i / P.w64, w = i % P.w64;
                        const uint64_t q = base + k;
                        const uint64_t tl = P.t_len ? P.t_len[q] : P.max_t;
                        if (t > tl) continue;
                        const uint64_t at = P.out_offsets ? P.out_offsets[q] : q * (P.max_t + 1) * P.w64;
                        P.traj[at + t * P.w64 + w] = wide_gather64(P, cur, L, k, w);
                    }
                }
                if (P.digests) {
                    const uint32_t ym = 0u - ((((uint32_t)t) * 0x9E3779B1u) >> 31);
                    for (uint32_t r = X.r0; r < X.r1; ++r) {
                        const uint32_t v = cur[r * L + c];
                        B[2][r * L + c] ^= v;
                        B[3][r * L + c] ^= v & ym;
                    }
                }
                if (t == T) break;
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                __syncthreads();
                if (wide_perturb(P, X, t + 1, nxt, pmv, sched_at)) __syncthreads();
                uint32_t* s = cur; cur = nxt; nxt = s;
                ++group_steps;
            }
            __syncthreads();
            for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
                const uint64_t q = base + k;
                if (P.digests) {
                    uint64_t dg = kDigestSeed;
                    for (uint32_t w = 0; w < P.w64; ++w) dg = (dg ^ wide_gather64(P, B[2], L, k, w)) * kDigestPrime;
                    for (uint32_t w = 0; w < P.w64; ++w) dg = (dg ^ wide_gather64(P, B[3], L, k, w)) * kDigestPrime;
                    for (uint32_t w = 0; w < P.w64; ++w) dg = (dg ^ wide_gather64(P, cur, L, k, w)) * kDigestPrime;
                    P.digests[q] = dg;
                }
                if (P.final_states)
                    for (uint32_t w = 0; w < P.w64; ++w) P.final_states[q * P.w64 + w] = wide_gather64(P, cur, L, k, w);
            }
            if (tid == 0) {
                uint64_t ref = 0;
                for (uint32_t k = 0; k < n_valid; ++k) ref += P.t_len ? P.t_len[base + k] : P.max_t;
                steps_ref += ref;
            }
        } else if (mode == kWideTarget) {
            // ---- first t >= T_p with s(t) & mask == code (target.py:109-133); a trajectory whose cycle has closed
            //      (Brent from T_max = max T_p of the group, when every trajectory is autonomous) has shown all its
            //      states and ends without a hit
            uint32_t* T = B[2];
            uint64_t t = 0, power = 1, lamc = 0;
            // (as bsx_target.hip: a max_t at or beyond the step limit is the limit, and reaching it is BSX_ERR_STEP_LIMIT)
            const uint64_t t_cap = (P.cap_inf || P.max_t >= P.step_limit) ? P.step_limit : P.max_t;
            for (;;) {
                uint32_t mism = 0, diff = 0;
                for (uint32_t r = X.r0; r < X.r1; ++r) {
                    const uint32_t v = cur[r * L + c];
                    if (r < P.n_nodes && ((P.tmask[r >> 5] >> (r & 31u)) & 1u))
                        mism |= v ^ (((P.tcode[r >> 5] >> (r & 31u)) & 1u) ? 0xFFFFFFFFu : 0u);
                    if (t > tp_max) {
                        diff |= v ^ T[r * L + c];
                        if (lamc == power) T[r * L + c] = v;
                    } else if (t == tp_max) {
                        T[r * L + c] = v;
                    }
                }
                red[tid] = mism;
                red[kWideThreads + tid] = diff;
                __syncthreads();
                bool left = false;
                if (tid < L) {
                    uint32_t m = 0, df = 0;
                    for (uint32_t s = 0; s < nslices; ++s) { m |= red[s * L + tid]; df |= red[kWideThreads + s * L + tid]; }
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32 * tid + b;
                        if (sta[k] != ST_ACTIVE) continue;
                        const uint64_t tp = tpa[k];
                        bool done = false;
                        if (t >= tp && !((m >> b) & 1u)) {
                            P.t_hit[base + k] = (uint32_t)t; done = true;
                            steps_ref += t;
                        } else if (t > tp_max && !((df >> b) & 1u)) {
                            done = true; steps_ref += t;             // cycle closed without a hit
                        } else if (t >= tp && t >= t_cap) {
                            done = true;
                            if (t_cap == P.step_limit) ++limit_hits;            // unbounded (or beyond the limit)
                            else steps_ref += t;
                        }
                        if (done) sta[k] = ST_NONE;
                        else left = true;
                    }
                }
                if (t > tp_max && lamc == power) { power <<= 1; lamc = 0; }
                if (!__syncthreads_or(left)) break;
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                __syncthreads();
                if (wide_perturb(P, X, t + 1, nxt, pmv, sched_at)) __syncthreads();
                uint32_t* s = cur; cur = nxt; nxt = s;
                ++t; ++group_steps;
                if (t > tp_max) ++lamc;
            }
        } else {
            // ---- attract.  Warm-up: bit b runs while t <= T_p(b), so the matrix ends at s(T_p) for every b
            for (uint32_t t = 1; t <= tp_max; ++t) {
                if (tid < L) {
                    uint32_t act = 0;
                    for (uint32_t b = 0; b < 32; ++b) act |= (t <= tpa[32 * tid + b] ? 1u : 0u) << b;
                    col[tid] = act;
                }
                __syncthreads();
                wide_step<K, KW>(P, X, cur, nxt, fmv, col[c]);
                __syncthreads();
                if (wide_perturb(P, X, t, nxt, pmv, sched_at)) __syncthreads();
                uint32_t* s = cur; cur = nxt; nxt = s;
                ++group_steps;
            }
            uint32_t* x0 = P.x0 + (size_t)blockIdx.x * RL;
            for (uint32_t r = X.r0; r < X.r1; ++r) x0[r * L + c] = cur[r * L + c];
            // caps: found iff T_p + mu + lambda <= max_t (S7); Brent closes the cycle within 3 (mu + lambda) + 2 steps
            // (as bsx_attract.hip: max_t - T_p at or beyond a quarter of the step limit counts as unbounded, ~0, and
            // a trajectory that runs into the step limit then makes the call fail with BSX_ERR_STEP_LIMIT)
            auto cap_of = [&](uint32_t k) -> uint64_t {
                if (P.cap_inf) return ~0ull;
                if (P.max_t < tpa[k]) return ~0ull - 1;                        // max_t < T_p: never found
                return P.max_t - tpa[k] >= P.step_limit / 4 ? ~0ull : P.max_t - tpa[k];
            };
            if (tid < L) {
                for (uint32_t b = 0; b < 32; ++b) {
                    const uint32_t k = 32 * tid + b;
                    if (sta[k] == ST_ACTIVE && !P.cap_inf && P.max_t < tpa[k]) sta[k] = ST_NONE;
                }
            }
            // ---- Brent's detector in lock step; the tortoise lives in B[2]
            {
                uint32_t* T = B[2];
                for (uint32_t r = X.r0; r < X.r1; ++r) T[r * L + c] = cur[r * L + c];
                uint64_t tau = 0, power = 1, lamc = 0;
                for (;;) {
                    bool left = false;
                    if (tid < L)
                        for (uint32_t b = 0; b < 32; ++b) left = left || sta[32 * tid + b] == ST_ACTIVE;
                    if (!__syncthreads_or(left)) break;
                    wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                    ++tau; ++lamc; ++group_steps;
                    const bool tele = lamc == power;
                    uint32_t diff = 0;
                    for (uint32_t r = X.r0; r < X.r1; ++r) {          // (own rows only: no barrier between write and read)
                        const uint32_t v = nxt[r * L + c];
                        diff |= v ^ T[r * L + c];
                        if (tele) T[r * L + c] = v;
                    }
                    red[tid] = diff;
                    __syncthreads();
                    if (tid < L) {
                        uint32_t df = 0;
                        for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                        for (uint32_t b = 0; b < 32; ++b) {
                            const uint32_t k = 32 * tid + b;
                            if (sta[k] != ST_ACTIVE) continue;
                            const uint64_t cap = cap_of(k);
                            if (!((df >> b) & 1u)) {
                                lam[k] = (uint32_t)lamc;
                                sta[k] = (uint64_t)lamc > cap ? ST_NONE : ST_CAND;
                                if (sta[k] == ST_NONE) steps_ref += P.max_t;
                            } else if (cap == ~0ull ? tau >= P.step_limit : tau >= 3 * cap + 2) {
                                sta[k] = ST_NONE;
                                if (cap == ~0ull) ++limit_hits;
                                else steps_ref += P.max_t;
                            }
                        }
                    }
                    if (tele) { power <<= 1; lamc = 0; }
                    uint32_t* s = cur; cur = nxt; nxt = s;
                }
            }
            // ---- mu: y = s(T_p + lambda) (bit b frozen after lambda_b steps) in B[0] / B[1], x = s(T_p) in B[2] / B[3]
            uint32_t lam_max = 0;
            if (tid == 0) misc[2] = 0;
            __syncthreads();
            if (tid < L)
                for (uint32_t b = 0; b < 32; ++b)
                    if (sta[32 * tid + b] == ST_CAND) atomicMax(&misc[2], lam[32 * tid + b]);
            __syncthreads();
            lam_max = misc[2];
            if (lam_max) {
                uint32_t* ya = B[0]; uint32_t* yb = B[1];
                uint32_t* xa = B[2]; uint32_t* xb = B[3];
                for (uint32_t r = X.r0; r < X.r1; ++r) { ya[r * L + c] = x0[r * L + c]; xa[r * L + c] = x0[r * L + c]; }
                for (uint32_t m = 0; m < lam_max; ++m) {
                    if (tid < L) {
                        uint32_t act = 0;
                        for (uint32_t b = 0; b < 32; ++b) act |= (m < lam[32 * tid + b] ? 1u : 0u) << b;
                        col[tid] = act;
                    }
                    __syncthreads();
                    wide_step<K, KW>(P, X, ya, yb, fmv, col[c]);
                    __syncthreads();
                    uint32_t* s = ya; ya = yb; yb = s;
                    ++group_steps;
                }
                for (uint64_t m = 0;; ++m) {
                    uint32_t diff = 0;
                    for (uint32_t r = X.r0; r < X.r1; ++r) diff |= ya[r * L + c] ^ xa[r * L + c];
                    red[tid] = diff;
                    __syncthreads();
                    bool left = false;
                    if (tid < L) {
                        uint32_t df = 0;
                        for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                        for (uint32_t b = 0; b < 32; ++b) {
                            const uint32_t k = 32 * tid + b;
                            if (sta[k] != ST_CAND) continue;
                            const uint64_t cap = cap_of(k);
                            if (!((df >> b) & 1u)) {
                                mua[k] = (uint32_t)m;
                                sta[k] = ST_FOUND;
                                steps_ref += (uint64_t)tpa[k] + m + lam[k];
                            } else if (m + 1 + lam[k] > cap) {
                                sta[k] = ST_NONE;
                                steps_ref += P.max_t;
                            } else {
                                left = true;
                            }
                        }
                    }
                    if (!__syncthreads_or(left)) break;
                    wide_step<K, KW>(P, X, ya, yb, fmv, 0xFFFFFFFFu);
                    wide_step<K, KW>(P, X, xa, xb, fmv, 0xFFFFFFFFu);
                    __syncthreads();
                    uint32_t* s = ya; ya = yb; yb = s;
                    s = xa; xa = xb; xb = s;
                    group_steps += 2;
                }
                // ---- key: minimum over a lap of lam_max steps from y (on the cycle of every found bit), min in xa
                cur = ya; nxt = yb;
                uint32_t* mn = xa;
                for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = cur[r * L + c];
                for (uint32_t m = 1; m < lam_max; ++m) {
                    wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                    __syncthreads();
                    uint32_t* s = cur; cur = nxt; nxt = s;
                    ++group_steps;
                    uint32_t lt = 0, eq = 0xFFFFFFFFu;
                    for (uint32_t r = X.r1; r-- > X.r0;) {
                        const uint32_t v = cur[r * L + c], w = mn[r * L + c];
                        lt |= eq & ~v & w;
                        eq &= ~(v ^ w);
                    }
                    red[tid] = lt;
                    red[kWideThreads + tid] = eq;
                    __syncthreads();
                    if (tid < L) {
                        uint32_t LT = 0, EQ = 0xFFFFFFFFu;
                        for (uint32_t s2 = nslices; s2-- > 0;) {
                            LT |= EQ & red[s2 * L + tid];
                            EQ &= red[kWideThreads + s2 * L + tid];
                        }
                        col[L + tid] = LT;
                    }
                    __syncthreads();
                    const uint32_t sel = col[L + c];
                    for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = wbfi(sel, cur[r * L + c], mn[r * L + c]);
                }
                __syncthreads();
                nxt = mn;       // key matrix for the records below
            }
            // ---- per-problem records
            for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
                const uint64_t q = base + k;
                const bool keep = sta[k] == ST_FOUND && (uint64_t)lam[k] <= P.max_len;      // attract.py:294
                const uint64_t tl = (uint64_t)tpa[k] + mua[k];
                P.info[4 * q + 0] = keep ? 1u : 0u;
                P.info[4 * q + 1] = keep ? lam[k] : 0u;
                P.info[4 * q + 2] = keep ? (uint32_t)tl : 0u;
                P.info[4 * q + 3] = keep ? (uint32_t)(tl >> 32) : 0u;
                for (uint32_t w = 0; w < P.w64; ++w) P.keys[q * P.w64 + w] = keep ? wide_gather64(P, nxt, L, k, w) : 0ull;
            }
        }
        steps_exec += group_steps * n_valid;
        __syncthreads();
    }
    if (steps_ref) atomicAdd(&P.ctr[0], steps_ref);
    if (tid == 0 && steps_exec) atomicAdd(&P.ctr[1], steps_exec);
    if (limit_hits) atomicAdd(&P.ctr[2], limit_hits);
}

// s(0) as w64 words and the variant number of the listed samples (bsx_sample_problems): one thread per sample, which
// owns its w64 output words.
__global__ __launch_bounds__(256) void k_sample_problems(const WideSampleListParams Q) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q.n) return;
    const uint64_t j = Q.samples[q];
    const uint64_t kb = sample_block_key(Q.k0, j >> 6);
    uint64_t* out = Q.states + q * Q.w64;
    // 'any' nodes are ascending (wide_lower_space), so one pass over them fills the words in order: each word is built
    // in a register and stored once
    uint32_t a = 0;
    for (uint32_t w = 0; w < Q.w64; ++w) {
        uint64_t word = (uint64_t)Q.origin[2 * w] | ((uint64_t)Q.origin[2 * w + 1] << 32);
        for (; a < Q.n_any && (Q.any_nodes[a] >> 6) == w; ++a)
            if (sample_any_bit(kb, a, j)) word |= 1ull << (Q.any_nodes[a] & 63u);
        out[w] = word;
    }
    if (Q.variants) Q.variants[q] = sample_variant_of(kb, Q.n_any, j, Q.variant_count);
}

hipError_t launch_sample_problems(const WideSampleListParams& Q, hipStream_t st) {
    const uint64_t blocks = (Q.n + 255) / 256;
    hipLaunchKernelGGL(k_sample_problems, dim3((uint32_t)blocks), dim3(256), 0, st, Q);
    return hipGetLastError();
}

// A call over samples of a seed (bsx_run_attract_sampled, bsx_run_target_sampled, bsx_run_simulate_sampled,
// bsx_run_trajectories_sampled): the branch of Q.mode behind the sampled set-up
template <int K, bool KW>
static const void* wide_sampled_fn(uint32_t mode) {
    if (mode == kWideTarget) return (const void*)k_wide<K, KW, true, (int)kWideTarget>;
    if (mode == kWideSimulate) return (const void*)k_wide<K, KW, true, (int)kWideSimulate>;
    return (const void*)k_wide<K, KW, true>;
}

template <int K>
static hipError_t launch_wide_sampled_k(dim3 grid, size_t shmem, hipStream_t st, const WideParams& Q) {
    const void* fn = Q.wdesc ? wide_sampled_fn<K, true>(Q.mode) : wide_sampled_fn<K, false>(Q.mode);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_sampled(int k, dim3 grid, size_t shmem, hipStream_t st, const WideParams& Q) {
    switch (k) {
        case 1: return launch_wide_sampled_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_sampled_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_sampled_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_sampled_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_sampled_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_sampled_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

template <int K>
static hipError_t launch_wide_k(dim3 grid, size_t shmem, hipStream_t st, const WideParams& P) {
    const void* fn = P.wdesc ? (const void*)k_wide<K, true> : (const void*)k_wide<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideParams*>(&P)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide(int k, dim3 grid, size_t shmem, hipStream_t st, const WideParams& P) {
    switch (k) {
        case 1: return launch_wide_k<1>(grid, shmem, st, P);
        case 2: return launch_wide_k<2>(grid, shmem, st, P);
        case 3: return launch_wide_k<3>(grid, shmem, st, P);
        case 4: return launch_wide_k<4>(grid, shmem, st, P);
        case 5: return launch_wide_k<5>(grid, shmem, st, P);
        case 6: return launch_wide_k<6>(grid, shmem, st, P);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// Attractor profile (bsx_run_attractor_profile on the wide family; layout and step function of k_wide).
namespace {

typedef Planes<(int)kWideProfileRows, kWideProfilePlanes> WidePlanes;

// Calls f(r, word) for every row r this thread owns: bit b of word = node r's bit in the key of attractor 32 c + b of
// the group (0 beyond n_valid and for padding rows).  The 32 key words of a 64-row block are loaded once per block.
template <typename F>
__device__ __forceinline__ void wide_key_rows(const WideProfileParams& Q, const WideCtx& X, uint64_t base, uint32_t n_valid, F f) {
    uint64_t kw[32];
    uint32_t have = kWideNone;
    for (uint32_t r = X.r0; r < X.r1; ++r) {
        if ((r >> 6) != have) {
            have = r >> 6;
#pragma unroll
            for (int b = 0; b < 32; ++b) {
                const uint32_t k = 32u * X.c + (uint32_t)b;
                kw[b] = (k < n_valid && have < Q.net.w64) ? Q.keys[(base + k) * Q.key_stride + have] : 0ull;
            }
        }
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) word |= (uint32_t)((kw[b] >> (r & 63u)) & 1ull) << b;
        f(r, r < Q.net.n_nodes ? word : 0u);
    }
}

// on_counts[attractor 32 c + b][node r0 + I] += count of bit b of owned row I; one owner per (attractor, node)
template <int I>
__device__ __forceinline__ void wide_flush_rows(const WidePlanes& pl, const WideProfileParams& Q, const WideCtx& X, uint64_t base,
                                                uint32_t n_valid) {
    const uint32_t r = X.r0 + (uint32_t)I;
    if ((uint32_t)I < Q.net.rows_ps && r < Q.net.n_nodes) {
        for (uint32_t b = 0; b < 32u; ++b) {
            const uint32_t k = 32u * X.c + b;
            const uint32_t cnt = planes_count_at<I>(pl, b);
            if (k < n_valid && cnt) Q.on_counts[(base + k) * Q.net.n_nodes + r] += cnt;
        }
    }
    if constexpr (I + 1 < (int)kWideProfileRows) wide_flush_rows<I + 1>(pl, Q, X, base, n_valid);
}

}  // namespace

template <int K, bool KW>
__global__ __launch_bounds__(kWideThreads) void k_wide_profile(const WideProfileParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const WideParams& P = Q.net;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t nslices = kWideThreads / L;
    uint32_t* cur = sm;
    uint32_t* nxt = sm + RL;
    uint32_t* fmv = sm + 2 * RL;                    // [n_fslots][2][L]  all zero: no variations here
    uint32_t* red = fmv + 2 * P.n_fslots * L;       // [256]             per-thread partials
    uint32_t* col = red + kWideThreads;             // [2][L]            live masks of step t and t + 1
    uint32_t* len = col + 2 * L;                    // [G]               lengths (0 beyond n_valid)
    uint32_t* misc = len + G;                       // [8]
    unsigned long long steps_exec = 0;
    for (uint32_t i = tid; i < 2 * P.n_fslots * L; i += kWideThreads) fmv[i] = 0;

    const uint64_t n_groups = (Q.count + G - 1) / G;
    for (uint64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
        const uint64_t base = group * G;
        const uint32_t n_valid = (uint32_t)((Q.count - base) < G ? (Q.count - base) : G);
        if (tid < 8) misc[tid] = 0;
        __syncthreads();
        // ---- lengths, and the keys deposited into the matrix
        for (uint32_t k = tid; k < G; k += kWideThreads) {
            const uint32_t l = k < n_valid ? (uint32_t)Q.lengths[base + k] : 0u;
            len[k] = l;
            if (l) atomicMax(&misc[0], l);
        }
        wide_key_rows(Q, X, base, n_valid, [&](uint32_t r, uint32_t word) { cur[r * L + c] = word; });
        __syncthreads();
        const uint32_t lam_max = misc[0];
        if (tid < L) {
            uint32_t act = 0;
            for (uint32_t b = 0; b < 32; ++b) act |= (len[32 * tid + b] ? 1u : 0u) << b;
            col[tid] = act;
        }
        __syncthreads();
        // ---- the walk: bit b counts, is stored and advances while t < length_b
        WidePlanes pl;
        planes_clear(pl);
        uint32_t pending = 0;
        for (uint32_t t = 0; t < lam_max; ++t) {
            const uint32_t live = col[(t & 1u) * L + c];
            if (Q.on_counts) {
                uint32_t v[kWideProfileRows];
#pragma unroll
                for (int i = 0; i < (int)kWideProfileRows; ++i) v[i] = (uint32_t)i < P.rows_ps ? cur[(X.r0 + (uint32_t)i) * L + c] & live : 0u;
                planes_add(pl, v);
                if (++pending == WidePlanes::kFlushEvery) {
                    wide_flush_rows<0>(pl, Q, X, base, n_valid);
                    planes_clear(pl);
                    pending = 0;
                }
            }
            if (Q.states) {
                for (uint32_t i = tid; i < n_valid * P.w64; i += kWideThreads) {
                    const uint32_t k = i / P.w64, w = i % P.w64;
                    if (t < len[k]) Q.states[Q.state_offsets[base + k] + (uint64_t)t * P.w64 + w] = wide_gather64(P, cur, L, k, w);
                }
            }
            wide_step<K, KW>(P, X, cur, nxt, fmv, live);
            if (tid < L) {
                uint32_t act = 0;
                for (uint32_t b = 0; b < 32; ++b) act |= (t + 1 < len[32 * tid + b] ? 1u : 0u) << b;
                col[((t + 1) & 1u) * L + tid] = act;
            }
            __syncthreads();
            uint32_t* s = cur; cur = nxt; nxt = s;
        }
        if (Q.on_counts && pending) wide_flush_rows<0>(pl, Q, X, base, n_valid);
        // ---- closed: bit b was frozen at f^length_b(key_b); no row may differ from the key in that bit
        if (Q.closed) {
            uint32_t diff = 0;
            wide_key_rows(Q, X, base, n_valid, [&](uint32_t r, uint32_t word) { diff |= word ^ cur[r * L + c]; });
            red[tid] = diff;
            __syncthreads();
            if (tid < L) {
                uint32_t df = 0;
                for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                for (uint32_t b = 0; b < 32; ++b) {
                    const uint32_t k = 32 * tid + b;
                    if (k < n_valid) Q.closed[base + k] = ((df >> b) & 1u) ? 0 : 1;
                }
            }
        }
        steps_exec += (unsigned long long)lam_max * n_valid;
        __syncthreads();
    }
    if (tid == 0 && steps_exec) atomicAdd(&Q.ctr[1], steps_exec);
}

template <int K>
static hipError_t launch_wide_profile_k(dim3 grid, size_t shmem, hipStream_t st, const WideProfileParams& Q) {
    const void* fn = Q.net.wdesc ? (const void*)k_wide_profile<K, true> : (const void*)k_wide_profile<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideProfileParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_profile(int k, dim3 grid, size_t shmem, hipStream_t st, const WideProfileParams& Q) {
    switch (k) {
        case 1: return launch_wide_profile_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_profile_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_profile_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_profile_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_profile_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_profile_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// Damage spreading (bsx_run_damage_sampled; include/bsx.h has the definition, bsx_wide.h the layout).  Per lock step: two
// wide_step calls, one vertical counter add per owned row of X ^ Y, the counters of the slices combined per sample
// through LDS, and the step's three sums reduced per wave and then per workgroup.
namespace {
typedef Planes<1, (int)kWideDamagePlanes> DamagePlanes;
}

template <int K, bool KW>
__global__ __launch_bounds__(kWideThreads) void k_wide_damage(const WideDamageParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const WideParams& P = Q.net;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t nslices = kWideThreads / L;
    const uint32_t n_bins = P.n_nodes + 1;
    const uint32_t n_acc = Q.acc_lds ? 3 * (Q.n_steps + 1) : 0;
    const uint32_t mask_words = (Q.n_free + 31u) >> 5;             // of a sample's chosen positions; <= rows / 32
    uint32_t* B[4] = {sm, sm + RL, sm + 2 * RL, sm + 3 * RL};       // X: 0 / 1, Y: 2 / 3
    uint32_t* fmv = sm + 4 * RL;                    // [n_fslots][2][L]  all zero: no variations here
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(fmv + 2 * P.n_fslots * L);      // [n_steps + 1][3] (acc_lds)
    uint32_t* pln = reinterpret_cast<uint32_t*>(acc + n_acc);       // [6][256]  every thread's planes
    uint32_t* keys = pln + kWideDamagePlanes * kWideThreads;        // [L][4]    block keys of the columns
    uint32_t* gacc = keys + 4 * L;                  // [2][4]            sums of step t in half t & 1
    uint32_t* lh = gacc + 8;                        // [n_nodes + 1]     histogram of the step (hist)
    unsigned long long steps_exec = 0;
    for (uint32_t i = tid; i < 2 * P.n_fslots * L; i += kWideThreads) fmv[i] = 0;
    for (uint32_t i = tid; i < n_acc; i += kWideThreads) acc[i] = 0ull;
    if (Q.hist)
        for (uint32_t i = tid; i < n_bins; i += kWideThreads) lh[i] = 0;
    // sums[t][q] += v: in LDS until the workgroup ends (one owner per address and phase), else straight to HBM
    auto add = [&](uint32_t t, uint32_t q, unsigned long long v) {
        if (Q.acc_lds) acc[3 * t + q] += v;
        else if (v) atomicAdd(&Q.sums[3 * (size_t)t + q], v);
    };

    const uint64_t n_groups = (P.count + G - 1) / G;
    for (uint64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
        const uint64_t base = group * G;
        const uint32_t n_valid = (uint32_t)((P.count - base) < G ? (P.count - base) : G);
        // ---- x(0) = y(0) = origin | 'any' words of the sampled source; the chosen-position masks (matrix 3) start empty
        for (uint32_t i = tid; i < RL; i += kWideThreads) {
            const uint32_t r = i >> P.lshift;
            B[0][i] = B[2][i] = (r < P.n_nodes && ((P.origin[r >> 5] >> (r & 31u)) & 1u)) ? 0xFFFFFFFFu : 0u;
        }
        for (uint32_t i = tid; i < mask_words * G; i += kWideThreads) B[3][i] = 0;
        if (tid < L) {
            const SampleColumn sc = sample_column(P.sample_k0, P.sample_first + base + 32ull * tid);
            keys[4 * tid + 0] = (uint32_t)sc.kb0; keys[4 * tid + 1] = (uint32_t)(sc.kb0 >> 32);
            keys[4 * tid + 2] = (uint32_t)sc.kb1; keys[4 * tid + 3] = (uint32_t)(sc.kb1 >> 32);
        }
        __syncthreads();
        for (uint32_t i = tid; i < P.n_any * L; i += kWideThreads) {
            const uint32_t a = i >> P.lshift, cw = i & (L - 1);
            const SampleColumn sc = wide_sample_column(keys, cw, P.sample_first + base + 32ull * cw);
            const uint32_t n_bits = n_valid > 32 * cw ? (n_valid - 32 * cw < 32u ? n_valid - 32 * cw : 32u) : 0u;
            const uint32_t word = sample_column_word(sc, a, n_bits);
            B[0][P.any_nodes[a] * L + cw] = word;
            B[2][P.any_nodes[a] * L + cw] = word;
        }
        __syncthreads();
        // ---- y(0): n_flips distinct free nodes inverted per sample.  The positions chosen so far are a bit mask in LDS
        // (word w of sample k at B[3][w * G + k]), not a list in registers.
        for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
            const uint32_t cw = k >> 5, bit = 1u << (k & 31u);
            const SampleColumn sc = wide_sample_column(keys, cw, P.sample_first + base + 32ull * cw);
            const uint64_t kb = sample_column_key(sc, k & 31u);
            const uint32_t lane = sample_column_lane(sc, k & 31u);
            for (uint32_t i = 0; i < Q.n_flips; ++i) {
                const uint32_t p = damage_choose(damage_draw(kb, P.n_any, lane, i), Q.n_free, i, B[3] + k, G);
                if (p < Q.n_free) atomicXor(&B[2][Q.free_nodes[p] * L + cw], bit);
            }
        }
        __syncthreads();
        uint32_t *xc = B[0], *xn = B[1], *yc = B[2], *yn = B[3];
        uint32_t group_steps = 0;
        for (uint32_t t = 0;; ++t) {
            uint32_t* ga = gacc + 4 * (t & 1u);
            if (tid < 4) ga[tid] = 0;               // (last read two steps ago, or in the group before)
            // ---- d(t): column sums of X ^ Y over the owned rows (written by this thread), then over the slices
            DamagePlanes pl;
            planes_clear(pl);
            for (uint32_t r = X.r0; r < X.r1; ++r) {
                const uint32_t s[1] = {xc[r * L + c] ^ yc[r * L + c]};
                planes_add(pl, s);
            }
#pragma unroll
            for (int j = 0; j < (int)kWideDamagePlanes; ++j) pln[j * kWideThreads + tid] = pl.p[j][0];
            __syncthreads();
            uint32_t sd = 0, sd2 = 0, mg = 0;       // per group and step: sum d <= 2^21, sum d^2 <= 2^31
            for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
                const uint32_t cw = k >> 5, b = k & 31u;
                uint32_t d = 0;
                for (uint32_t s = 0; s < nslices; ++s) {
                    uint32_t cnt = 0;
#pragma unroll
                    for (int j = 0; j < (int)kWideDamagePlanes; ++j) cnt |= ((pln[j * kWideThreads + s * L + cw] >> b) & 1u) << j;
                    d += cnt;
                }
                sd += d; sd2 += d * d; mg += d == 0 ? 1u : 0u;
                if (Q.hist) atomicAdd(&lh[d], 1u);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                sd += __shfl_xor(sd, off); sd2 += __shfl_xor(sd2, off); mg += __shfl_xor(mg, off);
            }
            if ((tid & 63u) == 0) { atomicAdd(&ga[0], sd); atomicAdd(&ga[1], sd2); atomicAdd(&ga[2], mg); }
            const bool last = t == Q.n_steps;
            if (!last) {
                wide_step<K, KW>(P, X, xc, xn, fmv, 0xFFFFFFFFu);
                wide_step<K, KW>(P, X, yc, yn, fmv, 0xFFFFFFFFu);
                ++group_steps;
            }
            __syncthreads();
            if (tid < 3) add(t, tid, ga[tid]);
            if (Q.hist) {
                for (uint32_t i = tid; i < n_bins; i += kWideThreads) {
                    const uint32_t v = lh[i];
                    if (v) { atomicAdd(&Q.hist[(size_t)t * n_bins + i], (unsigned long long)v); lh[i] = 0; }
                }
            }
            if (last) break;
            if (ga[2] == n_valid) {
                // every pair of the group has merged, and merged pairs stay merged: d = 0 from here on
                for (uint32_t t2 = t + 1 + tid; t2 <= Q.n_steps; t2 += kWideThreads) {
                    add(t2, 2, n_valid);
                    if (Q.hist) atomicAdd(&Q.hist[(size_t)t2 * n_bins], (unsigned long long)n_valid);
                }
                break;
            }
            uint32_t* s = xc; xc = xn; xn = s;
            s = yc; yc = yn; yn = s;
        }
        steps_exec += 2ull * group_steps * n_valid;
        __syncthreads();
    }
    for (uint32_t i = tid; i < n_acc; i += kWideThreads)
        if (acc[i]) atomicAdd(&Q.sums[i], acc[i]);
    if (tid == 0 && steps_exec) atomicAdd(&P.ctr[1], steps_exec);
}

template <int K>
static hipError_t launch_wide_damage_k(dim3 grid, size_t shmem, hipStream_t st, const WideDamageParams& Q) {
    const void* fn = Q.net.wdesc ? (const void*)k_wide_damage<K, true> : (const void*)k_wide_damage<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideDamageParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_damage(int k, dim3 grid, size_t shmem, hipStream_t st, const WideDamageParams& Q) {
    switch (k) {
        case 1: return launch_wide_damage_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_damage_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_damage_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_damage_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_damage_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_damage_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// Node influence (bsx_run_influence_sampled; include/bsx.h has the definition, bsx_wide.h / bsx_influence.h the layout).
// A workgroup's work items are (source, group) pairs: damage's set-up with one row of Y inverted instead of drawn flips,
// then per lock step two wide_step calls and the counts of X ^ Y per row.
//
// Counts.  Behind the step every thread holds the words it has just written for its owned rows of its column; row r of a
// slice lies in the L adjacent lanes of that slice.  Most rows are zero in an ordered network, so a lane does nothing for
// a zero word and adds the popcount of a nonzero one to the row's LDS counter: up to L adders on one address, which the
// LDS serialises.  (BSX_INFLUENCE_COUNTS = 1 builds the alternative: one ballot per row, and where a wave holds a nonzero
// word the popcounts summed over the slice's L lanes by shuffles, then one adder per row.  It measured 9 to 25 % slower,
// DESIGN.md "Node influence" in section 5 has the figures; 0 compiles the count stage out.  Both are for measurements only.)
// The counters and the per-column ORs come in two halves by the parity of t: a step's half is flushed and cleared behind
// the step's barrier, while the next step already adds to the other half, so a lock step has one barrier.
#if !defined(BSX_INFLUENCE_COUNTS)
#define BSX_INFLUENCE_COUNTS 2
#endif

template <int K, bool KW>
__global__ __launch_bounds__(kWideThreads) void k_wide_influence(const WideInfluenceParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const WideParams& P = Q.net;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t T = Q.n_steps, n = P.n_nodes;
    uint32_t* B[4] = {sm, sm + RL, sm + 2 * RL, sm + 3 * RL};       // X: 0 / 1, Y: 2 / 3
    uint32_t* fmv = sm + 4 * RL;                    // [n_fslots][2][L]  all zero: no variations here
    uint32_t* cnt = fmv + 2 * P.n_fslots * L;       // [2][rows]         counts of step t in half t & 1; zero between steps
    uint32_t* colv = cnt + 2 * P.rows;              // [2][L]            OR of the column's diff words, likewise
    uint32_t* keys = colv + 2 * L;                  // [L][4]            block keys of the columns
    unsigned long long steps_exec = 0;
    for (uint32_t i = tid; i < 2 * P.n_fslots * L; i += kWideThreads) fmv[i] = 0;
    for (uint32_t i = tid; i < 2 * P.rows + 2 * L; i += kWideThreads) cnt[i] = 0;

    for (uint64_t pi = blockIdx.x; pi < Q.n_items; pi += gridDim.x) {
        const InfluenceItem item = influence_item_of(Q.p0 + pi, Q.g_per, Q.n_samples, G);
        const uint32_t n_valid = item.n_valid;
        const uint64_t j_first = Q.first_sample + item.first;               // the group's first sample
        const uint32_t src = Q.sources[item.source];                        // uniform: a scalar load
        const size_t row0 = (size_t)item.source * T;                        // row (source, t) of the tables is row0 + t - 1
        // ---- x(0) = y(0) = origin | 'any' words of the sampled source (damage's set-up)
        for (uint32_t i = tid; i < RL; i += kWideThreads) {
            const uint32_t r = i >> P.lshift;
            B[0][i] = B[2][i] = (r < n && ((P.origin[r >> 5] >> (r & 31u)) & 1u)) ? 0xFFFFFFFFu : 0u;
        }
        if (tid < L) {
            const SampleColumn sc = sample_column(P.sample_k0, j_first + 32ull * tid);
            keys[4 * tid + 0] = (uint32_t)sc.kb0; keys[4 * tid + 1] = (uint32_t)(sc.kb0 >> 32);
            keys[4 * tid + 2] = (uint32_t)sc.kb1; keys[4 * tid + 3] = (uint32_t)(sc.kb1 >> 32);
        }
        __syncthreads();
        for (uint32_t i = tid; i < P.n_any * L; i += kWideThreads) {
            const uint32_t a = i >> P.lshift, cw = i & (L - 1);
            const SampleColumn sc = wide_sample_column(keys, cw, j_first + 32ull * cw);
            const uint32_t n_bits = n_valid > 32 * cw ? (n_valid - 32 * cw < 32u ? n_valid - 32 * cw : 32u) : 0u;
            const uint32_t word = sample_column_word(sc, a, n_bits);
            B[0][P.any_nodes[a] * L + cw] = word;
            B[2][P.any_nodes[a] * L + cw] = word;
        }
        __syncthreads();
        // ---- y(0): row `src` inverted in the valid bits of every column; the bits behind the end of a ragged group stay
        // equal in X and Y, and so are never counted
        uint32_t valid = 0;                         // of column tid (tid < L)
        if (tid < L) {
            const uint32_t n_bits = n_valid > 32 * tid ? (n_valid - 32 * tid < 32u ? n_valid - 32 * tid : 32u) : 0u;
            valid = n_bits >= 32u ? 0xFFFFFFFFu : (1u << n_bits) - 1u;
            B[2][src * L + tid] ^= valid;
        }
        __syncthreads();
        uint32_t *xc = B[0], *xn = B[1], *yc = B[2], *yn = B[3];
        uint32_t group_steps = 0;
        for (uint32_t t = 1; t <= T; ++t) {
            uint32_t* ct = cnt + (t & 1u) * P.rows;
            uint32_t* cv = colv + (t & 1u) * L;
            wide_step<K, KW>(P, X, xc, xn, fmv, 0xFFFFFFFFu);
            wide_step<K, KW>(P, X, yc, yn, fmv, 0xFFFFFFFFu);
            ++group_steps;
            // ---- the rows this thread has just written: OR of the diff words, counts of the nonzero ones
            uint32_t orv = 0;
            for (uint32_t r = X.r0; r < X.r1; ++r) {
                const uint32_t d = xn[r * L + c] ^ yn[r * L + c];
                orv |= d;
#if BSX_INFLUENCE_COUNTS == 1
                if (__builtin_amdgcn_ballot_w64(d != 0u)) {
                    uint32_t s = (uint32_t)__builtin_popcount(d);
                    for (uint32_t off = 1; off < L && off < 64u; off <<= 1) s += __shfl_xor(s, (int)off);
                    if ((c & 63u) == 0 && s) atomicAdd(&ct[r], s);      // (L > 64: a row spans waves, hence an add, not a store)
                }
#elif BSX_INFLUENCE_COUNTS == 2
                if (d) atomicAdd(&ct[r], (uint32_t)__builtin_popcount(d));
#endif
            }
            if (orv) atomicOr(&cv[c], orv);
            const bool alive = __syncthreads_or(orv != 0u);
            // ---- flush: one global add per nonzero (source, t, row); merged = the valid bits that no row has set
            uint32_t* out = Q.influence + (row0 + t - 1) * n;
            for (uint32_t i = tid; i < n; i += kWideThreads) {
                const uint32_t v = ct[i];
                if (v) { atomicAdd(&out[i], v); ct[i] = 0; }
            }
            if (Q.n_merged) {
                uint32_t mg = 0;
                if (tid < L) { mg = (uint32_t)__builtin_popcount(valid & ~cv[tid]); cv[tid] = 0; }
                if (tid < ((L + 63u) & ~63u)) {         // the waves that hold a column: whole waves, so the shuffles are uniform
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) mg += __shfl_xor(mg, off);
                    if ((tid & 63u) == 0 && mg) atomicAdd(&Q.n_merged[row0 + t - 1], (unsigned long long)mg);
                }
            } else if (tid < L) {
                cv[tid] = 0;
            }
            if (!alive) {
                // every pair of the group has merged, and merged pairs stay merged: nothing differs from here on
                if (Q.n_merged)
                    for (uint32_t t2 = t + 1 + tid; t2 <= T; t2 += kWideThreads) atomicAdd(&Q.n_merged[row0 + t2 - 1], (unsigned long long)n_valid);
                break;
            }
            uint32_t* s = xc; xc = xn; xn = s;
            s = yc; yc = yn; yn = s;
        }
        steps_exec += 2ull * group_steps * n_valid;
        __syncthreads();
    }
    if (tid == 0 && steps_exec) atomicAdd(&P.ctr[1], steps_exec);
}

template <int K>
static hipError_t launch_wide_influence_k(dim3 grid, size_t shmem, hipStream_t st, const WideInfluenceParams& Q) {
    const void* fn = Q.net.wdesc ? (const void*)k_wide_influence<K, true> : (const void*)k_wide_influence<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideInfluenceParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_influence(int k, dim3 grid, size_t shmem, hipStream_t st, const WideInfluenceParams& Q) {
    switch (k) {
        case 1: return launch_wide_influence_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_influence_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_influence_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_influence_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_influence_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_influence_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// Attractor transitions (bsx_run_attractor_transitions_wide; bsx_wide.h has the stages, bsx_wtrans.h the lookup and
// the classification).  The walk is k_wide's attract branch with T_p = 0, no schedule and no variations.
namespace {

// Deposits the 64-bit state words src(k, w) of the group's trajectories k into matrix `dst` (rows this thread owns,
// as wide_key_rows): bit b of dst[r][c] = node r of trajectory 32 c + b.
template <typename F>
__device__ __forceinline__ void wide_trans_deposit(const WideParams& P, const WideCtx& X, uint32_t* dst, F src) {
    uint64_t kw[32];
    uint32_t have = kWideNone;
    for (uint32_t r = X.r0; r < X.r1; ++r) {
        if ((r >> 6) != have) {
            have = r >> 6;
#pragma unroll
            for (int b = 0; b < 32; ++b) kw[b] = have < P.w64 ? src(32u * X.c + (uint32_t)b, have) : 0ull;
        }
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) word |= (uint32_t)((kw[b] >> (r & 63u)) & 1ull) << b;
        dst[r * X.L + X.c] = r < P.n_nodes ? word : 0u;
    }
}

// largest q with row_first[q] <= g  (row_first ascending, row_first[0] == 0)
__device__ __forceinline__ uint32_t wide_trans_row_of(const uint64_t* row_first, uint64_t n_rows, uint64_t g) {
    uint64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (row_first[mid] <= g) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}

// Insert-or-add into the HBM edge table (as trans_edge_global of bsx_trans_kernel.h): the key word is claimed by one
// 64-bit CAS; count and sum take atomic adds.  At most one round of the table.
__device__ __forceinline__ void wide_trans_edge_global(const WideTransParams& Q, unsigned long long key, unsigned long long count,
                                                       unsigned long long sum_mu) {
    uint64_t at = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & Q.edge_mask;
    for (uint64_t probe = 0; probe <= Q.edge_mask; ++probe, at = (at + 1) & Q.edge_mask) {
        TransEdgeSlot* slot = Q.edges + at;
        unsigned long long seen = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0) seen = atomicCAS(&slot->key, 0ull, key);
        if (seen == 0 || seen == key) {
            atomicAdd(&slot->count, count);
            if (sum_mu) atomicAdd(&slot->sum_mu, sum_mu);
            return;
        }
    }
    atomicAdd(&Q.ctr->edge_overflow, 1u);
}

}  // namespace

template <int K, bool KW>
__global__ __launch_bounds__(kWideThreads) void k_wide_trans(const WideTransParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const WideParams& P = Q.net;
    const bool flips = Q.stage == kWideTransFlips;
    // refused tables (a row that is not closed or undecided, two rows on one cycle) are known on the device only: the
    // launches before this one left them in the counters, and no flip is walked
    if (flips && (Q.ctr->open_row != kTransNoRow || Q.ctr->dup_row != kTransNoRow || Q.ctr->probe_full || Q.ctr->rows_undecided)) return;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t nslices = kWideThreads / L;
    uint32_t* B[4] = {sm, sm + RL, sm + 2 * RL, sm + 3 * RL};
    uint32_t* fmv = sm + 4 * RL;                    // [n_fslots][2][L]  all zero: no variations here
    uint32_t* red = fmv + 2 * P.n_fslots * L;       // [2][256]          per-thread partials
    uint32_t* col = red + 2 * kWideThreads;         // [8][L]            per-column masks
    uint32_t* src = col + 8 * L;                    // [G] flips: index of the listed state
    uint32_t* lam = src + G;                        // [G] lambda
    uint32_t* mua = lam + G;                        // [G] mu (while the group is set up: the flipped node)
    uint32_t* sta = mua + G;                        // [G] state of the trajectory's search
    uint32_t* misc = sta + G;                       // [8]
    enum : uint32_t { ST_ACTIVE = 0, ST_CAND = 1, ST_FOUND = 2, ST_NONE = 3, ST_INVALID = 4 };
    unsigned long long steps_exec = 0;
    unsigned int limit_hits = 0;
    for (uint32_t i = tid; i < 2 * P.n_fslots * L; i += kWideThreads) fmv[i] = 0;
    // found iff mu + lambda <= max_t; a max_t at or beyond a quarter of the step limit counts as unbounded (k_wide), and
    // the rows' own walks are never capped
    const uint64_t cap = (!flips || P.cap_inf || P.max_t >= P.step_limit / 4) ? ~0ull : P.max_t;

    const uint64_t n_groups = (Q.count + G - 1) / G;
    for (uint64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
        const uint64_t base = group * G;
        const uint32_t n_valid = (uint32_t)((Q.count - base) < G ? (Q.count - base) : G);
        if (tid < 8) misc[tid] = 0;
        for (uint32_t k = tid; k < G; k += kWideThreads) {
            uint32_t st = ST_INVALID, g = 0, node = 0;
            if (k < n_valid) {
                const uint64_t id = Q.first + base + k;
                if (flips) {
                    const uint64_t s = id / Q.n_free;
                    g = (uint32_t)s;                                    // (< BSX_TRANS_MAX_STATES)
                    node = Q.free_nodes[(uint32_t)(id - s * Q.n_free)];
                    st = ST_ACTIVE;
                } else if (Q.closed[id]) {
                    st = ST_ACTIVE;
                }
            }
            src[k] = g; mua[k] = node; sta[k] = st; lam[k] = 0;
        }
        __syncthreads();
        // ---- x_0: a row's key, or a listed state with one bit inverted
        wide_trans_deposit(P, X, B[0], [&](uint32_t k, uint32_t w) -> uint64_t {
            if (sta[k] != ST_ACTIVE) return 0ull;
            if (!flips) return Q.keys[(Q.first + base + k) * Q.key_stride + w];
            const uint64_t word = Q.states[(uint64_t)src[k] * P.w64 + w];
            return (mua[k] >> 6) == w ? word ^ (1ull << (mua[k] & 63u)) : word;
        });
        __syncthreads();
        for (uint32_t k = tid; k < G; k += kWideThreads) mua[k] = 0;
        uint32_t* cur = B[0];
        uint32_t* nxt = B[1];
        uint64_t group_steps = 0;
        uint32_t* x0 = P.x0 + (size_t)blockIdx.x * RL;
        for (uint32_t r = X.r0; r < X.r1; ++r) x0[r * L + c] = cur[r * L + c];
        // ---- Brent's detector in lock step; the tortoise lives in B[2]
        {
            uint32_t* T = B[2];
            for (uint32_t r = X.r0; r < X.r1; ++r) T[r * L + c] = cur[r * L + c];
            uint64_t tau = 0, power = 1, lamc = 0;
            for (;;) {
                bool left = false;
                if (tid < L)
                    for (uint32_t b = 0; b < 32; ++b) left = left || sta[32 * tid + b] == ST_ACTIVE;
                if (!__syncthreads_or(left)) break;
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                ++tau; ++lamc; ++group_steps;
                const bool tele = lamc == power;
                uint32_t diff = 0;
                for (uint32_t r = X.r0; r < X.r1; ++r) {          // (own rows only: no barrier between write and read)
                    const uint32_t v = nxt[r * L + c];
                    diff |= v ^ T[r * L + c];
                    if (tele) T[r * L + c] = v;
                }
                red[tid] = diff;
                __syncthreads();
                if (tid < L) {
                    uint32_t df = 0;
                    for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32 * tid + b;
                        if (sta[k] != ST_ACTIVE) continue;
                        if (!((df >> b) & 1u)) {
                            lam[k] = (uint32_t)lamc;
                            sta[k] = (uint64_t)lamc > cap ? ST_NONE : ST_CAND;
                        } else if (cap == ~0ull ? tau >= P.step_limit : tau >= 3 * cap + 2) {
                            sta[k] = ST_NONE;
                            if (cap == ~0ull) ++limit_hits;
                        }
                    }
                }
                if (tele) { power <<= 1; lamc = 0; }
                uint32_t* s = cur; cur = nxt; nxt = s;
            }
        }
        // ---- mu: y = s(lambda) (bit b frozen after lambda_b steps) in B[0] / B[1], x = s(0) in B[2] / B[3]
        if (tid == 0) misc[2] = 0;
        __syncthreads();
        if (tid < L)
            for (uint32_t b = 0; b < 32; ++b)
                if (sta[32 * tid + b] == ST_CAND) atomicMax(&misc[2], lam[32 * tid + b]);
        __syncthreads();
        const uint32_t lam_max = misc[2];
        uint32_t* mn = B[2];
        if (lam_max) {
            uint32_t* ya = B[0]; uint32_t* yb = B[1];
            uint32_t* xa = B[2]; uint32_t* xb = B[3];
            for (uint32_t r = X.r0; r < X.r1; ++r) { ya[r * L + c] = x0[r * L + c]; xa[r * L + c] = x0[r * L + c]; }
            for (uint32_t m = 0; m < lam_max; ++m) {
                if (tid < L) {
                    uint32_t act = 0;
                    for (uint32_t b = 0; b < 32; ++b) act |= (m < lam[32 * tid + b] ? 1u : 0u) << b;
                    col[tid] = act;
                }
                __syncthreads();
                wide_step<K, KW>(P, X, ya, yb, fmv, col[c]);
                __syncthreads();
                uint32_t* s = ya; ya = yb; yb = s;
                ++group_steps;
            }
            for (uint64_t m = 0;; ++m) {
                uint32_t diff = 0;
                for (uint32_t r = X.r0; r < X.r1; ++r) diff |= ya[r * L + c] ^ xa[r * L + c];
                red[tid] = diff;
                __syncthreads();
                bool left = false;
                if (tid < L) {
                    uint32_t df = 0;
                    for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32 * tid + b;
                        if (sta[k] != ST_CAND) continue;
                        if (!((df >> b) & 1u)) {
                            mua[k] = (uint32_t)m;
                            sta[k] = ST_FOUND;
                        } else if (m + 1 + lam[k] > cap) {
                            sta[k] = ST_NONE;
                        } else if (m >= P.step_limit) {
                            sta[k] = ST_NONE;
                            ++limit_hits;
                        } else {
                            left = true;
                        }
                    }
                }
                if (!__syncthreads_or(left)) break;
                wide_step<K, KW>(P, X, ya, yb, fmv, 0xFFFFFFFFu);
                wide_step<K, KW>(P, X, xa, xb, fmv, 0xFFFFFFFFu);
                __syncthreads();
                uint32_t* s = ya; ya = yb; yb = s;
                s = xa; xa = xb; xb = s;
                group_steps += 2;
            }
            // ---- key: minimum over a lap of lam_max steps from y (on the cycle of every found bit), min in xa
            cur = ya; nxt = yb;
            mn = xa;
            for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = cur[r * L + c];
            for (uint32_t m = 1; m < lam_max; ++m) {
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                __syncthreads();
                uint32_t* s = cur; cur = nxt; nxt = s;
                ++group_steps;
                uint32_t lt = 0, eq = 0xFFFFFFFFu;
                for (uint32_t r = X.r1; r-- > X.r0;) {
                    const uint32_t v = cur[r * L + c], w = mn[r * L + c];
                    lt |= eq & ~v & w;
                    eq &= ~(v ^ w);
                }
                red[tid] = lt;
                red[kWideThreads + tid] = eq;
                __syncthreads();
                if (tid < L) {
                    uint32_t LT = 0, EQ = 0xFFFFFFFFu;
                    for (uint32_t s2 = nslices; s2-- > 0;) {
                        LT |= EQ & red[s2 * L + tid];
                        EQ &= red[kWideThreads + s2 * L + tid];
                    }
                    col[L + tid] = LT;
                }
                __syncthreads();
                const uint32_t sel = col[L + c];
                for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = wbfi(sel, cur[r * L + c], mn[r * L + c]);
            }
        }
        __syncthreads();
        if (!flips) {
            // ---- per row: true period, mu, canonical key
            for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
                const uint64_t q = Q.first + base + k;
                const bool found = sta[k] == ST_FOUND;
                Q.row_info[2 * q + 0] = found ? lam[k] : 0u;
                Q.row_info[2 * q + 1] = found ? mua[k] : 0u;
                for (uint32_t w = 0; w < P.w64; ++w) Q.row_keys[q * P.w64 + w] = found ? wide_gather64(P, mn, L, k, w) : 0ull;
            }
        } else {
            // ---- per flip: the key among the rows' keys, the edge; the group's edges meet in LDS first (in the first
            //      matrix: the minimum lies in the third or fourth, nothing else is read any more)
            TransEdgeSlot* lds_edges = reinterpret_cast<TransEdgeSlot*>(B[0]);
            for (uint32_t e = tid; e < kTransLdsEdges; e += kWideThreads) lds_edges[e] = TransEdgeSlot{0ull, 0ull, 0ull};
            __syncthreads();
            for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
                const uint64_t f = Q.first + base + k;
                const uint32_t node = Q.free_nodes[(uint32_t)(f - (uint64_t)src[k] * Q.n_free)];
                const uint32_t q = wide_trans_row_of(Q.row_first, Q.n_rows, src[k]);
                const bool found = sta[k] == ST_FOUND;
                uint32_t row = kWtransNoRow;
                if (found)
                    row = wtrans_find_of(Q.owners, Q.slot_mask, Q.row_keys, P.w64, [&](uint32_t w) { return wide_gather64(P, mn, L, k, w); });
                const WtransEdge edge = wtrans_classify(found, lam[k], mua[k], row, P.cap_inf ? kWtransInf : P.max_t);
                if (Q.node_exits && edge.dst != q) atomicAdd(&Q.node_exits[(uint64_t)q * P.n_nodes + node], 1u);
                const unsigned long long key = (((unsigned long long)q << 32) | edge.dst) + 1ull;
                uint32_t at = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & (kTransLdsEdges - 1);
                bool placed = false;
                for (uint32_t probe = 0; probe < kTransLdsProbes && !placed; ++probe, at = (at + 1) & (kTransLdsEdges - 1)) {
                    unsigned long long seen = lds_edges[at].key;
                    if (seen == 0) seen = atomicCAS(&lds_edges[at].key, 0ull, key);
                    if (seen == 0 || seen == key) {
                        atomicAdd(&lds_edges[at].count, 1ull);
                        if (edge.mu) atomicAdd(&lds_edges[at].sum_mu, (unsigned long long)edge.mu);
                        placed = true;
                    }
                }
                if (!placed) wide_trans_edge_global(Q, key, 1ull, edge.mu);
            }
            __syncthreads();
            for (uint32_t e = tid; e < kTransLdsEdges; e += kWideThreads)
                if (lds_edges[e].key) wide_trans_edge_global(Q, lds_edges[e].key, lds_edges[e].count, lds_edges[e].sum_mu);
        }
        steps_exec += group_steps * n_valid;
        __syncthreads();
    }
    if (tid == 0 && steps_exec) atomicAdd(&Q.ctr->steps_exec, steps_exec);
    if (limit_hits) atomicAdd(&Q.ctr->step_limit_hits, limit_hits);
}

// One thread per row, behind the rows' walks: a row that is not closed (or not a whole number of its periods) is an
// open row; a length that is a proper multiple of the period repeats its own states; every other row claims a slot of
// the row-key table for its canonical key.  On an occupied slot the two keys are compared in row_keys, which the launch
// before this one wrote: nothing is half-visible, nothing spins.  Equal keys are two rows on one cycle: the later one
// is named.
__global__ __launch_bounds__(256) void k_wide_trans_build(const WideTransParams Q) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q.n_rows) return;
    const uint32_t w64 = Q.net.w64;
    if (!Q.closed[q]) { atomicMin(&Q.ctr->open_row, (unsigned int)q); return; }
    const uint32_t period = Q.row_info[2 * q], mu = Q.row_info[2 * q + 1];
    if (period == 0) { atomicAdd(&Q.ctr->rows_undecided, 1u); return; }        // (its walk ran into the step limit)
    const uint64_t length = Q.lengths[q];
    if (mu != 0 || length % period != 0) { atomicMin(&Q.ctr->open_row, (unsigned int)q); return; }
    if (length != period) { atomicMin(&Q.ctr->dup_row, (unsigned int)q); return; }
    const uint64_t* mine = Q.row_keys + q * w64;
    uint64_t at = wtrans_hash(mine, w64) & Q.slot_mask;
    for (uint64_t probe = 0; probe <= Q.slot_mask; ++probe, at = (at + 1) & Q.slot_mask) {
        const uint32_t owner = atomicCAS(&Q.owners[at], 0u, (uint32_t)q + 1u);
        if (owner == 0) return;
        if (wtrans_key_equal(mine, Q.row_keys + (uint64_t)(owner - 1) * w64, w64)) {
            const uint32_t other = owner - 1;
            atomicMin(&Q.ctr->dup_row, (uint32_t)q > other ? (uint32_t)q : other);
            return;
        }
    }
    atomicAdd(&Q.ctr->probe_full, 1u);
}

template <int K>
static hipError_t launch_wide_trans_k(dim3 grid, size_t shmem, hipStream_t st, const WideTransParams& Q) {
    const void* fn = Q.net.wdesc ? (const void*)k_wide_trans<K, true> : (const void*)k_wide_trans<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideTransParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_trans(int k, dim3 grid, size_t shmem, hipStream_t st, const WideTransParams& Q) {
    switch (k) {
        case 1: return launch_wide_trans_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_trans_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_trans_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_trans_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_trans_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_trans_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_wide_trans_build(const WideTransParams& Q, hipStream_t st) {
    const uint64_t blocks = (Q.n_rows + 255) / 256;
    hipLaunchKernelGGL(k_wide_trans_build, dim3((uint32_t)blocks), dim3(256), 0, st, Q);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Mutant screens over samples (bsx_run_screen_sampled; include/bsx.h has the definition, bsx_wide.h / bsx_screen.h the
// layout).  A workgroup's work items are (mutant, group) pairs: the sampled source's set-up, then k_wide's attract phases
// with T_p = 0 (the body of k_wide_trans's row stage, copied: a shared body changed the figures of the older kernels), and
// behind every wide_step the override of the mutant's rows.
namespace {

// The mutant of a workgroup's pair: up to BSX_SCREEN_MAX_NODES (row, word) pairs, uniform over the workgroup; an unused
// entry has row kWideNone, which no thread owns.
struct WideMutant {
    uint32_t row[BSX_SCREEN_MAX_NODES];
    uint32_t word[BSX_SCREEN_MAX_NODES];        // all ones for value 1, 0 for value 0
};

// Behind wide_step(cur -> nxt, act): the thread that owns row v of its column rewrites the word it has just written
// itself (no barrier), under the same freeze mask: a frozen bit keeps its value, a live one has the mutant's.
__device__ __forceinline__ void wide_screen_override(const WideMutant& M, const WideCtx& X, const uint32_t* cur, uint32_t* nxt, uint32_t act) {
#pragma unroll
    for (int i = 0; i < BSX_SCREEN_MAX_NODES; ++i) {
        const uint32_t v = M.row[i];
        if (v >= X.r0 && v < X.r1) nxt[v * X.L + X.c] = wbfi(act, M.word[i], cur[v * X.L + X.c]);
    }
}

}  // namespace

template <int K, bool KW>
__global__ __launch_bounds__(kWideThreads) void k_wide_screen(const WideScreenParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const WideParams& P = Q.net;
    WideCtx X;
    X.L = P.L;
    X.tid = threadIdx.x;
    X.c = X.tid & (P.L - 1);
    X.slice = X.tid >> P.lshift;
    X.r0 = X.slice * P.rows_ps;
    X.r1 = X.r0 + P.rows_ps;
    X.RL = P.rows * P.L;
    const uint32_t L = P.L, c = X.c, RL = X.RL, G = 32 * L, tid = X.tid;
    const uint32_t nslices = kWideThreads / L;
    uint32_t* B[4] = {sm, sm + RL, sm + 2 * RL, sm + 3 * RL};
    uint32_t* fmv = sm + 4 * RL;                    // [n_fslots][2][L]  all zero: no variations here
    uint32_t* red = fmv + 2 * P.n_fslots * L;       // [2][256]          per-thread partials
    uint32_t* col = red + 2 * kWideThreads;         // [8][L]            per-column masks (set-up: the columns' block keys)
    uint32_t* lam = col + 8 * L;                    // [G] lambda
    uint32_t* mua = lam + G;                        // [G] mu
    uint32_t* sta = mua + G;                        // [G] state of the trajectory's search
    uint32_t* misc = sta + G;                       // [8]
    enum : uint32_t { ST_ACTIVE = 0, ST_CAND = 1, ST_FOUND = 2, ST_NONE = 3, ST_INVALID = 4 };
    unsigned long long steps_ref = 0, steps_exec = 0, limit_hits = 0;
    for (uint32_t i = tid; i < 2 * P.n_fslots * L; i += kWideThreads) fmv[i] = 0;
    // found iff mu + lambda <= max_t (T_p = 0); a max_t at or beyond a quarter of the step limit counts as unbounded (k_wide)
    const uint64_t cap = (P.cap_inf || P.max_t >= P.step_limit / 4) ? ~0ull : P.max_t;

    for (uint64_t pi = blockIdx.x; pi < Q.n_pairs; pi += gridDim.x) {
        const ScreenPair pair = screen_pair_of(Q.p0 + pi, Q.g_per, Q.n_samples, G);
        const uint32_t n_valid = pair.n_valid;
        const uint64_t j_first = Q.first_sample + pair.group * G;           // the group's first sample
        const uint64_t rec0 = pi * G;                                       // its first record of this launch
        // ---- the pair's mutant (uniform: scalar loads)
        WideMutant M;
        {
            const uint32_t m0 = Q.mut_offsets[pair.mutant], m1 = Q.mut_offsets[pair.mutant + 1];
#pragma unroll
            for (int i = 0; i < BSX_SCREEN_MAX_NODES; ++i) {
                const bool have = m0 + (uint32_t)i < m1;
                M.row[i] = have ? Q.mut_nodes[2 * (m0 + i)] : kWideNone;
                M.word[i] = have && Q.mut_nodes[2 * (m0 + i) + 1] ? 0xFFFFFFFFu : 0u;
            }
        }
        // ---- s(0) = origin | 'any' words of the sampled source, whatever the mutant is
        for (uint32_t i = tid; i < RL; i += kWideThreads) {
            const uint32_t r = i >> P.lshift;
            B[0][i] = (r < P.n_nodes && ((P.origin[r >> 5] >> (r & 31u)) & 1u)) ? 0xFFFFFFFFu : 0u;
        }
        if (tid < 8) misc[tid] = 0;
        if (tid < L) {
            const SampleColumn sc = sample_column(P.sample_k0, j_first + 32ull * tid);
            col[4 * tid + 0] = (uint32_t)sc.kb0; col[4 * tid + 1] = (uint32_t)(sc.kb0 >> 32);
            col[4 * tid + 2] = (uint32_t)sc.kb1; col[4 * tid + 3] = (uint32_t)(sc.kb1 >> 32);
        }
        __syncthreads();
        for (uint32_t i = tid; i < P.n_any * L; i += kWideThreads) {
            const uint32_t a = i >> P.lshift, cw = i & (L - 1);
            const SampleColumn sc = wide_sample_column(col, cw, j_first + 32ull * cw);
            const uint32_t n_bits = n_valid > 32 * cw ? (n_valid - 32 * cw < 32u ? n_valid - 32 * cw : 32u) : 0u;
            B[0][P.any_nodes[a] * L + cw] = sample_column_word(sc, a, n_bits);
        }
        for (uint32_t k = tid; k < G; k += kWideThreads) {
            sta[k] = k < n_valid ? ST_ACTIVE : ST_INVALID;
            lam[k] = 0; mua[k] = 0;
        }
        __syncthreads();
        uint32_t* cur = B[0];
        uint32_t* nxt = B[1];
        uint64_t group_steps = 0;
        uint32_t* x0 = P.x0 + (size_t)blockIdx.x * RL;
        for (uint32_t r = X.r0; r < X.r1; ++r) x0[r * L + c] = cur[r * L + c];
        // ---- Brent's detector in lock step; the tortoise lives in B[2]
        {
            uint32_t* T = B[2];
            for (uint32_t r = X.r0; r < X.r1; ++r) T[r * L + c] = cur[r * L + c];
            uint64_t tau = 0, power = 1, lamc = 0;
            for (;;) {
                bool left = false;
                if (tid < L)
                    for (uint32_t b = 0; b < 32; ++b) left = left || sta[32 * tid + b] == ST_ACTIVE;
                if (!__syncthreads_or(left)) break;
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                wide_screen_override(M, X, cur, nxt, 0xFFFFFFFFu);
                ++tau; ++lamc; ++group_steps;
                const bool tele = lamc == power;
                uint32_t diff = 0;
                for (uint32_t r = X.r0; r < X.r1; ++r) {          // (own rows only: no barrier between write and read)
                    const uint32_t v = nxt[r * L + c];
                    diff |= v ^ T[r * L + c];
                    if (tele) T[r * L + c] = v;
                }
                red[tid] = diff;
                __syncthreads();
                if (tid < L) {
                    uint32_t df = 0;
                    for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32 * tid + b;
                        if (sta[k] != ST_ACTIVE) continue;
                        if (!((df >> b) & 1u)) {
                            lam[k] = (uint32_t)lamc;
                            sta[k] = (uint64_t)lamc > cap ? ST_NONE : ST_CAND;
                            if (sta[k] == ST_NONE) steps_ref += P.max_t;
                        } else if (cap == ~0ull ? tau >= P.step_limit : tau >= 3 * cap + 2) {
                            sta[k] = ST_NONE;
                            if (cap == ~0ull) ++limit_hits;
                            else steps_ref += P.max_t;
                        }
                    }
                }
                if (tele) { power <<= 1; lamc = 0; }
                uint32_t* s = cur; cur = nxt; nxt = s;
            }
        }
        // ---- mu: y = s(lambda) (bit b frozen after lambda_b steps) in B[0] / B[1], x = s(0) in B[2] / B[3]
        if (tid == 0) misc[2] = 0;
        __syncthreads();
        if (tid < L)
            for (uint32_t b = 0; b < 32; ++b)
                if (sta[32 * tid + b] == ST_CAND) atomicMax(&misc[2], lam[32 * tid + b]);
        __syncthreads();
        const uint32_t lam_max = misc[2];
        uint32_t* mn = B[2];
        if (lam_max) {
            uint32_t* ya = B[0]; uint32_t* yb = B[1];
            uint32_t* xa = B[2]; uint32_t* xb = B[3];
            for (uint32_t r = X.r0; r < X.r1; ++r) { ya[r * L + c] = x0[r * L + c]; xa[r * L + c] = x0[r * L + c]; }
            for (uint32_t m = 0; m < lam_max; ++m) {
                if (tid < L) {
                    uint32_t act = 0;
                    for (uint32_t b = 0; b < 32; ++b) act |= (m < lam[32 * tid + b] ? 1u : 0u) << b;
                    col[tid] = act;
                }
                __syncthreads();
                wide_step<K, KW>(P, X, ya, yb, fmv, col[c]);
                wide_screen_override(M, X, ya, yb, col[c]);
                __syncthreads();
                uint32_t* s = ya; ya = yb; yb = s;
                ++group_steps;
            }
            for (uint64_t m = 0;; ++m) {
                uint32_t diff = 0;
                for (uint32_t r = X.r0; r < X.r1; ++r) diff |= ya[r * L + c] ^ xa[r * L + c];
                red[tid] = diff;
                __syncthreads();
                bool left = false;
                if (tid < L) {
                    uint32_t df = 0;
                    for (uint32_t s = 0; s < nslices; ++s) df |= red[s * L + tid];
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t k = 32 * tid + b;
                        if (sta[k] != ST_CAND) continue;
                        if (!((df >> b) & 1u)) {
                            mua[k] = (uint32_t)m;
                            sta[k] = ST_FOUND;
                            steps_ref += m + lam[k];
                        } else if (m + 1 + lam[k] > cap) {
                            sta[k] = ST_NONE;
                            steps_ref += P.max_t;
                        } else {
                            left = true;
                        }
                    }
                }
                if (!__syncthreads_or(left)) break;
                wide_step<K, KW>(P, X, ya, yb, fmv, 0xFFFFFFFFu);
                wide_screen_override(M, X, ya, yb, 0xFFFFFFFFu);
                wide_step<K, KW>(P, X, xa, xb, fmv, 0xFFFFFFFFu);
                wide_screen_override(M, X, xa, xb, 0xFFFFFFFFu);
                __syncthreads();
                uint32_t* s = ya; ya = yb; yb = s;
                s = xa; xa = xb; xb = s;
                group_steps += 2;
            }
            // ---- key: minimum over a lap of lam_max steps from y (on the cycle of every found bit), min in xa
            cur = ya; nxt = yb;
            mn = xa;
            for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = cur[r * L + c];
            for (uint32_t m = 1; m < lam_max; ++m) {
                wide_step<K, KW>(P, X, cur, nxt, fmv, 0xFFFFFFFFu);
                wide_screen_override(M, X, cur, nxt, 0xFFFFFFFFu);
                __syncthreads();
                uint32_t* s = cur; cur = nxt; nxt = s;
                ++group_steps;
                uint32_t lt = 0, eq = 0xFFFFFFFFu;
                for (uint32_t r = X.r1; r-- > X.r0;) {
                    const uint32_t v = cur[r * L + c], w = mn[r * L + c];
                    lt |= eq & ~v & w;
                    eq &= ~(v ^ w);
                }
                red[tid] = lt;
                red[kWideThreads + tid] = eq;
                __syncthreads();
                if (tid < L) {
                    uint32_t LT = 0, EQ = 0xFFFFFFFFu;
                    for (uint32_t s2 = nslices; s2-- > 0;) {
                        LT |= EQ & red[s2 * L + tid];
                        EQ &= red[kWideThreads + s2 * L + tid];
                    }
                    col[L + tid] = LT;
                }
                __syncthreads();
                const uint32_t sel = col[L + c];
                for (uint32_t r = X.r0; r < X.r1; ++r) mn[r * L + c] = wbfi(sel, cur[r * L + c], mn[r * L + c]);
            }
        }
        __syncthreads();
        // ---- per-trajectory records of the pair (k < n_valid: bits of a ragged last column stay ST_INVALID, unwritten)
        for (uint32_t k = tid; k < n_valid; k += kWideThreads) {
            const uint64_t q = rec0 + k;
            const bool keep = sta[k] == ST_FOUND && (uint64_t)lam[k] <= P.max_len;
            P.info[4 * q + 0] = keep ? 1u : 0u;
            P.info[4 * q + 1] = keep ? lam[k] : 0u;
            P.info[4 * q + 2] = keep ? mua[k] : 0u;
            P.info[4 * q + 3] = 0u;
            for (uint32_t w = 0; w < P.w64; ++w) P.keys[q * P.w64 + w] = keep ? wide_gather64(P, mn, L, k, w) : 0ull;
        }
        steps_exec += group_steps * n_valid;
        __syncthreads();
    }
    if (steps_ref) atomicAdd(&P.ctr[0], steps_ref);
    if (tid == 0 && steps_exec) atomicAdd(&P.ctr[1], steps_exec);
    if (limit_hits) atomicAdd(&P.ctr[2], limit_hits);
}

template <int K>
static hipError_t launch_wide_screen_k(dim3 grid, size_t shmem, hipStream_t st, const WideScreenParams& Q) {
    const void* fn = Q.net.wdesc ? (const void*)k_wide_screen<K, true> : (const void*)k_wide_screen<K, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<WideScreenParams*>(&Q)};
    return hipLaunchKernel(fn, grid, dim3(kWideThreads), args, shmem, st);
}

hipError_t launch_wide_screen(int k, dim3 grid, size_t shmem, hipStream_t st, const WideScreenParams& Q) {
    switch (k) {
        case 1: return launch_wide_screen_k<1>(grid, shmem, st, Q);
        case 2: return launch_wide_screen_k<2>(grid, shmem, st, Q);
        case 3: return launch_wide_screen_k<3>(grid, shmem, st, Q);
        case 4: return launch_wide_screen_k<4>(grid, shmem, st, Q);
        case 5: return launch_wide_screen_k<5>(grid, shmem, st, Q);
        case 6: return launch_wide_screen_k<6>(grid, shmem, st, Q);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace bsx
