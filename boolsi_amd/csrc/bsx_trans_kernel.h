// k_trans_walk: one lane = one single-node flip of one cycle state of a listed attractor (bsx_run_attractor_transitions).
// Included by bsx_trans_nw*.hip, which instantiate it per state width; table probe and edge inserts are shared with
// bsx_trans.hip.
#pragma once
#include "bsx_kernels_common.h"
#include "bsx_trans.h"
#include "bsx_walk.h"

namespace bsx {

template <int NW>
struct TransState { uint32_t w[NW]; };

__device__ __forceinline__ uint32_t trans_slot_of(uint32_t hash, uint32_t slot_shift) { return (hash * 0x9E3779B1u) >> slot_shift; }

template <int NW>
__device__ __forceinline__ bool trans_state_equals(const TransTable& T, uint64_t g, const uint32_t (&s)[NW]) {
    const uint64_t* p = T.states + g * T.w64;
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < (NW + 1) / 2; ++w) {
        if ((uint32_t)w < T.w64) {
            const uint64_t word = p[w];
            d |= (uint32_t)word ^ s[2 * w];
            if (2 * w + 1 < NW) d |= (uint32_t)(word >> 32) ^ s[2 * w + 1];
            else d |= (uint32_t)(word >> 32);
        } else {
            d |= s[2 * w];
            if (2 * w + 1 < NW) d |= s[2 * w + 1];
        }
    }
    return d == 0;
}

// -> index of the listed state equal to s, or ~0.  At most one round of the table.
template <int NW>
__device__ __forceinline__ uint64_t trans_find(const TransTable& T, const uint32_t (&s)[NW]) {
    const uint32_t mask = 0xFFFFFFFFu >> T.slot_shift;
    uint32_t at = trans_slot_of(hash_state<NW>(s), T.slot_shift);
    for (uint32_t probe = 0; probe <= mask; ++probe, at = (at + 1) & mask) {
        const uint32_t owner = T.slots[at];
        if (owner == 0) return ~0ull;
        if (trans_state_equals<NW>(T, owner - 1, s)) return owner - 1;
    }
    return ~0ull;
}

__device__ __forceinline__ uint32_t trans_edge_hash(unsigned long long key) {
    const unsigned long long m = key * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(m >> 32);
}

// Insert-or-add into the HBM edge table: the key word is claimed by one 64-bit CAS; count and sum take atomic adds.
__device__ __forceinline__ void trans_edge_global(const TransParams& P, unsigned long long key, unsigned long long count,
                                                  unsigned long long sum_mu) {
    uint64_t at = trans_edge_hash(key) & P.edge_mask;
    for (uint64_t probe = 0; probe <= P.edge_mask; ++probe, at = (at + 1) & P.edge_mask) {
        TransEdgeSlot* slot = P.edges + at;
        unsigned long long seen = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0) seen = atomicCAS(&slot->key, 0ull, key);
        if (seen == 0 || seen == key) {
            atomicAdd(&slot->count, count);
            if (sum_mu) atomicAdd(&slot->sum_mu, sum_mu);
            return;
        }
    }
    atomicAdd(&P.ctr->edge_overflow, 1u);
}

template <int NW, int K, int LM>
__global__ __launch_bounds__(profile_block(NW)) void k_trans_walk(const TransParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // refused tables (a row that is not closed, two rows that share a state) are known on the device only: nothing is walked
    if (P.ctr->open_row != kTransNoRow || P.ctr->dup_row != kTransNoRow || P.ctr->probe_full) return;
    uint32_t* smem_free;
    const NetView<NW, K, LM> nv = stage_network<NW, K, LM>(P.net, smem, smem_free);
    TransEdgeSlot* lds_edges = reinterpret_cast<TransEdgeSlot*>(smem_free);         // (16-byte aligned: stage_network)
    for (uint32_t e = threadIdx.x; e < kTransLdsEdges; e += blockDim.x) lds_edges[e] = TransEdgeSlot{0ull, 0ull, 0ull};
    __syncthreads();
    uint32_t fm[NW], fv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { fm[w] = P.fixmask[w]; fv[w] = P.fixval[w]; }
    typedef TransState<NW> S;
    auto step = [&](const S& x) {
        S y;
        net_step<NW, K>(nv, x.w, fm, fv, y.w);
        return y;
    };
    auto lookup = [&](const S& x, uint32_t& d, uint32_t& len) {
        const uint64_t g = trans_find<NW>(P.tab, x.w);
        if (g == ~0ull) return false;
        d = P.tab.state_row[g];
        len = (uint32_t)P.lengths[d];
        return true;
    };
    auto eq = [](const S& a, const S& b) { return eq_words<NW>(a.w, b.w); };

    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t end = P.flip0 + P.flip_count;
    uint64_t steps = 0;
    for (uint64_t f = P.flip0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += stride) {
        const uint64_t g = f / P.n_free;
        const uint32_t node = P.free_nodes[(uint32_t)(f - g * P.n_free)];
        const uint32_t q = P.tab.state_row[g];
        S x0;
        const uint64_t* src = P.tab.states + g * P.tab.w64;
#pragma unroll
        for (int w = 0; w < (NW + 1) / 2; ++w) {
            const uint64_t word = (uint32_t)w < P.tab.w64 ? src[w] : 0ull;
            x0.w[2 * w] = (uint32_t)word;
            if (2 * w + 1 < NW) x0.w[2 * w + 1] = (uint32_t)(word >> 32);
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) x0.w[w] ^= ((node >> 5) == (uint32_t)w) ? 1u << (node & 31) : 0u;
        const WalkResult r = walk_flip<S>(x0, P.max_t, P.step_limit, step, lookup, eq);
        steps += r.steps;
        if (r.outcome == kWalkStepLimit) { atomicAdd(&P.ctr->step_limit_hits, 1u); continue; }
        const uint32_t dst = r.outcome == kWalkHit ? r.dst : r.outcome == kWalkOutside ? kTransOutside : kTransUnresolved;
        const unsigned long long mu = r.outcome == kWalkHit ? r.mu : 0u;
        if (P.node_exits && dst != q) atomicAdd(&P.node_exits[(uint64_t)q * P.net.n_nodes + node], 1u);
        const unsigned long long key = (((unsigned long long)q << 32) | dst) + 1ull;
        // the workgroup's LDS table first: the tag by one CAS, count and sum by LDS atomics
        uint32_t at = trans_edge_hash(key) & (kTransLdsEdges - 1);
        bool placed = false;
        for (uint32_t probe = 0; probe < kTransLdsProbes && !placed; ++probe, at = (at + 1) & (kTransLdsEdges - 1)) {
            unsigned long long seen = lds_edges[at].key;
            if (seen == 0) seen = atomicCAS(&lds_edges[at].key, 0ull, key);
            if (seen == 0 || seen == key) {
                atomicAdd(&lds_edges[at].count, 1ull);
                if (mu) atomicAdd(&lds_edges[at].sum_mu, mu);
                placed = true;
            }
        }
        if (!placed) trans_edge_global(P, key, 1ull, mu);
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kTransLdsEdges; e += blockDim.x)
        if (lds_edges[e].key) trans_edge_global(P, lds_edges[e].key, lds_edges[e].count, lds_edges[e].sum_mu);
    wave_atomic_add(&P.ctr->steps_exec, (unsigned long long)steps, (int)(threadIdx.x & 63));
}

template <int NW, int K>
static hipError_t launch_trans_nk(int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P) {
    const void* fn;
    BSX_KERNEL_FOR_MODE(k_trans_walk, NW, K, lut_mode, fn);
    if (!fn) return hipErrorInvalidValue;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<TransParams*>(&P)};
    return hipLaunchKernel(fn, grid, dim3(profile_block(NW)), args, shmem, st);
}

// one definition per state width, each in its own translation unit (bsx_trans_nw*.hip)
#define BSX_TRANS_WALK_UNIT(NWV)                                                                                                  \
    hipError_t launch_trans_walk_nw##NWV(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P) {    \
        BSX_DISPATCH_K(launch_trans_nk, NWV)                                                                                      \
    }

}  // namespace bsx
