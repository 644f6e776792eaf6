// Attractor transitions (bsx_run_attractor_transitions): the cycle-state table in HBM (k_trans_build), the drain of
// the edge table (k_trans_drain) and the dispatch of k_trans_walk over the state width (bsx_trans_nw*.hip).
#include "bsx_kernels_common.h"
#include "bsx_trans.h"

namespace bsx {

// Build and walk must agree on a state's hash, and the walk hashes registers with hash_state<NW>.  So the build does
// what hash_state<NW> does, for a width known at run time: the 32-bit words beyond the state are zero, and a zero word
// leaves hash_state's xor-rotate sum unchanged.
__device__ __forceinline__ uint32_t trans_hash_words(const uint64_t* p, uint32_t w64) {
    constexpr int kRot[8] = {0, 5, 10, 15, 20, 25, 3, 8};       // hash_state's rotations
    uint32_t h = 0;
    for (uint32_t w = 0; w < 2 * w64 && w < 8; ++w) {
        const uint32_t v = (uint32_t)(p[w >> 1] >> (32 * (w & 1)));
        h ^= w == 0 ? v : (v << kRot[w]) | (v >> (32 - kRot[w]));
    }
    h ^= h >> 16;
    h ^= h >> 8;
    return h;
}

// largest q with row_first[q] <= g  (row_first ascending, row_first[0] == 0, g < n_states)
__device__ __forceinline__ uint32_t trans_row_of(const uint64_t* row_first, uint64_t n_rows, uint64_t g) {
    uint64_t lo = 0, hi = n_rows;                   // row_first[lo] <= g < row_first[hi] (hi == n_rows: the end)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (row_first[mid] <= g) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}

// One thread per listed state g: its row into state_row, its index + 1 into the first free slot of its probe
// sequence.  On an occupied slot the two states are compared in `states`, which the profile launch before this one
// wrote: nothing is half-visible, nothing spins.  Equal states are a refusal (a duplicate row, or a length that is a
// multiple of the period): the later of the two rows is named.  Threads q < n_rows also report rows that did not close.
__global__ __launch_bounds__(256) void k_trans_build(const TransTable T, const uint8_t* closed, uint64_t n_rows, const uint64_t* row_first,
                                                      TransCtr* ctr) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T.n_states) return;
    if (g < n_rows && !closed[g]) atomicMin(&ctr->open_row, (unsigned int)g);
    const uint32_t row = trans_row_of(row_first, n_rows, g);
    T.state_row[g] = row;
    const uint64_t* mine = T.states + g * T.w64;
    const uint32_t mask = 0xFFFFFFFFu >> T.slot_shift;
    uint32_t at = (trans_hash_words(mine, T.w64) * 0x9E3779B1u) >> T.slot_shift;
    for (uint32_t probe = 0; probe <= mask; ++probe, at = (at + 1) & mask) {
        uint32_t owner = atomicCAS(&T.slots[at], 0u, (uint32_t)g + 1u);
        if (owner == 0) return;
        const uint64_t* theirs = T.states + (uint64_t)(owner - 1) * T.w64;
        uint64_t diff = 0;
        for (uint32_t w = 0; w < T.w64; ++w) diff |= mine[w] ^ theirs[w];
        if (diff == 0) {
            const uint32_t other = trans_row_of(row_first, n_rows, owner - 1);
            atomicMin(&ctr->dup_row, row > other ? row : other);
            return;
        }
    }
    atomicAdd(&ctr->probe_full, 1u);
}

// packs the occupied slots of the edge table behind one cursor; the host sorts
__global__ __launch_bounds__(256) void k_trans_drain(const TransEdgeSlot* edges, uint64_t slots, TransEdge* out, uint64_t cap, TransCtr* ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= slots || edges[i].key == 0) return;
    const unsigned long long at = atomicAdd(&ctr->n_edges, 1ull);
    if (at >= cap) return;
    const unsigned long long key = edges[i].key - 1ull;
    out[at] = TransEdge{(uint32_t)(key >> 32), (uint32_t)key, edges[i].count, edges[i].sum_mu};
}

hipError_t launch_trans_build(const TransTable& tab, const uint8_t* closed, uint64_t n_rows, const uint64_t* row_first, TransCtr* ctr,
                              hipStream_t st) {
    const uint64_t blocks = (tab.n_states + 255) / 256;
    hipLaunchKernelGGL(k_trans_build, dim3((uint32_t)blocks), dim3(256), 0, st, tab, closed, n_rows, row_first, ctr);
    return hipGetLastError();
}

hipError_t launch_trans_drain(const TransEdgeSlot* edges, uint64_t slots, TransEdge* out, uint64_t cap, TransCtr* ctr, hipStream_t st) {
    const uint64_t blocks = (slots + 255) / 256;
    hipLaunchKernelGGL(k_trans_drain, dim3((uint32_t)blocks), dim3(256), 0, st, edges, slots, out, cap, ctr);
    return hipGetLastError();
}

size_t trans_lds_bytes() { return (size_t)kTransLdsEdges * sizeof(TransEdgeSlot); }

hipError_t launch_trans_walk_nw1(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P);
hipError_t launch_trans_walk_nw2(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P);
hipError_t launch_trans_walk_nw4(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P);
hipError_t launch_trans_walk_nw8(int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P);

hipError_t launch_trans_walk(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const TransParams& P) {
    switch (nw) {
        case 1: return launch_trans_walk_nw1(k, lut_mode, grid, shmem, st, P);
        case 2: return launch_trans_walk_nw2(k, lut_mode, grid, shmem, st, P);
        case 4: return launch_trans_walk_nw4(k, lut_mode, grid, shmem, st, P);
        case 8: return launch_trans_walk_nw8(k, lut_mode, grid, shmem, st, P);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace bsx
