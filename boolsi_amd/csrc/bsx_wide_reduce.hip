// Device-side reduction of what k_wide leaves per problem (bsx_wide.h has the layouts):
//   k_wide_reduce_attract  folds a chunk's (info, keys) records into an HBM table keyed by the whole key;
//   k_wide_reduce_drain    packs the table's ready slots into bsx_attr_rec2w-shaped records behind one cursor;
//   k_wide_reduce_target   counts a chunk's hits and bins their first-hit times.
// They run on the engine's stream right behind the k_wide launch whose records they read, so the host waits once
// per call, not once per chunk.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bsx_device.h"
#include "bsx_wide.h"

namespace bsx {

namespace {

constexpr uint32_t kReduceThreads = 256;
constexpr uint32_t kLdsProbes = 8;
static_assert(kWideReduceTile <= 1024 && (kWideReduceTile & (kWideReduceTile - 1)) == 0, "the LDS tag holds a 10-bit record index");
static_assert((kWideReduceLdsSlots & (kWideReduceLdsSlots - 1)) == 0 && kWideReduceLdsSlots <= kReduceThreads, "one flushing thread per LDS entry");

__device__ __forceinline__ uint32_t wr_hash(const uint64_t* key, uint32_t w64) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint32_t w = 0; w < w64; ++w) {
        h = (h ^ key[w]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 29;
    }
    return (uint32_t)h ^ (uint32_t)(h >> 32);
}

__device__ __forceinline__ unsigned long long wr_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64);
        const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// Insert-or-add by key, the slot protocol of table_insert (bsx_kernels_common.h): CAS claims the slot, the key is
// stored, a release store publishes "ready"; readers load the state with acquire and compare the whole key.  One
// loop with every exit inside its body, so lanes that spin on a slot cannot starve the lane of their own wave that
// is writing it.  Bounded: a spin gives up after 2^20 looks, a probe sequence after one round of the table (only a
// table without a free slot ends that way, i.e. more distinct keys than slots >= 2 * cap); both set a flag.
__device__ __forceinline__ void wr_insert(WideSlot* table, uint64_t mask, unsigned long long* hdr, const uint64_t* key,
                                          uint32_t w64, uint32_t hsh, uint32_t length, unsigned long long count,
                                          unsigned long long sl, unsigned long long sl2_lo, unsigned long long sl2_hi) {
    uint64_t at = (uint64_t)(hsh ^ (hsh >> 15)) & mask;
    uint64_t probes = 0;
    uint32_t spins = 0;
    bool done = false;
    while (!done) {
        WideSlot* e = table + at;
        uint32_t st = __hip_atomic_load(&e->state, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        bool mine = false;
        if (st == 0u) {
            st = atomicCAS(&e->state, 0u, 1u);
            if (st == 0u) {
                for (uint32_t w = 0; w < w64; ++w) __hip_atomic_store(&e->key[w], key[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&e->length, length, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&e->state, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                mine = true;
            }
        }
        if (!mine && st == 1u) {                // somebody is writing the key: look again (bounded)
            if (++spins > (1u << 20)) { atomicOr(&hdr[kHdrOverflow], 2ull); done = true; }
            continue;
        }
        bool same = mine;
        if (!mine) {                            // st == 2: ready
            unsigned long long d = 0;
            for (uint32_t w = 0; w < w64; ++w) d |= __hip_atomic_load(&e->key[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ key[w];
            same = d == 0;
        }
        if (same) {
            // multi-word adds: a word's carry out is decided by the value its own atomic returns, so every carry is
            // added exactly once whatever the order of the adders
            atomicAdd(&e->count, count);
            const unsigned long long o1 = atomicAdd(&e->sum_l[0], sl);
            if (o1 + sl < o1) atomicAdd(&e->sum_l[1], 1ull);
            const unsigned long long o2 = atomicAdd(&e->sum_l2[0], sl2_lo);
            const unsigned long long up = sl2_hi + ((o2 + sl2_lo < o2) ? 1ull : 0ull);     // sl2_hi < 2^13: no wrap
            if (up) {
                const unsigned long long o3 = atomicAdd(&e->sum_l2[1], up);
                if (o3 + up < o3) atomicAdd(&e->sum_l2[2], 1ull);
            }
            done = true;
        } else {
            at = (at + 1) & mask;
            spins = 0;
            if (++probes > mask) { atomicOr(&hdr[kHdrOverflow], 1ull); done = true; }
        }
    }
}

}  // namespace

// One workgroup per tile of kWideReduceTile records.  Sweeps have few attractors and many problems, so the tile is
// combined in a small LDS table first and each occupied entry leaves as ONE global insert.  An LDS entry is claimed
// by a single CAS on its tag (bit 31 set, 21 hash bits, the tile index of the record whose key stands for the entry),
// so a tag is complete as soon as it is visible and nothing spins; the full key is compared against that
// representative's record in HBM.  A record that finds no entry within kLdsProbes goes to the HBM table directly.
__global__ __launch_bounds__(kReduceThreads) void k_wide_reduce_attract(const uint32_t* __restrict__ info,
                                                                        const uint64_t* __restrict__ keys, uint64_t m,
                                                                        uint32_t w64, WideSlot* table, uint64_t mask,
                                                                        unsigned long long* hdr) {
    __shared__ uint32_t tag[kWideReduceLdsSlots];
    __shared__ uint32_t cnt[kWideReduceLdsSlots];
    __shared__ uint32_t s2_hi[kWideReduceLdsSlots];         // < 2^2 per record (+ carries), 1024 records: fits
    __shared__ unsigned long long s1[kWideReduceLdsSlots];  // < 2^33 per record: fits
    __shared__ unsigned long long s2_lo[kWideReduceLdsSlots];
    const uint32_t tid = threadIdx.x;
    if (tid < kWideReduceLdsSlots) { tag[tid] = 0; cnt[tid] = 0; s2_hi[tid] = 0; s1[tid] = 0; s2_lo[tid] = 0; }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kWideReduceTile;
    unsigned long long none = 0;
    for (uint32_t r = tid; r < kWideReduceTile; r += kReduceThreads) {
        const uint64_t q = base + r;
        if (q >= m) break;
        const uint4 in = reinterpret_cast<const uint4*>(info)[q];
        if (!in.x) { ++none; continue; }
        const uint64_t* key = keys + q * w64;
        const uint32_t hsh = wr_hash(key, w64);
        const unsigned long long l = (unsigned long long)in.z | ((unsigned long long)in.w << 32);
        const unsigned long long l2_lo = l * l, l2_hi = __umul64hi(l, l);
        const uint32_t mytag = 0x80000000u | ((hsh >> 11) << 10) | r;
        uint32_t at = hsh & (kWideReduceLdsSlots - 1);
        bool placed = false;
        for (uint32_t p = 0; p < kLdsProbes && !placed; ++p) {
            uint32_t cur = __hip_atomic_load(&tag[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == 0u) {
                cur = atomicCAS(&tag[at], 0u, mytag);
                if (cur == 0u) cur = mytag;
            }
            if (((cur ^ mytag) & 0xFFFFFC00u) == 0u) {
                const uint32_t rep = cur & (kWideReduceTile - 1);
                bool same = rep == r;
                if (!same) {
                    const uint64_t* other = keys + (base + rep) * w64;
                    unsigned long long d = 0;
                    for (uint32_t w = 0; w < w64; ++w) d |= key[w] ^ other[w];
                    same = d == 0;
                }
                if (same) {
                    atomicAdd(&cnt[at], 1u);
                    atomicAdd(&s1[at], l);
                    const unsigned long long old = atomicAdd(&s2_lo[at], l2_lo);
                    const uint32_t up = (uint32_t)l2_hi + ((old + l2_lo < old) ? 1u : 0u);
                    if (up) atomicAdd(&s2_hi[at], up);
                    placed = true;
                }
            }
            at = (at + 1) & (kWideReduceLdsSlots - 1);
        }
        if (!placed) wr_insert(table, mask, hdr, key, w64, hsh, in.y, 1ull, l, l2_lo, l2_hi);
    }
    none = wr_wave_sum(none);                   // one atomic per wave
    if ((tid & 63u) == 0 && none) atomicAdd(&hdr[kHdrNone], none);
    __syncthreads();
    if (tid < kWideReduceLdsSlots && tag[tid]) {
        const uint64_t q = base + (tag[tid] & (kWideReduceTile - 1));
        const uint64_t* key = keys + q * w64;
        wr_insert(table, mask, hdr, key, w64, wr_hash(key, w64), info[4 * q + 1], cnt[tid], s1[tid], s2_lo[tid], s2_hi[tid]);
    }
}

// Ready slots -> dense records out[0 .. min(cursor, cap)), in no particular order (the host sorts them).  The cursor
// counts every ready slot, so the host sees "more than cap" without the records.  Threads 0..3 of block 0 copy the
// counters that the k_wide launches accumulated into the header.
__global__ __launch_bounds__(kReduceThreads) void k_wide_reduce_drain(const WideSlot* __restrict__ table, uint64_t slots,
                                                                      WideAttrRec* out, uint64_t cap, unsigned long long* hdr,
                                                                      const unsigned long long* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kReduceThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kReduceThreads + threadIdx.x; i < slots; i += stride) {
        const WideSlot& e = table[i];
        if (e.state != 2u) continue;
        const unsigned long long at = atomicAdd(&hdr[kHdrCursor], 1ull);
        if (at >= cap) continue;
        WideAttrRec& r = out[at];
#pragma unroll
        for (uint32_t w = 0; w < kWideMaxW32 / 2; ++w) r.key[w] = e.key[w];
        r.length = e.length;
        r.count[0] = e.count; r.count[1] = 0;
        r.sum_l[0] = e.sum_l[0]; r.sum_l[1] = e.sum_l[1]; r.sum_l[2] = 0;
        r.sum_l2[0] = e.sum_l2[0]; r.sum_l2[1] = e.sum_l2[1]; r.sum_l2[2] = e.sum_l2[2]; r.sum_l2[3] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) hdr[kHdrCtr + threadIdx.x] = ctr[threadIdx.x];
}

// Hits and histogram of first-hit times of a chunk (last bin = that time or later; bins == 0: count only).  The
// workgroup bins in LDS, the hit count leaves each wave as one atomic, each non-empty bin each workgroup as one.
__global__ __launch_bounds__(kReduceThreads) void k_wide_reduce_target(const uint32_t* __restrict__ t_hit, uint64_t m,
                                                                       unsigned long long* hist, uint32_t bins,
                                                                       unsigned long long* hdr) {
    __shared__ uint32_t lh[kTargetHistBins];    // a workgroup sees fewer than 2^32 problems (chunks are <= 2^24)
    const uint32_t tid = threadIdx.x;
    for (uint32_t b = tid; b < bins; b += kReduceThreads) lh[b] = 0;
    __syncthreads();
    unsigned long long hits = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kReduceThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kReduceThreads + tid; q < m; q += stride) {
        const uint32_t t = t_hit[q];
        if (t == kWideNone) continue;
        ++hits;
        if (bins) atomicAdd(&lh[t < bins - 1 ? t : bins - 1], 1u);
    }
    hits = wr_wave_sum(hits);
    if ((tid & 63u) == 0 && hits) atomicAdd(&hdr[kHdrHits], hits);
    __syncthreads();
    for (uint32_t b = tid; b < bins; b += kReduceThreads)
        if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
}

hipError_t launch_wide_reduce_attract(const uint32_t* info, const uint64_t* keys, uint64_t m, uint32_t w64, WideSlot* table,
                                      uint64_t slots, unsigned long long* hdr, hipStream_t st) {
    const uint32_t grid = (uint32_t)((m + kWideReduceTile - 1) / kWideReduceTile);
    hipLaunchKernelGGL(k_wide_reduce_attract, dim3(grid), dim3(kReduceThreads), 0, st, info, keys, m, w64, table, slots - 1, hdr);
    return hipGetLastError();
}

hipError_t launch_wide_reduce_drain(const WideSlot* table, uint64_t slots, WideAttrRec* out, uint64_t cap, unsigned long long* hdr,
                                    const unsigned long long* ctr, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((slots + kReduceThreads - 1) / kReduceThreads, 2048);
    hipLaunchKernelGGL(k_wide_reduce_drain, dim3(grid), dim3(kReduceThreads), 0, st, table, slots, out, cap, hdr, ctr);
    return hipGetLastError();
}

hipError_t launch_wide_reduce_target(const uint32_t* t_hit, uint64_t m, unsigned long long* hist, uint32_t bins,
                                     unsigned long long* hdr, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((m + 4 * kReduceThreads - 1) / (4 * kReduceThreads), 1024);
    hipLaunchKernelGGL(k_wide_reduce_target, dim3(grid), dim3(kReduceThreads), 0, st, t_hit, m, hist, bins, hdr);
    return hipGetLastError();
}

}  // namespace bsx
