// Device-side reduction of what k_wide_screen leaves per trajectory (bsx_wide.h / bsx_screen.h have the layouts):
//   k_screen_reduce  folds a launch's (info, keys) records into an HBM table keyed by (mutant, whole key);
//   k_screen_drain   packs the table's ready slots into bsx_screen_rec-shaped records behind one cursor.
// The kernels of bsx_wide_reduce.hip with the mutant in the key: a record's mutant follows from its position in the
// launch (screen_pair_of), and so does whether the record exists at all (a ragged group's tail is never read).  They run
// on the engine's stream right behind the k_wide_screen launch whose records they read, so the host waits once per call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bsx_device.h"
#include "bsx_sample.h"
#include "bsx_screen.h"
#include "bsx_wide.h"

namespace bsx {

namespace {

constexpr uint32_t kReduceThreads = 256;
constexpr uint32_t kLdsProbes = 8;
static_assert(kWideReduceTile <= 1024 && (kWideReduceTile & (kWideReduceTile - 1)) == 0, "the LDS tag holds a 10-bit record index");
static_assert((kWideReduceLdsSlots & (kWideReduceLdsSlots - 1)) == 0 && kWideReduceLdsSlots <= kReduceThreads, "one flushing thread per LDS entry");

__device__ __forceinline__ uint32_t sr_hash(uint64_t mutant, const uint64_t* key, uint32_t w64) {
    uint64_t h = (0x9E3779B97F4A7C15ull ^ mutant) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
    for (uint32_t w = 0; w < w64; ++w) {
        h = (h ^ key[w]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 29;
    }
    return (uint32_t)h ^ (uint32_t)(h >> 32);
}

// Insert-or-add by (mutant, key): the slot protocol of wr_insert (bsx_wide_reduce.hip).  CAS claims the slot, mutant and
// key are stored, a release store publishes "ready"; readers load the state with acquire and compare mutant and whole key.
// One loop with every exit inside its body.  Bounded: a spin gives up after 2^20 looks, a probe sequence after one round
// of the table; both set a flag.
__device__ __forceinline__ void sr_insert(ScreenSlot* table, uint64_t mask, unsigned long long* hdr, uint64_t mutant, const uint64_t* key,
                                          uint32_t w64, uint32_t hsh, uint32_t length, unsigned long long count,
                                          unsigned long long sl, unsigned long long sl2_lo, unsigned long long sl2_hi) {
    uint64_t at = (uint64_t)(hsh ^ (hsh >> 15)) & mask;
    uint64_t probes = 0;
    uint32_t spins = 0;
    bool done = false;
    while (!done) {
        ScreenSlot* e = table + at;
        uint32_t st = __hip_atomic_load(&e->state, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        bool mine = false;
        if (st == 0u) {
            st = atomicCAS(&e->state, 0u, 1u);
            if (st == 0u) {
                __hip_atomic_store(&e->mutant, (unsigned long long)mutant, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
            unsigned long long d = __hip_atomic_load(&e->mutant, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ mutant;
            for (uint32_t w = 0; w < w64; ++w) d |= __hip_atomic_load(&e->key[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ key[w];
            same = d == 0;
        }
        if (same) {
            // multi-word adds: a word's carry out is decided by the value its own atomic returns
            atomicAdd(&e->count, count);
            const unsigned long long o1 = atomicAdd(&e->sum_l[0], sl);
            if (o1 + sl < o1) atomicAdd(&e->sum_l[1], 1ull);
            const unsigned long long o2 = atomicAdd(&e->sum_l2[0], sl2_lo);
            const unsigned long long up = sl2_hi + ((o2 + sl2_lo < o2) ? 1ull : 0ull);
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

// One workgroup per tile of kWideReduceTile records of a launch of n_pairs pairs from p0 (G records each).  As
// k_wide_reduce_attract: the tile is combined in a small LDS table first (an entry is claimed by one CAS on its tag:
// bit 31, 21 hash bits, the tile index of the record that stands for the entry) and each occupied entry leaves as one
// global insert.  A tile spans up to 1024 / G groups, so possibly several mutants: the mutant is in the hash and in the
// comparison with the representative.
__global__ __launch_bounds__(kReduceThreads) void k_screen_reduce(const uint32_t* __restrict__ info, const uint64_t* __restrict__ keys,
                                                                  uint64_t n_pairs, uint64_t p0, uint64_t g_per, uint64_t n_samples,
                                                                  uint32_t G, uint32_t w64, ScreenSlot* table, uint64_t mask,
                                                                  unsigned long long* hdr) {
    __shared__ uint32_t tag[kWideReduceLdsSlots];
    __shared__ uint32_t cnt[kWideReduceLdsSlots];
    __shared__ uint32_t s2_hi[kWideReduceLdsSlots];
    __shared__ unsigned long long s1[kWideReduceLdsSlots];
    __shared__ unsigned long long s2_lo[kWideReduceLdsSlots];
    const uint32_t tid = threadIdx.x;
    if (tid < kWideReduceLdsSlots) { tag[tid] = 0; cnt[tid] = 0; s2_hi[tid] = 0; s1[tid] = 0; s2_lo[tid] = 0; }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kWideReduceTile;
    const uint64_t m = n_pairs * G;
    for (uint32_t r = tid; r < kWideReduceTile; r += kReduceThreads) {
        const uint64_t q = base + r;
        if (q >= m) break;
        const uint64_t pi = q / G;
        const ScreenPair pair = screen_pair_of(p0 + pi, g_per, n_samples, G);
        if ((uint32_t)(q - pi * G) >= pair.n_valid) continue;          // behind the end of a ragged group: never written
        const uint4 in = reinterpret_cast<const uint4*>(info)[q];
        if (!in.x) continue;                                            // (none = n_samples - the counts, on the host)
        const uint64_t* key = keys + q * w64;
        const uint32_t hsh = sr_hash(pair.mutant, key, w64);
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
                    const uint64_t rq = base + rep;
                    const uint64_t* other = keys + rq * w64;
                    unsigned long long d = (unsigned long long)((p0 + rq / G) / g_per) ^ (unsigned long long)pair.mutant;
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
        if (!placed) sr_insert(table, mask, hdr, pair.mutant, key, w64, hsh, in.y, 1ull, l, l2_lo, l2_hi);
    }
    __syncthreads();
    if (tid < kWideReduceLdsSlots && tag[tid]) {
        const uint64_t q = base + (tag[tid] & (kWideReduceTile - 1));
        const uint64_t mutant = (p0 + q / G) / g_per;
        const uint64_t* key = keys + q * w64;
        sr_insert(table, mask, hdr, mutant, key, w64, sr_hash(mutant, key, w64), info[4 * q + 1], cnt[tid], s1[tid], s2_lo[tid], s2_hi[tid]);
    }
}

// Ready slots -> dense records out[0 .. min(cursor, cap)), in no particular order (the host sorts them).  The cursor
// counts every ready slot, so the host sees "more than cap" without the records.  Threads 0..3 of block 0 copy the
// counters that the k_wide_screen launches accumulated into the header.
__global__ __launch_bounds__(kReduceThreads) void k_screen_drain(const ScreenSlot* __restrict__ table, uint64_t slots, ScreenRec* out,
                                                                 uint64_t cap, unsigned long long* hdr,
                                                                 const unsigned long long* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kReduceThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kReduceThreads + threadIdx.x; i < slots; i += stride) {
        const ScreenSlot& e = table[i];
        if (e.state != 2u) continue;
        const unsigned long long at = atomicAdd(&hdr[kHdrCursor], 1ull);
        if (at >= cap) continue;
        ScreenRec& o = out[at];
        o.mutant = e.mutant;
        WideAttrRec& r = o.rec;
#pragma unroll
        for (uint32_t w = 0; w < kWideMaxW32 / 2; ++w) r.key[w] = e.key[w];
        r.length = e.length;
        r.count[0] = e.count; r.count[1] = 0;
        r.sum_l[0] = e.sum_l[0]; r.sum_l[1] = e.sum_l[1]; r.sum_l[2] = 0;
        r.sum_l2[0] = e.sum_l2[0]; r.sum_l2[1] = e.sum_l2[1]; r.sum_l2[2] = e.sum_l2[2]; r.sum_l2[3] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) hdr[kHdrCtr + threadIdx.x] = ctr[threadIdx.x];
}

hipError_t launch_screen_reduce(const uint32_t* info, const uint64_t* keys, uint64_t n_pairs, uint64_t p0, uint64_t g_per, uint64_t n_samples,
                                uint32_t G, uint32_t w64, ScreenSlot* table, uint64_t slots, unsigned long long* hdr, hipStream_t st) {
    const uint32_t grid = (uint32_t)((n_pairs * G + kWideReduceTile - 1) / kWideReduceTile);
    hipLaunchKernelGGL(k_screen_reduce, dim3(grid), dim3(kReduceThreads), 0, st, info, keys, n_pairs, p0, g_per, n_samples, G, w64, table,
                       slots - 1, hdr);
    return hipGetLastError();
}

hipError_t launch_screen_drain(const ScreenSlot* table, uint64_t slots, ScreenRec* out, uint64_t cap, unsigned long long* hdr,
                               const unsigned long long* ctr, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((slots + kReduceThreads - 1) / kReduceThreads, 2048);
    hipLaunchKernelGGL(k_screen_drain, dim3(grid), dim3(kReduceThreads), 0, st, table, slots, out, cap, hdr, ctr);
    return hipGetLastError();
}

}  // namespace bsx
