// per-lane attractor profile kernel: states, per-node on-counts and closure of listed attractors (bsx_run_attractor_profile)
#include "bsx_kernels_common.h"
#include "bsx_planes.h"

namespace bsx {

// ------------------------------------------------------------------------------------------------
// One lane = one attractor: s(0) = its key state, s(t + 1) = f(s(t)) under the origin's fixed nodes, t < length
// (attract.py:22-25: the listed states of an attractor start at its key state).  Lanes of a wave run their own
// lengths; nothing waits on another lane or workgroup.
//   on-counts: vertical counters in registers (bsx_planes.h), flushed into the lane's own row every 2^P - 1 states;
//   states:    the packed words of every state, as k_simulate stores a trajectory;
//   closed:    f^length(key) == key -- the state the loop ends on.
// Workgroup size: profile_block(NW), bsx_device.h.
template <int NW, int K, int LM>
__global__ __launch_bounds__(profile_block(NW)) void k_attractor_profile(const ProfileParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* smem_free;
    const NetView<NW, K, LM> nv = stage_network<NW, K, LM>(P.net, smem, smem_free);
    typedef Planes<NW, kProfilePlanes> Pl;
    uint32_t fm[NW], fv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { fm[w] = P.fixmask[w]; fv[w] = P.fixval[w]; }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t steps = 0;
    for (uint64_t qi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; qi < P.count; qi += stride) {
        const uint32_t len = (uint32_t)P.lengths[qi];
        uint32_t key[NW], s[NW];
#pragma unroll
        for (int w = 0; w < (NW + 1) / 2; ++w) {
            const uint64_t word = (uint32_t)w < P.w64 ? P.keys[qi * P.key_stride + w] : 0ull;
            key[2 * w] = (uint32_t)word;
            if (2 * w + 1 < NW) key[2 * w + 1] = (uint32_t)(word >> 32);
        }
        copy_words<NW>(s, key);
        uint32_t* row = P.on_counts ? P.on_counts + qi * P.net.n_nodes : nullptr;
        uint64_t* out = P.states ? P.states + P.state_offsets[qi] : nullptr;
        Pl pl;
        planes_clear(pl);
        uint32_t pending = 0;
        for (uint32_t t = 0; t < len; ++t) {
            if (row) {
                planes_add(pl, s);
                if (++pending == Pl::kFlushEvery) { planes_flush(pl, row, P.net.n_nodes); pending = 0; }
            }
            if (out) {
#pragma unroll
                for (int w = 0; w < (NW + 1) / 2; ++w) {
                    uint64_t word = s[2 * w];
                    if (2 * w + 1 < NW) word |= (uint64_t)s[2 * w + 1] << 32;
                    if ((uint32_t)w < P.w64) out[(uint64_t)t * P.w64 + w] = word;
                }
            }
            uint32_t nxt[NW];
            net_step<NW, K>(nv, s, fm, fv, nxt);
            copy_words<NW>(s, nxt);
        }
        steps += len;
        if (row && pending) planes_flush(pl, row, P.net.n_nodes);
        if (P.closed) P.closed[qi] = eq_words<NW>(s, key) ? 1 : 0;
    }
    wave_atomic_add(&P.ctr->steps_ref, (unsigned long long)steps, (int)(threadIdx.x & 63));
    wave_atomic_add(&P.ctr->steps_exec, (unsigned long long)steps, (int)(threadIdx.x & 63));
}


template <int NW, int K>
static hipError_t launch_profile_nk(int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const ProfileParams& P) {
    const void* fn;
    BSX_KERNEL_FOR_MODE(k_attractor_profile, NW, K, lut_mode, fn);
    if (!fn) return hipErrorInvalidValue;
    void* args[] = {const_cast<ProfileParams*>(&P)};
    return hipLaunchKernel(fn, grid, dim3(profile_block(NW)), args, shmem, st);
}
template <int NW, int K>
static hipError_t configure_profile_nk(int lut_mode, dim3, size_t shmem, hipStream_t, const int&) {
    const void* fn;
    BSX_KERNEL_FOR_MODE(k_attractor_profile, NW, K, lut_mode, fn);
    if (!fn) return hipErrorInvalidValue;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
}

hipError_t launch_profile(int nw, int k, int lut_mode, dim3 grid, size_t shmem, hipStream_t st, const ProfileParams& P) {
    BSX_DISPATCH(launch_profile_nk)
}
// Allow the instantiation used by a network to take `shmem` bytes of dynamic LDS (as configure_simulate).
hipError_t configure_profile(int nw, int k, int lut_mode, size_t shmem) {
    const dim3 grid(1);
    const hipStream_t st = nullptr;
    const int P = 0;
    BSX_DISPATCH(configure_profile_nk)
}

}  // namespace bsx
