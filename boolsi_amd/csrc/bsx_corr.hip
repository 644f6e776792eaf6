// Node correlations of an attractor table (bsx_run_node_correlations, bsx_corr_api.cpp): from the on-counts the profile
// kernels left in HBM to S = D^T diag(w) D, where D holds the centred frequency-weighted ranks (bsx_ranks.h).
//   k_corr_observe     on_counts[q][i] / lengths[q] -> sort keys key[i][q] (the bits of the double) and payload q
//   (rocprim)          segmented radix sort, one segment per column
//   k_corr_rank_fwd    per column: prefix sums of the gathered frequencies, P[lb] of every tie group
//   k_corr_rank_bwd    per column: P[ub] of every tie group -> rank2 -> d2, scattered to D[i][q] (and ranks[q][i])
//   k_corr_cov         upper-triangle 16 x 16 tiles of S per chunk of kCorrChunk attractors, v_mfma_f64_16x16x4_f64
//   k_corr_reduce      adds the chunk partials in chunk order, writes both triangles
// No floating-point atomics anywhere: S is the same bit for bit from run to run.
#include <hip/hip_runtime.h>

#include <cstring>      // (before rocprim: its headers use memset without including it)
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "bsx_corr.h"
#include "bsx_ranks.h"

namespace bsx {

// ------------------------------------------------------------------------------------------------
// Observe and transpose: 32 attractors x 32 columns per workgroup through LDS, so that the on-counts are read along
// the nodes and the keys written along the attractors.  An observation is on_count / length in IEEE double division;
// a non-negative double orders as its bits do as an unsigned integer.
constexpr int kObsTile = 32;

__global__ __launch_bounds__(256) void k_corr_observe(const CorrBatch B) {
    __shared__ uint64_t tile[kObsTile][kObsTile + 1];
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint64_t q0 = (uint64_t)blockIdx.x * kObsTile;
    const uint32_t c0 = blockIdx.y * kObsTile;
#pragma unroll
    for (uint32_t r = 0; r < kObsTile; r += 8) {
        const uint64_t q = q0 + ty + r;
        const uint32_t c = c0 + tx;
        uint64_t bits = 0;
        if (q < B.n && c < B.n_cols) {
            const double obs = (double)B.on_counts[q * B.n_nodes + B.col0 + c] / (double)B.lengths[q];
            bits = (uint64_t)__double_as_longlong(obs);
        }
        tile[ty + r][tx] = bits;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kObsTile; r += 8) {
        const uint32_t c = c0 + ty + r;
        const uint64_t q = q0 + tx;
        if (q < B.n && c < B.n_cols) {
            B.keys[(uint64_t)c * B.n + q] = tile[tx][ty + r];
            B.vals[(uint64_t)c * B.n + q] = (uint32_t)q;
        }
    }
}

hipError_t launch_corr_observe(const CorrBatch& B, hipStream_t st) {
    const dim3 grid((uint32_t)((B.n + kObsTile - 1) / kObsTile), (B.n_cols + kObsTile - 1) / kObsTile);
    hipLaunchKernelGGL(k_corr_observe, grid, dim3(256), 0, st, B);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Sort: column c of the batch is the segment [c n, (c + 1) n).  (At most 2^31 cells per batch: bsx_corr_api.cpp.)
struct ColumnOffset {
    uint64_t n;
    __host__ __device__ unsigned int operator()(unsigned int c) const { return (unsigned int)(c * n); }
};

hipError_t corr_sort_columns(const CorrBatch& B, void* temp, size_t* temp_bytes, hipStream_t st) {
    const auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned int>(0u), ColumnOffset{B.n});
    const auto end = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned int>(1u), ColumnOffset{B.n});
    return rocprim::segmented_radix_sort_pairs(temp, *temp_bytes, (const unsigned long long*)B.keys, (unsigned long long*)B.keys_sorted,
                                               (const uint32_t*)B.vals, B.vals_sorted, (unsigned int)(B.n * B.n_cols), B.n_cols,
                                               begin, end, 0u, 64u, st);
}

// ------------------------------------------------------------------------------------------------
// Ranks: one workgroup per column walks its sorted column kCorrRankBlock * kCorrRankItems positions at a time, thread
// t holding kCorrRankItems consecutive positions, with the scans' running values carried from step to step.
// Exclusive scan of one value per thread over the workgroup (4 waves), `total` = all of them combined.
template <class Op>
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t v, uint64_t ident, Op op, uint64_t* wave_tot, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d);
        if (lane >= d) x = op(y, x);
    }
    if (lane == 63) wave_tot[w] = x;
    __syncthreads();
    uint64_t pre = ident;
    total = ident;
#pragma unroll
    for (uint32_t i = 0; i < kCorrRankBlock / 64; ++i) {
        if (i < w) pre = op(pre, wave_tot[i]);
        total = op(total, wave_tot[i]);
    }
    uint64_t ex = __shfl_up((unsigned long long)x, 1u);
    if (lane == 0) ex = ident;
    __syncthreads();        // wave_tot is free for the next scan
    return op(pre, ex);
}

struct OpSum { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };
struct OpLastHead { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return keep_last_head(a, b); } };
struct OpNearestTail { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return keep_nearest_tail(a, b); } };

// forwards: P (exclusive prefix sums of the frequencies in sorted order) and, for every position, P at the head of
// its tie group.  Writes lo[p] = P[lb] over the unsorted keys, which nobody reads any more, and p_incl[p] = P[p + 1].
__global__ __launch_bounds__(kCorrRankBlock) void k_corr_rank_fwd(const CorrBatch B) {
    __shared__ uint64_t wave_tot[kCorrRankBlock / 64];
    const uint64_t n = B.n, col = (uint64_t)blockIdx.x * n;
    const uint64_t* keys = B.keys_sorted + col;
    const uint32_t* vals = B.vals_sorted + col;
    uint64_t* lo = B.keys + col;
    uint64_t* p_incl = B.p_incl + col;
    uint64_t carry_sum = 0, carry_head = 0;
    for (uint64_t base = 0; base < n; base += (uint64_t)kCorrRankBlock * kCorrRankItems) {
        const uint64_t p0 = base + (uint64_t)threadIdx.x * kCorrRankItems;
        uint64_t key[kCorrRankItems], f[kCorrRankItems], mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < kCorrRankItems; ++j) {
            const bool in = p0 + j < n;
            key[j] = in ? keys[p0 + j] : 0ull;
            f[j] = in ? B.freq[vals[p0 + j]] : 0ull;
            mine += f[j];
        }
        uint64_t total;
        uint64_t run = carry_sum + block_scan_excl(mine, 0ull, OpSum(), wave_tot, total);
        carry_sum += total;
        uint64_t prev = p0 > 0 && p0 < n ? keys[p0 - 1] : 0ull;
        uint64_t hv[kCorrRankItems], best = 0;
#pragma unroll
        for (uint32_t j = 0; j < kCorrRankItems; ++j) {
            const bool in = p0 + j < n;
            hv[j] = in ? head_value(tie_head(p0 + j, prev, key[j]), run) : 0ull;
            best = keep_last_head(best, hv[j]);
            prev = key[j];
            run += f[j];
            if (in) p_incl[p0 + j] = run;
        }
        uint64_t head = keep_last_head(carry_head, block_scan_excl(best, 0ull, OpLastHead(), wave_tot, total));
        carry_head = keep_last_head(carry_head, total);
#pragma unroll
        for (uint32_t j = 0; j < kCorrRankItems; ++j) {
            head = keep_last_head(head, hv[j]);
            if (p0 + j < n) lo[p0 + j] = head;
        }
    }
}

// backwards (step r of the walk is position n - 1 - r): P at the end of every tie group, then rank2 and d2, scattered
// to the attractor the position belongs to.
__global__ __launch_bounds__(kCorrRankBlock) void k_corr_rank_bwd(const CorrBatch B) {
    __shared__ uint64_t wave_tot[kCorrRankBlock / 64];
    const uint64_t n = B.n, col = (uint64_t)blockIdx.x * n;
    const uint64_t* keys = B.keys_sorted + col;
    const uint32_t* vals = B.vals_sorted + col;
    const uint64_t* lo = B.keys + col;
    const uint64_t* p_incl = B.p_incl + col;
    const uint32_t node = B.col0 + blockIdx.x;
    double* d_row = B.d + (uint64_t)node * n;
    uint64_t carry_tail = kRankNoTail;
    for (uint64_t base = 0; base < n; base += (uint64_t)kCorrRankBlock * kCorrRankItems) {
        const uint64_t r0 = base + (uint64_t)threadIdx.x * kCorrRankItems;
        uint64_t next = r0 > 0 && r0 < n ? keys[n - r0] : 0ull;         // the position after n - 1 - r0
        uint64_t tv[kCorrRankItems], best = kRankNoTail;
#pragma unroll
        for (uint32_t j = 0; j < kCorrRankItems; ++j) {
            tv[j] = kRankNoTail;
            if (r0 + j < n) {
                const uint64_t p = n - 1 - (r0 + j), key = keys[p];
                tv[j] = tail_value(tie_tail(p, n, key, next), p_incl[p]);
                next = key;
            }
            best = keep_nearest_tail(best, tv[j]);
        }
        uint64_t total;
        uint64_t tail = keep_nearest_tail(carry_tail, block_scan_excl(best, kRankNoTail, OpNearestTail(), wave_tot, total));
        carry_tail = keep_nearest_tail(carry_tail, total);
#pragma unroll
        for (uint32_t j = 0; j < kCorrRankItems; ++j) {
            tail = keep_nearest_tail(tail, tv[j]);
            if (r0 + j < n) {
                const uint64_t p = n - 1 - (r0 + j);
                const uint64_t rank2 = rank2_of(lo[p], tail);
                const uint32_t q = vals[p];
                d_row[q] = (double)centred2_of(rank2, B.total);
                if (B.ranks) B.ranks[(uint64_t)q * B.n_nodes + node] = average_rank_of(rank2);
            }
        }
    }
}

hipError_t launch_corr_ranks(const CorrBatch& B, hipStream_t st) {
    hipLaunchKernelGGL(k_corr_rank_fwd, dim3(B.n_cols), dim3(kCorrRankBlock), 0, st, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_corr_rank_bwd, dim3(B.n_cols), dim3(kCorrRankBlock), 0, st, B);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Covariance: S[a][b] = sum over q of (w_q d_qa) d_qb.  One wave per (chunk of kCorrChunk attractors, tile pair
// ta <= tb); 64 attractors of both tiles' 16 rows of D at a time go through LDS (read along q, 512 bytes per row),
// then 16 MFMA steps of 4 attractors each.  v_mfma_f64_16x16x4_f64: lane l gives A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; result register r of lane l is row (l >> 4) + 4 r, column l & 15.  Rows at or above n_nodes and
// attractors at or above n are zeros.  The row stride of 68 doubles spreads a wave's 64-bit LDS reads over all banks.
typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr uint32_t kCovK = 64, kCovStride = 68;

__device__ __forceinline__ void tile_pair_of(uint32_t pair, uint32_t tiles, uint32_t& ta, uint32_t& tb) {
    ta = 0;
    while (pair >= tiles - ta) { pair -= tiles - ta; ++ta; }
    tb = ta + pair;
}

__global__ __launch_bounds__(64) void k_corr_cov(const double* __restrict__ d, const uint64_t* __restrict__ freq, uint64_t n,
                                                  uint32_t n_nodes, double* __restrict__ partials) {
    __shared__ double lds_a[kCorrTile][kCovStride], lds_b[kCorrTile][kCovStride];
    const uint32_t lane = threadIdx.x, tiles = (n_nodes + kCorrTile - 1) / kCorrTile;
    uint32_t ta, tb;
    tile_pair_of(blockIdx.y, tiles, ta, tb);
    const uint64_t q_begin = (uint64_t)blockIdx.x * kCorrChunk;
    const uint64_t q_end = q_begin + kCorrChunk < n ? q_begin + kCorrChunk : n;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (uint64_t q0 = q_begin; q0 < q_end; q0 += kCovK) {
        const uint64_t q = q0 + lane;
        const bool in = q < q_end;
        const double w = in ? (double)freq[q] : 0.0;
#pragma unroll
        for (uint32_t r = 0; r < kCorrTile; ++r) {
            const uint32_t ia = ta * kCorrTile + r, ib = tb * kCorrTile + r;
            const double a = in && ia < n_nodes ? d[(uint64_t)ia * n + q] : 0.0;
            const double b = in && ib < n_nodes ? d[(uint64_t)ib * n + q] : 0.0;
            lds_a[r][lane] = w * a;
            lds_b[r][lane] = b;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t ks = 0; ks < kCovK / 4; ++ks) {
            const double a = lds_a[lane & 15u][4 * ks + (lane >> 4)];
            const double b = lds_b[lane & 15u][4 * ks + (lane >> 4)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = partials + ((uint64_t)blockIdx.x * gridDim.y + blockIdx.y) * (kCorrTile * kCorrTile);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) out[((lane >> 4) + 4 * r) * kCorrTile + (lane & 15u)] = acc[r];
}

// One workgroup per tile pair, one thread per element: the chunk partials in chunk order.  A diagonal tile's lower
// half is not used (its two halves were rounded differently); every element is written to both triangles.
__global__ __launch_bounds__(kCorrTile * kCorrTile) void k_corr_reduce(const double* __restrict__ partials, uint64_t n_chunks,
                                                                        uint32_t n_nodes, double* __restrict__ s_matrix) {
    const uint32_t tiles = (n_nodes + kCorrTile - 1) / kCorrTile, e = threadIdx.x;
    uint32_t ta, tb;
    tile_pair_of(blockIdx.x, tiles, ta, tb);
    const uint32_t i = ta * kCorrTile + e / kCorrTile, j = tb * kCorrTile + e % kCorrTile;
    if (i >= n_nodes || j >= n_nodes || i > j) return;
    double s = 0.0;
    for (uint64_t c = 0; c < n_chunks; ++c) s += partials[(c * gridDim.x + blockIdx.x) * (kCorrTile * kCorrTile) + e];
    s_matrix[(uint64_t)i * n_nodes + j] = s;
    s_matrix[(uint64_t)j * n_nodes + i] = s;
}

hipError_t launch_corr_cov(const double* d, const uint64_t* freq, uint64_t n, uint32_t n_nodes, double* partials, hipStream_t st) {
    const dim3 grid((uint32_t)((n + kCorrChunk - 1) / kCorrChunk), corr_tile_pairs(n_nodes));
    hipLaunchKernelGGL(k_corr_cov, grid, dim3(64), 0, st, d, freq, n, n_nodes, partials);
    return hipGetLastError();
}

hipError_t launch_corr_reduce(const double* partials, uint64_t n_chunks, uint32_t n_nodes, double* s_matrix, hipStream_t st) {
    hipLaunchKernelGGL(k_corr_reduce, dim3(corr_tile_pairs(n_nodes)), dim3(kCorrTile * kCorrTile), 0, st, partials, n_chunks, n_nodes,
                       s_matrix);
    return hipGetLastError();
}

}  // namespace bsx
