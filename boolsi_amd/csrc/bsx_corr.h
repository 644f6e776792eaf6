// Launch interface of the node-correlation kernels (bsx_corr.hip) for bsx_corr_api.cpp.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace bsx {

constexpr uint32_t kCorrChunk = 4096;           // BSX_CORR_CHUNK (include/bsx.h): attractors per covariance partial
constexpr uint32_t kCorrTile = 16;              // nodes per side of a covariance tile (one f64 MFMA result)
constexpr uint32_t kCorrRankBlock = 256;        // threads of a rank workgroup ...
constexpr uint32_t kCorrRankItems = 4;          // ... and sorted positions per thread and step of its walk
constexpr uint64_t kCorrBatchCells = 1ull << 24;    // cells (columns x attractors) sorted and ranked at a time

inline uint32_t corr_tiles(uint32_t n_nodes) { return (n_nodes + kCorrTile - 1) / kCorrTile; }
inline uint32_t corr_tile_pairs(uint32_t n_nodes) { const uint32_t t = corr_tiles(n_nodes); return t * (t + 1) / 2; }

// the columns [col0, col0 + n_cols) of one batch; every array of the batch is n_cols rows of n entries
struct CorrBatch {
    const uint32_t* on_counts;      // [n][n_nodes]
    const uint64_t* lengths;        // [n]
    const uint64_t* freq;           // [n]
    uint64_t n;
    uint32_t n_nodes, col0, n_cols;
    uint64_t total;                 // T
    uint64_t* keys;                 // observe: sort keys, column-major; after the sort: lo (P[lb]) per sorted position
    uint64_t* keys_sorted;
    uint32_t* vals;                 // observe: the attractor index
    uint32_t* vals_sorted;
    uint64_t* p_incl;               // rank, forward walk: inclusive prefix sum per sorted position
    double* d;                      // [n_nodes][n]: centred double ranks (twice the centred rank)
    double* ranks;                  // [n][n_nodes] or null
};

hipError_t launch_corr_observe(const CorrBatch& B, hipStream_t st);
// temp == nullptr: only *temp_bytes is written (nothing is launched)
hipError_t corr_sort_columns(const CorrBatch& B, void* temp, size_t* temp_bytes, hipStream_t st);
hipError_t launch_corr_ranks(const CorrBatch& B, hipStream_t st);       // two launches: forward and backward walk
hipError_t launch_corr_cov(const double* d, const uint64_t* freq, uint64_t n, uint32_t n_nodes, double* partials, hipStream_t st);
hipError_t launch_corr_reduce(const double* partials, uint64_t n_chunks, uint32_t n_nodes, double* s_matrix, hipStream_t st);

}  // namespace bsx
