// bsx_run_node_correlations (include/bsx.h): the matrix S behind the frequency-weighted Spearman correlations of a
// whole attractor table.  The profile stage (bsx_table_host.h) leaves the on-counts in HBM, wanted on the device
// whether or not the caller takes them; the kernels of bsx_corr.hip turn them into ranks and S.  Everything is
// checked before anything is launched; the handle's problem space, cycle journal and mirror image are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_corr.h"
#include "bsx_ranks.h"
#include "bsx_table_host.h"

using namespace bsx;

static_assert(kCorrChunk == BSX_CORR_CHUNK, "the header states the chunk size");
static_assert(sizeof(bsx_u128) == 16, "frequencies are (lo, hi) word pairs");

extern "C" int bsx_run_node_correlations(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                         const bsx_u128* frequencies, uint64_t n, double* s_matrix, double* ranks,
                                         uint32_t* on_counts, uint8_t* closed, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return BSX_OK;
    const TableView table{keys, key_stride, lengths, n};
    TableSizes sizes;
    if (int rc = table_check_args(h, "bsx_run_node_correlations", table, false, nullptr, sizes)) return rc;
    if (!frequencies || !s_matrix) return fail(h, BSX_ERR_INVALID, "bsx_run_node_correlations: frequencies or s_matrix is null");
    uint64_t total = 0;
    switch (corr_total(&frequencies[0].lo, n, &total)) {
        case kCorrTotalOk: break;
        case kCorrTotalZeroFrequency: return fail(h, BSX_ERR_INVALID, "bsx_run_node_correlations: a frequency of 0");
        case kCorrTotalHighWord: return fail(h, BSX_ERR_RANGE_TOO_LARGE, "bsx_run_node_correlations: a frequency of 2^64 or more");
        case kCorrTotalTooLarge: return fail(h, BSX_ERR_RANGE_TOO_LARGE, "bsx_run_node_correlations: total frequency of 2^62 or more");
    }
    const uint32_t n_nodes = h->n_nodes;
    if (n > BSX_CORR_MAX_CELLS / n_nodes)
        return fail(h, BSX_ERR_UNSUPPORTED, "bsx_run_node_correlations: more than 2^31 cells (attractors x nodes)");
    HIPCHK(h, hipSetDevice(h->device));

    // the profile: on-counts stay on the device; its collect waits for the device once and fills `pst`
    const ProfileOut out{on_counts, nullptr, closed};
    ProfileWant want = profile_want(out);
    want.on_counts = true;
    ProfileDev prof;
    bsx_stats pst{};
    if (int rc = profile_stage(h, table, want, nullptr, 0, prof)) return rc;
    if (int rc = profile_enqueue(h, table, prof)) return rc;
    if (int rc = profile_collect(h, table, prof, out, sizes.sum_len, &pst, t_begin)) return rc;

    // columns per batch: the sort's and the ranks' working set is 32 bytes per cell of a batch plus rocprim's own
    const uint64_t batch_cells = h->knobs.corr_batch_cells ? std::min<uint64_t>(h->knobs.corr_batch_cells, BSX_CORR_MAX_CELLS)
                                                           : kCorrBatchCells;
    const uint32_t batch_cols = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_nodes, batch_cells / n));
    const uint64_t cells = (uint64_t)batch_cols * n;                    // (<= 2^31: one column at the most, or batch_cells)
    const uint64_t n_chunks = (n + kCorrChunk - 1) / kCorrChunk;
    const uint32_t pairs = corr_tile_pairs(n_nodes);

    std::vector<uint64_t> freq(n);
    for (uint64_t q = 0; q < n; ++q) freq[q] = frequencies[q].lo;
    DevBuf<uint64_t> d_freq, d_len, d_keys, d_keys_sorted, d_pincl;
    DevBuf<uint32_t> d_vals, d_vals_sorted;
    DevBuf<double> d_d, d_ranks, d_partials, d_s;
    DevBuf<unsigned char> d_temp;
    HIPCHK(h, d_freq.upload(freq));
    HIPCHK(h, d_len.alloc(n));
    HIPCHK(h, hipMemcpy(d_len.p, lengths, n * 8, hipMemcpyHostToDevice));
    HIPCHK(h, d_keys.alloc(cells));
    HIPCHK(h, d_keys_sorted.alloc(cells));
    HIPCHK(h, d_pincl.alloc(cells));
    HIPCHK(h, d_vals.alloc(cells));
    HIPCHK(h, d_vals_sorted.alloc(cells));
    HIPCHK(h, d_d.alloc((uint64_t)n_nodes * n));
    if (ranks) HIPCHK(h, d_ranks.alloc((uint64_t)n_nodes * n));
    HIPCHK(h, d_partials.alloc(n_chunks * pairs * kCorrTile * kCorrTile));
    HIPCHK(h, d_s.alloc((uint64_t)n_nodes * n_nodes));

    CorrBatch B{};
    B.on_counts = prof.on_counts.p; B.lengths = d_len.p; B.freq = d_freq.p;
    B.n = n; B.n_nodes = n_nodes; B.total = total;
    B.keys = d_keys.p; B.keys_sorted = d_keys_sorted.p; B.vals = d_vals.p; B.vals_sorted = d_vals_sorted.p;
    B.p_incl = d_pincl.p; B.d = d_d.p; B.ranks = ranks ? d_ranks.p : nullptr;
    uint32_t launches = 0;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (uint32_t col0 = 0; col0 < n_nodes; col0 += batch_cols) {
        B.col0 = col0;
        B.n_cols = std::min(batch_cols, n_nodes - col0);
        size_t temp_bytes = 0;
        HIPCHK(h, corr_sort_columns(B, nullptr, &temp_bytes, h->stream));
        if (d_temp.n < temp_bytes) {                                    // (frees the old one: not while the device uses it)
            HIPCHK(h, hipStreamSynchronize(h->stream));
            HIPCHK(h, d_temp.alloc(temp_bytes));
        }
        HIPCHK(h, launch_corr_observe(B, h->stream));
        HIPCHK(h, corr_sort_columns(B, d_temp.p, &temp_bytes, h->stream));
        HIPCHK(h, launch_corr_ranks(B, h->stream));
        launches += 4;                                                  // (the sort counted as one)
    }
    HIPCHK(h, launch_corr_cov(d_d.p, d_freq.p, n, n_nodes, d_partials.p, h->stream));
    HIPCHK(h, launch_corr_reduce(d_partials.p, n_chunks, n_nodes, d_s.p, h->stream));
    launches += 2;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(s_matrix, d_s.p, (uint64_t)n_nodes * n_nodes * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (ranks) HIPCHK(h, hipMemcpyAsync(ranks, d_ranks.p, (uint64_t)n_nodes * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (stats) {
        *stats = pst;
        stats->kernel_ms += ms;
        stats->kernel_launches += launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}
