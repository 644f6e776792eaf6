// bsx_run_damage_sampled (include/bsx.h has the definition): damage spreading over sampled pairs of states, the sums behind
// a Derrida curve.  Host side of k_wide_damage (bsx_wide.hip) over the WideHost the sampled calls work on: the handle's own,
// or the second lowering of a handle of the <= BSX_MAX_NODES family (sample_host, bsx_sample_api.cpp).  Every check comes
// before the first launch; the accumulators are zeroed once on the device, the launches of BSX_WIDE_CHUNK samples add to
// them, and the host waits once.  The caller's arrays are written only when the call succeeds.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_table_lower.h"
#include "bsx_wide_host.h"
// (behind the HIP runtime, which defines what BSX_HD expands to)
#include "bsx_sample.h"

using namespace bsx;

static_assert(BSX_DAMAGE_MAX_FLIPS <= 64, "flip i draws D with argument n_any + 65 + 64 i + lane: 64 lanes per flip");

extern "C" int bsx_run_damage_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint32_t n_flips,
                                      uint32_t n_steps, uint64_t* sum_d, uint64_t* sum_d2, uint64_t* n_merged, uint64_t* hist,
                                      bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (!sum_d || !sum_d2 || !n_merged) return fail(h, BSX_ERR_INVALID, "sum_d / sum_d2 / n_merged is null");
    if (first_sample + n_samples < first_sample) return fail(h, BSX_ERR_INVALID, "first_sample + n_samples wraps");
    if (n_flips == 0 || n_flips > BSX_DAMAGE_MAX_FLIPS) return fail(h, BSX_ERR_INVALID, "n_flips must be 1 .. BSX_DAMAGE_MAX_FLIPS");
    if (n_samples > (1ull << 40)) return fail(h, BSX_ERR_RANGE_TOO_LARGE, "at most 2^40 samples per call");
    if (n_steps > 65535u) return fail(h, BSX_ERR_UNSUPPORTED, "at most 65535 steps");
    const uint64_t n_t = (uint64_t)n_steps + 1, n_bins = (uint64_t)h->n_nodes + 1;
    if (hist && n_t * n_bins > (1ull << 24)) return fail(h, BSX_ERR_UNSUPPORTED, "hist has more than 2^24 cells");
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    WideHost& W = *Wp;
    const WideSpace& S = W.space;
    if (S.n_fv) return fail(h, BSX_ERR_UNSUPPORTED, "damage spreading: the problem space has fixed-node variations");
    if (S.n_pv) return fail(h, BSX_ERR_UNSUPPORTED, "damage spreading: the problem space has perturbation variations");
    if (S.n_sched) return fail(h, BSX_ERR_UNSUPPORTED, "damage spreading: the origin has a perturbation schedule");
    std::vector<uint32_t> free_nodes;
    for (uint32_t i = 0; i < W.net.n; ++i)
        if (!((S.fixmask[i >> 5] >> (i & 31u)) & 1u)) free_nodes.push_back(i);
    if (n_flips > free_nodes.size()) return fail(h, BSX_ERR_INVALID, "n_flips exceeds the number of nodes the origin does not fix");
    const uint32_t rows = W.net.rows, L = S.L;
    if (rows / (kWideThreads / L) > kWideProfileRows)
        return fail(h, BSX_ERR_UNSUPPORTED, "damage spreading: more rows per thread than the kernel's counters hold");
    // LDS: the sums of all steps stay in the workgroup where they fit beside the matrices, else every group adds to HBM
    const size_t lds_limit = 159 * 1024;
    size_t shmem = (size_t)wide_damage_lds_words(rows, L, S.n_fslots, W.net.n, hist != nullptr, (uint32_t)n_t) * 4;
    const bool acc_lds = shmem <= lds_limit;
    if (!acc_lds) shmem = (size_t)wide_damage_lds_words(rows, L, S.n_fslots, W.net.n, hist != nullptr, 0) * 4;
    if (shmem > lds_limit) return fail(h, BSX_ERR_UNSUPPORTED, "damage spreading: the group's tables do not fit the LDS");

    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_samples == 0) {
        for (uint64_t t = 0; t < n_t; ++t) sum_d[t] = sum_d2[t] = n_merged[t] = 0;
        if (hist) std::fill(hist, hist + n_t * n_bins, 0ull);
        return BSX_OK;
    }

    DevBuf<uint32_t> d_free;
    DevBuf<unsigned long long> d_sums, d_hist;
    HIPCHK(h, d_free.upload(free_nodes));
    HIPCHK(h, d_sums.alloc(3 * n_t));
    HIPCHK(h, hipMemsetAsync(d_sums.p, 0, 3 * n_t * 8, h->stream));
    if (hist) {
        HIPCHK(h, d_hist.alloc(n_t * n_bins));
        HIPCHK(h, hipMemsetAsync(d_hist.p, 0, n_t * n_bins * 8, h->stream));
    }
    WideDamageParams Q{};
    WideParams& P = Q.net;
    wide_fill_net(W, P);
    std::memcpy(P.origin, S.origin, sizeof(P.origin));
    P.n_any = S.n_any;
    P.any_nodes = W.d_any.p;
    P.ctr = W.d_ctr.p;
    P.sample_k0 = sample_k0(seed);
    Q.n_flips = n_flips; Q.n_steps = n_steps;
    Q.n_free = (uint32_t)free_nodes.size(); Q.acc_lds = acc_lds ? 1u : 0u;
    Q.free_nodes = d_free.p;
    Q.sums = d_sums.p;
    Q.hist = hist ? d_hist.p : nullptr;

    const uint64_t chunk = std::min<uint64_t>(n_samples, wide_chunk(h, W, 1ull << 18));
    uint32_t launches = 0;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (const Chunk c : chunks(n_samples, chunk)) {
        P.sample_first = first_sample + c.first;
        P.count = c.count;
        HIPCHK(h, launch_wide_damage((int)W.net.K, dim3((uint32_t)wide_blocks(h, W, c.count, shmem)), shmem, h->stream, Q));
        ++launches;
    }
    // the call's one wait: counters, sums and histogram come back behind the last launch
    unsigned long long ctr[4] = {0, 0, 0, 0};
    std::vector<unsigned long long> sums(3 * n_t), cells(hist ? n_t * n_bins : 0);
    float ms = 0.f;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sums.data(), d_sums.p, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (hist) HIPCHK(h, hipMemcpyAsync(cells.data(), d_hist.p, cells.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));

    for (uint64_t t = 0; t < n_t; ++t) {
        sum_d[t] = sums[3 * t]; sum_d2[t] = sums[3 * t + 1]; n_merged[t] = sums[3 * t + 2];
    }
    if (hist) std::copy(cells.begin(), cells.end(), hist);
    put_stats(stats, n_samples, 2 * n_samples * n_steps, ctr[1], ms, launches, t_begin);
    return BSX_OK;
}
