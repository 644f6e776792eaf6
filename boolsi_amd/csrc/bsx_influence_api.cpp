// bsx_run_influence_sampled (include/bsx.h has the definition): the per-node influence matrix over samples, every source
// node on the same sampled states, in one device call.  Host side of k_wide_influence (bsx_wide.hip) over the WideHost the
// sampled calls work on: the handle's own, or the second lowering of a handle of the <= BSX_MAX_NODES family (sample_host,
// bsx_sample_api.cpp).  Every check comes before the first launch (bsx_influence.h has those that need no device); the
// table is zeroed once on the device, the launches of BSX_WIDE_CHUNK trajectories in whole (source, group) items add to it,
// and the host waits once.  The caller's arrays are written only when the call succeeds.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bsx_table_lower.h"
#include "bsx_wide_host.h"
// (behind the HIP runtime, which defines what BSX_HD expands to)
#include "bsx_sample.h"
#include "bsx_influence.h"

using namespace bsx;

extern "C" int bsx_run_influence_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, const uint32_t* sources,
                                         uint32_t n_sources, uint32_t n_steps, uint32_t* influence, uint64_t* n_merged, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    const double t_begin = now_ms();
    if (const InfluenceStatus s = influence_check_args(influence != nullptr, sources != nullptr, n_sources, n_steps, first_sample, n_samples))
        return fail(h, s.status, s.msg.c_str());
    HIPCHK(h, hipSetDevice(h->device));
    WideHost* Wp = nullptr;
    if (int rc = sample_host(h, &Wp)) return rc;
    WideHost& W = *Wp;
    const WideSpace& S = W.space;
    const uint32_t n = W.net.n, rows = W.net.rows, L = S.L, T = n_steps;
    if (const InfluenceStatus s = influence_check_sources(n, S.fixmask, sources, n_sources)) return fail(h, s.status, s.msg.c_str());
    if (const InfluenceStatus s = influence_check_sizes(n_samples, n_sources, T, n)) return fail(h, s.status, s.msg.c_str());
    if (S.n_fv) return fail(h, BSX_ERR_UNSUPPORTED, "influence: the problem space has fixed-node variations");
    if (S.n_pv) return fail(h, BSX_ERR_UNSUPPORTED, "influence: the problem space has perturbation variations");
    if (S.n_sched) return fail(h, BSX_ERR_UNSUPPORTED, "influence: the origin has a perturbation schedule");
    const size_t shmem = (size_t)wide_influence_lds_words(rows, L, S.n_fslots) * 4;
    if (shmem > 159 * 1024) return fail(h, BSX_ERR_UNSUPPORTED, "influence: the group's tables do not fit the LDS");

    const size_t n_rows = (size_t)n_sources * T, n_cells = n_rows * n;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_samples == 0) {
        std::fill(influence, influence + n_cells, 0u);
        if (n_merged) std::fill(n_merged, n_merged + n_rows, 0ull);
        return BSX_OK;
    }

    const InfluenceLayout lay = influence_layout(n_samples, n_sources, L, wide_chunk(h, W, 1ull << 18));
    DevBuf<uint32_t> d_sources, d_cells;
    DevBuf<unsigned long long> d_merged;
    HIPCHK(h, d_sources.upload(std::vector<uint32_t>(sources, sources + n_sources)));
    HIPCHK(h, d_cells.alloc(n_cells));
    HIPCHK(h, hipMemsetAsync(d_cells.p, 0, n_cells * sizeof(uint32_t), h->stream));
    if (n_merged) {
        HIPCHK(h, d_merged.alloc(n_rows));
        HIPCHK(h, hipMemsetAsync(d_merged.p, 0, n_rows * 8, h->stream));
    }
    WideInfluenceParams Q{};
    WideParams& P = Q.net;
    wide_fill_net(W, P);
    std::memcpy(P.origin, S.origin, sizeof(P.origin));
    P.n_any = S.n_any;
    P.any_nodes = W.d_any.p;
    P.ctr = W.d_ctr.p;
    P.sample_k0 = sample_k0(seed);
    Q.first_sample = first_sample; Q.n_samples = n_samples;
    Q.g_per = lay.g_per;
    Q.n_steps = T;
    Q.sources = d_sources.p;
    Q.influence = d_cells.p;
    Q.n_merged = n_merged ? d_merged.p : nullptr;

    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>(lay.chunk_items, wide_blocks(h, W, lay.chunk_items * lay.G, shmem)));
    uint32_t launches = 0;
    HIPCHK(h, hipMemsetAsync(W.d_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (const Chunk c : chunks(lay.items, lay.chunk_items)) {
        Q.p0 = c.first; Q.n_items = c.count;
        HIPCHK(h, launch_wide_influence((int)W.net.K, dim3((uint32_t)std::min<uint64_t>(c.count, blocks)), shmem, h->stream, Q));
        ++launches;
    }
    // the call's one wait: counters, table and merged counts come back behind the last launch
    unsigned long long ctr[4] = {0, 0, 0, 0};
    std::vector<uint32_t> cells(n_cells);
    std::vector<unsigned long long> merged(n_merged ? n_rows : 0);
    float ms = 0.f;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(ctr, W.d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cells.data(), d_cells.p, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (n_merged) HIPCHK(h, hipMemcpyAsync(merged.data(), d_merged.p, n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));

    std::copy(cells.begin(), cells.end(), influence);
    if (n_merged) std::copy(merged.begin(), merged.end(), n_merged);
    const uint64_t problems = (uint64_t)n_sources * n_samples;     // <= 2^40
    put_stats(stats, problems, 2 * problems * T, ctr[1], ms, launches, t_begin);
    return BSX_OK;
}
