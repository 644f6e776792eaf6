// Functional-graph mode of attract (include/bsx.h: bsx_run_attract_fgraph; kernels: bsx_fgraph.hip).
#include <cstring>

#include "bsx_attract_host.h"

using namespace bsx;

// ------------------------------------------------------------------------------------------------
// Functional-graph mode (bsx_fgraph.hip): attract over [first, first + count) of a space whose n <= 32 nodes
// are all 'any', from N = 2^n-sized arrays.  Same results as bsx_run_attract.
extern "C" int bsx_run_attract_fgraph(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                                      uint64_t max_len, bsx_attr_rec* table, uint32_t cap, uint32_t* n_out,
                                      uint64_t* n_no_attractor, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (h->wide) return fail(h, BSX_ERR_UNSUPPORTED, "networks of the wide-state family (more than BSX_MAX_NODES nodes, or BSX_WIDE=1): use bsx_run_attract_wide");
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (int rc = check_range(h, first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    const uint32_t n = h->n_nodes;
    if (n > 32 || h->sp.n_any != n || !h->sp.identity_any || h->sp.n_fv || h->sp.n_pv || h->lut_mode == 2)
        return fail(h, BSX_ERR_UNSUPPORTED, "functional-graph mode needs n <= 32 nodes, all of them 'any', and no variations");
    const uint32_t tp = h->sp.tp_origin;                    // origin perturbations: the search starts at s(T_p)
    const double t_begin = now_ms();
    HIPCHK(h, hipSetDevice(h->device));
    *n_out = 0;
    if (n_no_attractor) *n_no_attractor = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (h->table_dirty) { MergedTable stale; if (int rc = drain_attractor_table(h, stale)) return rc; }
    {
        uint64_t want = 1ull << 16;
        while (want < 2 * (uint64_t)cap) want *= 2;
        if (h->table_slots < want) {
            HIPCHK(h, h->d_table.alloc(want));
            HIPCHK(h, hipMemset(h->d_table.p, 0, want * sizeof(LogRec)));
            h->table_slots = want;
        }
    }
    const uint64_t N = 1ull << n;
    const uint32_t cus = (uint32_t)h->prop.multiProcessorCount;
    const bool capped = max_t != BSX_T_INF;
    const uint64_t cap_rel = capped ? max_t - tp : UINT64_MAX;     // found iff mu + lambda <= max_t - T_p (S7)
    // doubling rounds: 2^rounds must reach every transient that can still be "found"; without a cap, every
    // transient (mu < N)
    uint32_t rounds = 0;
    while (rounds < n && (!capped || (1ull << rounds) <= cap_rel)) ++rounds;
    const uint64_t walk_cap = capped ? std::max<uint64_t>(cap_rel, 1) : (1ull << 22);
    const uint32_t cand_cap = 1u << 22;

    DevBuf<uint32_t>& succ = h->d_fg_a;
    DevBuf<uint32_t>& ja = h->d_fg_b;
    DevBuf<uint32_t>& jb = h->d_fg_c;
    HIPCHK(h, succ.reserve(N));
    HIPCHK(h, ja.reserve(std::max<uint64_t>(N, 1024)));         // phase D reuses ja + jb as one array of N pairs
    HIPCHK(h, jb.reserve(std::max<uint64_t>(N, 1024)));
    DevBuf<uint32_t> d_bits, d_cand;
    DevBuf<unsigned int> d_small;       // [0] candidate cursor, [1] cyclic, [2] open, [3] changed
    HIPCHK(h, d_bits.alloc((N + 31) / 32));
    HIPCHK(h, hipMemsetAsync(d_bits.p, 0, ((N + 31) / 32) * 4, h->stream));
    HIPCHK(h, d_cand.alloc(cand_cap));
    HIPCHK(h, d_small.alloc(4));
    HIPCHK(h, hipMemsetAsync(d_small.p, 0, 16, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));

    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    uint32_t launches = 0;
    // A: successor array
    {
        const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cus * 4, (N + kBlock - 1) / kBlock));
        HIPCHK(h, launch_fg_succ((int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), h->shmem, h->stream, h->net, h->sp, N, succ.p, 0));
        ++launches;
        if (tp) {
            HIPCHK(h, h->d_fg_warm.reserve(N));
            HIPCHK(h, launch_fg_succ((int)h->net.k_mux, h->lut_mode, dim3((uint32_t)blocks), h->shmem, h->stream, h->net, h->sp, N, h->d_fg_warm.p, tp));
            ++launches;
        }
    }
    // B: landing points f^(2^rounds)(s)
    const uint32_t* land = succ.p;
    for (uint32_t r = 0; r < rounds; ++r) {
        uint32_t* out = (r & 1) ? jb.p : ja.p;
        HIPCHK(h, launch_fg_double(land, out, N, cus, h->stream));
        land = out;
        ++launches;
    }
    // C: candidates -> cycle states
    HIPCHK(h, launch_fg_mark(land, N, d_bits.p, cus, h->stream));
    HIPCHK(h, launch_fg_collect(d_bits.p, (N + 31) / 32, d_cand.p, cand_cap, d_small.p, cus, h->stream));
    launches += 2;
    unsigned int small[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(small, d_small.p, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t n_cand = small[0];
    if (n_cand > cand_cap) return fail(h, BSX_ERR_UNSUPPORTED, "functional-graph mode: more than 2^22 distinct landing points (use the trajectory path)");
    uint32_t cyc_slots = 1024;
    while (cyc_slots < 4 * (uint64_t)n_cand) cyc_slots *= 2;
    DevBuf<unsigned char> d_cyc;
    HIPCHK(h, d_cyc.alloc((size_t)(cyc_slots + 1) * fg_cyc_entry_bytes()));
    HIPCHK(h, hipMemsetAsync(d_cyc.p, 0, (size_t)(cyc_slots + 1) * fg_cyc_entry_bytes(), h->stream));
    HIPCHK(h, launch_fg_cycles(succ.p, d_cand.p, n_cand, walk_cap, d_cyc.p, cyc_slots - 1, d_small.p + 1, d_small.p + 2, h->stream));
    ++launches;
    HIPCHK(h, hipMemcpyAsync(small, d_small.p, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!capped && small[2]) return fail(h, BSX_ERR_STEP_LIMIT, "functional-graph mode: a cycle longer than 2^22 states (no time cap given)");
    // D: (entry state, mu) by in-place pointer jumping; pairs live in ja..jb (N x 8 bytes)
    if ((const void*)(ja.p + N) != (const void*)jb.p) {
        // the two halves are separate allocations: use a dedicated pair array instead
        HIPCHK(h, h->d_fg_pair.reserve(N));
    }
    unsigned long long* pair = ((const void*)(ja.p + N) == (const void*)jb.p) ? reinterpret_cast<unsigned long long*>(ja.p) : h->d_fg_pair.p;
    HIPCHK(h, launch_fg_pair_init(succ.p, d_cyc.p, cyc_slots - 1, pair, N, cus, h->stream));
    ++launches;
    const uint32_t d_cap = capped ? (uint32_t)std::min<uint64_t>(cap_rel, 0xFFFFFFFEull) : 0xFFFFFFFEu;
    for (uint32_t r = 0; r < n + 2; ++r) {
        HIPCHK(h, hipMemsetAsync(d_small.p + 3, 0, 4, h->stream));
        HIPCHK(h, launch_fg_pair_jump(pair, N, d_cap, d_small.p + 3, cus, h->stream));
        ++launches;
        HIPCHK(h, hipMemcpyAsync(small, d_small.p, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (!small[3]) break;
    }
    // E: aggregate the requested problems
    AttractParams P{};
    P.ctr = h->d_ctr;
    P.table = h->d_table.p;
    P.table_mask = h->table_slots - 1;
    const uint64_t first_state = first->init_digits[0];
    HIPCHK(h, launch_fg_aggregate(pair, d_cyc.p, cyc_slots - 1, tp ? h->d_fg_warm.p : nullptr, tp, first_state, count, cap_rel, max_len,
                                  capped ? max_t : 0, P, cus, h->stream));
    ++launches;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    Counters ctr{};
    HIPCHK(h, hipMemcpyAsync(&ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->table_dirty = true;
    if (ctr.table_overflow) { MergedTable junk; (void)drain_attractor_table(h, junk); return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's table capacity"); }
    MergedTable merged;
    if (int rc = drain_attractor_table(h, merged)) return rc;
    if (merged.size() > cap) return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's table capacity");
    uint32_t i = 0;
    for (auto& kv : merged) {                       // (at most 2^32 problems: every sum fits the record)
        const WideRec& w = kv.second;
        bsx_attr_rec& a = table[i++];
        for (int k = 0; k < BSX_MAX_WORDS; ++k) a.key[k] = w.key[k];
        a.length = w.length; a.count = (uint64_t)w.count; a.sum_l = w.sum_l.w[0];
        a.sum_l2_lo = w.sum_l2.w[0]; a.sum_l2_hi = w.sum_l2.w[1];
    }
    *n_out = i;
    if (n_no_attractor) *n_no_attractor = ctr.n_none;
    if (stats) {
        stats->problems = count;
        stats->state_steps = ctr.steps_ref;
        stats->executed_steps = N * (1 + (uint64_t)tp);     // one network update per state of the space (+ the warm-up map)
        stats->kernel_ms = ms;
        stats->kernel_launches = launches;
        stats->total_ms = now_ms() - t_begin;
    }
    return BSX_OK;
}
