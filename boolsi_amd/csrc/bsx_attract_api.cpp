// Host side of attract (include/bsx.h: bsx_run_attract, bsx_run_attract2): one waited-for pass of the detector / lean /
// class-pool kernels, the tile ladder over a segment of the space, and the two entry points.  The cube cascade that takes
// the aligned blocks is bsx_cascade.cpp (analysis: bsx_cube_plan.cpp), the exact wide-integer merge bsx_merge.h, the
// functional-graph mode bsx_fgraph_api.cpp.
// No CPU compute path exists here: every problem is resolved by gfx950 kernels (bsx_attract.hip, bsx_lean.hip,
// bsx_pool_kernel.h, bsx_fgraph.hip); the host only reads truth tables (which digits can matter) and adds up sums.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bsx_attract_host.h"

using namespace bsx;

namespace {
constexpr uint64_t kFastMinProblems = 8192;     // below this the general kernel alone is used
constexpr uint64_t kDiscoverySample = 65536;    // problems (sampled over the range) run through the detector when nothing is cached yet
constexpr uint64_t kLeanTile = 1ull << 28;      // problems per lean-kernel launch (straggler list: 4 B each)
constexpr uint32_t kFastSteps = 48;             // FAST phase length (steps without a cached cycle state), first guess
constexpr uint64_t kProbeTile = 1ull << 22;     // lean tiles while the FAST length is being calibrated
constexpr uint64_t kGeneralTile = 1ull << 32;   // problems per launch of the general kernel (32-bit offsets)
}  // namespace

namespace bsx {

// One launch of the general / lean / pool kernel over P.count work items + merge of its log into `merged` (null:
// results discarded).  The host waits for it: these passes decide what runs next (stragglers, calibration).
int launch_attract_pass(bsx_handle h, AttractParams& P, int kind, DevBuf<LogRec>& d_log, MergedTable* merged,
                        AttractRun& run, Totals& tot) {
    const double pt0 = now_ms();
    const bool fast = kind != kPassGeneral;
    if (!fast) h->journal_stale = true;         // the detector may publish attractors
    size_t shmem = h->shmem_attract;
    if (fast) {
        uint32_t slots = h->cache_lds_slots;
        if (int rc = lean_mirror_slots(h, &slots, &tot)) return rc;
        P.cc.lds_slots = slots;
        shmem = h->shmem + (size_t)slots * h->cache_stride + 32 + (kind == kPassPool ? pool_extra_bytes(h->net.nw) : lean_acc_bytes(h->net.nw));
    }
    const Launch L = plan_persistent(h, P.count, shmem);
    P.chunk = L.chunk;
    // plain tiles, whose cost per problem varies by region: every wave starts with one piece and takes the rest from the
    // cursor (measured on config 3's plain tiles: fixed three-quarter shares 2.5 ms against 1.9 ms)
    if (kind == kPassPool) P.chunk_first = P.chunk;
    if (h->knobs.chunk) { P.chunk = h->knobs.chunk; P.chunk_first = P.chunk; }     // tuning knob
    const uint64_t waves = (uint64_t)L.grid.x * kWavesPerBlock;
    const uint64_t log_cap = waves * kTableSlots + (1u << 16);
    if (d_log.n < log_cap) HIPCHK(h, d_log.alloc(log_cap));
    P.log = d_log.p;
    P.log_cap = log_cap;
    P.ctr = h->d_ctr;
    P.level_in = nullptr;
    // results that are kept may spill from the log into the HBM attractor table (general kernel only: the
    // lean / pool kernels write at most one record per workgroup and cached attractor)
    P.table = (merged && !fast && h->table_slots) ? h->d_table.p : nullptr;
    P.table_mask = h->table_slots ? h->table_slots - 1 : 0;
    if (kind == kPassPool) if (int rc = ensure_mirror_image(h, P, shmem)) return rc;
    const double pt1 = now_ms();
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (kind == kPassPool) HIPCHK(h, launch_attract_pool((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, L.grid, shmem, h->stream, P));
    else if (kind == kPassLean) HIPCHK(h, launch_attract_fast((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, L.grid, shmem, h->stream, P));
    else HIPCHK(h, launch_attract((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, L.grid, shmem, h->stream, P));
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    const double pt2 = now_ms();
    HIPCHK(h, hipMemcpyAsync(h->h_ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++tot.syncs;
    run.ctr = *h->h_ctr;
    const double pt3 = now_ms();
    HIPCHK(h, hipEventElapsedTime(&run.ms, h->ev0, h->ev1));
    tot.prof[0] += pt1 - pt0; tot.prof[1] += pt2 - pt1; tot.prof[2] += pt3 - pt2; tot.prof[3] += run.ms;
    if (h->knobs.debug)
        std::fprintf(stderr, "[bsx] %s pass: %llu problems, %llu lane-steps, %llu stragglers, %.3f ms (BSX_DIAG build: %llu wave iterations, %llu service rounds)\n",
                     kind == kPassPool ? "pool" : fast ? "lean" : "general", (unsigned long long)P.count, (unsigned long long)run.ctr.steps_exec,
                     (unsigned long long)run.ctr.n_stragglers, run.ms, (unsigned long long)run.ctr.wave_iters,
                     (unsigned long long)run.ctr.service_rounds);
    if (h->knobs.debug && run.ctr.wave_iters)
        std::fprintf(stderr, "[bsx]   diag: kept after fresh stages %llu, lanes into pool stages %llu, kept after pool stages %llu, merged away %llu\n",
                     (unsigned long long)run.ctr.diag[0], (unsigned long long)run.ctr.diag[1], (unsigned long long)run.ctr.diag[2], (unsigned long long)run.ctr.diag[3]);
    if (h->knobs.debug && run.ctr.phase_max[0])
        std::fprintf(stderr, "[bsx]   diag: %u workgroups; prologue / loop / epilogue, us: mean %.1f / %.1f / %.1f, slowest %.1f / %.1f / %.1f\n", L.grid.x,
                     run.ctr.phase_sum[0] / 100.0 / L.grid.x, run.ctr.phase_sum[1] / 100.0 / L.grid.x, run.ctr.phase_sum[2] / 100.0 / L.grid.x,
                     run.ctr.phase_max[0] / 100.0, run.ctr.phase_max[1] / 100.0, run.ctr.phase_max[2] / 100.0);
    if (!merged) return BSX_OK;                 // results discarded (discovery): a full log does not matter
    if (run.ctr.table_inserts) h->table_dirty = true;
    if (run.ctr.log_overflow) return fail(h, BSX_ERR_TABLE_FULL, "device attractor log overflowed");
    if (run.ctr.table_overflow) return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's table capacity (device table full)");
    const uint64_t n_log = std::min<uint64_t>(run.ctr.log_cursor, log_cap);
    std::vector<LogRec> log(n_log);
    if (n_log) { HIPCHK(h, hipMemcpy(log.data(), d_log.p, n_log * sizeof(LogRec), hipMemcpyDeviceToHost)); ++tot.syncs; }
    merge_records(*merged, log.data(), log.size(), h->net.nw);
    return BSX_OK;
}

// Entries of the HBM attractor table -> `merged`; the table is left empty for the next call.
int drain_attractor_table(bsx_handle h, MergedTable& merged) {
    if (!h->table_dirty) return BSX_OK;
    h->table_dirty = false;
    DevBuf<unsigned long long> d_cursor;
    DevBuf<LogRec> d_out;
    HIPCHK(h, d_cursor.alloc(1));
    HIPCHK(h, hipMemsetAsync(d_cursor.p, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, d_out.alloc(h->table_slots));
    HIPCHK(h, launch_table_drain(h->d_table.p, h->table_slots, d_out.p, h->table_slots, d_cursor.p, h->stream));
    unsigned long long n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, d_cursor.p, sizeof(n), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<LogRec> recs(n);
    if (n) HIPCHK(h, hipMemcpy(recs.data(), d_out.p, n * sizeof(LogRec), hipMemcpyDeviceToHost));
    merged.reserve(merged.size() + n);
    merge_records(merged, recs.data(), recs.size(), h->net.nw);
    return BSX_OK;
}

int ensure_attractor_table(bsx_handle h, uint32_t cap) {
    if (h->table_dirty) { MergedTable stale; if (int rc = drain_attractor_table(h, stale)) return rc; }     // a failed call left entries behind
    // HBM attractor table behind the log: two slots per entry of the caller's table (kept zeroed between calls)
    uint64_t want = 1ull << 16;
    while (want < 2 * (uint64_t)cap) want *= 2;
    if (h->table_slots < want) {
        HIPCHK(h, h->d_table.alloc(want));
        HIPCHK(h, hipMemset(h->d_table.p, 0, want * sizeof(LogRec)));
        h->table_slots = want;
        h->table_dirty = false;
    }
    return BSX_OK;
}

}  // namespace bsx

namespace {

// first + delta for spaces whose initial-state digits fit one word (the fast path's precondition)
void advance_first(DevSpace& sp, const bsx_index& first, uint64_t delta) {
    for (int w = 0; w < 4; ++w) sp.first_digits[w] = first.init_digits[w];
    sp.first_digits[0] += delta;
    sp.first_variant = first.variant;
}

// ---- one segment: [first, first + count) inside the space the handle currently describes ------------------------------
// (for a plain space -- no variations, at most 64 'any' nodes -- the segment lies within its 2^n_any initial states,
// count <= 2^64; with variations the index carries into the variant number)
int attract_segment(bsx_handle h, const bsx_index& first, u128 count, uint64_t max_t, uint64_t max_len,
                    bsx_problem_rec* per_problem, Totals& tot) {
    DevBuf<LogRec>& d_log = h->d_log;
    DevBuf<ProblemRec32> d_pp;
    if (per_problem) HIPCHK(h, d_pp.alloc((size_t)count));

    AttractParams P{};
    P.net = h->net;
    P.sp = h->sp;
    set_first(P.sp, &first);
    P.count = 0;
    P.cap_rel_inf = max_t == BSX_T_INF ? 1 : 0;
    P.max_t = max_t;
    P.max_len = max_len;
    P.ctr = h->d_ctr;
    P.per_problem = per_problem ? d_pp.p : nullptr;
    P.cc.journal = h->d_cc_journal.p;
    P.cc.journal_count = h->d_cc_count.p;
    P.cc.claims = h->d_cc_claims.p;
    // cycles depend on the fixed nodes: with fixed-node variations they differ per problem
    P.cc.enabled = (h->cache_enabled && h->sp.n_fv == 0) ? 1u : 0u;
    P.cc.lds_slots = h->cache_lds_slots;
    if (!h->fast_steps) h->fast_steps = kFastSteps;
    P.fast_steps = h->fast_steps;
    P.pad = h->knobs.service_lanes;

    MergedTable& merged = tot.merged;

    // Fast path: simple enumeration (no variations, 'any' nodes = nodes 0..a-1 or a few runs, a <= 64), cycle cache on.
    // [discovery prefix with the detector] -> lean / pool kernel -> stragglers.
    // (a short uniform warm-up is fine; its length enters the lean kernel's 32-bit sums of trajectory_l^2)
    const bool simple = h->sp.n_any <= 64 && (h->sp.identity_any || h->sp.n_runs) && !h->sp.n_fv && !h->sp.n_pv && h->sp.tp_origin <= 200;
    bool use_fast = P.cc.enabled && simple && h->fast_ok && count >= kFastMinProblems;
    use_fast = use_fast && h->knobs.lean;       // tuning / test knob
    if (h->knobs.debug) std::fprintf(stderr, "[bsx] attract: count %llu%s cache %u identity %u n_any %u n_fv %u n_pv %u tp %u fast_ok %d -> lean path %d\n", (unsigned long long)count, (count >> 64) ? " (+2^64)" : "", P.cc.enabled, h->sp.identity_any, h->sp.n_any, h->sp.n_fv, h->sp.n_pv, h->sp.tp_origin, (int)h->fast_ok, (int)use_fast);
    u128 done = 0;
    if (use_fast) {
        unsigned int known = 0;
        if (h->journal_stale || h->h_journal.empty()) {
            HIPCHK(h, hipMemcpy(&known, h->d_cc_count.p, sizeof(known), hipMemcpyDeviceToHost));
            ++tot.syncs;
        } else known = (unsigned int)h->h_journal.size();
        if (known == 0) {
            // Nothing cached yet: run the detector over a pseudo-random sample of the range (all digit
            // positions vary), only to fill the cycle cache; its results are discarded and every problem
            // is counted exactly once below.
            const uint64_t m = (uint64_t)std::min<u128>(count, kDiscoverySample);
            std::vector<uint32_t> sample(m);
            for (uint64_t i = 0; i < m; ++i) {
                uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;        // splitmix64 finaliser
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                sample[i] = (uint32_t)((z ^ (z >> 31)) % (uint64_t)std::min<u128>(count, (u128)1 << 32));
            }
            DevBuf<uint32_t> d_sample;
            HIPCHK(h, d_sample.upload(sample));
            AttractParams Q = P;
            Q.count = m;
            Q.offsets = d_sample.p;
            Q.per_problem = nullptr;
            AttractRun r;
            if (int rc = launch_attract_pass(h, Q, kPassGeneral, d_log, nullptr, r, tot)) return rc;
            tot.book(r, false, false);
            HIPCHK(h, hipMemcpy(&known, h->d_cc_count.p, sizeof(known), hipMemcpyDeviceToHost));
            ++tot.syncs;
            if (known == 0) use_fast = false;           // nothing cacheable was found
        }
    }
    // Lean kernel over tiles; what it cannot resolve (attractors not cached yet, long transients) goes
    // through the detector right after each tile, which also teaches the cache for the next tile.
    // The first tiles of a space are small probes: if most of their stragglers did end on a cached
    // cycle state (just later than the FAST length), the FAST length is quadrupled for what follows.
    // BSX_MERGE: 2 (default) class-pool kernel, 1 lean kernel with the in-lane sibling merge, 0 lean kernel
    // without merging (A/B runs, tests)
    int merge_mode = h->knobs.merge;
    if (merge_mode == 2 && !h->pool_ok) merge_mode = 1;
    const bool merge_lanes = merge_mode != 0;
    // Lean / pool kernel over [done, seg_end) in tiles, then the detector over whatever the fast path gave up on.
    auto run_tiles = [&](u128 seg_end) -> int {
    while (use_fast && h->fast_ok && done < seg_end) {
        const uint64_t tile = (uint64_t)std::min<u128>(seg_end - done, h->fast_calibrated ? kLeanTile : kProbeTile);
        if (int rc = lean_mirror_slots(h, nullptr, &tot)) return rc;          // (refreshes h->h_journal if the detector ran since)
        const unsigned int known_before_tile = (unsigned int)h->h_journal.size();
        // straggler list: one word per problem, or up to three per class (base + 64-bit member mask) from the
        // pool kernel -- probe tiles get room for every problem as a class of its own, big tiles for a third
        // (more stragglers than that and the lean path is the wrong tool anyway)
        const uint64_t strag_cap = h->fast_calibrated ? tile : 3 * tile;
        DevBuf<uint32_t>& d_strag = h->d_strag;
        if (d_strag.n < strag_cap) HIPCHK(h, d_strag.alloc(strag_cap));
        AttractParams Q = P;
        advance_first(Q.sp, first, (uint64_t)done);
        Q.count = tile;
        Q.fast_steps = h->fast_steps;
        // the pool kernel first runs with member counts (classes of different groups merge too); that only works
        // while nothing has to go back to the general kernel, so a tile that raises the abort flag is repeated
        // with member masks.  Per-problem records need the masks from the start.
        bool counting = merge_mode == 2 && !per_problem && (h->fast_calibrated || h->knobs.force_counting);     // (knob: tests)
        Q.merge = counting ? 2u : (merge_lanes ? 1u : 0u);
        Q.per_problem = per_problem ? d_pp.p + (uint64_t)done : nullptr;
        Q.stragglers = d_strag.p;
        Q.stragglers_cap = strag_cap;
        AttractRun r;
        MergedTable tile_table;         // folded into `merged` only if the pass is accepted
        if (int rc = launch_attract_pass(h, Q, merge_mode == 2 ? kPassPool : kPassLean, d_log, &tile_table, r, tot)) return rc;
        if (counting && (r.ctr.straggler_overflow & 2u)) {
            tot.kernel_ms += r.ms; ++tot.launches;              // dropped pass
            counting = false;
            Q.merge = 1u;
            tile_table.clear();
            r = AttractRun{};
            if (int rc = launch_attract_pass(h, Q, kPassPool, d_log, &tile_table, r, tot)) return rc;
        }
        if (r.ctr.straggler_overflow) {
            // more (group, mask) pairs than the list holds: the cache does not cover this space.  Drop the
            // pass and give the rest of the range to the detector.
            tot.kernel_ms += r.ms; ++tot.launches;
            h->fast_ok = false;
            break;
        }
        fold_table(merged, tile_table);
        tot.book(r, true);
        uint64_t late = 0;
        if (r.ctr.n_stragglers) {
            uint64_t n_list = r.ctr.n_stragglers;
            if (merge_lanes) {
                // (group base, member mask words) records -> problem offsets, ascending
                const size_t rec = merge_mode == 2 ? 3 : 2;     // the pool kernel's groups have 64 members
                std::vector<uint32_t> pairs(rec * r.ctr.straggler_classes);
                HIPCHK(h, hipMemcpy(pairs.data(), d_strag.p, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
                ++tot.syncs;
                std::vector<uint32_t> offs;
                offs.reserve(n_list);
                for (size_t c = 0; c + rec <= pairs.size(); c += rec)
                    for (size_t wd = 1; wd < rec; ++wd)
                        for (uint32_t left = pairs[c + wd]; left; left &= left - 1)
                            offs.push_back(pairs[c] + (uint32_t)(32 * (wd - 1)) + (uint32_t)__builtin_ctz(left));
                std::sort(offs.begin(), offs.end());
                n_list = offs.size();
                HIPCHK(h, hipMemcpy(d_strag.p, offs.data(), offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            }
            AttractParams S = Q;
            S.count = n_list;
            S.offsets = d_strag.p;
            S.stragglers = nullptr;
            S.merge = 0;
            AttractRun rs;
            if (int rc = launch_attract_pass(h, S, kPassGeneral, d_log, &merged, rs, tot)) return rc;
            tot.book(rs, true);
            late = rs.ctr.n_cache_resolved;
        }
        done += tile;
        const bool many = r.ctr.n_stragglers > tile / 32;
        if (h->knobs.debug) std::fprintf(stderr, "[bsx] tile %llu: %llu stragglers, %llu of them ended on a cached cycle state; FAST length %u\n", (unsigned long long)tile, (unsigned long long)r.ctr.n_stragglers, (unsigned long long)late, h->fast_steps);
        if (many && 2 * late >= r.ctr.n_stragglers && h->fast_steps < kFastStepsMax) {
            h->fast_steps = std::min(kFastStepsMax, h->fast_steps * 4);     // long transients: give FAST more steps
        } else {
            if (tile >= kFastMinProblems) h->fast_calibrated = true;
            if (r.ctr.n_stragglers > tile / 2) {
                // Most of the tile went to the detector.  If that taught the cache new attractors (a region of the
                // space nobody had visited), the next tile will do better; if not -- cycles too long to cache,
                // or more attractors than the mirror holds -- the lean path is the wrong tool for this space.
                unsigned int known_now = 0;
                HIPCHK(h, hipMemcpy(&known_now, h->d_cc_count.p, sizeof(known_now), hipMemcpyDeviceToHost));
                ++tot.syncs;
                if (known_now <= known_before_tile) h->fast_ok = false;
            }
        }
    }
    // not (or no longer) a case for the lean path: the detector takes the rest, 2^32 problems per launch
    while (done < seg_end) {
        const uint64_t tile = (uint64_t)std::min<u128>(seg_end - done, kGeneralTile);
        AttractParams Q = P;
        const bsx_index at = index_plus(first, done, h->sp.n_any);
        set_first(Q.sp, &at);
        Q.count = tile;
        Q.per_problem = per_problem ? d_pp.p + (uint64_t)done : nullptr;
        AttractRun r;
        if (int rc = launch_attract_pass(h, Q, kPassGeneral, d_log, &merged, r, tot)) return rc;
        tot.book(r, true);
        done += tile;
    }
    return BSX_OK;
    };

    // ---- cube collapse: aligned blocks of >= 2^kCubeMinBits problems are enumerated by their relevant digits
    // only (see build_cube).  Everything before the first / after the last such block goes through the tiles.
    // (a warm-up under origin perturbations is fine: the first update still depends on the relevant digits only)
    const bool cubes_ok = use_fast && merge_mode == 2 && !per_problem &&
                          h->knobs.cubes && h->sp.n_any >= kCubeMinBits;     // (BSX_CUBES=0: off -- A/B runs, tests)
    if (cubes_ok) {
        // [first, first + count) in digit values; blocks are aligned in the digit value, not in the offset
        const u128 lo = first.init_digits[0], hi = lo + count;
        const u128 unit = (u128)1 << kCubeMinBits;
        u128 at = (lo + unit - 1) / unit * unit;
        const u128 body_end = hi / unit * unit;
        const CascadeEnv env{P, max_t, max_len, tot, d_log};
        if (at < body_end) {
            if (int rc = run_tiles(at - lo)) return rc;
            while (at < body_end) {
                uint32_t a_bits = kCubeMaxBits;
                while (a_bits > kCubeMinBits && ((at & (((u128)1 << a_bits) - 1)) != 0 || at + ((u128)1 << a_bits) > body_end)) --a_bits;
                a_bits = std::min(a_bits, h->sp.n_any);
                bool collapsed = false;
                // a block that does not collapse is tried again in halves down to 2^32 problems, below that it is the tiles' turn
                for (;;) {
                    if (int rc = run_block(h, env, (uint64_t)at, a_bits, collapsed)) return rc;
                    if (collapsed || a_bits <= 32) break;
                    --a_bits;
                }
                const u128 block_end = (at - lo) + ((u128)1 << a_bits);
                if (collapsed) done = block_end;
                else if (int rc = run_tiles(block_end)) return rc;
                at += (u128)1 << a_bits;
            }
        }
    }
    if (int rc = run_tiles(count)) return rc;

    if (per_problem) {
        const uint32_t nw = h->net.nw;
        const uint64_t n = (uint64_t)count;
        std::vector<ProblemRec32> pp(n);
        HIPCHK(h, hipMemcpy(pp.data(), d_pp.p, n * sizeof(ProblemRec32), hipMemcpyDeviceToHost));
        for (uint64_t p = 0; p < n; ++p) {
            bsx_problem_rec o{};
            for (uint32_t w = 0; w < nw; ++w) o.key[w >> 1] |= (uint64_t)pp[p].key[w] << (32 * (w & 1));
            o.length = pp[p].length; o.trajectory_l = pp[p].trajectory_l; o.found = pp[p].found;
            per_problem[p] = o;
        }
    }
    return BSX_OK;
}

// Spaces with more than 64 'any' nodes (e.g. a 128-node network with every node 'any'): only the 64 lowest initial-state
// digits change inside 2^64 consecutive problems.  Such a stretch is run as the space in which exactly those are 'any'
// and the higher digits belong to the origin state -- a plain space, which gets the lean / pool / cube paths.  (Same
// network, same fixed nodes: the cycle cache carries over from stretch to stretch.)
int attract_high_digits(bsx_handle h, const bsx_index& first, u128 count, uint64_t max_t, uint64_t max_len, Totals& tot) {
    struct Restore {                    // the handle describes the whole space again, whatever happens below
        bsx_handle h; DevSpace sp; std::vector<uint32_t> any;
        ~Restore() { h->sp = sp; h->model.any = any; }
    } restore{h, h->sp, h->model.any};
    const DevSpace whole = h->sp;
    const std::vector<uint32_t> any = h->model.any;
    bool identity = true;
    for (uint32_t j = 0; j < 64; ++j) identity = identity && any[j] == j;
    bsx_index at = first;
    while (count) {
        const u128 room = ((u128)1 << 64) - at.init_digits[0];
        const u128 seg = std::min(count, room);
        DevSpace sv = whole;
        for (uint32_t j = 64; j < whole.n_any; ++j)
            if ((at.init_digits[j >> 6] >> (j & 63)) & 1ull) sv.origin[any[j] >> 5] |= 1u << (any[j] & 31);
        sv.n_any = 64;
        sv.identity_any = identity ? 1 : 0;
        sv.n_runs = 0;
        if (!identity) {
            uint32_t j = 0, r = 0;
            while (j < 64) {
                uint32_t len = 1;
                while (j + len < 64 && any[j + len] == any[j] + len && ((any[j] + len) >> 5) == (any[j] >> 5)) ++len;
                sv.deposit[2 * r] = j | (any[j] >> 5) << 8 | (any[j] & 31u) << 16;
                sv.deposit[2 * r + 1] = len >= 32 ? 0xFFFFFFFFu : (1u << len) - 1u;
                ++r;
                j += len;
            }
            sv.n_runs = r;                  // <= 64 = kMaxDepositRuns
        }
        h->sp = sv;
        h->model.any.assign(any.begin(), any.begin() + 64);
        bsx_index f{};
        f.init_digits[0] = at.init_digits[0];
        const int rc = attract_segment(h, f, seg, max_t, max_len, nullptr, tot);
        h->sp = whole;
        h->model.any = any;
        if (rc) return rc;
        at = index_plus(at, seg, whole.n_any);
        count -= seg;
    }
    return BSX_OK;
}

// attract.py:262-302 semantics for every problem of [first, first + count): the body of both entry points.
int attract_core(bsx_handle h, const bsx_index& first, u128 count, uint64_t max_t, uint64_t max_len, uint32_t cap,
                 bsx_problem_rec* per_problem, Totals& tot) {
    if (int rc = ensure_attractor_table(h, cap)) return rc;
    int rc;
    if (h->sp.n_any > 64 && !h->sp.n_fv && !h->sp.n_pv && h->sp.tp_origin <= 200 && !per_problem && count >= (1u << 13) &&
        h->cache_enabled && h->knobs.lean)
        rc = attract_high_digits(h, first, count, max_t, max_len, tot);
    else
        rc = attract_segment(h, first, count, max_t, max_len, per_problem, tot);
    if (rc) return rc;
    if (int rc2 = drain_attractor_table(h, tot.merged)) return rc2;
    if (tot.merged.size() > cap) return fail(h, BSX_ERR_TABLE_FULL, "more distinct attractors than the caller's table capacity");
    if (h->knobs.profile)
        std::fprintf(stderr, "[bsx] profile: passes: setup %.3f, enqueue %.3f, wait %.3f (kernels %.3f), split estimates %.3f, reading the counters %.3f; %u host syncs\n",
                     tot.prof[0], tot.prof[1], tot.prof[2], tot.prof[3], tot.prof[4], tot.prof[5], tot.syncs);
    return BSX_OK;
}

int attract_preamble(bsx_handle h, const bsx_index* first, u128 count, uint64_t max_t) {
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    if (int rc = check_range(h, first, count)) return rc;
    if (int rc = check_max_t(h, max_t)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return BSX_OK;
}

bool fgraph_knob(bsx_handle h) {            // knob: route eligible calls through the functional-graph mode
    return h->knobs.fgraph && h->n_nodes <= 32 && h->sp.n_any == h->n_nodes && h->sp.identity_any && !h->sp.n_fv &&
           !h->sp.n_pv && h->lut_mode != 2;
}

}  // namespace

extern "C" int bsx_run_attract(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                               uint64_t max_len, bsx_attr_rec* table, uint32_t cap, uint32_t* n_out,
                               uint64_t* n_no_attractor, bsx_problem_rec* per_problem, bsx_stats* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (h->wide) return fail(h, BSX_ERR_UNSUPPORTED, "networks of the wide-state family (more than BSX_MAX_NODES nodes, or BSX_WIDE=1): use bsx_run_attract_wide");
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (int rc = attract_preamble(h, first, count, max_t)) return rc;
    const double t_begin = now_ms();
    *n_out = 0;
    if (n_no_attractor) *n_no_attractor = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;
    if (!per_problem && fgraph_knob(h))
        return bsx_run_attract_fgraph(h, first, count, max_t, max_len, table, cap, n_out, n_no_attractor, stats);
    if (per_problem && count > (1ull << 32)) return fail(h, BSX_ERR_INVALID, "at most 2^32 problems per call with per-problem records");

    Totals tot;
    if (int rc = attract_core(h, *first, count, max_t, max_len, cap, per_problem, tot)) return rc;
    uint32_t i = 0;
    for (auto& kv : tot.merged) {
        const WideRec& w = kv.second;
        if ((w.count >> 64) != 0 || !w.sum_l.fits(1) || !w.sum_l2.fits(2))
            return fail(h, BSX_ERR_RANGE_TOO_LARGE, "an attractor's count / sum of trajectory lengths exceeds the 64-bit fields of bsx_attr_rec: use bsx_run_attract2");
        bsx_attr_rec& a = table[i++];
        for (int k = 0; k < BSX_MAX_WORDS; ++k) a.key[k] = w.key[k];
        a.length = w.length; a.count = (uint64_t)w.count; a.sum_l = w.sum_l.w[0];
        a.sum_l2_lo = w.sum_l2.w[0]; a.sum_l2_hi = w.sum_l2.w[1];
    }
    *n_out = i;
    if (n_no_attractor) *n_no_attractor = (uint64_t)tot.n_none;
    if (stats) {
        stats->problems = count;
        stats->state_steps = (uint64_t)tot.steps_ref;           // (count < 2^64 and trajectories < 2^31: may wrap only beyond 2^33 x ... problems; bsx_run_attract2 is wide)
        stats->executed_steps = tot.steps_exec;
        stats->kernel_ms = tot.kernel_ms;
        stats->kernel_launches = tot.launches;
        stats->total_ms = now_ms() - t_begin;
    }
    if (tot.limit_hits) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit without closing its cycle");
    return BSX_OK;
}

extern "C" int bsx_run_attract2(bsx_handle h, bsx_u128 first_flat, bsx_u128 count_flat, uint64_t max_t, uint64_t max_len,
                                bsx_attr_rec2* table, uint32_t cap, uint32_t* n_out, bsx_u128* n_no_attractor,
                                bsx_stats2* stats) {
    if (!h) return BSX_ERR_INVALID;
    h->knobs = Knobs::from_env();
    if (h->wide) return fail(h, BSX_ERR_UNSUPPORTED, "networks of the wide-state family (more than BSX_MAX_NODES nodes, or BSX_WIDE=1): use bsx_run_attract_wide");
    if (!table || !n_out) return fail(h, BSX_ERR_INVALID, "table / n_out is null");
    if (!h->have_net || !h->have_space) return fail(h, BSX_ERR_STATE, "network / problem space not set");
    // flat index I = init_digits + variant * 2^n_any (batching.py:212-229)
    const u128 I = ((u128)first_flat.hi << 64) | first_flat.lo, count = ((u128)count_flat.hi << 64) | count_flat.lo;
    const uint32_t n_any = h->sp.n_any;
    bsx_index first{};
    if (n_any >= 128) { first.init_digits[0] = (uint64_t)I; first.init_digits[1] = (uint64_t)(I >> 64); }
    else {
        const u128 low = I & (((u128)1 << n_any) - 1), variant = I >> n_any;
        if ((variant >> 64) != 0) return fail(h, BSX_ERR_UNSUPPORTED, "variant part of the problem index exceeds 64 bits");
        first.init_digits[0] = (uint64_t)low; first.init_digits[1] = (uint64_t)(low >> 64);
        first.variant = (uint64_t)variant;
    }
    if (int rc = attract_preamble(h, &first, count, max_t)) return rc;
    const double t_begin = now_ms();
    *n_out = 0;
    if (n_no_attractor) *n_no_attractor = bsx_u128{0, 0};
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (count == 0) return BSX_OK;

    Totals tot;
    if (int rc = attract_core(h, first, count, max_t, max_len, cap, nullptr, tot)) return rc;
    uint32_t i = 0;
    for (auto& kv : tot.merged) {
        const WideRec& w = kv.second;
        bsx_attr_rec2& a = table[i++];
        for (int k = 0; k < BSX_MAX_WORDS; ++k) a.key[k] = w.key[k];
        a.length = w.length;
        a.count.lo = (uint64_t)w.count; a.count.hi = (uint64_t)(w.count >> 64);
        for (int k = 0; k < 3; ++k) a.sum_l[k] = w.sum_l.w[k];
        for (int k = 0; k < 4; ++k) a.sum_l2[k] = w.sum_l2.w[k];
    }
    *n_out = i;
    if (n_no_attractor) { n_no_attractor->lo = (uint64_t)tot.n_none; n_no_attractor->hi = (uint64_t)(tot.n_none >> 64); }
    if (stats) {
        stats->problems = count_flat;
        stats->state_steps.lo = (uint64_t)tot.steps_ref; stats->state_steps.hi = (uint64_t)(tot.steps_ref >> 64);
        stats->executed_steps = tot.steps_exec;
        stats->kernel_ms = tot.kernel_ms;
        stats->dominant_ms = tot.dominant_ms;
        stats->dominant_executed_steps = tot.dominant_exec;
        stats->dominant_launches = tot.dominant_launches;
        stats->lower_ms = tot.lower_ms;
        stats->lower_executed_steps = tot.lower_exec;
        stats->lower_launches = tot.lower_launches;
        stats->kernel_launches = tot.launches;
        stats->host_syncs = tot.syncs;
        stats->total_ms = now_ms() - t_begin;
    }
    if (tot.limit_hits) return fail(h, BSX_ERR_STEP_LIMIT, "a trajectory reached the internal step limit without closing its cycle");
    return BSX_OK;
}
