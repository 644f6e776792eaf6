// The cube cascade of attract (DESIGN.md "deeper collapse", "levels chained on the device", "sub-blocks"): the chains of
// launches of a block or of its sub-blocks -- planned from bsx_cube_plan.h's analysis, enqueued blind, waited for once,
// evaluated from their counter blocks with bsx_merge.h's exact sums -- and the cache-mirror helpers those launches share
// with the plain passes of bsx_attract_api.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bsx_attract_host.h"

using namespace bsx;

namespace {
constexpr uint64_t kUnresCap = 1ull << 16;      // cascade: unresolved classes a level may list
constexpr uint64_t kNearBytes = 1ull << 32;     // cascade: list of the classes a level hands to the level below (segments, and two
                                                // packed lists alternated by level, per side stream: a 2^63 block of the north star
                                                // lists 7.5e7 classes of 12 bytes at its top)
}  // namespace

namespace bsx {

// LDS mirror size for the lean / pool kernels: they fill the mirror once from the journal, so it only has
// to hold what the journal holds (4 slots per state keeps probe chains short); a smaller mirror leaves
// the LDS to more workgroups.  The general kernel inserts while it runs and keeps the full size.
static int mirror_slots_for(bsx_handle h, uint32_t* slots_out) {
    // At least 2 slots per entry (a cube pass adds one representative entry per state), 4 where that still lets
    // two workgroups share a CU's LDS: at n = 64 a pool workgroup is 75.7 KiB + mirror, so a 256-slot mirror
    // already halves the occupancy (measured: 3 instead of 6 waves per SIMD, profiles/r02_pmc notes).
    const uint64_t entries = (h->cube_mirror ? 2 : 1) * h->journal_states;
    uint32_t slots = 64;
    while (slots < 2 * entries && slots < h->cache_lds_slots) slots *= 2;
    const size_t fixed = h->shmem + 32 + pool_extra_bytes(h->net.nw);
    while (slots < 4 * entries && slots < h->cache_lds_slots && fixed + (size_t)2 * slots * h->cache_stride <= 80 * 1024) slots *= 2;
    h->mirror_slots = *slots_out = std::min(slots, h->cache_lds_slots);
    if (h->knobs.debug) std::fprintf(stderr, "[bsx] mirror: %llu cycle states cached, %u slots\n", (unsigned long long)h->journal_states, *slots_out);
    return BSX_OK;
}

int lean_mirror_slots(bsx_handle h, uint32_t* slots_out, Totals* tot) {
    uint32_t ignored = 0;
    if (!slots_out) slots_out = &ignored;
    if (!h->journal_stale) return mirror_slots_for(h, slots_out);
    unsigned int known = 0;
    HIPCHK(h, hipMemcpy(&known, h->d_cc_count.p, sizeof(known), hipMemcpyDeviceToHost));
    if (tot) ++tot->syncs;
    known = std::min<unsigned int>(known, kCycleJournalCap);
    h->h_journal.resize(known);
    if (known) HIPCHK(h, hipMemcpy(h->h_journal.data(), h->d_cc_journal.p, known * sizeof(CycleRecord), hipMemcpyDeviceToHost));
    uint64_t states = 0;
    uint32_t taken = 0;
    for (const CycleRecord& r : h->h_journal) {
        if (taken >= (uint32_t)kTagAcc + kLdsAcc) break;
        if (!r.ready || r.length == 0 || r.length > kCycleCacheMaxLen) continue;
        states += r.length;
        ++taken;
    }
    h->journal_states = states;
    h->journal_stale = false;
    return mirror_slots_for(h, slots_out);
}

// The pool kernel's cache mirror as an image in HBM: rebuilt (one workgroup) only when the journal or the mirror
// size has changed; every workgroup of the passes that follow copies it instead of regenerating the cycles.
int ensure_mirror_image(bsx_handle h, AttractParams& P, size_t shmem) {
    if (!h->knobs.mirror_image) { P.mirror_image = nullptr; P.mirror_out = nullptr; return BSX_OK; }
    const size_t words = 4 + (size_t)P.cc.lds_slots * (h->cache_stride / 4);
    if (h->image_n != h->h_journal.size() || h->image_slots != P.cc.lds_slots || h->d_mirror.n < words) {
        HIPCHK(h, h->d_mirror.reserve(words));
        AttractParams B = P;
        B.count = 0;
        B.level_in = nullptr;
        B.mirror_image = nullptr;
        B.mirror_out = h->d_mirror.p;
        HIPCHK(h, launch_attract_pool((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, dim3(1), shmem, h->stream, B));
        h->image_n = h->h_journal.size();
        h->image_slots = P.cc.lds_slots;
    }
    P.mirror_image = h->d_mirror.p;
    P.mirror_out = nullptr;
    return BSX_OK;
}

}  // namespace bsx

namespace {

// Relevant digits whose influence dies out first become the lowest class-index bits (k_digit_lifetimes):
// the classes that merge after a step or two then sit in the same batch.  A heuristic for speed only.
int order_cube_digits(bsx_handle h, Cube& c) {
    const uint32_t r = (uint32_t)c.rel.size();
    if (r < 2 || r > 64 || !h->knobs.cube_order) return BSX_OK;
    uint64_t need = 0;
    for (uint32_t q = 0; q < r; ++q) need |= 1ull << c.rel[q];
    // (measured once per digit and problem space: the launch + copy + wait would otherwise sit inside every call)
    if (need & ~h->life_valid) {
        LifetimeParams L{};
        L.net = h->net;
        for (int w = 0; w < kMaxW32; ++w) { L.fixmask[w] = h->sp.fixmask[w]; L.fixval[w] = h->sp.fixval[w]; L.base[w] = c.base[w]; L.free_mask[w] = c.free_mask[w]; }
        L.n_digits = r;
        for (uint32_t q = 0; q < r; ++q) L.node[q] = h->model.any[c.rel[q]];
        HIPCHK(h, h->d_life.reserve(64));
        HIPCHK(h, hipMemsetAsync(h->d_life.p, 0, 64 * sizeof(uint32_t), h->stream));
        L.out = h->d_life.p;
        HIPCHK(h, launch_digit_lifetimes((int)h->net.nw, (int)h->net.k_mux, h->lut_mode, h->shmem, h->stream, L));
        uint32_t measured[64];
        HIPCHK(h, hipMemcpyAsync(measured, h->d_life.p, sizeof(measured), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint32_t q = 0; q < r; ++q) h->life_cache[c.rel[q]] = measured[q];
        h->life_valid |= need;
    }
    uint32_t life[64];
    for (uint32_t q = 0; q < r; ++q) life[q] = h->life_cache[c.rel[q]];
    std::vector<uint32_t> idx(r);
    for (uint32_t q = 0; q < r; ++q) idx[q] = q;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return life[x] < life[y]; });
    std::vector<uint32_t> rel(r);
    for (uint32_t q = 0; q < r; ++q) rel[q] = c.rel[idx[q]];
    c.rel = rel;
    return BSX_OK;
}

// The counter blocks of a finished chain -> h->h_ctr, and the one wait of the chain.  k_publish, the chain's last
// kernel, stores the blocks into the pinned host buffer and then the call's sequence number into h->h_flag; the host
// spins on that word (asking the stream now and then whether it has failed) instead of sleeping in
// hipStreamSynchronize behind a DMA copy, whose wake-up cost tens of microseconds per call.  BSX_SPIN_WAIT=0: the
// plain copy + wait.
int fetch_counters(bsx_handle h, uint32_t n_blocks) {
    if (!h->knobs.spin_wait) {
        HIPCHK(h, hipMemcpyAsync(h->h_ctr, h->d_ctr, sizeof(Counters) * n_blocks, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return BSX_OK;
    }
    const uint32_t seq = ++h->flag_seq ? h->flag_seq : ++h->flag_seq;       // never 0
    HIPCHK(h, launch_publish(reinterpret_cast<const uint32_t*>(h->d_ctr), reinterpret_cast<uint32_t*>(h->h_ctr),
                             (uint32_t)(sizeof(Counters) / 4 * n_blocks), const_cast<uint32_t*>(h->h_flag), seq,
                             reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(h->d_level) + kPublishTicketOffset), h->stream));
    uint32_t polls = 0;
    while (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) != seq) {
        __builtin_ia32_pause();
        if ((++polls & 0xFFFFu) == 0) {                     // every few hundred microseconds: is the stream still alive?
            const hipError_t q = hipStreamQuery(h->stream);
            if (q == hipSuccess) {                          // drained; the flag store is visible by now, or never will be
                if (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) == seq) break;
                return fail(h, BSX_ERR_HIP, "the cascade finished without publishing its counters");
            }
            if (q != hipErrorNotReady) { h->error = std::string("hipStreamQuery: ") + hipGetErrorString(q); return BSX_ERR_HIP; }
        }
    }
    return BSX_OK;
}

CascadeShape cascade_shape(bsx_handle h, const CascadeEnv& env) {
    CascadeShape sh{};
    sh.tp = h->sp.tp_origin;            // the search starts at s(T_p); class times count from there
    sh.cap_rel = env.max_t == BSX_T_INF ? BSX_T_INF : env.max_t - sh.tp;
    sh.cap_rel32 = (sh.cap_rel == BSX_T_INF || sh.cap_rel >= (kStepLimit / 4)) ? 0xFFFFFFFFu : (uint32_t)sh.cap_rel;
    sh.fast_steps = (uint32_t)std::min<uint64_t>((uint64_t)sh.cap_rel32 + 1, std::min<uint32_t>(kFastStepsMax, std::max(192u, 4 * h->fast_steps)));
    // BSX_CUBE_DEPTH caps the top level (1 = first update only)
    uint32_t max_depth = h->knobs.cube_depth ? h->knobs.cube_depth : 8;
    if (h->plan.cube_depth_cap) max_depth = std::min(max_depth, h->plan.cube_depth_cap);
    // with a warm-up the search starts at s(T_p): classes that share F^d, d <= T_p, share every state that counts,
    // so no class has to be handed down -- one pass at the best such depth
    if (sh.tp) max_depth = (uint32_t)std::min<uint64_t>(max_depth, sh.tp);
    sh.max_depth = std::max(1u, std::min(max_depth, sh.fast_steps > 1 ? sh.fast_steps - 1 : 1u));
    // (an explicit BSX_CUBE_DEPTH keeps the plain rule "fewest digits": tests force levels onto small spaces with it)
    sh.forced_depth = h->knobs.cube_depth != 0;
    return sh;
}

// ---- one cube: the whole cascade as ONE chain of launches -----------------------------------------------------------
// Level d of a block enumerates the assignments of the digits F^d still depends on (top level) or, below it, the digits
// level d adds on top of every class the level above has listed as "near a cycle" (DESIGN.md "Deeper collapse").  How many
// classes a level lists is only known on the device, so the chain is enqueued blind: the level's workgroups pack the list
// themselves (each reserves a span of it on a LevelDesc's cursor, which after the launch is the list's length), the next
// level's launch (full persistent grid) reads the length there and sizes its own work split.  Every level counts into its
// own Counters block; the host waits once -- for one chain, or for the chains of all sub-blocks of a split block -- reads
// the blocks, and only then looks at what happened: a segment overflow (-> the cube is redone from a shallower top),
// unresolved classes (attractors nobody has cached yet -> the detector runs from the listed states; if one of them sat on a
// cycle the cube is repeated with the richer cache).  Passes are accepted or discarded whole.
struct ChainLevel {
    uint32_t depth = 0, k_bits = 0, r_here = 0, unit_shift = 0;
    bool per_parent = false;        // depth 1, evaluated per listed class (LeafProgram) instead of per child
    Cube cube;
};
struct Chain {
    Cube c1;
    std::vector<uint64_t> rel_mask;
    std::vector<ChainLevel> lv;     // index 0 = top (depth `top`) .. top - 1 (depth 1); empty = not eligible
    uint32_t top = 1;
    uint32_t ctr_base = 0;          // its levels count into counter blocks ctr_base .. ctr_base + top - 1
    uint32_t desc_base = 0;         // ... and hand over through descriptors desc_base .. desc_base + top
    uint32_t index = 0;             // which chain of the batch (leaf program, events)
    dim3 top_grid;
};
enum ChainVerdict { kChainOk = 0, kChainLower = 1, kChainRepeat = 2, kChainGiveUp = 3 };

// Levels of the cascade for cube c1 from the top `top` (0: chosen by the estimate).  ch.lv stays empty if the cube does not
// qualify (more classes at the top than the 49-bit member counts, in units of one fresh class, can add up).
int plan_chain(bsx_handle h, const CascadeShape& sh, const Cube& c1, uint32_t top, Chain& ch) {
    ch.c1 = c1;
    ch.lv.clear();
    cube_levels(h->model, h->sp, c1, sh.max_depth, ch.rel_mask);
    ch.top = top ? std::min<uint32_t>(top, (uint32_t)ch.rel_mask.size()) : choose_top(h->plan, sh, ch.rel_mask, sh.max_depth);
    if (__builtin_popcountll(ch.rel_mask[ch.top - 1]) > 47) return BSX_OK;
    ch.lv.resize(ch.top);
    for (uint32_t i = 0; i < ch.top; ++i) {
        const uint32_t d = ch.top - i;
        const uint64_t here = ch.rel_mask[d - 1], digits = i == 0 ? here : here & ~ch.rel_mask[d];
        ChainLevel& l = ch.lv[i];
        l.depth = d;
        l.r_here = (uint32_t)__builtin_popcountll(here);
        l.cube = c1;
        l.cube.rel.clear();
        for (uint32_t j = 0; j < c1.a; ++j) if ((digits >> j) & 1ull) l.cube.rel.push_back(j);
        if (i == 0) if (int rc = order_cube_digits(h, l.cube)) return rc;
        plan_cube(h->model, h->sp, l.cube);
        l.k_bits = (uint32_t)l.cube.rel.size();
        l.unit_shift = c1.n_free - l.r_here;            // members of one fresh class = the unit of this level's counts
    }
    return BSX_OK;
}

// What a batch of chains shares on the device: mirror size, grid, segment size, buffers.
struct ChainBatch {
    uint32_t slots = 0;
    size_t shmem = 0;
    Launch full{};
    uint64_t seg_cap = 0;
    uint32_t n_side = 0;            // sets of list buffers in use; > 1: lower levels on that many side streams
    bool two_tops = false;          // the tops of consecutive chains alternate between the handle's stream and h->top2
};

// Mirror check + buffers for a batch of chains.  ok = false: the cached attractors do not fit the mirror (no cubes then).
int prepare_batch(bsx_handle h, const CascadeEnv& env, const std::vector<Chain*>& chains, ChainBatch& B, bool& ok) {
    ok = false;
    const uint32_t nw = h->net.nw, rec_words = nw + 3;
    // every cached attractor must be in the mirror, or a class could sit on a cycle nobody recognises
    h->cube_mirror = true;
    const int rc_m = lean_mirror_slots(h, &B.slots, &env.tot);
    h->cube_mirror = false;
    if (rc_m) return rc_m;
    uint64_t states = 0;
    for (const CycleRecord& jr : h->h_journal) states += jr.length;
    if (h->h_journal.size() > (size_t)kTagAcc + kLdsAcc || 4 * states > h->cache_lds_slots) return BSX_OK;
    B.shmem = h->shmem + (size_t)B.slots * h->cache_stride + 32 + pool_extra_bytes(nw);
    B.full = plan_persistent(h, ~0ull >> 8, B.shmem);           // the persistent grid (lower levels: size unknown here)
    // classes a level may hand down: as many as the largest top level has (a level that lists more than that is not worth its
    // launch: the cube is redone shallower), at most what 4 GiB hold; split evenly over the workgroups' segments
    uint32_t top_bits = 16, blocks = 0;
    bool lists = false;
    for (const Chain* ch : chains) {
        if (ch->lv.empty()) continue;
        top_bits = std::max(top_bits, ch->lv[0].k_bits);
        lists = lists || ch->top > 1;
        blocks += ch->top;
    }
    const uint64_t list_cap = std::min<uint64_t>(kNearBytes / (4 * (nw + 1)), 1ull << top_bits);
    B.seg_cap = h->knobs.cube_near_cap ? h->knobs.cube_near_cap : std::max<uint64_t>(64, list_cap / B.full.grid.x);     // (knob, tests: force the shallower restart)
    // the lower levels of consecutive chains run on side streams (BSX_CUBE_STREAMS=1: everything on the handle's stream)
    uint32_t n_lists = 0;
    for (const Chain* ch : chains) n_lists += (!ch->lv.empty() && ch->top > 1) ? 1u : 0u;
    B.n_side = std::min<uint32_t>(n_lists, (uint32_t)h->knobs.cube_streams);
    if (B.n_side < 2) B.n_side = lists ? 1 : 0;
    for (uint32_t sl = 0; sl < B.n_side; ++sl) {
        HIPCHK(h, h->d_near_seg[sl].reserve((size_t)B.full.grid.x * B.seg_cap * (nw + 1)));      // (state + the tag of its cycle)
        for (auto& list : h->d_near_list[sl]) HIPCHK(h, list.reserve((size_t)B.full.grid.x * B.seg_cap * (nw + 1)));
        if (B.n_side > 1 && !h->side[sl]) HIPCHK(h, hipStreamCreateWithFlags(&h->side[sl], hipStreamNonBlocking));
    }
    HIPCHK(h, h->d_unres.reserve((size_t)std::max(blocks, 1u) * kUnresCap * rec_words));
    // two tops side by side list into two slots' segments: only with side streams (one slot = one stream, everything in order)
    B.two_tops = h->knobs.cube_top_streams == 2 && B.n_side > 1;
    if (B.two_tops && !h->top2) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->top2, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_top2, hipEventDisableTiming));
    }
    ok = true;
    return BSX_OK;
}

// The launches of one chain, enqueued on the handle's stream (nothing is waited for).
// With side streams (B.n_side > 1) only the top level runs on the handle's stream (or, every other chain, on the second top
// stream: B.two_tops, so that a top's workgroups take the CUs the previous top's free); the lower levels -- short launches that
// mostly wait on memory -- follow on side stream `slot`, next to the following chains' top levels.
// slot_busy[slot] = the event behind the last chain that used the slot's list buffers.
// Level i reads the list d_near_list[slot][(i - 1) & 1] and writes d_near_list[slot][i & 1] (a level must not write into the
// list it reads); the next level's length is the cursor in descriptor desc_base + i + 1, cleared by run_batch's fill.
int enqueue_chain(bsx_handle h, const CascadeEnv& env, const CascadeShape& sh, const ChainBatch& B, Chain& ch, uint32_t slot,
                  std::vector<hipEvent_t>& slot_busy) {
    const uint32_t nw = h->net.nw, rec_words = nw + 3;
    const bool side = B.n_side > 1 && ch.top > 1;
    // (B.two_tops: the top of an odd chain on h->top2, which run_batch has put behind the fill and the first chain's image)
    hipStream_t const main_st = (B.two_tops && (ch.index & 1u)) ? h->top2 : h->stream, tail_st = side ? h->side[slot] : h->stream;
    hipEvent_t* const ev = h->ev_chain.data() + 3 * (size_t)ch.index;       // top in, top out (= the hand-over), chain done
    if (side && slot_busy[slot]) HIPCHK(h, hipStreamWaitEvent(main_st, slot_busy[slot], 0));   // (the buffers' previous user has finished)
    AttractParams Q0 = env.P;
    Q0.cc.lds_slots = B.slots;
    Q0.merge = 3;
    Q0.fast_steps = sh.fast_steps;
    Q0.per_problem = nullptr;
    Q0.offsets = nullptr;
    Q0.states = nullptr;
    Q0.log = nullptr; Q0.log_cap = 0; Q0.table = nullptr; Q0.table_mask = 0;
    for (int w = 0; w < kMaxW32; ++w) { Q0.cube_umask[w] = ch.c1.umask[w]; Q0.cube_free[w] = ch.c1.free_mask[w]; }
    if (int rc = ensure_mirror_image(h, Q0, B.shmem)) return rc;
    for (uint32_t i = 0; i < ch.top; ++i) {
        ChainLevel& l = ch.lv[i];
        AttractParams Q = Q0;
        Q.sp = l.cube.sp;
        Q.ctr = h->d_ctr + ch.ctr_base + i;
        Q.cube_shift = 0;                               // counts in units of one fresh class (2^unit_shift problems)
        Q.cube_depth = l.depth;
        Q.entry_shift = l.k_bits;
        Q.stragglers = h->d_unres.p + (size_t)(ch.ctr_base + i) * kUnresCap * rec_words;
        Q.stragglers_cap = kUnresCap * rec_words;
        Q.near = l.depth > 1 ? h->d_near_seg[slot].p : nullptr;
        Q.near_list = l.depth > 1 ? h->d_near_list[slot][i & 1].p : nullptr;
        Q.level_out = l.depth > 1 ? h->d_level + ch.desc_base + i + 1 : nullptr;
        Q.near_cap = l.depth > 1 ? B.seg_cap : 0;
        dim3 grid = B.full.grid;
        if (i == 0) {
            Q.count = 1ull << l.k_bits;
            Q.entries = nullptr;
            Q.level_in = nullptr;
            const Launch L = plan_persistent(h, Q.count, B.shmem);
            grid = L.grid;
            const uint64_t n_waves = (uint64_t)grid.x * (kPoolBlockThreads / 64);
            // passes under 2^28 classes: even fixed shares, no traffic on the cursor's one address (their classes
            // cost about the same everywhere); larger ones: one piece each, the rest from the cursor
            if (Q.count < (1ull << 28)) { Q.chunk_first = ((Q.count + n_waves - 1) / n_waves + 63) / 64 * 64; Q.chunk = 0; }
            else { Q.chunk_first = L.chunk; Q.chunk = L.chunk; }
            if (h->knobs.chunk) { Q.chunk = h->knobs.chunk; Q.chunk_first = Q.chunk; }
            ch.top_grid = grid;
            HIPCHK(h, hipEventRecord(ev[0], main_st));
        } else {
            Q.count = 0;
            Q.entries = h->d_near_list[slot][(i - 1) & 1].p;    // (packed by the level above)
            Q.level_in = h->d_level + ch.desc_base + i;
            Q.chunk = 0; Q.chunk_first = 0;
            // the lower-level build of the kernel: no pool, no rings (its LDS is the tables alone)
            Q.lower_build = (Q.mirror_image && h->knobs.cube_lower) ? 1u : 0u;
            // ... and at depth 1, where it qualifies, per parent instead of per child (BSX_CUBE_LEAF=0: per child)
            if (Q.lower_build && l.depth == 1 && h->knobs.cube_leaf) {
                LeafProgram& prog = h->h_leaf[ch.index];
                if (build_leaf_program(h->model, h->sp, l.cube.rel, prog)) {
                    HIPCHK(h, hipMemcpyAsync(h->d_leaf.p + ch.index, &prog, sizeof(LeafProgram), hipMemcpyHostToDevice, tail_st));
                    Q.leaf = h->d_leaf.p + ch.index;
                    Q.entry_shift = 0;                  // work items = the listed entries themselves
                    l.per_parent = true;
                }
            }
        }
        const size_t shmem_here = Q.lower_build ? h->shmem + (size_t)B.slots * h->cache_stride + 32 + pool_lower_extra_bytes(nw) : B.shmem;
        hipStream_t const st = i == 0 ? main_st : tail_st;
        HIPCHK(h, launch_attract_pool((int)nw, (int)h->net.k_mux, h->lut_mode, grid, shmem_here, st, Q));
        if (i == 0) HIPCHK(h, hipEventRecord(ev[1], main_st));
        if (i == 0 && side) HIPCHK(h, hipStreamWaitEvent(tail_st, ev[1], 0));     // the rest of the chain: on the side stream, behind the list
    }
    if (side) {
        HIPCHK(h, hipEventRecord(ev[2], tail_st));
        slot_busy[slot] = ev[2];
    }
    return BSX_OK;
}

// What a finished chain's counter blocks (in h->h_ctr) say: its sums into pass_* (only meaningful for kChainOk).
int evaluate_chain(bsx_handle h, const CascadeEnv& env, const CascadeShape& sh, const Chain& ch, MergedTable& pass_table,
                   u128& pass_none, u128& pass_ref, int& verdict, uint32_t& lower_to) {
    const AttractParams& P = env.P;
    Totals& tot = env.tot;
    const uint64_t max_t = env.max_t, max_len = env.max_len;
    const uint32_t nw = h->net.nw, rec_words = nw + 3;
    verdict = kChainOk;
    uint64_t n_entries = 0;
    for (uint32_t i = 0; i < ch.top; ++i) {
        const ChainLevel& l = ch.lv[i];
        const Counters& c = h->ctr_seen[ch.ctr_base + i];  // (the batch's blocks as fetched: the detector pass below reuses h_ctr's first)
        const uint64_t classes = i == 0 ? 1ull << l.k_bits : n_entries << l.k_bits;
        if (i > 0 && n_entries == 0) break;
        tot.steps_exec += c.steps_exec;
        if (h->knobs.debug)
            std::fprintf(stderr, "[bsx] cube 2^%u (%u digits free) at digit value %llu%s: depth %u%s, %u digits here (%u relevant), %llu classes, %llu near a cycle, %llu unresolved\n",
                         ch.c1.a, ch.c1.n_free, (unsigned long long)ch.c1.d_lo, ch.c1.fix_mask ? " [sub-block]" : "", l.depth, i == 0 ? " (top)" : l.per_parent ? " (per parent)" : "", l.k_bits, l.r_here,
                         (unsigned long long)classes, (unsigned long long)c.near_classes, (unsigned long long)c.straggler_classes);
        if (h->knobs.debug && c.phase_max[0])       // (BSX_DIAG build; workgroups that left before staging count in neither)
            std::fprintf(stderr, "[bsx]   diag: depth %u prologue / loop / epilogue, us summed over workgroups %.1f / %.1f / %.1f, slowest %.1f / %.1f / %.1f\n", l.depth,
                         c.phase_sum[0] / 100.0, c.phase_sum[1] / 100.0, c.phase_sum[2] / 100.0, c.phase_max[0] / 100.0, c.phase_max[1] / 100.0, c.phase_max[2] / 100.0);
        if (h->knobs.debug && l.per_parent) {
            const LeafProgram& prog = h->h_leaf[ch.index];
            std::fprintf(stderr, "[bsx] per-parent level: kb %u, %u enumerated rules, %u free rules, m %u\n", prog.kb, prog.n_enum, prog.n_free, prog.m);
        }
        if (c.straggler_overflow) { verdict = kChainGiveUp; return BSX_OK; }      // too many unresolved classes: not a space for cubes
        if (c.near_overflow) { verdict = kChainLower; lower_to = l.depth - 1; return BSX_OK; }     // start over, shallower
        // (how many classes a level lists feeds the estimate that chooses later chains' tops: near_seen below)
        n_entries = c.near_classes;
        {
            double* seen = h->plan.near_seen[i == 0 ? 0 : 1][std::min<uint32_t>(l.depth, kMaxCubeLevels)];
            seen[0] += (double)classes; seen[1] += (double)c.near_classes;
        }
        const uint32_t us = l.unit_shift;
        merge_cube_counters(pass_table, c, us, nw);
        fold_cube_level(c, us, max_t, pass_none, pass_ref);
        const uint64_t n_unres = c.straggler_classes;
        if (!n_unres) continue;
        // the detector runs from each listed state: a class that was not on a cycle yet gets its exact
        // result (all members share the rest of the trajectory); one that sits on a cycle needs that
        // attractor in the cache -- the detector has just published it -- and the pass is repeated
        if (n_unres > kUnresCap) { verdict = kChainGiveUp; return BSX_OK; }
        std::vector<uint32_t> recs(n_unres * rec_words);
        HIPCHK(h, hipMemcpy(recs.data(), h->d_unres.p + (size_t)(ch.ctr_base + i) * kUnresCap * rec_words, recs.size() * 4, hipMemcpyDeviceToHost));
        ++tot.syncs;
        std::vector<uint32_t> st(n_unres * nw);
        for (uint64_t q = 0; q < n_unres; ++q) std::copy(recs.begin() + q * rec_words, recs.begin() + q * rec_words + nw, st.begin() + q * nw);
        DevBuf<uint32_t> d_states;
        DevBuf<ProblemRec32> d_res;
        HIPCHK(h, d_states.upload(st));
        HIPCHK(h, d_res.alloc(n_unres));
        AttractParams S = P;
        S.sp = l.cube.sp;
        S.sp.tp_origin = 0;                     // the listed states are past the warm-up
        S.count = n_unres;
        S.states = d_states.p;
        S.per_problem = d_res.p;
        S.max_len = BSX_T_INF;
        S.merge = 0;
        AttractRun rs;
        if (int rc2 = launch_attract_pass(h, S, kPassGeneral, env.d_log, nullptr, rs, tot)) return rc2;
        tot.book(rs, false);
        std::vector<ProblemRec32> res(n_unres);
        HIPCHK(h, hipMemcpy(res.data(), d_res.p, n_unres * sizeof(ProblemRec32), hipMemcpyDeviceToHost));
        ++tot.syncs;
        for (uint64_t q = 0; q < n_unres; ++q)
            if (!book_unresolved_class(pass_table, pass_none, pass_ref, recs.data() + q * rec_words, res[q], nw, us, sh.tp, sh.cap_rel, max_t, max_len)) {
                verdict = kChainRepeat;                     // on a cycle: members' mu unknown
                return BSX_OK;
            }
    }
    return BSX_OK;
}

// Enqueue the chains (counter blocks and descriptors laid out one after the other), wait once, account the device time.
int run_batch(bsx_handle h, const CascadeEnv& env, const CascadeShape& sh, const ChainBatch& B, std::vector<Chain*>& chains) {
    Totals& tot = env.tot;
    uint32_t blocks = 0, n_live = 0;
    for (Chain* ch : chains) {
        if (ch->lv.empty()) continue;
        ch->ctr_base = blocks;
        ch->desc_base = blocks + n_live;
        ch->index = n_live++;
        blocks += ch->top;
    }
    if (!n_live) return BSX_OK;
    if (blocks > kMaxChainBlocks || n_live > kMaxChains) return fail(h, BSX_ERR_INVALID, "internal: too many chains in one batch");
    while (h->ev_chain.size() < 3 * (size_t)n_live) {
        hipEvent_t e = nullptr;
        HIPCHK(h, hipEventCreate(&e));
        h->ev_chain.push_back(e);
    }
    if (!h->h_leaf) HIPCHK(h, hipHostMalloc((void**)&h->h_leaf, sizeof(LeafProgram) * kMaxChains, hipHostMallocDefault));
    HIPCHK(h, h->d_leaf.reserve(kMaxChains));
    const double pt0 = now_ms();
    // (descriptors and the counter blocks are one stretch of memory: one fill)
    HIPCHK(h, hipMemsetAsync(h->d_level, 0, kLevelDescBytes + sizeof(Counters) * blocks, h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    {
        std::vector<hipEvent_t> slot_busy(std::max(1u, B.n_side), nullptr);
        uint32_t n_listing = 0;                         // chains with lower levels so far: they take the slots in turn
        for (Chain* ch : chains) {
            if (ch->lv.empty()) continue;
            const uint32_t slot = (B.n_side > 1 && ch->top > 1) ? n_listing++ % B.n_side : 0u;
            if (int rc = enqueue_chain(h, env, sh, B, *ch, slot, slot_busy)) return rc;
            // the second top stream starts behind the first chain's top-in event: the fill, and the mirror image if that chain
            // had to rebuild it (ensure_mirror_image launches on the handle's stream, in front of that event)
            if (B.two_tops && ch->index == 0) HIPCHK(h, hipStreamWaitEvent(h->top2, h->ev_chain[0], 0));
        }
        if (B.two_tops) {                               // join: tops without lower levels end on their own stream
            HIPCHK(h, hipEventRecord(h->ev_top2, h->top2));
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_top2, 0));
        }
        for (hipEvent_t e : slot_busy) if (e) HIPCHK(h, hipStreamWaitEvent(h->stream, e, 0));      // join
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    const double pt1 = now_ms();
    if (int rc = fetch_counters(h, blocks)) return rc;
    ++tot.syncs;
    const double pt2 = now_ms();
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) {      // (events precede k_publish: complete by now, but ask nicely)
        HIPCHK(h, hipEventSynchronize(h->ev1));
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    }
    tot.prof[1] += pt1 - pt0; tot.prof[2] += pt2 - pt1; tot.prof[3] += ms;
    tot.kernel_ms += ms;
    // evaluate_chain reads this copy: a detector pass started for one chain's unresolved classes counts into h_ctr's first
    // block again, which belongs to whichever chain was enqueued first -- not necessarily the one evaluated first
    h->ctr_seen.assign(h->h_ctr, h->h_ctr + blocks);
    for (Chain* ch : chains) {
        if (ch->lv.empty()) continue;
        float ms_top = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms_top, h->ev_chain[3 * ch->index], h->ev_chain[3 * ch->index + 1]));
        tot.launches += ch->top;
        tot.dominant_ms += ms_top;
        tot.dominant_exec += h->h_ctr[ch->ctr_base].steps_exec;
        ++tot.dominant_launches;
        if (h->knobs.debug) {             // the estimate against what the chain took, level by level
            std::string line;
            double sum = ms_top * 1e3;
            char buf[96];
            std::snprintf(buf, sizeof buf, "d%u %.0f", ch->top, ms_top * 1e3);
            line += buf;
            for (uint32_t i = 1; i < ch->top; ++i) {
                const Counters& c = h->h_ctr[ch->ctr_base + i];
                const double us = (c.t_last && c.t_first_not) ? (double)(c.t_last - ~c.t_first_not) / h->wall_clock_khz * 1e3 : 0.0;
                sum += us;
                std::snprintf(buf, sizeof buf, " | d%u %.0f", ch->top - i, us);
                line += buf;
            }
            std::fprintf(stderr, "[bsx] chain %u: estimated %.0f us, took %.0f us (%s)\n", ch->index, chain_cost_us(h->plan, ch->rel_mask, ch->top), sum, line.c_str());
        }
        for (uint32_t i = 1; i < ch->top; ++i) {
            const Counters& c = h->h_ctr[ch->ctr_base + i];
            if (!c.t_last || !c.t_first_not) continue;      // (an empty list: every workgroup left at once)
            tot.lower_ms += (double)(c.t_last - ~c.t_first_not) / h->wall_clock_khz;     // ticks -> ms
            tot.lower_exec += c.steps_exec;
            ++tot.lower_launches;
        }
    }
    ++tot.launches;         // (k_publish)
    return BSX_OK;
}

// A set of cubes (one block, or the sub-blocks of a split block): plan, enqueue all their chains, wait once, look -- and
// again, for those whose counters ask for it, from a shallower top / with the richer cache.  The results are kept aside until
// every cube is in; collapsed = they are in env.tot (all of them, or none).
int run_cubes(bsx_handle h, const CascadeEnv& env, const std::vector<Cube>& cubes, bool& collapsed) {
    collapsed = false;
    Totals& tot = env.tot;
    const CascadeShape sh = cascade_shape(h, env);
    std::vector<uint32_t> top(cubes.size(), 0);             // 0: the estimate chooses
    std::vector<char> done(cubes.size(), 0);
    Totals part;
    const CascadeEnv env_part{env.P, env.max_t, env.max_len, part, env.d_log};
    auto book_device_time = [&]() {                         // (device time and launches count whether or not the results are kept)
        tot.steps_exec += part.steps_exec; tot.kernel_ms += part.kernel_ms; tot.launches += part.launches;
        tot.dominant_ms += part.dominant_ms; tot.dominant_exec += part.dominant_exec; tot.dominant_launches += part.dominant_launches;
        tot.lower_ms += part.lower_ms; tot.lower_exec += part.lower_exec; tot.lower_launches += part.lower_launches;
        tot.syncs += part.syncs; tot.limit_hits += part.limit_hits;
        for (int s = 0; s < 6; ++s) tot.prof[s] += part.prof[s];
    };
    for (int attempt = 0; attempt < 32; ++attempt) {
        const double pt_plan = now_ms();
        std::vector<Chain> chains;
        std::vector<size_t> who;
        chains.reserve(cubes.size());
        for (size_t i = 0; i < cubes.size(); ++i) {
            if (done[i]) continue;
            chains.emplace_back();
            who.push_back(i);
            if (int rc = plan_chain(h, sh, cubes[i], top[i], chains.back())) return rc;
            if (chains.back().lv.empty()) { book_device_time(); return BSX_OK; }
        }
        if (chains.empty()) break;
        std::vector<Chain*> ptrs;
        uint32_t blocks = 0;
        for (Chain& ch : chains) { ptrs.push_back(&ch); blocks += ch.top; }
        if (blocks > kMaxChainBlocks || chains.size() > kMaxChains) { book_device_time(); return BSX_OK; }
        // the chains whose lower levels are estimated to take longest go first: their tails run on the side streams while the
        // others' top levels still keep the handle's stream busy, instead of being what the batch ends on
        if (ptrs.size() > 2 && h->knobs.cube_order_tails) {
            auto tail_us = [&](const Chain* ch) {
                const double top_us = kLevelOverheadUs + std::ldexp(1.0, __builtin_popcountll(ch->rel_mask[ch->top - 1])) * (ch->top + 0.3) / 4.5e5;
                return chain_cost_us(h->plan, ch->rel_mask, ch->top) - top_us;
            };
            std::vector<std::pair<double, Chain*>> keyed;
            for (Chain* ch : ptrs) keyed.emplace_back(-tail_us(ch), ch);
            std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<double, Chain*>& a, const std::pair<double, Chain*>& b) { return a.first < b.first; });
            for (size_t i = 0; i < ptrs.size(); ++i) ptrs[i] = keyed[i].second;
        }
        ChainBatch B;
        bool ok = false;
        if (int rc = prepare_batch(h, env_part, ptrs, B, ok)) return rc;
        if (!ok) { book_device_time(); return BSX_OK; }
        part.prof[0] += now_ms() - pt_plan;
        if (int rc = run_batch(h, env_part, sh, B, ptrs)) return rc;
        bool repeat = false;
        const double pt_eval = now_ms();
        for (size_t q = 0; q < chains.size(); ++q) {
            MergedTable pass_table;
            u128 pass_none = 0, pass_ref = 0;
            int verdict = kChainOk;
            uint32_t lower_to = 0;
            if (int rc = evaluate_chain(h, env_part, sh, chains[q], pass_table, pass_none, pass_ref, verdict, lower_to)) return rc;
            if (verdict == kChainOk) {
                fold_table(part.merged, pass_table);
                part.n_none += pass_none;
                part.steps_ref += pass_ref;
                done[who[q]] = 1;
            } else if (verdict == kChainLower && lower_to >= 1) {
                if (h->knobs.debug)
                    std::fprintf(stderr, "[bsx] chain %u: a list overflowed, again from depth %u\n", chains[q].index, lower_to);
                top[who[q]] = lower_to;
                // (a whole block remembers that for the rest of the problem; one sub-block of a dozen, whose lists are anybody's
                // guess while the tree is grown on guesses, does not cap the others)
                if (cubes.size() == 1) h->plan.cube_depth_cap = lower_to;
            } else if (verdict == kChainRepeat) {
                repeat = true;
            } else {                                        // not a space for cubes
                book_device_time();
                return BSX_OK;
            }
        }
        part.prof[5] += now_ms() - pt_eval;
        if (repeat) {
            unsigned int known = 0;
            HIPCHK(h, hipMemcpy(&known, h->d_cc_count.p, sizeof(known), hipMemcpyDeviceToHost));
            ++part.syncs;
            // the attractor cannot be cached: no cube for this block (else: the detector pass marked the journal stale)
            if (known <= h->h_journal.size()) { book_device_time(); return BSX_OK; }
        }
    }
    book_device_time();
    for (char d : done) if (!d) return BSX_OK;
    fold_table(tot.merged, part.merged);
    tot.n_none += part.n_none;
    tot.steps_ref += part.steps_ref;
    collapsed = true;
    return BSX_OK;
}

}  // namespace

namespace bsx {

// One aligned block: as the sub-blocks of its split tree where that pays (all their chains enqueued one after the other, one
// wait), else as one cube.  collapsed = false: the caller runs the block through the plain tiles.
int run_block(bsx_handle h, const CascadeEnv& env, uint64_t d_lo, uint32_t a_bits, bool& collapsed) {
    collapsed = false;
    const CascadeShape sh = cascade_shape(h, env);
    const bool forced = h->knobs.cube_split == 1;         // BSX_CUBE_SPLIT: "0" no sub-blocks (A/B runs, tests); "1" whatever the size
    if (h->knobs.cube_split != 0 && sh.tp == 0 && (a_bits >= kSplitMinBits || forced)) {
        // the tree grown for the first block of a size serves the others of that size too, as long as the estimate says it
        // helps there (the high digits differ, so the dependence may); a large block that it does not help gets its own
        std::vector<std::pair<uint64_t, uint64_t>>& tree = h->plan.split_cache[a_bits];
        auto estimate = [&]() {
            double est = 0;
            for (const auto& l : tree) est += cube_cost_us(h->model, h->sp, h->plan, sh, d_lo, a_bits, l.first, l.second);
            return est;
        };
        double experience = 0;                      // top-level classes whose listing the handle has seen so far
        for (uint32_t d = 0; d <= kMaxCubeLevels; ++d) experience += h->plan.near_seen[0][d][0];
        auto grow = [&]() {
            const double t0 = now_ms();
            std::vector<SplitLeaf> fresh;
            plan_split(h->model, h->sp, h->plan, sh, d_lo, a_bits, forced, fresh);
            tree.clear();
            for (const SplitLeaf& l : fresh) tree.emplace_back(l.mask, l.vals);
            h->plan.split_learned[a_bits] = experience;
            if (h->knobs.debug)
                std::fprintf(stderr, "[bsx] split tree for blocks of 2^%u: %zu leaves, planned in %.2f ms (list fractions from %.3g classes seen)\n", a_bits,
                             tree.size(), now_ms() - t0, experience);
        };
        const double pt_est = now_ms();
        const double whole = cube_cost_us(h->model, h->sp, h->plan, sh, d_lo, a_bits, 0, 0);
        bool use = false;
        // (a tree grown on guesses, or on what small blocks showed, is grown again when the handle has seen 64 times more)
        if (tree.empty() || experience > 64.0 * (h->plan.split_learned[a_bits] + 1024.0)) { grow(); use = tree.size() > 1; }
        else if (tree.size() > 1) {
            use = forced || estimate() < 0.8 * whole;
            // (a large block the tree does not help gets its own -- a few times per block size, not for every block of a sweep)
            if (!use && a_bits >= 60 && h->plan.split_regrown[a_bits] < 2) { ++h->plan.split_regrown[a_bits]; grow(); use = tree.size() > 1; }
        }
        env.tot.prof[4] += now_ms() - pt_est;
        if (use) {
            std::vector<Cube> cubes(tree.size());
            bool eligible = true;
            for (size_t i = 0; i < tree.size() && eligible; ++i) {
                build_cube(h->model, h->sp, d_lo, a_bits, cubes[i], nullptr, tree[i].first, tree[i].second);
                // (a sub-block that does not shrink at least fourfold has no cube path of its own: the block goes unsplit)
                if (!cubes[i].ok || cubes[i].rel.size() + 2 > cubes[i].n_free) eligible = false;
            }
            if (eligible) {
                if (int rc = run_cubes(h, env, cubes, collapsed)) return rc;
                if (collapsed) return BSX_OK;
            }
        }
    }
    Cube c;
    build_cube(h->model, h->sp, d_lo, a_bits, c);
    // worth it when the block shrinks at least fourfold (otherwise the tiles do as well and keep member masks)
    if (c.ok && c.rel.size() + 2 <= a_bits) return run_cubes(h, env, std::vector<Cube>{c}, collapsed);
    return BSX_OK;
}

}  // namespace bsx
