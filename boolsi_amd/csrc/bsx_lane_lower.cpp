// bsx_lane_lower.h: the arithmetic of the per-lane family's host side.  No HIP here.
#include "bsx_lane_lower.h"

#include <algorithm>
#include <array>

namespace bsx {

void lane_lower_network(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets,
                        const uint64_t* tt_words, uint64_t cache_lds_kb, int want_lut_mode, LaneNet& net, HostModel& model) {
    net = LaneNet{};
    const uint32_t nw = n_nodes <= 32 ? 1 : n_nodes <= 64 ? 2 : n_nodes <= 128 ? 4 : 8;
    uint32_t k_mux = 1;
    std::vector<uint32_t> wide;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k > (uint32_t)kMaxMuxK) wide.push_back(i);
        else k_mux = std::max(k_mux, k);
    }

    // LDS budget: masks (+pad) [+ LUT] [+ cycle-cache mirror].  The LUT stays in LDS while a workgroup
    // fits in 144 KiB: one entry per state byte if that fits, else (beyond 64 nodes) one entry per 4 state
    // bits -- a 16x smaller table for twice the lookups -- else the byte table is read through L2.
    const size_t mask_bytes = (((size_t)(1u << k_mux) * nw + 3) & ~size_t(3)) * 4;
    const size_t cache_stride = ((2 * nw + 2 + 3) & ~3u) * 4;
    uint32_t slots = 1;
    size_t cache_lds = kCycleCacheLdsBytes;
    if (cache_lds_kb) cache_lds = (size_t)cache_lds_kb * 1024;               // tuning knob
    while ((size_t)slots * 2 * cache_stride <= cache_lds) slots *= 2;
    const size_t cache_bytes = (size_t)slots * cache_stride + 16 + 16      // + header + alignment
                               + lean_acc_bytes(nw);                         // + lean kernel's per-attractor tables
    const size_t entry_bytes = (size_t)k_mux * nw * 4;
    const size_t fixed_bytes = mask_bytes + cache_bytes + 64;
    const bool nibble_fits = nw >= 4 && fixed_bytes + (size_t)nw * 8 * 16 * entry_bytes <= 144 * 1024;
    int lut_mode = 0;                                                       // kLutGlobal
    if (fixed_bytes + (size_t)nw * 4 * 256 * entry_bytes <= 144 * 1024) lut_mode = 1;      // kLutLdsByte
    else if (nibble_fits) lut_mode = 2;                                     // kLutLdsNibble
    if (want_lut_mode == 0 || (want_lut_mode == 2 && nibble_fits)) lut_mode = want_lut_mode;   // test knob: force a smaller-footprint mode
    const uint32_t chunk_bits = lut_mode == 2 ? 4 : 8, chunk_entries = 1u << chunk_bits;
    const uint32_t n_chunks = nw * 32 / chunk_bits;     // zero entries for the chunks beyond n keep the gather branch-free
    net.masks.assign((size_t)(1u << k_mux) * nw, 0);
    net.lut.assign((size_t)n_chunks * chunk_entries * k_mux * nw, 0);
    // entry = [slot j][word w]; 6-word entries in two planes: words 0..3 of every entry, then words 4..5 (net_step)
    const bool planar = k_mux * nw == 6 && lut_mode != 2;
    const size_t plane_b = (size_t)n_chunks * chunk_entries * 4;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k > (uint32_t)kMaxMuxK) continue;
        const uint64_t tt = tt_words[tt_word_offsets[i]];
        for (uint32_t idx = 0; idx < (1u << k_mux); ++idx)      // replicate over the unused high slots
            if ((tt >> (idx & ((1u << k) - 1))) & 1ull) net.masks[(size_t)idx * nw + (i >> 5)] |= 1u << (i & 31);
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t p = pred_idx[pred_offsets[i] + j];
            const uint32_t chunk = p / chunk_bits, bit = p % chunk_bits;
            for (uint32_t v = 0; v < chunk_entries; ++v)
                if ((v >> bit) & 1u) {
                    const size_t ent = (size_t)chunk * chunk_entries + v;
                    const uint32_t word = j * nw + (i >> 5);
                    const size_t at = !planar ? ent * k_mux * nw + word : (word < 4 ? ent * 4 + word : plane_b + ent * 2 + (word - 4));
                    net.lut[at] |= 1u << (i & 31);
                }
        }
    }
    for (uint32_t i : wide) {
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        net.wdesc.push_back(i); net.wdesc.push_back(k);
        net.wdesc.push_back((uint32_t)net.wpreds.size()); net.wdesc.push_back((uint32_t)net.wtt.size());
        for (uint32_t j = pred_offsets[i]; j < pred_offsets[i + 1]; ++j) net.wpreds.push_back(pred_idx[j]);
        for (uint32_t w = tt_word_offsets[i]; w < tt_word_offsets[i + 1]; ++w) {
            net.wtt.push_back((uint32_t)tt_words[w]);
            net.wtt.push_back((uint32_t)(tt_words[w] >> 32));
        }
    }
    net.nw = nw; net.k_mux = k_mux; net.n_chunks = n_chunks; net.n_wide = (uint32_t)wide.size();
    net.lut_mode = lut_mode;
    net.cache_lds_slots = slots; net.cache_stride = cache_stride; net.cache_bytes = cache_bytes;
    net.shmem = mask_bytes + (lut_mode ? net.lut.size() * 4 : 0) + 64;
    net.shmem_attract = net.shmem + cache_bytes;

    model.n_nodes = n_nodes;
    model.nw = nw;
    model.pred_offsets.assign(pred_offsets, pred_offsets + n_nodes + 1);
    model.pred_idx.clear();
    if (pred_offsets[n_nodes]) model.pred_idx.assign(pred_idx, pred_idx + pred_offsets[n_nodes]);
    model.tt0.resize(n_nodes);
    for (uint32_t i = 0; i < n_nodes; ++i) model.tt0[i] = tt_words[tt_word_offsets[i]];
}

LowerStatus lane_lower_space(uint32_t n, uint32_t nw, uint32_t w64, const uint64_t* origin_state_words, const uint32_t* any_nodes,
                             uint32_t n_any, const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var,
                             uint32_t n_fixed_var, const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var,
                             uint32_t n_pert_var, LaneSpace& out) {
    out = LaneSpace{};
    DevSpace& sp = out.sp;
    for (uint32_t w = 0; w < w64; ++w) {
        uint64_t word = origin_state_words[w];
        if (w == w64 - 1 && (n & 63)) word &= (1ull << (n & 63)) - 1;
        sp.origin[2 * w] = (uint32_t)word;
        if (2 * w + 1 < (uint32_t)kMaxW32) sp.origin[2 * w + 1] = (uint32_t)(word >> 32);
    }
    std::vector<uint32_t>& any = out.any;
    any.resize(n_any);
    bool identity = true;
    for (uint32_t j = 0; j < n_any; ++j) {
        if (any_nodes[j] >= n || (j && any_nodes[j] <= any_nodes[j - 1]))
            return {BSX_ERR_INVALID, "'any' nodes must be ascending node indices"};
        any[j] = any_nodes[j];
        identity = identity && any_nodes[j] == j;
        sp.origin[any_nodes[j] >> 5] &= ~(1u << (any_nodes[j] & 31));   // digit decides
    }
    for (uint32_t j = 0; j < n_fixed; ++j) {
        if (fixed[j].node >= n || fixed[j].value > 1) return {BSX_ERR_INVALID, "bad fixed node entry"};
        sp.fixmask[fixed[j].node >> 5] |= 1u << (fixed[j].node & 31);
        if (fixed[j].value) sp.fixval[fixed[j].node >> 5] |= 1u << (fixed[j].node & 31);
        else sp.fixval[fixed[j].node >> 5] &= ~(1u << (fixed[j].node & 31));
    }
    for (uint32_t j = 0; j < n_fixed_var; ++j) {
        if (fixed_var[j].node >= n || fixed_var[j].range > 3) return {BSX_ERR_INVALID, "bad fixed-node variation"};
        out.fv.push_back(fixed_var[j].node); out.fv.push_back(fixed_var[j].range);
    }
    uint32_t tp_origin = 0;
    for (uint32_t j = 0; j < n_sched; ++j) {
        if (sched[j].node >= n || sched[j].value > 1 || sched[j].t == 0) return {BSX_ERR_INVALID, "bad perturbation entry"};
        tp_origin = std::max(tp_origin, sched[j].t);
    }
    for (uint32_t j = 0; j < n_pert_var; ++j) {
        if (pert_var[j].node >= n || pert_var[j].range > 3 || pert_var[j].t == 0) return {BSX_ERR_INVALID, "bad perturbation variation"};
        out.pv.push_back(pert_var[j].t); out.pv.push_back(pert_var[j].node); out.pv.push_back(pert_var[j].range);
    }
    if (((uint64_t)tp_origin + 1) * nw * 8 > (1ull << 30)) return {BSX_ERR_UNSUPPORTED, "perturbation schedule too long for the dense table"};
    out.set.assign((size_t)(tp_origin + 1) * nw, 0);
    out.clr.assign((size_t)(tp_origin + 1) * nw, 0);
    for (uint32_t j = 0; j < n_sched; ++j) {
        const size_t at = (size_t)sched[j].t * nw + (sched[j].node >> 5);
        const uint32_t m = 1u << (sched[j].node & 31);
        if (sched[j].value) { out.set[at] |= m; out.clr[at] &= ~m; } else { out.clr[at] |= m; out.set[at] &= ~m; }
    }
    {
        std::vector<std::array<uint32_t, 3>> ordered;
        for (uint32_t j = 0; j < n_sched; ++j) ordered.push_back({sched[j].t, sched[j].node, sched[j].value});
        std::stable_sort(ordered.begin(), ordered.end(), [](const auto& a, const auto& b) { return a[0] < b[0]; });
        for (const auto& e : ordered) { out.sched.push_back(e[0]); out.sched.push_back(e[1]); out.sched.push_back(e[2]); }
    }
    sp.n_any = n_any;
    sp.identity_any = identity ? 1 : 0;
    // deposit plan for scattered 'any' nodes: runs of consecutive nodes inside one 32-bit state word
    sp.n_runs = 0;
    if (!identity && n_any && n_any <= 64) {
        std::vector<uint32_t> plan;
        uint32_t j = 0;
        while (j < n_any) {
            uint32_t len = 1;
            while (j + len < n_any && any[j + len] == any[j] + len && ((any[j] + len) >> 5) == (any[j] >> 5)) ++len;
            plan.push_back(j | (any[j] >> 5) << 8 | (any[j] & 31u) << 16);
            plan.push_back(len >= 32 ? 0xFFFFFFFFu : (1u << len) - 1u);
            j += len;
        }
        if (plan.size() <= 2 * kMaxDepositRuns) {
            sp.n_runs = (uint32_t)(plan.size() / 2);
            std::copy(plan.begin(), plan.end(), sp.deposit);
        }
    }
    // number of variants = product of the variation radices (batching.py:10-46), saturating at 2^64
    {
        u128 v = 1;
        auto times = [&](uint32_t range) { if (v <= UINT64_MAX) v *= (range == BSX_RANGE_MAYBE_TRUE_OR_FALSE ? 3u : 2u); };
        for (uint32_t j = 0; j < n_fixed_var; ++j) times(fixed_var[j].range);
        for (uint32_t j = 0; j < n_pert_var; ++j) times(pert_var[j].range);
        out.variant_count_saturated = v > UINT64_MAX;
        out.variant_count = out.variant_count_saturated ? UINT64_MAX : (uint64_t)v;
    }
    out.tp_max = tp_origin;
    for (uint32_t j = 0; j < n_pert_var; ++j) out.tp_max = std::max(out.tp_max, pert_var[j].t);
    sp.n_fv = n_fixed_var;
    sp.n_pv = n_pert_var;
    sp.tp_origin = tp_origin;
    return {};
}

LowerStatus range_check(const bsx_index* first, u128 count, uint32_t n_any, uint64_t variant_count, bool saturated) {
    if (!first) return {BSX_ERR_INVALID, "first index is null"};
    for (uint32_t b = n_any; b < 64 * BSX_MAX_WORDS; ++b)
        if ((first->init_digits[b >> 6] >> (b & 63)) & 1ull)
            return {BSX_ERR_INVALID, "init_digits has bits at or above n_any"};
    if (!saturated && first->variant >= variant_count)
        return {BSX_ERR_INVALID, "variant number outside the problem space"};
    if (count == 0) return {};
    // last = init_digits + (count - 1), up to 257 bits; what lies above bit n_any carries into the variant
    uint64_t sum[6] = {0, 0, 0, 0, 0, 0};
    u128 add = count - 1, carry = 0;
    for (int w = 0; w < 5; ++w) {
        carry += (w < 4 ? first->init_digits[w] : 0ull);
        carry += (uint64_t)add;
        add >>= 64;
        sum[w] = (uint64_t)carry;
        carry >>= 64;
    }
    sum[5] = (uint64_t)carry;
    u128 over = 0;                                          // (sum >> n_any); at most 129 bits, of which 128 are kept ...
    for (uint32_t b = n_any; b < 384 && b < n_any + 128; ++b)
        over |= (u128)((sum[b >> 6] >> (b & 63)) & 1ull) << (b - n_any);
    bool beyond = false;                                    // ... and anything above them is past every space
    for (uint32_t b = n_any + 128; b < 384; ++b) beyond = beyond || ((sum[b >> 6] >> (b & 63)) & 1ull);
    const u128 last_variant = (u128)first->variant + (uint64_t)over;       // (`over` itself may fill all 128 bits: no sum with it)
    if (beyond || (over >> 64) != 0 || (last_variant >> 64) != 0 || (!saturated && (uint64_t)last_variant >= variant_count))
        return {BSX_ERR_INVALID, "first + count runs past the end of the problem space"};
    return {};
}

bsx_index index_plus(const bsx_index& first, u128 delta, uint32_t n_any) {
    bsx_index r = first;
    u128 carry = 0;
    for (int w = 0; w < 4; ++w) {
        carry += r.init_digits[w];
        carry += (uint64_t)delta;
        delta >>= 64;
        r.init_digits[w] = (uint64_t)carry;
        carry >>= 64;
    }
    if (n_any < 256) {
        uint64_t over = 0;
        for (uint32_t b = n_any; b < 256 && b < n_any + 64; ++b) {
            over |= ((r.init_digits[b >> 6] >> (b & 63)) & 1ull) << (b - n_any);
            r.init_digits[b >> 6] &= ~(1ull << (b & 63));
        }
        for (uint32_t b = n_any + 64; b < 256; ++b) r.init_digits[b >> 6] &= ~(1ull << (b & 63));   // (range_check: none set)
        r.variant += over;
    }
    return r;
}

void target_words(uint32_t w64, const uint64_t* mask_words, const uint64_t* code_words, uint32_t* tmask, uint32_t* tcode) {
    for (uint32_t w = 0; w < w64; ++w) {
        tmask[2 * w] = (uint32_t)mask_words[w]; tcode[2 * w] = (uint32_t)code_words[w];
        if (2 * w + 1 < (uint32_t)kMaxW32) { tmask[2 * w + 1] = (uint32_t)(mask_words[w] >> 32); tcode[2 * w + 1] = (uint32_t)(code_words[w] >> 32); }
    }
}

void variant_fixed_nodes(const std::vector<uint32_t>& fv, uint64_t variant, uint32_t* fixmask, uint32_t* fixval) {
    uint64_t v = variant;
    for (size_t j = 0; j + 1 < fv.size(); j += 2) {
        const uint32_t node = fv[j], range = fv[j + 1];
        const uint32_t radix = range == BSX_RANGE_MAYBE_TRUE_OR_FALSE ? 3 : 2, dg = (uint32_t)(v % radix);
        v /= radix;
        int st = -1;
        if (range == BSX_RANGE_MAYBE_FALSE) st = dg ? 0 : -1;
        else if (range == BSX_RANGE_MAYBE_TRUE) st = dg ? 1 : -1;
        else if (range == BSX_RANGE_TRUE_OR_FALSE) st = dg ? 1 : 0;
        else st = dg == 0 ? -1 : (dg == 1 ? 0 : 1);
        if (st >= 0) {
            fixmask[node >> 5] |= 1u << (node & 31);
            fixval[node >> 5] = (fixval[node >> 5] & ~(1u << (node & 31))) | ((uint32_t)st << (node & 31));
        }
    }
}

void target_cube_words(const Cube& c, TargetParams& P) {
    uint32_t in_mask = 0;
    for (int w = 0; w < kMaxW32; ++w) {
        P.rep_mask[w] = P.tmask[w] & ~c.umask[w];
        P.rep_code[w] = P.tcode[w] & P.tmask[w] & ~c.umask[w];
        in_mask += (uint32_t)__builtin_popcount(P.tmask[w] & c.umask[w]);
    }
    P.count = 1ull << c.rel.size();
    P.cube = 1;
    P.cube_shift = c.a - (uint32_t)c.rel.size();
    P.cube_t0_shift = in_mask;
}

void target_cube_shares(uint64_t n_waves, uint32_t chunk, TargetParams& P) {
    // even fixed shares, no cursor traffic (P.count <= 2^64 / ... classes of about equal cost)
    if (P.count < (1ull << 28)) { P.chunk_first = ((P.count + n_waves - 1) / n_waves + 63) / 64 * 64; P.chunk = 0; }
    else { P.chunk_first = 0; P.chunk = chunk; }
}

uint64_t target_listing_piece(uint64_t left, uint64_t hits_wanted) {
    return std::min<uint64_t>(left, std::max<uint64_t>(1ull << kCubeMinBits, 4 * hits_wanted));
}

bool target_cubes_ok(const DevSpace& sp, bool variant_count_saturated) {
    return sp.n_any >= kCubeMinBits && sp.n_any <= 64 && (sp.identity_any || sp.n_runs) && !sp.n_pv && !sp.tp_origin &&
           !variant_count_saturated;
}

CountPiece count_piece(const bsx_index& first, uint64_t done, uint64_t count, uint32_t n_any, bool cubes_ok) {
    CountPiece p;
    if (!cubes_ok) {
        p.n = std::min<uint64_t>(count - done, 1ull << 32);
        return p;
    }
    // (variant, digit value) of problem first + done; the segment of the range inside this variant
    const u128 space = (u128)1 << n_any;
    const u128 pos = (u128)first.init_digits[0] + done;
    p.variant = first.variant + (uint64_t)(pos >> n_any);
    const u128 digit = pos & (space - 1);
    const uint64_t seg = (uint64_t)std::min<u128>(count - done, space - digit);
    const u128 unit = (u128)1 << kCubeMinBits;
    const u128 seg_end = digit + seg;
    const u128 at = (digit + unit - 1) / unit * unit;       // the body: the whole units of the segment
    const u128 body_end = seg_end / unit * unit;
    if (at >= body_end) { p.n = seg; return p; }            // no body (left): the tail, or a segment that holds no unit
    if (at > digit) { p.n = (uint64_t)(at - digit); return p; }     // the head
    uint32_t a_bits = std::min<uint32_t>(kCubeMaxBits, n_any);
    while (a_bits > kCubeMinBits && ((at & (((u128)1 << a_bits) - 1)) != 0 || at + ((u128)1 << a_bits) > body_end)) --a_bits;
    p.block = true;
    p.digit = (uint64_t)at;
    p.a_bits = a_bits;
    p.n = 1ull << a_bits;
    return p;
}

uint64_t lane_sim_blocks(uint64_t count, uint32_t compute_units) {
    return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)compute_units * 4, (count + kBlock - 1) / kBlock));
}

// K <= 3 and n <= 128: second-generation kernel (8-byte rows, constants in registers); BSX_SLICED=1 keeps the first
bool sliced_gen2(uint32_t n_nodes, uint32_t k_mux, int knob_sliced) {
    return k_mux <= 3 && sliced_rows(n_nodes) <= 128 && knob_sliced != 1;
}

bool sliced_ok(uint32_t n_nodes, const DevNet& net, const DevSpace& sp, int knob_sliced, bool want_trajectories, bool want_final,
               bool want_digests, uint64_t max_t, uint64_t count) {
    return knob_sliced != 0 && (want_final || want_digests) && !want_trajectories &&
           (!want_digests || sliced_gen2(n_nodes, net.k_mux, knob_sliced)) &&      // digests: gen 2 keeps them per row in registers
           !sp.n_fv && !sp.n_pv && !net.n_wide && max_t >= 64 && max_t < kStepLimit &&
           count >= 2048 && (size_t)sliced_rows(n_nodes) * 136 * 4 <= 160 * 1024;
}

SlicedShape sliced_shape(uint32_t n_nodes, uint32_t k_mux, int knob_sliced, uint64_t count, uint32_t compute_units) {
    SlicedShape s;
    s.rows = sliced_rows(n_nodes);
    s.gen2 = sliced_gen2(n_nodes, k_mux, knob_sliced);
    // (first generation: descriptors, buffer 0, buffer 1; buffer 1, the last, is also the scratch of the initial
    // transposition, 32 x 64 words, which 16 rows do not hold)
    s.shmem = s.gen2 ? (size_t)s.rows * 1024 + (4096 + 64) * 4 : ((size_t)s.rows * (8 + 64) + (size_t)std::max(s.rows, 32u) * 64) * 4;
    s.groups = s.gen2 ? (count + 4095) / 4096 : (count + 2047) / 2048;
    s.per_cu = s.gen2 ? 1 : std::max<size_t>(1, (160 * 1024) / s.shmem);
    s.blocks = std::max<uint64_t>(1, std::min<uint64_t>(s.groups, (uint64_t)compute_units * s.per_cu));
    return s;
}

void sliced_row_desc(const HostModel& m, const DevSpace& sp, uint32_t k_mux, std::vector<uint32_t>& desc) {
    const uint32_t n = m.n_nodes;
    desc.assign((size_t)sliced_rows(n) * 8, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = m.pred_offsets[i + 1] - m.pred_offsets[i];
        for (uint32_t j = 0; j < k; ++j) desc[(size_t)i * 8 + j] = m.pred_idx[m.pred_offsets[i] + j];
        uint64_t tt = 0;
        const bool fixed = (sp.fixmask[i >> 5] >> (i & 31)) & 1u;
        if (fixed) tt = ((sp.fixval[i >> 5] >> (i & 31)) & 1u) ? ~0ull : 0ull;     // model.py:45-47
        else
            for (uint32_t idx = 0; idx < (1u << k_mux); ++idx)
                if ((m.tt0[i] >> (idx & ((1u << k) - 1))) & 1ull) tt |= 1ull << idx;
        desc[(size_t)i * 8 + 6] = (uint32_t)tt;
        desc[(size_t)i * 8 + 7] = (uint32_t)(tt >> 32);
    }
}

}  // namespace bsx
