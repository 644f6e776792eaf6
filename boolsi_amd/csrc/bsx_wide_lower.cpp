// bsx_wide_lower.h: the arithmetic of the wide-state family's host side.  No HIP here.
#include "bsx_wide_lower.h"

#include <algorithm>
#include <array>

namespace bsx {

LowerStatus check_network_arrays(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets) {
    for (uint32_t i = 0; i < n_nodes; ++i) {
        if (pred_offsets[i + 1] < pred_offsets[i]) return {BSX_ERR_INVALID, "pred_offsets not monotone"};
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k > BSX_MAX_PREDECESSORS) return {BSX_ERR_UNSUPPORTED, "node with more than BSX_MAX_PREDECESSORS predecessors"};
        if (k && !pred_idx) return {BSX_ERR_INVALID, "pred_idx is null"};
        for (uint32_t j = pred_offsets[i]; j < pred_offsets[i + 1]; ++j) {
            if (pred_idx[j] >= n_nodes) return {BSX_ERR_INVALID, "predecessor index out of range"};
            if (j > pred_offsets[i] && pred_idx[j] <= pred_idx[j - 1])
                return {BSX_ERR_INVALID, "predecessors must be strictly ascending"};
        }
        const uint32_t need_words = k <= 6 ? 1u : (1u << (k - 6));
        if (tt_word_offsets[i + 1] - tt_word_offsets[i] != need_words)
            return {BSX_ERR_INVALID, "truth table of a node must have ceil(2^k / 64) words"};
    }
    return {};
}

void wide_lower_network(uint32_t n_nodes, const uint32_t* pred_offsets, const uint32_t* pred_idx, const uint32_t* tt_word_offsets,
                        const uint64_t* tt_words, WideNet& net) {
    net.n = n_nodes;
    net.rows = (n_nodes + 63) & ~63u;
    net.w64 = (n_nodes + 63) / 64;
    net.pred_offsets.assign(pred_offsets, pred_offsets + n_nodes + 1);
    net.pred_idx.clear();
    if (pred_offsets[n_nodes]) net.pred_idx.assign(pred_idx, pred_idx + pred_offsets[n_nodes]);
    net.tt_offsets.assign(tt_word_offsets, tt_word_offsets + n_nodes + 1);
    net.tt.assign(tt_words, tt_words + tt_word_offsets[n_nodes]);
    net.wdesc.clear(); net.wpreds.clear(); net.wtt.clear();
    net.K = 1;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = pred_offsets[i + 1] - pred_offsets[i];
        if (k <= 6) { net.K = std::max(net.K, k); continue; }
        net.wdesc.push_back(k); net.wdesc.push_back((uint32_t)net.wpreds.size()); net.wdesc.push_back((uint32_t)net.wtt.size());
        for (uint32_t j = pred_offsets[i]; j < pred_offsets[i + 1]; ++j) net.wpreds.push_back(pred_idx[j]);
        for (uint32_t w = tt_word_offsets[i]; w < tt_word_offsets[i + 1]; ++w) {
            net.wtt.push_back((uint32_t)tt_words[w]);
            net.wtt.push_back((uint32_t)(tt_words[w] >> 32));
        }
    }
}

LowerStatus wide_lower_space(const WideNet& net, const uint64_t* origin_state_words, const uint32_t* any_nodes, uint32_t n_any,
                             const bsx_fixed* fixed, uint32_t n_fixed, const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                             const bsx_pert* sched, uint32_t n_sched, const bsx_pert_var* pert_var, uint32_t n_pert_var, WideSpace& sp) {
    const uint32_t n = net.n;
    sp = WideSpace{};
    for (uint32_t i = 0; i < n; ++i)
        if ((origin_state_words[i >> 6] >> (i & 63)) & 1ull) sp.origin[i >> 5] |= 1u << (i & 31);
    sp.any.resize(n_any);
    for (uint32_t j = 0; j < n_any; ++j) {
        if (any_nodes[j] >= n || (j && any_nodes[j] <= any_nodes[j - 1]))
            return {BSX_ERR_INVALID, "'any' nodes must be ascending node indices"};
        sp.any[j] = any_nodes[j];
        sp.origin[any_nodes[j] >> 5] &= ~(1u << (any_nodes[j] & 31));
    }
    std::vector<int> fixed_val(n, -1), slot_of(n, -1);
    for (uint32_t j = 0; j < n_fixed; ++j) {
        if (fixed[j].node >= n || fixed[j].value > 1) return {BSX_ERR_INVALID, "bad fixed node entry"};
        fixed_val[fixed[j].node] = (int)fixed[j].value;
        sp.fixmask[fixed[j].node >> 5] |= 1u << (fixed[j].node & 31);
    }
    for (uint32_t j = 0; j < n_fixed_var; ++j) {
        const uint32_t node = fixed_var[j].node;
        if (node >= n || fixed_var[j].range > 3) return {BSX_ERR_INVALID, "bad fixed-node variation"};
        if (slot_of[node] < 0) slot_of[node] = (int)sp.n_fslots++;
        sp.fv.push_back(node); sp.fv.push_back(fixed_var[j].range); sp.fv.push_back((uint32_t)slot_of[node]);
    }
    std::vector<std::array<uint32_t, 3>> ordered;
    for (uint32_t j = 0; j < n_sched; ++j) {
        if (sched[j].node >= n || sched[j].value > 1 || sched[j].t == 0) return {BSX_ERR_INVALID, "bad perturbation entry"};
        sp.tp_origin = std::max(sp.tp_origin, sched[j].t);
        ordered.push_back({sched[j].t, sched[j].node, sched[j].value});
    }
    std::stable_sort(ordered.begin(), ordered.end(), [](const auto& a, const auto& b) { return a[0] < b[0]; });
    for (const auto& e : ordered) { sp.sched.push_back(e[0]); sp.sched.push_back(e[1]); sp.sched.push_back(e[2]); }
    sp.tp_max = sp.tp_origin;
    for (uint32_t j = 0; j < n_pert_var; ++j) {
        if (pert_var[j].node >= n || pert_var[j].range > 3 || pert_var[j].t == 0) return {BSX_ERR_INVALID, "bad perturbation variation"};
        sp.pv.push_back(pert_var[j].t); sp.pv.push_back(pert_var[j].node); sp.pv.push_back(pert_var[j].range);
        sp.tp_max = std::max(sp.tp_max, pert_var[j].t);
    }
    // row descriptors: K-input mux (tables replicated over unused inputs; origin fixed nodes are constant rules),
    // fixed-variation slot, index of the per-trajectory path for nodes with more than 6 predecessors
    sp.desc.assign((size_t)net.rows * kWideDescWords, 0);
    uint32_t wide_at = 0;
    for (uint32_t i = 0; i < net.rows; ++i) {
        uint32_t* d = &sp.desc[(size_t)i * kWideDescWords];
        d[5] = d[6] = kWideNone;
        if (i >= n) continue;                   // padding rows: constant 0
        d[5] = slot_of[i] >= 0 ? (uint32_t)slot_of[i] : kWideNone;
        const uint32_t k = net.pred_offsets[i + 1] - net.pred_offsets[i];
        if (k > 6) {
            const uint32_t at = wide_at++;
            if (fixed_val[i] < 0) { d[6] = at; continue; }
        }
        uint64_t bits = 0;
        if (fixed_val[i] >= 0) {
            bits = fixed_val[i] ? ~0ull : 0ull;
        } else {
            const uint64_t t = net.tt[net.tt_offsets[i]];
            for (uint32_t idx = 0; idx < 64; ++idx)
                if ((t >> (idx & ((1u << k) - 1))) & 1ull) bits |= 1ull << idx;
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t p = net.pred_idx[net.pred_offsets[i] + j];
                d[j >> 1] |= p << (16 * (j & 1));
            }
        }
        d[3] = (uint32_t)bits; d[4] = (uint32_t)(bits >> 32);
    }
    sp.n_any = n_any; sp.n_fv = n_fixed_var; sp.n_pv = n_pert_var; sp.n_sched = n_sched;
    // columns per group: the largest power of two <= 64 whose four matrices and tables fit the LDS
    for (uint32_t L = 64; L >= 4; L >>= 1) {
        const size_t bytes = (size_t)wide_lds_words(net.rows, L, sp.n_fslots, sp.n_pv) * 4;
        if (bytes <= 159 * 1024) { sp.L = L; sp.shmem = bytes; break; }
    }
    if (!sp.L) return {BSX_ERR_UNSUPPORTED, "wide network: state matrices do not fit the LDS"};
    // number of variants = product of the variation radices, saturating at 2^64
    unsigned __int128 v = 1;
    auto times = [&](uint32_t range) { if (v <= UINT64_MAX) v *= (range == BSX_RANGE_MAYBE_TRUE_OR_FALSE ? 3u : 2u); };
    for (uint32_t j = 0; j < n_fixed_var; ++j) times(fixed_var[j].range);
    for (uint32_t j = 0; j < n_pert_var; ++j) times(pert_var[j].range);
    sp.variant_count_saturated = v > UINT64_MAX;
    sp.variant_count = sp.variant_count_saturated ? UINT64_MAX : (uint64_t)v;
    return {};
}

void wide_target_words(uint32_t n_nodes, const uint64_t* mask_words, const uint64_t* code_words, uint32_t* tmask, uint32_t* tcode) {
    std::fill(tmask, tmask + kWideMaxW32, 0u);
    std::fill(tcode, tcode + kWideMaxW32, 0u);
    for (uint32_t i = 0; i < n_nodes; ++i) {
        if ((mask_words[i >> 6] >> (i & 63)) & 1ull) tmask[i >> 5] |= 1u << (i & 31);
        if ((code_words[i >> 6] >> (i & 63)) & 1ull) tcode[i >> 5] |= 1u << (i & 31);
    }
}

LowerStatus wide_split_flat(bsx_u128 first_flat, uint32_t n_any, bsx_index& first) {
    using u128 = unsigned __int128;
    first = bsx_index{};
    if (n_any >= 128) {
        first.init_digits[0] = first_flat.lo; first.init_digits[1] = first_flat.hi;
        return {};
    }
    const u128 flat = ((u128)first_flat.hi << 64) | first_flat.lo;
    const u128 digits = n_any ? (flat & ((((u128)1) << n_any) - 1)) : 0;
    const u128 variant = flat >> n_any;
    if (variant >> 64) return {BSX_ERR_INVALID, "first lies beyond the problem space"};
    first.init_digits[0] = (uint64_t)digits; first.init_digits[1] = (uint64_t)(digits >> 64);
    first.variant = (uint64_t)variant;
    return {};
}

uint64_t wide_grid_blocks(uint64_t count, uint32_t L, size_t shmem, uint32_t compute_units) {
    const uint32_t G = 32 * L;
    const uint64_t groups = (count + G - 1) / G;
    const uint32_t per_cu = std::max<uint32_t>(1, (uint32_t)((160 * 1024) / shmem));
    return std::max<uint64_t>(1, std::min<uint64_t>(groups, (uint64_t)compute_units * per_cu));
}

}  // namespace bsx
