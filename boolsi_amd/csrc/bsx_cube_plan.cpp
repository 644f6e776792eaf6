// Cube analysis and planning: see bsx_cube_plan.h.  Built by the host compiler alone (no HIP).
#include "bsx_cube_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace bsx {

// ---- cube collapse: which of the `a` lowest initial-state digits can the FIRST update of the
// block starting at digit value d_lo depend on?  A node's rule, restricted to the block's fixed bits, depends
// on a free predecessor iff flipping it changes the output for some assignment of the rule's other free
// inputs; a digit is relevant iff its node is such a predecessor of some node (fixed nodes have constant
// rules, model.py:45-47).  f(s) is then a function of the relevant digits alone -- exactly, not heuristically.
void build_cube(const HostModel& m, const DevSpace& sp, uint64_t d_lo, uint32_t a, Cube& c, const uint32_t* fixmask, uint64_t fix_mask, uint64_t fix_vals) {
    if (!fixmask) fixmask = sp.fixmask;      // (target passes: the fixed nodes of the block's fixed-node variant)
    const uint32_t n = m.n_nodes, nw = m.nw;
    c.d_lo = d_lo; c.a = a; c.rel.clear(); c.ok = false;
    const uint64_t low = a >= 64 ? ~0ull : (1ull << a) - 1ull;
    c.fix_mask = fix_mask & low; c.fix_vals = fix_vals & c.fix_mask;
    c.free_digits = low & ~c.fix_mask;
    c.n_free = (uint32_t)__builtin_popcountll(c.free_digits);
    uint32_t base[kMaxW32];     // origin bits + the block's fixed digits
    for (int w = 0; w < kMaxW32; ++w) { base[w] = sp.origin[w]; c.umask[w] = 0; c.free_mask[w] = 0; }
    std::vector<char> is_free(n, 0), relevant(n, 0);
    for (uint32_t j = 0; j < sp.n_any; ++j) {
        const uint32_t node = m.any[j];
        if (j < a && ((c.free_digits >> j) & 1ull)) { is_free[node] = 1; c.free_mask[node >> 5] |= 1u << (node & 31); }
        else if (j < a ? ((c.fix_vals >> j) & 1ull) != 0 : ((d_lo >> j) & 1ull) != 0) base[node >> 5] |= 1u << (node & 31);
    }
    for (uint32_t i = 0; i < n; ++i) {
        if ((fixmask[i >> 5] >> (i & 31)) & 1u) continue;
        const uint32_t k = m.pred_offsets[i + 1] - m.pred_offsets[i];
        const uint32_t* preds = m.pred_idx.data() + m.pred_offsets[i];
        if (k > (uint32_t)kMaxMuxK) {                    // wide rule: every free input counts (conservative)
            for (uint32_t j = 0; j < k; ++j) if (is_free[preds[j]]) relevant[preds[j]] = 1;
            continue;
        }
        const uint64_t tt = m.tt0[i];
        uint32_t free_slots = 0, fixed_idx = 0;
        for (uint32_t j = 0; j < k; ++j) {
            if (is_free[preds[j]]) free_slots |= 1u << j;
            else if ((base[preds[j] >> 5] >> (preds[j] & 31)) & 1u) fixed_idx |= 1u << j;
        }
        for (uint32_t j = 0; j < k; ++j) {
            if (!((free_slots >> j) & 1u) || relevant[preds[j]]) continue;
            const uint32_t others = free_slots & ~(1u << j);
            uint32_t x = 0;
            do {                                        // all assignments of the other free inputs
                const uint32_t idx = fixed_idx | x;
                if (((tt >> idx) ^ (tt >> (idx | (1u << j)))) & 1ull) { relevant[preds[j]] = 1; break; }
                x = (x - others) & others;
            } while (x);
        }
    }
    for (uint32_t j = 0; j < a; ++j) {
        if (!((c.free_digits >> j) & 1ull)) continue;
        const uint32_t node = m.any[j];
        if (relevant[node]) c.rel.push_back(j);
        else c.umask[node >> 5] |= 1u << (node & 31);
    }
    for (uint32_t w = 0; w < (uint32_t)kMaxW32; ++w) c.base[w] = w < nw ? base[w] : 0u;
    c.ok = c.rel.size() <= kMaxDepositRuns;
}

// Enumeration space of the cube: class-index bit q -> the node of c.rel[q] (one deposit run per relevant
// digit, in the order c.rel lists them), everything else fixed.
void plan_cube(const HostModel& m, const DevSpace& space, Cube& c) {
    DevSpace sp = space;
    for (uint32_t w = 0; w < (uint32_t)kMaxW32; ++w) sp.origin[w] = c.base[w];
    sp.n_any = (uint32_t)c.rel.size();
    sp.identity_any = 0;
    for (int w = 0; w < 4; ++w) sp.first_digits[w] = 0;
    sp.first_variant = 0;
    sp.n_runs = (uint32_t)c.rel.size();
    for (uint32_t q = 0; q < c.rel.size(); ++q) {
        const uint32_t node = m.any[c.rel[q]];
        sp.deposit[2 * q] = q | (node >> 5) << 8 | (node & 31u) << 16;
        sp.deposit[2 * q + 1] = 1u;
    }
    c.sp = sp;
}


// Deeper collapse: the digits of the block that F^d(x) still depends on, d = 1 .. max_depth, as masks over the
// digit index (out[d - 1]; a <= 63).  Constant propagation over the block: a node's value after s updates is
// 0, 1 or "varies" with the set of free digits it may depend on; a rule is restricted to the inputs that are
// constant over the block and counts a varying input only if the restricted truth table is sensitive to it.
// An over-approximation (never misses a dependence), and out[0] is build_cube's set.  out[d] is a subset of
// out[d - 1]: the members of a depth-d class share F^d(x) and everything after it.
void cube_levels(const HostModel& m, const DevSpace& sp, const Cube& c, uint32_t max_depth, std::vector<uint64_t>& out) {
    const uint32_t n = m.n_nodes;
    const uint32_t* fixmask = sp.fixmask;
    std::vector<uint8_t> val(n), nval(n);       // 0 / 1 / 2 = varies
    std::vector<uint64_t> dep(n, 0), ndep(n, 0);
    for (uint32_t i = 0; i < n; ++i) val[i] = (c.base[i >> 5] >> (i & 31)) & 1u;
    for (uint32_t j = 0; j < c.a; ++j)
        if ((c.free_digits >> j) & 1ull) { const uint32_t node = m.any[j]; val[node] = 2; dep[node] = 1ull << j; }
    out.clear();
    for (uint32_t d = 1; d <= max_depth; ++d) {
        uint64_t all = 0;
        for (uint32_t i = 0; i < n; ++i) {
            ndep[i] = 0;
            if ((fixmask[i >> 5] >> (i & 31)) & 1u) { nval[i] = (sp.fixval[i >> 5] >> (i & 31)) & 1u; continue; }
            const uint32_t k = m.pred_offsets[i + 1] - m.pred_offsets[i];
            const uint32_t* preds = m.pred_idx.data() + m.pred_offsets[i];
            if (k > (uint32_t)kMaxMuxK) {                // wide rule: varies with whatever its inputs vary with (conservative)
                nval[i] = 2;
                for (uint32_t j = 0; j < k; ++j) ndep[i] |= dep[preds[j]];
                continue;
            }
            const uint64_t tt = m.tt0[i];
            uint32_t var_slots = 0, fixed_idx = 0;
            for (uint32_t j = 0; j < k; ++j) {
                if (val[preds[j]] == 2) var_slots |= 1u << j;
                else if (val[preds[j]]) fixed_idx |= 1u << j;
            }
            uint32_t seen = 0, sens = 0, x = 0;
            do {                                        // all assignments of the varying inputs
                const uint32_t idx = fixed_idx | x;
                seen |= 1u << ((tt >> idx) & 1ull);
                for (uint32_t j = 0; j < k; ++j)
                    if (((var_slots >> j) & 1u) && (((tt >> idx) ^ (tt >> (idx ^ (1u << j)))) & 1ull)) sens |= 1u << j;
                x = (x - var_slots) & var_slots;
            } while (x);
            if (seen != 3u) { nval[i] = seen >> 1; continue; }
            nval[i] = 2;
            for (uint32_t j = 0; j < k; ++j) if ((sens >> j) & 1u) ndep[i] |= dep[preds[j]];
        }
        // the origin's perturbation schedule overrides the rules at time d (model.py:68-71): constants for every member
        for (size_t e = 0; e + 2 < m.sched.size(); e += 3)
            if (m.sched[e] == d) { nval[m.sched[e + 1]] = (uint8_t)m.sched[e + 2]; ndep[m.sched[e + 1]] = 0; }
        all = 0;
        for (uint32_t i = 0; i < n; ++i) all |= ndep[i];
        out.push_back(all);
        val.swap(nval);
        dep.swap(ndep);
    }
}

// The depth-1 level's program (bsx_device.h: LeafProgram) for the block `c1` and the digits `added` that level adds: which
// nodes' rules read an added digit, with which inputs.  False if the level does not qualify (too many digits or dependent
// nodes, a dependent rule with more than kLeafMaxK inputs): the per-child pass takes it then.
bool build_leaf_program(const HostModel& m, const DevSpace& sp, const std::vector<uint32_t>& added_digits, LeafProgram& L) {
    const uint32_t n = m.n_nodes;
    if (added_digits.empty() || added_digits.size() > kLeafMaxBits) return false;
    static_assert(kLeafMaxBits <= 16 && kLeafMaxDeps <= 64, "digit_node[], the free rules' 64-bit masks (bsx_leaf.h)");
    std::memset(&L, 0, sizeof(L));
    L.kb = (uint32_t)added_digits.size();
    std::vector<int> digit_of(n, -1);                                   // node -> position in added_digits
    for (uint32_t q = 0; q < L.kb; ++q) {
        const uint32_t node = m.any[added_digits[q]];
        digit_of[node] = (int)q;
        L.added[node >> 5] |= 1u << (node & 31);
    }
    // the dependent rules, and which digits are entangled: read by a rule that reads another added digit as well (from the
    // wiring alone, as `dependent` is)
    std::vector<uint32_t> dep_nodes, dep_digits;                        // per dependent rule: node, the added digits it reads (mask)
    uint32_t entangled = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t reads = 0;
        const uint32_t k = m.pred_offsets[i + 1] - m.pred_offsets[i];
        const uint32_t* preds = m.pred_idx.data() + m.pred_offsets[i];
        if (!((sp.fixmask[i >> 5] >> (i & 31)) & 1u))                 // (a fixed node's rule is a constant, model.py:45-47)
            for (uint32_t j = 0; j < k; ++j) if (digit_of[preds[j]] >= 0) reads |= 1u << digit_of[preds[j]];
        if (!reads) { L.indep[i >> 5] |= 1u << (i & 31); continue; }
        if (k > kLeafMaxK || dep_nodes.size() == kLeafMaxDeps) return false;
        dep_nodes.push_back(i);
        dep_digits.push_back(reads);
        if (reads & (reads - 1u)) entangled |= reads;
    }
    // the program's numbering: entangled digits first, each class in the order of added_digits
    std::vector<uint32_t> number(L.kb, 0);
    L.m = (uint32_t)__builtin_popcount(entangled);
    for (uint32_t q = 0, e = 0, f = L.m; q < L.kb; ++q) {
        number[q] = ((entangled >> q) & 1u) ? e++ : f++;
        L.digit_node[number[q]] = (uint16_t)m.any[added_digits[q]];
    }
    // enumerated rules in node order, then the free rules by digit (node order within a digit)
    std::vector<std::pair<uint32_t, uint32_t>> order;                   // (0 or 1 + the free digit's number, rule)
    for (uint32_t r = 0; r < dep_nodes.size(); ++r)
        order.emplace_back((dep_digits[r] & entangled) ? 0u : 1u + number[(uint32_t)__builtin_ctz(dep_digits[r])], r);
    std::sort(order.begin(), order.end());
    for (const auto& o : order) {
        const uint32_t i = dep_nodes[o.second];
        const uint32_t k = m.pred_offsets[i + 1] - m.pred_offsets[i];
        const uint32_t* preds = m.pred_idx.data() + m.pred_offsets[i];
        LeafDep& d = L.dep[L.n_dep++];
        d.node = (uint16_t)i;
        d.k = (uint16_t)(o.first ? k | ((o.first - 1u) << 8) : k);
        (o.first ? L.n_free : L.n_enum)++;
        for (uint32_t j = 0; j < k; ++j)
            d.in[j] = digit_of[preds[j]] >= 0 ? (uint16_t)(0x8000u | number[(uint32_t)digit_of[preds[j]]]) : (uint16_t)preds[j];
        d.tt = (uint32_t)(m.tt0[i] & ((1ull << (1u << k)) - 1ull));   // inputs beyond k: their selectors are 0 (the low half)
    }
    return true;
}

// Estimated device time of a cascade in microseconds, so that a block is not pushed through levels that cost more than they
// save and so that sub-blocks can be compared (plan_split).  rel_mask[d - 1] = digits F^d depends on.  The top level `top`
// enumerates 2^r_top classes at (top + 0.3) updates each; of the classes of level d + 1 the fraction f(d + 1) is listed, and
// each listed class has 2^(r_d - r_(d + 1)) children at level d.  Rates as measured on the north star (profiles/r03_levels.md):
// 4.5e11 class updates per second in the per-child passes, 1.5e12 children per second in the depth-1 level per parent,
// kLevelOverheadUs for every level that has anything to do.  (A least-squares fit over 107 per-parent levels says 95 us +
// 1.75e12 children/s; pricing that latency in made the trees worse -- more, smaller chains -- on every block size tried.)  f is what this handle has seen at that depth so far
// (PlanState::near_seen; the top level and the levels below it apart: children of listed classes are far more often near a
// cycle than classes at large), else a guess that grows with the depth.
double near_fraction(const PlanState& ps, uint32_t d, bool is_top) {
    d = std::min<uint32_t>(d, kMaxCubeLevels);
    const auto& seen = ps.near_seen[is_top ? 0 : 1];
    if (seen[d][0] >= 1024.0) return std::min(1.0, seen[d][1] / seen[d][0]);
    // nothing seen at this depth: the nearest depth that has been, a factor of two per level (deeper = nearer to the cycles)
    for (uint32_t off = 1; off <= kMaxCubeLevels; ++off) {
        if (d > off && seen[d - off][0] >= 1024.0) return std::min(1.0, seen[d - off][1] / seen[d - off][0] * std::ldexp(1.0, (int)off));
        if (d + off <= kMaxCubeLevels && seen[d + off][0] >= 1024.0) return std::min(1.0, seen[d + off][1] / seen[d + off][0] * std::ldexp(1.0, -(int)off));
    }
    return is_top ? std::min(1.0, 0.0025 * std::ldexp(1.0, (int)d - 2)) : 0.1;
}

double chain_cost_us(const PlanState& ps, const std::vector<uint64_t>& rel_mask, uint32_t top) {
    int r_above = __builtin_popcountll(rel_mask[top - 1]);
    double n = std::ldexp(1.0, r_above);
    double cost = kLevelOverheadUs + n * (top + 0.3) / 4.5e5;
    for (uint32_t d = top - 1; d >= 1; --d) {
        const double parents = n * near_fraction(ps, d + 1, d + 1 == top);
        if (parents < 1.0) { cost += 5.0 * d; break; }                  // (launches that find an empty list)
        const int r_d = __builtin_popcountll(rel_mask[d - 1]), kb = r_d - r_above;
        n = parents * std::ldexp(1.0, kb);
        cost += kLevelOverheadUs + ((d == 1 && kb >= 1 && kb <= (int)kLeafMaxBits) ? n / 1.5e6 + parents / 2.0e4 : n * (d + 0.3) / 4.5e5);
        r_above = r_d;
    }
    return cost;
}

// -> the top level (depth) that minimises the estimate, and the estimate
uint32_t choose_top(const PlanState& ps, const CascadeShape& sh, const std::vector<uint64_t>& rel_mask, uint32_t max_depth, double* est_out) {
    uint32_t top = 1;
    double best = 0;
    for (uint32_t d = 1; d <= max_depth && d <= rel_mask.size(); ++d) {
        const double est = sh.forced_depth ? (double)__builtin_popcountll(rel_mask[d - 1]) : chain_cost_us(ps, rel_mask, d);
        if (d == 1 || est < best) { best = est; top = d; }
    }
    if (est_out) *est_out = sh.forced_depth ? chain_cost_us(ps, rel_mask, top) : best;
    return top;
}

// ---- splitting a block into sub-blocks ---------------------------------------------------------------------------------
// The digits F^d depends on over a whole block are the union over everything the block contains.  Fix one well-chosen digit
// and, in a network of canalizing rules, whole sub-trees of dependence disappear in each half: the two sub-blocks together
// have fewer classes than the block (north star, 2^63 problems: 2^32 classes at depth 4; after a dozen greedy splits
// 2^25.4).  plan_split grows that tree greedily on the cost estimate -- at each node the digit whose two halves are cheapest
// together, as long as that saves at least 15 % and the node is worth more than a few launches -- and returns the leaves
// as (fix_mask, fix_vals) over the digit index.  Any tree is correct (the leaves partition the block); only speed depends
// on it, so the tree found for the first block of a size is reused for the other blocks of that size in the space.

// the estimate for the (sub-)block with the digits `mask` fixed at `vals`; top_rel = the digits its top level enumerates
double cube_cost_us(const HostModel& m, const DevSpace& sp, const PlanState& ps, const CascadeShape& sh, uint64_t d_lo, uint32_t a_bits,
                    uint64_t mask, uint64_t vals, uint64_t* top_rel) {
    Cube c;
    std::vector<uint64_t> rel_mask;
    build_cube(m, sp, d_lo, a_bits, c, nullptr, mask, vals);
    cube_levels(m, sp, c, sh.max_depth, rel_mask);
    double est = 0;
    const uint32_t top = choose_top(ps, sh, rel_mask, sh.max_depth, &est);
    if (top_rel) *top_rel = rel_mask[top - 1];
    return est;
}

void plan_split(const HostModel& m, const DevSpace& sp, const PlanState& ps, const CascadeShape& sh, uint64_t d_lo, uint32_t a_bits, bool forced,
                std::vector<SplitLeaf>& leaves) {
    leaves.clear();
    const double min_cost_us = 3 * kLevelOverheadUs;        // below this a node is a handful of launches: not worth halving
    std::vector<SplitLeaf> todo{{0, 0}};
    while (!todo.empty()) {
        const SplitLeaf nd = todo.back();
        todo.pop_back();
        uint64_t top_rel = 0;
        const double here = cube_cost_us(m, sp, ps, sh, d_lo, a_bits, nd.mask, nd.vals, &top_rel);
        bool split = false;
        // (forced -- BSX_CUBE_SPLIT=1, tests: a tree of eight leaves whatever the estimates say)
        if (forced ? leaves.size() + todo.size() + 2 <= 8 : (here > min_cost_us && leaves.size() + todo.size() + 2 <= kMaxChains)) {
            double best = 0;
            int best_digit = -1;
            for (uint64_t left = top_rel; left; left &= left - 1) {
                const int j = __builtin_ctzll(left);
                const double both = cube_cost_us(m, sp, ps, sh, d_lo, a_bits, nd.mask | (1ull << j), nd.vals) +
                                    cube_cost_us(m, sp, ps, sh, d_lo, a_bits, nd.mask | (1ull << j), nd.vals | (1ull << j));
                if (best_digit < 0 || both < best) { best = both; best_digit = j; }
            }
            if (best_digit >= 0 && (forced || best < 0.85 * here)) {
                todo.push_back(SplitLeaf{nd.mask | (1ull << best_digit), nd.vals});
                todo.push_back(SplitLeaf{nd.mask | (1ull << best_digit), nd.vals | (1ull << best_digit)});
                split = true;
            }
        }
        if (!split) leaves.push_back(nd);
    }
}

}  // namespace bsx
