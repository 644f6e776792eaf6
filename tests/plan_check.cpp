// Stand-alone driver for the engine's host arithmetic that runs without a GPU (tests/test_plan_host.py): the cube
// planner (boolsi_amd/csrc/bsx_cube_plan.cpp) and the exact merge (bsx_merge.h).  Reads commands from stdin, one per
// line, every number in hex; answers on stdout, one line per query.  Builds with the host C++ compiler alone:
//   c++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Iboolsi_amd/csrc tests/plan_check.cpp boolsi_amd/csrc/bsx_cube_plan.cpp
//
//   net N NW | node I K P.. TT | origin W*8 | fixmask W*8 | fixval W*8 | any C NODE.. | sched C (T NODE VAL)..
//   seen WHICH DEPTH CLASSES NEAR | seenclear
//   cube D_LO A FIX_MASK FIX_VALS DEPTH              -> cube OK REL LEVEL..
//   top D_LO A FIX_MASK FIX_VALS DEPTH FORCED        -> top TOP EST COST..      (costs as C99 hex floats)
//   split D_LO A FORCED DEPTH FORCED_DEPTH           -> split MASK:VALS ..
//   mreset | ctr NW SHIFT MAX_T, then slot / sums lines, then end | unres NW SHIFT TP CAP_REL MAX_T MAX_LEN W.. -> unres BOOKED
//   mdump                                            -> rec lines, then sums NONE_HI NONE_LO REF_HI REF_LO
//   ushift / usigned / umul W*4 ARGS                 -> u256 W*4
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "bsx_cube_plan.h"
#include "bsx_merge.h"

using namespace bsx;

namespace {

struct Reader {
    std::istringstream in;
    explicit Reader(const std::string& line) : in(line) {}
    uint64_t u() {
        std::string tok;
        if (!(in >> tok)) { std::fprintf(stderr, "plan_check: missing field\n"); std::exit(2); }
        return std::strtoull(tok.c_str(), nullptr, 16);
    }
    template <size_t N> void words(uint32_t (&out)[N]) { for (size_t i = 0; i < N; ++i) out[i] = (uint32_t)u(); }
};

void print_u256(const U256& v) { std::printf(" %" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64, v.w[0], v.w[1], v.w[2], v.w[3]); }
void print_u128(u128 v) { std::printf(" %" PRIx64 " %" PRIx64, (uint64_t)(v >> 64), (uint64_t)v); }

CascadeShape shape(uint32_t max_depth, bool forced_depth) {
    CascadeShape sh{};
    sh.cap_rel = BSX_T_INF; sh.cap_rel32 = 0xFFFFFFFFu; sh.fast_steps = 192;
    sh.max_depth = max_depth; sh.forced_depth = forced_depth;
    return sh;
}

}  // namespace

int main() {
    HostModel m;
    DevSpace sp{};
    PlanState ps;
    MergedTable table;
    u128 pass_none = 0, pass_ref = 0;
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        Reader r(line);
        if (!(r.in >> cmd)) continue;
        if (cmd == "net") {
            m = HostModel();
            sp = DevSpace{};
            m.n_nodes = (uint32_t)r.u(); m.nw = (uint32_t)r.u();
            m.pred_offsets.assign(1, 0);
            m.tt0.clear();
        } else if (cmd == "node") {
            r.u();                                      // (the index: nodes come in order)
            const uint32_t k = (uint32_t)r.u();
            for (uint32_t j = 0; j < k; ++j) m.pred_idx.push_back((uint32_t)r.u());
            m.pred_offsets.push_back((uint32_t)m.pred_idx.size());
            m.tt0.push_back(r.u());
        } else if (cmd == "origin") r.words(sp.origin);
        else if (cmd == "fixmask") r.words(sp.fixmask);
        else if (cmd == "fixval") r.words(sp.fixval);
        else if (cmd == "any") {
            m.any.resize(r.u());
            for (uint32_t& v : m.any) v = (uint32_t)r.u();
            sp.n_any = (uint32_t)m.any.size();
        } else if (cmd == "sched") {
            m.sched.resize(3 * r.u());
            for (uint32_t& v : m.sched) v = (uint32_t)r.u();
            sp.tp_origin = 0;
            for (size_t e = 0; e < m.sched.size(); e += 3) sp.tp_origin = std::max(sp.tp_origin, m.sched[e]);
        } else if (cmd == "seenclear") ps = PlanState();
        else if (cmd == "seen") {
            const uint64_t which = r.u(), d = r.u();
            ps.near_seen[which][d][0] = (double)r.u();
            ps.near_seen[which][d][1] = (double)r.u();
        } else if (cmd == "cube" || cmd == "top") {
            const uint64_t d_lo = r.u();
            const uint32_t a = (uint32_t)r.u();
            const uint64_t fix_mask = r.u(), fix_vals = r.u();
            const uint32_t depth = (uint32_t)r.u();
            Cube c;
            build_cube(m, sp, d_lo, a, c, nullptr, fix_mask, fix_vals);
            std::vector<uint64_t> levels;
            cube_levels(m, sp, c, depth, levels);
            if (cmd == "cube") {
                uint64_t rel = 0;
                for (uint32_t j : c.rel) rel |= 1ull << j;
                std::printf("cube %d %" PRIx64, (int)c.ok, rel);
                for (uint64_t l : levels) std::printf(" %" PRIx64, l);
            } else {
                const CascadeShape sh = shape(depth, r.u() != 0);
                double est = 0;
                const uint32_t top = choose_top(ps, sh, levels, depth, &est);
                std::printf("top %x %a", top, est);
                for (uint32_t d = 1; d <= depth; ++d) std::printf(" %a", chain_cost_us(ps, levels, d));
            }
            std::printf("\n");
        } else if (cmd == "split") {
            const uint64_t d_lo = r.u();
            const uint32_t a = (uint32_t)r.u();
            const bool forced = r.u() != 0;
            const uint32_t depth = (uint32_t)r.u();
            const CascadeShape sh = shape(depth, r.u() != 0);
            std::vector<SplitLeaf> leaves;
            plan_split(m, sp, ps, sh, d_lo, a, forced, leaves);
            std::printf("split");
            for (const SplitLeaf& l : leaves) std::printf(" %" PRIx64 ":%" PRIx64, l.mask, l.vals);
            std::printf("\n");
        } else if (cmd == "mreset") {
            table.clear();
            pass_none = pass_ref = 0;
        } else if (cmd == "ctr") {
            const uint32_t nw = (uint32_t)r.u(), shift = (uint32_t)r.u();
            const uint64_t max_t = r.u();
            Counters c;
            std::memset(&c, 0, sizeof(c));
            while (std::getline(std::cin, line)) {
                Reader q(line);
                q.in >> cmd;
                if (cmd == "end") break;
                if (cmd == "slot") {
                    const uint64_t a = q.u();
                    q.words(c.acc_key[a]);
                    c.acc_len[a] = (unsigned int)q.u();
                    c.acc_cnt[a] = q.u(); c.acc_sl[a] = q.u(); c.acc_sl2_lo[a] = q.u(); c.acc_sl2_hi[a] = q.u();
                    c.fix_cnt[a] = q.u(); c.fix_sl[a] = q.u(); c.fix_sl2[a] = q.u();
                } else if (cmd == "sums") {
                    c.n_none = q.u(); c.steps_ref = q.u(); c.fix_none = q.u(); c.fix_ref = q.u(); c.fix_capfail = q.u();
                }
            }
            merge_cube_counters(table, c, shift, nw);
            fold_cube_level(c, shift, max_t, pass_none, pass_ref);
        } else if (cmd == "unres") {
            const uint32_t nw = (uint32_t)r.u(), shift = (uint32_t)r.u();
            const uint64_t tp = r.u(), cap_rel = r.u(), max_t = r.u(), max_len = r.u();
            uint32_t rec[kMaxW32 + 3];
            for (uint32_t w = 0; w < nw + 3; ++w) rec[w] = (uint32_t)r.u();
            ProblemRec32 pr{};
            r.words(pr.key);
            pr.length = (uint32_t)r.u(); pr.trajectory_l = (uint32_t)r.u(); pr.found = (uint32_t)r.u();
            std::printf("unres %d\n", (int)book_unresolved_class(table, pass_none, pass_ref, rec, pr, nw, shift, tp, cap_rel, max_t, max_len));
        } else if (cmd == "mdump") {
            for (const auto& kv : table) {
                const WideRec& w = kv.second;
                std::printf("rec %" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64, w.key[0], w.key[1], w.key[2], w.key[3], w.length);
                print_u128(w.count);
                print_u256(w.sum_l);
                print_u256(w.sum_l2);
                std::printf("\n");
            }
            std::printf("sums");
            print_u128(pass_none);
            print_u128(pass_ref);
            std::printf("\n");
        } else if (cmd == "ushift" || cmd == "usigned" || cmd == "umul") {
            U256 v;
            for (uint64_t& w : v.w) w = r.u();
            if (cmd == "ushift") { const uint64_t lo = r.u(), hi = r.u(); v.add_shifted(lo, hi, (uint32_t)r.u()); }
            else if (cmd == "usigned") v.add_signed((int64_t)r.u());
            else { const uint64_t lo = r.u(), hi = r.u(); v.add_mul(((u128)hi << 64) | lo, r.u()); }
            std::printf("u256");
            print_u256(v);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "plan_check: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
