// Stand-alone driver for the per-parent level's count (boolsi_amd/csrc/bsx_leaf.h) and its program
// (bsx_cube_plan.cpp: build_leaf_program), for tests/test_leaf_factor_host.py.  Reads commands from stdin, one per line,
// every number in hex; answers on stdout, one line per query.  Builds with the host C++ compiler alone:
//   c++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Iboolsi_amd/csrc tests/leaf_check.cpp boolsi_amd/csrc/bsx_cube_plan.cpp
//
//   net N NW | node I K P.. TT | fixmask W*8 | fixval W*8 | any C NODE..            (as tests/plan_check.cpp)
//   program C DIGIT..        -> program OK KB M N_ENUM N_FREE | digits NODE.. | then one line per rule:
//                               rule NODE K FREE_DIGIT TT IN..      (the program stays loaded for `count`)
//   count NW PARENT*NW CAND*NW -> count HITS_OF_ALL_CHILDREN then, for every power-of-two split, parts P HITS_PER_PART.. CHILDREN_PER_PART
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "bsx_cube_plan.h"
#include "bsx_leaf.h"

using namespace bsx;

namespace {

struct Reader {
    std::istringstream in;
    explicit Reader(const std::string& line) : in(line) {}
    uint64_t u() {
        std::string tok;
        if (!(in >> tok)) { std::fprintf(stderr, "leaf_check: missing field\n"); std::exit(2); }
        return std::strtoull(tok.c_str(), nullptr, 16);
    }
    template <size_t N> void words(uint32_t (&out)[N]) { for (size_t i = 0; i < N; ++i) out[i] = (uint32_t)u(); }
};

template <int NW>
void count(Reader& r, const LeafProgram& L, const uint32_t* rules) {
    uint32_t Sp[NW], C[NW];
    for (uint32_t& w : Sp) w = (uint32_t)r.u();
    for (uint32_t& w : C) w = (uint32_t)r.u();
    std::printf("count %x\n", leaf_count<NW>(Sp, C, rules, L.kb, L.m, L.n_enum, L.n_free, 0u, 1u));
    for (uint32_t parts = 1; parts <= leaf_units(L.m); parts <<= 1) {
        std::printf("parts %x", parts);
        for (uint32_t part = 0; part < parts; ++part) std::printf(" %x", leaf_count<NW>(Sp, C, rules, L.kb, L.m, L.n_enum, L.n_free, part, parts));
        std::printf(" %x\n", leaf_children_per_part(L.kb, L.m, parts));
    }
}

}  // namespace

int main() {
    HostModel m;
    DevSpace sp{};
    static LeafProgram L;
    static uint32_t rules[kLeafMaxDeps * 4];
    static_assert(sizeof(rules) == sizeof(L.dep), "a rule is four words");
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
        } else if (cmd == "fixmask") r.words(sp.fixmask);
        else if (cmd == "fixval") r.words(sp.fixval);
        else if (cmd == "any") {
            m.any.resize(r.u());
            for (uint32_t& v : m.any) v = (uint32_t)r.u();
            sp.n_any = (uint32_t)m.any.size();
        } else if (cmd == "program") {
            std::vector<uint32_t> digits(r.u());
            for (uint32_t& v : digits) v = (uint32_t)r.u();
            const bool ok = build_leaf_program(m, sp, digits, L);
            std::printf("program %d %x %x %x %x\n", (int)ok, L.kb, L.m, L.n_enum, L.n_free);
            if (!ok) { std::memset(&L, 0, sizeof(L)); continue; }
            std::memcpy(rules, L.dep, sizeof(rules));
            std::printf("digits");
            for (uint32_t q = 0; q < L.kb; ++q) std::printf(" %x", (unsigned)L.digit_node[q]);
            std::printf("\n");
            for (uint32_t i = 0; i < L.n_dep; ++i) {
                const LeafDep& d = L.dep[i];
                std::printf("rule %x %x %x %x", (unsigned)d.node, (unsigned)(d.k & 0xFFu), (unsigned)(d.k >> 8), d.tt);
                for (uint32_t j = 0; j < (d.k & 0xFFu); ++j) std::printf(" %x", (unsigned)d.in[j]);
                std::printf("\n");
            }
        } else if (cmd == "count") {
            const uint32_t nw = (uint32_t)r.u();
            if (nw == 2) count<2>(r, L, rules);
            else if (nw == 4) count<4>(r, L, rules);
            else { std::fprintf(stderr, "leaf_check: state words %u\n", nw); return 2; }
        } else {
            std::fprintf(stderr, "leaf_check: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
