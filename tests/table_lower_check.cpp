// Stand-alone driver of boolsi_amd/csrc/bsx_table_lower.cpp for tests/test_table_lower_host.py: built with the host C++
// compiler and no HIP include path.  Reads commands (hexadecimal tokens) on stdin and prints what the unit answers.
//   keys N v..  lens N v..  offs N v..  fix N v..     the table's arrays and the fix mask (32-bit words)
//   limit family knob                                 -> "limit" step limit          (family: 0 per lane, 1 wide)
//   check stride n null_keys want_states null_offs w64 n_nodes limit
//                                                     -> "check status message" | "check 0 sum_len state_words"
//   limits n sum_len edges_ok n_edges_ok              -> "limits status message"
//   sizes family n sum_len n_free edge_cap            -> "sizes" flips slot_bits n_slots most_edges out_cap edge_slots
//   plan family w64 n_nodes edge_cap                  -> "plan" sum_len and the six sizes, then "free", "first", "offsets"   (lens, fix)
//   chunks count chunk                                -> "chunks" size (first count)..
//   launches family n flips knob                      -> "launches" profile_launches trans_launches flip_chunk
//   status family open dup probe step overflow undecided n_edges edge_cap    -> "status status text"
//   finish N (src dst count sum_mu)..                 -> "finish" sum_mu (src dst count sum_mu)..
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "bsx_table_lower.h"

using namespace bsx;

static uint64_t num() {
    uint64_t v = 0;
    if (!(std::cin >> std::hex >> v)) { std::fprintf(stderr, "table_lower_check: number expected\n"); std::exit(2); }
    return v;
}

template <typename T>
static void list(std::vector<T>& v) {
    v.resize(num());
    for (T& x : v) x = (T)num();
}

template <typename T>
static void put(const char* name, const std::vector<T>& v) {
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %llx", (unsigned long long)x);
    std::printf("\n");
}

static void put_sizes(const TransSizes& s) {
    std::printf(" %llx %x %llx %llx %llx %llx\n", (unsigned long long)s.flips, s.slot_bits, (unsigned long long)s.n_slots,
                (unsigned long long)s.most_edges, (unsigned long long)s.out_cap, (unsigned long long)s.edge_slots);
}

int main() {
    std::vector<uint64_t> keys, lens, offs;
    std::vector<uint32_t> fix;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "keys") list(keys);
        else if (cmd == "lens") list(lens);
        else if (cmd == "offs") list(offs);
        else if (cmd == "fix") list(fix);
        else if (cmd == "limit") {
            const TableFamily family = (TableFamily)num();
            std::printf("limit %llx\n", (unsigned long long)table_step_limit(family, (uint32_t)num()));
        } else if (cmd == "check") {
            TableView t;
            t.key_stride = (uint32_t)num();
            t.n = num();
            const bool null_keys = num() != 0, want_states = num() != 0, null_offs = num() != 0;
            const uint32_t w64 = (uint32_t)num(), n_nodes = (uint32_t)num();
            const uint64_t limit = num();
            if (keys.size() != t.n * t.key_stride || lens.size() != t.n || (!null_offs && offs.size() != t.n)) {
                std::fprintf(stderr, "table_lower_check: array sizes\n");
                return 2;
            }
            t.keys = null_keys ? nullptr : keys.data();
            t.lengths = lens.data();
            TableSizes out;
            out.sum_len = out.state_words = 0xA5A5;             // (written on success only)
            const LowerStatus s = table_check(t, want_states, null_offs ? nullptr : offs.data(), w64, n_nodes, limit, out);
            if (s) std::printf("check %d %s\n", s.status, s.msg);
            else std::printf("check 0 %llx %llx\n", (unsigned long long)out.sum_len, (unsigned long long)out.state_words);
        } else if (cmd == "limits") {
            const uint64_t n = num(), sum_len = num();
            int dummy = 0;
            const void* edges = num() ? &dummy : nullptr;
            const void* n_edges = num() ? &dummy : nullptr;
            const LowerStatus s = trans_limits(n, sum_len, edges, n_edges);
            std::printf("limits %d %s\n", s.status, s.msg);
        } else if (cmd == "sizes") {
            const TableFamily family = (TableFamily)num();
            const uint64_t n = num(), sum_len = num();
            const uint32_t n_free = (uint32_t)num();
            std::printf("sizes");
            put_sizes(trans_sizes(family, n, sum_len, n_free, num()));
        } else if (cmd == "plan") {
            const TableFamily family = (TableFamily)num();
            const uint32_t w64 = (uint32_t)num(), n_nodes = (uint32_t)num();
            if (fix.size() * 32 < n_nodes) { std::fprintf(stderr, "table_lower_check: fix mask words\n"); return 2; }
            const TransPlan p = trans_plan(family, lens.data(), lens.size(), w64, fix.data(), n_nodes, num());
            std::printf("plan %llx", (unsigned long long)p.sum_len);
            put_sizes(p.sz);
            put("free", p.free_nodes);
            put("first", p.row_first);
            put("offsets", p.offsets);
        } else if (cmd == "chunks") {
            const uint64_t count = num(), chunk = num();
            std::printf("chunks %llx", (unsigned long long)chunks(count, chunk).size());
            for (const Chunk c : chunks(count, chunk)) std::printf(" %llx %llx", (unsigned long long)c.first, (unsigned long long)c.count);
            std::printf("\n");
        } else if (cmd == "launches") {
            const TableFamily family = (TableFamily)num();
            const uint64_t n = num(), flips = num(), knob = num();
            std::printf("launches %x %x %llx\n", profile_launches(family, n), trans_launches(family, n, flips, knob),
                        (unsigned long long)trans_flip_chunk(family, knob));
        } else if (cmd == "status") {
            const TableFamily family = (TableFamily)num();
            TransCtr tc{};
            tc.open_row = (unsigned)num(); tc.dup_row = (unsigned)num(); tc.probe_full = (unsigned)num();
            tc.step_limit_hits = (unsigned)num(); tc.edge_overflow = (unsigned)num(); tc.rows_undecided = (unsigned)num();
            tc.n_edges = num();
            std::string text;
            const int status = trans_status(family, tc, num(), text);
            std::printf("status %d %s\n", status, text.c_str());
        } else if (cmd == "finish") {
            std::vector<TransEdge> got(num());
            for (TransEdge& e : got) { e.src = (uint32_t)num(); e.dst = (uint32_t)num(); e.count = num(); e.sum_mu = num(); }
            std::vector<bsx_trans_edge> edges(got.size());
            const uint64_t sum_mu = trans_finish_edges(got, edges.data());
            std::printf("finish %llx", (unsigned long long)sum_mu);
            for (const bsx_trans_edge& e : edges)
                std::printf(" %x %x %llx %llx", e.src, e.dst, (unsigned long long)e.count, (unsigned long long)e.sum_mu);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "table_lower_check: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
