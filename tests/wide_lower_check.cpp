// Stand-alone driver of boolsi_amd/csrc/bsx_wide_lower.cpp for tests/test_wide_lower_host.py: built with the host C++
// compiler and no HIP include path.  Reads commands (hexadecimal tokens) on stdin and prints what the unit lowered.
//   po N v..  pi N v..  tto N v..  tt N v..      the four network arrays (pi 0: a null pointer)
//   net n                                        -> "net status message" | "net 0 n rows w64 K", wdesc, wpreds, wtt
//   origin N w..  any N v..  fixed N (node value)..  fvar N (node range)..  sched N (t node value)..  pvar N (t node range)..
//   space                                        -> "space status message" | "space 0 ...", the arrays, one per line
//   target N mask.. code..                       -> "target" tmask[32] tcode[32]        (N words each)
//   flat lo hi n_any                             -> "flat status message" | "flat 0" digits[4] variant
//   grid count L shmem cus                       -> "grid" blocks
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "bsx_wide_lower.h"

using namespace bsx;

static uint64_t num() {
    uint64_t v = 0;
    if (!(std::cin >> std::hex >> v)) { std::fprintf(stderr, "wide_lower_check: number expected\n"); std::exit(2); }
    return v;
}

template <typename T>
static void list(std::vector<T>& v, uint32_t per = 1) {
    v.resize(num() * per);
    for (T& x : v) x = (T)num();
}

template <typename T>
static void put(const char* name, const T* v, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n; ++i) std::printf(" %llx", (unsigned long long)v[i]);
    std::printf("\n");
}

int main() {
    std::vector<uint32_t> po, pi, tto, any, fixed, fvar, sched, pvar;
    std::vector<uint64_t> tt, origin;
    WideNet net;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "po") list(po);
        else if (cmd == "pi") list(pi);
        else if (cmd == "tto") list(tto);
        else if (cmd == "tt") list(tt);
        else if (cmd == "origin") list(origin);
        else if (cmd == "any") list(any);
        else if (cmd == "fixed") list(fixed, 2);
        else if (cmd == "fvar") list(fvar, 2);
        else if (cmd == "sched") list(sched, 3);
        else if (cmd == "pvar") list(pvar, 3);
        else if (cmd == "net") {
            const uint32_t n = (uint32_t)num();
            if (po.size() != (size_t)n + 1 || tto.size() != (size_t)n + 1) { std::fprintf(stderr, "wide_lower_check: offsets\n"); return 2; }
            const uint32_t* pidx = pi.empty() ? nullptr : pi.data();
            LowerStatus s = wide_check_size(n);
            if (!s) s = check_network_arrays(n, po.data(), pidx, tto.data());
            if (s) { std::printf("net %d %s\n", s.status, s.msg); continue; }
            wide_lower_network(n, po.data(), pidx, tto.data(), tt.data(), net);
            std::printf("net 0 %x %x %x %x\n", net.n, net.rows, net.w64, net.K);
            put("wdesc", net.wdesc.data(), net.wdesc.size());
            put("wpreds", net.wpreds.data(), net.wpreds.size());
            put("wtt", net.wtt.data(), net.wtt.size());
        } else if (cmd == "space") {
            static_assert(sizeof(bsx_fixed) == 8 && sizeof(bsx_fixed_var) == 8 && sizeof(bsx_pert) == 12 && sizeof(bsx_pert_var) == 12,
                          "the entries are packed uint32 fields");
            std::vector<bsx_fixed> fx(fixed.size() / 2);
            std::vector<bsx_fixed_var> fv(fvar.size() / 2);
            std::vector<bsx_pert> sc(sched.size() / 3);
            std::vector<bsx_pert_var> pv(pvar.size() / 3);
            for (size_t j = 0; j < fx.size(); ++j) fx[j] = bsx_fixed{fixed[2 * j], fixed[2 * j + 1]};
            for (size_t j = 0; j < fv.size(); ++j) fv[j] = bsx_fixed_var{fvar[2 * j], fvar[2 * j + 1]};
            for (size_t j = 0; j < sc.size(); ++j) sc[j] = bsx_pert{sched[3 * j], sched[3 * j + 1], sched[3 * j + 2]};
            for (size_t j = 0; j < pv.size(); ++j) pv[j] = bsx_pert_var{pvar[3 * j], pvar[3 * j + 1], pvar[3 * j + 2]};
            if (origin.size() != net.w64) { std::fprintf(stderr, "wide_lower_check: origin words\n"); return 2; }
            WideSpace sp;
            const LowerStatus s = wide_lower_space(net, origin.data(), any.data(), (uint32_t)any.size(), fx.data(), (uint32_t)fx.size(),
                                                   fv.data(), (uint32_t)fv.size(), sc.data(), (uint32_t)sc.size(), pv.data(),
                                                   (uint32_t)pv.size(), sp);
            if (s) { std::printf("space %d %s\n", s.status, s.msg); continue; }
            std::printf("space 0 %x %x %x %llx %x %x %zx %x %x %x %x\n", sp.n_fslots, sp.tp_origin, sp.tp_max,
                        (unsigned long long)sp.variant_count, (unsigned)sp.variant_count_saturated, sp.L, sp.shmem, sp.n_any, sp.n_fv,
                        sp.n_pv, sp.n_sched);
            put("origin", sp.origin, kWideMaxW32);
            put("fixmask", sp.fixmask, kWideMaxW32);
            put("any", sp.any.data(), sp.any.size());
            put("fv", sp.fv.data(), sp.fv.size());
            put("pv", sp.pv.data(), sp.pv.size());
            put("sched", sp.sched.data(), sp.sched.size());
            put("desc", sp.desc.data(), sp.desc.size());
        } else if (cmd == "target") {
            std::vector<uint64_t> mask(num()), code(mask.size());
            for (uint64_t& w : mask) w = num();
            for (uint64_t& w : code) w = num();
            uint32_t out[2 * kWideMaxW32];
            for (uint32_t& w : out) w = 0xA5A5A5A5u;            // (the unit must write every word)
            wide_target_words(net.n, mask.data(), code.data(), out, out + kWideMaxW32);
            put("target", out, 2 * kWideMaxW32);
        } else if (cmd == "flat") {
            bsx_u128 flat;
            flat.lo = num(); flat.hi = num();
            bsx_index first;
            const LowerStatus s = wide_split_flat(flat, (uint32_t)num(), first);
            if (s) { std::printf("flat %d %s\n", s.status, s.msg); continue; }
            std::printf("flat 0 %llx %llx %llx %llx %llx\n", (unsigned long long)first.init_digits[0], (unsigned long long)first.init_digits[1],
                        (unsigned long long)first.init_digits[2], (unsigned long long)first.init_digits[3], (unsigned long long)first.variant);
        } else if (cmd == "grid") {
            const uint64_t count = num();
            const uint32_t L = (uint32_t)num();
            const size_t shmem = (size_t)num();
            std::printf("grid %llx\n", (unsigned long long)wide_grid_blocks(count, L, shmem, (uint32_t)num()));
        } else {
            std::fprintf(stderr, "wide_lower_check: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
