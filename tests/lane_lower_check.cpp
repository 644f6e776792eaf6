// Stand-alone driver of boolsi_amd/csrc/bsx_lane_lower.cpp for tests/test_lane_lower_host.py: built with the host C++
// compiler and no HIP include path.  Reads commands (hexadecimal tokens) on stdin and prints what the unit made of them.
//   po N v..  pi N v..  tto N v..  tt N v..      the four network arrays (pi 0: a null pointer)
//   net n cache_kb lut                           (lut: 0 = by the rule, else the forced mode + 1)
//        -> "net nw k_mux n_chunks n_wide lut_mode slots cache_stride cache_bytes shmem shmem_attract",
//           masks, lut, wdesc, wpreds, wtt, mpo, mpi, mtt0 (the model's copies), one per line
//   origin N w..  any N v..  fixed N (node value)..  fvar N (node range)..  sched N (t node value)..  pvar N (t node range)..
//   space                                        -> "space status message" | "space 0 n_any identity n_runs n_fv n_pv tp_origin
//                                                   tp_max variants saturated", origin, fixmask, fixval, deposit, any, fv, pv, set, clr, sched
//   range d0 d1 d2 d3 variant lo hi n_any variants saturated      -> "range status message"    (lo hi: the count)
//   plus d0 d1 d2 d3 variant lo hi n_any         -> "plus" d0 d1 d2 d3 variant
//   target N mask.. code..                       -> "target" tmask[8] tcode[8]
//   variant v                                    -> "variant" fixmask[8] fixval[8]     (the last space's fixed nodes and variations)
//   cube a n_rel umask[8] tmask[8] tcode[8]      -> "cube" count cube cube_shift cube_t0_shift rep_mask[8] rep_code[8]
//   shares count n_waves chunk                   -> "shares" chunk_first chunk
//   listing left wanted                          -> "listing" problems
//   cubesok n_any identity n_runs n_pv tp_origin saturated         -> "cubesok" 0|1
//   plan d0 variant count n_any cubes            -> "plan" (n block digit a_bits variant)..
//   simblocks count cus                          -> "simblocks" blocks
//   sliced n k knob count cus                    -> "sliced" gen2 rows shmem groups per_cu blocks       (knob: BSX_SLICED + 1)
//   slicedok n k n_wide n_fv n_pv knob traj final digests max_t count  -> "slicedok" 0|1
//   rowdesc k                                    -> "rowdesc" words        (the last net's model, the last space's fixed nodes)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "bsx_lane_lower.h"

using namespace bsx;

static uint64_t num() {
    uint64_t v = 0;
    if (!(std::cin >> std::hex >> v)) { std::fprintf(stderr, "lane_lower_check: number expected\n"); std::exit(2); }
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

static bsx_index index_in() {
    bsx_index x{};
    for (int w = 0; w < 4; ++w) x.init_digits[w] = num();
    x.variant = num();
    return x;
}

static u128 wide_in() {
    const uint64_t lo = num(), hi = num();
    return ((u128)hi << 64) | lo;
}

int main() {
    std::vector<uint32_t> po, pi, tto, any, fixed, fvar, sched, pvar;
    std::vector<uint64_t> tt, origin;
    LaneNet net;
    HostModel model;
    LaneSpace sp;
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
            const uint64_t cache_kb = num();
            const int want = (int)num() - 1;
            if (po.size() != (size_t)n + 1 || tto.size() != (size_t)n + 1 || tt.size() != tto[n] || pi.size() != po[n]) {
                std::fprintf(stderr, "lane_lower_check: offsets\n");
                return 2;
            }
            lane_lower_network(n, po.data(), pi.empty() ? nullptr : pi.data(), tto.data(), tt.data(), cache_kb, want, net, model);
            std::printf("net %x %x %x %x %x %x %zx %zx %zx %zx\n", net.nw, net.k_mux, net.n_chunks, net.n_wide, (unsigned)net.lut_mode,
                        net.cache_lds_slots, net.cache_stride, net.cache_bytes, net.shmem, net.shmem_attract);
            put("masks", net.masks.data(), net.masks.size());
            put("lut", net.lut.data(), net.lut.size());
            put("wdesc", net.wdesc.data(), net.wdesc.size());
            put("wpreds", net.wpreds.data(), net.wpreds.size());
            put("wtt", net.wtt.data(), net.wtt.size());
            if (model.n_nodes != n || model.nw != net.nw) { std::fprintf(stderr, "lane_lower_check: model head\n"); return 2; }
            put("mpo", model.pred_offsets.data(), model.pred_offsets.size());
            put("mpi", model.pred_idx.data(), model.pred_idx.size());
            put("mtt0", model.tt0.data(), model.tt0.size());
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
            const uint32_t n = model.n_nodes, w64 = (n + 63) / 64;
            if (origin.size() != w64) { std::fprintf(stderr, "lane_lower_check: origin words\n"); return 2; }
            const LowerStatus s = lane_lower_space(n, model.nw, w64, origin.data(), any.data(), (uint32_t)any.size(), fx.data(),
                                                   (uint32_t)fx.size(), fv.data(), (uint32_t)fv.size(), sc.data(), (uint32_t)sc.size(),
                                                   pv.data(), (uint32_t)pv.size(), sp);
            if (s) { std::printf("space %d %s\n", s.status, s.msg); continue; }
            std::printf("space 0 %x %x %x %x %x %x %x %llx %x\n", sp.sp.n_any, sp.sp.identity_any, sp.sp.n_runs, sp.sp.n_fv, sp.sp.n_pv,
                        sp.sp.tp_origin, sp.tp_max, (unsigned long long)sp.variant_count, (unsigned)sp.variant_count_saturated);
            put("origin", sp.sp.origin, kMaxW32);
            put("fixmask", sp.sp.fixmask, kMaxW32);
            put("fixval", sp.sp.fixval, kMaxW32);
            put("deposit", sp.sp.deposit, 2 * (size_t)sp.sp.n_runs);
            put("any", sp.any.data(), sp.any.size());
            put("fv", sp.fv.data(), sp.fv.size());
            put("pv", sp.pv.data(), sp.pv.size());
            put("set", sp.set.data(), sp.set.size());
            put("clr", sp.clr.data(), sp.clr.size());
            put("sched", sp.sched.data(), sp.sched.size());
        } else if (cmd == "range") {
            const bsx_index first = index_in();
            const u128 count = wide_in();
            const uint32_t n_any = (uint32_t)num();
            const uint64_t variants = num();
            const LowerStatus s = range_check(&first, count, n_any, variants, num() != 0);
            std::printf("range %d %s\n", s.status, s.msg);
        } else if (cmd == "plus") {
            const bsx_index first = index_in();
            const u128 delta = wide_in();
            const bsx_index r = index_plus(first, delta, (uint32_t)num());
            const uint64_t out[5] = {r.init_digits[0], r.init_digits[1], r.init_digits[2], r.init_digits[3], r.variant};
            put("plus", out, 5);
        } else if (cmd == "target") {
            std::vector<uint64_t> mask(num()), code(mask.size());
            for (uint64_t& w : mask) w = num();
            for (uint64_t& w : code) w = num();
            uint32_t out[2 * kMaxW32] = {};
            target_words((uint32_t)mask.size(), mask.data(), code.data(), out, out + kMaxW32);
            put("target", out, 2 * kMaxW32);
        } else if (cmd == "variant") {
            uint32_t out[2 * kMaxW32];
            for (int w = 0; w < kMaxW32; ++w) { out[w] = sp.sp.fixmask[w]; out[kMaxW32 + w] = sp.sp.fixval[w]; }
            variant_fixed_nodes(sp.fv, num(), out, out + kMaxW32);
            put("variant", out, 2 * kMaxW32);
        } else if (cmd == "cube") {
            Cube c{};
            c.a = (uint32_t)num();
            c.rel.resize(num());
            for (uint32_t& w : c.umask) w = (uint32_t)num();
            TargetParams P{};
            for (uint32_t& w : P.tmask) w = (uint32_t)num();
            for (uint32_t& w : P.tcode) w = (uint32_t)num();
            target_cube_words(c, P);
            std::printf("cube %llx %x %x %x", (unsigned long long)P.count, P.cube, P.cube_shift, P.cube_t0_shift);
            for (uint32_t w : P.rep_mask) std::printf(" %x", w);
            for (uint32_t w : P.rep_code) std::printf(" %x", w);
            std::printf("\n");
        } else if (cmd == "shares") {
            TargetParams P{};
            P.count = num();
            const uint64_t n_waves = num();
            target_cube_shares(n_waves, (uint32_t)num(), P);
            std::printf("shares %llx %x\n", (unsigned long long)P.chunk_first, P.chunk);
        } else if (cmd == "listing") {
            const uint64_t left = num();
            std::printf("listing %llx\n", (unsigned long long)target_listing_piece(left, num()));
        } else if (cmd == "cubesok") {
            DevSpace s{};
            s.n_any = (uint32_t)num(); s.identity_any = (uint32_t)num(); s.n_runs = (uint32_t)num();
            s.n_pv = (uint32_t)num(); s.tp_origin = (uint32_t)num();
            std::printf("cubesok %d\n", (int)target_cubes_ok(s, num() != 0));
        } else if (cmd == "plan") {
            bsx_index first{};
            first.init_digits[0] = num();
            first.variant = num();
            const uint64_t count = num();
            const uint32_t n_any = (uint32_t)num();
            const bool cubes = num() != 0;
            std::printf("plan");
            for (uint64_t done = 0; done < count;) {
                const CountPiece p = count_piece(first, done, count, n_any, cubes);
                if (!p.n || p.n > count - done) { std::fprintf(stderr, "lane_lower_check: piece of %llu problems\n", (unsigned long long)p.n); return 2; }
                std::printf(" %llx %x %llx %x %llx", (unsigned long long)p.n, (unsigned)p.block, (unsigned long long)p.digit, p.a_bits,
                            (unsigned long long)p.variant);
                done += p.n;
            }
            std::printf("\n");
        } else if (cmd == "simblocks") {
            const uint64_t count = num();
            std::printf("simblocks %llx\n", (unsigned long long)lane_sim_blocks(count, (uint32_t)num()));
        } else if (cmd == "sliced") {
            const uint32_t n = (uint32_t)num(), k = (uint32_t)num();
            const int knob = (int)num() - 1;
            const uint64_t count = num();
            const SlicedShape s = sliced_shape(n, k, knob, count, (uint32_t)num());
            std::printf("sliced %x %x %zx %llx %llx %llx\n", (unsigned)s.gen2, s.rows, s.shmem, (unsigned long long)s.groups,
                        (unsigned long long)s.per_cu, (unsigned long long)s.blocks);
        } else if (cmd == "slicedok") {
            DevNet dn{};
            DevSpace s{};
            const uint32_t n = (uint32_t)num();
            dn.k_mux = (uint32_t)num(); dn.n_wide = (uint32_t)num();
            s.n_fv = (uint32_t)num(); s.n_pv = (uint32_t)num();
            const int knob = (int)num() - 1;
            const bool traj = num() != 0, fin = num() != 0, dig = num() != 0;
            const uint64_t max_t = num();
            std::printf("slicedok %d\n", (int)sliced_ok(n, dn, s, knob, traj, fin, dig, max_t, num()));
        } else if (cmd == "rowdesc") {
            std::vector<uint32_t> desc;
            sliced_row_desc(model, sp.sp, (uint32_t)num(), desc);
            put("rowdesc", desc.data(), desc.size());
        } else {
            std::fprintf(stderr, "lane_lower_check: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
