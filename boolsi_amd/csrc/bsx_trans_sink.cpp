// EdgeSink (bsx_table_host.h): what bsx_run_attractor_transitions and bsx_run_attractor_transitions_wide do alike
// around their own walk kernels -- the edge table and the counters before, k_trans_drain behind, and after the call's
// one wait the status, the sorted edge list, the exits and the closure.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "bsx_table_host.h"

namespace bsx {

int EdgeSink::prepare(bsx_handle h, const TransPlan& plan, bool want_exits) {
    const uint64_t exit_cells = plan.row_first.size() * h->n_nodes;
    HIPCHK(h, d_row_first.upload(plan.row_first));
    HIPCHK(h, d_free.upload(plan.free_nodes));
    HIPCHK(h, d_edges.alloc(plan.sz.edge_slots));
    HIPCHK(h, d_out.alloc(plan.sz.out_cap));
    HIPCHK(h, d_tc.alloc(1));
    if (want_exits) HIPCHK(h, d_exits.alloc(exit_cells));
    tc = trans_ctr_initial();
    HIPCHK(h, hipMemcpyAsync(d_tc.p, &tc, sizeof(tc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_edges.p, 0, plan.sz.edge_slots * sizeof(TransEdgeSlot), h->stream));
    if (want_exits) HIPCHK(h, hipMemsetAsync(d_exits.p, 0, exit_cells * sizeof(uint32_t), h->stream));
    return BSX_OK;
}

int EdgeSink::drain(bsx_handle h, const TransPlan& plan) {
    HIPCHK(h, launch_trans_drain(d_edges.p, plan.sz.edge_slots, d_out.p, plan.sz.out_cap, d_tc.p, h->stream));
    return BSX_OK;
}

int EdgeSink::finish(bsx_handle h, const std::string& who, const ProfileDev& prof, const TransOut& out, uint64_t* sum_mu) {
    std::string text;
    if (const int status = trans_status(table_family(h), tc, out.edge_cap, text)) return fail(h, status, who + ": " + text);
    std::vector<TransEdge> got(tc.n_edges);
    if (tc.n_edges) HIPCHK(h, hipMemcpy(got.data(), d_out.p, tc.n_edges * sizeof(TransEdge), hipMemcpyDeviceToHost));
    *sum_mu = trans_finish_edges(got, out.edges);
    *out.n_edges = tc.n_edges;
    // (n > 0 rows: the buffers hold exactly [n][n_nodes] cells and [n] flags)
    if (out.node_exits) HIPCHK(h, hipMemcpy(out.node_exits, d_exits.p, d_exits.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out.closed) HIPCHK(h, hipMemcpy(out.closed, prof.closed.p, prof.closed.n, hipMemcpyDeviceToHost));
    return BSX_OK;
}

}  // namespace bsx
