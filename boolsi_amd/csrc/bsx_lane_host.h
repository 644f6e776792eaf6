// Private to the host files of the per-lane family's target and simulate modes (bsx_target_api.cpp: bsx_run_target,
// bsx_run_target_summary; bsx_simulate_api.cpp: bsx_run_simulate, bsx_run_trajectories): the one timed launch they share.
// What they upload and the shapes they launch come from bsx_lane_lower.h.
#pragma once
#include "bsx_engine.h"
#include "bsx_host.h"
#include "bsx_lane_lower.h"

namespace bsx {

// One timed launch on the handle's stream: zeroes d_ctr, records ev0, runs `launch` (-> a status: it enqueues on
// h->stream with P.ctr = h->d_ctr), records ev1, brings the counters back, waits, reads the device time.
template <typename Launch>
inline int lane_timed_launch(bsx_handle h, Counters& ctr, float& ms, Launch&& launch) {
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, sizeof(Counters), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = launch()) return rc;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(&ctr, h->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    return BSX_OK;
}

}  // namespace bsx
