// Every environment variable the library reads, in one place.  Knobs::from_env() is called at the start of the ABI
// entry points (bsx_create, bsx_set_network and every bsx_run_*) and the result kept on the handle: a caller may
// change the environment between two calls on one live handle.  None of these changes a result; they pick code paths
// (A/B runs, tests), tune, or print.  No HIP here.
#pragma once
#include <cstdint>

namespace bsx {

struct Knobs {
    bool debug = false;             // BSX_DEBUG (set): one line per pass / cube level / chain on stderr
    bool profile = false;           // BSX_PROFILE (set): host time per section of an attract call on stderr
    bool cycle_cache = true;        // BSX_CYCLE_CACHE=0: no cycle-state cache (read by bsx_create only)
    uint64_t cache_lds_kb = 0;      // BSX_CACHE_LDS_KB: LDS budget of the cache mirror, at least 1 (0 = not set)
    int lut_mode = -1;              // BSX_LUT_MODE=0|2: force a smaller-footprint gather table (-1 = not set)
    bool lean = true;               // BSX_LEAN=0: the general kernel alone
    int merge = 2;                  // BSX_MERGE: 2 class-pool kernel, 1 lean kernel with sibling merge, 0 without
    bool force_counting = false;    // BSX_FORCE_COUNTING (set): member counts on probe tiles too
    uint32_t service_lanes = 0;     // BSX_SERVICE_LANES: lean kernel's service-lane override (0 = default)
    uint32_t chunk = 0;             // BSX_CHUNK: problems per dequeue, at least 64 (0 = not set)
    bool mirror_image = true;       // BSX_MIRROR_IMAGE=0: every workgroup regenerates the cache mirror
    bool spin_wait = true;          // BSX_SPIN_WAIT=0: copy + hipStreamSynchronize instead of k_publish and the spin
    bool fgraph = false;            // BSX_FGRAPH=1: route eligible bsx_run_attract calls through the functional-graph mode
    bool cubes = true;              // BSX_CUBES=0: no cube collapse (attract and target summary)
    bool cube_order = true;         // BSX_CUBE_ORDER=0: relevant digits stay in ascending order
    bool cube_order_tails = true;   // BSX_CUBE_ORDER_TAILS=0: a batch's chains stay in block order
    bool cube_lower = true;         // BSX_CUBE_LOWER=0: lower levels run the full build of the pool kernel
    bool cube_leaf = true;          // BSX_CUBE_LEAF=0: depth 1 per child, never per parent
    uint32_t cube_depth = 0;        // BSX_CUBE_DEPTH: deepest top level, 1 .. kMaxCubeLevels; set = "fewest digits" rule (0 = not set)
    uint64_t cube_near_cap = 0;     // BSX_CUBE_NEAR_CAP: classes per hand-over segment, at least 1 (0 = not set)
    int cube_streams = 0;           // BSX_CUBE_STREAMS: side streams of a batch, 1 .. kSideStreams (default: all)
    int cube_top_streams = 2;       // BSX_CUBE_TOP_STREAMS=1: every top on the handle's stream (default 2: the tops of consecutive chains
                                    // alternate between two streams; needs side streams, so BSX_CUBE_STREAMS=1 implies 1)
    int cube_split = -1;            // BSX_CUBE_SPLIT: 0 no sub-blocks, 1 split whatever the size (-1 = the estimate decides)
    int sliced = -1;                // BSX_SLICED: 0 per-lane simulate kernel, 1 first-generation sliced kernel (-1 = by shape)
    bool wide = false;              // BSX_WIDE=1: the wide-state family for every network
    bool wide_host_reduce = false;  // BSX_WIDE_HOST_REDUCE=1: wide results reduced on the host, chunk by chunk
    bool wide_chunk_set = false;    // BSX_WIDE_CHUNK (not empty): problems per k_wide launch of a chunked run,
    uint64_t wide_chunk = 0;        // ... clamped where it is used (the lower bound depends on the network)
    uint32_t wide_step_limit = 0;   // BSX_WIDE_STEP_LIMIT: 16 .. kWideStepLimit (default: kWideStepLimit)
    uint64_t corr_batch_cells = 0;  // BSX_CORR_BATCH_CELLS: cells (columns x attractors) per sort batch of the node correlations (0 = not set)
    uint32_t trans_step_limit = 0;  // BSX_TRANS_STEP_LIMIT: 1 .. kStepLimit, per walk of the attractor transitions (default: kStepLimit)
    uint64_t wtrans_chunk = 0;      // BSX_WTRANS_CHUNK: flips per launch of the wide attractor transitions, at least 1 (0 = not set)

    static Knobs from_env();
};

}  // namespace bsx
