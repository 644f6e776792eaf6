// Knobs::from_env: the library's only reader of the environment (bsx_knobs.h lists the variables).
#include "bsx_knobs.h"

#include <algorithm>
#include <cstdlib>

#include "bsx_device.h"
#include "bsx_wide.h"

namespace bsx {

Knobs Knobs::from_env() {
    auto is_set = [](const char* name) { return std::getenv(name) != nullptr; };
    auto starts_with = [](const char* name, char c) { const char* e = std::getenv(name); return e && e[0] == c; };
    // "0" / "1" by the first character, anything else (or unset): -1
    auto zero_or_one = [&](const char* name) { return starts_with(name, '0') ? 0 : starts_with(name, '1') ? 1 : -1; };
    Knobs k;
    k.debug = is_set("BSX_DEBUG");
    k.profile = is_set("BSX_PROFILE");
    k.cycle_cache = !starts_with("BSX_CYCLE_CACHE", '0');
    if (const char* e = std::getenv("BSX_CACHE_LDS_KB")) k.cache_lds_kb = std::max<size_t>(1, (size_t)std::atoi(e));
    if (const char* e = std::getenv("BSX_LUT_MODE")) k.lut_mode = std::atoi(e);
    if (const char* e = std::getenv("BSX_LEAN")) k.lean = std::atoi(e) != 0;
    if (const char* e = std::getenv("BSX_MERGE")) k.merge = std::atoi(e);
    k.force_counting = is_set("BSX_FORCE_COUNTING");
    if (const char* e = std::getenv("BSX_SERVICE_LANES")) k.service_lanes = (uint32_t)std::atoi(e);
    if (const char* e = std::getenv("BSX_CHUNK")) k.chunk = (uint32_t)std::max(64, std::atoi(e));
    k.mirror_image = !starts_with("BSX_MIRROR_IMAGE", '0');
    k.spin_wait = !starts_with("BSX_SPIN_WAIT", '0');
    k.fgraph = starts_with("BSX_FGRAPH", '1');
    k.cubes = !starts_with("BSX_CUBES", '0');
    k.cube_order = !starts_with("BSX_CUBE_ORDER", '0');
    k.cube_order_tails = !starts_with("BSX_CUBE_ORDER_TAILS", '0');
    k.cube_lower = !starts_with("BSX_CUBE_LOWER", '0');
    k.cube_leaf = !starts_with("BSX_CUBE_LEAF", '0');
    if (const char* e = std::getenv("BSX_CUBE_DEPTH")) k.cube_depth = (uint32_t)std::max(1, std::min((int)kMaxCubeLevels, std::atoi(e)));
    if (const char* e = std::getenv("BSX_CUBE_NEAR_CAP")) k.cube_near_cap = (uint64_t)std::max(1, std::atoi(e));
    const char* streams = std::getenv("BSX_CUBE_STREAMS");
    k.cube_streams = std::max(1, std::min((int)kSideStreams, streams ? std::atoi(streams) : (int)kSideStreams));
    k.cube_top_streams = starts_with("BSX_CUBE_TOP_STREAMS", '1') ? 1 : 2;
    k.cube_split = zero_or_one("BSX_CUBE_SPLIT");
    k.sliced = zero_or_one("BSX_SLICED");
    k.wide = starts_with("BSX_WIDE", '1');
    k.wide_host_reduce = starts_with("BSX_WIDE_HOST_REDUCE", '1');
    if (const char* e = std::getenv("BSX_WIDE_CHUNK")) if (e[0]) { k.wide_chunk_set = true; k.wide_chunk = std::strtoull(e, nullptr, 10); }
    k.wide_step_limit = kWideStepLimit;
    if (const char* e = std::getenv("BSX_WIDE_STEP_LIMIT")) k.wide_step_limit = std::max(16u, std::min(kWideStepLimit, (uint32_t)std::atoi(e)));
    if (const char* e = std::getenv("BSX_CORR_BATCH_CELLS")) k.corr_batch_cells = std::strtoull(e, nullptr, 10);
    k.trans_step_limit = kStepLimit;
    if (const char* e = std::getenv("BSX_TRANS_STEP_LIMIT")) k.trans_step_limit = std::max(1u, std::min(kStepLimit, (uint32_t)std::atoi(e)));
    if (const char* e = std::getenv("BSX_WTRANS_CHUNK")) k.wtrans_chunk = std::max(1ull, std::strtoull(e, nullptr, 10));
    return k;
}

}  // namespace bsx
