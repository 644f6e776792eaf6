// What a lowering unit (bsx_lane_lower.h, bsx_wide_lower.h, bsx_table_lower.h) answers when it refuses its input.  No HIP here.
#pragma once
#include "bsx.h"

namespace bsx {

struct LowerStatus {        // BSX_OK, or the status and the text for bsx_last_error
    int status = BSX_OK;
    const char* msg = "";
    explicit operator bool() const { return status != BSX_OK; }
};

}  // namespace bsx
