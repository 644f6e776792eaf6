// k_trans_walk (bsx_trans_kernel.h) for 8-word states
#include "bsx_trans_kernel.h"
namespace bsx { BSX_TRANS_WALK_UNIT(8) }
