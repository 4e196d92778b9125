// fattn_launch_kv_ext.hip -- the prefill pre-pass over a Q4_1 / Q5_0 / Q5_1 / IQ4_NL cache
// (fattn_launch.h launch_prepass_kv_ext): its rows staged to f16 for the f16
// prefill bodies, in a translation unit of its own.
#include "fattn_launch.h"

namespace fattn {
void launch_prepass_kv_ext(int stage_kt, dim3 grid, hipStream_t st, const PfPrepassArgs& pa) {
    if (is_codebook(stage_kt)) return iq4nl_launch_prepass(grid, st, pa);  // (fattn_launch_iq4_nl_conv.hip)
    launch_prepass(ValueList<FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>(), stage_kt, grid, st, pa);
}
}  // namespace fattn
