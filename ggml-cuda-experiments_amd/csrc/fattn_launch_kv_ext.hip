// fattn_launch_kv_ext.hip -- the prefill pre-pass over a Q4_1 / Q5_0 / Q5_1 cache
// (fattn_launch.h launch_prepass_kv_ext): its rows staged to f16 for the f16
// prefill bodies, in a translation unit of its own.
#include "fattn_launch.h"

namespace fattn {
void launch_prepass_kv_ext(int stage_kt, dim3 grid, hipStream_t st, const PfPrepassArgs& pa) {
    launch_prepass(ExtTypes(), stage_kt, grid, st, pa);
}
}  // namespace fattn
