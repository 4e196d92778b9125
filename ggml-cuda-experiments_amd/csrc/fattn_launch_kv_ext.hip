// fattn_launch_kv_ext.hip -- the prefill pre-pass over a Q4_1 / Q5_0 / Q5_1 cache
// (fattn_launch.h launch_prepass_kv_ext): its rows staged to f16 for the f16
// prefill bodies, in a translation unit of its own.
#include "fattn_launch.h"

namespace fattn {
void launch_prepass_kv_ext(int stage_kt, dim3 grid, hipStream_t st, const PfPrepassArgs& pa) {
    if (stage_kt == FATTN_TYPE_Q4_1) hipLaunchKernelGGL(pf_prepass_kernel<FATTN_TYPE_Q4_1>, grid, dim3(256), 0, st, pa);
    else if (stage_kt == FATTN_TYPE_Q5_0) hipLaunchKernelGGL(pf_prepass_kernel<FATTN_TYPE_Q5_0>, grid, dim3(256), 0, st, pa);
    else hipLaunchKernelGGL(pf_prepass_kernel<FATTN_TYPE_Q5_1>, grid, dim3(256), 0, st, pa);
}
}  // namespace fattn
