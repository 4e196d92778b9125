// fattn_launch_q4_1_d256.hip -- the head-dim-256 split kernels over a Q4_1 K / V
// cache (fattn_launch.h launch_kv_ext), in their own translation unit so they
// build in parallel with the others.
#include "fattn_launch.h"

namespace fattn {
template int launch_kv_ext<FATTN_TYPE_Q4_1, 256>(const Plan&, hipStream_t, const Events&);
}  // namespace fattn
