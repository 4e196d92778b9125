// fattn_launch_bf16_d256.hip -- the head-dim-256 split kernels over a BF16 K / V
// cache (fattn_launch.h launch_bf16), in their own translation unit so they
// build in parallel with the others.
#include "fattn_launch.h"

namespace fattn {
template int launch_bf16<256>(const Plan&, hipStream_t, const Events&);
}  // namespace fattn
