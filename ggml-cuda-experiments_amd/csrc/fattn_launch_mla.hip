// fattn_launch_mla.hip -- the MLA kernels (fattn_mla.h: K dim 576, V dim 512,
// f16), instantiated once: V as a view of K or of its own, with and without a mask.
#include "fattn_launch.h"

namespace fattn {

namespace {

// (one instantiation per kernel: launch_kernel caches the LDS attribute per launch site)
template <bool VOWN, bool HM>
int launch_mla_form(const Plan& pl, hipStream_t st, const Events& ev) {
    auto kern = fattn_mla_kernel<VOWN, HM>;
    MlaArgs ma;
    ma.a = pl.a;
    ma.v_off = VOWN ? 0 : pl.mla_v_off;
    ma.raw16 = 0;
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(kMlaWaves * kWave), pl.lds, st, ma);
        if (pl.a.merge_launch == 1) launch_mla_merge(pl, st);
    });
}

}  // namespace

// one wave per packed row; as few load slots per lane as the chunks need
void launch_mla_merge(const Plan& pl, hipStream_t st) {
    const dim3 grid(kMlaRows / 4, pl.grid.y, pl.grid.z);
    if (pl.a.n_chunks <= 4) hipLaunchKernelGGL(fattn_mla_merge_kernel<4>, grid, dim3(256), 0, st, pl.a);
    else if (pl.a.n_chunks <= 8) hipLaunchKernelGGL(fattn_mla_merge_kernel<8>, grid, dim3(256), 0, st, pl.a);
    else hipLaunchKernelGGL(fattn_mla_merge_kernel<16>, grid, dim3(256), 0, st, pl.a);
}

int launch_mla(const Plan& pl, hipStream_t st, const Events& ev) {
    if (pl.kt != FATTN_TYPE_F16) return launch_mla_q(pl, st, ev);
    if (pl.mla_v_off < 0)
        return pl.a.has_mask ? launch_mla_form<true, true>(pl, st, ev) : launch_mla_form<true, false>(pl, st, ev);
    return pl.a.has_mask ? launch_mla_form<false, true>(pl, st, ev) : launch_mla_form<false, false>(pl, st, ev);
}

}  // namespace fattn
