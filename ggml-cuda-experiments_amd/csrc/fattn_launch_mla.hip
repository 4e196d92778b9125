// fattn_launch_mla.hip -- the MLA kernels (fattn_mla.h: K dim 576, V dim 512,
// f16), instantiated once: V as a view of K or of its own, with and without a mask.
#include "fattn_launch.h"

namespace fattn {

namespace {

// (one instantiation per kernel: launch_kernel caches the LDS attribute per launch site)
template <bool VOWN, bool HM, typename A>
int launch_mla_a(const Plan& pl, hipStream_t st, const Events& ev) {
    auto kern = fattn_mla_kernel<VOWN, HM, FATTN_TYPE_F16, false, A>;
    MlaArgsT<A> ma;
    ma.a = launch_args<A>(pl);
    ma.v_off = VOWN ? 0 : pl.mla_v_off;
    ma.raw16 = 0;
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(kMlaWaves * kWave), pl.lds, st, ma);
        if (pl.a.merge_launch == 1) launch_chunk_merge<MlaMergeGeom, kMlaDV>(dim3(kMlaRows / 4, pl.grid.y, pl.grid.z), pl, st);
    });
}
template <bool VOWN, bool HM>
int launch_mla_form(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_mla_a<VOWN, HM, typename decltype(tag)::type>(pl, st, ev); });
}

}  // namespace

int launch_mla(const Plan& pl, hipStream_t st, const Events& ev) {
    if (pl.kt != FATTN_TYPE_F16) return launch_mla_q(pl, st, ev);
    if (pl.mla_v_off < 0)
        return pl.a.has_mask ? launch_mla_form<true, true>(pl, st, ev) : launch_mla_form<true, false>(pl, st, ev);
    return pl.a.has_mask ? launch_mla_form<false, true>(pl, st, ev) : launch_mla_form<false, false>(pl, st, ev);
}
template <bool VOWN, bool HM>
int launch_mla_form(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_mla_a<VOWN, HM, typename decltype(tag)::type>(pl, st, ev); });
}

}  // namespace fattn
