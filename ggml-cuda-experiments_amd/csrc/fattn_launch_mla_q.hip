// fattn_launch_mla_q.hip -- the MLA kernel (fattn_mla.h) over a Q8_0 / Q4_0
// cache whose V is a view of K: raw tiles by dword LDS-DMA, converted once per
// tile into the f16 image the f16 form loads.  With and without a mask.
#include "fattn_launch.h"

namespace fattn {

namespace {

// (one instantiation per kernel: launch_kernel caches the LDS attribute per launch site)
template <int KT, bool HM, bool SOLO, typename A>
int launch_mla_q_a(const Plan& pl, hipStream_t st, const Events& ev) {
    auto kern = fattn_mla_kernel<false, HM, KT, SOLO, A>;
    MlaArgsT<A> ma;
    ma.a = launch_args<A>(pl);
    // V starts b whole blocks into K's rows: 64 b bytes into the image's rows
    ma.v_off = pl.mla_v_off / TypeInfo<KT>::block_bytes * (QK * 2);
    ma.raw16 = SOLO && pl.mla_raw16;
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(kMlaWaves * kWave), pl.lds, st, ma);
        if (pl.a.merge_launch == 1) launch_chunk_merge<MlaMergeGeom, kMlaDV>(dim3(kMlaRows / 4, pl.grid.y, pl.grid.z), pl, st);
    });
}
template <int KT, bool HM, bool SOLO>
int launch_mla_q_form(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_mla_q_a<KT, HM, SOLO, typename decltype(tag)::type>(pl, st, ev); });
}

template <int KT>
int launch_mla_q_type(const Plan& pl, hipStream_t st, const Events& ev) {
    const bool solo = pl.mla_solo;
    if (solo) return pl.a.has_mask ? launch_mla_q_form<KT, true, true>(pl, st, ev) : launch_mla_q_form<KT, false, true>(pl, st, ev);
    return pl.a.has_mask ? launch_mla_q_form<KT, true, false>(pl, st, ev) : launch_mla_q_form<KT, false, false>(pl, st, ev);
}

}  // namespace

int launch_mla_q(const Plan& pl, hipStream_t st, const Events& ev) {
    return visit(QuantTypes(), pl.kt, (int)FATTN_ERR_UNSUPPORTED_TYPE, [&](auto k) { return launch_mla_q_type<decltype(k)::value>(pl, st, ev); });
}

}  // namespace fattn
