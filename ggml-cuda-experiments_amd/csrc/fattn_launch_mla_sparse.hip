// fattn_launch_mla_sparse.hip -- the MLA kernel (fattn_mla.h) in its gathered
// form, fattn_ext_sparse: the tile walk runs over the query row's slot list.
// F16 (V a view of K, or of its own) and Q8_0 / Q4_0 (V a view of K; all four
// waves alike, or SOLO), each with and without the rows' log-sum-exp.  No mask.
#include "fattn_plan.h"

namespace fattn {

namespace {

// (one instantiation per kernel: launch_kernel caches the LDS attribute per launch site)
template <bool VOWN, int KT, bool SOLO, typename A>
int launch_mla_sparse_a(const Plan& pl, const SparseIdx& sx, hipStream_t st) {
    auto kern = fattn_mla_kernel<VOWN, false, KT, SOLO, A, true>;
    MlaSparseArgsT<A> ma;
    ma.a = launch_args<A>(pl);
    // (quantised: V starts b whole blocks into K's rows, 64 b bytes into the image's)
    if constexpr (KT != FATTN_TYPE_F16) ma.v_off = pl.mla_v_off / TypeInfo<KT>::block_bytes * (QK * 2);
    else ma.v_off = VOWN ? 0 : pl.mla_v_off;
    ma.raw16 = 0;
    ma.idx = sx.data;
    ma.i_nb1 = sx.nb1, ma.i_nb2 = sx.nb2, ma.i_nb3 = sx.nb3;
    ma.i_ne2 = sx.ne2, ma.i_ne3 = sx.ne3;
    ma.n_kv = sx.n_kv;
    return launch_kernel((const void*)kern, pl, st, Events(), [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(kMlaWaves * kWave), pl.lds, st, ma);
        if (pl.a.merge_launch == 1) launch_chunk_merge<MlaMergeGeom, kMlaDV>(dim3(kMlaRows / 4, pl.grid.y, pl.grid.z), pl, st);
    });
}
template <bool VOWN, int KT, bool SOLO>
int launch_mla_sparse_form(const Plan& pl, const SparseIdx& sx, hipStream_t st) {
    return with_args(pl, [&](auto tag) { return launch_mla_sparse_a<VOWN, KT, SOLO, typename decltype(tag)::type>(pl, sx, st); });
}

}  // namespace

int launch_mla_sparse(const Plan& pl, const SparseIdx& sx, hipStream_t st) {
    if (pl.kt == FATTN_TYPE_F16)
        return pl.mla_v_off < 0 ? launch_mla_sparse_form<true, FATTN_TYPE_F16, false>(pl, sx, st)
                                : launch_mla_sparse_form<false, FATTN_TYPE_F16, false>(pl, sx, st);
    return visit(QuantTypes(), pl.kt, (int)FATTN_ERR_UNSUPPORTED_TYPE, [&](auto k) {
        constexpr int KT = decltype(k)::value;
        return pl.mla_solo ? launch_mla_sparse_form<false, KT, true>(pl, sx, st) : launch_mla_sparse_form<false, KT, false>(pl, sx, st);
    });
}

}  // namespace fattn
