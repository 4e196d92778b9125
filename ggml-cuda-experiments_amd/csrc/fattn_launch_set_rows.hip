// fattn_launch_set_rows.hip -- fattn_set_rows (include/fattn.h): the validation
// of the three views and the instantiations of set_rows_kernel
// (fattn_set_rows.h), in a translation unit of their own.  Nothing allocates;
// nothing synchronises (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fattn_set_rows.h"

using namespace fattn;

namespace {

// Units (32-element blocks) over all planes from which a lane group takes
// kSetRowsUnroll of them: 2^17 units are 4096 workgroups at one unit per group,
// still 1024 -- four per CU of an MI355X -- at four.  Below that the chip is not
// full either way and the launch dominates; one unit per group keeps more
// workgroups in flight there.
constexpr int64_t kUnrollMinUnits = 1 << 17;

template <int T, int K>
void launch_k(bool vec, dim3 grid, hipStream_t st, const SetRowsArgs& a) {
    grid.x = (a.units + 32u * K - 1u) / (32u * K);
    if (vec) hipLaunchKernelGGL((set_rows_kernel<T, true, K>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((set_rows_kernel<T, false, K>), grid, dim3(256), 0, st, a);
}
template <int T>
void launch(bool vec, bool unroll, dim3 grid, hipStream_t st, const SetRowsArgs& a) {
    if (unroll) launch_k<T, kSetRowsUnroll>(vec, grid, st, a);
    else launch_k<T, 1>(vec, grid, st, a);
}

}  // namespace

extern "C" int fattn_set_rows(const fattn_tensor* src, const fattn_tensor* idx, const fattn_tensor* dst, void* stream) {
    if (!src || !idx || !dst || !src->data || !idx->data || !dst->data) return FATTN_ERR_INVALID_ARG;
    if (src->type != FATTN_TYPE_F32) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (idx->type != FATTN_TYPE_I64 && idx->type != FATTN_TYPE_I32) return FATTN_ERR_UNSUPPORTED_TYPE;
    const int t = dst->type;
    if (!in_list(SetRowsTypes(), t)) return FATTN_ERR_UNSUPPORTED_TYPE;
    for (int i = 0; i < 4; i++)
        if (src->ne[i] <= 0 || idx->ne[i] <= 0 || dst->ne[i] <= 0) return FATTN_ERR_INVALID_ARG;
    const int64_t ne0 = src->ne[0], nr = src->ne[1], ne2 = src->ne[2], ne3 = src->ne[3];
    const int64_t ne11 = idx->ne[1], ne12 = idx->ne[2];
    if (dst->ne[0] != ne0 || dst->ne[2] != ne2 || dst->ne[3] != ne3) return FATTN_ERR_INVALID_ARG;
    if (idx->ne[0] != nr || idx->ne[3] != 1 || ne2 % ne11 || ne3 % ne12) return FATTN_ERR_INVALID_ARG;
    const int64_t ue = type_desc(t).block_elems;
    if (ne0 % ue) return FATTN_ERR_INVALID_ARG;
    // units of one [ne0, nr] plane are numbered in 32 bits (one division per thread)
    const int64_t upr = (ne0 + QK - 1) / QK;
    if (upr > INT32_MAX || nr > INT32_MAX / upr) return FATTN_ERR_INVALID_ARG;
    const int64_t es = idx->type == FATTN_TYPE_I64 ? 8 : 4;
    const bool use1 = ne11 > 1, use2 = ne12 > 1;  // idx nb[1] / nb[2] are looked at only then
    if (src->nb[0] != 4 || dst->nb[0] != (int64_t)fattn_row_size(t, ue) || idx->nb[0] < es)
        return FATTN_ERR_BAD_STRIDE;
    if ((use1 && idx->nb[1] < 0) || (use2 && idx->nb[2] < 0)) return FATTN_ERR_BAD_STRIDE;
    if ((uintptr_t)src->data % 4 || src->nb[1] % 4 || src->nb[2] % 4 || src->nb[3] % 4) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)dst->data % 2 || dst->nb[1] % 2 || dst->nb[2] % 2 || dst->nb[3] % 2) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)idx->data % es || idx->nb[0] % es || (use1 && idx->nb[1] % es) || (use2 && idx->nb[2] % es))
        return FATTN_ERR_ALIGNMENT;

    SetRowsArgs a;
    a.src = (const uint8_t*)src->data;
    a.idx = (const uint8_t*)idx->data;
    a.dst = (uint8_t*)dst->data;
    a.ne0 = ne0; a.n_slots = dst->ne[1]; a.ne2 = ne2; a.ne3 = ne3; a.ne11 = ne11; a.ne12 = ne12;
    a.snb1 = src->nb[1]; a.snb2 = src->nb[2]; a.snb3 = src->nb[3];
    a.inb0 = idx->nb[0]; a.inb1 = use1 ? idx->nb[1] : 0; a.inb2 = use2 ? idx->nb[2] : 0;
    a.dnb1 = dst->nb[1]; a.dnb2 = dst->nb[2]; a.dnb3 = dst->nb[3];
    a.upr = (uint32_t)upr;
    a.units = (uint32_t)(upr * nr);
    a.idx64 = idx->type == FATTN_TYPE_I64;
    a.dst_small = a.n_slots < ((int64_t)1 << 32) && a.dnb1 >= 0 && a.dnb1 < ((int64_t)1 << 32);
    const int64_t q32 = 32 / upr;
    a.r32 = (uint32_t)(32 % upr);
    a.ds_next = q32 * a.snb1 + (int64_t)a.r32 * QK * 4;
    a.ds_wrap = a.ds_next + a.snb1 - upr * QK * 4;
    a.di_next = q32 * a.inb0;
    a.di_wrap = a.di_next + a.inb0;
    a.dd_next = a.r32;
    a.dd_wrap = (int64_t)a.r32 - upr;
    // the 16-B source path: every row base a multiple of 16 (strides of a
    // dimension of one element are never multiplied by anything but 0)
    const bool vec = (uintptr_t)src->data % 16 == 0 && (nr == 1 || src->nb[1] % 16 == 0) &&
                     (ne2 == 1 || src->nb[2] % 16 == 0) && (ne3 == 1 || src->nb[3] % 16 == 0);
    const dim3 grid(1, (unsigned)std::min<int64_t>(ne2, 65535), (unsigned)std::min<int64_t>(ne3, 65535));  // x: launch_k
    // (a plane of fewer than 8 workgroups' worth of units is not worth the idle passes of its last workgroup)
    const bool unroll = a.units >= 8 * 32 * kSetRowsUnroll && (double)a.units * (double)ne2 * (double)ne3 >= (double)kUnrollMinUnits;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    visit(SetRowsTypes(), t, 0, [&](auto tc) {
        launch<decltype(tc)::value>(vec, unroll, grid, st, a);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}
