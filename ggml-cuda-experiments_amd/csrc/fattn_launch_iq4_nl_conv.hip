// fattn_launch_iq4_nl_conv.hip -- the IQ4_NL instantiations of the conversion,
// cache-write, K-shift and prefill-staging kernels (fattn_quant.h, fattn_set_rows.h,
// fattn_k_shift.h, fattn_pf.h), launched from the units that dispatch on the type.
// A translation unit of their own: like the type's split kernels it is built
// without the packed-f32 VALU forms (Makefile NOPK_UNITS), and the other types'
// kernels keep the flags they had.
#include "fattn_k_shift.h"
#include "fattn_pf.h"

namespace fattn {
constexpr int T = FATTN_TYPE_IQ4_NL;

void iq4nl_launch_dequant(dim3 grid, hipStream_t st, const uint8_t* src, float* dst, int64_t nblocks) {
    hipLaunchKernelGGL(dequant_kernel<T>, grid, dim3(256), 0, st, src, dst, nblocks);
}
void iq4nl_launch_quant(dim3 grid, hipStream_t st, const float* src, uint8_t* dst, int64_t nblocks) {
    hipLaunchKernelGGL(quant_kernel<T>, grid, dim3(256), 0, st, src, dst, nblocks);
}
void iq4nl_launch_cpy(dim3 grid, hipStream_t st, const CpyArgs& a, int64_t units) {
    hipLaunchKernelGGL(cpy_f32_kernel<T>, grid, dim3(256), 0, st, a, units);
}
void iq4nl_launch_set_rows(bool vec, bool unroll, dim3 grid, hipStream_t st, const SetRowsArgs& a) {
    void (*kern)(SetRowsArgs) = unroll ? (vec ? set_rows_kernel<T, true, kSetRowsUnroll> : set_rows_kernel<T, false, kSetRowsUnroll>)
                                       : (vec ? set_rows_kernel<T, true, 1> : set_rows_kernel<T, false, 1>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a);
}
void iq4nl_launch_k_shift(bool neox, dim3 grid, hipStream_t st, const KShiftArgs& a) {
    void (*kern)(KShiftArgs) = neox ? k_shift_kernel<T, true, false> : k_shift_kernel<T, false, false>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, a);
}
void iq4nl_launch_prepass(dim3 grid, hipStream_t st, const PfPrepassArgs& pa) {
    hipLaunchKernelGGL(pf_prepass_kernel<T>, grid, dim3(256), 0, st, pa);
}
}  // namespace fattn
