// fattn_launch_k_shift.hip -- fattn_k_shift (include/fattn.h): the validation of
// the cache view, the shift tensor and the rope parameters, and the
// instantiations of k_shift_kernel (fattn_k_shift.h), in a translation unit of
// their own.  Nothing allocates; nothing synchronises (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fattn_k_shift.h"

using namespace fattn;

namespace {

template <int T, bool NEOX>
void launch(bool vec, dim3 grid, hipStream_t st, const KShiftArgs& a) {
    if constexpr (is_quant(T)) {
        hipLaunchKernelGGL((k_shift_kernel<T, NEOX, false>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_shift_kernel<T, NEOX, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_shift_kernel<T, NEOX, false>), grid, dim3(256), 0, st, a);
    }
}

bool finite_pos(float x) { return std::isfinite(x) && x > 0.0f; }

// ggml_rope_yarn_corr_dim, in f32
float corr_dim(int n_dims, int n_ctx_orig, float n_rot, float base) {
    return (float)n_dims * logf((float)n_ctx_orig / (n_rot * 2.0f * 3.14159265358979323846f)) / (2.0f * logf(base));
}

}  // namespace

extern "C" int fattn_k_shift(const fattn_tensor* k, const fattn_tensor* shift, const float* freq_factors,
                             const fattn_rope* rope, void* stream) {
    if (!k || !shift || !rope || !k->data || !shift->data) return FATTN_ERR_INVALID_ARG;
    const int t = k->type;
    if (!in_list(KShiftTypes(), t)) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (shift->type != FATTN_TYPE_I32) return FATTN_ERR_UNSUPPORTED_TYPE;
    for (int i = 0; i < 4; i++)
        if (k->ne[i] <= 0 || shift->ne[i] <= 0) return FATTN_ERR_INVALID_ARG;
    const int64_t ne0 = k->ne[0], n_slots = k->ne[1], ne2 = k->ne[2], ne3 = k->ne[3], ns = shift->ne[1];
    if (shift->ne[0] != n_slots || ne3 % ns || shift->ne[2] != 1 || shift->ne[3] != 1) return FATTN_ERR_INVALID_ARG;
    const TypeDesc td = type_desc(KShiftTypes(), t);
    const bool block = td.block_elems == QK;
    if (ne0 % (block ? QK : 4)) return FATTN_ERR_INVALID_ARG;
    if (ne0 > 256) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    const fattn_rope& r = *rope;
    if (r.n_dims < 8 || r.n_dims > ne0 || r.n_dims % 8) return FATTN_ERR_INVALID_ARG;
    if (r.mode != 0 && r.mode != 2) return FATTN_ERR_INVALID_ARG;
    if (!finite_pos(r.freq_base) || !finite_pos(r.freq_scale)) return FATTN_ERR_INVALID_ARG;
    if (!std::isfinite(r.ext_factor) || r.ext_factor < 0.0f) return FATTN_ERR_INVALID_ARG;
    if (!std::isfinite(r.attn_factor) || !std::isfinite(r.beta_fast) || !std::isfinite(r.beta_slow)) return FATTN_ERR_INVALID_ARG;
    if (r.ext_factor != 0.0f && r.n_ctx_orig <= 0) return FATTN_ERR_INVALID_ARG;
    // a row never leaves its wave: upr <= 8 lane groups; the waves of one plane are numbered in 32 bits
    const int64_t upr = (ne0 + QK - 1) / QK;
    if (n_slots > INT32_MAX / upr || ne2 > INT32_MAX || ne3 > INT32_MAX) return FATTN_ERR_INVALID_ARG;
    const bool use1 = ns > 1;  // shift nb[1] is looked at only then
    if (k->nb[0] != td.block_bytes || shift->nb[0] < 4 || (use1 && shift->nb[1] < 0)) return FATTN_ERR_BAD_STRIDE;
    const int ka = t == FATTN_TYPE_F32 ? 4 : 2;
    if ((uintptr_t)k->data % ka || k->nb[1] % ka || k->nb[2] % ka || k->nb[3] % ka) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)shift->data % 4 || shift->nb[0] % 4 || (use1 && shift->nb[1] % 4)) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)freq_factors % 4) return FATTN_ERR_ALIGNMENT;

    KShiftArgs a;
    a.k = (uint8_t*)k->data;
    a.shift = (const uint8_t*)shift->data;
    a.ff = freq_factors;
    a.knb1 = k->nb[1]; a.knb2 = k->nb[2]; a.knb3 = k->nb[3];
    a.snb0 = shift->nb[0]; a.snb1 = use1 ? shift->nb[1] : 0;
    a.n_slots = n_slots;
    a.ne2 = (int32_t)ne2; a.ne3 = (int32_t)ne3; a.ns = (int32_t)ns;  // (ns <= ne3)
    a.upr = (uint32_t)upr;
    a.rpw = (uint32_t)(8 / upr);
    a.n_dims = r.n_dims;
    a.theta_scale = powf(r.freq_base, -2.0f / (float)r.n_dims);
    a.freq_scale = r.freq_scale;
    a.ext_factor = r.ext_factor;
    a.m = r.attn_factor;
    a.lo = 0.0f;
    a.den = 1.0f;
    if (r.ext_factor != 0.0f) {
        const float lo = std::max(0.0f, floorf(corr_dim(r.n_dims, r.n_ctx_orig, r.beta_fast, r.freq_base)));
        const float hi = std::min((float)(r.n_dims - 1), ceilf(corr_dim(r.n_dims, r.n_ctx_orig, r.beta_slow, r.freq_base)));
        a.lo = lo;
        a.den = std::max(0.001f, hi - lo);
        a.m = r.attn_factor * (1.0f + 0.1f * logf(1.0f / r.freq_scale));
    }
    // the 16-B (F32) / 8-B (F16, BF16) path: every row base such a multiple (strides
    // of a dimension of one element are never multiplied by anything but 0)
    const int va = t == FATTN_TYPE_F32 ? 16 : 8;
    const bool vec = !block && (uintptr_t)k->data % va == 0 && (n_slots == 1 || k->nb[1] % va == 0) &&
                     (ne2 == 1 || k->nb[2] % va == 0) && (ne3 == 1 || k->nb[3] % va == 0);
    const int64_t waves = (n_slots + a.rpw - 1) / a.rpw;
    const int64_t gz = std::min<int64_t>(ne3, 65535);
    // heads: all walked by one lane group once the other two grid dims fill the chip, spread over y below that
    const int64_t gy = std::min<int64_t>(std::min<int64_t>(ne2, 65535), std::max<int64_t>(1, (kKShiftFullWaves + waves * gz - 1) / (waves * gz)));
    const dim3 grid((unsigned)((waves + 3) / 4), (unsigned)gy, (unsigned)gz);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    visit(KShiftTypes(), t, 0, [&](auto tc) {
        if (r.mode == 2) launch<decltype(tc)::value, true>(vec, grid, st, a);
        else launch<decltype(tc)::value, false>(vec, grid, st, a);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}
