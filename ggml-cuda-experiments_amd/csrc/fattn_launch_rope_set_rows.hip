// fattn_launch_rope_set_rows.hip -- fattn_rope_set_rows (include/fattn.h): the
// validation of the views and the rope parameters, and the instantiations of
// rope_set_rows_kernel (fattn_rope_set_rows.h), in a translation unit of their
// own.  The unit holds set_rows_block<IQ4_NL> and is therefore built without the
// packed-f32 VALU forms (Makefile NOPK_UNITS).  Nothing allocates; nothing
// synchronises (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fattn_rope_set_rows.h"

using namespace fattn;

namespace {

// fattn_set_rows' threshold: units over all planes (of both parts) from which a
// lane group takes kSetRowsUnroll of them, every part with at least
// kUnrollMinPlane units in a plane
constexpr int64_t kUnrollMinUnits = 1 << 17;
constexpr int64_t kUnrollMinPlane = 8 * 32 * kSetRowsUnroll;

using DstTypes = RowTypes;  // F32 / F16 / BF16 and the six block types

bool finite_pos(float x) { return std::isfinite(x) && x > 0.0f; }

// ggml_rope_yarn_corr_dim, in f32
float corr_dim(int n_dims, int n_ctx_orig, float n_rot, float base) {
    return (float)n_dims * logf((float)n_ctx_orig / (n_rot * 2.0f * 3.14159265358979323846f)) / (2.0f * logf(base));
}

// One part (src, idx, dst) under fattn_set_rows' rules, BF16 and F32 dst
// included; rope: the row limits of a rotated part.  Fills a, bb, vec.
int check_part(const fattn_tensor* src, const fattn_tensor* idx, const fattn_tensor* dst, bool rope, SetRowsArgs& a, int& bb,
               bool& vec) {
    if (!src->data || !dst->data) return FATTN_ERR_INVALID_ARG;
    if (src->type != FATTN_TYPE_F32) return FATTN_ERR_UNSUPPORTED_TYPE;
    const int t = dst->type;
    if (!in_list(DstTypes(), t)) return FATTN_ERR_UNSUPPORTED_TYPE;
    for (int i = 0; i < 4; i++)
        if (src->ne[i] <= 0 || dst->ne[i] <= 0) return FATTN_ERR_INVALID_ARG;
    const int64_t ne0 = src->ne[0], nr = src->ne[1], ne2 = src->ne[2], ne3 = src->ne[3];
    const int64_t ne11 = idx->ne[1], ne12 = idx->ne[2];
    if (dst->ne[0] != ne0 || dst->ne[2] != ne2 || dst->ne[3] != ne3) return FATTN_ERR_INVALID_ARG;
    if (idx->ne[0] != nr || ne2 % ne11 || ne3 % ne12) return FATTN_ERR_INVALID_ARG;
    const TypeDesc td = type_desc(DstTypes(), t);
    const bool block = td.block_elems == QK;
    if (ne0 % (block ? QK : rope ? 4 : 1)) return FATTN_ERR_INVALID_ARG;
    if (rope && ne0 > 256) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    // units of one [ne0, nr] plane are numbered in 32 bits
    const int64_t upr = (ne0 + QK - 1) / QK;
    if (upr > INT32_MAX || nr > INT32_MAX / upr) return FATTN_ERR_INVALID_ARG;
    if (src->nb[0] != 4 || dst->nb[0] != td.block_bytes) return FATTN_ERR_BAD_STRIDE;
    if ((uintptr_t)src->data % 4 || src->nb[1] % 4 || src->nb[2] % 4 || src->nb[3] % 4) return FATTN_ERR_ALIGNMENT;
    const int da = t == FATTN_TYPE_F32 ? 4 : 2;
    if ((uintptr_t)dst->data % da || dst->nb[1] % da || dst->nb[2] % da || dst->nb[3] % da) return FATTN_ERR_ALIGNMENT;

    bb = block ? td.block_bytes : QK * td.block_bytes;
    a.src = (const uint8_t*)src->data;
    a.idx = (const uint8_t*)idx->data;
    a.dst = (uint8_t*)dst->data;
    a.ne0 = ne0; a.n_slots = dst->ne[1]; a.ne2 = ne2; a.ne3 = ne3; a.ne11 = ne11; a.ne12 = ne12;
    a.snb1 = src->nb[1]; a.snb2 = src->nb[2]; a.snb3 = src->nb[3];
    a.inb0 = idx->nb[0]; a.inb1 = ne11 > 1 ? idx->nb[1] : 0; a.inb2 = ne12 > 1 ? idx->nb[2] : 0;
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
    a.dd_next = (int64_t)a.r32 * bb;  // (bytes)
    a.dd_wrap = ((int64_t)a.r32 - upr) * bb;
    // the 16-B source path: every row base a multiple of 16 (strides of a
    // dimension of one element are never multiplied by anything but 0)
    vec = (uintptr_t)src->data % 16 == 0 && (nr == 1 || src->nb[1] % 16 == 0) && (ne2 == 1 || src->nb[2] % 16 == 0) &&
          (ne3 == 1 || src->nb[3] % 16 == 0);
    return FATTN_OK;
}

template <int MODE, bool VEC>
void launch(bool unroll, dim3 grid, hipStream_t st, const RopeSetRowsArgs& a) {
    if constexpr (MODE == 0) {
        if (unroll) {
            hipLaunchKernelGGL((rope_set_rows_kernel<MODE, VEC, kSetRowsUnroll>), grid, dim3(256), 0, st, a);
            return;
        }
    }
    hipLaunchKernelGGL((rope_set_rows_kernel<MODE, VEC, 1>), grid, dim3(256), 0, st, a);
}
template <int MODE>
void launch(bool vec, bool unroll, dim3 grid, hipStream_t st, const RopeSetRowsArgs& a) {
    if (vec) launch<MODE, true>(unroll, grid, st, a);
    else launch<MODE, false>(unroll, grid, st, a);
}

}  // namespace

extern "C" int fattn_rope_set_rows(const fattn_tensor* k_src, const fattn_tensor* pos, const fattn_tensor* idx,
                                   const fattn_tensor* k_dst, const float* freq_factors, const fattn_rope* rope,
                                   const fattn_tensor* v_src, const fattn_tensor* v_dst, void* stream) {
    if (!k_src || !idx || !k_dst || !idx->data || (rope && (!pos || !pos->data))) return FATTN_ERR_INVALID_ARG;
    if ((v_src == nullptr) != (v_dst == nullptr)) return FATTN_ERR_INVALID_ARG;
    if (idx->type != FATTN_TYPE_I64 && idx->type != FATTN_TYPE_I32) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (rope && pos->type != FATTN_TYPE_I32) return FATTN_ERR_UNSUPPORTED_TYPE;
    for (int i = 0; i < 4; i++)
        if (idx->ne[i] <= 0 || (rope && pos->ne[i] <= 0)) return FATTN_ERR_INVALID_ARG;
    if (idx->ne[3] != 1) return FATTN_ERR_INVALID_ARG;

    RopeSetRowsArgs a = {};
    bool kvec = false, vvec = true;
    int rc = check_part(k_src, idx, k_dst, rope != nullptr, a.k, a.kbb, kvec);
    if (rc != FATTN_OK) return rc;
    a.kt = k_dst->type;
    const int64_t nr = k_src->ne[1], ne3 = k_src->ne[3];
    if (rope) {
        const fattn_rope& r = *rope;
        const int64_t np = pos->ne[1];
        if (pos->ne[0] != nr || ne3 % np || pos->ne[2] != 1 || pos->ne[3] != 1) return FATTN_ERR_INVALID_ARG;
        if (r.n_dims < 8 || r.n_dims > a.k.ne0 || r.n_dims % 8) return FATTN_ERR_INVALID_ARG;
        if (r.mode != 0 && r.mode != 2) return FATTN_ERR_INVALID_ARG;
        if (!finite_pos(r.freq_base) || !finite_pos(r.freq_scale)) return FATTN_ERR_INVALID_ARG;
        if (!std::isfinite(r.ext_factor) || r.ext_factor < 0.0f) return FATTN_ERR_INVALID_ARG;
        if (!std::isfinite(r.attn_factor) || !std::isfinite(r.beta_fast) || !std::isfinite(r.beta_slow)) return FATTN_ERR_INVALID_ARG;
        if (r.ext_factor != 0.0f && r.n_ctx_orig <= 0) return FATTN_ERR_INVALID_ARG;
        if (a.k.ne2 > INT32_MAX || ne3 > INT32_MAX) return FATTN_ERR_INVALID_ARG;
        const bool use1 = np > 1;  // pos nb[1] is looked at only then
        if (pos->nb[0] < 4 || (use1 && pos->nb[1] < 0)) return FATTN_ERR_BAD_STRIDE;
    }
    // the index tensor's strides (shared by both parts)
    const int64_t es = idx->type == FATTN_TYPE_I64 ? 8 : 4;
    const bool use1 = idx->ne[1] > 1, use2 = idx->ne[2] > 1;  // idx nb[1] / nb[2] are looked at only then
    if (idx->nb[0] < es || (use1 && idx->nb[1] < 0) || (use2 && idx->nb[2] < 0)) return FATTN_ERR_BAD_STRIDE;
    if ((uintptr_t)idx->data % es || idx->nb[0] % es || (use1 && idx->nb[1] % es) || (use2 && idx->nb[2] % es))
        return FATTN_ERR_ALIGNMENT;
    if (rope) {
        if ((uintptr_t)pos->data % 4 || pos->nb[0] % 4 || (pos->ne[1] > 1 && pos->nb[1] % 4)) return FATTN_ERR_ALIGNMENT;
        if ((uintptr_t)freq_factors % 4) return FATTN_ERR_ALIGNMENT;
    }
    if (v_src) {
        rc = check_part(v_src, idx, v_dst, false, a.v, a.vbb, vvec);
        if (rc != FATTN_OK) return rc;
        if (v_src->ne[1] != nr || v_src->ne[3] != ne3) return FATTN_ERR_INVALID_ARG;
        a.vt = v_dst->type;
    }

    const int64_t gz = std::min<int64_t>(ne3, 65535);
    const int64_t ne2v = v_src ? a.v.ne2 : 0;
    const double units = (double)a.k.units * (double)a.k.ne2 * (double)ne3 + (double)a.v.units * (double)ne2v * (double)ne3;
    // (only without a rope: beside the rotated rows the four-unit form measured slower)
    const bool unroll = !rope && units >= (double)kUnrollMinUnits && a.k.units >= kUnrollMinPlane && (!v_src || a.v.units >= kUnrollMinPlane);
    const int64_t U = unroll ? kSetRowsUnroll : 1;
    int64_t gy = std::min<int64_t>(std::max(a.k.ne2, ne2v), 65535);
    int mode = 0;
    if (rope) {
        const fattn_rope& r = *rope;
        mode = r.mode == 2 ? 2 : 1;
        a.pos = (const uint8_t*)pos->data;
        a.pnb0 = pos->nb[0];
        a.pnb1 = pos->ne[1] > 1 ? pos->nb[1] : 0;
        a.np = (int32_t)pos->ne[1];  // (np <= ne3)
        a.nr = nr;
        a.rpw = 8 / a.k.upr;
        KShiftArgs& kr = a.rope;
        kr.ff = freq_factors;
        kr.n_dims = r.n_dims;
        kr.theta_scale = powf(r.freq_base, -2.0f / (float)r.n_dims);
        kr.freq_scale = r.freq_scale;
        kr.ext_factor = r.ext_factor;
        kr.m = r.attn_factor;
        kr.lo = 0.0f;
        kr.den = 1.0f;
        if (r.ext_factor != 0.0f) {
            const float lo = std::max(0.0f, floorf(corr_dim(r.n_dims, r.n_ctx_orig, r.beta_fast, r.freq_base)));
            const float hi = std::min((float)(r.n_dims - 1), ceilf(corr_dim(r.n_dims, r.n_ctx_orig, r.beta_slow, r.freq_base)));
            kr.lo = lo;
            kr.den = std::max(0.001f, hi - lo);
            kr.m = r.attn_factor * (1.0f + 0.1f * logf(1.0f / r.freq_scale));
        }
        const int64_t waves = (nr + a.rpw - 1) / a.rpw;
        a.nk = (uint32_t)((waves + 3) / 4);
        // heads: all walked by one lane group once the other two grid dims fill the chip, spread over y
        // below that (fattn_k_shift's rule)
        gy = std::min<int64_t>(std::min<int64_t>(a.k.ne2, 65535), std::max<int64_t>(1, (kKShiftFullWaves + waves * gz - 1) / (waves * gz)));
    } else {
        a.nk = (uint32_t)((a.k.units + 32 * U - 1) / (32 * U));
    }
    const int64_t nv = v_src ? (a.v.units + 32 * U - 1) / (32 * U) : 0;
    const dim3 grid((unsigned)(a.nk + nv), (unsigned)gy, (unsigned)gz);
    const bool vec = kvec && vvec;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    if (mode == 2) launch<2>(vec, unroll, grid, st, a);
    else if (mode == 1) launch<1>(vec, unroll, grid, st, a);
    else launch<0>(vec, unroll, grid, st, a);
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}
