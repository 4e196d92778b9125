// fattn_launch_lse.hip -- fattn_lse_merge (include/fattn.h): the validation and
// the kernel that merges normalised partial outputs over disjoint key ranges
// by their log-sum-exps -- the chunk merge of the split-KV plans
// (merge_row_parts, fattn_tile.h: fa_reduce, src/flash_row_float.h:415-472), from
// outside a launch and in natural-log units.  A translation unit of its own.
// Nothing allocates; nothing synchronises (graph-capturable).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fattn.h"
#include "fattn_common.h"

using namespace fattn;

namespace {

struct LseMergeArgs {
    const float* outs;   // part p: [n_rows][dv] at p * out_stride floats
    const float* lses;   // part p: [n_rows] at p * lse_stride floats
    const float* sinks;  // [n_head] raw logits, or null
    float* dst;          // [n_rows][dv]
    float* lse_out;      // [n_rows], or null
    int64_t out_stride, lse_stride, n_rows;
    int n_parts, dv, n_head;
};

constexpr int kMergeRowsWg = 4;  // one wave per row

// e^d, d <= 0, through v_exp_f32 with the product d log2(e) carried in two
// floats: rounded to one, its error |d log2e| 2^-24 is a RELATIVE error of the
// weight of ln 2 times that -- 20 ulp for a part (or every part, under a dominant
// sink) 14 below the row's max.  p = d hi rounded, e = the rounding's error (fma)
// plus d lo, and 2^(p + e) = 2^p (1 + e ln 2) to first order (|e| < 2^-17)
__device__ __forceinline__ float exp_nat(float d) {
    constexpr float kHi = 1.44269502162933349609375f, kLo = 1.92596299112661746e-8f;  // log2(e) = kHi + kLo
    const float p = d * kHi;
    const float e = __builtin_fmaf(d, kHi, -p) + d * kLo;
    return __builtin_amdgcn_exp2f(p) * __builtin_fmaf(0.6931471805599453f, e, 1.0f);
}

// One wave per row.  Lane p < n_parts holds lse_p; the max and the sum of the
// weights w_p = e^(lse_p - M) reduce on the VALU (seg_reduce: DPP + permlane
// swaps).  Lane l owns the 16-byte column pieces l and l + 64 (dv / 4 <= 128
// pieces) and walks the parts in order, w_p broadcast by readlane: fixed order,
// deterministic.  A part of weight 0 -- lse_p = -inf, or e^(lse_p - M)
// underflowed -- is dropped by selection, so its (NaN) row never reaches the
// sum as 0 * NaN.  Every part's piece is loaded whether it counts or not: the
// loads do not depend on the weights and overlap.
__global__ __launch_bounds__(kMergeRowsWg* kWave) void fattn_lse_merge_kernel(const LseMergeArgs a) {
    constexpr float kNegInf = -__builtin_inff();
    constexpr float kLn2 = 0.6931471805599453f;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kMergeRowsWg + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // (wave-uniform: EXEC stays full for the reductions)
    const int NP = a.n_parts;
    const float lp = lane < NP ? a.lses[lane * a.lse_stride + row] : kNegInf;
    const float Mk = seg_reduce<true>(lp, 64);
    const float* sinks = a.sinks;
    const float s = sinks ? sinks[row % a.n_head] : kNegInf;  // (wave-uniform)
    const float M = fmaxf(Mk, s);                             // the sink is one more term, taken at max(M, s)
    const float w = (lp == kNegInf) ? 0.0f : exp_nat(lp - M);
    float L = seg_reduce<false>(w, 64);
    if (s != kNegInf) L += exp_nat(s - M);
    const bool dead = Mk == kNegInf;  // no part holds a key: NaN, or zeros with sinks, by selection
    const float fill = sinks ? 0.0f : __builtin_nanf("");
    const int wi = __builtin_bit_cast(int, w);
    const float* src = a.outs + row * a.dv;
    float* out = a.dst + row * a.dv;
    const int pieces = a.dv >> 2;
    for (int c = lane; c < pieces; c += kWave) {  // (at most two passes: dv <= 512)
        // part 0 starts the sum as a product, not 0 + product: with one part and no sink
        // w = L = 1 and the row is copied bit for bit, -0 included
        const float w0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, 0));
        const f32x4 v0 = *(const f32x4*)(src + 4 * c);
        f32x4 acc = w0 != 0.0f ? w0 * v0 : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int p = 1; p < NP; p++) {  // wave-uniform
            const float wp = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, p));
            const f32x4 v = *(const f32x4*)(src + p * a.out_stride + 4 * c);
            acc = wp != 0.0f ? acc + wp * v : acc;
        }
        *(f32x4*)(out + 4 * c) = dead ? f32x4{fill, fill, fill, fill} : acc / L;
    }
    if (a.lse_out) {  // (wave-uniform)
        if (lane == 0) a.lse_out[row] = dead ? s : M + kLn2 * __builtin_amdgcn_logf(L);
    }
}

}  // namespace

extern "C" int fattn_lse_merge(const float* outs, const float* lses, int32_t n_parts, int64_t n_rows, int32_t dv,
                               int64_t out_part_stride, int64_t lse_part_stride, const float* sinks, int32_t n_head,
                               float* dst, float* lse_out, void* stream) {
    if (!outs || !lses || !dst) return FATTN_ERR_INVALID_ARG;
    if (n_parts < 1 || n_parts > 64 || n_rows < 1 || n_rows > INT32_MAX) return FATTN_ERR_INVALID_ARG;
    if (sinks && n_head < 1) return FATTN_ERR_INVALID_ARG;
    if (dv < 4 || dv > 512 || dv % 4) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    if (out_part_stride < n_rows * dv || out_part_stride % 4 || lse_part_stride < n_rows) return FATTN_ERR_BAD_STRIDE;
    if ((uintptr_t)outs % 16 || (uintptr_t)dst % 16) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)lses % 4 || (uintptr_t)lse_out % 4 || (uintptr_t)sinks % 4) return FATTN_ERR_ALIGNMENT;
    LseMergeArgs a;
    a.outs = outs;
    a.lses = lses;
    a.sinks = sinks;
    a.dst = dst;
    a.lse_out = lse_out;
    a.out_stride = out_part_stride;
    a.lse_stride = lse_part_stride;
    a.n_rows = n_rows;
    a.n_parts = n_parts;
    a.dv = dv;
    a.n_head = sinks ? n_head : 1;
    const dim3 grid((unsigned)((n_rows + kMergeRowsWg - 1) / kMergeRowsWg));
    (void)hipGetLastError();
    hipLaunchKernelGGL(fattn_lse_merge_kernel, grid, dim3(kMergeRowsWg * kWave), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}
