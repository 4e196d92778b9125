// fattn_quant.h -- ggml Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 row conversions on gfx950.
//
// The reference has no quantized code at all; these follow the
// published upstream-ggml algorithms (ggml-quants.c quantize_row_q8_0_ref,
// quantize_row_q4_0_ref, dequantize_row_q8_0, dequantize_row_q4_0), restated in
// oracle/fattn_oracle.c (Q4_1 / Q5_0 / Q5_1: quantize_row_q4_1_ref, _q5_0_ref,
// _q5_1_ref and their dequantize_row_*, restated in tests/kv_types.py), and are
// bit-exact with that restatement: every
// multiply/add is a separately rounded IEEE op (contraction off + barriers),
// divisions are correctly rounded (hipcc default), f32->f16 is round-to-nearest-even.
//
// Layout: one thread per 32-element block; a wave covers 64 consecutive blocks,
// so the block reads/writes of a wave are contiguous.  These are the
// KV-cache write side (ggml cpy f32 -> q8_0/q4_0) and the dequant unit check.
#pragma once

#include "fattn_common.h"

namespace fattn {

// hipcc contracts a*b+c into FMA by default (even written as __fmul_rn /
// __fadd_rn) and folds f16(a*b) into v_fma_mix with a +0 addend (losing -0);
// ggml's reference evaluates each op separately.  The pragma and this barrier
// keep every operation individually rounded.
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// One ggml block -> its 32 f32 values (dequantize_row_q8_0 / _q4_0 / _q4_1 / _q5_0 / _q5_1)
template <int T>
__device__ __forceinline__ void dequant_block(const uint8_t* __restrict__ blk, float* __restrict__ y) {
#pragma clang fp contract(off)
    static_assert(is_quant(T), "");
    const float d = (float)__builtin_bit_cast(f16, (uint16_t)(blk[0] | (blk[1] << 8)));
    if constexpr (T == FATTN_TYPE_Q8_0) {
#pragma unroll
        for (int j = 0; j < QK; j += 4) {
            f32x4 v;
            v.x = (float)(int8_t)blk[2 + j] * d;
            v.y = (float)(int8_t)blk[3 + j] * d;
            v.z = (float)(int8_t)blk[4 + j] * d;
            v.w = (float)(int8_t)blk[5 + j] * d;
            *(f32x4*)(y + j) = v;
        }
    } else {
        constexpr int zero = T == FATTN_TYPE_Q4_0 ? 8 : code_zero(T);  // (Q4_0's 8: the kernels' nibble trick takes it, not code_zero)
        float m = 0.0f;
        if constexpr (has_min(T)) m = (float)__builtin_bit_cast(f16, (uint16_t)(blk[2] | (blk[3] << 8)));
        uint32_t qh = 0;
        if constexpr (has_qh(T)) {
            const uint8_t* h = blk + qh_off(T);
            qh = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24);
        }
#pragma unroll
        for (int j = 0; j < QK / 2; j++) {
            const int b = blk[qs_off(T) + j];
            const int q0 = (b & 0x0F) | (int)(((qh >> j) & 1u) << 4);
            const int q1 = (b >> 4) | (int)(((qh >> (j + 16)) & 1u) << 4);
            if constexpr (has_min(T)) {
                y[j] = opaque((float)q0 * d) + m;
                y[j + QK / 2] = opaque((float)q1 * d) + m;
            } else {
                y[j] = (float)(q0 - zero) * d;
                y[j + QK / 2] = (float)(q1 - zero) * d;
            }
        }
    }
}

// block type -> f32: one thread per block
template <int T>
__global__ __launch_bounds__(256) void dequant_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t nblocks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    dequant_block<T>(src + i * TypeInfo<T>::block_bytes, dst + i * QK);
}

// f16 / bf16 -> f32 (bf16: exact, the bits shifted up): one thread per element
template <int T>
__global__ __launch_bounds__(256) void dequant_row16_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
    static_assert(is_row16(T), "");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (T == FATTN_TYPE_F16) dst[i] = (float)__builtin_bit_cast(f16, src[i]);
    else dst[i] = __builtin_bit_cast(float, (uint32_t)src[i] << 16);
}

// f32 -> bf16 bits, ggml_compute_fp32_to_bf16 bit for bit, in integer arithmetic
// (the hardware convert's NaN payload is not promised to match): a NaN keeps its
// top 16 bits and is made quiet; everything else rounds to nearest even on the
// 16 dropped bits -- subnormals kept, overflow to inf
__host__ __device__ __forceinline__ uint16_t f32_to_bf16_bits(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    return (uint16_t)((u + (0x7fffu + ((u >> 16) & 1u))) >> 16);
}

// f32 -> bf16, one thread per element
// (a template, so that only the translation unit that launches it holds it)
template <int T = FATTN_TYPE_BF16>
__global__ __launch_bounds__(256) void quant_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dst[i] = f32_to_bf16_bits(src[i]);
}

// One ggml block of 32 values -> Q8_0 {f16 d; int8 qs[32]} (quantize_row_q8_0_ref)
__device__ __forceinline__ void quant_block_q8_0(const float (&xv)[QK], uint8_t* blk) {
#pragma clang fp contract(off)
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < QK; j++) amax = fmaxf(amax, fabsf(xv[j]));
    const float d = amax / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    const uint16_t dh = __builtin_bit_cast(uint16_t, (f16)opaque(d));
    blk[0] = dh & 0xff;
    blk[1] = dh >> 8;
#pragma unroll
    for (int j = 0; j < QK; j++) blk[2 + j] = (uint8_t)(int8_t)roundf(xv[j] * id);
}

// One ggml block of 32 values -> Q4_0 {f16 d; u8 qs[16]} (quantize_row_q4_0_ref)
__device__ __forceinline__ void quant_block_q4_0(const float (&xv)[QK], uint8_t* blk) {
#pragma clang fp contract(off)
    float amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int j = 0; j < QK; j++) {
        if (amax < fabsf(xv[j])) {
            amax = fabsf(xv[j]);
            mx = xv[j];
        }
    }
    const float d = mx * -0.125f;  // == mx / -8 exactly (power of two), keeps -0.0
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    const uint16_t dh = __builtin_bit_cast(uint16_t, (f16)opaque(d));
    blk[0] = dh & 0xff;
    blk[1] = dh >> 8;
#pragma unroll
    for (int j = 0; j < QK / 2; j++) {
        const int8_t t0 = (int8_t)(opaque(xv[j] * id) + 8.5f);
        const int8_t t1 = (int8_t)(opaque(xv[j + QK / 2] * id) + 8.5f);
        const uint8_t q0 = (uint8_t)(t0 < 15 ? t0 : 15);
        const uint8_t q1 = (uint8_t)(t1 < 15 ? t1 : 15);
        blk[2 + j] = (uint8_t)(q0 | (q1 << 4));
    }
}

// One ggml block of 32 values -> Q4_1 / Q5_0 / Q5_1 (quantize_row_q4_1_ref,
// quantize_row_q5_0_ref, quantize_row_q5_1_ref).  Q4_1 / Q5_1: d = (max - min) /
// 15 (31), q = (x - min) / d + 0.5 truncated (Q4_1 clamps at 15, Q5_1 does not);
// Q5_0: d = (the first element of largest |x|) / -16, q = min(31, x / d + 16.5).
// The low four bits go to qs (element j low nibble, j + 16 high), bit 4 to qh.
template <int T>
__device__ __forceinline__ void quant_block_ext(const float (&xv)[QK], uint8_t* blk) {
#pragma clang fp contract(off)
    static_assert(is_kv_ext(T), "");
    float d, mn = 0.0f;
    if constexpr (T == FATTN_TYPE_Q5_0) {
        float amax = 0.0f, mx = 0.0f;
#pragma unroll
        for (int j = 0; j < QK; j++) {
            if (amax < fabsf(xv[j])) {
                amax = fabsf(xv[j]);
                mx = xv[j];
            }
        }
        d = mx * -0.0625f;  // == mx / -16 exactly (power of two), keeps -0.0
    } else {
        float mxv = -3.402823466e+38f;
        mn = 3.402823466e+38f;
#pragma unroll
        for (int j = 0; j < QK; j++) {
            if (xv[j] < mn) mn = xv[j];
            if (xv[j] > mxv) mxv = xv[j];
        }
        d = opaque(mxv - mn) / (T == FATTN_TYPE_Q4_1 ? 15.0f : 31.0f);
        const uint16_t mh = __builtin_bit_cast(uint16_t, (f16)opaque(mn));
        blk[2] = mh & 0xff;
        blk[3] = mh >> 8;
    }
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    const uint16_t dh = __builtin_bit_cast(uint16_t, (f16)opaque(d));
    blk[0] = dh & 0xff;
    blk[1] = dh >> 8;
    uint32_t qh = 0;
#pragma unroll
    for (int j = 0; j < QK / 2; j++) {
        uint32_t q0, q1;
        if constexpr (T == FATTN_TYPE_Q5_0) {
            const int8_t t0 = (int8_t)(opaque(xv[j] * id) + 16.5f);
            const int8_t t1 = (int8_t)(opaque(xv[j + QK / 2] * id) + 16.5f);
            q0 = (uint32_t)(t0 < 31 ? t0 : 31);
            q1 = (uint32_t)(t1 < 31 ? t1 : 31);
        } else if constexpr (T == FATTN_TYPE_Q4_1) {
            const int8_t t0 = (int8_t)(opaque(opaque(xv[j] - mn) * id) + 0.5f);
            const int8_t t1 = (int8_t)(opaque(opaque(xv[j + QK / 2] - mn) * id) + 0.5f);
            q0 = (uint32_t)(t0 < 15 ? t0 : 15);
            q1 = (uint32_t)(t1 < 15 ? t1 : 15);
        } else {
            q0 = (uint8_t)(opaque(opaque(xv[j] - mn) * id) + 0.5f);
            q1 = (uint8_t)(opaque(opaque(xv[j + QK / 2] - mn) * id) + 0.5f);
        }
        blk[qs_off(T) + j] = (uint8_t)((q0 & 0x0F) | ((q1 & 0x0F) << 4));
        qh |= ((q0 & 0x10u) >> 4) << j;
        qh |= ((q1 & 0x10u) >> 4) << (j + QK / 2);
    }
    if constexpr (has_qh(T)) {
        uint8_t* h = blk + qh_off(T);
        h[0] = qh & 0xff;
        h[1] = (qh >> 8) & 0xff;
        h[2] = (qh >> 16) & 0xff;
        h[3] = qh >> 24;
    }
}

// the block function of type T
template <int T>
__device__ __forceinline__ void quant_block(const float (&xv)[QK], uint8_t* blk) {
    if constexpr (T == FATTN_TYPE_Q8_0) quant_block_q8_0(xv, blk);
    else if constexpr (T == FATTN_TYPE_Q4_0) quant_block_q4_0(xv, blk);
    else quant_block_ext<T>(xv, blk);
}

template <int T>
__global__ __launch_bounds__(256) void quant_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                    int64_t nblocks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    const float* x = src + i * QK;
    float xv[QK];
#pragma unroll
    for (int j = 0; j < QK; j += 4) {
        const f32x4 v = *(const f32x4*)(x + j);
        xv[j] = v.x; xv[j + 1] = v.y; xv[j + 2] = v.z; xv[j + 3] = v.w;
    }
    quant_block<T>(xv, dst + i * TypeInfo<T>::block_bytes);
}

// Strided f32 -> F16 / BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 copy: ggml's GGML_OP_CPY into a KV-cache view
// (upstream ggml cpy f32 -> f16/q8_0/q4_0).  src and dst
// have the same ne (ne0 = row length, a multiple of 32 for the block types)
// and any byte strides nb1..nb3; rows are contiguous (src nb0 = 4, dst nb0 =
// element / block size).  One thread per 32-element block (per element for
// F16): the writes of one token's K rows land straight in the cache, whether
// it is laid out [Hkv][N][row] (head stride > row) or [N][Hkv][row].
struct CpyArgs {
    const uint8_t* src;
    uint8_t* dst;
    int64_t ne0, ne1, ne2, ne3;
    int64_t snb1, snb2, snb3;
    int64_t dnb1, dnb2, dnb3;
};

template <int T>
__global__ __launch_bounds__(256) void cpy_f32_kernel(const CpyArgs a, int64_t units) {
    constexpr int UE = is_row16(T) ? 1 : QK;  // elements per unit
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= units) return;
    const int64_t upr = a.ne0 / UE;
    const int64_t b = i % upr, r = i / upr;
    const int64_t i1 = r % a.ne1, i2 = (r / a.ne1) % a.ne2, i3 = r / (a.ne1 * a.ne2);
    const float* x = (const float*)(a.src + i1 * a.snb1 + i2 * a.snb2 + i3 * a.snb3) + b * UE;
    uint8_t* y = a.dst + i1 * a.dnb1 + i2 * a.dnb2 + i3 * a.dnb3;
    if constexpr (T == FATTN_TYPE_F16) {
        *(uint16_t*)(y + b * 2) = __builtin_bit_cast(uint16_t, (f16)x[0]);
    } else if constexpr (T == FATTN_TYPE_BF16) {
        *(uint16_t*)(y + b * 2) = f32_to_bf16_bits(x[0]);
    } else {
        float xv[QK];
#pragma unroll
        for (int j = 0; j < QK; j++) xv[j] = x[j];
        quant_block<T>(xv, y + b * TypeInfo<T>::block_bytes);
    }
}

// Prefill K/V staging (the prefill planner's default for Q8_0 / Q4_0 caches):
// the quantised rows of every (sequence, kv head) -- contiguous blocks, head
// base at ik3 * nb3 + ik2 * nb2 -- become f16 rows [Skv][Hkv][N][D] in the
// caller's workspace, h(q * d) with one f16 rounding: the value the in-kernel
// dequantisation of every other kernel produces (src/utils.h:10-11), so the
// f16 prefill kernel over the staged rows computes the same attention.  The
// prefill re-reads each K/V tile once per 256-row query tile (16 times at
// n_q = 4096); staging converts it once (35.7 MB read, 67 MB written at the
// prefill shape) instead of 16 times in the MFMA loop.  Thread = 8 values of
// one block (16 B of f16 written); grid (blocks * 4 / 256, Hkv, Skv).
template <int KT>
__device__ __forceinline__ void kv_stage_f16_block(const uint8_t* __restrict__ src, int64_t nb2, int64_t nb3,
                                                   uint16_t* __restrict__ dst, int64_t nblk, int64_t bx, int head,
                                                   int seq, int gy) {
    const int64_t t = bx * 256 + threadIdx.x;
    if (t >= 4 * nblk) return;
    const int64_t b = t >> 2;
    const int j = (int)(t & 3);
    const uint8_t* blk8 = src + (int64_t)seq * nb3 + (int64_t)head * nb2 + b * TypeInfo<KT>::block_bytes;
    const uint16_t* blk = (const uint16_t*)blk8;  // (blocks are 2-byte aligned)
    f16x8 h;
    if constexpr (is_kv_ext(KT)) {
        // Q4_1 / Q5_0 / Q5_1: the f16 the split kernel's K operand (k_operand_ext,
        // fattn_split.h) produces for the same element.  Q5_0: h((q - 16) d), the
        // exact product rounded once.  Q4_1 / Q5_1: the f16 fma h(q d + m) of the
        // exact code and the block's two f16 fields -- one rounding of the exact
        // sum, where f32 arithmetic (dequantize_row_*, then f16) rounds the sum to
        // f32 first: the two differ by one f16 ulp where that f32 rounding lands on
        // an f16 tie, and nowhere else.
        const f16 d = __builtin_bit_cast(f16, blk[0]);
        f16 m = (f16)0.0f;
        if constexpr (has_min(KT)) m = __builtin_bit_cast(f16, blk[1]);
        uint32_t qh8 = 0;  // the fifth bits of elements 8j .. 8j + 7
        if constexpr (has_qh(KT)) qh8 = ((uint32_t)blk[qh_off(KT) / 2 + (j >> 1)] >> (8 * (j & 1))) & 0xFFu;
        const uint16_t* qw = blk + qs_off(KT) / 2 + 4 * (j & 1);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t w = qw[e];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const uint32_t by = k ? w >> 8 : w & 0xFF;
                const int q = (int)((j < 2 ? by & 0x0F : by >> 4) | (((qh8 >> (2 * e + k)) & 1u) << 4));
                if constexpr (has_min(KT)) h[2 * e + k] = __builtin_fmaf16((f16)q, d, m);
                else h[2 * e + k] = (f16)(q - code_zero(KT)) * d;
            }
        }
    } else {
        const float d = (float)__builtin_bit_cast(f16, blk[0]);
        const uint16_t* qw = (const uint16_t*)(blk8 + 2 + (KT == FATTN_TYPE_Q8_0 ? 8 * j : 8 * (j & 1)));
        uint32_t by[8];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t w = qw[e];
            by[2 * e] = w & 0xFF;
            by[2 * e + 1] = w >> 8;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float q;
            if constexpr (KT == FATTN_TYPE_Q8_0) q = (float)(int8_t)by[e];
            else q = (float)((int)(j < 2 ? by[e] & 0x0F : by[e] >> 4) - 8);  // elements 0-15 low nibbles, 16-31 high
            h[e] = (f16)(q * d);  // exact product (<= 19 significant bits), one rounding to f16
        }
    }
    uint16_t* y = dst + (((int64_t)seq * gy + head) * nblk + b) * QK + 8 * j;
    *(f16x8*)y = h;
}
template <int KT>
__global__ __launch_bounds__(256) void kv_stage_f16_kernel(const uint8_t* __restrict__ src, int64_t nb2, int64_t nb3,
                                                           uint16_t* __restrict__ dst, int64_t nblk) {
    kv_stage_f16_block<KT>(src, nb2, nb3, dst, nblk, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.y);
}

}  // namespace fattn
