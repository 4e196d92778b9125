// fattn_quant.h -- ggml Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL row conversions on gfx950.
//
// The reference has no quantized code at all; these follow the
// published upstream-ggml algorithms (ggml-quants.c quantize_row_q8_0_ref,
// quantize_row_q4_0_ref, dequantize_row_q8_0, dequantize_row_q4_0), restated in
// oracle/fattn_oracle.c (Q4_1 / Q5_0 / Q5_1: quantize_row_q4_1_ref, _q5_0_ref,
// _q5_1_ref and their dequantize_row_*, restated in tests/kv_types.py; IQ4_NL:
// the cache-write quantiser and dequantize_row_iq4_nl, restated in
// tests/iq4_nl.py).  They are bit-exact with those restatements: every
// multiply/add is a separately rounded IEEE op (contraction off + barriers),
// divisions are correctly rounded (hipcc default), f32->f16 is round-to-nearest-even.
//
// Each type's rule is stated once, in the pieces below (scan_*, block_scale,
// block_code, block_value, iq4nl_*).  A layout holds only what is about the
// layout -- which elements a thread has, how partial statistics merge, how codes
// pack into bytes: quant_block / dequant_block here, set_rows_block
// (fattn_set_rows.h) and k_shift_load_block (fattn_k_shift.h).
//
// Layout of this file's kernels: one thread per 32-element block; a wave covers
// 64 consecutive blocks, so the block reads/writes of a wave are contiguous.
// These are the KV-cache write side (ggml cpy f32 -> a block type) and the
// dequant unit check.
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

// f32 -> the bits of a block's f16 field d or m
__device__ __forceinline__ uint32_t f16_bits(float x) { return __builtin_bit_cast(uint16_t, (f16)opaque(x)); }
// ... and the low 16 bits of v into a block, little-endian, as the one-thread-per-block kernels store: by the byte
__device__ __forceinline__ void store_u8x2(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}

// ---- The rule of each block type (quantize_row_*_ref, dequantize_row_*), one step per function

// The block statistics, scanned in element order over a whole block (N = 32) or
// a lane's share of one (N = 4; fattn_set_rows.h merges the shares).
// Q8_0: the largest |x|, by value -- no tie rule
template <int N>
__device__ __forceinline__ float scan_absmax(const float (&x)[N]) {
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < N; j++) amax = fmaxf(amax, fabsf(x[j]));
    return amax;
}
// Q4_0 / Q5_0 / IQ4_NL: mx = the FIRST element of largest |x| (the strict compare
// keeps the earlier of two equal ones; it gives d its sign); all zero: mx = +0
template <int N>
__device__ __forceinline__ void scan_amax(const float (&x)[N], float& amax, float& mx) {
    amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int j = 0; j < N; j++) {
        if (amax < fabsf(x[j])) {
            amax = fabsf(x[j]);
            mx = x[j];
        }
    }
}
// Q4_1 / Q5_1: the first of the smallest and the first of the largest value (-0.0 == +0.0)
template <int N>
__device__ __forceinline__ void scan_minmax(const float (&x)[N], float& mn, float& mxv) {
    mn = 3.402823466e+38f, mxv = -3.402823466e+38f;
#pragma unroll
    for (int j = 0; j < N; j++) {
        if (x[j] < mn) mn = x[j];
        if (x[j] > mxv) mxv = x[j];
    }
}

// The scale from the block's statistics -- mx: what the type's scan gives (Q8_0
// amax, Q4_1 / Q5_1 the maximum), mn: the minimum of Q4_1 / Q5_1 (its f16 bits are
// the block's m) -- and its reciprocal for block_code.  f16_bits(d) is the
// block's d; IQ4_NL: d is the scale its codes are chosen with, the one it stores
// is refitted (iq4nl_scale_bits).
struct BlockScale {
    float d, id;
};
template <int T>
__device__ __forceinline__ BlockScale block_scale(float mx, float mn) {
#pragma clang fp contract(off)
    static_assert(is_quant(T), "");
    BlockScale s;
    if constexpr (T == FATTN_TYPE_Q8_0) s.d = mx / 127.0f;
    else if constexpr (T == FATTN_TYPE_Q4_0) s.d = mx * -0.125f;   // == mx / -8 exactly (power of two), keeps -0.0
    else if constexpr (T == FATTN_TYPE_Q5_0) s.d = mx * -0.0625f;  // == mx / -16, likewise
    else if constexpr (is_codebook(T)) s.d = mx / -127.0f;
    else s.d = opaque(mx - mn) / (T == FATTN_TYPE_Q4_1 ? 15.0f : 31.0f);
    s.id = s.d != 0.0f ? 1.0f / s.d : 0.0f;
    return s;
}

// One element's code, 0 .. 255 (IQ4_NL: iq4nl_code).  Q4_0 / Q5_0: min(15 / 31,
// x id + 8.5 / 16.5 truncated to int8); Q4_1: min(15, (x - mn) id + 0.5 truncated
// to int8); Q5_1: the same truncated to uint8, no clamp.
template <int T>
__device__ __forceinline__ uint32_t block_code(float x, float id, float mn) {
#pragma clang fp contract(off)
    static_assert(is_quant(T) && !is_codebook(T), "");
    if constexpr (T == FATTN_TYPE_Q8_0) {
        return (uint8_t)(int8_t)roundf(x * id);
    } else if constexpr (T == FATTN_TYPE_Q4_0) {
        const int8_t t = (int8_t)(opaque(x * id) + 8.5f);
        return (uint8_t)(t < 15 ? t : 15);
    } else if constexpr (T == FATTN_TYPE_Q5_0) {
        const int8_t t = (int8_t)(opaque(x * id) + 16.5f);
        return (uint32_t)(t < 31 ? t : 31) & 0xFFu;
    } else if constexpr (T == FATTN_TYPE_Q4_1) {
        const int8_t t = (int8_t)(opaque(opaque(x - mn) * id) + 0.5f);
        return (uint32_t)(t < 15 ? t : 15) & 0xFFu;
    } else {
        return (uint8_t)(opaque(opaque(x - mn) * id) + 0.5f);
    }
}

// One element of dequantize_row_*: the code q (Q8_0: its byte; IQ4_NL: its
// codebook entry, a float from iq4nl_values4), the block's d and m -> x
template <int T, typename Q>
__device__ __forceinline__ float block_value(Q q, float d, float m) {
#pragma clang fp contract(off)
    static_assert(is_quant(T), "");
    constexpr int zero = T == FATTN_TYPE_Q4_0 ? 8 : code_zero(T);  // (Q4_0's 8: the kernels' nibble trick takes it, not code_zero)
    if constexpr (is_codebook(T)) return d * q;
    else if constexpr (T == FATTN_TYPE_Q8_0) return (float)(int8_t)q * d;
    else if constexpr (has_min(T)) return opaque((float)q * d) + m;
    else return (float)((int)q - zero) * d;
}

// One ggml block -> its 32 f32 values: a thread unpacks the codes byte by byte
template <int T>
__device__ __forceinline__ void dequant_block(const uint8_t* __restrict__ blk, float* __restrict__ y) {
    static_assert(is_quant(T), "");
    const float d = (float)__builtin_bit_cast(f16, (uint16_t)(blk[0] | (blk[1] << 8)));
    if constexpr (T == FATTN_TYPE_Q8_0) {
#pragma unroll
        for (int j = 0; j < QK; j += 4) {
            f32x4 v;
            v.x = block_value<T>(blk[2 + j], d, 0.0f);
            v.y = block_value<T>(blk[3 + j], d, 0.0f);
            v.z = block_value<T>(blk[4 + j], d, 0.0f);
            v.w = block_value<T>(blk[5 + j], d, 0.0f);
            *(f32x4*)(y + j) = v;
        }
    } else if constexpr (is_codebook(T)) {
#pragma unroll
        for (int j = 0; j < QK / 2; j += 4) {  // four bytes of qs: elements j .. j + 3 and j + 16 .. j + 19
            const uint8_t* q = blk + qs_off(T) + j;
            const uint32_t w = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            float lo[4], hi[4];
            iq4nl_values4(w & 0x0F0F0F0Fu, lo);
            iq4nl_values4((w >> 4) & 0x0F0F0F0Fu, hi);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                y[j + k] = block_value<T>(lo[k], d, 0.0f);
                y[j + k + QK / 2] = block_value<T>(hi[k], d, 0.0f);
            }
        }
    } else {
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
            y[j] = block_value<T>((b & 0x0F) | (int)(((qh >> j) & 1u) << 4), d, m);
            y[j + QK / 2] = block_value<T>((b >> 4) | (int)(((qh >> (j + 16)) & 1u) << 4), d, m);
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

// IQ4_NL, ggml's cache write f32 -> iq4_nl.  iq4nl_code: best_index of v = x * id,
// the codebook entry nearest to v with a tie going up.  ggml bisects the table
// on `v < kv[mav]`; the interval that finds, kv[mu - 1] <= v < kv[mu], is the one
// with mu - 1 = the number of entries kv[1 .. 14] that are not above v (counted
// with the same compare, negated: a NaN climbs to mu = 15 as it does there).
// The two ends come back through the codebook; `kvq` is kv[code] for the refit.
__device__ __forceinline__ uint32_t iq4nl_code(float v, float& kvq) {
#pragma clang fp contract(off)
    uint32_t mu = 1;
#pragma unroll
    for (int i = 1; i < 15; i++) mu += !(v < (float)kIq4nlValues[i]);
    const uint32_t t = iq4nl_lut4((mu - 1) | (mu << 8));
    const float lo = (float)(int)(t & 0xFFu) - 128.0f, hi = (float)(int)((t >> 8) & 0xFFu) - 128.0f;
    const bool down = opaque(v - lo) < opaque(hi - v);
    uint32_t q = down ? mu - 1 : mu;
    kvq = down ? lo : hi;
    if (v >= 113.0f) q = 15, kvq = 113.0f;
    if (v <= -127.0f) q = 0, kvq = -127.0f;
    return q;
}
// The refit of d over a block: sumqx, sumq2 are sequential chains over j = 0 .. 15
// of (w v x)[j] + (w v x)[j + 16] and (w v v)[j] + (w v v)[j + 16], w = x x, every
// operation rounded on its own.  One element's two products:
__device__ __forceinline__ void iq4nl_terms(float x, float v, float& qx, float& q2) {
#pragma clang fp contract(off)
    const float wv = opaque(opaque(x * x) * v);
    qx = opaque(wv * x);
    q2 = opaque(wv * v);
}
// ... and the stored scale from the sums (d0: the scale the codes were chosen with)
__device__ __forceinline__ uint32_t iq4nl_scale_bits(float sumqx, float sumq2, float d0) {
    return f16_bits(sumq2 > 0.0f ? sumqx / sumq2 : d0);
}

// One ggml block of 32 values -> its bytes: a thread scans all 32, then packs
// element j with element j + 16 (low nibble, high nibble of qs[j]; the fifth
// bits into bits j, j + 16 of qh); Q8_0: a byte per element
template <int T>
__device__ __forceinline__ void quant_block(const float (&xv)[QK], uint8_t* blk) {
#pragma clang fp contract(off)
    [[maybe_unused]] float amax;
    float mn = 0.0f, mx;
    if constexpr (T == FATTN_TYPE_Q8_0) mx = scan_absmax(xv);
    else if constexpr (has_min(T)) scan_minmax(xv, mn, mx);
    else scan_amax(xv, amax, mx);
    const BlockScale s = block_scale<T>(mx, mn);
    if constexpr (has_min(T)) store_u8x2(blk + 2, f16_bits(mn));
    if constexpr (T == FATTN_TYPE_Q8_0) {
        store_u8x2(blk, f16_bits(s.d));
#pragma unroll
        for (int j = 0; j < QK; j++) blk[2 + j] = (uint8_t)block_code<T>(xv[j], s.id, mn);
    } else if constexpr (is_codebook(T)) {
        float sumqx = 0.0f, sumq2 = 0.0f;
#pragma unroll
        for (int j = 0; j < QK / 2; j++) {
            float v0, v1, a0, a1, b0, b1;
            const uint32_t q0 = iq4nl_code(opaque(xv[j] * s.id), v0);
            const uint32_t q1 = iq4nl_code(opaque(xv[j + QK / 2] * s.id), v1);
            blk[2 + j] = (uint8_t)(q0 | (q1 << 4));
            iq4nl_terms(xv[j], v0, a0, b0);
            iq4nl_terms(xv[j + QK / 2], v1, a1, b1);
            sumqx = opaque(sumqx + opaque(a0 + a1));
            sumq2 = opaque(sumq2 + opaque(b0 + b1));
        }
        store_u8x2(blk, iq4nl_scale_bits(sumqx, sumq2, s.d));
    } else {
        store_u8x2(blk, f16_bits(s.d));
        uint32_t qh = 0;
#pragma unroll
        for (int j = 0; j < QK / 2; j++) {
            const uint32_t q0 = block_code<T>(xv[j], s.id, mn), q1 = block_code<T>(xv[j + QK / 2], s.id, mn);
            // (Q4_0 keeps the low code whole, as ggml's `q0 | (q1 << 4)` does)
            blk[qs_off(T) + j] = (uint8_t)((T == FATTN_TYPE_Q4_0 ? q0 : q0 & 0x0F) | ((q1 & 0x0F) << 4));
            qh |= ((q0 & 0x10u) >> 4) << j;
            qh |= ((q1 & 0x10u) >> 4) << (j + QK / 2);
        }
        if constexpr (has_qh(T)) {
            store_u8x2(blk + qh_off(T), qh);
            store_u8x2(blk + qh_off(T) + 2, qh >> 16);
        }
    }
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

// Strided f32 -> F16 / BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL copy: ggml's GGML_OP_CPY into a KV-cache view
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

// The IQ4_NL instantiations of the three kernels above live in fattn_launch_iq4_nl_conv.hip
// (with those of set_rows_kernel, k_shift_kernel and the staging pre-pass): the type's
// kernels are built with flags of their own (Makefile NOPK_UNITS), the other types' are not
void iq4nl_launch_dequant(dim3 grid, hipStream_t st, const uint8_t* src, float* dst, int64_t nblocks);
void iq4nl_launch_quant(dim3 grid, hipStream_t st, const float* src, uint8_t* dst, int64_t nblocks);
void iq4nl_launch_cpy(dim3 grid, hipStream_t st, const CpyArgs& a, int64_t units);

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
    if constexpr (is_codebook(KT)) {
        // IQ4_NL: h(kv[q] d), the exact product rounded once -- the bits of the split
        // kernel's K operand.  The thread's 8 codes are one nibble of 8 bytes of qs: two lookups
        const f16 d = __builtin_bit_cast(f16, blk[0]);
        const uint16_t* qw = blk + 1 + 4 * (j & 1);
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const uint32_t w = (uint32_t)qw[2 * e] | ((uint32_t)qw[2 * e + 1] << 16);
            float v[4];
            iq4nl_values4((j < 2 ? w : w >> 4) & 0x0F0F0F0Fu, v);
#pragma unroll
            for (int k = 0; k < 4; k++) h[4 * e + k] = (f16)v[k] * d;
        }
    } else if constexpr (is_kv_ext(KT)) {
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
