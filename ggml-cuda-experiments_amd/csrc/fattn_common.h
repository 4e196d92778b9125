// fattn_common.h -- shared device helpers for the gfx950 attention kernels.
//
// Replaces src/tensor-mma.h (WMMA 16x16x16 fragments, WARP_SIZE 32) and the
// warp_reduce_* butterflies of src/cuda_info.h:46-85 with CDNA4 primitives:
// wave64 shuffles and __builtin_amdgcn_mfma_f32_16x16x32_f16.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/fattn_debug.h"

namespace fattn {

constexpr int kWave = 64;

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

typedef __attribute__((address_space(3))) uint8_t lds_u8;

// ggml block geometry
constexpr int QK = 32;

// ---------------------------------------------------------------- types
// A compile-time list of ints (ggml types, head dims), membership in it, and
// the one dispatcher from a run-time value to a template argument:
// f(std::integral_constant<int, V>()) for the V of the list equal to v, `none`
// where v is not of the list.
template <int... Vs>
struct ValueList {};
template <int... Vs>
__host__ __device__ constexpr bool in_list(ValueList<Vs...>, int v) {
    return ((v == Vs) || ...);
}
template <int... Vs, typename R, typename F>
R visit(ValueList<Vs...>, int v, R none, F&& f) {
    R r = none;
    (void)((v == Vs ? (r = f(std::integral_constant<int, Vs>()), true) : false) || ...);
    return r;
}

// One description per type: TypeInfo<T> is all the library knows about the
// layout of T.  Rows of 16-bit elements (block_elems = 1) or of ggml blocks of
// 32 elements {f16 d; [f16 m;] [u8 qh[4];] qs}: element j of a 4- / 5-bit block
// in the low nibble of qs[j], j + 16 in the high one, bit j of the
// little-endian u32 qh its fifth bit; x = q d + m (has_min) or (q - code_zero) d.
template <int BE, int BB, bool MIN = false, bool QH = false, int QHO = 4, int QSO = 2, int ZERO = 0>
struct RowLayout {
    static constexpr int block_elems = BE, block_bytes = BB;
    static constexpr bool has_min = MIN, has_qh = QH;        // the block holds m / qh
    static constexpr int qh_off = QHO, qs_off = QSO;         // ... byte offsets of qh and qs in it
    static constexpr int code_zero = ZERO;                   // the code's zero point, where the kernels subtract one
};
template <int T>
struct TypeInfo;
template <> struct TypeInfo<FATTN_TYPE_F32> : RowLayout<1, 4> { static constexpr const char* name = "f32"; };
template <> struct TypeInfo<FATTN_TYPE_F16> : RowLayout<1, 2> { static constexpr const char* name = "f16"; };
// BF16 rows are raw 16-bit elements like F16 rows: the same bytes per row, the
// same HBM -> LDS -> VGPR moves (is_row16); only the MFMA that takes them differs
template <> struct TypeInfo<FATTN_TYPE_BF16> : RowLayout<1, 2> { static constexpr const char* name = "bf16"; };
template <> struct TypeInfo<FATTN_TYPE_Q8_0> : RowLayout<QK, 34> { static constexpr const char* name = "q8_0"; };  // {f16 d; int8 qs[32]}
template <> struct TypeInfo<FATTN_TYPE_Q4_0> : RowLayout<QK, 18> { static constexpr const char* name = "q4_0"; };  // {f16 d; u8 qs[16]}, x = (q - 8) d
template <> struct TypeInfo<FATTN_TYPE_Q4_1> : RowLayout<QK, 20, true, false, 4, 4> { static constexpr const char* name = "q4_1"; };
template <> struct TypeInfo<FATTN_TYPE_Q5_0> : RowLayout<QK, 22, false, true, 2, 6, 16> { static constexpr const char* name = "q5_0"; };
template <> struct TypeInfo<FATTN_TYPE_Q5_1> : RowLayout<QK, 24, true, true, 4, 8> { static constexpr const char* name = "q5_1"; };

// The type lists every dispatch site names (a new cache type joins the ones it belongs to)
using CacheTypes = ValueList<FATTN_TYPE_F16, FATTN_TYPE_BF16, FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0, FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>;
using RowTypes = ValueList<FATTN_TYPE_F32, FATTN_TYPE_F16, FATTN_TYPE_BF16, FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0, FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>;  // fattn_row_size
using CoreTypes = ValueList<FATTN_TYPE_F16, FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0>;  // every kernel family; mixed K / V pairs; MLA
using QuantTypes = ValueList<FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0>;                 // ... the block types among them
// the three block types with a fifth bit and / or an affine term (is_kv_ext):
// only the split kernel and the prefill staging take them
using ExtTypes = ValueList<FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>;
using SplitOnlyTypes = ValueList<FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1, FATTN_TYPE_BF16>;  // K and V of one type, D = 64 / 128 / 256
using StageTypes = ValueList<FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0, FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>;  // block types: staged to f16 for prefill, quantize / dequantize
using SetRowsTypes = ValueList<FATTN_TYPE_F16, FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0, FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1>;  // (no BF16)
using KShiftTypes = RowTypes;  // fattn_k_shift rotates every row type in place, an F32 view included

// TypeInfo by run-time type: the row of type t, or the empty row (block_elems = 0)
struct TypeDesc {
    const char* name;
    int block_elems, block_bytes;
    bool has_min, has_qh;
    int qh_off, qs_off, code_zero;
};
template <int T>
constexpr TypeDesc desc_of() {
    using I = TypeInfo<T>;
    return {I::name, I::block_elems, I::block_bytes, I::has_min, I::has_qh, I::qh_off, I::qs_off, I::code_zero};
}
template <int... Ts>
__host__ __device__ constexpr TypeDesc type_desc(ValueList<Ts...>, int t) {
    TypeDesc d = {"?", 0, 0, false, false, 4, 2, 0};
    ((t == Ts ? (void)(d = desc_of<Ts>()) : (void)0), ...);
    return d;
}
__host__ __device__ constexpr TypeDesc type_desc(int t) { return type_desc(CacheTypes(), t); }

constexpr const char* type_name(int t) { return type_desc(t).name; }
__host__ __device__ constexpr bool is_row16(int t) { return type_desc(t).block_bytes == 2 && type_desc(t).block_elems == 1; }
__host__ __device__ constexpr bool is_quant(int t) { return type_desc(t).block_elems == QK; }  // the ggml block types a cache may hold
__host__ __device__ constexpr bool is_kv_ext(int t) { return in_list(ExtTypes(), t); }
__host__ __device__ constexpr bool has_min(int t) { return type_desc(t).has_min; }
__host__ __device__ constexpr bool has_qh(int t) { return type_desc(t).has_qh; }
__host__ __device__ constexpr int qh_off(int t) { return type_desc(t).qh_off; }
__host__ __device__ constexpr int qs_off(int t) { return type_desc(t).qs_off; }
__host__ __device__ constexpr int code_zero(int t) { return type_desc(t).code_zero; }
constexpr int kQ8Bytes = TypeInfo<FATTN_TYPE_Q8_0>::block_bytes;
constexpr int kQ4Bytes = TypeInfo<FATTN_TYPE_Q4_0>::block_bytes;

// bytes of one row of k elements (fattn_row_size); 0: no whole number of blocks, or no such type
constexpr size_t row_size(int type, int64_t k) {
    const TypeDesc d = type_desc(RowTypes(), type);
    return d.block_elems == 0 || k % d.block_elems ? 0 : (size_t)(k / d.block_elems) * d.block_bytes;
}

// waves per SIMD of the split kernel's register budget: its __launch_bounds__
// and the planner's occupancy figure (size_split)
// (Q4_1 / Q5_0 / Q5_1: the qh words and the second accumulator spill at 4)
__host__ __device__ constexpr int split_bounds_wps(int kt, int gran, int D) {
    return (is_row16(kt) || gran == 4 || D == 256 || is_kv_ext(kt)) ? 2 : 4;
}

template <int T, int D>
constexpr int row_bytes() {
    return D / TypeInfo<T>::block_elems * TypeInfo<T>::block_bytes;
}

// ---------------------------------------------------------------- bit helpers

__device__ __forceinline__ uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}
__device__ __forceinline__ uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t shift) {
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
}
__device__ __forceinline__ f16x2 as_h2(uint32_t x) { return __builtin_bit_cast(f16x2, x); }
__device__ __forceinline__ uint32_t as_u32(f16x2 x) { return __builtin_bit_cast(uint32_t, x); }

// f16 pair with both halves = the f16 whose bits are the low 16 bits of x
__device__ __forceinline__ f16x2 bcast_h(uint32_t bits16) {
    const uint32_t b = bits16 & 0xffffu;
    return as_h2(b | (b << 16));
}

// Four int8 (two's complement, packed in a dword) -> two f16 pairs holding the
// exact integer values.  Magic-number trick: f16 bits 0x64uu = 1024 + uu, so
// with uu = q ^ 0x80 = q + 128 the value is 1152 + q; subtracting 1152 is exact.
__device__ __forceinline__ void i8x4_to_h2x2(uint32_t w, f16x2& lo, f16x2& hi) {
    const uint32_t t = w ^ 0x80808080u;
    const uint32_t p0 = perm_b32(0x64646464u, t, 0x04010400u);  // bytes: t0,0x64,t1,0x64
    const uint32_t p1 = perm_b32(0x64646464u, t, 0x04030402u);  // bytes: t2,0x64,t3,0x64
    const f16x2 off = {(f16)-1152.0f, (f16)-1152.0f};
    lo = as_h2(p0) + off;
    hi = as_h2(p1) + off;
}

// Four nibbles already isolated in the low 4 bits of each byte of w ->
// two f16 pairs holding (nib - 8) exactly (Q4_0 offset).
__device__ __forceinline__ void u4x4_to_h2x2(uint32_t w, f16x2& lo, f16x2& hi) {
    const uint32_t p0 = perm_b32(0x64646464u, w, 0x04010400u);
    const uint32_t p1 = perm_b32(0x64646464u, w, 0x04030402u);
    const f16x2 off = {(f16)-1032.0f, (f16)-1032.0f};
    lo = as_h2(p0) + off;
    hi = as_h2(p1) + off;
}

// ---------------------------------------------------------------- LDS reads
// The ggml block rows sit in LDS exactly as in HBM, so a block's qs bytes are
// only 2-byte aligned.  read8_at<MOD8>() returns the 8 bytes at `off` where
// off % 8 == MOD8 is known at compile time.

template <int MOD8>
__device__ __forceinline__ u32x2 read8_at(const uint8_t* smem, uint32_t off) {
    u32x2 r;
    if constexpr (MOD8 == 0) {
        r = *(const u32x2*)(smem + off);
    } else if constexpr (MOD8 == 4) {
        r.x = *(const uint32_t*)(smem + off);
        r.y = *(const uint32_t*)(smem + off + 4);
    } else if constexpr (MOD8 == 2) {
        const u32x2 w01 = *(const u32x2*)(smem + off - 2);
        const uint32_t w2 = *(const uint32_t*)(smem + off + 6);
        r.x = alignbyte(w01.y, w01.x, 2);
        r.y = alignbyte(w2, w01.y, 2);
    } else {  // 6
        const uint32_t w0 = *(const uint32_t*)(smem + off - 2);
        const u32x2 w12 = *(const u32x2*)(smem + off + 2);
        r.x = alignbyte(w12.x, w0, 2);
        r.y = alignbyte(w12.y, w12.x, 2);
    }
    return r;
}

// 4 / 8 bytes at an LDS offset with off % 4 == MOD4 (0 or 2) known at compile
// time, by dword reads only (Q5_0's qh and qs sit 2 bytes off a dword in every
// other block)
template <int MOD4>
__device__ __forceinline__ uint32_t read4_mod4(const uint8_t* smem, uint32_t off) {
    static_assert(MOD4 == 0 || MOD4 == 2, "");
    if constexpr (MOD4 == 0) {
        return *(const uint32_t*)(smem + off);
    } else {
        const uint32_t w0 = *(const uint32_t*)(smem + off - 2);
        const uint32_t w1 = *(const uint32_t*)(smem + off + 2);
        return alignbyte(w1, w0, 2);
    }
}
template <int MOD4>
__device__ __forceinline__ u32x2 read8_mod4(const uint8_t* smem, uint32_t off) {
    static_assert(MOD4 == 0 || MOD4 == 2, "");
    u32x2 r;
    if constexpr (MOD4 == 0) {
        r.x = *(const uint32_t*)(smem + off);
        r.y = *(const uint32_t*)(smem + off + 4);
    } else {
        const uint32_t w0 = *(const uint32_t*)(smem + off - 2);
        const uint32_t w1 = *(const uint32_t*)(smem + off + 2);
        const uint32_t w2 = *(const uint32_t*)(smem + off + 6);
        r.x = alignbyte(w1, w0, 2);
        r.y = alignbyte(w2, w1, 2);
    }
    return r;
}

// Four bits (x < 16) -> bit 4 of the four bytes of a dword: bit k lands at
// 7k + k = 8k by one multiply (the 16 partial products sit at distinct bits: no carry)
__device__ __forceinline__ uint32_t bits4_to_bit4(uint32_t x) { return ((x * 0x00204081u) & 0x01010101u) << 4; }

// ---------------------------------------------------------------- wave reductions
// wave64 replacements for warp_reduce_max / warp_reduce_sum (cuda_info.h:46-85).
// Attention only needs the 4 lanes {l, l^16, l^32, l^48} that share one MFMA
// column.  gfx950's v_permlane16_swap / v_permlane32_swap exchange rows of 16 /
// halves of 32 lanes on the VALU (no LDS round trip like ds_bpermute):
// swap(a=x, b=x) leaves a = x with odd rows <- even rows and b = x with even
// rows <- odd rows, so op(a, b) is the xor-16 (resp. xor-32) reduction in every
// lane.  Written as inline asm with both registers in/out: through the
// __builtin_amdgcn_permlane*_swap intrinsics hipcc (ROCm 7.2) stores the first
// result for both when the operands are copies of one value (caught by
// tests/test_gpu_prims.py).  The s_nop covers the VALU-write -> permlane hazard,
// which the compiler does not see inside the asm.
__device__ __forceinline__ float xor16_pair(float x, bool is_max) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return is_max ? fmaxf(a, b) : a + b;
}
__device__ __forceinline__ float xor32_pair(float x, bool is_max) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return is_max ? fmaxf(a, b) : a + b;
}
__device__ __forceinline__ float grp4_max(float x) { return xor32_pair(xor16_pair(x, true), true); }
__device__ __forceinline__ float grp4_sum(float x) { return xor32_pair(xor16_pair(x, false), false); }

// Segmented reductions over contiguous power-of-two lane groups of `seg`
// lanes (seg <= 64, wave-uniform), entirely on the VALU: DPP quad_perm (xor 1,
// xor 2), row_half_mirror / row_mirror (pair the 4- / 8-lane halves once
// those are uniform), then the permlane swaps for rows / halves.  Every lane
// ends with its group's result.  EXEC must be full.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
template <bool IS_MAX>
__device__ __forceinline__ float seg_reduce(float x, int seg) {
    auto op = [](float a, float b) { return IS_MAX ? fmaxf(a, b) : a + b; };
    if (seg > 1) x = op(x, dpp_mov<0xB1>(x));   // quad_perm [1,0,3,2]
    if (seg > 2) x = op(x, dpp_mov<0x4E>(x));   // quad_perm [2,3,0,1]
    if (seg > 4) x = op(x, dpp_mov<0x141>(x));  // row_half_mirror
    if (seg > 8) x = op(x, dpp_mov<0x140>(x));  // row_mirror
    if (seg > 16) x = xor16_pair(x, IS_MAX);
    if (seg > 32) x = xor32_pair(x, IS_MAX);
    return x;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, kWave));
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m, kWave);
    return x;
}

// ---------------------------------------------------------------- sc1 memory ops
// Write-through stores / L1-bypassing loads for data handed between workgroups
// of one launch (MI355X_MICROARCH.md, inter-workgroup visibility).
// Stores: inline asm with no destination register (nothing for the compiler
// to misplace); callers drain them with an explicit s_waitcnt vmcnt(0).  The
// trailing s_nop covers the VMEM-store-data hazard (a store of more than 8
// bytes must not have its data VGPRs overwritten by the next VALU instruction):
// hipcc's hazard recognizer does not see inside inline asm, and with the
// multi-query kernel's register pressure it reused the data registers of one
// store as the address of the next at once (elements .x/.y corrupted).
__device__ __forceinline__ void st_sc1(void* p, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_sc1_x2(void* p, u32x2 v) {
    asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
// Loads of handed-off words: compiler-tracked (relaxed agent-scope atomic
// loads lower to global_load_dword(x2) ... sc1), so hipcc places every wait
// itself -- no register is live before its data has landed.
__device__ __forceinline__ u32x2 ld_sc1_x2(const void* p) {
    const uint64_t x = __hip_atomic_load((const uint64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return u32x2{(uint32_t)x, (uint32_t)(x >> 32)};
}
__device__ __forceinline__ uint32_t ld_sc1_u32(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Keeps uses of a value loaded by an UNTRACKED inline-asm load below the
// explicit wait that retires it (the split kernel's Q and mask-word prefetch,
// the only such loads left; tools/isa_hazard_check.py audits the ISA).
// Integer scalars / vectors only: with a float-vector "+v"/"=v" operand hipcc
// (ROCm 7.2) mis-assigned the elements (a bit_cast of .y read .x's register).
// The comment "RETIRED(tag) <registers>" marks, for tools/isa_hazard_check.py,
// the point from which the loads of `tag` have landed (the caller's wait sits
// just before it; volatile asm statements keep their source order).
template <int TAG, typename T>
__device__ __forceinline__ void reg_fence(T& v) {
    static_assert(!__is_same(T, f32x4) && !__is_same(T, f32x2), "float vector asm operands are miscompiled");
    asm volatile("; RETIRED(%1) %0" : "+v"(v) : "n"(TAG));
}

// ---------------------------------------------------------------- score transform
// ggml's FLASH_ATTN_EXT scalars beside `scale` (op_params[1], [2]): ALiBi
// (max_bias) and the logit soft cap.  Every kernel turns an MFMA accumulator
// s = q.k into a score at one statement, u = fma(s, scale, mask); with either
// scalar live that statement becomes xf_score():
//     x = s * scale                        (no cap)
//     x = cap * tanh(s * (scale / cap))    (cap > 0)
//     u = x + slope(h) * mask
// `live` is a kernel argument (wave-uniform): with both off the kernels keep
// their one fma and branch around this code.  The host (fill_args) fills the
// struct; live bit 1 is set only with a mask (max_bias without one changes
// nothing, as in ggml).
struct ScoreXf {
    int live;         // bit 0: soft cap, bit 1: ALiBi slopes; 0: u = s * scale + mask
    float cap;        // logit_softcap
    float scale_cap;  // scale / cap
    // log2 of ggml's slope bases m0 = 2^-(max_bias / n2), m1 = 2^-(max_bias / 2 / n2),
    // n2 = 2^floor(log2 n_head_total): slope(h) = m0^(h + 1) for h < n2, else m1^(2 (h - n2) + 1)
    float m0_log2, m1_log2;
    int n2;
    int head_first;   // global index of q head 0 (head-sharded launches)
};

// slope of q head iq2 (the launch's index): one v_exp_f32, once per lane and
// kernel.  Always > 0, so a -inf mask value stays -inf and +-0 stays +-0.
__device__ __forceinline__ float xf_slope(const ScoreXf& x, int iq2) {
    if (!(x.live & 2)) return 1.0f;
    const int h = x.head_first + iq2;
    const float e = h < x.n2 ? x.m0_log2 * (float)(h + 1) : x.m1_log2 * (float)(2 * (h - x.n2) + 1);
    return __builtin_amdgcn_exp2f(e);
}

// the score (natural units) of accumulator s under mask value m.  tanh from
// v_exp_f32 / v_rcp_f32, no libm: tanh(t) = 1 - 2 / (1 + 2^(2 log2e t)), which
// saturates to +-1 exactly as the exponential overflows to inf or underflows
// to 0.  Both instructions are good to 1 ulp, and for small t the subtraction
// from 1 leaves an absolute error of about 1e-7 in tanh, so about cap * 1e-7
// in the logit -- 4e-5 at cap = 400, far below the f16 rounding of P.
__device__ __forceinline__ float xf_score(const ScoreXf& x, float scale, float s, float m, float slope) {
    float v;
    if (x.live & 1) {
        const float e = __builtin_amdgcn_exp2f(s * x.scale_cap * 2.8853900817779268f);
        v = __builtin_fmaf(-2.0f * x.cap, __builtin_amdgcn_rcpf(1.0f + e), x.cap);
    } else {
        v = s * scale;
    }
    return __builtin_fmaf(slope, m, v);
}

// ---------------------------------------------------------------- attention sinks
// ggml's FLASH_ATTN_EXT src[4]: one extra logit per q head that joins the
// softmax denominator and has no value row (include/fattn.h).  Every kernel
// ends a row with a state (M, L, acc): M the reference max in log2 units, L =
// sum 2^(score - M), acc = sum 2^(score - M) v.  With the raw sink s
// (natural units: not scaled, capped or sloped) the row is
//     acc / (L + 2^(s log2e - M)),
// so sink_inv() returns the factor that stands where 1 / L stood, once per
// output row, at the sites that normalise into dst (never where a chunk
// partial is published).  Overflow-safe form: with mm = max(M, s'),
// e = 2^(M - mm), the factor is e / (L e + 2^(s' - mm)) -- both exponents
// <= 0 and one of them 0, so the denominator lies in [min(L, 1), L + 1] and no
// finite sink gives inf or NaN; a sink far above M gives e = 0 and a zero
// row, one far below (or -inf: no sink) gives 1 / L.
// `dead`: the row's mask was -inf everywhere (M = -inf, L = 0; the factor is
// NaN then, and acc may be too).  ggml's row is S = 1, VKQ = 0: the caller
// writes zeros by selection, sink_row().
__device__ __forceinline__ float sink_inv(float M, float L, float sink, bool& dead) {
    const float s = sink * 1.4426950408889634f;
    dead = !(L > 0.0f) || M == -__builtin_inff();
    const float mm = fmaxf(M, s);
    const float e = __builtin_amdgcn_exp2f(M - mm);
    return e / __builtin_fmaf(L, e, __builtin_amdgcn_exp2f(s - mm));
}
__device__ __forceinline__ float sink_row(float acc, float inv, bool dead) { return dead ? 0.0f : acc * inv; }
__device__ __forceinline__ f32x4 sink_row(f32x4 acc, float inv, bool dead) {
    return dead ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : acc * inv;
}

// ---------------------------------------------------------------- row log-sum-exp
// fattn_ext_lse: the natural-log LSE of a row's final scores from the state
// (M, L) the row is normalised with, ln2 (M + log2 L); with a raw sink s
// (-inf: none) the sink is one more term, in sink_inv()'s overflow-safe form:
// mm = max(M, s'), ln2 (mm + log2(L 2^(M - mm) + 2^(s' - mm))) -- with s =
// -inf that is L * 1 + 0, the sinkless value bit for bit.  `dead` (sink_inv's:
// no live key) selects the sink itself -- -inf without one --, never the
// outcome of -inf + -inf or of a NaN L.  Called once per output row behind a
// wave-uniform `if (lse_of(a))`, after the row's dst stores (SplitArgsLse, fattn_tile.h).
__device__ __forceinline__ bool row_dead(float M, float L) { return !(L > 0.0f) || M == -__builtin_inff(); }
__device__ __forceinline__ float row_lse(float M, float L, float sink, bool dead) {
    const float s = sink * 1.4426950408889634f;
    const float mm = fmaxf(M, s);
    const float t = __builtin_fmaf(L, __builtin_amdgcn_exp2f(M - mm), __builtin_amdgcn_exp2f(s - mm));
    return dead ? sink : 0.6931471805599453f * (mm + __builtin_amdgcn_logf(t));
}

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- bf16 operands
// v_mfma_f32_16x16x32_bf16 over a BF16 cache.  The operands travel as the f16x8
// register images the f16 path uses (the LDS reads move bits); K and V enter
// exactly.  The f32 B operand (Q, P) enters as TWO bf16 vectors, hi = bf16(x)
// and lo = bf16(x - hi), both round-to-nearest-even (v_cvt_pk_bf16_f32), and
// each k-step issues two MFMAs into one accumulator: 16 operand bits where one
// bf16 has 8 and f16 has 11
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 mfma16_bf(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// x[0..7] -> (hi, lo) bf16 vectors (as f16x8 register images)
__device__ __forceinline__ void bf16_split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        h[j] = (__bf16)x[j];
        l[j] = (__bf16)(x[j] - (float)h[j]);  // exact difference (|x - hi| <= ulp_bf16 / 2), then one rounding
    }
    hi = __builtin_bit_cast(f16x8, h);
    lo = __builtin_bit_cast(f16x8, l);
}

}  // namespace fattn
