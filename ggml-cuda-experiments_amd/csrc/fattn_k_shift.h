// fattn_k_shift.h -- the K-shift of llama.cpp's build_rope_shift: the RoPE
// rotation of a K cache IN PLACE by a per-slot position delta, for an F32 / F16 /
// BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 cache (include/fattn.h fattn_k_shift,
// DESIGN.md §20).  One launch reads each cache block once, dequantises it into
// registers, rotates it, requantises it with ggml's rules and writes it back:
// no f32 temporary, no LDS memory.
//
// Layout: that of fattn_set_rows.h -- EIGHT LANES PER 32-ELEMENT BLOCK, lane l
// holding elements 4l .. 4l+3 -- so the store half is set_rows_block<T>
// unchanged (butterfly, tie rules).  A ROW NEVER LEAVES ITS WAVE: ne0 <= 256 is
// at most eight blocks = 64 lanes; a row of upr blocks takes upr lane groups
// and a wave holds 8 / upr rows (lane groups past them idle: they compute on
// zeros and skip their loads and stores).  The unit of the grid's x is the
// wave, numbered over the slots; y strides over the heads, z over the
// sequences.
//
// Pairs.  NORMAL pairs (2i, 2i+1) sit inside a lane.  A NEOX pair (i, i +
// n_dims/2) spans two lanes n_dims/8 apart in the same wave (n_dims % 8 == 0:
// the four elements of a lane have their partners in ONE lane): the partner's
// four values come by ds_bpermute.  Each lane needs four angles there and its
// partner the same four; each computes two and they exchange (sin, cos), so
// both modes cost two powf + two sincosf per lane and angle set.
//
// Heads share the angle: the shift is a function of (slot, sequence), so a lane
// computes its angles once per sequence and walks the heads its grid row owns
// with them (the host decides how many: kKShiftFullWaves).
//
// In place without ordering between lanes: every cache byte is loaded by lanes
// of the ONE wave that stores it, in load instructions that precede the stores
// in program order, and every store's data depends on those loads (a block's
// d / m / qh words are read by all eight of its lanes and all eight depend on
// them through the scale), so the wave's wait for its loads precedes its first
// store.  Rows of different waves do not overlap (the caller's contract).  No
// pointer is __restrict__: the next head's loads stay behind this head's stores.
#pragma once

#include "fattn_set_rows.h"

namespace fattn {

struct KShiftArgs {
    uint8_t* k;
    const uint8_t* shift;
    const float* ff;     // freq_factors or NULL
    int64_t knb1, knb2, knb3;
    int64_t snb0, snb1;  // shift strides in bytes (snb1 = 0 with one plane)
    int64_t n_slots;
    int32_t ne2, ne3, ns;
    uint32_t upr, rpw;   // blocks per row (the last may be partial for F32 / F16 / BF16), rows per wave
    // ggml's rope_yarn parameters, the launch-constant part worked out on the host
    int32_t n_dims;
    float theta_scale;   // powf(freq_base, -2 / n_dims)
    float freq_scale, ext_factor;
    float m;             // attn_factor (* (1 + 0.1 logf(1 / freq_scale)) when ext_factor != 0)
    float lo, den;       // corr dims: low, max(0.001, high - low)
};

// (cos, sin) of pair i at position delta p: ggml's rope_yarn, every operation
// rounded on its own, sincosf / powf the accurate library functions
__device__ __forceinline__ void k_shift_angle(const KShiftArgs& a, int p, int i, float& c, float& s) {
#pragma clang fp contract(off)
    float theta_extrap = (float)p * powf(a.theta_scale, (float)i);
    if (a.ff) theta_extrap = theta_extrap / a.ff[i];
    float theta = a.freq_scale * theta_extrap;
    if (a.ext_factor != 0.0f) {
        const float y = ((float)i - a.lo) / a.den;
        const float mix = (1.0f - fminf(1.0f, fmaxf(0.0f, y))) * a.ext_factor;
        theta = opaque(theta * (1.0f - mix)) + opaque(theta_extrap * mix);
    }
    sincosf(theta, &s, &c);
}

// THE rotation, shared by every cache type: equal x, angle and m give the same
// f32 y whatever block it came from
__device__ __forceinline__ void k_shift_rotate(float x0, float x1, float c, float s, float m, float& y0, float& y1) {
#pragma clang fp contract(off)
    y0 = opaque(opaque(x0 * c) * m) - opaque(opaque(x1 * s) * m);
    y1 = opaque(opaque(x0 * s) * m) + opaque(opaque(x1 * c) * m);
}

// The load half: the lane's four dequantised elements 4l .. 4l+3 of the block at
// blk, with the arithmetic of dequant_block<T>.  Blocks are only 2-byte aligned:
// every access is a 16-bit load.
template <int T>
__device__ __forceinline__ void k_shift_load_block(const uint8_t* blk, int l, float (&x)[4]) {
#pragma clang fp contract(off)
    static_assert(is_quant(T), "");
    const uint16_t* h = (const uint16_t*)blk;
    const float d = (float)__builtin_bit_cast(f16, h[0]);
    if constexpr (T == FATTN_TYPE_Q8_0) {
        const uint32_t w = (uint32_t)h[1 + 2 * l] | ((uint32_t)h[2 + 2 * l] << 16);
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = (float)(int8_t)(w >> (8 * k)) * d;
    } else {
        constexpr int zero = T == FATTN_TYPE_Q4_0 ? 8 : code_zero(T);
        // elements j and j + 16 share byte qs[j]: lanes l and l ^ 4 read the same four bytes
        const int o = qs_off(T) / 2 + 2 * (l & 3);
        const uint32_t w = (uint32_t)h[o] | ((uint32_t)h[o + 1] << 16);
        const uint32_t nib = (l < 4 ? w : w >> 4) & 0x0F0F0F0Fu;
        uint32_t hb = 0;  // the fifth bits of the four elements: bits 4l .. 4l+3 of qh
        if constexpr (has_qh(T)) hb = ((uint32_t)h[qh_off(T) / 2 + (l >> 2)] >> (4 * (l & 3))) & 0xFu;
        float m = 0.0f;
        if constexpr (has_min(T)) m = (float)__builtin_bit_cast(f16, h[1]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = (int)(((nib >> (8 * k)) & 0xFu) | (((hb >> k) & 1u) << 4));
            if constexpr (has_min(T)) x[k] = opaque((float)q * d) + m;
            else x[k] = (float)(q - zero) * d;
        }
    }
}

// F32 / F16 / BF16: four elements at p; VEC: p is 16-B (F32) / 8-B (16-bit types) aligned
template <int T, bool VEC>
__device__ __forceinline__ void k_shift_load_elems(const uint8_t* p, float (&x)[4]) {
    if constexpr (T == FATTN_TYPE_F32) {
        if constexpr (VEC) {
            const f32x4 v = *(const f32x4*)p;
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = ((const float*)p)[k];
        }
    } else {
        uint32_t hb[4];
        if constexpr (VEC) {
            const u32x2 v = *(const u32x2*)p;
            hb[0] = v.x & 0xFFFFu; hb[1] = v.x >> 16; hb[2] = v.y & 0xFFFFu; hb[3] = v.y >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) hb[k] = ((const uint16_t*)p)[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (T == FATTN_TYPE_F16) x[k] = (float)__builtin_bit_cast(f16, (uint16_t)hb[k]);
            else x[k] = __builtin_bit_cast(float, hb[k] << 16);
        }
    }
}
// ... and their store: y itself, f16 round-to-nearest-even, or the BF16 rule of fattn_quantize
template <int T, bool VEC>
__device__ __forceinline__ void k_shift_store_elems(uint8_t* p, const float (&y)[4]) {
    if constexpr (T == FATTN_TYPE_F32) {
        if constexpr (VEC) {
            *(f32x4*)p = f32x4{y[0], y[1], y[2], y[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) ((float*)p)[k] = y[k];
        }
    } else {
        uint32_t hb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (T == FATTN_TYPE_F16) hb[k] = __builtin_bit_cast(uint16_t, (f16)opaque(y[k]));
            else hb[k] = f32_to_bf16_bits(y[k]);
        }
        if constexpr (VEC) {
            *(u32x2*)p = u32x2{hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16)};
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) store_u16(p + 2 * k, hb[k]);
        }
    }
}

__device__ __forceinline__ float lane_read(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(lane << 2, __builtin_bit_cast(int, v)));
}

// T: the cache type; NEOX: pairs (i, i + n_dims/2), else (2i, 2i+1); VEC (F32 /
// F16 / BF16 only): every row base is a multiple of 16 / 8 bytes.
// Grid: x = ceil(waves / 4) with waves = ceil(n_slots / rpw); y strides over ne2, z over ne3.
template <int T, bool NEOX, bool VEC>
__global__ __launch_bounds__(256) void k_shift_kernel(const KShiftArgs a) {
    constexpr bool kBlock = is_quant(T);
    constexpr int kBB = kBlock ? TypeInfo<T>::block_bytes : QK * TypeInfo<T>::block_bytes;  // bytes of 32 elements
    const int lane = threadIdx.x & 63, l = lane & 7;
    const uint32_t g = (uint32_t)lane >> 3;
    const uint32_t rw = g / a.upr, b = g - rw * a.upr;  // row of the wave, block of the row
    const int64_t n = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * a.rpw + rw;
    const bool row_ok = rw < a.rpw && n < a.n_slots;
    const int e = (int)b * QK + 4 * l;  // the lane's first element
    // (n_dims % 8 == 0 and e % 4 == 0: a lane's four elements rotate together or not at all)
    const bool rot = e < a.n_dims;
    // what the launch rewrites: whole blocks that begin below n_dims; F32 / F16 / BF16 the rotated elements only
    const bool mine = kBlock ? (int)b * QK < a.n_dims : rot;
    const int hd = a.n_dims >> 1;
    const bool low = e < hd;  // NEOX: this lane holds x0 (else x1) of its pairs
    // the two angles this lane computes: NORMAL its own pairs e/2, e/2 + 1; NEOX two of the
    // four it shares with its partner (the low lane the first two)
    int ia = 0, partner = lane;
    if (rot) {
        if constexpr (NEOX) {
            ia = low ? e : e - hd + 2;
            partner = low ? lane + (a.n_dims >> 3) : lane - (a.n_dims >> 3);
        } else {
            ia = e >> 1;
        }
    }
    const int64_t roff = n * a.knb1 + (int64_t)b * kBB + (kBlock ? 0 : l * 4 * TypeInfo<T>::block_bytes);
    for (int64_t i3 = blockIdx.z; i3 < a.ne3; i3 += gridDim.z) {
        int p = 0;
        if (row_ok) p = *(const int32_t*)(a.shift + n * a.snb0 + (a.ns == 1 ? 0 : i3 % a.ns) * a.snb1);
        const bool touch = row_ok && p != 0 && mine;
        if (__builtin_amdgcn_ballot_w64(touch) == 0) continue;  // (wave-uniform: nothing of this wave's rows moves)
        float c[NEOX ? 4 : 2], s[NEOX ? 4 : 2];
        {
            float c0, s0, c1, s1;
            k_shift_angle(a, p, ia, c0, s0);
            k_shift_angle(a, p, ia + 1, c1, s1);
            if constexpr (NEOX) {
                const float pc0 = lane_read(c0, partner), ps0 = lane_read(s0, partner);
                const float pc1 = lane_read(c1, partner), ps1 = lane_read(s1, partner);
                c[0] = low ? c0 : pc0; s[0] = low ? s0 : ps0;
                c[1] = low ? c1 : pc1; s[1] = low ? s1 : ps1;
                c[2] = low ? pc0 : c0; s[2] = low ? ps0 : s0;
                c[3] = low ? pc1 : c1; s[3] = low ? ps1 : s1;
            } else {
                c[0] = c0; s[0] = s0; c[1] = c1; s[1] = s1;
            }
        }
        for (int64_t i2 = blockIdx.y; i2 < a.ne2; i2 += gridDim.y) {
            uint8_t* q = a.k + roff + i2 * a.knb2 + i3 * a.knb3;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4];
            if (touch) {
                if constexpr (kBlock) k_shift_load_block<T>(q, l, x);
                else k_shift_load_elems<T, VEC>(q, x);
            }
            if constexpr (NEOX) {
                float xp[4];
#pragma unroll
                for (int k = 0; k < 4; k++) xp[k] = lane_read(x[k], partner);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float y0, y1;
                    k_shift_rotate(low ? x[k] : xp[k], low ? xp[k] : x[k], c[k], s[k], a.m, y0, y1);
                    y[k] = rot ? (low ? y0 : y1) : x[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    float y0, y1;
                    k_shift_rotate(x[2 * k], x[2 * k + 1], c[k], s[k], a.m, y0, y1);
                    y[2 * k] = rot ? y0 : x[2 * k];
                    y[2 * k + 1] = rot ? y1 : x[2 * k + 1];
                }
            }
            if constexpr (kBlock) {
                set_rows_block<T>(y, l, touch, q);
            } else {
                if (touch) k_shift_store_elems<T, VEC>(q, y);
            }
        }
    }
}

// Waves below which the heads are spread over the grid's y instead of walked by
// one lane group: 256 CUs x 4 SIMDs x 8 waves.  Past it the chip is full either
// way and the walk computes each slot's angles once for all its heads.
constexpr int64_t kKShiftFullWaves = 8192;

}  // namespace fattn
