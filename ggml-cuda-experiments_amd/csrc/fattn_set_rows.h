// fattn_set_rows.h -- GGML_OP_SET_ROWS f32 -> F16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1:
// the KV-cache write by slot index (include/fattn.h fattn_set_rows).
//
// Layout: EIGHT LANES PER 32-ELEMENT BLOCK.  Lane l of a group holds elements
// 4l .. 4l+3, one 16-B load, so a wave's load instruction covers 1 KiB of
// contiguous row (8 blocks) where the one-thread-per-block kernel of
// fattn_quant.h has neighbouring lanes 128 B apart.  The unit is (row, block in
// row), numbered over one [ne0, nr] plane: short rows pack several rows into a
// wave, long rows span waves; (i2, i3) come from the grid's y / z.  The eight
// lanes load the same index word.  Large writes give each lane group four units,
// 32 apart, with all their loads issued first (set_rows_kernel's K).
//
// The block statistics stay in registers: each lane scans its four elements as
// the sequential reference does, then a 3-step xor butterfly (DPP quad_perm for
// xor 1 / 2, ds_swizzle for xor 4; no LDS memory) merges the eight partial
// results.  The merges reproduce the reference's strict-compare scans bit for
// bit -- see merge_amax / merge_min / merge_max.  The arithmetic after them is
// that of quant_block_* (fattn_quant.h): contraction off, the same opaque()
// barriers, the same truncations and clamps.
//
// Packing: element j shares a byte with j + 16, i.e. lane l with lane l + 4: one
// exchange of the four packed codes.  qh is an OR-reduction of four bits per
// lane.  dst is only 2-byte aligned (blocks are 18 .. 34 B), so the block goes
// out as 2-byte stores spread over the lanes: qs two bytes per lane (Q8_0 four),
// d / m / qh from lanes 0 .. 3.  F16 rows use dword stores where the address
// allows.
//
// No lane leaves before the cross-lane steps: a unit past the end, or one whose
// slot is out of range, computes on zeros and skips only its stores.
#pragma once

#include "fattn_quant.h"

namespace fattn {

struct SetRowsArgs {
    const uint8_t* src;
    const uint8_t* idx;
    uint8_t* dst;
    int64_t ne0, n_slots, ne2, ne3, ne11, ne12;
    int64_t snb1, snb2, snb3;
    int64_t inb0, inb1, inb2;
    int64_t dnb1, dnb2, dnb3;
    uint32_t upr;    // units (32-element blocks; the last may be partial for F16) per row
    uint32_t units;  // upr * nr, <= 2^31 - 1
    int32_t idx64;   // index element: 1 = I64, 0 = I32
    int32_t dst_small;  // n_slots and dst nb[1] are both below 2^32
    // 32 units further on (the next pass of a lane group): r32 = 32 % upr blocks and
    // 32 / upr rows, one row more and upr blocks less when the block index wraps.
    // ds_*: src byte deltas, di_*: index byte deltas, dd_*: dst deltas in units
    uint32_t r32;
    int64_t ds_next, ds_wrap, di_next, di_wrap, dd_next, dd_wrap;
};

// the value of lane (l ^ S), S = 1, 2 or 4
template <int S>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v) {
    static_assert(S == 1 || S == 2 || S == 4, "");
    if constexpr (S == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    else if constexpr (S == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (4 << 10) | 0x1F);  // bit mode: and 0x1F, or 0, xor 4
}
template <int S>
__device__ __forceinline__ float xor_lane(float v) {
    return __builtin_bit_cast(float, xor_lane<S>(__builtin_bit_cast(uint32_t, v)));
}

// One butterfly step of `if (amax < |x|) { amax = |x|; mx = x; }` (Q4_0 / Q5_0):
// the FIRST element of largest |x| wins.  The partner's group of S lanes lies
// wholly below this lane's (l & S) or wholly above it; on equal |x| the lower
// group's element is kept, as the sequential scan keeps the earlier one.  amax
// is never NaN (a NaN never passes the strict compare), so `!(p < a)` is `a <= p`.
template <int S>
__device__ __forceinline__ void merge_amax(float& amax, float& mx, int l) {
    const float pa = xor_lane<S>(amax), pm = xor_lane<S>(mx);
    const bool take = (l & S) ? !(pa < amax) : (amax < pa);
    amax = take ? pa : amax;
    mx = take ? pm : mx;
}
// `if (x < mn) mn = x` / `if (x > mxv) mxv = x` (Q4_1 / Q5_1): the first of equal
// values is kept, and -0.0 == +0.0 is equal -- compare-and-select with the lane
// order as the tie-break; v_min_f32 / v_max_f32 order the two zeros and would
// change the sign of a zero m (and of a zero d).
template <int S>
__device__ __forceinline__ void merge_min(float& mn, int l) {
    const float p = xor_lane<S>(mn);
    const bool take = (l & S) ? !(mn < p) : (p < mn);
    mn = take ? p : mn;
}
template <int S>
__device__ __forceinline__ void merge_max(float& mxv, int l) {
    const float p = xor_lane<S>(mxv);
    const bool take = (l & S) ? !(mxv > p) : (p > mxv);
    mxv = take ? p : mxv;
}
template <int S>
__device__ __forceinline__ void merge_or(uint32_t& v) {
    v |= xor_lane<S>(v);
}

__device__ __forceinline__ void store_u16(uint8_t* p, uint32_t v) { *(uint16_t*)p = (uint16_t)v; }

// The lane's share of one block of type T: x = elements 4l .. 4l+3; `write`
// guards every store (the cross-lane steps run regardless).
template <int T>
__device__ __forceinline__ void set_rows_block(const float (&x)[4], int l, bool write, uint8_t* blk) {
#pragma clang fp contract(off)
    if constexpr (T == FATTN_TYPE_Q8_0) {
        float amax = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) amax = fmaxf(amax, fabsf(x[k]));
        amax = fmaxf(amax, xor_lane<1>(amax));  // by value: no tie rule
        amax = fmaxf(amax, xor_lane<2>(amax));
        amax = fmaxf(amax, xor_lane<4>(amax));
        const float d = amax / 127.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        const uint32_t dh = __builtin_bit_cast(uint16_t, (f16)opaque(d));
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) w |= (uint32_t)(uint8_t)(int8_t)roundf(x[k] * id) << (8 * k);
        if (write) {
            if (l == 0) store_u16(blk, dh);
            store_u16(blk + 2 + 4 * l, w);
            store_u16(blk + 4 + 4 * l, w >> 16);
        }
    } else {
        float d, mn = 0.0f;
        if constexpr (!has_min(T)) {
            float amax = 0.0f, mx = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (amax < fabsf(x[k])) {
                    amax = fabsf(x[k]);
                    mx = x[k];
                }
            }
            merge_amax<1>(amax, mx, l);
            merge_amax<2>(amax, mx, l);
            merge_amax<4>(amax, mx, l);
            d = mx * (T == FATTN_TYPE_Q4_0 ? -0.125f : -0.0625f);  // == mx / -8 (-16) exactly, keeps -0.0
        } else {
            float mxv = -3.402823466e+38f;
            mn = 3.402823466e+38f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (x[k] < mn) mn = x[k];
                if (x[k] > mxv) mxv = x[k];
            }
            merge_min<1>(mn, l);
            merge_max<1>(mxv, l);
            merge_min<2>(mn, l);
            merge_max<2>(mxv, l);
            merge_min<4>(mn, l);
            merge_max<4>(mxv, l);
            d = opaque(mxv - mn) / (T == FATTN_TYPE_Q4_1 ? 15.0f : 31.0f);
        }
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        const uint32_t dh = __builtin_bit_cast(uint16_t, (f16)opaque(d));
        uint32_t w = 0;  // the four codes, one per byte
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t q;
            if constexpr (T == FATTN_TYPE_Q4_0) {
                const int8_t t = (int8_t)(opaque(x[k] * id) + 8.5f);
                q = (uint8_t)(t < 15 ? t : 15);
            } else if constexpr (T == FATTN_TYPE_Q5_0) {
                const int8_t t = (int8_t)(opaque(x[k] * id) + 16.5f);
                q = (uint32_t)(t < 31 ? t : 31) & 0xFFu;
            } else if constexpr (T == FATTN_TYPE_Q4_1) {
                const int8_t t = (int8_t)(opaque(opaque(x[k] - mn) * id) + 0.5f);
                q = (uint32_t)(t < 15 ? t : 15) & 0xFFu;
            } else {
                q = (uint8_t)(opaque(opaque(x[k] - mn) * id) + 0.5f);
            }
            w |= q << (8 * k);
        }
        // lanes l and l ^ 4 hold elements j and j + 16 of bytes qs[4(l&3) .. 4(l&3)+3]
        const uint32_t pw = xor_lane<4>(w);
        const uint32_t lo = l < 4 ? w : pw, hi = l < 4 ? pw : w;
        // (Q4_0 keeps the low code whole, as quant_block_q4_0's `q0 | (q1 << 4)` does)
        const uint32_t qs = (T == FATTN_TYPE_Q4_0 ? lo : lo & 0x0F0F0F0Fu) | ((hi & 0x0F0F0F0Fu) << 4);
        uint32_t qh = 0;
        if constexpr (has_qh(T)) {
            // bit 4 of code k -> bit 4l + k
            qh = (((w >> 4) & 1u) | ((w >> 11) & 2u) | ((w >> 18) & 4u) | ((w >> 25) & 8u)) << (4 * l);
            merge_or<1>(qh);
            merge_or<2>(qh);
            merge_or<4>(qh);
        }
        if (write) {
            store_u16(blk + qs_off(T) + 4 * (l & 3) + (l < 4 ? 0 : 2), l < 4 ? qs : qs >> 16);
            if (l == 0) store_u16(blk, dh);
            if constexpr (has_min(T)) {
                const uint32_t mh = __builtin_bit_cast(uint16_t, (f16)opaque(mn));
                if (l == 1) store_u16(blk + 2, mh);
            }
            if constexpr (has_qh(T)) {
                if (l == 2) store_u16(blk + qh_off(T), qh);
                if (l == 3) store_u16(blk + qh_off(T) + 2, qh >> 16);
            }
        }
    }
}

// T: the dst type; VEC: src base and nb[1..3] are 16-B multiples (one 16-B load
// per lane), else the dword path (the same lane-to-element mapping, four loads);
// K: units per lane group.  A workgroup takes 32 K consecutive units, its pass j
// the units base + 32 j + (thread / 8): every load instruction of a wave still
// covers 8 consecutive blocks.  The K index and source loads are all issued
// before the first conversion -- with K = 1 a wave has 1 KiB in flight and large
// writes are bound by memory latency, not bandwidth; the host
// picks K = 4 once there are units enough to fill the chip that way.
// Grid: x = ceil(units / (32 K)), y / z stride over ne2 / ne3.
template <int T, bool VEC, int K>
__global__ __launch_bounds__(256) void set_rows_kernel(const SetRowsArgs a) {
    constexpr bool kF16 = T == FATTN_TYPE_F16;
    constexpr int kBB = TypeInfo<T>::block_bytes * (kF16 ? QK : 1);  // dst bytes of one whole unit
    const int l = threadIdx.x & 7;
    // Per pass j, independent of the plane: whether the unit exists, its index
    // row, and the byte offsets of the lane's share in the src row, of the index
    // and of the unit in the dst row.  Pass 0 pays the one division; pass j + 1
    // is 32 units on: (q32, r32) = (32 / upr, 32 % upr) rows and blocks further,
    // with at most one wrap -- offsets move by uniform deltas the host worked
    // out, no per-pass multiply (64-bit and 32-bit integer multiplies are
    // quarter rate, and this kernel is bound by its VALU work once the loads
    // overlap).
    bool in_range[K];
    int64_t soff[K], ioff[K], doff[K];
    int n[K];  // elements of the lane (4; less in an F16 tail)
    {
        const uint32_t u0 = blockIdx.x * (32u * K) + (threadIdx.x >> 3);
        const uint32_t i0 = u0 / a.upr;
        uint32_t bj = u0 - i0 * a.upr;
        soff[0] = (int64_t)i0 * a.snb1 + ((int64_t)bj * QK + 4 * l) * 4;
        ioff[0] = (int64_t)i0 * a.inb0;
        doff[0] = (int64_t)bj * kBB;
#pragma unroll
        for (int j = 0; j < K; j++) {
            in_range[j] = u0 + 32u * j < a.units;
            n[j] = 4;
            if constexpr (kF16) {
                const int64_t left = a.ne0 - ((int64_t)bj * QK + 4 * l);
                n[j] = (int)(left < 4 ? (left > 0 ? left : 0) : 4);
            }
            if (j + 1 < K) {
                const uint32_t bn = bj + a.r32;
                const bool wrap = bn >= a.upr;
                bj = wrap ? bn - a.upr : bn;
                soff[j + 1] = soff[j] + (wrap ? a.ds_wrap : a.ds_next);
                ioff[j + 1] = ioff[j] + (wrap ? a.di_wrap : a.di_next);
                doff[j + 1] = doff[j] + (wrap ? a.dd_wrap : a.dd_next) * kBB;
            }
        }
    }
    for (int64_t i3 = blockIdx.z; i3 < a.ne3; i3 += gridDim.z) {
        const int64_t i13 = a.ne12 == 1 ? 0 : a.ne12 == a.ne3 ? i3 : i3 % a.ne12;
        for (int64_t i2 = blockIdx.y; i2 < a.ne2; i2 += gridDim.y) {
            const int64_t i12 = a.ne11 == 1 ? 0 : a.ne11 == a.ne2 ? i2 : i2 % a.ne11;
            const uint8_t* splane = a.src + i2 * a.snb2 + i3 * a.snb3;
            const uint8_t* iplane = a.idx + i12 * a.inb1 + i13 * a.inb2;
            uint8_t* dplane = a.dst + i2 * a.dnb2 + i3 * a.dnb3;
            int64_t slot[K];
            float x[K][4];
#pragma unroll
            for (int j = 0; j < K; j++) {
                slot[j] = -1;
#pragma unroll
                for (int k = 0; k < 4; k++) x[j][k] = 0.0f;
                if (in_range[j]) {
                    const uint8_t* ip = iplane + ioff[j];
                    slot[j] = a.idx64 ? *(const int64_t*)ip : (int64_t)*(const int32_t*)ip;
                    const float* xp = (const float*)(splane + soff[j]);
                    if (VEC && n[j] == 4) {
                        const f32x4 v = *(const f32x4*)xp;
                        x[j][0] = v.x; x[j][1] = v.y; x[j][2] = v.z; x[j][3] = v.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (k < n[j]) x[j][k] = xp[k];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < K; j++) {
                // 64-bit compare before any address arithmetic: negative and >= n_slots both fail
                const bool write = (uint64_t)slot[j] < (uint64_t)a.n_slots;
                // (dst_small: n_slots and nb[1] below 2^32 -- one 32 x 32 -> 64 multiply)
                const int64_t roff = !write ? 0
                                     : a.dst_small ? (int64_t)((uint64_t)(uint32_t)slot[j] * (uint32_t)a.dnb1)
                                                   : slot[j] * a.dnb1;
                uint8_t* blk = dplane + roff + doff[j];
                if constexpr (kF16) {
                    uint32_t h[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) h[k] = __builtin_bit_cast(uint16_t, (f16)x[j][k]);
                    uint8_t* y = blk + 8 * l;
                    if (write) {
                        if (n[j] == 4 && ((uintptr_t)y & 3) == 0) {
                            *(uint32_t*)y = h[0] | (h[1] << 16);
                            *(uint32_t*)(y + 4) = h[2] | (h[3] << 16);
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; k++)
                                if (k < n[j]) store_u16(y + 2 * k, h[k]);
                        }
                    }
                } else {
                    set_rows_block<T>(x[j], l, write, blk);
                }
            }
        }
    }
}

// units per lane group of the large-write form, and the unit count from which the host takes it
constexpr int kSetRowsUnroll = 4;

}  // namespace fattn
