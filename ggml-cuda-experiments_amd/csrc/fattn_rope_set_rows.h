// fattn_rope_set_rows.h -- ggml_rope_ext + GGML_OP_SET_ROWS for K and
// GGML_OP_SET_ROWS for V in ONE launch: the write side of a decode step
// (include/fattn.h fattn_rope_set_rows).  k_cur is rotated in
// registers and requantised with ggml's rules; no f32 row is ever written.
//
// One grid, two parts.  Workgroups [0, nk) of grid x take K, the rest take V
// (the branch is uniform per workgroup); y strides over the heads of either
// part, z over the sequences.  The two dst types are run-time values in SGPRs:
// rsr_store() switches on them once per unit, one inlined body per type, so the
// kernel count is MODE x VEC x U and not K type x V type.
//
// Lanes: fattn_set_rows.h's EIGHT LANES PER 32-ELEMENT BLOCK, lane l holding
// elements 4l .. 4l+3 from one 16-B source load; the store half is
// set_rows_block<T> unchanged, the F32 / F16 / BF16 stores fattn_k_shift.h's.
//
// V, and K without a rope (MODE 0), are set_rows_kernel's units: (row, block in
// row) numbered over one [ne0, nr] plane; a large rope-less write gives a lane
// group U = 4 units with every index and source load issued before the first
// conversion (rsr_plain_units).
//
// A rotated K row (MODE 1 / 2) never leaves its wave, as in fattn_k_shift.h:
// upr <= 8 lane groups per row, 8 / upr rows per wave, the wave the unit of grid
// x.  NORMAL pairs sit inside a lane.  A NEOX partner's four values come by a
// SECOND 16-B LOAD of the source -- it is read-only here, and the line is the
// one a neighbouring lane group of the same wave has just fetched -- instead of
// the K-shift's four ds_bpermute per head; the angles still cross by
// ds_bpermute, two computed per lane and two received, so NEOX costs what
// NORMAL does.  The angle depends on (token, pos plane, pair) only: a lane
// computes it once per sequence and walks the heads its grid row owns
// (rsr_rope_rows).
//
// No lane leaves before the cross-lane steps: a lane group past the end, or one
// whose slot is out of range, computes on zeros and skips only its stores.
#pragma once

#include "fattn_k_shift.h"

namespace fattn {

struct RopeSetRowsArgs {
    // The two parts, as fattn_set_rows describes one -- except that dd_next /
    // dd_wrap are BYTES here (the unit's dst bytes are a run-time value).
    // v.units == 0: a K-only launch.
    SetRowsArgs k, v;
    int32_t kt, vt;      // dst types
    int32_t kbb, vbb;    // dst bytes of one whole 32-element unit
    uint32_t nk;         // workgroups of grid x that take K
    // the rotated form of K: pos[nr, np], rows per wave, and the rope (the fields k_shift_angle reads)
    const uint8_t* pos;
    int64_t pnb0, pnb1;  // (pnb1 = 0 with one plane)
    int64_t nr;
    int32_t np;
    uint32_t rpw;
    KShiftArgs rope;
};

// F32 / F16 / BF16: the lane's n <= 4 elements at p (fattn_k_shift.h's stores; a row's tail element by element)
template <int T>
__device__ __forceinline__ void rsr_store_elems(uint8_t* p, const float (&y)[4], int n) {
    constexpr int eb = TypeInfo<T>::block_bytes;
    if (n == 4) {
        if (((uintptr_t)p & (4 * eb - 1)) == 0) k_shift_store_elems<T, true>(p, y);
        else k_shift_store_elems<T, false>(p, y);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k < n) {
                if constexpr (T == FATTN_TYPE_F32) ((float*)p)[k] = y[k];
                else if constexpr (T == FATTN_TYPE_F16) store_u16(p + 2 * k, f16_bits(y[k]));
                else store_u16(p + 2 * k, f32_to_bf16_bits(y[k]));
            }
        }
    }
}

// The lane's share of one unit of run-time type t (wave-uniform) at blk: y =
// elements 4l .. 4l+3, n of them in the row.  Every lane of the group calls it;
// `write` guards the stores.
__device__ __forceinline__ void rsr_store(int t, const float (&y)[4], int l, int n, bool write, uint8_t* blk) {
    switch (t) {
    case FATTN_TYPE_Q8_0: set_rows_block<FATTN_TYPE_Q8_0>(y, l, write, blk); break;
    case FATTN_TYPE_Q4_0: set_rows_block<FATTN_TYPE_Q4_0>(y, l, write, blk); break;
    case FATTN_TYPE_Q4_1: set_rows_block<FATTN_TYPE_Q4_1>(y, l, write, blk); break;
    case FATTN_TYPE_Q5_0: set_rows_block<FATTN_TYPE_Q5_0>(y, l, write, blk); break;
    case FATTN_TYPE_Q5_1: set_rows_block<FATTN_TYPE_Q5_1>(y, l, write, blk); break;
    case FATTN_TYPE_IQ4_NL: set_rows_block<FATTN_TYPE_IQ4_NL>(y, l, write, blk); break;
    case FATTN_TYPE_F16:
        if (write) rsr_store_elems<FATTN_TYPE_F16>(blk + 8 * l, y, n);
        break;
    case FATTN_TYPE_BF16:
        if (write) rsr_store_elems<FATTN_TYPE_BF16>(blk + 8 * l, y, n);
        break;
    default:  // F32
        if (write) rsr_store_elems<FATTN_TYPE_F32>(blk + 16 * l, y, n);
        break;
    }
}

template <bool VEC>
__device__ __forceinline__ void rsr_load4(const uint8_t* p, int n, float (&x)[4]) {
    if (VEC && n == 4) {
        const f32x4 v = *(const f32x4*)p;
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) x[k] = ((const float*)p)[k];
    }
}

__device__ __forceinline__ int64_t rsr_slot(const uint8_t* ip, int idx64) {
    return idx64 ? *(const int64_t*)ip : (int64_t)*(const int32_t*)ip;
}
// the dst row of a slot: 0 unless in range (64-bit compare before any address arithmetic)
__device__ __forceinline__ int64_t rsr_row_off(const SetRowsArgs& a, int64_t slot, bool& write) {
    write = (uint64_t)slot < (uint64_t)a.n_slots;
    return !write ? 0 : a.dst_small ? (int64_t)((uint64_t)(uint32_t)slot * (uint32_t)a.dnb1) : slot * a.dnb1;
}

// set_rows_kernel's unit body with the dst type a run-time value: workgroup bx of
// the part takes the 32 U units from 32 U bx on, pass j the units base + 32 j +
// (thread / 8); the U index and source loads precede the first conversion.
template <bool VEC, int U>
__device__ __forceinline__ void rsr_plain_units(const SetRowsArgs& a, int t, int bb, uint32_t bx) {
    const int l = threadIdx.x & 7;
    bool in_range[U];
    int64_t soff[U], ioff[U], doff[U];
    int n[U];  // elements of the lane (4; less in the tail of an F32 / F16 / BF16 row)
    {
        const uint32_t u0 = bx * (32u * U) + (threadIdx.x >> 3);
        const uint32_t i0 = u0 / a.upr;
        uint32_t bj = u0 - i0 * a.upr;
        soff[0] = (int64_t)i0 * a.snb1 + ((int64_t)bj * QK + 4 * l) * 4;
        ioff[0] = (int64_t)i0 * a.inb0;
        doff[0] = (int64_t)bj * bb;
#pragma unroll
        for (int j = 0; j < U; j++) {
            in_range[j] = u0 + 32u * j < a.units;
            const int64_t left = a.ne0 - ((int64_t)bj * QK + 4 * l);
            n[j] = (int)(left < 4 ? (left > 0 ? left : 0) : 4);
            if (j + 1 < U) {
                const uint32_t bn = bj + a.r32;
                const bool wrap = bn >= a.upr;
                bj = wrap ? bn - a.upr : bn;
                soff[j + 1] = soff[j] + (wrap ? a.ds_wrap : a.ds_next);
                ioff[j + 1] = ioff[j] + (wrap ? a.di_wrap : a.di_next);
                doff[j + 1] = doff[j] + (wrap ? a.dd_wrap : a.dd_next);
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
            int64_t slot[U];
            float x[U][4];
#pragma unroll
            for (int j = 0; j < U; j++) {
                slot[j] = -1;
#pragma unroll
                for (int k = 0; k < 4; k++) x[j][k] = 0.0f;
                if (in_range[j]) {
                    slot[j] = rsr_slot(iplane + ioff[j], a.idx64);
                    rsr_load4<VEC>(splane + soff[j], n[j], x[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < U; j++) {
                bool write;
                const int64_t roff = rsr_row_off(a, slot[j], write);
                rsr_store(t, x[j], l, n[j], write, dplane + roff + doff[j]);
            }
        }
    }
}

// The rotated K rows.  Wave 4 bx + (thread / 64) of the part holds rows rpw w ..
// rpw w + rpw - 1 of the [ne0, nr] plane; the heads i2 = y, y + gridDim.y, ... are
// walked one at a time with one set of angles per sequence.
template <bool NEOX, bool VEC>
__device__ __forceinline__ void rsr_rope_rows(const RopeSetRowsArgs& A, uint32_t bx) {
    const SetRowsArgs& a = A.k;
    const KShiftArgs& r = A.rope;
    const int lane = threadIdx.x & 63, l = lane & 7;
    const uint32_t g = (uint32_t)lane >> 3;
    const uint32_t rw = g / a.upr, b = g - rw * a.upr;  // row of the wave, block of the row
    const int64_t tok = ((int64_t)bx * 4 + (threadIdx.x >> 6)) * A.rpw + rw;
    const int e = (int)b * QK + 4 * l;  // the lane's first element (ne0 % 4 == 0: all four or none)
    const bool lane_ok = rw < A.rpw && tok < A.nr && e < a.ne0;
    if (__builtin_amdgcn_ballot_w64(lane_ok) == 0) return;  // (wave-uniform: a wave past the last row)
    // (n_dims % 8 == 0 and e % 4 == 0: a lane's four elements rotate together or not at all)
    const bool rot = e < r.n_dims;
    const int hd = r.n_dims >> 1;
    const bool low = e < hd;  // NEOX: this lane holds x0 (else x1) of its pairs
    // the two angles this lane computes, as in k_shift_kernel; pe: the first element of the NEOX partner
    int ia = 0, partner = lane, pe = e;
    if (rot) {
        if constexpr (NEOX) {
            ia = low ? e : e - hd + 2;
            partner = low ? lane + (r.n_dims >> 3) : lane - (r.n_dims >> 3);
            pe = low ? e + hd : e - hd;
        } else {
            ia = e >> 1;
        }
    }
    const int64_t trow = tok * a.snb1;
    const int64_t ioff = tok * a.inb0;
    const int64_t doff = (int64_t)b * A.kbb;
    for (int64_t i3 = blockIdx.z; i3 < a.ne3; i3 += gridDim.z) {
        const int64_t i13 = a.ne12 == 1 ? 0 : a.ne12 == a.ne3 ? i3 : i3 % a.ne12;
        int p = 0;
        if (lane_ok) p = *(const int32_t*)(A.pos + tok * A.pnb0 + (A.np == 1 ? 0 : i3 % A.np) * A.pnb1);
        float c[NEOX ? 4 : 2], s[NEOX ? 4 : 2];
        {
            float c0, s0, c1, s1;
            k_shift_angle(r, p, ia, c0, s0);
            k_shift_angle(r, p, ia + 1, c1, s1);
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
            int64_t slot = -1;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4];
            [[maybe_unused]] float xp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (lane_ok) {
                const int64_t i12 = a.ne11 == 1 ? 0 : a.ne11 == a.ne2 ? i2 : i2 % a.ne11;
                slot = rsr_slot(a.idx + ioff + i12 * a.inb1 + i13 * a.inb2, a.idx64);
                const uint8_t* srow = a.src + trow + i2 * a.snb2 + i3 * a.snb3;
                rsr_load4<VEC>(srow + (int64_t)e * 4, 4, x);
                if constexpr (NEOX) {
                    if (rot) rsr_load4<VEC>(srow + (int64_t)pe * 4, 4, xp);
                }
            }
            if constexpr (NEOX) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float y0, y1;
                    k_shift_rotate(low ? x[k] : xp[k], low ? xp[k] : x[k], c[k], s[k], r.m, y0, y1);
                    y[k] = rot ? (low ? y0 : y1) : x[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    float y0, y1;
                    k_shift_rotate(x[2 * k], x[2 * k + 1], c[k], s[k], r.m, y0, y1);
                    y[2 * k] = rot ? y0 : x[2 * k];
                    y[2 * k + 1] = rot ? y1 : x[2 * k + 1];
                }
            }
            bool write;
            const int64_t roff = rsr_row_off(a, slot, write);
            rsr_store(A.kt, y, l, 4, write, a.dst + i2 * a.dnb2 + i3 * a.dnb3 + roff + doff);
        }
    }
}

// MODE: 0 = no rope (K is a plain part like V), 1 = NORMAL, 2 = NEOX; VEC: the
// bases and nb[1..3] of both sources are 16-B multiples; U: units per lane group
// of a plain part -- kSetRowsUnroll only without a rope: next to the rotated rows
// the four-unit form LOST (its registers halve the waves that hide the powf /
// sincosf latency; DESIGN.md §23 has the numbers), and so did walking the heads
// of a rotated row four at a time.
// Grid: x = nk + V's workgroups (rotated K: ceil(waves / 4); a plain part:
// ceil(units / (32 U))), y strides over the heads, z over ne3.
template <int MODE, bool VEC, int U>
__global__ __launch_bounds__(256) void rope_set_rows_kernel(const RopeSetRowsArgs A) {
    static_assert(MODE == 0 || U == 1, "");
    if (blockIdx.x < A.nk) {
        if constexpr (MODE == 0) rsr_plain_units<VEC, U>(A.k, A.kt, A.kbb, blockIdx.x);
        else rsr_rope_rows<MODE == 2, VEC>(A, blockIdx.x);
    } else {
        rsr_plain_units<VEC, U>(A.v, A.vt, A.vbb, blockIdx.x - A.nk);
    }
}

}  // namespace fattn
