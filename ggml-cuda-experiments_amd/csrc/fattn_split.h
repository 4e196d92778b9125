// fattn_split.h -- split-KV ("flash decoding") attention kernel for gfx950.
//
// Replaces flash_attn_row / flash_attn_row_fast (src/flash_row_float.h:4-413)
// and, for small query counts, flash_attn_ext_f16 (src/flash-llama.h:5-438).
// Same math: s = scale*q.k + mask, online softmax (max, sum) per KV chunk,
// unnormalised P.V, merged with the log-sum-exp rule of fa_reduce
// (src/flash_row_float.h:429-471) -- but built MI355X-first:
//
//  * Work unit: one workgroup = 4, 8 or 16 waves = (KV chunk, 16 packed query rows).
//    The 16 MFMA rows pack (query row x q-head) pairs that share one KV head
//    (GQA broadcast ik2 = iq2 / (ne02/ne12), flash-llama.h:128-140), so a
//    32q/8kv decode packs 4 heads into one tile instead of re-reading K/V 4x.
//  * Each wave owns a contiguous slice of the chunk and streams it in steps of
//    32 positions.  The raw ggml rows (f16 / bf16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 blocks, exactly as in
//    HBM) plus the step's mask rows are copied HBM -> LDS with
//    global_load_lds_dwordx4 (fully coalesced 1 KiB per wave instruction; a
//    dword-granular variant serves arbitrary ggml row strides), NBUF steps in
//    flight per wave, retired with counted s_waitcnt vmcnt -- no workgroup
//    barrier inside the loop.
//  * Dequantisation happens on the LDS -> VGPR hop straight into MFMA operand
//    layout: K as the A operand of S^T = K.Q^T (v_mfma_f32_16x16x32_f16),
//    V (transposed by byte gathers for Q8_0/Q4_0, by ds_read_b64_tr_b16 for f16)
//    as the A operand of O^T = V^T.P^T.  The "swapped" products keep each
//    query column on one lane group, so P feeds PV with no lane movement and
//    the row max/sum need only two xor-shuffles (wave64: lanes l, l^16, l^32,
//    l^48).  Dequant is h(q*d) with one f16 rounding -- exactly the oracle's
//    fp16 rounding of the dequantised value (src/utils.h:10-11).  A bf16 cache
//    takes the f16 rows' moves bit for bit and v_mfma_f32_16x16x32_bf16: K and V
//    exact, Q and P as bf16 hi / lo operand pairs (bf16_split8, fattn_common.h).
//  * fp32 MFMA accumulators, fp32 softmax state (the reference keeps fp16).
//  * The waves' states merge through LDS (or, for one-row tiles, per wave);
//    with several chunks the partials (O, m, l) go to the caller's workspace
//    and merge in the last-arriving workgroup or wave (one-row tiles) or in a
//    second launch, fattn_chunk_merge_kernel (multi-row tiles).
#pragma once

#include "fattn_tile.h"

namespace fattn {


template <int KT, int VT, int D>
struct SplitCfg {
    static constexpr int KTT = KT;
    static constexpr int VTT = (VT == VT_F16T) ? FATTN_TYPE_F16 : VT;
    static constexpr int rowK = row_bytes<KT, D>();
    static constexpr int rowV = row_bytes<VTT, D>();
    static constexpr int kBytes = kStep * rowK;
    static constexpr int vBytes = kStep * rowV;
    static constexpr int mBytes = kRows * kStep * 2;  // up to 16 distinct mask rows
    static constexpr int stepBytes = (kBytes + vBytes + mBytes + 15) / 16 * 16;
    static constexpr int vscBytes = 0;
    static constexpr int kMergeStride = D + 4;  // floats; +16 B per row spreads rows over banks
    static constexpr int mergeBytes = kRows * kMergeStride * 4 + kRows * 2 * 4;
    // bytes of LDS one wave needs with nbuf steps in flight
    static constexpr int wave_bytes(int nbuf) {
        const int w = (nbuf * stepBytes + vscBytes + 15) / 16 * 16;
        return w > mergeBytes ? w : mergeBytes;
    }
    static constexpr int lds_bytes(int nbuf) { return kSplitWaves * wave_bytes(nbuf); }
};

// ---------------------------------------------------------------- HBM -> LDS
template <int KT, int VT, int D, int GRAN>
struct StepPlan {
    using C = SplitCfg<KT, VT, D>;
    static constexpr int PK = C::kBytes / GRAN;
    static constexpr int PV = C::vBytes / GRAN;
    // K and V come through different buffer descriptors: separate instructions
    static constexpr int NIK = (PK + kWave - 1) / kWave;
    static constexpr int NIV = (PV + kWave - 1) / kWave;
    static constexpr int NIKV = NIK + NIV;
    // mask granule: LDS-DMA writes lane*4 bytes for sub-dword sizes, so the
    // generic path moves dwords (2 positions) and needs even-padded mask rows
    static constexpr int MG = GRAN == 16 ? 16 : 4;
    static constexpr int MPR = kStep * 2 / MG;           // mask pieces per row
    // all 16 mask rows are always requested so every step issues the same,
    // compile-time instruction count; rows past n_q fall outside the mask
    // descriptor and cost no memory traffic
    static constexpr int PM = kRows * MPR;
    static constexpr int NIM = PM / kWave;
    static_assert(PM % kWave == 0, "");
};

// split kernel: tile geometry of the mask rows it stages
__device__ __forceinline__ void split_mask_src(const SplitArgs& a, StepSrc& rs, int ik2, int hs) {
    rs.mh0 = ik2 * a.rk2 + hs * a.R;
    rs.mhn = min(a.R, a.rk2 - hs * a.R);
    rs.mrows = a.m_hp ? kRows : a.QPT;
}

// split kernel: byte offset of the mask row staged as row r of a step's 16.
// One plane for all heads: query row mrow0 + r (the R packed heads share it).
// Head planes (a.m_hp): packed row r = (query row r / R, head r % R) in its own
// head's plane; rows the tile does not have point past the descriptor (zeros,
// no traffic -- the planner keeps m_span_h + a row's bytes inside 32 bits)
__device__ __forceinline__ uint32_t mask_row_off(const SplitArgs& a, const StepSrc& rs, int mrow0, int r) {
    if (!a.m_hp) return (uint32_t)(mrow0 + r) * (uint32_t)a.m_nb1;
    const int rq = div_R(a, r), hh = r - rq * a.R;
    const bool ok = rq < a.QPT && mrow0 + rq < a.NQ && hh < rs.mhn;
    return ok ? (uint32_t)(mrow0 + rq) * (uint32_t)a.m_nb1 + mask_head_off(a, rs.mh0 + hh) : a.m_span_h;
}

// split kernel: this lane's byte offset (row + piece) in each of a step's NIM
// mask instructions, position 0 -- computed once per wave, ahead of the loop
// (computed per step, the head-plane geometry stayed live in SGPRs across the
// loop and the dword-path bodies spilled)
template <int KT, int VT, int D, int GRAN>
__device__ __forceinline__ void mask_lane_offsets(const SplitArgs& a, const StepSrc& rs, int mrow0, int lane,
                                                  uint32_t (&ml)[StepPlan<KT, VT, D, GRAN>::NIM]) {
    using P = StepPlan<KT, VT, D, GRAN>;
#pragma unroll
    for (int i = 0; i < P::NIM; i++) {
        const int q = i * kWave + lane;
        ml[i] = mask_row_off(a, rs, mrow0, q / P::MPR) + (q % P::MPR) * P::MG;
    }
}

// One step = [K rows | V rows | mask rows] for positions [n0, n0+32), copied
// as raw bytes.  GRAN = 16: 16-B pieces (quantised rows contiguous, f16 rows
// 16-B aligned); GRAN = 4: dword pieces for any ggml row stride.
template <int KT, int VT, int D, int GRAN, bool HM>
__device__ __forceinline__ void issue_step(const SplitArgs& a, const StepSrc& rs, int n0,
                                           const uint32_t (&ml)[StepPlan<KT, VT, D, GRAN>::NIM], uint8_t* buf,
                                           int lane, bool kv_live = true) {
#ifdef FATTN_DIAG_NOMEM
    return;  // diagnostic build only: compute on whatever LDS holds (compute latency)
#endif
    using C = SplitCfg<KT, VT, D>;
    using P = StepPlan<KT, VT, D, GRAN>;
    const uint32_t kn1 = (uint32_t)a.k_nb1, vn1 = (uint32_t)a.v_nb1;
    // a step that is -inf for the whole tile: K and V through empty
    // descriptors (every load out of range: zeros, no traffic)
    i32x4 ksrd = rs.k, vsrd = rs.v;
    ksrd.z = __builtin_amdgcn_readfirstlane(kv_live ? rs.k.z : 0);
    vsrd.z = __builtin_amdgcn_readfirstlane(kv_live ? rs.v.z : 0);
#pragma unroll
    for (int i = 0; i < P::NIK; i++) {
        const int p = i * kWave + lane;
        const int byte = p * GRAN;
        uint32_t off;
        if constexpr (is_row16(KT)) {
            // f16 / bf16 rows: 16-B chunks XOR-swizzled by row (conflict-free ds_read_b128)
            constexpr int SW = swz_mask(C::rowK / 16);
            const int row = byte / C::rowK;
            const int chunk = ((byte % C::rowK) / 16) ^ (row & SW);
            off = (uint32_t)(n0 + row) * kn1 + chunk * 16 + (byte & 15);
        } else if constexpr (GRAN == 16) {
            off = (uint32_t)n0 * C::rowK + byte;
        } else {
            const int row = byte / C::rowK;
            off = (uint32_t)(n0 + row) * kn1 + (byte % C::rowK);
        }
        if (P::PK % kWave == 0 || p < P::PK) dma<GRAN, kDecodeNT>(ksrd, lds_addr(buf + i * kWave * GRAN), off);
    }
    // K, then the mask, then V: a step's S^T and softmax start once K and the
    // mask have landed, while V is still in flight
    if constexpr (HM) {
        uint8_t* mbuf = buf + C::kBytes + C::vBytes;
#pragma unroll
        for (int i = 0; i < P::NIM; i++) {
            const int mr = (i * kWave + lane) / P::MPR;
            const uint32_t moff = ml[i] + (uint32_t)n0 * 2;
            // 16-B path (one instruction, rows 0..15): lanes of rows past the
            // tile's query rows stay idle -- row 0's lanes always issue it, so
            // the per-step instruction count (vmcnt budget) is unchanged
            // (head planes: all 16 rows, one per packed (query row, head) pair)
            if (GRAN != 16 || mr < rs.mrows) dma<P::MG>(rs.m, lds_addr(mbuf + i * kWave * P::MG), moff);
        }
    }
    uint8_t* vbuf = buf + C::kBytes;
#pragma unroll
    for (int i = 0; i < P::NIV; i++) {
        const int p = i * kWave + lane;
        const int byte = p * GRAN;
        uint32_t off;
        if constexpr (VT == VT_F16T) {
            // V^T tile: D rows (one per head dim) of kStep f16; needs N % 32 == 0
            const int d = byte / (kStep * 2);
            off = (uint32_t)d * (uint32_t)a.v_nb0 + (uint32_t)n0 * 2 + (byte % (kStep * 2));
        } else if constexpr (is_row16(VT)) {
            constexpr int SW = swz_mask(C::rowV / 16);
            const int row = byte / C::rowV;
            const int chunk = ((byte % C::rowV) / 16) ^ (((row & 7) << 1) & SW);
            off = (uint32_t)(n0 + row) * vn1 + chunk * 16 + (byte & 15);
        } else if constexpr (GRAN == 16) {
            off = (uint32_t)n0 * C::rowV + byte;
        } else {
            const int row = byte / C::rowV;
            off = (uint32_t)(n0 + row) * vn1 + (byte % C::rowV);
        }
        if (P::PV % kWave == 0 || p < P::PV) dma<GRAN, kDecodeNT>(vsrd, lds_addr(vbuf + i * kWave * GRAN), off);
    }
}

// ---------------------------------------------------------------- block scales
// Quantised V: the A operand of P.V is the exact integer code plus the f16
// magic number 1024 (0x6400 | code), the block scale folded into P; v_code_off
// is what the epilogue takes off per unit of corr[b] = sum P d_b: 1024 plus the
// code's zero point (Q8_0: 128 by the sign flip, Q4_0: 8, Q5_0: 16) or, for the
// unsigned codes of Q4_1 / Q5_1, their centre v_code_centre (8 / 16).  The
// centre is not in the format: P d is rounded to f16, so the product sum carries
// sum eps_r P_r d_r (q_r - c) -- half the error with c at the middle of the code
// range than with c = 0 -- and c sum P d comes back exactly through the second
// accumulator (q d + m = (q - c) d + (m + c d))
template <int VT>
constexpr int v_code_centre() { return VT == FATTN_TYPE_Q4_1 ? 8 : VT == FATTN_TYPE_Q5_1 ? 16 : 0; }
template <int VT>
constexpr float v_code_off() {
    return VT == FATTN_TYPE_Q8_0 ? 1152.0f : VT == FATTN_TYPE_Q4_0 ? 1032.0f : VT == FATTN_TYPE_Q5_0 ? 1040.0f
           : 1024.0f + (float)v_code_centre<VT>();
}
// per-block f32 accumulators a wave carries beside O: corr[b], and for Q4_1 /
// Q5_1 behind them sum P (m_b + c d_b) (plain P, not the rounded P d: exact f16
// products summed in f32), which the epilogue adds to the block's 32 columns
// f16x8 registers of the Q^T operand a wave holds across its loop: one per
// k-step, two (the hi parts, then the lo parts) over a BF16 cache
template <int KT, int D>
constexpr int qop_len() { return (D + QK - 1) / QK * (KT == FATTN_TYPE_BF16 ? 2 : 1); }
template <int VT, int D>
constexpr int corr_len() { return (D + QK - 1) / QK * (has_min(VT) ? 2 : 1); }

// Column-packed V scales (one-row tiles, Q8_0 / Q4_0 V): of the 16 MFMA columns
// of a one-row tile only column 0 is live, so columns 0 .. D/QK - 1 all carry the
// tile's one query row (same Q operand, mask row, slope: the same S^T, softmax
// state and P on each), and column b's lanes fold the scales of V block b alone
// into P -- one P'_b per lane, one corr -- where the plain form builds P'_b of
// every block on every lane.  Block b's O^T tiles 2b, 2b+1 are then read from
// column b; that column holds there exactly what column 0 holds in the plain
// form (same operands, same MFMAs, same order): bit-identical results.
// EPI: the kernel's epilogue (split_epilogue); 1 and 2 are the one-row forms.
// (Q4_1 / Q5_0 / Q5_1 keep the plain form: their kernels sit at 2 waves per
// SIMD by the qh words and the second accumulator, not by the scales.)
template <int VT, int EPI>
constexpr bool col_packed() { return EPI != 0 && (VT == FATTN_TYPE_Q8_0 || VT == FATTN_TYPE_Q4_0); }
// f32 accumulators beside O in the kernel: one corr when column-packed
template <int VT, int D, bool CP>
constexpr int corr_regs() { return CP ? 1 : corr_len<VT, D>(); }

// The f16 scale of block b of a raw ggml row sits at byte BB*b.  row_scales()
// fetches the dwords holding all of a row's scales (2 x ds_read2_b32 for 4
// blocks); scale_bits() extracts block b's 16 bits.
template <int T, int D>
struct RowScales {
    uint32_t w[D / QK];
};
// whether block b's scale sits in the high half of its dword (rows that are a
// whole number of dwords); rows that are not (D = 96) read each scale as a u16
template <int T, int D>
__host__ __device__ constexpr bool scale_hi(int b) {
    return row_bytes<T, D>() % 4 == 0 && ((TypeInfo<T>::block_bytes * b) & 2) != 0;
}
template <int T, int D>
__device__ __forceinline__ RowScales<T, D> row_scales(const uint8_t* row) {
    constexpr int BB = TypeInfo<T>::block_bytes;
    RowScales<T, D> s;
#pragma unroll
    for (int b = 0; b < D / QK; b++) {
        if constexpr (row_bytes<T, D>() % 4 != 0) s.w[b] = *(const uint16_t*)(row + BB * b);
        else s.w[b] = *(const uint32_t*)(row + ((BB * b) & ~3));
    }
    return s;
}
template <int T, int D>
__device__ __forceinline__ uint32_t scale_bits(const RowScales<T, D>& s, int b) {
    return scale_hi<T, D>(b) ? (s.w[b] >> 16) : (s.w[b] & 0xffffu);
}
// block b's f16 scale in both halves, by one v_perm (b is unrolled)
template <int T, int D>
__device__ __forceinline__ uint32_t scale_bcast(const RowScales<T, D>& s, int b) {
    return perm_b32(s.w[b], s.w[b], scale_hi<T, D>(b) ? 0x03020302u : 0x01000100u);
}
// f16 pair {scale of row r0, scale of row r1} for block b
template <int T, int D>
__device__ __forceinline__ f16x2 scale_pair(const RowScales<T, D>& s0, const RowScales<T, D>& s1, int b) {
    constexpr int BB = TypeInfo<T>::block_bytes;
    // v_perm: low half from s0.w[b], high half from s1.w[b]
    return as_h2(((BB * b) & 2) ? perm_b32(s1.w[b], s0.w[b], 0x07060302u) : perm_b32(s1.w[b], s0.w[b], 0x05040100u));
}

// 8 bytes at a 2-byte-aligned LDS offset whose alignment is known only at run
// time (Q8_0 / Q4_0 rows of D = 96: 102 / 54 B, so odd rows start 2 B off a
// dword): three dword reads and two v_alignbyte with the shift in a VGPR
__device__ __forceinline__ u32x2 read8_any(const uint8_t* smem, uint32_t off) {
    const uint32_t base = off & ~3u, sh = off & 3u;
    const uint32_t w0 = *(const uint32_t*)(smem + base);
    const uint32_t w1 = *(const uint32_t*)(smem + base + 4);
    const uint32_t w2 = *(const uint32_t*)(smem + base + 8);
    u32x2 r;
    r.x = alignbyte(w1, w0, sh);
    r.y = alignbyte(w2, w1, sh);
    return r;
}

// ---------------------------------------------------------------- operands
// K operand (A of S^T = K.Q^T) for tile t (16 rows), block/k-step b:
// lane l -> row 16t + (l&15), elements d = 32b + 8(l>>4) + j.
template <int KT, int D>
__device__ __forceinline__ f16x8 k_operand(const uint8_t* kb, int row, int g, int b, uint32_t dbits) {
    if constexpr (is_row16(KT)) {  // (bf16 rows: the same bits, as an f16x8 register image)
        constexpr int CPR = D * 2 / 16;
        const int chunk = (4 * b + g) ^ (row & swz_mask(CPR));
        const f16x8 r = *(const f16x8*)(kb + row * (D * 2) + chunk * 16);
        if constexpr (D % QK != 0) {  // D = 80: the last k-step's dims past D read as zero
            if (b == D / QK && 4 * b + g >= CPR) return f16x8{};
        }
        return r;
    } else if constexpr (KT == FATTN_TYPE_Q8_0) {
        constexpr int RB = row_bytes<KT, D>();
        const uint32_t base = row * RB + kQ8Bytes * b;
        u32x2 raw;
        if constexpr (RB % 4 != 0) {
            raw = read8_any(kb, base + 2 + 8 * g);
        } else switch ((kQ8Bytes * b + 2) & 7) {  // b is a compile-time constant after unrolling
            case 0: raw = read8_at<0>(kb, base + 2 + 8 * g); break;
            case 2: raw = read8_at<2>(kb, base + 2 + 8 * g); break;
            case 4: raw = read8_at<4>(kb, base + 2 + 8 * g); break;
            default: raw = read8_at<6>(kb, base + 2 + 8 * g); break;
        }
        const f16x2 d = as_h2(dbits);
        f16x2 h0, h1, h2, h3;
        i8x4_to_h2x2(raw.x, h0, h1);
        i8x4_to_h2x2(raw.y, h2, h3);
        h0 *= d; h1 *= d; h2 *= d; h3 *= d;
        f16x8 r;
        r.s01 = h0; r.s23 = h1; r.s45 = h2; r.s67 = h3;
        return r;
    } else {  // Q4_0
        constexpr int RB = row_bytes<KT, D>();
        const uint32_t base = row * RB + kQ4Bytes * b;
        u32x2 raw;
        if constexpr (RB % 4 != 0) {
            raw = read8_any(kb, base + 2 + 8 * (g & 1));
        } else switch ((kQ4Bytes * b + 2) & 7) {
            case 0: raw = read8_at<0>(kb, base + 2 + 8 * (g & 1)); break;
            case 2: raw = read8_at<2>(kb, base + 2 + 8 * (g & 1)); break;
            case 4: raw = read8_at<4>(kb, base + 2 + 8 * (g & 1)); break;
            default: raw = read8_at<6>(kb, base + 2 + 8 * (g & 1)); break;
        }
        const uint32_t sh = (g >> 1) * 4;
        const f16x2 d = as_h2(dbits);
        f16x2 h0, h1, h2, h3;
        u4x4_to_h2x2((raw.x >> sh) & 0x0F0F0F0Fu, h0, h1);
        u4x4_to_h2x2((raw.y >> sh) & 0x0F0F0F0Fu, h2, h3);
        h0 *= d; h1 *= d; h2 *= d; h3 *= d;
        f16x8 r;
        r.s01 = h0; r.s23 = h1; r.s45 = h2; r.s67 = h3;
        return r;
    }
}

// ... for Q4_1 / Q5_0 / Q5_1 rows: the 5-bit (4-bit) code from the nibble and
// the qh bit as the exact f16 1024 + code, minus 1024 + zero point (exact);
// Q5_0: times d, one f16 rounding of the exact product; Q4_1 / Q5_1: one packed
// f16 fma q d + m, one rounding of the exact sum.  Rows are whole dwords, so
// within a row d (and m) share the dword at BB b (Q5_0: BB b & ~3, d in either
// half), qh and qs sit at a compile-time offset modulo 4 (b is unrolled)
template <int KT, int D>
__device__ __forceinline__ f16x8 k_operand_ext(const uint8_t* kb, int row, int g, int b) {
    constexpr int BB = TypeInfo<KT>::block_bytes;
    constexpr int RB = row_bytes<KT, D>();
    static_assert(RB % 4 == 0, "rows of whole dwords");
    const uint32_t base = row * RB;
    const uint32_t dm = *(const uint32_t*)(kb + base + ((BB * b) & ~3));
    const uint32_t qo = BB * b + qs_off(KT);
    const u32x2 raw = (qo & 2) ? read8_mod4<2>(kb, base + qo + 8 * (g & 1)) : read8_mod4<0>(kb, base + qo + 8 * (g & 1));
    const uint32_t sh = (g >> 1) * 4;
    uint32_t cx = (raw.x >> sh) & 0x0F0F0F0Fu, cy = (raw.y >> sh) & 0x0F0F0F0Fu;
    if constexpr (has_qh(KT)) {
        const uint32_t ho = BB * b + qh_off(KT);
        const uint32_t qh = (ho & 2) ? read4_mod4<2>(kb, base + ho) : read4_mod4<0>(kb, base + ho);
        const uint32_t q8 = (qh >> (8 * g)) & 0xFFu;  // the fifth bits of elements 8g .. 8g + 7
        cx |= bits4_to_bit4(q8 & 0xFu);
        cy |= bits4_to_bit4(q8 >> 4);
    }
    constexpr f16 zo = (f16)(-1024.0f - (float)code_zero(KT));
    const f16x2 off = {zo, zo};
    f16x2 h0 = as_h2(perm_b32(0x64646464u, cx, 0x04010400u)) + off, h1 = as_h2(perm_b32(0x64646464u, cx, 0x04030402u)) + off;
    f16x2 h2 = as_h2(perm_b32(0x64646464u, cy, 0x04010400u)) + off, h3 = as_h2(perm_b32(0x64646464u, cy, 0x04030402u)) + off;
    if constexpr (has_min(KT)) {
        const f16x2 d = as_h2(perm_b32(dm, dm, 0x01000100u)), m = as_h2(perm_b32(dm, dm, 0x03020302u));
        h0 = __builtin_elementwise_fma(h0, d, m);
        h1 = __builtin_elementwise_fma(h1, d, m);
        h2 = __builtin_elementwise_fma(h2, d, m);
        h3 = __builtin_elementwise_fma(h3, d, m);
    } else {
        const f16x2 d = as_h2(perm_b32(dm, dm, ((BB * b) & 2) ? 0x03020302u : 0x01000100u));
        h0 *= d; h1 *= d; h2 *= d; h3 *= d;
    }
    f16x8 r;
    r.s01 = h0; r.s23 = h1; r.s45 = h2; r.s67 = h3;
    return r;
}

// V operand (A of O^T = V^T.P^T) for column group c (16 columns):
// lane l -> column dc = 16c + (l&15); element j = 4t + r <-> row 16t + 4g + r.
// For quantised V the per-(row, block) scales come from the compact array
// vsc[b][row] (f16) built once per step.
__device__ __forceinline__ uint32_t lds_u8_pair(const uint8_t* p0, const uint8_t* p1) {
    return (uint32_t)(*p0) | ((uint32_t)(*p1) << 16);
}

template <int VT, int D>
__device__ __forceinline__ f16x8 v_operand_f16(const uint8_t* vb, int c, int g, int i) {
    if constexpr (VT == VT_F16T) {
        const uint8_t* p = vb + (16 * c + i) * (kStep * 2) + 8 * g;
        const u32x2 lo = *(const u32x2*)p;
        const u32x2 hi = *(const u32x2*)(p + 32);
        u32x4 r = {lo.x, lo.y, hi.x, hi.y};
        return __builtin_bit_cast(f16x8, r);
    } else {
        constexpr int RB = D * 2;
        constexpr int CPR = RB / 16;
        const int q = i >> 2, p = i & 3;
        const int chunk = 2 * c + (p >> 1);
        const int r0 = 4 * g + q, r1 = 16 + 4 * g + q;
        const int a0 = r0 * RB + ((chunk ^ (((r0 & 7) << 1) & swz_mask(CPR))) * 16) + (p & 1) * 8;
        const int a1 = r1 * RB + ((chunk ^ (((r1 & 7) << 1) & swz_mask(CPR))) * 16) + (p & 1) * 8;
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + a0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + a1));
        u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        u32x4 r = {l2.x, l2.y, h2.x, h2.y};
        return __builtin_bit_cast(f16x8, r);
    }
}

// ---------------------------------------------------------------- kernel


template <int D, int CB = 2, typename A>
__device__ __forceinline__ void combine_tile(const A& a, int64_t tile, int qt, int hs, int ik2, int iq3,
                                             int rv, int row_base, uint8_t* smem);

// One-row tiles (decode with n_q * H / Hkv == 1 per tile), up to 32 parts per
// tile: each WAVE is a part.  It stores its (O, m, l) write-through (sc1),
// drains, and counts itself on the tile's arrival word; the wave that counts
// last merges all parts alone -- lane i owns dims 2i, 2i+1, every part's
// values come in one round trip, weights by wave reductions -- and writes dst.
// No LDS merge and no workgroup barrier: waves leave as they finish.  Same
// fa_reduce math as combine_tile (src/flash_row_float.h:415-472), fixed order.
constexpr int kWaveMergeParts = 64;  // parts per tile (one (m, l) pair per lane)
constexpr int kWaveMergeBatch = 32;  // parts loaded per round trip
template <int D, bool VQ8, int NW = kSplitWaves, bool CP = false, typename A>
__device__ __forceinline__ void wave_merge_epilogue(const A& a, const f32x4 (&o)[D / 16], float m_run,
                                                    float l_tot, int chunk, int wave, int lane, int qt, int hs,
                                                    int ik2, int iq3, int y) {
    static_assert(D == 128, "lane i <-> dims 2i, 2i+1");
    constexpr int NB = D / QK;
    constexpr int NC = D / 16;
    constexpr float kNegInf = -__builtin_inff();
    const int g = lane >> 4, m = lane & 15;
    const int NP = a.n_chunks * NW;
    const int64_t tile = (int64_t)iq3 * gridDim.y + y;
    const int part = chunk * NW + wave;
    float* po = a.ws_o + (tile * NP + part) * D;  // row 0 of the part: [NP][D] per tile
    auto bits = [](float x) { return __builtin_bit_cast(uint32_t, x); };
    if constexpr (CP) {  // block b's dims sit on column b (col_packed): one masked write per block
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (m != b) continue;
            if constexpr (VQ8) {
                const f32x4 e = o[2 * b], od = o[2 * b + 1];
                st_sc1(po + 32 * b + 8 * g, u32x4{bits(e.x), bits(od.x), bits(e.y), bits(od.y)});
                st_sc1(po + 32 * b + 8 * g + 4, u32x4{bits(e.z), bits(od.z), bits(e.w), bits(od.w)});
            } else {
#pragma unroll
                for (int c = 2 * b; c < 2 * b + 2; c++)
                    st_sc1(po + 16 * c + 4 * g, u32x4{bits(o[c].x), bits(o[c].y), bits(o[c].z), bits(o[c].w)});
            }
        }
        if (lane == 0) st_sc1_x2(a.ws_ml + 2 * (tile * NP + part), u32x2{bits(m_run), bits(l_tot)});
    } else if (m == 0) {  // column 0 = the tile's row; its dims sit on lanes 0, 16, 32, 48
        if constexpr (VQ8) {
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const f32x4 e = o[2 * b], od = o[2 * b + 1];
                st_sc1(po + 32 * b + 8 * g, u32x4{bits(e.x), bits(od.x), bits(e.y), bits(od.y)});
                st_sc1(po + 32 * b + 8 * g + 4, u32x4{bits(e.z), bits(od.z), bits(e.w), bits(od.w)});
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; c++)
                st_sc1(po + 16 * c + 4 * g, u32x4{bits(o[c].x), bits(o[c].y), bits(o[c].z), bits(o[c].w)});
        }
        if (g == 0) st_sc1_x2(a.ws_ml + 2 * (tile * NP + part), u32x2{bits(m_run), bits(l_tot)});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FATTN_SSTAMP(12);
    int last = 0;
    if (lane == 0) last = arrive_last(a, tile, NP);
    last = __builtin_amdgcn_readfirstlane(last);
    FATTN_SSTAMP(14);
    if (!last) return;
    // ---- merge: lane half h = lane / 32 takes the parts of parity h, dims
    // 4 (lane % 32) .. +3, one 16-B load per part (parts past NP fall outside
    // the descriptor: zeros, no traffic, weight 0); the halves meet by one
    // permlane32 swap.  Every load of a batch is issued before one wait.
    const int h = lane >> 5, d4 = 4 * (lane & 31);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the loads below the count)
    const __amdgpu_buffer_rsrc_t osrd = make_rsrc(a.ws_o + tile * NP * D, (uint32_t)(NP * D * 4));
    const __amdgpu_buffer_rsrc_t msrd = make_rsrc(a.ws_ml + 2 * tile * NP, (uint32_t)(NP * 8));
    constexpr int kIt = kWaveMergeBatch / 2;  // part pairs per round trip
    u32x4 v[kIt];
    auto issue = [&](int p0) {
#pragma unroll
        for (int i = 0; i < kIt; i++) v[i] = ld_sc1_buf(osrd, (uint32_t)(((p0 + 2 * i + h) * D + d4) * 4));
    };
    issue(0);
    const uint32_t mlm = ld_sc1_buf_b32(msrd, (uint32_t)(lane * 8));      // lane p: m of part p
    const uint32_t mll = ld_sc1_buf_b32(msrd, (uint32_t)(lane * 8 + 4));  //          l of part p
    FATTN_SSTAMP(15);
    const float mp = lane < NP ? __builtin_bit_cast(float, mlm) : kNegInf;
    const float M = seg_reduce<true>(mp, 64);
    const float w = (mp == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(mp - M);
    const float L = seg_reduce<false>(lane < NP ? w * __builtin_bit_cast(float, mll) : 0.0f, 64);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p0 = 0; p0 < NP; p0 += kWaveMergeBatch) {  // wave-uniform
        if (p0 > 0) issue(p0);
#pragma unroll
        for (int i = 0; i < kIt; i++) {
            const int wi = __builtin_bit_cast(int, w);
            const float we = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, p0 + 2 * i));
            const float wo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, p0 + 2 * i + 1));
            const float wp = h ? wo : we;
            acc += wp * __builtin_bit_cast(f32x4, v[i]);
        }
    }
    acc.x = xor32_pair(acc.x, false);
    acc.y = xor32_pair(acc.y, false);
    acc.z = xor32_pair(acc.z, false);
    acc.w = xor32_pair(acc.w, false);
    if (h) return;  // lanes 0..31 store the row, 16 B each
    const int rq = div_R(a, 0);
    const int riq1 = qt * a.QPT + rq;
    const int riq2 = ik2 * a.rk2 + hs * a.R;
    const int64_t row = ((int64_t)iq3 * a.NQ + riq1) * a.H + riq2;
    float* out = a.dst + row * D + d4;
    if (const float* sinks = a.sinks) {  // (wave-uniform) the head's sink joins the merged row's denominator
        bool dead;
        const float inv = sink_inv(M, L, sinks[riq2], dead);
        *(f32x4*)out = sink_row(acc, inv, dead);
    } else {
        const float inv = L == 0.0f ? __builtin_nanf("") : 1.0f / L;  // L == 0 (row fully masked) -> NaN like the reference
        *(f32x4*)out = acc * inv;
    }
    if (float* const lse = lse_of(a)) {  // (wave-uniform) the merged row's log-sum-exp, one lane
        if (lane == 0) lse[row] = row_lse(M, L, a.sinks ? a.sinks[riq2] : kNegInf, row_dead(M, L));
    }
    FATTN_SSTAMP(13);
}

// One-row tiles, NW waves per workgroup: every wave writes its row-0 state
// (O, m, l) into its own LDS region (its steps have all landed), one barrier,
// then wave 0 merges the NW states (lane (h, dl): states p = h mod PPR, dims
// 4dl..4dl+3, one ds_read_b128 each).  With one chunk it writes dst; with
// several it publishes the workgroup's row write-through, drains, counts the
// workgroup on the tile's arrival word, and the last workgroup's wave 0 merges
// the chunks (merge_row_parts).  The cross-workgroup hand-off carries one row
// per workgroup instead of one per wave.
template <int D, bool VQ8, int NW, bool CP = false, typename A>
__device__ __forceinline__ void wg_row_merge(const A& a, const f32x4 (&o)[D / 16], float m_run, float l_tot,
                                             int chunk, int wave, int lane, int qt, int hs, int ik2, int iq3,
                                             int y, uint8_t* smem, int region) {
    constexpr int NB = D / QK;
    constexpr int NC = D / 16;
    constexpr float kNegInf = -__builtin_inff();
    constexpr int LPP = D / 4;
    constexpr int PPR = 64 % LPP == 0 ? 64 / LPP : 1;  // (D = 80 / 96: one part per lane row)
    const int g = lane >> 4, m = lane & 15;
    float* so = (float*)(smem + wave * region);  // [D] O row, then (m, l)
    if constexpr (CP) {  // block b's dims sit on column b (col_packed): one masked write per block
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (m != b) continue;
            if constexpr (VQ8) {
                const f32x4 e = o[2 * b], od = o[2 * b + 1];
                *(f32x4*)(so + 32 * b + 8 * g) = f32x4{e.x, od.x, e.y, od.y};
                *(f32x4*)(so + 32 * b + 8 * g + 4) = f32x4{e.z, od.z, e.w, od.w};
            } else {
                *(f32x4*)(so + 32 * b + 4 * g) = o[2 * b];
                *(f32x4*)(so + 32 * b + 16 + 4 * g) = o[2 * b + 1];
            }
        }
        if (lane == 0) *(f32x2*)(so + D) = f32x2{m_run, l_tot};
    } else if (m == 0) {  // column 0 = the tile's row; its dims sit on lanes 0, 16, 32, 48
        if constexpr (VQ8) {
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const f32x4 e = o[2 * b], od = o[2 * b + 1];
                *(f32x4*)(so + 32 * b + 8 * g) = f32x4{e.x, od.x, e.y, od.y};
                *(f32x4*)(so + 32 * b + 8 * g + 4) = f32x4{e.z, od.z, e.w, od.w};
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; c++) *(f32x4*)(so + 16 * c + 4 * g) = o[c];
        }
        if (g == 0) *(f32x2*)(so + D) = f32x2{m_run, l_tot};
    }
    __syncthreads();
    if (wave != 0) return;
    FATTN_SSTAMP(11);
    // ---- wave 0: merge the NW states
    const int h = lane / LPP, d4 = 4 * (lane % LPP);
    const f32x2 ml = lane < NW ? *(const f32x2*)((const float*)(smem + lane * region) + D) : f32x2{kNegInf, 0.0f};
    const float M = seg_reduce<true>(ml.x, 64);
    const float w = (ml.x == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(ml.x - M);
    const float L = seg_reduce<false>(w * ml.y, 64);
    const int wi = __builtin_bit_cast(int, w);
    constexpr int NI = (NW + PPR - 1) / PPR;
    f32x4 part[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = PPR * i + h;
        part[i] = p < NW ? *(const f32x4*)((const float*)(smem + p * region) + d4) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < NI; i++) {
        float wp = 0.0f;
#pragma unroll
        for (int j = 0; j < PPR; j++) {
            const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, (PPR * i + j) & 63));
            wp = (h == j && PPR * i + j < NW) ? wj : wp;
        }
        acc += wp * part[i];
    }
    if constexpr (PPR == 4) {
        acc.x = xor16_pair(acc.x, false);
        acc.y = xor16_pair(acc.y, false);
        acc.z = xor16_pair(acc.z, false);
        acc.w = xor16_pair(acc.w, false);
    }
    if constexpr (PPR >= 2) {
        acc.x = xor32_pair(acc.x, false);
        acc.y = xor32_pair(acc.y, false);
        acc.z = xor32_pair(acc.z, false);
        acc.w = xor32_pair(acc.w, false);
    }
    const int riq1 = qt * a.QPT;
    const int riq2 = ik2 * a.rk2 + hs * a.R;
    const int64_t row = ((int64_t)iq3 * a.NQ + riq1) * a.H + riq2;
    float* out = a.dst + row * D;
    if (a.n_chunks == 1) {
        if (h == 0) {
            if (const float* sinks = a.sinks) {  // (wave-uniform)
                bool dead;
                const float inv = sink_inv(M, L, sinks[riq2], dead);
                *(f32x4*)(out + d4) = sink_row(acc, inv, dead);
            } else {
                const float inv = L == 0.0f ? __builtin_nanf("") : 1.0f / L;
                *(f32x4*)(out + d4) = acc * inv;
            }
        }
        if (float* const lse = lse_of(a)) {  // (wave-uniform)
            if (lane == 0) lse[row] = row_lse(M, L, a.sinks ? a.sinks[riq2] : kNegInf, row_dead(M, L));
        }
        return;
    }
#ifdef FATTN_DIAG_NOPUBLISH
    if (acc.x == 12345.0f) a.dst[0] = L;  // diagnostic build only: stop after the workgroup merge
    return;
#endif
    const int64_t tile = (int64_t)iq3 * gridDim.y + y;
    float* po = a.ws_o + (tile * a.n_chunks + chunk) * D;
    auto bits = [](float x) { return __builtin_bit_cast(uint32_t, x); };
    if (h == 0) st_sc1(po + d4, u32x4{bits(acc.x), bits(acc.y), bits(acc.z), bits(acc.w)});
    if (lane == 0) st_sc1_x2(a.ws_ml + 2 * (tile * a.n_chunks + chunk), u32x2{bits(M), bits(L)});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FATTN_SSTAMP(12);
#ifdef FATTN_DIAG_NOATOMIC
    return;  // diagnostic build only: stop after the published row drained
#endif
    int last = 0;
    if (lane == 0) last = arrive_last(a, tile, a.n_chunks);
    last = __builtin_amdgcn_readfirstlane(last);
    FATTN_SSTAMP(14);
    if (!last) return;
    // as few load slots per lane as the chunk count needs (a slot past it is
    // still an issued instruction; config 3: 8 chunks = 4 slots)
    const float* po_all = a.ws_o + tile * a.n_chunks * D;
    const float* pml_all = a.ws_ml + 2 * tile * a.n_chunks;
    const int need = (a.n_chunks + merge_ppr<D>() - 1) / merge_ppr<D>();
    auto sink = [&]() -> const float* {
        const float* sinks = a.sinks;
        return sinks ? sinks + riq2 : nullptr;
    };
    float* lse_row = lse_at(a, row);  // (wave-uniform)
    if (need <= 4) merge_row_parts<D, 4>(po_all, pml_all, a.n_chunks, out, lane, D, 2, sink, lse_row);
    else if (need <= 8) merge_row_parts<D, 8>(po_all, pml_all, a.n_chunks, out, lane, D, 2, sink, lse_row);
    else merge_row_parts<D>(po_all, pml_all, a.n_chunks, out, lane, D, 2, sink, lse_row);
    FATTN_SSTAMP(13);
}

// Tail of a split-KV workgroup: the waves' (O, m, l) states merge.  EPI (the
// plan's a.wave_merge, a template parameter so that each kernel carries only
// its own epilogue's registers -- combine_tile's in-flight loads made the
// whole kernel spill): 0 = through LDS (wave w's image at smem + w * region)
// and then across the tile's chunks via the last-arriving workgroup
// (combine_tile); 1 = one-row tiles, every wave publishes and the
// last-arriving wave merges (wave_merge_epilogue); 2 = one-row tiles, LDS
// merge and one published row per workgroup (wg_row_merge).  `active`: this
// wave holds a state (waves >= NW must be inactive).  `sync_first`: the images
// alias step buffers, so wait for every wave before writing them.
template <int KT, int VT, int D, int NW, int EPI, typename A>
__device__ __forceinline__ void split_epilogue(const A& a, f32x4 (&o)[D / 16], float m_run, float l_run,
                                               float (&corr)[corr_regs<VT, D, col_packed<VT, EPI>()>()], int wave, int lane,
                                               int qt, int hs, int ik2, int iq3, int y, int chunk, uint8_t* smem, int region,
                                               bool active, bool sync_first) {
    using C = SplitCfg<KT, VT, D>;
    constexpr int NB = D / QK;
    constexpr int NC = D / 16;
    constexpr float kNegInf = -__builtin_inff();
    constexpr bool kVQ8 = C::VTT == FATTN_TYPE_Q8_0;
    constexpr bool kVQ = !is_row16(C::VTT);
    constexpr float kVOff = v_code_off<C::VTT>();
    constexpr bool CP = col_packed<C::VTT, EPI>();
    const int g = lane >> 4;
    const int m = lane & 15;
    // split_step keeps the reference max in natural units; the merges work in log2
    m_run = m_run == kNegInf ? kNegInf : m_run * 1.4426950408889634f;
    const float l_tot = grp4_sum(l_run);
    if constexpr (CP) {
        // column b's one corr is block b's; the tiles of block b are read from column b
        // alone (wave_merge_epilogue, wg_row_merge), every other tile of that column is
        // never read
        const float cb = kVOff * grp4_sum(corr[0]);
#pragma unroll
        for (int c = 0; c < NC; c++) o[c] -= cb;
    } else if constexpr (kVQ) {
        // O^T tiles of block b (columns 32b..32b+31) carry kVOff * sum(P'_b) too
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const float cb = kVOff * grp4_sum(corr[b]);
            o[2 * b] -= cb;
            o[2 * b + 1] -= cb;
            if constexpr (has_min(C::VTT)) {  // + sum P (m_b + c d_b), the affine term of the block's 32 columns
                const float mb = grp4_sum(corr[NB + b]);
                o[2 * b] += mb;
                o[2 * b + 1] += mb;
            }
        }
    }
    if constexpr (EPI == 1) {
        static_assert(D == 128, "per-wave merge: lane i <-> dims 2i, 2i+1");
        wave_merge_epilogue<D, kVQ8, NW, CP>(a, o, m_run, l_tot, chunk, wave, lane, qt, hs, ik2, iq3, y);
        return;
    } else if constexpr (EPI == 2) {
        wg_row_merge<D, kVQ8, NW, CP>(a, o, m_run, l_tot, chunk, wave, lane, qt, hs, ik2, iq3, y, smem, region);
        return;
    }
    constexpr int MS = C::kMergeStride;
    // the merge images alias step buffers other waves may still be reading
    if (sync_first) __syncthreads();
    float* mo = (float*)(smem + wave * region);    // [16][MS]
    float* mml = (float*)(smem + wave * region + kRows * MS * 4);  // [16][2]
    // valid rows of this tile form a prefix [0, rv); only those are merged
    const int rv = tile_rows(a, qt, hs);
    if (m >= rv || !active) {
        // nothing of this column is needed
    } else if constexpr (kVQ8) {
        // tile E_b holds columns 32b + 2(4g+reg), O_b the odd neighbours
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const f32x4 e = o[2 * b], od = o[2 * b + 1];
            *(f32x4*)(mo + m * MS + 32 * b + 8 * g) = f32x4{e.x, od.x, e.y, od.y};
            *(f32x4*)(mo + m * MS + 32 * b + 8 * g + 4) = f32x4{e.z, od.z, e.w, od.w};
        }
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) *(f32x4*)(mo + m * MS + 16 * c + 4 * g) = o[c];
    }
    if (g == 0 && m < rv && active) {
        mml[2 * m] = m_run;
        mml[2 * m + 1] = l_tot;
    }
    __syncthreads();
    FATTN_SSTAMP(11);

    constexpr int EPT = epi_ept<D>();  // outputs per thread: 16 rows x D over 256 threads
    const int tm = threadIdx.x / 16;
    const int tj = threadIdx.x % 16;
    const int d0 = tj * EPT;
    const bool dok = d0 < D;  // (D = 80 / 96: the last threads of a row hold no dims)
    float M = kNegInf;
    float mw[NW], lw[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const float* ml = (const float*)(smem + w * region + kRows * MS * 4);
        mw[w] = tm < rv ? ml[2 * tm] : kNegInf;
        lw[w] = tm < rv ? ml[2 * tm + 1] : 0.0f;
        M = fmaxf(M, mw[w]);
    }
    // Attention sinks, single chunk (the row is normalised below): the sink is one
    // more part of the merge -- max s log2e, sum 1, no O row -- so it joins M and
    // L here and 1 / L stays the factor: sink_inv()'s value in the merge's own
    // overflow-safe form, with no second normalising statement in a body that
    // sits at its SGPR limit.  Mk: the max over the keys alone; a fully masked
    // row (Mk = -inf) keeps L = 0, so the select on L == 0 below still finds it.
    // Without sinks ms = -inf leaves M and L as they were, bit for bit
    const float Mk = M;
    float ms = kNegInf, sraw = kNegInf;  // (sraw: the raw sink, the log-sum-exp of a row without a live key)
    if (a.n_chunks == 1 && a.sinks != nullptr && tm < rv) {  // (wave-uniform but for the row bound)
        sraw = a.sinks[ik2 * a.rk2 + hs * a.R + (tm - div_R(a, tm) * a.R)];
        ms = sraw * 1.4426950408889634f;
    }
    M = fmaxf(M, ms);
    float L = (ms == kNegInf || Mk == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(ms - M);
    float acc[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) acc[e] = 0.0f;
    if (tm < rv) {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const float wt = (mw[w] == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(mw[w] - M);
            L += wt * lw[w];
            const float* ow = (const float*)(smem + w * region) + tm * MS + (dok ? d0 : 0);
#pragma unroll
            for (int e = 0; e < EPT; e++) acc[e] += wt * ow[e];
        }
    }
    auto head_of = [&](int r) { return ik2 * a.rk2 + hs * a.R + (r - div_R(a, r) * a.R); };  // q head of packed row r (in-kernel merge)
    auto dst_idx = [&](int r) -> int64_t {  // packed row r's row of dst (and entry of lse)
        const int rq = div_R(a, r);
        const int riq1 = qt * a.QPT + rq;
        const int riq2 = ik2 * a.rk2 + hs * a.R + (r - rq * a.R);
        return ((int64_t)iq3 * a.NQ + riq1) * a.H + riq2;
    };
    auto dst_row = [&](int r) -> float* { return a.dst + dst_idx(r) * D; };
    if (a.n_chunks == 1) {
        if (tm < rv && dok) {
            const int64_t idx = dst_idx(tm);
            float* out = a.dst + idx * D + d0;
            // L == 0: the row has no live key -- NaN like the reference, zeros with
            // sinks; by selection either way
            const float inv = 1.0f / L;
            const bool none = L == 0.0f;
            const float fill = a.sinks != nullptr ? 0.0f : __builtin_nanf("");  // (wave-uniform)
#pragma unroll
            for (int e = 0; e < EPT; e += 4) {
                f32x4 v;
                v.x = none ? fill : acc[e] * inv;
                v.y = none ? fill : acc[e + 1] * inv;
                v.z = none ? fill : acc[e + 2] * inv;
                v.w = none ? fill : acc[e + 3] * inv;
                *(f32x4*)(out + e) = v;
            }
            // the row's log-sum-exp, one thread per row: the sink, where live, is in M and
            // L already (above); nothing but the pointer is fetched for it
            if (float* const lse = lse_of(a)) {  // (wave-uniform)
                if (tj == 0) lse[idx] = !(L > 0.0f) ? sraw : row_lse(M, L, kNegInf, false);
            }
        }
        FATTN_SSTAMP(12);
        return;
    }

#ifdef FATTN_DIAG_NOPUBLISH
    // diagnostic build only: stop after the 4-wave merge
    if (acc[0] == 12345.0f) a.dst[0] = L;
    return;
#endif
    // ---- several chunks: the workgroup that arrives last for the tile merges
    // all partials (no second launch).  Hand-off (MI355X_MICROARCH.md,
    // inter-workgroup visibility, first row of the sc1 table): partial bytes
    // stored sc1 (write-through), each storing wave drains vmcnt, barrier, ONE
    // agent-scope atomic add per workgroup on the tile's own 256-B line; the
    // last adder reads the others' partials with sc1 loads -- all of them in
    // one round trip -- while its own stays in LDS.
    const int64_t tile = (int64_t)iq3 * gridDim.y + y;
    if (a.merge_launch == 1 && a.part_f16) {
        if constexpr (EPT % 4 == 0) {
            if (tm < rv) {
                const int64_t slot = (tile * a.n_chunks + chunk) * kRows + tm;
                if (dok) store_part_f16<EPT>((uint16_t*)a.ws_o + slot * D + d0, acc, L);
                if (tj == 0) *(f32x2*)(a.ws_ml + 2 * slot) = f32x2{M, L};
            }
        }
        return;
    }
    if (tm < rv) {
        const int64_t slot = (tile * a.n_chunks + chunk) * kRows + tm;
        auto bits = [](float x) { return __builtin_bit_cast(uint32_t, x); };
        if (dok) {
#pragma unroll
            for (int e = 0; e < EPT; e += 4)
                st_sc1(a.ws_o + slot * D + d0 + e,
                       u32x4{bits(acc[e]), bits(acc[e + 1]), bits(acc[e + 2]), bits(acc[e + 3])});
        }
        if (tj == 0) st_sc1_x2(a.ws_ml + 2 * slot, u32x2{bits(M), bits(L)});
    }
    // second-launch merge (fattn_chunk_merge_kernel): the kernel boundary orders
    // these stores before its loads; no drain, no counter
    if (a.merge_launch == 1) return;
    if (a.merge_launch == 2) {
        // in-kernel: wait for the tile's chunks, then every workgroup merges a
        // share of the tile's rows, one wave per row (row r: wave r mod NW of
        // chunk (r / NW) mod n_chunks), as the merge launch would
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains
        __syncthreads();
        int* flag = (int*)smem;  // (every wave is done reading the merge images)
        if (threadIdx.x == 0) *flag = tile_arrive_wait(a, tile, a.n_chunks);
        __syncthreads();
        const bool ok = *flag != 0;
        FATTN_SSTAMP(12);
        for (int r = chunk * NW + wave; r < rv; r += NW * a.n_chunks) {  // wave-uniform
            const int64_t s0 = tile * a.n_chunks * kRows + r;  // chunk 0's row r
            float* out = dst_row(r);
            if (ok) {
                merge_row_parts<D, 8>(a.ws_o + s0 * D, a.ws_ml + 2 * s0, a.n_chunks, out, lane, kRows * D, 2 * kRows,
                                      [&]() -> const float* {
                                          const float* sinks = a.sinks;
                                          return sinks ? sinks + head_of(r) : nullptr;
                                      },
                                      lse_at(a, dst_idx(r)));
            } else if (lane < D / 4) {
                *(f32x4*)(out + 4 * lane) = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""),
                                                  __builtin_nanf("")};
            }
        }
        FATTN_SSTAMP(13);
        return;
    }
    // every storing wave drains: the merging workgroup reads its own partial back too
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef FATTN_DIAG_NOATOMIC
    return;  // diagnostic build only: stop after the published stores drained
#endif
    __syncthreads();  // every storing wave has drained; every wave is done reading the merge image
    int* last_flag = (int*)smem;
    if (threadIdx.x == 0) *last_flag = arrive_last(a, tile, a.n_chunks);
    __syncthreads();
    FATTN_SSTAMP(12);
    if (!*last_flag) return;
    combine_tile<D, (D == 128 && !is_row16(KT)) ? 8 : 2>(a, tile, qt, hs, ik2, iq3, rv, 0, smem);
    FATTN_SSTAMP(13);
}

// The P.V MFMA pair of block b of a Q8_0 / Q4_0 V step (split_step): the A
// operands are the exact integer codes of this lane's 8 rows (4g..4g+3,
// 16+4g..16+4g+3) as f16 magic numbers 0x64xx = 1024 + xx (v_code_off), `pbd`
// the block's scales folded into P.  Q8_0: one u16 per row carries columns 2i
// (-> tile E_b = oe) and 2i+1 (-> tile O_b = oo), bytes xor 0x80: 1152 + q.
// Q4_0: byte i carries column i (low nibble, oe) and 16 + i (high nibble, oo):
// 1032 + (nib - 8).  b is unrolled at every call site.
template <int VT, int D>
__device__ __forceinline__ void pv_block_q(const uint8_t* vb, int b, int g, int i16, const f16x8& pbd, f32x4& oe,
                                           f32x4& oo) {
    static_assert(VT == FATTN_TYPE_Q8_0 || VT == FATTN_TYPE_Q4_0, "");
    constexpr int BB = TypeInfo<VT>::block_bytes;
    constexpr int RV = row_bytes<VT, D>();
    const int rA = 4 * g, rB = 16 + 4 * g;
    uint32_t w[8];
    u32x4 a0, a1;
    if constexpr (VT == FATTN_TYPE_Q8_0) {
        const uint8_t* cp = vb + b * BB + 2 + 2 * i16;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            w[r] = *(const uint16_t*)(cp + (rA + r) * RV);
            w[4 + r] = *(const uint16_t*)(cp + (rB + r) * RV);
        }
#pragma unroll
        for (int pr = 0; pr < 4; pr++) {
            // bytes [e_r, o_r, e_r+1, o_r+1] -> xor 0x80 -> f16 magic 0x64xx
            const uint32_t t2 = (w[2 * pr] | (w[2 * pr + 1] << 16)) ^ 0x80808080u;
            a0[pr] = perm_b32(0x64646464u, t2, 0x04020400u);
            a1[pr] = perm_b32(0x64646464u, t2, 0x04030401u);
        }
    } else {
        const uint8_t* cp = vb + b * BB + 2 + i16;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            w[r] = cp[(rA + r) * RV];
            w[4 + r] = cp[(rB + r) * RV];
        }
#pragma unroll
        for (int pr = 0; pr < 4; pr++) {
            const uint32_t x = w[2 * pr] | (w[2 * pr + 1] << 16);
            a0[pr] = (x & 0x000F000Fu) | 0x64006400u;
            a1[pr] = ((x >> 4) & 0x000F000Fu) | 0x64006400u;
        }
    }
    oe = mfma16(__builtin_bit_cast(f16x8, a0), pbd, oe);
    oo = mfma16(__builtin_bit_cast(f16x8, a1), pbd, oo);
}

// One 32-position step of one wave: S^T = K.Q^T for the step's two 16-row
// key tiles, scale + mask, online softmax of the wave's 16 packed columns,
// O^T += V^T.P^T.  `buf` is the step's LDS image [K rows | V rows | mask rows];
// `mrow`: the staged mask row of this lane's column (its query row's, or with
// head planes its own packed row's).  `wait_v()` runs between the softmax and
// P.V (the split kernel waits there for the step's V, which it issues last).
// `first`: o, l are still zero.
// Used by fattn_split_kernel.
// XF: max_bias / logit_softcap live -- the scores through xf_score (`slope`:
// this column's q head's); a template parameter, because the arguments and
// the slope held across the loop by a wave-uniform branch cost the bodies at
// their register limit spills (profiles/op_params/registers.txt).
template <int KT, int VT, int D, bool HM, bool XF, bool CP, typename WaitV>
__device__ __forceinline__ void split_step(const SplitArgs& a, const uint8_t* buf, const f16x8 (&qop)[qop_len<KT, D>()], int mrow,
                                           float slope, int g, int i16, int nvalid, bool first, float& m_run, float& l_run,
                                           f32x4 (&o)[D / 16], float (&corr)[corr_regs<VT, D, CP>()], WaitV&& wait_v) {
    using C = SplitCfg<KT, VT, D>;
    constexpr int NB = (D + QK - 1) / QK;  // k-steps of S^T (D = 80: the last one half zero)
    constexpr int NC = D / 16;
    constexpr float kNegInf = -__builtin_inff();
    constexpr bool kVQ8 = C::VTT == FATTN_TYPE_Q8_0;
    constexpr bool kVQ = !is_row16(C::VTT);
    const float log2e = 1.4426950408889634f;
    const uint8_t* kb = buf;
    const uint8_t* vb = buf + C::kBytes;
    const uint8_t* mb = buf + C::kBytes + C::vBytes;

    // -- S^T = K.Q^T for the two 16-row tiles
    f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        st[t] = f32x4{0, 0, 0, 0};
        if constexpr (KT == FATTN_TYPE_BF16) {
            // K exact; Q as its bf16 hi and lo parts, two MFMAs per k-step into one accumulator
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const f16x8 kop = k_operand<KT, D>(kb, 16 * t + i16, g, b, 0);
                st[t] = mfma16_bf(kop, qop[b], st[t]);
                st[t] = mfma16_bf(kop, qop[NB + b], st[t]);
            }
        } else if constexpr (KT == FATTN_TYPE_F16) {
#pragma unroll
            for (int b = 0; b < NB; b++) st[t] = mfma16(k_operand<KT, D>(kb, 16 * t + i16, g, b, 0), qop[b], st[t]);
        } else if constexpr (is_kv_ext(KT)) {
#pragma unroll
            for (int b = 0; b < NB; b++) st[t] = mfma16(k_operand_ext<KT, D>(kb, 16 * t + i16, g, b), qop[b], st[t]);
        } else {
            const RowScales<KT, D> ks = row_scales<KT, D>(kb + (16 * t + i16) * C::rowK);
#pragma unroll
            for (int b = 0; b < NB; b++)
                st[t] = mfma16(k_operand<KT, D>(kb, 16 * t + i16, g, b, scale_bcast(ks, b)), qop[b], st[t]);
        }
    }

    // -- u = s * scale + mask in one v_fma_mix per score (the f16 mask converts
    // inside it); positions past this wave's slice -> -inf
    float sv[8];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if constexpr (HM) {
            const uint8_t* mp = mb + mrow * (kStep * 2) + (16 * t + 4 * g) * 2;
            const u32x2 mw = *(const u32x2*)mp;
            const f16x2 m01 = as_h2(mw.x), m23 = as_h2(mw.y);
            sv[4 * t + 0] = __builtin_fmaf(st[t][0], a.scale, (float)m01.x);
            sv[4 * t + 1] = __builtin_fmaf(st[t][1], a.scale, (float)m01.y);
            sv[4 * t + 2] = __builtin_fmaf(st[t][2], a.scale, (float)m23.x);
            sv[4 * t + 3] = __builtin_fmaf(st[t][3], a.scale, (float)m23.y);
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++) sv[4 * t + r] = st[t][r] * a.scale;
        }
    }
    // max_bias / logit_softcap: the scores through xf_score instead (the fmas
    // above are then dead code)
    if constexpr (XF) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float mv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (HM) {
                const u32x2 mw = *(const u32x2*)(mb + mrow * (kStep * 2) + (16 * t + 4 * g) * 2);
                const f16x2 m01 = as_h2(mw.x), m23 = as_h2(mw.y);
                mv[0] = (float)m01.x; mv[1] = (float)m01.y; mv[2] = (float)m23.x; mv[3] = (float)m23.y;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) sv[4 * t + r] = xf_score(a.xf, a.scale, st[t][r], mv[r], slope);
        }
    }
    if (nvalid < kStep) {  // wave-uniform: only a slice's partial last step
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (16 * (j >> 2) + 4 * g + (j & 3) >= nvalid) sv[j] = kNegInf;
    }

    // -- online softmax for column m (the 4 lanes l, l^16, l^32, l^48 share it).
    // m_run is the reference max the exponentials use (natural units); it
    // moves only when a score exceeds it by more than kRescaleNat, so p stays
    // <= 2^kRescaleLog2 and most steps skip the rescale (deferred max).
    float tmax = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])),
                       fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
    tmax = grp4_max(tmax);
    if (__builtin_amdgcn_ballot_w64(tmax > m_run + kRescaleNat)) {
        const float m_new = fmaxf(m_run, tmax);
        if (!first) {  // o, l are still 0 at a wave's first step
            // (the branch is the wave's, by ballot: a column that has had no live key yet and has
            // none in this step comes here with m_run = m_new = -inf, and exp2(-inf - -inf) is NaN,
            // which 0 * NaN would keep in l and o once a later step brings it a key -- 1 there, as
            // in fattn_bd.h / fattn_pf.h: l and o are still 0; m_run = -inf with m_new finite: 0)
            const float alpha = (m_new == kNegInf) ? 1.0f : __builtin_amdgcn_exp2f((m_run - m_new) * log2e);
            l_run *= alpha;
#pragma unroll
            for (int c = 0; c < NC; c++) o[c] *= alpha;
            if constexpr (kVQ) {
#pragma unroll
                for (int b = 0; b < corr_regs<VT, D, CP>(); b++) corr[b] *= alpha;
            }
        }
        m_run = m_new;
    }
    const float m_off = (m_run == kNegInf) ? 0.0f : -m_run * log2e;
    float pv[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pv[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[j], log2e, m_off));
    l_run += ((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]));

    f16x8 pb;
    if constexpr (C::VTT != FATTN_TYPE_BF16) {
        pb.s0 = (f16)pv[0]; pb.s1 = (f16)pv[1]; pb.s2 = (f16)pv[2]; pb.s3 = (f16)pv[3];
        pb.s4 = (f16)pv[4]; pb.s5 = (f16)pv[5]; pb.s6 = (f16)pv[6]; pb.s7 = (f16)pv[7];
    }

    // -- O^T += V^T.P^T (V of step s landed)
    [[maybe_unused]] f16x8 plo;
    if constexpr (C::VTT == FATTN_TYPE_BF16) bf16_split8(pv, pb, plo);  // (before the wait: V may still fly)
    wait_v();
    if constexpr (C::VTT == FATTN_TYPE_BF16) {
        // V exact; P as its bf16 hi and lo parts (p <= 2^kRescaleLog2: both finite),
        // two MFMAs per column group into one accumulator
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const f16x8 vop = v_operand_f16<VT, D>(vb, c, g, i16);
            o[c] = mfma16_bf(vop, pb, o[c]);
            o[c] = mfma16_bf(vop, plo, o[c]);
        }
    } else if constexpr (C::VTT == FATTN_TYPE_F16) {
#pragma unroll
        for (int c = 0; c < NC; c++) o[c] = mfma16(v_operand_f16<VT, D>(vb, c, g, i16), pb, o[c]);
    } else if constexpr (CP) {
        // column-packed (col_packed): this lane's column c folds block min(c, NB - 1)
        // alone -- the scales of its 8 rows (4g..4g+3, 16+4g..16+4g+3) as u16 reads at
        // a per-lane offset (columns >= NB: a valid block, their tiles are never
        // read), one P' and one corr; every block's MFMA pair takes that P'
        static_assert(D % QK == 0, "quantised rows are whole blocks");
        constexpr int BB = TypeInfo<C::VTT>::block_bytes;
        const int rA = 4 * g, rB = 16 + 4 * g;
        const uint8_t* sp = vb + BB * min(i16, NB - 1);
        uint32_t sw[8];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sw[r] = *(const uint16_t*)(sp + (rA + r) * C::rowV);
            sw[4 + r] = *(const uint16_t*)(sp + (rB + r) * C::rowV);
        }
        const f16x2 d01 = as_h2(perm_b32(sw[1], sw[0], 0x05040100u)), d23 = as_h2(perm_b32(sw[3], sw[2], 0x05040100u));
        const f16x2 d45 = as_h2(perm_b32(sw[5], sw[4], 0x05040100u)), d67 = as_h2(perm_b32(sw[7], sw[6], 0x05040100u));
        f16x8 pbd;
        pbd.s01 = pb.s01 * d01;
        pbd.s23 = pb.s23 * d23;
        pbd.s45 = pb.s45 * d45;
        pbd.s67 = pb.s67 * d67;
        const f16x2 one2 = {(f16)1.0f, (f16)1.0f};
        corr[0] = __builtin_amdgcn_fdot2(pbd.s01, one2, corr[0], false);
        corr[0] = __builtin_amdgcn_fdot2(pbd.s23, one2, corr[0], false);
        corr[0] = __builtin_amdgcn_fdot2(pbd.s45, one2, corr[0], false);
        corr[0] = __builtin_amdgcn_fdot2(pbd.s67, one2, corr[0], false);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            pv_block_q<C::VTT, D>(vb, b, g, i16, pbd, o[2 * b], o[2 * b + 1]);
        }
    } else {
        const int rA = 4 * g, rB = 16 + 4 * g;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            constexpr int BB = TypeInfo<C::VTT>::block_bytes;
            // block-b scales of this lane's 8 rows (4g..4g+3, 16+4g..16+4g+3):
            // the dword holding each, then f16 pairs {row r, row r+1}
            uint32_t sw[8];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if constexpr (C::rowV % 4 != 0) {  // D = 96: rows not a whole number of dwords
                    sw[r] = *(const uint16_t*)(vb + (rA + r) * C::rowV + BB * b);
                    sw[4 + r] = *(const uint16_t*)(vb + (rB + r) * C::rowV + BB * b);
                } else {
                    sw[r] = *(const uint32_t*)(vb + (rA + r) * C::rowV + ((BB * b) & ~3));
                    sw[4 + r] = *(const uint32_t*)(vb + (rB + r) * C::rowV + ((BB * b) & ~3));
                }
            }
            const uint32_t sel = scale_hi<C::VTT, D>(b) ? 0x07060302u : 0x05040100u;  // b is unrolled
            const f16x2 d01 = as_h2(perm_b32(sw[1], sw[0], sel)), d23 = as_h2(perm_b32(sw[3], sw[2], sel));
            const f16x2 d45 = as_h2(perm_b32(sw[5], sw[4], sel)), d67 = as_h2(perm_b32(sw[7], sw[6], sel));
            // P'_b = P * d_b (element j <-> row of element j of the A operand)
            f16x8 pbd;
            pbd.s01 = pb.s01 * d01;
            pbd.s23 = pb.s23 * d23;
            pbd.s45 = pb.s45 * d45;
            pbd.s67 = pb.s67 * d67;
            const f16x2 one2 = {(f16)1.0f, (f16)1.0f};
            corr[b] = __builtin_amdgcn_fdot2(pbd.s01, one2, corr[b], false);
            corr[b] = __builtin_amdgcn_fdot2(pbd.s23, one2, corr[b], false);
            corr[b] = __builtin_amdgcn_fdot2(pbd.s45, one2, corr[b], false);
            corr[b] = __builtin_amdgcn_fdot2(pbd.s67, one2, corr[b], false);
            if constexpr (!is_kv_ext(C::VTT)) {  // Q8_0 / Q4_0
                pv_block_q<C::VTT, D>(vb, b, g, i16, pbd, o[2 * b], o[2 * b + 1]);
            } else {
                // Q4_1 / Q5_0 / Q5_1: byte i of qs carries column i (low nibble) and 16 + i
                // (high nibble), bits i and 16 + i of the row's qh their fifth bits
                constexpr int VTT = C::VTT;
                if constexpr (has_min(VTT)) {
                    // the second accumulator sum P (m_b + c d_b): m in the high halves of the
                    // d | m dwords; c d is exact in f16 (c a power of two)
                    const f16x2 m01 = as_h2(perm_b32(sw[1], sw[0], 0x07060302u)), m23 = as_h2(perm_b32(sw[3], sw[2], 0x07060302u));
                    const f16x2 m45 = as_h2(perm_b32(sw[5], sw[4], 0x07060302u)), m67 = as_h2(perm_b32(sw[7], sw[6], 0x07060302u));
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s01, m01, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s23, m23, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s45, m45, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s67, m67, corr[NB + b], false);
                    constexpr f16 cc = (f16)(float)v_code_centre<VTT>();
                    const f16x2 c2 = {cc, cc};
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s01, d01 * c2, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s23, d23 * c2, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s45, d45 * c2, corr[NB + b], false);
                    corr[NB + b] = __builtin_amdgcn_fdot2(pb.s67, d67 * c2, corr[NB + b], false);
                }
                const uint8_t* cp = vb + b * BB + qs_off(VTT) + i16;
                uint32_t w[8], hb[8];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    w[r] = cp[(rA + r) * C::rowV];
                    w[4 + r] = cp[(rB + r) * C::rowV];
                }
                if constexpr (has_qh(VTT)) {
                    // {bit i16 at bit 0, bit 16 + i16 at bit 16} of each row's qh
                    const int HO = BB * b + qh_off(VTT);  // (b is unrolled: a constant)
#pragma unroll
                    for (int r = 0; r < 8; r++) {
                        const uint8_t* hp = vb + ((r < 4 ? rA : rB - 4) + r) * C::rowV + HO;
                        uint32_t qh;
                        if (HO % 4 == 0) qh = *(const uint32_t*)hp;
                        else qh = (uint32_t)*(const uint16_t*)hp | ((uint32_t)*(const uint16_t*)(hp + 2) << 16);
                        hb[r] = (qh >> i16) & 0x00010001u;
                    }
                }
                u32x4 al, ah;  // f16 pairs 1024 + code (exact)
#pragma unroll
                for (int pr = 0; pr < 4; pr++) {
                    const uint32_t x = w[2 * pr] | (w[2 * pr + 1] << 16);
                    al[pr] = (x & 0x000F000Fu) | 0x64006400u;
                    ah[pr] = ((x >> 4) & 0x000F000Fu) | 0x64006400u;
                    if constexpr (has_qh(VTT)) {
                        al[pr] |= perm_b32(hb[2 * pr + 1], hb[2 * pr], 0x0c040c00u) << 4;
                        ah[pr] |= perm_b32(hb[2 * pr + 1], hb[2 * pr], 0x0c060c02u) << 4;
                    }
                }
                o[2 * b] = mfma16(__builtin_bit_cast(f16x8, al), pbd, o[2 * b]);
                o[2 * b + 1] = mfma16(__builtin_bit_cast(f16x8, ah), pbd, o[2 * b + 1]);
            }
        }
    }

}

// waves per SIMD the split kernel's register budget allows (__launch_bounds__)
template <int KT, int D, int GRAN>
constexpr int split_waves_per_simd() {
    return split_bounds_wps(KT, GRAN, D);
}

// NWV waves per workgroup (4, 8 or 16), each streaming its own slice of the
// chunk.  More waves per CU put more LDS-DMA instructions in flight from more
// issuing waves (tools/hbm_probe: a 35.7 MB read takes 8.3 us from 256 4-wave
// workgroups, 6.4 us from 16 waves per CU) and let the SIMDs interleave the
// steps' dependent LDS -> VALU -> MFMA chains.
// XF (split_step): instantiated for NWV = 4 only; the planner sizes a launch
// with max_bias / logit_softcap live for 4 waves (size_split).
template <int KT, int VT, int D, int GRAN, bool HM, int NWV, int EPI, bool XF = false, typename A = SplitArgs>
__global__ __launch_bounds__(NWV * kWave, split_bounds_wps(KT, GRAN, D)) void fattn_split_kernel(
    const A a) {
    using C = SplitCfg<KT, VT, D>;
    using P = StepPlan<KT, VT, D, GRAN>;
    constexpr int NI = P::NIKV + (HM ? P::NIM : 0);  // VMEM instructions per step
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NB = (D + QK - 1) / QK;  // 32-wide k-steps of QK^T (= ggml blocks per row; D = 80: 3)
    constexpr int NC = D / 16;   // 16-wide output column groups (MFMA tiles of O^T)
    constexpr float kNegInf = -__builtin_inff();
    // quantised V: the A operand is the exact integer code plus the magic-number
    // offset (v_code_off: 1152 for Q8_0, 1032 for Q4_0, ...) with the block scale folded
    // into P; corr[b] accumulates sum(P * d_b) so the offset comes off once in the
    // epilogue (Q4_1 / Q5_1: corr[NB + b] accumulates sum(P * (m_b + c d_b)), added there)

    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; readfirstlane lets the compiler see it, so the
    // slice bounds, loop counts and LDS-DMA bases (M0) stay scalar
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int i16 = lane & 15;
    FATTN_SSTAMP_INIT();
    FATTN_SSTAMP(0);

    // ---- tile decode: y -> (kv head, head subgroup, query-row tile)
    int chunk, y, iq3;
    tile_coords(a, chunk, y, iq3);
    int qt, hs, ik2, ik3;
    tile_decode<true>(a, y, iq3, qt, hs, ik2, ik3);

    // this lane's MFMA column m = i16 -> (query row, q head); column-packed
    // (col_packed): columns 0 .. D/QK - 1 all carry the tile's one row, packed row 0
    constexpr bool CP = col_packed<C::VTT, EPI>();
    const int m = (CP && i16 < D / QK) ? 0 : i16;
    const int mq = div_R(a, m);
    const int mh = hs * a.R + (m - mq * a.R);
    const int iq1 = qt * a.QPT + mq;
    const int iq2 = ik2 * a.rk2 + mh;
    const bool row_ok = (m < a.QPT * a.R) && (iq1 < a.NQ) && (mh < a.rk2);
    const int mrow = a.m_hp ? m : (mq < a.QPT ? mq : 0);  // this column's staged mask row (split_step)
    const float slope = XF ? xf_slope(a.xf, iq2) : 1.0f;  // this column's q head's ALiBi slope

    // ---- this wave's KV slice
    const int wl = a.chunk_len / NWV;
    const int c_hi = min(a.N, (chunk + 1) * a.chunk_len);
    const int w_lo = chunk * a.chunk_len + wave * wl;
    const int w_hi = min(c_hi, w_lo + wl);
    const int nsteps = w_hi > w_lo ? (w_hi - w_lo + kStep - 1) / kStep : 0;
    const int nbuf = a.nbuf;

    StepSrc rs = kv_sources<HM>(a, ik2, ik3, iq3);
    split_mask_src(a, rs, ik2, hs);
    uint8_t* wbuf = smem + wave * a.wave_bytes;
    const int mrow0 = qt * a.QPT;
    uint32_t ml[P::NIM];
    mask_lane_offsets<KT, VT, D, GRAN>(a, rs, mrow0, lane, ml);

    // Staggered priorities: the waves of a CU otherwise interleave their DMA
    // issue, so every wave's last piece lands near the end of the burst and
    // all compute starts late; by priority the first waves' steps land first
    // and their compute overlaps the rest of the stream.
    // (split_prio 1: no priorities; 2: staggered only while the first steps issue)
    // (NWV > 4: by the wave's rank among the waves of its SIMD, wave / 4)
    if (a.split_prio != 1) {
        switch (__builtin_amdgcn_readfirstlane(NWV == 4 ? wave : wave >> 2)) {
            case 0: __builtin_amdgcn_s_setprio(3); break;
            case 1: __builtin_amdgcn_s_setprio(2); break;
            case 2: __builtin_amdgcn_s_setprio(1); break;
            default: break;
        }
    }

    // ---- Q^T operand (B of S^T = K.Q^T), rounded to f16 like src/utils.h:10
    // (lanes of unused columns point past the descriptor: zeros, no traffic).
    // Loaded first, as asm (no compiler wait), so that waiting for Q leaves the
    // steps' LDS-DMA behind it in flight: compute starts as soon as step 0's K
    // and mask land.
    u32x4 qraw[NB][2];
    {
        const i32x4 qs = make_srd(a.q + (int64_t)iq3 * a.q_nb3, a.q_span);
        const uint32_t qoff = row_ok ? (uint32_t)iq1 * (uint32_t)a.q_nb1 + (uint32_t)iq2 * (uint32_t)a.q_nb2 + 32 * g
                                     : a.q_span;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            // (D = 80: dims past D come from past the descriptor, as zeros)
            const uint32_t qb = (D % QK == 0 || 32 * b + 8 * g < D) ? qoff + 128 * b : a.q_span;
            qraw[b][0] = ld_buf_untracked<kTagQ>(qs, qb);
            qraw[b][1] = ld_buf_untracked<kTagQ>(qs, qb + 16);
        }
    }
    // ---- -inf steps (src/flash-llama.h:275-278 skips their compute): a step
    // whose mask is -inf for every key of every query row of the tile adds
    // exp(-inf) = 0 to o and l.  Its K and V are not fetched: their DMA goes
    // through empty descriptors (no HBM traffic, zeros in LDS; the mask still
    // lands, so every score is -inf and the step's compute adds exactly 0).
    // Loop and vmcnt accounting are unchanged.  The mask words of the wave's
    // steps are read here beside Q (their wait is Q's): one (row, step) pair
    // of 64 B per lane, when the tile's rows x steps fit the wave and the
    // wave has at least 4 steps; the prologue's steps are fetched regardless.
    // Measured (profiles/r02_skip): config 3 (2 steps per wave, no prefetch)
    // unchanged; 8 heads x N = 32768 with 70 % of the cache masked 16.1 vs
    // 17.1-17.5 us; the same unmasked 17.6-18.2 vs 16.9-17.5 us (the loads
    // ahead of the first wait).  Reading the words after step 0 instead, or
    // skipping by control flow in the loop, measured slower everywhere.
    const int pro = min(nbuf, nsteps);  // steps issued before the loop
    // (head planes: one staged row per packed (query row, head) pair -- all of
    // them are looked at)
    const int n_rows = !HM ? 0 : a.m_hp ? tile_rows(a, qt, hs) : min(a.QPT, a.NQ - mrow0);
    const bool pre = HM && a.step_skip && nsteps >= 4 && n_rows * nsteps <= kWave;
    u32x4 mraw[4] = {};
    if (pre) {
        const int r = lane / nsteps, st = lane - r * nsteps;
        const uint32_t moff = r < n_rows ? mask_row_off(a, rs, mrow0, r) + (uint32_t)(w_lo + st * kStep) * 2
                                         : a.m_span_h;  // past the descriptor: no traffic
#pragma unroll
        for (int j = 0; j < 4; j++) mraw[j] = ld_buf_untracked<kTagMaskWords>(rs.m, moff + 16 * j);
    }
    for (int s = 0; s < pro; s++) {
        issue_step<KT, VT, D, GRAN, HM>(a, rs, w_lo + s * kStep, ml, wbuf + s * C::stepBytes, lane);
    }
    // this launch's stamp on the tile's arrival word, by each lane that will
    // count an arrival: issued after the prologue's DMA, so no wait is spent
    // on it (at most one DMA instruction's worth in the counted waits below)
    if (a.n_chunks > 1 && a.merge_launch != 1 && lane == 0 && (EPI == 1 || wave == 0))
        arrival_begin(a, (int64_t)iq3 * gridDim.y + y);

    FATTN_SSTAMP(1);
    if (a.split_prio == 2) __builtin_amdgcn_s_setprio(0);
    wait_steps<NI>(pro);  // Q and the mask words landed (the steps issued after them may fly on)
    // every untracked result, on every path, passes its fence right behind
    // that wait (nothing reads or moves those registers before it)
#pragma unroll
    for (int b = 0; b < NB; b++) {
        reg_fence<kTagQ>(qraw[b][0]);
        reg_fence<kTagQ>(qraw[b][1]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) reg_fence<kTagMaskWords>(mraw[j]);
    f16x8 qop[qop_len<KT, D>()];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const f32x4 x0 = __builtin_bit_cast(f32x4, qraw[b][0]), x1 = __builtin_bit_cast(f32x4, qraw[b][1]);
        if constexpr (KT == FATTN_TYPE_BF16) {
            // bf16 cache: Q as its bf16 hi and lo parts (qop[b], qop[NB + b]; bf16_split8)
            const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            bf16_split8(x, qop[b], qop[NB + b]);
        } else {
            f16x8 h;
            h.s0 = (f16)x0.x; h.s1 = (f16)x0.y; h.s2 = (f16)x0.z; h.s3 = (f16)x0.w;
            h.s4 = (f16)x1.x; h.s5 = (f16)x1.y; h.s6 = (f16)x1.z; h.s7 = (f16)x1.w;
            qop[b] = h;
        }
    }
    // bit s: step s has a live key (steps past 64 and unprefetched waves: all)
    uint64_t live = ~0ull;
    if (pre) {
        constexpr uint32_t kNegInf2 = 0xFC00FC00u;  // two f16 -inf
        bool lv = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            lv |= (mraw[j].x != kNegInf2) | (mraw[j].y != kNegInf2) | (mraw[j].z != kNegInf2) | (mraw[j].w != kNegInf2);
        }
        const uint64_t bl = __builtin_amdgcn_ballot_w64(lv && lane < n_rows * nsteps);
        live = 0;
        for (int r = 0; r < n_rows; r++) live |= bl >> (r * nsteps);
    }

    float m_run = kNegInf;  // reference max (natural units) of column m
    float l_run = 0.0f;     // this lane's partial row sum
    f32x4 o[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) o[c] = f32x4{0, 0, 0, 0};
    float corr[corr_regs<VT, D, CP>()];
#pragma unroll
    for (int b = 0; b < corr_regs<VT, D, CP>(); b++) corr[b] = 0.0f;

    int cur = 0;  // buffer of step s
    for (int s = 0; s < nsteps; s++) {
        const int ahead = min(nbuf - 1, nsteps - 1 - s);  // steps issued after step s
        // K and mask of step s landed (its V and the later steps may fly on)
        wait_steps_plus<NI, P::NIV>(ahead);
        if (s < 8) FATTN_SSTAMP(2 + s);
#ifdef FATTN_DIAG_NOCOMPUTE
        // diagnostic build only: memory-side ceiling of this access pattern
        wait_steps<NI>(ahead);
        if (s + nbuf < nsteps) {
            issue_step<KT, VT, D, GRAN, HM>(a, rs, w_lo + (s + nbuf) * kStep, ml, wbuf + cur * C::stepBytes, lane);
        }
        cur = (cur + 1 == nbuf) ? 0 : cur + 1;
        continue;
#endif
        const int n0 = w_lo + s * kStep;
        int s_opaque = s;  // hides "first step" from loop peeling (a second copy of the body)
        asm volatile("" : "+s"(s_opaque));
        split_step<KT, VT, D, HM, XF, CP>(a, wbuf + cur * C::stepBytes, qop, mrow, slope, g, i16, min(kStep, w_hi - n0),
                                          s_opaque == 0, m_run, l_run, o, corr, [&] { wait_steps<NI>(ahead); });
        if (nsteps <= 4 && s < 2) FATTN_SSTAMP(6 + 2 * s);  // (stamps build: step s computed)

        // -- refill this buffer with step s + nbuf (K/V not fetched if -inf)
        if (s + nbuf < nsteps) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int sn = s + nbuf;
            issue_step<KT, VT, D, GRAN, HM>(a, rs, w_lo + sn * kStep, ml, wbuf + cur * C::stepBytes, lane,
                                            sn >= 64 || ((live >> sn) & 1));
            if (nsteps <= 4 && s < 2) FATTN_SSTAMP(7 + 2 * s);  // (stamps build: step s + nbuf issued)
        }
        cur = (cur + 1 == nbuf) ? 0 : cur + 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#ifdef FATTN_DIAG_NOTAIL
    // diagnostic build only: stop before the merge / publish tail
    {
        float keep = l_run + m_run;  // keep the loop's results (all of O) alive
#pragma unroll
        for (int c = 0; c < NC; c++) keep += o[c].x + o[c].y + o[c].z + o[c].w;
        if (keep == 12345.0f) a.dst[0] = keep;
    }
    return;
#endif
    FATTN_SSTAMP(10);
    split_epilogue<KT, VT, D, NWV, EPI>(a, o, m_run, l_run, corr, wave, lane, qt, hs, ik2, iq3, y, chunk, smem, a.wave_bytes,
                                   true, false);
    FATTN_SSTAMP_FLUSH();
}

// ---------------------------------------------------------------- loader waves
// The split kernel with the refill of its later steps taken off the compute
// waves (one-row tiles whose whole chunk fits the LDS; config 3).  In
// fattn_split_kernel each wave issues its own steps: a wave that issues step
// s + 1 before computing step s stalls on the CU's full memory queue before it
// can compute (both steps in flight: 12.2 vs 11.3 us), and a wave that issues
// it after computing step s leaves that queue idle for the whole of step s's
// compute (stamps, round 6: step 0 lands at 3.9 us, is computed by 5.7, step 1
// issued at 6.2).  Here each compute wave issues its step 0 (as before), the
// workgroup meets at one barrier, and NLD loader waves then issue every later
// step of every compute wave -- into the queue behind all of step 0 -- and hand
// each (wave, step) over by two LDS flags (K + mask landed, V landed), set
// behind counted vmcnt waits; the compute waves never wait on an issue.  (A
// first form whose loaders issued step 0 too took 13.5 us: the loaders could
// flag step 0 only after issuing everything, profiles/r06_c.)  Same compute
// (split_step) and epilogue (wg_row_merge).  Every step of the chunk is
// resident: LDS = NWV x steps x stepBytes + flags.
constexpr int kSplitLoaders = 4;
constexpr int kSplitLdFlagBytes = 256;  // [8 waves][<= 2 steps][2] u32 flags, past the step buffers

// (LDS flag of a (wave, step) hand-off: relaxed atomic load, polled with
// s_sleep; the empty asm keeps every later LDS read below the poll -- LDS
// instructions of one wave execute in order, and the loader set the flag only
// after its counted wait saw the DMA data written)
__device__ __forceinline__ void wait_lds_flag(const uint32_t* f) {
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0)
        __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}

template <int KT, int VT, int D, bool HM, int NWV, int NLD, typename A = SplitArgs>
__global__ __launch_bounds__((NWV + NLD) * kWave, 1) void fattn_split_ld_kernel(const A a) {
    using C = SplitCfg<KT, VT, D>;
    using P = StepPlan<KT, VT, D, 16>;
    constexpr int NI = P::NIKV + (HM ? P::NIM : 0);  // VMEM instructions per step
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NB = (D + QK - 1) / QK;
    constexpr int NC = D / 16;
    constexpr float kNegInf = -__builtin_inff();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int i16 = lane & 15;
    FATTN_SSTAMP_INIT();
    FATTN_SSTAMP(0);

    int chunk, y, iq3;
    tile_coords(a, chunk, y, iq3);
    int qt, hs, ik2, ik3;
    tile_decode<true>(a, y, iq3, qt, hs, ik2, ik3);
    const int wl = a.chunk_len / NWV;    // positions per compute wave
    const int spw = a.nbuf;              // steps per compute wave, all resident (planner: nbuf == steps)
    const int mrow0 = qt * a.QPT;
    const int c_hi = min(a.N, (chunk + 1) * a.chunk_len);
    uint32_t* flags = (uint32_t*)(smem + NWV * a.wave_bytes);  // [NWV][spw][2]: K + mask, V (step 0 unused)
    StepSrc rs = kv_sources<HM>(a, ik2, ik3, iq3);
    split_mask_src(a, rs, ik2, hs);
    uint32_t ml[P::NIM];
    mask_lane_offsets<KT, VT, D, 16>(a, rs, mrow0, lane, ml);

    if (wave >= NWV) {
        // ---- loader: zero the flags, meet the compute waves once they have
        // issued their step 0, then units u = (s - 1) * NWV + w, s >= 1, dealt
        // round-robin; U units per loader, issued back to back, handed over
        // oldest first (K + mask when all but the unit's V and the later
        // units landed, V when all but the later units)
        const int L = wave - NWV;
        if (L == 0 && lane < NWV * spw * 2) flags[lane] = 0u;
        __syncthreads();
        const int U = (spw - 1) * NWV / NLD;  // (planner: <= 4, a whole number)
        for (int k = 0; k < U; k++) {
            const int u = L + NLD * k, w = u % NWV, s = 1 + u / NWV;
            const int n0 = chunk * a.chunk_len + w * wl + s * kStep;
            issue_step<KT, VT, D, 16, HM>(a, rs, n0, ml, smem + w * a.wave_bytes + s * C::stepBytes, lane);
        }
        FATTN_SSTAMP(1);
        for (int k = 0; k < U; k++) {
            const int u = L + NLD * k, w = u % NWV, s = 1 + u / NWV;
            uint32_t* f = flags + (w * spw + s) * 2;
            wait_steps_plus<NI, P::NIV>(U - 1 - k);
            if (lane == 0) __hip_atomic_store(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            wait_steps<NI>(U - 1 - k);
            if (lane == 0) __hip_atomic_store(f + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();  // wg_row_merge's one barrier (the loaders then leave)
        FATTN_SSTAMP_FLUSH();
        return;
    }

    // ---- compute wave: the split kernel's, its later steps refilled by the loaders
    // (column-packed as there: columns 0 .. D/QK - 1 carry the tile's one row)
    constexpr bool CP = col_packed<C::VTT, 2>();
    const int m = (CP && i16 < D / QK) ? 0 : i16;
    const int mq = div_R(a, m);
    const int mh = hs * a.R + (m - mq * a.R);
    const int iq1 = qt * a.QPT + mq;
    const int iq2 = ik2 * a.rk2 + mh;
    const bool row_ok = (m < a.QPT * a.R) && (iq1 < a.NQ) && (mh < a.rk2);
    const int mrow = a.m_hp ? m : (mq < a.QPT ? mq : 0);  // this column's staged mask row (split_step)
    const int w_lo = chunk * a.chunk_len + wave * wl;
    const int w_hi = min(c_hi, w_lo + wl);
    const int nsteps = w_hi > w_lo ? (w_hi - w_lo + kStep - 1) / kStep : 0;
    uint8_t* wbuf = smem + wave * a.wave_bytes;
    // Q first, untracked (its wait leaves step 0's DMA in flight), then step 0
    // (fetched whatever the wave's slice: the loaders' counts assume it)
    u32x4 qraw[NB][2];
    {
        const i32x4 qs = make_srd(a.q + (int64_t)iq3 * a.q_nb3, a.q_span);
        const uint32_t qoff = row_ok ? (uint32_t)iq1 * (uint32_t)a.q_nb1 + (uint32_t)iq2 * (uint32_t)a.q_nb2 + 32 * g
                                     : a.q_span;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const uint32_t qb = (D % QK == 0 || 32 * b + 8 * g < D) ? qoff + 128 * b : a.q_span;
            qraw[b][0] = ld_buf_untracked<kTagQ>(qs, qb);
            qraw[b][1] = ld_buf_untracked<kTagQ>(qs, qb + 16);
        }
    }
    issue_step<KT, VT, D, 16, HM>(a, rs, w_lo, ml, wbuf, lane);
    if (a.n_chunks > 1 && lane == 0 && wave == 0) arrival_begin(a, (int64_t)iq3 * gridDim.y + y);
    FATTN_SSTAMP(1);
    __syncthreads();  // every compute wave's step 0 is in the queue: the loaders may issue
    wait_steps<NI>(1);  // Q landed (step 0 may fly on)
#pragma unroll
    for (int b = 0; b < NB; b++) {
        reg_fence<kTagQ>(qraw[b][0]);
        reg_fence<kTagQ>(qraw[b][1]);
    }
    f16x8 qop[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const f32x4 x0 = __builtin_bit_cast(f32x4, qraw[b][0]), x1 = __builtin_bit_cast(f32x4, qraw[b][1]);
        f16x8 h;
        h.s0 = (f16)x0.x; h.s1 = (f16)x0.y; h.s2 = (f16)x0.z; h.s3 = (f16)x0.w;
        h.s4 = (f16)x1.x; h.s5 = (f16)x1.y; h.s6 = (f16)x1.z; h.s7 = (f16)x1.w;
        qop[b] = h;
    }

    float m_run = kNegInf;
    float l_run = 0.0f;
    f32x4 o[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) o[c] = f32x4{0, 0, 0, 0};
    float corr[corr_regs<VT, D, CP>()];
#pragma unroll
    for (int b = 0; b < corr_regs<VT, D, CP>(); b++) corr[b] = 0.0f;
    for (int s = 0; s < nsteps; s++) {
        const uint32_t* f = flags + (wave * spw + s) * 2;
        if (s == 0) wait_steps_plus<NI, P::NIV>(0);  // own DMA: K + mask landed
        else wait_lds_flag(f);
        if (s < 2) FATTN_SSTAMP(2 + s);
        const int n0 = w_lo + s * kStep;
        int s_opaque = s;
        asm volatile("" : "+s"(s_opaque));
        split_step<KT, VT, D, HM, false, CP>(a, wbuf + s * C::stepBytes, qop, mrow, 1.0f, g, i16, min(kStep, w_hi - n0), s_opaque == 0,
                                  m_run, l_run, o, corr, [&] {
                                      if (s == 0) wait_vmcnt_c<0>();
                                      else wait_lds_flag(f + 1);
                                  });
        if (s < 2) FATTN_SSTAMP(6 + 2 * s);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    FATTN_SSTAMP(10);
    split_epilogue<KT, VT, D, NWV, 2>(a, o, m_run, l_run, corr, wave, lane, qt, hs, ik2, iq3, y, chunk, smem,
                                      a.wave_bytes, true, false);
    FATTN_SSTAMP_FLUSH();
}

// ---------------------------------------------------------------- merge launch
// the second-launch merge of the split kernel's multi-row tiles
// (fattn_chunk_merge_kernel, fattn_tile.h): 16-row tiles with head subgroups
struct SplitMergeGeom : MergeGeomBase {
    static constexpr int rows = kRows;
    static constexpr bool hsub = true;
};

// ---------------------------------------------------------------- combine
// Log-sum-exp merge of a tile's chunk partials (fa_reduce,
// flash_row_float.h:415-472, in fp32 and parallel), run by the tile's last
// workgroup.  16 thread groups = rv rows x G chunk subsets.  Every thread
// issues its (m, l) load and its first batch of partial loads before one wait
// (one memory round trip when ceil(n_chunks / G) <= CB); the (m, l) pairs
// reduce with VALU segmented reductions (DPP + permlane swaps); the G subsets
// of a row are summed with all LDS reads in flight at once.  Fixed order:
// deterministic.  Partial row rr is packed row row_base + rr of the tile
// (row_base != 0: the multi-query kernel's 16-row subtiles).  Written for
// 256 threads; in a 512-thread workgroup the upper half only joins the
// barriers (its groups, rows and chunks are all out of range).
template <int D, int CB, typename A>
__device__ __forceinline__ void combine_tile(const A& a, int64_t tile, int qt, int hs, int ik2, int iq3,
                                             int rv, int row_base, uint8_t* smem) {
    constexpr float kNegInf = -__builtin_inff();
    constexpr int EPT = epi_ept<D>();
    // CB = chunks per load batch: with 8 (the split kernel at D = 128) every
    // thread's partials come in ONE memory round trip up to 8 chunks per thread
    // (config 4: 32 chunks x 4 rows); batch slots past the thread's chunks
    // issue no load
    float(*red)[D] = (float(*)[D])smem;                                // [16][D]
    float(*wts)[64] = (float(*)[64])(smem + kRows * D * 4);            // [16][64]
    float* rowL = (float*)(smem + kRows * D * 4 + kRows * 64 * 4);     // [16]
    const int NCH = a.n_chunks;
    const int G = max(1, kRows / max(rv, 1));
    const int grp = threadIdx.x / 16, tj = threadIdx.x % 16, d0 = tj * EPT;
    const int64_t sb = tile * NCH;
    const int r = grp / G, cg = grp % G;
    const bool active = grp < rv * G && d0 < D;  // (D = 80 / 96: threads past the row's dims idle)
    const int kmax = active ? (NCH - cg + G - 1) / G : 0;
    auto fl = [](uint32_t x) { return __builtin_bit_cast(float, x); };
    // partial loads of chunks cg + (k0 + kk) * G through a buffer descriptor
    // over this tile's partials: slots past kmax use an out-of-range offset
    // (zeros, no memory traffic; zero weight too).  Every lane executes every
    // load -- an asm load under a branch would leave a register copy (phi)
    // reading the destination before its wait.
    const uint32_t obytes = (uint32_t)(NCH * kRows * D * 4);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the loads below the count)
    const __amdgpu_buffer_rsrc_t osrd = make_rsrc(a.ws_o + sb * kRows * D, obytes);
    auto issue = [&](u32x4 (&v)[CB][EPT / 4], int k0) {
#pragma unroll
        for (int kk = 0; kk < CB; kk++) {
            const int c = cg + (k0 + kk) * G;
            const uint32_t off =
                (k0 + kk < kmax) ? (uint32_t)(((c * kRows + (active ? r : 0)) * D + d0) * 4) : obytes;
#pragma unroll
            for (int e = 0; e < EPT / 4; e++) v[kk][e] = ld_sc1_buf(osrd, off + 16 * e);
        }
    };
    u32x4 v[CB][EPT / 4];
    issue(v, 0);
    // (m, l) of chunk c of row r in thread r * NCP + c (NCP = next power of
    // two >= NCH, <= 64)
    const int NCP = a.ncp;
    const int mr = threadIdx.x / NCP, mc = threadIdx.x % NCP;
    const bool has_ml = mr < rv && mc < NCH;
    const u32x2 mlb = ld_sc1_x2(a.ws_ml + 2 * ((sb + min(mc, NCH - 1)) * kRows + (has_ml ? mr : 0)));
    const float mlm = has_ml ? fl(mlb.x) : kNegInf;
    const float Mr = seg_reduce<true>(mlm, NCP);
    const float wt = (mlm == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(mlm - Mr);
    const float Lr = seg_reduce<false>(has_ml ? wt * fl(mlb.y) : 0.0f, NCP);
    if (mr < rv) {
        wts[mr][mc] = wt;
        // with sinks rowL holds the row's whole factor instead (sink_inv: M is known
        // here and nowhere below), -1 for a fully masked row -- a factor is >= 0
        if (mc == 0) {
            float lr = Lr;
            if (const float* sinks = a.sinks) {  // (wave-uniform)
                const int pr = row_base + mr;
                bool dead;
                const float inv = sink_inv(Mr, Lr, sinks[ik2 * a.rk2 + hs * a.R + (pr - div_R(a, pr) * a.R)], dead);
                lr = dead ? -1.0f : inv;
            }
            rowL[mr] = lr;
            // the row's log-sum-exp: (Mr, Lr) are known here and nowhere below, so this
            // one store stands before the row's dst stores
            if (float* const lse = lse_of(a)) {  // (wave-uniform)
                const int pr = row_base + mr, rq = div_R(a, pr);
                const int riq2 = ik2 * a.rk2 + hs * a.R + (pr - rq * a.R);
                lse[((int64_t)iq3 * a.NQ + qt * a.QPT + rq) * a.H + riq2] =
                    row_lse(Mr, Lr, a.sinks ? a.sinks[riq2] : kNegInf, row_dead(Mr, Lr));
            }
        }
    }
    __syncthreads();

    // fold this thread's chunks
    if (active) {
        float s8[EPT];
#pragma unroll
        for (int e = 0; e < EPT; e++) s8[e] = 0.0f;
        for (int k0 = 0; k0 < kmax; k0 += CB) {
            if (k0 > 0) issue(v, k0);
#pragma unroll
            for (int kk = 0; kk < CB; kk++) {
                const int c = cg + (k0 + kk) * G;
                const float w = (k0 + kk < kmax) ? wts[r][min(c, NCH - 1)] : 0.0f;
#pragma unroll
                for (int e = 0; e < EPT / 4; e++) {
                    s8[4 * e] += w * fl(v[kk][e].x);
                    s8[4 * e + 1] += w * fl(v[kk][e].y);
                    s8[4 * e + 2] += w * fl(v[kk][e].z);
                    s8[4 * e + 3] += w * fl(v[kk][e].w);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < EPT; e += 4) *(f32x4*)&red[grp][d0 + e] = f32x4{s8[e], s8[e + 1], s8[e + 2], s8[e + 3]};
    }
    __syncthreads();

    // sum the G subsets of each row, normalise, store: thread -> (row, 4 dims),
    // all of its 16-B LDS reads issued before any is consumed
    // (a 512-thread workgroup's upper half takes no part)
    for (int t = threadIdx.x; t < rv * (D / 4) && threadIdx.x < kSplitWaves * kWave; t += kSplitWaves * kWave) {
        const int rr = t / (D / 4), dq = (t % (D / 4)) * 4;
        f32x4 part[kRows];
#pragma unroll
        for (int k = 0; k < kRows; k++) part[k] = *(const f32x4*)&red[min(rr * G + k, kRows - 1)][dq];
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kRows; k++) x += (k < G) ? part[k] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // (with sinks rowL holds the factor, -1 for a fully masked row: above)
        const float Lrow = rowL[rr];
        const bool with_sinks = a.sinks != nullptr;  // (wave-uniform)
        const float inv = with_sinks ? Lrow : 1.0f / Lrow;
        const bool none = with_sinks ? Lrow < 0.0f : Lrow == 0.0f;
        const float fill = with_sinks ? 0.0f : __builtin_nanf("");
        const int pr = row_base + rr;  // packed row within the tile
        const int rq = div_R(a, pr);
        const int riq1 = qt * a.QPT + rq;
        const int riq2 = ik2 * a.rk2 + hs * a.R + (pr - rq * a.R);
        f32x4 o4;
#pragma unroll
        for (int j = 0; j < 4; j++) o4[j] = none ? fill : x[j] * inv;
        *(f32x4*)(a.dst + (((int64_t)iq3 * a.NQ + riq1) * a.H + riq2) * D + dq) = o4;
    }
}

}  // namespace fattn
