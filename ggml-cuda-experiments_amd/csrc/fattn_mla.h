// fattn_mla.h -- multi-head latent attention (DeepSeek-V2/V3/R1, Kimi-K2 after
// weight absorption) for gfx950: K rows of 576 f16 (64 RoPE dims + the 512-dim
// latent), V rows of 512 f16 that are -- in llama.cpp's graph -- a view of the
// same cache rows, one kv head, 16 ... 128 query heads.
//
// None of the other kernels can take the shape: the split kernel holds a
// 16-row Q operand and the O accumulators per wave with two waves per SIMD, the
// multi-query kernel stops at 64 heads per kv head, and both read V as a second
// tensor.  Here one workgroup of 4 waves (one per SIMD, up to 512 registers
// each) owns 64 packed (query row x q head) rows of one kv head, 16 per wave,
// and walks its KV chunk in 32-key tiles:
//
//  * all 256 threads copy a tile's K rows (32 x 1152 B = 9 x 16-B pieces per
//    thread) and its 64 mask rows (dword pieces: mask rows are only 4-byte
//    aligned) HBM -> LDS by LDS-DMA; the 16-B chunks of a row are XOR-swizzled
//    on the source side (mla_ksw), so the image serves the row reads of
//    S^T = K.Q^T and the transposed reads of O^T = V^T.P^T alike;
//  * V AS A VIEW OF K (MlaArgs::v_off >= 0): nothing else is loaded -- the V
//    operand is a ds_read_b64_tr_b16 of the K image, v_off bytes into each row;
//    three tiles in the ring (two in flight behind the one being computed).
//    V of its own (VOWN): a second image per tile (32 x 1024 B, the split
//    kernel's f16 V swizzle), two tiles in the ring;
//  * every wave: 36 MFMAs for the scores of its 16 rows against the 32 keys
//    (18 k-steps of 32 dims x 2 key subtiles), online softmax in the log2
//    domain with the deferred max, 32 MFMAs for O^T (512 columns).  The Q
//    operand is 72 VGPRs, O^T 128 accumulator registers.
//
// One workgroup barrier per tile.  Keys past N are set to -inf in the last
// tile (their rows are descriptor zero-fill: a zero score is not -inf).  Waves
// whose 16 rows are all past the tile's rows (H = 16 decode: three of four)
// only copy.  The KV sequence splits over chunks (grid.x) to fill the chip;
// chunk partials (f32 O, (m, l)) merge in a second launch by the LSE rule
// (merge_row_parts at 256 columns, twice per row), where the sink enters.
//
// A Q8_0 / Q4_0 CACHE (V a view of K, whole blocks in):
// the ring holds RAW tiles (32 rows of 18 blocks, by LDS-DMA) and every tile is
// dequantised once, in LDS, into the f16 K image above -- the tile loop then
// runs unchanged over that image, so the result is the f16 form's bit for bit.
// The pipeline is skewed (iteration s converts tile s + 1, then computes tile
// s: still one barrier per tile).  Where no tile has more than one wave's rows
// (H = 16 decode) wave 0 computes and waves 1 - 3 load and convert (SOLO).
#pragma once

#include "fattn_split.h"  // v_operand_f16
#include "fattn_tile.h"

namespace fattn {

constexpr int kMlaDK = 576;   // K row: 64 RoPE dims + the 512-dim latent (either order)
constexpr int kMlaDV = 512;
constexpr int kMlaWaves = 4;
constexpr int kMlaRows = 64;  // packed rows per workgroup (16 per wave)
constexpr int kMlaVOffMax = 128;

template <typename A>
struct MlaArgsT {
    A a;  // SplitArgs, or SplitArgsLse: the kernel fattn_ext_lse launches (fattn_tile.h)
    int v_off;  // view form: byte offset of V's row inside K's row (0 .. 128, a multiple of 16); else 0
    int raw16;  // SOLO form of a quantised cache: contiguous rows on a 16-B aligned plane -- whole tiles land in 16-B pieces
};
using MlaArgs = MlaArgsT<SplitArgs>;

// KT: the cache's type.  F16: the ring holds f16 tiles as they come from HBM.
// Q8_0 / Q4_0 (V a view of K only): the ring holds RAW tiles -- 32 rows of 18
// blocks, landed in dword pieces -- and two f16 images that all 256 threads
// convert them into (mla_convert_tile), in the layout the f16 form loads.
template <bool VOWN, int KT = FATTN_TYPE_F16>
struct MlaCfg {
    static constexpr bool QUANT = KT != FATTN_TYPE_F16;
    static_assert(!QUANT || ((KT == FATTN_TYPE_Q8_0 || KT == FATTN_TYPE_Q4_0) && !VOWN), "");
    static constexpr int NT = kMlaWaves * kWave;
    static constexpr int rowK = kMlaDK * 2, rowV = kMlaDV * 2;
    static constexpr int CPK = rowK / 16, CPV = rowV / 16;  // 16-B chunks per row: 72, 64
    static constexpr int kBytes = kStep * rowK;             // 36,864
    static constexpr int vBytes = VOWN ? kStep * rowV : 0;  // 32,768
    static constexpr int mBytes = kMlaRows * kStep * 2;     // 64 mask rows x 32 f16
    static constexpr int tileBytes = kBytes + vBytes + mBytes;
    static constexpr int nBuf = VOWN ? 2 : 3;
    // quantised cache: a raw row is 612 B (Q8_0) / 324 B (Q4_0); a raw tile's
    // 4896 / 2592 dwords take 20 / 11 dword DMAs of the workgroup, the last one
    // part-filled (its other lanes are requested past the descriptor and write
    // zeros: the slot is padded to whole instructions, 20,480 / 11,264 B)
    static constexpr int blockBytes = QUANT ? TypeInfo<KT>::block_bytes : 0;
    static constexpr int rawRow = kMlaDK / QK * blockBytes;
    static constexpr int rawDw = kStep * rawRow / 4;
    static constexpr int NIR = (rawDw + NT - 1) / NT;
    static constexpr int rawBytes = NIR * NT * 4;
    static constexpr int slotBytes = rawBytes + mBytes;     // raw tile | mask rows: 24,576 / 15,360
    static constexpr int nRaw = 3, nImg = 2;
    static constexpr int ldsBytes = QUANT ? nImg * kBytes + nRaw * slotBytes  // 147,456 / 119,808
                                          : nBuf * tileBytes;                 // 122,880 / 147,456
    static constexpr int NIK = QUANT ? NIR : kBytes / 16 / NT;  // 9 (f16)
    static constexpr int NIV = vBytes / 16 / NT;            // 8
    static constexpr int NIM = mBytes / 4 / NT;             // 4
    static_assert(kBytes % (16 * NT) == 0 && vBytes % (16 * NT) == 0 && mBytes % (4 * NT) == 0, "");
    static_assert(ldsBytes <= 163840, "");
    static constexpr int ni(bool hm) { return NIK + NIV + (hm ? NIM : 0); }
};

// XOR of the 16-B chunk index of K-image row r.  The row stride is 288 dwords
// (32 banks mod 64): even rows start on banks 0-31, odd rows on 32-63, and a
// group of 8 chunks covers one half.  Bijective in (r >> 1) & 7, so the 8 even
// (odd) rows of a 16-row ds_read_b128 group take 8 distinct slots; (x >> 1)
// bijective in (r >> 1) & 3, so the 4 even (odd) rows of a transposed read's
// 32-lane half take 4 distinct chunk PAIRS.
__device__ __forceinline__ int mla_ksw(int r) { return (((r >> 1) & 3) << 1) | ((r >> 3) & 1); }

// The K chunk (8 dims) that lane group g feeds to MFMA k-step b.  Which dims a
// k-step sums is free as long as Q's operand agrees: groups g and g + 1 of one
// ds_read_b128 lane group read chunks 8 apart -- the other bank half -- in the
// first 64 chunks; the last 8 chunks (k-steps 16, 17) have no partner half and
// keep 4 b + g (a 2-way conflict on 2 of 18 reads).
__device__ __forceinline__ int mla_kchunk(int b, int g) {
    return b < 16 ? 16 * (b >> 2) + 8 * (g & 1) + 2 * (b & 3) + (g >> 1) : 64 + 4 * (b - 16) + g;
}

// This lane's LDS byte offsets, tile-relative, so that every read of the tile
// loop is one of a few registers plus an immediate (the swizzles XOR only the
// low bits of a chunk index; the part of the index that counts up in the loop
// sits above them).
//   K operand (A of S^T = K.Q^T), key row 16 t + i16, k-step b:
//     b < 16:  k[t][b & 3] + 256 (b >> 2);   b >= 16:  k2[t][b - 16]
//   V operand (A of O^T = V^T.P^T; v_operand_f16's lane mapping: lane l ->
//   column 16 c + (l & 15), element j = 4 t + r <-> key 16 t + 4 g + r), key row
//   16 t + 4 g + (i16 >> 2), column group c:
//     view of K, vc0 chunks into each row:  v[t][c & 3] + 128 (c >> 2)
//     V's own image (1024-B rows, chunk ^ ((row & 7) << 1)):  v[t][c & 7] + 256 (c >> 3)
template <bool VOWN>
struct MlaLaneOffs {
    int k[2][4], k2[2][2];
    int v[2][VOWN ? 8 : 4];
};
template <bool VOWN>
__device__ __forceinline__ MlaLaneOffs<VOWN> mla_lane_offs(int g, int i16, int vc0) {
    MlaLaneOffs<VOWN> L;
    const int gp = 8 * (g & 1) + (g >> 1);  // mla_kchunk(b, g) = 16 (b >> 2) + (gp | 2 (b & 3)), b < 16
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int row = 16 * t + i16, sw = mla_ksw(row);
#pragma unroll
        for (int bb = 0; bb < 4; bb++) L.k[t][bb] = row * (kMlaDK * 2) + (((gp | (2 * bb)) ^ sw) << 4);
#pragma unroll
        for (int bb = 0; bb < 2; bb++) L.k2[t][bb] = row * (kMlaDK * 2) + ((64 + ((4 * bb + g) ^ sw)) << 4);
        const int q = i16 >> 2, p = i16 & 3;
        const int vr = 16 * t + 4 * g + q;
        if constexpr (VOWN) {
#pragma unroll
            for (int j = 0; j < 8; j++)
                L.v[t][j] = vr * (kMlaDV * 2) + (((2 * j + (p >> 1)) ^ ((vr & 7) << 1)) << 4) + (p & 1) * 8;
        } else {
            // chunk vc0 + (p >> 1) + 2 j <= 15: the XOR stays below 16, 8 (c >> 2) adds above it
#pragma unroll
            for (int j = 0; j < 4; j++)
                L.v[t][j] = vr * (kMlaDK * 2) + (((vc0 + (p >> 1) + 2 * j) ^ mla_ksw(vr)) << 4) + (p & 1) * 8;
        }
    }
    return L;
}

// One raw tile -> the f16 K image.  A group of 8 lanes (l8 = lane & 7) owns CNT
// image slots l8 + 8 i, i = i0 .. i0 + CNT - 1, of one row.  Slot cs holds chunk
// c = cs ^ mla_ksw(row) (8 elements: a quarter of block c >> 2), as the f16
// form's source-side swizzle leaves it; the XOR stays below 8, so the block and
// the quarter move by constants with i.  Values: h(q d), the exact product
// rounded once (kv_stage_f16_block's, the oracle's K operand).
//   reads: a block's qs start 2 mod 4 in even blocks, 0 mod 4 in odd ones
//   (34 / 18-B blocks in rows of whole dwords): three aligned dwords and a byte
//   alignment by the offset's bit 1.  Q4_0: quarters 0 / 1 are the low nibbles
//   of qs[0..7] / qs[8..15], quarters 2 / 3 the high ones.
//   writes: ds_write_b128 goes in groups of 8 contiguous lanes -- one row's
//   128 contiguous bytes, 32 distinct banks: conflict-free.
template <int KT, int CNT>
__device__ __forceinline__ void mla_convert_part(const uint8_t* raw, uint8_t* img, int row, int l8, int i0) {
    constexpr int BB = TypeInfo<KT>::block_bytes, RR = kMlaDK / QK * BB;
    const int c0 = l8 ^ mla_ksw(row);
    const int sub = c0 & 3;
    const uint32_t b0 = row * RR + (c0 >> 2) * BB + 2 * BB * i0;             // the block of i = i0
    const uint32_t q0 = b0 + 2 + 8 * (KT == FATTN_TYPE_Q8_0 ? sub : sub & 1);  // its 8 code bytes
    const uint32_t qa = q0 & ~3u, sh = q0 & 2u;                              // (2 BB is 0 mod 4: the same for every i)
    uint8_t* out = img + row * (kMlaDK * 2) + l8 * 16 + 128 * i0;
#pragma unroll
    for (int i = 0; i < CNT; i++) {
        const uint32_t dbits = *(const uint16_t*)(raw + b0 + 2 * BB * i);
        const uint32_t w0 = *(const uint32_t*)(raw + qa + 2 * BB * i);
        const uint32_t w1 = *(const uint32_t*)(raw + qa + 2 * BB * i + 4);
        const uint32_t w2 = *(const uint32_t*)(raw + qa + 2 * BB * i + 8);
        uint32_t x0 = alignbyte(w1, w0, sh), x1 = alignbyte(w2, w1, sh);
        const f16x2 d2 = bcast_h(dbits);
        f16x2 h0, h1, h2, h3;
        if constexpr (KT == FATTN_TYPE_Q8_0) {
            i8x4_to_h2x2(x0, h0, h1);
            i8x4_to_h2x2(x1, h2, h3);
        } else {
            const uint32_t ns = 2 * (sub & 2);  // 0: low nibbles, 4: high
            u4x4_to_h2x2((x0 >> ns) & 0x0F0F0F0Fu, h0, h1);
            u4x4_to_h2x2((x1 >> ns) & 0x0F0F0F0Fu, h2, h3);
        }
        const u32x4 r = {as_u32(h0 * d2), as_u32(h1 * d2), as_u32(h2 * d2), as_u32(h3 * d2)};
        *(u32x4*)(out + 128 * i) = r;
    }
}
// ... by all 256 threads (thread t: row t >> 3, all nine slots), or -- SOLO, a
// tile whose rows fill one wave (H = 16 decode): wave 0 computes and waves 1 - 3
// convert -- by the 192 threads u = t - 64: rows 0 .. 23 as above, then three
// slots each of rows 24 .. 31 (12 chunks per thread).
template <int KT, bool SOLO>
__device__ __forceinline__ void mla_convert_tile(const uint8_t* raw, uint8_t* img, int tid) {
    constexpr int NS = kMlaDK / 64;  // 9
    if constexpr (!SOLO) return mla_convert_part<KT, NS>(raw, img, tid >> 3, tid & 7, 0);
    if (tid < kWave) return;
    const int g8 = (tid - kWave) >> 3;  // 0 .. 23
    mla_convert_part<KT, NS>(raw, img, g8, tid & 7, 0);
    const int third = (g8 * 11) >> 5;   // g8 / 3
    mla_convert_part<KT, NS / 3>(raw, img, 24 + third, tid & 7, 3 * (g8 - 3 * third));
}

__device__ __forceinline__ f16x8 mla_tr_pair(const uint8_t* lo_p, const uint8_t* hi_p) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo_p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi_p);
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 r = {l2.x, l2.y, h2.x, h2.y};
    return __builtin_bit_cast(f16x8, r);
}

template <int N>
__device__ __forceinline__ void mla_wait_tiles(int pending) {
    if (pending <= 0) wait_vmcnt_c<0>();
    else wait_vmcnt_c<N>();
}

// SOLO (quantised cache only; the launcher's choice): no tile of the launch has
// more than one wave's 16 rows (H = 16 decode), so wave 0 computes and waves
// 1 - 3 load and convert -- the conversion leaves the computing wave's chain.
template <bool VOWN, bool HM, int KT = FATTN_TYPE_F16, bool SOLO = false, typename A = SplitArgs>
__global__ __launch_bounds__(kMlaWaves* kWave, 1) void fattn_mla_kernel(const MlaArgsT<A> ma) {
    using C = MlaCfg<VOWN, KT>;
    constexpr bool QUANT = C::QUANT;
    static_assert(QUANT || !SOLO, "");
    const A& a = ma.a;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NB = kMlaDK / QK;   // 18 k-steps
    constexpr int NC = kMlaDV / 16;   // 32 column groups
    constexpr int KB = 3, VB = 8;     // k-steps / column groups per batch of LDS reads (12 b128 / 16 tr_b64 in flight)
    static_assert(NB % KB == 0 && NC % VB == 0, "");
    constexpr int NI = C::ni(HM);
    constexpr int PRE = C::nBuf - 1;  // tiles issued ahead of the one being computed (f16)
    constexpr float kNegInf = -__builtin_inff();
    constexpr float kDeferLog2 = 8.0f;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int i16 = lane & 15;

    // Two row tiles per kv head (rk2 = 128) read the same K rows: with
    // SplitArgs::xcd_group the workgroups are renumbered so that the pair sits
    // on one XCD (hardware deals consecutive workgroup ids round-robin over the
    // 8 XCDs), 8 ids apart -- dispatched together, the second read of a row is
    // an L2 hit.  Linear id L -> (pair P, head subgroup): P = L % 8 + 8 (L / 16),
    // hs = (L / 8) % 2; the grid's size is a multiple of 16 (size_mla).
    int chunk = blockIdx.x, y = blockIdx.y, iq3 = blockIdx.z;
    if (a.xcd_group) {
        const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        int pr = (lin & 7) + 8 * (lin >> 4);
        const int yh = gridDim.y >> 1;  // y without the head subgroup: qt + n_qt * ik2
        chunk = pr % (int)gridDim.x;
        pr /= (int)gridDim.x;
        const int yy = pr % yh;
        iq3 = pr / yh;
        y = yy % a.n_qt + a.n_qt * (((lin >> 3) & 1) + 2 * (yy / a.n_qt));
    }
    int qt, hs, ik2, ik3;
    tile_decode<true>(a, y, iq3, qt, hs, ik2, ik3);
    const int nvalid = tile_rows(a, qt, hs);       // the tile's rows: a prefix of its 64
    const bool active = wave * kRows < nvalid;     // (wave-uniform) this wave has rows to compute

    // this lane's packed row p -> (query row, q head)
    const int p = kRows * wave + i16;
    const int rq = div_R(a, p);
    const int iq1 = qt * a.QPT + rq;
    const int iq2 = ik2 * a.rk2 + hs * a.R + (p - rq * a.R);
    const bool row_ok = p < nvalid;

    const int c_lo = chunk * a.chunk_len;
    const int c_hi = min(a.N, c_lo + a.chunk_len);
    const int ntiles = (c_hi - c_lo + kStep - 1) / kStep;

    const StepSrc rs = kv_sources<HM>(a, ik2, ik3, iq3, VOWN ? a.v_span : 0);

    // ---- Q^T operands (B of S^T = K.Q^T), rounded to f16 like src/utils.h:10;
    // k-step b of lane group g holds the dims of chunk mla_kchunk(b, g)
    f16x8 qop[NB];
    if (active) {
        const auto qs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.q + (int64_t)iq3 * a.q_nb3), 0,
                                                          a.q_span, 0x00020000);
        const uint32_t qoff = row_ok ? (uint32_t)iq1 * (uint32_t)a.q_nb1 + (uint32_t)iq2 * (uint32_t)a.q_nb2 : a.q_span;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const uint32_t o = row_ok ? qoff + 32 * mla_kchunk(b, g) : qoff;
            const f32x4 x0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(qs, o, 0, 0));
            const f32x4 x1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(qs, o + 16, 0, 0));
            f16x8 h;
            h.s0 = (f16)x0.x; h.s1 = (f16)x0.y; h.s2 = (f16)x0.z; h.s3 = (f16)x0.w;
            h.s4 = (f16)x1.x; h.s5 = (f16)x1.y; h.s6 = (f16)x1.z; h.s7 = (f16)x1.w;
            qop[b] = h;
        }
    } else {
#pragma unroll
        for (int b = 0; b < NB; b++) qop[b] = f16x8{};
    }

    // ---- this lane's mask pieces: instruction i stages packed rows 16 i ..
    // 16 i + 15, 16 dwords each; row (query row, head) reads its own head's
    // plane; rows the tile does not have stay outside the descriptor
    uint32_t moff[C::NIM];
    if constexpr (HM) {
#pragma unroll
        for (int i = 0; i < C::NIM; i++) {
            const int pr = 16 * i + (tid >> 4);
            const int mq = div_R(a, pr);
            const int mh = ik2 * a.rk2 + hs * a.R + (pr - mq * a.R);
            moff[i] = pr < nvalid ? (uint32_t)(qt * a.QPT + mq) * (uint32_t)a.m_nb1 + mask_head_off(a, mh) + (tid & 15) * 4
                                  : 0xFFFFFFFFu;
        }
    }

    // Copy tile [n0, n0 + 32) into `buf`: K image | V image (VOWN) | mask rows.
    // Lane-linear LDS-DMA: LDS slot (row, cs) takes the row's chunk cs ^ swizzle.
    // Rows from c_hi on are requested past the descriptor: zeros, no traffic.
    auto issue = [&](int n0, uint8_t* buf) {
        const uint32_t lb = __builtin_amdgcn_readfirstlane(lds_addr(buf) + wave * kWave * 16);
#pragma unroll
        for (int i = 0; i < C::NIK; i++) {
            const int pc = i * C::NT + tid;
            const int row = pc / C::CPK, cs = pc - row * C::CPK;
            const uint32_t off = n0 + row < c_hi
                                     ? (uint32_t)(n0 + row) * (uint32_t)a.k_nb1 + (uint32_t)((cs ^ mla_ksw(row)) * 16)
                                     : a.k_span;
            dma<16>(rs.k, lb + i * C::NT * 16, off);
        }
        if constexpr (VOWN) {
#pragma unroll
            for (int i = 0; i < C::NIV; i++) {
                const int pc = i * C::NT + tid;
                const int row = pc / C::CPV, cs = pc - row * C::CPV;
                const uint32_t off = n0 + row < c_hi
                                         ? (uint32_t)(n0 + row) * (uint32_t)a.v_nb1 + (uint32_t)((cs ^ ((row & 7) << 1)) * 16)
                                         : a.v_span;
                dma<16>(rs.v, lb + C::kBytes + i * C::NT * 16, off);
            }
        }
        if constexpr (HM) {
            const uint32_t lm = __builtin_amdgcn_readfirstlane(lds_addr(buf) + C::kBytes + C::vBytes + wave * kWave * 4);
#pragma unroll
            for (int i = 0; i < C::NIM; i++)
                dma<4>(rs.m, lm + i * C::NT * 4, moff[i] == 0xFFFFFFFFu ? a.m_span_h : moff[i] + (uint32_t)n0 * 2);
        }
    };
    auto buf_of = [&](int s) { return smem + (s % C::nBuf) * C::tileBytes; };
    // Quantised cache: raw tile [n0, n0 + 32) | mask rows into a raw slot.  Dword
    // w of the tile is dword w % (rawRow / 4) of row w / (rawRow / 4); dwords
    // past the tile (the last instruction's tail) and rows from c_hi on are
    // requested past the descriptor.
    // SOLO: waves 1 - 3 issue all of it, wave-sized pieces dealt round-robin
    // (piece j: dwords 64 j .. 64 j + 63)
    constexpr bool solo = SOLO;
    auto raw_off = [&](int w, int n0) -> uint32_t {
        constexpr int RD = QUANT ? C::rawRow / 4 : 1;
        const int row = w / RD, col = w - row * RD;
        return w < C::rawDw && n0 + row < c_hi ? (uint32_t)(n0 + row) * (uint32_t)a.k_nb1 + (uint32_t)(col * 4) : a.k_span;
    };
    auto issue_raw = [&](int n0, uint8_t* slot) {
        if constexpr (solo) {
            if (wave == 0) return;
            const int h = wave - 1;
            // pieces: 80 / 44 of the raw tile; of the mask rows only wave 0's 16 (4 pieces of 4 rows)
            constexpr int NP = C::NIR * kMlaWaves, NPM = kRows / 4;
            // Contiguous rows on a 16-B aligned plane (MlaArgs::raw16): a whole tile is
            // one 16-B aligned run of 32 x 612 = 16 x 1224 (Q4_0: 16 x 648) bytes and
            // lands in 20 (11) wave pieces of 16 B a lane -- a quarter of the requests.
            // Not the part-filled last tile of N: its rows from N on must read as
            // zeros, and a 16-B piece can straddle the end of a 612-B row.
            constexpr int NP16 = (kStep * C::rawRow / 16 + kWave - 1) / kWave;
            if (ma.raw16 && n0 + kStep <= c_hi) {
#pragma unroll
                for (int jj = 0; jj < (NP16 + 2) / 3; jj++) {
                    const int j = 3 * jj + h;
                    const int pc = j * kWave + lane;
                    if (j < NP16)
                        dma<16>(rs.k, lds_addr(slot) + j * kWave * 16,
                                pc < kStep * C::rawRow / 16 ? (uint32_t)n0 * (uint32_t)C::rawRow + (uint32_t)pc * 16 : a.k_span);
                }
            } else {
                // (only a chunk's last tile, or every tile of a cache that does not
                // qualify: the offsets are redone per tile, not kept in registers)
                int lane_o = lane;
                if (ma.raw16) asm volatile("" : "+v"(lane_o));
#pragma unroll
                for (int jj = 0; jj < (NP + 2) / 3; jj++) {
                    const int j = 3 * jj + h;
                    if (j < NP) dma<4>(rs.k, lds_addr(slot) + j * kWave * 4, raw_off(j * kWave + lane_o, n0));
                }
            }
            const int lane_o = lane;
            if constexpr (HM) {
#pragma unroll
                for (int jj = 0; jj < (NPM + 2) / 3; jj++) {
                    const int j = 3 * jj + h;  // piece j: 4 packed rows of 16 dwords (moff's rows, re-dealt)
                    if (j < NPM) {
                        const int pr = 4 * j + (lane_o >> 4);
                        const int mq = div_R(a, pr);
                        const int mh = ik2 * a.rk2 + hs * a.R + (pr - mq * a.R);
                        const uint32_t mo = pr < nvalid ? (uint32_t)(qt * a.QPT + mq) * (uint32_t)a.m_nb1 + mask_head_off(a, mh) +
                                                              (lane_o & 15) * 4 + (uint32_t)n0 * 2
                                                        : a.m_span_h;
                        dma<4>(rs.m, lds_addr(slot) + C::rawBytes + j * kWave * 4, mo);
                    }
                }
            }
            return;
        }
        const uint32_t lb = __builtin_amdgcn_readfirstlane(lds_addr(slot) + wave * kWave * 4);
#pragma unroll
        for (int i = 0; i < C::NIR; i++) dma<4>(rs.k, lb + i * C::NT * 4, raw_off(i * C::NT + tid, n0));
        if constexpr (HM) {
            const uint32_t lm = __builtin_amdgcn_readfirstlane(lds_addr(slot) + C::rawBytes + wave * kWave * 4);
#pragma unroll
            for (int i = 0; i < C::NIM; i++)
                dma<4>(rs.m, lm + i * C::NT * 4, moff[i] == 0xFFFFFFFFu ? a.m_span_h : moff[i] + (uint32_t)n0 * 2);
        }
    };
    auto img_of = [&](int s) { return smem + (s & 1) * C::kBytes; };
    auto raw_of = [&](int s) { return smem + C::nImg * C::kBytes + (s % C::nRaw) * C::slotBytes; };

    // (Q's loads are compiler-tracked and converted above: they have landed)
    if constexpr (QUANT) {
        // A SKEWED pipeline, one barrier per tile: iteration s converts raw tile
        // s + 1 into the image tile s - 1 was computed from, then computes tile s.
        // Prologue: raw tiles 0 and 1 in flight, tile 0 converted.
        // (SOLO: a loading wave has issued 26 or 27 (14 / 15) + 1 or 2 mask pieces
        // of tile 1; waiting down to the smallest count is safe for all three)
        // (16-B pieces: 6 or 7 (3 or 4) of them; the smaller count is safe for both forms)
        constexpr int NI_SOLO = (kStep * C::rawRow / 16 + kWave - 1) / kWave / 3 + (HM ? kRows / 4 / 3 : 0);
        issue_raw(c_lo, raw_of(0));
        if (ntiles > 1) {
            issue_raw(c_lo + kStep, raw_of(1));
            if constexpr (solo) wait_vmcnt_c<NI_SOLO>();
            else wait_vmcnt_c<NI>();
        } else {
            wait_vmcnt_c<0>();
        }
        __syncthreads();
        mla_convert_tile<KT, SOLO>(raw_of(0), img_of(0), tid);
    } else {
        for (int s = 0; s < PRE && s < ntiles; s++) issue(c_lo + s * kStep, buf_of(s));
    }

    float m_run = kNegInf, l_run = 0.0f;
    f32x4 o[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) o[c] = f32x4{0, 0, 0, 0};
    const float log2e = 1.4426950408889634f;
    const MlaLaneOffs<VOWN> L = mla_lane_offs<VOWN>(g, i16, ma.v_off >> 4);

    // One barrier per tile: past the barrier of iteration s every thread's
    // pieces of tile s have landed and every wave is done with tile s - 1,
    // whose buffer takes tile s + PRE.
    // Quantised cache: past the barrier of iteration s every thread's pieces of
    // raw tile s + 1 have landed (the only DMAs in flight), image s is whole
    // (written in iteration s - 1, or the prologue) and every wave is done with
    // tile s - 1: its image takes tile s + 1, and its raw slot -- whose mask rows
    // tile s - 1 read to the end -- takes raw tile s + 2.
    for (int s = 0; s < ntiles; s++) {
        if constexpr (QUANT) {
            wait_vmcnt_c<0>();
            __syncthreads();
            if (s + 2 < ntiles) issue_raw(c_lo + (s + 2) * kStep, raw_of(s + 2));
            if (s + 1 < ntiles) mla_convert_tile<KT, SOLO>(raw_of(s + 1), img_of(s + 1), tid);
        } else {
            mla_wait_tiles<(PRE - 1) * NI>(min(PRE - 1, ntiles - 1 - s));
            __syncthreads();
            if (s + PRE < ntiles) issue(c_lo + (s + PRE) * kStep, buf_of(s + PRE));
        }
        if (!active) continue;
        const uint8_t* kb = QUANT ? img_of(s) : buf_of(s);
        const uint8_t* vb = kb + C::kBytes;
        const uint8_t* mb = QUANT ? raw_of(s) + C::rawBytes : kb + C::kBytes + C::vBytes;
        const int n0 = c_lo + s * kStep;

        // -- S^T = K.Q^T for the two 16-key subtiles
        // The operands are read in batches, each issued one batch ahead of the
        // MFMAs that take it (sched_barrier keeps hipcc from sinking a read to
        // its use: left alone it emitted read, wait lgkmcnt(0), MFMA 36 times
        // over, one exposed LDS latency per MFMA)
        f32x4 st[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
        {
            f16x8 ka[2][KB][2];
            auto kload = [&](int b0, f16x8(&dst)[KB][2]) {
#pragma unroll
                for (int bb = 0; bb < KB; bb++) {
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const int b = b0 + bb;
                        const int ko = b < 16 ? L.k[t][b & 3] + 256 * (b >> 2) : L.k2[t][b - 16];
                        dst[bb][t] = *(const f16x8*)(kb + ko);
                    }
                }
            };
            kload(0, ka[0]);
#pragma unroll
            for (int i = 0; i < NB / KB; i++) {
                if (i + 1 < NB / KB) kload((i + 1) * KB, ka[(i + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int bb = 0; bb < KB; bb++) {
#pragma unroll
                    for (int t = 0; t < 2; t++) st[t] = mfma16(ka[i & 1][bb][t], qop[i * KB + bb], st[t]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // (the first V batch does not wait for P: its reads fly under the softmax)
        f16x8 va[2][VB];
        auto vload = [&](int c0, f16x8(&dst)[VB]) {
#pragma unroll
            for (int cc = 0; cc < VB; cc++) {
                const int c = c0 + cc;
                if constexpr (VOWN) dst[cc] = mla_tr_pair(vb + L.v[0][c & 7] + 256 * (c >> 3), vb + L.v[1][c & 7] + 256 * (c >> 3));
                else dst[cc] = mla_tr_pair(kb + L.v[0][c & 3] + 128 * (c >> 2), kb + L.v[1][c & 3] + 128 * (c >> 2));
            }
        };
        vload(0, va[0]);
        __builtin_amdgcn_sched_barrier(0);
        // -- scores in log2 units: lane holds keys n0 + 16 t + 4 g + r of its row
        float sv[8];
        {
            float mk[8];
#pragma unroll
            for (int j = 0; j < 8; j++) mk[j] = 0.0f;
            if constexpr (HM) {
                const uint8_t* mr = mb + (kRows * wave + i16) * (kStep * 2) + 8 * g;
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const u32x2 w2 = *(const u32x2*)(mr + 32 * t);
                    const f16x2 m01 = as_h2(w2.x), m23 = as_h2(w2.y);
                    mk[4 * t + 0] = (float)m01.x; mk[4 * t + 1] = (float)m01.y;
                    mk[4 * t + 2] = (float)m23.x; mk[4 * t + 3] = (float)m23.y;
                }
            }
            if (a.xf.live) {  // max_bias / logit_softcap (wave-uniform): the slope of the lane's own q head
                const float slope = xf_slope(a.xf, iq2);
#pragma unroll
                for (int j = 0; j < 8; j++) sv[j] = xf_score(a.xf, a.scale, st[j >> 2][j & 3], mk[j], slope) * log2e;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) sv[j] = st[j >> 2][j & 3] * a.scale_log2 + mk[j] * log2e;
            }
            // keys past the chunk's end (the last tile of N): zero-filled rows, no score
            if (n0 + kStep > c_hi) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (n0 + 16 * (j >> 2) + 4 * g + (j & 3) >= c_hi) sv[j] = kNegInf;
            }
        }
        float tmax = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
        tmax = grp4_max(tmax);
        // deferred max (fattn_mq.h): the reference max moves only when a tile's
        // max passes it by more than kDeferLog2; O and l are scaled together
        if (__builtin_amdgcn_ballot_w64(tmax > m_run + kDeferLog2)) {
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = (m_new == kNegInf) ? 1.0f : __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int c = 0; c < NC; c++) o[c] *= alpha;
            m_run = m_new;
        }
        const float m_use = (m_run == kNegInf) ? 0.0f : m_run;
        float pv[8];
#pragma unroll
        for (int j = 0; j < 8; j++) pv[j] = __builtin_amdgcn_exp2f(sv[j] - m_use);
        l_run += ((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]));
        f16x8 pb;
        pb.s0 = (f16)pv[0]; pb.s1 = (f16)pv[1]; pb.s2 = (f16)pv[2]; pb.s3 = (f16)pv[3];
        pb.s4 = (f16)pv[4]; pb.s5 = (f16)pv[5]; pb.s6 = (f16)pv[6]; pb.s7 = (f16)pv[7];
        // -- O^T += V^T.P^T
#pragma unroll
        for (int i = 0; i < NC / VB; i++) {
            if (i + 1 < NC / VB) vload((i + 1) * VB, va[(i + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cc = 0; cc < VB; cc++) o[i * VB + cc] = mfma16(va[i & 1][cc], pb, o[i * VB + cc]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (!active) return;
    const float l_tot = grp4_sum(l_run);

    if (a.n_chunks == 1) {
        if (!row_ok) return;
        const int64_t row = ((int64_t)iq3 * a.NQ + iq1) * a.H + iq2;
        float* out = a.dst + row * kMlaDV + 4 * g;
        float sraw = kNegInf;  // (the row's raw sink: a term of its log-sum-exp below)
        if (a.sinks) {  // (wave-uniform; m_run is the row's reference max in log2 units)
            bool dead;
            sraw = a.sinks[iq2];
            const float inv = sink_inv(m_run, l_tot, sraw, dead);
#pragma unroll
            for (int c = 0; c < NC; c++) *(f32x4*)(out + 16 * c) = sink_row(o[c], inv, dead);
        } else {
            const float inv = 1.0f / l_tot;  // fully masked row -> NaN like the reference
#pragma unroll
            for (int c = 0; c < NC; c++) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = l_tot == 0.0f ? __builtin_nanf("") : o[c][r] * inv;
                *(f32x4*)(out + 16 * c) = v;
            }
        }
        // the row's log-sum-exp, behind its dst stores: the O registers are dead here
        if (float* const lse = lse_of(a)) {  // (wave-uniform)
            if (g == 0) lse[row] = row_lse(m_run, l_tot, sraw, row_dead(m_run, l_tot));
        }
        return;
    }
    // ---- several chunks: the wave's 16 rows as f32 partials [tile][chunk][64 rows];
    // the kernel boundary orders these stores before the merge launch's loads
    const int64_t tile = (int64_t)iq3 * gridDim.y + y;
    const int64_t slot = (tile * a.n_chunks + chunk) * kMlaRows + p;
#pragma unroll
    for (int c = 0; c < NC; c++) *(f32x4*)(a.ws_o + slot * kMlaDV + 16 * c + 4 * g) = o[c];
    if (g == 0) *(f32x2*)(a.ws_ml + 2 * slot) = f32x2{m_run, l_tot};
}

// the second-launch merge of a split plan (fattn_chunk_merge_kernel,
// fattn_tile.h, at D = kMlaDV: two 256-column parts per row): 64-row tiles with
// head subgroups, f32 partials read with plain loads (the kernel boundary made
// them visible), at least 4 load slots per lane
struct MlaMergeGeom : MergeGeomBase {
    static constexpr int rows = kMlaRows;
    static constexpr bool hsub = true;
    static constexpr bool sc1 = false;
    static constexpr bool f16 = false;
    static constexpr int min_kit = 4;
};

}  // namespace fattn
