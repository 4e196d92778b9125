// fattn_plan.h -- the launch planner (host only; included by fattn_api.hip).
//
// make_plan validates the ggml views, picks the kernel (head dim x K type x V
// type x addressing granule), sizes the split-KV grid for the device's CUs and
// lays out the workspace.  It is a pure function of the params, a snapshot of
// the planner overrides (Options) and the CU count: no HIP call, no global read.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "fattn_launch.h"

namespace fattn {

// ---------------------------------------------------------------- options
// One row per fattn_set_option override (include/fattn_debug.h): its id, its
// default and its legal values -- 0 (every option's "auto" / "off") or lo..hi,
// or, where the range has holes, the values of `set`.  Ids of removed
// experiments (7-9, 14-18, 23, 27) have no row and are rejected.
struct OptionRow {
    int id, def, lo, hi;
    uint64_t set;  // bit v: v is legal (0 = the lo..hi rule)
    bool flag;     // any value is legal, stored as value != 0
    bool legal(int v) const {
        if (flag) return true;
        if (set) return v >= 0 && v < 64 && (set >> v & 1);
        return v == 0 || (v >= lo && v <= hi);
    }
    int stored(int v) const { return flag ? v != 0 : v; }
};
constexpr OptionRow opt_range(int id, int lo, int hi, int def = 0) { return {id, def, lo, hi, 0, false}; }
constexpr OptionRow opt_among(int id, std::initializer_list<int> vs, int def = 0) {
    uint64_t set = 0;
    for (int v : vs) set |= (uint64_t)1 << v;
    return {id, def, 0, 0, set, false};
}
constexpr OptionRow opt_flag(int id) { return {id, 0, 0, 0, 0, true}; }

constexpr OptionRow kOptionTable[] = {
    opt_among(FATTN_OPT_MQ_ROWS_PER_WAVE, {0, 16, 32}),
    opt_flag(FATTN_OPT_MQ_DISABLE),
    opt_range(FATTN_OPT_SPLIT_STEPS, 1, 64),
    opt_range(FATTN_OPT_SPLIT_INFLIGHT, 1, 4),
    opt_range(FATTN_OPT_PF, 1, 2),                     // 0 auto, 1 never, 2 whenever eligible
    opt_among(FATTN_OPT_PF_STAGGER, {0, 2, 4, 6}, 2),  // (bit 0: removed)
    opt_range(FATTN_OPT_SPLIT_WAVE_MERGE, 1, 1),  // 1: one-row split tiles merge through LDS + combine_tile as other tiles
    opt_range(FATTN_OPT_SPLIT_PRIO, 1, 2),
    opt_range(FATTN_OPT_PF_SKIP, 1, 1),           // 1: masked prefill without the live-block pre-pass
    opt_range(FATTN_OPT_MQ_MIN_ROWS, 32, INT_MAX),  // 0: kMqMinRowsDefault; a given value also lifts the `wide` gate
    opt_among(FATTN_OPT_SPLIT_WAVES, {0, 4, 8, 16}),
    opt_range(FATTN_OPT_SPLIT_SKIP, 1, 1),        // 1: the split kernel loads and computes every step
    opt_range(FATTN_OPT_SPLIT_MERGE, 1, 1),       // 1: multi-row split tiles merge in the last-arriving workgroup
    opt_range(FATTN_OPT_BD, 1, 3),                // 0 auto, 1 never, 2 / 3 whenever eligible
    opt_range(FATTN_OPT_MERGE_IN_KERNEL, 1, 1),
    opt_range(FATTN_OPT_BD_XCD, 1, 2),            // 0 auto (on), 1 off, 2 on
    opt_range(FATTN_OPT_SPLIT_XCD, 1, 2),
    opt_range(FATTN_OPT_PF_STAGE, 1, 2),          // 0 auto (staged to f16), 1 in-kernel dequantisation, 2 staged
    // 2, 3: round 5's unpipelined one-wave-per-SIMD forms, removed (slower)
    opt_among(FATTN_OPT_PF_FORM, {0, 1, 4, 5, 6}),
    opt_range(FATTN_OPT_SPLIT_LOADERS, 1, 2),
    opt_range(FATTN_OPT_MERGE_PLAIN, 1, 2),       // 0 auto (sc1 loads), 1 sc1, 2 plain loads
    opt_range(FATTN_OPT_PART_F16, 1, 2),          // 0 auto (f16 where supported), 1 f32, 2 f16
    opt_range(FATTN_OPT_GQA_UNPACK, 1, 2),        // 0 auto (packed), 1 packed, 2 one q head per tile
};
constexpr int kOptionSlots = 34;  // option ids index the value arrays directly

inline const OptionRow* find_option(int id) {
    for (const OptionRow& r : kOptionTable)
        if (r.id == id) return &r;
    return nullptr;
}

// The planner's view of the overrides: a plain copy, taken once per call, so
// one plan is sized under one setting whatever other threads set meanwhile.
struct Options {
    int v[kOptionSlots] = {};
    Options() {
        for (const OptionRow& r : kOptionTable) v[r.id] = r.def;
    }
    int operator[](int id) const { return v[id]; }
};

constexpr int kMqMinRowsDefault = 64;  // multi-query kernel from this many packed rows per kv head

// ---------------------------------------------------------------- LDS sizes
constexpr int kLdsPerCU = 163840;

// LDS bytes of one workgroup of `kern` at compile-time (K type, V type, D);
// 0 exactly when there is no such kernel (has_kernel).  Split kernel: `waves`
// waves with `nbuf` steps in flight each (a wave's bytes are this / waves; the
// loader form adds its flags).
template <int KT, int VT, int D>
int lds_bytes_of(Kernel kern, int waves, int nbuf) {
    switch (kern) {
        case Kernel::Split:
        case Kernel::SplitLd:
            if constexpr (has_kernel(Kernel::Split, KT, VT, D)) {
                if (kern == Kernel::SplitLd && !split_ld_ok(KT, VT, D)) break;
                using C = SplitCfg<KT, VT, D>;
                const int w = std::max((nbuf * C::stepBytes + C::vscBytes + 15) / 16 * 16, (int)C::mergeBytes);
                return waves * w + (kern == Kernel::SplitLd ? kSplitLdFlagBytes : 0);
            }
            break;
        case Kernel::Mq:  // D = 256: 64-row workgroups only (256 rows' mask tiles do not fit beside the D = 256 images)
            if constexpr (has_kernel(Kernel::Mq, KT, VT, D)) {
                if constexpr (D != 256) {
                    if (waves == 8) return MQCfg<KT, D, 8, 32>::ldsBytes;
                }
                return MQCfg<KT, D, 4, 16>::ldsBytes;
            }
            break;
        case Kernel::Pf:
            if constexpr (has_kernel(Kernel::Pf, KT, VT, D)) return PfCfg<KT, D>::ldsBytes;
            break;
        case Kernel::Pf4:
            if constexpr (has_kernel(Kernel::Pf4, KT, VT, D)) return Pf4Cfg<D>::ldsBytes;
            break;
        case Kernel::Bd:
            if constexpr (has_kernel(Kernel::Bd, KT, VT, D)) return BdCfg<KT, D>::ldsBytes;
            break;
        case Kernel::Bdp:
            if constexpr (has_kernel(Kernel::Bdp, KT, VT, D)) return BdpCfg<KT, D>::ldsBytes;
            break;
        case Kernel::Mla: break;  // (size_mla: MlaCfg, no head dim of this table)
    }
    return 0;
}

// the one dispatch from the plan's runtime (K type, V type, D) to the kernels' constants
inline int lds_bytes(Kernel kern, int kt, int vt, int D, int waves, int nbuf = 0) {
    return visit(CacheTypes(), kt, 0, [&](auto k) {
        return visit(VTypes(), vt, 0, [&](auto v) {
            return visit(HeadDims(), D, 0, [&](auto d) {
                return lds_bytes_of<decltype(k)::value, decltype(v)::value, decltype(d)::value>(kern, waves, nbuf);
            });
        });
    });
}

// ---------------------------------------------------------------- helpers
// Tile packing: R q heads of a kv head x QPT query rows fill a tile of `rows`
// packed rows; a kv head's rk2 heads take n_hsub tiles, the NQ query rows n_qt.
inline void pack_tiles(SplitArgs& a, int rows, int R, int64_t NQ) {
    a.R = R;
    a.R_inv = 1.0f / (float)R;
    a.QPT = rows / R;
    a.n_hsub = (a.rk2 + R - 1) / R;
    a.n_qt = (int)((NQ + a.QPT - 1) / a.QPT);
}

// Workspace of a split-KV plan: [arrival words, one 256-B line per tile][(m, l)
// pair per partial row, padded to 256 B][O per partial row, D floats].  No
// zeroing needed: each launch epoch-stamps its arrival words.
inline void layout_partials(Plan& pl, size_t tiles, size_t parts, bool arrival = true) {
    pl.cnt_bytes = arrival ? tiles * kCntStride * sizeof(uint32_t) : 0;
    pl.ml_bytes = (parts * 2 * sizeof(float) + 255) / 256 * 256;
    pl.ws_bytes = pl.cnt_bytes + pl.ml_bytes + parts * pl.D * 4;
}

inline int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// combine_tile limits: one (chunk, row) pair per thread for the (m, l) loads
inline bool combine_ok(int64_t nch, int rv) { return nch <= 64 && next_pow2((int)nch) * rv <= 256; }

// f16 chunk partials (SplitArgs::part_f16) for the second-launch merges of the
// split kernel's multi-row tiles and the batched-decode kernels: not at D = 64
// (merge_row_parts_h), not with the in-kernel merges
inline bool part_f16_ok(const Options& o, int merge_launch, int D) {
    return merge_launch == 1 && D != 64 && o[FATTN_OPT_PART_F16] != 1;
}

// ---------------------------------------------------------------- validation
// What validation learns about the views, for the steps after it
struct Views {
    int64_t D, NQ, H, S, N, Hkv, Skv;
    int64_t n_head_total;
    bool mixed, v_trans, g16, has_mask;
    bool mla = false;      // K dim 576 / V dim 512 (check_views_mla); D is K's
    int64_t mla_v_off = -1;  // ... V is a view of K, this many bytes into each row; -1: V of its own
    int64_t m_ne2 = 1, m_ne3 = 1, m_nb2 = 0, m_nb3 = 0;  // mask planes
    int64_t k_span, v_span, m_span, m_span_h, q_span;    // byte spans addressed through the 32-bit buffer descriptors
};
constexpr int64_t kSpanMax = (int64_t)0xFFFFFFF0;

// The span of a row-strided K / V view with its N rows rounded up to whole key
// tiles.  A kernel that fetches whole tiles forms the offset (n0 + row) * nb[1]
// of the rows from N to the end of the last tile like any other and counts on
// them to fall past the descriptor (zeros, no traffic).  They do while the
// offset does not wrap in 32 bits: with rows tens of MiB apart, row N + 1 of a
// view whose span is near the limit lands back INSIDE the descriptor, and
// whatever bytes lie there reach the K and V tiles (a NaN among them survives
// the zero probability: 0 * NaN).  make_plan therefore holds this span, not
// the view's own, to kSpanMax for the split kernel -- the one kernel that uses
// such rows unguarded (the MLA kernel guards them, the batched-decode kernels
// skip their 32-key quarters, the others take whole tiles only).
inline int64_t tile_span(int64_t span, int64_t nb1, int64_t N, int64_t tile) {
    return span + ((N + tile - 1) / tile * tile - N) * nb1;
}

// ggml's op_params[1], [2] and the global head numbering of the slopes
inline int check_scalars(const fattn_params* p, Views& w, int64_t H) {
    if (!std::isfinite(p->max_bias) || p->max_bias < 0.0f) return FATTN_ERR_INVALID_ARG;
    if (!std::isfinite(p->logit_softcap) || p->logit_softcap < 0.0f) return FATTN_ERR_INVALID_ARG;
    w.n_head_total = p->n_head_total == 0 ? H : (int64_t)p->n_head_total;
    if (p->head_first < 0 || (int64_t)p->head_first + H > w.n_head_total) return FATTN_ERR_INVALID_ARG;
    return FATTN_OK;
}

// the mask view and its planes (w.has_mask, w.m_*)
inline int check_mask(const fattn_tensor& mk, Views& w, int64_t N, int64_t NQ, int64_t H, int64_t S) {
    w.has_mask = mk.data != nullptr;
    if (!w.has_mask) return FATTN_OK;
    // rows padded to an even length (ggml pads to GGML_KQ_MASK_PAD), dword aligned
    if (mk.type != FATTN_TYPE_F16 || mk.ne[0] < N + (N & 1) || mk.ne[1] < NQ) return FATTN_ERR_INVALID_ARG;
    if ((uintptr_t)mk.data % 4 || mk.nb[1] % 4) return FATTN_ERR_ALIGNMENT;
    // mask planes: ne[2] per head, ne[3] per sequence, read by the query's
    // indices as ggml does (iq2 % ne[2], iq3 % ne[3]); a count below 1 reads
    // as 1 (zeroed structs), and a count of 1 has no stride to look at
    w.m_ne2 = std::max<int64_t>(1, mk.ne[2]);
    w.m_ne3 = std::max<int64_t>(1, mk.ne[3]);
    if (H % w.m_ne2 || S % w.m_ne3) return FATTN_ERR_INVALID_ARG;
    if (w.m_ne2 > 1) w.m_nb2 = mk.nb[2];
    if (w.m_ne3 > 1) w.m_nb3 = mk.nb[3];
    if (w.m_nb2 % 4 || w.m_nb3 % 4) return FATTN_ERR_ALIGNMENT;
    if (w.m_nb2 < 0 || w.m_nb3 < 0) return FATTN_ERR_BAD_STRIDE;
    // (mask_head_off takes iq2 % ne[2] through a float quotient)
    if (w.m_ne2 > 1 && H >= (int64_t)1 << 24) return FATTN_ERR_INVALID_ARG;
    return FATTN_OK;
}

// The one pair of unequal row lengths: q.ne[0] = k.ne[0] = 576, v.ne[0] = 512,
// not transposed (multi-head latent attention, include/fattn.h).
// f16 rows: 16-B pieces only, bases and nb[1..3] multiples of 16.  V is a VIEW of
// K when it starts 0 .. 128 bytes (a multiple of 16) into K's first row with K's
// strides (a stride of a dim of one element is not looked at): the kernel then
// loads each cache row once and takes V out of the K tile.
// Q8_0 / Q4_0 rows (18 blocks, 612 / 324 B): dword pieces, bases and nb[1..3]
// multiples of 4; V MUST be such a view, 0, 1 or 2 whole blocks into the row.
inline int check_views_mla(const fattn_params* p, Views& w) {
    const fattn_tensor &q = p->q, &k = p->k, &v = p->v, &mk = p->mask;
    if (k.ne[0] != kMlaDK || v.ne[0] != kMlaDV) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    const bool quant = in_list(QuantTypes(), k.type);
    const int64_t bb = quant ? (int64_t)row_size(k.type, QK) : 2;  // nb[0]: a block's / an element's bytes
    const int64_t rowK = quant ? kMlaDK / QK * bb : kMlaDK * 2, rowV = quant ? kMlaDV / QK * bb : kMlaDV * 2;
    if ((k.type != FATTN_TYPE_F16 && !quant) || v.type != k.type || k.nb[0] != bb || v.nb[0] != bb) return FATTN_ERR_UNSUPPORTED_TYPE;
    w.mla = true;
    const int64_t NQ = w.NQ = q.ne[1], H = w.H = q.ne[2], S = w.S = q.ne[3];
    const int64_t N = w.N = k.ne[1], Hkv = w.Hkv = k.ne[2], Skv = w.Skv = k.ne[3];
    if (NQ <= 0 || H <= 0 || S <= 0 || N <= 0 || Hkv <= 0 || Skv <= 0) return FATTN_ERR_INVALID_ARG;
    if (v.ne[1] != N || v.ne[2] != Hkv || v.ne[3] != Skv) return FATTN_ERR_INVALID_ARG;
    if (H % Hkv || S % Skv) return FATTN_ERR_INVALID_ARG;
    if (N > (int64_t)1 << 30 || NQ * H * S > (int64_t)1 << 31) return FATTN_ERR_INVALID_ARG;
    w.mixed = w.v_trans = false;
    if ((uintptr_t)q.data % 16 || q.nb[1] % 16 || q.nb[2] % 16 || q.nb[3] % 16) return FATTN_ERR_ALIGNMENT;
    if (const int rc = check_scalars(p, w, H)) return rc;
    const int64_t off = (int64_t)((uintptr_t)v.data - (uintptr_t)k.data);
    const bool same_nb = (N == 1 || v.nb[1] == k.nb[1]) && (Hkv == 1 || v.nb[2] == k.nb[2]) && (Skv == 1 || v.nb[3] == k.nb[3]);
    // a quantised cache has no V of its own: the view is looked at before the
    // alignment (a V 17 bytes into the row is no view, not a misaligned one)
    if (quant && !((uintptr_t)v.data >= (uintptr_t)k.data && off <= 2 * bb && off % bb == 0 && same_nb)) return FATTN_ERR_UNSUPPORTED_TYPE;
    // (a quantised V is K's base plus whole blocks of 34 / 18 B -- 2 mod 4 one
    // block in: the kernel never addresses through it, only K's base counts)
    const int al = quant ? 4 : 16;
    for (const fattn_tensor* t : {&k, &v})
        if ((!(quant && t == &v) && (uintptr_t)t->data % al) || t->nb[1] % al || t->nb[2] % al || t->nb[3] % al)
            return FATTN_ERR_ALIGNMENT;
    // (rows may be padded, not overlapped: a row past N must lie past the span)
    if (k.nb[1] < rowK || v.nb[1] < rowV) return FATTN_ERR_BAD_STRIDE;
    if (const int rc = check_mask(mk, w, N, NQ, H, S)) return rc;
    w.g16 = !quant;
    if ((uintptr_t)v.data >= (uintptr_t)k.data && off <= (quant ? 2 * bb : kMlaVOffMax) && same_nb) w.mla_v_off = off;
    w.k_span = (N - 1) * k.nb[1] + rowK;
    w.v_span = (N - 1) * v.nb[1] + rowV;
    w.m_span = w.has_mask ? (NQ - 1) * mk.nb[1] + mk.ne[0] * 2 : 0;
    w.m_span_h = w.m_span + (w.m_ne2 - 1) * w.m_nb2;
    w.q_span = (NQ - 1) * q.nb[1] + (H - 1) * q.nb[2] + kMlaDK * 4;
    if (w.k_span > kSpanMax || w.v_span > kSpanMax || w.m_span_h > kSpanMax || w.q_span > kSpanMax) return FATTN_ERR_BAD_STRIDE;
    return FATTN_OK;
}

inline int check_views(const fattn_params* p, Views& w) {
    if (!p || !p->q.data || !p->k.data || !p->v.data || !p->dst) return FATTN_ERR_INVALID_ARG;
    const fattn_tensor &q = p->q, &k = p->k, &v = p->v, &mk = p->mask;
    if (q.type != FATTN_TYPE_F32 || q.nb[0] != 4) return FATTN_ERR_UNSUPPORTED_TYPE;
    const int64_t D = w.D = q.ne[0];
    if (D == kMlaDK) return check_views_mla(p, w);
    if (D != 64 && D != 80 && D != 96 && D != 128 && D != 256) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    if (D % QK && (k.type != FATTN_TYPE_F16 || v.type != FATTN_TYPE_F16)) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    // BF16: K and V both BF16 (no mixed pair), D = 64 / 128 / 256, rows not transposed
    const bool bf16 = k.type == FATTN_TYPE_BF16 || v.type == FATTN_TYPE_BF16;
    if (bf16 && k.type != v.type) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (bf16 && D == 96) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    if (k.ne[0] != D || v.ne[0] != D) return FATTN_ERR_INVALID_ARG;
    const int64_t NQ = w.NQ = q.ne[1], H = w.H = q.ne[2], S = w.S = q.ne[3];
    const int64_t N = w.N = k.ne[1], Hkv = w.Hkv = k.ne[2], Skv = w.Skv = k.ne[3];
    if (NQ <= 0 || H <= 0 || S <= 0 || N <= 0 || Hkv <= 0 || Skv <= 0) return FATTN_ERR_INVALID_ARG;
    if (v.ne[1] != N || v.ne[2] != Hkv || v.ne[3] != Skv) return FATTN_ERR_INVALID_ARG;
    if (H % Hkv || S % Skv) return FATTN_ERR_INVALID_ARG;
    if (N > (int64_t)1 << 30 || NQ * H * S > (int64_t)1 << 31) return FATTN_ERR_INVALID_ARG;
    if (!is_row16(k.type) && !is_quant(k.type)) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (!is_row16(v.type) && !is_quant(v.type)) return FATTN_ERR_UNSUPPORTED_TYPE;
    // mixed K/V types (llama.cpp's separate cache types, e.g. K Q8_0 with V F16):
    // the split kernel, head dims 64 / 128 / 256
    w.mixed = k.type != v.type;
    if (w.mixed && D != 64 && D != 128 && D != 256) return FATTN_ERR_UNSUPPORTED_TYPE;
    // Q4_1 / Q5_0 / Q5_1: K and V of one type, not at D = 96 (Q5_0 rows of 66 B
    // are no whole number of dwords; the three share one rule)
    if (is_kv_ext(k.type) || is_kv_ext(v.type)) {
        if (w.mixed) return FATTN_ERR_UNSUPPORTED_TYPE;
        if (D == 96) return FATTN_ERR_UNSUPPORTED_HEAD_DIM;
    }
    if ((uintptr_t)q.data % 16 || q.nb[1] % 16 || q.nb[2] % 16 || q.nb[3] % 16) return FATTN_ERR_ALIGNMENT;
    if (const int rc = check_scalars(p, w, H)) return rc;

    const size_t rowK = row_size(k.type, D), rowV = row_size(v.type, D);
    // K rows must be contiguous (nb[0] = element size / block granular)
    if (is_row16(k.type) && k.nb[0] != 2) return FATTN_ERR_BAD_STRIDE;
    if (v.type == FATTN_TYPE_BF16 && v.nb[0] != 2) return FATTN_ERR_BAD_STRIDE;  // (no transposed BF16 V)
    if (is_quant(k.type) && k.nb[0] != (int64_t)row_size(k.type, 32)) return FATTN_ERR_BAD_STRIDE;
    w.v_trans = false;
    if (v.type == FATTN_TYPE_F16 && v.nb[0] != 2) {
        if (v.nb[1] != 2) return FATTN_ERR_BAD_STRIDE;
        w.v_trans = true;
        if (N % kStep || v.nb[0] % 16 || (uintptr_t)v.data % 16) return FATTN_ERR_BAD_STRIDE;
        // the transposed-V kernels exist for f16 K only (flash_row_float.h's layout)
        if (k.type != FATTN_TYPE_F16) return FATTN_ERR_UNSUPPORTED_TYPE;
    }
    if (is_quant(v.type) && v.nb[0] != (int64_t)row_size(v.type, 32)) return FATTN_ERR_BAD_STRIDE;
    if (k.nb[1] % 2 || k.nb[2] % 4 || k.nb[3] % 4 || (uintptr_t)k.data % 4) return FATTN_ERR_ALIGNMENT;
    if (v.nb[1] % 2 || v.nb[2] % 4 || v.nb[3] % 4 || (uintptr_t)v.data % 4) return FATTN_ERR_ALIGNMENT;

    if (const int rc = check_mask(mk, w, N, NQ, H, S)) return rc;

    // fast path: 16-B pieces.  Quantised rows: contiguous per head (a step of
    // 32 rows is one run of bytes); f16 rows: 16-B aligned
    auto rows16 = [&](const fattn_tensor& t, size_t row) {
        const bool base = (uintptr_t)t.data % 16 == 0 && t.nb[2] % 16 == 0 && t.nb[3] % 16 == 0;
        return is_quant(t.type) ? base && t.nb[1] == (int64_t)row && N % kStep == 0 : base && t.nb[1] % 16 == 0;
    };
    bool g16 = rows16(k, rowK);
    if (!w.v_trans)
        g16 = g16 && rows16(v, rowV);
    else
        g16 = g16 && v.nb[2] % 16 == 0 && v.nb[3] % 16 == 0;
    if (w.has_mask) g16 = g16 && (uintptr_t)mk.data % 16 == 0 && mk.nb[1] % 16 == 0 && N % kStep == 0;
    if (w.has_mask) g16 = g16 && w.m_nb2 % 16 == 0 && w.m_nb3 % 16 == 0;  // (every plane's base 16-B aligned)
    w.g16 = g16;
    if (!g16 && w.v_trans) return FATTN_ERR_BAD_STRIDE;
    // the dword-granular path needs dword rows (D = 96 Q8_0 / Q4_0 rows are 102 / 54 B:
    // contiguous 16-B-aligned caches only)
    if (!g16 && (k.nb[1] % 4 || (!w.v_trans && v.nb[1] % 4))) return FATTN_ERR_ALIGNMENT;

    w.k_span = (N - 1) * k.nb[1] + (int64_t)rowK;
    w.v_span = w.v_trans ? (D - 1) * v.nb[0] + N * 2 : (N - 1) * v.nb[1] + (int64_t)rowV;
    // (one plane's; a sequence plane moves the descriptor's base, the head
    // planes are offsets inside it: m_span_h)
    w.m_span = w.has_mask ? (NQ - 1) * mk.nb[1] + mk.ne[0] * 2 : 0;
    w.m_span_h = w.m_span + (w.m_ne2 - 1) * w.m_nb2;
    w.q_span = (NQ - 1) * q.nb[1] + (H - 1) * q.nb[2] + D * 4;
    if (w.k_span > kSpanMax || w.v_span > kSpanMax || w.m_span_h > kSpanMax || w.q_span > kSpanMax) return FATTN_ERR_BAD_STRIDE;
    return FATTN_OK;
}

// ---------------------------------------------------------------- kernel arguments
// The views, shapes and score transform as the kernels take them, with the
// split kernel's 16-row packing (choose_kernel repacks for the other kernels)
inline void fill_args(const fattn_params* p, const Views& w, SplitArgs& a) {
    const fattn_tensor &q = p->q, &k = p->k, &v = p->v, &mk = p->mask;
    std::memset(&a, 0, sizeof(a));
    a.q = (const uint8_t*)q.data;
    a.k = (const uint8_t*)k.data;
    a.v = (const uint8_t*)v.data;
    a.mask = (const uint8_t*)mk.data;
    a.dst = p->dst;
    a.q_nb1 = q.nb[1]; a.q_nb2 = q.nb[2]; a.q_nb3 = q.nb[3];
    a.k_nb1 = k.nb[1]; a.k_nb2 = k.nb[2]; a.k_nb3 = k.nb[3];
    a.v_nb0 = v.nb[0]; a.v_nb1 = v.nb[1]; a.v_nb2 = v.nb[2]; a.v_nb3 = v.nb[3];
    a.m_nb1 = w.has_mask ? mk.nb[1] : 0;
    a.m_nb2 = w.m_nb2; a.m_nb3 = w.m_nb3;
    a.m_ne2 = (int)w.m_ne2; a.m_ne3 = (int)w.m_ne3;
    a.m_ne2_inv = 1.0f / (float)w.m_ne2;
    a.m_hg = 1;
    a.NQ = (int)w.NQ; a.H = (int)w.H; a.S = (int)w.S; a.N = (int)w.N;
    a.rk2 = (int)(w.H / w.Hkv);
    a.rk3 = (int)(w.S / w.Skv);
    pack_tiles(a, kRows, std::min(a.rk2, kRows), w.NQ);
    a.has_mask = w.has_mask ? 1 : 0;
    a.scale_log2 = p->scale * 1.4426950408889634f;
    a.scale = p->scale;
    // the score transform (ScoreXf): the cap whenever given, the slopes only
    // with a mask to scale (max_bias without one: the plan of max_bias = 0)
    if (p->logit_softcap > 0.0f) {
        a.xf.live |= 1;
        a.xf.cap = p->logit_softcap;
        a.xf.scale_cap = p->scale / p->logit_softcap;
    }
    if (p->max_bias > 0.0f && w.has_mask) {
        int n2 = 1;
        while ((int64_t)n2 * 2 <= w.n_head_total) n2 *= 2;
        a.xf.live |= 2;
        a.xf.m0_log2 = -(p->max_bias / (float)n2);
        a.xf.m1_log2 = -(p->max_bias / 2.0f / (float)n2);
        a.xf.n2 = n2;
        a.xf.head_first = p->head_first;
    }
    a.k_span = (uint32_t)w.k_span;
    a.v_span = (uint32_t)w.v_span;
    a.m_span = (uint32_t)w.m_span;
    a.m_span_h = (uint32_t)w.m_span_h;
    a.q_span = (uint32_t)w.q_span;
}

// ---------------------------------------------------------------- kernel choice
// Picks pl.kernel (the prefill and split kernels' second forms are chosen by
// their sizing: size_pf, size_split) and packs the tiles for it.
inline void choose_kernel(const fattn_params* p, const Views& w, const Options& o, Plan& pl) {
    SplitArgs& a = pl.a;
    const int64_t D = w.D, NQ = w.NQ, N = w.N, Hkv = w.Hkv, S = w.S;
    const int kt = p->k.type;
    const int opt_pf = o[FATTN_OPT_PF], opt_bd = o[FATTN_OPT_BD];
    // many query rows per kv head (batched decode, prefill): the multi-query
    // kernel dequantises each K/V tile once for 64 rows.  Whole head groups
    // are packed (R = rk2, a power of two <= 64).
    // (below 256 packed rows per kv head the split kernel measures faster:
    // config 5, 64 rows, 15.5 vs 37.6 us at 4 heads; FATTN_OPT_MQ_MIN_ROWS)
    // (any rk2 <= 64: with R = rk2 not a power of two a tile packs
    // floor(rows / R) whole head groups and its last rows stay empty)
    const int64_t rows = NQ * a.rk2;  // packed rows per kv head
    const bool heads_ok = rows >= 32 && a.rk2 <= 64;
    const bool packed_ok = !o[FATTN_OPT_MQ_DISABLE] && !w.mixed && w.g16 && heads_ok;
    // (Q4_1 / Q5_0 / Q5_1: none of the multi-query and batched-decode kernels -- their
    // shapes fall to the split kernel -- and prefill only through the f16 staging)
    const bool quant_ok = packed_ok && in_list(QuantTypes(), kt);
    const bool stage_ok = packed_ok && is_kv_ext(kt) && o[FATTN_OPT_PF_STAGE] != 1 && N * D * 2 <= kSpanMax;
    const bool mq_ok = quant_ok && has_kernel(Kernel::Mq, kt, kt, (int)D);
    // the same packing for f16 K/V rows (not transposed V): the prefill and
    // batched-decode kernels fill their f16 images by LDS-DMA straight from the rows
    const bool f16_ok = packed_ok && kt == FATTN_TYPE_F16 && !w.v_trans;
    // Both 64-row-tile kernels (multi-query, batched decode) need every KV
    // chunk to hold at least two 128-key tiles: a workgroup with one tile is all
    // prologue and epilogue (config-5 shard, 4 heads x 64 rows: split kernel
    // 9.4 + 4.3 us merge, multi-query 11.0 + 4.3, batched decode 10.9 + 4.4)
    const int64_t qpt64 = (quant_ok || f16_ok) ? 64 / a.rk2 : 1;  // query rows per 64-row tile (rk2 <= 64)
    const int64_t y64 = Hkv * ((NQ + qpt64 - 1) / qpt64);
    const bool wide = N * y64 * S >= (int64_t)2 * kBdKeys * pl.cus;
    // (the multi-query kernel shares one mask row among a query row's heads:
    // with head planes the planner leaves it, for the batched-decode or the
    // split kernel, as scale <= 0 leaves the prefill kernels)
    const int min_rows = o[FATTN_OPT_MQ_MIN_ROWS];  // (an explicit threshold wins over `wide`)
    const bool mq = mq_ok && w.m_ne2 == 1 && rows >= (min_rows ? min_rows : kMqMinRowsDefault) &&
                    (wide || rows >= 256 || min_rows != 0);
    // prefill shapes: 256-row workgroups over 64-key tiles, no KV split, when
    // the (kv head x query tile x seq) workgroups alone fill the chip
    // (f16 K/V rows, not transposed V: the same kernel, images filled by DMA)
    // (D = 80: f16 only, its images padded to 96 dims)
    // (D = 80's padding dims are DMA'd from 0x80000000 past the row offset,
    // outside the descriptor only while the spans stay within 2 GiB: fattn_pf.h)
    const bool d80_ok = f16_ok && w.k_span <= (int64_t)0x80000000 && w.v_span <= (int64_t)0x80000000;
    // (a staged cache: the f16 kernel)
    const bool pf_dim = has_kernel(Kernel::Pf, stage_ok ? FATTN_TYPE_F16 : kt, stage_ok ? FATTN_TYPE_F16 : kt, (int)D) && (D != 80 || d80_ok);
    const bool pf = (quant_ok || f16_ok || stage_ok) && opt_pf != 1 && pf_dim &&
                    p->kv_chunk <= 0 && N % kPfKeys == 0 && p->scale > 0.0f &&
                    (opt_pf == 2 || Hkv * S * ((rows + kPfRows - 1) / kPfRows) >= pl.cus);
    // batched decode (config 5: 64 query rows per kv head): 64-row workgroups
    // over 128-key tiles, the KV split over workgroups to fill the chip, the
    // chunk partials merged in a second launch; Q8_0 / Q4_0 and f16 K/V
    // (from 64 rows, when the chunks hold two tiles or more: `wide` above)
    // Q8_0 / Q4_0 take the compute / build-role form (fattn_bdp.h) unless
    // FATTN_OPT_BD = 2 asks for the all-waves form; head dims 64 and 96 (Q8_0 /
    // Q4_0) have the role form only (config-5 shape at D = 64: 19.2 us against
    // 21.3 for the multi-query kernel, profiles/r04_e)
    const Kernel bd_form = quant_ok && opt_bd != 2 ? Kernel::Bdp : Kernel::Bd;
    const bool bd_dim = (quant_ok || f16_ok) && has_kernel(bd_form, kt, kt, (int)D);
    const bool bd = !pf && opt_bd != 1 && bd_dim && N % kStep == 0 && (opt_bd >= 2 || (rows >= kBdRows && wide));

    if (pf) {
        pl.kernel = Kernel::Pf;
        pack_tiles(a, kPfRows, a.rk2, NQ);
    } else if (bd) {
        pl.kernel = bd_form;
        pack_tiles(a, kBdRows, a.rk2, NQ);
    } else if (mq) {
        pl.kernel = Kernel::Mq;
        // 256 rows per workgroup once that still gives one workgroup per CU
        const int64_t wg256 = Hkv * S * ((rows + 255) / 256);
        const int rpw = o[FATTN_OPT_MQ_ROWS_PER_WAVE];
        pl.nw = D == 256 ? 4 : rpw ? (rpw == 32 ? 8 : 4) : wg256 >= pl.cus ? 8 : 4;  // (D = 256: lds_bytes)
        pack_tiles(a, pl.nw == 8 ? 256 : 64, a.rk2, NQ);
    } else {
        pl.kernel = Kernel::Split;
        // GQA decode of one query row (config 4): one q head per split tile instead
        // of the kv head's R heads packed -- one-row tiles, so the in-launch row
        // merge (wg_row_merge) replaces the merge launch; each K/V byte is read
        // by the R tiles of its kv head (the first from HBM, the rest mostly from
        // the caches) (FATTN_OPT_GQA_UNPACK)
        if (NQ == 1 && a.rk2 > 1 && o[FATTN_OPT_GQA_UNPACK] == 2) pack_tiles(a, kRows, 1, NQ);
    }
}

// ---------------------------------------------------------------- sizing
// Split-KV sizing.  A workgroup has nwv waves (4, 8 or 16); every wave streams
// `spw` steps of 32 positions.  One-row tiles (decode without GQA packing) with
// at least 6 steps per CU take 8 waves per workgroup, one step in flight each
// (config 3: 8 waves x 2 steps, 11.3 us against 11.8 with 16 waves x 1 step
// all requested at once, 12.4 with both steps of the 8 waves in flight, 12.6
// for the 4-wave form; config 2: 8 x 1); multi-row tiles keep 4 waves up to 8
// steps per CU (config 4: 10.8 vs 11.3 us; config 5's 8-rank shard, 4 heads:
// 11.7 vs 12.0) and take 8 from 16 (round 5, same box: 4-rank shard 14.0 vs
// 15.2 us, 2-rank shard 19.6 vs 19.9; profiles/r05_l).  The grid is sized so that
// all (Y x S x chunks) workgroups are co-resident, limited by LDS (steps in
// flight) and registers.
inline int size_split(Plan& pl, const Options& o, int kv_chunk, int64_t Y, int64_t S, int64_t N, int64_t NQ) {
    SplitArgs& a = pl.a;
    auto lds = [&](int nbuf, int nwv) { return lds_bytes(Kernel::Split, pl.kt, pl.vt, pl.D, nwv, nbuf); };
    const int64_t steps = (N + kStep - 1) / kStep;
    const int wps = split_bounds_wps(pl.kt, pl.gran, pl.D);  // __launch_bounds__ waves/SIMD
    const int rv_max = std::min<int64_t>(kRows, (int64_t)a.R * std::min<int64_t>(a.QPT, NQ));
    const int64_t total = steps * Y * S;
    const bool fused_merge = o[FATTN_OPT_SPLIT_MERGE] != 0;
    int nwv = 4;
    // (max_bias / logit_softcap live: 4 waves, the form whose bodies carry the
    // score transform -- launch_split_e; FATTN_OPT_SPLIT_WAVES does not apply)
    if (pl.gran == 16 && !a.xf.live) {
        if (o[FATTN_OPT_SPLIT_WAVES] > 0) {
            nwv = o[FATTN_OPT_SPLIT_WAVES];
        } else if (kv_chunk <= 0) {
            const int64_t per_cu = total / pl.cus;
            nwv = ((rv_max == 1 && per_cu >= 6) || (rv_max > 1 && per_cu >= 16)) ? 8 : 4;
        }
        nwv = std::min(nwv, 4 * wps);
        while (nwv > 4 && lds(1, nwv) > kLdsPerCU) nwv /= 2;
    }
    const int quantum = kStep * nwv;
    auto chunks = [&](int64_t spw_) { return (N + spw_ * quantum - 1) / (spw_ * quantum); };
    auto fit = [&](int nb) {  // steps in flight, LDS permitting
        while (nb > 1 && lds(nb, nwv) > kLdsPerCU) nb--;
        return nb;
    };
    // steps in flight per wave: 2 with 4 waves, 1 with more (the measured
    // optima; more bytes requested at once land later for every wave)
    auto inflight = [&](int spw_) { return fit(std::min(spw_, nwv == 4 ? 2 : 1)); };
    int spw = 1;
    if (kv_chunk > 0) {
        spw = (int)((kv_chunk + quantum - 1) / quantum);
        // a forced chunk is a lower bound: grow it until the combine fits
        while (chunks(spw) != 1 && !combine_ok(chunks(spw), rv_max)) spw++;
    } else {
        spw = (int)std::max<int64_t>(1, (total + (int64_t)pl.cus * nwv / 2) / ((int64_t)pl.cus * nwv));
        spw = (int)std::min<int64_t>(spw, (steps + nwv - 1) / nwv);
        for (;;) {
            const int wgs_cu = std::max(1, std::min(4 * wps / nwv, kLdsPerCU / lds(inflight(spw), nwv)));
            const int64_t slots = (int64_t)pl.cus * wgs_cu * nwv;
            const int64_t need = (int64_t)((steps + spw - 1) / spw) * Y * S;  // waves at this spw
            const int64_t nch = chunks(spw);
            if ((need <= slots && combine_ok(nch, rv_max)) || nch == 1) break;
            spw++;
        }
        // multi-row tiles with long per-wave slices: twice the chunks (two
        // workgroups per CU); their merge is a second launch from 4 chunks on
        // (config 5 on one GPU: 16 -> 8 steps per wave, 2 -> 4 chunks, 36.5 ->
        // 30.0 us; halving again, 8 chunks: 36.1)
        if (rv_max > 1 && spw >= 8 && !fused_merge && combine_ok(chunks(spw / 2), rv_max)) spw /= 2;
        if (o[FATTN_OPT_SPLIT_STEPS] > 0) {
            spw = (int)std::min<int64_t>(o[FATTN_OPT_SPLIT_STEPS], (steps + nwv - 1) / nwv);
            if (chunks(spw) > 1 && !combine_ok(chunks(spw), rv_max)) return FATTN_ERR_INVALID_ARG;
        }
    }
    int nbuf = o[FATTN_OPT_SPLIT_INFLIGHT] > 0 ? fit(std::min(spw, o[FATTN_OPT_SPLIT_INFLIGHT])) : inflight(spw);
    pl.nwv = nwv;
    a.step_skip = o[FATTN_OPT_SPLIT_SKIP] ? 0 : 1;
    a.split_prio = o[FATTN_OPT_SPLIT_PRIO];
    a.chunk_len = spw * quantum;
    a.n_chunks = (int)((N + a.chunk_len - 1) / a.chunk_len);
    a.ncp = next_pow2(a.n_chunks);
    if (a.n_chunks > 1 && !combine_ok(a.n_chunks, rv_max)) return FATTN_ERR_INVALID_ARG;
    // epilogue: one-row tiles with few parts publish per wave and the last wave
    // merges (4-wave form, D = 128); other one-row tiles merge their waves in
    // LDS and publish one row per workgroup; multi-row tiles: combine_tile
    a.wave_merge = 0;
    if (rv_max == 1 && !o[FATTN_OPT_SPLIT_WAVE_MERGE]) {
        if (nwv == 4 && a.n_chunks > 1 && pl.D == 128 && a.n_chunks * nwv <= kWaveMergeParts) a.wave_merge = 1;
        else if (nwv > 4 || a.n_chunks > 1) a.wave_merge = 2;
    }
    // loader waves (fattn_split_ld_kernel): one-row tiles on 8 waves whose
    // whole chunk fits the LDS (every step resident), 16-B rows, D = 64 / 128,
    // one K / V type; 4 loader waves issue it all up front
    if (o[FATTN_OPT_SPLIT_LOADERS] == 2 && pl.gran == 16 && a.wave_merge == 2 && nwv == 8 && spw >= 2 && spw <= 3 &&
        split_ld_ok(pl.kt, pl.vt, pl.D) && o[FATTN_OPT_SPLIT_INFLIGHT] == 0 &&
        lds(spw, nwv) + kSplitLdFlagBytes <= kLdsPerCU) {
        pl.kernel = Kernel::SplitLd;
        nbuf = spw;
    }
    a.nbuf = nbuf;
    a.wave_bytes = lds(nbuf, nwv) / nwv;
    pl.lds = lds_bytes(pl.kernel, pl.kt, pl.vt, pl.D, nwv, nbuf);
    // multi-row tiles (and one-row tiles forced onto the same epilogue) with 4
    // or more chunks: the chunk partials merge in a second launch, one wave per
    // (tile, row) instead of one workgroup per tile (config 5 shard: 11.8 vs
    // 14.8 us, config 4: 10.0 vs 10.7; with 2 chunks per tile, config 5 on
    // one GPU, the extra launch costs more than it saves: 36.6 vs 35.6).
    // FATTN_OPT_SPLIT_MERGE = 1: always the last-arriving workgroup (combine_tile).
    // FATTN_OPT_MERGE_IN_KERNEL = 1, with the whole grid co-resident: inside
    // the launch instead, the tile's workgroups waiting for each other and each
    // merging a share of the rows (tile_arrive_wait): measured 0.6-1.1 us
    // slower than the second launch (config 4 10.7-10.9 vs 10.0-10.3 us, the
    // config-5 8-rank shard 12.2 vs 11.6-11.7; profiles/r03_merge)
    const int64_t wgs_cu = std::max(1, std::min(4 * wps / nwv, kLdsPerCU / pl.lds));
    const bool resident = (int64_t)a.n_chunks * Y * S <= (int64_t)pl.cus * wgs_cu;
    a.merge_launch = (a.n_chunks >= 4 && a.wave_merge == 0 && !fused_merge)
                         ? ((resident && o[FATTN_OPT_MERGE_IN_KERNEL]) ? 2 : 1) : 0;
    // (auto: f16 partials for tiles of 8+ rows -- the 8-rank config-5 shard
    // 11.67 -> 11.50 us; config 4's 4-row tiles were 10.09 -> 10.33 us, so
    // they keep f32; profiles/r06_f)
    // (a BF16 cache: f32 partials always -- O / l of a V past 65504 is the overflow the type avoids)
    a.part_f16 = pl.kt != FATTN_TYPE_BF16 && part_f16_ok(o, a.merge_launch, pl.D) && (o[FATTN_OPT_PART_F16] == 2 || rv_max >= 8) ? 1 : 0;
    pl.grid = dim3(a.n_chunks, (unsigned)Y, (unsigned)S);
    // XCD-grouped order (tile_coords): a tile's chunk workgroups on one XCD.
    // Default for the one-row tiles that merge in-kernel (wg_row_merge):
    // config 3 11.80 vs 11.95 us, six alternating rounds (profiles/r05_a)
    const bool xcd_auto = a.wave_merge == 2 && a.n_chunks > 1;
    const int opt_xcd = o[FATTN_OPT_SPLIT_XCD];
    a.xcd_group = (opt_xcd == 2 || (opt_xcd == 0 && xcd_auto)) && (a.n_chunks * Y * S) % 8 == 0 ? 1 : 0;
    // partial rows per (tile, chunk): one per wave (wave_merge 1), one per
    // workgroup (2), or the tile's kRows
    if (a.n_chunks > 1)
        layout_partials(pl, (size_t)S * Y, (size_t)S * Y * a.n_chunks * (a.wave_merge == 1 ? nwv : a.wave_merge == 2 ? 1 : kRows));
    return FATTN_OK;
}

// Multi-query sizing: 64 or 256 packed rows per workgroup, KV split only when the
// (kv head x query tile x seq) workgroups cannot fill the chip (two per CU at
// 64 rows, one at 256).
inline int size_mq(Plan& pl, const Options& o, int kv_chunk, int64_t Y, int64_t S, int64_t N) {
    SplitArgs& a = pl.a;
    const int64_t tiles = N / kStep;  // N % kStep == 0 (16-B path)
    const int64_t base = Y * S;
    const int subs = pl.nw == 8 ? 16 : 4;  // 16-row subtiles per tile
    int64_t nch;
    if (kv_chunk > 0) {
        nch = (N + kv_chunk - 1) / kv_chunk;
    } else {
        const int64_t want = pl.nw == 8 ? pl.cus : 2 * pl.cus;
        nch = (want + base - 1) / base;
        nch = std::min<int64_t>(nch, std::max<int64_t>(1, tiles / 4));  // >= 4 tiles per workgroup
    }
    nch = std::max<int64_t>(1, std::min<int64_t>(nch, tiles));
    int64_t tpc = (tiles + nch - 1) / nch;
    // the chunk partials merge in a second launch (one wave per packed row,
    // at most 64 chunks: one (m, l) pair per lane); FATTN_OPT_SPLIT_MERGE = 1:
    // in the tile's last-arriving workgroup (at most 16 chunks per 16-row subtile)
    const bool fused = o[FATTN_OPT_SPLIT_MERGE] != 0;
    // the merge launch's grid.y is Y x the 16-row subtiles per tile: where that
    // would pass the 65535 grid limit the KV sequence is not split (so many
    // tiles fill the chip without it; a requested kv_chunk is a hint)
    if (!fused && Y * subs > 65535) tpc = tiles;
    for (;;) {
        nch = (tiles + tpc - 1) / tpc;
        if (nch == 1 || (fused ? combine_ok(nch, kRows) : nch <= kWaveMergeParts)) break;
        tpc++;
    }
    a.chunk_len = (int)(tpc * kStep);
    a.n_chunks = (int)nch;
    a.merge_launch = (nch > 1 && !fused) ? 1 : 0;
    // (f16 partials: the config-5 shape at D = 256 55.14 -> 50.82 us, profiles/r06_p)
    a.part_f16 = part_f16_ok(o, a.merge_launch, pl.D) ? 1 : 0;
    a.ncp = next_pow2(a.n_chunks);
    pl.lds = lds_bytes(Kernel::Mq, pl.kt, pl.vt, pl.D, pl.nw);
    pl.grid = dim3(a.n_chunks, (unsigned)Y, (unsigned)S);
    if (a.n_chunks > 1) layout_partials(pl, (size_t)S * Y, (size_t)S * Y * subs * a.n_chunks * kRows);
    return FATTN_OK;
}

// Batched-decode sizing: one 8-wave workgroup (64 packed rows, 134 KiB of
// LDS) per CU; the KV sequence of each (kv head x 64-row tile) splits into
// chunks of whole 128-key tiles until the workgroups cover the CUs (at most
// 64 chunks: the merge launch takes one (m, l) pair per lane).
inline int size_bd(Plan& pl, const Options& o, int kv_chunk, int64_t Y, int64_t S, int64_t N) {
    SplitArgs& a = pl.a;
    const int64_t tiles = (N + kBdKeys - 1) / kBdKeys;
    pl.lds = lds_bytes(pl.kernel, pl.kt, pl.vt, pl.D, kBdWaves);
    if (pl.lds <= 0) return FATTN_ERR_UNSUPPORTED_TYPE;
    // workgroups per CU by LDS (the f16 D = 64 form fits two): the KV split
    // fills every resident slot, not one per CU
    const int64_t per_cu = std::max<int64_t>(1, kLdsPerCU / pl.lds);
    int64_t nch = kv_chunk > 0 ? (N + kv_chunk - 1) / kv_chunk : (pl.cus * per_cu + Y * S - 1) / (Y * S);
    nch = std::max<int64_t>(1, std::min<int64_t>(nch, tiles));
    int64_t tpc = (tiles + nch - 1) / nch;
    nch = (tiles + tpc - 1) / tpc;
    while (nch > kWaveMergeParts) {
        tpc++;
        nch = (tiles + tpc - 1) / tpc;
    }
    a.chunk_len = (int)(tpc * kBdKeys);
    a.n_chunks = (int)nch;
    a.ncp = next_pow2(a.n_chunks);
    pl.grid = dim3(a.n_chunks, (unsigned)Y, (unsigned)S);
    // XCD-grouped workgroup order (bd_tile_coords): whole tiles per XCD, so a
    // tile's Q rows come from HBM once (config 5: 49.7 vs 53.4 MB per launch,
    // 24.8-24.9 vs 25.1-25.4 us kernel + merge; profiles/r04_f)
    a.xcd_group = o[FATTN_OPT_BD_XCD] != 1 && (a.n_chunks * Y * S) % 8 == 0 ? 1 : 0;
    // the chunk partials merge inside the launch (bd_tile_merge: the tile's
    // workgroups wait for each other, so only when the whole grid is
    // co-resident -- one workgroup per CU by LDS) or in a second launch
    const bool resident = nch * Y * S <= (int64_t)pl.cus * per_cu;
    a.merge_launch = nch == 1 ? 0 : (resident && o[FATTN_OPT_MERGE_IN_KERNEL]) ? 2 : 1;
    // (f16 partials: config 5 22.81 -> 20.90 us, its 2-rank shard 19.78 -> 16.16
    // us, same box, profiles/r06_f)
    a.part_f16 = part_f16_ok(o, a.merge_launch, pl.D) ? 1 : 0;
    // partials: [S][Y][chunks][64 rows]; arrival words for the in-kernel merge only
    if (nch > 1) layout_partials(pl, (size_t)S * Y, (size_t)S * Y * nch * kBdRows, a.merge_launch == 2);
    return FATTN_OK;
}

// Prefill sizing: one workgroup per (kv head x query tile x seq), the whole KV
// sequence each; the pre-pass (staged f16 rows, live-block flags) in the workspace
inline int size_pf(Plan& pl, const Options& o, const fattn_params* p, const Views& w, int64_t Y) {
    SplitArgs& a = pl.a;
    const int64_t D = w.D, N = w.N, Hkv = w.Hkv, Skv = w.Skv;
    a.chunk_len = (int)N;
    a.pf_stagger = o[FATTN_OPT_PF_STAGGER];
    a.n_chunks = 1;
    a.ncp = 1;
    // Q8_0 / Q4_0: staged to f16 rows in the workspace, then the f16 kernel
    // (each K/V tile is otherwise dequantised once per 256-row query tile)
    // (only while the f16 rows stay addressable by the kernels' 32-bit
    // descriptors and tile offsets, N * D * 2 bytes per (kv head, seq): a
    // longer cache keeps the in-kernel dequantisation rather than wrap)
    pl.pf_stage = is_quant(pl.kt) && o[FATTN_OPT_PF_STAGE] != 1 && (int64_t)N * D * 2 <= kSpanMax;
    if (pl.pf_stage) {
        pl.stage_kt = pl.kt;
        pl.kt = pl.vt = FATTN_TYPE_F16;
        pl.stage_k = (const uint8_t*)p->k.data;
        pl.stage_v = (const uint8_t*)p->v.data;
        pl.stage_k_nb2 = p->k.nb[2]; pl.stage_k_nb3 = p->k.nb[3];
        pl.stage_v_nb2 = p->v.nb[2]; pl.stage_v_nb3 = p->v.nb[3];
        pl.stage_hkv = (int)Hkv;
        pl.stage_skv = (int)Skv;
        pl.stage_bytes = (size_t)Skv * Hkv * N * D * 2;
        // the staged rows: [Skv][Hkv][N][D] f16, contiguous
        a.k_nb1 = a.v_nb1 = D * 2;
        a.k_nb2 = a.v_nb2 = N * D * 2;
        a.k_nb3 = a.v_nb3 = Hkv * N * D * 2;
        a.k_span = a.v_span = (uint32_t)(N * D * 2);
    }
    // f16 rows (native or staged) at D = 128: the one-wave-per-SIMD body
    // (auto: the lean balanced schedule, form 6 -- the balanced form 5 was
    // 0-4 % faster than the 8-wave body on f16 rows, 12-21 % on staged Q8_0
    // with the zero mask and 1-3 % faster than the pipelined form 4
    // (profiles/r05_h, r05_p); the lean form's chains started from -m / c
    // take 1.5 % (f16) to 3.6 % (Q8_0 zero mask) off it, profiles/r06_c;
    // form 1 keeps the 8-wave body)
    const int form = o[FATTN_OPT_PF_FORM] == 0 ? 6 : o[FATTN_OPT_PF_FORM];
    // (max_bias / logit_softcap live: fattn_pf_kernel, which has the score
    // transform -- the one-wave-per-SIMD bodies' asm chains do not)
    if (pl.kt == FATTN_TYPE_F16 && D == 128 && form >= 4 && !a.xf.live) pl.kernel = Kernel::Pf4;
    pl.pf4_sched = form - 2;  // 4: pipelined (SCHED 2), 5: balanced (SCHED 3), 6: lean (SCHED 4)
    pl.lds = lds_bytes(pl.kernel, pl.kt, pl.vt, pl.D, 0);
    pl.grid = dim3(1, (unsigned)Y, (unsigned)w.S);
    // workspace: live-block flags, n_qt x N/64 bytes (masked prefill).  They
    // share the front of the workspace with the split-KV arrival words; a
    // later decode supersedes whatever the flags left there (its epoch
    // stamp, arrival_begin in fattn_split.h), so nothing is re-zeroed.
    pl.pf_flags = w.has_mask && !o[FATTN_OPT_PF_SKIP];
    // (one table per sequence plane and group of head planes, pf_flag_table)
    if (w.m_ne2 % a.rk2 == 0) a.m_hg = (int)(w.m_ne2 / a.rk2);
    if (pl.pf_flags) pl.cnt_bytes = ((size_t)w.m_ne3 * a.m_hg * a.n_qt * (N / kPfKeys) + 255) / 256 * 256;
    pl.ws_bytes = pl.cnt_bytes;
    if (pl.pf_stage) {
        pl.stage_off = pl.cnt_bytes;
        pl.ws_bytes = pl.stage_off + 2 * pl.stage_bytes;
    }
    return FATTN_OK;
}

// MLA sizing: one 4-wave workgroup (64 packed rows; 120 KiB of LDS with V a
// view of K, 144 KiB with V of its own) per CU; the KV sequence of each (kv
// head x 64-row tile x seq) splits into chunks of whole 32-key tiles until the
// workgroups cover the CUs -- at least 4 tiles a chunk (a workgroup's prologue
// is two tiles deep), at most 64 chunks (the merge takes one (m, l) pair per
// lane).  kv_chunk is a hint, rounded up to tiles.  Chunk partials: f32,
// [S][Y][chunks][64 rows] x 512, merged in a second launch (no arrival words).
inline int size_mla(Plan& pl, int kv_chunk, int64_t Y, int64_t S, int64_t N) {
    SplitArgs& a = pl.a;
    const bool own = pl.mla_v_off < 0;
    const int64_t tiles = (N + kStep - 1) / kStep;
    // (the cache's type picks the LDS figure and nothing else: a quantised
    // cache is cut into the chunks of the f16 one)
    pl.lds = visit(QuantTypes(), pl.kt, own ? MlaCfg<true>::ldsBytes : MlaCfg<false>::ldsBytes,
                   [](auto k) { return MlaCfg<false, decltype(k)::value>::ldsBytes; });
    int64_t nch;
    if (kv_chunk > 0) {
        nch = (N + kv_chunk - 1) / kv_chunk;
    } else {
        nch = (pl.cus + Y * S - 1) / (Y * S);
        nch = std::min<int64_t>(nch, std::max<int64_t>(1, tiles / 4));
    }
    nch = std::max<int64_t>(1, std::min<int64_t>(nch, tiles));
    int64_t tpc = (tiles + nch - 1) / nch;
    nch = (tiles + tpc - 1) / tpc;
    while (nch > kWaveMergeParts) {
        tpc++;
        nch = (tiles + tpc - 1) / tpc;
    }
    a.chunk_len = (int)(tpc * kStep);
    a.n_chunks = (int)nch;
    a.ncp = next_pow2(a.n_chunks);
    a.nbuf = own ? MlaCfg<true>::nBuf : MlaCfg<false>::nBuf;  // (quantised: three raw slots)
    a.merge_launch = nch > 1 ? 1 : 0;
    pl.grid = dim3(a.n_chunks, (unsigned)Y, (unsigned)S);
    // two row tiles per kv head: the pair on one XCD, so that its K rows come
    // from HBM once (fattn_mla_kernel; H = 128, N = 4096, 32 sequences: V of its
    // own 114.1 -> 106.7 us, V a view of K 103.7 -> 103.3 us)
    a.xcd_group = a.n_hsub == 2 && (nch * Y * S) % 16 == 0 ? 1 : 0;
    if (nch > 1) {
        const size_t parts = (size_t)S * Y * nch * kMlaRows;
        pl.cnt_bytes = 0;
        pl.ml_bytes = (parts * 2 * sizeof(float) + 255) / 256 * 256;
        pl.ws_bytes = pl.ml_bytes + parts * kMlaDV * 4;
    }
    return FATTN_OK;
}

// ---------------------------------------------------------------- the planner
// make_plan's plan, before its last check
inline int size_plan(const fattn_params* p, const Options& o, int cus, Plan& pl) {
    Views w;
    const int rc = check_views(p, w);
    if (rc != FATTN_OK) return rc;
    pl = Plan();
    pl.cus = cus;
    pl.merge_plain = o[FATTN_OPT_MERGE_PLAIN] == 2;
    pl.kt = p->k.type;
    pl.vt = w.v_trans ? VT_F16T : p->v.type;
    pl.D = (int)w.D;
    pl.gran = w.g16 ? 16 : 4;
    SplitArgs& a = pl.a;
    fill_args(p, w, a);
    // K dim 576 / V dim 512: one kernel for every shape of the op, 64 packed
    // rows per tile (whole head groups up to 64 heads; rk2 = 128: two tiles)
    if (w.mla) {
        pl.kernel = Kernel::Mla;
        pl.DV = kMlaDV;
        pl.mla_v_off = (int)w.mla_v_off;
        pack_tiles(a, kMlaRows, (int)std::min<int64_t>(a.rk2, kMlaRows), w.NQ);
        if (pl.kt != FATTN_TYPE_F16) {
            // (tile_rows: at most min(QPT, NQ) x R rows a tile)
            pl.mla_solo = std::min<int64_t>(a.QPT, w.NQ) * a.R <= kRows;
            pl.mla_raw16 = pl.mla_solo && p->k.nb[1] == (int64_t)row_size(pl.kt, kMlaDK) && (uintptr_t)p->k.data % 16 == 0 &&
                           (w.Hkv == 1 || p->k.nb[2] % 16 == 0) && (w.Skv == 1 || p->k.nb[3] % 16 == 0);
        }
        const int64_t Ym = (int64_t)w.Hkv * a.n_hsub * a.n_qt;
        if (Ym > 65535 || w.S > 65535) return FATTN_ERR_INVALID_ARG;
        return size_mla(pl, p->kv_chunk, Ym, w.S, w.N);
    }
    choose_kernel(p, w, o, pl);
    const int64_t Y = (int64_t)w.Hkv * a.n_hsub * a.n_qt;
    if (Y > 65535 || w.S > 65535) return FATTN_ERR_INVALID_ARG;
    switch (pl.kernel) {
        case Kernel::Pf: return size_pf(pl, o, p, w, Y);
        case Kernel::Bd:
        case Kernel::Bdp: return size_bd(pl, o, p->kv_chunk, Y, w.S, w.N);
        case Kernel::Mq: return size_mq(pl, o, p->kv_chunk, Y, w.S, w.N);
        default: break;
    }
    // split kernel with head planes: one staged mask row per packed (query row,
    // head) pair; its rows past the tile take offset m_span_h plus a step's
    // position, which must stay past the descriptor in 32 bits
    if (w.m_ne2 > 1) {
        a.m_hp = 1;
        if (w.m_span_h + w.m_span + 64 > kSpanMax) return FATTN_ERR_BAD_STRIDE;
    }
    // split kernel: whole 32-key steps without a row guard (issue_step), so the
    // rows up to the end of the last step must not wrap (tile_span; a
    // transposed V has N % 32 == 0 and no such rows)
    if (tile_span(w.k_span, p->k.nb[1], w.N, kStep) > kSpanMax ||
        (!w.v_trans && tile_span(w.v_span, p->v.nb[1], w.N, kStep) > kSpanMax))
        return FATTN_ERR_BAD_STRIDE;
    return size_split(pl, o, p->kv_chunk, Y, w.S, w.N, w.NQ);
}

// Validate and build the launch plan for a device of `cus` compute units.
// Returns FATTN_OK or an error -- the launcher's own for a plan whose kernel
// the library does not have (has_kernel: choose_kernel and the launchers read
// the same table, so this cannot happen; it would show here, not at launch).
inline int make_plan(const fattn_params* p, const Options& o, int cus, Plan& pl) {
    const int rc = size_plan(p, o, cus, pl);
    if (rc != FATTN_OK) return rc;
    if (!has_kernel(pl.kernel, pl.kt, pl.vt, pl.D)) return pl.kernel == Kernel::SplitLd ? FATTN_ERR_INVALID_ARG : FATTN_ERR_UNSUPPORTED_TYPE;
    return FATTN_OK;
}

}  // namespace fattn
