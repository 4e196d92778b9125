// fattn_tile.h -- what the kernel families share on the device: the kernel
// arguments (SplitArgs), the counted waits, buffer descriptors and LDS-DMA, the
// tiles' arrival words, the mask-plane and tile geometry (tile_decode,
// kv_sources), the diagnostic stamps, the one-row chunk merge (merge_row_parts,
// store_part_f16) and the merge launch built on it (fattn_chunk_merge_kernel).
// Included by fattn_split.h and by every kernel header for what it uses.
#pragma once

#include "fattn_common.h"

namespace fattn {

constexpr int kSplitWaves = 4;
constexpr int kStep = 32;   // KV positions per wave step (= one PV k-step)
constexpr int kRows = 16;   // packed query rows per workgroup (MFMA N)
constexpr int VT_F16T = 100;  // V f16 stored transposed ([D][N], flash_row_float.h:177)
constexpr int kCntStride = 64;  // uint32 words between arrival counters (256 B: atomics to one line serialise)
// deferred max (cdna_hip_programming.md T13): the exponentials' reference max
// moves only when a score exceeds it by more than 2^3 in p, so p <= 8 (and P*d
// of a V block stays far inside f16 range)
constexpr float kRescaleLog2 = 3.0f;
constexpr float kRescaleNat = kRescaleLog2 * 0.6931471805599453f;
constexpr bool kDecodeNT = true;   // decode K/V: read once per launch

struct SplitArgs {
    const uint8_t* q;
    const uint8_t* k;
    const uint8_t* v;
    const uint8_t* mask;
    float* dst;
    uint32_t* ws_cnt;   // [S][Y] chunk arrival words (64-bit), one per 256-B line (arrival_begin/arrive_last)
    float* ws_o;        // [S][Y][C][16][D] chunk partials
    float* ws_ml;       // [S][Y][C][16][2]
    int64_t q_nb1, q_nb2, q_nb3;
    int64_t k_nb1, k_nb2, k_nb3;
    int64_t v_nb0, v_nb1, v_nb2, v_nb3;
    int64_t m_nb1;
    // mask planes (ggml's mask ne[2] / ne[3]): query head iq2 of sequence iq3 reads
    // plane (iq2 % m_ne2, iq3 % m_ne3), m_nb2 / m_nb3 bytes apart (any order, gaps,
    // 0 = one plane repeated).  A workgroup serves one iq3, so the sequence plane
    // moves its descriptor's base (mask_seq_base); the head plane is a per-row
    // offset (mask_head_off) inside a descriptor of m_span_h bytes
    int64_t m_nb2, m_nb3;
    int m_ne2, m_ne3;       // plane counts, >= 1 (1, 1: one plane for every head and sequence)
    float m_ne2_inv;        // 1 / m_ne2 (mask_head_off)
    uint32_t m_span_h;      // m_span + (m_ne2 - 1) * m_nb2: the bytes of one sequence plane's descriptor
    int m_hp;               // split kernel: 1 = head planes -- one staged mask row per packed (query
                            // row, head) pair instead of one per query row (mask_row_off)
    int m_hg;               // prefill: flag tables per sequence plane (groups of head planes, pf_flag_table)
    uint32_t k_span, v_span, m_span, q_span;  // bytes addressed per (kv head, seq) / mask plane / seq of Q
    int NQ, H, S;       // q ne1, ne2, ne3
    int N;              // kv length
    int rk2, rk3;       // H/Hkv, S/Skv
    int R;              // q-heads packed per tile
    int QPT;            // query rows per tile
    int n_hsub, n_qt;   // head subgroups, query-row tiles
    float R_inv;        // 1/R: m / R == int((m + 0.5) * R_inv) exactly for m, R <= 16
    int chunk_len;      // positions per workgroup (multiple of kStep*kSplitWaves)
    int n_chunks;
    int ncp;            // next power of two >= n_chunks (combine kernel)
    float scale_log2;   // scale * log2(e)
    float scale;        // the softmax scale (split_step works in natural units)
    int has_mask;
    int nbuf;           // steps in flight per wave (1..4); LDS per wave = wave_bytes
    int wave_bytes;
    int pf_stagger;     // prefill kernel: SIMD partner waves run their phases staggered
    const uint8_t* pf_flags;  // prefill: [m_ne3][m_hg][n_qt][N/64] live-block flags (pf_mask_flags_block), or null
    int split_prio;     // split kernel wave priorities: 0 staggered 3/2/1/0, 1 none, 2 staggered while issuing
    int wave_merge;     // split kernel epilogue: 0 = LDS merge of the waves + combine_tile;
                        // 1 = one-row tiles: every wave publishes its own partial and the
                        // last-arriving WAVE merges them (no LDS merge, no barriers);
                        // 2 = one-row tiles: LDS merge, then one partial per workgroup
                        // (wg_row_merge)
    uint64_t arrival_stamp;  // kArrivalTag | launch epoch << kArrivalEpochShift (arrival_begin)
    int merge_launch;   // chunk partials of multi-row tiles: 1 = merged by a second launch
                        // (fattn_chunk_merge_kernel), 2 = inside the launch (tile_arrive_wait: grid co-resident)
    int step_skip;      // split kernel: 1 = skip steps whose mask is all -inf for the tile (FATTN_OPT_SPLIT_SKIP)
    int xcd_group;      // workgroups in XCD-grouped order (tile_coords; grid size % 8 == 0): batched decode, split kernel
    int part_f16;       // merge_launch 1: each chunk partial stored as O / l in f16 beside its (m, l) in f32
                        // (half the partial bytes; store_part_f16, merge_row_parts_h)
    ScoreXf xf;         // max_bias / logit_softcap (xf_score, fattn_common.h); xf.live == 0: off.  Last: the
                        // fields above keep their kernarg offsets
    const float* sinks; // attention sinks, one raw f32 logit per q head of this launch (fattn_ext_sinks;
                        // sink_inv, fattn_common.h), or null: off.  Appended behind xf, which keeps its
                        // offset as every field above it does.  Read only in the epilogues that
                        // normalise into dst, under a wave-uniform branch outside every tile loop
};

// fattn_ext_lse: the kernels' arguments with the pointer the rows' log-sum-exp
// goes to (f32 [S][NQ][H]; row_lse, fattn_common.h).  Every kernel that
// normalises into dst is a template over its argument type: over SplitArgs it
// is the kernel of a launch without lse -- lse_of() is a constant null there,
// so none of the log-sum-exp code exists in it and its argument block, registers
// and instructions are those it had before there was an lse --, over
// SplitArgsLse the one fattn_ext_lse launches (launch_args, fattn_launch.h).
// One lane per output row stores one float after the row's dst stores, behind
// the row guards of the dst store.
struct SplitArgsLse : SplitArgs {
    float* lse;
};
__device__ __forceinline__ constexpr float* lse_of(const SplitArgs&) { return nullptr; }
__device__ __forceinline__ float* lse_of(const SplitArgsLse& a) { return a.lse; }
// entry `row` of it, or null: off
template <typename A>
__device__ __forceinline__ float* lse_at(const A& a, int64_t row) {
    float* const lse = lse_of(a);
    return lse ? lse + row : nullptr;
}

// XOR mask of the 16-B chunk swizzle of an LDS row of `cpr` chunks: the largest
// power of two dividing cpr, minus one, so that chunk ^ (x & mask) stays a
// bijection on [0, cpr) (cpr = 16 / 8 for D = 128 / 64 f16 rows; 12 and 10 for
// the D = 96 / 80 rows, whose swizzle works within groups of 4 / 2 chunks)
__host__ __device__ constexpr int swz_mask(int cpr) { return (cpr & -cpr) - 1; }

// epilogue outputs per thread (16 threads per row): D / 16 where that is a
// multiple of 4 (D = 64, 128, 256), else 8 with D / 8 threads of the 16 active
template <int D>
constexpr int epi_ept() { return (D / 16) % 4 == 0 ? D / 16 : 8; }

// ---------------------------------------------------------------- counted waits
template <int N>
__device__ __forceinline__ void wait_vmcnt_c() {
    static_assert(N >= 0, "");
    constexpr int n = N > 63 ? 63 : N;  // vmcnt is 6 bits; waiting for fewer is still correct
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory");
}

// wait until at most `outstanding` whole steps (NI instructions each) remain
template <int NI>
__device__ __forceinline__ void wait_steps(int outstanding) {
    switch (__builtin_amdgcn_readfirstlane(outstanding)) {
        case 0: wait_vmcnt_c<0>(); break;
        case 1: wait_vmcnt_c<NI>(); break;
        case 2: wait_vmcnt_c<2 * NI>(); break;
        default: wait_vmcnt_c<3 * NI>(); break;
    }
}

// wait until at most `outstanding` whole steps plus EXTRA instructions remain
// (EXTRA = the V part of the oldest pending step: its K and mask have landed)
template <int NI, int EXTRA>
__device__ __forceinline__ void wait_steps_plus(int outstanding) {
    switch (__builtin_amdgcn_readfirstlane(outstanding)) {
        case 0: wait_vmcnt_c<EXTRA>(); break;
        case 1: wait_vmcnt_c<NI + EXTRA>(); break;
        case 2: wait_vmcnt_c<2 * NI + EXTRA>(); break;
        default: wait_vmcnt_c<3 * NI + EXTRA>(); break;
    }
}

// ---------------------------------------------------------------- descriptors, LDS-DMA
typedef __attribute__((address_space(3))) void lds_void;
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Buffer descriptor (4 SGPRs): base, stride 0, num_records = bytes, raw dword
// format.  Offsets at or past `bytes` fetch nothing and write ZEROS to LDS
// (tests/test_gpu_prims.py::test_lds_dma_partial_exec).
__device__ __forceinline__ i32x4 make_srd(const void* base, uint32_t bytes) {
    const uint64_t p = (uint64_t)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)p);
    r.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const lds_void*)p; }

// Buffer resource for compiler-tracked buffer loads (the hand-off reads of the
// chunk merges): built from readfirstlane'd inputs, so it is provably
// wave-uniform and no waterfall loop wraps the loads (cdna_hip_programming.md
// T20).  Offsets at or past num_records return zeros without memory traffic.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    const uint64_t p = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, (int)n, 0x00020000);
}
constexpr int kAuxSc1 = 16;  // buffer-load cache policy: sc1 (L1 bypass; MI355X_MICROARCH.md sc1 table)

// L1-bypassing (sc1) 16-B / 4-B loads of handed-off partials.  Compiler-tracked
// builtins: hipcc inserts the waits and never reads a register before its data
// landed (round 3's asm forms had three such miscompiles).
__device__ __forceinline__ u32x4 ld_sc1_buf(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kAuxSc1));
}
__device__ __forceinline__ uint32_t ld_sc1_buf_b32(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, kAuxSc1);
}

// 16-B load into registers through a buffer descriptor, as asm: UNTRACKED --
// hipcc inserts no wait for it, so waiting for it leaves the LDS-DMA issued
// after it in flight (a tracked load would make hipcc drain every DMA with
// vmcnt(0) at its first use, cdna_hip_programming.md §5 trap (b)).  The caller
// retires it with a counted wait and then passes every result through
// reg_fence<TAG>() before any use.  The asm comments "UNTRACKED(tag)" on the
// load and "RETIRED(tag)" on the fence let tools/isa_hazard_check.py prove on
// the ISA that no instruction touches the destination registers between the
// load and its fence on any path (tests/test_isa_hazards.py).
enum : int { kTagQ = 1, kTagMaskWords = 2 };  // bit masks
template <int TAG>
__device__ __forceinline__ u32x4 ld_buf_untracked(const i32x4& srd, uint32_t off) {
    u32x4 v;
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen ; UNTRACKED(%3)"
                 : "=v"(v)
                 : "v"(off), "s"(srd), "i"(TAG)
                 : "memory");
    return v;
}

// HBM -> LDS, one piece per lane at lds + lane*BYTES.  Inline asm: through the
// builtin, hipcc treats the LDS base as a per-lane value, and around an
// exec-masked (partial) instruction it built per-lane phis of (LDS base,
// offset) pairs whose readfirstlane'd M0 no longer matched the inactive
// lanes' offsets -- and it tracks the DMA in its s_waitcnt bookkeeping, so
// the first LDS read after it would wait for every DMA in flight.  Here the
// LDS address is an M0 operand ("{m0}": hipcc writes M0 itself, straight
// from the address arithmetic -- one s_add per DMA where the asm's own
// save / set / restore of the reserved M0 cost three s_mov; the prefill
// body issues 8 DMAs a tile with one wave per SIMD, where every scalar
// instruction takes an issue slot).  s_nop 4 opens the string: hipcc pads
// its own VMEM instructions but not an asm one, and it re-materialises the
// descriptor's words with v_readfirstlane right before the statement -- a
// VALU SGPR write needs 5 wait states before a VMEM instruction reads it
// (cdna_hip_programming.md 'Insert its wait states'; with s_nop 0 multi-chunk
// decodes read through a stale descriptor word; tools/isa_hazard_check.py
// audits every asm VMEM instruction for it).  It also covers M0 -> LDS-DMA
// (1 state).  Not tracked by the compiler's s_waitcnt bookkeeping: every
// consumer waits with an explicit vmcnt.
// NT: non-temporal policy for bytes one CU reads once (the decode KV stream,
// MI355X_MICROARCH.md 'nt-weights'); never for tiles other workgroups re-read.
// PAD: the opening s_nop's count -- 4 (5 wait states) unless the caller's
// descriptor is provably not freshly VALU-written (pf4's loop: its descriptors
// are loop-invariant SGPRs; tools/isa_hazard_check.py checks every call site
// on the shipped ISA, so a PAD that is too small fails the CPU test suite)
template <int BYTES, bool NT = false, int PAD = 4>
__device__ __forceinline__ void dma(const i32x4& srd, uint32_t lds_any, uint32_t off) {
    static_assert(BYTES == 16 || BYTES == 4, "");
    static_assert(PAD >= 0 && PAD <= 4, "");
    // wave-uniform by construction; readfirstlane keeps it an SGPR operand even
    // where divergent code around the call hides that from the compiler
    const uint32_t lds = __builtin_amdgcn_readfirstlane(lds_any);
#define FATTN_DMA_ASM(INSN, MOD)                                                                          \
    asm volatile("s_nop %3\n\t" INSN " %0, %1, 0 offen" MOD : : "v"(off), "s"(srd), "{m0}"(lds), "n"(PAD) \
                 : "memory")
    if constexpr (BYTES == 16 && NT) FATTN_DMA_ASM("buffer_load_dwordx4", " nt lds");
    else if constexpr (BYTES == 16) FATTN_DMA_ASM("buffer_load_dwordx4", " lds");
    else if constexpr (NT) FATTN_DMA_ASM("buffer_load_dword", " nt lds");
    else FATTN_DMA_ASM("buffer_load_dword", " lds");
#undef FATTN_DMA_ASM
}

struct StepSrc {
    i32x4 k, v, m;
    int mh0, mhn;  // split kernel, head planes: the tile's first q head and its head count (mask_row_off)
    int mrows;     // split kernel, 16-B path: staged mask rows that are requested
};

// ---------------------------------------------------------------- arrivals
// The chunks of a tile meet through one 64-bit arrival word per tile,
// [0xFF | launch epoch : 32 | generation : 8 | arrivals : 16].  Each arriving
// lane first stamps the word with its launch's tag and epoch (atomic max, no
// return; the split kernel issues it right after its prologue's DMA, off every
// critical path): a word left by an earlier launch (re-armed or, after an
// aborted launch, mid-count) or never zeroed (top 8 bits not all ones) is
// superseded and the count restarts at 0.  The last arriver re-arms the word
// (count 0, same epoch, generation + 1), so a replayed graph finds it clean;
// workgroups that wait for a tile's arrivals (bd_tile_merge) watch for the
// count to complete or the generation to move.
// Launches sharing one workspace must be stream-ordered.
constexpr uint64_t kArrivalTag = 0xFFull << 56;
constexpr int kArrivalEpochShift = 24;

__device__ __forceinline__ uint64_t* arrival_word(const SplitArgs& a, int64_t tile) {
    return (uint64_t*)(a.ws_cnt + tile * kCntStride);
}

// by the lane that later calls arrive_last, before it (same-lane order)
__device__ __forceinline__ void arrival_begin(const SplitArgs& a, int64_t tile) {
    (void)__hip_atomic_fetch_max(arrival_word(a, tile), a.arrival_stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane: count this arrival; true for the tile's n-th (last) arriver,
// which re-arms the word
__device__ __forceinline__ bool arrive_last(const SplitArgs& a, int64_t tile, int n) {
    uint64_t* w = arrival_word(a, tile);
    const uint64_t old = __hip_atomic_fetch_add(w, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (old & 0xFFFF) == (uint64_t)(n - 1);
    if (last) {
        const uint64_t gen = ((old >> 16) + 1) & 0xFF;
        __hip_atomic_store(w, (old & ~0xFFFFFFull) | gen << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return last;
}

// In-kernel chunk merge (SplitArgs::merge_launch == 2, every workgroup of the
// grid co-resident): one lane per workgroup, after every storing wave stored
// its partials sc1 and drained and the workgroup met at a barrier, counts the
// workgroup on the tile's arrival word (stamped in the prologue).  The last
// arriver re-arms the word (count 0, generation + 1) and returns at once; the
// others poll it (sc1 loads, relaxed) until the count is complete or the
// generation has moved.  Then every workgroup of the tile may load the tile's
// partials with sc1 loads, the other waves behind a barrier
// (MI355X_MICROARCH.md, inter-workgroup visibility, first row of the sc1
// table).  Returns 0 only when the bounded poll gave up (a fault: the caller
// writes NaN rows instead of merging).
__device__ __forceinline__ int tile_arrive_wait(const SplitArgs& a, int64_t tile, int n) {
    uint64_t* w = arrival_word(a, tile);
    const uint64_t old = __hip_atomic_fetch_add(w, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t gen = (uint32_t)(old >> 16) & 0xFFu;
    if ((int)(old & 0xFFFF) == n - 1) {
        __hip_atomic_store(w, (old & ~0xFFFFFFull) | (uint64_t)((gen + 1) & 0xFFu) << 16, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        return 1;
    }
    for (uint32_t spins = 0; spins < (1u << 20); spins++) {
        const uint32_t lo = ld_sc1_u32((const uint32_t*)w);
        if (((lo >> 16) & 0xFFu) != gen || (int)(lo & 0xFFFF) >= n) return 1;
        __builtin_amdgcn_s_sleep(2);
    }
    return 0;
}

// ---------------------------------------------------------------- mask planes
__device__ __forceinline__ int div_R(const SplitArgs& a, int m);

// base of the sequence plane that the workgroup's iq3 reads (the query's
// sequence, not the KV's: sequences that share one KV may differ in mask)
__device__ __forceinline__ const uint8_t* mask_seq_base(const SplitArgs& a, int iq3) {
    return a.m_ne3 == 1 ? a.mask : a.mask + (int64_t)(iq3 % a.m_ne3) * a.m_nb3;
}

// byte offset of q head iq2's plane, (iq2 % m_ne2) * m_nb2, without a runtime
// division: the quotient by float, at most one off (iq2 < 2^24), then corrected
__device__ __forceinline__ uint32_t mask_head_off(const SplitArgs& a, int iq2) {
    if (a.m_ne2 == 1) return 0u;
    int r = iq2 - (int)(((float)iq2 + 0.5f) * a.m_ne2_inv) * a.m_ne2;
    r = r < 0 ? r + a.m_ne2 : r >= a.m_ne2 ? r - a.m_ne2 : r;
    return (uint32_t)r * (uint32_t)a.m_nb2;
}

// ---------------------------------------------------------------- tile geometry
// A tile packs rows m = (query row m / R, head m % R).  No runtime integer
// division (hipcc expands those into long scalar loops).
__device__ __forceinline__ int div_R(const SplitArgs& a, int m) { return (int)(((float)m + 0.5f) * a.R_inv); }

// number of valid rows of tile (qt, hs); they form a prefix [0, rv)
__device__ __forceinline__ int tile_rows(const SplitArgs& a, int qt, int hs) {
    const int rows_q = min(a.QPT, a.NQ - qt * a.QPT);
    const int heads = min(a.R, a.rk2 - hs * a.R);
    return rows_q * heads;  // heads < R only when R == 16 (then QPT == 1)
}

// Tile y of a sequence -> (query-row tile qt, head subgroup hs, kv head ik2) and
// the sequence's kv sequence: y = qt + n_qt * (hs + n_hsub * ik2), ik3 = iq3 / rk3.
// HSUB = false: the kernels whose plans pack whole head groups (R = rk2,
// n_hsub == 1) leave the head subgroup out of the arithmetic; hs = 0.
// (Results through references, not a struct: returned as a struct, the MLA
// kernel's register allocation moved and one form spilled 20 B to scratch.)
template <bool HSUB>
__device__ __forceinline__ void tile_decode(const SplitArgs& a, int y, int iq3, int& qt, int& hs, int& ik2, int& ik3) {
    qt = 0, hs = 0, ik2 = y, ik3 = iq3;  // common case without runtime division
    if constexpr (HSUB) {
        if (a.n_qt != 1 || a.n_hsub != 1) {
            qt = y % a.n_qt;
            hs = (y / a.n_qt) % a.n_hsub;
            ik2 = y / (a.n_qt * a.n_hsub);
        }
    } else {
        if (a.n_qt != 1) {
            qt = y % a.n_qt;
            ik2 = y / a.n_qt;
        }
    }
    if (a.rk3 != 1) ik3 = iq3 / a.rk3;
}

// the K, V and mask descriptors of kv head ik2 of kv sequence ik3 and of the
// mask's sequence plane of iq3 (v_span: MLA's V as a view of K passes 0)
template <bool HM>
__device__ __forceinline__ StepSrc kv_sources(const SplitArgs& a, int ik2, int ik3, int iq3, uint32_t v_span) {
    StepSrc rs;
    rs.k = make_srd(a.k + (int64_t)ik2 * a.k_nb2 + (int64_t)ik3 * a.k_nb3, a.k_span);
    rs.v = make_srd(a.v + (int64_t)ik2 * a.v_nb2 + (int64_t)ik3 * a.v_nb3, v_span);
    rs.m = make_srd(mask_seq_base(a, iq3), HM ? a.m_span_h : 0);
    return rs;
}
template <bool HM>
__device__ __forceinline__ StepSrc kv_sources(const SplitArgs& a, int ik2, int ik3, int iq3) {
    return kv_sources<HM>(a, ik2, ik3, iq3, a.v_span);
}

// ---------------------------------------------------------------- diagnostics
// Diagnostic build only (-DFATTN_STAMPS, libfattn_stamps.so, tools/stamps.py):
// lane 0 of every wave records s_memrealtime (100 MHz) at phase boundaries into
// g_stamps[block][16 wave slots][16]: 0 start, 1 first steps issued, 2+s data of
// step s in LDS (s < 8), 10 loop done, 11 waves merged (LDS), 12 partial
// published and drained, 14 arrival atomic returned, 15 merger's loads in,
// 13 tile merged and stored (merging wave).  No stamp executes in the product
// library.
#ifdef FATTN_STAMPS
static __device__ unsigned long long* g_stamps;  // one per translation unit (fattn_launch_d*.hip)
#define FATTN_STAMP(k)                                                                          \
    do {                                                                                        \
        if (lane == 0 && g_stamps) {                                                            \
            const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                     \
            const int64_t blk_ = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; \
            g_stamps[(blk_ * 16 + wave) * 16 + (k)] = t_;                                \
        }                                                                                       \
    } while (0)
// any lane: slot k of wave 0's record = max(slot, v)
#define FATTN_STAMP_MAX(k, v)                                                                   \
    do {                                                                                        \
        if (g_stamps) {                                                                         \
            const int64_t blk_ = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; \
            atomicMax(&g_stamps[blk_ * 16 * 16 + (k)], (unsigned long long)(v));      \
        }                                                                                       \
    } while (0)
// The split kernel keeps its stamps in LDS (a static array) and each wave
// stores its own at the kernel's end (FATTN_SSTAMP_FLUSH): a global store per
// stamp would be counted by vmcnt and every counted wait would wait for it
// too, stretching the very timeline it measures (round 3's stamps: a 17 us
// span for an 11 us launch).
__device__ __forceinline__ unsigned long long* split_stamp_slots() {
    __shared__ unsigned long long s[16 * 16];
    return s;
}
#define FATTN_SSTAMP(k)                                                                          \
    do {                                                                                         \
        if (lane == 0) split_stamp_slots()[wave * 16 + (k)] = __builtin_amdgcn_s_memrealtime();  \
    } while (0)
#define FATTN_SSTAMP_INIT()                                                                      \
    do {                                                                                         \
        if (lane < 16) split_stamp_slots()[wave * 16 + lane] = 0ull;                             \
    } while (0)
#define FATTN_SSTAMP_FLUSH()                                                                     \
    do {                                                                                         \
        if (lane < 16 && g_stamps) {                                                             \
            const int64_t blk_ = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; \
            g_stamps[(blk_ * 16 + wave) * 16 + lane] = split_stamp_slots()[wave * 16 + lane];    \
        }                                                                                        \
    } while (0)
#else
#define FATTN_STAMP(k) do { } while (0)
#define FATTN_STAMP_MAX(k, v) do { } while (0)
#define FATTN_SSTAMP(k) do { } while (0)
#define FATTN_SSTAMP_INIT() do { } while (0)
#define FATTN_SSTAMP_FLUSH() do { } while (0)
#endif

// ---------------------------------------------------------------- workgroup order
// workgroup -> (KV chunk, tile y, sequence iq3).  Blocks are dealt round-robin
// over the 8 XCDs (MI355X_MICROARCH.md, workgroup dispatch: observed placement,
// used for speed only), so in the plain order the chunks of one kv head sit on
// 8 different L2s (batched decode: each fetches the head's Q rows, 32 KB f32,
// from HBM; split kernel: the tile's chunk partials cross XCDs).  The
// XCD-grouped order (a.xcd_group) gives each XCD whole tiles -- all their
// chunks.  Any bijection is correct; the planner sets xcd_group only for
// grids of a multiple of 8 workgroups.
__device__ __forceinline__ void tile_coords(const SplitArgs& a, int& chunk, int& y, int& iq3) {
    chunk = blockIdx.x;
    y = blockIdx.y;
    iq3 = blockIdx.z;
    if (a.xcd_group) {
        const uint32_t gx = gridDim.x, gy = gridDim.y;
        const uint32_t G = gx * gy * gridDim.z;
        const uint32_t L = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const uint32_t L2 = (L % 8) * (G / 8) + L / 8;
        chunk = (int)(L2 % gx);
        y = (int)((L2 / gx) % gy);
        iq3 = (int)(L2 / (gx * gy));
    }
}

// ---------------------------------------------------------------- chunk merge (one row, one wave)
// Log-sum-exp merge of NP <= 64 one-row partials of a tile: O rows [NP][D]
// f32 and (m in log2 units, l) pairs [NP][2], written write-through by other
// workgroups of this launch (sc1 loads: first row of the hand-off table,
// MI355X_MICROARCH.md).  One wave: lane (h, dl) = (lane / (D/4), lane % (D/4))
// loads 16 B of every part p = h (mod 64 / (D/4)); every load of a batch is
// issued before one wait; the lane groups meet by permlane swaps.  Fixed
// order (deterministic).  `out` = the tile's dst row.  fa_reduce math,
// src/flash_row_float.h:415-472, in fp32.
template <int D>
constexpr int merge_ppr() { return 64 % (D / 4) == 0 ? 64 / (D / 4) : 1; }  // parts per lane row (4, 2, 1)

// `sink_of()`: the address of the row's q head's sink (SplitArgs::sinks), or
// null: no sinks.  A callable, so that it is evaluated where the row is
// normalised and the pointer is not held across the loads above it.
struct NoSink {
    __device__ __forceinline__ const float* operator()() const { return nullptr; }
};
template <int D, int kIt = 16, int AUX = kAuxSc1, typename SinkOf = NoSink>  // kIt: loads per lane per round trip; AUX: the loads' cache bits
__device__ __forceinline__ void merge_row_parts(const float* parts_o, const float* parts_ml, int NP, float* out,
                                                int lane, int ostride = D, int mstride = 2, SinkOf sink_of = SinkOf(),
                                                float* lse_row = nullptr) {
    constexpr float kNegInf = -__builtin_inff();
    constexpr int LPP = D / 4;              // lanes per part
    constexpr int PPR = merge_ppr<D>();     // D = 80 / 96: 1
    const int h = lane / LPP, d4 = 4 * (lane % LPP);
    // (part p's O row at p * ostride floats, its (m, l) at p * mstride)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the loads below the count)
    const __amdgpu_buffer_rsrc_t osrd = make_rsrc(parts_o, (uint32_t)(NP * ostride * 4));
    const __amdgpu_buffer_rsrc_t msrd = make_rsrc(parts_ml, (uint32_t)(NP * mstride * 4));
    u32x4 v[kIt];
    auto issue = [&](int p0) {
#pragma unroll
        for (int i = 0; i < kIt; i++)
            v[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 osrd, (uint32_t)(((p0 + PPR * i + h) * ostride + d4) * 4), 0, AUX));
    };
    issue(0);
    const uint32_t mlm = __builtin_amdgcn_raw_buffer_load_b32(msrd, (uint32_t)(lane * mstride * 4), 0, AUX);  // lane p: m of part p
    const uint32_t mll = __builtin_amdgcn_raw_buffer_load_b32(msrd, (uint32_t)(lane * mstride * 4 + 4), 0, AUX);  // l of part p
    const float mp = lane < NP ? __builtin_bit_cast(float, mlm) : kNegInf;
    const float M = seg_reduce<true>(mp, 64);
    const float w = (mp == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(mp - M);
    const float L = seg_reduce<false>(lane < NP ? w * __builtin_bit_cast(float, mll) : 0.0f, 64);
    const int wi = __builtin_bit_cast(int, w);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p0 = 0; p0 < NP; p0 += kIt * PPR) {  // wave-uniform
        if (p0 > 0) issue(p0);
#pragma unroll
        for (int i = 0; i < kIt; i++) {
            float wp = 0.0f;
#pragma unroll
            for (int j = 0; j < PPR; j++) {
                const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, (p0 + PPR * i + j) & 63));
                wp = (h == j) ? wj : wp;
            }
            acc += wp * __builtin_bit_cast(f32x4, v[i]);
        }
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
    if (h) return;
    const float* sink = sink_of();
    if (sink) {  // (wave-uniform)
        bool dead;
        const float inv = sink_inv(M, L, *sink, dead);
        *(f32x4*)(out + d4) = sink_row(acc, inv, dead);
    } else {
        const float inv = L == 0.0f ? __builtin_nanf("") : 1.0f / L;  // L == 0 (row fully masked) -> NaN like the reference
        *(f32x4*)(out + d4) = acc * inv;
    }
    // (wave-uniform) `lse_row`: the row's entry of SplitArgsLse::lse, or null
    if (lse_row && lane == 0) *lse_row = row_lse(M, L, sink ? *sink : kNegInf, row_dead(M, L));
}

// f16 chunk partials (SplitArgs::part_f16, second-launch merges): the
// partial's EPT dims of O / l rounded to f16 -- bounded by max |v|, where the
// unnormalised O is not -- (a fully masked chunk, l = 0, stores zeros: its
// merge weight is 0); the (m, l) pair stays f32.  Plain stores: the kernel
// boundary orders them before the merge launch's loads.
template <int EPT>
__device__ __forceinline__ void store_part_f16(uint16_t* dst, const float (&acc)[EPT], float L) {
    static_assert(EPT % 4 == 0, "");
    const float inv = L > 0.0f ? 1.0f / L : 0.0f;
    uint32_t w[EPT / 2];
#pragma unroll
    for (int e = 0; e < EPT; e += 2) {
        const f16x2 hp = {(_Float16)(acc[e] * inv), (_Float16)(acc[e + 1] * inv)};
        w[e / 2] = __builtin_bit_cast(uint32_t, hp);
    }
    // (16-B stores when EPT is a multiple of 8 -- dst is then 16-B aligned --,
    // else 8-B ones: the batched-decode epilogue's 12 dims at D = 96)
    if constexpr (EPT % 8 == 0) {
#pragma unroll
        for (int e = 0; e < EPT / 2; e += 4) *(u32x4*)(dst + 2 * e) = u32x4{w[e], w[e + 1], w[e + 2], w[e + 3]};
    } else {
#pragma unroll
        for (int e = 0; e < EPT / 2; e += 2) *(u32x2*)(dst + 2 * e) = u32x2{w[e], w[e + 1]};
    }
}

// The merge of NP f16 partials of one row (merge_row_parts' fa_reduce LSE
// merge, src/flash_row_float.h:415-472, in fp32, fixed order): lane (h, dl) =
// (lane / (D/8), lane % (D/8)) loads 16 B = 8 dims of every part p = h (mod
// 64 / (D/8)); part p weighs w_p l_p, w_p = 2^(m_p - M), and the row is
// sum_p w_p l_p O~_p / sum_p w_p l_p.  Plain loads (a second launch).  D = 80,
// 96, 128, 256 (D = 64 keeps f32 partials: 8 parts per lane row would need a
// third lane-swap level).
template <int D>
constexpr int merge_ppr_h() { return 64 % (D / 8) == 0 ? 64 / (D / 8) : 1; }  // (4, 2, 1)
template <int D, int kIt, typename SinkOf = NoSink>
__device__ __forceinline__ void merge_row_parts_h(const uint16_t* parts_o, const float* parts_ml, int NP, float* out,
                                                  int lane, int ostride, int mstride, SinkOf sink_of = SinkOf(),
                                                  float* lse_row = nullptr) {
    constexpr float kNegInf = -__builtin_inff();
    constexpr int LPP = D / 8;
    constexpr int PPR = merge_ppr_h<D>();
    static_assert(PPR == 1 || PPR == 2 || PPR == 4, "");
    const int h = lane / LPP, d8 = 8 * (lane % LPP);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the loads below the count)
    const __amdgpu_buffer_rsrc_t osrd = make_rsrc(parts_o, (uint32_t)(NP * ostride * 2));
    const __amdgpu_buffer_rsrc_t msrd = make_rsrc(parts_ml, (uint32_t)(NP * mstride * 4));
    u32x4 v[kIt];
    auto issue = [&](int p0) {
#pragma unroll
        for (int i = 0; i < kIt; i++)
            v[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 osrd, (uint32_t)(((p0 + PPR * i + h) * ostride + d8) * 2), 0, 0));
    };
    issue(0);
    const uint32_t mlm = __builtin_amdgcn_raw_buffer_load_b32(msrd, (uint32_t)(lane * mstride * 4), 0, 0);
    const uint32_t mll = __builtin_amdgcn_raw_buffer_load_b32(msrd, (uint32_t)(lane * mstride * 4 + 4), 0, 0);
    const float mp = lane < NP ? __builtin_bit_cast(float, mlm) : kNegInf;
    const float M = seg_reduce<true>(mp, 64);
    const float w = (mp == kNegInf) ? 0.0f : __builtin_amdgcn_exp2f(mp - M) * __builtin_bit_cast(float, mll);
    const float L = seg_reduce<false>(lane < NP ? w : 0.0f, 64);
    const int wi = __builtin_bit_cast(int, w);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.0f;
    for (int p0 = 0; p0 < NP; p0 += kIt * PPR) {  // wave-uniform
        if (p0 > 0) issue(p0);
#pragma unroll
        for (int i = 0; i < kIt; i++) {
            float wp = 0.0f;
#pragma unroll
            for (int j = 0; j < PPR; j++) {
                const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(wi, (p0 + PPR * i + j) & 63));
                wp = (h == j) ? wj : wp;
            }
            const f16x8 x = __builtin_bit_cast(f16x8, v[i]);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += wp * (float)x[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        if constexpr (PPR == 4) acc[e] = xor16_pair(acc[e], false);
        if constexpr (PPR >= 2) acc[e] = xor32_pair(acc[e], false);
    }
    if (h) return;
    const float* sink = sink_of();
    if (sink) {  // (wave-uniform; L = sum_p w_p l_p is the row's whole sum at reference M)
        bool dead;
        const float inv = sink_inv(M, L, *sink, dead);
        *(f32x4*)(out + d8) = sink_row(f32x4{acc[0], acc[1], acc[2], acc[3]}, inv, dead);
        *(f32x4*)(out + d8 + 4) = sink_row(f32x4{acc[4], acc[5], acc[6], acc[7]}, inv, dead);
    } else {
        const float inv = L == 0.0f ? __builtin_nanf("") : 1.0f / L;  // L == 0 (row fully masked) -> NaN like the reference
        *(f32x4*)(out + d8) = f32x4{acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv};
        *(f32x4*)(out + d8 + 4) = f32x4{acc[4] * inv, acc[5] * inv, acc[6] * inv, acc[7] * inv};
    }
    if (lse_row && lane == 0) *lse_row = row_lse(M, L, sink ? *sink : kNegInf, row_dead(M, L));
}

// ---------------------------------------------------------------- merge launch
// Second launch of a plan whose multi-row tiles are split over KV chunks
// (SplitArgs::merge_launch == 1): one wave per (tile, packed row) merges the
// row's chunk partials (merge_row_parts: the fa_reduce LSE merge of
// src/flash_row_float.h:415-472 in fp32, fixed order) and writes the normalised
// dst row.  The last-arriver form (combine_tile) pulls a whole tile's 16 rows x
// chunks into ONE workgroup (config 5 shard: 128 KB, 6.4 us of a 14.7 us
// launch); here the same bytes spread over (tiles x rows) waves, and the kernel
// boundary replaces drain + counter.
// Geom: what the kernel families' partial layouts differ in.  The partial of
// chunk c of row r of slot block b sits at slot (b * n_chunks + c) * rows + r;
// grid.y runs over the slot blocks, b = tile y * subs + sub, grid.x * 4 over r.
struct MergeGeomBase {
    static constexpr int subs = 1;      // slot blocks (subtiles of `rows` packed rows) per tile
    static constexpr bool sc1 = true;   // has the form that loads the partials sc1 ...
    static constexpr bool plain = true; // ... the plain-load form (FATTN_OPT_MERGE_PLAIN; MLA: its only one) ...
    static constexpr bool f16 = true;   // ... and the f16-partial form (SplitArgs::part_f16; never at D = 64)
    static constexpr int min_kit = 2;   // fewest load slots per lane (launch_chunk_merge)
};
// each family's header states its own: static constexpr int rows (packed rows
// per slot block) and bool hsub (its tiles have head subgroups: tile_decode)

// D: dst's row length; rows wider than 256 columns -- the widest row one wave
// of merge_row_parts covers -- go as 256-column parts, each reducing the
// (m, l) pairs anew (MLA: 512).  KIT: loads per lane per round trip, >= the
// tile's chunks / merge_ppr<D>() when possible.  PLAIN: the partials read with
// plain loads instead of sc1 (the kernel boundary already made the stores
// visible).  F16: the f16 partials of SplitArgs::part_f16 (merge_row_parts_h,
// plain loads).
constexpr int merge_span(int D) { return D > 256 ? 256 : D; }
template <typename Geom, int D, int KIT, bool PLAIN, bool F16, typename A = SplitArgs>
__global__ __launch_bounds__(256) void fattn_chunk_merge_kernel(const A a) {
    constexpr int W = merge_span(D);
    static_assert(D % W == 0 && (W == D || !F16), "");
    const int lane = threadIdx.x & 63;
    const int tm = blockIdx.x * 4 + (threadIdx.x >> 6);  // row of the slot block
    const int ys = blockIdx.y, iq3 = blockIdx.z;
    int y = ys, p = tm;  // tile, packed row of the tile
    if constexpr (Geom::subs != 1) y = ys / Geom::subs, p = Geom::rows * (ys % Geom::subs) + tm;
    int qt, hs, ik2, ik3;
    tile_decode<Geom::hsub>(a, y, iq3, qt, hs, ik2, ik3);
    // the tile's valid rows, a prefix (no head subgroups: whole head groups, R = rk2)
    if (p >= (Geom::hsub ? tile_rows(a, qt, hs) : min(a.QPT, a.NQ - qt * a.QPT) * a.R)) return;
    const int64_t slot0 = ((int64_t)iq3 * gridDim.y + ys) * a.n_chunks * Geom::rows + tm;  // chunk 0's row
    const int rq = div_R(a, p);
    const int riq2 = ik2 * a.rk2 + hs * a.R + (p - rq * a.R);
    const int64_t row = ((int64_t)iq3 * a.NQ + qt * a.QPT + rq) * a.H + riq2;  // dst's row, lse's entry
    float* out = a.dst + row * D;
    auto sink = [&]() -> const float* { return a.sinks ? a.sinks + riq2 : nullptr; };  // (one row, one head per wave)
    float* lse_row = lse_at(a, row);  // (wave-uniform; a constant null without lse)
    if constexpr (F16) {
        merge_row_parts_h<D, KIT>((const uint16_t*)a.ws_o + slot0 * D, a.ws_ml + 2 * slot0, a.n_chunks, out, lane,
                                  Geom::rows * D, 2 * Geom::rows, sink, lse_row);
    } else {
#pragma unroll
        for (int c = 0; c < D; c += W)  // (rows of several spans: the first one writes the row's lse)
            merge_row_parts<W, KIT, PLAIN ? 0 : kAuxSc1>(a.ws_o + slot0 * D + c, a.ws_ml + 2 * slot0, a.n_chunks, out + c,
                                                        lane, Geom::rows * D, 2 * Geom::rows, sink, c == 0 ? lse_row : nullptr);
    }
}

}  // namespace fattn
