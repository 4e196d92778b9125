// fattn_launch.h -- the launch plan and the kernel launchers, shared by the
// planner (fattn_plan.h), the C ABI (fattn_api.hip) and the per-head-dim translation units
// (fattn_launch_d*.hip: each instantiates launch_types<D>, so the kernels of
// the head dims compile in parallel).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "fattn_quant.h"
#include "fattn_mq.h"
#include "fattn_pf.h"
#include "fattn_pf4.h"
#include "fattn_bd.h"
#include "fattn_bdp.h"
#include "fattn_split.h"
#include "fattn_mla.h"

namespace fattn {

constexpr int kMaxDevices = 64;

// the kernel a plan launches (one of them: the planner's choose_kernel and sizing)
enum class Kernel {
    Split,    // split-KV kernel (fattn_split.h): every wave issues its own steps
    SplitLd,  // ... with kSplitLoaders loader waves beside the compute waves (fattn_split_ld_kernel)
    Mq,       // multi-query kernel (fattn_mq.h)
    Pf,       // prefill kernel, the 8-wave body (fattn_pf.h)
    Pf4,      // ... its one-wave-per-SIMD body (fattn_pf4.h; f16 rows, D = 128)
    Bd,       // batched-decode kernel, all waves alike (fattn_bd.h)
    Bdp,      // ... in its compute / build-role form (fattn_bdp.h; Q8_0 / Q4_0)
    Mla,      // MLA kernel (fattn_mla.h): K dim 576, V dim 512; f16, or Q8_0 / Q4_0 with V a view of K
};

// ---------------------------------------------------------------- which kernels exist
// The one statement of the (kernel, K type, V type, head dim) the library
// instantiates: the launchers' `if constexpr` guards, the planner's choice
// (choose_kernel), its LDS sizes (lds_bytes_of) and make_plan's last check all
// read it.  vt may be VT_F16T; Kernel::Mla: D is K's row length.
using HeadDims = ValueList<64, 80, 96, 128, 256>;
using VTypes = ValueList<FATTN_TYPE_F16, FATTN_TYPE_BF16, FATTN_TYPE_Q8_0, FATTN_TYPE_Q4_0, FATTN_TYPE_Q4_1, FATTN_TYPE_Q5_0, FATTN_TYPE_Q5_1, VT_F16T>;  // CacheTypes and the transposed f16 V
// head dims of the split kernel over mixed K / V types and over SplitOnlyTypes
constexpr bool split_dim3(int D) { return D == 64 || D == 128 || D == 256; }
// the split kernel's loader-wave form (fattn_split_ld_kernel): one K / V type of CoreTypes, D = 64 / 128
constexpr bool split_ld_ok(int kt, int vt, int D) { return kt == vt && in_list(CoreTypes(), kt) && (D == 64 || D == 128); }

template <Kernel K>
using KernelC = std::integral_constant<Kernel, K>;

constexpr bool has_kernel(Kernel kern, int kt, int vt, int D) {
    const bool f16 = kt == FATTN_TYPE_F16 && vt == FATTN_TYPE_F16;
    const bool quant = kt == vt && in_list(QuantTypes(), kt);  // Q8_0 / Q4_0: the kernels below the split kernel
    switch (kern) {
        case Kernel::Split:
            if (kt == FATTN_TYPE_F16 && vt == VT_F16T) return in_list(HeadDims(), D);
            if (kt != vt) return in_list(CoreTypes(), kt) && in_list(CoreTypes(), vt) && split_dim3(D);
            if (in_list(SplitOnlyTypes(), kt)) return split_dim3(D);
            return f16 ? in_list(HeadDims(), D) : quant && D != 80 && in_list(HeadDims(), D);  // (80 is not a whole number of ggml blocks)
        case Kernel::SplitLd: return split_ld_ok(kt, vt, D);
        case Kernel::Mq: return quant && split_dim3(D);
        case Kernel::Pf: return (f16 && D == 80) || ((f16 || quant) && (D == 64 || D == 96 || D == 128));
        case Kernel::Pf4: return f16 && D == 128;
        case Kernel::Bd: return (quant && D == 128) || (f16 && (D == 64 || D == 96 || D == 128));  // (Q8_0 / Q4_0: D = 128 only)
        case Kernel::Bdp: return quant && (D == 64 || D == 96 || D == 128);
        case Kernel::Mla: return kt == vt && in_list(CoreTypes(), kt) && D == kMlaDK;
    }
    return false;
}

struct Plan {
    SplitArgs a = {};
    float* lse = nullptr;  // fattn_ext_lse's pointer (launch_ext sets it; no part of the plan): which kernels launch, with_args

    Kernel kernel = Kernel::Split;
    int kt = 0, vt = 0;  // vt may be VT_F16T
    int D = 0;           // head dim (Kernel::Mla: K's, 576)
    int DV = 0;          // Kernel::Mla: V's row length, 512 -- dst's last dim (0 on every other plan: D)
    int mla_v_off = -1;  // Kernel::Mla: V is a view of K, this many bytes into each row (Q8_0 / Q4_0: whole blocks); -1: V of its own
    // Kernel::Mla over Q8_0 / Q4_0: no tile has more than one wave's 16 rows -- wave 0 computes, waves 1 - 3 load
    // and convert (fattn_mla_kernel's SOLO); ... and the rows are contiguous on 16-B aligned planes (16-B pieces)
    bool mla_solo = false, mla_raw16 = false;
    int gran = 0;
    dim3 grid;
    int lds = 0;
    size_t ws_bytes = 0, cnt_bytes = 0, ml_bytes = 0;
    int cus = 0;  // compute units of the device the plan is for
    int nwv = 0;  // split kernel: waves per workgroup (4, 8, 16)
    int nw = 0;   // mq kernel: waves per workgroup: 4 (16 rows each) or 8 (32 rows each)
    bool merge_plain = false;  // second-launch merges (split, batched decode): plain loads (FATTN_OPT_MERGE_PLAIN)
    bool pf_flags = false;  // masked prefill: live-block flags pre-pass (tile-range skipping)
    int pf4_sched = 0;      // Kernel::Pf4: its schedule (fattn_pf4_kernel's SCHED)
    // prefill over Q8_0 / Q4_0: the rows staged to f16 in the workspace first
    // (kv_stage_f16_kernel), then the f16 prefill kernel (kt = vt = F16 then)
    bool pf_stage = false;
    int stage_kt = 0;                                  // the cache's type
    const uint8_t *stage_k = nullptr, *stage_v = nullptr;  // the cache's K / V
    int64_t stage_k_nb2 = 0, stage_k_nb3 = 0, stage_v_nb2 = 0, stage_v_nb3 = 0;
    int stage_hkv = 0, stage_skv = 0;
    size_t stage_off = 0, stage_bytes = 0;             // per K (or V): Skv * Hkv * N * D * 2
};

// Every kernel that normalises into dst exists over SplitArgs and over
// SplitArgsLse (fattn_tile.h): go(type tag) launches the former, or with
// pl.lse the latter -- the kernels that also store the rows' log-sum-exp.
template <typename T>
struct ArgsTag {
    using type = T;
};
template <typename A>
A launch_args(const Plan& pl) {
    A a;
    static_cast<SplitArgs&>(a) = pl.a;
    if constexpr (std::is_same<A, SplitArgsLse>::value) a.lse = pl.lse;
    return a;
}
template <typename F>
auto with_args(const Plan& pl, F&& go) {
    return pl.lse ? go(ArgsTag<SplitArgsLse>()) : go(ArgsTag<SplitArgs>());
}

struct Events {
    hipEvent_t begin = nullptr, end = nullptr;
};

// Launch with errors attributed to this launch only: a pending error left on
// the thread by other code is cleared first; FATTN_DEBUG=1 names a failure.
template <typename F>
int launch_kernel(const void* kern, const Plan& pl, hipStream_t st, const Events& ev, F&& go) {
    (void)hipGetLastError();
    // large dynamic LDS must be allowed per kernel and per device: cached per
    // (launch site = F's instantiation, device); a lost race only repeats the call
    static std::atomic<int> lds_set[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    if (pl.lds > 65536 && pl.lds > lds_set[dev].load(std::memory_order_relaxed)) {
        // the query loads the code object (HIP loads kernels lazily; setting an
        // attribute of a kernel whose module is not loaded yet fails)
        hipFuncAttributes fa;
        (void)hipFuncGetAttributes(&fa, kern);
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds) == hipSuccess) {
            lds_set[dev].store(pl.lds, std::memory_order_relaxed);
        } else if (std::getenv("FATTN_DEBUG")) {
            std::fprintf(stderr, "fattn: hipFuncSetAttribute(%d B LDS) failed; launching anyway\n", pl.lds);
        }
        (void)hipGetLastError();
    }
    if (ev.begin) (void)hipEventRecord(ev.begin, st);
    go();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (std::getenv("FATTN_DEBUG"))
            std::fprintf(stderr, "fattn: launch grid (%u,%u,%u) lds %d failed: %s\n", pl.grid.x, pl.grid.y, pl.grid.z,
                         pl.lds, hipGetErrorString(e));
        return FATTN_ERR_LAUNCH;
    }
    if (ev.end) (void)hipEventRecord(ev.end, st);
    return FATTN_OK;
}

// Merge the chunk partials in a second launch (fattn_chunk_merge_kernel over the
// kernel family's Geom), one wave per packed row, with as few load slots per
// lane (KIT) as the chunk count allows (the slots past it still cost issue
// cycles); f16 partials (16-B loads of 8 dims, merge_ppr_h parts per lane row;
// not at D = 64), else sc1 or plain loads of f32 ones -- of these forms, the
// ones the Geom has.
template <typename Geom, int D>
void launch_chunk_merge(dim3 grid, const Plan& pl, hipStream_t st) {
    auto pick = [&](int parts_per_row, auto plain, auto f16) {
        constexpr bool PLAIN = decltype(plain)::value, F16 = decltype(f16)::value;
        const int need = (pl.a.n_chunks + parts_per_row - 1) / parts_per_row;
        auto go = [&](auto kit) {
            with_args(pl, [&](auto tag) {
                using A = typename decltype(tag)::type;
                hipLaunchKernelGGL((fattn_chunk_merge_kernel<Geom, D, decltype(kit)::value, PLAIN, F16, A>), grid, dim3(256), 0, st,
                                   launch_args<A>(pl));
                return 0;
            });
        };
        if constexpr (Geom::min_kit <= 2) {
            if (need <= 2) return go(std::integral_constant<int, 2>());
        }
        if (need <= 4) go(std::integral_constant<int, 4>());
        else if (need <= 8) go(std::integral_constant<int, 8>());
        else go(std::integral_constant<int, 16>());
    };
    constexpr int ppr = merge_ppr<merge_span(D)>();
    if constexpr (Geom::f16 && D != 64) {
        if (pl.a.part_f16) return pick(merge_ppr_h<D>(), std::false_type(), std::true_type());
    }
    if constexpr (Geom::plain) {
        if (!Geom::sc1 || pl.merge_plain) return pick(ppr, std::true_type(), std::false_type());
    }
    if constexpr (Geom::sc1) pick(ppr, std::false_type(), std::false_type());
}

template <int KT, int VT, int D, int GRAN, bool HM, int NWV, int EPI, typename A>
int launch_split_a(const Plan& pl, hipStream_t st, const Events& ev) {
    if (pl.kernel == Kernel::SplitLd) {
        if constexpr (GRAN == 16 && NWV == 8 && EPI == 2 && split_ld_ok(KT, VT, D)) {
            auto lk = fattn_split_ld_kernel<KT, VT, D, HM, NWV, kSplitLoaders, A>;
            return launch_kernel((const void*)lk, pl, st, ev, [&] {
                hipLaunchKernelGGL(lk, pl.grid, dim3((NWV + kSplitLoaders) * kWave), pl.lds, st, launch_args<A>(pl));
            });
        }
        return FATTN_ERR_INVALID_ARG;
    }
    void (*kern)(A) = fattn_split_kernel<KT, VT, D, GRAN, HM, NWV, EPI, false, A>;
    // max_bias / logit_softcap live: the bodies with the score transform, which
    // exist for 4 waves (the planner sizes such a launch so: size_split)
    if (pl.a.xf.live) {
        if constexpr (NWV == 4) kern = fattn_split_kernel<KT, VT, D, GRAN, HM, NWV, EPI, true, A>;
        else return FATTN_ERR_INVALID_ARG;
    }
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(NWV * kWave), pl.lds, st, launch_args<A>(pl));
        if constexpr (EPI == 0) {
            // multi-row tiles: the chunk partials merge in a second launch --
            // unless they merge in-kernel (2)
            if (pl.a.merge_launch == 1) {
                // one wave per packed row a tile can hold: R heads x the query
                // rows it really has (config 4's 4-row GQA tiles, QPT 4 but one
                // query row: one workgroup per tile, not four)
                const int qrows = pl.a.QPT < pl.a.NQ ? pl.a.QPT : pl.a.NQ;
                const int rows = qrows * pl.a.R < kRows ? qrows * pl.a.R : kRows;
                launch_chunk_merge<SplitMergeGeom, D>(dim3((unsigned)((rows + 3) / 4), pl.grid.y, pl.grid.z), pl, st);
            }
        }
    });
}

template <int KT, int VT, int D, int GRAN, bool HM, int NWV, int EPI>
int launch_split_e(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_split_a<KT, VT, D, GRAN, HM, NWV, EPI, typename decltype(tag)::type>(pl, st, ev); });
}

// the plan's epilogue (a.wave_merge): 1 only for 4 waves at D = 128
template <int KT, int VT, int D, int GRAN, bool HM, int NWV>
int launch_split_w(const Plan& pl, hipStream_t st, const Events& ev) {
    if constexpr (NWV == 4 && D == 128) {
        if (pl.a.wave_merge == 1) return launch_split_e<KT, VT, D, GRAN, HM, NWV, 1>(pl, st, ev);
    }
    if (pl.a.wave_merge == 2) return launch_split_e<KT, VT, D, GRAN, HM, NWV, 2>(pl, st, ev);
    if (pl.a.wave_merge != 0) return FATTN_ERR_INVALID_ARG;
    return launch_split_e<KT, VT, D, GRAN, HM, NWV, 0>(pl, st, ev);
}

// 8 / 16 waves per workgroup: the 16-B path only; 16 needs the 4-waves-per-SIMD
// register budget (split_waves_per_simd); the planner never asks otherwise
template <int KT, int VT, int D, int GRAN, bool HM>
int launch_split_hm(const Plan& pl, hipStream_t st, const Events& ev) {
    if constexpr (GRAN == 16) {
        if (pl.nwv == 8) return launch_split_w<KT, VT, D, GRAN, HM, 8>(pl, st, ev);
        if constexpr (split_waves_per_simd<KT, D, GRAN>() == 4) {
            if (pl.nwv == 16) return launch_split_w<KT, VT, D, GRAN, HM, 16>(pl, st, ev);
        }
    }
    if (pl.nwv != 4) return FATTN_ERR_INVALID_ARG;
    return launch_split_w<KT, VT, D, GRAN, HM, 4>(pl, st, ev);
}

template <int KT, int VT, int D, int GRAN>
int launch_split(const Plan& pl, hipStream_t st, const Events& ev) {
    return pl.a.has_mask ? launch_split_hm<KT, VT, D, GRAN, true>(pl, st, ev)
                         : launch_split_hm<KT, VT, D, GRAN, false>(pl, st, ev);
}

template <int KT, int VT, int D>
int launch_gran(const Plan& pl, hipStream_t st, const Events& ev) {
    if constexpr (VT == VT_F16T) {
        return launch_split<KT, VT, D, 16>(pl, st, ev);
    } else {
        return pl.gran == 16 ? launch_split<KT, VT, D, 16>(pl, st, ev) : launch_split<KT, VT, D, 4>(pl, st, ev);
    }
}

template <int KT, int D, int NW, bool HM, typename A>
int launch_mq_a(const Plan& pl, hipStream_t st, const Events& ev) {
    auto kern = fattn_mq_kernel<KT, D, NW, HM, A>;
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(NW * kWave), pl.lds, st, launch_args<A>(pl));
        if (pl.a.merge_launch) {
            // the chunk partials of every 16-row subtile (4 per 64-row tile,
            // 16 per 256-row tile) merge in a second launch
            constexpr int SUBS = NW == 8 ? 16 : 4;
            launch_chunk_merge<MqMergeGeom<SUBS>, D>(dim3(kRows / 4, pl.grid.y * SUBS, pl.grid.z), pl, st);
        }
    });
}

template <int KT, int D, int NW, bool HM>
int launch_mq_hm(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_mq_a<KT, D, NW, HM, typename decltype(tag)::type>(pl, st, ev); });
}

template <int KT, int D>
int launch_mq(const Plan& pl, hipStream_t st, const Events& ev) {
    if constexpr (D != 256) {  // D = 256: 64-row workgroups only (LDS)
        if (pl.nw == 8)
            return pl.a.has_mask ? launch_mq_hm<KT, D, 8, true>(pl, st, ev) : launch_mq_hm<KT, D, 8, false>(pl, st, ev);
    }
    return pl.a.has_mask ? launch_mq_hm<KT, D, 4, true>(pl, st, ev) : launch_mq_hm<KT, D, 4, false>(pl, st, ev);
}

// the prefill pre-pass staging a cache of one of `Types` (pf_prepass_kernel<stage_kt>)
template <typename Types>
void launch_prepass(Types, int stage_kt, dim3 grid, hipStream_t st, const PfPrepassArgs& pa) {
    visit(Types(), stage_kt, 0, [&](auto t) {
        hipLaunchKernelGGL(pf_prepass_kernel<decltype(t)::value>, grid, dim3(256), 0, st, pa);
        return 0;
    });
}
// ... of ExtTypes (instantiated in fattn_launch_kv_ext.hip)
void launch_prepass_kv_ext(int stage_kt, dim3 grid, hipStream_t st, const PfPrepassArgs& pa);

template <int KT, int D, bool HM, typename A>
int launch_pf_a(const Plan& pl, hipStream_t st, const Events& ev) {
    // (max_bias / logit_softcap live: the body with the score transform; the
    // planner keeps such launches off the one-wave-per-SIMD bodies)
    void (*kern)(A) = pl.a.xf.live ? fattn_pf_kernel<KT, D, HM, true, A> : fattn_pf_kernel<KT, D, HM, false, A>;
    int waves = kPfWaves;
    if constexpr (has_kernel(Kernel::Pf4, KT, KT, D)) {
        if (pl.kernel == Kernel::Pf4) {
            if (pl.pf4_sched == 4) kern = fattn_pf4_kernel<D, HM, 4, A>;
            else if (pl.pf4_sched == 3) kern = fattn_pf4_kernel<D, HM, 3, A>;
            else kern = fattn_pf4_kernel<D, HM, 2, A>;
            waves = kPf4Waves;
        }
    }
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        // the pre-pass, one launch: the quantised cache's rows -> f16 rows in the
        // workspace (K and V), and the mask's live / +-0 block flags
        bool staged = false;
        if constexpr (KT == FATTN_TYPE_F16 && D % QK == 0) staged = pl.pf_stage;
        const bool flags = HM && pl.a.pf_flags;
        if (staged || flags) {
            PfPrepassArgs pa{};
            pa.nblk = (int64_t)pl.a.N * D / QK;
            pa.per_head = staged ? (int)((4 * pa.nblk + 255) / 256) : 0;
            pa.hkv = pl.stage_hkv, pa.skv = pl.stage_skv;
            pa.k = pl.stage_k, pa.v = pl.stage_v;
            pa.k_nb2 = pl.stage_k_nb2, pa.k_nb3 = pl.stage_k_nb3, pa.v_nb2 = pl.stage_v_nb2, pa.v_nb3 = pl.stage_v_nb3;
            pa.k16 = (uint16_t*)pl.a.k, pa.v16 = (uint16_t*)pl.a.v;
            pa.mask = pl.a.mask, pa.m_nb1 = pl.a.m_nb1, pa.NQ = pl.a.NQ, pa.QPT = pl.a.QPT;
            pa.m_nb2 = pl.a.m_nb2, pa.m_nb3 = pl.a.m_nb3, pa.m_ne2 = pl.a.m_ne2, pa.m_ne3 = pl.a.m_ne3, pa.m_hg = pl.a.m_hg;
            pa.ntiles = pl.a.N / kPfKeys, pa.n_qt = pl.a.n_qt, pa.flags = (uint8_t*)pl.a.pf_flags;
            // one flag table per (sequence plane, head-plane group)
            const int64_t nfl = flags ? (int64_t)pa.ntiles * pl.a.n_qt * pl.a.m_ne3 * pl.a.m_hg : 0;
            const int64_t nst = staged ? 2 * (int64_t)pa.per_head * pa.hkv * pa.skv : 0;
            const dim3 g((unsigned)(nst + nfl));
            if (!staged) hipLaunchKernelGGL(pf_prepass_kernel<0>, g, dim3(256), 0, st, pa);
            else if (is_kv_ext(pl.stage_kt)) launch_prepass_kv_ext(pl.stage_kt, g, st, pa);
            else launch_prepass(QuantTypes(), pl.stage_kt, g, st, pa);
        }
        hipLaunchKernelGGL(kern, pl.grid, dim3(waves * kWave), pl.lds, st, launch_args<A>(pl));
    });
}
template <int KT, int D, bool HM>
int launch_pf_hm(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_pf_a<KT, D, HM, typename decltype(tag)::type>(pl, st, ev); });
}

// D = 128: the all-waves form, or the role form for quantised K/V (Kernel::Bdp);
// D = 64 / 96: the role form only for quantised K/V, the all-waves form's f16
// image ring for f16
template <int KT, int D, bool HM, typename A>
int launch_bd_a(const Plan& pl, hipStream_t st, const Events& ev) {
    void (*kern)(A) = nullptr;
    if constexpr (has_kernel(Kernel::Bd, KT, KT, D)) {
        if (pl.kernel == Kernel::Bd) kern = fattn_bd_kernel<KT, D, HM, A>;
    }
    if constexpr (has_kernel(Kernel::Bdp, KT, KT, D)) {
        if (pl.kernel == Kernel::Bdp) kern = fattn_bdp_kernel<KT, D, HM, A>;
    }
    if (kern == nullptr) return FATTN_ERR_UNSUPPORTED_TYPE;
    return launch_kernel((const void*)kern, pl, st, ev, [&] {
        hipLaunchKernelGGL(kern, pl.grid, dim3(kBdWaves * kWave), pl.lds, st, launch_args<A>(pl));
        if (pl.a.merge_launch == 1) launch_chunk_merge<BdMergeGeom, D>(dim3(kBdRows / 4, pl.grid.y, pl.grid.z), pl, st);
    });
}
template <int KT, int D, bool HM>
int launch_bd_hm(const Plan& pl, hipStream_t st, const Events& ev) {
    return with_args(pl, [&](auto tag) { return launch_bd_a<KT, D, HM, typename decltype(tag)::type>(pl, st, ev); });
}

template <int KT, int D>
int launch_bd(const Plan& pl, hipStream_t st, const Events& ev) {
    return pl.a.has_mask ? launch_bd_hm<KT, D, true>(pl, st, ev) : launch_bd_hm<KT, D, false>(pl, st, ev);
}

template <int KT, int D>
int launch_pf(const Plan& pl, hipStream_t st, const Events& ev) {
    return pl.a.has_mask ? launch_pf_hm<KT, D, true>(pl, st, ev) : launch_pf_hm<KT, D, false>(pl, st, ev);
}

// split kernel over mixed K / V cache types (instantiated once per D in
// fattn_launch_mixed_d<D>.hip; D = 64, 128, 256)
template <int D>
int launch_mixed(const Plan& pl, hipStream_t st, const Events& ev) {
    constexpr int none = FATTN_ERR_UNSUPPORTED_TYPE;
    return visit(CoreTypes(), pl.kt, none, [&](auto k) {
        return visit(CoreTypes(), pl.vt, none, [&](auto v) {
            constexpr int KT = decltype(k)::value, VT = decltype(v)::value;
            if constexpr (KT != VT) return launch_gran<KT, VT, D>(pl, st, ev);
            else return none;
        });
    });
}
extern template int launch_mixed<64>(const Plan&, hipStream_t, const Events&);
extern template int launch_mixed<128>(const Plan&, hipStream_t, const Events&);
extern template int launch_mixed<256>(const Plan&, hipStream_t, const Events&);

// split kernel over a Q4_1 / Q5_0 / Q5_1 cache (K and V of type T; instantiated
// once per (T, D) in fattn_launch_<type>_d<D>.hip; D = 64, 128, 256)
template <int T, int D>
int launch_kv_ext(const Plan& pl, hipStream_t st, const Events& ev) {
    static_assert(is_kv_ext(T), "");
    return launch_gran<T, T, D>(pl, st, ev);
}
#define FATTN_KV_EXT_EXTERN(T)                                                        \
    extern template int launch_kv_ext<T, 64>(const Plan&, hipStream_t, const Events&);  \
    extern template int launch_kv_ext<T, 128>(const Plan&, hipStream_t, const Events&); \
    extern template int launch_kv_ext<T, 256>(const Plan&, hipStream_t, const Events&);
FATTN_KV_EXT_EXTERN(FATTN_TYPE_Q4_1)
FATTN_KV_EXT_EXTERN(FATTN_TYPE_Q5_0)
FATTN_KV_EXT_EXTERN(FATTN_TYPE_Q5_1)
#undef FATTN_KV_EXT_EXTERN

// split kernel over a BF16 cache (K and V both BF16: raw bf16 rows into
// v_mfma_f32_16x16x32_bf16, Q and P as bf16 hi / lo pairs; instantiated once per
// D in fattn_launch_bf16_d<D>.hip; D = 64, 128, 256).  The only kernel of the
// type: no loader-wave form, and the planner sends every shape here
template <int D>
int launch_bf16(const Plan& pl, hipStream_t st, const Events& ev) {
    return launch_gran<FATTN_TYPE_BF16, FATTN_TYPE_BF16, D>(pl, st, ev);
}
extern template int launch_bf16<64>(const Plan&, hipStream_t, const Events&);
extern template int launch_bf16<128>(const Plan&, hipStream_t, const Events&);
extern template int launch_bf16<256>(const Plan&, hipStream_t, const Events&);

// every kernel of head dim D (defined here, instantiated once per D in
// fattn_launch_d<D>.hip)
template <int D>
int launch_types(const Plan& pl, hipStream_t st, const Events& ev) {
    // a (kernel, type, D) the library has no instantiation of (has_kernel) is this error
    constexpr int none = FATTN_ERR_UNSUPPORTED_TYPE;
    // K and V of one type of `types` that has one of `kerns` at this D: go(type)
    auto same = [&](auto types, auto go, auto... kerns) {
        if (pl.kt != pl.vt) return none;
        return visit(types, pl.kt, none, [&](auto k) {
            if constexpr ((has_kernel(decltype(kerns)::value, decltype(k)::value, decltype(k)::value, D) || ...)) return go(k);
            else return none;
        });
    };
    switch (pl.kernel) {
        case Kernel::Pf:
        case Kernel::Pf4:
            return same(CoreTypes(), [&](auto k) { return launch_pf<decltype(k)::value, D>(pl, st, ev); }, KernelC<Kernel::Pf>());
        case Kernel::Bd:
        case Kernel::Bdp:  // (a type with either form: launch_bd_hm picks)
            return same(CoreTypes(), [&](auto k) { return launch_bd<decltype(k)::value, D>(pl, st, ev); }, KernelC<Kernel::Bd>(), KernelC<Kernel::Bdp>());
        case Kernel::Mq:
            return same(QuantTypes(), [&](auto k) { return launch_mq<decltype(k)::value, D>(pl, st, ev); }, KernelC<Kernel::Mq>());
        case Kernel::Split:
        case Kernel::SplitLd:
            if constexpr (split_dim3(D)) {  // (the translation units of their own: extern templates above)
                if (pl.kt != pl.vt && pl.vt != VT_F16T) return launch_mixed<D>(pl, st, ev);
                if (pl.kt == pl.vt && in_list(SplitOnlyTypes(), pl.kt))
                    return visit(SplitOnlyTypes(), pl.kt, none, [&](auto k) {
                        constexpr int KT = decltype(k)::value;
                        if constexpr (is_row16(KT)) return pl.kernel == Kernel::Split ? launch_bf16<D>(pl, st, ev) : none;
                        else return launch_kv_ext<KT, D>(pl, st, ev);
                    });
            }
            if (pl.kt == FATTN_TYPE_F16 && pl.vt == VT_F16T) return launch_gran<FATTN_TYPE_F16, VT_F16T, D>(pl, st, ev);
            return same(CoreTypes(), [&](auto k) { return launch_gran<decltype(k)::value, decltype(k)::value, D>(pl, st, ev); }, KernelC<Kernel::Split>());
        case Kernel::Mla: break;  // (launch_mla: no head dim of this table)
    }
    return none;
}

// the MLA kernels (instantiated in fattn_launch_mla.hip)
int launch_mla(const Plan& pl, hipStream_t st, const Events& ev);
// ... over a Q8_0 / Q4_0 cache (instantiated in fattn_launch_mla_q.hip)
int launch_mla_q(const Plan& pl, hipStream_t st, const Events& ev);

extern template int launch_types<64>(const Plan&, hipStream_t, const Events&);
extern template int launch_types<80>(const Plan&, hipStream_t, const Events&);
extern template int launch_types<96>(const Plan&, hipStream_t, const Events&);
extern template int launch_types<128>(const Plan&, hipStream_t, const Events&);
extern template int launch_types<256>(const Plan&, hipStream_t, const Events&);

}  // namespace fattn
