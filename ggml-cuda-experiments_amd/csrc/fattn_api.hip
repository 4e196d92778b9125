// fattn_api.hip -- the C-ABI entry points (include/fattn.h, fattn_debug.h).
//
// The reference launches its kernels inline from host code with hard-coded
// template parameters (src/kernel_test.h:157-199, src/flash-matrix.cu:179-255).
// Here the host side validates the ggml views, picks the instantiation
// (head dim x K type x V type x addressing granule) and sizes the split-KV grid
// for the device's CUs (the planner, fattn_plan.h), then launches on the
// caller's stream (fattn_launch.h).  Nothing allocates; nothing synchronises
// (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fattn_plan.h"

using namespace fattn;

namespace {

constexpr int kCUsDefault = 256;  // MI355X; used when no device can be queried (host-only planning)

// compute units of the current device, queried once per device
int device_cus() {
    static std::atomic<int> cache[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        return kCUsDefault;
    }
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = kCUsDefault;
    }
    cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// fattn_set_option overrides (process-wide): one atomic per row of
// kOptionTable, indexed by option id.  Every entry point that plans copies them
// once (current_options) and plans from the copy, so a plan never mixes two
// values of one option; options set one after the other on another thread may
// still be seen one without the other -- overrides are meant to be set before
// launches, by tests and benchmarks.
struct OptionStore {
    std::atomic<int> v[kOptionSlots];
    OptionStore() {
        for (std::atomic<int>& x : v) x.store(0, std::memory_order_relaxed);
        for (const OptionRow& r : kOptionTable) v[r.id].store(r.def, std::memory_order_relaxed);
    }
};
OptionStore g_options;

Options current_options() {
    Options o;
    for (const OptionRow& r : kOptionTable) o.v[r.id] = g_options.v[r.id].load(std::memory_order_relaxed);
    return o;
}

// the plan of `p` under the current overrides, for the current device
int plan_now(const fattn_params* p, Plan& pl) { return make_plan(p, current_options(), device_cus(), pl); }

// launch epochs for the arrival words (SplitArgs::arrival_stamp); 32 bits, 0 skipped
std::atomic<uint32_t> g_epoch{0};

}  // namespace

extern "C" {

#ifdef FATTN_STAMPS
// diagnostic build only: where the split kernel writes its phase stamps
int fattn_debug_set_stamps_d64(void*);
int fattn_debug_set_stamps_d80(void*);
int fattn_debug_set_stamps_d96(void*);
int fattn_debug_set_stamps_d128(void*);
int fattn_debug_set_stamps_d256(void*);
int fattn_debug_set_stamps(void* dev_ptr) {
    return fattn_debug_set_stamps_d64(dev_ptr) | fattn_debug_set_stamps_d80(dev_ptr) | fattn_debug_set_stamps_d96(dev_ptr) |
           fattn_debug_set_stamps_d128(dev_ptr) | fattn_debug_set_stamps_d256(dev_ptr);
}
// grid of the plan: out[0..2] = chunks, Y, S
int fattn_debug_plan(const fattn_params* p, int* out) {
    Plan pl;
    const int rc = plan_now(p, pl);
    if (rc) return rc;
    out[0] = (int)pl.grid.x;
    out[1] = (int)pl.grid.y;
    out[2] = (int)pl.grid.z;
    return 0;
}
#endif

int fattn_set_option(int option, int value) {
    const OptionRow* r = find_option(option);
    if (!r || !r->legal(value)) return FATTN_ERR_INVALID_ARG;
    g_options.v[option].store(r->stored(value), std::memory_order_relaxed);
    return FATTN_OK;
}

const char* fattn_version(void) { return "fattn-gfx950 0.2"; }

const char* fattn_strerror(int s) {
    switch (s) {
        case FATTN_OK: return "ok";
        case FATTN_ERR_INVALID_ARG: return "invalid argument";
        case FATTN_ERR_UNSUPPORTED_TYPE: return "unsupported tensor type";
        case FATTN_ERR_UNSUPPORTED_HEAD_DIM: return "unsupported head dim (64, 80 (f16 K/V), 96 (not q4_1 / q5_0 / q5_1 / bf16), 128, 256; K 576 with V 512: f16, or q8_0 / q4_0 with V a view of K)";
        case FATTN_ERR_BAD_STRIDE: return "unsupported strides / layout";
        case FATTN_ERR_WORKSPACE: return "workspace too small";
        case FATTN_ERR_LAUNCH: return "HIP launch failed";
        case FATTN_ERR_ALIGNMENT: return "misaligned pointer or stride";
        default: return "unknown error";
    }
}

size_t fattn_row_size(int type, int64_t k) { return row_size(type, k); }

int fattn_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace && workspace_bytes) return FATTN_ERR_INVALID_ARG;
    if (!workspace_bytes) return FATTN_OK;
    return hipMemsetAsync(workspace, 0, workspace_bytes, (hipStream_t)stream) == hipSuccess ? FATTN_OK
                                                                                          : FATTN_ERR_LAUNCH;
}

size_t fattn_workspace_size(const fattn_params* p) {
    Plan pl;
    if (plan_now(p, pl) != FATTN_OK) return 0;
    return pl.ws_bytes;
}

int fattn_describe(const fattn_params* p, char* out, size_t cap) {
    Plan pl;
    const int rc = plan_now(p, pl);
    if (rc != FATTN_OK) return rc;
    auto tn = [](int t) { return t == VT_F16T ? "f16T" : type_name(t); };
    const char* hm = pl.a.has_mask ? "mask" : "nomask";
    // the second-launch merge `name` of the plan, or its in-kernel merge (split, batched decode)
    char merge[64] = "";
    auto merged_by = [&](const char* name) {
        if (pl.a.merge_launch == 1)
            std::snprintf(merge, sizeof merge, " + %s%s", name, pl.a.part_f16 ? "(f16 partials)" : pl.merge_plain ? "(plain)" : "");
        else if (pl.a.merge_launch == 2)
            std::snprintf(merge, sizeof merge, " (in-kernel merge)");
    };
    const char* xcd = pl.a.xcd_group ? " (xcd order)" : "";
    // The merge launch is one kernel, fattn_chunk_merge_kernel (fattn_tile.h); the
    // plan names it by its geometry: fattn_merge_kernel = SplitMergeGeom,
    // fattn_bd_merge_kernel = BdMergeGeom, fattn_mq_merge_kernel = MqMergeGeom,
    // fattn_mla_merge_kernel = MlaMergeGeom (the plan vocabulary callers and tests read)
    char kern[160];
    switch (pl.kernel) {
        case Kernel::Mla: {  // (f32 partials, plain loads: no other merge form)
            char vform[24] = "v=own";
            if (pl.mla_v_off >= 0) std::snprintf(vform, sizeof vform, "v=k+%d", pl.mla_v_off);
            // (quantised cache: wave 0 computes, waves 1 - 3 load and convert; ... whole tiles in 16-B pieces)
            const char* solo = pl.mla_raw16 ? " (solo, 16-B tiles)" : pl.mla_solo ? " (solo)" : "";
            std::snprintf(kern, sizeof kern, "fattn_mla_kernel<%s,DK%d,DV%d,%s,%s>%s%s%s", tn(pl.kt), pl.D, pl.DV, hm, vform, solo,
                          xcd, pl.a.merge_launch ? " + fattn_mla_merge_kernel" : "");
            break;
        }
        case Kernel::Pf:
        case Kernel::Pf4: {
            const bool pre = pl.pf_stage || pl.pf_flags;  // (the pre-pass: one launch, pf_prepass_kernel)
            const char* body = pl.kernel == Kernel::Pf ? "fattn_pf_kernel"
                               : pl.pf4_sched == 4     ? "fattn_pf4_kernel(lean)"
                               : pl.pf4_sched == 3     ? "fattn_pf4_kernel(balanced)"
                                                       : "fattn_pf4_kernel(pipelined)";
            char stage[32] = "";
            if (pl.pf_stage) std::snprintf(stage, sizeof stage, "kv_stage_f16<%s>", tn(pl.stage_kt));
            std::snprintf(kern, sizeof kern, "%s%s%s%s%s%s<%s,D%d,%s>", pre ? "pf_prepass[" : "", stage,
                          pl.pf_stage && pl.pf_flags ? " + " : "", pl.pf_flags ? "pf_mask_flags" : "", pre ? "] + " : "",
                          body, tn(pl.kt), pl.D, hm);
            break;
        }
        case Kernel::Bd:
        case Kernel::Bdp:
            merged_by("fattn_bd_merge_kernel");
            std::snprintf(kern, sizeof kern, "%s<%s,D%d,%s>%s%s", pl.kernel == Kernel::Bdp ? "fattn_bdp_kernel" : "fattn_bd_kernel",
                          tn(pl.kt), pl.D, hm, xcd, merge);
            break;
        case Kernel::Mq:  // (no plain-load merge, no in-kernel merge)
            if (pl.a.merge_launch)
                std::snprintf(merge, sizeof merge, " + fattn_mq_merge_kernel%s", pl.a.part_f16 ? "(f16 partials)" : "");
            std::snprintf(kern, sizeof kern, "fattn_mq_kernel<%s,D%d,%dwaves,%s>%s", tn(pl.kt), pl.D, pl.nw, hm, merge);
            break;
        case Kernel::Split:
        case Kernel::SplitLd: {
            const bool ld = pl.kernel == Kernel::SplitLd;
            merged_by("fattn_merge_kernel");
            std::snprintf(kern, sizeof kern, "%s<%s,%s,D%d,gran%d,%s,%dwaves%s>%s%s", ld ? "fattn_split_ld_kernel" : "fattn_split_kernel",
                          tn(pl.kt), tn(pl.vt), pl.D, pl.gran, hm, pl.nwv, ld ? "+4loaders" : "", xcd, merge);
            break;
        }
    }
    char planes[48] = "";
    if (pl.a.m_ne2 > 1 || pl.a.m_ne3 > 1) std::snprintf(planes, sizeof planes, " mask planes (%d,%d)", pl.a.m_ne2, pl.a.m_ne3);
    // (only what is live in the plan: max_bias without a mask names nothing)
    char xf[64] = "";
    int xn = 0;
    if (pl.a.xf.live & 1) xn = std::snprintf(xf, sizeof xf, " softcap %g", (double)p->logit_softcap);
    if (pl.a.xf.live & 2) std::snprintf(xf + xn, sizeof xf - xn, " alibi %g", (double)p->max_bias);
    const int n = std::snprintf(out, cap, "%s grid(%u,%u,%u) lds %d chunk %d steps/slots %d ws %zu%s%s", kern, pl.grid.x,
                                pl.grid.y, pl.grid.z, pl.lds, pl.a.chunk_len, pl.a.nbuf, pl.ws_bytes, planes, xf);
    return n < 0 || (size_t)n >= cap ? FATTN_ERR_INVALID_ARG : FATTN_OK;
}

}  // extern "C"

namespace {

// The one launch path of fattn_ext / fattn_ext_events / fattn_ext_sinks /
// fattn_ext_lse.  The plan is a function of `p` alone: `sinks` (null: off) only
// rides along as a kernel argument of the plan's kernels (SplitArgs::sinks), and
// with `lse` the same plan launches its kernels' instantiations over
// SplitArgsLse, which also store the rows' log-sum-exp (Plan::lse, with_args)
int launch_ext(const fattn_params* p, const float* sinks, float* lse, void* stream, void* ev_begin, void* ev_end) {
    Plan pl;
    const int rc = plan_now(p, pl);
    if (rc != FATTN_OK) return rc;
    if ((uintptr_t)sinks % 4) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)lse % 4) return FATTN_ERR_ALIGNMENT;
    pl.a.sinks = sinks;
    pl.lse = lse;
    if (pl.ws_bytes) {
        if (!p->workspace || p->workspace_bytes < pl.ws_bytes || (uintptr_t)p->workspace % 16) return FATTN_ERR_WORKSPACE;
        uint8_t* w = (uint8_t*)p->workspace;
        pl.a.ws_cnt = (uint32_t*)w;
        uint32_t e = g_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
        if (e == 0) e = g_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
        pl.a.arrival_stamp = kArrivalTag | (uint64_t)e << kArrivalEpochShift;
        pl.a.ws_ml = (float*)(w + pl.cnt_bytes);
        pl.a.ws_o = (float*)(w + pl.cnt_bytes + pl.ml_bytes);  // (prefill pre-pass: the f16 rows)
        if (pl.pf_flags) pl.a.pf_flags = w;
        if (pl.pf_stage) {
            pl.a.k = w + pl.stage_off;
            pl.a.v = w + pl.stage_off + pl.stage_bytes;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    Events ev;
    ev.begin = (hipEvent_t)ev_begin;
    ev.end = (hipEvent_t)ev_end;
    if (pl.kernel == Kernel::Mla) return launch_mla(pl, st, ev);
    switch (pl.D) {
        case 64: return launch_types<64>(pl, st, ev);
        case 80: return launch_types<80>(pl, st, ev);
        case 96: return launch_types<96>(pl, st, ev);
        case 128: return launch_types<128>(pl, st, ev);
        default: return launch_types<256>(pl, st, ev);
    }
}

// one 256-thread workgroup per 256 units (elements or blocks) of the conversion kernels
dim3 grid256(int64_t units) { return dim3((unsigned)((units + 255) / 256)); }

}  // namespace

extern "C" {

int fattn_ext(const fattn_params* p, void* stream) { return launch_ext(p, nullptr, nullptr, stream, nullptr, nullptr); }

int fattn_ext_events(const fattn_params* p, void* stream, void* ev_begin, void* ev_end) {
    return launch_ext(p, nullptr, nullptr, stream, ev_begin, ev_end);
}

int fattn_ext_sinks(const fattn_params* p, const float* sinks, void* stream) {
    return launch_ext(p, sinks, nullptr, stream, nullptr, nullptr);
}

int fattn_ext_lse(const fattn_params* p, const float* sinks, float* lse, void* stream) {
    return launch_ext(p, sinks, lse, stream, nullptr, nullptr);
}

int fattn_ext_f16_launch(const void* q, const void* k, const void* v, const void* mask, float* dst, float scale,
                         int ne00, int ne01, int ne02, int ne03, int ne10, int ne11, int ne12, int ne13, int ne31,
                         int nb31, int nb01, int nb02, int nb03, int nb11, int nb12, int nb13, int ne0, int ne1,
                         int ne2, int ne3, int k_type, int v_type, void* workspace, size_t workspace_bytes,
                         void* stream) {
    // flash-llama.h:120-125: V shares K's shape and strides -- so one row size:
    // mixed K / V types need the struct form (fattn_ext) with V's own strides.
    // The same one ne10 is K's and V's row length: the list cannot name the MLA
    // shape (K dim 576, V dim 512), which only fattn_ext / fattn_ext_sinks take --
    // ne00 = 576 here is FATTN_ERR_UNSUPPORTED_HEAD_DIM (V read as 576 wide)
    (void)ne0; (void)ne1; (void)ne2; (void)ne3;
    if (k_type != v_type) return FATTN_ERR_INVALID_ARG;
    fattn_params p;
    std::memset(&p, 0, sizeof(p));
    p.q = {q, FATTN_TYPE_F32, 0, {ne00, ne01, ne02, ne03}, {4, nb01, nb02, nb03}};
    const int64_t kb0 = type_desc(k_type).block_bytes, vb0 = type_desc(v_type).block_bytes;
    p.k = {k, k_type, 0, {ne10, ne11, ne12, ne13}, {kb0, nb11, nb12, nb13}};
    p.v = {v, v_type, 0, {ne10, ne11, ne12, ne13}, {vb0, nb11, nb12, nb13}};
    // mask rows hold nb31 / 2 halves: ggml pads them (GGML_KQ_MASK_PAD) past ne11,
    // which an odd ne11 needs (the kernels read rows in dword pieces)
    if (mask)
        p.mask = {mask, FATTN_TYPE_F16, 0, {nb31 / 2, ne31, 1, 1}, {2, nb31, (int64_t)nb31 * ne31, (int64_t)nb31 * ne31}};
    p.dst = dst;
    p.scale = scale;
    p.workspace = workspace;
    p.workspace_bytes = workspace_bytes;
    return fattn_ext(&p, stream);
}

static void fill_row_params(fattn_params& p, const float* query, const void* key, const void* value, const void* mask,
                            float* qkv, int head_dim, int kv_size, int num_heads, float scale, int head_stride,
                            int r_kv_heads) {
    std::memset(&p, 0, sizeof(p));
    const int64_t D = head_dim, N = kv_size, H = num_heads, Hkv = num_heads / r_kv_heads;
    p.q = {query, FATTN_TYPE_F32, 0, {D, 1, H, 1}, {4, D * H * 4, D * 4, D * H * 4}};
    // key [Hkv][N][D] f16 (flash_row_float.h:19,58): kv head offset head_stride elements
    p.k = {key, FATTN_TYPE_F16, 0, {D, N, Hkv, 1}, {2, D * 2, (int64_t)head_stride * 2, (int64_t)head_stride * 2 * Hkv}};
    // value f16 transposed [Hkv][D][N] (flash_row_float.h:177)
    p.v = {value, FATTN_TYPE_F16, 0, {D, N, Hkv, 1}, {N * 2, 2, (int64_t)head_stride * 2, (int64_t)head_stride * 2 * Hkv}};
    if (mask) p.mask = {mask, FATTN_TYPE_F16, 0, {N, 1, 1, 1}, {2, N * 2, N * 2, N * 2}};
    p.dst = qkv;  // [1][H][D] == qkv[h*D + d] (flash_row_float.h:469)
    p.scale = scale;
}

// The ABI (kernel_test.h:155's inline sizing) does not name r_kv_heads, and
// the plan -- rows per tile, chunks, merge layout -- depends on it: size for
// the largest plan over every r that divides num_heads, with and without a mask.
size_t fattn_row_workspace_size(int head_dim, int kv_size, int num_heads) {
    if (num_heads <= 0) return 0;
    size_t best = 0;
    static const float dummy_f[4] = {0, 0, 0, 0};
    const Options opts = current_options();
    const int cus = device_cus();
    for (int r = 1; r <= num_heads; r++) {
        if (num_heads % r) continue;
        for (int m = 0; m < 2; m++) {
            fattn_params p;
            fill_row_params(p, dummy_f, dummy_f, dummy_f, m ? dummy_f : nullptr, (float*)dummy_f, head_dim, kv_size,
                            num_heads, 1.0f, head_dim * kv_size, r);
            p.q.data = (const void*)(uintptr_t)16;  // alignment-only placeholders
            p.k.data = p.v.data = (const void*)(uintptr_t)16;
            if (m) p.mask.data = (const void*)(uintptr_t)16;
            Plan pl;
            if (make_plan(&p, opts, cus, pl) == FATTN_OK) best = std::max(best, pl.ws_bytes);
        }
    }
    return best;
}

int fattn_row(const float* query, const void* key, const void* value, const void* mask, void* tmp, size_t tmp_bytes,
              float* qkv, int head_dim, int kv_size, int num_heads, float scale, int head_stride, int r_kv_heads,
              void* stream) {
    if (r_kv_heads <= 0 || num_heads % r_kv_heads) return FATTN_ERR_INVALID_ARG;
    fattn_params p;
    fill_row_params(p, query, key, value, mask, qkv, head_dim, kv_size, num_heads, scale, head_stride, r_kv_heads);
    p.workspace = tmp;
    p.workspace_bytes = tmp_bytes;
    return fattn_ext(&p, stream);
}

int fattn_dequantize(int type, const void* src, float* dst, int64_t k, int64_t n_rows, void* stream) {
    if (!src || !dst || k <= 0 || n_rows <= 0) return FATTN_ERR_INVALID_ARG;
    if (!in_list(CacheTypes(), type)) return FATTN_ERR_UNSUPPORTED_TYPE;
    if (is_quant(type) && k % QK) return FATTN_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = k * n_rows;
    visit(CacheTypes(), type, 0, [&](auto tc) {
        constexpr int T = decltype(tc)::value;
        if constexpr (is_row16(T)) hipLaunchKernelGGL(dequant_row16_kernel<T>, grid256(n), dim3(256), 0, st, (const uint16_t*)src, dst, n);
        else hipLaunchKernelGGL(dequant_kernel<T>, grid256(n / QK), dim3(256), 0, st, (const uint8_t*)src, dst, n / QK);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}

int fattn_quantize(int type, const float* src, void* dst, int64_t k, int64_t n_rows, void* stream) {
    if (!src || !dst || k <= 0 || n_rows <= 0) return FATTN_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (type == FATTN_TYPE_BF16) {  // per element: any row length, 4-byte aligned src, 2-byte aligned dst
        if ((uintptr_t)src % 4 || (uintptr_t)dst % 2) return FATTN_ERR_ALIGNMENT;
        const int64_t n = k * n_rows;
        hipLaunchKernelGGL(quant_bf16_kernel<>, grid256(n), dim3(256), 0, st, src, (uint16_t*)dst, n);
        return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
    }
    if (k % QK) return FATTN_ERR_INVALID_ARG;
    if ((uintptr_t)src % 16) return FATTN_ERR_ALIGNMENT;
    if (!is_quant(type)) return FATTN_ERR_UNSUPPORTED_TYPE;
    const int64_t nb = k * n_rows / QK;
    visit(StageTypes(), type, 0, [&](auto tc) {
        hipLaunchKernelGGL(quant_kernel<decltype(tc)::value>, grid256(nb), dim3(256), 0, st, src, (uint8_t*)dst, nb);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}

int fattn_cpy(const fattn_tensor* src, const fattn_tensor* dst, void* stream) {
    if (!src || !dst || !src->data || !dst->data) return FATTN_ERR_INVALID_ARG;
    if (src->type != FATTN_TYPE_F32 || src->nb[0] != 4) return FATTN_ERR_UNSUPPORTED_TYPE;
    const int t = dst->type;
    if (!in_list(CacheTypes(), t)) return FATTN_ERR_UNSUPPORTED_TYPE;
    for (int i = 0; i < 4; i++)
        if (src->ne[i] != dst->ne[i] || src->ne[i] <= 0) return FATTN_ERR_INVALID_ARG;
    const int64_t ue = type_desc(t).block_elems;
    if (src->ne[0] % ue) return FATTN_ERR_INVALID_ARG;
    if (dst->nb[0] != (int64_t)fattn_row_size(t, ue)) return FATTN_ERR_BAD_STRIDE;
    if ((uintptr_t)src->data % 4 || src->nb[1] % 4 || src->nb[2] % 4 || src->nb[3] % 4) return FATTN_ERR_ALIGNMENT;
    if ((uintptr_t)dst->data % 2 || dst->nb[1] % 2 || dst->nb[2] % 2 || dst->nb[3] % 2) return FATTN_ERR_ALIGNMENT;
    CpyArgs a;
    a.src = (const uint8_t*)src->data;
    a.dst = (uint8_t*)dst->data;
    a.ne0 = src->ne[0]; a.ne1 = src->ne[1]; a.ne2 = src->ne[2]; a.ne3 = src->ne[3];
    a.snb1 = src->nb[1]; a.snb2 = src->nb[2]; a.snb3 = src->nb[3];
    a.dnb1 = dst->nb[1]; a.dnb2 = dst->nb[2]; a.dnb3 = dst->nb[3];
    const int64_t units = a.ne0 / ue * a.ne1 * a.ne2 * a.ne3;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    visit(CacheTypes(), t, 0, [&](auto tc) {
        hipLaunchKernelGGL(cpy_f32_kernel<decltype(tc)::value>, grid256(units), dim3(256), 0, st, a, units);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? FATTN_OK : FATTN_ERR_LAUNCH;
}

}  // extern "C"
