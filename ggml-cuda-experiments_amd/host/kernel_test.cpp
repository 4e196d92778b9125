// kernel_test.cpp -- MI355X counterpart of the reference's launch/verify harness
// (src/kernel_test.h:1-249, entered from main() in src/flash-matrix.cu:341-346).
//
// Same flags and the same flow: synthetic inputs from rand() in the order
// Q, K, V, mask (kernel_test.h:45-48; srand never called -> glibc seed 1),
// a CPU reference with the reference's arithmetic (kernel_test.h:50-62: operands
// rounded through fp16, fp32 accumulation, single-pass online softmax), the GPU
// path through the C ABI (include/fattn.h), a timed launch and the max-diff
// report (kernel_test.h:201-234).  Differences from the reference harness, all
// additive: a pass/fail threshold and exit code (the reference prints a diff
// with no threshold), warmup + repeated timing (median), and K/V types.
//
//   --no-kv-parallel     the flash_attn_ext branch (kernel_test.h:180-199): the call goes
//                        through fattn_ext_f16_launch with kernel_test.h:191-198's argument
//                        list -- 32-row padded mask (row 0 = the mask, kernel_test.h:74-85),
//                        ne31 = 32, nb31 = kv_size*2, nb01 = nb02 = head_dim*4, V not
//                        transposed.  The default branch is flash_attn_row + fa_reduce
//                        (kernel_test.h:161-162): fattn_row with V transposed.
//   --n-warps N          accepted for compatibility (kernel_test.h:9-13); the gfx950
//                        kernels pick their own wave counts
//   --kv-size N          KV length, min 256 on the GPU path (kernel_test.h:14-18)
//   --kv-type T          f16 (default, as the reference) | q8_0 | q4_0 | q4_1 | q5_0 | q5_1 | bf16
//                        (bf16: the cache written by fattn_cpy; the reference over the bf16-rounded
//                        values, rounded on the host; not with --set-rows, which has no bf16 form)
//   --cpu-only           the CPU reference alone (BASELINE config 1: no GPU is touched,
//                        any kv_size); with --dump FILE its f32 output is written raw
//   --head-dim D --heads H --kv-heads Hkv --iters I --tol T
//   --n-q N              query rows (the reference's batch / ne01, flash-llama.h:7-32;
//                        src/flash-matrix.cu:76): Q [n_q][H][D], mask [rows >= n_q, padded
//                        to 32][N'], dst [n_q][H][D]; n_q > 1 takes the ext branch
//   --mask random|zero|none   mask values (default random, kernel_test.h:48)
//   --check-rows R       verify R query rows at the start, middle and end of the
//                        sequence (all rows when n_q <= 3R; the CPU reference is slow)
//   --config N           BASELINE.json's configs: 1 (CPU only: 1 head, D 64, N 128),
//                        2 (f16, 32 heads, D 128, N 2048, flash_attn_row), 3 (Q8_0,
//                        32 heads, N 4096), 4 (Q4_0, 32 q / 8 kv heads, N 8192), 5 (Q8_0,
//                        n_q 64, N 4096); "prefill" (Q8_0, n_q = N = 4096, 32 heads,
//                        zero mask: SURVEY 8(d)'s MFMA shape); later flags override
//   --max-bias F         ggml's max_bias (ALiBi): head h adds slope(h) * mask to its scores
//   --softcap F          ggml's logit_softcap: cap * tanh(score / cap) before the mask
//                        (both default 0 = off; either takes the fattn_params call, with
//                        n_head_total / head_first set per device under --ngpu)
//   --sinks BASE         ggml's attention sinks (src[4], fattn_ext_sinks): head h of the model
//                        gets the raw extra logit BASE + 0.25 * (h % 8) in its softmax
//                        denominator (the global head index under --ngpu: device g passes
//                        its own slice); the CPU reference applies the same
//   --lse                also the rows' log-sum-exp (fattn_ext_lse): the CPU reference computes it
//                        (with --sinks the sink is one of its terms), the GPU path launches
//                        fattn_ext_lse and prints `lse max abs err` beside the verification line
//                        (passes at 1e-4 of max(1, |lse|)); with --cpu-only --dump FILE it goes to FILE.lse.
//                        One device; the call goes through the fattn_params form
//   --set-rows           build the K / V caches with fattn_set_rows (GGML_OP_SET_ROWS) from the
//                        f32 K / V instead of fattn_quantize / the host's f16 rounding: row n
//                        goes to slot perm[n] of a seeded permutation, and the CPU reference
//                        sees K, V and the mask columns in slot order (Q has no KV axis); implies
//                        --no-kv-parallel (flash_attn_row's transposed V is no row write)
//   --mla [--v-off 0|64] multi-head latent attention (DeepSeek-V2/V3, Kimi-K2): one kv head, K rows
//                        of 576 f16, V the 512 elements of the same rows from element 0 (latent
//                        first) or 64 (RoPE dims first, llama.cpp's order) -- a view of K, so each
//                        cache row is read once; --heads (default 16) / --kv-size / --n-q / --mask
//                        / --iters / --tol / --cpu-only / --dump apply, scale = 1 / sqrt(192); the
//                        CPU reference is plain C++ over K dim 576 and V dim 512.  With
//                        --kv-type q8_0|q4_0 the cache rows are quantised (fattn_quantize; on the
//                        host with --cpu-only), V is the view --v-off 0|32|64 elements (whole
//                        blocks) in, and the reference takes the blocks dequantised on the host
//   --k-shift DELTA [--rope-mode norm|neox]   llama.cpp's K-shift (fattn_k_shift): the K / V caches of
//                        --kv-type are encoded on the host, every slot of the K cache is rotated in place by
//                        the RoPE of DELTA positions on the GPU (n_dims = --head-dim, mode neox by default,
//                        freq_base 10000), the host recomputes the same in plain C++ (decode, rotate,
//                        encode) and the CPU reference attends over that cache; one query row;
//                        --heads / --kv-heads / --kv-size / --head-dim (a multiple of 32, <= 256) / --mask /
//                        --iters / --tol / --cpu-only apply.  Prints how many cache bytes differ from the
//                        host's shift (sinf / cosf ulps may flip a code) and the verification line
//   --ngpu G             head-shard over G GPUs of this host (kv heads Hkv/G and their q
//                        heads per device, fattn_ext on each, one RCCL all-gather of the
//                        outputs, permuted into the ggml dst layout): BASELINE config 5's
//                        multi-GPU form, timed as kernel + gather
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fattn.h"

#define HIP_CHECK(x)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #x); \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

namespace {

// ---- host fp16 (round to nearest even), the conversions utils.h relies on
uint16_t f2h(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u) return (uint16_t)(sign | (ax > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
    if (ax < 0x38800000u) {
        if (ax <= 0x33000000u) return (uint16_t)sign;
        const uint32_t e = ax >> 23, m = (ax & 0x7fffffu) | 0x800000u, sh = 126u - e;
        uint32_t q = m >> sh;
        const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return (uint16_t)(sign | q);
    }
    uint32_t h = ((((ax >> 23) - 112u) << 10) | ((ax & 0x7fffffu) >> 13));
    const uint32_t rem = ax & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
}
float h2f(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) {
            x = sign;
        } else {
            int ee = -1;
            do {
                ee++;
                m <<= 1;
            } while (!(m & 0x400u));
            x = sign | ((uint32_t)(112 - ee) << 23) | ((m & 0x3ffu) << 13);
        }
    } else if (e == 31) {
        x = sign | 0x7f800000u | (m << 13);
    } else {
        x = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &x, 4);
    return f;
}
float rh(float x) { return h2f(f2h(x)); }

// kernel_test.h:45-48 / utils.h:57-61
void random_fill(std::vector<float>& a) {
    for (auto& x : a) x = 1.0f - ((float)rand() * 1.0f / (float)RAND_MAX) * 2.0f;
}

// kernel_test.h:50-62 with utils.h:5-49 arithmetic, per (query row, head):
// q [NQ][H][D], k / v [Hkv][N][D], mask [NQ][N], out [NQ][H][D]; only the rows
// listed (all of them for the reference's n_q = 1), heads over threads (the
// per-head arithmetic and its order are the reference's, so the bits are too)
// max_bias / softcap: ggml's FLASH_ATTN_EXT scalars (include/fattn.h), by its
// host formulas -- score = cap * tanhf(acc * (scale / cap)) (softcap > 0) plus
// slope(h) * mask; with both 0 the statements below are the reference's.
// sinks (null: none): ggml's src[4], one raw logit per head joining (M, S) after
// the row's last key by ggml's statement; the row is then the plain row times
// g = vs * S_plain / S -- the factor form, so P keeps the plain row's f16 rounding
bool dump_floats(const char* path, const std::vector<float>& x) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(x.data(), sizeof(float), x.size(), f) != x.size()) {
        fprintf(stderr, "cannot write %s\n", path);
        return false;
    }
    fclose(f);
    return true;
}

// --lse: the natural-log log-sum-exp of a row with running max M and sum S =
// sum exp(score - M); with a sink the sink is one more term, taken at
// max(M, sink).  A row without a live key (M = -inf): the sink, or -inf
float row_lse(float M, float S, const float* sink) {
    if (M == -INFINITY) return sink ? *sink : -INFINITY;
    if (!sink || *sink == -INFINITY) return M + logf(S);
    return *sink > M ? *sink + logf(S * expf(M - *sink) + 1.0f) : M + logf(S + expf(*sink - M));
}

// `lse max abs err` of --lse over rows x heads; the pass mark is on the error relative to max(1, |ref|): 1e-4
bool lse_check(const std::vector<float>& ref, const std::vector<float>& got, const std::vector<int>& rows, int H) {
    float worst = 0.0f, worst_abs = 0.0f;
    for (int r : rows)
        for (int h = 0; h < H; h++) {
            const float a = ref[(size_t)r * H + h], b = got[(size_t)r * H + h];
            float e = fabsf(a - b) / std::max(1.0f, fabsf(a));
            if (a == b) e = 0.0f;  // (both -inf)
            worst = std::isnan(e) ? INFINITY : std::max(worst, e);
            worst_abs = a == b ? worst_abs : std::isnan(e) ? INFINITY : std::max(worst_abs, fabsf(a - b));
        }
    printf("lse max abs err %.3g (%.3g of max(1, |lse|), tol 1e-04): %s\n", worst_abs, worst, worst <= 1e-4f ? "PASS" : "FAIL");
    return worst <= 1e-4f;
}

void cpu_reference(const std::vector<float>& q, const std::vector<float>& k, const std::vector<float>& v,
                   const std::vector<float>& mask, std::vector<float>& out, int N, int D, int H, int Hkv, float scale,
                   const std::vector<int>& rows, int threads = 1, float max_bias = 0.0f, float softcap = 0.0f,
                   const std::vector<float>* sinks = nullptr, std::vector<float>* lse = nullptr) {
    const int r = H / Hkv;
    int n2 = 1;
    while (n2 * 2 <= H) n2 *= 2;
    const float m0 = powf(2.0f, -max_bias / (float)n2), m1 = powf(2.0f, -(max_bias / 2.0f) / (float)n2);
    const bool xf = max_bias > 0.0f || softcap > 0.0f;
    std::vector<float> qh(q.size()), kh(k.size()), vh(v.size());
    for (size_t i = 0; i < q.size(); i++) qh[i] = rh(q[i]);
    for (size_t i = 0; i < k.size(); i++) kh[i] = rh(k[i]);
    for (size_t i = 0; i < v.size(); i++) vh[i] = rh(v[i]);
    auto head = [&](int h) {
        std::vector<float> s(N);
        const float* kk = kh.data() + (size_t)(h / r) * D * N;
        const float* vv = vh.data() + (size_t)(h / r) * D * N;
        for (int row : rows) {
            const float* qq = qh.data() + ((size_t)row * H + h) * D;
            const float* mrow = mask.data() + (size_t)row * N;
            for (int c = 0; c < N; c++) {
                float acc = 0.0f;
                for (int i = 0; i < D; i++) {
                    const float p = qq[i] * kk[(size_t)c * D + i];
                    acc = acc + p;
                }
                s[c] = acc * scale + mrow[c];
                if (xf) {
                    const float slope = max_bias > 0.0f ? (h < n2 ? powf(m0, (float)(h + 1)) : powf(m1, (float)(2 * (h - n2) + 1))) : 1.0f;
                    const float x = softcap > 0.0f ? softcap * tanhf(acc * (scale / softcap)) : acc * scale;
                    s[c] = x + slope * mrow[c];
                }
            }
            float M = -INFINITY, S = 0.0f;
            for (int i = 0; i < N; i++) {
                if (s[i] > M) {
                    S = 1.0f + S * expf(M - s[i]);
                    M = s[i];
                } else {
                    S += expf(s[i] - M);
                }
            }
            for (int i = 0; i < N; i++) s[i] = expf(s[i] - M) / S;
            float gsink = 1.0f;
            if (sinks) {
                const float sk = (*sinks)[h];
                float vs = 1.0f, Ss = S;
                if (sk > M) {
                    vs = expf(M - sk);
                    Ss = Ss * vs + 1.0f;
                } else {
                    Ss += expf(sk - M);
                }
                gsink = vs * S / Ss;
                if (M == -INFINITY) {  // mask -inf everywhere: S = 1, VKQ = 0
                    gsink = 0.0f;
                    for (int i = 0; i < N; i++) s[i] = 0.0f;
                }
            }
            if (lse) (*lse)[(size_t)row * H + h] = row_lse(M, S, sinks ? &(*sinks)[h] : nullptr);
            float* o = out.data() + ((size_t)row * H + h) * D;
            for (int c = 0; c < D; c++) {
                float acc = 0.0f;
                for (int i = 0; i < N; i++) {
                    const float p = rh(s[i]) * vv[(size_t)i * D + c];
                    acc = acc + p;
                }
                o[c] = sinks ? acc * gsink : acc;
            }
        }
    };
    threads = std::max(1, std::min(threads, H));
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (int h = t; h < H; h += threads) head(h);
        });
    for (auto& th : pool) th.join();
}

const char* type_name(int t) {
    return t == FATTN_TYPE_Q8_0 ? "q8_0" : t == FATTN_TYPE_Q4_0 ? "q4_0" : t == FATTN_TYPE_Q4_1 ? "q4_1"
           : t == FATTN_TYPE_Q5_0 ? "q5_0" : t == FATTN_TYPE_Q5_1 ? "q5_1" : t == FATTN_TYPE_BF16 ? "bf16" : "f16";
}

// f32 -> the f32 value of its bf16 rounding (ggml_compute_fp32_to_bf16: NaN kept
// and made quiet, else round to nearest even on the 16 dropped bits)
float round_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t h = (u & 0x7fffffffu) > 0x7f800000u ? (u >> 16) | 64u : (u + (0x7fffu + ((u >> 16) & 1u))) >> 16;
    u = h << 16;
    std::memcpy(&f, &u, 4);
    return f;
}

bool is_kv_ext(int t) { return t == FATTN_TYPE_Q4_1 || t == FATTN_TYPE_Q5_0 || t == FATTN_TYPE_Q5_1; }

// ggml's dequantize_row_q4_1 / _q5_0 / _q5_1 in plain C++ (this file builds with
// -ffp-contract=off: every operation rounded on its own): `rows` rows of D values
// from blocks {f16 d; [f16 m;] [u8 qh[4];] u8 qs[16]}
void dequant_host(int type, const uint8_t* src, float* dst, int D, int64_t rows) {
    const bool has_m = type != FATTN_TYPE_Q5_0, has_qh = type != FATTN_TYPE_Q4_1;
    const int bb = 2 + (has_m ? 2 : 0) + (has_qh ? 4 : 0) + 16;
    const int64_t nblk = rows * (D / 32);
    for (int64_t i = 0; i < nblk; i++) {
        const uint8_t* b = src + i * bb;
        const float d = h2f((uint16_t)(b[0] | (b[1] << 8)));
        const float m = has_m ? h2f((uint16_t)(b[2] | (b[3] << 8))) : 0.0f;
        const uint8_t* hp = b + (has_m ? 4 : 2);
        const uint32_t qh = has_qh ? (uint32_t)hp[0] | ((uint32_t)hp[1] << 8) | ((uint32_t)hp[2] << 16) | ((uint32_t)hp[3] << 24) : 0u;
        const uint8_t* qs = b + bb - 16;
        float* y = dst + i * 32;
        for (int j = 0; j < 16; j++) {
            const int q0 = (qs[j] & 0x0F) | (int)(((qh >> j) & 1u) << 4);
            const int q1 = (qs[j] >> 4) | (int)(((qh >> (j + 16)) & 1u) << 4);
            if (has_m) {
                y[j] = (float)q0 * d + m;
                y[j + 16] = (float)q1 * d + m;
            } else {
                y[j] = (float)(q0 - 16) * d;
                y[j + 16] = (float)(q1 - 16) * d;
            }
        }
    }
}

void print_array(const char* name, const float* a, int count) {  // utils.h:63-71
    printf("---------------- %s ------------------\n", name);
    for (int i = 0; i < count; i++) printf("%0.4ff, ", a[i]);
    printf("\n");
}

int parse_type(const std::string& s) {
    if (s == "f16") return FATTN_TYPE_F16;
    if (s == "q8_0") return FATTN_TYPE_Q8_0;
    if (s == "q4_0") return FATTN_TYPE_Q4_0;
    if (s == "q4_1") return FATTN_TYPE_Q4_1;
    if (s == "q5_0") return FATTN_TYPE_Q5_0;
    if (s == "q5_1") return FATTN_TYPE_Q5_1;
    if (s == "bf16") return FATTN_TYPE_BF16;
    fprintf(stderr, "unknown --kv-type %s\n", s.c_str());
    exit(2);
}

// --mla: multi-head latent attention, K rows of 576 f16, V the 512 elements of
// the same rows from element v_off on (one kv head; include/fattn.h).  The CPU
// reference is cpu_reference's arithmetic over the two row lengths: operands
// rounded through fp16, fp32 accumulation, single-pass online softmax, P
// rounded to f16.  q [NQ][H][576], kv [N][576], mask [NQ][N], out [NQ][H][512].
constexpr int kMlaDK = 576, kMlaDV = 512;

void cpu_reference_mla(const std::vector<float>& q, const std::vector<float>& kv, const std::vector<float>& mask,
                       std::vector<float>& out, int N, int H, int NQ, int v_off, float scale, int threads,
                       std::vector<float>* lse = nullptr) {
    std::vector<float> qh(q.size()), kh(kv.size());
    for (size_t i = 0; i < q.size(); i++) qh[i] = rh(q[i]);
    for (size_t i = 0; i < kv.size(); i++) kh[i] = rh(kv[i]);
    auto head = [&](int h) {
        std::vector<float> s(N);
        for (int row = 0; row < NQ; row++) {
            const float* qq = qh.data() + ((size_t)row * H + h) * kMlaDK;
            const float* mrow = mask.data() + (size_t)row * N;
            for (int c = 0; c < N; c++) {
                float acc = 0.0f;
                for (int i = 0; i < kMlaDK; i++) {
                    const float p = qq[i] * kh[(size_t)c * kMlaDK + i];
                    acc = acc + p;
                }
                s[c] = acc * scale + mrow[c];
            }
            float M = -INFINITY, S = 0.0f;
            for (int i = 0; i < N; i++) {
                if (s[i] > M) {
                    S = 1.0f + S * expf(M - s[i]);
                    M = s[i];
                } else {
                    S += expf(s[i] - M);
                }
            }
            for (int i = 0; i < N; i++) s[i] = rh(expf(s[i] - M) / S);
            if (lse) (*lse)[(size_t)row * H + h] = row_lse(M, S, nullptr);
            float* o = out.data() + ((size_t)row * H + h) * kMlaDV;
            for (int c = 0; c < kMlaDV; c++) {
                float acc = 0.0f;
                for (int i = 0; i < N; i++) {
                    const float p = s[i] * kh[(size_t)i * kMlaDK + v_off + c];
                    acc = acc + p;
                }
                o[c] = acc;
            }
        }
    };
    threads = std::max(1, std::min(threads, H));
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (int h = t; h < H; h += threads) head(h);
        });
    for (auto& th : pool) th.join();
}

// ggml's quantize_row_q8_0_ref / quantize_row_q4_0_ref and their dequantisation
// in plain C++ (every operation rounded on its own): `rows` rows of D values.
// The --mla --cpu-only path has no device to quantise on.
void quant_host_q80_q40(int type, const float* src, uint8_t* dst, int D, int64_t rows) {
    const int bb = type == FATTN_TYPE_Q8_0 ? 34 : 18;
    for (int64_t i = 0; i < rows * (D / 32); i++) {
        const float* x = src + i * 32;
        uint8_t* b = dst + i * bb;
        float amax = 0.0f, mx = 0.0f;
        for (int j = 0; j < 32; j++)
            if (amax < fabsf(x[j])) amax = fabsf(x[j]), mx = x[j];
        const float d = type == FATTN_TYPE_Q8_0 ? amax / 127.0f : mx / -8.0f;
        const float id = d ? 1.0f / d : 0.0f;
        const uint16_t dh = f2h(d);
        b[0] = (uint8_t)(dh & 0xFF), b[1] = (uint8_t)(dh >> 8);
        if (type == FATTN_TYPE_Q8_0) {
            for (int j = 0; j < 32; j++) b[2 + j] = (uint8_t)(int8_t)roundf(x[j] * id);
        } else {
            for (int j = 0; j < 16; j++) {
                const uint8_t q0 = (uint8_t)std::min(15, (int)(int8_t)(x[j] * id + 8.5f));
                const uint8_t q1 = (uint8_t)std::min(15, (int)(int8_t)(x[j + 16] * id + 8.5f));
                b[2 + j] = (uint8_t)(q0 | (q1 << 4));
            }
        }
    }
}
void dequant_host_q80_q40(int type, const uint8_t* src, float* dst, int D, int64_t rows) {
    const int bb = type == FATTN_TYPE_Q8_0 ? 34 : 18;
    for (int64_t i = 0; i < rows * (D / 32); i++) {
        const uint8_t* b = src + i * bb;
        const float d = h2f((uint16_t)(b[0] | (b[1] << 8)));
        float* y = dst + i * 32;
        if (type == FATTN_TYPE_Q8_0) {
            for (int j = 0; j < 32; j++) y[j] = (float)(int8_t)b[2 + j] * d;
        } else {
            for (int j = 0; j < 16; j++) {
                y[j] = (float)((b[2 + j] & 0x0F) - 8) * d;
                y[j + 16] = (float)((b[2 + j] >> 4) - 8) * d;
            }
        }
    }
}

// the --mla flow: inputs from rand() in the order Q, KV, mask; the CPU
// reference; fattn_ext with V = K + v_off elements; timing and the verification
// line of the other branches.  --kv-type q8_0 | q4_0: the cache rows are
// quantised (fattn_quantize; on the host with --cpu-only), the reference takes
// the blocks dequantised on the host, and V is the view v_off / 32 blocks in.
int run_mla(int H, int N, int NQ, int v_off, int kv_type, const std::string& mask_kind, bool cpu_only, int iters, float tol,
            const char* dump, bool use_lse) {
    const bool quant = kv_type == FATTN_TYPE_Q8_0 || kv_type == FATTN_TYPE_Q4_0;
    if (kv_type != FATTN_TYPE_F16 && !quant) {
        fprintf(stderr, "--mla: --kv-type f16|q8_0|q4_0\n");
        return 2;
    }
    if (H <= 0 || N <= 0 || NQ <= 0 || (v_off != 0 && v_off != kMlaDK - kMlaDV && !(quant && v_off == 32))) {
        fprintf(stderr, "--mla: --heads, --kv-size, --n-q positive, --v-off 0|64 (q8_0 / q4_0: 0|32|64)\n");
        return 2;
    }
    const float scale = 1.0f / sqrtf(192.0f);  // the model family's: 128 nope + 64 rope dims before absorption
    std::vector<float> query((size_t)kMlaDK * H * NQ), kv((size_t)kMlaDK * N), mask((size_t)N * NQ);
    random_fill(query);
    random_fill(kv);
    random_fill(mask);
    if (mask_kind != "random") std::fill(mask.begin(), mask.end(), 0.0f);
    const size_t rowb = quant ? fattn_row_size(kv_type, kMlaDK) : (size_t)kMlaDK * 2;
    std::vector<uint8_t> blocks;
    if (quant) {
        blocks.resize(rowb * N);
        if (cpu_only) {
            quant_host_q80_q40(kv_type, kv.data(), blocks.data(), kMlaDK, N);
        } else {
            float* d_f;
            void* d_b;
            HIP_CHECK(hipMalloc(&d_f, 4 * kv.size()));
            HIP_CHECK(hipMalloc(&d_b, blocks.size()));
            HIP_CHECK(hipMemcpy(d_f, kv.data(), 4 * kv.size(), hipMemcpyHostToDevice));
            const int qrc = fattn_quantize(kv_type, d_f, d_b, kMlaDK, N, nullptr);
            if (qrc) {
                fprintf(stderr, "quantize failed: %s\n", fattn_strerror(qrc));
                return 2;
            }
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(blocks.data(), d_b, blocks.size(), hipMemcpyDeviceToHost));
            HIP_CHECK(hipFree(d_f));
            HIP_CHECK(hipFree(d_b));
        }
        dequant_host_q80_q40(kv_type, blocks.data(), kv.data(), kMlaDK, N);  // (the reference rounds to f16: h(q d))
    }
    const int threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    std::vector<float> ref((size_t)kMlaDV * H * NQ), got(ref.size());
    std::vector<float> lse_ref((size_t)H * NQ), lse_got(lse_ref.size());
    cpu_reference_mla(query, kv, mask, ref, N, H, NQ, v_off, scale, threads, use_lse ? &lse_ref : nullptr);
    print_array("Reference", ref.data(), 16);
    if (use_lse) print_array("Reference LSE", lse_ref.data(), std::min(16, H * NQ));
    if (cpu_only) {
        if (dump) {
            FILE* f = fopen(dump, "wb");
            if (!f || fwrite(ref.data(), sizeof(float), ref.size(), f) != ref.size()) {
                fprintf(stderr, "cannot write %s\n", dump);
                return 2;
            }
            fclose(f);
            if (use_lse && !dump_floats((std::string(dump) + ".lse").c_str(), lse_ref)) return 2;
        }
        return 0;
    }
    const bool has_mask = mask_kind != "none";
    const int mask_rows = (NQ + 31) / 32 * 32, Np = N + (N & 1);
    std::vector<uint16_t> mask16((size_t)Np * mask_rows, f2h(0.0f));
    if (!quant) {
        blocks.resize(rowb * N);
        uint16_t* kv16 = (uint16_t*)blocks.data();
        for (size_t i = 0; i < kv.size(); i++) kv16[i] = f2h(kv[i]);
    }
    for (int r = 0; r < NQ; r++)
        for (int i = 0; i < N; i++) mask16[(size_t)r * Np + i] = f2h(mask[(size_t)r * N + i]);
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    float *d_q, *d_out, *d_lse = nullptr;
    void *d_kv, *d_mask, *d_ws;
    if (use_lse) HIP_CHECK(hipMalloc(&d_lse, 4 * lse_got.size()));
    HIP_CHECK(hipMalloc(&d_q, 4 * query.size()));
    HIP_CHECK(hipMalloc(&d_out, 4 * got.size()));
    HIP_CHECK(hipMalloc(&d_kv, blocks.size()));
    HIP_CHECK(hipMalloc(&d_mask, 2 * mask16.size()));
    HIP_CHECK(hipMemcpyAsync(d_q, query.data(), 4 * query.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_kv, blocks.data(), blocks.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_mask, mask16.data(), 2 * mask16.size(), hipMemcpyHostToDevice, st));
    fattn_params p;
    std::memset(&p, 0, sizeof(p));
    const int64_t rk = (int64_t)rowb, eb = quant ? (int64_t)fattn_row_size(kv_type, 32) : 2;
    p.q = {d_q, FATTN_TYPE_F32, 0, {kMlaDK, NQ, H, 1}, {4, (int64_t)H * kMlaDK * 4, kMlaDK * 4, (int64_t)NQ * H * kMlaDK * 4}};
    p.k = {d_kv, kv_type, 0, {kMlaDK, N, 1, 1}, {eb, rk, rk * N, rk * N}};
    // V: a view of the same rows, v_off elements in (ggml_view of the cache's latent part)
    p.v = {(const uint8_t*)d_kv + (quant ? (int64_t)fattn_row_size(kv_type, v_off) : 2 * v_off), kv_type, 0, {kMlaDV, N, 1, 1},
           {eb, rk, rk * N, rk * N}};
    if (has_mask)
        p.mask = {d_mask, FATTN_TYPE_F16, 0, {Np, mask_rows, 1, 1},
                  {2, (int64_t)Np * 2, (int64_t)Np * 2 * mask_rows, (int64_t)Np * 2 * mask_rows}};
    p.dst = d_out;
    p.scale = scale;
    const size_t ws_bytes = std::max<size_t>(fattn_workspace_size(&p), 16);
    HIP_CHECK(hipMalloc(&d_ws, ws_bytes));
    int rc = fattn_workspace_init(d_ws, ws_bytes, st);
    p.workspace = d_ws;
    p.workspace_bytes = ws_bytes;
    rc = rc ? rc : fattn_ext_lse(&p, nullptr, d_lse, st);  // (d_lse null: fattn_ext)
    if (rc) {
        fprintf(stderr, "launch failed: %s\n", fattn_strerror(rc));
        return 2;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    hipEvent_t start, stop;
    HIP_CHECK(hipEventCreate(&start));
    HIP_CHECK(hipEventCreate(&stop));
    std::vector<float> times;
    for (int it = 0; it < iters; it++) {
        HIP_CHECK(hipEventRecord(start, st));
        rc = fattn_ext_lse(&p, nullptr, d_lse, st);
        HIP_CHECK(hipEventRecord(stop, st));
        HIP_CHECK(hipEventSynchronize(stop));
        if (rc) {
            fprintf(stderr, "launch failed: %s\n", fattn_strerror(rc));
            return 2;
        }
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, start, stop));
        times.push_back(ms);
    }
    std::sort(times.begin(), times.end());
    const float millis = times[times.size() / 2];
    HIP_CHECK(hipMemcpy(got.data(), d_out, 4 * got.size(), hipMemcpyDeviceToHost));
    print_array("MLA HIP", got.data(), 16);
    float max_diff = 0.0f, max_ref = 0.0f;
    int row_idx = 0, head_idx = 0, dim_idx = 0;
    for (int r = 0; r < NQ; r++)
        for (int h = 0; h < H; h++) {
            const size_t o = ((size_t)r * H + h) * kMlaDV;
            for (int i = 0; i < kMlaDV; i++) {
                const float dd = fabsf(ref[o + i] - got[o + i]);
                max_ref = std::max(max_ref, fabsf(ref[o + i]));
                if (dd > max_diff || std::isnan(dd)) {
                    max_diff = std::isnan(dd) ? INFINITY : dd;
                    row_idx = r, head_idx = h, dim_idx = i;
                }
            }
        }
    const float worst_rel = max_diff / std::max(max_ref, 1e-30f);
    const double bytes = (double)(kMlaDK + kMlaDV) * H * NQ * 4 + (double)rowb * N + (has_mask ? 2.0 * N * NQ : 0.0);
    const double flops = 2.0 * N * (kMlaDK + kMlaDV) * H * NQ;
    printf("\ncuda time: %.4f ms  (%.1f GB/s, %.3f TFLOP/s; median of %d)\n", millis, bytes / millis / 1e6,
           flops / millis / 1e9, iters);
    const size_t at = ((size_t)row_idx * H + head_idx) * kMlaDV + dim_idx;
    printf("R (%.4f) CUDA(%.4f) diff: %.4f - row = %d, head = %d, dim = %d\n", ref[at], got[at], max_diff, row_idx,
           head_idx, dim_idx);
    printf("checked %d of %d query rows x %d heads; n_q %d, 1 GPU(s)\n", NQ, NQ, H, NQ);
    printf("normwise rel err %.3g (tol %.1g): %s\n", worst_rel, tol, worst_rel <= tol ? "PASS" : "FAIL");
    bool lse_ok = true;
    if (use_lse) {
        HIP_CHECK(hipMemcpy(lse_got.data(), d_lse, 4 * lse_got.size(), hipMemcpyDeviceToHost));
        std::vector<int> all_rows(NQ);
        for (int r = 0; r < NQ; r++) all_rows[r] = r;
        lse_ok = lse_check(lse_ref, lse_got, all_rows, H);
    }
    return worst_rel <= tol && lse_ok ? 0 : 1;
}

// ggml's quantize_row_q4_1_ref / _q5_0_ref / _q5_1_ref in plain C++ (every
// operation rounded on its own; the strict-compare scans keep the first of equals)
void quant_host_ext(int type, const float* src, uint8_t* dst, int D, int64_t rows) {
    const bool has_m = type != FATTN_TYPE_Q5_0, has_qh = type != FATTN_TYPE_Q4_1;
    const int bb = 2 + (has_m ? 2 : 0) + (has_qh ? 4 : 0) + 16;
    for (int64_t i = 0; i < rows * (D / 32); i++) {
        const float* x = src + i * 32;
        uint8_t* b = dst + i * bb;
        float d, mn = 0.0f;
        if (!has_m) {
            float amax = 0.0f, mx = 0.0f;
            for (int j = 0; j < 32; j++)
                if (amax < fabsf(x[j])) amax = fabsf(x[j]), mx = x[j];
            d = mx / -16.0f;
        } else {
            float mxv = -3.402823466e+38f;
            mn = 3.402823466e+38f;
            for (int j = 0; j < 32; j++) {
                if (x[j] < mn) mn = x[j];
                if (x[j] > mxv) mxv = x[j];
            }
            d = (mxv - mn) / (type == FATTN_TYPE_Q4_1 ? 15.0f : 31.0f);
            const uint16_t mh = f2h(mn);
            b[2] = (uint8_t)(mh & 0xFF), b[3] = (uint8_t)(mh >> 8);
        }
        const float id = d ? 1.0f / d : 0.0f;
        const uint16_t dh = f2h(d);
        b[0] = (uint8_t)(dh & 0xFF), b[1] = (uint8_t)(dh >> 8);
        auto code = [&](float v) -> uint32_t {
            if (type == FATTN_TYPE_Q5_0) return (uint32_t)std::min(31, (int)(int8_t)(v * id + 16.5f));
            if (type == FATTN_TYPE_Q4_1) return (uint32_t)std::min(15, (int)(int8_t)((v - mn) * id + 0.5f));
            return (uint8_t)((v - mn) * id + 0.5f);
        };
        uint32_t qh = 0;
        uint8_t* qs = b + bb - 16;
        for (int j = 0; j < 16; j++) {
            const uint32_t q0 = code(x[j]), q1 = code(x[j + 16]);
            qs[j] = (uint8_t)((q0 & 0x0F) | ((q1 & 0x0F) << 4));
            qh |= ((q0 >> 4) & 1u) << j;
            qh |= ((q1 >> 4) & 1u) << (j + 16);
        }
        if (has_qh) {
            uint8_t* hp = b + (has_m ? 4 : 2);
            hp[0] = (uint8_t)qh, hp[1] = (uint8_t)(qh >> 8), hp[2] = (uint8_t)(qh >> 16), hp[3] = (uint8_t)(qh >> 24);
        }
    }
}

// rows of any cache type on the host: f32 -> bytes and back
void encode_host(int type, const float* src, uint8_t* dst, int D, int64_t rows) {
    if (type == FATTN_TYPE_F16 || type == FATTN_TYPE_BF16) {
        uint16_t* h = (uint16_t*)dst;
        for (int64_t i = 0; i < rows * D; i++) {
            if (type == FATTN_TYPE_F16) {
                h[i] = f2h(src[i]);
            } else {
                const float r = round_bf16(src[i]);
                uint32_t u;
                std::memcpy(&u, &r, 4);
                h[i] = (uint16_t)(u >> 16);
            }
        }
    } else if (is_kv_ext(type)) {
        quant_host_ext(type, src, dst, D, rows);
    } else {
        quant_host_q80_q40(type, src, dst, D, rows);
    }
}
void decode_host(int type, const uint8_t* src, float* dst, int D, int64_t rows) {
    if (type == FATTN_TYPE_F16 || type == FATTN_TYPE_BF16) {
        const uint16_t* h = (const uint16_t*)src;
        for (int64_t i = 0; i < rows * D; i++) {
            if (type == FATTN_TYPE_F16) {
                dst[i] = h2f(h[i]);
            } else {
                const uint32_t u = (uint32_t)h[i] << 16;
                std::memcpy(&dst[i], &u, 4);
            }
        }
    } else if (is_kv_ext(type)) {
        dequant_host(type, src, dst, D, rows);
    } else {
        dequant_host_q80_q40(type, src, dst, D, rows);
    }
}

// include/fattn.h's rotation of one row by the position delta p, in plain C++
// (n_dims = D, freq_base 10000, freq_scale 1, no YaRN, attn_factor 1)
void rope_row_host(float* x, int D, int p, bool neox) {
    const float theta_scale = powf(10000.0f, -2.0f / (float)D);
    for (int i = 0; i < D / 2; i++) {
        const float theta = (float)p * powf(theta_scale, (float)i);
        const float c = cosf(theta), s = sinf(theta);
        float& x0 = x[neox ? i : 2 * i];
        float& x1 = x[neox ? i + D / 2 : 2 * i + 1];
        const float y0 = x0 * c - x1 * s, y1 = x0 * s + x1 * c;
        x0 = y0, x1 = y1;
    }
}

// the --k-shift flow: inputs from rand() in the order Q, K, V, mask; the K / V
// caches [Hkv][N][row] of --kv-type encoded on the host; fattn_k_shift rotates
// every slot of the K cache by DELTA on the GPU (one shift tensor in device
// memory); the host recomputes the same (decode, rope_row_host, encode) and the
// CPU reference attends over THAT cache; fattn_ext attends over the GPU's.  The
// verification line is that of the other branches.  --cpu-only: the host's
// shift and the reference alone.
int run_k_shift(int delta, bool neox, int D, int H, int Hkv, int N, int kv_type, const std::string& mask_kind, bool cpu_only,
                int iters, float tol) {
    const size_t rb = fattn_row_size(kv_type, D);
    if (H <= 0 || Hkv <= 0 || N <= 0 || H % Hkv || rb == 0 || D % 32 || D > 256 || D < 32) {
        fprintf(stderr, "--k-shift: heads a positive multiple of kv-heads, head-dim a multiple of 32 up to 256\n");
        return 2;
    }
    const float scale = 1.0f / sqrtf((float)D);
    std::vector<float> query((size_t)D * H), key((size_t)D * N * Hkv), value((size_t)D * N * Hkv), mask((size_t)N);
    random_fill(query);
    random_fill(key);
    random_fill(value);
    random_fill(mask);
    if (mask_kind != "random") std::fill(mask.begin(), mask.end(), 0.0f);
    const int64_t nrows = (int64_t)N * Hkv;
    std::vector<uint8_t> kbytes(rb * nrows), vbytes(rb * nrows), kshift(rb * nrows);
    encode_host(kv_type, key.data(), kbytes.data(), D, nrows);
    encode_host(kv_type, value.data(), vbytes.data(), D, nrows);
    // the host's shift: what the cache holds -> rotated -> what the cache then holds
    std::vector<float> kref(key.size()), vref(value.size());
    decode_host(kv_type, kbytes.data(), kref.data(), D, nrows);
    decode_host(kv_type, vbytes.data(), vref.data(), D, nrows);
    if (delta != 0) {
        for (int64_t r = 0; r < nrows; r++) rope_row_host(&kref[(size_t)r * D], D, delta, neox);
        encode_host(kv_type, kref.data(), kshift.data(), D, nrows);
        decode_host(kv_type, kshift.data(), kref.data(), D, nrows);
    } else {
        kshift = kbytes;  // (a zero delta touches nothing)
    }
    const int threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    std::vector<float> ref((size_t)D * H), got(ref.size());
    cpu_reference(query, kref, vref, mask, ref, N, D, H, Hkv, scale, {0}, threads);
    printf("k-shift: %s cache [%d][%d][%d], every slot by %d, rope mode %s\n", type_name(kv_type), Hkv, N, D, delta,
           neox ? "neox" : "norm");
    print_array("Reference", ref.data(), std::min(16, D * H));
    if (cpu_only) return 0;

    const bool has_mask = mask_kind != "none";
    const int Np = N + (N & 1);
    std::vector<uint16_t> mask16((size_t)Np * 32, f2h(0.0f));
    for (int i = 0; i < N; i++) mask16[i] = f2h(mask[i]);
    std::vector<int32_t> shift(N, delta);
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    float *d_q, *d_out;
    void *d_k, *d_v, *d_mask, *d_ws, *d_shift;
    HIP_CHECK(hipMalloc(&d_q, 4 * query.size()));
    HIP_CHECK(hipMalloc(&d_out, 4 * got.size()));
    HIP_CHECK(hipMalloc(&d_k, kbytes.size()));
    HIP_CHECK(hipMalloc(&d_v, vbytes.size()));
    HIP_CHECK(hipMalloc(&d_mask, 2 * mask16.size()));
    HIP_CHECK(hipMalloc(&d_shift, 4 * shift.size()));
    HIP_CHECK(hipMemcpyAsync(d_q, query.data(), 4 * query.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_k, kbytes.data(), kbytes.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_v, vbytes.data(), vbytes.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_mask, mask16.data(), 2 * mask16.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_shift, shift.data(), 4 * shift.size(), hipMemcpyHostToDevice, st));
    const int64_t eb = kv_type == FATTN_TYPE_F16 || kv_type == FATTN_TYPE_BF16 ? 2 : (int64_t)fattn_row_size(kv_type, 32);
    const fattn_tensor tk = {d_k, kv_type, 0, {D, N, Hkv, 1}, {eb, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkv}};
    const fattn_tensor ts = {d_shift, FATTN_TYPE_I32, 0, {N, 1, 1, 1}, {4, 4 * (int64_t)N, 4 * (int64_t)N, 4 * (int64_t)N}};
    const fattn_rope rope = {D, neox ? 2 : 0, 0, 10000.0f, 1.0f, 0.0f, 1.0f, 32.0f, 1.0f};
    hipEvent_t start, stop;
    HIP_CHECK(hipEventCreate(&start));
    HIP_CHECK(hipEventCreate(&stop));
    HIP_CHECK(hipEventRecord(start, st));
    int rc = fattn_k_shift(&tk, &ts, nullptr, &rope, st);
    HIP_CHECK(hipEventRecord(stop, st));
    if (rc) {
        fprintf(stderr, "k_shift failed: %s\n", fattn_strerror(rc));
        return 2;
    }
    HIP_CHECK(hipEventSynchronize(stop));
    float shift_ms = 0;
    HIP_CHECK(hipEventElapsedTime(&shift_ms, start, stop));
    std::vector<uint8_t> kgot(kbytes.size());
    HIP_CHECK(hipMemcpy(kgot.data(), d_k, kgot.size(), hipMemcpyDeviceToHost));
    int64_t differ = 0;
    for (size_t i = 0; i < kgot.size(); i++) differ += kgot[i] != kshift[i];
    std::vector<float> kdev(key.size());
    decode_host(kv_type, kgot.data(), kdev.data(), D, nrows);
    float max_dx = 0.0f, max_x = 0.0f;
    for (size_t i = 0; i < kdev.size(); i++) {
        const float dd = fabsf(kdev[i] - kref[i]);
        max_dx = std::isnan(dd) ? INFINITY : std::max(max_dx, dd);
        max_x = std::max(max_x, fabsf(kref[i]));
    }
    printf("k-shift: one launch %.4f ms (first call); %lld of %zu cache bytes differ from the host's shift, max |dx| %.3g of max |x| %.3g\n",
           shift_ms, (long long)differ, kgot.size(), max_dx, max_x);

    fattn_params p;
    std::memset(&p, 0, sizeof(p));
    p.q = {d_q, FATTN_TYPE_F32, 0, {D, 1, H, 1}, {4, (int64_t)H * D * 4, (int64_t)D * 4, (int64_t)H * D * 4}};
    p.k = tk;
    p.v = {d_v, kv_type, 0, {D, N, Hkv, 1}, {eb, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkv}};
    if (has_mask) p.mask = {d_mask, FATTN_TYPE_F16, 0, {Np, 32, 1, 1}, {2, (int64_t)Np * 2, (int64_t)Np * 64, (int64_t)Np * 64}};
    p.dst = d_out;
    p.scale = scale;
    const size_t ws_bytes = std::max<size_t>(fattn_workspace_size(&p), 16);
    HIP_CHECK(hipMalloc(&d_ws, ws_bytes));
    rc = fattn_workspace_init(d_ws, ws_bytes, st);
    p.workspace = d_ws;
    p.workspace_bytes = ws_bytes;
    std::vector<float> times;
    for (int it = 0; it < iters && !rc; it++) {
        HIP_CHECK(hipEventRecord(start, st));
        rc = fattn_ext(&p, st);
        HIP_CHECK(hipEventRecord(stop, st));
        HIP_CHECK(hipEventSynchronize(stop));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, start, stop));
        times.push_back(ms);
    }
    if (rc) {
        fprintf(stderr, "launch failed: %s\n", fattn_strerror(rc));
        return 2;
    }
    std::sort(times.begin(), times.end());
    HIP_CHECK(hipMemcpy(got.data(), d_out, 4 * got.size(), hipMemcpyDeviceToHost));
    print_array("K-shift HIP", got.data(), std::min(16, D * H));
    float max_diff = 0.0f, max_ref = 0.0f;
    int head_idx = 0, dim_idx = 0;
    for (int h = 0; h < H; h++)
        for (int i = 0; i < D; i++) {
            const float dd = fabsf(ref[(size_t)h * D + i] - got[(size_t)h * D + i]);
            max_ref = std::max(max_ref, fabsf(ref[(size_t)h * D + i]));
            if (dd > max_diff || std::isnan(dd)) {
                max_diff = std::isnan(dd) ? INFINITY : dd;
                head_idx = h, dim_idx = i;
            }
        }
    const float worst_rel = max_diff / std::max(max_ref, 1e-30f);
    printf("\ncuda time: %.4f ms  (attention over the shifted cache; median of %d)\n", times[times.size() / 2], iters);
    const size_t at = (size_t)head_idx * D + dim_idx;
    printf("R (%.4f) CUDA(%.4f) diff: %.4f - row = 0, head = %d, dim = %d\n", ref[at], got[at], max_diff, head_idx, dim_idx);
    printf("checked 1 of 1 query rows x %d heads; n_q 1, 1 GPU(s)\n", H);
    printf("normwise rel err %.3g (tol %.1g): %s\n", worst_rel, tol, worst_rel <= tol ? "PASS" : "FAIL");
    return worst_rel <= tol ? 0 : 1;
}

}  // namespace

#define RCCL_CHECK(x)                                                                           \
    do {                                                                                          \
        ncclResult_t r_ = (x);                                                                    \
        if (r_ != ncclSuccess) {                                                                  \
            fprintf(stderr, "RCCL error %s at %s:%d (%s)\n", ncclGetErrorString(r_), __FILE__, __LINE__, #x); \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

int main(int argc, const char* argv[]) {
    int kv_size = 512, num_warps = 8, head_dim = 128, num_heads = 32, num_kv_heads = 8, iters = 20;
    int kv_type = FATTN_TYPE_F16, n_q = 1, check_rows = 64, ngpu = 1;
    bool parallel_kv = true, cpu_only = false, use_lse = false;
    std::string mask_kind = "random";
    const char* dump = nullptr;
    float tol = 1e-3f, max_bias = 0.0f, softcap = 0.0f, sink_base = 0.0f;
    bool use_sinks = false, set_rows = false, mla = false, heads_given = false;
    int mla_v_off = 0, k_shift_delta = 0;
    bool k_shift = false, rope_neox = true;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (++i >= argc) {
                fprintf(stderr, "missing value for %s\n", a.c_str());
                exit(2);
            }
            return argv[i];
        };
        if (a == "--no-kv-parallel") parallel_kv = false;
        else if (a == "--n-warps") num_warps = atoi(next());
        else if (a == "--kv-size") kv_size = atoi(next());
        else if (a == "--cpu-only") cpu_only = true;
        else if (a == "--set-rows") set_rows = true;
        else if (a == "--dump") dump = next();
        else if (a == "--kv-type") kv_type = parse_type(next());
        else if (a == "--head-dim") head_dim = atoi(next());
        else if (a == "--heads") num_heads = atoi(next()), heads_given = true;
        else if (a == "--kv-heads") num_kv_heads = atoi(next());
        else if (a == "--iters") iters = std::max(1, atoi(next()));
        else if (a == "--tol") tol = (float)atof(next());
        else if (a == "--n-q") n_q = atoi(next());
        else if (a == "--check-rows") check_rows = std::max(1, atoi(next()));
        else if (a == "--ngpu") ngpu = atoi(next());
        else if (a == "--max-bias") max_bias = (float)atof(next());
        else if (a == "--softcap") softcap = (float)atof(next());
        else if (a == "--sinks") sink_base = (float)atof(next()), use_sinks = true;
        else if (a == "--mla") mla = true;
        else if (a == "--lse") use_lse = true;
        else if (a == "--v-off") mla_v_off = atoi(next());
        else if (a == "--k-shift") k_shift = true, k_shift_delta = atoi(next());
        else if (a == "--rope-mode") {
            const std::string m = next();
            if (m != "norm" && m != "neox") {
                fprintf(stderr, "--rope-mode norm|neox\n");
                return 2;
            }
            rope_neox = m == "neox";
        }
        else if (a == "--mask") {
            mask_kind = next();
            if (mask_kind != "random" && mask_kind != "zero" && mask_kind != "none") {
                fprintf(stderr, "--mask random|zero|none\n");
                return 2;
            }
        } else if (a == "--config") {
            // BASELINE.json configs[N - 1] (and SURVEY 8(d)'s prefill shape)
            const std::string c = next();
            if (c == "1") {
                cpu_only = true, num_heads = num_kv_heads = 1, head_dim = 64, kv_size = 128;
            } else if (c == "2") {
                kv_type = FATTN_TYPE_F16, num_heads = num_kv_heads = 32, head_dim = 128, kv_size = 2048;
            } else if (c == "3") {
                parallel_kv = false, kv_type = FATTN_TYPE_Q8_0, num_heads = num_kv_heads = 32, kv_size = 4096;
            } else if (c == "4") {
                parallel_kv = false, kv_type = FATTN_TYPE_Q4_0, num_heads = 32, num_kv_heads = 8, kv_size = 8192;
            } else if (c == "5") {
                parallel_kv = false, kv_type = FATTN_TYPE_Q8_0, num_heads = num_kv_heads = 32, kv_size = 4096,
                n_q = 64;
            } else if (c == "prefill") {
                parallel_kv = false, kv_type = FATTN_TYPE_Q8_0, num_heads = num_kv_heads = 32, kv_size = 4096,
                n_q = 4096, mask_kind = "zero";
            } else {
                fprintf(stderr, "--config 1|2|3|4|5|prefill\n");
                return 2;
            }
        } else {
            fprintf(stderr, "unknown flag %s\n", a.c_str());
            return 2;
        }
    }
    if (num_warps != 8 && num_warps != 4 && num_warps != 2 && num_warps != 1)
        printf("invalid num_warps, should be 2, 4, 8\n");  // kernel_test.h:176-178 (informational)
    if (!cpu_only) kv_size = std::max(256, kv_size);      // kernel_test.h:14-18
    if (k_shift)
        return run_k_shift(k_shift_delta, rope_neox, head_dim, num_heads, num_kv_heads, kv_size, kv_type, mask_kind, cpu_only, iters, tol);
    // (the model family's smallest head count unless --heads says otherwise)
    if (mla) return run_mla(heads_given ? num_heads : 16, kv_size, n_q, mla_v_off, kv_type, mask_kind, cpu_only, iters, tol, dump, use_lse);
    if (n_q > 1 || ngpu > 1) parallel_kv = false;        // flash_attn_row is one query row on one device
    const bool op_xf = max_bias != 0.0f || softcap != 0.0f;
    if (op_xf) parallel_kv = false;                      // (neither positional list carries the two scalars)
    if (use_sinks) parallel_kv = false;                  // (nor the sinks: fattn_ext_sinks takes fattn_params)
    if (set_rows) parallel_kv = false;                   // (SET_ROWS writes rows: no transposed V)
    if (use_lse) parallel_kv = false;                    // (fattn_ext_lse takes fattn_params)
    if (use_lse && ngpu > 1) {
        fprintf(stderr, "--lse runs on one device\n");
        return 2;
    }

    const int D = head_dim, H = num_heads, Hkv = num_kv_heads, N = kv_size, NQ = n_q;
    const float scale = 1.0f / sqrtf((float)D);
    if (H <= 0 || Hkv <= 0 || N <= 0 || D <= 0 || NQ <= 0 || H % Hkv) {
        fprintf(stderr, "heads must be a positive multiple of kv-heads\n");
        return 2;
    }
    if (ngpu < 1 || Hkv % ngpu) {
        fprintf(stderr, "--ngpu must divide the kv heads (%d)\n", Hkv);
        return 2;
    }
    // the rand() stream in kernel_test.h:45-48's order: Q, K, V, then the mask
    // (n_q rows; row 0 is the reference's one mask row)
    std::vector<float> query((size_t)D * H * NQ), key((size_t)D * N * Hkv), value((size_t)D * N * Hkv),
        mask((size_t)N * NQ);
    random_fill(query);
    random_fill(key);
    random_fill(value);
    random_fill(mask);
    if (mask_kind != "random") std::fill(mask.begin(), mask.end(), 0.0f);  // "none": zeros on the CPU, no mask on the GPU
    // --set-rows: row n of K / V lands in slot perm[n] (Fisher-Yates over an LCG of
    // its own: the rand() stream above stays the reference's); from here on key,
    // value and the mask columns are in slot order, key_src / value_src as drawn
    std::vector<int64_t> perm;
    std::vector<float> key_src, value_src;
    if (set_rows && !cpu_only) {
        perm.resize(N);
        for (int n = 0; n < N; n++) perm[n] = n;
        uint64_t lcg = 0x9E3779B97F4A7C15ull;
        for (int n = N - 1; n > 0; n--) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(perm[n], perm[(lcg >> 33) % (uint64_t)(n + 1)]);
        }
        key_src = key, value_src = value;
        const std::vector<float> mask_src = mask;
        for (int h = 0; h < Hkv; h++)
            for (int n = 0; n < N; n++) {
                std::memcpy(&key[((size_t)h * N + perm[n]) * D], &key_src[((size_t)h * N + n) * D], sizeof(float) * D);
                std::memcpy(&value[((size_t)h * N + perm[n]) * D], &value_src[((size_t)h * N + n) * D], sizeof(float) * D);
            }
        for (int r = 0; r < NQ; r++)
            for (int n = 0; n < N; n++) mask[(size_t)r * N + perm[n]] = mask_src[(size_t)r * N + n];
    }
    // the query rows the CPU reference checks: all of them, or check_rows at
    // the start, middle and end of the sequence
    std::vector<int> rows;
    if (NQ <= 3 * check_rows) {
        for (int i = 0; i < NQ; i++) rows.push_back(i);
    } else {
        for (int b : {0, NQ / 2 - check_rows / 2, NQ - check_rows})
            for (int i = 0; i < check_rows; i++) rows.push_back(b + i);
    }
    const int threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    std::vector<float> sinks(H);
    for (int h = 0; h < H; h++) sinks[h] = sink_base + 0.25f * (float)(h % 8);
    const std::vector<float>* sinks_ref = use_sinks ? &sinks : nullptr;

    if (cpu_only) {  // BASELINE config 1: kernel_test.h:50-66 on the host, nothing else
        std::vector<float> out((size_t)D * H * NQ), lse((size_t)H * NQ);
        cpu_reference(query, key, value, mask, out, N, D, H, Hkv, scale, rows, threads, max_bias, softcap, sinks_ref,
                      use_lse ? &lse : nullptr);
        print_array("Reference", out.data(), std::min(16, D * H));
        if (use_lse) print_array("Reference LSE", lse.data(), std::min(16, H * NQ));
        if (dump) {
            FILE* f = fopen(dump, "wb");
            if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) {
                fprintf(stderr, "cannot write %s\n", dump);
                return 2;
            }
            fclose(f);
            if (use_lse && !dump_floats((std::string(dump) + ".lse").c_str(), lse)) return 2;
        }
        return 0;
    }

    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ngpu > ndev) {
        fprintf(stderr, "--ngpu %d but %d devices\n", ngpu, ndev);
        return 2;
    }
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, 0));
    printf("GPU: %s (%s), CUs: %d, LDS/block max: %zu KB, HBM: %zu MB%s\n", prop.name, prop.gcnArchName,
           prop.multiProcessorCount, prop.sharedMemPerBlock / 1024, prop.totalGlobalMem >> 20,
           ngpu > 1 ? " (x --ngpu)" : "");

    // K/V values as the kernels see them: f16 rounding on the host, or
    // quantised on device 0 (fattn_quantize) and dequantised back for the CPU
    // reference (fattn_dequantize; Q4_1 / Q5_0 / Q5_1: dequant_host)
    const size_t rb = fattn_row_size(kv_type, D);
    std::vector<float> kref = key, vref = value;
    std::vector<uint8_t> kbytes(rb * N * Hkv), vbytes(rb * N * Hkv);
    const bool vtrans = parallel_kv && kv_type == FATTN_TYPE_F16;
    {
        HIP_CHECK(hipSetDevice(0));
        hipStream_t st0;
        HIP_CHECK(hipStreamCreate(&st0));
        if (kv_type == FATTN_TYPE_F16 && !set_rows) {
            uint16_t* k16 = (uint16_t*)kbytes.data();
            uint16_t* v16 = (uint16_t*)vbytes.data();
            for (size_t i = 0; i < key.size(); i++) k16[i] = f2h(key[i]);
            for (int h = 0; h < Hkv; h++)
                for (int n = 0; n < N; n++)
                    for (int d = 0; d < D; d++) {
                        const size_t src = ((size_t)h * N + n) * D + d;
                        const size_t dst = vtrans ? ((size_t)h * D + d) * N + n : src;
                        v16[dst] = f2h(value[src]);
                    }
        } else {
            float *d_kf, *d_vf;
            void *d_kq, *d_vq;
            HIP_CHECK(hipMalloc(&d_kf, sizeof(float) * key.size()));
            HIP_CHECK(hipMalloc(&d_vf, sizeof(float) * value.size()));
            HIP_CHECK(hipMalloc(&d_kq, kbytes.size()));
            HIP_CHECK(hipMalloc(&d_vq, vbytes.size()));
            HIP_CHECK(hipMemcpyAsync(d_kf, key.data(), 4 * key.size(), hipMemcpyHostToDevice, st0));
            HIP_CHECK(hipMemcpyAsync(d_vf, value.data(), 4 * value.size(), hipMemcpyHostToDevice, st0));
            int rc;
            void* d_idx = nullptr;
            if (set_rows) {
                // ggml_set_rows(cache, cur, idxs) per tensor: f32 [D, N, Hkv] rows as drawn,
                // one I64 index row for every head, the cache [Hkv][N][row]
                HIP_CHECK(hipMemcpyAsync(d_kf, key_src.data(), 4 * key.size(), hipMemcpyHostToDevice, st0));
                HIP_CHECK(hipMemcpyAsync(d_vf, value_src.data(), 4 * value.size(), hipMemcpyHostToDevice, st0));
                HIP_CHECK(hipMalloc(&d_idx, sizeof(int64_t) * N));
                HIP_CHECK(hipMemcpyAsync(d_idx, perm.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, st0));
                const int64_t eb = kv_type == FATTN_TYPE_F16 ? 2 : (int64_t)fattn_row_size(kv_type, 32);
                const fattn_tensor ti = {d_idx, FATTN_TYPE_I64, 0, {N, 1, 1, 1}, {8, 8 * (int64_t)N, 8 * (int64_t)N, 8 * (int64_t)N}};
                fattn_tensor ts = {d_kf, FATTN_TYPE_F32, 0, {D, N, Hkv, 1}, {4, (int64_t)D * 4, (int64_t)D * 4 * N, (int64_t)D * 4 * N * Hkv}};
                fattn_tensor td = {d_kq, kv_type, 0, {D, N, Hkv, 1}, {eb, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkv}};
                rc = fattn_set_rows(&ts, &ti, &td, st0);
                ts.data = d_vf, td.data = d_vq;
                rc = rc ? rc : fattn_set_rows(&ts, &ti, &td, st0);
            } else if (kv_type == FATTN_TYPE_BF16) {
                // the cache write of a bf16 cache: GGML_OP_CPY f32 -> bf16 into the [Hkv][N][row] view
                fattn_tensor ts = {d_kf, FATTN_TYPE_F32, 0, {D, N, Hkv, 1}, {4, (int64_t)D * 4, (int64_t)D * 4 * N, (int64_t)D * 4 * N * Hkv}};
                fattn_tensor td = {d_kq, kv_type, 0, {D, N, Hkv, 1}, {2, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkv}};
                rc = fattn_cpy(&ts, &td, st0);
                ts.data = d_vf, td.data = d_vq;
                rc = rc ? rc : fattn_cpy(&ts, &td, st0);
            } else {
                rc = fattn_quantize(kv_type, d_kf, d_kq, D, (int64_t)N * Hkv, st0);
                rc = rc ? rc : fattn_quantize(kv_type, d_vf, d_vq, D, (int64_t)N * Hkv, st0);
            }
            if (kv_type != FATTN_TYPE_F16 && kv_type != FATTN_TYPE_BF16) {
                rc = rc ? rc : fattn_dequantize(kv_type, d_kq, d_kf, D, (int64_t)N * Hkv, st0);
                rc = rc ? rc : fattn_dequantize(kv_type, d_vq, d_vf, D, (int64_t)N * Hkv, st0);
            }
            if (rc) {
                fprintf(stderr, "%s failed: %s\n", set_rows ? "set_rows" : "quantize", fattn_strerror(rc));
                return 2;
            }
            if (kv_type == FATTN_TYPE_BF16) {  // the reference's values: the bf16 roundings, in plain C++ on the host
                for (auto& x : kref) x = round_bf16(x);
                for (auto& x : vref) x = round_bf16(x);
            } else if (kv_type != FATTN_TYPE_F16) {  // (f16: the reference rounds key / value itself)
                HIP_CHECK(hipMemcpyAsync(kref.data(), d_kf, 4 * key.size(), hipMemcpyDeviceToHost, st0));
                HIP_CHECK(hipMemcpyAsync(vref.data(), d_vf, 4 * value.size(), hipMemcpyDeviceToHost, st0));
            }
            HIP_CHECK(hipMemcpyAsync(kbytes.data(), d_kq, kbytes.size(), hipMemcpyDeviceToHost, st0));
            HIP_CHECK(hipMemcpyAsync(vbytes.data(), d_vq, vbytes.size(), hipMemcpyDeviceToHost, st0));
            HIP_CHECK(hipStreamSynchronize(st0));
            if (is_kv_ext(kv_type)) {  // (the reference's values from the blocks, on the host)
                dequant_host(kv_type, kbytes.data(), kref.data(), D, (int64_t)N * Hkv);
                dequant_host(kv_type, vbytes.data(), vref.data(), D, (int64_t)N * Hkv);
            }
            HIP_CHECK(hipFree(d_kf));
            HIP_CHECK(hipFree(d_vf));
            HIP_CHECK(hipFree(d_kq));
            HIP_CHECK(hipFree(d_vq));
            if (d_idx) HIP_CHECK(hipFree(d_idx));
        }
        HIP_CHECK(hipStreamSynchronize(st0));
        HIP_CHECK(hipStreamDestroy(st0));
    }

    // CPU reference (kernel_test.h:50-66) on the checked rows
    std::vector<float> qkv((size_t)D * H * NQ, 0.0f), qkv_gpu((size_t)D * H * NQ);
    std::vector<float> lse_ref((size_t)H * NQ), lse_gpu(lse_ref.size());
    cpu_reference(query, kref, vref, mask, qkv, N, D, H, Hkv, scale, rows, threads, max_bias, softcap, sinks_ref,
                  use_lse ? &lse_ref : nullptr);
    print_array("Reference", qkv.data(), 16);

    // ---- per device: its head shard (kv heads [g Hkv/G, (g+1) Hkv/G) and their
    // q heads; G = 1: everything), inputs, workspace, stream
    const int G = ngpu, Hl = H / G, Hkvl = Hkv / G;
    // mask f16: one row for flash_attn_row; rows padded to a multiple of 32
    // (row i = query i's mask, the rest zeros) for flash_attn_ext
    // (kernel_test.h:74-85), each padded to an even length (ggml pads to
    // GGML_KQ_MASK_PAD; the kernels read rows in dword pieces)
    const bool has_mask = mask_kind != "none";
    const int mask_rows = parallel_kv ? 1 : (NQ + 31) / 32 * 32;
    const int Np = parallel_kv ? N : N + (N & 1);
    std::vector<uint16_t> mask16((size_t)Np * mask_rows, f2h(0.0f));
    for (int r = 0; r < NQ && r < mask_rows; r++)
        for (int i = 0; i < N; i++) mask16[(size_t)r * Np + i] = f2h(mask[(size_t)r * N + i]);
    struct Dev {
        hipStream_t st;
        float *q, *out, *gather;
        float* sinks;  // this device's heads' sinks (--sinks), or null
        float* lse;    // [n_q][Hl] log-sum-exps (--lse), or null
        void *k, *v, *mask, *ws;
        size_t ws_bytes;
        fattn_params p;
    };
    std::vector<Dev> dv(G);
    const int r_kv_heads = H / Hkv;
    for (int g = 0; g < G; g++) {
        Dev& d = dv[g];
        HIP_CHECK(hipSetDevice(g));
        HIP_CHECK(hipStreamCreate(&d.st));
        // this shard's Q [NQ][Hl][D] and K / V rows [Hkvl][N][row]
        std::vector<float> qs((size_t)NQ * Hl * D);
        for (int r = 0; r < NQ; r++)
            std::memcpy(&qs[(size_t)r * Hl * D], &query[((size_t)r * H + g * Hl) * D], sizeof(float) * Hl * D);
        HIP_CHECK(hipMalloc(&d.q, sizeof(float) * qs.size()));
        HIP_CHECK(hipMalloc(&d.out, sizeof(float) * NQ * Hl * D));
        HIP_CHECK(hipMalloc(&d.gather, sizeof(float) * NQ * H * D));
        const size_t kvb = rb * N * Hkvl;
        HIP_CHECK(hipMalloc(&d.k, kvb));
        HIP_CHECK(hipMalloc(&d.v, kvb));
        HIP_CHECK(hipMalloc(&d.mask, 2 * mask16.size()));
        HIP_CHECK(hipMemcpyAsync(d.q, qs.data(), 4 * qs.size(), hipMemcpyHostToDevice, d.st));
        HIP_CHECK(hipMemcpyAsync(d.k, kbytes.data() + kvb * g, kvb, hipMemcpyHostToDevice, d.st));
        HIP_CHECK(hipMemcpyAsync(d.v, vbytes.data() + kvb * g, kvb, hipMemcpyHostToDevice, d.st));
        HIP_CHECK(hipMemcpyAsync(d.mask, mask16.data(), 2 * mask16.size(), hipMemcpyHostToDevice, d.st));
        d.lse = nullptr;
        if (use_lse) HIP_CHECK(hipMalloc(&d.lse, sizeof(float) * NQ * Hl));
        d.sinks = nullptr;
        if (use_sinks) {  // the slice of the model's sinks that belongs to this device's q heads
            HIP_CHECK(hipMalloc(&d.sinks, sizeof(float) * Hl));
            HIP_CHECK(hipMemcpyAsync(d.sinks, sinks.data() + (size_t)g * Hl, sizeof(float) * Hl, hipMemcpyHostToDevice, d.st));
        }
        // the ext plan: the flash_attn_ext argument list of kernel_test.h:191-198
        // (n_q = 1) or its ne01 = n_q form, as a fattn_params view
        std::memset(&d.p, 0, sizeof(d.p));
        const int64_t eb = kv_type == FATTN_TYPE_F16 || kv_type == FATTN_TYPE_BF16 ? 2 : (int64_t)fattn_row_size(kv_type, 32);
        d.p.q = {d.q, FATTN_TYPE_F32, 0, {D, NQ, Hl, 1}, {4, (int64_t)Hl * D * 4, D * 4, (int64_t)NQ * Hl * D * 4}};
        d.p.k = {d.k, kv_type, 0, {D, N, Hkvl, 1}, {eb, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkvl}};
        d.p.v = {d.v, kv_type, 0, {D, N, Hkvl, 1}, {eb, (int64_t)rb, (int64_t)rb * N, (int64_t)rb * N * Hkvl}};
        if (has_mask)
            d.p.mask = {d.mask, FATTN_TYPE_F16, 0, {Np, mask_rows, 1, 1},
                        {2, (int64_t)Np * 2, (int64_t)Np * 2 * mask_rows, (int64_t)Np * 2 * mask_rows}};
        d.p.dst = d.out;
        d.p.scale = scale;
        d.p.max_bias = max_bias;
        d.p.logit_softcap = softcap;
        d.p.n_head_total = H;     // the slopes are the unsharded model's: this device's q head 0 is head g * Hl
        d.p.head_first = g * Hl;
        d.ws_bytes = parallel_kv ? fattn_row_workspace_size(D, N, H) : fattn_workspace_size(&d.p);
        d.ws_bytes = std::max<size_t>(d.ws_bytes, 16);
        HIP_CHECK(hipMalloc(&d.ws, d.ws_bytes));
        if (int zr = fattn_workspace_init(d.ws, d.ws_bytes, d.st)) {
            fprintf(stderr, "fattn_workspace_init failed: %s\n", fattn_strerror(zr));
            return 2;
        }
        d.p.workspace = d.ws;
        d.p.workspace_bytes = d.ws_bytes;
    }
    if (parallel_kv && kv_type != FATTN_TYPE_F16) {
        fprintf(stderr, "the flash_attn_row branch takes f16 K/V (use --no-kv-parallel for %s)\n",
                type_name(kv_type));
        return 2;
    }
    std::vector<ncclComm_t> comms(G);
    if (G > 1) {
        std::vector<int> devs(G);
        for (int g = 0; g < G; g++) devs[g] = g;
        RCCL_CHECK(ncclCommInitAll(comms.data(), G, devs.data()));
    }
    // one step: every device's attention (flash_attn_row with V transposed,
    // kernel_test.h:161-162; the positional flash_attn_ext call of
    // kernel_test.h:191-198 when n_q = 1 on one device; the fattn_params form
    // otherwise), then with G > 1 one all-gather of the shards' outputs
    auto launch = [&]() -> int {
        for (int g = 0; g < G; g++) {
            Dev& d = dv[g];
            HIP_CHECK(hipSetDevice(g));
            int rc;
            if (parallel_kv)
                rc = fattn_row(d.q, d.k, d.v, d.mask, d.ws, d.ws_bytes, d.out, D, N, H, scale, D * N, r_kv_heads, d.st);
            else if (NQ == 1 && G == 1 && has_mask && !op_xf && !use_sinks && !use_lse)
                rc = fattn_ext_f16_launch(d.q, d.k, d.v, d.mask, d.out, scale,
                                          D, 1, H, 1,
                                          D, N, Hkv, 1,
                                          mask_rows, Np * 2,
                                          D * 4, D * 4, D * H * 4,
                                          (int)rb, (int)rb * N, (int)rb * N * Hkv,
                                          D, H, 1, 1,
                                          kv_type, kv_type, d.ws, d.ws_bytes, d.st);
            else
                rc = use_lse ? fattn_ext_lse(&d.p, d.sinks, d.lse, d.st)
                     : use_sinks ? fattn_ext_sinks(&d.p, d.sinks, d.st) : fattn_ext(&d.p, d.st);
            if (rc) return rc;
        }
        if (G > 1) {
            RCCL_CHECK(ncclGroupStart());
            for (int g = 0; g < G; g++)
                RCCL_CHECK(ncclAllGather(dv[g].out, dv[g].gather, (size_t)NQ * Hl * D, ncclFloat, comms[g], dv[g].st));
            RCCL_CHECK(ncclGroupEnd());
        }
        return 0;
    };
    auto sync_all = [&] {
        for (int g = 0; g < G; g++) {
            HIP_CHECK(hipSetDevice(g));
            HIP_CHECK(hipStreamSynchronize(dv[g].st));
        }
    };
    int rc = launch();
    if (rc) {
        fprintf(stderr, "launch failed: %s\n", fattn_strerror(rc));
        return 2;
    }
    sync_all();
    // timing on device 0's stream (G > 1: events around every device's step,
    // device 0's span; the gather makes the devices wait for each other)
    HIP_CHECK(hipSetDevice(0));
    hipEvent_t start, stop;
    HIP_CHECK(hipEventCreate(&start));
    HIP_CHECK(hipEventCreate(&stop));
    std::vector<float> times;
    for (int it = 0; it < iters; it++) {
        HIP_CHECK(hipSetDevice(0));
        HIP_CHECK(hipEventRecord(start, dv[0].st));
        rc = launch();
        HIP_CHECK(hipSetDevice(0));
        HIP_CHECK(hipEventRecord(stop, dv[0].st));
        HIP_CHECK(hipEventSynchronize(stop));
        sync_all();
        if (rc) {
            fprintf(stderr, "launch failed: %s\n", fattn_strerror(rc));
            return 2;
        }
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, start, stop));
        times.push_back(ms);
    }
    std::sort(times.begin(), times.end());
    const float millis = times[times.size() / 2];
    // the output in the ggml dst layout [n_q][H][D]: device 0's gather buffer
    // [G][n_q][Hl][D] permuted (G > 1), or its output
    HIP_CHECK(hipSetDevice(0));
    if (G > 1) {
        std::vector<float> gath((size_t)NQ * H * D);
        HIP_CHECK(hipMemcpy(gath.data(), dv[0].gather, 4 * gath.size(), hipMemcpyDeviceToHost));
        for (int g = 0; g < G; g++)
            for (int r = 0; r < NQ; r++)
                std::memcpy(&qkv_gpu[((size_t)r * H + g * Hl) * D], &gath[(((size_t)g * NQ + r) * Hl) * D],
                            sizeof(float) * Hl * D);
    } else {
        HIP_CHECK(hipMemcpy(qkv_gpu.data(), dv[0].out, 4 * qkv_gpu.size(), hipMemcpyDeviceToHost));
    }
    print_array(parallel_kv ? "Parallel KV HIP" : "No paralell KV HIP", qkv_gpu.data(), 16);

    // kernel_test.h:215-234 (+ a normwise relative error -- the max |diff| over
    // the max |reference| -- and a threshold), over the checked rows
    float max_diff = 0.0f, max_ref = 0.0f;
    int row_idx = 0, head_idx = 0, dim_idx = 0;
    for (int r : rows)
        for (int h = 0; h < H; h++) {
            const size_t o = ((size_t)r * H + h) * D;
            for (int i = 0; i < D; i++) {
                const float dd = fabsf(qkv[o + i] - qkv_gpu[o + i]);
                max_ref = std::max(max_ref, fabsf(qkv[o + i]));
                if (dd > max_diff || std::isnan(dd)) {
                    max_diff = std::isnan(dd) ? INFINITY : dd;
                    row_idx = r, head_idx = h, dim_idx = i;
                }
            }
        }
    const float worst_rel = max_diff / std::max(max_ref, 1e-30f);
    const double bytes = (double)D * H * NQ * 4 * 2 + 2.0 * rb * N * Hkv + (has_mask ? 2.0 * N * NQ : 0.0);
    const double flops = 4.0 * N * D * H * NQ;
    printf("\ncuda time: %.4f ms  (%.1f GB/s, %.3f TFLOP/s; median of %d%s)\n", millis, bytes / millis / 1e6,
           flops / millis / 1e9, iters, G > 1 ? ", kernel + all-gather" : "");
    printf("R (%.4f) CUDA(%.4f) diff: %.4f - row = %d, head = %d, dim = %d\n",
           qkv[((size_t)row_idx * H + head_idx) * D + dim_idx], qkv_gpu[((size_t)row_idx * H + head_idx) * D + dim_idx],
           max_diff, row_idx, head_idx, dim_idx);
    printf("checked %zu of %d query rows x %d heads; n_q %d, %d GPU(s)\n", rows.size(), NQ, H, NQ, G);
    printf("normwise rel err %.3g (tol %.1g): %s\n", worst_rel, tol, worst_rel <= tol ? "PASS" : "FAIL");
    bool lse_ok = true;
    if (use_lse) {
        HIP_CHECK(hipMemcpy(lse_gpu.data(), dv[0].lse, 4 * lse_gpu.size(), hipMemcpyDeviceToHost));
        lse_ok = lse_check(lse_ref, lse_gpu, rows, H);
    }
    for (int g = 0; g < G; g++) {
        if (G > 1) RCCL_CHECK(ncclCommDestroy(comms[g]));
    }
    return worst_rel <= tol && lse_ok ? 0 : 1;
}
