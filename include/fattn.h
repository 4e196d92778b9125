/*
 * fattn.h -- C ABI of the MI355X (gfx950) flash-attention-with-quantized-KV
 * kernels.  Plain C: device pointers, sizes, ggml ne/nb conventions, an opaque
 * hipStream_t.  No torch / HIP C++ types cross this boundary.
 *
 * What each entry point replaces in FSSRepo/ggml-cuda-experiments
 * (/root/reference, read-only):
 *
 *   fattn_ext()          <- flash_attn_ext_f16<D,Q,C><<<...>>>, the ggml
 *                           GGML_OP_FLASH_ATTN_EXT kernel, src/flash-llama.h:5-32
 *                           (launched at src/kernel_test.h:191-198 and
 *                           src/flash-matrix.cu:198-206).  Same argument meaning
 *                           (q/k/v/mask as ggml ne/nb views, f32 dst in the
 *                           permuted [seq][n_q][H][D] layout of flash-llama.h:434),
 *                           extended with K/V element types F16 / BF16 / Q8_0 /
 *                           Q4_0 / Q4_1 / Q5_0 / Q5_1.
 *   fattn_ext_sinks()    fattn_ext() with upstream ggml's src[4], the per-head attention
 *                           sinks (absent from the reference; see its comment below).
 *   fattn_ext_f16_launch()  the positional argument list of flash-llama.h:7-32,
 *                           verbatim (ne00..ne03, ne10..ne13, ne31, nb31,
 *                           nb01..nb03, nb11..nb13, ne0..ne3), for call sites
 *                           that pass it that way; K/V types added at the end.
 *   fattn_row()          <- flash_attn_row<128,nw,2,256> + fa_reduce<128,nw>
 *                           (src/flash_row_float.h:4-6, 415-416; launched at
 *                           src/kernel_test.h:161-162, src/flash-matrix.cu:226-227):
 *                           decode with query f32 [H][D], key f16 [Hkv][N][D],
 *                           value f16 TRANSPOSED [Hkv][D][N], mask f16 [N],
 *                           out f32 [H][D]; `tmp` is the caller-owned split-KV
 *                           scratch exactly like d_temporal (kernel_test.h:155).
 *   fattn_workspace_size()  the size of that scratch (kernel_test.h:155 computes
 *                           it inline).
 *   fattn_dequantize() / fattn_quantize()   ggml Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / BF16 row conversion on the
 *                           GPU (bit-exact with upstream ggml; absent from the
 *                           reference) -- the KV-cache write side.
 *   fattn_cpy() / fattn_set_rows()   the cache write itself: GGML_OP_CPY into a
 *                           contiguous view, and GGML_OP_SET_ROWS, rows scattered to
 *                           the slots an index tensor in device memory names (what
 *                           llama.cpp emits since mid-2025); both absent from the reference.
 *   fattn_k_shift()      the last node of the cache's life cycle: llama.cpp's K-shift
 *                           (build_rope_shift), the RoPE rotation of a cache of any type in
 *                           place by per-slot position deltas, one launch; absent from the reference.
 *
 * Conventions:
 *   - every pointer is a device pointer the caller allocated; the library never
 *     allocates on the hot path; `stream` is a hipStream_t (NULL = default).
 *   - return value: FATTN_OK (0) or a negative fattn_status; nothing is launched
 *     when an error is returned.  fattn_strerror() names the code.
 *   - stream-ordered and asynchronous; thread-compatible.  Global state: a
 *     per-device CU count cache, a launch-epoch counter that stamps the split-KV
 *     arrival words (monotonic; any thread may advance it), and the planner
 *     overrides of fattn_debug.h (tests, benchmarks; all off by default).
 *   - this header lists the drop-in entry points only; the diagnostics (planner
 *     overrides, the plan as text, an event-bracketed launch) are declared in
 *     fattn_debug.h, exported by the same library.
 */
#ifndef FATTN_H
#define FATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types: the ggml_type numbering */
enum fattn_type {
    FATTN_TYPE_F32 = 0,
    FATTN_TYPE_F16 = 1,
    FATTN_TYPE_Q4_0 = 2,
    FATTN_TYPE_Q4_1 = 3,
    FATTN_TYPE_Q5_0 = 6,
    FATTN_TYPE_Q5_1 = 7,
    FATTN_TYPE_Q8_0 = 8,
    FATTN_TYPE_I32 = 26,  /* index tensors of fattn_set_rows only: every other entry point rejects them */
    FATTN_TYPE_I64 = 27,
    FATTN_TYPE_BF16 = 30, /* 2 bytes per element; K / V of fattn_ext, dst of fattn_cpy (not of fattn_set_rows) */
};

enum fattn_status {
    FATTN_OK = 0,
    FATTN_ERR_INVALID_ARG = -1,     /* NULL pointer, bad shape, ne not divisible */
    FATTN_ERR_UNSUPPORTED_TYPE = -2,
    FATTN_ERR_UNSUPPORTED_HEAD_DIM = -3,  /* D must be 64, 80 (f16 K/V only), 96 (not Q4_1 / Q5_0 / Q5_1 / BF16), 128 or 256 -- or the MLA pair, K 576 with V 512 (f16, Q8_0 or Q4_0) */
    FATTN_ERR_BAD_STRIDE = -4,       /* layout the kernels cannot address */
    FATTN_ERR_WORKSPACE = -5,        /* workspace too small */
    FATTN_ERR_LAUNCH = -6,           /* HIP launch failure */
    FATTN_ERR_ALIGNMENT = -7,
};

/* A ggml tensor view: ne[i] elements along dim i, nb[i] byte stride of dim i. */
typedef struct fattn_tensor {
    const void* data;
    int32_t type;
    int32_t pad_;
    int64_t ne[4];
    int64_t nb[4];
} fattn_tensor;

/* GGML_OP_FLASH_ATTN_EXT:
 *   q    f32  ne = [D, n_q, H, S]        (any nb with nb[0] == 4)
 *   k    F16/BF16/Q8_0/Q4_0/Q4_1/Q5_0/Q5_1  ne = [D, N, Hkv, Skv]  rows contiguous (nb[0] = type size)
 *   v    the same types  ne = [D, N, Hkv, Skv]; rows contiguous, or for F16 only (not BF16)
 *        transposed (nb[1] == 2, nb[0] == N*2 style strides).  v's type may
 *        differ from k's (llama.cpp's separate K / V cache types) at D = 64,
 *        128 and 256: the split-KV kernel takes every such pair of F16 / Q8_0 /
 *        Q4_0.  Q4_1 / Q5_0 / Q5_1 (the other classic 32-element blocks of
 *        llama.cpp's --cache-type-k/-v: 20 / 22 / 24 bytes, {d, [m], [qh], qs}):
 *        K and V of one such type, at D = 64, 128 and 256.  Every decode shape
 *        runs the split-KV kernel over the raw blocks; prefill shapes at D = 64 /
 *        128 stage the rows to f16 first (as Q8_0 / Q4_0 do), at D = 256 they run
 *        the split-KV kernel.  Not supported: D = 96 with one of the three
 *        (FATTN_ERR_UNSUPPORTED_HEAD_DIM: Q5_0 rows would be 66 bytes, no whole
 *        number of dwords) and a pair that mixes one of them with any other
 *        type (FATTN_ERR_UNSUPPORTED_TYPE)
 *        BF16 (ggml type 30, llama.cpp's --cache-type-k/-v bf16: the cache of a
 *        bf16-trained model, whose K norms and outlier V channels pass f16's
 *        65504): K and V both BF16, at D = 64, 128 and 256, under the F16 row
 *        rules unchanged -- nb[0] == 2, rows contiguous, [Hkv][N][row],
 *        [N][Hkv][row] and padded rows all qualify, the 16-B path when bases and
 *        strides are multiples of 16 and the dword path otherwise.  Every shape
 *        (one-row decode, GQA tiles, batched decode, prefill-sized n_q) runs the
 *        split-KV kernel over the raw rows; nothing is staged or converted to f16.
 *        Values: K and V enter v_mfma_f32_16x16x32_bf16 exactly (any finite bf16,
 *        up to 3.4e38); Q and the unnormalised probabilities enter as two bf16
 *        operands each, hi = bf16(x) and lo = bf16(x - hi) (round to nearest
 *        even), two MFMAs into one f32 accumulator -- 16 operand bits, so the
 *        result is closer to exact arithmetic than the F16 path's (11 bits).
 *        Accumulators, softmax state and every chunk partial are f32 (a BF16
 *        plan never takes f16 partials).  Mask, mask planes, scale, max_bias,
 *        logit_softcap, n_head_total / head_first, sinks, kv_chunk and the
 *        workspace rules keep their meaning; the workspace is the F16 split
 *        plan's with f32 partials.  fattn_describe:
 *        fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>...  Refused, before
 *        anything launches: BF16 paired with any other K / V type
 *        (FATTN_ERR_UNSUPPORTED_TYPE), D = 80 / 96 (FATTN_ERR_UNSUPPORTED_HEAD_DIM),
 *        a transposed BF16 V, v.nb[0] != 2 (FATTN_ERR_BAD_STRIDE), the MLA shape
 *        (FATTN_ERR_UNSUPPORTED_TYPE); fattn_row stays f16-only.  The cache write
 *        is fattn_cpy / fattn_quantize; fattn_set_rows has NO BF16 form yet (a
 *        BF16 dst there is FATTN_ERR_UNSUPPORTED_TYPE)
 *   mask F16 ne = [N', rows >= n_q] with N' >= N rounded up to even (ggml pads
 *        mask rows to GGML_KQ_MASK_PAD), 4-byte aligned rows; row = query
 *        index; or data == NULL for no mask.  ne[2] and ne[3] are plane counts,
 *        read as ggml's FLASH_ATTN_EXT reads them: query head iq2 of sequence
 *        iq3 takes its row from
 *            data + iq1*nb[1] + (iq2 % ne[2])*nb[2] + (iq3 % ne[3])*nb[3]
 *        -- ne[3] planes per stream (each sequence its own length, padding or
 *        window), ne[2] per head (ALiBi-style biases); the indices are the
 *        query's, so sequences that share one KV (S > Skv) may still differ in
 *        mask.  ne[2] must divide H and ne[3] must divide S
 *        (FATTN_ERR_INVALID_ARG); a count < 1 reads as 1 (zeroed structs), and
 *        (1, 1) is one plane for every head and sequence.  nb[2] / nb[3]: any
 *        non-negative multiples of 4 (FATTN_ERR_ALIGNMENT) -- either order of
 *        planes, gaps, or 0 to repeat a plane -- looked at only where the
 *        count exceeds 1; a stride that is no multiple of 16 turns the 16-B
 *        path off, as nb[1] % 16 does.  One sequence plane with all its head
 *        planes, (rows - 1)*nb[1] + N'*2 + (ne[2] - 1)*nb[2] bytes, must stay
 *        below 4 GiB (FATTN_ERR_BAD_STRIDE).  The masked prefill's workspace
 *        grows with the plane count (fattn_workspace_size)
 *   dst  f32 contiguous [S][n_q][H][D]
 *   H % Hkv == 0 (GQA broadcast), S % Skv == 0.
 *   Spans: nb[2] / nb[3] of every tensor are 64-bit (planes may lie more than
 *   4 GiB apart); inside one plane the kernels address with 32 bits, so the
 *   bytes one (kv head, sequence) plane of K or V covers, (N - 1)*nb[1] + row
 *   ((D - 1)*nb[0] + 2 N for a transposed V), and the bytes the rows and heads
 *   of one sequence of Q cover, (n_q - 1)*nb[1] + (H - 1)*nb[2] + 4 D, must not
 *   exceed 0xFFFFFFF0 (FATTN_ERR_BAD_STRIDE).  The split-KV kernel fetches K
 *   and V in whole 32-key steps: where it runs, the limit holds for N rounded
 *   up to a multiple of 32 -- it bites only a cache whose rows lie MiB apart
 *   and whose span ends within one step of 4 GiB.
 *   softmax(scale * q.k^T + mask) . v per (seq, head, query row).  A row whose
 *   mask is -inf everywhere yields NaN, as the reference's softmax does
 *   (src/utils.h:30-49).
 *   max_bias, logit_softcap: the other two floats of ggml's op_params
 *        (op_params[1], op_params[2]), with ggml's meaning.  For q head h
 *        (global index, below), s = q.k and mask value m (0 without a mask):
 *            x = s * scale                        logit_softcap == 0
 *            x = cap * tanh(s * (scale / cap))    logit_softcap  > 0 (cap = logit_softcap)
 *            score = x + slope(h) * m
 *        slope(h) = 1 when max_bias == 0; else, with n = n_head_total and
 *        n2 = 2^floor(log2 n), 2^(-(max_bias / n2) * (h + 1)) for h < n2 and
 *        2^(-(max_bias / 2 / n2) * (2 * (h - n2) + 1)) past it -- ALiBi from
 *        one shared distance mask, without H pre-multiplied head planes (a head
 *        plane, ne[2] > 1, is still scaled by the slope of the query's head).
 *        max_bias without a mask changes nothing: same plan, same output bits.
 *        The slope is > 0, so -inf stays -inf.  h = head_first + iq2:
 *        a head-sharded launch passes the global index of its q head 0 and the
 *        unsharded head count n_head_total (0 = q.ne[2]); head_first >= 0 and
 *        head_first + H <= n_head_total.  A negative, NaN or infinite max_bias
 *        or logit_softcap is FATTN_ERR_INVALID_ARG.  tanh is built from
 *        v_exp_f32 / v_rcp_f32 (1 - 2 / (1 + 2^(2 log2e t))): exact saturation,
 *        absolute error about 1e-7, so about cap * 1e-7 in a logit.  With either
 *        live, prefill shapes run fattn_pf_kernel rather than the one-wave-
 *        per-SIMD bodies; the multi-query kernel applies the slope per lane
 *        (GQA tiles keep their plan).  The struct grew by these four fields:
 *        zero-initialise it (memset / = {0}); zeros are the earlier behaviour. */
typedef struct fattn_params {
    fattn_tensor q, k, v, mask;
    float* dst;
    float scale;
    int32_t kv_chunk;      /* split-KV chunk length in positions; 0 = auto */
    void* workspace;       /* split-KV scratch, >= fattn_workspace_size() bytes.  Zero a new
                              allocation once (fattn_workspace_init): a launch stamps its
                              arrival words with a fresh epoch by atomic max, which
                              supersedes any word an earlier launch left (re-armed, or
                              mid-count after an abort) and any word whose top 8 bits are
                              not all ones -- but an uninitialised word that happens to
                              read 0xFF in its top bits with an epoch field ahead of the
                              launch's would outrank the stamp.  No re-zeroing is needed
                              between launches.  Launches that share one workspace must be
                              ordered on one stream */
    size_t workspace_bytes;
    /* ggml's other two op_params floats (see above); all four zero = softmax(scale * q.k^T + mask) */
    float max_bias;        /* ALiBi; 0 = off */
    float logit_softcap;   /* 0 = off */
    int32_t n_head_total;  /* heads of the unsharded model, for the slopes; 0 = q.ne[2] */
    int32_t head_first;    /* global index of q head 0 (head-sharded launches); 0 otherwise */
} fattn_params;

size_t fattn_workspace_size(const fattn_params* p);
/* Zero a workspace (hipMemsetAsync on `stream`); call once per allocation.  The
 * split-KV chunks of a tile meet through 64-bit arrival words kept at the front
 * of the workspace, [0xFF | epoch:32 | generation:8 | count:16]; each launch
 * stamps them with its own epoch (atomic max) before counting, so memory left by
 * an earlier or an aborted launch is superseded -- but not a never-initialised
 * word whose top 8 bits are all ones with an epoch above the current one (e.g.
 * 0xFF fill), which this call clears.  The last arriver re-arms a word (count 0,
 * generation + 1), so a replayed graph finds it clean. */
int fattn_workspace_init(void* workspace, size_t workspace_bytes, void* stream);
int fattn_ext(const fattn_params* p, void* stream);

/* MULTI-HEAD LATENT ATTENTION (DeepSeek-V2 / V3 / R1, Kimi-K2 after weight
 * absorption): the one shape of GGML_OP_FLASH_ATTN_EXT whose V rows are shorter
 * than its K rows.  fattn_ext and fattn_ext_sinks take it; no other symbol, no
 * struct change.
 *   q    F32  ne = [576, n_q, H, S]      alignment as above (16-B base and nb[1..3])
 *   k    F16  ne = [576, N, Hkv, Skv]    nb[0] == 2
 *   v    F16  ne = [512, N, Hkv, Skv]    nb[0] == 2 (not transposed)
 *   dst  f32 contiguous [S][n_q][H][512] -- the last dim is V's
 *   H % Hkv == 0 with any ratio (the models: Hkv = 1, H = 16 ... 128),
 *   S % Skv == 0, any N >= 1.
 *   k.data, v.data and nb[1..3] of both: multiples of 16 (FATTN_ERR_ALIGNMENT) --
 *   rows are 1152 B and 1024 B, so natural caches, [N][Hkv][row] layouts and
 *   rows padded by a multiple of 16 qualify; there is no dword path.  Rows may
 *   be padded, not overlapped: k.nb[1] >= 1152, v.nb[1] >= 1024, and the
 *   per-plane byte spans stay below 4 GiB (FATTN_ERR_BAD_STRIDE).
 *   V AS A VIEW OF K -- what llama.cpp builds, V being the 512-element latent of
 *   the same cache row: when v.data == k.data + off with 0 <= off <= 128 (off a
 *   multiple of 16 by the alignment rule) and v.nb[1..3] == k.nb[1..3] (a stride
 *   of a dim of one element is not compared), each cache row is read from HBM
 *   ONCE and V is taken out of the K tile in LDS.  off = 0: the latent first;
 *   off = 128: the 64 RoPE dims first (llama.cpp's order).  Any other V is
 *   loaded on its own, same results.  fattn_describe says which: v=k+<off> or
 *   v=own.
 *   Everything else keeps its meaning: the mask contract (f16, 4-byte aligned
 *   rows, ne[2] / ne[3] planes, N' >= N rounded up to even), scale, max_bias,
 *   logit_softcap, n_head_total, head_first, sinks, kv_chunk as a hint (rounded
 *   up to 32-key tiles, at most 64 chunks), the workspace rules
 *   (fattn_workspace_size(p) a function of p alone, 0 for a single chunk;
 *   several chunks merge in a second launch, nothing is allocated, the launch
 *   is capturable), NaN for a row masked -inf everywhere and zeros with sinks.
 *   A Q8_0 OR Q4_0 CACHE (llama.cpp's --cache-type-k; with MLA there is no V
 *   cache, so K's type is the cache's type):
 *   k    Q8_0 | Q4_0  ne = [576, N, Hkv, Skv]: 18 blocks per row, nb[0] the
 *        block size (34 / 18 B), rows of 612 / 324 B, k.nb[1] >= that (padded,
 *        not overlapped)
 *   v    K's type, ne = [512, N, Hkv, Skv], and it MUST be a view of K:
 *        v.data == k.data + b * nb[0] with b = 0, 1 or 2 whole blocks (byte 0 /
 *        34 / 68 for Q8_0, 0 / 18 / 36 for Q4_0; b = 2 is llama.cpp's row with
 *        the 64 RoPE dims first, ggml_row_size(type_k, 64)), v.nb[0] == k.nb[0]
 *        and v.nb[1..3] == k.nb[1..3] (a stride of a one-element dim is not
 *        compared)
 *   k.data and nb[1..3]: multiples of 4 (FATTN_ERR_ALIGNMENT) -- these rows are
 *   whole dwords, not 16-B multiples, and a natural cache (612-B row stride)
 *   works unpadded.  v.data is k.data plus whole blocks (2 mod 4 one block in):
 *   only K's base is addressed.  Spans below 4 GiB as above.  q, mask, dst, every
 *   scalar, sinks, kv_chunk and the workspace rules are those of the f16 form:
 *   the workspace is 0 bytes for one chunk and the f16 view plan's for several
 *   (the cache is never staged to f16 in memory).
 *   Values: element (n, j) of K is the f16 rounding of ggml's dequantisation,
 *   h(qs[j] * d) for Q8_0 and h((nibble - 8) * d) for Q4_0 (the product is exact
 *   in f32: one rounding); V is elements [32 b, 32 b + 512) of the same.  A
 *   launch returns bit for bit what the f16 form returns over an f16 cache
 *   holding those values (same shape, mask, scalars, sinks and kv_chunk).
 *   fattn_describe: fattn_mla_kernel<q8_0,DK576,DV512,...,v=k+68>.
 *   Refused: q.ne[0] == 576 with any K / V row lengths but (576, 512)
 *   FATTN_ERR_UNSUPPORTED_HEAD_DIM (looked at before the types); a transposed V,
 *   Q4_1 / Q5_0 / Q5_1, K and V of different types, or a Q8_0 / Q4_0 K whose V is
 *   not such a view (a buffer of its own, an offset of no 0 / 1 / 2 whole
 *   blocks, other strides) FATTN_ERR_UNSUPPORTED_TYPE.  Every other head dim
 *   keeps k.ne[0] == v.ne[0] == q.ne[0] (FATTN_ERR_INVALID_ARG). */

/* fattn_ext with attention sinks: src[4] of ggml's GGML_OP_FLASH_ATTN_EXT (the
 * gpt-oss family).  A sink is one extra logit per q head: it joins the softmax
 * denominator and has no value row.  ggml passes it as a tensor of its own, and
 * so does this entry point -- fattn_params does not grow.
 *   sinks  device pointer to q.ne[2] contiguous f32 values, indexed by the
 *          launch's LOCAL q head iq2: a head-sharded launch passes
 *          sinks + head_first (no formula, so no global numbering as for the
 *          slopes).  4-byte aligned, else FATTN_ERR_ALIGNMENT -- checked, like
 *          every other validation, before anything launches; invalid params
 *          return what fattn_ext returns for them, whatever sinks is.
 *          NULL: exactly fattn_ext(p, stream) -- same code path, same bits.
 * After the whole KV range a row with running max M and sum S in natural-log
 * units (scale, the soft cap and slope * mask already in them) takes the sink
 * s = sinks[iq2] as ggml does:
 *     if (s > M) { ms = expf(M - s); VKQ *= ms; S = S * ms + 1; } else S += expf(s - M);
 *     out = VKQ / S
 * in closed form out = O / (L + exp(s - M)): the plain output times
 * g = 1 / (1 + exp(s - lse)), lse the row's log-sum-exp.
 *   - the sink is RAW: not multiplied by scale, not capped, no ALiBi slope.
 *   - a row whose mask is -inf everywhere has S = 1, VKQ = 0: with sinks such a
 *     row is zeros, not the NaN of fattn_ext.
 *   - sinks[h] = -inf: no sink for that head.  NaN or +inf in the array is
 *     undefined (the library cannot read device memory to check it).
 * Sinks never change the plan, the grid, the workspace size or the describe
 * string: fattn_workspace_size(p) and fattn_describe(p) are functions of p
 * alone, so fattn_describe(p) is also the plan of the sinks launch.  The sink
 * enters once per output row, in the epilogue that normalises into dst (after
 * the chunk merge of a split-KV plan); the tile loops are untouched. */
int fattn_ext_sinks(const fattn_params* p, const float* sinks, void* stream);

/* fattn_ext_sinks(p, sinks, stream) that also writes the rows' log-sum-exp: the
 * one number per row that lets a caller combine launches over pieces of one KV
 * range (KV-sharded decode across GPUs, a prefix cache plus a tail) with
 * fattn_lse_merge below.
 *   lse    device pointer to S * n_q * H contiguous f32 values, [S][n_q][H]:
 *          dst's layout without its last dim (the MLA shape too).  4-byte
 *          aligned, else FATTN_ERR_ALIGNMENT -- checked beside sinks, after the
 *          params: invalid params return what fattn_ext returns for them,
 *          whatever lse is.  NULL: exactly fattn_ext_sinks -- same code path,
 *          same bits.
 * Each entry is the natural-log log-sum-exp of the row's FINAL scores -- after
 * scale, logit_softcap and slope(h) * mask, the scores whose softmax weights V.
 *   - sinks != NULL: the sink is one of the terms, so lse is the log of the
 *     denominator dst was divided by and dst * exp(lse) is the unnormalised row
 *     either way.  A KV-sharded caller passes sinks = NULL to the shard launches
 *     and gives the sinks to the merge, once.
 *   - a row whose mask is -inf everywhere: lse = -inf (dst NaN, as without lse)
 *     without sinks, lse = sinks[h] (dst zeros) with sinks; -inf is written by
 *     selection, never computed.
 * dst is bit for bit what the launch without lse writes.  The plan, the grid,
 * the workspace size and fattn_describe(p) stay functions of p alone; every plan
 * and every cache type serves it: one lane per output row stores one float in
 * the epilogue that normalises into dst, behind the row guards of the dst
 * store.  (Under fattn_debug.h's diagnostic in-kernel chunk merge, a row that
 * option leaves NaN -- its own documentation -- has an undefined lse.)  No events and
 * no positional form; fattn_row is unchanged. */
int fattn_ext_lse(const fattn_params* p, const float* sinks, float* lse, void* stream);

/* The merge of n_parts normalised partial outputs of one set of rows over
 * disjoint key ranges, by their log-sum-exps (the fa_reduce rule the kernels
 * use between split-KV chunks, from outside).
 *   outs  part p at outs + p * out_part_stride floats, f32 [n_rows][dv]
 *   lses  part p at lses + p * lse_part_stride floats, f32 [n_rows]
 *         -- what an all-gather of per-rank (dst, lse) yields.  Rows in dst's
 *         [S][n_q][H] order: row r belongs to head r % n_head.
 *   sinks NULL, or n_head raw f32 logits indexed like fattn_ext_sinks' (n_head
 *         is read only then): the sink joins the merged denominator, once.
 *   dst   f32 [n_rows][dv]; must not alias outs.  lse_out: f32 [n_rows] or NULL.
 * Per row: M = max_p lse_p, w_p = exp(lse_p - M), L = sum_p w_p,
 *     dst = sum_p w_p out_p / L,   lse_out = M + ln L.
 * A part with lse_p = -inf contributes nothing, by selection: its out_p row
 * (NaN) never reaches the sum.  With a finite sink s, L gains exp(s - M), taken
 * at max(M, s).  All parts -inf: a NaN row and lse_out = -inf without sinks, a
 * zero row and lse_out = s with sinks.  n_parts = 1 without sinks copies bit
 * for bit.
 * Validated before anything launches: NULL outs / lses / dst, n_parts outside
 * 1 .. 64, n_rows outside 1 .. 2^31 - 1, n_head < 1 with sinks
 * FATTN_ERR_INVALID_ARG; dv no multiple of 4 in 4 .. 512
 * FATTN_ERR_UNSUPPORTED_HEAD_DIM; out_part_stride < n_rows * dv or no multiple
 * of 4, lse_part_stride < n_rows FATTN_ERR_BAD_STRIDE; outs / dst not 16-byte
 * aligned, lses / lse_out / sinks not 4-byte aligned FATTN_ERR_ALIGNMENT.
 * Stream-ordered; allocates nothing, needs no workspace, capturable. */
int fattn_lse_merge(const float* outs, const float* lses, int32_t n_parts, int64_t n_rows, int32_t dv,
                    int64_t out_part_stride, int64_t lse_part_stride, const float* sinks, int32_t n_head,
                    float* dst, float* lse_out, void* stream);

/* flash-llama.h:7-32 argument list (K and V share nb11..nb13, flash-llama.h:123-125;
 * mask rows padded to ne31, nb31 bytes per row; one mask plane -- the list has
 * no ne32 / ne33 -- as for fattn_row below).  The one ne10 is K's and V's row
 * length, so the list cannot name the MLA shape (K 576, V 512): that one goes
 * through fattn_ext / fattn_ext_sinks only, and ne00 = 576 here is
 * FATTN_ERR_UNSUPPORTED_HEAD_DIM. */
int fattn_ext_f16_launch(const void* q, const void* k, const void* v, const void* mask, float* dst, float scale,
                         int ne00, int ne01, int ne02, int ne03, int ne10, int ne11, int ne12, int ne13, int ne31,
                         int nb31, int nb01, int nb02, int nb03, int nb11, int nb12, int nb13, int ne0, int ne1,
                         int ne2, int ne3, int k_type, int v_type, void* workspace, size_t workspace_bytes,
                         void* stream);

/* flash_attn_row + fa_reduce (flash_row_float.h): query f32 [H][D], key f16
 * [Hkv][N][D] (head_stride = D*N elements), value f16 [Hkv][D][N], mask f16 [N],
 * qkv f32 [H][D]; r_kv_heads = H / Hkv.  tmp: >= fattn_row_workspace_size(),
 * its arrival words are epoch-stamped per launch (as for fattn_params.workspace). */
size_t fattn_row_workspace_size(int head_dim, int kv_size, int num_heads);
int fattn_row(const float* query, const void* key, const void* value, const void* mask, void* tmp,
              size_t tmp_bytes, float* qkv, int head_dim, int kv_size, int num_heads, float scale,
              int head_stride, int r_kv_heads, void* stream);

/* ggml row conversions on the GPU (n_rows rows of k elements each, contiguous).
 * dequantize: Q8_0/Q4_0/Q4_1/Q5_0/Q5_1/F16/BF16 -> f32 (bit-exact with ggml dequantize_row_*;
 *             BF16: exact, the bits shifted up by 16).
 * quantize:   f32 -> Q8_0/Q4_0/Q4_1/Q5_0/Q5_1 (bit-exact with ggml quantize_row_*_ref), or
 *             f32 -> BF16 (any k >= 1, src 4-byte aligned): ggml_compute_fp32_to_bf16 bit for
 *             bit, in integer arithmetic -- with u the f32 bits, a NaN ((u & 0x7fffffff) >
 *             0x7f800000) gives (u >> 16) | 64 (kept, made quiet), anything else
 *             (u + 0x7fff + ((u >> 16) & 1)) >> 16: round to nearest even, subnormals kept,
 *             overflow to inf. */
int fattn_dequantize(int type, const void* src, float* dst, int64_t k, int64_t n_rows, void* stream);
int fattn_quantize(int type, const float* src, void* dst, int64_t k, int64_t n_rows, void* stream);

/* GGML_OP_CPY f32 -> F16 / BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 into a strided view: the KV-cache write
 * (quantize-on-write; upstream ggml cpy_f32_q /
 * cpy_f32_f16, absent from the reference).  src: f32, nb[0] = 4; dst: same ne,
 * nb[0] = element / block bytes, any nb[1..3] -- e.g. one token's Hkv rows
 * written into a [Hkv][N][row] cache (nb1 = N * row bytes) or a [N][Hkv][row]
 * cache (nb1 = row bytes).  ne[0] a multiple of 32 for the block types; BF16 under
 * the F16 rules (any ne0 >= 1, nb[0] == 2).  Values bit-exact with ggml
 * quantize_row_*_ref / f16 round-to-nearest-even / the BF16 rule of fattn_quantize. */
int fattn_cpy(const fattn_tensor* src, const fattn_tensor* dst, void* stream);

/* GGML_OP_SET_ROWS f32 -> F16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1: the KV-cache write by slot
 * index (upstream ggml_set_rows(a, b, c) with dst = a, src = b, idx = c; absent
 * from the reference).  The slots are data in device memory, not launch
 * arguments: one captured graph serves every decode step.  (No BF16 dst yet:
 * FATTN_ERR_UNSUPPORTED_TYPE; a BF16 cache is written with fattn_cpy.)
 *   src  F32  ne = [ne0, nr, ne2, ne3]; nb[0] == 4, nb[1..3] any multiples of 4,
 *        4-byte aligned base (a 16-byte aligned base with nb[1..3] multiples of
 *        16 reads 16 B per lane, anything else 4 B at a time: same bytes written)
 *   idx  I64 or I32  ne = [nr, ne11, ne12, 1] with ne2 % ne11 == 0 and
 *        ne3 % ne12 == 0 -- ggml's broadcast: one index row for all heads /
 *        streams, or one per head / per stream.  Base and nb multiples of the
 *        element size, nb[0] >= the element size; nb[1] / nb[2] any non-negative
 *        multiples (0 repeats a row), looked at only where the count exceeds 1
 *   dst  F16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1  ne = [ne0, n_slots, ne2, ne3]; nb[0] = element /
 *        block bytes, nb[1..3] and the base multiples of 2 as for fattn_cpy, so a
 *        [N][Hkv][row] and a [Hkv][N][row] cache are both expressible.  ne0 a
 *        multiple of 32 for the block types, any ne0 >= 1 for F16
 * For every (i, i2, i3):
 *     slot = idx.data[i*nb[0] + (i2 % ne11)*nb[1] + (i3 % ne12)*nb[2]]
 * read at full width and compared with n_slots in 64 bits (an I64 value is never
 * truncated); when 0 <= slot < n_slots the dst row at slot*nb[1] + i2*nb[2] +
 * i3*nb[3] becomes the conversion of the src row at i*nb[1] + i2*nb[2] + i3*nb[3]:
 * the bytes of ggml quantize_row_*_ref / the f16 round-to-nearest-even, exactly
 * those fattn_cpy and fattn_quantize write.  No other byte of dst changes.
 *   - AN OUT-OF-RANGE SLOT WRITES NOTHING: that row is skipped.  ggml asserts on
 *     the host; the library cannot read device memory, and never stores out of
 *     bounds.  This is the contract, not an error path: the call still returns 0.
 *   - duplicate slots in one launch: some one of the rows wins, as in ggml.
 * Validated before anything launches: NULL or a shape (any ne <= 0, ne that do
 * not match, ne0 % 32 for a block type, more than 2^31 - 1 blocks in one
 * [ne0, nr] plane) FATTN_ERR_INVALID_ARG; a type FATTN_ERR_UNSUPPORTED_TYPE; a
 * wrong nb[0] or a negative idx stride FATTN_ERR_BAD_STRIDE; alignment
 * FATTN_ERR_ALIGNMENT.  Stream-ordered; allocates nothing, does not
 * synchronise, capturable. */
int fattn_set_rows(const fattn_tensor* src, const fattn_tensor* idx, const fattn_tensor* dst, void* stream);

/* THE K-SHIFT: the RoPE rotation of a K cache IN PLACE by a per-slot position
 * delta -- the graph llama.cpp's build_rope_shift schedules for context shifting
 * and llama_memory_seq_add / seq_div (cast to f32 when the cache is quantised,
 * ggml_rope_ext_inplace, copy back), as ONE launch that reads each cache block
 * once, dequantises it in registers, rotates it, requantises it and writes it
 * back: no f32 temporary.  Absent from the reference.  The deltas are data in
 * device memory, so one captured graph serves every shift.
 *   k      F32 / F16 / BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1  ne = [ne0, n_slots, Hkv, S],
 *          oriented like fattn_set_rows' dst ([N][Hkv][row] and [Hkv][N][row]
 *          caches are both views); nb[0] = element / block bytes; base and
 *          nb[1..3] multiples of 2 (4 for F32).  ne0 <= 256, a multiple of 32 for
 *          the block types and of 4 otherwise; a longer row is passed as the view
 *          of its leading part (the 64 RoPE dims of an MLA cache row: ne0 = 64,
 *          nb[1] = 1152 / 612 / 324).  Rows must not overlap (the caller's duty)
 *   shift  I32  ne = [n_slots, ns, 1, 1] with S % ns == 0: sequence i3 reads plane
 *          i3 % ns; heads never index it.  Base and strides multiples of 4,
 *          nb[0] >= 4, nb[1] non-negative (looked at only when ns > 1)
 *   freq_factors  NULL, or n_dims / 2 f32 values in device memory (ggml's src[2])
 *   rope   ggml_rope_ext's parameters (below)
 * For every row (n, h, s) with p = shift[n, s % ns]:
 *   - p == 0: NO BYTE OF THE ROW IS TOUCHED (ggml would requantise it: the first
 *     deviation, and the better outcome -- an unshifted row keeps its bits).
 *   - 32-element blocks that lie wholly at or past n_dims are never touched
 *     either (the second deviation, same reason); for F32 / F16 / BF16 only the
 *     elements below n_dims are written.
 *   - every other block of the row is rewritten: x = ggml's dequantize_row_* of
 *     it (exact for F32 / F16 / BF16); for pair i < n_dims / 2, with (x0, x1) =
 *     elements (2i, 2i+1) for mode 0 and (i, i + n_dims/2) for mode 2, all in f32,
 *     every operation rounded on its own:
 *         theta_scale  = powf(freq_base, -2.0f / n_dims)
 *         theta_extrap = p * powf(theta_scale, i) / (freq_factors ? freq_factors[i] : 1)
 *         theta = freq_scale * theta_extrap,  m = attn_factor
 *         if (ext_factor != 0) {            -- ggml's rope_yarn
 *             corr(b) = n_dims * logf(n_ctx_orig / (b * 2 pi)) / (2 * logf(freq_base))
 *             lo = max(0, floorf(corr(beta_fast))),  hi = min(n_dims - 1, ceilf(corr(beta_slow)))
 *             mix = (1 - min(1, max(0, (i - lo) / max(0.001f, hi - lo)))) * ext_factor
 *             theta = theta * (1 - mix) + theta_extrap * mix
 *             m *= 1 + 0.1f * logf(1 / freq_scale)
 *         }
 *         y0 = x0 * cos(theta) * m - x1 * sin(theta) * m
 *         y1 = x0 * sin(theta) * m + x1 * cos(theta) * m
 *     (sinf / cosf with full range reduction: |theta| reaches 1e5); elements at
 *     or past n_dims pass through.  The block then holds exactly the bytes
 *     fattn_set_rows / fattn_cpy write for y: quantize_row_*_ref with its tie
 *     rules, f16 round-to-nearest-even, the BF16 rule of fattn_quantize, y itself
 *     for F32.  The rotation is one function for all eight types: equal x, p and
 *     parameters give the same f32 y.
 * Limits: ne0 <= 256; modes 0 (GGML_ROPE_TYPE_NORMAL) and 2 (GGML_ROPE_TYPE_NEOX)
 * only -- no M-RoPE / vision modes.
 * Validated before anything launches: NULL k / shift / rope or a NULL data, any
 * ne <= 0, shift.ne[0] != n_slots, S % ns, shift.ne[2..3] != 1, ne0 no multiple
 * of 32 (block types) / 4 (others), n_dims outside 8 .. ne0 or n_dims % 8, mode
 * not 0 / 2, freq_base or freq_scale not finite and positive, ext_factor negative
 * or not finite, attn_factor / beta_fast / beta_slow not finite, ext_factor != 0
 * with n_ctx_orig <= 0, more than 2^31 - 1 blocks in one [ne0, n_slots] plane
 * FATTN_ERR_INVALID_ARG; a k type outside the list or a shift that is not I32
 * FATTN_ERR_UNSUPPORTED_TYPE; ne0 > 256 FATTN_ERR_UNSUPPORTED_HEAD_DIM; a wrong
 * k.nb[0], shift.nb[0] < 4 or a negative shift.nb[1] FATTN_ERR_BAD_STRIDE;
 * alignment (k as above, shift and freq_factors multiples of 4)
 * FATTN_ERR_ALIGNMENT.  Stream-ordered; allocates nothing, does not synchronise,
 * capturable. */
typedef struct fattn_rope {
    int32_t n_dims;      /* leading elements of each row that are rotated (ggml n_rot) */
    int32_t mode;        /* 0 = GGML_ROPE_TYPE_NORMAL: pairs (2i, 2i+1); 2 = GGML_ROPE_TYPE_NEOX: pairs (i, i + n_dims/2) */
    int32_t n_ctx_orig;  /* read only when ext_factor != 0 */
    float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
} fattn_rope;
int fattn_k_shift(const fattn_tensor* k, const fattn_tensor* shift, const float* freq_factors,
                  const fattn_rope* rope, void* stream);

const char* fattn_strerror(int status);
/* bytes of one row of k elements (0 if unsupported; BF16: 2 k) */
size_t fattn_row_size(int type, int64_t k);
/* library version string */
const char* fattn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FATTN_H */
