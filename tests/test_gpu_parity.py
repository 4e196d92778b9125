"""GPU parity: the HIP path (C ABI -> libfattn.so) against the CPU oracle.

Bar (BASELINE.json north_star): dequant / quantize bit-exact; attention within
1e-3 normwise relative error per output row (problems.attn_rel_err), NaN rows
(fully masked) identical.  BASELINE configs 2-5 run at their full sizes.
"""
import zlib

import numpy as np
import pytest

import fattn
from gpu_util import graph_replay, run_gpu, upload, views
from oracle import oracle as orc
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-3


# ------------------------------------------------------------------ unit: dequant / quantize

@pytest.mark.parametrize("typ", [fattn.TYPE_Q8_0, fattn.TYPE_Q4_0])
def test_dequantize_bitexact(dev, typ):
    import torch
    rng = np.random.default_rng(1)
    nblk = 4096
    bb = orc.BLOCK_BYTES[typ]
    blocks = rng.integers(0, 256, size=(nblk, bb), dtype=np.uint8)
    # finite scales spanning normals and subnormals, both signs
    d = orc.f32_to_f16_bits(rng.choice([1, -1], nblk).astype(np.float32) *
                            np.exp2(rng.uniform(-24, 8, nblk)).astype(np.float32))
    blocks[:, 0:2] = d.view(np.uint8).reshape(nblk, 2)
    ref = orc.dequantize(blocks.reshape(-1), typ, nblk * 32).reshape(-1)
    got = fattn.dequantize(torch.from_numpy(blocks.reshape(-1)).to(dev), typ, 128).cpu().numpy().reshape(-1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_dequantize_f16_exhaustive(dev):
    import torch
    bits = np.arange(65536, dtype=np.uint16)
    bits = bits[(bits & 0x7c00) != 0x7c00]  # finite only
    ref = orc.f16_bits_to_f32(bits)
    n = bits.size // 64 * 64
    got = fattn.dequantize(torch.from_numpy(bits[:n].view(np.int16)).to(dev), fattn.TYPE_F16, 64).cpu().numpy()
    assert np.array_equal(got.reshape(-1).view(np.uint32), ref[:n].view(np.uint32))


@pytest.mark.parametrize("typ", [fattn.TYPE_Q8_0, fattn.TYPE_Q4_0])
def test_quantize_bitexact(dev, typ):
    import torch
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((512, 128)) * np.exp2(rng.uniform(-10, 10, (512, 1)))).astype(np.float32)
    x[3] = 0.0  # all-zero block -> d = 0, id = 0
    x[7, :32] = 1.0
    ref = orc.quantize(x, typ)
    got = fattn.quantize(torch.from_numpy(x).to(dev), typ).cpu().numpy()
    assert np.array_equal(got, ref.reshape(got.shape))


# ------------------------------------------------------------------ BASELINE configs (full size)

@pytest.mark.parametrize("layout", ["head", "pos"])
def test_config2_f16_decode(dev, layout):
    p = make_problem(D=128, NQ=1, H=32, N=2048, kv_type="f16", layout=layout, seed=20)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


def test_config2_f16_vtrans(dev):
    """flash_row_float layout: V stored transposed [Hkv][D][N]."""
    p = make_problem(D=128, NQ=1, H=32, N=2048, kv_type="f16", v_trans=True, seed=21)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


@pytest.mark.parametrize("layout", ["head", "pos"])
def test_config3_q8_0(dev, layout):
    p = make_problem(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", layout=layout, seed=30)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("case", [
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", layout="pos"),            # config 3, llama.cpp rows
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", mask="tail"),             # whole chunks -inf
    dict(D=128, NQ=1, H=32, N=2048, kv_type="f16"),                           # config 2's f16
    dict(D=64, NQ=1, H=16, N=16384, kv_type="q4_0"),                          # D = 64, 16+ chunks
    dict(D=256, NQ=1, H=8, N=8192, kv_type="q8_0"),                           # D = 256
], ids=["cfg3_pos", "cfg3_tail", "f16", "d64_q4", "d256"])
def test_row_merge_xcd_order_bit_identical(dev, case):
    """One-row tiles: the XCD-grouped workgroup order (FATTN_OPT_SPLIT_XCD,
    the default for them) gives the plain order's bits and the oracle's
    answer -- the chunk merge sums in a fixed order whichever workgroup
    arrives last."""
    p = make_problem(seed=33, **case)
    ref = p.oracle()
    with fattn.options({fattn.OPT_SPLIT_XCD: 1}):
        base = run_gpu(p)
    with fattn.options({fattn.OPT_SPLIT_XCD: 2}):  # (the auto rule covers the 8-wave row merge only)
        t = upload(p)
        att = fattn.Attention(*views(p, t), t["dst"], p.scale)
        assert "(xcd order)" in att.describe(), att.describe()
        for _ in range(3):
            t["dst"].fill_(float("nan"))
            att()
            got = t["dst"].cpu().numpy()
            assert np.array_equal(got, base, equal_nan=True)
    assert attn_rel_err(got, ref) <= RTOL


@pytest.mark.parametrize("case", [
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0"),                          # config 3
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", layout="pos"),            # llama.cpp rows
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", mask="tail"),             # whole chunks -inf
    dict(D=128, NQ=1, H=32, N=4000, kv_type="q8_0"),                          # ragged last chunk
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", mask="none"),             # no mask
    dict(D=128, NQ=1, H=32, N=2048, kv_type="f16"),                           # config 2
    dict(D=128, NQ=1, H=32, N=8192, kv_type="q4_0"),                          # Q4_0
    dict(D=64, NQ=1, H=32, N=8192, kv_type="q8_0"),                           # D = 64
    dict(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", extreme=True),            # rescales
], ids=["cfg3", "cfg3_pos", "cfg3_tail", "ragged", "nomask", "cfg2_f16", "q4", "d64", "extreme"])
def test_split_loader_waves(dev, case):
    """The loader-wave split kernel (FATTN_OPT_SPLIT_LOADERS = 2,
    fattn_split_ld_kernel): 4 loader waves issue every step up front and hand
    each over by LDS flags; the compute and the chunk merge are the split
    kernel's, so the result equals the 8-wave form's bit for bit and the
    oracle's within 1e-3 -- over repeated launches on one workspace."""
    p = make_problem(seed=35, **case)
    ref = p.oracle()
    base = run_gpu(p)
    with fattn.options({fattn.OPT_SPLIT_LOADERS: 2}):
        t = upload(p)
        att = fattn.Attention(*views(p, t), t["dst"], p.scale)
        if "fattn_split_ld_kernel" not in att.describe():
            pytest.skip("plan not eligible: " + att.describe())
        for _ in range(3):
            t["dst"].fill_(float("nan"))
            att()
            got = t["dst"].cpu().numpy()
            assert np.array_equal(got, base, equal_nan=True)
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


def test_config4_q4_0_gqa(dev):
    p = make_problem(D=128, NQ=1, H=32, Hkv=8, N=8192, kv_type="q4_0", seed=40)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


def test_config5_batch64_shard(dev):
    """Config 5's per-GPU shard: 64 query rows, 4 of the 32 heads, N=4096, Q8_0."""
    p = make_problem(D=128, NQ=64, H=4, N=4096, kv_type="q8_0", seed=50)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


# ------------------------------------------------------------------ multi-query kernel (fattn_mq.h)
# Quantised K/V with >= 32 query rows per kv head and the 16-B layout route to
# the multi-query kernel (64 packed rows per workgroup, tile dequantised once).

def test_config5_full_batch64(dev):
    """Config 5 on one GPU: 64 query rows x 32 heads, N=4096, Q8_0 (split-KV merge)."""
    p = make_problem(D=128, NQ=64, H=32, N=4096, kv_type="q8_0", seed=51)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


def test_config5_shape_f16_full(dev):
    """Config 5's shape over the reference's own cache type (f16 K/V, 64 query
    rows x 32 heads, N = 4096): the batched-decode kernel's f16 path, every
    row against the oracle."""
    p = make_problem(D=128, NQ=64, H=32, N=4096, kv_type="f16", seed=52)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_bd_kernel<f16" in d, d
    got, ref = run_gpu(p), p.oracle(n_threads=16)
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.fixture
def mq_on():
    """The multi-query kernel from 32 packed rows per kv head (the planner
    takes it from 64 rows when every KV chunk holds two 128-key tiles, or
    from 256 rows; an explicit threshold overrides both)."""
    fattn.set_option(fattn.OPT_MQ_MIN_ROWS, 32)
    fattn.set_option(fattn.OPT_BD, 1)  # (64+ rows at D = 128 would take the batched-decode kernel)
    yield
    fattn.set_option(fattn.OPT_MQ_MIN_ROWS, 0)  # the planner default
    fattn.set_option(fattn.OPT_BD, 0)


MQ_CASES = [
    dict(D=128, kv_type="q8_0", NQ=256, H=4, Hkv=4, N=256, mask="causal"),      # prefill, no split
    dict(D=64, kv_type="q4_0", NQ=256, H=4, Hkv=4, N=256, mask="causal"),
    dict(D=128, kv_type="q4_0", NQ=40, H=16, Hkv=4, N=320, mask="random"),      # R=4, ragged query tile
    dict(D=64, kv_type="q8_0", NQ=9, H=16, Hkv=2, N=96, mask="random"),         # R=8, QPT=8, 2 tiles
    dict(D=128, kv_type="q8_0", NQ=1, H=64, Hkv=1, N=64, mask="none"),          # R=64, QPT=1
    dict(D=128, kv_type="q4_0", NQ=33, H=2, Hkv=2, N=2048, mask="neginf_blocks"),
    dict(D=64, kv_type="q8_0", NQ=70, H=2, Hkv=2, N=32, mask="random", S=2),     # one tile, 2 sequences
    dict(D=128, kv_type="q8_0", NQ=300, H=2, Hkv=2, N=256, mask="none"),        # no mask: DMA budget w/o mask
    dict(D=128, kv_type="q4_0", NQ=64, H=8, Hkv=8, N=1024, mask="none"),
    dict(D=128, kv_type="q8_0", NQ=40, H=24, Hkv=4, N=320, mask="random"),      # R=6: 10 queries x 6 heads a tile
    dict(D=64, kv_type="q4_0", NQ=20, H=14, Hkv=2, N=256, mask="causal"),       # R=7
]


@pytest.mark.parametrize("case", MQ_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_mq_sweep(dev, mq_on, case):
    p = make_problem(seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_mq_kernel" in d or "fattn_pf_kernel" in d, d
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


MQ256_CASES = [
    dict(kv_type="q8_0", NQ=256, H=4, Hkv=4, N=256, mask="causal"),       # prefill-shaped, no split
    dict(kv_type="q4_0", NQ=64, H=8, Hkv=2, N=1024, mask="random"),       # R = 4, KV split + merge launch
    dict(kv_type="q8_0", NQ=50, H=2, Hkv=2, N=320, mask="neginf_blocks", S=2),  # ragged tile, 2 seqs
    dict(kv_type="q8_0", NQ=300, H=2, Hkv=2, N=128, mask="none"),
]


@pytest.mark.parametrize("case", MQ256_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_mq_d256(dev, mq_on, case):
    """The multi-query kernel at D = 256 (64-row workgroups: a 256-row tile's
    mask rows do not fit beside the D = 256 images)."""
    p = make_problem(D=256, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_mq_kernel" in d and "D256,4waves" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("case", [
    dict(D=256, kv_type="q4_0", NQ=64, H=8, Hkv=2, N=1024, mask="random"),   # R = 4, KV split + merge launch
    dict(D=256, kv_type="q8_0", NQ=64, H=4, Hkv=4, N=2048, mask="neginf_blocks"),
    dict(D=128, kv_type="q8_0", NQ=48, H=8, Hkv=2, N=1024, extreme=True),
], ids=["d256_q4_gqa", "d256_q8_neginf", "d128_extreme"])
def test_mq_f16_partials(dev, mq_on, case):
    """The multi-query kernel's second-launch merge over f16 chunk partials
    (FATTN_OPT_PART_F16 = 2, the default's choice too), chunked so the merge
    runs: against the oracle."""
    p = make_problem(seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + 7, **case)
    with fattn.options({fattn.OPT_PART_F16: 2}):
        t = upload(p, dev)
        d = fattn.Attention(*views(p, t), t["dst"], p.scale, kv_chunk=256).describe()
        assert "fattn_mq_merge_kernel(f16 partials)" in d, d
        got = run_gpu(p, kv_chunk=256)
    ref = p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.fixture
def rpw64():
    """Force the 256-row workgroups (8 waves x 32 rows) on small problems."""
    fattn.set_option(fattn.OPT_MQ_ROWS_PER_WAVE, 32)
    yield
    fattn.set_option(fattn.OPT_MQ_ROWS_PER_WAVE, 0)


MQ64_CASES = [
    dict(D=128, kv_type="q8_0", NQ=300, H=2, Hkv=2, N=256, mask="causal"),      # ragged 256-row tile
    dict(D=128, kv_type="q4_0", NQ=64, H=16, Hkv=2, N=512, mask="random"),      # R=8: 32 queries x 8 heads
    dict(D=64, kv_type="q8_0", NQ=256, H=2, Hkv=2, N=128, mask="none"),
    dict(D=64, kv_type="q4_0", NQ=100, H=4, Hkv=4, N=96, mask="neginf_blocks", S=2),
    dict(D=128, kv_type="q8_0", NQ=300, H=2, Hkv=2, N=256, mask="none"),
]


@pytest.mark.parametrize("case", MQ64_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_mq_rpw64_sweep(dev, mq_on, rpw64, case):
    p = make_problem(seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


@pytest.mark.parametrize("chunk", [64, 1000])
def test_mq_rpw64_split(dev, mq_on, rpw64, chunk):
    """256-row workgroups with split-KV partials (16 subtiles merged per tile)."""
    p = make_problem(D=128, NQ=260, H=2, N=1024, kv_type="q8_0", seed=23)
    assert attn_rel_err(run_gpu(p, kv_chunk=chunk), p.oracle()) <= RTOL


def test_mq_matches_split_kernel(dev, mq_on):
    """The two kernels on one problem (multi-query vs split-KV forced)."""
    p = make_problem(D=128, NQ=64, H=4, Hkv=2, N=512, kv_type="q4_0", seed=24)
    a = run_gpu(p)
    fattn.set_option(fattn.OPT_MQ_DISABLE, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_MQ_DISABLE, 0)
    assert attn_rel_err(a, b) <= RTOL
    assert attn_rel_err(a, p.oracle()) <= RTOL


@pytest.mark.parametrize("chunk", [32, 96, 512, 100000])
def test_mq_chunking_invariance(dev, mq_on, chunk):
    p = make_problem(D=128, NQ=48, H=8, Hkv=2, N=1024, kv_type="q8_0", seed=17)
    assert attn_rel_err(run_gpu(p, kv_chunk=chunk), p.oracle()) <= RTOL


@pytest.mark.parametrize("kt", ["q8_0", "q4_0"])
def test_mq_extreme_rescale(dev, mq_on, kt):
    p = make_problem(D=128, NQ=64, H=2, N=1024, kv_type=kt, seed=18, extreme=True)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


@pytest.mark.parametrize("rpw", [0, 32])
@pytest.mark.parametrize("kt", ["q8_0", "q4_0"])
def test_mq_rescale_ramp(dev, mq_on, kt, rpw):
    """Scores rising along the sequence: many deferred-max steps and rescales."""
    fattn.set_option(fattn.OPT_MQ_ROWS_PER_WAVE, rpw)
    try:
        p = make_problem(D=128, NQ=64, H=4, N=2048, kv_type=kt, seed=25, ramp=12.0, mask="none")
        got = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_MQ_ROWS_PER_WAVE, 0)
    assert attn_rel_err(got, p.oracle()) <= RTOL


def test_mq_fully_masked_rows_are_nan(dev, mq_on):
    p = make_problem(D=128, NQ=40, H=2, N=256, kv_type="q4_0", mask="zero", seed=19)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[5, :] = -np.inf
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert np.isnan(ref[:, 5]).all() and np.isnan(got[:, 5]).all()
    assert attn_rel_err(got, ref) <= RTOL


# ------------------------------------------------------------------ mixed K / V cache types
# llama.cpp takes separate K and V cache types (-ctk / -ctv); the split kernel
# is instantiated for every pair of F16 / Q8_0 / Q4_0 at D = 64, 128, 256.

MIXED_PAIRS = [("q8_0", "f16"), ("q4_0", "f16"), ("f16", "q8_0"), ("f16", "q4_0"), ("q8_0", "q4_0"), ("q4_0", "q8_0")]


@pytest.mark.parametrize("kt,vt", MIXED_PAIRS, ids=lambda x: x)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_mixed_kv_types_decode(dev, kt, vt, D):
    p = make_problem(D=D, NQ=1, H=8, N=1024, kv_type=kt, v_type=vt, seed=60 + D)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert d.startswith(f"fattn_split_kernel<{kt},{vt},D{D},"), d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("kt,vt", MIXED_PAIRS[:3], ids=lambda x: x)
@pytest.mark.parametrize("case", [
    dict(NQ=16, H=32, Hkv=8, N=2048, mask="causal"),         # GQA multi-row tiles, merge launch
    dict(NQ=3, H=8, Hkv=2, N=800, layout="pos", mask="tail"),  # llama.cpp [N][Hkv] cache, dword path, tails
    dict(NQ=64, H=4, Hkv=4, N=4096),                         # config 5's shard shape
], ids=["gqa_causal", "pos_tail", "cfg5_shard"])
def test_mixed_kv_types_multirow(dev, kt, vt, case):
    p = make_problem(D=128, kv_type=kt, v_type=vt, seed=61, **case)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


# ------------------------------------------------------------------ batched-decode kernel (fattn_bd.h)
# 64 packed rows per workgroup, 128-key tiles over 8 waves, chunk partials
# merged by a second launch.  The planner takes it from 64 packed rows per kv
# head (D = 128, Q8_0 / Q4_0, contiguous rows); FATTN_OPT_BD = 2 forces it.

@pytest.fixture
def bd_force():
    fattn.set_option(fattn.OPT_BD, 2)
    yield
    fattn.set_option(fattn.OPT_BD, 0)


BD_CASES = [
    dict(kv_type="q8_0", NQ=64, H=8, Hkv=8, N=4096, mask="random"),          # config 5 shape, 8 heads
    dict(kv_type="q4_0", NQ=64, H=4, Hkv=4, N=2048, mask="random"),
    dict(kv_type="q8_0", NQ=16, H=16, Hkv=4, N=1024, mask="random"),         # GQA: 16 queries x 4 heads
    dict(kv_type="q4_0", NQ=8, H=64, Hkv=8, N=512, mask="random"),           # R = 8
    dict(kv_type="q8_0", NQ=40, H=2, Hkv=2, N=800, mask="random"),           # ragged rows, N % 128 = 32
    dict(kv_type="q8_0", NQ=130, H=2, Hkv=2, N=4064, mask="random"),         # three query tiles, tail quarter
    dict(kv_type="q8_0", NQ=64, H=2, Hkv=2, N=96, mask="random"),            # one partial tile
    dict(kv_type="q4_0", NQ=64, H=4, Hkv=4, N=1024, mask="none"),
    dict(kv_type="q8_0", NQ=64, H=2, Hkv=2, N=2048, mask="neginf_blocks"),   # -inf block skip
    dict(kv_type="q8_0", NQ=64, H=2, Hkv=2, N=1024, mask="causal"),
    dict(kv_type="q8_0", NQ=33, H=2, Hkv=2, N=1024, mask="random", S=2),     # ne03 batch
    dict(kv_type="q4_0", NQ=64, H=4, Hkv=2, N=640, mask="tail", S=2, Skv=1),  # seq broadcast, padded cache
    # GQA ratios that are not powers of two (R = 6, 3, 48): a tile packs floor(64 / R)
    # whole head groups, its last rows stay empty
    dict(kv_type="q8_0", NQ=64, H=24, Hkv=4, N=1024, mask="random"),
    dict(kv_type="q4_0", NQ=40, H=12, Hkv=4, N=768, mask="causal"),
    dict(kv_type="q8_0", NQ=5, H=48, Hkv=1, N=512, mask="random"),
    dict(kv_type="f16", NQ=64, H=24, Hkv=4, N=1024, mask="random"),
    # f16 K/V (the reference's own cache type): images filled by LDS-DMA from the rows
    dict(kv_type="f16", NQ=64, H=8, Hkv=8, N=4096, mask="random"),           # config 5 shape, 8 heads
    dict(kv_type="f16", NQ=16, H=16, Hkv=4, N=1024, mask="random"),          # GQA
    dict(kv_type="f16", NQ=40, H=2, Hkv=2, N=800, mask="random"),            # ragged rows, N % 128 = 32
    dict(kv_type="f16", NQ=64, H=2, Hkv=2, N=96, mask="random"),             # one partial tile
    dict(kv_type="f16", NQ=64, H=4, Hkv=4, N=1024, mask="none"),
    dict(kv_type="f16", NQ=64, H=2, Hkv=2, N=2048, mask="neginf_blocks"),
    dict(kv_type="f16", NQ=64, H=4, Hkv=2, N=1056, mask="causal", layout="pos"),  # llama.cpp's [N][Hkv] cache
    dict(kv_type="f16", NQ=33, H=2, Hkv=2, N=1024, mask="random", S=2),      # ne03 batch
    dict(kv_type="f16", NQ=64, H=4, Hkv=2, N=640, mask="tail", S=2, Skv=1),  # seq broadcast, padded cache
]


@pytest.mark.parametrize("case", BD_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bd_sweep(dev, bd_force, case):
    p = make_problem(D=128, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_bd_kernel" in d, d
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("case", [
    dict(NQ=64, H=8, Hkv=8, N=4096, mask="random"),                  # config-5 shape, 8 heads
    dict(NQ=16, H=16, Hkv=4, N=1024, mask="causal"),                 # GQA
    dict(NQ=40, H=12, Hkv=4, N=800, mask="random"),                  # R = 3, ragged rows, partial tile
    dict(NQ=64, H=4, Hkv=2, N=1056, mask="neginf_blocks", layout="pos"),  # llama.cpp's [N][Hkv] cache
    dict(NQ=33, H=2, Hkv=2, N=1024, mask="none", S=2),               # ne03 batch, no mask
], ids=["cfg5x8", "gqa4", "gqa3", "pos", "batch2"])
def test_bd_f16_dims(dev, bd_force, case, D):
    """The f16 image ring of the batched-decode kernel at head dims 64 and 96
    (D / 2 1-KiB image pieces per 128-key tile; Q rows of D / 4 16-B chunks)."""
    p = make_problem(D=D, kv_type="f16", seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + D, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert d.startswith("fattn_bd_kernel<f16") and f"D{D}" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


# ------------------------------------------------------------------ batched decode, role form (fattn_bdp.h)
# Q8_0 / Q4_0: compute waves 0-3 and build (dequantising) waves 4-7, 64-key
# tiles, one barrier per tile; FATTN_OPT_BD = 3 forces it (0 picks it too).

@pytest.fixture
def bdp_force():
    fattn.set_option(fattn.OPT_BD, 3)
    yield
    fattn.set_option(fattn.OPT_BD, 0)


BDP_CASES = [c for c in BD_CASES if c["kv_type"] != "f16"] + [
    dict(kv_type="q8_0", NQ=64, H=2, Hkv=2, N=192, mask="random"),           # 3 tiles: raw ring never refilled
    dict(kv_type="q4_0", NQ=64, H=2, Hkv=2, N=320, mask="causal"),           # 5 tiles: one refill
    dict(kv_type="q8_0", NQ=64, H=4, Hkv=4, N=1056, mask="random", layout="pos"),
]


@pytest.mark.parametrize("case", BDP_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bdp_sweep(dev, bdp_force, case):
    p = make_problem(D=128, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + 7, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    if case.get("layout") == "pos":  # (quantised rows not contiguous per head: the split kernel)
        assert "fattn_bdp_kernel" not in d, d
    else:
        assert "fattn_bdp_kernel" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("chunk", [128, 384, 1024, 100000])
@pytest.mark.parametrize("mask", ["random", "neginf_blocks", "causal"])
def test_bdp_chunking_and_masks(dev, bdp_force, chunk, mask):
    """One to many 64-key tiles per workgroup (the raw ring's refills, the
    mask ring's), masks that skip whole 32 x 32 blocks."""
    p = make_problem(D=128, NQ=64, H=4, N=2048, kv_type="q8_0", mask=mask, seed=37)
    got, ref = run_gpu(p, kv_chunk=chunk), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("kt", ["q8_0", "q4_0"])
def test_bdp_rescale(dev, bdp_force, kt):
    p = make_problem(D=128, NQ=64, H=2, N=2048, kv_type=kt, seed=38, extreme=True)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL
    p = make_problem(D=128, NQ=64, H=2, N=4096, kv_type=kt, seed=39, ramp=12.0, mask="none")
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


def test_bdp_fully_masked_rows_are_nan_and_deterministic(dev, bdp_force):
    p = make_problem(D=128, NQ=64, H=2, N=1024, kv_type="q8_0", mask="random", seed=41)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[7, :] = -np.inf
    m[63, :] = -np.inf
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert np.isnan(got[:, 7]).all() and np.isnan(got[:, 63]).all()
    assert attn_rel_err(got, ref) <= RTOL
    again = run_gpu(p)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_bdp_matches_bd_bitwise_inputs(dev):
    """The role form against the all-waves form on one problem (same
    dequantisation, same products; only the merge order of the key groups
    differs), and both against the oracle."""
    p = make_problem(D=128, NQ=64, H=8, Hkv=4, N=4096, kv_type="q8_0", seed=44)
    with fattn.options({fattn.OPT_BD: 3}):
        a = run_gpu(p)
    with fattn.options({fattn.OPT_BD: 2}):
        b = run_gpu(p)
    assert attn_rel_err(a, b) <= RTOL
    assert attn_rel_err(a, p.oracle()) <= RTOL


@pytest.mark.parametrize("form", [2, 3])
@pytest.mark.parametrize("case", [
    dict(kv_type="q8_0", NQ=64, H=8, Hkv=8, N=4096, mask="random"),           # 8 chunks x 8 tiles: grid % 8 == 0
    dict(kv_type="q4_0", NQ=40, H=12, Hkv=4, N=768, mask="causal"),           # R = 3, 2 row tiles
    dict(kv_type="q8_0", NQ=64, H=4, Hkv=2, N=1024, mask="random", S=2),      # ne03 batch
], ids=["cfg5x8", "gqa3", "batch2"])
def test_bd_xcd_order(dev, case, form):
    """The XCD-grouped workgroup order (FATTN_OPT_BD_XCD = 2) relabels the
    grid only: same plan, results against the oracle and bit-identical to the
    plain order (each workgroup's arithmetic is unchanged)."""
    p = make_problem(D=128, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + 3, **case)
    t = upload(p, dev)
    with fattn.options({fattn.OPT_BD: form, fattn.OPT_BD_XCD: 2}):
        d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
        got = run_gpu(p)
    with fattn.options({fattn.OPT_BD: form, fattn.OPT_BD_XCD: 1}):
        plain = run_gpu(p)
    gx, gy, gz = (int(x) for x in d.split("grid(")[1].split(")")[0].split(","))
    assert ("(xcd order)" in d) == ((gx * gy * gz) % 8 == 0), d
    assert attn_rel_err(got, p.oracle()) <= RTOL
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


# head dim 64: the role form with one half-block per build wave (FATTN_OPT_BD = 3)
BDP64_CASES = [
    dict(kv_type="q8_0", NQ=64, H=8, Hkv=8, N=4096, mask="random"),
    dict(kv_type="q4_0", NQ=64, H=4, Hkv=4, N=2048, mask="random"),
    dict(kv_type="q8_0", NQ=16, H=16, Hkv=4, N=1024, mask="causal"),
    dict(kv_type="q4_0", NQ=40, H=12, Hkv=4, N=768, mask="random"),          # R = 3
    dict(kv_type="q8_0", NQ=40, H=2, Hkv=2, N=800, mask="random"),           # ragged rows, partial tile
    dict(kv_type="q8_0", NQ=64, H=2, Hkv=2, N=192, mask="neginf_blocks"),
    dict(kv_type="q4_0", NQ=64, H=4, Hkv=2, N=640, mask="tail", S=2, Skv=1),
    dict(kv_type="q8_0", NQ=64, H=4, Hkv=4, N=1024, mask="none"),
]


@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("case", BDP64_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bdp_d64(dev, bdp_force, case, D):
    """Head dims 64 and 96 (D = 96: 102 / 54-B rows, three ggml blocks dealt
    as six half-blocks over the four build waves; Q rows of 24 16-B chunks)."""
    p = make_problem(D=D, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + 9, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_bdp_kernel" in d and f"D{D}" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("chunk", [128, 1024])
def test_bdp_d64_chunking(dev, bdp_force, chunk, D):
    p = make_problem(D=D, NQ=64, H=4, N=2048, kv_type="q8_0", mask="causal", seed=46)
    got, ref = run_gpu(p, kv_chunk=chunk), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("case,chunk", [
    (dict(NQ=1024, H=8, N=1024, mask="causal"), 0),   # 16 query tiles x 2 chunks of 4 tiles
    (dict(NQ=1024, H=8, N=1024, mask="random"), 0),
    (dict(NQ=64, H=1, N=512, mask="causal"), 512),     # one workgroup, 4 tiles, one chunk
    (dict(NQ=64, H=1, N=512, mask="random"), 512),
    (dict(NQ=64, H=1, N=512, mask="neginf_blocks"), 512),
    (dict(NQ=64, H=4, N=4096, mask="neginf_blocks"), 1024),
], ids=["causal-16qt", "random-16qt", "causal-1wg", "random-1wg", "neginf-1wg", "neginf-8tiles"])
@pytest.mark.parametrize("kt", ["q8_0", "f16"])
def test_bd_masked_multitile(dev, bd_force, case, chunk, kt):
    """Masked problems whose workgroups walk several 128-key tiles: the mask
    of tile s + 1 is fetched while tile s computes (a one-workgroup launch
    leaves the least time for it to land).  A register-held form of that
    prefetch failed exactly these cases (rows 31 / 63 NaN).  f16: the image
    pair of tile s + 1 is filled while tile s computes from the other."""
    p = make_problem(D=128, kv_type=kt, seed=43, **case)
    got, ref = run_gpu(p, kv_chunk=chunk), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("kt", ["q8_0", "f16"])
@pytest.mark.parametrize("chunk", [128, 384, 1024, 100000])
def test_bd_chunking_invariance(dev, bd_force, chunk, kt):
    p = make_problem(D=128, NQ=64, H=4, N=2048, kv_type=kt, seed=27)
    assert attn_rel_err(run_gpu(p, kv_chunk=chunk), p.oracle()) <= RTOL


@pytest.mark.parametrize("kt", ["q8_0", "q4_0", "f16"])
def test_bd_extreme_rescale(dev, bd_force, kt):
    p = make_problem(D=128, NQ=64, H=2, N=2048, kv_type=kt, seed=28, extreme=True)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


@pytest.mark.parametrize("kt", ["q8_0", "q4_0", "f16"])
def test_bd_rescale_ramp(dev, bd_force, kt):
    p = make_problem(D=128, NQ=64, H=2, N=4096, kv_type=kt, seed=29, ramp=12.0, mask="none")
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


def test_bd_fully_masked_rows_are_nan(dev, bd_force):
    p = make_problem(D=128, NQ=64, H=2, N=1024, kv_type="q8_0", mask="random", seed=31)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[5, :] = -np.inf
    m[40, :] = -np.inf
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert np.isnan(ref[:, 5]).all() and np.isnan(got[:, 5]).all()
    assert np.isnan(got[:, 40]).all()
    assert attn_rel_err(got, ref) <= RTOL


@pytest.mark.parametrize("kt", ["q8_0", "f16"])
def test_bd_deterministic(dev, bd_force, kt):
    p = make_problem(D=128, NQ=64, H=4, N=4096, kv_type=kt, seed=32)
    a, b = run_gpu(p), run_gpu(p)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bd_matches_split_kernel(dev, bd_force):
    """The batched-decode kernel against the split kernel on one problem."""
    p = make_problem(D=128, NQ=64, H=4, Hkv=2, N=1024, kv_type="q4_0", seed=33)
    a = run_gpu(p)
    fattn.set_option(fattn.OPT_MQ_DISABLE, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_MQ_DISABLE, 0)
    assert attn_rel_err(a, b) <= RTOL
    assert attn_rel_err(a, p.oracle()) <= RTOL


@pytest.mark.parametrize("kt,N,chunk", [("q8_0", 4096, 0), ("q4_0", 2048, 256), ("f16", 1024, 128), ("q8_0", 96, 32),
                                        ("q8_0", 4096, 256),    # 64 parts: two load batches
                                        ("q8_0", 4096, 128)])   # 128 parts: workgroup-level merge
def test_wave_merge(dev, kt, N, chunk):
    """One-row split tiles (n_q = 1, H == Hkv): per-wave partials merged by the
    last-arriving wave, against the oracle and against the workgroup-level merge
    (FATTN_OPT_SPLIT_WAVE_MERGE = 1)."""
    p = make_problem(D=128, NQ=1, H=8, N=N, kv_type=kt, mask="random", seed=41)
    a = run_gpu(p, kv_chunk=chunk)
    fattn.set_option(fattn.OPT_SPLIT_WAVE_MERGE, 1)
    try:
        b = run_gpu(p, kv_chunk=chunk)
    finally:
        fattn.set_option(fattn.OPT_SPLIT_WAVE_MERGE, 0)
    ref = p.oracle()
    assert attn_rel_err(a, ref) <= RTOL
    assert attn_rel_err(b, ref) <= RTOL


def test_wave_merge_fully_masked_is_nan(dev):
    p = make_problem(D=128, NQ=1, H=4, N=2048, kv_type="q8_0", mask="zero", seed=42)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[0, :] = -np.inf
    p.mask_bits = orc.f32_to_f16_bits(m)
    got = run_gpu(p)
    assert np.isnan(got).all()


# ------------------------------------------------------------------ prefill kernel (fattn_pf.h)
# 256-row workgroups over 64-key tiles (32x32 MFMA); auto-selected when the
# workgroups fill the chip, forced here (OPT_PF = 2) on small problems.

@pytest.fixture(params=[(0, 1), (1, 1), (0, 4), (0, 5), (0, 6)],
                ids=["staged", "inkernel_deq", "staged_pf4p", "staged_pf4b", "staged_pf4l"])
def pf_force(request):
    """The prefill kernels on every eligible problem: Q8_0 / Q4_0 K/V staged
    to f16 first (the default) or dequantised inside the kernel
    (FATTN_OPT_PF_STAGE = 1); the f16 body in its 8-wave form (fattn_pf.h)
    or one wave per SIMD (fattn_pf4.h, D = 128; FATTN_OPT_PF_FORM = the
    pipelined 4 and the balanced 5)."""
    stage, form = request.param
    fattn.set_option(fattn.OPT_PF, 2)
    fattn.set_option(fattn.OPT_PF_STAGE, stage)
    fattn.set_option(fattn.OPT_PF_FORM, form)
    yield
    fattn.set_option(fattn.OPT_PF, 0)
    fattn.set_option(fattn.OPT_PF_STAGE, 0)
    fattn.set_option(fattn.OPT_PF_FORM, 0)


@pytest.mark.parametrize("case", [
    dict(kv_type="f16", NQ=256, H=4, Hkv=4, N=512, mask="random"),
    dict(kv_type="q8_0", NQ=512, H=4, Hkv=2, N=256, mask="causal"),           # staged, GQA, causal
    dict(kv_type="q4_0", NQ=300, H=2, Hkv=2, N=384, mask="none"),             # ragged query tiles, no mask
    dict(kv_type="f16", NQ=256, H=2, Hkv=2, N=256, S=2, mask="random", layout="pos"),  # two sequences, [N][Hkv]
    dict(kv_type="q8_0", NQ=256, H=2, Hkv=2, N=1024, mask="random", extreme=True),     # rescales
    dict(kv_type="f16", NQ=256, H=2, Hkv=2, N=128, mask="random"),            # two tiles (prologue paths)
    dict(kv_type="f16", NQ=256, H=2, Hkv=2, N=64, mask="random"),             # one tile
    dict(kv_type="q8_0", NQ=300, H=2, Hkv=2, N=512, mask="zero"),             # +-0 mask: the ZM body
], ids=["f16", "q8_causal_gqa", "q4_nomask_ragged", "f16_seq2_pos", "q8_extreme", "two_tiles", "one_tile", "q8_zero_mask"])
def test_pf4_bit_identical_to_pf(dev, case):
    """The one-wave-per-SIMD prefill body (fattn_pf4_kernel) runs the 8-wave
    body's arithmetic in the same order -- per 64-key tile the same S^T
    chains, tile max, deferred-rescale rule, exponentials, row-sum pairing and
    P.V accumulation order -- so its output has the same bits, and the
    oracle's answer."""
    p = make_problem(seed=88, **case)
    outs = {}
    fattn.set_option(fattn.OPT_PF, 2)
    try:
        for form in (1, 4, 5, 6):
            fattn.set_option(fattn.OPT_PF_FORM, form)
            t = upload(p)
            att = fattn.Attention(*views(p, t), t["dst"], p.scale)
            assert ("fattn_pf4_kernel" in att.describe()) == (form >= 4), att.describe()
            assert ("(pipelined)" in att.describe()) == (form == 4), att.describe()
            assert ("(lean)" in att.describe()) == (form == 6), att.describe()
            assert ("(balanced)" in att.describe()) == (form == 5), att.describe()
            att()
            outs[form] = t["dst"].cpu().numpy()
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
        fattn.set_option(fattn.OPT_PF_FORM, 0)
    assert np.array_equal(outs[1], outs[4], equal_nan=True)
    # the lean form (S^T chains started from -m / c) is not bit-identical -- the
    # -m / c enters the f32 accumulation -- but within the oracle's bar,
    # with the same NaN rows
    assert np.array_equal(np.isnan(outs[6]), np.isnan(outs[1]))
    assert attn_rel_err(outs[6], p.oracle()) <= RTOL
    assert attn_elem_err(outs[6], p.oracle()) <= 1.0
    assert np.array_equal(outs[1], outs[5], equal_nan=True)
    assert attn_rel_err(outs[4], p.oracle()) <= RTOL


@pytest.mark.parametrize("case", [
    dict(kv_type="q8_0", NQ=256, H=4, Hkv=4, N=512, mask="random"),
    dict(kv_type="q4_0", NQ=512, H=4, Hkv=2, N=256, mask="causal"),
    dict(kv_type="q8_0", NQ=256, H=2, Hkv=2, N=512, D=96, mask="none"),
    dict(kv_type="q4_0", NQ=256, H=2, Hkv=2, N=256, D=64, mask="random"),
    dict(kv_type="q8_0", NQ=256, H=2, Hkv=2, N=256, S=2, mask="random"),
], ids=["q8", "q4_causal_gqa", "q8_d96", "q4_d64", "q8_seq2"])
def test_pf_staged_equals_inkernel_dequant(dev, case):
    """kv_stage_f16 writes h(q * d) -- the value the prefill kernel's own
    dequantisation puts in its f16 images -- so the staged prefill (default)
    and the in-kernel form give the same bits, and the oracle's answer."""
    p = make_problem(seed=77, **case)
    fattn.set_option(fattn.OPT_PF, 2)
    try:
        outs = {}
        for st in (2, 1):
            fattn.set_option(fattn.OPT_PF_STAGE, st)
            t = upload(p)
            att = fattn.Attention(*views(p, t), t["dst"], p.scale)
            assert ("kv_stage_f16" in att.describe()) == (st == 2), att.describe()
            att()
            outs[st] = t["dst"].cpu().numpy()
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
        fattn.set_option(fattn.OPT_PF_STAGE, 0)
    assert np.array_equal(outs[1], outs[2], equal_nan=True)
    assert attn_rel_err(outs[2], p.oracle()) <= RTOL


PF_CASES = [
    dict(kv_type="q8_0", NQ=256, H=4, Hkv=4, N=256, mask="causal"),
    dict(kv_type="q4_0", NQ=256, H=2, Hkv=2, N=512, mask="random"),
    dict(kv_type="q4_0", NQ=64, H=16, Hkv=4, N=512, mask="random"),          # R=4: 64 queries x 4 heads
    dict(kv_type="q8_0", NQ=40, H=16, Hkv=2, N=128, mask="random"),          # R=8, ragged query tile
    dict(kv_type="q8_0", NQ=300, H=2, Hkv=2, N=256, mask="none"),            # two query tiles, ragged
    dict(kv_type="q8_0", NQ=100, H=2, Hkv=2, N=192, mask="neginf_blocks", S=2),  # odd tile count, 2 seqs
    dict(kv_type="q4_0", NQ=256, H=2, Hkv=2, N=64, mask="zero"),             # one tile
    dict(kv_type="q8_0", NQ=4, H=64, Hkv=1, N=128, mask="random"),           # R=64, QPT=4
    dict(kv_type="q8_0", NQ=100, H=24, Hkv=4, N=256, mask="causal"),         # R=6: QPT=42, 252 rows a tile
    dict(kv_type="q4_0", NQ=90, H=20, Hkv=4, N=192, mask="random"),          # R=5
    dict(kv_type="f16", NQ=64, H=24, Hkv=2, N=128, mask="random"),           # R=12, QPT=21
    # f16 K/V: images filled by LDS-DMA straight from the rows
    dict(kv_type="f16", NQ=256, H=4, Hkv=4, N=256, mask="causal"),
    dict(kv_type="f16", NQ=100, H=8, Hkv=2, N=192, mask="random", layout="pos"),  # rows strided by Hkv
    dict(kv_type="f16", NQ=300, H=2, Hkv=2, N=128, mask="none", S=2),
    dict(kv_type="f16", NQ=256, H=2, Hkv=2, N=64, mask="neginf_blocks"),        # one tile
]


@pytest.mark.parametrize("case", PF_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_pf_sweep(dev, pf_force, case):
    p = make_problem(D=128, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


PF64_CASES = [
    dict(kv_type="q8_0", NQ=256, H=4, Hkv=4, N=512, mask="causal"),
    dict(kv_type="q4_0", NQ=300, H=2, Hkv=2, N=256, mask="random"),           # two query tiles, ragged
    dict(kv_type="q8_0", NQ=64, H=16, Hkv=4, N=192, mask="zero"),             # R = 4, odd tile count
    dict(kv_type="f16", NQ=256, H=4, Hkv=4, N=256, mask="neginf_blocks"),
    dict(kv_type="f16", NQ=100, H=8, Hkv=2, N=128, mask="none", layout="pos", S=2),
]


@pytest.mark.parametrize("case", PF64_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_pf_d64(dev, pf_force, case):
    """The prefill kernel at D = 64: four K dim slices / two V dim blocks per
    image, waves 0-3 dequantise (one half block each)."""
    p = make_problem(D=64, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_pf_kernel" in d and "D64" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


PF96_CASES = [
    dict(kv_type="q8_0", NQ=256, H=4, Hkv=4, N=512, mask="causal"),           # 102-B rows
    dict(kv_type="q4_0", NQ=300, H=2, Hkv=2, N=256, mask="random"),           # 54-B rows, ragged tiles
    dict(kv_type="q8_0", NQ=64, H=24, Hkv=4, N=192, mask="zero"),             # R = 6 (QPT 42)
    dict(kv_type="f16", NQ=256, H=4, Hkv=4, N=256, mask="neginf_blocks"),     # 192-B rows, direct fill
    dict(kv_type="f16", NQ=100, H=8, Hkv=2, N=128, mask="none", layout="pos", S=2),
]


@pytest.mark.parametrize("case", PF96_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_pf_d96(dev, pf_force, case):
    """The prefill kernel at D = 96: six K dim slices /
    three V dim blocks per image, waves 0-5 dequantise (one half block each);
    f16: 24 1-KiB image pieces per tile, three per wave."""
    p = make_problem(D=96, seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_pf_kernel" in d and "D96" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


PF80_CASES = [
    dict(NQ=256, H=4, Hkv=4, N=256, mask="causal"),
    dict(NQ=300, H=2, Hkv=2, N=192, mask="random"),                           # ragged query tiles
    dict(NQ=64, H=24, Hkv=4, N=128, mask="zero"),                             # R = 6
    dict(NQ=100, H=8, Hkv=2, N=128, mask="none", layout="pos", S=2),          # [N][Hkv] rows, 2 sequences
    dict(NQ=256, H=2, Hkv=2, N=256, mask="neginf_blocks"),
]


@pytest.mark.parametrize("case", PF80_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_pf_d80_f16(dev, pf_force, case):
    """The prefill kernel at D = 80 (f16 K/V): images laid out as 96 dims, the
    16 past D zero in Q, K and V (DMA'd from past the descriptor), the output's
    padding dims not stored -- the neighbouring heads' dst rows stay intact."""
    p = make_problem(D=80, kv_type="f16", seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000 + 5, **case)
    t = upload(p, dev)
    d = fattn.Attention(*views(p, t), t["dst"], p.scale).describe()
    assert "fattn_pf_kernel" in d and "D80" in d, d
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("kt", ["q8_0", "q4_0"])
def test_pf_rescale(dev, pf_force, kt):
    """Large scores and scores rising along the sequence: deferred-max rescales."""
    for extreme, ramp, seed in ((True, 0.0, 26), (False, 12.0, 27)):
        p = make_problem(D=128, NQ=256, H=2, N=2048, kv_type=kt, seed=seed, extreme=extreme, ramp=ramp,
                         mask="none" if ramp else "random")
        assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


def test_pf_fully_masked_rows_are_nan(dev, pf_force):
    p = make_problem(D=128, NQ=256, H=2, N=256, kv_type="q8_0", mask="zero", seed=28)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[7, :] = -np.inf
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert np.isnan(ref[:, 7]).all() and np.isnan(got[:, 7]).all()
    assert attn_rel_err(got, ref) <= RTOL


@pytest.mark.parametrize("kt", ["q8_0", "f16"])
def test_pf_zero_mask_blocks(dev, pf_force, kt):
    """Mask blocks classified by the pre-pass: all +-0 (flag 2: the block's mask
    DMA fetches nothing, zeros land), mixed, all -inf (skipped), and -0.0
    entries -- two query tiles x eight key tiles, against the oracle."""
    p = make_problem(D=128, NQ=512, H=2, N=512, kv_type=kt, mask="random", seed=47)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[:, 0:128] = 0.0                     # zero blocks for both query tiles
    m[:256, 128:192] = -0.0               # negative zeros still add nothing
    m[256:, 192:256] = -np.inf            # one fully masked block of the second tile
    m[:256, 448:512] = 0.0
    m[300, 448] = 0.5                     # one value breaks the second tile's zero block
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL
    assert attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("skip", [0, 1], ids=["range", "noprepass"])
@pytest.mark.parametrize("kt", ["q8_0", "f16"])
def test_pf_causal_block_skip(dev, kt, skip):
    """Causal prefill (n_q = N = 1024, 8 heads): the prefill kernel skips every
    wave's fully masked 32 x 64 blocks; against the multi-query / split kernel
    (no skipping) and one head against the oracle."""
    p = make_problem(D=128, NQ=1024, H=8, N=1024, kv_type=kt, mask="causal", seed=43)
    fattn.set_option(fattn.OPT_PF, 2)
    fattn.set_option(fattn.OPT_PF_SKIP, skip)
    try:
        a = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
        fattn.set_option(fattn.OPT_PF_SKIP, 0)
    fattn.set_option(fattn.OPT_PF, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
    assert np.isfinite(a).all()
    assert attn_rel_err(a, b) <= RTOL
    sub = make_problem(D=128, NQ=1024, H=1, N=1024, kv_type=kt, mask="causal", seed=43)
    sub.q = np.ascontiguousarray(p.q[:, :, 3:4, :])
    sub.k_bytes = np.ascontiguousarray(p.k_bytes.reshape(p.Hkv, -1)[3:4].reshape(-1))
    sub.v_bytes = np.ascontiguousarray(p.v_bytes.reshape(p.Hkv, -1)[3:4].reshape(-1))
    sub.mask_bits = p.mask_bits
    assert attn_rel_err(a[:, :, 3:4, :], sub.oracle()) <= RTOL


def test_pf_f16_prefill_full(dev):
    """f16 K/V at the prefill shape (n_q = N = 4096, 32 heads, random mask): the
    prefill kernel against the split-KV kernel, and every head x three
    query-row blocks (start, middle, end of the sequence) against the oracle."""
    p = make_problem(D=128, NQ=4096, H=32, N=4096, kv_type="f16", seed=33)
    a = run_gpu(p)
    fattn.set_option(fattn.OPT_PF, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
    assert np.isfinite(a).all()
    assert attn_rel_err(a, b) <= RTOL
    rows = np.r_[0:128, 2048:2176, 3968:4096]
    sub = make_problem(D=128, NQ=len(rows), H=32, N=4096, kv_type="f16", seed=33)
    sub.q = np.ascontiguousarray(p.q[:, rows])
    sub.k_bytes, sub.v_bytes = p.k_bytes, p.v_bytes
    sub.mask_bits = np.ascontiguousarray(p.mask_bits[rows])
    ref = sub.oracle(n_threads=16)
    assert attn_rel_err(a[:, rows], ref) <= RTOL
    assert attn_elem_err(a[:, rows], ref) <= 1.0


def test_pf_prefill_full_matches_mq(dev):
    """The prefill shape at full size (n_q = N = 4096, 32 heads, Q8_0, random mask):
    the prefill kernel (auto-selected) against the multi-query kernel, and all
    32 heads x three query-row blocks of 128 rows (start, middle, end of the
    sequence) against the oracle."""
    p = make_problem(D=128, NQ=4096, H=32, N=4096, kv_type="q8_0", seed=29)
    a = run_gpu(p)
    fattn.set_option(fattn.OPT_PF, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
    assert np.isfinite(a).all()
    assert attn_rel_err(a, b) <= RTOL
    # every head x three query-row blocks (start, middle, end of the sequence)
    # against the oracle: the rows are independent, so the sub-problem is the
    # same K / V with those rows of Q and of the mask
    rows = np.r_[0:128, 2048:2176, 3968:4096]
    sub = make_problem(D=128, NQ=len(rows), H=32, N=4096, kv_type="q8_0", seed=29)
    sub.q = np.ascontiguousarray(p.q[:, rows])
    sub.k_bytes, sub.v_bytes = p.k_bytes, p.v_bytes
    sub.mask_bits = np.ascontiguousarray(p.mask_bits[rows])
    ref = sub.oracle(n_threads=16)
    assert attn_rel_err(a[:, rows], ref) <= RTOL
    assert attn_elem_err(a[:, rows], ref) <= 1.0


def test_pf_prefill_full_zero_mask_bench_plan(dev):
    """bench.py's prefill line, pinned at its full size: n_q = N = 4096, 32
    heads, Q8_0 K/V, SURVEY §8d's zero mask, auto plan -- one pre-pass launch
    staging the rows to f16 (kv_stage_f16) and flagging the mask blocks (every block flagged +-0, so every
    workgroup runs the lean body's ZM form: no mask DMA, reads or waits)
    and fattn_pf4_kernel(lean).  All 32 heads x three 128-row blocks
    against the oracle, and the whole output against the multi-query kernel."""
    p = make_problem(D=128, NQ=4096, H=32, N=4096, kv_type="q8_0", mask="zero", seed=31)
    assert not p.mask_bits.any() or np.all((p.mask_bits & 0x7FFF) == 0)
    t = upload(p)
    att = fattn.Attention(*views(p, t), t["dst"], p.scale)
    d = att.describe()
    assert d.startswith("pf_prepass[kv_stage_f16<q8_0> + pf_mask_flags] + fattn_pf4_kernel(lean)<f16,D128,mask>"), d
    a = run_gpu(p)
    assert np.isfinite(a).all()
    fattn.set_option(fattn.OPT_PF, 1)
    try:
        b = run_gpu(p)
    finally:
        fattn.set_option(fattn.OPT_PF, 0)
    assert attn_rel_err(a, b) <= RTOL
    rows = np.r_[0:128, 2048:2176, 3968:4096]
    sub = make_problem(D=128, NQ=len(rows), H=32, N=4096, kv_type="q8_0", mask="zero", seed=31)
    sub.q = np.ascontiguousarray(p.q[:, rows])
    sub.k_bytes, sub.v_bytes = p.k_bytes, p.v_bytes
    sub.mask_bits = np.ascontiguousarray(p.mask_bits[rows])
    ref = sub.oracle(n_threads=16)
    assert attn_rel_err(a[:, rows], ref) <= RTOL
    assert attn_elem_err(a[:, rows], ref) <= 1.0


# ------------------------------------------------------------------ sweep

CASES = []
for D in (64, 128):
    for kt in ("f16", "q8_0", "q4_0"):
        for layout in ("head", "pos", "padded"):
            CASES.append(dict(D=D, kv_type=kt, layout=layout, NQ=1, H=4, Hkv=4, N=256, mask="random"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=3, H=8, Hkv=2, N=100, mask="causal"))
        CASES.append(dict(D=D, kv_type=kt, layout="pos", NQ=17, H=4, Hkv=4, N=200, mask="random"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=2, H=6, Hkv=2, N=96, mask="none"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=5, H=32, Hkv=1, N=64, mask="neginf_blocks"))
        CASES.append(dict(D=D, kv_type=kt, layout="pos", NQ=1, H=2, Hkv=2, N=1, mask="random"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=4, H=2, Hkv=2, N=33, mask="random", S=3))
# head_dim 256: split-KV kernel only
for kt in ("f16", "q8_0", "q4_0"):
    for layout in ("head", "pos", "padded"):
        CASES.append(dict(D=256, kv_type=kt, layout=layout, NQ=1, H=4, Hkv=4, N=512, mask="random"))
    CASES.append(dict(D=256, kv_type=kt, layout="head", NQ=9, H=8, Hkv=2, N=300, mask="causal"))
    CASES.append(dict(D=256, kv_type=kt, layout="head", NQ=1, H=2, Hkv=2, N=4096, mask="random"))  # chunk merge


# head_dims 80 (f16 only) and 96 (the reference's mem_copy
# experiment pads 80 -> 128, src/flash-matrix.cu:18-65): split-KV kernel, padded-free rows
# (Q8_0 / Q4_0 rows of D = 96 are 102 / 54 B, not whole dwords: those caches
# need the contiguous [Hkv][N][row] layout and N % 32 == 0 -- test_abi checks
# the rejection of the others)
for D, kts in ((96, ("f16", "q8_0", "q4_0")), (80, ("f16",))):
    for kt in kts:
        f16 = kt == "f16"
        for layout in (("head", "pos") if f16 else ("head",)):
            CASES.append(dict(D=D, kv_type=kt, layout=layout, NQ=1, H=4, Hkv=4, N=256, mask="random"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=1, H=32, Hkv=32, N=4096, mask="random"))  # chunk merge
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=1, H=32, Hkv=8, N=4096, mask="random"))   # GQA tiles
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=9, H=8, Hkv=2, N=300 if f16 else 320, mask="causal"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=64, H=4, Hkv=4, N=1024, mask="random"))
        CASES.append(dict(D=D, kv_type=kt, layout="head", NQ=4, H=2, Hkv=2, N=33 if f16 else 64, mask="random", S=3))
    CASES.append(dict(D=D, kv_type="f16", layout="head", NQ=1, H=4, Hkv=4, N=512, mask="random", v_trans=True))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_sweep(dev, case):
    p = make_problem(seed=zlib.crc32(str(sorted(case.items())).encode()) % 1000, **case)
    got, ref = run_gpu(p), p.oracle()
    assert attn_rel_err(got, ref) <= RTOL


@pytest.mark.parametrize("chunk", [128, 256, 1024, 100000])
def test_chunking_invariance(dev, chunk):
    """Forced split-KV chunk sizes (many partials / single chunk) agree with the oracle."""
    p = make_problem(D=128, NQ=2, H=8, Hkv=4, N=1500, kv_type="q8_0", layout="pos", seed=7)
    assert attn_rel_err(run_gpu(p, kv_chunk=chunk), p.oracle()) <= RTOL


@pytest.mark.parametrize("kt", ["f16", "q8_0", "q4_0"])
def test_extreme_rescale(dev, kt):
    """Large scores force the online-softmax rescale branch (guide rule 26)."""
    p = make_problem(D=128, NQ=4, H=4, N=1024, kv_type=kt, seed=8, extreme=True)
    assert attn_rel_err(run_gpu(p), p.oracle()) <= RTOL


def test_fully_masked_rows_are_nan(dev):
    p = make_problem(D=64, NQ=3, H=2, N=128, kv_type="q8_0", mask="zero", seed=9)
    m = orc.f16_bits_to_f32(p.mask_bits)
    m[1, :] = -np.inf   # row 1 sees nothing -> NaN (src/utils.h:30-49 semantics)
    p.mask_bits = orc.f32_to_f16_bits(m)
    got, ref = run_gpu(p), p.oracle()
    assert np.isnan(ref[:, 1]).all() and np.isnan(got[:, 1]).all()
    assert attn_rel_err(got, ref) <= RTOL


def test_deterministic(dev):
    p = make_problem(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", seed=11)
    a, b = run_gpu(p), run_gpu(p)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ reference entry points

def test_kernel_test_flow(dev):
    """src/kernel_test.h as the reference runs it: srand(1) (glibc default seed),
    random() fill order Q, K, V, mask; GQA 32/8, D=128, kv_size=512; CPU
    reference = kernel_test.h:50-62; GPU = fattn_row with V transposed
    (-DFA_KV_BLOCK_256 layout, kernel_test.h:96-105) and f16 mask."""
    import torch
    D, H, Hkv, N = 128, 32, 8, 512
    orc.srand(1)
    query = orc.random(D * H)
    key = orc.random(D * N * Hkv)
    value = orc.random(D * N * Hkv)
    mask = orc.random(N)
    ref = orc.kernel_test_cpu(query, key, value, mask, N, D, H, Hkv)
    kf16 = orc.f32_to_f16_bits(key)
    vt = orc.f32_to_f16_bits(value.reshape(Hkv, N, D).transpose(0, 2, 1).copy())
    mf16 = orc.f32_to_f16_bits(mask)
    d = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    qkv = torch.empty(H * D, dtype=torch.float32, device=dev)
    fattn.row(d(query), d(kf16), d(vt), d(mf16), qkv, D, N, H, 1.0 / np.sqrt(np.float32(D)), D * N, H // Hkv)
    torch.cuda.synchronize()
    got = qkv.cpu().numpy()
    # the reference's CPU side adds the f32 mask, the GPU the f16 one (as the reference does)
    assert attn_rel_err(got.reshape(H, D), ref.reshape(H, D)) <= RTOL


def test_ext_f16_launch_positional(dev):
    """flash-llama.h:7-32 argument list, as kernel_test.h:191-198 passes it."""
    import torch
    p = make_problem(D=128, NQ=1, H=32, Hkv=8, N=512, kv_type="f16", mask="random", seed=12, mask_pad=512)
    t = upload(p, dev)
    L = fattn.lib()
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    D, N = 128, 512
    mrows = p.mask_bits.shape[0]
    rc = L.fattn_ext_f16_launch(
        t["q"].data_ptr(), t["k"].data_ptr(), t["v"].data_ptr(), t["mask"].data_ptr(), t["dst"].data_ptr(),
        p.scale, D, 1, 32, 1, D, N, 8, 1, mrows, N * 2, D * 4 * 32, D * 4, D * 32 * 4,
        D * 2, D * N * 2, D * N * 8 * 2, D, 32, 1, 1, fattn.TYPE_F16, fattn.TYPE_F16, ws.data_ptr(), ws.numel(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fattn.strerror(rc)
    torch.cuda.synchronize()
    assert attn_rel_err(t["dst"].cpu().numpy(), p.oracle()) <= RTOL


def test_graph_capture(dev):
    """The launch path allocates nothing and does not sync: capturable into a HIP graph."""
    p = make_problem(D=128, NQ=1, H=32, N=4096, kv_type="q8_0", seed=13)
    t = upload(p, dev)
    att = fattn.Attention(*views(p, t), t["dst"], p.scale)
    _, (out,) = graph_replay(att, t["dst"], replays=1)
    assert attn_rel_err(out, p.oracle()) <= RTOL


@pytest.mark.parametrize("hkv", [8, 32], ids=["gqa4-workgroup-merge", "mha-wave-merge"])
def test_chunk_merge_handoff_stress(dev, hkv):
    """The last-arriving workgroup of a tile merges the chunk partials of the
    others (sc1 stores -> drain -> agent atomic add -> sc1 loads).  Stress the
    hand-off the way MI355X_MICROARCH.md asks: one workspace reused across
    plans with different chunk counts (the arrival counters must re-arm to
    zero), a competing copy stream for uneven load, and every output word
    checked on every launch."""
    import torch
    p = make_problem(D=128, NQ=1, H=32, Hkv=hkv, N=4096, kv_type="q8_0", seed=21)
    ref = p.oracle()
    t = upload(p, dev)
    qv, kv, vv, mv = views(p, t)
    ws_bytes = 0
    atts = []
    for chunk in (128, 256, 512, 1024, 0):
        a = fattn.Attention(qv, kv, vv, mv, t["dst"], p.scale, kv_chunk=chunk)
        atts.append(a)
        ws_bytes = max(ws_bytes, a.workspace.numel())
    shared = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    for a in atts:
        a.workspace = shared
        a.p.workspace = shared.data_ptr()
        a.p.workspace_bytes = shared.numel()
    noise_src = torch.randn(1 << 26, device=dev)
    noise_dst = torch.empty_like(noise_src)
    side = torch.cuda.Stream()
    multi = 0
    for it in range(40):
        with torch.cuda.stream(side):
            for _ in range(it % 4):
                noise_dst.copy_(noise_src)
        t["dst"].fill_(float("nan"))
        att = atts[it % len(atts)]
        att()
        torch.cuda.synchronize()
        multi += fattn.workspace_size(att.p) > 0
        got = t["dst"].cpu().numpy()
        assert attn_rel_err(got, ref) <= RTOL, f"iteration {it} (plan {it % len(atts)})"
    assert multi > 0
    # arrival words re-armed: every tile's word (one per 256-B line) counts 0
    # again; the top bits keep the tag and the last launch's epoch
    # (plans whose partials merge in a second launch never touch the words)
    words = shared[: hkv * 256].view(torch.int64)[::32]
    assert int((words & 0xFFFF).abs().sum()) == 0
    assert bool(((((words >> 56) & 0xFF) == 0xFF) | (words == 0)).all())
