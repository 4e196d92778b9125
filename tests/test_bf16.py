"""CPU: the BF16 KV-cache type (ggml type 30) -- the row size, the plans the
planner picks for it (the split kernel on every shape, f32 chunk partials, the
F16 split plan's grid and workspace), what stays rejected, the numpy rounding
rule (tests/bf16.py) against known answers written out by hand, and the
numerical design: the bf16 hi / lo operand pairs are under the project's 1e-3
bar against float64 where one bf16 operand is over it."""
import functools
import json
import os

import numpy as np
import pytest

import bf16
import fattn
import kv_types as kt
from plans import plan_params as abi_params
from problems import attn_elem_err, attn_rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_kat.json")
BF16, F16 = fattn.TYPE_BF16, fattn.TYPE_F16
# a one-row decode, a 64-row batched shape, a prefill shape
SHAPES = {"decode": dict(), "batched": dict(NQ=64), "prefill": dict(NQ=4096, H=8, Hkv=8, N=4096)}


_params = functools.partial(abi_params, kt=BF16)   # (the BF16 cache of the same shapes)


def test_constants_and_row_size():
    assert BF16 == 30 == bf16.TYPE_BF16 and fattn.TYPE_NAMES["bf16"] == BF16
    for k in (1, 32, 100, 128, 576):
        assert fattn.row_size(BF16, k) == 2 * k


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("D", [64, 128, 256])
def test_every_shape_is_the_split_kernel(D, shape):
    """The bf16 body is the only kernel of the type: no mq / bd / bdp / pf / pf4
    plan, no f16 staging pre-pass, no loader-wave form, no f16 partials -- and
    the grid, LDS and workspace of the F16 split plan with f32 partials."""
    kw = SHAPES[shape]
    d = fattn.describe(_params(D=D, **kw))
    assert d.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran16,mask,"), d
    assert "f16 partials" not in d and "prepass" not in d and "stage" not in d, d
    ws = fattn.workspace_size(_params(D=D, **kw))
    with fattn.options({fattn.OPT_PF: 1, fattn.OPT_BD: 1, fattn.OPT_MQ_DISABLE: 1, fattn.OPT_PART_F16: 1}):
        f = fattn.describe(_params(D=D, kt=F16, **kw))
        assert f.startswith(f"fattn_split_kernel<f16,f16,D{D},"), f
        assert d == f.replace("<f16,f16,", "<bf16,bf16,"), (d, f)
        assert ws == fattn.workspace_size(_params(D=D, kt=F16, **kw))
    assert (ws > 0) == ("grid(1," not in d)
    # whatever the overrides ask for
    for opts in ({fattn.OPT_PF: 2}, {fattn.OPT_BD: 3}, {fattn.OPT_SPLIT_LOADERS: 2}, {fattn.OPT_PART_F16: 2},
                 {fattn.OPT_MQ_MIN_ROWS: 32}):
        with fattn.options(opts):
            d2 = fattn.describe(_params(D=D, **kw))
        assert d2.startswith(f"fattn_split_kernel<bf16,bf16,D{D},") and "f16 partials" not in d2, (opts, d2)


def test_plan_grids():
    assert "8waves> (xcd order) grid(8,32,1)" in fattn.describe(_params())
    assert "4waves> (xcd order) grid(8,32,1)" in fattn.describe(_params(D=256))
    d = fattn.describe(_params(NQ=64))
    assert "+ fattn_merge_kernel grid(4,128,1)" in d, d
    assert "grid(2,2048,1)" in fattn.describe(_params(NQ=4096, H=8, Hkv=8, N=4096))
    # 8-row GQA tiles over 8 chunks: F16 takes f16 partials here, BF16 never
    kw = dict(H=16, Hkv=2, N=2048, kv_chunk=256)
    assert "fattn_merge_kernel(f16 partials)" in fattn.describe(_params(kt=F16, **kw))
    d = fattn.describe(_params(**kw))
    assert d.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves> + fattn_merge_kernel grid(8,2,1)"), d
    # the dword path: V rows padded by 8 bytes (strides no multiples of 16)
    N, rb = 4096, 256 + 8
    d = fattn.describe(_params(v_nb=(2, rb, rb * N, rb * N * 32)))
    assert d.startswith("fattn_split_kernel<bf16,bf16,D128,gran4,mask,4waves>"), d


def test_rejections():
    def status(**kw):
        with pytest.raises(fattn.FattnError) as e:
            fattn.describe(_params(**kw))
        return str(e.value)
    for other in (F16, fattn.TYPE_Q8_0, fattn.TYPE_Q4_0, fattn.TYPE_Q4_1, fattn.TYPE_Q5_0, fattn.TYPE_Q5_1):
        assert "UNSUPPORTED_TYPE" in status(kt=BF16, vt=other)
        assert "UNSUPPORTED_TYPE" in status(kt=other, vt=BF16)
    assert "UNSUPPORTED_HEAD_DIM" in status(D=80)
    assert "UNSUPPORTED_HEAD_DIM" in status(D=96)
    # a transposed V ([D][N]: nb0 = N * 2, nb1 = 2) exists for F16 only
    N = 4096
    tr = (N * 2, 2, 128 * N * 2, 128 * N * 2 * 32)
    assert fattn.describe(_params(kt=F16, v_nb=tr)).startswith("fattn_split_kernel<f16,f16T,")
    assert "BAD_STRIDE" in status(v_nb=tr)
    # the MLA shape has no BF16 form
    assert fattn.describe(_params(D=576, kt=F16, dv=512, H=16, Hkv=1)).startswith("fattn_mla_kernel<f16,")
    assert "UNSUPPORTED_TYPE" in status(D=576, dv=512, H=16, Hkv=1)


def test_existing_types_keep_their_plans():
    assert "fattn_split_kernel<q8_0,q8_0,D128,gran16,mask,8waves>" in fattn.describe(abi_params())
    assert "fattn_split_kernel<f16,f16,D128,gran16,mask,8waves>" in fattn.describe(abi_params(N=2048, kt=F16))
    assert fattn.describe(abi_params(NQ=64)).startswith("fattn_bdp_kernel<q8_0")
    assert "fattn_pf4_kernel(lean)<f16,D128" in fattn.describe(abi_params(NQ=4096, kt=F16))


# ------------------------------------------------------------------ the rounding rule

def test_known_answers():
    kat = json.load(open(GOLDEN))["cases"]
    x = np.array([int(c[0], 16) for c in kat], dtype=np.uint32).view(np.float32)
    got = bf16.f32_to_bf16_bits(x)
    for (src, want, note), g in zip(kat, got):
        assert int(g) == int(want, 16), (src, want, hex(int(g)), note)
    # the file covers what the edge rows of the GPU conversion tests hold
    assert np.array_equal(bf16.edge_values()[:len(kat)].view(np.uint32), x.view(np.uint32))


def test_known_answer_values():
    """A few of them spelled out here too, so that the file cannot drift."""
    f = lambda u: np.array([u], dtype=np.uint32).view(np.float32)
    b = lambda u: int(bf16.f32_to_bf16_bits(f(u))[0])
    assert b(0x3F808000) == 0x3F80 and b(0x3F818000) == 0x3F82          # ties to even, both directions
    assert b(0x7F7FFFFF) == 0x7F80 and b(0x7F7F7FFF) == 0x7F7F          # FLT_MAX -> inf; the largest finite value
    assert b(0x7F800001) == 0x7FC0 and b(0xFF800001) == 0xFFC0          # a signalling NaN stays a NaN
    assert b(0x00018000) == 0x0002 and b(0x80000000) == 0x8000          # subnormals and -0 kept


def test_round_trip_and_nearest():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(20000) * np.exp(rng.uniform(-60, 60, 20000))).astype(np.float32)
    y = bf16.round_bf16(x)
    assert np.array_equal(bf16.round_bf16(y), y)                        # idempotent: bf16 -> f32 is exact
    u = bf16.f32_to_bf16_bits(x).astype(np.int64)
    for nb in (u - 1, u + 1):                                           # no neighbour is nearer
        z = bf16.bf16_bits_to_f32(nb.astype(np.uint16)).astype(np.float64)
        assert np.all(np.abs(y.astype(np.float64) - x) <= np.abs(z - x))
    assert np.array_equal(bf16.encode_rows(x.reshape(-1, 8)).reshape(-1).view("<u2"), u.astype(np.uint16))


# ------------------------------------------------------------------ the numerical design

@pytest.mark.parametrize("D", [64, 128, 256])
def test_hi_lo_operands_are_the_design(D):
    """On the seeds of the GPU one-row cases: the emulated kernel with Q and P as
    bf16 hi / lo pairs is under attn_rel_err 1e-3 (and attn_elem_err 1) against
    float64; with one bf16 per operand, or with Q alone split, it is over."""
    gpu, _ = kt.reference_pair("bf16", D=D, NQ=1, H=4, N=544, mask="random", seed=21 + D)
    ref = bf16.reference_f64(gpu)
    both = bf16.emulate(gpu)
    rel, elem = attn_rel_err(both, ref), attn_elem_err(both, ref)
    print(f"BF16 emulate D{D} hi/lo rel={rel:.3e} elem={elem:.4f}")
    assert rel <= 1e-3 and elem <= 1.0
    assert rel <= 1e-4   # sixteen operand bits: two orders below the bar
    for sq, sp in ((False, False), (True, False)):
        one = attn_rel_err(bf16.emulate(gpu, split_q=sq, split_p=sp), ref)
        print(f"BF16 emulate D{D} split_q={sq} split_p={sp} rel={one:.3e}")
        assert one > 1e-3


def test_cache_values_are_exact_in_f16():
    gpu, ref = kt.reference_pair("bf16", D=64, NQ=1, H=2, N=96, mask="none", seed=1)
    assert np.array_equal(gpu.k_f32, ref.k_f32)
    assert np.array_equal(gpu.k_f32.astype(np.float16).astype(np.float32), gpu.k_f32)
    assert np.array_equal(bf16.bf16_bits_to_f32(gpu.k_bytes.view("<u2")).reshape(gpu.k_f32.shape), gpu.k_f32)
    # ... and the float64 reference agrees with the frozen oracle over the F16 views to f16 operand precision
    assert attn_rel_err(ref.oracle(), bf16.reference_f64(gpu)) <= 1e-3
