"""GPU: what the BF16 KV-cache type has of its own (the cases it shares with the
other oracle-less types run in tests/test_gpu_kv_types.py) -- the conversions
bit-exact against the numpy rule (tests/bf16.py), its GQA and prefill shapes,
the operand split, and the range f16 cannot hold.

In range (K / V = bf16 roundings of U[-1, 1], exact in f16 too): against the
frozen oracle over F16 views of the same values AND against the float64
reference.  Out of f16's range (K x 2^20, V x 2^18 with rows at 1e30, Q x 2^17):
against float64 alone -- no f16 view of those values exists.  Bars: the
project's own, attn_rel_err <= 1e-3 and attn_elem_err <= 1 (tests/problems.py).
Every case prints its figures ("BF16 ...") before it asserts."""
import dataclasses

import numpy as np
import pytest

import bf16
import fattn
import kv_types as kt
from gpu_util import run_described, views as gpu_views
from oracle import oracle as orc
from problems import attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
T = fattn.TYPE_BF16


def _pair(**kw):
    return kt.cached_pair("bf16", **kw)


def _both(tag, desc, got, oracle, f64):
    return kt.check_both("bf16", tag, desc, got, oracle, f64)


# ------------------------------------------------------------------ conversions

def test_quantize_dequantize_bit_exact(dev):
    """fattn_quantize / fattn_dequantize against numpy: 64 x 128 random values,
    the edge values (ties, +-0, subnormals, the largest finite value, overflow to
    inf, +-inf, quiet and signalling NaNs) and a row far outside f16's range."""
    import torch
    x = kt.conv_input(kt.KV_TYPES["bf16"])
    want = bf16.encode_rows(x)
    got = fattn.quantize(torch.from_numpy(x).to(dev), T).cpu().numpy()
    assert got.shape == want.shape == (66, 256)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:8], got[tuple(bad[0])] if len(bad) else None)
    y = fattn.dequantize(torch.from_numpy(want).to(dev), T, 128).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), bf16.bf16_bits_to_f32(want.view("<u2")).view(np.uint32))
    assert np.array_equal(y.view(np.uint32), want.view("<u2").astype(np.uint32) << 16)


def test_set_rows_still_refuses_bf16(dev):
    """The stated gap: fattn_set_rows has no BF16 form."""
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    s = fattn.View(buf.data_ptr(), fattn.TYPE_F32, (32, 2, 1, 1), (4, 128, 256, 256))
    i = fattn.View(idx.data_ptr(), fattn.TYPE_I64, (2, 1, 1, 1), (8, 16, 16, 16))
    d = fattn.View(buf.data_ptr() + 1024, T, (32, 4, 1, 1), (2, 64, 256, 256))
    with pytest.raises(fattn.FattnError) as e:
        fattn.set_rows(s, i, d)
    assert e.value.code == -2


# ------------------------------------------------------------------ attention, in range

@pytest.mark.parametrize("D", [64, 128, 256])
def test_gqa_tile_second_launch_merge(dev, D):
    """GQA 4 x 3 query rows = 12 packed rows per tile, two sequences sharing one
    KV, 4 chunks: the chunk partials (f32) merge in a second launch."""
    gpu, _, oracle, f64 = _pair(D=D, NQ=3, H=8, Hkv=2, N=512, S=2, Skv=1, mask="random", seed=9)
    got, desc = run_described(gpu, dev, kv_chunk=128)
    assert desc.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran16,mask,4waves> + fattn_merge_kernel grid(4,2,2)"), desc
    assert "f16 partials" not in desc, desc
    _both(f"gqa merge_launch D{D}", desc, got, oracle, f64)


def test_gqa_tile_single_chunk(dev):
    gpu, _, oracle, f64 = _pair(D=128, NQ=3, H=8, Hkv=2, N=288, S=2, Skv=1, mask="random", seed=9)
    got, desc = run_described(gpu, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,"), desc
    _both("gqa D128", desc, got, oracle, f64)


def test_prefill_shape_runs_the_split_kernel(dev):
    """NQ = 64 over N = 256, asked for the prefill kernels: BF16 has none (no f16 staging either)."""
    gpu, _, oracle, f64 = _pair(D=128, NQ=64, H=2, N=256, mask="causal", seed=43)
    with fattn.options({fattn.OPT_PF: 2}):
        got, desc = run_described(gpu, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,"), desc
    _both("prefill_shape", desc, got, oracle, f64)


# ------------------------------------------------------------------ the operand split

def test_hi_lo_operands_beat_f16_operands(dev):
    """The in-range one-row D = 128 case through the BF16 kernel and, over F16
    views of the same values, the F16 kernel: the BF16 launch's error against
    float64 is not larger.  Sixteen operand bits (bf16 hi + lo) against f16's
    eleven -- about 3e-6 against 3e-4 in the emulation; one bf16 operand would
    give about 2e-3."""
    gpu, ref, _, f64 = _pair(D=128, NQ=1, H=4, N=544, mask="random", seed=21 + 128)
    got_b, desc_b = run_described(gpu, dev, kv_chunk=128)
    got_h, desc_h = run_described(ref, dev, kv_chunk=128)
    assert desc_h.startswith("fattn_split_kernel<f16,f16,D128,"), desc_h
    eb, eh = attn_rel_err(got_b, f64), attn_rel_err(got_h, f64)
    print(f"BF16 operand_split rel bf16={eb:.3e} f16={eh:.3e} | {desc_b}")
    assert eb <= eh, (eb, eh)


# ------------------------------------------------------------------ range: what f16 cannot hold

def _range_base(**kw):
    base = make_problem(kv_type="f16", layout="head", **kw)
    return base, bf16.cache_values(base.k_f32), bf16.cache_values(base.v_f32)


def _range_check(tag, gpu, dev, kv_chunk, want_desc):
    f64 = bf16.reference_f64(gpu)
    assert np.isfinite(f64).all()
    got, desc = run_described(gpu, dev, kv_chunk=kv_chunk)
    assert desc.startswith(want_desc), desc
    assert "f16 partials" not in desc, desc
    kt.check("bf16", tag, desc, got, f64, "f64")


def test_range_large_k(dev):
    """K = bf16(U[-1, 1]) x 2^20 with scale = 2^-20 / sqrt(D): the f16 encoding of this K is inf."""
    base, k, v = _range_base(D=128, NQ=1, H=4, N=544, mask="random", seed=51)
    k = (k * np.float32(2.0 ** 20)).astype(np.float32)
    h = orc.f16_bits_to_f32(orc.f32_to_f16_bits(k))
    assert np.isinf(h).mean() > 0.9
    gpu = bf16.over_cache(base, k, v, scale=float(np.float32(2.0 ** -20) / np.sqrt(np.float32(128))))
    _range_check("range K*2^20", gpu, dev, 128, "fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>")


def test_range_large_v_second_launch_merge(dev):
    """V = bf16(U[-1, 1]) x 2^18 with a few rows at 1e30, on 8-row GQA tiles over 4
    chunks: the second-launch merge, whose partials must be f32 (an F16 cache takes
    f16 partials on this plan: O / l of these values overflows them)."""
    base, k, v = _range_base(D=128, NQ=1, H=16, Hkv=2, N=1024, mask="random", seed=53)
    v = (v * np.float32(2.0 ** 18)).astype(np.float32)
    v[:, :, [3, 500, 777, 1023], :] = bf16.round_bf16(np.float32([1e30]))[0]
    # (|x| >= 65520 rounds to inf in f16: every |u| >= 2^-2, three values in four)
    assert np.isinf(orc.f16_bits_to_f32(orc.f32_to_f16_bits(v))).mean() > 0.7
    gpu = bf16.over_cache(base, k, v)
    as_f16 = dataclasses.replace(gpu, kv_type=fattn.TYPE_F16, v_type=fattn.TYPE_F16)   # (the plan only: same strides)
    f16_desc = fattn.describe(fattn.ext_params(*gpu_views(as_f16, dict.fromkeys(("q", "k", "v", "mask"), _P())), 1 << 20,
                                               gpu.scale, kv_chunk=256))
    assert "fattn_merge_kernel(f16 partials)" in f16_desc, f16_desc
    _range_check("range V*2^18+1e30 merge_launch", gpu, dev, 256,
                 "fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves> + fattn_merge_kernel grid(4,2,1)")


def test_range_large_q(dev):
    """Q scaled by 2^17 with scale scaled down to match: the f16 rounding of this Q is inf."""
    base, k, v = _range_base(D=128, NQ=1, H=4, N=544, mask="random", seed=55)
    q = (base.q * np.float32(2.0 ** 17)).astype(np.float32)
    assert np.isinf(orc.f16_bits_to_f32(orc.f32_to_f16_bits(q))).mean() > 0.4
    gpu = bf16.over_cache(base, k, v, q=q, scale=float(np.float32(base.scale) * np.float32(2.0 ** -17)))
    _range_check("range Q*2^17", gpu, dev, 128, "fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>")


class _P:
    """A placeholder device tensor for host-only planning (gpu_util.views takes data_ptr())."""

    def data_ptr(self):
        return 1 << 20
