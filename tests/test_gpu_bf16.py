"""GPU: the BF16 KV-cache type -- the conversions bit-exact against the numpy
rule (tests/bf16.py), and attention over BF16 caches on every form of the split
kernel it takes.

In range (K / V = bf16 roundings of U[-1, 1], exact in f16 too): against the
frozen oracle over F16 views of the same values AND against the float64
reference.  Out of f16's range (K x 2^20, V x 2^18 with rows at 1e30, Q x 2^17):
against float64 alone -- no f16 view of those values exists.  Bars: the
project's own, attn_rel_err <= 1e-3 and attn_elem_err <= 1 (tests/problems.py).
Every case prints its figures ("BF16 ...") before it asserts."""
import dataclasses
import functools

import numpy as np
import pytest

import bf16
import fattn
import mask_planes as mp
import op_params as op
import sinks as sk
import views
from gpu_util import upload, views as gpu_views
from oracle import oracle as orc
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-3
T = fattn.TYPE_BF16


def _check(tag, desc, got, ref, what):
    rel, elem = attn_rel_err(got, ref), attn_elem_err(got, ref)
    print(f"BF16 {tag} vs {what} rel={rel:.3e} elem={elem:.4f} | {desc}")
    assert rel <= RTOL, (what, rel, desc)
    assert elem <= 1.0, (what, elem, desc)
    return rel


@functools.lru_cache(maxsize=None)
def _pair(layout="head", **kw):
    """(gpu problem, F16 problem, oracle output, float64 output), computed once per shape."""
    gpu, ref = bf16.reference_pair(layout=layout, **kw)
    return gpu, ref, ref.oracle(), bf16.reference_f64(gpu)


def _run(gpu, dev, kv_chunk=0):
    import torch
    t = upload(gpu, dev)
    att = fattn.Attention(*gpu_views(gpu, t), t["dst"], gpu.scale, kv_chunk=kv_chunk)
    desc = att.describe()
    att()
    torch.cuda.synchronize()
    return t["dst"].cpu().numpy(), desc


def _both(tag, desc, got, oracle, f64):
    _check(tag, desc, got, oracle, "oracle(f16 views)")
    return _check(tag, desc, got, f64, "f64")


# ------------------------------------------------------------------ conversions

def _conv_input():
    rng = np.random.default_rng(11)
    x = (3.0 * (1.0 - 2.0 * rng.random((64, 128), dtype=np.float32))).astype(np.float32)
    scaled = (x[:1] * np.float32(2.0 ** 100)).astype(np.float32)          # far outside f16's range
    return np.concatenate([x, bf16.edge_values().reshape(1, 128), scaled], axis=0)   # 66 rows


def test_quantize_dequantize_bit_exact(dev):
    """fattn_quantize / fattn_dequantize against numpy: 64 x 128 random values,
    the edge values (ties, +-0, subnormals, the largest finite value, overflow to
    inf, +-inf, quiet and signalling NaNs) and a row far outside f16's range."""
    import torch
    x = _conv_input()
    want = bf16.encode_rows(x)
    got = fattn.quantize(torch.from_numpy(x).to(dev), T).cpu().numpy()
    assert got.shape == want.shape == (66, 256)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:8], got[tuple(bad[0])] if len(bad) else None)
    y = fattn.dequantize(torch.from_numpy(want).to(dev), T, 128).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), bf16.bf16_bits_to_f32(want.view("<u2")).view(np.uint32))
    assert np.array_equal(y.view(np.uint32), want.view("<u2").astype(np.uint32) << 16)


def test_cpy_into_pos_cache_view(dev):
    """fattn_cpy f32 -> BF16 into a [N][Hkv][row] cache view at position p0: the
    written rows bit-exact with numpy, every other byte untouched."""
    import torch
    D, Hkv, N, p0 = 128, 3, 80, 7
    rb = fattn.row_size(T, D)
    x = _conv_input()                       # 66 rows = 22 tokens x 3 heads
    ntok = len(x) // Hkv
    cur = x.reshape(ntok, Hkv, D)
    rng = np.random.default_rng(3)
    cache0 = rng.integers(0, 256, size=N * Hkv * rb, dtype=np.uint8)
    cache = torch.from_numpy(cache0.copy()).to(dev)
    src = torch.from_numpy(np.ascontiguousarray(cur)).to(dev)
    sv = fattn.View(src.data_ptr(), fattn.TYPE_F32, (D, Hkv, ntok, 1), (4, D * 4, Hkv * D * 4, ntok * Hkv * D * 4))
    dv = fattn.View(cache.data_ptr() + p0 * Hkv * rb, T, (D, Hkv, ntok, 1), (2, rb, Hkv * rb, N * Hkv * rb))
    fattn.cpy(sv, dv)
    torch.cuda.synchronize()
    want = cache0.copy().reshape(N, Hkv, rb)
    want[p0:p0 + ntok] = bf16.encode_rows(cur)
    assert np.array_equal(cache.cpu().numpy().reshape(N, Hkv, rb), want)


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

@pytest.mark.parametrize("mask", ["none", "random", "tail"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_one_row_decode(dev, D, mask):
    """One-row tiles over 5 chunks of 128 (the last one 32 positions: uneven wave
    slices, waves without a step), the per-wave (D = 128) and the per-workgroup
    row merge; "tail": whole chunks -inf."""
    gpu, _, oracle, f64 = _pair(D=D, NQ=1, H=4, N=544, mask=mask, seed=21 + D)
    got, desc = _run(gpu, dev, kv_chunk=128)
    assert desc.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran16,{'nomask' if mask == 'none' else 'mask'},4waves>"), desc
    assert "grid(5,4,1)" in desc, desc
    _both(f"one_row D{D} {mask}", desc, got, oracle, f64)


@pytest.mark.parametrize("layout,N", [("pos", 77), ("padded", 96)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_ragged_dword_path(dev, D, layout, N):
    """The dword-granular path: a [N][Hkv][row] cache with N = 77 (a partial last
    step) and padded rows at N = 96."""
    gpu, _, oracle, f64 = _pair(layout=layout, D=D, NQ=1, H=4, N=N, mask="random", seed=5 + N)
    got, desc = _run(gpu, dev)
    assert desc.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran4,mask,4waves>"), desc
    _both(f"{layout} D{D} N{N}", desc, got, oracle, f64)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_gqa_tile_second_launch_merge(dev, D):
    """GQA 4 x 3 query rows = 12 packed rows per tile, two sequences sharing one
    KV, 4 chunks: the chunk partials (f32) merge in a second launch."""
    gpu, _, oracle, f64 = _pair(D=D, NQ=3, H=8, Hkv=2, N=512, S=2, Skv=1, mask="random", seed=9)
    got, desc = _run(gpu, dev, kv_chunk=128)
    assert desc.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran16,mask,4waves> + fattn_merge_kernel grid(4,2,2)"), desc
    assert "f16 partials" not in desc, desc
    _both(f"gqa merge_launch D{D}", desc, got, oracle, f64)


def test_gqa_tile_single_chunk(dev):
    gpu, _, oracle, f64 = _pair(D=128, NQ=3, H=8, Hkv=2, N=288, S=2, Skv=1, mask="random", seed=9)
    got, desc = _run(gpu, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,"), desc
    _both("gqa D128", desc, got, oracle, f64)


@pytest.mark.parametrize("D", [64, 128])
def test_one_row_eight_waves(dev, D):
    """The planner's 8-wave form of one-row tiles (the config-2 plan in small):
    workgroup row merge, then the last-arriving workgroup's merge of the chunks."""
    gpu, _, oracle, f64 = _pair(D=D, NQ=1, H=4, N=1024, mask="random", seed=17)
    with fattn.options({fattn.OPT_SPLIT_WAVES: 8}):
        got, desc = _run(gpu, dev, kv_chunk=256)
    assert desc.startswith(f"fattn_split_kernel<bf16,bf16,D{D},gran16,mask,8waves>"), desc
    assert "grid(4,4,1)" in desc, desc
    _both(f"one_row 8w D{D}", desc, got, oracle, f64)


@functools.lru_cache(maxsize=None)
def _op_case():
    return bf16.reference_pair(D=128, NQ=2, H=4, Hkv=2, N=544, mask="none", seed=31)


def _run_view(vp_gpu, dev, kv_chunk=128, cls=views.GpuView):
    gv = cls(vp_gpu, dev, kv_chunk=kv_chunk)
    desc = gv.describe()
    got = gv.run()
    assert gv.guards_intact(), desc
    return got, desc


def test_logit_softcap(dev):
    gpu, ref = _op_case()
    o = op.one_plane(ref, op.random_mask(2, 544, 1), logit_softcap=12.0)
    og = bf16.swap_kv(o, gpu)
    got, desc = _run_view(og, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>") and "softcap 12" in desc, desc
    _both("softcap", desc, got, op.reference(o), bf16.reference_f64(og))


def test_max_bias_with_mask(dev):
    gpu, ref = _op_case()
    o = op.one_plane(ref, op.distance_mask(2, 544) / np.float32(64.0), max_bias=8.0)
    og = bf16.swap_kv(o, gpu)
    got, desc = _run_view(og, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>") and "alibi 8" in desc, desc
    _both("alibi", desc, got, op.reference(o), bf16.reference_f64(og))


def test_sinks(dev):
    gpu, ref = _op_case()
    o = sk.with_sinks(op.one_plane(ref, op.random_mask(2, 544, 2)), np.array([0.5, -1.0, 2.0, -np.inf], dtype=np.float32))
    og = bf16.swap_kv(o, gpu)
    got, desc = _run_view(og, dev, cls=sk.SinkGpuView)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>"), desc
    _both("sinks", desc, got, sk.reference(o), bf16.reference_f64(og, sinks=o.sinks))


def test_per_head_mask_planes(dev):
    gpu, ref = _op_case()
    pp = mp.add_planes(ref, ne2=4, ne3=1)
    pg = bf16.swap_kv(pp, gpu)
    got, desc = _run_view(pg, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,4waves>") and "mask planes (4,1)" in desc, desc
    _both("head_planes", desc, got, pp.oracle(), bf16.reference_f64(pg))


def test_prefill_shape_runs_the_split_kernel(dev):
    """NQ = 64 over N = 256, asked for the prefill kernels: BF16 has none (no f16 staging either)."""
    gpu, _, oracle, f64 = _pair(D=128, NQ=64, H=2, N=256, mask="causal", seed=43)
    with fattn.options({fattn.OPT_PF: 2}):
        got, desc = _run(gpu, dev)
    assert desc.startswith("fattn_split_kernel<bf16,bf16,D128,gran16,mask,"), desc
    _both("prefill_shape", desc, got, oracle, f64)


def test_graph_replay_bits(dev):
    """A captured launch (several chunks: arrival words in the workspace) replayed
    twice on the same workspace: the same bits as the eager launch, both times."""
    import torch
    gpu, _, oracle, f64 = _pair(D=128, NQ=1, H=4, N=544, mask="random", seed=21 + 128)
    t = upload(gpu, dev)
    att = fattn.Attention(*gpu_views(gpu, t), t["dst"], gpu.scale, kv_chunk=128)
    assert "grid(5,4,1)" in att.describe(), att.describe()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        att(s.cuda_stream)
    torch.cuda.synchronize()
    eager = t["dst"].cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        att(s.cuda_stream)
    outs = []
    for _ in range(2):
        t["dst"].fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        outs.append(t["dst"].cpu().numpy().copy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), eager.view(np.uint32))
    _both("graph", att.describe(), outs[1], oracle, f64)


def test_harness_kv_type(dev):
    """kernel_test --kv-type bf16: the cache written by fattn_cpy, its CPU
    reference over the bf16-rounded values, its own max-diff check."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ggml-cuda-experiments_amd", "bin", "kernel_test")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (make harness)")
    r = subprocess.run([exe, "--iters", "3", "--no-kv-parallel", "--kv-type", "bf16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


# ------------------------------------------------------------------ the operand split

def test_hi_lo_operands_beat_f16_operands(dev):
    """The in-range one-row D = 128 case through the BF16 kernel and, over F16
    views of the same values, the F16 kernel: the BF16 launch's error against
    float64 is not larger.  Sixteen operand bits (bf16 hi + lo) against f16's
    eleven -- about 3e-6 against 3e-4 in the emulation; one bf16 operand would
    give about 2e-3."""
    gpu, ref, _, f64 = _pair(D=128, NQ=1, H=4, N=544, mask="random", seed=21 + 128)
    got_b, desc_b = _run(gpu, dev, kv_chunk=128)
    got_h, desc_h = _run(ref, dev, kv_chunk=128)
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
    got, desc = _run(gpu, dev, kv_chunk=kv_chunk)
    assert desc.startswith(want_desc), desc
    assert "f16 partials" not in desc, desc
    _check(tag, desc, got, f64, "f64")


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
