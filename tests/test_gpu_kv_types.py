"""GPU: the KV-cache types the frozen oracle does not know -- Q4_1 / Q5_0 / Q5_1
and BF16 (the rows of tests/kv_types.py's KV_TYPES).  The conversions bit-exact
against the numpy restatement, and attention over caches of these types on
every plan they take (the split kernel in each of its forms; for the block
types the staged prefill too) against the frozen oracle given F16 views of the
f16 rounding of what the kernel reads -- and, for BF16, against the float64
reference as well.  Bars: the project's own, attn_rel_err <= 1e-3 and
attn_elem_err <= 1 (tests/problems.py).  Every case prints its figures
("KVT ..." / "BF16 ...") before it asserts.  What only BF16 has (its range, the
operand split, its own GQA and prefill shapes) is in tests/test_gpu_bf16.py."""
import functools

import numpy as np
import pytest

import bf16
import fattn
import kv_types as kt
import mask_planes as mp
import op_params as op
import sinks as sk
import views
from gpu_util import graph_replay, run_described, run_kernel_test, upload, views as gpu_views

pytestmark = pytest.mark.gpu
NAMES = ("q4_1", "q5_0", "q5_1")
ALL = NAMES + ("bf16",)


# ------------------------------------------------------------------ conversions

@pytest.mark.parametrize("name", NAMES)
def test_quantize_dequantize_bit_exact(dev, name):
    """fattn_quantize / fattn_dequantize against numpy: 64 rows x 128 random
    values and the edge blocks (all zero, all equal, a lone +-max at element 0 /
    31, -0.0, a tie for |max|, the known-answer block)."""
    import torch
    typ = kt.TYPES[name]
    x = kt.conv_input(kt.KV_TYPES[name])
    want = kt.quantize(x, typ)
    got = fattn.quantize(torch.from_numpy(x).to(dev), typ).cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, bad[:8], got[tuple(bad[0])] if len(bad) else None)
    y = fattn.dequantize(torch.from_numpy(want).to(dev), typ, 128).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), kt.dequantize(want, typ, 128).view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_known_answer_blocks_on_gpu(dev, name):
    import json
    import os

    import torch
    kat = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kv_types_kat.json")))
    typ = kt.TYPES[name]
    x = kt.kat_input().reshape(1, 32)
    got = fattn.quantize(torch.from_numpy(x).to(dev), typ).cpu().numpy()
    assert got.tobytes().hex() == kat[name]["bytes"]
    y = fattn.dequantize(torch.from_numpy(got).to(dev), typ, 32).cpu().numpy().reshape(32)
    for j, want in kat[name]["y"].items():
        assert y[int(j)] == np.float32(want)
    if kat[name]["exact"]:
        assert np.array_equal(y, x.reshape(32))


@pytest.mark.parametrize("name", ALL)
def test_cpy_into_pos_cache_view(dev, name):
    """fattn_cpy f32 -> the type into a [N][Hkv][row] cache view at position p0:
    the written rows bit-exact with numpy, every other byte untouched."""
    import torch
    t = kt.KV_TYPES[name]
    D, Hkv, N, p0 = 128, 3, 80, 7
    rb = fattn.row_size(t.typ, D)
    x = kt.conv_input(t)                    # 66 rows = 22 tokens x 3 heads
    ntok = len(x) // Hkv
    cur = x.reshape(ntok, Hkv, D)
    rng = np.random.default_rng(3)
    cache0 = rng.integers(0, 256, size=N * Hkv * rb, dtype=np.uint8)
    cache = torch.from_numpy(cache0.copy()).to(dev)
    src = torch.from_numpy(np.ascontiguousarray(cur)).to(dev)
    sv = fattn.View(src.data_ptr(), fattn.TYPE_F32, (D, Hkv, ntok, 1), (4, D * 4, Hkv * D * 4, ntok * Hkv * D * 4))
    dv = fattn.View(cache.data_ptr() + p0 * Hkv * rb, t.typ, (D, Hkv, ntok, 1), (t.eb, rb, Hkv * rb, N * Hkv * rb))
    fattn.cpy(sv, dv)
    torch.cuda.synchronize()
    want = cache0.copy().reshape(N, Hkv, rb)
    want[p0:p0 + ntok] = t.encode(cur)
    assert np.array_equal(cache.cpu().numpy().reshape(N, Hkv, rb), want)


# ------------------------------------------------------------------ attention: the split kernel

@pytest.mark.parametrize("mask", ["none", "random", "tail"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("name", ALL)
def test_one_row_decode(dev, name, D, mask):
    """One-row tiles over 5 chunks of 128 (the last one 32 positions: uneven
    wave slices, waves without a step), the per-wave (D = 128) and the
    per-workgroup row merge; "tail": whole chunks -inf."""
    gpu, _, oracle, f64 = kt.cached_pair(name, D=D, NQ=1, H=4, N=544, mask=mask, seed=21 + D)
    got, desc = run_described(gpu, dev, kv_chunk=128)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D{D},gran16,{'nomask' if mask == 'none' else 'mask'},4waves>"), desc
    assert "grid(5,4,1)" in desc, desc
    kt.check_both(name, f"one_row D{D} {mask}", desc, got, oracle, f64)


@pytest.mark.parametrize("layout,N", [("pos", 77), ("padded", 96)])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("name", ALL)
def test_ragged_dword_path(dev, name, D, layout, N):
    """The dword-granular path: a [N][Hkv][row] cache with N = 77 (a partial last
    step) and padded rows at N = 96."""
    gpu, _, oracle, f64 = kt.cached_pair(name, layout=layout, D=D, NQ=1, H=4, N=N, mask="random", seed=5 + N)
    got, desc = run_described(gpu, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D{D},gran4,mask,4waves>"), desc
    kt.check_both(name, f"{layout} D{D} N{N}", desc, got, oracle, f64)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("name", NAMES)
def test_gqa_multi_row_tile(dev, name, D):
    """GQA 4 x 3 query rows = 12 packed rows per tile, two sequences sharing one KV."""
    gpu, _, oracle, _ = kt.cached_pair(name, D=D, NQ=3, H=8, Hkv=2, N=288, S=2, Skv=1, mask="random", seed=9)
    got, desc = run_described(gpu, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D{D},gran16,mask,"), desc
    kt.check(name, f"gqa D{D}", desc, got, oracle)


@pytest.mark.parametrize("waves", [0, 8])
@pytest.mark.parametrize("name", NAMES)
def test_second_launch_merge(dev, name, waves):
    """8 chunks of 4-row tiles: the chunk partials merge in a second launch; with
    8 waves per workgroup too (FATTN_OPT_SPLIT_WAVES)."""
    gpu, _, oracle, _ = kt.cached_pair(name, D=128, NQ=1, H=8, Hkv=2, N=2048, mask="random", seed=13)
    with fattn.options({fattn.OPT_SPLIT_WAVES: waves}):
        got, desc = run_described(gpu, dev, kv_chunk=256)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D128,gran16,mask,{waves or 4}waves> + fattn_merge_kernel"), desc
    assert "grid(8,2,1)" in desc, desc
    kt.check(name, f"merge_launch {waves or 4}w", desc, got, oracle)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ALL)
def test_one_row_eight_waves(dev, name, D):
    """The planner's 8-wave form of one-row tiles (the decode configurations'
    plan in small): workgroup row merge, then the last-arriving workgroup's
    merge of the chunks."""
    gpu, _, oracle, f64 = kt.cached_pair(name, D=D, NQ=1, H=4, N=1024, mask="random", seed=17)
    with fattn.options({fattn.OPT_SPLIT_WAVES: 8}):
        got, desc = run_described(gpu, dev, kv_chunk=256)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D{D},gran16,mask,8waves>"), desc
    assert "grid(4,4,1)" in desc, desc
    kt.check_both(name, f"one_row 8w D{D}", desc, got, oracle, f64)


@functools.lru_cache(maxsize=None)
def _op_case(name):
    return kt.reference_pair(name, D=128, NQ=2, H=4, Hkv=2, N=544, mask="none", seed=31)


def _run_view(vp_gpu, dev, kv_chunk=128, sinks=None):
    gv = views.GpuView(vp_gpu, dev, kv_chunk, sinks=sinks)
    desc = gv.describe()
    got = gv.run()
    assert gv.guards_intact(), desc
    return got, desc


@pytest.mark.parametrize("name", ALL)
def test_logit_softcap(dev, name):
    gpu, ref = _op_case(name)
    o = op.one_plane(ref, op.random_mask(2, 544, 1), logit_softcap=12.0)
    og = views.swap_kv(o, gpu)
    got, desc = _run_view(og, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D128,gran16,mask,4waves>") and "softcap 12" in desc, desc
    kt.check_both(name, "softcap", desc, got, op.reference(o), lambda: bf16.reference_f64(og))


@pytest.mark.parametrize("name", ALL)
def test_max_bias_with_mask(dev, name):
    gpu, ref = _op_case(name)
    o = op.one_plane(ref, op.distance_mask(2, 544) / np.float32(64.0), max_bias=8.0)
    og = views.swap_kv(o, gpu)
    got, desc = _run_view(og, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D128,gran16,mask,4waves>") and "alibi 8" in desc, desc
    kt.check_both(name, "alibi", desc, got, op.reference(o), lambda: bf16.reference_f64(og))


@pytest.mark.parametrize("name", ALL)
def test_sinks(dev, name):
    gpu, ref = _op_case(name)
    o = sk.with_sinks(op.one_plane(ref, op.random_mask(2, 544, 2)), np.array([0.5, -1.0, 2.0, -np.inf], dtype=np.float32))
    og = views.swap_kv(o, gpu)
    got, desc = _run_view(og, dev, sinks=o.sinks)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D128,gran16,mask,4waves>"), desc
    kt.check_both(name, "sinks", desc, got, sk.reference(o), lambda: bf16.reference_f64(og, sinks=o.sinks))


@pytest.mark.parametrize("name", ALL)
def test_per_head_mask_planes(dev, name):
    gpu, ref = _op_case(name)
    pp = mp.add_planes(ref, ne2=4, ne3=1)
    pg = views.swap_kv(pp, gpu)
    got, desc = _run_view(pg, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D128,gran16,mask,4waves>") and "mask planes (4,1)" in desc, desc
    kt.check_both(name, "head_planes", desc, got, pp.oracle(), lambda: bf16.reference_f64(pg))


# ------------------------------------------------------------------ attention: prefill through the staging

@pytest.mark.parametrize("mask", ["causal", "zero"])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("name", NAMES)
def test_prefill_staged(dev, name, D, mask):
    """FATTN_OPT_PF = 2: the cache's rows staged to f16 by the pre-pass, then the
    f16 prefill bodies (D = 128: the one-wave-per-SIMD body, D = 64: the 8-wave one)."""
    gpu, _, oracle, _ = kt.cached_pair(name, D=D, NQ=256, H=2, N=192, mask=mask, seed=41)
    with fattn.options({fattn.OPT_PF: 2}):
        got, desc = run_described(gpu, dev)
    assert f"kv_stage_f16<{name}>" in desc, desc
    assert ("fattn_pf4_kernel(lean)<f16,D128" if D == 128 else "fattn_pf_kernel<f16,D64") in desc, desc
    kt.check(name, f"prefill D{D} {mask}", desc, got, oracle)


@pytest.mark.parametrize("name", NAMES)
def test_prefill_shape_d256_runs_the_split_kernel(dev, name):
    gpu, _, oracle, _ = kt.cached_pair(name, D=256, NQ=64, H=2, N=192, mask="causal", seed=43)
    with fattn.options({fattn.OPT_PF: 2}):
        got, desc = run_described(gpu, dev)
    assert desc.startswith(f"fattn_split_kernel<{name},{name},D256,"), desc
    kt.check(name, "prefill_shape D256", desc, got, oracle)


# ------------------------------------------------------------------ graph capture

@pytest.mark.parametrize("name", ALL)
def test_graph_replay_bits(dev, name):
    """A captured launch (several chunks: arrival words in the workspace) replayed
    twice on the same workspace: the same bits as the eager launch, both times."""
    gpu, _, oracle, f64 = kt.cached_pair(name, D=128, NQ=1, H=4, N=544, mask="random", seed=21 + 128)
    t = upload(gpu, dev)
    att = fattn.Attention(*gpu_views(gpu, t), t["dst"], gpu.scale, kv_chunk=128)
    assert "grid(5,4,1)" in att.describe(), att.describe()
    eager, outs = graph_replay(att, t["dst"])
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), eager.view(np.uint32))
    kt.check_both(name, "graph", att.describe(), outs[1], oracle, f64)


# ------------------------------------------------------------------ the kernel_test harness

@pytest.mark.parametrize("name", ALL)
def test_harness_kv_type(dev, name):
    """kernel_test --kv-type q4_1|q5_0|q5_1|bf16: the cache quantised on the GPU
    (BF16: written by fattn_cpy), its CPU reference over K / V decoded from the
    cache in plain C++ on the host, its own max-diff check."""
    r = run_kernel_test(["--iters", "3", "--no-kv-parallel", "--kv-type", name])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
