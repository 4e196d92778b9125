"""MLA attention over a Q8_0 / Q4_0 cache (V a view of K; include/fattn.h) on
the GPU.  Two checks per case, over the WHOLE dst allocation with the sentinel
bands around it and the workspace tail intact:

  (a) attn_rel_err <= 1e-3 and attn_elem_err <= 1 against tests/mla.py's
      padded-V reference over the logical K = h(dequantize(blocks)), NaN
      positions coinciding -- the project's bars;
  (b) BIT-EQUALITY with the f16 MLA launch over an f16 cache holding the logical
      K, at the same shape, mask, scalars, sinks and kv_chunk: the conversion
      pass writes the very image the f16 form loads, and size_mla cuts both
      caches into the same chunks.

Every case prints its figures (`MLAQ_ERR <type> <case> rel=... elem=...`)
before it asserts.  Every byte outside the logical cache rows is 0x7e poison.
Shapes are (H, Hkv, n_q, N, S / Skv), the ones of tests/test_gpu_mla.py: each
the smallest that reaches its path.  The kernel has three forms and check()
asserts which one a case runs: all four waves load, convert and compute (more
than 16 rows a tile: rows5, prefill, H = 128); "solo", wave 0 computing and
waves 1 - 3 loading dword pieces (16 rows a tile over padded rows, [N][Hkv][row]
or a base at +4); and solo with whole tiles in 16-B pieces (contiguous rows, 16-B
aligned base: the decode and chunked cases, whose N = 173 / 416 also run the
dword pieces of a part-filled last tile).
"""
import numpy as np
import pytest

import mla
import mla_quant as mq
import op_params as op
from gpu_util import WS_TAIL_BYTES, graph_replay, run_kernel_test
from mla import DK, Shape
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu

RTOL = 1e-3
TYPS = ("q8_0", "q4_0")

CHUNKED = Shape(16, 1, 1, 416)       # kv_chunk = 128: 4 chunks, the last of one tile
ROWS5 = Shape(16, 1, 5, 224)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def check(c, ref, tag, dev, plan="", kv_chunk=0, layout="head", base=0, f16_layout=None):
    """(a) and (b) of one case; returns the quantised launch's dst."""
    g = mq.QGpu(c, "quant", layout, base, kv_chunk=kv_chunk, dev=dev)
    d = g.describe()
    # the kernel's forms: 16 rows a tile at most -> (solo), and with contiguous rows on an aligned base 16-B tiles
    sh = c.shape
    solo = min(sh.NQ, 64 // min(sh.H // sh.Hkv, 64)) * min(sh.H // sh.Hkv, 64) <= 16
    word = "" if not solo else " (solo, 16-B tiles)" if layout == "head" and base == 0 else " (solo)"
    assert d.split(">", 1)[1].startswith(word + (" grid" if "xcd" not in d and "merge" not in d else "")), d
    assert ("solo" in d) == solo, d
    b = c.v_off // 32 * mq.BLOCK[c.typ]
    assert f"fattn_mla_kernel<{c.typ},DK576,DV512," in d and f"v=k+{b}>" in d and plan in d, d
    got = g.run()
    rel, el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    print(f"MLAQ_ERR {c.typ} v=k+{b} {tag} rel={rel:.3e} elem={el:.3f} [{d}]")
    assert g.guards_intact(), "dst guard bands or workspace tail overwritten"
    assert rel <= RTOL, (tag, rel)
    assert el <= 1.0, (tag, el)
    f = mq.QGpu(c, "f16", f16_layout or ("pos" if layout == "pos" else "head"), kv_chunk=kv_chunk, dev=dev)
    df = f.describe()
    assert "fattn_mla_kernel<f16," in df and f"v=k+{2 * c.v_off}>" in df, df
    dq = d.replace(" (solo, 16-B tiles)", "").replace(" (solo)", "")
    assert df.split("> ", 1)[1].split(" lds ")[0] == dq.split("> ", 1)[1].split(" lds ")[0], (d, df)    # the same grid
    assert f.ws_bytes == g.ws_bytes
    want = f.run()
    assert f.guards_intact()
    assert np.array_equal(bits(got), bits(want)), (tag, int((bits(got) != bits(want)).sum()), "words differ from the f16 launch")
    return got


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("N,mask", [(160, "none"), (160, "random"), (160, "tail"), (173, "none"), (173, "random"), (173, "tail")])
def test_one_row_decode(dev, typ, N, mask):
    c, ref = mq.cached(Shape(16, 1, 1, N), typ, mask)
    check(c, ref, f"decode-N{N}-{mask}", dev, "grid(1,1,1)")


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("v_off", [0, 32])
def test_v_zero_and_one_block_in(dev, typ, v_off):
    c, ref = mq.cached(Shape(16, 1, 1, 173), typ, "random", v_off)
    check(c, ref, f"decode-N173-b{v_off // 32}", dev, "grid(1,1,1)")
    c, ref = mq.cached(ROWS5, typ, "random", v_off)
    check(c, ref, f"rows5-b{v_off // 32}", dev, "grid(1,2,1)")


@pytest.mark.parametrize("typ", TYPS)
def test_several_chunks_short_last(dev, typ):
    c, ref = mq.cached(CHUNKED, typ, "random")
    check(c, ref, "chunked-416", dev, "+ fattn_mla_merge_kernel grid(4,1,1)", kv_chunk=128)


@pytest.mark.parametrize("typ", TYPS)
def test_two_row_tiles_per_kv_head_shared_kv(dev, typ):
    c, ref = mq.cached(Shape(128, 1, 1, 160, 2, 1), typ, "random")
    check(c, ref, "h128-skv1", dev, ",2,2)")


@pytest.mark.parametrize("typ", TYPS)
def test_two_row_tiles_paired_on_one_xcd(dev, typ):
    c, ref = mq.cached(Shape(128, 1, 1, 256, 4, 4), typ, "random")
    check(c, ref, "h128-xcd", dev, "(xcd order) + fattn_mla_merge_kernel grid(2,2,4)")


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("layout,base", [("head", 0), ("pos", 0), ("pad20", 0), ("pad16", 0), ("head", 4)],
                         ids=["head", "pos", "pad20", "pad16", "base4"])
def test_layouts(dev, typ, layout, base):
    """[Hkv][N][row]; [N][Hkv][row] (Q8_0: a 1224-B stride); rows padded by 20 B
    and by 16 B (strides that are no multiple of 16); a cache base at +4 B."""
    sh = Shape(32, 2, 1, 192, 4, 2)
    c, ref = mq.cached(sh, typ, "random")
    g = check(c, ref, f"hkv2-{layout}-base{base}", dev, "grid(1,2,4)", layout=layout, base=base)
    assert not np.isnan(g).any()


@pytest.mark.parametrize("typ", TYPS)
def test_a_mask_row_per_query_row(dev, typ):
    c, ref = mq.cached(ROWS5, typ, "random")
    check(c, ref, "rows5", dev, "grid(1,2,1)")


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("mask", ["causal", "zero"])
def test_prefill_sized(dev, typ, mask):
    c, ref = mq.cached(Shape(16, 1, 96, 128), typ, mask)
    check(c, ref, f"prefill-{mask}", dev, "grid(1,24,1)")


def _planes(ne3, ne2, NQ, N):
    return np.stack([np.stack([mla.mask_random(NQ, N, 31 * i3 + i2) for i2 in range(ne2)]) for i3 in range(ne3)])


def _op_case(typ, which, what):
    sh = CHUNKED if which == "chunked" else ROWS5
    if what == "softcap":
        return mq.make_case(sh, typ, "random", logit_softcap=7.5)
    if what == "alibi":
        return mq.make_case(sh, typ, planes=op.distance_mask(sh.NQ, sh.N)[None, None], max_bias=8.0)
    if what == "sinks":
        s = np.random.default_rng(77).uniform(-2.0, 4.0, sh.H).astype(np.float32)
        s[3] = -np.inf
        return mq.make_case(sh, typ, "random", sinks=s)
    if what == "head-planes":
        return mq.make_case(sh, typ, planes=_planes(1, sh.H, sh.NQ, sh.N), ne2=sh.H)
    sh2 = Shape(sh.H, 1, sh.NQ, sh.N, 2, 2)
    return mq.make_case(sh2, typ, planes=_planes(2, 1, sh.NQ, sh.N), ne3=2)


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("what", ["softcap", "alibi", "sinks", "head-planes", "seq-planes"])
@pytest.mark.parametrize("which", ["chunked", "rows5"])
def test_scalars_and_planes(dev, typ, which, what):
    c = _op_case(typ, which, what)
    check(c, c.reference(), f"{which}-{what}", dev, "grid(4,1," if which == "chunked" else "", kv_chunk=128 if which == "chunked" else 0)


@pytest.mark.parametrize("typ", TYPS)
def test_fully_masked_row(dev, typ):
    """Row 2's mask is -inf everywhere: NaN without sinks, zeros with sinks."""
    m = mla.mask_random(ROWS5.NQ, ROWS5.N, 5)
    m[2, :] = -np.inf
    c = mq.make_case(ROWS5, typ, planes=m[None, None])
    ref = c.reference()
    assert np.isnan(ref[0, 2]).all() and not np.isnan(ref[0, [0, 1, 3, 4]]).any()
    got = check(c, ref, "masked-row", dev)
    assert np.isnan(got[0, 2]).all() and not np.isnan(got[0, [0, 1, 3, 4]]).any()
    cs = mq.make_case(ROWS5, typ, planes=m[None, None], sinks=np.linspace(-1.0, 2.0, ROWS5.H).astype(np.float32))
    refs = cs.reference()
    assert (refs[0, 2] == 0).all()
    gots = check(cs, refs, "masked-row-sinks", dev)
    assert (gots[0, 2] == 0).all()


@pytest.mark.parametrize("typ", TYPS)
def test_shared_workspace_after_d128_decode(dev, typ):
    """One workspace filled with 0xFF, initialised with fattn_workspace_init, then
    a D = 128 split decode and the MLA decode ordered on it."""
    import torch

    import fattn
    import views
    p128 = make_problem(D=128, NQ=1, H=8, N=1024, kv_type="q8_0", seed=3)
    g128 = views.GpuView(views.make_view(p128), dev)
    c, ref = mq.cached(CHUNKED, typ, "random")
    probe = mq.QGpu(c, kv_chunk=128, dev=dev)
    assert g128.ws_bytes > 0 and probe.ws_bytes > 0
    n = max(g128.ws_bytes, probe.ws_bytes)
    ws = torch.full(((n + 3) // 4 + WS_TAIL_BYTES // 4,), -1, dtype=torch.int32, device=dev)   # 0xFF bytes
    assert fattn.lib().fattn_workspace_init(ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
    g128.p.workspace, g128.p.workspace_bytes = ws.data_ptr(), n
    g = mq.QGpu(c, kv_chunk=128, dev=dev, ws=ws)
    got128 = g128.run()
    got = g.run()
    assert attn_rel_err(got128, p128.oracle()) <= RTOL
    rel, el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    print(f"MLAQ_ERR {typ} v=k+{2 * mq.BLOCK[typ]} shared-ws rel={rel:.3e} elem={el:.3f}")
    assert rel <= RTOL and el <= 1.0
    assert np.array_equal(bits(got), bits(mq.QGpu(c, "f16", kv_chunk=128, dev=dev).run()))
    assert (ws.view(torch.uint8)[n:].cpu().numpy() == 0xFF).all()


@pytest.mark.parametrize("typ", TYPS)
def test_graph_capture_replays_identically(dev, typ):
    c, ref = mq.cached(CHUNKED, typ, "random")
    g = mq.QGpu(c, kv_chunk=128, dev=dev)
    _, outs = graph_replay(g.launch, g.dst)
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    assert attn_rel_err(outs[0].reshape(ref.shape), ref) <= RTOL
    assert np.array_equal(bits(outs[0].reshape(ref.shape)), bits(mq.QGpu(c, "f16", kv_chunk=128, dev=dev).run()))
    assert g.guards_intact()


def test_set_rows_then_attention(dev):
    """fattn_set_rows writes f32 [576, nr] rows into a Q8_0 [N][1][612] cache by
    I64 slots; fattn_ext over that cache is bit-equal to the launch over the
    host-built cache of the same rows."""
    import ctypes as C

    import torch

    import fattn
    sh = CHUNKED
    N, rb = sh.N, mq.ROW["q8_0"]
    rng = np.random.default_rng(4421)                        # mq.cache(sh, "q8_0", 0)'s draws: q, then the rows
    rng.standard_normal((sh.S, sh.NQ, sh.H, DK), dtype=np.float32)
    x = rng.standard_normal((N, DK), dtype=np.float32)
    blocks, _, _ = mq.cache(sh, "q8_0")
    assert np.array_equal(mq.orc.quantize(x, mq.TYPES["q8_0"]), blocks[0, 0])
    perm = np.random.default_rng(12).permutation(N).astype(np.int64)
    src = torch.from_numpy(np.ascontiguousarray(x[perm])).to(dev)      # src row i = x[perm[i]] goes to slot perm[i]
    idx = torch.from_numpy(perm).to(dev)
    cache = torch.full((N * rb + 256,), 0x7E, dtype=torch.uint8, device=dev)
    ts = fattn.View(src.data_ptr(), fattn.TYPE_F32, (DK, N, 1, 1), (4, DK * 4, DK * 4 * N, DK * 4 * N)).c()
    ti = fattn.View(idx.data_ptr(), fattn.TYPE_I64, (N, 1, 1, 1), (8, 8 * N, 8 * N, 8 * N)).c()
    td = fattn.View(cache.data_ptr(), fattn.TYPE_Q8_0, (DK, N, 1, 1), (34, rb, rb * N, rb * N)).c()
    rc = fattn.lib().fattn_set_rows(C.byref(ts), C.byref(ti), C.byref(td), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    c, ref = mq.cached(sh, "q8_0", "random")
    want = mq.QGpu(c, kv_chunk=128, dev=dev).run()
    g = mq.QGpu(c, kv_chunk=128, dev=dev, k_tensor=cache)
    got = g.run()
    assert g.guards_intact()
    assert np.array_equal(bits(got), bits(want))
    assert attn_rel_err(got, ref) <= RTOL and attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("typ", TYPS)
@pytest.mark.parametrize("v_off", [0, 64])
def test_kernel_test_harness(dev, typ, v_off):
    r = run_kernel_test(["--mla", "--kv-type", typ, "--v-off", v_off, "--heads", "16", "--kv-size", "416", "--n-q", "2", "--iters", "3"])
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout
