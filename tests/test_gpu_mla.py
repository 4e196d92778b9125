"""MLA attention (K dim 576, V dim 512, V a view of K; include/fattn.h) on the
GPU against tests/mla.py's padded-V reference.

Bars: the project's own -- attn_rel_err <= 1e-3 and attn_elem_err <= 1, NaN
positions coinciding -- over the WHOLE dst allocation, with the sentinel bands
around it and the workspace tail intact.  Every case prints its two figures
(`MLA_ERR <form> <case> rel=... elem=...`) before it asserts.

Shapes are (H, Hkv, n_q, N, S / Skv), each the smallest that reaches its path:
one wave of four busy (16 rows), a partly filled last wave (80 rows = 5 query
rows x 16 heads over two tiles), two row tiles per kv head (128 heads), several
chunks with a one-tile last chunk (416 keys in chunks of 128), N no multiple of
32 (173), and a prefill-sized n_q (96 rows x 16 heads = 24 tiles).
"""
import numpy as np
import pytest

import mla
import op_params as op
from gpu_util import WS_TAIL_BYTES, graph_replay, run_kernel_test
from mla import Shape
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu

RTOL = 1e-3

DECODE = Shape(16, 1, 1, 160)
CHUNKED = Shape(16, 1, 1, 416)       # kv_chunk = 128: 4 chunks, the last of one tile
ROWS5 = Shape(16, 1, 5, 224)


def check(g, ref: np.ndarray, tag: str, plan: str = ""):
    d = g.describe()
    assert "fattn_mla_kernel" in d and plan in d, d
    got = g.run()
    rel, el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    form = d.split("v=")[1].split(">")[0]
    print(f"MLA_ERR v={form} {tag} rel={rel:.3e} elem={el:.3f} [{d}]")
    assert g.guards_intact(), "dst guard bands or workspace tail overwritten"
    assert rel <= RTOL, (tag, rel)
    assert el <= 1.0, (tag, el)
    return got


@pytest.mark.parametrize("N,mask", [(160, "none"), (160, "random"), (160, "tail"), (173, "random"), (173, "tail")])
def test_one_row_decode(dev, N, mask):
    c, ref = mla.cached(Shape(16, 1, 1, N), mask)
    check(mla.MlaGpu(c, dev=dev), ref, f"decode-N{N}-{mask}", "grid(1,1,1)")


def test_several_chunks_short_last(dev):
    c, ref = mla.cached(CHUNKED, "random")
    g = mla.MlaGpu(c, kv_chunk=128, dev=dev)
    assert g.ws_bytes > 0
    check(g, ref, "chunked-416", "grid(4,1,1)")


@pytest.mark.parametrize("skv", [2, 1], ids=["own-kv", "shared-kv"])
def test_two_row_tiles_per_kv_head(dev, skv):
    c, ref = mla.cached(Shape(128, 1, 1, 256, 2, skv), "random")
    check(mla.MlaGpu(c, dev=dev), ref, f"h128-skv{skv}", ",2,2)")


def test_two_row_tiles_paired_on_one_xcd(dev):
    """16 workgroups: the planner renumbers them so that a kv head's two row tiles share an XCD."""
    c, ref = mla.cached(Shape(128, 1, 1, 256, 4, 4), "random")
    check(mla.MlaGpu(c, dev=dev), ref, "h128-xcd", "(xcd order) + fattn_mla_merge_kernel grid(2,2,4)")


@pytest.mark.parametrize("layout", mla.LAYOUTS)
def test_head_strides(dev, layout):
    c, ref = mla.cached(Shape(32, 2, 1, 192), "random")
    check(mla.MlaGpu(c, layout=layout, dev=dev), ref, f"hkv2-{layout}", "grid(1,2,1)")


def test_partly_filled_last_tile(dev):
    c, ref = mla.cached(ROWS5, "random")   # (a different mask row per query row)
    check(mla.MlaGpu(c, dev=dev), ref, "rows5", "grid(1,2,1)")


@pytest.mark.parametrize("mask", ["causal", "zero"])
def test_prefill_sized(dev, mask):
    c, ref = mla.cached(Shape(16, 1, 96, 128), mask)
    check(mla.MlaGpu(c, dev=dev), ref, f"prefill-{mask}", "grid(1,24,1)")


@pytest.mark.parametrize("v_form", mla.V_FORMS)
@pytest.mark.parametrize("which", ["chunked", "rows5"])
def test_v_forms(dev, which, v_form):
    """V at byte 0 of K's rows, at byte 128, and a separate buffer with the same values."""
    c, ref = mla.cached(CHUNKED if which == "chunked" else ROWS5, "random")
    g = mla.MlaGpu(c, v_form=v_form, kv_chunk=128 if which == "chunked" else 0, dev=dev)
    check(g, ref, f"{which}-{v_form}", {"view0": "v=k+0>", "view128": "v=k+128>", "own": "v=own>"}[v_form])


def _planes(ne3, ne2, NQ, N):
    return np.stack([np.stack([mla.mask_random(NQ, N, 31 * i3 + i2) for i2 in range(ne2)]) for i3 in range(ne3)])


def _op_case(which: str, what: str) -> mla.Case:
    sh = CHUNKED if which == "chunked" else ROWS5
    if what == "softcap":
        return mla.make_case(sh, "random", logit_softcap=7.5)
    if what == "alibi":
        return mla.make_case(sh, planes=op.distance_mask(sh.NQ, sh.N)[None, None], max_bias=8.0)
    if what == "sinks":
        s = np.random.default_rng(77).uniform(-2.0, 4.0, sh.H).astype(np.float32)
        s[3] = -np.inf
        return mla.make_case(sh, "random", sinks=s)
    if what == "head-planes":
        return mla.make_case(sh, planes=_planes(1, sh.H, sh.NQ, sh.N), ne2=sh.H)
    sh2 = Shape(sh.H, 1, sh.NQ, sh.N, 2, 2)
    return mla.make_case(sh2, planes=_planes(2, 1, sh.NQ, sh.N), ne3=2)


@pytest.mark.parametrize("what", ["softcap", "alibi", "sinks", "head-planes", "seq-planes"])
@pytest.mark.parametrize("which", ["chunked", "rows5"])
def test_scalars_and_planes(dev, which, what):
    c = _op_case(which, what)
    g = mla.MlaGpu(c, kv_chunk=128 if which == "chunked" else 0, dev=dev)
    if which == "chunked":
        assert "grid(4,1," in g.describe(), g.describe()
    check(g, c.reference(), f"{which}-{what}")


def test_fully_masked_row(dev):
    """Row 2's mask is -inf everywhere: NaN without sinks, zeros with sinks."""
    m = mla.mask_random(ROWS5.NQ, ROWS5.N, 5)
    m[2, :] = -np.inf
    c = mla.make_case(ROWS5, planes=m[None, None])
    ref = c.reference()
    assert np.isnan(ref[0, 2]).all() and not np.isnan(ref[0, [0, 1, 3, 4]]).any()
    got = check(mla.MlaGpu(c, dev=dev), ref, "masked-row")
    assert np.isnan(got[0, 2]).all()
    cs = mla.make_case(ROWS5, planes=m[None, None], sinks=np.linspace(-1.0, 2.0, ROWS5.H).astype(np.float32))
    refs = cs.reference()
    assert (refs[0, 2] == 0).all()
    gots = check(mla.MlaGpu(cs, dev=dev), refs, "masked-row-sinks")
    assert (gots[0, 2] == 0).all()


def test_shared_workspace_after_d128_decode(dev):
    """One workspace filled with 0xFF, initialised with fattn_workspace_init, then
    a D = 128 split decode and the MLA decode ordered on it."""
    import torch

    import fattn
    import views
    p128 = make_problem(D=128, NQ=1, H=8, N=1024, kv_type="q8_0", seed=3)
    g128 = views.GpuView(views.make_view(p128), dev)
    c, ref = mla.cached(CHUNKED, "random")
    probe = mla.MlaGpu(c, kv_chunk=128, dev=dev)
    assert g128.ws_bytes > 0 and probe.ws_bytes > 0
    n = max(g128.ws_bytes, probe.ws_bytes)
    ws = torch.full(((n + 3) // 4 + WS_TAIL_BYTES // 4,), -1, dtype=torch.int32, device=dev)   # 0xFF bytes
    rc = fattn.lib().fattn_workspace_init(ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    g128.p.workspace, g128.p.workspace_bytes = ws.data_ptr(), n
    g = mla.MlaGpu(c, kv_chunk=128, dev=dev, ws=ws)
    got128 = g128.run()
    got = g.run()
    assert attn_rel_err(got128, p128.oracle()) <= RTOL
    rel, el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    print(f"MLA_ERR v=k+128 shared-ws rel={rel:.3e} elem={el:.3f}")
    assert rel <= RTOL and el <= 1.0
    assert (ws.view(torch.uint8)[n:].cpu().numpy() == 0xFF).all()


def test_graph_capture_replays_identically(dev):
    c, ref = mla.cached(CHUNKED, "random")
    g = mla.MlaGpu(c, kv_chunk=128, dev=dev)
    _, outs = graph_replay(g.launch, g.dst)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert attn_rel_err(outs[0].reshape(ref.shape), ref) <= RTOL
    assert g.guards_intact()


@pytest.mark.parametrize("v_off", [0, 64])
def test_kernel_test_harness(dev, v_off):
    r = run_kernel_test(["--mla", "--v-off", v_off, "--heads", "16", "--kv-size", "416", "--n-q", "2", "--iters", "3"])
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "PASS" in r.stdout
