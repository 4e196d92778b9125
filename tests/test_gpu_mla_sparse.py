"""fattn_ext_sparse (include/fattn.h: MLA attention over per-query slot lists) on the GPU.
Reference: tests/mla.py's padded-V reference over a COMPACTED case per (sequence, query row,
kv head) -- a cache holding the rows K[e_j] of the list's valid entries in list order: duplicates
count twice, invalid entries are gone.  A row with no valid entry is the header's rule.  Bars:
tests/test_gpu_mla.py's over the whole dst, guard bands and workspace tail intact; lse:
tests/lse.py's.  Every case prints its figures before it asserts."""
import itertools

import numpy as np
import pytest

import fattn
import lse as ls
import mla
import mla_quant as mq
import op_params as op
import sinks as sk
from gpu_util import SENTINEL, WS_TAIL_BYTES, capture, check_bars, run_kernel_test
from mla import DK, DV, Shape
from oracle import oracle as orc
from problems import Problem

pytestmark = pytest.mark.gpu

H16 = Shape(16, 1, 1, 300)


def make_lists(sh: Shape, topk: int, e2=1, e3=1, seed=0, dead=()) -> np.ndarray:
    """i32 [e3][e2][NQ][topk]: shuffled slots with two -1, one entry >= N and two
    duplicates per list; dead: slices of list positions set to -1 in every list."""
    rng = np.random.default_rng(811 + seed)
    out = np.empty((e3, e2, sh.NQ, topk), dtype=np.int32)
    for l in out.reshape(-1, topk):
        l[:] = rng.permutation(max(sh.N, topk))[:topk] % sh.N
        l[[2, topk - 1]], l[7], l[[5, 11]] = -1, sh.N + 3, l[[9, 3]]
        for d in dead:
            l[d] = -1
    return out


def compact_case(q, k, vp, softcap, sinks) -> mla.Case:
    """The one-row MLA case of q [H][576] over the gathered rows k / padded v [n][576]."""
    bits = lambda x: orc.f32_to_f16_bits(x).view(np.uint8).reshape(-1)
    n, rb = len(k), DK * 2
    nb = (2, rb, rb * n, rb * n)
    prob = Problem(DK, 1, len(q), 1, n, 1, 1, orc.TYPE_F16, "head", mla.SCALE, np.ascontiguousarray(q[None, None]), bits(k),
                   bits(vp), nb, nb, None, False, k[None, None], vp[None, None], orc.TYPE_F16)
    return mla.Case(Shape(len(q), 1, 1, n), 0, sk.with_sinks(op.one_plane(prob, None, logit_softcap=softcap), sinks),
                    softcap == 0.0 and sinks is None)


def reference(c: mla.Case, lists, softcap=0.0, sinks=None):
    """(dst f32 [S][NQ][H][512], lse f64 [S][NQ][H]) of the sparse launch of c's q and cache over `lists`."""
    sh, b = c.shape, c.ref.base
    rk2, rk3 = sh.H // sh.Hkv, sh.S // sh.Skv
    e3, e2 = lists.shape[:2]
    dst, lse = np.empty((sh.S, sh.NQ, sh.H, DV), np.float32), np.empty((sh.S, sh.NQ, sh.H))
    for s, i, h2 in itertools.product(range(sh.S), range(sh.NQ), range(sh.Hkv)):
        l = lists[s % e3, h2 % e2, i]
        e, hs = l[(l >= 0) & (l < sh.N)], slice(h2 * rk2, (h2 + 1) * rk2)
        if len(e) == 0:
            dst[s, i, hs], lse[s, i, hs] = (np.nan, -np.inf) if sinks is None else (0.0, sinks[hs])
            continue
        cc = compact_case(b.q[s, i, hs], np.ascontiguousarray(b.k_f32[s // rk3, h2][e]),
                          np.ascontiguousarray(b.v_f32[s // rk3, h2][e]), softcap, None if sinks is None else sinks[hs])
        dst[s, i, hs], lse[s, i, hs] = cc.reference()[0, 0], ls.lse_ref(cc.ref, cc.ref.sinks)[0, 0]
    return dst, lse


def sparse_gpu(g, lists, dev, sinks=None):
    """g (mla.gpu_launch's) turned into the fattn_ext_sparse launch over `lists`, with an lse buffer
    and a workspace of exactly sparse_workspace_size bytes before its sentinel tail."""
    import torch
    g = ls.LseLaunch.of(g)
    g.idx_t = torch.from_numpy(lists).to(dev)
    e3, e2, nq, topk = lists.shape
    g.idx = fattn.View(g.idx_t.data_ptr(), fattn.TYPE_I32, (topk, nq, e2, e3), (4, 4 * topk, 4 * topk * nq, 4 * topk * nq * e2))
    g.sinks_t = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks, np.float32)).to(dev)
    g.ws_bytes, g.own_ws = fattn.sparse_workspace_size(g.p, g.idx), True
    g.ws_all = torch.full(((g.ws_bytes + 3) // 4 + WS_TAIL_BYTES // 4,), SENTINEL, dtype=torch.int32, device=dev)
    g.p.workspace, g.p.workspace_bytes = (g.ws_all.data_ptr(), g.ws_bytes) if g.ws_bytes else (None, 0)
    g.launch = lambda stream=None: fattn.flash_attn_ext_sparse(g.p, g.idx, stream, sinks=g.sinks_t, lse=g.lse)
    return g


def check(g, ref, tag):
    got = g.run()
    check_bars(got, ref[0], lambda rel, el: f"MLA_SPARSE_ERR {tag} rel={rel:.3e} elem={el:.3f} ws={g.ws_bytes}")
    assert g.guards_intact(), "dst / lse guard bands or workspace tail overwritten"
    ls.check_lse(g.lse_out(), ref[1], tag)
    return got


S16, S77 = np.linspace(-1.0, 2.0, 16).astype(np.float32), np.random.default_rng(77).uniform(-2.0, 4.0, 16).astype(np.float32)
CASES = {  # id: (shape, topk, launch kw, list kw, logit_softcap, sinks, kv_chunk)
    **{f"tiles3-{v}": (H16, 70, {"v_form": v}, {}, 0.0, None, 0) for v in mla.V_FORMS},   # three tiles, the last of 6 entries
    "dead-first-tile": (H16, 70, {}, {"dead": (slice(0, 32),)}, 0.0, None, 0),
    "dead-first-tile-sinks": (H16, 70, {}, {"dead": (slice(0, 32),)}, 0.0, S16, 0),
    "dead-all": (H16, 70, {}, {"dead": (slice(0, 70),)}, 0.0, None, 0),
    "dead-all-sinks": (H16, 70, {}, {"dead": (slice(0, 70),)}, 0.0, S16, 0),
    # topk 416 in chunks of 128: chunk 1 all invalid, the last a single tile
    "chunks4": (Shape(16, 1, 1, 500), 416, {}, {"dead": (slice(128, 256),)}, 0.0, None, 128),
    "chunks4-softcap-sinks": (Shape(16, 1, 1, 500), 416, {}, {"dead": (slice(128, 256),)}, 7.5, S77, 128),
    "nq3": (Shape(16, 1, 3, 200), 96, {}, {}, 0.0, None, 0),
    "s2-e3-2-pos": (Shape(16, 1, 1, 200, 2, 2), 96, {"layout": "pos"}, {"e3": 2}, 0.0, None, 0),
    "s2-e3-1": (Shape(16, 1, 1, 200, 2, 1), 96, {}, {}, 0.0, None, 0),
    "hkv2-e2-2-pad": (Shape(32, 2, 2, 200), 96, {"layout": "pad"}, {"e2": 2}, 0.0, None, 0),
    "h128-two-row-tiles": (Shape(128, 1, 1, 200), 96, {}, {}, 0.0, None, 0),
}


@pytest.mark.parametrize("name", CASES)
def test_against_the_compacted_reference(dev, name):
    sh, topk, kw, lkw, softcap, sinks, kv_chunk = CASES[name]
    c = mla.make_case(sh, logit_softcap=softcap)
    lists = make_lists(sh, topk, **lkw)
    g = sparse_gpu(mla.MlaGpu(c, kv_chunk=kv_chunk, dev=dev, **kw), lists, dev, sinks)
    assert (g.ws_bytes > 0) == (kv_chunk > 0)
    got = check(g, reference(c, lists, softcap, sinks), name)
    if name.startswith("dead-all"):
        assert np.isnan(got).all() if sinks is None else (got == 0).all()


@pytest.mark.parametrize("H", [16, 32], ids=["solo", "all4"])
@pytest.mark.parametrize("typ", ["q8_0", "q4_0"])
def test_quantised_equals_f16_over_dequantised(dev, typ, H):
    sh = Shape(H, 1, 1, 300)
    c = mq.make_case(sh, typ)
    lists = make_lists(sh, 70)
    gq = sparse_gpu(mq.QGpu(c, dev=dev), lists, dev)
    gf = sparse_gpu(mq.QGpu(c, form="f16", dev=dev), lists, dev)
    got = check(gq, reference(c, lists), f"{typ}-h{H}")
    assert np.array_equal(got.view(np.uint32), gf.run().view(np.uint32))
    assert np.array_equal(gq.lse_out().view(np.uint32), gf.lse_out().view(np.uint32))


@pytest.mark.parametrize("sh,kv_chunk", [(Shape(16, 1, 1, 173), 0), (Shape(128, 1, 1, 416), 128)], ids=["h16-n173", "h128-n416-chunks"])
def test_identity_list_is_the_dense_launch(dev, sh, kv_chunk):
    c = mla.make_case(sh)
    s = np.linspace(-1.0, 2.0, sh.H).astype(np.float32)
    dense = ls.LseLaunch.of(mla.gpu_launch(mla.MlaLaunch(c), kv_chunk, dev))
    sparse = sparse_gpu(mla.MlaGpu(c, kv_chunk=kv_chunk, dev=dev), np.arange(sh.N, dtype=np.int32).reshape(1, 1, 1, -1), dev, s)
    dense.sinks_t = sparse.sinks_t
    assert np.array_equal(sparse.run().view(np.uint32), dense.run().view(np.uint32))
    assert np.array_equal(sparse.lse_out().view(np.uint32), dense.lse_out().view(np.uint32))
    assert sparse.ws_bytes == dense.ws_bytes and sparse.guards_intact()


def test_captured_launch_follows_the_list_buffer(dev):
    import torch
    c = mla.make_case(H16)
    lists = [make_lists(H16, 70, seed=s) for s in (0, 1)]
    g = sparse_gpu(mla.MlaGpu(c, dev=dev), lists[0], dev)
    graph = capture(g.launch)
    for l in lists[::-1] + lists:   # (several replays: the eager launch saw lists[0])
        g.idx_t.copy_(torch.from_numpy(l).to(dev))
        g.dst.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check_bars(g.dst.cpu().numpy().reshape(1, 1, 16, DV), reference(c, l)[0], lambda rel, el: f"MLA_SPARSE_ERR graph rel={rel:.3e} elem={el:.3f}")
    assert g.guards_intact()


def test_kernel_test_harness(dev):
    r = run_kernel_test(["--mla", "--sparse", "70", "--heads", "16", "--kv-size", "300", "--iters", "3"])
    print(r.stdout[-600:])
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
