"""fattn_ext_sparse (include/fattn.h) on the CPU, over made-up pointers (nothing is launched): the symbols, the
validation order, the workspace rule, and the dense MLA plans unchanged around a sparse sizing call."""
import ctypes as C

import pytest

import fattn
from test_abi import header_symbols
from test_mla import ALIGN, BASE, HEAD_DIM, INVALID, STRIDE, TYPE, WORKSPACE, params

IDX = 6 * BASE


def lists(topk=70, NQ=1, e2=1, e3=1, ptr=IDX, typ=fattn.TYPE_I32, nb=None):
    return fattn.View(ptr, typ, (topk, NQ, e2, e3), nb or (4, 4 * topk, 4 * topk * NQ, 4 * topk * NQ * e2))


def status(p, idx, sinks=None, lse=None) -> int:
    return fattn.lib().fattn_ext_sparse(C.byref(p), C.byref(idx.c()) if idx else None, sinks, lse, None)


def test_symbols_are_declared_and_exported():
    for name in ("fattn_ext_sparse_workspace_size", "fattn_ext_sparse"):
        assert name in fattn.EXPORTS and name in header_symbols() and hasattr(fattn.lib(), name)


@pytest.mark.parametrize("want,pkw,ikw", [
    (INVALID, {"mask": True}, {}),                                   # the list is the mask
    (HEAD_DIM, {"dk": 128, "dv": 128, "dq": 128, "own": True}, {}),  # a dense shape fattn_ext serves
    (HEAD_DIM, {"dv": 256, "own": True}, {"typ": fattn.TYPE_I64}),   # p's own status comes first
    (INVALID, {}, None),
    (INVALID, {}, {"topk": (1 << 24) + 1}),
    (INVALID, {"NQ": 2}, {"NQ": 3}),
    (INVALID, {"H": 48, "Hkv": 3}, {"e2": 2}),                       # e2 is 1 or Hkv
    (INVALID, {"S": 4, "Skv": 2}, {"e3": 3}),                        # S % e3
    (TYPE, {}, {"typ": fattn.TYPE_I64, "nb": (8, 560, 560, 560)}),   # ... before its strides
    (STRIDE, {}, {"nb": (8, 560, 560, 560)}),
    (STRIDE, {"NQ": 2}, {"NQ": 2, "nb": (4, -280, 0, 0)}),
    (ALIGN, {}, {"ptr": IDX + 2}),
    (ALIGN, {"NQ": 2}, {"NQ": 2, "nb": (4, 282, 0, 0)}),
    (STRIDE, {}, {"ptr": IDX + 2, "nb": (2, 280, 280, 280)}),        # ... the stride before the alignment
])
def test_validation_order(want, pkw, ikw):
    p, idx = params(**pkw), None if ikw is None else lists(**ikw)
    assert status(p, idx) == want
    assert fattn.sparse_workspace_size(p, idx) == 0 if idx else True


def test_sinks_lse_and_workspace_come_last():
    p = params(N=4096, kv_chunk=128)
    idx = lists(416)
    assert status(p, idx, sinks=7 * BASE + 2) == ALIGN and status(p, idx, lse=7 * BASE + 2) == ALIGN
    assert status(p, idx) == WORKSPACE
    # more than 65535 tiles in grid.y: one per query row here, where the dense plan packs four rows a tile
    assert status(params(NQ=70000), lists(NQ=70000)) == INVALID


@pytest.mark.parametrize("kw", [{}, {"H": 128}, {"own": True}, {"H": 48, "Hkv": 3, "S": 2, "Skv": 2}])
def test_workspace_is_the_dense_plan_s_for_the_same_chunks(kw):
    """0 for one chunk; else the dense MLA plan's figure at n_q = 1 over topk keys in as many chunks; idx.data unread."""
    e2 = kw.get("Hkv", 1)
    assert fattn.sparse_workspace_size(params(N=4096, **kw), lists(70, e2=e2)) == 0
    sparse = params(N=4096, kv_chunk=128, **kw)
    idx = lists(416, e2=e2)
    got = fattn.sparse_workspace_size(sparse, idx)
    assert got == fattn.workspace_size(params(N=416, kv_chunk=128, **kw)) > 0
    assert got == fattn.sparse_workspace_size(sparse, lists(416, e2=e2, ptr=9 * BASE))
    assert fattn.sparse_workspace_size(params(N=4096, NQ=3, kv_chunk=128, **kw), lists(416, NQ=3, e2=e2)) == 3 * got


def test_dense_plans_do_not_move():
    cases = [{}, {"H": 128, "S": 32, "Skv": 32, "N": 4096}, {"NQ": 4, "S": 8, "Skv": 8, "N": 2048}, {"NQ": 512, "N": 512}]
    before = [(fattn.describe(params(**kw)), fattn.workspace_size(params(**kw))) for kw in cases]
    for kw in cases:
        fattn.sparse_workspace_size(params(**kw), lists(2048, NQ=kw.get("NQ", 1)))
    assert before == [(fattn.describe(params(**kw)), fattn.workspace_size(params(**kw))) for kw in cases]
