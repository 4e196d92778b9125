"""GPU: views at the 32-bit limits of the buffer descriptors, on every kernel
family (tests/big_views.py; the host side is tests/test_big_views.py).

One arena of 4.5 GiB holds the big view of every case in turn; the logical
problems are tiny.  Every attention case prints `BIGV <tag> rel=.. elem=.. |
<describe>` and then checks

  (a) the oracle of the logical problem: attn_rel_err <= 1e-3 and attn_elem_err
      <= 1, NaN positions coinciding (both return inf otherwise) -- a poisoned
      byte that reaches an output element fails here,
  (b) the compact twin (the same logical problem, rows back to back or 8 bytes
      apart for the dword path): the same describe line and the same bits,
  (c) dst's guard bands and the workspace tail.

A view the planner rejects (Case.status) asserts that status.  The cache-write
cases (fattn_set_rows, fattn_cpy) compare the rows written with the reference
encoding bit for bit and require every other byte of the arena untouched.
"""
import numpy as np
import pytest

import big_views as bv
import fattn
import set_rows as sr
from problems import attn_elem_err, attn_rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-3


@pytest.fixture(scope="module")
def arena(dev):
    import torch
    a = torch.empty(bv.ARENA_BYTES, dtype=torch.uint8, device=dev)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", bv.CASES, ids=[c.id for c in bv.CASES])
def test_big_view(dev, arena, case):
    import torch
    lay = bv.big_layout(case)
    assert lay.bytes <= arena.numel()
    with fattn.options(dict(case.opts)):
        if case.status:
            with pytest.raises(fattn.FattnError) as e:
                fattn.describe(lay.params(arena.data_ptr(), kv_chunk=case.kv_chunk))
            assert e.value.code == case.status
            return
        g = bv.BigGpu(lay, arena, case.kv_chunk)
        d = g.describe()
        assert case.kernel in d and not (case.avoid and case.avoid in d), d
        got = g.run()
        tw = bv.twin_layout(case)
        small = torch.empty(tw.bytes, dtype=torch.uint8, device=dev)
        t = bv.BigGpu(tw, small, case.kv_chunk)
        d_twin = t.describe()
        got_twin = t.run()
    ref = bv.logical(case)[1]
    e_rel, e_el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    line = f"BIGV {case.tag} rel={e_rel:.3e} elem={e_el:.3f} | {d}"
    print(line)
    # (a)
    assert e_rel <= RTOL, line
    assert e_el <= 1.0, line
    # (b)
    if case.twin:
        assert d_twin == d, (d, d_twin)
        assert np.array_equal(got.view(np.uint32), got_twin.view(np.uint32)), line
    else:
        assert attn_rel_err(got_twin, ref) <= RTOL and attn_elem_err(got_twin, ref) <= 1.0, d_twin
    # (c)
    assert g.guards_intact() and t.guards_intact(), line


# ------------------------------------------------------------------ the cache-write side

POISON64 = 0x7E7E7E7E7E7E7E7E
FAR = bv.FAR
BASE = 4096     # the cache view starts here: the bytes before it are watched too

# (tag, op, dst type, index type, ne0, nr, ne2, n_slots, slots, dst (nb1, nb2), big src nb2)
WRITES = [
    ("set_rows-q8_0-i64-mul64", "set_rows", "q8_0", fattn.TYPE_I64, 128, 5, 2, 5, (4, 0, 3, -1, 5), (bv.GiB + 32, 4096), 0),
    ("set_rows-f16-i32-mul64", "set_rows", "f16", fattn.TYPE_I32, 80, 5, 2, 5, (4, 0, 3, -1, 5), (bv.GiB + 32, 4096), 0),
    ("set_rows-q8_0-i32-nb1-64bit", "set_rows", "q8_0", fattn.TYPE_I32, 128, 3, 2, 2, (1, 0, 2), (FAR, 4096), 0),
    ("set_rows-f16-i64-nb1-64bit", "set_rows", "f16", fattn.TYPE_I64, 80, 3, 2, 2, (1, 0, 2), (FAR, 4096), 0),
    ("set_rows-q8_0-i64-dst-nb2", "set_rows", "q8_0", fattn.TYPE_I64, 128, 4, 2, 9, (7, 2, 8, 0), (None, FAR), 0),
    ("set_rows-f16-i32-dst-nb2", "set_rows", "f16", fattn.TYPE_I32, 80, 4, 2, 9, (7, 2, 8, 0), (None, FAR), 0),
    ("set_rows-q8_0-i64-src-nb2", "set_rows", "q8_0", fattn.TYPE_I64, 128, 4, 2, 9, (7, 2, 8, 0), (None, None), FAR),
    ("set_rows-f16-i32-src-nb2", "set_rows", "f16", fattn.TYPE_I32, 80, 4, 2, 9, (7, 2, 8, 0), (None, None), FAR),
    ("cpy-q8_0-nb1", "cpy", "q8_0", 0, 128, 2, 2, 2, (0, 1), (FAR, 4096), 0),
    ("cpy-f16-nb1", "cpy", "f16", 0, 80, 2, 2, 2, (0, 1), (FAR, 4096), 0),
    ("cpy-q8_0-nb2", "cpy", "q8_0", 0, 128, 3, 2, 3, (0, 1, 2), (None, FAR), 0),
    ("cpy-f16-nb2", "cpy", "f16", 0, 80, 3, 2, 3, (0, 1, 2), (None, FAR), 0),
]


def _all_poison(arena) -> bool:
    import torch
    a = arena.view(torch.int64)
    step = 1 << 25      # 256 MiB at a time: the comparison's temporary stays small
    ok = torch.ones((), dtype=torch.bool, device=arena.device)
    for i in range(0, a.numel(), step):
        ok &= (a[i:i + step] == POISON64).all()
    return bool(ok.item())


@pytest.mark.parametrize("w", WRITES, ids=[w[0] for w in WRITES])
def test_cache_write(dev, arena, w):
    """fattn_set_rows / fattn_cpy into (or, src-nb2, out of) a view of the arena
    with a stride past 2^32 or slot * nb[1] past 2^32: the rows written equal
    set_rows.encode() bit for bit at the 64-bit addresses, and no other byte of
    the arena changed."""
    import torch
    tag, op, tname, ityp, ne0, nr, ne2, n_slots, slots, (nb1, nb2), src_nb2 = w
    typ = sr.TYPES[tname]
    rb, eb = sr.row_bytes(typ, ne0), sr.elem_bytes(typ)
    src = sr.source_rows(ne2 * nr, ne0, seed=len(tag)).reshape(1, ne2, nr, ne0)
    want = sr.encode(src, typ)                                   # [1][ne2][nr][rb]
    arena.view(torch.int64).fill_(POISON64)
    # src: a compact device tensor, or f32 rows in the arena with planes src_nb2 apart
    s_nb = (4, ne0 * 4, src_nb2 or nr * ne0 * 4, ne2 * (src_nb2 or nr * ne0 * 4))
    if src_nb2:
        s_view = torch.as_strided(arena, (ne2, nr, ne0 * 4), (src_nb2, ne0 * 4, 1), BASE)
        s_view.copy_(torch.from_numpy(src[0].view(np.uint8).reshape(ne2, nr, ne0 * 4)).to(dev))
        s_ptr = arena.data_ptr() + BASE
        cache = torch.full((n_slots * ne2 * rb + 2 * BASE,), 0x7E, dtype=torch.uint8, device=dev)
        d_nb = (eb, rb, n_slots * rb, ne2 * n_slots * rb)
    else:
        s_t = torch.from_numpy(src).to(dev)
        s_ptr = s_t.data_ptr()
        cache = arena
        nb1 = rb if nb1 is None else nb1
        nb2 = n_slots * nb1 if nb2 is None else nb2
        d_nb = (eb, nb1, nb2, ne2 * nb2)
        assert BASE + (n_slots - 1) * nb1 + (ne2 - 1) * nb2 + rb <= arena.numel()
    sv = fattn.View(s_ptr, fattn.TYPE_F32, (ne0, nr, ne2, 1), s_nb)
    dv = fattn.View(cache.data_ptr() + BASE, typ, (ne0, n_slots, ne2, 1), d_nb)
    if op == "set_rows":
        idx = np.array(slots, dtype=sr.IDX_DTYPE[ityp]).reshape(1, 1, nr)
        i_t = torch.from_numpy(idx.reshape(-1)).to(dev)
        es = idx.itemsize
        fattn.set_rows(sv, fattn.View(i_t.data_ptr(), ityp, (nr, 1, 1, 1), (es, es * nr, es * nr, es * nr)), dv)
    else:
        assert tuple(slots) == tuple(range(n_slots)) and nr == n_slots
        fattn.cpy(sv, dv)
    torch.cuda.synchronize()
    # the rows that must have been written, by 64-bit address
    offs, rows = [], []
    for i2 in range(ne2):
        for i, slot in enumerate(slots):
            if 0 <= slot < n_slots:
                offs.append(BASE + slot * d_nb[1] + i2 * d_nb[2])
                rows.append(want[0, i2, i])
    ix = torch.tensor(offs, dtype=torch.int64, device=dev)[:, None] + torch.arange(rb, device=dev)[None, :]
    got = cache[ix].cpu().numpy()
    bad = [o for o, g_, r in zip(offs, got, rows) if not np.array_equal(g_, r)]
    print(f"BIGV {tag}: {len(offs)} rows of {rb} B, highest at byte {max(offs)}, mismatching {len(bad)}")
    assert not bad, (tag, bad)
    # every other byte untouched: put the poison back over the rows and look at the whole allocation
    cache[ix] = 0x7E
    if src_nb2:
        assert bool((cache == 0x7E).all().item()), tag
        s_view.fill_(0x7E)
    assert _all_poison(arena), tag
