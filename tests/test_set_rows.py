"""CPU: fattn_set_rows (GGML_OP_SET_ROWS, the KV-cache write by slot index) --
the symbol and its validation codes without touching a GPU, and the reference
side of tests/test_gpu_set_rows.py: the edge blocks of tests/set_rows.py give
the bytes that tell a wrong tie rule from the right one, and set_rows_ref
applies ggml's broadcast and the out-of-range skip."""
import ctypes as C

import numpy as np
import pytest

import fattn
import kv_types as kt
import set_rows as sr

PTR = 1 << 20   # made-up device pointers: nothing launches when validation fails


def _views(typ=fattn.TYPE_Q8_0, ityp=None, ne0=128, nr=8, ne2=2, ne3=1, n_slots=32):
    ityp = fattn.TYPE_I64 if ityp is None else ityp
    es = 8 if ityp == fattn.TYPE_I64 else 4
    rb, eb = sr.row_bytes(typ, ne0), sr.elem_bytes(typ)
    src = fattn.View(PTR, fattn.TYPE_F32, (ne0, nr, ne2, ne3), (4, ne0 * 4, ne0 * 4 * nr, ne0 * 4 * nr * ne2))
    idx = fattn.View(PTR, ityp, (nr, 1, 1, 1), (es, es * nr, es * nr, es * nr))
    dst = fattn.View(PTR, typ, (ne0, n_slots, ne2, ne3), (eb, rb * ne2, rb, rb * ne2 * n_slots))
    return src, idx, dst


def _rc(src, idx, dst):
    s, i, d = (None if v is None else v.c() for v in (src, idx, dst))
    ref = lambda t: None if t is None else C.byref(t)
    return fattn.lib().fattn_set_rows(ref(s), ref(i), ref(d), None)


def _with(view, **kw):
    d = dict(ptr=view.ptr, type=view.type, ne=list(view.ne), nb=list(view.nb))
    for k, v in kw.items():
        if k in ("ptr", "type"):
            d[k] = v
        else:                       # ne1=..., nb0=...
            d[k[:2]][int(k[2])] = v
    return fattn.View(d["ptr"], d["type"], tuple(d["ne"]), tuple(d["nb"]))


def test_symbol_exported():
    assert "fattn_set_rows" in fattn.EXPORTS
    assert hasattr(fattn.lib(), "fattn_set_rows")
    assert (fattn.TYPE_I32, fattn.TYPE_I64) == (26, 27)
    # index types stay index types: no row size, no KV type
    assert fattn.row_size(fattn.TYPE_I32, 128) == 0 and fattn.row_size(fattn.TYPE_I64, 128) == 0


def test_null_and_shape_are_invalid_arg():
    s, i, d = _views()
    assert _rc(None, i, d) == -1 and _rc(s, None, d) == -1 and _rc(s, i, None) == -1
    assert _rc(_with(s, ptr=0), i, d) == -1 and _rc(s, _with(i, ptr=0), d) == -1 and _rc(s, i, _with(d, ptr=0)) == -1
    for k in range(4):                                        # any ne <= 0
        for bad in (0, -1):
            assert _rc(_with(s, **{f"ne{k}": bad}), i, d) == -1
            assert _rc(s, _with(i, **{f"ne{k}": bad}), d) == -1
            assert _rc(s, i, _with(d, **{f"ne{k}": bad})) == -1
    assert _rc(s, i, _with(d, ne0=96)) == -1                  # row lengths differ
    assert _rc(s, i, _with(d, ne2=3)) == -1 and _rc(s, i, _with(d, ne3=2)) == -1
    assert _rc(s, _with(i, ne0=7), d) == -1                   # one index per src row
    assert _rc(s, _with(i, ne3=2), d) == -1                   # idx.ne[3] must be 1
    s3, i3, d3 = _views(ne2=6, ne3=4)
    assert _rc(s3, _with(i3, ne1=4), d3) == -1                # 6 % 4
    assert _rc(s3, _with(i3, ne2=3), d3) == -1                # 4 % 3
    s100, i100, d100 = _views(ne0=100)                        # not whole blocks
    assert _rc(s100, i100, _with(d100, nb0=34)) == -1


def test_types_are_unsupported_type():
    s, i, d = _views()
    assert _rc(_with(s, type=fattn.TYPE_F16), i, d) == -2     # src must be f32
    for t in (fattn.TYPE_F32, fattn.TYPE_F16, fattn.TYPE_Q8_0, 5):
        assert _rc(s, _with(i, type=t), d) == -2              # idx: I32 / I64 only
    for t in (fattn.TYPE_F32, fattn.TYPE_I32, fattn.TYPE_I64, 30):
        assert _rc(s, i, _with(d, type=t)) == -2              # dst: F16 and the five block types


def test_other_entry_points_reject_index_types():
    s, i, d = _views()
    for t in (fattn.TYPE_I32, fattn.TYPE_I64):
        a, b = s.c(), _with(d, type=t).c()
        assert fattn.lib().fattn_cpy(C.byref(a), C.byref(b), None) == -2
        assert fattn.lib().fattn_quantize(t, PTR, PTR, 128, 1, None) == -2
        assert fattn.lib().fattn_dequantize(t, PTR, PTR, 128, 1, None) == -2


def test_nb0_is_bad_stride():
    s, i, d = _views()
    assert _rc(_with(s, nb0=8), i, d) == -4
    assert _rc(s, i, _with(d, nb0=18)) == -4
    assert _rc(s, _with(i, nb0=4), d) == -4                   # I64 indices closer than 8 bytes
    assert _rc(s, _with(i, nb0=0), d) == -4
    s32, i32, d32 = _views(ityp=fattn.TYPE_I32)
    assert _rc(s32, _with(i32, nb0=2), d32) == -4
    sf, if_, df = _views(typ=fattn.TYPE_F16)
    assert _rc(sf, if_, _with(df, nb0=4)) == -4


def test_alignment():
    s, i, d = _views()
    assert _rc(_with(s, ptr=PTR + 2), i, d) == -7
    for k in (1, 2, 3):
        assert _rc(_with(s, **{f"nb{k}": s.nb[k] + 2}), i, d) == -7
        assert _rc(s, i, _with(d, **{f"nb{k}": d.nb[k] + 1}), ) == -7
    assert _rc(s, i, _with(d, ptr=PTR + 1)) == -7
    assert _rc(s, _with(i, ptr=PTR + 4), d) == -7             # I64 base
    assert _rc(s, _with(i, nb0=12), d) == -7
    s32, i32, d32 = _views(ityp=fattn.TYPE_I32)
    assert _rc(s32, _with(i32, ptr=PTR + 2), d32) == -7
    assert _rc(s32, _with(i32, nb0=6), d32) == -7
    # idx nb[1] / nb[2] are looked at only where the count exceeds 1
    s2, i2, d2 = _views(ne2=2, ne3=2)
    assert _rc(s2, _with(i2, ne1=2, nb1=12), d2) == -7
    assert _rc(s2, _with(i2, ne2=2, nb2=20), d2) == -7
    assert _rc(s2, _with(i2, ne1=2, nb1=-64), d2) == -4       # a negative stride


def test_tie_blocks_discriminate():
    """The reference bytes of the edge blocks: a reduction that breaks ties the
    wrong way writes other bytes."""
    b = sr.tie_blocks()
    assert b.shape == (9, 32) and sr.all_edge_blocks().shape == (17, 32)
    q50 = kt.quantize(b, kt.TYPE_Q5_0)
    d_sign = [int(q50[n, 1]) >> 7 for n in range(4)]
    assert d_sign == [0, 1, 0, 0]                                  # + - + +
    q40 = sr.encode(b, sr.TYPE_Q4_0)
    assert [int(q40[n, 1]) >> 7 for n in range(4)] == [0, 1, 0, 0]
    for typ in (kt.TYPE_Q4_1, kt.TYPE_Q5_1):
        q = kt.quantize(b, typ)
        assert bytes(q[4, 2:4]) == b"\x00\x00" and bytes(q[5, 2:4]) == b"\x00\x80"   # m = +0.0 / -0.0
        assert bytes(q[6, 0:4]) == b"\x00\x00\x00\x80"             # all -0.0: d = +0, m = -0
        assert bytes(q[7, 2:4]) == b"\x00\x00" and bytes(q[8, 2:4]) == b"\x00\x80"
    # an all-zero |max| scan keeps mx = +0.0: d = +0 / -16 = -0.0
    assert bytes(q50[6, 0:2]) == b"\x00\x80" and bytes(q50[7, 0:2]) == b"\x00\x80"


def test_encode_matches_the_type_references():
    x = sr.source_rows(6, 128)
    assert np.array_equal(x.reshape(-1, 32)[:17], sr.all_edge_blocks())
    assert sr.encode(x, sr.TYPE_F16).shape == (6, 256)
    assert np.array_equal(sr.encode(x, sr.TYPE_F16).view(np.float16), x.astype(np.float16))
    for name, typ in sr.TYPES.items():
        assert sr.encode(x, typ).shape == (6, sr.row_bytes(typ, 128)), name


@pytest.mark.parametrize("layout", ["pos", "head"])
def test_ref_skips_and_broadcasts(layout):
    typ, ne0, nr, ne2, ne3, n_slots = sr.TYPE_Q8_0, 32, 4, 2, 2, 6
    cache, off, nb = sr.cache_alloc(typ, ne0, n_slots, ne2, ne3, layout)
    src = sr.source_rows(ne3 * ne2 * nr, ne0).reshape(ne3, ne2, nr, ne0)
    rows = sr.encode(src, typ)
    rb = rows.shape[-1]
    idx = np.array([[[4, -1, n_slots, 1]]], dtype=np.int64)   # one row for every head and stream
    out = sr.set_rows_ref(cache, src, idx, typ, n_slots, off, nb)
    want = cache.copy()
    for i3 in range(ne3):
        for i2 in range(ne2):
            for i, slot in ((0, 4), (3, 1)):
                o = off + slot * nb[1] + i2 * nb[2] + i3 * nb[3]
                want[o:o + rb] = rows[i3, i2, i]
    assert np.array_equal(out, want)
    assert not np.array_equal(out, cache)
    assert np.array_equal(out[:off], cache[:off])             # the guard
    # one index row per head, shared by the streams
    idx2 = np.array([[[0, 1, 2, 3], [5, 4, 3, 2]]], dtype=np.int64)
    out2 = sr.set_rows_ref(cache, src, idx2, typ, n_slots, off, nb)
    o = off + 5 * nb[1] + 1 * nb[2] + 1 * nb[3]
    assert np.array_equal(out2[o:o + rb], rows[1, 1, 0])
    o = off + 0 * nb[1] + 0 * nb[2] + 1 * nb[3]
    assert np.array_equal(out2[o:o + rb], rows[1, 0, 0])
    # nothing but whole rows of the view changed
    changed = np.flatnonzero(out2 != cache)
    assert len(changed) and changed.min() >= off


def test_place_helpers():
    src = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    for tm in (False, True):
        flat, off, nb = sr.place_src(src, token_major=tm, base_off=4, row_pad=8)
        for (i3, i2, i, e) in ((0, 0, 0, 0), (1, 2, 3, 4), (0, 1, 2, 3)):
            o = off + e * nb[0] + i * nb[1] + i2 * nb[2] + i3 * nb[3]
            assert flat[o // 4] == src[i3, i2, i, e]
    idx = sr.permuted_slots(10, (2, 3, 4))
    flat, ne, nb = sr.place_idx(idx, sr.TYPE_I32, stride0=2)
    assert ne == (4, 3, 2, 1) and flat.dtype == np.int32
    assert flat[(1 * nb[2] + 2 * nb[1] + 3 * nb[0]) // 4] == idx[1, 2, 3]
