"""CPU: fattn_rope_set_rows -- the symbol and every validation code without touching a GPU.  Every call here
must fail validation: a valid one would launch over the made-up pointers."""
import ctypes as C

import pytest

import fattn
import k_shift as ks
from gpu_util import run_kernel_test

PTR = 1 << 20   # made-up device pointers


def _part(typ, ne0, nr, ne3):
    rb, eb = ks.row_bytes(typ, ne0), ks.elem_bytes(typ)
    return (fattn.View(PTR, fattn.TYPE_F32, (ne0, nr, 2, ne3), (4, ne0 * 4, ne0 * 4 * nr, ne0 * 8 * nr)),
            fattn.View(PTR, typ, (ne0, 32, 2, ne3), (eb, rb * 2, rb, rb * 64)))


def _args(typ=fattn.TYPE_Q8_0, ne0=128, nr=8, ne3=1, np_=1):
    (k_src, k_dst), (v_src, v_dst) = _part(typ, ne0, nr, ne3), _part(fattn.TYPE_Q4_0, 64, nr, ne3)
    pos = fattn.View(PTR, fattn.TYPE_I32, (nr, np_, 1, 1), (4, 4 * nr, 4 * nr * np_, 4 * nr * np_))
    idx = fattn.View(PTR, fattn.TYPE_I64, (nr, 1, 1, 1), (8, 8 * nr, 8 * nr, 8 * nr))
    return dict(k_src=k_src, pos=pos, idx=idx, k_dst=k_dst, ff=None, rope=ks.Rope(128), v_src=v_src, v_dst=v_dst)


def _rc(a):
    ts = {n: None if a[n] is None else a[n].c() for n in ("k_src", "pos", "idx", "k_dst", "v_src", "v_dst")}
    ref = lambda n: None if ts[n] is None else C.byref(ts[n])
    rp = None if a["rope"] is None else a["rope"].c()
    return fattn.lib().fattn_rope_set_rows(ref("k_src"), ref("pos"), ref("idx"), ref("k_dst"), a["ff"],
                                           None if rp is None else C.byref(rp), ref("v_src"), ref("v_dst"), None)


def _edit(a, name, **kw):
    """View `name` of the arguments a with ptr / type / neN / nbN replaced."""
    v = a[name]
    d = dict(ptr=v.ptr, type=v.type, ne=list(v.ne), nb=list(v.nb))
    for key, val in kw.items():
        if key in ("ptr", "type"):
            d[key] = val
        else:
            d[key[:2]][int(key[2])] = val
    a[name] = fattn.View(d["ptr"], d["type"], tuple(d["ne"]), tuple(d["nb"]))


CASES = [   # (code, argument, its edit): a view's fields, or the value that replaces the argument
    (-1, "k_src", None), (-1, "idx", None), (-1, "k_dst", None), (-1, "pos", None), (-1, "v_src", None), (-1, "v_dst", None),
    (-1, "k_src", dict(ptr=0)), (-1, "v_dst", dict(ptr=0)), (-1, "k_dst", dict(ne0=96)), (-1, "k_dst", dict(ne2=3)),
    (-1, "idx", dict(ne0=7)), (-1, "idx", dict(ne3=2)), (-1, "pos", dict(ne0=7)), (-1, "pos", dict(ne2=2)), (-1, "pos", dict(ne1=2)),
    (-1, "v_src", dict(ne1=4)), (-1, "v_src", dict(ne0=48)), (-1, "rope", ks.Rope(136)), (-1, "rope", ks.Rope(100)),
    (-1, "rope", ks.Rope(128, 8)), (-1, "rope", ks.Rope(128, freq_base=0.0)), (-1, "rope", ks.Rope(128, ext_factor=1.0)),
    (-2, "k_src", dict(type=fattn.TYPE_F16)), (-2, "v_src", dict(type=fattn.TYPE_Q8_0)), (-2, "idx", dict(type=fattn.TYPE_F32)),
    (-2, "pos", dict(type=fattn.TYPE_I64)), (-2, "k_dst", dict(type=fattn.TYPE_I32)), (-2, "v_dst", dict(type=5)),
    (-4, "k_src", dict(nb0=8)), (-4, "k_dst", dict(nb0=18)), (-4, "v_dst", dict(nb0=34)), (-4, "idx", dict(nb0=4)), (-4, "pos", dict(nb0=2)),
    (-7, "k_src", dict(ptr=PTR + 2)), (-7, "k_src", dict(nb1=514)), (-7, "k_dst", dict(ptr=PTR + 1)), (-7, "v_dst", dict(nb2=19)),
    (-7, "idx", dict(ptr=PTR + 4)), (-7, "pos", dict(ptr=PTR + 2)), (-7, "pos", dict(nb0=6)), (-7, "ff", PTR + 2),
]


@pytest.mark.parametrize("code,name,edit", CASES, ids=[f"{c[0]}-{c[1]}-{i}" for i, c in enumerate(CASES)])
def test_validation(code, name, edit):
    a = _args()
    if isinstance(edit, dict):
        _edit(a, name, **edit)
    else:
        a[name] = edit
    assert _rc(a) == code


def test_symbol_strides_and_long_rows():
    assert "fattn_rope_set_rows" in fattn.EXPORTS and hasattr(fattn.lib(), "fattn_rope_set_rows")
    a = _args(ne3=2, np_=2)
    _edit(a, "pos", nb1=-32)                                  # a negative stride of the second pos plane
    assert _rc(a) == -4
    for typ, ptr in ((fattn.TYPE_F32, PTR + 2), (fattn.TYPE_BF16, PTR + 1)):   # both are dst types here; F32 is 4-byte aligned
        a = _args(typ=typ)
        _edit(a, "k_dst", ptr=ptr)
        assert _rc(a) == -7
    # ne0 = 288 is refused with a rope; without one K is accepted and validation stops at V: its NULL data, its alignment
    a = _args(ne0=288)
    a["rope"] = ks.Rope(64)
    _edit(a, "v_dst", ptr=0)
    assert _rc(a) == -3
    a.update(rope=None, pos=None)
    assert _rc(a) == -1
    _edit(a, "v_dst", ptr=PTR + 1)
    assert _rc(a) == -7


def test_harness_rope_set_rows_cpu_only():
    r = run_kernel_test(["--rope-set-rows", "--kv-type", "q8_0", "--rope-mode", "neox", "--cpu-only", "--kv-size", "96",
                         "--heads", "4", "--kv-heads", "2"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rope-set-rows" in r.stdout
