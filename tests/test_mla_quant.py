"""MLA attention over a Q8_0 / Q4_0 cache (V a view of K; include/fattn.h) on
the CPU: the validation contract with made-up pointers (nothing is launched),
the plan as fattn_describe prints it, the workspace rule against the f16 view
plan, mla_v_view on quantised views, the test cache's own values and the
harness's CPU path."""
import ctypes as C
import numpy as np
import pytest

import fattn
import mla
import mla_quant as mq
from gpu_util import run_kernel_test
from mla import DK, DV, Shape

OK, INVALID, TYPE, HEAD_DIM, STRIDE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5, -7
BASE = 1 << 24
T = {"q8_0": fattn.TYPE_Q8_0, "q4_0": fattn.TYPE_Q4_0}
BB = {"q8_0": 34, "q4_0": 18}
TYPS = ("q8_0", "q4_0")


def params(typ="q8_0", b=2, H=16, Hkv=1, NQ=1, N=160, S=1, Skv=1, mask=False, k_nb=None, v_nb=None, k_ptr=2 * BASE, v_ptr=None,
           vtype=None, v_nb0=None, kv_chunk=0, pad=0, **kw):
    """typ "f16": the f16 view plan of the same shape (V 64 b bytes in)."""
    if typ == "f16":
        kt, bb, rk = fattn.TYPE_F16, 2, DK * 2
        off = 64 * b
    else:
        kt, bb, rk = T[typ], BB[typ], 18 * BB[typ]
        off = bb * b
    rk += pad
    k_nb = k_nb or (bb, rk, rk * N, rk * N * Hkv)
    q = fattn.View(BASE, fattn.TYPE_F32, (DK, NQ, H, S), (4, H * DK * 4, DK * 4, NQ * H * DK * 4))
    k = fattn.View(k_ptr, kt, (DK, N, Hkv, Skv), k_nb)
    v = fattn.View(v_ptr if v_ptr is not None else k_ptr + off, kt if vtype is None else vtype, (DV, N, Hkv, Skv),
                   v_nb or ((bb if v_nb0 is None else v_nb0),) + tuple(k_nb[1:]))
    m = None
    if mask:
        ne0 = (N + 63) // 64 * 64
        m = fattn.View(4 * BASE, fattn.TYPE_F16, (ne0, NQ, 1, 1), (2, ne0 * 2, ne0 * 2 * NQ, ne0 * 2 * NQ))
    return fattn.ext_params(q, k, v, m, 5 * BASE, mla.SCALE, 0, 0, kv_chunk, **kw)


def status(p) -> int:
    buf = C.create_string_buffer(512)
    return fattn.lib().fattn_describe(C.byref(p), buf, len(buf))


# ------------------------------------------------------------------ validation

@pytest.mark.parametrize("typ", TYPS)
def test_the_shape_is_accepted_over_a_quantised_view_cache(typ):
    """The shapes of test_mla.py::test_the_shape_is_accepted (but V of its own)."""
    for kw in ({}, {"H": 128, "S": 32, "Skv": 32, "N": 4096}, {"H": 64}, {"H": 48, "Hkv": 3}, {"N": 1}, {"N": 173, "mask": True},
               {"NQ": 96, "N": 128}, {"S": 4, "Skv": 2}, {"max_bias": 8.0, "mask": True}, {"logit_softcap": 30.0}):
        for b in (0, 1, 2):
            assert status(params(typ, b, **kw)) == OK, (kw, b)


@pytest.mark.parametrize("typ", TYPS)
def test_a_v_that_is_no_such_view_is_a_type_error(typ):
    bb, rk = BB[typ], 18 * BB[typ]
    rv = 16 * bb
    # V in a buffer of its own, with its own or with K's strides
    assert status(params(typ, v_ptr=3 * BASE, v_nb=(bb, rv, rv * 160, rv * 160))) == TYPE
    assert status(params(typ, v_ptr=3 * BASE)) == TYPE
    assert status(params(typ, v_ptr=2 * BASE - bb)) == TYPE            # before K
    # offsets that are no 0 / 1 / 2 whole blocks
    for off in (17, 35, 102, 3 * bb, 4, 16, 2 * bb + 4):
        assert status(params(typ, v_ptr=2 * BASE + off)) == TYPE, off
    # other strides: rows, heads, sequences, blocks
    assert status(params(typ, v_nb=(bb, rk + 4, (rk + 4) * 160, (rk + 4) * 160))) == TYPE
    assert status(params(typ, H=32, Hkv=2, v_nb=(bb, rk, rk * 160 + 4, (rk * 160 + 4) * 2))) == TYPE
    assert status(params(typ, S=2, Skv=2, v_nb=(bb, rk, rk * 160, rk * 160 + 4))) == TYPE
    assert status(params(typ, v_nb0=2)) == TYPE
    assert status(params(typ, k_nb=(2, rk, rk * 160, rk * 160))) == TYPE
    # ... a stride of a dim of one element is not compared (Hkv = Skv = 1 here)
    assert status(params(typ, v_nb=(bb, rk, 7 * 4, 9 * 4))) == OK
    # mixed types: f16 V on a quantised K, the other block type, a quantised V on an f16 K
    other = "q4_0" if typ == "q8_0" else "q8_0"
    assert status(params(typ, vtype=fattn.TYPE_F16)) == TYPE
    assert status(params(typ, vtype=T[other])) == TYPE
    assert status(params("f16", vtype=T[typ])) == TYPE


def test_the_other_block_types_stay_refused():
    for t, bb in ((fattn.TYPE_Q5_0, 22), (fattn.TYPE_Q4_1, 20), (fattn.TYPE_Q5_1, 24)):
        rk = 18 * bb
        q = fattn.View(BASE, fattn.TYPE_F32, (DK, 1, 16, 1), (4, 16 * DK * 4, DK * 4, 16 * DK * 4))
        k = fattn.View(2 * BASE, t, (DK, 160, 1, 1), (bb, rk, rk * 160, rk * 160))
        v = fattn.View(2 * BASE + 2 * bb, t, (DV, 160, 1, 1), (bb, rk, rk * 160, rk * 160))
        assert status(fattn.ext_params(q, k, v, None, 5 * BASE, mla.SCALE, 0, 0, 0)) == TYPE, t


@pytest.mark.parametrize("typ", TYPS)
def test_alignment_is_4_bytes(typ):
    bb, rk = BB[typ], 18 * BB[typ]
    # a natural cache (612 / 324-B row stride), a base at +4, rows padded by 4 / 20 B, [N][Hkv][row]
    assert status(params(typ)) == OK
    assert status(params(typ, k_ptr=2 * BASE + 4)) == OK
    assert status(params(typ, pad=4)) == OK
    assert status(params(typ, pad=20)) == OK
    assert status(params(typ, H=32, Hkv=2, k_nb=(bb, 2 * rk, rk, 2 * rk * 160))) == OK
    # a base or a stride that is 2 mod 4
    assert status(params(typ, k_ptr=2 * BASE + 2)) == ALIGN
    assert status(params(typ, pad=2)) == ALIGN
    assert status(params(typ, H=32, Hkv=2, k_nb=(bb, rk, rk * 160 + 2, (rk * 160 + 2) * 2))) == ALIGN
    assert status(params(typ, S=2, Skv=2, k_nb=(bb, rk, rk * 160, rk * 160 + 2))) == ALIGN
    # overlapping rows, spans of 4 GiB
    assert status(params(typ, k_nb=(bb, rk - 4, rk * 160, rk * 160))) == STRIDE
    assert status(params(typ, N=1 << 23)) == (STRIDE if typ == "q8_0" else OK)     # 4.8 GiB / 2.5 GiB of rows
    assert status(params(typ, N=1 << 24)) == STRIDE
    # the f16 form keeps its 16-B rule
    assert status(params("f16", k_ptr=2 * BASE + 4)) == ALIGN


def test_the_row_length_check_still_comes_first():
    p = params("q8_0")
    p.v.ne[0] = DK
    assert status(p) == HEAD_DIM
    p = params("q8_0")
    p.k.ne[0] = 512
    assert status(p) == HEAD_DIM


def test_shapes_scalars_and_mask_keep_their_rules():
    assert status(params("q8_0", H=16, Hkv=3)) == INVALID
    assert status(params("q4_0", N=0)) == INVALID
    assert status(params("q8_0", max_bias=-1.0)) == INVALID
    assert status(params("q8_0", head_first=4, n_head_total=16)) == INVALID
    p = params("q8_0", mask=True)
    p.mask.data = 4 * BASE + 2
    assert status(p) == ALIGN


# ------------------------------------------------------------------ the plan

@pytest.mark.parametrize("typ", TYPS)
def test_describe_names_the_solo_form_and_its_16_byte_tiles(typ):
    """No tile with more than 16 rows: wave 0 computes, waves 1 - 3 load and
    convert; contiguous rows on 16-B aligned planes land in 16-B pieces."""
    bb, rk = BB[typ], 18 * BB[typ]
    word = lambda **kw: fattn.describe(params(typ, **kw)).split(">", 1)[1].split(" grid")[0].replace(" + fattn_mla_merge_kernel", "")
    assert word() == word(N=173, mask=True) == word(H=32, Hkv=2, S=4, Skv=2) == " (solo, 16-B tiles)"
    assert word(k_ptr=2 * BASE + 4) == word(pad=4) == word(pad=16) == " (solo)"
    assert word(H=32, Hkv=2, k_nb=(bb, 2 * rk, rk, 2 * rk * 160)) == " (solo)"                       # [N][Hkv][row]
    assert word(H=32, Hkv=2, k_nb=(bb, rk, rk * 160 + 4, (rk * 160 + 4) * 2)) == " (solo)"          # planes 4 mod 16
    for kw in ({"NQ": 5}, {"H": 32}, {"H": 128}, {"NQ": 96, "N": 128}, {"H": 16, "NQ": 2}):
        assert word(**kw) in ("", " (xcd order)"), kw
    assert "solo" not in fattn.describe(params("f16"))


@pytest.mark.parametrize("typ,lds", [("q8_0", 147456), ("q4_0", 119808)])
def test_describe_names_the_type_and_the_byte_offset(typ, lds):
    for b in (0, 1, 2):
        d = fattn.describe(params(typ, b))
        assert d.startswith(f"fattn_mla_kernel<{typ},DK576,DV512,nomask,v=k+{b * BB[typ]}>"), d
        assert f"lds {lds}" in d and "grid(1,1,1)" in d and d.endswith("ws 0"), d
    assert fattn.describe(params(typ, mask=True)).startswith(f"fattn_mla_kernel<{typ},DK576,DV512,mask,v=k+{2 * BB[typ]}>")
    # the suffixes of the f16 plans
    d = fattn.describe(params(typ, H=128, S=32, Skv=32, N=4096))
    assert "(xcd order) + fattn_mla_merge_kernel grid(4,2,32)" in d, d
    # strings of f16 plans do not change
    assert fattn.describe(params("f16")).startswith("fattn_mla_kernel<f16,DK576,DV512,nomask,v=k+128> grid(1,1,1) lds 122880 ")


@pytest.mark.parametrize("typ", TYPS)
def test_workspace_and_chunks_are_the_f16_view_plans(typ):
    assert fattn.workspace_size(params(typ, N=160)) == 0
    p = params(typ, N=416, kv_chunk=128)
    assert "grid(4,1,1)" in fattn.describe(p)
    assert fattn.workspace_size(p) == fattn.workspace_size(params("f16", N=416, kv_chunk=128)) == 4 * 64 * 512 * 4 + 4 * 64 * 8
    strip = lambda d: d.replace(" (solo, 16-B tiles)", "").replace(" (solo)", "")
    tail = lambda d: strip(d).split("> ", 1)[1].replace(d.split("lds ")[1].split(" ")[0], "LDS")
    for kw in ({"N": 160}, {"N": 416, "kv_chunk": 128}, {"N": 4096, "kv_chunk": 32}, {"H": 128, "S": 32, "Skv": 32, "N": 4096},
               {"NQ": 4, "S": 8, "Skv": 8, "N": 2048}, {"NQ": 512, "N": 512}, {"N": 173, "mask": True}):
        dq, df = fattn.describe(params(typ, **kw)), fattn.describe(params("f16", **kw))
        assert tail(dq) == tail(df), (dq, df)       # grid, chunk, slots, workspace: only the LDS figure differs
        assert fattn.workspace_size(params(typ, **kw)) == fattn.workspace_size(params("f16", **kw))
    # a function of p alone; launch errors come before any launch
    assert fattn.describe(p) == fattn.describe(params(typ, N=416, kv_chunk=128))
    assert fattn.lib().fattn_ext(C.byref(p), None) == WORKSPACE
    assert fattn.lib().fattn_ext_sinks(C.byref(p), 6 * BASE + 2, None) == ALIGN


@pytest.mark.parametrize("typ", TYPS)
def test_mla_v_view_on_quantised_views(typ):
    bb, rk = BB[typ], 18 * BB[typ]
    k = fattn.View(2 * BASE, T[typ], (DK, 160, 1, 1), (bb, rk, rk * 160, rk * 160))
    v = fattn.mla_v_view(k)
    assert (v.ptr, v.type, tuple(v.ne), tuple(v.nb)) == (2 * BASE + 2 * bb, T[typ], (DV, 160, 1, 1), tuple(k.nb))
    assert fattn.mla_v_view(k, 0).ptr == 2 * BASE and fattn.mla_v_view(k, 32).ptr == 2 * BASE + bb
    assert fattn.mla_v_view(k, 64).ptr == 2 * BASE + fattn.row_size(T[typ], 64)
    for bad in (8, 16, 96, -32):
        with pytest.raises(ValueError):
            fattn.mla_v_view(k, bad)
    with pytest.raises(ValueError):
        fattn.mla_v_view(fattn.View(2 * BASE, T[typ], (512, 160, 1, 1), (bb, 16 * bb, 16 * bb * 160, 16 * bb * 160)))
    with pytest.raises(ValueError):
        fattn.mla_v_view(fattn.View(2 * BASE, fattn.TYPE_Q5_0, (DK, 160, 1, 1), (22, 396, 396 * 160, 396 * 160)))
    q = fattn.View(BASE, fattn.TYPE_F32, (DK, 3, 16, 2), (4, 16 * DK * 4, DK * 4, 3 * 16 * DK * 4))
    assert fattn.dst_shape(q, v) == (2, 3, 16, DV)


# ------------------------------------------------------------------ the test cache

@pytest.mark.parametrize("typ", TYPS)
def test_launch_side_holds_the_logical_values(typ):
    """The blocks of a QLaunch in every layout dequantise to the case's K; the
    f16 launch holds the same values; V is K's elements from v_off on."""
    sh = Shape(32, 2, 1, 96, 2, 2)
    for v_off in (0, 32, 64):
        c = mq.make_case(sh, typ, "random", v_off)
        b = c.ref.base
        assert np.array_equal(b.v_f32[..., :DV], b.k_f32[..., v_off:v_off + DV]) and (b.v_f32[..., DV:] == 0).all()
        for layout, base in (("head", 0), ("pos", 0), ("pad20", 0), ("pad16", 4)):
            L = mq.QLaunch(c, "quant", layout, base)
            assert status(L.params()) == OK
            rows = np.lib.stride_tricks.as_strided(L.k_buf[base:], shape=(2, 2, 96, mq.ROW[typ]),
                                                   strides=(L.k_nb[3], L.k_nb[2], L.k_nb[1], 1))
            k = mq.orc.dequantize(np.ascontiguousarray(rows), mq.TYPES[typ], DK)
            assert np.array_equal(mq.orc.f16_bits_to_f32(mq.orc.f32_to_f16_bits(k)), b.k_f32)
            # every byte outside the rows is poison
            seen = np.zeros(len(L.k_buf), dtype=bool)
            np.lib.stride_tricks.as_strided(seen[base:], shape=rows.shape, strides=rows.strides, writeable=True)[...] = True
            assert (L.k_buf[~seen] == 0x7E).all()
            F = mq.QLaunch(c, "f16", "head" if layout != "pos" else "pos")
            assert status(F.params()) == OK and F.v_off_bytes == 2 * v_off
    # the f16 rounding is one rounding of an exact product: h(q * d) in f64 agrees
    blocks, k, _ = mq.cache(sh, typ)
    blk = np.ascontiguousarray(blocks).reshape(-1, mq.BLOCK[typ])
    d = blk[:, :2].copy().view(np.float16).astype(np.float64)
    if typ == "q8_0":
        qv = blk[:, 2:].view(np.int8).astype(np.float64)
    else:
        qv = np.concatenate([blk[:, 2:] & 15, blk[:, 2:] >> 4], axis=1).astype(np.float64) - 8.0
    assert np.array_equal((qv * d).astype(np.float16).astype(np.float32).reshape(k.shape), k)


# ------------------------------------------------------------------ the harness

@pytest.mark.parametrize("typ", TYPS)
def test_kernel_test_mla_quant_cpu_only(tmp_path, typ):
    outs = {}
    for v_off in (0, 32, 64):
        f = tmp_path / f"mla{v_off}.bin"
        r = run_kernel_test(["--mla", "--kv-type", typ, "--v-off", v_off, "--cpu-only", "--heads", "4", "--kv-size", "96", "--n-q", "2",
                             "--dump", f])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Reference" in r.stdout
        o = np.fromfile(f, dtype=np.float32)
        assert o.shape == (2 * 4 * DV,) and np.isfinite(o).all()
        outs[v_off] = o
    assert not np.array_equal(outs[0], outs[64]) and not np.array_equal(outs[32], outs[64])
    # the quantised cache's values are not the f16 cache's
    f = tmp_path / "mla_f16.bin"
    r = run_kernel_test(["--mla", "--v-off", "64", "--cpu-only", "--heads", "4", "--kv-size", "96", "--n-q", "2", "--dump", f])
    assert r.returncode == 0
    o16 = np.fromfile(f, dtype=np.float32)
    assert not np.array_equal(o16, outs[64])
    assert np.abs(o16 - outs[64]).max() < (0.05 if typ == "q8_0" else 0.5)      # ... but close to them
    # --v-off 32 stays an f16 error, other offsets and types are refused
    for extra in (["--v-off", "32"], ["--kv-type", typ, "--v-off", "16"], ["--kv-type", "q5_0"]):
        r = run_kernel_test(["--mla", "--cpu-only"] + extra, timeout=60)
        assert r.returncode == 2, extra
