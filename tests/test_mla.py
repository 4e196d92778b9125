"""MLA attention (K dim 576, V dim 512, V a view of K; include/fattn.h) on the
CPU: the validation contract with made-up pointers (nothing is launched), the
plan as fattn_describe prints it, the workspace rule, the padded-V reference's
identity with the oracle's primitives, the harness's CPU path, and the refusals
that must stay as they were."""
import ctypes as C
import numpy as np
import pytest

import fattn
import mla
from gpu_util import run_kernel_test
from mla import DK, DV, Shape

OK, INVALID, TYPE, HEAD_DIM, STRIDE, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5, -7
BASE = 1 << 24


def params(H=16, Hkv=1, NQ=1, N=160, S=1, Skv=1, v_off=128, own=False, mask=False, dk=DK, dv=DV, dq=DK, ktype=fattn.TYPE_F16,
           vtype=fattn.TYPE_F16, k_nb=None, v_nb=None, k_ptr=2 * BASE, v_ptr=None, q_ptr=BASE, v_nb0=2, mask_ne0=None,
           mask_ptr=4 * BASE, kv_chunk=0, **kw):
    rk = dk * 2
    k_nb = k_nb or (2, rk, rk * N, rk * N * Hkv)
    q = fattn.View(q_ptr, fattn.TYPE_F32, (dq, NQ, H, S), (4, H * dq * 4, dq * 4, NQ * H * dq * 4))
    k = fattn.View(k_ptr, ktype, (dk, N, Hkv, Skv), k_nb)
    if own:
        rv = dv * 2
        v = fattn.View(v_ptr or 3 * BASE, vtype, (dv, N, Hkv, Skv), v_nb or (v_nb0, rv, rv * N, rv * N * Hkv))
    else:
        v = fattn.View(v_ptr or k_ptr + v_off, vtype, (dv, N, Hkv, Skv), v_nb or (v_nb0,) + tuple(k_nb[1:]))
    m = None
    if mask:
        ne0 = mask_ne0 or (N + 63) // 64 * 64
        m = fattn.View(mask_ptr, fattn.TYPE_F16, (ne0, NQ, 1, 1), (2, ne0 * 2, ne0 * 2 * NQ, ne0 * 2 * NQ))
    return fattn.ext_params(q, k, v, m, 5 * BASE, mla.SCALE, 0, 0, kv_chunk, **kw)


def status(p) -> int:
    buf = C.create_string_buffer(512)
    return fattn.lib().fattn_describe(C.byref(p), buf, len(buf))


# ------------------------------------------------------------------ validation

def test_the_shape_is_accepted():
    for kw in ({}, {"H": 128, "S": 32, "Skv": 32, "N": 4096}, {"H": 64}, {"H": 48, "Hkv": 3}, {"N": 1}, {"N": 173, "mask": True},
               {"NQ": 96, "N": 128}, {"own": True}, {"S": 4, "Skv": 2}, {"max_bias": 8.0, "mask": True}, {"logit_softcap": 30.0}):
        assert status(params(**kw)) == OK, kw


def test_row_lengths_other_than_576_512_are_head_dim_errors():
    assert status(params(dv=DK, own=True)) == HEAD_DIM          # V as wide as K
    assert status(params(dk=512, own=True)) == HEAD_DIM
    assert status(params(dv=256, own=True)) == HEAD_DIM
    assert status(params(dk=512, dv=576, own=True)) == HEAD_DIM
    # ... whatever the types are: the pair is looked at first
    assert status(params(dv=DK, own=True, ktype=fattn.TYPE_Q8_0, vtype=fattn.TYPE_Q8_0, k_nb=(34, 612, 612 * 160, 612 * 160),
                         v_nb=(34, 612, 612 * 160, 612 * 160))) == HEAD_DIM


def test_quantised_or_transposed_kv_is_a_type_error():
    q8k = (34, 612, 612 * 160, 612 * 160)
    q8v = (34, 544, 544 * 160, 544 * 160)
    assert status(params(own=True, ktype=fattn.TYPE_Q8_0, vtype=fattn.TYPE_Q8_0, k_nb=q8k, v_nb=q8v)) == TYPE
    assert status(params(own=True, ktype=fattn.TYPE_Q8_0, k_nb=q8k)) == TYPE
    assert status(params(own=True, vtype=fattn.TYPE_Q4_0, v_nb=(18, 288, 288 * 160, 288 * 160))) == TYPE
    assert status(params(own=True, v_nb=(160 * 2, 2, DV * 160 * 2, DV * 160 * 2))) == TYPE     # transposed V
    assert status(params(k_nb=(4, DK * 2, DK * 2 * 160, DK * 2 * 160), own=True)) == TYPE


def test_alignment_of_k_and_v():
    rk = DK * 2
    assert status(params(k_ptr=2 * BASE + 4, own=True)) == ALIGN
    assert status(params(k_ptr=2 * BASE + 8, own=True)) == ALIGN
    assert status(params(v_ptr=3 * BASE + 4, own=True)) == ALIGN
    assert status(params(v_off=8)) == ALIGN                       # a view 8 B into the row
    assert status(params(k_nb=(2, rk + 8, (rk + 8) * 160, (rk + 8) * 160), own=True)) == ALIGN
    assert status(params(Hkv=2, H=32, k_nb=(2, rk, rk * 160 + 4, (rk * 160 + 4) * 2), own=True)) == ALIGN
    assert status(params(S=2, Skv=2, k_nb=(2, rk, rk * 160, rk * 160 + 8), own=True)) == ALIGN
    assert status(params(own=True, v_nb=(2, 1024 + 4, 1028 * 160, 1028 * 160))) == ALIGN
    # padded rows and the [N][Hkv][row] layout qualify
    assert status(params(k_nb=(2, rk + 64, (rk + 64) * 160, (rk + 64) * 160))) == OK
    assert status(params(Hkv=2, H=32, k_nb=(2, 2 * rk, rk, 2 * rk * 160))) == OK
    # Q's rules are today's
    assert status(params(q_ptr=BASE + 4)) == ALIGN
    assert status(params(q_ptr=BASE + 8)) == ALIGN


def test_strides_and_spans():
    rk = DK * 2
    assert status(params(k_nb=(2, rk - 16, rk * 160, rk * 160), own=True)) == STRIDE   # overlapping rows
    n = 1 << 22                                                                         # 4.5 GiB of K rows
    assert status(params(N=n)) == STRIDE
    assert status(params(N=n // 2)) == OK
    assert status(params(N=1 << 21, k_nb=(2, 2 * rk + 64, (2 * rk + 64) << 21, (2 * rk + 64) << 21))) == STRIDE


def test_shapes_and_scalars():
    assert status(params(H=16, Hkv=3)) == INVALID
    assert status(params(S=3, Skv=2)) == INVALID
    assert status(params(N=0)) == INVALID
    assert status(params(max_bias=-1.0)) == INVALID
    assert status(params(logit_softcap=float("nan"))) == INVALID
    assert status(params(head_first=4, n_head_total=16)) == INVALID
    assert status(params(head_first=16, n_head_total=32)) == OK


def test_mask_contract():
    assert status(params(mask=True, N=173, mask_ne0=174)) == OK      # N rounded up to even
    assert status(params(mask=True, N=173, mask_ne0=173)) == INVALID
    assert status(params(mask=True, mask_ptr=4 * BASE + 2)) == ALIGN
    assert status(params(mask=True, mask_ptr=4 * BASE + 4)) == OK    # 4-byte aligned rows are enough
    p = params(mask=True, H=16)
    p.mask.ne[2] = 3
    assert status(p) == INVALID                                      # head planes must divide H
    p.mask.ne[2], p.mask.nb[2] = 16, 2
    assert status(p) == ALIGN


def test_launch_errors_come_before_any_launch():
    """A misaligned sinks pointer and a missing workspace are refused in launch_ext, ahead of the first launch."""
    p = params(N=416, kv_chunk=128)
    assert fattn.workspace_size(p) > 0
    assert fattn.lib().fattn_ext_sinks(C.byref(p), 6 * BASE + 2, None) == ALIGN
    assert fattn.lib().fattn_ext(C.byref(p), None) == WORKSPACE


# ------------------------------------------------------------------ the plan

@pytest.mark.parametrize("kw,grid", [
    ({}, "grid(1,1,1)"),                                                 # one-row decode
    ({"H": 128, "S": 32, "Skv": 32, "N": 4096}, "grid(4,2,32)"),         # batched decode: two row tiles, 4 chunks
    ({"NQ": 4, "S": 8, "Skv": 8, "N": 2048}, "grid(16,1,8)"),            # several query rows and sequences
    ({"NQ": 512, "N": 512}, "grid(2,128,1)"),                            # prefill-sized
])
def test_describe_names_the_kernel(kw, grid):
    d = fattn.describe(params(**kw))
    assert d.startswith("fattn_mla_kernel<f16,DK576,DV512,nomask,v=k+128>"), d
    assert grid in d and "lds 122880" in d and "chunk " in d, d
    multi = not grid.startswith("grid(1,")
    assert ("+ fattn_mla_merge_kernel" in d) == multi, d
    assert (fattn.workspace_size(params(**kw)) > 0) == multi
    # two row tiles per kv head and a grid of a multiple of 16 workgroups: the pair shares an XCD
    assert ("(xcd order)" in d) == (kw.get("H") == 128), d


def test_describe_shows_the_v_form():
    assert "v=k+0>" in fattn.describe(params(v_off=0))
    assert "v=k+128>" in fattn.describe(params(v_off=128))
    assert "v=k+16>" in fattn.describe(params(v_off=16))
    d = fattn.describe(params(own=True))
    assert "v=own>" in d and "lds 147456" in d, d
    # past 128 B, or with other strides, V is loaded on its own
    assert "v=own>" in fattn.describe(params(v_off=144))
    assert "v=own>" in fattn.describe(params(v_nb=(2, DK * 2 + 64, (DK * 2 + 64) * 160, (DK * 2 + 64) * 160)))
    # a stride of a dim of one element is not looked at (Hkv = Skv = 1 here)
    assert "v=k+128>" in fattn.describe(params(v_nb=(2, DK * 2, 7 * 16, 9 * 16)))
    # the mla_v_view helper builds the aliased view
    k = fattn.View(2 * BASE, fattn.TYPE_F16, (DK, 160, 1, 1), (2, DK * 2, DK * 2 * 160, DK * 2 * 160))
    v = fattn.mla_v_view(k)
    assert (v.ptr, tuple(v.ne), tuple(v.nb)) == (2 * BASE + 128, (DV, 160, 1, 1), tuple(k.nb))
    assert fattn.mla_v_view(k, 0).ptr == 2 * BASE
    with pytest.raises(ValueError):
        fattn.mla_v_view(k, 4)
    q = fattn.View(BASE, fattn.TYPE_F32, (DK, 3, 16, 2), (4, 16 * DK * 4, DK * 4, 3 * 16 * DK * 4))
    assert fattn.dst_shape(q, v) == (2, 3, 16, DV)


def test_plan_is_a_function_of_params_alone():
    """Sinks never change the plan: describe and workspace_size take no sinks at
    all, and a launch with sinks is refused or accepted exactly as one without."""
    for kw in ({}, {"N": 416, "kv_chunk": 128}, {"mask": True, "NQ": 5, "N": 224}):
        p = params(**kw)
        assert fattn.describe(p) == fattn.describe(params(**kw))
        assert fattn.workspace_size(p) == fattn.workspace_size(params(**kw))
    p = params(N=416, kv_chunk=128)
    assert fattn.lib().fattn_ext_sinks(C.byref(p), 6 * BASE, None) == fattn.lib().fattn_ext(C.byref(p), None) == WORKSPACE


def test_workspace_zero_for_one_chunk_positive_for_several():
    assert fattn.workspace_size(params(N=160)) == 0
    assert "grid(1,1,1)" in fattn.describe(params(N=160))
    p = params(N=416, kv_chunk=128)
    assert "grid(4,1,1)" in fattn.describe(p)
    # [4 chunks][64 rows] x (512 f32 + (m, l)), the pairs padded to 256 B
    assert fattn.workspace_size(p) == 4 * 64 * 512 * 4 + 4 * 64 * 8
    # kv_chunk is a hint: at most 64 chunks
    assert "grid(64,1,1)" in fattn.describe(params(N=4096, kv_chunk=32))


# ------------------------------------------------------------------ the reference

def test_padded_reference_is_the_oracles_composition():
    c, ref = mla.cached(Shape(16, 1, 3, 160), "random")
    assert ref.shape == (1, 3, 16, DV) and not np.isnan(ref).any()
    un = mla.unpadded_reference(c)
    assert np.array_equal(un.view(np.uint32), ref.view(np.uint32))
    # ... and op_params.reference / sinks.reference (the scalars' path) reduce to it
    assert np.array_equal(mla.make_case(Shape(16, 1, 3, 160), "random", sinks=np.full(16, -np.inf, np.float32))
                          .reference().view(np.uint32), ref.view(np.uint32))
    # the padding columns of the padded problem's own output are exact zeros
    full = c.ref.oracle()
    assert (full[..., DV:] == 0).all()


def test_launch_side_holds_the_same_values():
    c, _ = mla.cached(Shape(32, 2, 1, 192), "random")
    b = c.ref.base
    for layout in mla.LAYOUTS:
        for v_form in mla.V_FORMS:
            L = mla.MlaLaunch(c, layout, v_form)
            p = L.params()
            assert status(p) == OK
            krows = np.lib.stride_tricks.as_strided(L.k_buf, shape=(1, 2, 192, DK * 2), strides=(L.k_nb[3], L.k_nb[2], L.k_nb[1], 1))
            k = mla.orc.f16_bits_to_f32(np.ascontiguousarray(krows).view(np.uint16))
            src = L.v_buf if v_form == "own" else L.k_buf[L.v_off_bytes:]
            vrows = np.lib.stride_tricks.as_strided(src, shape=(1, 2, 192, DV * 2), strides=(L.v_nb[3], L.v_nb[2], L.v_nb[1], 1))
            v = mla.orc.f16_bits_to_f32(np.ascontiguousarray(vrows).view(np.uint16))
            assert np.array_equal(v, b.v_f32[..., :DV])
            # q.k is the padded problem's, whatever the order of the row's dims
            assert np.allclose(np.einsum("snhd,shkd->snhk", L.q[:, :, :16], k[:, :1]),
                               np.einsum("snhd,shkd->snhk", b.q[:, :, :16], b.k_f32[:, :1]), atol=1e-3)


# ------------------------------------------------------------------ the harness

def test_kernel_test_mla_cpu_only(tmp_path):
    outs = []
    for v_off in (0, 64):
        f = tmp_path / f"mla{v_off}.bin"
        r = run_kernel_test(["--mla", "--v-off", v_off, "--cpu-only", "--heads", "4", "--kv-size", "96", "--n-q", "2", "--dump", f])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Reference" in r.stdout
        o = np.fromfile(f, dtype=np.float32)
        assert o.shape == (2 * 4 * DV,) and np.isfinite(o).all()
        outs.append(o)
    assert not np.array_equal(outs[0], outs[1])   # another 512 of the 576 columns
    r = run_kernel_test(["--mla", "--v-off", "32", "--cpu-only"], timeout=60)
    assert r.returncode == 2


# ------------------------------------------------------------------ what stays refused

def test_other_head_dims_stay_refused():
    for d in (512, 72, 112, 192):
        assert status(params(dq=d, dk=d, dv=d, own=True)) == HEAD_DIM, d
    # q of 576 against anything but (576, 512)
    assert status(params(dk=DK, dv=DK, own=True)) == HEAD_DIM
    assert status(params(dk=128, dv=128, own=True)) == HEAD_DIM
    # the old head dims: unequal K / V row lengths stay an invalid argument
    for d, dv in ((128, 64), (256, 128), (64, 128)):
        assert status(params(dq=d, dk=d, dv=dv, own=True)) == INVALID, (d, dv)
    assert status(params(dq=192, dk=192, dv=128, own=True)) == HEAD_DIM
    # the positional entry point has one ne10 for K and V: it cannot name the shape
    rc = fattn.lib().fattn_ext_f16_launch(BASE, 2 * BASE, 2 * BASE + 128, None, 5 * BASE, 0.07, DK, 1, 16, 1, DK, 160, 1, 1, 32,
                                          320, DK * 4, DK * 4, DK * 16 * 4, DK * 2, DK * 2 * 160, DK * 2 * 160, DV, 16, 1, 1,
                                          fattn.TYPE_F16, fattn.TYPE_F16, None, 0, None)
    assert rc == HEAD_DIM
