"""CPU: fattn_k_shift (the K-shift, RoPE of a K cache in place) -- the symbol and
every validation code without touching a GPU, and the reference side of
tests/test_gpu_k_shift.py: the identities of the rotation, and that the f32
restatement of the contract meets the derived tolerance against float64 on every
parameter set the GPU cases use."""
import ctypes as C
import math

import numpy as np
import pytest

import fattn
import k_shift as ks
from gpu_util import run_kernel_test

PTR = 1 << 20   # made-up device pointers: nothing launches when validation fails


def _views(typ=fattn.TYPE_Q8_0, ne0=128, n_slots=40, hkv=2, s=1, ns=1):
    rb, eb = ks.row_bytes(typ, ne0), ks.elem_bytes(typ)
    k = fattn.View(PTR, typ, (ne0, n_slots, hkv, s), (eb, rb * hkv, rb, rb * hkv * n_slots))
    sh = fattn.View(PTR, fattn.TYPE_I32, (n_slots, ns, 1, 1), (4, 4 * n_slots, 4 * n_slots * ns, 4 * n_slots * ns))
    return k, sh


def _rc(k, sh, rope=ks.Rope(128), ff=None):
    kc, sc = (None if v is None else v.c() for v in (k, sh))
    rp = None if rope is None else (rope if isinstance(rope, fattn.FattnRope) else rope.c())
    ref = lambda t: None if t is None else C.byref(t)
    return fattn.lib().fattn_k_shift(ref(kc), ref(sc), ff, ref(rp), None)


def _with(view, **kw):
    d = dict(ptr=view.ptr, type=view.type, ne=list(view.ne), nb=list(view.nb))
    for key, v in kw.items():
        if key in ("ptr", "type"):
            d[key] = v
        else:                       # ne1=..., nb0=...
            d[key[:2]][int(key[2])] = v
    return fattn.View(d["ptr"], d["type"], tuple(d["ne"]), tuple(d["nb"]))


def test_symbol_exported():
    assert "fattn_k_shift" in fattn.EXPORTS
    assert hasattr(fattn.lib(), "fattn_k_shift")
    assert C.sizeof(fattn.FattnRope) == 36
    assert (fattn.ROPE_NORMAL, fattn.ROPE_NEOX) == (0, 2)


def test_null_shape_and_rope_are_invalid_arg():
    k, sh = _views()
    assert _rc(None, sh) == -1 and _rc(k, None) == -1 and _rc(k, sh, None) == -1
    assert _rc(_with(k, ptr=0), sh) == -1 and _rc(k, _with(sh, ptr=0)) == -1
    for d in range(4):                                        # any ne <= 0
        for bad in (0, -1):
            assert _rc(_with(k, **{f"ne{d}": bad}), sh) == -1
            assert _rc(k, _with(sh, **{f"ne{d}": bad})) == -1
    assert _rc(k, _with(sh, ne0=39)) == -1                    # one delta per slot
    assert _rc(k, _with(sh, ne2=2)) == -1 and _rc(k, _with(sh, ne3=2)) == -1
    k3, sh3 = _views(s=3, ns=2)                               # 3 % 2
    assert _rc(k3, sh3) == -1
    assert _rc(*_views(ne0=112), ks.Rope(64)) == -1           # a block type: whole blocks
    assert _rc(*_views(typ=fattn.TYPE_Q8_0, ne0=80), ks.Rope(64)) == -1
    assert _rc(*_views(typ=fattn.TYPE_F16, ne0=66), ks.Rope(64)) == -1   # other types: multiples of 4
    for n_dims in (0, 4, -8, 136, 100, 12):                   # 8 .. ne0, multiples of 8
        assert _rc(k, sh, ks.Rope(n_dims)) == -1, n_dims
    for mode in (1, 3, 8, 24, -1):                            # no M-RoPE / vision modes
        assert _rc(k, sh, ks.Rope(128, mode)) == -1, mode
    inf, nan = float("inf"), float("nan")
    for bad in (0.0, -1.0, inf, nan):
        assert _rc(k, sh, ks.Rope(128, freq_base=bad)) == -1
        assert _rc(k, sh, ks.Rope(128, freq_scale=bad)) == -1
    for bad in (-0.5, inf, nan):
        assert _rc(k, sh, ks.Rope(128, ext_factor=bad, n_ctx_orig=4096)) == -1
    for bad in (inf, -inf, nan):
        assert _rc(k, sh, ks.Rope(128, attn_factor=bad)) == -1
        assert _rc(k, sh, ks.Rope(128, beta_fast=bad)) == -1
        assert _rc(k, sh, ks.Rope(128, beta_slow=bad)) == -1
    assert _rc(k, sh, ks.Rope(128, ext_factor=1.0, n_ctx_orig=0)) == -1
    assert _rc(k, sh, ks.Rope(128, ext_factor=1.0, n_ctx_orig=-4)) == -1
    # more than 2^31 - 1 blocks in one [ne0, n_slots] plane
    big = 2 ** 31 // 4
    kb, shb = _views(n_slots=big)
    assert _rc(kb, shb) == -1
    kb, shb = _views(typ=fattn.TYPE_F16, ne0=36, n_slots=2 ** 30)   # a partial block counts
    assert _rc(kb, shb, ks.Rope(32)) == -1


def test_types_are_unsupported_type():
    k, sh = _views()
    for t in (4, 5, 9, fattn.TYPE_I32, fattn.TYPE_I64, 31):
        assert _rc(_with(k, type=t), sh) == -2
    for t in (fattn.TYPE_I64, fattn.TYPE_F32, fattn.TYPE_F16, fattn.TYPE_Q8_0):
        assert _rc(k, _with(sh, type=t)) == -2


def test_long_rows_are_unsupported_head_dim():
    for typ, ne0 in ((fattn.TYPE_Q8_0, 288), (fattn.TYPE_F16, 576), (fattn.TYPE_F32, 260), (fattn.TYPE_Q4_0, 512)):
        assert _rc(*_views(typ=typ, ne0=ne0), ks.Rope(64)) == -3


def test_strides_are_bad_stride():
    k, sh = _views()
    assert _rc(_with(k, nb0=18), sh) == -4 and _rc(_with(k, nb0=1), sh) == -4
    kf, shf = _views(typ=fattn.TYPE_F16)
    assert _rc(_with(kf, nb0=4), shf) == -4
    k32, sh32 = _views(typ=fattn.TYPE_F32)
    assert _rc(_with(k32, nb0=2), sh32) == -4
    assert _rc(k, _with(sh, nb0=2)) == -4 and _rc(k, _with(sh, nb0=0)) == -4
    k2, sh2 = _views(s=2, ns=2)
    assert _rc(k2, _with(sh2, nb1=-160)) == -4
    # (every call here must fail validation: a valid one would launch over the made-up pointers)


def test_alignment():
    k, sh = _views()
    assert _rc(_with(k, ptr=PTR + 1), sh) == -7
    for d in (1, 2, 3):
        assert _rc(_with(k, **{f"nb{d}": k.nb[d] + 1}), sh) == -7
    k32, sh32 = _views(typ=fattn.TYPE_F32)
    assert _rc(_with(k32, ptr=PTR + 2), sh32) == -7
    for d in (1, 2, 3):
        assert _rc(_with(k32, **{f"nb{d}": k32.nb[d] + 2}), sh32) == -7
    assert _rc(k, _with(sh, ptr=PTR + 2)) == -7
    assert _rc(k, _with(sh, nb0=6)) == -7
    k2, sh2 = _views(s=2, ns=2)
    assert _rc(k2, _with(sh2, nb1=162)) == -7
    assert _rc(k, sh, ff=PTR + 2) == -7


# ------------------------------------------------------------------ the reference

def _x(ne0, rows=24, seed=2):
    rng = np.random.default_rng(seed)
    return (3.0 * (1.0 - 2.0 * rng.random((rows, ne0), dtype=np.float32))).astype(np.float32)


@pytest.mark.parametrize("mode", [ks.NORMAL, ks.NEOX])
def test_zero_shift_and_identity_parameters(mode):
    x = _x(128)
    r = ks.Rope(96, mode)
    zero = np.zeros(len(x), dtype=np.int32)
    assert np.array_equal(ks.rotate_f32(x, zero, r), x)
    assert np.array_equal(ks.rotate_f64(x, zero, r), x.astype(np.float64))
    y = ks.rotate_f32(x, np.full(len(x), 5, dtype=np.int32), r)
    assert np.array_equal(y[:, 96:], x[:, 96:]) and not np.array_equal(y[:, :96], x[:, :96])   # pass-through past n_dims
    # pair 0 turns by p radians (theta_scale^0 = 1): mode decides which element is its partner
    one = np.zeros((1, 128), dtype=np.float32)
    one[0, 0] = 1.0
    y = ks.rotate_f64(one, np.array([1]), r)
    partner = 48 if mode == ks.NEOX else 1
    assert abs(y[0, 0] - math.cos(1.0)) < 1e-15 and abs(y[0, partner] - math.sin(1.0)) < 1e-15
    assert np.count_nonzero(y) == 2
    # the cache reference leaves zero-shift rows, pass-through blocks and every byte outside the view alone
    for name in ("q8_0", "q5_1", "f16", "f32"):
        typ = ks.TYPES[name]
        alloc, off, nb = ks.make_cache(typ, 128, 12, 2, 1, "pos")
        ne = (128, 12, 2, 1)
        shift = ks.make_shift(12)
        out = ks.k_shift_ref(alloc, off, nb, typ, ne, shift, ks.Rope(64, mode))
        mask = ks.rewritten_mask(len(alloc), off, nb, typ, ne, shift, 64)
        assert mask.sum() == np.count_nonzero(shift) * 2 * ks.rewritten_bytes(typ, 64)
        assert np.array_equal(out[~mask], alloc[~mask]) and not np.array_equal(out[mask], alloc[mask])


@pytest.mark.parametrize("case", sorted(ks.ROTATION_CASES))
def test_f32_restatement_meets_the_derived_tolerance(case):
    """rotate_f32 (the contract in f32) lies within tol() of rotate_f64 on the GPU
    cases' parameters: the bound is attainable before a GPU is involved."""
    ne0, r, ff, big = ks.ROTATION_CASES[case]
    x = _x(ne0, rows=300)
    p = ks.make_shift(300, 1, seed=7, big=big)[0]
    want, got, t = ks.rotate_f64(x, p, r, ff), ks.rotate_f32(x, p, r, ff), ks.tol(x, p, r, ff)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(t, 1e-300)).max())
    print(f"KSHIFT f32-vs-f64 {case}: max err {err.max():.3e}, worst err / tol {worst:.3f}")
    assert (err <= t).all(), (case, worst)
    assert np.array_equal(got[:, r.n_dims:], x[:, r.n_dims:])
    # and the bound is no blanket: a wrong frequency, sign or pairing misses it by orders of magnitude
    wrong = ks.rotate_f64(x, -p, r, ff)
    assert (np.abs(wrong - want) > 1e3 * t)[p != 0].any()


@pytest.mark.parametrize("mode", [ks.NORMAL, ks.NEOX])
def test_shifts_compose(mode):
    """Shift a then shift b is shift a + b (attn_factor 1: the magnitude is kept)."""
    x = _x(128)
    for r, ff in ((ks.Rope(128, mode), None), (ks.Rope(64, mode, freq_base=500000.0), ks.FREQ_FACTORS_64[:32]),
                  (ks.Rope(128, mode, freq_scale=0.25, ext_factor=1.0, n_ctx_orig=4096, attn_factor=1.0 / (1.0 + 0.1 * math.log(4.0))), None)):
        a, b = np.full(len(x), 17), np.full(len(x), -4113)
        two = ks.rotate_f64(ks.rotate_f64(x, a, r, ff), b, r, ff)
        one = ks.rotate_f64(x, a + b, r, ff)
        # (YaRN: attn_factor is an f32, so m * m is 1 only to 2^-23 -- |x| <= 3 * sqrt(2))
        assert np.abs(two - one).max() < (1e-9 if r.ext_factor == 0 else 5 * 2.0 ** -23), (mode, r)


def test_raw_code_rows_hold_ties():
    """The raw-code blocks of the requantisation test: dequantised, a share of
    the Q4_0 / Q5_0 blocks have their largest |x| at both signs."""
    for name in ("q4_0", "q5_0"):
        typ = ks.TYPES[name]
        x = ks.decode(ks.raw_code_rows(typ, 40, 128), typ, 128).reshape(-1, 32)
        a = np.abs(x).max(axis=1, keepdims=True)
        both = ((x == a).any(axis=1) & (x == -a).any(axis=1) & (a[:, 0] > 0))
        assert both.sum() >= 5, (name, int(both.sum()))


def test_harness_k_shift_cpu_only():
    """kernel_test --k-shift --cpu-only: the host's own shift and reference, no GPU touched."""
    r = run_kernel_test(["--k-shift", "-256", "--kv-type", "q8_0", "--rope-mode", "neox", "--cpu-only", "--kv-size", "96",
                         "--heads", "4", "--kv-heads", "2"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k-shift" in r.stdout
