"""The K-shift (fattn_k_shift: llama.cpp's build_rope_shift, the RoPE rotation of
a K cache in place) restated in numpy, and what its tests share.

The contract (include/fattn.h): for every row (n, h, s) with p = shift[n, s % ns]
    p == 0                       no byte of the row changes
    blocks at or past n_dims     never change (F32 / F16 / BF16: elements at or past n_dims)
    every other block            x = dequantize(row); y = rope(x, p); block = quantize(y)

rotate_f64 is the contract's rotation in float64 over the f32 parameters;
rotate_f32 restates it in f32 in the header's operation order (what a correct
kernel computes up to the ulps of powf / sinf / cosf); k_shift_ref applies it to
raw cache bytes.  The discrete YaRN quantities (the correction dims lo / hi, a
floor and a ceil) are taken in f32 by both, as the library takes them.

tol() is DERIVED, not tuned.  With r = hypot(x0, x1) * m and theta the float64
angle of pair i:

    tol = r * (|theta| * (i + 4) * 2^-23 + 2^-21)

theta_scale carries about one ulp and its i-th power i of them; the other f32
steps of theta (p * pow, / ff, * freq_scale, the YaRN mix) add a few; an angle
error d moves (y0, y1) by r * d.  sin / cos (a few ulps), m and the four
products and one sum add a few ulps of r: 2^-21 is eight of f32's 2^-24.
"""
from __future__ import annotations

import dataclasses

import numpy as np
from numpy.lib.stride_tricks import as_strided

import bf16
import kv_types as kt
import set_rows as sr
from oracle import oracle as orc

F = np.float32
QK = 32
TYPE_F32, TYPE_F16, TYPE_BF16, TYPE_I32 = 0, 1, 30, 26
TYPES = {"f32": TYPE_F32, "f16": TYPE_F16, "bf16": TYPE_BF16, "q8_0": sr.TYPE_Q8_0, "q4_0": sr.TYPE_Q4_0,
         "q4_1": sr.TYPE_Q4_1, "q5_0": sr.TYPE_Q5_0, "q5_1": sr.TYPE_Q5_1}
ELEM_BYTES = {TYPE_F32: 4, TYPE_F16: 2, TYPE_BF16: 2}
NORMAL, NEOX = 0, 2


@dataclasses.dataclass(frozen=True)
class Rope:
    """ggml_rope_ext's parameters (fattn_rope), ggml's defaults."""
    n_dims: int
    mode: int = NEOX
    freq_base: float = 10000.0
    freq_scale: float = 1.0
    ext_factor: float = 0.0
    attn_factor: float = 1.0
    beta_fast: float = 32.0
    beta_slow: float = 1.0
    n_ctx_orig: int = 0

    def c(self):
        import fattn
        return fattn.rope_params(self.n_dims, self.mode, freq_base=self.freq_base, freq_scale=self.freq_scale,
                                 ext_factor=self.ext_factor, attn_factor=self.attn_factor, beta_fast=self.beta_fast,
                                 beta_slow=self.beta_slow, n_ctx_orig=self.n_ctx_orig)


# ------------------------------------------------------------------ rows of every type

def is_block(typ: int) -> bool:
    return typ not in ELEM_BYTES


def row_bytes(typ: int, ne0: int) -> int:
    return ne0 * ELEM_BYTES[typ] if typ in ELEM_BYTES else ne0 // QK * sr.BLOCK_BYTES[typ]


def elem_bytes(typ: int) -> int:
    return ELEM_BYTES.get(typ) or sr.BLOCK_BYTES[typ]


def encode(y: np.ndarray, typ: int) -> np.ndarray:
    """f32 [..., ne0] -> row bytes [..., row_bytes]: what fattn_set_rows / fattn_cpy write for y."""
    y = np.ascontiguousarray(y, dtype=F)
    if typ == TYPE_F32:
        return y.view(np.uint8).reshape(y.shape[:-1] + (y.shape[-1] * 4,))
    if typ == TYPE_BF16:
        return bf16.encode_rows(y)
    return sr.encode(y, typ)


def decode(rows: np.ndarray, typ: int, ne0: int) -> np.ndarray:
    """row bytes [..., row_bytes] -> f32 [..., ne0] (ggml's dequantize_row_*)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    lead = rows.shape[:-1]
    if typ == TYPE_F32:
        return rows.view(F).reshape(lead + (ne0,))
    if typ == TYPE_F16:
        return rows.view(np.float16).astype(F).reshape(lead + (ne0,))
    if typ == TYPE_BF16:
        return bf16.bf16_bits_to_f32(rows.view("<u2")).reshape(lead + (ne0,))
    if typ in (sr.TYPE_Q8_0, sr.TYPE_Q4_0):
        return orc.dequantize(rows, typ, ne0).reshape(lead + (ne0,))
    return kt.dequantize(rows, typ, ne0)


def rewritten_bytes(typ: int, n_dims: int) -> int:
    """The leading bytes of a shifted row that the launch rewrites."""
    return n_dims * ELEM_BYTES[typ] if typ in ELEM_BYTES else (n_dims + QK - 1) // QK * sr.BLOCK_BYTES[typ]


# ------------------------------------------------------------------ the rotation

def corr_dims(r: Rope):
    """(lo, hi) of ggml_rope_yarn_corr_dims, in f32."""
    def corr(b):
        return F(r.n_dims) * np.log(F(r.n_ctx_orig) / (F(b) * F(2.0) * F(np.pi))) / (F(2.0) * np.log(F(r.freq_base)))
    lo = max(F(0.0), np.floor(corr(r.beta_fast)))
    hi = min(F(r.n_dims - 1), np.ceil(corr(r.beta_slow)))
    return F(lo), F(hi)


def angles_f64(r: Rope, p: np.ndarray, ff=None):
    """(theta float64 [..., n_dims / 2], m float64) for position deltas p [...]."""
    i = np.arange(r.n_dims // 2, dtype=np.float64)
    base, fs, ext = float(F(r.freq_base)), float(F(r.freq_scale)), float(F(r.ext_factor))
    te = np.asarray(p, dtype=np.float64)[..., None] * base ** (-2.0 * i / r.n_dims)
    if ff is not None:
        te = te / np.asarray(ff, dtype=F).astype(np.float64)
    theta, m = fs * te, float(F(r.attn_factor))
    if ext != 0.0:
        lo, hi = (float(v) for v in corr_dims(r))
        mix = (1.0 - np.clip((i - lo) / max(0.001, hi - lo), 0.0, 1.0)) * ext
        theta = theta * (1.0 - mix) + te * mix
        m *= 1.0 + 0.1 * np.log(1.0 / fs)
    return theta, m


def _pairs(r: Rope, x: np.ndarray):
    h = r.n_dims // 2
    if r.mode == NEOX:
        return x[..., :h], x[..., h:r.n_dims]
    return x[..., 0:r.n_dims:2], x[..., 1:r.n_dims:2]


def _unpairs(r: Rope, x: np.ndarray, y0, y1) -> np.ndarray:
    out = np.array(x, copy=True)
    h = r.n_dims // 2
    if r.mode == NEOX:
        out[..., :h], out[..., h:r.n_dims] = y0, y1
    else:
        out[..., 0:r.n_dims:2], out[..., 1:r.n_dims:2] = y0, y1
    return out


def rotate_f64(x: np.ndarray, p: np.ndarray, r: Rope, ff=None) -> np.ndarray:
    """x [..., ne0] rotated by the deltas p [...] (broadcast against x's leading dims), in float64."""
    x = np.asarray(x, dtype=np.float64)
    theta, m = angles_f64(r, p, ff)
    x0, x1 = _pairs(r, x)
    c, s = np.cos(theta) * m, np.sin(theta) * m
    return _unpairs(r, x, x0 * c - x1 * s, x0 * s + x1 * c)


def rotate_f32(x: np.ndarray, p: np.ndarray, r: Rope, ff=None) -> np.ndarray:
    """The same in f32, every operation rounded on its own, in the header's order."""
    x = np.asarray(x, dtype=F)
    i = np.arange(r.n_dims // 2, dtype=F)
    theta_scale = np.power(F(r.freq_base), F(-2.0) / F(r.n_dims), dtype=F)
    te = np.asarray(p, dtype=np.int32).astype(F)[..., None] * np.power(theta_scale, i, dtype=F)
    if ff is not None:
        te = te / np.asarray(ff, dtype=F)
    theta, m = F(r.freq_scale) * te, F(r.attn_factor)
    if F(r.ext_factor) != 0:
        lo, hi = corr_dims(r)
        mix = (F(1.0) - np.minimum(F(1.0), np.maximum(F(0.0), (i - lo) / max(F(0.001), hi - lo)))) * F(r.ext_factor)
        theta = theta * (F(1.0) - mix) + te * mix
        m = m * (F(1.0) + F(0.1) * np.log(F(1.0) / F(r.freq_scale)))
    assert theta.dtype == F and np.asarray(m).dtype == F
    c, s = np.cos(theta), np.sin(theta)
    x0, x1 = _pairs(r, x)
    return _unpairs(r, x, x0 * c * m - x1 * s * m, x0 * s * m + x1 * c * m)


def tol(x: np.ndarray, p: np.ndarray, r: Rope, ff=None) -> np.ndarray:
    """float64 [..., ne0]: the module docstring's bound per element (0 for the pass-through elements)."""
    x = np.asarray(x, dtype=np.float64)
    theta, m = angles_f64(r, p, ff)
    x0, x1 = _pairs(r, x)
    i = np.arange(r.n_dims // 2, dtype=np.float64)
    t = np.hypot(x0, x1) * abs(m) * (np.abs(theta) * (i + 4.0) * 2.0 ** -23 + 2.0 ** -21)
    return _unpairs(r, np.zeros_like(x), t, t)


# ------------------------------------------------------------------ caches as raw bytes

def rows_view(alloc: np.ndarray, off: int, nb, typ: int, ne) -> np.ndarray:
    """The view's rows as a strided uint8 view [S][Hkv][n_slots][row_bytes] of the allocation (writeable)."""
    ne0, n_slots, hkv, s = ne
    return as_strided(alloc[off:], shape=(s, hkv, n_slots, row_bytes(typ, ne0)), strides=(nb[3], nb[2], nb[1], 1),
                      writeable=True)


def shift_planes(shift: np.ndarray, s: int) -> np.ndarray:
    """shift int32 [ns][n_slots] -> the delta of every row, [S][1][n_slots] (sequence i3 reads plane i3 % ns)."""
    ns = shift.shape[0]
    assert s % ns == 0
    return shift[np.arange(s) % ns][:, None, :]


def rewritten_mask(alloc_len: int, off: int, nb, typ: int, ne, shift: np.ndarray, n_dims: int) -> np.ndarray:
    """bool [alloc_len]: the bytes a launch may change."""
    mask = np.zeros(alloc_len, dtype=bool)
    v = rows_view(mask.view(np.uint8), off, nb, typ, ne)
    p = np.broadcast_to(shift_planes(shift, ne[3]), v.shape[:3])
    v[..., :rewritten_bytes(typ, n_dims)] = (p != 0)[..., None]
    return mask


def apply_rows(alloc: np.ndarray, off: int, nb, typ: int, ne, shift: np.ndarray, n_dims: int, y: np.ndarray) -> np.ndarray:
    """A copy of the allocation with encode(y) (y f32 [S][Hkv][n_slots][ne0]) in every rewritten block."""
    out = np.array(alloc, dtype=np.uint8, copy=True)
    v = rows_view(out, off, nb, typ, ne)
    new = encode(y, typ)
    nbytes = rewritten_bytes(typ, n_dims)
    sel = np.broadcast_to(shift_planes(shift, ne[3]) != 0, v.shape[:3])
    v[..., :nbytes] = np.where(sel[..., None], new[..., :nbytes], v[..., :nbytes])
    return out


def cache_values(alloc: np.ndarray, off: int, nb, typ: int, ne) -> np.ndarray:
    """f32 [S][Hkv][n_slots][ne0]: the view dequantised."""
    return decode(np.ascontiguousarray(rows_view(alloc, off, nb, typ, ne)), typ, ne[0])


def k_shift_ref(alloc: np.ndarray, off: int, nb, typ: int, ne, shift: np.ndarray, r: Rope, ff=None) -> np.ndarray:
    """fattn_k_shift over raw bytes in numpy: dequantise, rotate_f32, encode; returns the new allocation."""
    x = cache_values(alloc, off, nb, typ, ne)
    y = rotate_f32(x, np.broadcast_to(shift_planes(shift, ne[3]), x.shape[:3]), r, ff)
    return apply_rows(alloc, off, nb, typ, ne, shift, r.n_dims, y)


# ------------------------------------------------------------------ inputs

SHIFTS = np.array([0, 1, -1, 17, -17, 4096, -4096], dtype=np.int32)


def make_shift(n_slots: int, ns: int = 1, seed: int = 1, big: bool = False) -> np.ndarray:
    """int32 [ns][n_slots]: a seeded mix of 0, +-1, +-17, +-4096 (big: +-100000 too); slots 0 and 3 are 0 in plane 0."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([SHIFTS, np.array([100000, -100000], dtype=np.int32)]) if big else SHIFTS
    out = vals[rng.integers(0, len(vals), size=(ns, n_slots))].astype(np.int32)
    out[0, 0] = 0
    out[0, min(3, n_slots - 1)] = 0
    return out


def make_cache(typ: int, ne0: int, n_slots: int, hkv: int, s: int = 1, layout: str = "pos", seed: int = 9, row_pad: int = 0,
               values: np.ndarray = None):
    """(allocation uint8, off, nb): set_rows.cache_alloc's random-filled allocation
    (guard bytes before, between and after the planes; row_pad more bytes behind
    every row) with the rows of the view holding encode(values) -- values f32
    [S][Hkv][n_slots][ne0], seeded U[-3, 3] when None."""
    rb = row_bytes(typ, ne0) + row_pad
    eb = elem_bytes(typ)
    al = 4 if typ == TYPE_F32 else 2
    if layout == "pos":
        g = hkv * rb + (8 if typ == TYPE_F32 else 6)
        nb = (eb, hkv * rb, rb, n_slots * hkv * rb + g)
    elif layout == "head":
        g = rb + (8 if typ == TYPE_F32 else 6)
        nb2 = n_slots * rb + g
        nb = (eb, rb, nb2, hkv * nb2 + g)
    else:
        raise ValueError(layout)
    assert g % al == 0 and all(v % al == 0 for v in nb[1:])
    rng = np.random.default_rng(seed)
    alloc = rng.integers(0, 256, size=g + s * nb[3] + g, dtype=np.uint8)
    if values is None:
        values = (3.0 * (1.0 - 2.0 * rng.random((s, hkv, n_slots, ne0), dtype=F))).astype(F)
    rows_view(alloc, g, nb, typ, (ne0, n_slots, hkv, s))[..., :row_bytes(typ, ne0)] = encode(values, typ)
    return alloc, g, nb


def raw_code_rows(typ: int, n_rows: int, ne0: int, seed: int = 13) -> np.ndarray:
    """Block rows uint8 [n_rows][row_bytes] drawn as raw codes: every qs / qh byte
    uniform, d an f16 in [1/64, 1), m an f16 in (-2, 2).  Dequantised, such
    blocks hold what encoded real data rarely does: |max| ties of opposite sign
    (Q4_0 / Q5_0 blocks without the code 0: -7d against +7d, -15d against +15d)
    and repeated minima / maxima (Q4_1 / Q5_1), where the tie rules decide d's
    sign and the codes."""
    assert is_block(typ)
    rng = np.random.default_rng(seed)
    bb = sr.BLOCK_BYTES[typ]
    n = n_rows * (ne0 // QK)
    blocks = rng.integers(0, 256, size=(n, bb), dtype=np.uint8)
    d = (F(1.0 / 64.0) + rng.random(n, dtype=F) * F(63.0 / 64.0)).astype(np.float16)
    blocks[:, 0:2] = d.view(np.uint8).reshape(n, 2)
    if typ in (sr.TYPE_Q4_1, sr.TYPE_Q5_1):
        m = (F(2.0) * (F(1.0) - F(2.0) * rng.random(n, dtype=F))).astype(np.float16)
        blocks[:, 2:4] = m.view(np.uint8).reshape(n, 2)
    return blocks.reshape(n_rows, ne0 // QK * bb)


FREQ_FACTORS_64 = (1.0 + 7.0 * (np.arange(64, dtype=F) / F(63.0)) ** 2).astype(F)   # llama-3-style: 1 .. 8 over the pairs

# Every (ne0, rope, freq_factors, big shifts) the GPU rotation cases use; tests/test_k_shift.py
# shows on the CPU that rotate_f32 meets tol() on each of them
_YARN = dict(freq_scale=0.25, ext_factor=1.0, n_ctx_orig=4096, beta_fast=32.0, beta_slow=1.0)
ROTATION_CASES = {
    "neox-64": (64, Rope(64, NEOX), None, False),
    "norm-64": (64, Rope(64, NORMAL), None, False),
    "neox-128": (128, Rope(128, NEOX), None, False),
    "norm-128": (128, Rope(128, NORMAL), None, False),
    "neox-256": (256, Rope(256, NEOX), None, False),
    "norm-256": (256, Rope(256, NORMAL), None, False),
    "neox-64of128": (128, Rope(64, NEOX), None, False),
    "norm-64of128": (128, Rope(64, NORMAL), None, False),
    "neox-80of128": (128, Rope(80, NEOX), None, False),       # block 2 straddles n_dims
    "norm-80of128": (128, Rope(80, NORMAL), None, False),
    "neox-128-ff": (128, Rope(128, NEOX, freq_base=500000.0), FREQ_FACTORS_64, False),
    "norm-128-ff": (128, Rope(128, NORMAL, freq_base=500000.0), FREQ_FACTORS_64, False),
    "neox-128-yarn": (128, Rope(128, NEOX, **_YARN), None, False),
    "norm-128-yarn": (128, Rope(128, NORMAL, **_YARN), None, False),
    "neox-128-big": (128, Rope(128, NEOX), None, True),       # shifts of +-100000
    "neox-64-mla": (64, Rope(64, NEOX, attn_factor=0.8, **_YARN), None, False),
}
