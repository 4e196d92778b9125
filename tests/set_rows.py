"""GGML_OP_SET_ROWS (fattn_set_rows) restated in numpy, and the inputs its tests
share: edge blocks that put ties where a lane-parallel reduction can get them
wrong, cache allocations with guard bytes, and the view builders.

fattn_set_rows gives each 32-element block to eight lanes (lane l: elements
4l .. 4l+3) and merges the lanes' partial scans with a 3-step xor butterfly
(DESIGN.md §14).  ggml's reference scans are sequential with strict compares:
the FIRST element of largest |x| (Q4_0 / Q5_0: the sign of d), the FIRST of
equal minima / maxima with -0.0 == +0.0 (Q4_1 / Q5_1: the sign of a zero m and
of a zero d).  tie_blocks() places such ties inside one lane, in adjacent
lanes, across the two halves, and three ways.

References: oracle.quantize (Q8_0 / Q4_0), kv_types.quantize (Q4_1 / Q5_0 /
Q5_1), numpy astype(float16) (F16).
"""
from __future__ import annotations

import numpy as np

import kv_types as kt
from oracle import oracle as orc
from problems import elem_bytes, row_bytes  # noqa: F401

F = np.float32
QK = 32
TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q8_0 = 0, 1, 2, 8
TYPE_Q4_1, TYPE_Q5_0, TYPE_Q5_1 = 3, 6, 7
TYPE_I32, TYPE_I64 = 26, 27
TYPES = {"f16": TYPE_F16, "q8_0": TYPE_Q8_0, "q4_0": TYPE_Q4_0, "q4_1": TYPE_Q4_1, "q5_0": TYPE_Q5_0,
         "q5_1": TYPE_Q5_1}
BLOCK_BYTES = {TYPE_Q8_0: 34, TYPE_Q4_0: 18, TYPE_Q4_1: 20, TYPE_Q5_0: 22, TYPE_Q5_1: 24}
IDX_DTYPE = {TYPE_I32: np.int32, TYPE_I64: np.int64}


def encode(x: np.ndarray, typ: int) -> np.ndarray:
    """f32 [..., ne0] -> the row bytes [..., row_bytes] the cache must hold."""
    x = np.ascontiguousarray(x, dtype=F)
    if typ == TYPE_F16:
        return x.astype(np.float16).view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * 2,))
    if typ in (TYPE_Q8_0, TYPE_Q4_0):
        return orc.quantize(x, typ).reshape(x.shape[:-1] + (row_bytes(typ, x.shape[-1]),))
    return kt.quantize(x, typ)


# ------------------------------------------------------------------ edge blocks

def _positive(rng) -> np.ndarray:
    return (0.25 + 0.5 * rng.random(QK, dtype=F)).astype(F)


def tie_blocks() -> np.ndarray:
    """f32 [9][32], beyond kv_types.edge_blocks():
      0..3  |max| ties of opposite sign: inside one lane's four elements (4, 6),
            in adjacent lanes (7, 8), across the halves (9, 25), three-way
            (9, 25, 30); the first of them is -, +, -, - (Q5_0 / Q4_0: d of
            sign + - + +)
      4, 5  non-negative blocks whose minimum is a zero tie: +0.0 at element 2
            with -0.0 at 17 (m = 0x0000), and the reverse (m = 0x8000)
      6     all -0.0 (Q4_1 / Q5_1: d = 0x0000, m = 0x8000)
      7, 8  zeros of alternating sign, +0.0 first and -0.0 first"""
    rng = np.random.default_rng(78)
    small = lambda: (0.25 * (1.0 - 2.0 * rng.random(QK, dtype=F))).astype(F)
    b = np.zeros((9, QK), dtype=F)
    b[0] = small(); b[0, 4] = F(-2.5); b[0, 6] = F(2.5)
    b[1] = small(); b[1, 7] = F(2.5); b[1, 8] = F(-2.5)
    b[2] = small(); b[2, 9] = F(-2.5); b[2, 25] = F(2.5)
    b[3] = small(); b[3, 9] = F(-2.5); b[3, 25] = F(2.5); b[3, 30] = F(2.5)
    b[4] = _positive(rng); b[4, 2] = F(0.0); b[4, 17] = F(-0.0)
    b[5] = _positive(rng); b[5, 2] = F(-0.0); b[5, 17] = F(0.0)
    b[6] = F(-0.0)
    b[7, 1::2] = F(-0.0)
    b[8, 0::2] = F(-0.0)
    return b


def all_edge_blocks() -> np.ndarray:
    """kv_types.edge_blocks() (8) followed by tie_blocks() (9): f32 [17][32]."""
    return np.concatenate([kt.edge_blocks(), tie_blocks()], axis=0)


def source_rows(n_rows: int, ne0: int, seed: int = 5) -> np.ndarray:
    """f32 [n_rows][ne0]: every edge block (whole rows, as many as they fill),
    then seeded random rows -- one in three on a coarse grid (multiples of 0.25
    in [-3, 3]), so that ties for the extreme values are the rule there."""
    rng = np.random.default_rng(seed)
    x = (3.0 * (1.0 - 2.0 * rng.random((n_rows, ne0), dtype=F))).astype(F)
    x[2::3] = np.round(x[2::3] * 4.0) / 4.0
    if ne0 % QK == 0:
        e = all_edge_blocks()
        flat = x.reshape(-1, QK)
        n = min(len(e), len(flat))
        flat[:n] = e[:n]
    return x


# ------------------------------------------------------------------ the reference

def set_rows_ref(cache: np.ndarray, src: np.ndarray, idx: np.ndarray, typ: int, n_slots: int, dst_off: int,
                 dst_nb) -> np.ndarray:
    """ggml SET_ROWS over raw bytes, with fattn_set_rows's skip.
      cache  uint8 flat: the whole allocation (left unchanged; a copy is returned)
      src    f32 [ne3][ne2][nr][ne0]
      idx    integer [ne12][ne11][nr]; row i of plane (i2, i3) goes to slot
             idx[i3 % ne12][i2 % ne11][i]; a slot outside [0, n_slots) writes nothing
      dst    the view at byte dst_off with byte strides dst_nb = (nb0, nb1, nb2, nb3)"""
    out = np.array(cache, dtype=np.uint8, copy=True).reshape(-1)
    ne3, ne2, nr, ne0 = src.shape
    ne12, ne11, n_idx = idx.shape
    assert n_idx == nr and ne2 % ne11 == 0 and ne3 % ne12 == 0
    rows = encode(src, typ)
    rb = rows.shape[-1]
    for i3 in range(ne3):
        for i2 in range(ne2):
            for i in range(nr):
                slot = int(idx[i3 % ne12, i2 % ne11, i])
                if not 0 <= slot < n_slots:
                    continue
                o = dst_off + slot * dst_nb[1] + i2 * dst_nb[2] + i3 * dst_nb[3]
                assert 0 <= o and o + rb <= len(out)
                out[o:o + rb] = rows[i3, i2, i]
    return out


# ------------------------------------------------------------------ allocations and views

def cache_alloc(typ: int, ne0: int, n_slots: int, ne2: int, ne3: int = 1, layout: str = "pos", seed: int = 9):
    """A random-filled allocation with the cache view in its middle: at least one
    slot's bytes of guard before, between and after the planes.  Returns
    (bytes uint8 flat, dst_off, dst_nb).
      "pos"   [N][Hkv][row]: nb1 = Hkv * row, nb2 = row; one plane per i3
      "head"  [Hkv][N][row]: nb1 = row, nb2 = N * row + guard; a plane per (i2, i3)"""
    rb = row_bytes(typ, ne0)
    eb = elem_bytes(typ)
    if layout == "pos":
        g = ne2 * rb + 6           # (even, as dst strides must be; the planes need not be dword aligned)
        nb = (eb, ne2 * rb, rb, n_slots * ne2 * rb + g)
    elif layout == "head":
        g = rb + 6
        nb2 = n_slots * rb + g
        nb = (eb, rb, nb2, ne2 * nb2 + g)
    else:
        raise ValueError(layout)
    total = g + ne3 * nb[3] + g
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=total, dtype=np.uint8), g, nb


def place_src(src: np.ndarray, token_major: bool = False, base_off: int = 0, row_pad: int = 0):
    """src f32 [ne3][ne2][nr][ne0] -> (f32 flat buffer, byte offset, nb).
    token_major: memory order [ne3][nr][ne2][ne0], llama.cpp's k_cur seen per
    head; base_off / row_pad: bytes before the first row / after each row
    (multiples of 4; either one off a 16-B multiple forces the dword path)."""
    ne3, ne2, nr, ne0 = src.shape
    assert base_off % 4 == 0 and row_pad % 4 == 0
    stride = ne0 + row_pad // 4
    phys = np.transpose(src, (0, 2, 1, 3)) if token_major else src
    buf = np.full(phys.shape[:3] + (stride,), np.float32(777.0), dtype=F)
    buf[..., :ne0] = phys
    flat = np.concatenate([np.full(base_off // 4, np.float32(-555.0), dtype=F), buf.reshape(-1)])
    a, b = phys.shape[1], phys.shape[2]
    nb_mid = (stride * 4 * b, stride * 4)          # strides of phys dims 1, 2
    nb1, nb2 = (nb_mid[0], nb_mid[1]) if token_major else (nb_mid[1], nb_mid[0])
    return flat, base_off, (4, nb1, nb2, stride * 4 * a * b)


def place_idx(idx: np.ndarray, typ: int, stride0: int = 1, fill: int = -7):
    """idx [ne12][ne11][nr] -> (flat array of the index dtype, ne, nb); stride0:
    elements between consecutive indices (the gaps hold `fill`, an invalid slot)."""
    dt = IDX_DTYPE[typ]
    ne12, ne11, nr = idx.shape
    buf = np.full((ne12, ne11, nr * stride0), fill, dtype=dt)
    buf[..., ::stride0] = idx.astype(dt)
    es = buf.itemsize
    return buf.reshape(-1), (nr, ne11, ne12, 1), (es * stride0, es * nr * stride0, es * nr * stride0 * ne11,
                                                   es * nr * stride0 * ne11 * ne12)


def permuted_slots(n_slots: int, shape, seed: int = 3) -> np.ndarray:
    """int64 `shape` = [ne12][ne11][nr]: per index row the first nr slots of a
    seeded permutation of range(n_slots) (no duplicates within a row)."""
    rng = np.random.default_rng(seed)
    ne12, ne11, nr = shape
    out = np.zeros(shape, dtype=np.int64)
    for a in range(ne12):
        for b in range(ne11):
            out[a, b] = rng.permutation(n_slots)[:nr]
    return out
