"""ggml's Q4_1 / Q5_0 / Q5_1 block formats restated in numpy, and test problems
over caches of these types.

Blocks of 32 values (h() = an f16 field read as f32; every f32 operation is
rounded on its own, as numpy's are):

  Q4_1  20 B  f16 d; f16 m; u8 qs[16]             x = nib * h(d) + h(m)
  Q5_0  22 B  f16 d; u8 qh[4]; u8 qs[16]          x = ((nib | bit << 4) - 16) * h(d)
  Q5_1  24 B  f16 d; f16 m; u8 qh[4]; u8 qs[16]   x = (nib | bit << 4) * h(d) + h(m)

Element j (0..15) is the low nibble of qs[j], element j + 16 the high one; qh
is a little-endian u32 whose bit j is the fifth bit of element j.

Quantisation (ggml's quantize_row_q4_1_ref / _q5_0_ref / _q5_1_ref):
  Q4_1  min, max of the block (sequential scans from +-FLT_MAX with strict
        compares: the first element of the smallest / largest value);
        d = (max - min) / 15, id = d ? 1 / d : 0;
        q = min(15, (int8)((x - min) * id + 0.5))
  Q5_0  mx = the first element of largest |x| (strict <, from amax = 0: an
        all-zero block keeps mx = +0); d = mx / -16; q = min(31, (int8)(x * id + 16.5))
  Q5_1  d = (max - min) / 31; q = (uint8)((x - min) * id + 0.5), no clamp

The frozen oracle (oracle/) knows F16 / Q8_0 / Q4_0 only.  reference_pair()
therefore builds each problem twice over the same logical tensors: `gpu`, whose
K / V are blocks of the new type, and `ref`, whose K / V are F16 views holding
the f16 rounding of dequantize() of the same blocks -- the oracle rounds its
operands to f16 anyway.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable

import numpy as np

import bf16
from gpu_util import check_bars
from oracle import oracle as orc
from problems import LAYOUTS, make_problem, place_rows, row_bytes

F = np.float32
TYPE_Q4_1, TYPE_Q5_0, TYPE_Q5_1 = 3, 6, 7
TYPES = {"q4_1": TYPE_Q4_1, "q5_0": TYPE_Q5_0, "q5_1": TYPE_Q5_1}
BLOCK_BYTES = {TYPE_Q4_1: 20, TYPE_Q5_0: 22, TYPE_Q5_1: 24}
QS_OFF = {TYPE_Q4_1: 4, TYPE_Q5_0: 6, TYPE_Q5_1: 8}
QH_OFF = {TYPE_Q5_0: 2, TYPE_Q5_1: 4}
QK = 32


def _h_bytes(x: np.ndarray) -> np.ndarray:
    """f32 [n] -> f16 (round to nearest even) as bytes [n][2]."""
    return np.ascontiguousarray(x, dtype=F).astype(np.float16).view(np.uint8).reshape(-1, 2)


def _first_of(xb: np.ndarray, val: np.ndarray) -> np.ndarray:
    """Per block, the first element that equals val (-0 == +0): what a scan with strict compares keeps."""
    i = (xb == val[:, None]).argmax(axis=1)
    return xb[np.arange(len(xb)), i]


def quantize(x: np.ndarray, typ: int) -> np.ndarray:
    """f32 [..., D] -> uint8 [..., row_bytes]."""
    x = np.ascontiguousarray(x, dtype=F)
    D = x.shape[-1]
    assert D % QK == 0
    xb = x.reshape(-1, QK)
    n = len(xb)
    out = np.zeros((n, BLOCK_BYTES[typ]), dtype=np.uint8)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if typ == TYPE_Q5_0:
            a = np.abs(xb)
            i = a.argmax(axis=1)   # the first of the largest
            mx = np.where(a.max(axis=1) > 0, xb[np.arange(n), i], F(0.0)).astype(F)
            d = (mx / F(-16.0)).astype(F)
            idv = np.where(d != 0, F(1.0) / d, F(0.0)).astype(F)
            t = ((xb * idv[:, None]).astype(F) + F(16.5)).astype(F)
            q = np.minimum(31, t.astype(np.int8).astype(np.int32))
        else:
            mn = _first_of(xb, xb.min(axis=1))
            mxv = _first_of(xb, xb.max(axis=1))
            d = ((mxv - mn).astype(F) / F(15.0 if typ == TYPE_Q4_1 else 31.0)).astype(F)
            idv = np.where(d != 0, F(1.0) / d, F(0.0)).astype(F)
            t = (((xb - mn[:, None]).astype(F) * idv[:, None]).astype(F) + F(0.5)).astype(F)
            if typ == TYPE_Q4_1:
                q = np.minimum(15, t.astype(np.int8).astype(np.int32))
            else:
                q = t.astype(np.uint8).astype(np.int32)
            out[:, 2:4] = _h_bytes(mn)
    out[:, 0:2] = _h_bytes(d)
    q = q.astype(np.uint32)
    out[:, QS_OFF[typ]:] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    if typ in QH_OFF:
        qh = (((q >> 4) & 1) << np.arange(QK, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint64).astype("<u4")
        out[:, QH_OFF[typ]:QH_OFF[typ] + 4] = qh.view(np.uint8).reshape(n, 4)
    return out.reshape(x.shape[:-1] + (row_bytes(typ, D),))


def codes(blocks: np.ndarray, typ: int):
    """uint8 [n][BB] -> (d f32 [n], m f32 [n] (zeros for Q5_0), codes int32 [n][32])."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    h = lambda b: np.ascontiguousarray(b).view(np.float16).reshape(-1).astype(F)
    d = h(blocks[:, 0:2])
    m = h(blocks[:, 2:4]) if typ != TYPE_Q5_0 else np.zeros(len(blocks), dtype=F)
    qs = blocks[:, QS_OFF[typ]:].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)
    if typ in QH_OFF:
        qh = np.ascontiguousarray(blocks[:, QH_OFF[typ]:QH_OFF[typ] + 4]).view("<u4").reshape(-1).astype(np.int64)
        q = q | ((((qh[:, None] >> np.arange(QK)[None, :]) & 1) << 4).astype(np.int32))
    return d, m, q


def dequantize(rows: np.ndarray, typ: int, D: int) -> np.ndarray:
    """uint8 [..., row_bytes] -> f32 [..., D] (dequantize_row_q4_1 / _q5_0 / _q5_1)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    d, m, q = codes(rows.reshape(-1, BLOCK_BYTES[typ]), typ)
    if typ == TYPE_Q5_0:
        y = ((q - 16).astype(F) * d[:, None]).astype(F)
    else:
        y = ((q.astype(F) * d[:, None]).astype(F) + m[:, None]).astype(F)
    return y.reshape(rows.shape[:-1] + (D,))


# the issue's known-answer block: x[j] = (j - 10) * 0.25
def kat_input() -> np.ndarray:
    return ((np.arange(QK, dtype=F) - F(10.0)) * F(0.25)).astype(F)


def edge_blocks() -> np.ndarray:
    """f32 [8][32]: all zero; all equal; a lone +max at element 0; a lone -max
    at element 31; a -0.0 among other values; a tie for |max| with opposite
    signs (first negative); the same with the positive first; the known-answer
    block."""
    rng = np.random.default_rng(77)
    small = lambda: (0.25 * (1.0 - 2.0 * rng.random(QK, dtype=F))).astype(F)
    b = np.zeros((8, QK), dtype=F)
    b[1] = F(0.7312)
    b[2] = small(); b[2, 0] = F(3.75)
    b[3] = small(); b[3, 31] = F(-3.75)
    b[4] = small(); b[4, 5] = F(-0.0)
    b[5] = small(); b[5, 3] = F(-2.5); b[5, 20] = F(2.5)
    b[6] = small(); b[6, 3] = F(2.5); b[6, 20] = F(-2.5)
    b[7] = kat_input()
    return b


# ------------------------------------------------------------------ the cache types of the GPU suite

@dataclasses.dataclass(frozen=True)
class KvType:
    """A cache type the frozen oracle does not know, as tests/test_gpu_kv_types.py needs it."""
    name: str
    typ: int
    eb: int                  # nb[0]: the bytes of an element or block
    values: Callable         # U[-1, 1] f32 data -> the f32 values handed to encode (identity; BF16: its in-range values)
    encode: Callable         # f32 [..., D] -> row bytes u8 [..., row_bytes]
    decode: Callable         # (row bytes u8 [..., row_bytes], D) -> f32 [..., D], what a kernel reads
    conv_extra: Callable     # (x f32 [64][128]) -> two more rows of conversion input: the type's edge cases
    line: str                # the figure line of a case
    f64: bool                # checked against bf16.reference_f64 as well as against the oracle


def _bf16_extra(x):
    return np.concatenate([bf16.edge_values().reshape(1, 128), (x[:1] * F(2.0 ** 100)).astype(F)])   # (far outside f16's range)


def _quant(name, typ):
    return KvType(name, typ, BLOCK_BYTES[typ], lambda x: x, lambda x: quantize(x, typ), lambda rows, D: dequantize(rows, typ, D),
                  lambda x: edge_blocks().reshape(2, 128), "KVT " + name + " {tag} rel={rel:.3e} elem={elem:.3f} | {desc}", False)


KV_TYPES = {n: _quant(n, t) for n, t in TYPES.items()}
KV_TYPES["bf16"] = KvType("bf16", bf16.TYPE_BF16, 2, bf16.cache_values, bf16.encode_rows,
                          lambda rows, D: bf16.bf16_bits_to_f32(np.ascontiguousarray(rows).view("<u2")), _bf16_extra,
                          "BF16 {tag} vs {what} rel={rel:.3e} elem={elem:.4f} | {desc}", True)


def conv_input(t: KvType) -> np.ndarray:
    """f32 [66][128]: 64 rows of U[-3, 3] and the type's two edge rows."""
    rng = np.random.default_rng(11)
    x = (3.0 * (1.0 - 2.0 * rng.random((64, 128), dtype=F))).astype(F)
    return np.concatenate([x, t.conv_extra(x)], axis=0)


def reference_pair(kv_type: str, layout: str = "head", **kw):
    """(gpu, ref): problems.make_problem(**kw) over a cache of kv_type in `layout`,
    and the same problem over F16 rows (head layout) holding the f16 rounding of
    what a kernel reads from that cache, for the frozen oracle.  Both carry the
    encoded values as k_f32 / v_f32."""
    t = KV_TYPES[kv_type]
    base = make_problem(kv_type="f16", layout="head", **kw)
    D = base.D
    g, r = {}, {}
    for n, x in (("k", base.k_f32), ("v", base.v_f32)):
        x = t.values(x)
        rows = t.encode(x)                                           # [Skv][Hkv][N][rb]
        h16 = orc.f32_to_f16_bits(t.decode(rows, D))                 # [Skv][Hkv][N][D] u16
        (gb, gnb), (rb, rnb) = place_rows(rows, t.eb, *LAYOUTS[layout]), place_rows(h16.view(np.uint8), 2)
        g.update({n + "_bytes": gb, n + "_nb": gnb, n + "_f32": x})
        r.update({n + "_bytes": rb, n + "_nb": rnb, n + "_f32": x})
    return dataclasses.replace(base, kv_type=t.typ, v_type=t.typ, layout=layout, **g), dataclasses.replace(base, **r)


@functools.lru_cache(maxsize=None)
def cached_pair(kv_type: str, layout: str = "head", **kw):
    """(gpu problem, F16 problem, oracle output, float64 output or None), computed once per shape."""
    gpu, ref = reference_pair(kv_type, layout, **kw)
    return gpu, ref, ref.oracle(), bf16.reference_f64(gpu) if KV_TYPES[kv_type].f64 else None


def check(kv_type: str, tag, desc, got, ref, what="oracle(f16 views)"):
    """The suite's bars against one reference, the type's figure line printed first; returns the normwise error."""
    return check_bars(got, ref, lambda rel, elem: KV_TYPES[kv_type].line.format(tag=tag, what=what, rel=rel, elem=elem, desc=desc))[0]


def check_both(kv_type: str, tag, desc, got, oracle, f64):
    """check() against the oracle and, for a type with a float64 reference (f64() -> its output), against that."""
    check(kv_type, tag, desc, got, oracle)
    if KV_TYPES[kv_type].f64:
        return check(kv_type, tag, desc, got, f64() if callable(f64) else f64, "f64")
