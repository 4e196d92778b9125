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

import numpy as np

import views
from oracle import oracle as orc
from problems import Problem, make_problem, row_bytes  # noqa: F401 (row_bytes: this module's users take it from here)

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


def _place(rows: np.ndarray, typ: int, layout: str):
    """rows [Skv][Hkv][N][rb] -> (flat bytes, nb) in problems.make_problem's layouts."""
    Skv, Hkv, N, rb = rows.shape
    eb = 2 if typ == orc.TYPE_F16 else BLOCK_BYTES[typ]
    if layout == "head":
        return np.ascontiguousarray(rows).reshape(-1), (eb, rb, rb * N, rb * N * Hkv)
    if layout == "pos":
        return np.ascontiguousarray(rows.transpose(0, 2, 1, 3)).reshape(-1), (eb, rb * Hkv, rb, rb * N * Hkv)
    if layout == "padded":
        pad = rb + 8
        buf = np.zeros((Skv, Hkv, N, pad), dtype=np.uint8)
        buf[..., :rb] = rows
        return buf.reshape(-1), (eb, pad, pad * N, pad * N * Hkv)
    raise ValueError(layout)


def reference_pair(kv_type: str, layout: str = "head", **kw):
    """(gpu, ref): problems.make_problem(**kw) over a cache of kv_type in `layout`,
    and the same problem over F16 views of the f16-rounded dequantised blocks
    (head layout) for the frozen oracle."""
    typ = TYPES[kv_type]
    base = make_problem(kv_type="f16", layout="head", **kw)
    D = base.D
    out = {}
    for name, x in (("k", base.k_f32), ("v", base.v_f32)):
        blocks = quantize(x, typ)                                    # [Skv][Hkv][N][rb]
        h16 = orc.f32_to_f16_bits(dequantize(blocks, typ, D))        # [Skv][Hkv][N][D] u16
        out[name] = (_place(blocks, typ, layout), _place(h16.view(np.uint8).reshape(h16.shape[:3] + (D * 2,)), orc.TYPE_F16, "head"))
    (kb, knb), (kr, krnb) = out["k"]
    (vb, vnb), (vr, vrnb) = out["v"]
    gpu = dataclasses.replace(base, kv_type=typ, v_type=typ, layout=layout, k_bytes=kb, v_bytes=vb, k_nb=knb, v_nb=vnb)
    ref = dataclasses.replace(base, k_bytes=kr, v_bytes=vr, k_nb=krnb, v_nb=vrnb)
    return gpu, ref


def swap_kv(vp, gpu: Problem):
    """A views.ViewProblem (or a subclass: mask planes, op params, sinks) built
    over the F16 reference problem, with K / V replaced by the blocks of `gpu`
    (views.make_view cannot lay out a type the oracle does not know)."""
    pad = np.full(views.GUARD, views.KV_POISON, dtype=np.uint8)
    k = views.Buf(np.concatenate([gpu.k_bytes, pad]), 0, gpu.kv_type, gpu.kv_ne, gpu.k_nb)
    v = views.Buf(np.concatenate([gpu.v_bytes, pad]), 0, gpu.v_type, gpu.kv_ne, gpu.v_nb)
    return dataclasses.replace(vp, base=gpu, k=k, v=v)
