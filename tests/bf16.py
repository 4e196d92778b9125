"""BF16 (ggml type 30) in numpy: the f32 -> bf16 rounding rule, test problems
over BF16 caches, a float64 attention reference and an emulation of the split
kernel's bf16 operand roundings.

Rounding (ggml_compute_fp32_to_bf16), on the f32 bits u:

    NaN  (u & 0x7fffffff) > 0x7f800000:  h = (u >> 16) | 64       kept, made quiet
    else                                 h = (u + 0x7fff + ((u >> 16) & 1)) >> 16

round to nearest even on the 16 dropped bits; subnormals are kept, a value past
the largest finite bf16 becomes inf.  bf16 -> f32 is exact: bits << 16.

The frozen oracle (oracle/) knows F16 / Q8_0 / Q4_0 only.  kv_types.reference_pair()
builds each in-range problem twice over the same logical tensors: `gpu`, whose
K / V are bf16 rows, and `ref`, whose K / V are F16 rows of the SAME values --
K / V are bf16 roundings of U[-1, 1] with |x| < 2^-14 set to 0, so every value
has 8 significant bits and a normal f16 exponent: exact in both formats.

The kernel's arithmetic (emulate()): K and V enter the bf16 MFMA exactly; the
f32 B operands -- Q for S^T = K.Q^T, the unnormalised probabilities P for
O^T = V^T.P^T -- enter as hi = bf16(x) and lo = bf16(x - hi), two MFMAs into one
f32 accumulator.  split_q / split_p = False drop the lo part: one bf16 operand.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

import op_params as op
from oracle import oracle as orc
from problems import LAYOUTS, Problem, place_rows

TYPE_BF16 = 30
F = np.float32


# ------------------------------------------------------------------ the format

def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """f32 [...] -> uint16 [...] bf16 bits, the rule of the module docstring."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + (0x7FFF + ((u >> 16) & 1))) >> 16
    return np.where(nan, (u >> 16) | 64, rne).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F)


def round_bf16(x: np.ndarray) -> np.ndarray:
    """f32 -> the f32 value of its bf16 rounding."""
    return bf16_bits_to_f32(f32_to_bf16_bits(x))


def encode_rows(x: np.ndarray) -> np.ndarray:
    """f32 [..., D] -> bf16 row bytes uint8 [..., 2 D] (little endian)."""
    b = f32_to_bf16_bits(x)
    return b.view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * 2,))


def edge_values() -> np.ndarray:
    """f32 [128]: the rule's edge cases (ties both ways, +-0, subnormals, the
    largest finite value, a value that rounds up to inf, +-inf, quiet and
    signalling NaNs of either sign), padded with a ramp."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,
            0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
            0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0x7F80FFFF, 0x7FFFFFFF, 0xFFFFFFFF]
    out = ((np.arange(128, dtype=F) - F(64.0)) * F(0.37)).astype(F)
    out[:len(bits)] = np.array(bits, dtype=np.uint32).view(F)
    return out


# ------------------------------------------------------------------ problems

def cache_values(x: np.ndarray) -> np.ndarray:
    """U[-1, 1] data -> the in-range cache values: bf16 roundings with |x| < 2^-14
    set to 0 (exact in f16 as well)."""
    y = round_bf16(x)
    y[np.abs(y) < F(2.0 ** -14)] = F(0.0)
    assert np.array_equal(orc.f16_bits_to_f32(orc.f32_to_f16_bits(y)), y)
    return y


def over_cache(base: Problem, k: np.ndarray, v: np.ndarray, layout: str = "head", **repl) -> Problem:
    """`base` with K / V replaced by bf16 rows of k / v (f32 [Skv][Hkv][N][D], already bf16 values)."""
    assert np.array_equal(round_bf16(k), k, equal_nan=True) and np.array_equal(round_bf16(v), v, equal_nan=True)
    (kb, knb), (vb, vnb) = place_rows(encode_rows(k), 2, *LAYOUTS[layout]), place_rows(encode_rows(v), 2, *LAYOUTS[layout])
    return dataclasses.replace(base, kv_type=TYPE_BF16, v_type=TYPE_BF16, layout=layout, k_bytes=kb, v_bytes=vb,
                               k_nb=knb, v_nb=vnb, k_f32=k, v_f32=v, **repl)


# ------------------------------------------------------------------ float64 reference

def mask_planes_of(case) -> Optional[np.ndarray]:
    """float64 [S][H][NQ][N]: the mask row every (sequence, head, query row)
    reads, from a problems.Problem (one plane) or a views.ViewProblem / subclass
    (mask planes by (iq2 % ne2, iq3 % ne3)); None without a mask."""
    if isinstance(case, Problem):
        if case.mask_bits is None:
            return None
        m = orc.f16_bits_to_f32(np.ascontiguousarray(case.mask_bits[:case.NQ, :case.N])).astype(np.float64)
        return np.broadcast_to(m, (case.S, case.H) + m.shape)
    if case.mask is None:
        return None
    b = case.base
    out = np.empty((b.S, b.H, b.NQ, b.N))
    mk = case.mask
    ne2, ne3 = getattr(case, "ne2", 1), getattr(case, "ne3", 1)
    for s in range(b.S):
        for h in range(b.H):
            off = mk.off + (h % ne2) * mk.nb[2] + (s % ne3) * mk.nb[3]
            rows = np.lib.stride_tricks.as_strided(mk.data[off:].view(np.uint16), shape=(b.NQ, b.N), strides=(mk.nb[1], 2))
            out[s, h] = orc.f16_bits_to_f32(np.ascontiguousarray(rows))
    return out


def _scores(q, k, mask, scale, cap, slope):
    """float64 [NQ][N]: include/fattn.h's score of one (sequence, head)."""
    s = q @ k.T
    x = cap * np.tanh(s * (scale / cap)) if cap > 0 else s * scale
    if mask is not None:
        with np.errstate(invalid="ignore"):
            x = x + slope * mask
    return x


def reference_f64(case, sinks=None) -> np.ndarray:
    """float64 [S][NQ][H][D]: softmax(score) . V over the logical tensors as the
    kernel is given them -- Q in f32, K / V the cache's values (exact), the f16
    mask planes, scale / max_bias / logit_softcap / head numbering of the case,
    sinks (f32 [H], raw logits joining the denominator) -- every operation in
    float64.  A row masked -inf everywhere is NaN (zeros with sinks)."""
    b = case if isinstance(case, Problem) else case.base
    D, NQ, H, S, N = b.D, b.NQ, b.H, b.S, b.N
    rk2, rk3 = H // b.Hkv, S // b.Skv
    q, k, v = b.q.astype(np.float64), b.k_f32.astype(np.float64), b.v_f32.astype(np.float64)
    scale = float(F(getattr(case, "scale", b.scale)))
    cap = float(F(getattr(case, "logit_softcap", 0.0)))
    max_bias = float(getattr(case, "max_bias", 0.0))
    mask = mask_planes_of(case)
    sl = np.ones(H)
    if max_bias > 0 and mask is not None:
        first = getattr(case, "head_first", 0)
        sl = op.slopes(max_bias, getattr(case, "n_head_total", 0) or H)[first:first + H].astype(np.float64)
    out = np.empty((S, NQ, H, D))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            for h in range(H):
                x = _scores(q[s, :, h, :], k[s // rk3, h // rk2], None if mask is None else mask[s, h], scale, cap, sl[h])
                mx = x.max(axis=1, keepdims=True)
                if sinks is not None:
                    mx = np.maximum(mx, float(sinks[h]))
                e = np.exp(x - mx)
                den = e.sum(axis=1, keepdims=True)
                if sinks is not None:
                    den = den + np.exp(float(sinks[h]) - mx)
                o = (e @ v[s // rk3, h // rk2]) / den
                if sinks is not None:
                    o[~np.isfinite(x).any(axis=1)] = 0.0
                out[s, :, h, :] = o
    return out


# ------------------------------------------------------------------ the kernel's roundings

def _split(x: np.ndarray, both: bool) -> np.ndarray:
    """float64 value of the bf16 operand(s) standing for f32 x: hi (+ lo)."""
    x = x.astype(F)
    hi = round_bf16(x)
    if not both:
        return hi.astype(np.float64)
    lo = round_bf16((x - hi).astype(F))
    return hi.astype(np.float64) + lo.astype(np.float64)


def emulate(prob: Problem, split_q: bool = True, split_p: bool = True) -> np.ndarray:
    """float64 [S][NQ][H][D]: the split kernel's operand roundings over a
    one-plane problem -- K / V exact, Q and the unnormalised P = exp(s - max)
    (f32) as bf16 hi / lo pairs (or hi alone), products and sums exact (the f32
    accumulation error is far below a bf16 operand's), the row sum from the
    unrounded P as in the kernel."""
    b = prob
    rk2, rk3 = b.H // b.Hkv, b.S // b.Skv
    k, v = b.k_f32.astype(np.float64), b.v_f32.astype(np.float64)
    mask = mask_planes_of(b)
    qo = _split(b.q, split_q)
    out = np.empty((b.S, b.NQ, b.H, b.D))
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(b.S):
            for h in range(b.H):
                x = _scores(qo[s, :, h, :], k[s // rk3, h // rk2], None if mask is None else mask[s, h], float(F(b.scale)), 0.0, 1.0)
                p = np.exp(x - x.max(axis=1, keepdims=True)).astype(F)
                out[s, :, h, :] = (_split(p, split_p) @ v[s // rk3, h // rk2]) / p.astype(np.float64).sum(axis=1, keepdims=True)
    return out
