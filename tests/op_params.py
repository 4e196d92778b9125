"""ggml's max_bias (ALiBi) and logit_softcap on a tests/problems.Problem: the
launch side (an OpProblem carries the four fattn_params fields into the params
that views.GpuView builds) and the reference.

The frozen oracle (oracle/) has neither parameter, so the reference is
assembled from its primitives, per (sequence, head) over the head's query rows
(each output row is computed on its own, exactly as with one row per call):

  1. orc.mulmat_f32(q rows, K, None, NQ, N, D, scale  or  scale / cap, 1)
  2. cap * tanh(.) in float64, rounded to f32           (logit_softcap > 0)
  3. + slope[h] * mask row, in f32                       (a mask present)
  4. orc.softmax
  5. orc.mulmat_f32(P, V, None, NQ, D, N, 1.0, 0)

K and V come through orc.dequantize / orc.f16_bits_to_f32, the slopes from
ggml's host formula in f32.  With both parameters off the result is bit-equal
to the frozen oracle (tests/test_op_params.py pins that), and so it is under
max_bias where slope * mask is exact in f16 and the frozen oracle can run over
pre-multiplied head planes (premultiplied_planes).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from numpy.lib.stride_tricks import as_strided

import mask_planes as mp
import views
from oracle import oracle as orc
from problems import Problem


def slopes(max_bias: float, n_head: int) -> np.ndarray:
    """ggml's ALiBi slopes of heads 0 .. n_head - 1, f32 (ggml_compute_forward_flash_attn_ext:
    m0 = 2^(-max_bias / n2), m1 = 2^(-max_bias / 2 / n2), n2 = 2^floor(log2 n_head))."""
    if max_bias <= 0:
        return np.ones(n_head, dtype=np.float32)
    f = np.float32
    n2 = 1 << (int(n_head).bit_length() - 1)
    m0 = np.power(f(2.0), f(-f(max_bias) / f(n2)))
    m1 = np.power(f(2.0), f(-(f(max_bias) / f(2.0)) / f(n2)))
    out = np.empty(n_head, dtype=np.float32)
    for h in range(n_head):
        out[h] = np.power(m0, f(h + 1)) if h < n2 else np.power(m1, f(2 * (h - n2) + 1))
    return out


def distance_mask(NQ: int, N: int) -> np.ndarray:
    """f32 [NQ][N]: minus the distance to the causal diagonal (query i sits at
    position N - NQ + i), -inf past it.  Integers below 2048: exact in f16, and
    so is a power-of-two slope times them.  Position 0 is visible in every row."""
    m = np.full((NQ, N), -np.inf, dtype=np.float32)
    for i in range(NQ):
        d = N - NQ + i
        m[i, :d + 1] = -(d - np.arange(d + 1, dtype=np.float32))
    return m


def random_mask(NQ: int, N: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(4001 + seed)
    return (1.0 - 2.0 * rng.random((NQ, N), dtype=np.float32)).astype(np.float32)


@dataclass
class OpProblem(mp.PlaneProblem):
    max_bias: float = 0.0
    logit_softcap: float = 0.0
    n_head_total: int = 0
    head_first: int = 0

    def params(self, *args, **kw):
        p = super().params(*args, **kw)
        p.max_bias = self.max_bias
        p.logit_softcap = self.logit_softcap
        p.n_head_total = self.n_head_total
        p.head_first = self.head_first
        return p

    def reference(self) -> np.ndarray:
        return reference(self)


def with_params(vp, max_bias=0.0, logit_softcap=0.0, n_head_total=0, head_first=0) -> OpProblem:
    """vp: a views.ViewProblem or mask_planes.PlaneProblem."""
    return OpProblem(vp.base, vp.variants, vp.q, vp.k, vp.v, vp.mask, vp.scale, getattr(vp, "ne2", 1),
                     getattr(vp, "ne3", 1), float(max_bias), float(logit_softcap), int(n_head_total), int(head_first))


def one_plane(prob: Problem, plane, variants=(), **kw) -> OpProblem:
    """prob (mask="none") under one mask plane f32 [NQ][N] (None: no mask) and the parameters."""
    if plane is None:
        vp = views.make_view(prob, *variants)
        return with_params(vp, **kw)
    return with_params(mp.broadcast_of(mp.add_planes(prob, 1, 1, planes=np.asarray(plane, np.float32)[None, None],
                                                     variants=tuple(variants))), **kw)


def premultiplied_planes(prob: Problem, plane: np.ndarray, max_bias: float, n_head_total=0, head_first=0) -> mp.PlaneProblem:
    """The ALiBi launch the long way: H head planes slope[h] * plane (rounded to
    f16 by add_planes) for the frozen oracle, PlaneProblem.oracle()."""
    sl = slopes(max_bias, n_head_total or prob.H)[head_first:head_first + prob.H]
    planes = (sl[:, None, None] * np.asarray(plane, np.float32)[None]).astype(np.float32)[None]   # [1][H][NQ][N]
    return mp.add_planes(prob, prob.H, 1, planes=planes)


def _decode(buf: views.Buf) -> np.ndarray:
    """K or V view -> f32 [Skv][Hkv][N][D] (orc.dequantize / orc.f16_bits_to_f32)."""
    return views._decode(buf.data[buf.off:], buf.type, buf.ne, buf.nb)


def reference(op: OpProblem) -> np.ndarray:
    """f32 [S][NQ][H][D], assembled from the frozen oracle's primitives (module docstring)."""
    b = op.base
    D, NQ, H, S, N = b.D, b.NQ, b.H, b.S, b.N
    rk2, rk3 = H // b.Hkv, S // b.Skv
    K, V = _decode(op.k), _decode(op.v)
    qb = op.q
    qraw = qb.data[qb.off:]
    q = as_strided(qraw[:len(qraw) // 4 * 4].view(np.float32), shape=(S, H, NQ, D), strides=(qb.nb[3], qb.nb[2], qb.nb[1], 4))
    cap = np.float32(op.logit_softcap)
    scale = np.float32(op.scale)
    s_eff = float(scale / cap) if cap > 0 else float(scale)
    sl = slopes(op.max_bias, op.n_head_total or H)[op.head_first:op.head_first + H]
    assert len(sl) == H
    out = np.empty((S, NQ, H, D), dtype=np.float32)
    for s in range(S):
        for h in range(H):
            k, v = K[s // rk3, h // rk2], V[s // rk3, h // rk2]
            sc = orc.mulmat_f32(np.ascontiguousarray(q[s, h]), k, None, NQ, N, D, s_eff, 1).reshape(NQ, N)
            if cap > 0:
                sc = (float(cap) * np.tanh(sc.astype(np.float64))).astype(np.float32)
            if op.mask is not None:
                mbuf, _, mne, mnb = op.plane_of(h, s)
                rows = as_strided(mbuf.view(np.uint16), shape=(NQ, N), strides=(mnb[1], 2))
                m = orc.f16_bits_to_f32(np.ascontiguousarray(rows))
                with np.errstate(invalid="ignore"):
                    sc = (sc + (sl[h] * m).astype(np.float32)).astype(np.float32)
            p = orc.softmax(sc, N, NQ)
            out[s, :, h, :] = orc.mulmat_f32(p, v, None, NQ, D, N, 1.0, 0).reshape(NQ, D)
    return out
