"""Mask planes on a tests/problems.Problem: the mask of include/fattn.h with
ne[2] head planes and ne[3] sequence planes -- query head iq2 of sequence iq3
reads plane (iq2 % ne[2], iq3 % ne[3]), as ggml's FLASH_ATTN_EXT does.

add_planes takes a Problem built with mask="none" and lays (ne2, ne3) planes of
[NQ][ne0] f16 out as a poisoned view in the style of tests/views.py: f16 NaN
(0x7e00) in every pad column (N .. ne0), in the PLANE_GAP bytes between planes
and in the guard behind the last one.

  order    "sh"  [S'][H'][rows][ne0]: nb2 = plane stride, nb3 = ne2 plane strides
           "hs"  [H'][S'][rows][ne0]: nb3 = plane stride, nb2 = ne3 plane strides
  offset4  the plane stride grows by 4 B (stride % 16 == 4: the 16-B path is off)
  repeat   one stored plane, nb2 = nb3 = 0 (every (iq2, iq3) reads it)

Plane contents (default_planes): each plane U[-1, 1] from its own seed, then
-inf from L_p on, L_p cycling through N, N // 5 + 5, N // 2 + 3; position 0 is
always visible, so no row is NaN.  first="full" starts the cycle at the
full-length plane, first="short" at the shortest: a skip decision or flag table
taken from the wrong plane fails in one order or the other.

The oracle is frozen and broadcasts one plane: PlaneProblem.oracle() calls it
once per (sequence, head) slice with that slice's plane as a 2-D mask and
assembles the result.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import views
from oracle import oracle as orc
from problems import Problem

PLANE_GAP = 256


def plane_lengths(N: int, count: int, first: str = "full"):
    """Live length L_p of plane p (flat index i3 * ne2 + i2)."""
    cyc = (N, N // 5 + 5, N // 2 + 3)
    shift = {"full": 0, "short": 1}[first]
    return [cyc[(p + shift) % 3] for p in range(count)]


def default_planes(prob: Problem, ne2: int, ne3: int, first: str = "full", seed: int = 0) -> np.ndarray:
    """f32 [ne3][ne2][NQ][N]."""
    out = np.empty((ne3, ne2, prob.NQ, prob.N), dtype=np.float32)
    for p, L in enumerate(plane_lengths(prob.N, ne2 * ne3, first)):
        rng = np.random.default_rng(7919 * (seed + 1) + p)
        m = (1.0 - 2.0 * rng.random((prob.NQ, prob.N), dtype=np.float32)).astype(np.float32)
        m[:, max(1, L):] = -np.inf
        out[p // ne2, p % ne2] = m
    return out


@dataclass
class PlaneProblem(views.ViewProblem):
    ne2: int = 1
    ne3: int = 1

    def plane_of(self, iq2: int, iq3: int):
        """(buffer, type, ne, nb) of the plane head iq2 of sequence iq3 reads, as a 2-D mask."""
        m = self.mask
        off = m.off + (iq2 % self.ne2) * m.nb[2] + (iq3 % self.ne3) * m.nb[3]
        span = m.nb[1] * m.ne[1]
        return (m.data[off:], m.type, (m.ne[0], m.ne[1], 1, 1), (2, m.nb[1], span, span))

    def oracle(self, n_threads=4) -> np.ndarray:
        """The broadcasting oracle once per (sequence, head) slice, assembled."""
        b = self.base
        D, NQ, H, S, N = b.D, b.NQ, b.H, b.S, b.N
        rk2, rk3 = H // b.Hkv, S // b.Skv
        out = np.empty((S, NQ, H, D), dtype=np.float32)
        for s in range(S):
            for h in range(H):
                q = (self.q.data[self.q.off + s * self.q.nb[3] + h * self.q.nb[2]:], self.q.type, (D, NQ, 1, 1), self.q.nb)
                kv = []
                for t in (self.k, self.v):
                    o = t.off + (s // rk3) * t.nb[3] + (h // rk2) * t.nb[2]
                    kv.append((t.data[o:], t.type, (D, N, 1, 1), t.nb))
                out[s, :, h, :] = orc.flash_attn_ext(q, kv[0], kv[1], self.plane_of(h, s), self.scale,
                                                     n_threads=n_threads)[0, :, 0, :]
        return out


def add_planes(prob: Problem, ne2: int = 1, ne3: int = 1, order: str = "sh", offset4: bool = False,
               repeat: bool = False, first: str = "full", planes: Optional[np.ndarray] = None,
               variants: tuple = (), seed: int = 0) -> PlaneProblem:
    """prob (mask="none") with a mask of (ne2, ne3) planes.  planes: f32
    [ne3][ne2][NQ][N] contents (default_planes otherwise); with repeat, plane
    [0][0] is stored once.  variants: tests/views.py variants of Q and K/V."""
    assert prob.mask_bits is None, "build the problem with mask='none'"
    assert prob.H % ne2 == 0 and prob.S % ne3 == 0
    assert order in ("sh", "hs")
    NQ, N = prob.NQ, prob.N
    if planes is None:
        planes = default_planes(prob, ne2, ne3, first, seed)
    assert planes.shape == (ne3, ne2, NQ, N), planes.shape
    ne0 = (N + 63) // 64 * 64
    nb1 = ne0 * 2
    stride = NQ * nb1 + PLANE_GAP + (4 if offset4 else 0)
    n_stored = 1 if repeat else ne2 * ne3
    if repeat:
        nb2 = nb3 = 0
    elif order == "sh":
        nb2, nb3 = stride, ne2 * stride
    else:
        nb3, nb2 = stride, ne3 * stride
    total = (n_stored - 1) * stride + NQ * nb1 + views.GUARD
    total = (total + 1) // 2 * 2
    buf = np.full(total // 2, views.F16_NAN, dtype=np.uint16)
    for i3 in range(ne3):
        for i2 in range(ne2):
            if repeat and (i2 or i3):
                continue
            o = (i2 * nb2 + i3 * nb3) // 2
            rows = np.lib.stride_tricks.as_strided(buf[o:], shape=(NQ, N), strides=(nb1, 2), writeable=True)
            rows[...] = orc.f32_to_f16_bits(planes[i3, i2])
    base = views.make_view(prob, *variants)
    mask = views.Buf(buf.view(np.uint8), 0, orc.TYPE_F16, (ne0, NQ, ne2, ne3), (2, nb1, nb2, nb3))
    return PlaneProblem(base.base, base.variants, base.q, base.k, base.v, mask, base.scale, ne2, ne3)


def broadcast_of(pp: PlaneProblem) -> views.ViewProblem:
    """The same problem with plane (0, 0) alone as today's 2-D mask (ne[2] = ne[3] = 1)."""
    m = pp.mask
    span = m.nb[1] * m.ne[1]
    mask = views.Buf(m.data, m.off, m.type, (m.ne[0], m.ne[1], 1, 1), (2, m.nb[1], span, span))
    return views.ViewProblem(pp.base, pp.variants, pp.q, pp.k, pp.v, mask, pp.scale)
