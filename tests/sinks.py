"""Attention sinks (ggml FLASH_ATTN_EXT src[4], fattn_ext_sinks) on a
tests/op_params.OpProblem: the launch side (a SinkProblem carries one f32 sink
per q head; SinkGpuView uploads them and launches through
fattn.flash_attn_ext(p, sinks=...)) and the reference.

The frozen oracle (oracle/) has no sinks.  Appending the sink as an N+1-th
score column to orc.softmax is no usable reference: the oracle rounds P through
f16 in mulmat_f32, and a dominant sink pushes every P into the f16 subnormals
(sink 20 at N = 256: an all-zero output).  The reference is the factor form:

    out[row] = op_params.reference(op)[row] * g,   g = 1 / (1 + exp(s - lse))

with lse the row's log-sum-exp in float64 over the same f32 scores that
op_params.reference builds (scores(): after the cap and slope * mask), s the
raw sink of the row's head (not scaled, capped or sloped), g rounded to f32 and
the product taken in f32.  A row whose scores are all -inf is set to zero
explicitly (ggml: S = 1, VKQ = 0).  A sink of -inf gives g = 1: bit-equal to
op_params.reference.  tests/test_sinks.py pins the factor form to orc.softmax
over N + 1 columns.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
from numpy.lib.stride_tricks import as_strided

import op_params as op
import views
from oracle import oracle as orc


@dataclass
class SinkProblem(op.OpProblem):
    sinks: Optional[np.ndarray] = None   # f32 [H]: this launch's q heads' sinks (None: no sinks)

    def reference(self) -> np.ndarray:
        return reference(self)


def with_sinks(o: op.OpProblem, sinks) -> SinkProblem:
    """o: an op_params.OpProblem (op.one_plane / op.with_params)."""
    s = None if sinks is None else np.ascontiguousarray(sinks, dtype=np.float32)
    assert s is None or s.shape == (o.base.H,), s.shape
    return SinkProblem(o.base, o.variants, o.q, o.k, o.v, o.mask, o.scale, o.ne2, o.ne3, o.max_bias, o.logit_softcap,
                       o.n_head_total, o.head_first, s)


def scores(o: op.OpProblem):
    """Yields (s, h, f32 [NQ][N]): the scores op_params.reference hands to
    orc.softmax -- its steps 1 to 3, statement for statement."""
    b = o.base
    D, NQ, H, S, N = b.D, b.NQ, b.H, b.S, b.N
    rk2, rk3 = H // b.Hkv, S // b.Skv
    K = op._decode(o.k)
    qb = o.q
    qraw = qb.data[qb.off:]
    q = as_strided(qraw[:len(qraw) // 4 * 4].view(np.float32), shape=(S, H, NQ, D), strides=(qb.nb[3], qb.nb[2], qb.nb[1], 4))
    cap = np.float32(o.logit_softcap)
    scale = np.float32(o.scale)
    s_eff = float(scale / cap) if cap > 0 else float(scale)
    sl = op.slopes(o.max_bias, o.n_head_total or H)[o.head_first:o.head_first + H]
    for s in range(S):
        for h in range(H):
            sc = orc.mulmat_f32(np.ascontiguousarray(q[s, h]), K[s // rk3, h // rk2], None, NQ, N, D, s_eff, 1).reshape(NQ, N)
            if cap > 0:
                sc = (float(cap) * np.tanh(sc.astype(np.float64))).astype(np.float32)
            if o.mask is not None:
                mbuf, _, mne, mnb = o.plane_of(h, s)
                rows = as_strided(mbuf.view(np.uint16), shape=(NQ, N), strides=(mnb[1], 2))
                m = orc.f16_bits_to_f32(np.ascontiguousarray(rows))
                with np.errstate(invalid="ignore"):
                    sc = (sc + (sl[h] * m).astype(np.float32)).astype(np.float32)
            yield s, h, sc


def lse_rows(sc: np.ndarray) -> np.ndarray:
    """float64 [rows]: log-sum-exp of f32 score rows; -inf for a row of -inf."""
    x = sc.astype(np.float64)
    m = x.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return m + np.log(np.exp(x - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1))


def factor(lse: np.ndarray, sink: float) -> np.ndarray:
    """g = 1 / (1 + exp(s - lse)) in float64, rounded to f32 (lse = -inf: 0)."""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(np.float64(sink) - lse))).astype(np.float32)


def reference(sp: SinkProblem, sinks=None, plain: Optional[np.ndarray] = None, sc_list=None) -> np.ndarray:
    """f32 [S][NQ][H][D].  sinks: other values than sp.sinks (a capped or a
    mis-sliced array, for the CPU preconditions); plain: op_params.reference(sp)
    and sc_list: list(scores(sp)), when the caller already has them."""
    sk = sp.sinks if sinks is None else np.asarray(sinks, dtype=np.float32)
    out = (op.reference(sp) if plain is None else plain).copy()
    if sk is None:
        return out
    assert sk.shape == (sp.base.H,)
    for s, h, sc in (scores(sp) if sc_list is None else sc_list):
        lse = lse_rows(sc)
        g = factor(lse, sk[h])
        out[s, :, h, :] = out[s, :, h, :] * g[:, None]
        out[s, ~np.isfinite(lse), h, :] = 0.0
    return out


def SinkGpuView(sp: SinkProblem, dev="cuda", kv_chunk: int = 0):
    """views.GpuView (dst guard bands, exactly-sized workspace and its
    sentinel) that uploads the problem's sinks and launches
    fattn.flash_attn_ext(p, sinks=...)."""
    assert sp.sinks is not None
    return views.GpuView(sp, dev, kv_chunk, sinks=sp.sinks)


def run_null_sinks(g) -> np.ndarray:
    """g.run() of a gpu_util.GuardedLaunch with fattn_ext_sinks(p, NULL) through the C ABI itself as the launch."""
    import ctypes as C

    import fattn
    import torch
    g.dst.fill_(float("nan"))
    rc = fattn.lib().fattn_ext_sinks(C.byref(g.p), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return g.dst.cpu().numpy().reshape(g.out_shape)
