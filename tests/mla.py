"""Multi-head latent attention (include/fattn.h: K rows of 576 f16, V rows of
512 f16 that are a view of the same cache rows) as test problems: the
reference and the launch side.

THE REFERENCE.  The frozen oracle (oracle/) insists on one head dim, but its
output columns are independent: column c of a row is sum_n P[n] * V[n][c].  So
the reference is the oracle over K (576) and V ZERO-PADDED to 576 columns,
keeping output columns [:512].  A case carries that padded problem as a
tests/op_params.OpProblem / tests/sinks.SinkProblem (`ref`), so the scalars, the
mask planes and the sinks go through the very code the other head dims use:

    plain            ref.oracle()[..., :512]           (the frozen oracle itself)
    scalars, planes  op_params.reference(ref)[..., :512]
    sinks            sinks.reference(ref)[..., :512]

tests/test_mla.py pins the padded form to mulmat_f32 -> softmax -> mulmat_f32
over the unpadded V, bit for bit.

Inputs: q and k are N(0, 1), scale = 1 / sqrt(192) -- the model family's (128
nope + 64 rope dims before weight absorption) -- so scores have a standard
deviation of about 1.7.  V is the latent part of K's rows: elements
[v_off, v_off + 512).  Key 0 of every mask row stays finite (the oracle
reproduces the reference's quirk that a row whose FIRST score is -inf is NaN),
except where a test asks for a fully masked row.

THE LAUNCH SIDE.  MlaLaunch lays the same logical rows out as a cache:

    layout  "head"  [Skv][Hkv][N][row]      "pos"  [Skv][N][Hkv][row]
            "pad"   "head" with every row padded by 64 B
    v_form  "view0"   row = latent | rope,  V = K's rows from byte 0
            "view128" row = rope | latent,  V = K's rows from byte 128 (llama.cpp's order)
            "own"     row = rope | latent,  V a second buffer holding the latent (1024-B rows, same layout)

Every byte outside the logical rows is poison (0x7e: f16 NaN).  dst sits inside
a larger tensor with 4 KiB of sentinel on both sides and is compared WHOLE: a
kernel that writes 576 columns per row corrupts the next row or the guard.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import mask_planes as mp
import op_params as op
import sinks as sk
import views
from oracle import oracle as orc
from problems import Problem

DK, DV = 576, 512
SCALE = float(np.float32(1.0 / np.sqrt(np.float32(192.0))))
LAYOUTS = ("head", "pos", "pad")
V_FORMS = ("view0", "view128", "own")
ROW_PAD = 64


@dataclass(frozen=True)
class Shape:
    H: int
    Hkv: int
    NQ: int
    N: int
    S: int = 1
    Skv: int = 1


def _inputs(sh: Shape, v_off: int, seed: int):
    """q f32 [S][NQ][H][576], k f32 [Skv][Hkv][N][576] (f16-representable), v = k[..., v_off:v_off + 512]."""
    rng = np.random.default_rng(9176 + seed)
    q = rng.standard_normal((sh.S, sh.NQ, sh.H, DK), dtype=np.float32)
    k = rng.standard_normal((sh.Skv, sh.Hkv, sh.N, DK), dtype=np.float32)
    k = orc.f16_bits_to_f32(orc.f32_to_f16_bits(k))
    return q, k, np.ascontiguousarray(k[..., v_off:v_off + DV])


def padded_problem(sh: Shape, v_off: int = 64, seed: int = 0) -> Problem:
    """The reference's problem: D = 576 with V zero-padded to 576 columns, no mask."""
    q, k, v = _inputs(sh, v_off, seed)
    vp = np.zeros(k.shape, dtype=np.float32)
    vp[..., :DV] = v
    rb = DK * 2
    nb = (2, rb, rb * sh.N, rb * sh.N * sh.Hkv)
    kb = orc.f32_to_f16_bits(k).view(np.uint8).reshape(-1)
    vb = orc.f32_to_f16_bits(vp).view(np.uint8).reshape(-1)
    return Problem(DK, sh.NQ, sh.H, sh.Hkv, sh.N, sh.S, sh.Skv, orc.TYPE_F16, "head", SCALE, q, kb, vb, nb, nb, None,
                   False, k, vp, orc.TYPE_F16)


# ------------------------------------------------------------------ masks (f32 [NQ][N]; key 0 finite)

def mask_random(NQ: int, N: int, seed: int = 0) -> np.ndarray:
    """U[-1, 1] with about a quarter of the keys -inf, a different set per query row."""
    rng = np.random.default_rng(5003 + seed)
    m = (1.0 - 2.0 * rng.random((NQ, N), dtype=np.float32)).astype(np.float32)
    m[rng.random((NQ, N)) < 0.25] = -np.inf
    m[:, 0] = np.float32(0.25)
    return m


def mask_tail(NQ: int, N: int, seed: int = 0) -> np.ndarray:
    """A padded cache: -inf from about 3/8 of N on, one key later per query row."""
    rng = np.random.default_rng(5011 + seed)
    m = (1.0 - 2.0 * rng.random((NQ, N), dtype=np.float32)).astype(np.float32)
    for i in range(NQ):
        m[i, max(1, 3 * N // 8 + 5 + i):] = -np.inf
    return m


def mask_causal(NQ: int, N: int) -> np.ndarray:
    m = np.zeros((NQ, N), dtype=np.float32)
    for i in range(NQ):
        m[i, N - NQ + i + 1:] = -np.inf
    return m


def mask_zero(NQ: int, N: int) -> np.ndarray:
    return np.zeros((NQ, N), dtype=np.float32)


def make_mask(kind: str, NQ: int, N: int, seed: int = 0) -> Optional[np.ndarray]:
    if kind == "none":
        return None
    return {"random": lambda: mask_random(NQ, N, seed), "tail": lambda: mask_tail(NQ, N, seed),
            "causal": lambda: mask_causal(NQ, N), "zero": lambda: mask_zero(NQ, N)}[kind]()


# ------------------------------------------------------------------ cases

@dataclass
class Case:
    shape: Shape
    v_off: int                    # elements: where the latent starts in a K row (0 or 64)
    ref: sk.SinkProblem           # the padded D = 576 problem with mask planes, scalars and sinks
    plain: bool                   # no scalars, one plane, no sinks: the frozen oracle is the reference

    def reference(self) -> np.ndarray:
        """f32 [S][NQ][H][512]."""
        if self.plain:
            full = views.ViewProblem.oracle(self.ref)
        else:
            full = sk.reference(self.ref)   # (no sinks: op_params.reference)
        return np.ascontiguousarray(full[..., :DV])


def make_case(sh: Shape, mask: str = "none", v_off: int = 64, seed: int = 0, planes: Optional[np.ndarray] = None,
              ne2: int = 1, ne3: int = 1, max_bias: float = 0.0, logit_softcap: float = 0.0, sinks=None) -> Case:
    """mask: a make_mask kind for one plane, or `planes` f32 [ne3][ne2][NQ][N]."""
    prob = padded_problem(sh, v_off, seed)
    if planes is not None:
        vp = mp.add_planes(prob, ne2, ne3, planes=np.asarray(planes, np.float32))
        o = op.with_params(vp, max_bias=max_bias, logit_softcap=logit_softcap)
    else:
        o = op.one_plane(prob, make_mask(mask, sh.NQ, sh.N, seed), max_bias=max_bias, logit_softcap=logit_softcap)
    plain = planes is None and max_bias == 0.0 and logit_softcap == 0.0 and sinks is None
    return Case(sh, v_off, sk.with_sinks(o, sinks), plain)


@functools.lru_cache(maxsize=None)
def cached(sh: Shape, mask: str = "none", v_off: int = 64, seed: int = 0):
    """(case, reference) of a one-plane case without scalars, computed once per process."""
    c = make_case(sh, mask, v_off, seed)
    ref = c.reference()
    ref.setflags(write=False)
    return c, ref


def unpadded_reference(c: Case) -> np.ndarray:
    """mulmat_f32 -> softmax -> mulmat_f32 (oracle.py) over K (576) and the
    UNPADDED V (512), per (sequence, head): what the padded form must equal."""
    b = c.ref.base
    sh = c.shape
    K = b.k_f32
    V = np.ascontiguousarray(b.v_f32[..., :DV])
    out = np.empty((sh.S, sh.NQ, sh.H, DV), dtype=np.float32)
    rk2, rk3 = sh.H // sh.Hkv, sh.S // sh.Skv
    for s in range(sh.S):
        for h in range(sh.H):
            m = None
            if c.ref.mask is not None:
                mbuf, _, _, mnb = c.ref.plane_of(h, s)
                rows = np.lib.stride_tricks.as_strided(mbuf.view(np.uint16), shape=(sh.NQ, sh.N), strides=(mnb[1], 2))
                m = orc.f16_bits_to_f32(np.ascontiguousarray(rows))
            for i in range(sh.NQ):   # (mulmat_f32 takes ONE mask row for all of its rows: one query row per call)
                sc = orc.mulmat_f32(np.ascontiguousarray(b.q[s, i, h, :]), K[s // rk3, h // rk2], None if m is None else m[i],
                                    1, sh.N, DK, SCALE, 1)
                p = orc.softmax(sc, sh.N, 1)
                out[s, i, h, :] = orc.mulmat_f32(p, V[s // rk3, h // rk2], None, 1, DV, sh.N, 1.0, 0)
    return out


# ------------------------------------------------------------------ the launch side

def cache_rows(c: Case, v_form: str):
    """(K rows u8 [Skv][Hkv][N][1152], V rows u8 [Skv][Hkv][N][1024] or None, v byte offset or None)."""
    b = c.ref.base
    k, v = b.k_f32, np.ascontiguousarray(b.v_f32[..., :DV])
    rest = np.concatenate([k[..., :c.v_off], k[..., c.v_off + DV:]], axis=-1)   # the 64 RoPE dims
    if v_form == "view0":
        row, voff = np.concatenate([v, rest], axis=-1), 0
    else:
        row, voff = np.concatenate([rest, v], axis=-1), 2 * (DK - DV)
    return row, (v if v_form == "own" else None), (None if v_form == "own" else voff)


def logical_q(c: Case, v_form: str) -> np.ndarray:
    """Q with its dims in the cache row's order (the latent's dims where the latent sits)."""
    q = c.ref.base.q
    lat, rest = q[..., c.v_off:c.v_off + DV], np.concatenate([q[..., :c.v_off], q[..., c.v_off + DV:]], axis=-1)
    return np.ascontiguousarray(np.concatenate([lat, rest] if v_form == "view0" else [rest, lat], axis=-1))


def f16_cache(rows_f32: np.ndarray, layout: str):
    """f32 rows [Skv][Hkv][N][d] -> (poisoned u8 buffer, nb) of f16 rows in `layout`."""
    rows = orc.f32_to_f16_bits(rows_f32).view(np.uint8).reshape(rows_f32.shape[:3] + (rows_f32.shape[3] * 2,))
    return views.place_rows(rows, 2, "pos" if layout == "pos" else "head", ROW_PAD if layout == "pad" else 0, views.KV_POISON)


FAKE = {"q": 1 << 20, "k": 2 << 20, "v": 3 << 20, "mask": 4 << 20, "dst": 5 << 20}


class MlaLaunch:
    """The fattn params of a Case under (layout, v_form); ptrs: allocation
    addresses by name (device pointers), None: fake aligned ones for host-only planning."""

    def __init__(self, c: Case, layout: str = "head", v_form: str = "view128"):
        assert layout in LAYOUTS and v_form in V_FORMS
        self.c, self.layout, self.v_form = c, layout, v_form
        sh = c.shape
        krows, vrows, self.v_off_bytes = cache_rows(c, v_form)
        self.k_buf, self.k_nb = f16_cache(krows, layout)
        self.v_buf, self.v_nb = f16_cache(vrows, layout) if vrows is not None else (None, self.k_nb)
        self.q = logical_q(c, v_form)
        self.q_ne = (DK, sh.NQ, sh.H, sh.S)
        self.q_nb = (4, sh.H * DK * 4, DK * 4, sh.NQ * sh.H * DK * 4)
        self.k_ne = (DK, sh.N, sh.Hkv, sh.Skv)
        self.v_ne = (DV, sh.N, sh.Hkv, sh.Skv)
        self.n_out = sh.S * sh.NQ * sh.H * DV

    def params(self, ptrs=None, ws_ptr=0, ws_bytes=0, kv_chunk=0):
        import fattn
        ptrs = ptrs or FAKE
        r = self.c.ref
        kv = fattn.View(ptrs["k"], fattn.TYPE_F16, self.k_ne, self.k_nb)
        if self.v_form == "own":
            vv = fattn.View(ptrs["v"], fattn.TYPE_F16, self.v_ne, self.v_nb)
        else:
            vv = fattn.mla_v_view(kv, self.v_off_bytes // 2)
        m = r.mask
        mv = fattn.View(ptrs["mask"] + m.off, m.type, m.ne, m.nb) if m is not None else None
        return fattn.ext_params(fattn.View(ptrs["q"], fattn.TYPE_F32, self.q_ne, self.q_nb), kv, vv, mv, ptrs["dst"],
                                r.scale, ws_ptr, ws_bytes, kv_chunk, max_bias=r.max_bias, logit_softcap=r.logit_softcap,
                                n_head_total=r.n_head_total, head_first=r.head_first)


def gpu_launch(L, kv_chunk=0, dev="cuda", ws=None, k_tensor=None):
    """L (an MlaLaunch or a mla_quant.QLaunch) on the GPU: its
    gpu_util.GuardedLaunch -- dst [S][NQ][H][512] between the sentinel bands, the
    exactly-sized workspace with its sentinel tail or `ws`, a shared one.
    k_tensor: a device buffer that already holds the K cache, instead of L's."""
    import torch

    from gpu_util import GuardedLaunch
    r, sh = L.c.ref, L.c.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {"q": up(L.q.reshape(-1).view(np.uint8)), "k": up(L.k_buf) if k_tensor is None else k_tensor}
    if L.v_buf is not None:
        t["v"] = up(L.v_buf)
    if r.mask is not None:
        t["mask"] = up(r.mask.data)
    ptrs = {n: x.data_ptr() for n, x in t.items()}
    return GuardedLaunch(lambda dst: L.params(dict(ptrs, dst=dst), kv_chunk=kv_chunk), (sh.S, sh.NQ, sh.H, DV), t, dev,
                         sinks=r.sinks, ws=ws)


def MlaGpu(c: Case, layout="head", v_form="view128", kv_chunk=0, dev="cuda", ws=None):
    return gpu_launch(MlaLaunch(c, layout, v_form), kv_chunk, dev, ws)
