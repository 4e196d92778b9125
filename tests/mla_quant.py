"""MLA attention over a Q8_0 / Q4_0 cache (include/fattn.h: K rows of 18 blocks,
V a view of K 0, 1 or 2 whole blocks in) as test problems, on top of
tests/mla.py.

THE CACHE.  N(0, 1) rows of 576 values are quantised with the frozen oracle's
Q8_0 / Q4_0 routines; the LOGICAL K is h(dequantize(blocks)) -- the f16 rounding
of ggml's dequantisation, what the kernel's conversion pass must produce -- and V
is elements [v_off, v_off + 512) of the same rows, v_off = 32 b.  Here the
problem's K IS the cache row (no reordering of dims as in mla.cache_rows), so the
same Case serves the quantised launch and the f16 launch it must equal bit for
bit: an f16 cache holding the logical K, V a view 2 v_off bytes in.

THE REFERENCE is tests/mla.py's: the padded D = 576 problem over the logical K
through ref.oracle() / op_params.reference / sinks.reference.

THE LAUNCH SIDE.  QLaunch lays the rows (f16 or blocks) out as

    layout  "head"   [Skv][Hkv][N][row]        "pos"  [Skv][N][Hkv][row]
            "pad20"  "head" with every row padded by 20 B
            "pad16"  "head" with every row padded by 16 B (Q8_0: a 628-B stride, 4 mod 16)
    base    bytes the view starts into its allocation (4: a base that is no multiple of 16)

with every byte outside the logical rows 0x7e poison: NaN when read as f16 or
as a block's d.
"""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np

import mask_planes as mp
import mla
import op_params as op
import sinks as sk
import views
from mla import DK, DV, SCALE, Shape
from oracle import oracle as orc
from problems import Problem

TYPES = {"q8_0": orc.TYPE_Q8_0, "q4_0": orc.TYPE_Q4_0}
BLOCK = {"q8_0": 34, "q4_0": 18}
ROW = {"f16": DK * 2, "q8_0": 18 * 34, "q4_0": 18 * 18}
LAYOUTS = ("head", "pos", "pad20", "pad16")
PAD = {"head": 0, "pos": 0, "pad20": 20, "pad16": 16}


@functools.lru_cache(maxsize=None)
def cache(sh: Shape, typ: str, seed: int = 0):
    """(blocks u8 [Skv][Hkv][N][row], logical K f32 [Skv][Hkv][N][576], q f32 [S][NQ][H][576])."""
    rng = np.random.default_rng(4421 + seed)
    q = rng.standard_normal((sh.S, sh.NQ, sh.H, DK), dtype=np.float32)
    x = rng.standard_normal((sh.Skv, sh.Hkv, sh.N, DK), dtype=np.float32)
    blocks = orc.quantize(x, TYPES[typ])
    k = orc.f16_bits_to_f32(orc.f32_to_f16_bits(orc.dequantize(blocks, TYPES[typ], DK)))
    for a in (q, blocks, k):
        a.setflags(write=False)
    return blocks, k, q


def padded_problem(sh: Shape, typ: str, v_off: int, seed: int = 0) -> Problem:
    """mla.padded_problem over the logical K of the quantised cache."""
    _, k, q = cache(sh, typ, seed)
    vp = np.zeros(k.shape, dtype=np.float32)
    vp[..., :DV] = k[..., v_off:v_off + DV]
    rb = DK * 2
    nb = (2, rb, rb * sh.N, rb * sh.N * sh.Hkv)
    kb = orc.f32_to_f16_bits(k).view(np.uint8).reshape(-1)
    vb = orc.f32_to_f16_bits(vp).view(np.uint8).reshape(-1)
    return Problem(DK, sh.NQ, sh.H, sh.Hkv, sh.N, sh.S, sh.Skv, orc.TYPE_F16, "head", SCALE, np.array(q), kb, vb, nb, nb, None,
                   False, np.array(k), vp, orc.TYPE_F16)


class QCase(mla.Case):
    """A mla.Case whose K is the logical K of a `typ` cache (v_off in elements: 0, 32, 64)."""
    typ: str
    seed: int


def make_case(sh: Shape, typ: str, mask: str = "none", v_off: int = 64, seed: int = 0, planes: Optional[np.ndarray] = None,
              ne2: int = 1, ne3: int = 1, max_bias: float = 0.0, logit_softcap: float = 0.0, sinks=None) -> QCase:
    """mla.make_case over a quantised cache."""
    assert v_off in (0, 32, 64)
    prob = padded_problem(sh, typ, v_off, seed)
    if planes is not None:
        vp = mp.add_planes(prob, ne2, ne3, planes=np.asarray(planes, np.float32))
        o = op.with_params(vp, max_bias=max_bias, logit_softcap=logit_softcap)
    else:
        o = op.one_plane(prob, mla.make_mask(mask, sh.NQ, sh.N, seed), max_bias=max_bias, logit_softcap=logit_softcap)
    plain = planes is None and max_bias == 0.0 and logit_softcap == 0.0 and sinks is None
    c = QCase(sh, v_off, sk.with_sinks(o, sinks), plain)
    c.typ, c.seed = typ, seed
    return c


@functools.lru_cache(maxsize=None)
def cached(sh: Shape, typ: str, mask: str = "none", v_off: int = 64, seed: int = 0):
    """(case, reference) of a one-plane case without scalars, computed once per process."""
    c = make_case(sh, typ, mask, v_off, seed)
    ref = c.reference()
    ref.setflags(write=False)
    return c, ref


class QLaunch:
    """The fattn params of a QCase: form "quant" (the blocks, V b = v_off / 32
    blocks in) or "f16" (the logical K as f16 rows, V 2 v_off bytes in)."""

    def __init__(self, c: QCase, form: str = "quant", layout: str = "head", base: int = 0):
        assert form in ("quant", "f16") and layout in LAYOUTS
        self.c, self.form, self.layout, self.base = c, form, layout, base
        sh = c.shape
        blocks, k, _ = cache(sh, c.typ, c.seed)
        if form == "quant":
            self.type_name, rows, nb0 = c.typ, blocks, BLOCK[c.typ]
            self.v_off_bytes = c.v_off // 32 * BLOCK[c.typ]
        else:
            self.type_name, nb0 = "f16", 2
            rows = orc.f32_to_f16_bits(k).view(np.uint8).reshape(sh.Skv, sh.Hkv, sh.N, DK * 2)
            self.v_off_bytes = 2 * c.v_off
        self.k_buf, self.k_nb = views.place_rows(rows, nb0, "pos" if layout == "pos" else "head", PAD[layout], views.KV_POISON,
                                                 off=base)
        self.v_buf, self.v_nb = None, self.k_nb
        self.q = np.ascontiguousarray(c.ref.base.q)
        self.q_ne = (DK, sh.NQ, sh.H, sh.S)
        self.q_nb = (4, sh.H * DK * 4, DK * 4, sh.NQ * sh.H * DK * 4)
        self.k_ne = (DK, sh.N, sh.Hkv, sh.Skv)
        self.v_ne = (DV, sh.N, sh.Hkv, sh.Skv)
        self.n_out = sh.S * sh.NQ * sh.H * DV

    def params(self, ptrs=None, ws_ptr=0, ws_bytes=0, kv_chunk=0):
        import fattn
        ptrs = ptrs or mla.FAKE
        r = self.c.ref
        kv = fattn.View(ptrs["k"] + self.base, fattn.TYPE_NAMES[self.type_name], self.k_ne, self.k_nb)
        vv = fattn.mla_v_view(kv, self.c.v_off)
        assert vv.ptr == kv.ptr + self.v_off_bytes
        m = r.mask
        mv = fattn.View(ptrs["mask"] + m.off, m.type, m.ne, m.nb) if m is not None else None
        return fattn.ext_params(fattn.View(ptrs["q"], fattn.TYPE_F32, self.q_ne, self.q_nb), kv, vv, mv, ptrs["dst"],
                                r.scale, ws_ptr, ws_bytes, kv_chunk, max_bias=r.max_bias, logit_softcap=r.logit_softcap,
                                n_head_total=r.n_head_total, head_first=r.head_first)


def QGpu(c: QCase, form="quant", layout="head", base=0, kv_chunk=0, dev="cuda", ws=None, k_tensor=None):
    """mla.gpu_launch over a QLaunch (same dst guard bands, workspace tail and run()).  k_tensor: a device
    buffer that already holds the cache (written on the device), instead of the host-built one."""
    return mla.gpu_launch(QLaunch(c, form, layout, base), kv_chunk, dev, ws, k_tensor)
