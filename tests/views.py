"""View variants of a tests/problems.Problem: the same logical attention problem
with Q, the mask and K/V re-laid as ggml views of larger, poisoned buffers.

include/fattn.h promises the ggml view contract: Q is f32 with any nb whose
nb[0] is 4, the mask has N' >= N columns and rows >= n_q with 4-byte-aligned
rows, K/V take arbitrary nb[1..3], scale is a free float.  make_problem builds
one layout only (contiguous, base at the allocation start); make_view keeps the
logical tensors and changes the addresses:

  Q     q_headmajor   [S][H][NQ][D]: nb1 = row, nb2 = NQ * row
        q_rowpad      row stride D*4 + 16, nb3 padded by one extra row
        q_offset      the view starts 32 B into the allocation
        q_offset4/8   the same by 4 / 8 B (make_plan rejects these)
  mask  m_wide16      nb1 = ne0*2 + 32
        m_rows        ne1 = NQ rounded up to 32 (one more 32 when NQ % 32 == 0)
        m_cols        ne0 = N rounded up to 64, the pad columns poisoned
        m_align4      base offset 4 B
        m_stride4     nb1 = ne0*2 + 4 (nb1 % 16 == 4)
  K/V   kv_ctx        head layout, nb2 = n_ctx * row with n_ctx = N + 96
        kv_offset16   base 16 B into the allocation
        kv_offset4    base 4 B further (the dword path)
        kv_split_layout    K "head" ([Hkv][N]), V "pos" ([N][Hkv])
        kv_split_layout_r  K "pos", V "head"
        kv_pos        both "pos"
        kv_nb3_gap    256 poison bytes between the sequences (Skv = 2)

Every byte outside the view's logical elements is poison: f32 NaN around Q,
f16 NaN (0x7e00) around the mask, 0x7e bytes around K/V (an f16 element and a
Q8_0 / Q4_0 block scale read from them are both the NaN 0x7e7e, at any even
offset).  Variants compose.  exact_f64 is the float64 reference over the logical
tensors.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional

import numpy as np
from numpy.lib.stride_tricks import as_strided

from oracle import oracle as orc
from problems import GUARD, Problem, place_rows, row_bytes, scatter as _scatter  # noqa: F401 (GUARD: this module's users)

Q_VARIANTS = ("q_headmajor", "q_rowpad", "q_offset")
MASK_VARIANTS = ("m_wide16", "m_rows", "m_cols", "m_align4", "m_stride4")
KV_VARIANTS = ("kv_ctx", "kv_offset16", "kv_offset4", "kv_split_layout", "kv_split_layout_r", "kv_pos", "kv_nb3_gap")
ALL_VARIANTS = Q_VARIANTS + ("q_offset4", "q_offset8") + MASK_VARIANTS + KV_VARIANTS
# one composition of every variant (the two split layouts exclude each other)
COMPOSED = Q_VARIANTS + MASK_VARIANTS + ("kv_ctx", "kv_offset16", "kv_offset4", "kv_split_layout", "kv_nb3_gap")
# the composition that keeps every base and stride a multiple of 16 B
COMPOSED16 = Q_VARIANTS + ("m_wide16", "m_rows", "m_cols", "kv_ctx", "kv_offset16", "kv_nb3_gap")

F32_NAN = np.uint32(0x7FC00000)
F16_NAN = np.uint16(0x7E00)
KV_POISON = np.uint8(0x7E)
N_CTX_EXTRA = 96
FAKE_BASE = 1 << 20  # host-only planning: the allocation "address"


@dataclass
class Buf:
    """One tensor as a ggml view of a byte buffer: the view starts `off` bytes in."""
    data: np.ndarray   # flat uint8
    off: int
    type: int
    ne: tuple
    nb: tuple

    def tup(self):
        return (self.data[self.off:], self.type, self.ne, self.nb)


@dataclass
class ViewProblem:
    base: Problem
    variants: tuple
    q: Buf
    k: Buf
    v: Buf
    mask: Optional[Buf]
    scale: float

    def oracle(self, n_threads=8) -> np.ndarray:
        m = self.mask.tup() if self.mask is not None else None
        return orc.flash_attn_ext(self.q.tup(), self.k.tup(), self.v.tup(), m, self.scale, n_threads=n_threads)

    def params(self, ptrs=None, dst_ptr=FAKE_BASE, ws_ptr=0, ws_bytes=0, kv_chunk=0):
        """fattn params.  ptrs: allocation addresses by tensor name (device
        pointers); None = fake 4 KiB-aligned addresses for host-only planning."""
        import fattn
        ptrs = ptrs or {"q": FAKE_BASE, "k": 2 * FAKE_BASE, "v": 3 * FAKE_BASE, "mask": 4 * FAKE_BASE}
        vw = lambda b, n: fattn.View(ptrs[n] + b.off, b.type, b.ne, b.nb)
        return fattn.ext_params(vw(self.q, "q"), vw(self.k, "k"), vw(self.v, "v"),
                                vw(self.mask, "mask") if self.mask is not None else None,
                                dst_ptr, self.scale, ws_ptr, ws_bytes, kv_chunk)


def logical_rows(bytes_: np.ndarray, typ: int, ne, nb) -> np.ndarray:
    """The encoded rows [Skv][Hkv][N][row bytes] of a K or V view (rows contiguous)."""
    D, N, Hkv, Skv = ne
    rb = row_bytes(typ, D)
    return np.ascontiguousarray(as_strided(bytes_, shape=(Skv, Hkv, N, rb), strides=(nb[3], nb[2], nb[1], 1)))


def make_view(prob: Problem, *variants: str, scale: Optional[float] = None) -> ViewProblem:
    """The logical problem of `prob` under the named variants (none: the
    canonical layout, rebuilt through the same code).  scale overrides prob.scale."""
    vs = set(variants)
    unknown = vs - set(ALL_VARIANTS)
    assert not unknown, unknown
    assert not prob.v_trans
    D, NQ, H, S, N, Hkv, Skv = prob.D, prob.NQ, prob.H, prob.S, prob.N, prob.Hkv, prob.Skv

    # ---- Q: logical [S][NQ][H][D] f32
    row = D * 4 + (16 if "q_rowpad" in vs else 0)
    if "q_headmajor" in vs:
        nb1, nb2 = row, NQ * row
        qrows = prob.q.transpose(0, 2, 1, 3)           # [S][H][NQ][D]
        q_strides = lambda nb3: (4, nb1, nb2, nb3)     # (_scatter: innermost row axis first)
    else:
        nb1, nb2 = H * row, row
        qrows = prob.q                                 # [S][NQ][H][D]
        q_strides = lambda nb3: (4, nb2, nb1, nb3)
    nb3 = (NQ * H + (1 if "q_rowpad" in vs else 0)) * row
    q_off = (32 if "q_offset" in vs else 0) + (4 if "q_offset4" in vs else 0) + (8 if "q_offset8" in vs else 0)
    qb = np.ascontiguousarray(qrows, dtype=np.float32).view(np.uint8).reshape(qrows.shape[:3] + (D * 4,))
    q_buf = _scatter(qb, q_strides(nb3), q_off, np.array([F32_NAN]))
    q = Buf(q_buf, q_off, orc.TYPE_F32, (D, NQ, H, S), (4, nb1, nb2, nb3))

    # ---- mask: logical [NQ][ne0] f16 (columns from N on are padding)
    mask = None
    if prob.mask_bits is not None:
        mb = np.array(prob.mask_bits[:NQ], dtype=np.uint16)
        ne0 = mb.shape[1]
        if "m_cols" in vs:
            ne0 = (N + 63) // 64 * 64
            pad = np.full((NQ, ne0), F16_NAN, dtype=np.uint16)
            pad[:, :N] = mb[:, :N]
            mb = pad
        ne1 = NQ
        if "m_rows" in vs:
            ne1 = (NQ // 32 + 1) * 32 if NQ % 32 == 0 else (NQ + 31) // 32 * 32
            pad = np.full((ne1, ne0), F16_NAN, dtype=np.uint16)
            pad[:NQ] = mb
            mb = pad
        m_nb1 = ne0 * 2 + (32 if "m_wide16" in vs else 0) + (4 if "m_stride4" in vs else 0)
        m_off = 4 if "m_align4" in vs else 0
        m_buf = _scatter(mb.view(np.uint8).reshape(1, 1, ne1, ne0 * 2), (2, m_nb1, m_nb1 * ne1, m_nb1 * ne1), m_off,
                         np.array([F16_NAN]))
        mask = Buf(m_buf, m_off, orc.TYPE_F16, (ne0, ne1, 1, 1), (2, m_nb1, m_nb1 * ne1, m_nb1 * ne1))

    # ---- K / V: logical rows [Skv][Hkv][N][row bytes]
    if "kv_nb3_gap" in vs:
        assert Skv == 2, "kv_nb3_gap needs two KV sequences"
    n_ctx = N + (N_CTX_EXTRA if "kv_ctx" in vs else 0)
    kv_off = (16 if "kv_offset16" in vs else 0) + (4 if "kv_offset4" in vs else 0)
    gap = 256 if "kv_nb3_gap" in vs else 0
    k_layout = "pos" if ("kv_split_layout_r" in vs or "kv_pos" in vs) else "head"
    v_layout = "pos" if ("kv_split_layout" in vs or "kv_pos" in vs) else "head"
    assert not ("kv_split_layout" in vs and "kv_split_layout_r" in vs)

    def kv(bytes_, typ, nb_in, layout):
        eb = 2 if typ == orc.TYPE_F16 else orc.BLOCK_BYTES[typ]
        buf, nb = place_rows(logical_rows(bytes_, typ, prob.kv_ne, nb_in), eb, layout, fill=KV_POISON, off=kv_off,
                             n_ctx=n_ctx, gap=gap)
        return Buf(buf, kv_off, typ, prob.kv_ne, nb)

    k = kv(prob.k_bytes, prob.kv_type, prob.k_nb, k_layout)
    v = kv(prob.v_bytes, prob.v_type, prob.v_nb, v_layout)
    return ViewProblem(prob, tuple(variants), q, k, v, mask, float(np.float32(prob.scale if scale is None else scale)))


def swap_kv(vp: ViewProblem, gpu: Problem):
    """vp (or a subclass: mask planes, op params, sinks), built over an F16
    reference problem, with K / V replaced by the cache of `gpu` -- make_view
    cannot lay out a type the oracle does not know."""
    pad = np.full(GUARD, KV_POISON, dtype=np.uint8)
    k = Buf(np.concatenate([gpu.k_bytes, pad]), 0, gpu.kv_type, gpu.kv_ne, gpu.k_nb)
    v = Buf(np.concatenate([gpu.v_bytes, pad]), 0, gpu.v_type, gpu.kv_ne, gpu.v_nb)
    return dataclasses.replace(vp, base=gpu, k=k, v=v)


# ------------------------------------------------------------------ float64 reference

def _h(x: np.ndarray) -> np.ndarray:
    """f32 -> f16 (round to nearest even) -> float64."""
    return orc.f16_bits_to_f32(orc.f32_to_f16_bits(x)).astype(np.float64)


def _decode(bytes_, typ, ne, nb) -> np.ndarray:
    rows = logical_rows(bytes_, typ, ne, nb)
    D = ne[0]
    if typ == orc.TYPE_F16:
        return orc.f16_bits_to_f32(rows.view(np.uint16).reshape(rows.shape[:3] + (D,)))
    return orc.dequantize(rows.reshape(-1, rows.shape[-1]), typ, D).reshape(rows.shape[:3] + (D,))


def exact_f64(prob: Problem, scale: Optional[float] = None) -> np.ndarray:
    """softmax(scale * h(q).h(k)^T + mask) . h(v) in float64 over the logical
    tensors: q rounded to f16, K/V as stored (dequantised, then rounded to f16),
    the f16 mask, scale as its f32 value.  A row whose first N mask entries are
    all -inf is NaN.  Returns [S][NQ][H][D] float64."""
    scale = float(np.float32(prob.scale if scale is None else scale))
    D, NQ, H, S, N, Hkv, Skv = prob.D, prob.NQ, prob.H, prob.S, prob.N, prob.Hkv, prob.Skv
    q = _h(prob.q)                                                      # [S][NQ][H][D]
    k = _h(_decode(prob.k_bytes, prob.kv_type, prob.kv_ne, prob.k_nb))  # [Skv][Hkv][N][D]
    v = _h(_decode(prob.v_bytes, prob.v_type, prob.kv_ne, prob.v_nb))
    m = np.zeros((NQ, N))
    if prob.mask_bits is not None:
        m = orc.f16_bits_to_f32(np.ascontiguousarray(prob.mask_bits[:NQ, :N])).astype(np.float64)
    out = np.empty((S, NQ, H, D), dtype=np.float64)
    rk2, rk3 = H // Hkv, S // Skv
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(S):
            for h in range(H):
                sc = scale * (q[s, :, h, :] @ k[s // rk3, h // rk2].T) + m      # [NQ][N]
                mx = sc.max(axis=1, keepdims=True)
                e = np.exp(sc - mx)                                            # (-inf) - (-inf) = NaN: masked rows
                out[s, :, h, :] = (e / e.sum(axis=1, keepdims=True)) @ v[s // rk3, h // rk2]
    return out


# ------------------------------------------------------------------ GPU runner

def GpuView(vp: ViewProblem, dev="cuda", kv_chunk: int = 0, sinks=None):
    """A ViewProblem on the GPU: its gpu_util.GuardedLaunch (dst guard bands,
    the exactly-sized workspace and its sentinel tail), output [S][NQ][H][D].
    sinks: f32 [H], for a launch through fattn_ext_sinks."""
    import torch

    from gpu_util import GuardedLaunch
    up = lambda a: torch.from_numpy(a).to(dev)
    t = {"q": up(vp.q.data), "k": up(vp.k.data), "v": up(vp.v.data)}
    if vp.mask is not None:
        t["mask"] = up(vp.mask.data)
    ptrs = {n: x.data_ptr() for n, x in t.items()}
    b = vp.base
    return GuardedLaunch(lambda dst: vp.params(ptrs, dst, kv_chunk=kv_chunk), (b.S, b.NQ, b.H, b.D), t, dev, sinks=sinks)
