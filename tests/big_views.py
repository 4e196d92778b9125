"""Views at the 32-bit limits of the kernels' buffer descriptors.

Every attention kernel reads Q, K, V and the mask through a raw buffer
descriptor: a 64-bit plane base and a 32-bit byte offset.  The planner accepts a
plane span of up to SPAN_MAX bytes and any nb[2] / nb[3]; a row the kernel has
no use for must then lie PAST the span, in 32 bits.  tests/views.py pads by
bytes to kilobytes; this module lays the same small logical problems out with
strides of tens of MiB to GiB inside one device arena:

  Logical   the tensors of a case as encoded rows (from a problems.Problem, an
            MLA case of tests/mla.py or tests/mla_quant.py)
  layout()  pure integer arithmetic: ne / nb / base of Q, K, V and the mask in
            the arena, the bytes needed, the rows to write (Tensor.shape /
            .strides) -- usable with a fake arena address for host-only planning
  place()   one poison fill per region and one strided copy per tensor into a
            caller-supplied torch.uint8 arena (no per-row loop, no host array of
            the arena's size).  Poison as tests/views.py: 0x7e bytes around K/V,
            f16 0x7e00 around the mask, f32 NaN around Q
  wraps()   the rows past N of a view's last key tile whose 32-bit offset lands
            inside [0, span) again, and whether they land on poison

V lives V_IN_K = 1 MiB behind K where K's strides leave room (inside K's row
padding, or behind K's short planes); Q and the mask follow in regions of their
own.  CASES is the table tests/test_big_views.py plans on the host and
tests/test_gpu_big_views.py runs.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
from numpy.lib.stride_tricks import as_strided

import fattn
from problems import elem_bytes, row_bytes  # noqa: F401

MiB, GiB = 1 << 20, 1 << 30
SPAN_MAX = 0xFFFFFFF0            # fattn_plan.h kSpanMax
ARENA_BYTES = 4608 * MiB         # 4.5 GiB
V_IN_K = MiB
GUARD = 256                      # poison bytes after every region
FAKE_ARENA = 1 << 32             # host-only planning: the arena's "address"
FAKE_DST = 1 << 20
FAR = 4 * GiB + 64 * 1024        # planes more than 4 GiB apart
POISON_KV, POISON_MASK, POISON_Q = 0x7E7E7E7E, 0x7E007E00, 0x7FC00000   # as little-endian dwords

ROW16 = (fattn.TYPE_F16, fattn.TYPE_BF16)


def down16(x: int) -> int:
    return x // 16 * 16


# ------------------------------------------------------------------ logical tensors

@dataclass
class Logical:
    """The tensors of one case, free of any layout."""
    q: np.ndarray                       # f32 [S][NQ][H][Dq]
    k_type: int
    k_rows: np.ndarray                  # u8 [Skv][Hkv][N][row bytes]
    v_type: int
    v_rows: Optional[np.ndarray]        # u8 [Skv][Hkv][N][row bytes]; transposed: [Skv][Hkv][D][2 N]; None: a view of K
    dv: int                             # V's row length (dst's last dim)
    mask: Optional[np.ndarray]          # u16 [ne3][ne2][rows][ne0]
    scale: float
    v_trans: bool = False
    v_off: int = 0                      # V a view of K: bytes into each row

    @property
    def dq(self):
        return self.q.shape[3]

    @property
    def n(self):
        return self.k_rows.shape[2]


def _rows(bytes_, typ, ne, nb):
    D, N, Hkv, Skv = ne
    return np.ascontiguousarray(as_strided(bytes_, shape=(Skv, Hkv, N, row_bytes(typ, D)), strides=(nb[3], nb[2], nb[1], 1)))


def from_problem(prob, mask=None) -> Logical:
    """prob: a problems.Problem in any of its layouts (its rows are gathered).
    mask: u16 [ne3][ne2][rows][ne0] instead of prob.mask_bits (mask planes)."""
    k = _rows(prob.k_bytes, prob.kv_type, prob.kv_ne, prob.k_nb)
    if prob.v_trans:
        D, N, Hkv, Skv = prob.kv_ne
        v = np.ascontiguousarray(as_strided(prob.v_bytes, shape=(Skv, Hkv, D, 2 * N),
                                            strides=(prob.v_nb[3], prob.v_nb[2], prob.v_nb[0], 1)))
    else:
        v = _rows(prob.v_bytes, prob.v_type, prob.kv_ne, prob.v_nb)
    if mask is None and prob.mask_bits is not None:
        mask = np.ascontiguousarray(prob.mask_bits)[None, None]
    return Logical(np.ascontiguousarray(prob.q, dtype=np.float32), prob.kv_type, k, prob.v_type, v, prob.D, mask,
                   prob.scale, prob.v_trans)


def from_mla(launch) -> Logical:
    """launch: a mla.MlaLaunch or mla_quant.QLaunch in its "head" layout, no mask."""
    sh = launch.c.shape
    typ = fattn.TYPE_NAMES[getattr(launch, "type_name", "f16")]
    ne = (fattn.MLA_DK, sh.N, sh.Hkv, sh.Skv)
    k = _rows(launch.k_buf[getattr(launch, "base", 0):], typ, ne, launch.k_nb)
    v = None
    if launch.v_buf is not None:
        v = _rows(launch.v_buf, typ, (fattn.MLA_DV,) + ne[1:], launch.v_nb)
    return Logical(np.ascontiguousarray(launch.q, dtype=np.float32), typ, k, typ, v, fattn.MLA_DV, None,
                   launch.c.ref.scale, False, launch.v_off_bytes or 0)


# ------------------------------------------------------------------ layout

@dataclass
class Tensor:
    name: str            # q | k | v | mask
    type: int
    ne: tuple
    nb: tuple
    base: int            # of the view's first element, bytes into the arena
    shape: Optional[tuple]    # the rows to write: [n3][n2][n1][row bytes] ...
    strides: Optional[tuple]  # ... at these byte strides from base (None: a view of another tensor's rows)
    poison: int
    rows: Optional[np.ndarray] = field(default=None, repr=False)

    @property
    def row(self):
        return self.shape[3]

    @property
    def span(self):
        """One plane's bytes, as the planner counts them (k_span, v_span, m_span; Q: its nb[1] axis alone)."""
        return (self.shape[2] - 1) * self.strides[2] + self.shape[3]

    @property
    def extent(self):
        return sum((n - 1) * s for n, s in zip(self.shape[:3], self.strides[:3])) + self.shape[3]

    def intervals(self):
        """[start, end) of every row written, bytes into the arena."""
        out = []
        for idx in itertools.product(*(range(n) for n in self.shape[:3])):
            s = self.base + sum(i * st for i, st in zip(idx, self.strides[:3]))
            out.append((s, s + self.shape[3]))
        return out


@dataclass
class Layout:
    lg: Logical
    t: dict              # name -> Tensor (no "mask" without one)
    bytes: int           # the arena bytes the layout needs (guards included)

    def intervals(self):
        return sorted(iv for x in self.t.values() if x.shape is not None for iv in x.intervals())

    def params(self, arena_ptr=FAKE_ARENA, dst_ptr=FAKE_DST, ws_ptr=0, ws_bytes=0, kv_chunk=0):
        vw = lambda x: fattn.View(arena_ptr + x.base, x.type, x.ne, x.nb)
        m = self.t.get("mask")
        return fattn.ext_params(vw(self.t["q"]), vw(self.t["k"]), vw(self.t["v"]), vw(m) if m is not None else None,
                                dst_ptr, self.lg.scale, ws_ptr, ws_bytes, kv_chunk)


def _nb3(default, given):
    return tuple(d if g is None else g for d, g in zip(default, given or (None, None, None)))


def layout(lg: Logical, k_nb=None, v_nb=None, q_nb=None, m_nb=None, v_nb0=None, v_in_k=False, row_pad=0) -> Layout:
    """k_nb / v_nb / q_nb / m_nb: (nb1, nb2, nb3) in bytes, None entries (or
    None) for the compact default: rows back to back ([n3][n2][n1], Q in
    ggml's [S][NQ][H]), K / V rows row_pad bytes apart.  v_nb0: the transposed
    V's nb[0].  v_in_k: V's base V_IN_K bytes behind K's (V a view of K sits
    v_off bytes into K's rows whatever this says)."""
    S, NQ, H, Dq = lg.q.shape
    Skv, Hkv, N, rbk = lg.k_rows.shape
    t = {}
    cur = 0

    def region(x: Tensor):
        nonlocal cur
        cur = max(cur, (x.base + x.extent + GUARD + 4095) // 4096 * 4096)

    knb = _nb3((rbk + row_pad, N * (rbk + row_pad), Hkv * N * (rbk + row_pad)), k_nb)
    dk = Dq
    t["k"] = Tensor("k", lg.k_type, (dk, N, Hkv, Skv), (elem_bytes(lg.k_type),) + knb, 0, (Skv, Hkv, N, rbk),
                    (knb[2], knb[1], knb[0], 1), POISON_KV, lg.k_rows)
    region(t["k"])
    v_ne = (lg.dv, N, Hkv, Skv)
    if lg.v_rows is None:
        t["v"] = Tensor("v", lg.v_type, v_ne, t["k"].nb, lg.v_off, None, None, POISON_KV)
    else:
        vb = V_IN_K if v_in_k else cur
        if lg.v_trans:
            nb0 = 2 * N if v_nb0 is None else v_nb0
            vnb = _nb3((2, lg.dv * nb0, Hkv * lg.dv * nb0), v_nb)
            t["v"] = Tensor("v", lg.v_type, v_ne, (nb0,) + vnb, vb, (Skv, Hkv, lg.dv, 2 * N), (vnb[2], vnb[1], nb0, 1),
                            POISON_KV, lg.v_rows)
        else:
            rbv = lg.v_rows.shape[3]
            vnb = _nb3((rbv + row_pad, N * (rbv + row_pad), Hkv * N * (rbv + row_pad)), v_nb)
            t["v"] = Tensor("v", lg.v_type, v_ne, (elem_bytes(lg.v_type),) + vnb, vb, (Skv, Hkv, N, rbv),
                            (vnb[2], vnb[1], vnb[0], 1), POISON_KV, lg.v_rows)
        region(t["v"])
    qnb = _nb3((H * Dq * 4, Dq * 4, NQ * H * Dq * 4), q_nb)
    qrows = np.ascontiguousarray(lg.q.transpose(0, 2, 1, 3)).view(np.uint8).reshape(S, H, NQ, Dq * 4)
    t["q"] = Tensor("q", fattn.TYPE_F32, (Dq, NQ, H, S), (4,) + qnb, cur, (S, H, NQ, Dq * 4), (qnb[2], qnb[1], qnb[0], 1),
                    POISON_Q, qrows)
    region(t["q"])
    if lg.mask is not None:
        ne3, ne2, rows, ne0 = lg.mask.shape
        mnb = _nb3((ne0 * 2, rows * ne0 * 2, ne2 * rows * ne0 * 2), m_nb)
        mrows = np.ascontiguousarray(lg.mask).view(np.uint8).reshape(ne3, ne2, rows, ne0 * 2)
        t["mask"] = Tensor("mask", fattn.TYPE_F16, (ne0, rows, ne2, ne3), (2,) + mnb, cur, (ne3, ne2, rows, ne0 * 2),
                           (mnb[2], mnb[1], mnb[0], 1), POISON_MASK, mrows)
        region(t["mask"])
    return Layout(lg, t, cur)


def overlaps(lay: Layout):
    """Pairs of written rows that share a byte (none in a sound layout)."""
    iv = lay.intervals()
    return [(a, b) for a, b in zip(iv, iv[1:]) if b[0] < a[1]]


# ------------------------------------------------------------------ wrap witnesses

def wraps(lay: Layout, name: str, tile: int):
    """(row, 32-bit byte offset, on_poison) for every row in [N, N rounded up to
    `tile`) of tensor `name` whose offset row * nb[1], taken in 32 bits, lies
    inside [0, span): a kernel that forms it without a row < N guard reads the
    arena there, not zeros.  on_poison: none of the row's bytes (plane 0's) is a
    byte some tensor's row was written to."""
    x = lay.t[name]
    n, nb1 = x.shape[2], x.strides[2]
    iv = lay.intervals()
    out = []
    for r in range(n, (n + tile - 1) // tile * tile):
        off = (r * nb1) & 0xFFFFFFFF
        if off < x.span:
            lo, hi = x.base + off, x.base + off + x.row
            out.append((r, off, not any(a < hi and lo < b for a, b in iv)))
    return out


# ------------------------------------------------------------------ device placement

def place(lay: Layout, arena):
    """Poison every region of the layout, then write every tensor's rows with
    one strided copy.  arena: a torch.uint8 device tensor of at least lay.bytes."""
    import torch
    assert arena.dtype == torch.uint8 and arena.numel() >= lay.bytes and arena.data_ptr() % 16 == 0
    placed = [x for x in lay.t.values() if x.shape is not None]
    for x in placed:
        lo, hi = x.base // 4 * 4, min(arena.numel(), (x.base + x.extent + GUARD + 4095) // 4096 * 4096)
        arena[lo:hi].view(torch.int32).fill_(x.poison)
    for x in placed:
        torch.as_strided(arena, x.shape, x.strides, arena.storage_offset() + x.base).copy_(torch.from_numpy(x.rows).to(arena.device))


DST_GUARD_BYTES = 4096
SENTINEL = 0x5A5AA5A5
WS_TAIL_BYTES = 4096


class BigGpu:
    """A placed Layout on the GPU, as views.GpuView: dst between two 4 KiB
    sentinel bands, the workspace sized exactly with a sentinel tail."""

    def __init__(self, lay: Layout, arena, kv_chunk: int = 0):
        import torch
        dev = arena.device
        S, NQ, H, _ = lay.lg.q.shape
        self.lay, self.out_shape = lay, (S, NQ, H, lay.lg.dv)
        self.n_out = S * NQ * H * lay.lg.dv
        place(lay, arena)
        g = DST_GUARD_BYTES // 4
        self.dst_all = torch.full((g + self.n_out + g,), SENTINEL, dtype=torch.int32, device=dev)
        self.dst = self.dst_all[g:g + self.n_out].view(torch.float32)
        self.p = lay.params(arena.data_ptr(), self.dst.data_ptr(), kv_chunk=kv_chunk)
        self.ws_bytes = fattn.workspace_size(self.p)
        self.ws_all = torch.full(((self.ws_bytes + 3) // 4 + WS_TAIL_BYTES // 4,), SENTINEL, dtype=torch.int32, device=dev)
        if self.ws_bytes:
            self.ws_all.view(torch.uint8)[:self.ws_bytes].zero_()
            self.p.workspace = self.ws_all.data_ptr()
            self.p.workspace_bytes = self.ws_bytes

    def describe(self) -> str:
        return fattn.describe(self.p)

    def run(self) -> np.ndarray:
        import torch
        self.dst.fill_(float("nan"))
        fattn.flash_attn_ext(self.p)
        torch.cuda.synchronize()
        return self.dst.cpu().numpy().reshape(self.out_shape)

    def guards_intact(self) -> bool:
        import torch
        g = DST_GUARD_BYTES // 4
        d = self.dst_all.cpu().numpy().view(np.uint32)
        w = self.ws_all.view(torch.uint8)[self.ws_bytes:].cpu().numpy()
        want = np.full(self.ws_all.numel(), SENTINEL, dtype=np.uint32).view(np.uint8)[self.ws_bytes:]
        return bool((d[:g] == SENTINEL).all() and (d[g + self.n_out:] == SENTINEL).all() and np.array_equal(w, want))


# ------------------------------------------------------------------ the cases

@dataclass(frozen=True)
class Case:
    tag: str
    kind: str                 # std | bf16 | ext | mla | mlaq: where the logical problem and its reference come from
    kw: tuple                 # the problem's arguments, as sorted (name, value) pairs
    big: tuple                # layout() arguments of the big view, as pairs
    kernel: str               # what describe() must contain ...
    avoid: str = ""           # ... and what it must not
    opts: tuple = ()          # ((option, value), ...)
    kv_chunk: int = 0
    twin_pad: int = 0         # the compact twin's row_pad (8: the dword path, layout="padded")
    tile: int = 0             # key tile of the kernel; > 0: the case must have a wrap witness on poison in K
    planes: tuple = (1, 1)    # mask planes (ne2, ne3)
    twin: bool = True         # the compact twin takes the same plan (False: the case is about leaving it)
    status: int = 0           # the planner's answer to the big view (0: FATTN_OK, the case runs)

    @property
    def id(self):
        return self.tag


def _kw(**kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def logical(case: Case):
    """(Logical, reference f32/f64 [S][NQ][H][dv]) of a case, built once."""
    import mla
    import mla_quant
    from problems import make_problem
    kw = dict(case.kw)
    if case.kind == "std":
        if case.planes != (1, 1):
            import mask_planes as mp
            pp = mp.add_planes(make_problem(mask="none", **kw), *case.planes)
            m = pp.mask
            bits = np.ascontiguousarray(as_strided(m.data[m.off:].view(np.uint16), shape=(m.ne[3], m.ne[2], m.ne[1], m.ne[0]),
                                                   strides=(m.nb[3], m.nb[2], m.nb[1], 2)))
            return from_problem(pp.base, bits), pp.oracle()
        p = make_problem(**kw)
        return from_problem(p), p.oracle()
    if case.kind == "bf16":
        import bf16
        import kv_types
        gpu, _ = kv_types.reference_pair("bf16", **kw)
        return from_problem(gpu), bf16.reference_f64(gpu)
    if case.kind == "ext":
        import kv_types
        gpu, ref = kv_types.reference_pair(kw.pop("kv_type"), **kw)
        return from_problem(gpu), ref.oracle()
    sh = mla.Shape(**{k: v for k, v in kw.items() if k in ("H", "Hkv", "NQ", "N", "S", "Skv")})
    if case.kind == "mla":
        c, ref = mla.cached(sh)
        return from_mla(mla.MlaLaunch(c, "head", kw["v_form"])), ref
    c, ref = mla_quant.cached(sh, kw["typ"])
    return from_mla(mla_quant.QLaunch(c, "quant", "head")), ref


def big_layout(case: Case) -> Layout:
    return layout(logical(case)[0], **dict(case.big))


def twin_layout(case: Case) -> Layout:
    return layout(logical(case)[0], row_pad=case.twin_pad)


BAD_STRIDE = -4


def tail_tile(describe: str) -> int:
    """Keys per tile of the kernels whose rows past N the planner keeps from
    wrapping (tile_span, fattn_plan.h): the split kernel's 32-key step; 1 for
    the kernels that guard or never use such rows."""
    return 32 if describe.startswith("fattn_split") else 1


def nb1_for_span(span: int, n: int, row: int, align: int = 16) -> int:
    """The largest nb[1] (a multiple of align) whose n rows of `row` bytes span at most `span`."""
    return (span - row) // (n - 1) // align * align


def _cases():
    O = fattn
    c = []
    in_row = dict(v_in_k=True)                       # V inside K's row padding; heads 4 KiB apart inside the row
    a53 = dict(k_nb=(53 * MiB, 4096, None), v_nb=(53 * MiB, 4096, None), **in_row)
    a40 = dict(k_nb=(40 * MiB, 4096, None), v_nb=(40 * MiB, 4096, None), **in_row)
    a64 = dict(k_nb=(64 * MiB, 4096, None), v_nb=(64 * MiB, 4096, None), **in_row)
    P = lambda **b: tuple(sorted(b.items()))
    one = dict(D=128, NQ=1, H=4, Hkv=4, N=77, mask="none")
    # ---- group A: one plane's span near 4 GiB, the last key tile ragged or partly empty
    for kind, name, pad, seed in (("std", "f16", 0, 11), ("bf16", "bf16", 0, 12), ("std", "q8_0", 8, 13), ("std", "q4_0", 8, 14),
                                  ("ext", "q5_1", 8, 15)):
        kw = _kw(seed=seed, **one, **({} if kind == "bf16" else dict(kv_type=name)))
        kern = f"fattn_split_kernel<{name},{name},D128,gran{4 if pad else 16}"
        # nb[1] = 53 MiB: rows 78 .. 95 of the last 32-key step wrap back inside the descriptor, onto poison; the
        # split kernel has no row guard, so the planner refuses the view (tile_span, fattn_plan.h)
        c.append(Case(f"A-split-{name}-asissue", kind, kw, P(**a53), kern, twin_pad=pad, tile=32, status=BAD_STRIDE))
        # the nearest view it takes: the 96 rows of N rounded up to the step end just inside the limit
        near = nb1_for_span(SPAN_MAX, 96, row_bytes(fattn.TYPE_NAMES[name], 128))
        st = dict(k_nb=(near, 4096, None), v_nb=(near, 4096, None), **in_row)
        c.append(Case(f"A-split-{name}", kind, kw, P(**st), kern, twin_pad=pad))
    c.append(Case("A-split-gqa-f16", "std", _kw(kv_type="f16", D=128, NQ=3, H=8, Hkv=2, N=96, seed=16), P(**a40),
                  "fattn_split_kernel<f16,f16,D128,gran16", kv_chunk=32))
    vt0 = down16((SPAN_MAX - 2 * 96) // 127)
    c.append(Case("A-split-vtrans", "std", _kw(kv_type="f16", D=128, NQ=1, H=2, Hkv=2, N=96, v_trans=True, mask="none", seed=17),
                  P(v_nb0=vt0, v_nb=(None, 4096, None)), "fattn_split_kernel<f16,f16T,D128,gran16"))
    c.append(Case("A-bd-f16", "std", _kw(kv_type="f16", D=128, NQ=64, H=2, Hkv=2, N=96, seed=18), P(**a40),
                  "fattn_bd_kernel<f16,D128", opts=((O.OPT_BD, 2),), tile=128))
    pfk = dict(kv_type="f16", NQ=256, H=2, Hkv=2, N=64)
    c.append(Case("A-pf4-f16-d128", "std", _kw(D=128, seed=19, **pfk), P(**a64), "fattn_pf4_kernel", opts=((O.OPT_PF, 2),)))
    c.append(Case("A-pf-f16-d128", "std", _kw(D=128, seed=19, **pfk), P(**a64), "fattn_pf_kernel<f16,D128",
                  opts=((O.OPT_PF, 2), (O.OPT_PF_FORM, 1))))
    c.append(Case("A-pf-f16-d64", "std", _kw(D=64, seed=20, **pfk), P(**a64), "fattn_pf_kernel<f16,D64", opts=((O.OPT_PF, 2),)))
    # D = 80: the prefill kernel reads its padding dims 2 GiB past the row, outside the descriptor only while the spans stay within 2 GiB
    lo80 = nb1_for_span(1 << 31, 64, 160)
    for tag, nb1, kern, avoid in (("below", lo80, "fattn_pf_kernel<f16,D80", ""), ("above", lo80 + 16, "fattn_", "fattn_pf")):
        st = dict(k_nb=(nb1, 4096, None), v_nb=(nb1, 4096, None), **in_row)
        c.append(Case(f"A-d80-{tag}-2gib", "std", _kw(D=80, seed=21, **pfk), P(**st), kern, avoid, opts=((O.OPT_PF, 2),), twin=not avoid))
    mnb1 = nb1_for_span(SPAN_MAX, 173, 1152)
    for vf in ("view128", "own"):
        st = dict(k_nb=(mnb1, None, None), v_nb=(mnb1, None, None), **in_row)
        c.append(Case(f"A-mla-f16-{vf}", "mla", _kw(H=16, Hkv=1, NQ=1, N=173, v_form=vf), P(**st),
                      "fattn_mla_kernel<f16", tile=32))
    # ---- group B: planes more than 4 GiB apart, rows contiguous
    far2 = dict(k_nb=(None, FAR, None), v_nb=(None, FAR, None), **in_row)
    far3 = dict(k_nb=(None, None, FAR), v_nb=(None, None, FAR), **in_row)
    for i, (kind, kt) in enumerate((("std", "f16"), ("std", "q8_0"), ("ext", "q5_1"), ("bf16", None))):
        name = kt or "bf16"
        t = {} if kt is None else dict(kv_type=kt)
        g = "gran16"
        c.append(Case(f"B-split-row-{name}-nb2", kind, _kw(D=128, NQ=1, H=2, Hkv=2, N=256, seed=30 + i, **t), P(**far2),
                      f"fattn_split_kernel<{name},{name},D128,{g}"))
        c.append(Case(f"B-split-gqa-{name}-nb3", kind, _kw(D=128, NQ=3, H=8, Hkv=2, N=256, S=2, seed=34 + i, **t), P(**far3),
                      f"fattn_split_kernel<{name},{name},D128,{g}"))
    c.append(Case("B-mq-q8_0-nb2", "std", _kw(kv_type="q8_0", D=128, NQ=64, H=4, Hkv=2, N=256, seed=40), P(**far2),
                  "fattn_mq_kernel<q8_0,D128", opts=((O.OPT_MQ_MIN_ROWS, 32), (O.OPT_BD, 1))))
    c.append(Case("B-bd-q8_0-nb2", "std", _kw(kv_type="q8_0", D=128, NQ=64, H=2, Hkv=2, N=256, seed=41), P(**far2),
                  "fattn_bd_kernel<q8_0,D128", opts=((O.OPT_BD, 2),)))
    c.append(Case("B-bdp-q8_0-nb3", "std", _kw(kv_type="q8_0", D=128, NQ=64, H=2, Hkv=2, N=256, S=2, seed=42), P(**far3),
                  "fattn_bdp_kernel<q8_0,D128", opts=((O.OPT_BD, 3),)))
    pfq = dict(D=128, NQ=256, H=2, Hkv=2, N=128)
    c.append(Case("B-pf-q8_0-staged-nb2", "std", _kw(kv_type="q8_0", seed=43, **pfq), P(**far2), "kv_stage_f16<q8_0>",
                  opts=((O.OPT_PF, 2),)))
    c.append(Case("B-pf-q8_0-inkernel-nb2", "std", _kw(kv_type="q8_0", seed=43, **pfq), P(**far2), "fattn_pf_kernel<q8_0,D128",
                  opts=((O.OPT_PF, 2), (O.OPT_PF_STAGE, 1))))
    c.append(Case("B-pf-q5_1-staged-nb3", "ext", _kw(kv_type="q5_1", S=2, seed=44, **pfq), P(**far3), "kv_stage_f16<q5_1>",
                  opts=((O.OPT_PF, 2),)))
    c.append(Case("B-mla-q8_0-nb3", "mlaq", _kw(H=16, Hkv=1, NQ=1, N=172, S=2, Skv=2, typ="q8_0"),
                  P(k_nb=(None, None, FAR)), "fattn_mla_kernel<q8_0"))
    c.append(Case("B-split-merge-launch-nb2", "std", _kw(kv_type="f16", D=128, NQ=3, H=8, Hkv=2, N=800, seed=45), P(**far2),
                  "fattn_split_kernel<f16,f16,D128,gran16", kv_chunk=256))
    c.append(Case("B-split-merge-inlaunch-nb2", "std", _kw(kv_type="q8_0", D=128, NQ=1, H=2, Hkv=2, N=1536, seed=46), P(**far2),
                  "fattn_split_kernel<q8_0,q8_0,D128,gran16", kv_chunk=256))
    # ---- group C: K / V compact, the mask or Q large
    gqa = dict(kv_type="f16", D=128, NQ=3, H=8, Hkv=2, N=96)
    m19 = nb1_for_span(SPAN_MAX, 3, 128 * 2)
    c.append(Case("C-mask-nb1-split", "std", _kw(seed=50, **gqa), P(m_nb=(m19, None, None)), "fattn_split_kernel<f16,f16,D128,gran16"))
    c.append(Case("C-mask-nb1-bd", "std", _kw(kv_type="f16", D=128, NQ=3, H=32, Hkv=2, N=128, seed=51), P(m_nb=(m19, None, None)),
                  "fattn_bd_kernel<f16,D128", opts=((O.OPT_BD, 2),)))
    c.append(Case("C-mask-planes-split", "std", _kw(kv_type="f16", D=128, NQ=1, H=4, Hkv=4, N=96, seed=52),
                  P(m_nb=(None, head_plane_nb2(128 * 2, 1, 4), None)), "mask planes (4,1)", planes=(4, 1)))
    c.append(Case("C-mask-nb3-split", "std", _kw(kv_type="f16", D=128, NQ=3, H=8, Hkv=2, N=96, S=2, seed=53),
                  P(m_nb=(None, None, FAR)), "mask planes (1,2)", planes=(1, 2)))
    qs = (("nb2", dict(q_nb=(None, GiB, None)), {}), ("nb3", dict(q_nb=(None, None, FAR)), dict(S=2)))
    for name, st, extra in qs:
        c.append(Case(f"C-q-{name}-split", "std", _kw(kv_type="f16", D=128, NQ=3, H=4, Hkv=2, N=96, seed=54, **extra), P(**st),
                      "fattn_split_kernel<f16,f16,D128,gran16"))
        c.append(Case(f"C-q-{name}-pf", "std", _kw(kv_type="f16", D=128, NQ=256, H=4, Hkv=2, N=64, seed=55, **extra), P(**st),
                      "fattn_pf4_kernel", opts=((O.OPT_PF, 2),)))
        c.append(Case(f"C-q-{name}-mla", "mla", _kw(H=4, Hkv=1, NQ=3, N=173, v_form="view128", **extra,
                                                     **({"Skv": 2} if extra else {})), P(**st), "fattn_mla_kernel<f16"))
    return c


def head_plane_nb2(m_span: int, extra: int, ne2: int) -> int:
    """The largest mask nb[2] (a multiple of 16) the split kernel's head-plane
    rule accepts: m_span_h + m_span + 64 <= SPAN_MAX, m_span_h = m_span + (ne2 - 1) nb2."""
    return down16((SPAN_MAX - 64 - 2 * m_span) // (ne2 - 1))


CASES = _cases()
