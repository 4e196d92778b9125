"""The row log-sum-exp (fattn_ext_lse) and the merge of KV-sharded partials
(fattn_lse_merge): the launch side, the float64 references and the bar.

THE LAUNCH SIDE.  LseLaunch is a gpu_util.GuardedLaunch with an `lse` buffer of
its own: f32 [S][n_q][H], NaN-pre-filled, between 4 KiB sentinel bands; its
launch passes lse= (with_lse = False: the launch without it, over the same
buffers).  LseLaunch.of(g) adopts the launch any of the suites' builders made
(views.GpuView, mla.MlaGpu, mla_quant.QGpu).

THE REFERENCES, in float64:
  lse_ref(o, sinks)     log-sum-exp of the rows of sinks.scores(o) -- the f32
                        scores the assembled reference hands to orc.softmax,
                        after the cap and slope * mask --, logaddexp with the
                        raw sink where sinks are live; -inf for a row of -inf
  lse_ref(o, f64=True)  the same over scores64(o, round_q=False): a float64
                        product of Q as given (f32) and the cache's values, for
                        BF16 caches -- the oracle's f16 rounding of Q is not what
                        the hi / lo operands compute
  merge_ref             fattn_lse_merge's rule (include/fattn.h)

THE BAR.  The reference's own uncertainty is the distance between lse_ref(o)
and the log-sum-exp over scores64(o): the same f16-rounded operands, the
product in float64 instead of orc.mulmat_f32's f32 accumulation.  REF_WORST is
that distance measured over every case of tests/test_gpu_lse.py (suite_ops();
`python tests/lse.py` prints it), LSE_ATOL = 8 x REF_WORST: the margin covers
v_exp_f32 / v_log_f32 at about one ulp each, the kernels' other summation order
over D and over N, and the chunk merges.  The check is

    |lse_gpu - lse_ref| <= LSE_ATOL + 4 ulp_f32(|lse_ref|)

(ALiBi rows reach log-sum-exps in the hundreds); -inf positions coincide exactly.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
from numpy.lib.stride_tricks import as_strided

import op_params as op
import sinks as sk
import views
from gpu_util import DST_GUARD_BYTES, SENTINEL, GuardedLaunch

# worst |lse over orc.mulmat_f32's scores - lse over the float64 product| of the GPU suite's cases (CPU, `python tests/lse.py`)
REF_WORST = 2.315e-6   # (mla-f16-view-decode-n160; every D <= 256 case is below 1.3e-7)
LSE_ATOL = 8 * REF_WORST


# ------------------------------------------------------------------ the launch side

class LseLaunch(GuardedLaunch):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._init_lse()

    @classmethod
    def of(cls, g: GuardedLaunch) -> "LseLaunch":
        """g (built by any of the suites' builders) with an lse buffer of its own."""
        obj = cls.__new__(cls)
        obj.__dict__.update(g.__dict__)
        obj._init_lse()
        return obj

    def _init_lse(self):
        import torch
        self.n_rows = self.n_out // self.out_shape[-1]
        g = DST_GUARD_BYTES // 4
        self.lse_all = torch.full((g + self.n_rows + g,), SENTINEL, dtype=torch.int32, device=self.dst.device)
        self.lse = self.lse_all[g:g + self.n_rows].view(torch.float32)
        self.lse.fill_(float("nan"))
        self.with_lse = True

    def launch(self, stream=None):
        import fattn
        fattn.flash_attn_ext(self.p, stream, sinks=self.sinks_t, lse=self.lse if self.with_lse else None)

    def run(self) -> np.ndarray:
        self.lse.fill_(float("nan"))
        return super().run()

    def run_without(self) -> np.ndarray:
        """run() of the launch without lse: dst alone (a copy)."""
        self.with_lse = False
        try:
            return super().run().copy()
        finally:
            self.with_lse = True

    def lse_out(self) -> np.ndarray:
        """f32 [S][n_q][H] of the last run()."""
        return self.lse.cpu().numpy().reshape(self.out_shape[:-1])

    def guards_intact(self) -> bool:
        g = DST_GUARD_BYTES // 4
        b = self.lse_all.cpu().numpy().view(np.uint32)
        return bool(super().guards_intact() and (b[:g] == SENTINEL).all() and (b[g + self.n_rows:] == SENTINEL).all())


# ------------------------------------------------------------------ references

def scores64(o: op.OpProblem, round_q: bool = True):
    """Yields (s, h, float64 [NQ][N]): sinks.scores(o) with the product, the cap
    and slope * mask in float64.  round_q: Q rounded to f16 as orc.mulmat_f32
    rounds it (K is rounded as well: cache values are f16 numbers or their
    dequantisation, which the oracle rounds) -- False: Q and K as given."""
    b = o.base
    D, NQ, H, S, N = b.D, b.NQ, b.H, b.S, b.N
    rk2, rk3 = H // b.Hkv, S // b.Skv
    K = op._decode(o.k)
    qb = o.q
    qraw = qb.data[qb.off:]
    q = as_strided(qraw[:len(qraw) // 4 * 4].view(np.float32), shape=(S, H, NQ, D), strides=(qb.nb[3], qb.nb[2], qb.nb[1], 4))
    rnd = views._h if round_q else (lambda x: np.asarray(x, dtype=np.float64))
    cap = np.float32(o.logit_softcap)
    scale = np.float32(o.scale)
    s_eff = float(scale / cap) if cap > 0 else float(scale)
    sl = op.slopes(o.max_bias, o.n_head_total or H)[o.head_first:o.head_first + H].astype(np.float64)
    for s in range(S):
        for h in range(H):
            sc = (rnd(np.ascontiguousarray(q[s, h])) @ rnd(K[s // rk3, h // rk2]).T) * s_eff
            if cap > 0:
                sc = float(cap) * np.tanh(sc)
            if o.mask is not None:
                mbuf, _, mne, mnb = o.plane_of(h, s)
                rows = as_strided(mbuf.view(np.uint16), shape=(NQ, N), strides=(mnb[1], 2))
                from oracle import oracle as orc
                m = orc.f16_bits_to_f32(np.ascontiguousarray(rows)).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    sc = sc + sl[h] * m
            yield s, h, sc


def lse_ref(o: op.OpProblem, sinks=None, f64: bool = False, round_q: bool = False, sc_list=None) -> np.ndarray:
    """float64 [S][NQ][H] (module docstring).  f64: over scores64(o, round_q);
    sc_list: list(sinks.scores(o)) when the caller already has it."""
    b = o.base
    out = np.empty((b.S, b.NQ, b.H))
    for s, h, sc in (sc_list if sc_list is not None else scores64(o, round_q) if f64 else sk.scores(o)):
        r = sk.lse_rows(sc)
        if sinks is not None:
            r = np.logaddexp(r, np.float64(sinks[h]))
        out[s, :, h] = r
    return out


def ref_uncertainty(o: op.OpProblem, lse=None) -> float:
    """max |lse over the oracle's f32 scores - lse over the float64 product of the same rounded operands|.
    lse: lse_ref(o) when the caller already has it."""
    a, b = lse_ref(o) if lse is None else lse, lse_ref(o, f64=True, round_q=True)
    ok = np.isfinite(a)
    assert np.array_equal(ok, np.isfinite(b))
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


def merge_ref(outs, lses, sinks=None):
    """fattn_lse_merge in float64.  outs [P][..., dv], lses [P][...]; sinks: None
    or [n_head] raw logits, row r (flat, dst's [S][n_q][H] order) of head
    r % n_head.  Returns (dst [..., dv], lse_out [...])."""
    outs, lses = np.asarray(outs, dtype=np.float64), np.asarray(lses, dtype=np.float64)
    P, dv, shape = outs.shape[0], outs.shape[-1], lses.shape[1:]
    o, l = outs.reshape(P, -1, dv), lses.reshape(P, -1)
    R = l.shape[1]
    s = np.full(R, -np.inf) if sinks is None else np.asarray(sinks, dtype=np.float64)[np.arange(R) % len(sinks)]
    M = np.maximum(l.max(axis=0), s)
    Ms = np.where(np.isfinite(M), M, 0.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = np.where(np.isneginf(l), 0.0, np.exp(l - Ms))
        L = w.sum(axis=0) + np.where(np.isneginf(s), 0.0, np.exp(s - Ms))
        num = np.where((w > 0)[:, :, None], w[:, :, None] * o, 0.0).sum(axis=0)   # (by selection: no 0 * NaN)
        dst = num / L[:, None]
        lse = M + np.log(L)
    dead = np.isneginf(l).all(axis=0)
    dst[dead] = np.nan if sinks is None else 0.0
    lse[dead] = s[dead]
    return dst.reshape(shape + (dv,)), lse.reshape(shape)


def ulp32(x) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def check_lse(got, ref, tag: str) -> float:
    """The bar of the module docstring; prints the worst |error| (and the bound it met there) first."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    err = np.abs(got - ref)[fin]
    bound = (LSE_ATOL + 4 * ulp32(ref[fin]))
    worst = float(err.max()) if err.size and not np.isnan(err).any() else (float("nan") if err.size else 0.0)
    print(f"LSE {tag}: max |lse - ref| {worst:.3e} (bar {LSE_ATOL:.2e} + 4 ulp; |ref| <= {np.abs(ref[fin]).max() if fin.any() else 0:.3g}; "
          f"{int((~fin).sum())} rows -inf)")
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), f"{tag}: -inf rows differ"
    assert not np.isnan(got).any(), f"{tag}: NaN in lse (a row not written?)"
    assert (err <= bound).all(), f"{tag}: {worst:.3e}"
    return worst


# ------------------------------------------------------------------ the cases of the GPU suite

@dataclass
class Case:
    """One launch of tests/test_gpu_lse.py: `o` carries the reference's problem
    (sinks.scores / scores64), make(dev) builds the gpu_util.GuardedLaunch under
    `opts`, `want` is what describe() must say."""
    id: str
    o: op.OpProblem
    make: Callable
    want: tuple = ()
    opts: tuple = ()
    sinks: Optional[np.ndarray] = None
    f64: bool = False                      # BF16: the float64 reference over Q as given
    extra: dict = field(default_factory=dict)

    def lse_ref(self) -> np.ndarray:
        return lse_ref(self.o, self.sinks, self.f64)


def spec_op(spec, kind="random", **kw) -> op.OpProblem:
    """The plan table's row under one mask plane (a kind of tests/op_cases.plane, or f32 [NQ][N]) and the scalars."""
    import op_cases as t
    plane = kind if isinstance(kind, np.ndarray) else t.plane(spec, kind)
    return op.one_plane(t.problem(spec), plane, spec.variants, **kw)


def off_kernel(spec) -> str:
    """What describe() names with max_bias / logit_softcap off."""
    return "fattn_pf4_kernel(lean)" if spec.plan == "pf4shape" else spec.kernel


def spec_case(spec, kind="random", sinks=None, tag="", live=False, want=None, opts=None, kv_chunk=None, **kw) -> Case:
    o = spec_op(spec, kind, **kw)
    chunk = spec.kv_chunk if kv_chunk is None else kv_chunk
    return Case(spec.id + tag, o, lambda dev: views.GpuView(o, dev, chunk, sinks=sinks),
                ((spec.kernel if live else off_kernel(spec)),) if want is None else tuple(want),
                spec.opts if opts is None else tuple(opts), sinks)


@functools.lru_cache(maxsize=None)
def kv_case(kv_type: str) -> Case:
    """A one-row split decode at D = 128 over a cache type the oracle does not know (bf16, q5_1)."""
    import kv_types as kt
    gpu, ref = kt.reference_pair(kv_type, D=128, NQ=1, H=4, Hkv=4, N=256, mask="none", seed=21)
    o_ref = op.one_plane(ref, op.random_mask(1, 256, seed=3))
    o_gpu = views.swap_kv(o_ref, gpu)
    return Case(f"split_row-D128-{kv_type}-q1h4kv4n256", o_ref, lambda dev: views.GpuView(o_gpu, dev),
                (f"fattn_split_kernel<{kv_type},{kv_type},D128",), f64=kv_type == "bf16", extra={"gpu": o_gpu})


@functools.lru_cache(maxsize=None)
def mla_cases() -> tuple:
    import mla
    import mla_quant as mq
    from mla import Shape
    dec, chunked, rows5 = Shape(16, 1, 1, 160), Shape(16, 1, 1, 416), Shape(16, 1, 5, 224)
    out = []
    c = mla.make_case(dec, "random")
    out.append(Case("mla-f16-view-decode-n160", c.ref, lambda dev, c=c: mla.MlaGpu(c, dev=dev), ("fattn_mla_kernel<f16", "v=k+128", "grid(1,1,1)")))
    c = mla.make_case(chunked, "random")
    out.append(Case("mla-f16-view-4chunks", c.ref, lambda dev, c=c: mla.MlaGpu(c, kv_chunk=128, dev=dev),
                    ("fattn_mla_kernel<f16", "grid(4,1,1)", "fattn_mla_merge_kernel")))
    c = mla.make_case(rows5, "random")
    out.append(Case("mla-f16-own-rows5", c.ref, lambda dev, c=c: mla.MlaGpu(c, v_form="own", dev=dev), ("fattn_mla_kernel<f16", "v=own>")))
    c = mq.make_case(rows5, "q8_0", "random")
    out.append(Case("mla-q8_0-all4-rows5", c.ref, lambda dev, c=c: mq.QGpu(c, dev=dev), ("fattn_mla_kernel<q8_0",), extra={"no": "solo"}))
    c = mq.make_case(dec, "q8_0", "random")
    out.append(Case("mla-q8_0-solo-decode-n160", c.ref, lambda dev, c=c: mq.QGpu(c, dev=dev), ("fattn_mla_kernel<q8_0", "(solo")))
    return tuple(out)


def row_wg_case() -> Case:
    """A one-row decode over 1024 keys, 8 waves, chunks of 256: wg_row_merge's several-chunk path."""
    import fattn
    import plans
    spec = plans.Spec("row_wg_merge", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 1024), ((fattn.OPT_SPLIT_WAVES, 8),), kv_chunk=256)
    return spec_case(spec)


def every_plan() -> list:
    import plans
    cases = [spec_case(s) for s in plans.OP_SPECS]
    cases += [spec_case(s, want=(s.kernel,)) for s in plans.PLANE_SPECS if s.plan == "pf4"]
    return cases + list(mla_cases()) + [kv_case("bf16"), kv_case("q5_1")]


# ---- scalars and masks on plans.FAMILIES

def window_mask(NQ: int, N: int) -> np.ndarray:
    """f32 [NQ][N]: U[-1, 1] inside a window of N / 4 keys that slides with the
    query row and leaves rows i % 5 == 1 (every row when NQ == 1 is avoided: row 0
    keeps its window) without any key -- fully masked rows between live ones."""
    m = np.full((NQ, N), -np.inf, dtype=np.float32)
    rng = np.random.default_rng(881)
    w = max(8, N // 4)
    for i in range(NQ):
        if i % 5 == 1:
            continue
        lo = (i * 37) % (N - w + 1)
        m[i, lo:lo + w] = (1.0 - 2.0 * rng.random(w, dtype=np.float32)).astype(np.float32)
        m[i, 0] = np.float32(0.25)   # (the oracle's quirk: a row whose FIRST score is -inf is NaN)
    return m


def sink_values(H: int, N: int, centre=None) -> np.ndarray:
    """ln N + linspace(-2, 3, H), head h taking entry (5 h + 3) % H (tests/test_gpu_sinks.py).
    centre (a number, or one per head): what stands for ln N where the scores are not O(1)."""
    off = np.linspace(-2.0, 3.0, H)[(5 * np.arange(H) + 3) % H]
    return ((np.log(np.float64(N)) if centre is None else np.asarray(centre, dtype=np.float64)) + off).astype(np.float32)


def plane_case(spec, which: str) -> Case:
    """spec under per-head planes (ne2 = H) or per-sequence planes (S = 2 over one KV sequence, ne3 = 2)."""
    import mask_planes as mp
    import op_cases as t
    from problems import make_problem
    NQ, H, Hkv, N = spec.shape
    if which == "head":
        prob, ne2, ne3 = t.problem(spec), H, 1
    else:
        prob, ne2, ne3 = make_problem(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, kv_type=spec.kt, S=2, Skv=1, mask="none", seed=733), 1, 2
    o = op.with_params(mp.add_planes(prob, ne2, ne3, seed=5))
    return Case(f"{spec.id}-{which}-planes", o, lambda dev: views.GpuView(o, dev, spec.kv_chunk), (), spec.opts)


def scalar_cases(spec) -> list:
    NQ, H, Hkv, N = spec.shape
    s = sink_values(H, N)
    wm = window_mask(NQ, N)
    return [
        spec_case(spec, tag="-softcap", live=True, logit_softcap=4.0),
        spec_case(spec, "distance", tag="-alibi", live=True, max_bias=8.0),
        plane_case(spec, "head"), plane_case(spec, "seq"),
        spec_case(spec, sinks=s, tag="-sinks"),
        spec_case(spec, wm, tag="-window"),
        spec_case(spec, wm, sinks=s, tag="-window-sinks"),
    ]


# ---- KV shards

def shard_mask(NQ: int, N: int) -> np.ndarray:
    """A causal mask whose query rows are spread over the whole key range: row i
    sees keys [0, (i + 1) N / (NQ + 1)), values U[-1, 1] -- so the early rows are
    fully masked in the later key ranges (and a single row sees half the keys)."""
    rng = np.random.default_rng(97)
    m = (1.0 - 2.0 * rng.random((NQ, N), dtype=np.float32)).astype(np.float32)
    for i in range(NQ):
        m[i, max(1, (i + 1) * N // (NQ + 1)):] = -np.inf
    return m


def suite_ops():
    """Every (id, OpProblem) whose oracle-side scores the GPU suite's LSE checks rest on (BF16's float64 reference has none)."""
    import plans
    for c in every_plan():
        if not c.f64:
            yield c.id, c.o
    for spec in plans.FAMILIES:
        for c in scalar_cases(spec):
            yield c.id, c.o
        yield spec.id + "-shard", spec_op(spec, shard_mask(spec.shape[0], spec.shape[3]))
    yield "mla-shard", shard_mla().ref
    yield "row_wg_merge", row_wg_case().o
    for i in ("split_row-D128-q8_0-q1h4kv4n256", "split_row_tail-D128-q8_0-q1h4kv4n200", "split_chunks-D128-q8_0-q2h8kv4n1500"):
        yield i, spec_op(plans.OP_BY_ID[i])


@functools.lru_cache(maxsize=None)
def shard_mla():
    import mla
    sh = mla.Shape(16, 1, 1, 160)
    return mla.make_case(sh, planes=shard_mask(1, 160)[None, None])


if __name__ == "__main__":   # PYTHONPATH=.:ggml-cuda-experiments_amd python tests/lse.py (CPU only)
    worst = 0.0
    for name, o in suite_ops():
        u = ref_uncertainty(o)
        worst = max(worst, u)
        print(f"{u:.3e} {name}")
    print(f"REF_WORST = {worst:.3e}   LSE_ATOL = 8 x = {8 * worst:.3e}")
