"""The op's features in pairs on every cell of tests/plans.py's CELLS and
GQA_CELLS: the covering table, the problem of a case and its references.

THE FEATURES (one letter each; lse is requested in every case)
  c  logit_softcap 4 at scale 1.0 (the saturating setting of the op_params suite)
  a  max_bias 8 over op.distance_mask
  s  sinks
  h  head planes, ne2 = H
  q  sequence planes, S = 2 over Skv = 1, ne3 = 2
  w  lse.window_mask: fully masked rows between live ones

THE RECIPES -- four of them hold all 15 pairs:
  R1  c s h q   the planes of mask_planes.default_planes
  R2  a s w     dead rows are exactly 0.0 and their lse is the head's sink, bit for bit
  R3  c a h w   no sinks: dead rows are NaN, their lse -inf
  R4  a q w     n_head_total = 2 H, head_first = H: the slopes of the second half

STATIC SUBSTITUTIONS (from the cell alone, never from what a launch does)
  mq cells     R1 and R3 drop h (head planes leave fattn_mq_kernel): c s q, c a w
  pf4 cells    c and a are dropped (they move the plan to fattn_pf_kernel):
               s h q, s w, h w, q w
  NQ = 1       a one-row cell has one row per (sequence, head), so a window cannot
               leave a dead row beside a live one: w brings q with it there --
               sequence 0 keeps its window, sequence 1 is masked everywhere

THE MASK OF A CASE.  Without w: default_planes (U[-1, 1], -inf from a length that
differs from plane to plane on).  With w, plane p is its base -- op.distance_mask
under a, op.random_mask otherwise -- cut to lse.window_mask, whose keys (from 1
on) are rotated by 41 p and whose rows by p, so no two planes of a case agree on
the window or on the dead rows.  Under a, a live row also keeps its own position
(distance 0): the row's largest score stays O(1) whatever the slope, and with it
the log-sum-exp -- a window 600 keys from the diagonal under slope 1/2 alone
would put every score near -300, where the f32 scores of the assembled
reference carry 1.5e-5 and lse.REF_WORST (2.3e-6) could not hold.

SINKS are lse.sink_values: ln N + linspace(-2, 3, H) under the sinks suite's
permutation; under c or a the offsets are taken around each head's median
reference log-sum-exp instead of ln N (ALiBi heads differ by their slope: one
centre for all would leave the flat heads unmoved).

SEEDS.  A cell's tensors are seeded by crc32 of the cell's id, a case's planes
by crc32 of the case's id: nothing depends on the order the cases run in.

Every reference is one of the suites' own: sinks.reference (the factor form over
op_params.reference), lse.lse_ref, and for BF16 bf16.reference_f64.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import numpy as np

import fattn
import kv_types as kt
import lse as ls
import mask_planes as mp
import op_params as op
import plans
import sinks as sk
import views
from problems import attn_rel_err, make_problem

MOVES = 5e-2
ORDER = "cashqw"
NAMES = {"c": "logit_softcap", "a": "max_bias", "s": "sinks", "h": "head planes", "q": "sequence planes", "w": "window"}
RECIPES = {"R1": "cshq", "R2": "asw", "R3": "cahw", "R4": "aqw"}
MQ_RECIPES = {"R1": "csq", "R2": "asw", "R3": "caw", "R4": "aqw"}
PF4_RECIPES = {"R1": "shq", "R2": "sw", "R3": "hw", "R4": "qw"}
CAP, MAX_BIAS = 4.0, 8.0


def features(spec, recipe: str) -> str:
    """The live features of (cell, recipe), in ORDER (module docstring: the static substitutions)."""
    f = (MQ_RECIPES if spec.family == "mq" else PF4_RECIPES if spec.family == "pf4" else RECIPES)[recipe]
    if "w" in f and spec.shape[0] == 1 and "q" not in f:
        f += "q"
    return "".join(x for x in ORDER if x in f)


def pairs(feats: str) -> set:
    return {a + b for i, a in enumerate(feats) for b in feats[i + 1:]}


@dataclass(frozen=True)
class Combo:
    spec: plans.Spec
    recipe: str

    @property
    def id(self):
        return f"{self.spec.id}-{self.recipe}"

    @property
    def feats(self):
        return features(self.spec, self.recipe)

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) % 100000

    @property
    def ne(self):
        """(ne2, ne3) of the mask."""
        return (self.spec.shape[1] if "h" in self.feats else 1, 2 if "q" in self.feats else 1)

    @property
    def second_half(self):
        """R4: the launch is the second half of 2 H heads."""
        return self.recipe == "R4" and "a" in self.feats

    @property
    def f64(self):
        return kt.KV_TYPES[self.spec.kt].f64 if self.spec.kt in kt.KV_TYPES else False

    def markers(self) -> list:
        """What describe() carries for the live features."""
        out = []
        if self.ne != (1, 1):
            out.append(" mask planes (%d,%d)" % self.ne)
        if "c" in self.feats:
            out.append(" softcap 4")
        if "a" in self.feats:
            out.append(" alibi 8")
        return out


CASES = [Combo(s, r) for s in plans.CELLS for r in RECIPES] + [Combo(s, r) for s in plans.GQA_CELLS for r in ("R1", "R2")]
BY_ID = {c.id: c for c in CASES}
# cell x recipe the library refuses: id -> status (pinned by tests/test_combos.py; none today)
REFUSED = {}


# ------------------------------------------------------------------ the problem of a case

@functools.lru_cache(maxsize=8)
def _tensors(spec, S: int, scale: Optional[float]):
    """(the problem the reference reads, the problem the GPU reads or None when they are one)."""
    NQ, H, Hkv, N = spec.shape
    kw = dict(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, S=S, Skv=1, mask="none", scale=scale, seed=zlib.crc32(spec.id.encode()) % 100000)
    if spec.kt in kt.KV_TYPES:                       # a type the oracle does not know: F16 views of what the kernel reads
        gpu, ref = kt.reference_pair(spec.kt, **kw)
        return ref, gpu
    if spec.v_trans:
        return make_problem(kv_type="f16", **kw), make_problem(kv_type="f16", v_trans=True, **kw)
    return make_problem(kv_type=spec.kt, v_type=spec.vt or None, **kw), None


def window(NQ: int, N: int, p: int, dead: bool = False) -> np.ndarray:
    """lse.window_mask for plane p: the keys from 1 on rotated by 41 p, the rows by p (dead: no key at all)."""
    if dead:
        return np.full((NQ, N), -np.inf, dtype=np.float32)
    w = ls.window_mask(NQ, N)
    if p:
        w[:, 1:] = np.roll(w[:, 1:], 41 * p, axis=1)
        w = np.roll(w, p, axis=0)
    return w


def case_planes(c: Combo) -> np.ndarray:
    """f32 [ne3][ne2][NQ][N] (module docstring: the mask of a case)."""
    NQ, H, Hkv, N = c.spec.shape
    ne2, ne3 = c.ne
    if "w" not in c.feats:
        assert "a" not in c.feats
        return mp.default_planes(_tensors(c.spec, ne3, None)[0], ne2, ne3, seed=c.seed)
    out = np.empty((ne3, ne2, NQ, N), dtype=np.float32)
    for i3 in range(ne3):
        for i2 in range(ne2):
            p = i3 * ne2 + i2
            base = op.distance_mask(NQ, N) if "a" in c.feats else op.random_mask(NQ, N, seed=c.seed + p)
            win = window(NQ, N, p, dead=NQ == 1 and i3 == 1)
            m = np.where(np.isfinite(win), base, np.float32(-np.inf)).astype(np.float32)
            if "a" in c.feats:
                for i in np.flatnonzero(np.isfinite(win).any(axis=1)):
                    m[i, N - NQ + i] = 0.0
            out[i3, i2] = m
    return out


def problem_of(c: Combo, planes=None, **over) -> tuple:
    """(o, og): the OpProblem the references read and the one the GPU is given
    (the same object unless the cache is of a type the oracle does not know, or
    V is transposed).  planes / over: other planes or parameters than the
    case's, for the preconditions."""
    NQ, H, Hkv, N = c.spec.shape
    ne2, ne3 = c.ne
    ref, gpu = _tensors(c.spec, ne3, 1.0 if "c" in c.feats else None)
    planes = case_planes(c) if planes is None else planes
    kw = dict(logit_softcap=CAP if "c" in c.feats else 0.0, max_bias=MAX_BIAS if "a" in c.feats else 0.0,
              n_head_total=2 * H if c.second_half else 0, head_first=H if c.second_half else 0)
    kw.update(over)
    if (ne2, ne3) == (1, 1):
        o = op.one_plane(ref, planes[0, 0], c.spec.variants, **kw)
    else:
        o = op.with_params(mp.add_planes(ref, ne2, ne3, planes=planes, variants=tuple(c.spec.variants)), **kw)
    return o, (o if gpu is None else views.swap_kv(o, gpu))


@dataclass
class Built:
    """A case with its references, computed once."""
    case: Combo
    o: op.OpProblem                 # what the references read
    og: op.OpProblem                # what the GPU is given
    sinks: Optional[np.ndarray]
    plain: np.ndarray               # op_params.reference(o): without sinks
    ref: np.ndarray                 # sinks.reference: the expected dst
    lse_plain: np.ndarray           # lse.lse_ref(o): without sinks (-inf: a dead row)
    lse: np.ndarray                 # lse.lse_ref(o, sinks): the expected lse (BF16: over the float64 scores)

    @property
    def dead(self):
        """bool [S][NQ][H]: the rows without a key."""
        return np.isneginf(self.lse_plain)

    def f64(self):
        import bf16
        return bf16.reference_f64(self.og, sinks=self.sinks)


def _reference(o, sinks, plain=None, sc_list=None):
    return sk.reference(sk.with_sinks(o, sinks), plain=plain, sc_list=sc_list)


def seq_of(o, s: int):
    """Sequence s of o as a problem of its own over the same buffers (Q and the mask start at the sequence's
    planes; every case has one KV sequence): the references treat each (sequence, head) on its own."""
    assert o.base.Skv == 1
    q = dataclasses.replace(o.q, off=o.q.off + s * o.q.nb[3])
    m = None if o.mask is None else dataclasses.replace(o.mask, off=o.mask.off + (s % o.ne3) * o.mask.nb[3])
    return dataclasses.replace(o, base=dataclasses.replace(o.base, S=1), q=q, mask=m, ne3=1)


def plain_and_scores(o):
    """(op_params.reference(o), list(sinks.scores(o))), each sequence's reference and score pass on a thread of
    its own: the oracle's products are sequential C loops that release the GIL."""
    S = o.base.S
    with ThreadPoolExecutor(2 * S) as ex:
        refs = [ex.submit(op.reference, seq_of(o, s)) for s in range(S)]
        scs = [ex.submit(lambda s=s: list(sk.scores(seq_of(o, s)))) for s in range(S)]
        plain = np.concatenate([f.result() for f in refs], axis=0)
        sc_list = [(s, h, sc) for s in range(S) for _, h, sc in scs[s].result()]
    return plain, sc_list


def build(c: Combo) -> Built:
    NQ, H, Hkv, N = c.spec.shape
    o, og = problem_of(c)
    plain, sc_list = plain_and_scores(o)
    lse_plain = ls.lse_ref(o, sc_list=sc_list)
    sinks = None
    if "s" in c.feats:
        centre = None
        if "c" in c.feats or "a" in c.feats:
            centre = [np.median(lse_plain[:, :, h][np.isfinite(lse_plain[:, :, h])]) for h in range(H)]
        sinks = ls.sink_values(H, N, centre)
    ref = _reference(o, sinks, plain, sc_list)
    lse = ls.lse_ref(o, sinks, f64=True) if c.f64 else ls.lse_ref(o, sinks, sc_list=sc_list)
    return Built(c, o, og, sinks, plain, ref, lse_plain, lse)


# ------------------------------------------------------------------ preconditions

PRE_ROWS = 4    # the query rows the preconditions recompute the reference for


def moved(a: np.ndarray, b: np.ndarray) -> float:
    """attn_rel_err over the rows that are numbers in both (a rotation of the
    planes moves the dead rows too); without such a row, inf when the NaN rows
    differ -- attn_rel_err's own answer to that."""
    na, nb = np.isnan(a).any(axis=-1), np.isnan(b).any(axis=-1)
    ok = ~(na | nb)
    if not ok.any():
        return 0.0 if np.array_equal(na, nb) else float("inf")
    return attn_rel_err(a[ok], b[ok])


def moves_every_head(ref: np.ndarray, plain: np.ndarray) -> float:
    """min over heads of moved(reference with sinks, without)."""
    return min(moved(ref[:, :, h], plain[:, :, h]) for h in range(ref.shape[2]))


def preconditions(b: Built) -> dict:
    """feature -> how far the reference moves (attn_rel_err) when the feature is
    turned off, or given to the wrong head / sequence: each must be >= MOVES, so a
    kernel that dropped the feature, or indexed it by another head, cannot pass.
    The altered references are computed for the first PRE_ROWS query rows only
    (the same buffers, base.NQ cut): attn_rel_err is a maximum over rows, so what
    these rows move by bounds the whole reference's from below."""
    c, out = b.case, {}
    NQ, H = c.spec.shape[:2]
    rows = min(NQ, PRE_ROWS)
    planes = case_planes(c)

    def other(planes=None, **over):
        o = problem_of(c, planes, **over)[0]
        o = dataclasses.replace(o, base=dataclasses.replace(o.base, NQ=rows))
        return moved(b.ref[:, :rows], _reference(o, b.sinks))

    jobs = {}
    with ThreadPoolExecutor(4) as ex:
        if "c" in c.feats:
            jobs["c off"] = ex.submit(other, logit_softcap=0.0)
        if "a" in c.feats:
            jobs["a off"] = ex.submit(other, max_bias=0.0)
        if "h" in c.feats:
            jobs["h rotated"] = ex.submit(other, np.roll(planes, 1, axis=1))
        if "q" in c.feats:
            jobs["q swapped"] = ex.submit(other, planes[::-1].copy())
        if c.second_half:
            jobs["head_first - 1"] = ex.submit(other, head_first=H - 1)
        if "s" in c.feats:
            out["s off, every head"] = moves_every_head(b.ref, b.plain)
        out.update({k: f.result() for k, f in jobs.items()})
    return out


def dead_rows(c: Combo) -> np.ndarray:
    """bool [S][NQ][H] from the case's planes alone: the rows without a key."""
    d = np.isneginf(case_planes(c)).all(axis=-1)          # [ne3][ne2][NQ]
    ne3, ne2 = d.shape[:2]
    H = c.spec.shape[1]
    return np.stack([np.stack([d[s, h % ne2] for h in range(H)], axis=-1) for s in range(ne3)])


def dead_and_live_per_head(dead: np.ndarray) -> bool:
    return bool(dead.any(axis=(0, 1)).all() and (~dead).any(axis=(0, 1)).all())


# ------------------------------------------------------------------ the plan on the host

def describe(c: Combo, og=None) -> str:
    """fattn.describe of the case over fake pointers, under the cell's options."""
    og = problem_of(c)[1] if og is None else og
    with fattn.options(dict(c.spec.opts)):
        return fattn.describe(og.params(kv_chunk=c.spec.kv_chunk))


def check_plan(c: Combo, d: str):
    assert c.spec.kernel in d, (c.id, d)
    for m in c.markers():
        assert m in d, (c.id, m, d)
    for m in (" softcap", " alibi", " mask planes"):
        assert any(m in x for x in c.markers()) or m not in d, (c.id, m, d)
