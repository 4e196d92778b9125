"""GPU: mask planes (mask ne[2] / ne[3], include/fattn.h) on every plan.

Each case takes one plan at its smallest shape (the rows of
tests/plans.py's table, one type per distinct kernel body), gives the
mask (ne2, ne3) planes laid out as a poisoned view (tests/mask_planes.py) and

  (a) asserts fattn_describe names the intended kernel and the plane counts,
  (b) compares with the oracle assembled per (sequence, head) slice from that
      slice's own plane: attn_rel_err <= 1e-3 and attn_elem_err <= 1, the
      suite's bounds -- NaN positions must coincide, so one poisoned gap or pad
      column leaking into an output element fails the case,
  (c) checks dst's guard bands and the sentinel behind the exactly-sized
      workspace (gpu_util.GuardedLaunch).

The planes differ in where they turn -inf (N, N // 5 + 5, N // 2 + 3) and every
case runs with the full-length plane first and with the shortest first: a step
skip or a live-block table taken from another plane drops live keys in one
order or fetches dead ones -- and reads another plane's values -- in the other.
"""
import numpy as np
import pytest

import fattn
import mask_planes as mp
import views
from gpu_util import check_bars
from plans import BD, BDP, PF1, PF4, PLANE_SPECS as SPECS, Spec
from problems import make_problem

pytestmark = pytest.mark.gpu

BY_ID = {s.id: s for s in SPECS}
# the same plans with two q heads per kv head: the rows a 64- / 256-row tile
# packs alternate between two heads, so between two head planes
GQA = [
    Spec("bd", "fattn_bd_kernel<", 128, "f16", (40, 4, 2, 800), BD, tag="_gqa"),
    Spec("bd", "fattn_bd_kernel<", 128, "q8_0", (40, 4, 2, 800), BD, tag="_gqa"),
    Spec("bdp", "fattn_bdp_kernel<", 128, "q8_0", (64, 4, 2, 320), BDP, tag="_gqa"),
    Spec("pf", "fattn_pf_kernel<f16,D128", 128, "f16", (300, 4, 2, 384), PF1, tag="_gqa"),
    Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128", 128, "f16", (300, 4, 2, 384), PF4, tag="_gqa"),
]
HEAD_SPECS = [s for s in SPECS if s.plan in ("split_gqa_merge", "split_chunks", "mq", "bd", "bdp", "pf", "pf4")] + GQA

# (S, Skv, ne3): a plane per sequence; modulo reuse with two sequences per KV
# (sharing a KV must not mean sharing a mask); two planes over one KV
SEQ_SETTINGS = ((3, 3, 3), (4, 2, 2), (2, 1, 2))
ORDERS = ("full", "short")

_problems = {}


def _problem(spec, S, Skv):
    key = (spec.id, S, Skv)
    if key not in _problems:
        NQ, H, Hkv, N = spec.shape
        _problems[key] = make_problem(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, S=S, Skv=Skv, kv_type=spec.kt, mask="none",
                                      seed=300 + len(_problems))
    return _problems[key]


def _run(spec, pp, dev, want_kernel=True, gran4=False):
    """Launch pp under spec's options; (a) and (c); returns (describe, output)."""
    with fattn.options(dict(spec.opts)):
        g = views.GpuView(pp, dev, spec.kv_chunk)
        d = g.describe()
        if gran4:
            assert d.startswith("fattn_split_kernel<") and ",gran4," in d, d
        elif want_kernel:
            assert spec.kernel in d, d
        ne2, ne3 = getattr(pp, "ne2", 1), getattr(pp, "ne3", 1)
        if ne2 > 1 or ne3 > 1:
            assert d.endswith(f" mask planes ({ne2},{ne3})"), d
        else:
            assert "mask planes" not in d, d
        got = g.run()
    assert g.guards_intact(), d
    _run.last = g                                         # (the launch's buffers: the workspace front holds the prefill's flags)
    return d, got


def _check(tag, spec, pp, d, got):
    ref = pp.oracle()
    assert not np.isnan(ref).any()                        # (position 0 is visible in every plane)
    check_bars(got, ref, lambda e_or, e_el: f"PLANES {spec.id} {tag}: gpu->oracle {e_or:.3e} elem {e_el:.3f} | {d.split(' grid(')[0]}")


# ------------------------------------------------------------------ sequence planes

@pytest.mark.parametrize("first", ORDERS)
@pytest.mark.parametrize("S,Skv,ne3", SEQ_SETTINGS, ids=[f"S{s}kv{k}ne3_{n}" for s, k, n in SEQ_SETTINGS])
@pytest.mark.parametrize("spec", SPECS, ids=[s.id for s in SPECS])
def test_sequence_planes(dev, spec, S, Skv, ne3, first):
    pp = mp.add_planes(_problem(spec, S, Skv), 1, ne3, first=first, seed=S)
    d, got = _run(spec, pp, dev)
    _check(f"S{S}/{Skv} ne3={ne3} {first}", spec, pp, d, got)


# ------------------------------------------------------------------ head planes

def _head_cases():
    out = []
    for s in HEAD_SPECS:
        counts = [s.shape[1]] + ([2] if s.rk2 == 4 else [])
        out += [(s, ne2, first) for ne2 in counts for first in ORDERS]
    return out


HEAD_CASES = _head_cases()


@pytest.mark.parametrize("spec,ne2,first", HEAD_CASES, ids=[f"{s.id}-ne2_{n}-{f}" for s, n, f in HEAD_CASES])
def test_head_planes(dev, spec, ne2, first):
    """ne2 = H: a plane per head; ne2 = 2 at four q heads per kv head: the
    packed heads of one tile alternate planes.  The multi-query kernel does not
    take head planes: the planner must leave it (here for the split kernel)."""
    pp = mp.add_planes(_problem(spec, 2, 2), ne2, 1, first=first, seed=ne2)
    d, got = _run(spec, pp, dev, want_kernel=spec.plan != "mq")
    if spec.plan == "mq":
        assert "fattn_mq_kernel" not in d and "fattn_split_kernel<" in d, d
    _check(f"ne2={ne2} {first}", spec, pp, d, got)


BOTH = [BY_ID["split_gqa_merge-D128-q8_0-q3h8kv2n800"], GQA[1], GQA[4]]


@pytest.mark.parametrize("first", ORDERS)
@pytest.mark.parametrize("spec", BOTH, ids=[s.id for s in BOTH])
def test_head_and_sequence_planes_head_major(dev, spec, first):
    """Both counts above 1, the planes stored [H'][S'] (nb[3] < nb[2])."""
    pp = mp.add_planes(_problem(spec, 4, 2), 2, 2, order="hs", first=first, seed=11)
    assert pp.mask.nb[3] < pp.mask.nb[2]
    d, got = _run(spec, pp, dev)
    _check(f"ne=(2,2) hs {first}", spec, pp, d, got)


# ------------------------------------------------------------------ replication

@pytest.mark.parametrize("spec", SPECS, ids=[s.id for s in SPECS])
def test_replicated_planes_are_the_broadcast_launch(dev, spec):
    """ne3 = S stored copies of one plane, the same plane with nb[3] = 0, and
    ne2 = H copies where the plan string agrees apart from the suffix: only
    addresses change, so the output is bit-identical to today's one-plane launch."""
    S = 2
    p = _problem(spec, S, S)
    H = p.H
    one = mp.default_planes(p, 1, 1, "short", seed=21)
    d0, out0 = _run(spec, mp.broadcast_of(mp.add_planes(p, 1, 1, planes=one)), dev)
    bits = out0.view(np.uint32)
    for tag, ne2, ne3, rep in (("copies3", 1, S, False), ("nb3=0", 1, S, True), ("copies2", H, 1, False),
                               ("nb2=0", H, 1, True)):
        planes = np.broadcast_to(one, (ne3, ne2) + one.shape[2:]).copy()
        pp = mp.add_planes(p, ne2, ne3, repeat=rep, planes=planes)
        d, got = _run(spec, pp, dev, want_kernel=ne2 == 1 or spec.plan != "mq")
        same_plan = d == d0 + f" mask planes ({ne2},{ne3})"
        assert same_plan or ne2 > 1, (d, d0)               # sequence planes never change the plan
        if same_plan:
            assert np.array_equal(got.view(np.uint32), bits), (tag, d)
        else:
            _check(tag, spec, pp, d, got)


# ------------------------------------------------------------------ prefill tile ranges

RANGE_SPECS = [BY_ID["pf-D128-f16-q300h2kv2n384"], BY_ID["pf4-D128-f16-q300h2kv2n384"]]


def _range_planes(p, keep0):
    """causal: make_problem's "causal"; band: the 64 keys ending at the causal
    diagonal (keep0: position 0 visible as well)."""
    NQ, N = p.NQ, p.N
    causal = np.zeros((NQ, N), dtype=np.float32)
    band = np.zeros((NQ, N), dtype=np.float32)
    for i in range(NQ):
        dgn = N - NQ + i
        causal[i, dgn + 1:] = -np.inf
        band[i, dgn + 1:] = -np.inf
        band[i, (1 if keep0 else 0):max(0, dgn - 63)] = -np.inf
    return causal, band


def _expected_flags(plane, qpt):
    """pf_mask_flags of one plane: [n_qt][N / 64]; 0 all -inf, 2 all +-0, else 1."""
    NQ, N = plane.shape
    n_qt = (NQ + qpt - 1) // qpt
    out = np.empty((n_qt, N // 64), dtype=np.uint8)
    for qt in range(n_qt):
        for s in range(N // 64):
            blk = plane[qt * qpt:(qt + 1) * qpt, 64 * s:64 * s + 64]
            out[qt, s] = 0 if np.isneginf(blk).all() else 2 if (blk == 0).all() else 1
    return out


@pytest.mark.parametrize("order", ["causal_first", "band_first"])
@pytest.mark.parametrize("spec", RANGE_SPECS, ids=[s.id for s in RANGE_SPECS])
def test_prefill_ranges_follow_the_plane(dev, spec, order):
    """Two sequences, one under a causal plane and one under a 64-wide band
    ending at the causal diagonal: the live KV tile range of a query tile
    differs at both ends between the planes.

    The oracle keeps the reference's softmax quirk -- a row whose first score
    is -inf is NaN (fattn_oracle.c, orc_softmax) -- so under the band it is NaN
    on every row while the kernels, rightly, are not.  Hence two parts:
    (1) the band as stated: the flag tables the pre-pass left at the front of
        the workspace equal the tables computed here from each plane (they
        differ at both ends); the output equals, bit for bit, the two
        one-plane launches (all causal, all band) taken per sequence; and the
        causal sequence is within the suite's bounds of the oracle;
    (2) the band with position 0 visible too, where the oracle is defined on
        every row: the whole output against the assembled oracle."""
    p = _problem(spec, 2, 2)
    ci, bi = (0, 1) if order == "causal_first" else (1, 0)
    # ---- (1)
    causal, band = _range_planes(p, keep0=False)
    pl = [None, None]
    pl[ci], pl[bi] = causal, band
    pp = mp.add_planes(p, 1, 2, planes=np.stack(pl)[:, None])
    d, got = _run(spec, pp, dev)
    assert "pf_mask_flags" in d, d
    g = _run.last
    qpt = 256 // (p.H // p.Hkv)
    want = np.stack([_expected_flags(x, qpt) for x in pl])
    assert not np.array_equal(want[0], want[1])
    lo = lambda f: [int(np.argmax(r != 0)) for r in f]
    assert lo(_expected_flags(band, qpt)) != lo(_expected_flags(causal, qpt))      # the ranges' low ends differ too
    flags = g.ws_all.view(__import__("torch").uint8)[:want.size].cpu().numpy().reshape(want.shape)
    assert np.array_equal(flags, want), (flags, want)
    singles = {}
    for name, plane in (("causal", causal), ("band", band)):
        one = mp.broadcast_of(mp.add_planes(p, 1, 1, planes=plane[None, None]))
        singles[name] = _run(spec, one, dev)[1]
    assert np.array_equal(got[ci].view(np.uint32), singles["causal"][ci].view(np.uint32))
    assert np.array_equal(got[bi].view(np.uint32), singles["band"][bi].view(np.uint32))
    assert not np.isnan(got).any()
    ref = pp.oracle()
    assert np.isnan(ref[bi]).all() and not np.isnan(ref[ci]).any()                 # (the quirk, as documented above)
    check_bars(got[ci], ref[ci], lambda e_or, e_el: f"PLANES {spec.id} {order} causal sequence: gpu->oracle {e_or:.3e} elem {e_el:.3f}")
    # ---- (2)
    causal, band = _range_planes(p, keep0=True)
    pl[ci], pl[bi] = causal, band
    pp = mp.add_planes(p, 1, 2, planes=np.stack(pl)[:, None])
    d, got = _run(spec, pp, dev)
    _check(order + " band+0", spec, pp, d, got)


# ------------------------------------------------------------------ dword path

DW = BY_ID["split_row-D128-q8_0-q1h4kv4n256"]
DW_CASES = [(1, n3, S, Skv, f) for S, Skv, n3 in SEQ_SETTINGS for f in ORDERS] + [(4, 1, 2, 2, f) for f in ORDERS] + \
    [(2, 2, 2, 1, "short")]


@pytest.mark.parametrize("ne2,ne3,S,Skv,first", DW_CASES, ids=[f"ne{a}_{b}-S{s}kv{k}-{f}" for a, b, s, k, f in DW_CASES])
def test_plane_offset_4_takes_the_dword_kernel(dev, ne2, ne3, S, Skv, first):
    """A plane stride with stride % 16 == 4: the dword split kernel (gran4)."""
    pp = mp.add_planes(_problem(DW, S, Skv), ne2, ne3, offset4=True, first=first, seed=5)
    d, got = _run(DW, pp, dev, gran4=True)
    _check(f"offset4 ne=({ne2},{ne3}) {first}", DW, pp, d, got)
