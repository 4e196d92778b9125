"""GPU: ggml's max_bias (ALiBi) and logit_softcap on every plan.

One case per plan at its smallest shape -- the rows of
tests/test_gpu_mask_planes.py's table with the same forcing options, plus one
dword-path (gran4) split case and one mixed K / V pair -- each under

  alibi      max_bias 8 over the integer distance mask (-inf past the causal
             diagonal); where every slope is a power of two (H = 1, 2, 4, 8, 6)
             also against the frozen oracle over pre-multiplied head planes
  sat        scale 1.0, logit_softcap 4 (saturating), random mask and no mask
  mild       the default scale, logit_softcap 0.5, random mask
  both       scale 1.0, cap 4, max_bias 8, distance mask (one spec per kernel)

against the reference assembled from the frozen oracle's primitives
(tests/op_params.py), at the suite's own bound: attn_rel_err <= 1e-3 and
attn_elem_err <= 1, NaN positions coinciding.  Before a launch the case asserts
on the CPU that the parameters move the reference by >= 5e-2 (50 x the bound):
a kernel that ignored them could not pass.  Launches go through views.GpuView
(dst guard bands, the exactly-sized workspace's sentinel).  Every case prints
one OPPARAMS line with its errors.
"""
from dataclasses import dataclass

import numpy as np
import pytest

import fattn
import mask_planes as mp
import op_params as op
import views
from fattn import shard
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-3
MOVES = 5e-2


@dataclass(frozen=True)
class Spec:
    plan: str
    kernel: str               # what describe() must name with the parameters live
    D: int
    kt: str
    shape: tuple              # (NQ, H, Hkv, N)
    opts: tuple = ()
    kv_chunk: int = 0
    tag: str = ""
    vt: str = ""              # V type when it differs from K's
    variants: tuple = ()

    @property
    def id(self):
        NQ, H, Hkv, N = self.shape
        return f"{self.plan}{self.tag}-D{self.D}-{self.kt}-q{NQ}h{H}kv{Hkv}n{N}"


MQ = ((fattn.OPT_MQ_MIN_ROWS, 32), (fattn.OPT_BD, 1))
BD, BDP = ((fattn.OPT_BD, 2),), ((fattn.OPT_BD, 3),)
PF1 = ((fattn.OPT_PF, 2), (fattn.OPT_PF_FORM, 1))
PF4 = ((fattn.OPT_PF, 2),)
STAGED = "kv_stage_f16<q8_0> + pf_mask_flags] + "

SPECS = [
    Spec("split_row", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 256)),
    Spec("split_row", "fattn_split_kernel<", 128, "f16", (1, 4, 4, 256)),
    Spec("split_row_tail", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 200)),
    Spec("split_chunks", "fattn_split_kernel<", 128, "q8_0", (2, 8, 4, 1500), kv_chunk=256),
    Spec("split_gqa_merge", "fattn_split_kernel<", 128, "q8_0", (3, 8, 2, 800), kv_chunk=256),
    Spec("split_d80", "fattn_split_kernel<", 80, "f16", (9, 8, 2, 300)),
    Spec("mq", "fattn_mq_kernel<", 128, "q8_0", (40, 16, 4, 320), MQ),
    Spec("mq", "fattn_mq_kernel<q8_0,D256,4waves", 256, "q8_0", (50, 2, 2, 320), MQ),
    Spec("bd", "fattn_bd_kernel<", 128, "f16", (40, 2, 2, 800), BD),
    Spec("bd", "fattn_bd_kernel<", 128, "q8_0", (40, 2, 2, 800), BD),
    Spec("bdp", "fattn_bdp_kernel<", 64, "q8_0", (64, 2, 2, 320), BDP),
    Spec("bdp", "fattn_bdp_kernel<", 128, "q8_0", (64, 2, 2, 320), BDP),
    Spec("pf", "fattn_pf_kernel<f16,D128", 128, "f16", (300, 2, 2, 384), PF1),
    Spec("pf", STAGED + "fattn_pf_kernel<f16,D128", 128, "q8_0", (300, 2, 2, 384), PF1, tag="_staged"),
    Spec("pf", "fattn_pf_kernel<q8_0,D128", 128, "q8_0", (300, 2, 2, 384), PF1 + ((fattn.OPT_PF_STAGE, 1),),
         tag="_inkernel"),
    # the shape and options that take fattn_pf4_kernel(lean) with both parameters off
    Spec("pf4shape", "fattn_pf_kernel<f16,D128", 128, "f16", (300, 2, 2, 384), PF4),
    Spec("split_gran4", ",gran4,", 128, "q8_0", (1, 4, 4, 256), variants=("kv_offset4",)),
    Spec("split_mixed", "fattn_split_kernel<q8_0,f16,D128", 128, "q8_0", (1, 4, 4, 256), vt="f16"),
]
BY_ID = {s.id: s for s in SPECS}
# irrational slopes (H = 12: n2 = 8, heads 8 .. 11 from the formula's second branch), three q heads per kv head
GQA12 = [
    Spec("split_gqa_merge", "fattn_split_kernel<", 128, "q8_0", (3, 12, 4, 800), kv_chunk=256, tag="_h12"),
    Spec("bd", "fattn_bd_kernel<", 128, "f16", (40, 12, 4, 800), BD, tag="_h12"),
    Spec("pf", "fattn_pf_kernel<f16,D128", 128, "f16", (90, 12, 4, 384), PF1, tag="_h12"),   # (two 85-query tiles)
]
FAMILIES = [BY_ID[i] for i in ("split_gqa_merge-D128-q8_0-q3h8kv2n800", "mq-D128-q8_0-q40h16kv4n320",
                               "bd-D128-q8_0-q40h2kv2n800", "bdp-D128-q8_0-q64h2kv2n320",
                               "pf_staged-D128-q8_0-q300h2kv2n384")]
EXACT_H = (1, 2, 4, 8, 6)     # head counts whose slopes at max_bias 8 are all powers of two

_cache = {}


def _problem(spec, scale=None):
    key = ("p", spec.id, scale)
    if key not in _cache:
        NQ, H, Hkv, N = spec.shape
        _cache[key] = make_problem(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, kv_type=spec.kt, v_type=spec.vt or None,
                                   mask="none", seed=500 + len(_cache), scale=scale)
    return _cache[key]


def _plane(spec, kind):
    NQ, _, _, N = spec.shape
    if kind == "none":
        return None
    key = ("m", kind, NQ, N)
    if key not in _cache:
        _cache[key] = op.distance_mask(NQ, N) if kind == "distance" else op.random_mask(NQ, N)
    return _cache[key]


def _reference(spec, scale, kind, **kw):
    """The assembled reference of (spec, scale, mask kind, parameters), computed once."""
    key = ("r", spec.id, scale, kind, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = op.one_plane(_problem(spec, scale), _plane(spec, kind), spec.variants, **kw).reference()
    return _cache[key]


def _launch(spec, vp, dev, nomask=False, kernel=None):
    """vp under spec's options through views.GpuView: (describe, output)."""
    with fattn.options(dict(spec.opts)):
        g = views.GpuView(vp, dev, spec.kv_chunk)
        d = g.describe()
        want = spec.kernel if kernel is None else kernel
        if nomask:
            want = want.replace(" + pf_mask_flags", "")
        assert want in d, d
        got = g.run()
    assert g.guards_intact(), d
    return d, got


def _check(tag, spec, d, got, ref, what="assembled"):
    e_or, e_el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    line = f"OPPARAMS {spec.id} {tag}: gpu->{what} {e_or:.3e} elem {e_el:.3f} | {d.split(' grid(')[0]}{d[d.index(' ws '):]}"
    print(line)
    assert e_or <= RTOL, line
    assert e_el <= 1.0, line


def _case(spec, dev, tag, scale, kind, **kw):
    ref = _reference(spec, scale, kind, **kw)
    off = _reference(spec, scale, kind)
    assert not np.isnan(ref).any()
    moved = attn_rel_err(ref, off)
    assert moved >= MOVES, (tag, moved)                        # (the parameters matter on this problem)
    vp = op.one_plane(_problem(spec, scale), _plane(spec, kind), spec.variants, **kw)
    d, got = _launch(spec, vp, dev, nomask=kind == "none")
    if kw.get("logit_softcap"):
        assert f" softcap {kw['logit_softcap']:g}" in d, d
    if kw.get("max_bias"):
        assert d.endswith(f" alibi {kw['max_bias']:g}"), d
    _check(f"{tag} (moves {moved:.2g})", spec, d, got, ref)
    return d, got


IDS = [s.id for s in SPECS]


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_alibi(dev, spec):
    d, got = _case(spec, dev, "alibi", None, "distance", max_bias=8.0)
    if spec.shape[1] in EXACT_H:
        # slope * mask exact in f16: the frozen oracle over H pre-multiplied head planes
        key = ("pre", spec.id)
        if key not in _cache:
            _cache[key] = op.premultiplied_planes(_problem(spec), _plane(spec, "distance"), 8.0).oracle()
        _check("alibi", spec, d, got, _cache[key], what="oracle(premultiplied planes)")


@pytest.mark.parametrize("spec", GQA12, ids=[s.id for s in GQA12])
def test_alibi_irrational_slopes_gqa(dev, spec):
    _case(spec, dev, "alibi h12", None, "distance", max_bias=8.0)


@pytest.mark.parametrize("kind", ["random", "none"])
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_softcap_saturating(dev, spec, kind):
    _case(spec, dev, f"sat {kind}", 1.0, kind, logit_softcap=4.0)


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_softcap_mild(dev, spec):
    _case(spec, dev, "mild", None, "random", logit_softcap=0.5)


@pytest.mark.parametrize("spec", FAMILIES, ids=[s.id for s in FAMILIES])
def test_both(dev, spec):
    _case(spec, dev, "both", 1.0, "distance", max_bias=8.0, logit_softcap=4.0)
    both = _reference(spec, 1.0, "distance", max_bias=8.0, logit_softcap=4.0)
    assert attn_rel_err(both, _reference(spec, 1.0, "distance", max_bias=8.0)) >= MOVES
    assert attn_rel_err(both, _reference(spec, 1.0, "distance", logit_softcap=4.0)) >= MOVES


PLANES = [BY_ID["split_gqa_merge-D128-q8_0-q3h8kv2n800"], BY_ID["bd-D128-q8_0-q40h2kv2n800"]]


@pytest.mark.parametrize("spec", PLANES, ids=[s.id for s in PLANES])
def test_head_planes_under_max_bias(dev, spec):
    """ne[2] = H head planes and max_bias: the plane comes from iq2 % ne2, the slope from the query head."""
    p = _problem(spec)
    pp = mp.add_planes(p, p.H, 1, first="short", seed=3)
    on, off = op.with_params(pp, max_bias=8.0), op.with_params(pp)
    ref, ref_off = on.reference(), off.reference()
    moved = attn_rel_err(ref, ref_off)
    assert moved >= MOVES, moved
    d, got = _launch(spec, on, dev)
    assert f" mask planes ({p.H},1) alibi 8" in d, d
    _check(f"planes x alibi (moves {moved:.2g})", spec, d, got, ref)


SHARD = Spec("shard", "fattn_split_kernel<", 128, "q8_0", (2, 8, 4, 512))


@pytest.mark.parametrize("world", [2, 4])
def test_head_shards_take_the_global_slopes(dev, world):
    """H = 8, Hkv = 4 over 2 and 4 ranks, every rank's slice launched on this
    GPU with shard.slope_args(): assembled, the unsharded reference.  The same
    slices with head_first = 0 are wrong by far more than the bound -- asserted
    on the CPU reference."""
    NQ, H, Hkv, N = SHARD.shape
    p = _problem(SHARD)
    dist = _plane(SHARD, "distance")
    full = _reference(SHARD, None, "distance", max_bias=8.0)
    parts, wrong = [], []
    for rank in range(world):
        sh = shard.shard_heads(H, Hkv, world, rank)
        sub = make_problem(D=SHARD.D, NQ=NQ, H=sh.n_heads, Hkv=sh.n_kv, N=N, kv_type=SHARD.kt, mask="none", seed=1)
        sub.q = np.ascontiguousarray(p.q[:, :, sh.h0:sh.h1])
        sub.k_bytes = np.ascontiguousarray(p.k_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
        sub.v_bytes = np.ascontiguousarray(p.v_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
        vp = op.one_plane(sub, dist, max_bias=8.0, **sh.slope_args())
        d, got = _launch(SHARD, vp, dev)
        parts.append(got)
        wrong.append(op.one_plane(sub, dist, max_bias=8.0).reference())
    assert attn_rel_err(np.concatenate(wrong, axis=2), full) > MOVES
    _check(f"world {world}", SHARD, d, np.concatenate(parts, axis=2), full)


IDENT = [BY_ID[i] for i in ("split_row-D128-q8_0-q1h4kv4n256", "mq-D128-q8_0-q40h16kv4n320", "bd-D128-f16-q40h2kv2n800",
                            "pf4shape-D128-f16-q300h2kv2n384")]


@pytest.mark.parametrize("spec", IDENT, ids=[s.id for s in IDENT])
def test_identities(dev, spec):
    """max_bias > 0 without a mask is max_bias = 0 -- same plan string, same
    output bits -- and explicitly zeroed fields are a launch built without
    them (here the pf4 shape still takes fattn_pf4_kernel)."""
    p = _problem(spec)
    off_kernel = "fattn_pf4_kernel(lean)" if spec.plan == "pf4shape" else spec.kernel
    d0, out0 = _launch(spec, views.make_view(p, *spec.variants), dev, nomask=True, kernel=off_kernel)
    d1, out1 = _launch(spec, op.one_plane(p, None, spec.variants, max_bias=8.0), dev, nomask=True, kernel=off_kernel)
    assert d1 == d0 and "alibi" not in d1
    assert np.array_equal(out1.view(np.uint32), out0.view(np.uint32))
    m = _plane(spec, "random")
    plain = mp.broadcast_of(mp.add_planes(p, 1, 1, planes=m[None, None], variants=spec.variants))
    d2, out2 = _launch(spec, plain, dev, kernel=off_kernel)                       # views' params: no keywords
    d3, out3 = _launch(spec, op.with_params(plain), dev, kernel=off_kernel)       # the four fields set to zero
    assert d3 == d2
    assert np.array_equal(out3.view(np.uint32), out2.view(np.uint32))
