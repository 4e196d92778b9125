"""GPU: ggml's max_bias (ALiBi) and logit_softcap on every plan.

One case per plan at its smallest shape -- tests/plans.py's table, with one
dword-path (gran4) split case and one mixed K / V pair -- each under

  alibi      max_bias 8 over the integer distance mask (-inf past the causal
             diagonal); where every slope is a power of two (H = 1, 2, 4, 8, 6)
             also against the frozen oracle over pre-multiplied head planes
  sat        scale 1.0, logit_softcap 4 (saturating), random mask and no mask
  mild       the default scale, logit_softcap 0.5, random mask
  both       scale 1.0, cap 4, max_bias 8, distance mask (one spec per kernel)

against the reference assembled from the frozen oracle's primitives
(tests/op_params.py; tests/op_cases.py computes each once), at the suite's own
bound: attn_rel_err <= 1e-3 and attn_elem_err <= 1, NaN positions coinciding.  Before a launch the case asserts
on the CPU that the parameters move the reference by >= 5e-2 (50 x the bound):
a kernel that ignored them could not pass.  Launches go through views.GpuView
(dst guard bands, the exactly-sized workspace's sentinel).  Every case prints
one OPPARAMS line with its errors.
"""
import numpy as np
import pytest

import mask_planes as mp
import op_params as op
import views
from fattn import shard
from gpu_util import check_bars
from op_cases import launch as _launch, plane as _plane, premultiplied_oracle, problem as _problem, reference as _reference
from plans import BD, FAMILIES, IDENT, OP_BY_ID as BY_ID, OP_SPECS as SPECS, PF1, SHARD, Spec
from problems import attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
MOVES = 5e-2

# irrational slopes (H = 12: n2 = 8, heads 8 .. 11 from the formula's second branch), three q heads per kv head
GQA12 = [
    Spec("split_gqa_merge", "fattn_split_kernel<", 128, "q8_0", (3, 12, 4, 800), kv_chunk=256, tag="_h12"),
    Spec("bd", "fattn_bd_kernel<", 128, "f16", (40, 12, 4, 800), BD, tag="_h12"),
    Spec("pf", "fattn_pf_kernel<f16,D128", 128, "f16", (90, 12, 4, 384), PF1, tag="_h12"),   # (two 85-query tiles)
]
EXACT_H = (1, 2, 4, 8, 6)     # head counts whose slopes at max_bias 8 are all powers of two


def _check(tag, spec, d, got, ref, what="assembled"):
    check_bars(got, ref, lambda e_or, e_el: f"OPPARAMS {spec.id} {tag}: gpu->{what} {e_or:.3e} elem {e_el:.3f} | "
                                            f"{d.split(' grid(')[0]}{d[d.index(' ws '):]}")


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
        _check("alibi", spec, d, got, premultiplied_oracle(spec), what="oracle(premultiplied planes)")


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
