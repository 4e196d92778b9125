"""GPU: attention sinks (ggml FLASH_ATTN_EXT src[4], fattn_ext_sinks) on every
plan and at every site that normalises into dst.

The sink enters once per output row, in the epilogue (include/fattn.h,
DESIGN.md section 12); a miss at one of the sites is silent wrong output, so

  every plan   the rows of tests/plans.py's OP_SPECS with their
               forcing options, under a random mask and no mask (the pf rows
               also under the causal distance mask)
  every site   SITES maps each normalising site to the case that reaches it and
               to what describe() must (and must not) say for that to be so
  above max    sinks ln N + 20 (the s > M branch) against the reference, and
               1e4: finite and below 1e-30
  negligible   sinks -30 against the reference WITHOUT sinks; NULL bit-equal to
               fattn_ext
  masked rows  a plane whose query row 0 is -inf everywhere: exactly 0.0 with
               sinks, still NaN without
  scalars      with max_bias 8 and with logit_softcap 4: the sink is neither
               sloped nor capped
  shards       every rank's slice with HeadShard.sink_slice

against the factor-form reference of tests/sinks.py at the suite's own bound:
attn_rel_err <= 1e-3 and attn_elem_err <= 1, NaN positions coinciding (with
sinks there are none).  Sinks are ln N + linspace(-2, 3, H) under a fixed
non-monotonic permutation of the heads; before a launch the case asserts on
the CPU that they move the reference of EVERY head by >= 5e-2 (MOVES), so a
kernel that ignored them, or took another head's, could not pass.  Launches go
through sinks.SinkGpuView (gpu_util.GuardedLaunch's dst guard bands and
workspace sentinel).  Every case prints one SINKS line with its errors
(profiles/sinks/errors.txt).  No case runs under FATTN_OPT_MERGE_IN_KERNEL
(it may return OK with NaN rows by its own documentation, and waits on other
workgroups); it takes sinks through merge_row_parts like the merge kernels.
"""
from dataclasses import replace

import numpy as np
import pytest

import fattn
import op_cases as t
import op_params as op
import sinks as sk
import views
from fattn import shard
from gpu_util import check_bars
from plans import BD, FAMILIES, IDENT, MQ, OP_BY_ID as BY_ID, OP_SPECS as SPECS, SHARD, Spec
from problems import attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
MOVES = 5e-2

_cache = {}


def sink_values(H, N, lo=-2.0, hi=3.0, centre=None):
    """ln N + linspace(lo, hi, H), head h taking entry (5 h + 3) % H: not monotonic in h.
    centre: what stands for ln N (the rows' typical log-sum-exp) where the scores are not O(1)."""
    vals = (np.log(np.float64(N)) if centre is None else np.float64(centre)) + np.linspace(lo, hi, H)
    return vals[(5 * np.arange(H) + 3) % H].astype(np.float32)


def off_kernel(spec):
    """What describe() names with max_bias / logit_softcap off (sinks never change the plan)."""
    return "fattn_pf4_kernel(lean)" if spec.plan == "pf4shape" else spec.kernel


def _op(spec, kind, scale=None, **kw):
    plane = kind if isinstance(kind, np.ndarray) else t.plane(spec, kind)
    return op.one_plane(t.problem(spec, scale), plane, spec.variants, **kw)


def _plain(spec, kind, scale=None, **kw):
    """op_params.reference without sinks: the cache of tests/op_cases.py (computed once per session)."""
    if isinstance(kind, np.ndarray):
        key = ("plain", spec.id, scale, kind.tobytes(), tuple(sorted(kw.items())))
        if key not in _cache:
            _cache[key] = _op(spec, kind, scale, **kw).reference()
        return _cache[key]
    return t.reference(spec, scale, kind, **kw)


def _ref(spec, kind, sinks, scale=None, **kw):
    key = ("ref", spec.id, scale, kind.tobytes() if isinstance(kind, np.ndarray) else kind, sinks.tobytes(),
           tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = sk.reference(sk.with_sinks(_op(spec, kind, scale, **kw), sinks), plain=_plain(spec, kind, scale, **kw))
    return _cache[key]


def moves_every_head(ref, plain):
    """min over heads of attn_rel_err(reference with sinks, without) -- rows that are NaN without sinks left out."""
    ok = ~np.isnan(plain).any(axis=(0, 2, 3))
    return min(attn_rel_err(ref[:, ok, h:h + 1], plain[:, ok, h:h + 1]) for h in range(ref.shape[2]))


def _launch(spec, sp, dev, want, absent=(), null=False):
    with fattn.options(dict(spec.opts)):
        g = views.GpuView(sp, dev, spec.kv_chunk) if null else sk.SinkGpuView(sp, dev, spec.kv_chunk)
        d = g.describe()
        for w in (want,) if isinstance(want, str) else want:
            assert w in d, (w, d)
        for w in absent:
            assert w not in d, (w, d)
        assert "sink" not in d, d
        got = sk.run_null_sinks(g) if null else g.run()
    assert g.guards_intact(), d
    return d, got


def _check(tag, spec, d, got, ref):
    assert not np.isnan(ref).any()
    check_bars(got, ref, lambda e_or, e_el: f"SINKS {spec.id} {tag}: gpu->factor-form {e_or:.3e} elem {e_el:.3f} | "
                                            f"{d.split(' grid(')[0]}{d[d.index(' ws '):]}")
    assert not np.isnan(got).any(), (spec.id, tag)


def _kernel_for(spec, kind, live=False):
    k = spec.kernel if live else off_kernel(spec)
    return k.replace(" + pf_mask_flags", "") if isinstance(kind, str) and kind == "none" else k


def _case(spec, dev, kind, tag=None, want=None, absent=(), scale=None, centre=None, **kw):
    NQ, H, Hkv, N = spec.shape
    s = sink_values(H, N, centre=centre)
    ref, plain = _ref(spec, kind, s, scale, **kw), _plain(spec, kind, scale, **kw)
    moved = moves_every_head(ref, plain)
    assert moved >= MOVES, (spec.id, kind, moved)                 # (on the CPU: the sinks matter for every head)
    sp = sk.with_sinks(_op(spec, kind, scale, **kw), s)
    d, got = _launch(spec, sp, dev, want if want is not None else _kernel_for(spec, kind, bool(kw)), absent)
    _check(f"{tag or kind} (moves {moved:.2g})", spec, d, got, ref)
    return d, got


# ------------------------------------------------------------------ every plan

IDS = [s.id for s in SPECS]
PF_ROWS = [s for s in SPECS if s.plan in ("pf", "pf4shape")]


@pytest.mark.parametrize("kind", ["random", "none"])
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_every_plan(dev, spec, kind):
    _case(spec, dev, kind)


@pytest.mark.parametrize("spec", PF_ROWS, ids=[s.id for s in PF_ROWS])
def test_prefill_causal(dev, spec):
    _case(spec, dev, "distance")


# ------------------------------------------------------------------ every site

ROW4 = (1, 4, 4, 1024)
CH = (2, 8, 4, 1500)
MQROW, BDROW = BY_ID["mq-D128-q8_0-q40h16kv4n320"], BY_ID["bd-D128-q8_0-q40h2kv2n800"]
MERGE1 = ((fattn.OPT_SPLIT_MERGE, 1),)
FORCED = {s.id: s for s in [
    Spec("row_wave_merge", "fattn_split_kernel<", 128, "q8_0", ROW4, kv_chunk=256),
    Spec("row_wg_merge", "fattn_split_kernel<", 128, "q8_0", ROW4, ((fattn.OPT_SPLIT_WAVES, 8),), kv_chunk=256),
    Spec("row_wg_single", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 256), ((fattn.OPT_SPLIT_WAVES, 8),), kv_chunk=256),
    Spec("tile_single", "fattn_split_kernel<", 128, "q8_0", (3, 8, 2, 800), kv_chunk=1024),
    Spec("merge_f32", "fattn_split_kernel<", 128, "q8_0", CH, kv_chunk=256),
    Spec("merge_f16", "fattn_split_kernel<", 128, "q8_0", CH, ((fattn.OPT_PART_F16, 2),), kv_chunk=256),
    Spec("combine", "fattn_split_kernel<", 128, "q8_0", CH, MERGE1, kv_chunk=256),
    replace(MQROW, plan="mq_combine", opts=MQ + MERGE1, kv_chunk=64),
    replace(MQROW, plan="mq_single", kv_chunk=320),
    replace(MQROW, plan="mq_merge_f32", opts=MQ + ((fattn.OPT_PART_F16, 1),), kv_chunk=64),
    replace(MQROW, plan="mq_merge_f16", opts=MQ + ((fattn.OPT_PART_F16, 2),), kv_chunk=64),
    replace(BDROW, plan="bd_single", kv_chunk=800),
    replace(BY_ID["bdp-D128-q8_0-q64h2kv2n320"], plan="bdp_single", kv_chunk=320),
    replace(BDROW, plan="bd_merge_f32", opts=BD + ((fattn.OPT_PART_F16, 1),)),
    replace(BDROW, plan="bd_merge_f16"),
]}
PF8, PF4ROW = BY_ID["pf-D128-f16-q300h2kv2n384"], BY_ID["pf4shape-D128-f16-q300h2kv2n384"]
ALL = dict(BY_ID, **FORCED)
SPLIT_MERGE, MQ_MERGE, BD_MERGE = " + fattn_merge_kernel", " + fattn_mq_merge_kernel", " + fattn_bd_merge_kernel"
F16P = "(f16 partials)"
# site of the kernels' table -> (case, what describe() must say, what it must not)
SITES = {
    "fattn_split.h wave_merge_epilogue": ("row_wave_merge-D128-q8_0-q1h4kv4n1024", (",4waves>", " grid(4,4,1)"), (SPLIT_MERGE,)),
    "fattn_split.h merge_row_parts (wg_row_merge, last workgroup)":
        ("row_wg_merge-D128-q8_0-q1h4kv4n1024", (",8waves>", " grid(4,4,1)"), (SPLIT_MERGE,)),
    "fattn_split.h wg_row_merge, single chunk": ("row_wg_single-D128-q8_0-q1h4kv4n256", (",8waves>", " grid(1,4,1)"), ()),
    "fattn_split.h split_epilogue EPI 0, single chunk": ("tile_single-D128-q8_0-q3h8kv2n800", (",4waves>", " grid(1,"), ()),
    "fattn_split.h merge_row_parts (fattn_merge_kernel, f32 partials)":
        ("merge_f32-D128-q8_0-q2h8kv4n1500", (SPLIT_MERGE, " grid(6,"), (F16P,)),
    "fattn_split.h merge_row_parts_h (fattn_merge_kernel, f16 partials)":
        ("merge_f16-D128-q8_0-q2h8kv4n1500", (SPLIT_MERGE + F16P, " grid(6,"), ()),
    "fattn_split.h combine_tile": ("combine-D128-q8_0-q2h8kv4n1500", ("fattn_split_kernel<", " grid(6,"), (SPLIT_MERGE,)),
    "fattn_split.h combine_tile (fattn_mq_kernel)": ("mq_combine-D128-q8_0-q40h16kv4n320", ("fattn_mq_kernel<", " grid(5,"), (MQ_MERGE,)),
    "fattn_mq.h single-chunk store": ("mq_single-D128-q8_0-q40h16kv4n320", ("fattn_mq_kernel<", " grid(1,"), (MQ_MERGE,)),
    "fattn_mq.h merge_row_parts (fattn_mq_merge_kernel, f32 partials)":
        ("mq_merge_f32-D128-q8_0-q40h16kv4n320", (MQ_MERGE, " grid(5,"), (F16P,)),
    "fattn_mq.h merge_row_parts_h (fattn_mq_merge_kernel, f16 partials)":
        ("mq_merge_f16-D128-q8_0-q40h16kv4n320", (MQ_MERGE + F16P, " grid(5,"), ()),
    "fattn_bd.h bd_finish, single chunk": ("bd_single-D128-q8_0-q40h2kv2n800", ("fattn_bd_kernel<", " grid(1,"), (BD_MERGE,)),
    "fattn_bd.h merge_row_parts (fattn_bd_merge_kernel, f32 partials)":
        ("bd_merge_f32-D128-q8_0-q40h2kv2n800", ("fattn_bd_kernel<", BD_MERGE), (F16P,)),
    "fattn_bd.h merge_row_parts_h (fattn_bd_merge_kernel, f16 partials)":
        ("bd_merge_f16-D128-q8_0-q40h2kv2n800", ("fattn_bd_kernel<", BD_MERGE + F16P), ()),
    "fattn_bd.h bd_finish, single chunk (fattn_bdp_kernel)": ("bdp_single-D128-q8_0-q64h2kv2n320", ("fattn_bdp_kernel<", " grid(1,"), (BD_MERGE,)),
    "fattn_pf.h final store": (PF8.id, ("fattn_pf_kernel<f16,D128",), ("fattn_pf4_kernel",)),
    "fattn_pf4.h final store": (PF4ROW.id, ("fattn_pf4_kernel(lean)",), ()),
}


@pytest.mark.parametrize("site", list(SITES), ids=[s.replace(" ", "_") for s in SITES])
def test_every_site(dev, site):
    case, want, absent = SITES[site]
    _case(ALL[case], dev, "random", tag=f"site [{site}]", want=want, absent=absent)


# ------------------------------------------------------------------ sink above the max

FIDS = [s.id for s in FAMILIES]


@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_sink_far_above_the_max(dev, spec):
    """ln N + 20: the s > M branch, against the reference at the same bound."""
    NQ, H, Hkv, N = spec.shape
    s = np.full(H, np.log(N) + 20.0, dtype=np.float32)
    ref = _ref(spec, "random", s)
    assert 0 < np.abs(ref).max() < 1e-6
    d, got = _launch(spec, sk.with_sinks(_op(spec, "random"), s), dev, off_kernel(spec))
    _check("ln N + 20", spec, d, got, ref)


@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_huge_sink_is_finite_and_tiny(dev, spec):
    s = np.full(spec.shape[1], 1e4, dtype=np.float32)
    d, got = _launch(spec, sk.with_sinks(_op(spec, "random"), s), dev, off_kernel(spec))
    print(f"SINKS {spec.id} sinks 1e4: max |out| {np.abs(got).max():.3e}")
    assert np.isfinite(got).all() and (np.abs(got) < 1e-30).all()


# ------------------------------------------------------------------ negligible sink, NULL

@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_negligible_sink_is_the_plain_output(dev, spec):
    s = np.full(spec.shape[1], -30.0, dtype=np.float32)
    d, got = _launch(spec, sk.with_sinks(_op(spec, "random"), s), dev, off_kernel(spec))
    _check("sinks -30 vs no-sinks reference", spec, d, got, _plain(spec, "random"))


@pytest.mark.parametrize("spec", IDENT, ids=[s.id for s in IDENT])
def test_null_sinks_is_fattn_ext(dev, spec):
    """fattn_ext_sinks(p, NULL) and fattn_ext(p): the same bits."""
    for kind in ("random", "none"):
        o = _op(spec, kind)
        d0, out0 = t.launch(spec, o, dev, nomask=kind == "none", kernel=off_kernel(spec))
        d1, out1 = _launch(spec, o, dev, _kernel_for(spec, kind), null=True)
        assert d1 == d0
        assert np.array_equal(out1.view(np.uint32), out0.view(np.uint32)), (spec.id, kind)


# ------------------------------------------------------------------ fully masked rows

MASKED = [BY_ID["split_row-D128-q8_0-q1h4kv4n256"], FORCED["merge_f32-D128-q8_0-q2h8kv4n1500"],
          FORCED["tile_single-D128-q8_0-q3h8kv2n800"], BDROW, MQROW, PF8, PF4ROW]


def _row0_masked(spec):
    NQ, _, _, N = spec.shape
    key = ("row0", NQ, N)
    if key not in _cache:
        m = op.random_mask(NQ, N, seed=7)
        m[0] = -np.inf
        _cache[key] = m
    return _cache[key]


@pytest.mark.parametrize("spec", MASKED, ids=[s.id for s in MASKED])
def test_fully_masked_rows_are_zero(dev, spec):
    """Query row 0 is -inf everywhere (NQ = 1: the whole plane): 0.0 exactly
    with sinks, the other rows at the bound; without sinks the row is still NaN."""
    NQ, H, Hkv, N = spec.shape
    m, s = _row0_masked(spec), sink_values(H, N)
    o = _op(spec, m)
    ref, plain = _ref(spec, m, s), _plain(spec, m)
    assert np.isnan(plain[:, 0]).all() and not np.isnan(plain[:, 1:]).any()
    assert (ref[:, 0] == 0.0).all() and not np.isnan(ref).any()
    if NQ > 1:
        assert moves_every_head(ref, plain) >= MOVES
    d, got = _launch(spec, sk.with_sinks(o, s), dev, off_kernel(spec))
    assert (got[:, 0] == 0.0).all(), got[:, 0]
    _check("row 0 masked", spec, d, got, ref)
    d0, got0 = t.launch(spec, o, dev, kernel=off_kernel(spec))
    assert d0 == d
    assert np.isnan(got0[:, 0]).all() and not np.isnan(got0[:, 1:]).any()


# ------------------------------------------------------------------ with max_bias / logit_softcap

@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_sinks_under_max_bias(dev, spec):
    """The sink takes no slope."""
    NQ, H, Hkv, N = spec.shape
    d, got = _case(spec, dev, "distance", tag="alibi", max_bias=8.0)
    assert d.endswith(" alibi 8"), d
    s = sink_values(H, N)
    sloped = sk.reference(sk.with_sinks(_op(spec, "distance", max_bias=8.0), s), sinks=s * op.slopes(8.0, H),
                          plain=_plain(spec, "distance", max_bias=8.0))
    assert attn_rel_err(sloped, _ref(spec, "distance", s, max_bias=8.0)) >= MOVES


@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_sinks_under_softcap(dev, spec):
    """scale 1, logit_softcap 4: the sink is not capped -- the reference with
    4 tanh(s / 4) in its place differs by >= MOVES (CPU).  At scale 1 the scores
    saturate towards +-4 and a row's log-sum-exp lies near ln N + 3, not near
    ln N: sinks of ln N - 2 would move the weakest head by 0.016 only (CPU,
    all five rows), below MOVES.  So the same offsets -2 .. 3 are taken around
    the reference's own mean log-sum-exp (tests/sinks.py scores(), CPU) --
    stronger sinks under the same MOVES precondition."""
    NQ, H, Hkv, N = spec.shape
    key = ("lse", spec.id)
    if key not in _cache:
        _cache[key] = float(np.mean([sk.lse_rows(sc).mean() for _, _, sc in sk.scores(_op(spec, "random", 1.0, logit_softcap=4.0))]))
    d, got = _case(spec, dev, "random", tag=f"softcap (mean lse ln N + {_cache[key] - np.log(N):.2f})", scale=1.0,
                   centre=_cache[key], logit_softcap=4.0)
    assert " softcap 4" in d, d
    s = sink_values(H, N, centre=_cache[key])
    capped = sk.reference(sk.with_sinks(_op(spec, "random", 1.0, logit_softcap=4.0), s),
                          sinks=(4.0 * np.tanh(s.astype(np.float64) / 4.0)).astype(np.float32),
                          plain=_plain(spec, "random", 1.0, logit_softcap=4.0))
    assert attn_rel_err(capped, _ref(spec, "random", s, 1.0, logit_softcap=4.0)) >= MOVES


# ------------------------------------------------------------------ head shards

@pytest.mark.parametrize("world", [2, 4])
def test_head_shards_take_their_slice(dev, world):
    """H = 8, Hkv = 4 over 2 and 4 ranks, every rank's slice launched on this GPU
    with sink_slice: assembled, the unsharded reference.  The unsliced
    sinks[:H_slice] would be wrong by more than MOVES (CPU)."""
    NQ, H, Hkv, N = SHARD.shape
    p = t.problem(SHARD)
    m = t.plane(SHARD, "random")
    s = sink_values(H, N)
    full = _ref(SHARD, "random", s)
    assert moves_every_head(full, _plain(SHARD, "random")) >= MOVES
    parts, wrong = [], []
    for rank in range(world):
        sh = shard.shard_heads(H, Hkv, world, rank)
        sub = make_problem(D=SHARD.D, NQ=NQ, H=sh.n_heads, Hkv=sh.n_kv, N=N, kv_type=SHARD.kt, mask="none", seed=1)
        sub.q = np.ascontiguousarray(p.q[:, :, sh.h0:sh.h1])
        sub.k_bytes = np.ascontiguousarray(p.k_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
        sub.v_bytes = np.ascontiguousarray(p.v_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
        o = op.one_plane(sub, m)
        d, got = _launch(SHARD, sk.with_sinks(o, sh.sink_slice(s)), dev, SHARD.kernel)
        parts.append(got)
        wrong.append(sk.with_sinks(o, s[:sh.n_heads]).reference())
    assert attn_rel_err(np.concatenate(wrong, axis=2), full) > MOVES
    _check(f"world {world}", SHARD, d, np.concatenate(parts, axis=2), full)
