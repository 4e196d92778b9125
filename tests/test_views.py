"""The tensor-view contract on the CPU: the oracle honours ne/nb on every view
variant (tests/views.py) bit for bit, the oracle stays within half the 1e-3 bar
of a float64 reference, and the planner keeps, changes or rejects the plan on a
view exactly as make_plan documents (host-only planning, as in test_abi.py)."""
import functools

import numpy as np
import pytest

import fattn
import views
from problems import attn_rel_err, make_problem

RTOL = 1e-3
ERR_ALIGNMENT = -7


# ------------------------------------------------------------------ oracle invariance

@functools.lru_cache(maxsize=None)
def _inv_problem(D, kt):
    p = make_problem(D=D, NQ=5, H=4, Hkv=2, N=200, S=2, kv_type=kt, seed=D + len(kt))
    return p, p.oracle()


INV_VARIANTS = [(v,) for v in views.ALL_VARIANTS] + [(), views.COMPOSED, views.COMPOSED16]


@pytest.mark.parametrize("variants", INV_VARIANTS, ids=lambda v: "+".join(v) if len(v) < 3 else f"composed{len(v)}")
@pytest.mark.parametrize("kt", ["f16", "q8_0", "q4_0"])
@pytest.mark.parametrize("D", [64, 128])
def test_oracle_invariant_under_views(D, kt, variants):
    """Only addresses change, so the oracle's output must not: bit-identical to
    the canonical layout's, with every gap, pad row / column and guard poisoned."""
    p, ref = _inv_problem(D, kt)
    vp = views.make_view(p, *variants)
    got = vp.oracle()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.isnan(ref).any()


def test_views_are_poisoned_and_strided():
    """The builder itself: strides as the issue names them, NaN in every gap."""
    p, _ = _inv_problem(64, "q8_0")
    D, NQ, H, N = p.D, p.NQ, p.H, p.N
    vp = views.make_view(p, "q_headmajor")
    assert vp.q.nb == (4, D * 4, NQ * D * 4, H * NQ * D * 4)
    vp = views.make_view(p, "q_rowpad", "q_offset")
    assert vp.q.nb == (4, H * (D * 4 + 16), D * 4 + 16, (NQ * H + 1) * (D * 4 + 16)) and vp.q.off == 32
    qf = vp.q.data.view(np.float32)
    assert np.isnan(qf).sum() == qf.size - p.q.size          # everything but the logical elements
    vp = views.make_view(p, "m_wide16", "m_rows", "m_cols", "m_align4")
    assert vp.mask.ne == (256, 32, 1, 1) and vp.mask.nb[1] == 256 * 2 + 32 and vp.mask.off == 4
    mb = vp.mask.data.view(np.uint16)
    assert (mb == views.F16_NAN).sum() == mb.size - NQ * N
    vp = views.make_view(p, "kv_ctx", "kv_offset16", "kv_nb3_gap")
    rb = 68
    assert vp.k.nb == (34, rb, (N + 96) * rb, p.Hkv * (N + 96) * rb + 256) and vp.k.off == 16
    assert (vp.k.data == views.KV_POISON).sum() >= vp.k.data.size - p.k_bytes.size
    vp = views.make_view(p, "kv_split_layout")
    assert vp.k.nb[1] == rb and vp.v.nb[1] == p.Hkv * rb and vp.v.nb[2] == rb
    assert views.make_view(p, "m_stride4").mask.nb[1] % 16 == 4


# ------------------------------------------------------------------ oracle vs float64

SCALES = [None, 0.25, 1.0, 0.01, 0.0, -0.1]


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "default" if s is None else f"{s:g}")
@pytest.mark.parametrize("kt", ["f16", "q8_0", "q4_0"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_oracle_within_half_the_bar_of_float64(D, kt, scale):
    """The f32 oracle rounds the normalised probabilities to f16: a noisy ruler.
    Against a float64 softmax-attention over the same f16-rounded inputs it
    stays under RTOL / 2 (measured 2.6e-4 ... 4.7e-4 on this grid), so a kernel
    within RTOL of the oracle is within 1.5 RTOL of the true value at worst."""
    worst = 0.0
    for seed in range(3):
        p = make_problem(D=D, NQ=4, H=4, Hkv=2, N=512, kv_type=kt, seed=seed, scale=scale)
        worst = max(worst, attn_rel_err(p.oracle(), views.exact_f64(p)))
    print(f"oracle->exact_f64 D={D} {kt} scale={scale}: {worst:.3g}")
    assert worst <= RTOL / 2, worst


def test_exact_f64_masked_rows_are_nan():
    p = make_problem(D=64, NQ=3, H=2, N=64, kv_type="f16", seed=1)
    p.mask_bits[1, :p.N] = 0xFC00   # -inf over the first N positions of row 1
    ex, ref = views.exact_f64(p), p.oracle()
    assert np.isnan(ex[:, 1]).all() and not np.isnan(ex[:, [0, 2]]).any()
    assert np.array_equal(np.isnan(ex), np.isnan(ref))


# ------------------------------------------------------------------ planner on views

# (name, options, problem) -- the plans of the GPU matrix at their smallest shapes
PLANS = {
    "split": ({}, dict(D=128, NQ=1, H=4, Hkv=4, N=256)),
    "split_gqa": ({}, dict(D=64, NQ=3, H=8, Hkv=2, N=800)),
    "mq": ({fattn.OPT_MQ_MIN_ROWS: 32, fattn.OPT_BD: 1}, dict(D=128, NQ=40, H=16, Hkv=4, N=320)),
    "bd": ({fattn.OPT_BD: 2}, dict(D=128, NQ=40, H=2, Hkv=2, N=800)),
    "bdp": ({fattn.OPT_BD: 3}, dict(D=64, NQ=64, H=2, Hkv=2, N=320)),
    "pf": ({fattn.OPT_PF: 2}, dict(D=128, NQ=300, H=2, Hkv=2, N=384)),
}
PLAN_KERNEL = {"split": "fattn_split_kernel", "split_gqa": "fattn_split_kernel", "mq": "fattn_mq_kernel",
               "bd": "fattn_bd_kernel", "bdp": "fattn_bdp_kernel", "pf": "fattn_pf"}
ALIGNED = [(v,) for v in views.COMPOSED16] + [views.COMPOSED16]


@functools.lru_cache(maxsize=None)
def _plan_problem(plan, kt):
    return make_problem(S=2, kv_type=kt, seed=3, **PLANS[plan][1])


# (the multi-query and role-form kernels take Q8_0 / Q4_0 only)
PLAN_TYPES = [(pl, kt) for pl in PLANS for kt in ("f16", "q8_0", "q4_0") if not (pl in ("mq", "bdp") and kt == "f16")]


@pytest.mark.parametrize("plan,kt", PLAN_TYPES)
def test_aligned_views_keep_the_plan(plan, kt):
    """A 16-B-aligned Q, mask or KV view is the canonical problem at other
    addresses: the whole plan string (kernel, grid, LDS, chunking, workspace)
    stays."""
    p = _plan_problem(plan, kt)
    with fattn.options(PLANS[plan][0]):
        canon = fattn.describe(views.make_view(p).params())
        assert PLAN_KERNEL[plan] in canon, canon
        for vs in ALIGNED:
            d = fattn.describe(views.make_view(p, *vs).params())
            assert d == canon, (vs, d, canon)
        # (f16 rows: a "pos" layout keeps 16-B rows, so it keeps the plan too)
        if kt == "f16":
            for vs in (("kv_split_layout",), ("kv_split_layout_r",), ("kv_pos",)):
                d = fattn.describe(views.make_view(p, *vs).params())
                assert d == canon, (vs, d, canon)


# (f16 rows in the pos layout stay on the 16-B path: test_aligned_views_keep_the_plan)
DWORD_CASES = [(pl, kt, v) for pl in ("split", "mq", "bd", "bdp", "pf") for kt in ("f16", "q8_0", "q4_0")
               for v in ("m_align4", "m_stride4", "kv_offset4", "kv_split_layout", "kv_split_layout_r")
               if not (v.startswith("kv_split_layout") and kt == "f16")]


@pytest.mark.parametrize("plan,kt,variant", DWORD_CASES)
def test_dword_views_take_the_split_kernel(plan, kt, variant):
    """A mask or K/V base (or mask row stride) that is only 4-byte aligned, or a
    quantised K or V in the "pos" layout (rows of one head not contiguous),
    turns the 16-B fast path off: the split kernel at gran = 4 whatever the
    options asked for."""
    p = _plan_problem(plan, kt)
    with fattn.options(PLANS[plan][0]):
        d = fattn.describe(views.make_view(p, variant).params())
    assert d.startswith("fattn_split_kernel<") and ",gran4," in d, d


@pytest.mark.parametrize("variant", ["m_align4", "kv_offset4", "kv_split_layout", "kv_nb3_gap"])
@pytest.mark.parametrize("kt", ["q8_0", "q4_0"])
def test_d96_quant_dword_views(kt, variant):
    """D = 96 Q8_0 / Q4_0 rows are 102 / 54 B, not dword multiples: the dword
    path cannot address them (make_plan: FATTN_ERR_ALIGNMENT), the 16-B path can."""
    p = make_problem(D=96, NQ=1, H=4, Hkv=4, N=256, S=2, kv_type=kt, seed=4)
    prm = views.make_view(p, variant).params()
    if variant == "kv_nb3_gap":
        assert ",gran16," in fattn.describe(prm)
        return
    with pytest.raises(fattn.FattnError) as e:
        fattn.describe(prm)
    assert e.value.code == ERR_ALIGNMENT
    # (the same for a cache length that is no multiple of 32 rows)
    p = make_problem(D=96, NQ=9, H=8, Hkv=2, N=300, kv_type=kt, seed=4)
    with pytest.raises(fattn.FattnError) as e:
        fattn.describe(views.make_view(p).params())
    assert e.value.code == ERR_ALIGNMENT


@pytest.mark.parametrize("variant", ["q_offset4", "q_offset8"])
@pytest.mark.parametrize("plan", ["split", "pf"])
def test_q_offset_below_16_rejected(plan, variant):
    p = _plan_problem(plan, "q8_0")
    with fattn.options(PLANS[plan][0]):
        with pytest.raises(fattn.FattnError) as e:
            fattn.describe(views.make_view(p, variant).params())
        assert e.value.code == ERR_ALIGNMENT
        assert fattn.workspace_size(views.make_view(p, variant).params()) == 0


@pytest.mark.parametrize("scale", [0.0, -0.1, -1e-30])
@pytest.mark.parametrize("kt", ["f16", "q8_0"])
@pytest.mark.parametrize("shape,pf_opt", [
    (dict(D=128, NQ=300, H=2, Hkv=2, N=384), 2),         # the GPU matrix's shape: pf by FATTN_OPT_PF = 2 only
    (dict(D=64, NQ=4096, H=32, Hkv=32, N=4096), 0),      # a prefill the planner gives to pf by itself
    (dict(D=64, NQ=4096, H=32, Hkv=32, N=4096), 2),
], ids=["small-pf2", "prefill-auto", "prefill-pf2"])
def test_nonpositive_scale_never_plans_pf(shape, kt, scale, pf_opt):
    """The prefill kernels fold the scale into the exponent after the row max,
    which is the max of the scaled scores only for scale > 0: make_plan keeps
    them for positive scales and plans another kernel (no error) otherwise."""
    D, NQ, H, Hkv, N = (shape[k] for k in ("D", "NQ", "H", "Hkv", "N"))
    typ = fattn.TYPE_NAMES[kt]
    rb = fattn.row_size(typ, D)
    eb = 2 if kt == "f16" else fattn.BLOCK_BYTES[typ]
    ptr = views.FAKE_BASE
    kv = fattn.View(ptr, typ, (D, N, Hkv, 1), (eb, rb, rb * N, rb * N * Hkv))
    q = fattn.View(ptr, fattn.TYPE_F32, (D, NQ, H, 1), (4, H * D * 4, D * 4, NQ * H * D * 4))
    m = fattn.View(ptr, fattn.TYPE_F16, (N, NQ, 1, 1), (2, N * 2, N * 2 * NQ, N * 2 * NQ))
    with fattn.options({fattn.OPT_PF: pf_opt}):
        pos = fattn.describe(fattn.ext_params(q, kv, kv, m, ptr, 0.125))
        assert "fattn_pf" in pos, pos
        d = fattn.describe(fattn.ext_params(q, kv, kv, m, ptr, scale))   # (raises unless FATTN_OK)
    assert "fattn_pf" not in d and "pf_prepass" not in d, d
