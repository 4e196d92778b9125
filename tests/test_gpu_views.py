"""GPU: the tensor-view contract of include/fattn.h on every plan.

Each case takes one plan at its smallest shape and changes one thing about how
the tensors are addressed (tests/views.py) or the scale, then

  (a) asserts fattn_describe names the intended kernel (a view that silently
      fell back to the split kernel would test nothing),
  (b) compares with the CPU oracle run on the same views: attn_rel_err <= 1e-3
      and attn_elem_err <= 1, the suite's bounds,
  (c) so NaN positions coincide with the oracle's (both error functions return
      inf otherwise): one poisoned gap, pad row / column or context row leaking
      into any output element fails the case,
  (d) where the plan string equals the canonical layout's, requires the output
      bit-identical to the canonical-layout run: only addresses changed,
  (e) checks dst's 4 KiB guard bands and the sentinel behind the exactly-sized
      workspace.

Scale cases also compare with the float64 reference (views.exact_f64) at the
same 1e-3 and print both distances (the table of DESIGN.md section 5).
"""
import numpy as np
import pytest

import fattn
import views
from plans import Spec
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-3

QUANT = ("q8_0", "q4_0")
ALL3 = ("f16", "q8_0", "q4_0")
Q_ALL = ("q_headmajor", "q_rowpad", "q_offset")


def _specs():
    s = []
    for D in (64, 128, 256):
        for kt in ALL3:
            s.append(Spec("split_row", "fattn_split_kernel<", D, kt, (1, 4, 4, 256)))
            s.append(Spec("split_row_tail", "fattn_split_kernel<", D, kt, (1, 4, 4, 200)))
    for kt in ALL3:
        s.append(Spec("split_chunks", "fattn_split_kernel<", 128, kt, (2, 8, 4, 1500), kv_chunk=256))
        s.append(Spec("split_gqa_merge", "fattn_split_kernel<", 128, kt, (3, 8, 2, 800), kv_chunk=256))
    for shape in ((1, 4, 4, 256), (9, 8, 2, 300)):
        s.append(Spec("split_d80", "fattn_split_kernel<", 80, "f16", shape))
        # (D = 96 Q8_0 / Q4_0 rows are no dword multiple: N = 300 is rejected, test_views.py)
        for kt in (ALL3 if shape[3] % 32 == 0 else ("f16",)):
            s.append(Spec("split_d96", "fattn_split_kernel<", 96, kt, shape))
    mq = ((fattn.OPT_MQ_MIN_ROWS, 32), (fattn.OPT_BD, 1))
    for D in (64, 128):
        for kt in QUANT:
            s.append(Spec("mq", "fattn_mq_kernel<", D, kt, (40, 16, 4, 320), mq))
    s.append(Spec("mq", "fattn_mq_kernel<q8_0,D256,4waves", 256, "q8_0", (50, 2, 2, 320), mq))
    for kt in ("q8_0", "f16"):
        s.append(Spec("bd", "fattn_bd_kernel<", 128, kt, (40, 2, 2, 800), ((fattn.OPT_BD, 2),)))
    for D in (64, 128):
        for kt in QUANT:
            s.append(Spec("bdp", "fattn_bdp_kernel<", D, kt, (64, 2, 2, 320), ((fattn.OPT_BD, 3),)))
    pf1 = ((fattn.OPT_PF, 2), (fattn.OPT_PF_FORM, 1))
    for D in (64, 96, 128):
        s.append(Spec("pf", f"fattn_pf_kernel<f16,D{D}", D, "f16", (300, 2, 2, 384), pf1))
        s.append(Spec("pf", f"kv_stage_f16<q8_0> + pf_mask_flags] + fattn_pf_kernel<f16,D{D}", D, "q8_0",
                      (300, 2, 2, 384), pf1, tag="_staged"))
        s.append(Spec("pf", f"fattn_pf_kernel<q8_0,D{D}", D, "q8_0", (300, 2, 2, 384),
                      pf1 + ((fattn.OPT_PF_STAGE, 1),), tag="_inkernel"))
    s.append(Spec("pf", "fattn_pf_kernel<f16,D80", 80, "f16", (300, 2, 2, 384), ((fattn.OPT_PF, 2),)))
    pf = ((fattn.OPT_PF, 2),)
    s.append(Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128", 128, "f16", (300, 2, 2, 384), pf))
    s.append(Spec("pf4", "kv_stage_f16<q8_0> + pf_mask_flags] + fattn_pf4_kernel(lean)<f16,D128", 128, "q8_0",
                  (300, 2, 2, 384), pf, tag="_staged"))
    s.append(Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128,mask", 128, "f16", (300, 2, 2, 384), pf, mask="zero",
                  tag="_zeromask"))
    s.append(Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128,nomask", 128, "f16", (300, 2, 2, 384), pf, mask="none",
                  tag="_nomask"))
    return s


SPECS = _specs()
DWORD = ("m_align4", "m_stride4", "kv_offset4")


def _lands_on_dword_split(spec, variants):
    """The variants that turn the 16-B path off (make_plan's g16)."""
    return any(v in DWORD for v in variants) or (spec.kt != "f16" and any(v.startswith("kv_split_layout") for v in variants))


def _valid(spec, variant):
    NQ, H, Hkv, N = spec.shape
    if variant.startswith("m_") and spec.mask == "none":
        return False
    if variant == "m_cols" and N % 64 == 0:
        return False     # (split, and bd at N = 800: the other plans need N % 64 == 0)
    # D = 96 Q8_0 / Q4_0 cannot take the dword path at all (FATTN_ERR_ALIGNMENT, test_views.py)
    return not (spec.D == 96 and spec.kt != "f16" and _lands_on_dword_split(spec, (variant,)))


def _axes(spec):
    """The cases every (plan, D, type) gets: (axis id, variants, scale)."""
    out = [("canonical", (), None), ("q_all", Q_ALL, None),
           ("all16", tuple(v for v in views.COMPOSED16 if _valid(spec, v)), None)]
    if spec.family == "split" or spec.kt == "f16":
        # split: every type; f16 rows in the pos layout keep the plan's kernel
        dword = ("kv_split_layout", "kv_split_layout_r", "kv_offset4")
        if spec.family != "split":
            dword += ("m_align4",)
        elif spec.plan == "split_row" and spec.D == 128:
            dword += ("m_align4", "m_stride4")
    elif spec.tag != "_inkernel":
        # Q8_0 / Q4_0 on the other plans land on the dword split kernel: many query tiles there
        dword = ("m_align4", "kv_split_layout", "kv_offset4")
    else:
        dword = ()       # (the same views and split kernel as the staged spec)
    out += [(v, (v,), None) for v in dword if _valid(spec, v)]
    out += [("scale1", (), 1.0), ("scale0.01", (), 0.01)]
    out += [("scale0", (), 0.0), ("scale-0.1", (), -0.1)]    # (pf / pf4: the planner must leave the prefill kernels)
    return out


SINGLES = Q_ALL + ("m_wide16", "m_rows", "m_cols", "kv_ctx", "kv_offset16", "kv_nb3_gap")


def _cases():
    """One case per axis value and row of the plan table, not the product: the
    compositions, the dword views and the scales run on every (D, type) of a
    row, each single aligned variant on one of them in turn."""
    cases = [(s, a) for s in SPECS for a in _axes(s)]
    rows = {}
    for s in SPECS:
        rows.setdefault(s.row, []).append(s)
    for specs in rows.values():
        turn = 0
        for v in SINGLES:
            for k in range(len(specs)):
                s = specs[(turn + k) % len(specs)]
                if _valid(s, v):
                    cases.append((s, (v, (v,), None)))
                    turn += k + 1
                    break
    return sorted(cases, key=lambda c: SPECS.index(c[0]))    # (stable: a spec's cases stay together)


CASES = _cases()

_problems, _canon, _exact = {}, {}, {}


def _problem(spec):
    if spec.id not in _problems:
        NQ, H, Hkv, N = spec.shape
        _problems[spec.id] = make_problem(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, S=2, kv_type=spec.kt, mask=spec.mask,
                                          seed=SPECS.index(spec) + 100)
    return _problems[spec.id]


def _canonical(spec, dev):
    """The canonical layout's plan string and output at the default scale, run
    once per spec (under the spec's options, which the caller holds)."""
    if spec.id not in _canon:
        g = views.GpuView(views.make_view(_problem(spec)), dev, spec.kv_chunk)
        _canon[spec.id] = (g.describe(), g.run())
    return _canon[spec.id]


def _exact_f64(spec, scale):
    key = (spec.id, scale)
    if key not in _exact:
        _exact[key] = views.exact_f64(_problem(spec), scale)
    return _exact[key]


@pytest.mark.parametrize("spec,axis", CASES, ids=[f"{s.id}-{a[0]}" for s, a in CASES])
def test_view(dev, spec, axis):
    name, variants, scale = axis
    p = _problem(spec)
    vp = views.make_view(p, *variants, scale=scale)
    with fattn.options(dict(spec.opts)):
        canon_plan, canon_out = _canonical(spec, dev)
        assert spec.kernel in canon_plan, canon_plan
        g = views.GpuView(vp, dev, spec.kv_chunk)
        d = g.describe()
        # (a) the intended kernel
        if _lands_on_dword_split(spec, variants):
            assert d.startswith("fattn_split_kernel<") and ",gran4," in d, d
        elif spec.family in ("pf", "pf4") and scale is not None and scale <= 0:
            assert "fattn_pf" not in d and "pf_prepass" not in d, d
        else:
            assert spec.kernel in d, d
        got = g.run()
    # (b), (c) the oracle on the same views
    ref = vp.oracle()
    e_or, e_el = attn_rel_err(got, ref), attn_elem_err(got, ref)
    line = f"VIEWS {spec.id} {name}: gpu->oracle {e_or:.3e} elem {e_el:.3f}"
    e_ex = None
    if not variants:
        e_ex = attn_rel_err(got, _exact_f64(spec, scale))
        line += f" gpu->exact_f64 {e_ex:.3e}"
    print(line + " | " + d.split(" grid(")[0])
    assert e_or <= RTOL, line
    assert e_el <= 1.0, line
    if e_ex is not None:
        assert e_ex <= RTOL, line
    # (d) same plan, other addresses: the same bits
    if scale is None and d == canon_plan:
        assert np.array_equal(got.view(np.uint32), canon_out.view(np.uint32)), line
    # (e) nothing written outside dst and the workspace
    assert g.guards_intact(), line


@pytest.mark.parametrize("spec", SPECS, ids=[s.id for s in SPECS])
def test_canonical_layout_is_deterministic(dev, spec):
    """The premise of (d): the canonical layout run again, on fresh buffers,
    gives the same bits."""
    with fattn.options(dict(spec.opts)):
        plan, out = _canonical(spec, dev)
        g = views.GpuView(views.make_view(_problem(spec)), dev, spec.kv_chunk)
        assert g.describe() == plan
        for _ in range(2):
            assert np.array_equal(g.run().view(np.uint32), out.view(np.uint32)), plan
        assert g.guards_intact()
