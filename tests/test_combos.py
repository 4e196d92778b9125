"""The covering table of tests/combos.py on the CPU: its size, what every case
plans (fattn.describe over fake pointers, nothing launches), the pairs each
kernel family gets, and that every case's inputs can tell a kernel that honours
a feature from one that drops it or gives it to the wrong head."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import combos as cb
import fattn
import lse as ls
import op_params as op
import plans

# (kernel, K type, V type, head dim) per row of the table: has_kernel, csrc/fattn_launch.h:53 (MLA left out).
# "split" cells run at two shapes; "pf_staged" is no row of has_kernel -- kv_stage_f16<type> in front of the f16 bodies
CELL_COUNTS = {"split": 25, "split_vT": 5, "split_mixed": 18, "mq": 6, "pf": 10, "pf_staged": 15, "pf4": 1, "bd": 5, "bdp": 6}
N_SPECS = 116      # 25 x 2 + 66
N_GQA = 7
N_CASES = 478      # 116 x 4 recipes + 7 x 2


def test_counts():
    got = {g: len({(s.family, s.kt, s.vt, s.v_trans, s.D, s.tag) for s in specs}) for g, specs in plans.CELL_GROUPS.items()}
    assert got == CELL_COUNTS
    assert len(plans.CELL_GROUPS["split"]) == 50 and {s.shape for s in plans.CELL_GROUPS["split"]} == {(1, 4, 4, 544), (3, 8, 2, 800)}
    assert len(plans.CELLS) == N_SPECS and len(plans.GQA_CELLS) == N_GQA and len(cb.CASES) == N_CASES
    assert len({c.id for c in cb.CASES}) == N_CASES
    assert sorted(s.rk2 for s in plans.GQA_CELLS) == [6, 6, 6, 6, 7, 7, 20]
    assert all(c.recipe in ("R1", "R2") for c in cb.CASES if c.spec in plans.GQA_CELLS)


def test_cells_are_the_library_s():
    """Every cell plans (under its options, a plain mask) the kernel it names, and the types and head dims
    next to the table's are refused or land elsewhere: the table is has_kernel's, not a subset of it."""
    def plan(kt, D, vt=None, **kw):
        p = plans.plan_params(D=D, kt=fattn.TYPE_NAMES[kt], vt=fattn.TYPE_NAMES[vt] if vt else None, **kw)
        try:
            return fattn.describe(p)
        except fattn.FattnError as e:
            return e.code
    assert plan("q8_0", 80) < 0 and plan("q4_1", 96) < 0 and plan("bf16", 96) < 0 and plan("q5_0", 80) < 0
    assert plan("q8_0", 96, "f16") < 0 and plan("q4_1", 128, "f16") < 0 and plan("bf16", 128, "f16") < 0
    with fattn.options(dict(plans.MQ)):
        assert "fattn_mq_kernel" not in plan("q8_0", 96, NQ=40, H=16, Hkv=4, N=320)
        assert "fattn_mq_kernel" not in plan("f16", 128, NQ=40, H=16, Hkv=4, N=320)
    with fattn.options(dict(plans.BD)):
        assert "fattn_bd_kernel" not in plan("q8_0", 64, NQ=40, H=2, Hkv=2, N=800)
        assert "fattn_bd_kernel" not in plan("f16", 256, NQ=40, H=2, Hkv=2, N=800)
    with fattn.options(dict(plans.BDP)):
        assert "fattn_bdp_kernel" not in plan("f16", 128, NQ=64, H=2, Hkv=2, N=320)
        assert "fattn_bdp_kernel" not in plan("q8_0", 256, NQ=64, H=2, Hkv=2, N=320)
    with fattn.options(dict(plans.PF1)):
        assert "fattn_pf" not in plan("f16", 256, NQ=300, H=2, Hkv=2, N=384)
        assert "fattn_pf" not in plan("q8_0", 256, NQ=300, H=2, Hkv=2, N=384)


def test_recipes_cover_every_pair():
    every = cb.pairs(cb.ORDER)
    assert len(every) == 15
    assert set().union(*(cb.pairs(f) for f in cb.RECIPES.values())) == every
    assert len(set().union(*(cb.pairs(f) for f in cb.MQ_RECIPES.values()))) == 10
    assert len(set().union(*(cb.pairs(f) for f in cb.PF4_RECIPES.values()))) == 6
    assert all("h" not in f for f in cb.MQ_RECIPES.values()) and all("c" not in f and "a" not in f for f in cb.PF4_RECIPES.values())


@pytest.mark.parametrize("family,n", [("split", 15), ("bd", 15), ("bdp", 15), ("pf", 15), ("mq", 10), ("pf4", 6)])
def test_pairs_per_family(family, n):
    """The union of live-feature pairs over the family's cases, each cell taken alone."""
    cells = [s for s in plans.CELLS if s.family == family]
    assert cells
    for s in cells:
        got = set().union(*(cb.pairs(c.feats) for c in cb.CASES if c.spec == s))
        assert len(got) == n, (s.id, sorted(got))
    # the one-row substitution (w brings q) adds pairs, it drops none
    assert all(set(cb.features(s, r)) >= set(cb.RECIPES[r]) for s in cells for r in cb.RECIPES if family not in ("mq", "pf4"))


GROUPS = list(plans.CELL_GROUPS) + ["gqa"]


def _cases_of(group):
    specs = plans.GQA_CELLS if group == "gqa" else plans.CELL_GROUPS[group]
    return [c for c in cb.CASES if c.spec in specs]


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_plans_its_kernel_with_its_markers(group):
    """describe() names the cell's kernel with its <kt,(vt,)D... arguments and carries
    ' softcap 4', ' alibi 8' and ' mask planes (H,S)' exactly where the feature is live."""
    for c in _cases_of(group):
        if c.id in cb.REFUSED:
            continue
        d = cb.describe(c)
        cb.check_plan(c, d)
        assert "lse" not in d and "sink" not in d, d
        if c.spec.plan == "split_gqa_merge":
            assert " + fattn_merge_kernel" in d, d              # the chunks merge in a second launch
        if c.spec.plan == "split_row5":
            assert " grid(5,4," in d and " + fattn_merge_kernel" not in d, d


def test_refused_cases_return_their_status():
    """A cell x recipe the library refuses is pinned with its status, not skipped (the table holds none today)."""
    assert set(cb.REFUSED) <= set(cb.BY_ID)
    for cid, status in cb.REFUSED.items():
        with pytest.raises(fattn.FattnError) as e:
            cb.describe(cb.BY_ID[cid])
        assert e.value.code == status, cid


@pytest.mark.parametrize("group", GROUPS)
def test_window_cases_have_dead_and_live_rows_per_head(group):
    n = 0
    for c in _cases_of(group):
        if "w" in c.feats:
            assert cb.dead_and_live_per_head(cb.dead_rows(c)), c.id
            n += 1
        else:
            assert not cb.dead_rows(c).any(), c.id
    assert n >= len(_cases_of(group)) // 2


# one cell per family: its four recipes' preconditions
PRE_CELLS = ["split_gqa_merge-D64-q8_0-q3h8kv2n800", "split_row5-D128-q5_1-q1h4kv4n544", "mq-D64-q4_0-q40h16kv4n320",
             "bd-D64-f16-q40h2kv2n800", "bdp-D64-q8_0-q64h2kv2n320", "pf-D64-f16-q300h2kv2n384", "pf4-D128-f16-q300h2kv2n384"]


@pytest.mark.parametrize("recipe", list(cb.RECIPES))
@pytest.mark.parametrize("cell", PRE_CELLS)
def test_preconditions(cell, recipe):
    """Turning c or a off, dropping the sinks (every head), rotating the head planes by one head, swapping the
    two sequence planes, shifting head_first by one: each moves the reference by MOVES or more."""
    c = cb.BY_ID[f"{cell}-{recipe}"]
    b = cb.build(c)
    pre = cb.preconditions(b)
    want = {"c": "c off", "a": "a off", "s": "s off, every head", "h": "h rotated", "q": "q swapped"}
    assert set(pre) == {want[f] for f in c.feats if f in want} | ({"head_first - 1"} if c.second_half else set())
    assert all(v >= cb.MOVES for v in pre.values()), (c.id, pre)
    assert np.array_equal(b.dead, cb.dead_rows(c))
    if cell.startswith("split"):                                # the references taken per sequence are the whole ones, bit for bit
        assert np.array_equal(b.plain, op.reference(b.o), equal_nan=True)
        assert np.array_equal(b.lse_plain, ls.lse_ref(b.o))
    if b.sinks is not None:
        off = ls.sink_values(len(b.sinks), 1)                    # (centre ln 1 = 0: the offsets alone)
        assert len(set(off.tolist())) == len(off) and (len(off) < 3 or ((np.diff(off) < 0).any() and (np.diff(off) > 0).any()))
        assert np.array_equal(b.lse, ls.lse_ref(b.o, b.sinks)) and not np.isnan(b.ref).any() and (b.ref[b.dead] == 0.0).all()
    else:
        assert np.isnan(b.ref[b.dead]).all() and not np.isnan(b.ref[~b.dead]).any()


def test_lse_bar_is_unchanged():
    assert ls.REF_WORST == 2.315e-6 and ls.LSE_ATOL == 8 * ls.REF_WORST


@pytest.mark.slow
@pytest.mark.parametrize("group", GROUPS)
def test_lse_reference_uncertainty(group):
    """lse.ref_uncertainty(o) <= lse.REF_WORST for every case whose lse reference rests on the
    oracle's f32 scores (BF16's is the float64 one): the bar of tests/lse.py holds as it is."""
    cases = [c for c in _cases_of(group) if not c.f64]

    def one(c):
        return c.id, ls.ref_uncertainty(cb.problem_of(c)[0])
    with ThreadPoolExecutor(8) as ex:
        got = dict(ex.map(one, cases))
    worst = max(got, key=got.get)
    print(f"COMBO {group}: worst lse reference uncertainty {got[worst]:.3e} ({worst}); bar {ls.REF_WORST:.3e}")
    assert got[worst] <= ls.REF_WORST, {k: v for k, v in got.items() if v > ls.REF_WORST}
