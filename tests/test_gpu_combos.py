"""GPU: logit_softcap, max_bias, sinks, head planes, sequence planes and fully
masked rows, in pairs, with the row log-sum-exp requested, on every (kernel
family, K type, V type, head dim) the library instantiates and at q heads per
kv head that are no power of two (tests/plans.py's CELLS and GQA_CELLS under
the four recipes of tests/combos.py; the table itself is checked on the CPU by
tests/test_combos.py).

Every case, under its cell's options:

  preconditions  on the CPU, before anything launches: turning a live feature
                 off, rotating the head planes by one head, swapping the two
                 sequence planes or shifting head_first by one moves the
                 reference by >= MOVES = 5e-2 (sinks: every head), and a window
                 leaves every head a dead and a live row
  the plan       describe() names the cell's kernel and the live features' markers
  lse            the launch without lse leaves the lse buffer NaN; with it, dst
                 is bit-equal and lse is within lse.check_lse's bar of lse.lse_ref
  dst            attn_rel_err <= 1e-3 and attn_elem_err <= 1 against
                 sinks.reference (Q4_1 / Q5_0 / Q5_1 and BF16: kv_types.check_both)
  guards         dst's, lse's and the exactly-sized workspace's sentinels
  dead rows      with sinks exactly 0.0 and lse = the head's sink, bit for bit;
                 without, NaN and lse = -inf

and prints one `COMBO <id> <recipe>: ...` line with its errors and the plan
before it asserts (profiles/combos/errors.txt).  No case runs under
FATTN_OPT_MERGE_IN_KERNEL (tests/test_gpu_sinks.py says why).
"""
import numpy as np
import pytest

import combos as cb
import fattn
import kv_types as kt
import lse as ls
import views
from gpu_util import check_bars
from problems import attn_elem_err, attn_rel_err

pytestmark = pytest.mark.gpu
_state = {"launch_failed": None}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", cb.CASES, ids=[c.id for c in cb.CASES])
def test_combo(dev, case):
    spec = case.spec
    if _state["launch_failed"]:
        pytest.fail(f"not launched: the launch of {_state['launch_failed']} raised earlier in this process")
    if case.id in cb.REFUSED:                              # (pinned with its status by tests/test_combos.py)
        with pytest.raises(fattn.FattnError) as e:
            cb.describe(case)
        assert e.value.code == cb.REFUSED[case.id]
        return
    b = cb.build(case)
    pre = cb.preconditions(b)
    assert pre and all(v >= cb.MOVES for v in pre.values()), (case.id, pre)
    dead = b.dead
    assert np.array_equal(dead, cb.dead_rows(case))
    assert cb.dead_and_live_per_head(dead) if "w" in case.feats else not dead.any()

    with fattn.options(dict(spec.opts)):
        g = ls.LseLaunch.of(views.GpuView(b.og, dev, spec.kv_chunk, sinks=b.sinks))
        d = g.describe()
        cb.check_plan(case, d)
        assert "lse" not in d and "sink" not in d, d
        try:
            without = g.run_without()
            lse_untouched = bool(np.isnan(g.lse_out()).all())
            got = g.run().copy()
            lse = g.lse_out()
            intact = g.guards_intact()
        except Exception:
            _state["launch_failed"] = case.id               # (a device error is sticky: nothing more is launched)
            raise

    fin = np.isfinite(b.lse)
    with np.errstate(invalid="ignore"):
        lse_err = float(np.abs(lse.astype(np.float64) - b.lse)[fin].max())
    plan = d.split(" grid(")[0] + d[d.index(" ws "):]
    line = (f"COMBO {spec.id} {case.recipe}: [{case.feats}] gpu->reference {attn_rel_err(got, b.ref):.3e} elem {attn_elem_err(got, b.ref):.3f} "
            f"lse {lse_err:.3e} dead rows {int(dead.sum())} moves {min(pre.values()):.2g} | {plan}")
    print(line)

    assert lse_untouched, "the launch without lse wrote lse"
    assert np.array_equal(_bits(got), _bits(without)), f"{case.id}: dst differs from the launch without lse"
    if spec.kt in kt.KV_TYPES:
        kt.check_both(spec.kt, f"combo {case.recipe} {spec.id}", plan, got, b.ref, b.f64)
    else:
        check_bars(got, b.ref, lambda rel, elem: line)
    ls.check_lse(lse, b.lse, f"{case.id} | {plan}")
    assert intact, d

    if dead.any():
        if b.sinks is not None:
            want = np.broadcast_to(b.sinks[None, None, :], lse.shape)
            assert (got[dead] == 0.0).all(), "a fully masked row with a sink is exactly 0.0"
            assert np.array_equal(_bits(lse[dead]), _bits(want[dead])), "a fully masked row's lse is its head's sink"
        else:
            assert np.isnan(got[dead]).all() and np.isneginf(lse[dead]).all()
    assert not np.isnan(got[~dead]).any()
