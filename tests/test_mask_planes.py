"""Mask planes (mask ne[2] / ne[3], include/fattn.h) on the CPU: what make_plan
accepts, rejects and plans (host-only planning, as in test_views.py), the 4-D
mask_view, and the test builder's own assembled oracle (tests/mask_planes.py)."""
import functools

import numpy as np
import pytest

import fattn
import mask_planes as mp
import views
from problems import make_problem

ERR_INVALID_ARG, ERR_ALIGNMENT = -1, -7

# (name: options, problem) -- the plans of test_views.py at their smallest shapes, H a multiple of 4
PLANS = {
    "split": ({}, dict(D=128, NQ=1, H=4, Hkv=4, N=256)),
    "split_gqa": ({}, dict(D=64, NQ=3, H=8, Hkv=2, N=800)),
    "mq": ({fattn.OPT_MQ_MIN_ROWS: 32, fattn.OPT_BD: 1}, dict(D=128, NQ=40, H=16, Hkv=4, N=320)),
    "bd": ({fattn.OPT_BD: 2}, dict(D=128, NQ=40, H=2, Hkv=2, N=800)),
    "bdp": ({fattn.OPT_BD: 3}, dict(D=64, NQ=64, H=2, Hkv=2, N=320)),
    "pf": ({fattn.OPT_PF: 2}, dict(D=128, NQ=300, H=2, Hkv=2, N=384)),
}


@functools.lru_cache(maxsize=None)
def _problem(plan, S=2, mask="none"):
    return make_problem(S=S, kv_type="q8_0", seed=5, mask=mask, **PLANS[plan][1])


def _with_mask(pp, ne=None, nb=None):
    """pp's params with the mask's ne[2..3] / nb[2..3] overridden."""
    prm = pp.params()
    for i, x in (ne or {}).items():
        prm.mask.ne[i] = x
    for i, x in (nb or {}).items():
        prm.mask.nb[i] = x
    return prm


def _code(prm):
    with pytest.raises(fattn.FattnError) as e:
        fattn.describe(prm)
    return e.value.code


@pytest.mark.parametrize("plan", list(PLANS))
def test_plane_counts_must_divide(plan):
    """ne[2] must divide H and ne[3] must divide S: FATTN_ERR_INVALID_ARG, and no workspace."""
    p = _problem(plan, S=4)
    pp = mp.add_planes(p, 2, 2)
    with fattn.options(PLANS[plan][0]):
        fattn.describe(pp.params())                       # (2, 2) divide (H, 4): planned
        for ne in ({2: 3}, {3: 3}, {2: p.H + 1}, {3: 8}, {2: 2 * p.H}):
            prm = _with_mask(pp, ne=ne)
            assert _code(prm) == ERR_INVALID_ARG, ne
            assert fattn.workspace_size(prm) == 0


@pytest.mark.parametrize("plan", list(PLANS))
def test_plane_strides_are_dword_multiples(plan):
    """nb[2] or nb[3] % 4 != 0: FATTN_ERR_ALIGNMENT -- but only where the count
    exceeds 1 (a single plane has no stride: fattn_row passes N * 2 there)."""
    p = _problem(plan)
    pp = mp.add_planes(p, 2, 2)
    with fattn.options(PLANS[plan][0]):
        for i in (2, 3):
            assert _code(_with_mask(pp, nb={i: pp.mask.nb[i] + 2})) == ERR_ALIGNMENT
            assert _code(_with_mask(pp, nb={i: pp.mask.nb[i] + 1})) == ERR_ALIGNMENT
        one = mp.add_planes(p, 1, 1)
        canon = fattn.describe(one.params())
        assert fattn.describe(_with_mask(one, nb={2: 6, 3: 2})) == canon


@pytest.mark.parametrize("plan", list(PLANS))
def test_zero_counts_read_as_one(plan):
    """ne[2..3] = 0 (a zeroed struct) or negative plans exactly as 1."""
    p = _problem(plan)
    one = mp.add_planes(p, 1, 1)
    with fattn.options(PLANS[plan][0]):
        canon = fattn.describe(one.params())
        ws = fattn.workspace_size(one.params())
        for ne in ({2: 0, 3: 0}, {2: 0}, {3: 0}, {2: -1, 3: -5}):
            prm = _with_mask(one, ne=ne, nb={2: 0, 3: 0})
            assert fattn.describe(prm) == canon, ne
            assert fattn.workspace_size(prm) == ws


@pytest.mark.parametrize("plan", list(PLANS))
def test_one_plane_is_todays_call(plan):
    """With one plane the describe string (no suffix) and the workspace size
    are those of the 2-D mask of the same shape, whatever nb[2..3] hold."""
    p2 = _problem(plan, mask="random")
    one = mp.add_planes(_problem(plan), 1, 1)
    with fattn.options(PLANS[plan][0]):
        # today's call: the contiguous 2-D mask through mask_view's ne / nb
        v2 = views.make_view(p2)
        d2, ws2 = fattn.describe(v2.params()), fattn.workspace_size(v2.params())
        assert "mask planes" not in d2
        d1, ws1 = fattn.describe(one.params()), fattn.workspace_size(one.params())
        assert (d1, ws1) == (d2, ws2)
        assert fattn.describe(mp.broadcast_of(mp.add_planes(_problem(plan), 2, 2)).params()) == d2


@pytest.mark.parametrize("plan", list(PLANS))
def test_replicated_strides_are_accepted(plan):
    """nb[2] = nb[3] = 0: one stored plane read by every (head, sequence); the
    plan is the one-plane plan but for the suffix."""
    p = _problem(plan)
    one = mp.add_planes(p, 1, 1)
    rep = mp.add_planes(p, 2, 2, repeat=True)
    assert rep.mask.nb[2] == 0 and rep.mask.nb[3] == 0 and rep.mask.ne[2:] == (2, 2)
    with fattn.options(PLANS[plan][0]):
        d = fattn.describe(rep.params())
        assert d.endswith(" mask planes (2,2)"), d
        if plan == "mq":
            assert "fattn_mq_kernel" not in d, d          # (head planes: the planner leaves mq)
        d3 = fattn.describe(mp.add_planes(p, 1, 2, repeat=True).params())
        assert d3 == fattn.describe(one.params()) + " mask planes (1,2)"


@pytest.mark.parametrize("plan", list(PLANS))
def test_describe_suffix(plan):
    p = _problem(plan, S=4)
    with fattn.options(PLANS[plan][0]):
        for ne2, ne3 in ((1, 2), (2, 1), (2, 4), (p.H, 1)):
            d = fattn.describe(mp.add_planes(p, ne2, ne3).params())
            assert d.endswith(f" mask planes ({ne2},{ne3})"), d
        assert "mask planes" not in fattn.describe(mp.add_planes(p, 1, 1).params())


def test_mq_is_left_with_head_planes():
    """The multi-query kernel shares a mask row among a query row's heads: it
    takes sequence planes and is never planned with head planes."""
    opts, shape = PLANS["mq"]
    p = _problem("mq")
    with fattn.options(opts):
        assert "fattn_mq_kernel" in fattn.describe(mp.add_planes(p, 1, 1).params())
        assert "fattn_mq_kernel" in fattn.describe(mp.add_planes(p, 1, 2).params())
        for ne2 in (2, 4, 16):
            d = fattn.describe(mp.add_planes(p, ne2, 1).params())
            assert "fattn_mq_kernel" not in d and "fattn_split_kernel" in d, d
    with fattn.options({fattn.OPT_MQ_MIN_ROWS: 32}):      # (batched decode allowed: it takes head planes)
        big = make_problem(D=128, NQ=64, H=16, Hkv=4, N=4096, S=8, kv_type="q8_0", seed=1, mask="none")
        d = fattn.describe(mp.add_planes(big, 4, 1).params())
        assert "fattn_mq_kernel" not in d, d


@pytest.mark.parametrize("form", [1, 0], ids=["pf", "pf4"])
def test_pf_flag_tables_per_plane(form):
    """Masked prefill: one live-block flag table per sequence plane at the front
    of the workspace -- larger by the added tables (rounded to 256 B) and no more."""
    opts, shape = PLANS["pf"]
    p = _problem("pf")
    n_qt = (shape["NQ"] * (shape["H"] // shape["Hkv"]) + 255) // 256
    table = n_qt * (shape["N"] // 64)
    r256 = lambda x: (x + 255) // 256 * 256
    with fattn.options({**opts, fattn.OPT_PF_FORM: form}):
        one, two = mp.add_planes(p, 1, 1), mp.add_planes(p, 1, 2)
        d1, d2 = fattn.describe(one.params()), fattn.describe(two.params())
        assert "pf_mask_flags" in d1 and ("fattn_pf4_kernel" in d1) == (form == 0), d1
        assert d2.endswith(" mask planes (1,2)"), d2
        ws1, ws2 = fattn.workspace_size(one.params()), fattn.workspace_size(two.params())
        assert ws2 - ws1 == r256(2 * table) - r256(table)
        assert d2.split(" ws ")[0] == d1.split(" ws ")[0]
        # head planes: H / Hkv = 1 here, so each kv head's tiles read one plane -- a table per plane
        hp = mp.add_planes(p, 2, 2)
        assert fattn.workspace_size(hp.params()) - ws1 == r256(4 * table) - r256(table)
    # (a long prompt, where the rounding does not hide the size: 4 planes, 4 tables)
    big = make_problem(D=128, NQ=2048, H=8, Hkv=8, N=2048, S=4, kv_type="f16", seed=1, mask="none")
    with fattn.options({fattn.OPT_PF_FORM: form}):
        w1 = fattn.workspace_size(mp.add_planes(big, 1, 1).params())
        w4 = fattn.workspace_size(mp.add_planes(big, 1, 4).params())
        assert "fattn_pf" in fattn.describe(mp.add_planes(big, 1, 4).params())
        assert w1 == r256(8 * 32) and w4 == r256(4 * 8 * 32)


@pytest.mark.parametrize("plan", list(PLANS))
def test_plane_stride_off_16_takes_the_dword_path(plan):
    """nb[3] % 16 == 4 (or nb[2]): the planes' bases are only dword aligned, so
    the 16-B path is off as for nb[1] % 16 -- the split kernel at gran = 4."""
    p = _problem(plan)
    with fattn.options(PLANS[plan][0]):
        for ne2, ne3 in ((1, 2), (2, 1)):
            pp = mp.add_planes(p, ne2, ne3, offset4=True)
            assert pp.mask.nb[2 if ne2 > 1 else 3] % 16 == 4
            d = fattn.describe(pp.params())
            assert d.startswith("fattn_split_kernel<") and ",gran4," in d, d


def test_mask_view_4d():
    import torch
    m = torch.zeros((3, 2, 5, 64), dtype=torch.float16)
    v = fattn.mask_view(m)
    assert tuple(v.ne) == (64, 5, 2, 3) and tuple(v.nb) == (2, 128, 5 * 128, 2 * 5 * 128)
    assert v.ptr == m.data_ptr() and v.type == fattn.TYPE_F16
    v2 = fattn.mask_view(m[0, 0])                          # 2-D: unchanged
    assert tuple(v2.ne) == (64, 5, 1, 1) and tuple(v2.nb) == (2, 128, 640, 640)
    with pytest.raises(ValueError):
        fattn.mask_view(m.transpose(0, 1))


def test_builder_layout_and_poison():
    p = make_problem(D=64, NQ=5, H=4, Hkv=2, N=200, S=2, kv_type="q8_0", seed=2, mask="none")
    plane = 5 * 512
    for order, nb in (("sh", (plane + 256, 4 * (plane + 256))), ("hs", (2 * (plane + 256), plane + 256))):
        pp = mp.add_planes(p, 4, 2, order=order)
        assert pp.mask.ne == (256, 5, 4, 2) and pp.mask.nb == (2, 512) + nb
        mb = pp.mask.data.view(np.uint16)
        assert (mb == views.F16_NAN).sum() == mb.size - 8 * 5 * 200      # pad columns, gaps, guard
    assert mp.add_planes(p, 4, 2, offset4=True).mask.nb[2] == plane + 260
    assert mp.plane_lengths(200, 4, "full") == [200, 45, 103, 200]
    assert mp.plane_lengths(200, 4, "short") == [45, 103, 200, 45]
    pl = mp.default_planes(p, 2, 2, "short")
    assert np.isneginf(pl[0, 0, :, 45:]).all() and np.isfinite(pl[0, 0, :, :45]).all() and np.isfinite(pl[1, 0]).all()


@pytest.mark.parametrize("order", ["sh", "hs"])
def test_assembled_oracle_equals_broadcast_when_planes_are_copies(order):
    """The expected value of the GPU tests: per-(sequence, head) oracle calls,
    assembled.  With every plane a copy of one plane it must equal the one
    broadcasting oracle call bit for bit -- stored copies and nb = 0 alike."""
    p = make_problem(D=64, NQ=5, H=4, Hkv=2, N=200, S=4, Skv=2, kv_type="q8_0", seed=2, mask="none")
    one = mp.default_planes(p, 1, 1, "short")
    copies = np.broadcast_to(one, (2, 4) + one.shape[2:]).copy()
    ref = mp.broadcast_of(mp.add_planes(p, 1, 1, planes=one)).oracle()
    assert not np.isnan(ref).any()
    for pp in (mp.add_planes(p, 4, 2, order=order, planes=copies), mp.add_planes(p, 4, 2, repeat=True, planes=copies)):
        assert np.array_equal(pp.oracle().view(np.uint32), ref.view(np.uint32))
    # and differs as soon as one plane does
    copies[1, 3] = mp.default_planes(p, 1, 1, "full", seed=9)[0, 0]
    got = mp.add_planes(p, 4, 2, order=order, planes=copies).oracle()
    assert np.array_equal(got[[0, 2]], ref[[0, 2]]) and np.array_equal(got[:, :, :3], ref[:, :, :3])
    assert not np.array_equal(got[1, :, 3], ref[1, :, 3]) and not np.array_equal(got[3, :, 3], ref[3, :, 3])
