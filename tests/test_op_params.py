"""ggml's max_bias (ALiBi) and logit_softcap (fattn_params, include/fattn.h) on
the CPU: the assembled reference of tests/op_params.py pinned to the frozen
oracle, the ABI, what make_plan rejects and how the planner routes (host-only
planning, as in test_views.py), the shard helper and the kernel_test harness."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fattn
import mask_planes as mp
import op_params as op
import views
from fattn import shard
from gpu_util import run_kernel_test
from oracle import oracle as orc
from plans import plan_params as _params
from problems import attn_rel_err, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference

def test_slope_table():
    """ggml's slopes at max_bias = 8: H = 8 all powers of two; H = 6 (n2 = 4)
    1/4 .. 1/256 then 1/2, 1/8 from the second branch; H = 12 (n2 = 8) the
    second branch's odd powers of 2^-1/2."""
    assert np.array_equal(op.slopes(8.0, 8), np.float32(2.0) ** -np.arange(1, 9, dtype=np.float32))
    assert np.array_equal(op.slopes(8.0, 6), np.array([1 / 4, 1 / 16, 1 / 64, 1 / 256, 1 / 2, 1 / 8], dtype=np.float32))
    want12 = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625,
              0.70710678, 0.35355339, 0.17677670, 0.08838835]
    assert np.allclose(op.slopes(8.0, 12), want12, rtol=1e-6, atol=0)
    assert np.array_equal(op.slopes(0.0, 5), np.ones(5, dtype=np.float32))


@pytest.mark.parametrize("kt", ["q8_0", "f16"])
def test_reference_off_is_the_frozen_oracle(kt):
    """Both parameters off: the assembled reference is bit-equal to Problem.oracle()."""
    for mask in ("random", "none"):
        p = make_problem(D=128, NQ=3, H=4, Hkv=2, N=200, kv_type=kt, seed=11, mask=mask)
        vp = views.make_view(p)
        ref = op.with_params(vp).reference()
        assert np.array_equal(_bits(ref), _bits(p.oracle())), (kt, mask)


@pytest.mark.parametrize("kt", ["q8_0", "f16"])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (6, 2)])
def test_reference_alibi_is_the_frozen_oracle_over_premultiplied_planes(kt, H, Hkv):
    """max_bias = 8 at H = 8 and at H = 6 / Hkv = 2: every slope is a power of
    two and the mask is minus an integer distance, so slope * mask is exact in
    f16 -- the frozen oracle over H pre-multiplied head planes is bit-equal."""
    p = make_problem(D=128, NQ=3, H=H, Hkv=Hkv, N=200, kv_type=kt, seed=12, mask="none")
    dist = op.distance_mask(p.NQ, p.N)
    ref = op.one_plane(p, dist, max_bias=8.0).reference()
    long_way = op.premultiplied_planes(p, dist, 8.0).oracle()
    assert not np.isnan(ref).any()
    assert np.array_equal(_bits(ref), _bits(long_way))
    # and the feature moves the output far more than the suite's bound
    assert attn_rel_err(ref, op.one_plane(p, dist).reference()) >= 5e-2


def test_reference_softcap_moves_the_output():
    p = make_problem(D=128, NQ=3, H=4, Hkv=2, N=200, kv_type="q8_0", seed=13, mask="none", scale=1.0)
    m = op.random_mask(p.NQ, p.N)
    assert attn_rel_err(op.one_plane(p, m, logit_softcap=4.0).reference(), op.one_plane(p, m).reference()) >= 5e-2


# ------------------------------------------------------------------ ABI

SHAPES = {"config3": dict(), "config5": dict(NQ=64), "prefill": dict(NQ=4096)}


def test_fields_sit_at_the_end_of_the_struct():
    names = [f[0] for f in fattn.FattnParams._fields_]
    assert names[-4:] == ["max_bias", "logit_softcap", "n_head_total", "head_first"]
    assert names[-5] == "workspace_bytes"
    P = fattn.FattnParams
    assert P.max_bias.offset == P.workspace_bytes.offset + C.sizeof(C.c_size_t)
    assert C.sizeof(P) == P.max_bias.offset + 16
    with open(os.path.join(ROOT, "include", "fattn.h")) as f:
        hdr = f.read()
    body = hdr[hdr.index("typedef struct fattn_params"):hdr.index("} fattn_params;")]
    order = [body.index(x) for x in ("size_t workspace_bytes;", "float max_bias;", "float logit_softcap;",
                                     "int32_t n_head_total;", "int32_t head_first;")]
    assert order == sorted(order)
    assert fattn.lib().fattn_version().startswith(b"fattn-gfx950")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_zeroed_fields_plan_as_before(shape):
    """Explicit zeros are the call without the keywords: same describe, same workspace."""
    a = _params(**SHAPES[shape])
    b = _params(**SHAPES[shape], max_bias=0.0, logit_softcap=0.0, n_head_total=0, head_first=0)
    d = fattn.describe(a)
    assert fattn.describe(b) == d
    assert "softcap" not in d and "alibi" not in d
    assert fattn.workspace_size(a) == fattn.workspace_size(b)


BAD = [dict(max_bias=-1.0), dict(max_bias=float("nan")), dict(max_bias=float("inf")),
       dict(logit_softcap=-0.5), dict(logit_softcap=float("nan")), dict(logit_softcap=float("inf")),
       dict(head_first=-1), dict(head_first=1), dict(n_head_total=31), dict(n_head_total=40, head_first=9),
       dict(n_head_total=-32)]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_invalid_values_are_rejected(shape, kw):
    """Negative, NaN or infinite scalars, a negative head_first and head_first + H
    past n_head_total: FATTN_ERR_INVALID_ARG from fattn_ext (which returns before
    anything is launched -- the pointers here are fake) and no workspace."""
    p = _params(**SHAPES[shape], **kw)
    assert fattn.lib().fattn_ext(C.byref(p), None) == ERR_INVALID_ARG
    assert fattn.workspace_size(p) == 0
    with pytest.raises(fattn.FattnError) as e:
        fattn.describe(p)
    assert e.value.code == ERR_INVALID_ARG


def test_head_window_inside_the_total_is_accepted():
    fattn.describe(_params(n_head_total=40, head_first=8, max_bias=8.0))
    fattn.describe(_params(n_head_total=32, head_first=0))


# ------------------------------------------------------------------ planner

def test_suffixes_appear_only_when_live():
    base = fattn.describe(_params())
    assert fattn.describe(_params(logit_softcap=4.0)).endswith(" softcap 4")
    assert fattn.describe(_params(max_bias=8.0)).endswith(" alibi 8")
    assert fattn.describe(_params(max_bias=8.0, logit_softcap=0.5)).endswith(" softcap 0.5 alibi 8")
    # max_bias with no mask has no effect: the plan of max_bias = 0
    nm = fattn.describe(_params(mask=False))
    assert fattn.describe(_params(mask=False, max_bias=8.0)) == nm
    assert fattn.workspace_size(_params(mask=False, max_bias=8.0)) == fattn.workspace_size(_params(mask=False))
    assert fattn.describe(_params(mask=False, logit_softcap=4.0)).endswith(" softcap 4")
    assert "softcap" not in base and "alibi" not in base


@pytest.mark.parametrize("kw", [dict(logit_softcap=4.0), dict(max_bias=8.0)], ids=["softcap", "alibi"])
def test_prefill_leaves_pf4_when_live(kw):
    """The D = 128 f16 prefill shape: fattn_pf4_kernel(lean) with both off,
    fattn_pf_kernel<f16,D128 (which has the score transform) with either live;
    a staged Q8_0 prefill still stages."""
    f16 = dict(NQ=4096, kt=fattn.TYPE_F16)
    assert "fattn_pf4_kernel(lean)<f16,D128" in fattn.describe(_params(**f16))
    d = fattn.describe(_params(**f16, **kw))
    assert "fattn_pf_kernel<f16,D128" in d and "pf4" not in d, d
    q8 = fattn.describe(_params(NQ=4096))
    assert "kv_stage_f16<q8_0>" in q8 and "fattn_pf4_kernel(lean)<f16,D128" in q8
    d = fattn.describe(_params(NQ=4096, **kw))
    assert "kv_stage_f16<q8_0>" in d and "fattn_pf_kernel<f16,D128" in d and "pf4" not in d, d
    # the staged rows and the flag table are unchanged
    assert fattn.workspace_size(_params(NQ=4096, **kw)) == fattn.workspace_size(_params(NQ=4096))


def test_mq_keeps_gqa_tiles_under_max_bias():
    """The multi-query kernel applies the slope per lane (the q head of the
    lane's own packed row), so unlike head planes max_bias does not make the
    planner leave it -- with GQA (rk2 = 4) or without."""
    opts = {fattn.OPT_MQ_MIN_ROWS: 32, fattn.OPT_BD: 1}
    for shape in (dict(NQ=40, H=16, Hkv=4, N=320), dict(NQ=40, H=4, Hkv=4, N=320), dict(D=256, NQ=50, H=2, Hkv=2, N=320)):
        with fattn.options(opts):
            d0 = fattn.describe(_params(**shape))
            d1 = fattn.describe(_params(**shape, max_bias=8.0, logit_softcap=4.0))
        assert d0.startswith("fattn_mq_kernel<"), d0
        assert d1 == d0 + " softcap 4 alibi 8", (d0, d1)


def test_split_kernel_takes_four_waves_when_live():
    """The split kernel's bodies with the transform exist for 4 waves: config 3
    plans 8 waves with both off and 4 with either live; nothing is refused."""
    assert "8waves" in fattn.describe(_params())
    for kw in (dict(logit_softcap=4.0), dict(max_bias=8.0)):
        d = fattn.describe(_params(**kw))
        assert d.startswith("fattn_split_kernel<") and ",4waves>" in d, d
        with fattn.options({fattn.OPT_SPLIT_WAVES: 8}):
            assert ",4waves>" in fattn.describe(_params(**kw))


@pytest.mark.parametrize("D,kt", [(64, fattn.TYPE_Q4_0), (80, fattn.TYPE_F16), (96, fattn.TYPE_Q8_0), (128, fattn.TYPE_F16),
                                  (256, fattn.TYPE_Q8_0)])
@pytest.mark.parametrize("NQ", [1, 64, 4096])
def test_every_accepted_shape_is_accepted_with_the_parameters(D, kt, NQ):
    """The planner may re-route, it may not refuse."""
    fattn.describe(_params(D=D, kt=kt, NQ=NQ))
    fattn.describe(_params(D=D, kt=kt, NQ=NQ, max_bias=8.0, logit_softcap=30.0))
    fattn.describe(_params(D=D, kt=kt, NQ=NQ, mask=False, logit_softcap=30.0))


# ------------------------------------------------------------------ sharding

def test_shard_gives_the_global_slope_arguments():
    """A rank's slice must be launched with its first q head's GLOBAL index and
    the unsharded H.  Asserted on the CPU reference: the slices assembled with
    shard.slope_args() are the unsharded reference bit for bit; launched as
    stand-alone problems (head_first = 0, n_head_total = slice) they miss the
    suite's bound by orders of magnitude."""
    H, Hkv = 8, 4
    p = make_problem(D=64, NQ=2, H=H, Hkv=Hkv, N=96, kv_type="f16", seed=14, mask="none")
    dist = op.distance_mask(p.NQ, p.N)
    full = op.one_plane(p, dist, max_bias=8.0).reference()
    for world in (2, 4):
        good, bad = [], []
        for rank in range(world):
            sh = shard.shard_heads(H, Hkv, world, rank)
            assert sh.slope_args() == {"n_head_total": H, "head_first": sh.h0}
            sub = make_problem(D=64, NQ=2, H=sh.n_heads, Hkv=sh.n_kv, N=96, kv_type="f16", seed=14, mask="none")
            sub.q = np.ascontiguousarray(p.q[:, :, sh.h0:sh.h1])
            sub.k_bytes = np.ascontiguousarray(p.k_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
            sub.v_bytes = np.ascontiguousarray(p.v_bytes.reshape(1, Hkv, -1)[:, sh.kv0:sh.kv1]).reshape(-1)
            good.append(op.one_plane(sub, dist, max_bias=8.0, **sh.slope_args()).reference())
            bad.append(op.one_plane(sub, dist, max_bias=8.0).reference())
        assert np.array_equal(_bits(np.concatenate(good, axis=2)), _bits(full)), world
        assert attn_rel_err(np.concatenate(bad, axis=2), full) > 5e-2, world
    with pytest.raises(ValueError):
        shard.HeadShard(0, 2, 0, 2, 0, 4).slope_args()


# ------------------------------------------------------------------ harness

def test_harness_cpu_reference_has_the_parameters(tmp_path):
    """kernel_test --cpu-only --max-bias 8 --softcap 4 against the same
    formulas from the oracle's primitives over the harness's own inputs (the
    rand() stream in the order Q, K, V, mask; its mask stays f32).  The harness
    evaluates tanhf / expf in f32 with a single-pass softmax, the oracle's
    primitives a float64 tanh and a two-pass softmax: f32 rounding of logits of
    magnitude <= cap + |mask| (6e-7) through a softmax over 96 keys -- 1e-5 of
    a row's largest output is two orders above that and four below the
    feature's effect."""
    H, Hkv, D, N, NQ = 6, 2, 64, 96, 2
    base = ["--cpu-only", "--heads", str(H), "--kv-heads", str(Hkv), "--head-dim", str(D), "--kv-size", str(N),
            "--n-q", str(NQ)]
    outs = {}
    for tag, extra in (("on", ["--max-bias", "8", "--softcap", "4"]), ("off", [])):
        f = tmp_path / f"{tag}.bin"
        r = run_kernel_test(base + extra + ["--dump", f])
        assert r.returncode == 0, r.stderr
        outs[tag] = np.fromfile(f, dtype=np.float32).reshape(1, NQ, H, D)
    orc.srand(1)
    q = orc.random(D * H * NQ).reshape(NQ, H, D)
    k = orc.random(D * N * Hkv).reshape(Hkv, N, D)
    v = orc.random(D * N * Hkv).reshape(Hkv, N, D)
    m = orc.random(N * NQ).reshape(NQ, N)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    sl = op.slopes(8.0, H)
    want = {"on": np.empty((1, NQ, H, D), np.float32), "off": np.empty((1, NQ, H, D), np.float32)}
    for h in range(H):
        kk, vv = k[h // (H // Hkv)], v[h // (H // Hkv)]
        qh = np.ascontiguousarray(q[:, h])
        sc = orc.mulmat_f32(qh, kk, None, NQ, N, D, float(scale / np.float32(4.0)), 1).reshape(NQ, N)
        sc = (4.0 * np.tanh(sc.astype(np.float64))).astype(np.float32) + (sl[h] * m).astype(np.float32)
        want["on"][0, :, h] = orc.mulmat_f32(orc.softmax(sc, N, NQ), vv, None, NQ, D, N, 1.0, 0).reshape(NQ, D)
        sc = orc.mulmat_f32(qh, kk, None, NQ, N, D, float(scale), 1).reshape(NQ, N) + m   # (its mask argument is one row)
        want["off"][0, :, h] = orc.mulmat_f32(orc.softmax(sc, N, NQ), vv, None, NQ, D, N, 1.0, 0).reshape(NQ, D)
    assert attn_rel_err(outs["off"], want["off"]) <= 1e-5
    assert attn_rel_err(outs["on"], want["on"]) <= 1e-5
    assert attn_rel_err(want["on"], want["off"]) >= 5e-2
