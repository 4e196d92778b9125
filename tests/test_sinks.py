"""Attention sinks (ggml FLASH_ATTN_EXT src[4], fattn_ext_sinks) on the CPU: the
factor-form reference of tests/sinks.py pinned to the frozen oracle's own
softmax, the ABI (host-only planning with fake pointers: every check below
returns before anything would launch), and the shard helper."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fattn
import op_params as op
import sinks as sk
import views
from fattn import shard
from gpu_util import run_kernel_test
from oracle import oracle as orc
from plans import plan_params as _params
from problems import attn_rel_err, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_ALIGNMENT = -1, -7


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference

@pytest.mark.parametrize("NQ,N,spread,sink", [(5, 256, 4.0, 5.0), (3, 200, 1.0, -1.0), (4, 1500, 8.0, 9.0), (2, 64, 0.5, 20.0)])
def test_factor_form_is_the_oracles_softmax_with_one_more_column(NQ, N, spread, sink):
    """orc.softmax over N + 1 columns (the sink last), last column dropped, against
    orc.softmax over the N columns times g = 1 / (1 + exp(s - lse)): within
    N * 2^-23 of the largest entry, the worst-case rounding of an N-term f32 sum."""
    rng = np.random.default_rng(100 + N)
    sc = (spread * rng.standard_normal((NQ, N))).astype(np.float32)
    ext = np.concatenate([sc, np.full((NQ, 1), sink, dtype=np.float32)], axis=1)
    long_way = orc.softmax(np.ascontiguousarray(ext), N + 1, NQ).reshape(NQ, N + 1)[:, :N]
    g = sk.factor(sk.lse_rows(sc), sink)
    short = orc.softmax(np.ascontiguousarray(sc), N, NQ).reshape(NQ, N) * g[:, None]
    bound = N * 2.0 ** -23 * float(long_way.max())
    err = float(np.abs(short.astype(np.float64) - long_way.astype(np.float64)).max())
    print(f"SINKS factor form N={N} sink={sink}: err {err:.3e} = {err / bound:.3f} of the bound")
    assert long_way.max() > 0 and err <= bound, (err, bound)


def _problem(mask):
    p = make_problem(D=128, NQ=3, H=4, Hkv=2, N=200, kv_type="q8_0", seed=21, mask="none")
    return op.one_plane(p, mask(p.NQ, p.N) if mask else None)


@pytest.mark.parametrize("mask", [None, op.random_mask, op.distance_mask])
def test_sinks_of_minus_inf_are_the_plain_reference(mask):
    o = _problem(mask)
    ref = sk.with_sinks(o, np.full(4, -np.inf, dtype=np.float32)).reference()
    assert np.array_equal(_bits(ref), _bits(o.reference()))


def test_reference_moves_with_the_sinks_and_masked_rows_are_zero():
    o = _problem(op.random_mask)
    plain = o.reference()
    s = (np.log(200.0) + np.array([0.0, 1.0, -1.0, 2.0])).astype(np.float32)
    ref = sk.with_sinks(o, s).reference()
    lse = {(h): sk.lse_rows(sc) for _, h, sc in sk.scores(o)}
    for h in range(4):
        g = 1.0 / (1.0 + np.exp(float(s[h]) - lse[h]))
        assert np.allclose(ref[0, :, h], plain[0, :, h] * g[:, None], rtol=1e-6, atol=0)
    # a plane whose query row 0 is -inf everywhere: NaN without sinks, zeros with
    m = op.random_mask(3, 200)
    m[0] = -np.inf
    o = op.one_plane(make_problem(D=128, NQ=3, H=4, Hkv=2, N=200, kv_type="q8_0", seed=21, mask="none"), m)
    assert np.isnan(o.reference()[0, 0]).all()
    ref = sk.with_sinks(o, s).reference()
    assert (ref[0, 0] == 0.0).all() and not np.isnan(ref).any() and (ref[0, 1:] != 0.0).any()


# ------------------------------------------------------------------ ABI

def _header():
    with open(os.path.join(ROOT, "include", "fattn.h")) as f:
        return f.read()


def test_entry_point_is_exported_and_declared():
    assert "fattn_ext_sinks" in fattn.EXPORTS
    assert fattn.lib().fattn_ext_sinks is not None
    hdr = re.sub(r"\s+", " ", _header())
    assert "int fattn_ext_sinks(const fattn_params* p, const float* sinks, void* stream);" in hdr
    # the signatures that must not change
    assert "int fattn_ext(const fattn_params* p, void* stream);" in hdr
    assert "size_t fattn_workspace_size(const fattn_params* p);" in hdr
    dbg = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "fattn_debug.h")).read())
    assert "int fattn_describe(const fattn_params* p, char* out, size_t cap);" in dbg
    assert "fattn_ext_events(const fattn_params* p, void* stream, void* ev_begin, void* ev_end);" in dbg


def test_params_struct_did_not_grow():
    P = fattn.FattnParams
    assert [f[0] for f in P._fields_][-1] == "head_first" and C.sizeof(P) == P.max_bias.offset + 16
    assert not any("sink" in f[0] for f in P._fields_)


SHAPES = {"config3": dict(), "config5": dict(NQ=64), "prefill": dict(NQ=4096), "nomask": dict(mask=False)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_misaligned_sinks_pointer_is_an_alignment_error(shape):
    """Checked before the workspace and before anything launches: the params
    carry no workspace, and an aligned pointer gets past the check to
    FATTN_ERR_WORKSPACE where the plan needs one."""
    p = _params(**SHAPES[shape])
    L = fattn.lib()
    for off in (1, 2, 3, 5, 6, 7):
        assert L.fattn_ext_sinks(C.byref(p), (1 << 21) + off, None) == ERR_ALIGNMENT, off
    if fattn.workspace_size(p):
        assert L.fattn_ext_sinks(C.byref(p), 1 << 21, None) == -5


BAD = [dict(D=72), dict(H=6, Hkv=4), dict(max_bias=-1.0), dict(logit_softcap=float("nan")), dict(ptr=(1 << 20) + 4),
       dict(n_head_total=16, head_first=0)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_invalid_params_return_what_fattn_ext_returns(bad):
    p = _params(**bad)
    L = fattn.lib()
    want = L.fattn_ext(C.byref(p), None)
    assert want != 0
    for sinks in (None, 1 << 21, (1 << 21) + 2):
        assert L.fattn_ext_sinks(C.byref(p), sinks, None) == want, sinks


def test_plan_and_workspace_are_functions_of_the_params_alone():
    """describe and workspace_size take no sinks argument -- and the header says
    that the sinks launch runs that very plan."""
    hdr = re.sub(r"[\s\*]+", " ", _header())
    assert "Sinks never change the plan, the grid, the workspace size or the describe string" in hdr
    assert "fattn_describe(p) is also the plan of the sinks launch" in hdr
    assert fattn.lib().fattn_describe.argtypes[0]._type_ is fattn.FattnParams and len(fattn.lib().fattn_describe.argtypes) == 3
    assert len(fattn.lib().fattn_workspace_size.argtypes) == 1
    for shape in SHAPES.values():
        p = _params(**shape)
        d, ws = fattn.describe(p), fattn.workspace_size(p)
        fattn.lib().fattn_ext_sinks(C.byref(p), (1 << 21) + 2, None)     # (returns before it would launch)
        assert fattn.describe(p) == d and fattn.workspace_size(p) == ws and "sink" not in d


def test_python_mirror_rejects_events_with_sinks():
    p = _params()
    with pytest.raises(ValueError):
        fattn.flash_attn_ext(p, stream=0, ev_begin=1, ev_end=2, sinks=1 << 21)
    with pytest.raises(ValueError):
        fattn.flash_attn_ext(p, stream=0, ev_end=2, sinks=1 << 21)
    with pytest.raises(fattn.FattnError) as e:                          # a pointer goes straight to the C ABI
        fattn.flash_attn_ext(p, stream=0, sinks=(1 << 21) + 2)
    assert e.value.code == ERR_ALIGNMENT


def test_python_mirror_checks_a_sinks_tensor():
    """A torch tensor is checked before its pointer is taken: dtype, contiguity,
    device and the head count (all raise before the library is called)."""
    import torch
    p = _params(H=32)
    for bad in (torch.zeros(32, dtype=torch.float64), torch.zeros(64)[::2], torch.zeros(32), torch.zeros(31)):
        with pytest.raises(ValueError):
            fattn.flash_attn_ext(p, stream=0, sinks=bad)


def test_retarget_can_switch_sinks_off():
    att = fattn.Attention.__new__(fattn.Attention)
    att.p, att.sinks = _params(), 1 << 21
    att.retarget(sinks=None)
    assert att.sinks == 1 << 21
    att.retarget(sinks=1 << 22)
    assert att.sinks == 1 << 22
    att.retarget(sinks=fattn.NO_SINKS)
    assert att.sinks is None


@pytest.mark.parametrize("kw", [dict(), dict(max_bias=8.0), dict(logit_softcap=4.0), dict(max_bias=8.0, logit_softcap=0.5)])
def test_scores_are_the_plain_references_scores(kw):
    """tests/sinks.py scores() restates steps 1 to 3 of op_params.reference: its
    steps 4 and 5 over those scores rebuild that reference bit for bit, so the
    log-sum-exp is taken from the very scores the plain reference used."""
    for mask in (None, op.random_mask, op.distance_mask):
        p = make_problem(D=128, NQ=3, H=6, Hkv=2, N=200, kv_type="q8_0", seed=22, mask="none", scale=1.0 if kw else None)
        o = op.one_plane(p, mask(p.NQ, p.N) if mask else None, **kw)
        V = op._decode(o.v)
        out = np.empty((1, p.NQ, p.H, p.D), dtype=np.float32)
        for s, h, sc in sk.scores(o):
            out[s, :, h, :] = orc.mulmat_f32(orc.softmax(sc, p.N, p.NQ), V[s, h // 3], None, p.NQ, p.D, p.N, 1.0, 0).reshape(p.NQ, p.D)
        assert np.array_equal(_bits(out), _bits(o.reference())), (kw, mask)


# ------------------------------------------------------------------ shards

@pytest.mark.parametrize("world", [2, 4, 8])
def test_sink_slice(world):
    H, Hkv = 32, 8
    s = np.arange(H, dtype=np.float32) * 0.5 - 3.0
    got = []
    for rank in range(world):
        sh = shard.shard_heads(H, Hkv, world, rank)
        part = sh.sink_slice(s)
        assert part.shape == (sh.n_heads,) and np.array_equal(part, s[sh.h0:sh.h1])
        assert np.shares_memory(part, s)
        got.append(part)
        with pytest.raises(ValueError):
            sh.sink_slice(s[:H - 1])
    assert np.array_equal(np.concatenate(got), s)


# ------------------------------------------------------------------ harness

def test_harness_cpu_reference_has_the_sinks(tmp_path):
    """kernel_test --cpu-only --sinks 3 against the factor form over the
    harness's own inputs (the rand() stream in the order Q, K, V, mask; its mask
    stays f32): head h gets 3 + 0.25 (h % 8).  f32 expf against a float64
    log-sum-exp over 96 keys: 1e-5 of a row's largest output, as for the
    harness's other parameters (tests/test_op_params.py)."""
    H, Hkv, D, N, NQ = 10, 2, 64, 96, 2
    base = ["--cpu-only", "--heads", str(H), "--kv-heads", str(Hkv), "--head-dim", str(D), "--kv-size", str(N),
            "--n-q", str(NQ)]
    outs = {}
    for tag, extra in (("on", ["--sinks", "3"]), ("off", [])):
        f = tmp_path / f"{tag}.bin"
        r = run_kernel_test(base + extra + ["--dump", f])
        assert r.returncode == 0, r.stderr
        outs[tag] = np.fromfile(f, dtype=np.float32).reshape(1, NQ, H, D)
    orc.srand(1)
    q = orc.random(D * H * NQ).reshape(NQ, H, D)
    k = orc.random(D * N * Hkv).reshape(Hkv, N, D)
    orc.random(D * N * Hkv)
    m = orc.random(N * NQ).reshape(NQ, N)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    want = outs["off"].copy()
    for h in range(H):
        sc = orc.mulmat_f32(np.ascontiguousarray(q[:, h]), k[h // (H // Hkv)], None, NQ, N, D, float(scale), 1).reshape(NQ, N) + m
        want[0, :, h] *= sk.factor(sk.lse_rows(sc), 3.0 + 0.25 * (h % 8))[:, None]
    assert attn_rel_err(outs["on"], want) <= 1e-5
    assert min(attn_rel_err(want[:, :, h:h + 1], outs["off"][:, :, h:h + 1]) for h in range(H)) >= 5e-2
    assert not np.allclose(outs["on"][0, :, 0] / outs["off"][0, :, 0], outs["on"][0, :, 1] / outs["off"][0, :, 1])  # per head
