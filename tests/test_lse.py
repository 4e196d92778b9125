"""The row log-sum-exp (fattn_ext_lse) and the KV-shard merge (fattn_lse_merge) on
the CPU: the ABI (host-only planning with fake pointers: every check below
returns before anything would launch), the float64 references of tests/lse.py,
the shard helpers and the harness's CPU path."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fattn
import lse as ls
import op_params as op
import plans
import sinks as sk
from fattn import shard
from gpu_util import run_kernel_test
from oracle import oracle as orc
from plans import plan_params as _params
from problems import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, HEAD_DIM, BAD_STRIDE, WORKSPACE, ALIGNMENT = -1, -3, -4, -5, -7
A = 1 << 21   # a made-up, 16-byte aligned device address


def _header():
    return open(os.path.join(ROOT, "include", "fattn.h")).read()


# ------------------------------------------------------------------ the ABI

def test_entry_points_are_exported_and_declared():
    assert "fattn_ext_lse" in fattn.EXPORTS and "fattn_lse_merge" in fattn.EXPORTS
    L = fattn.lib()
    assert L.fattn_ext_lse is not None and L.fattn_lse_merge is not None
    hdr = re.sub(r"\s+", " ", _header())
    assert "int fattn_ext_lse(const fattn_params* p, const float* sinks, float* lse, void* stream);" in hdr
    assert ("int fattn_lse_merge(const float* outs, const float* lses, int32_t n_parts, int64_t n_rows, int32_t dv, "
            "int64_t out_part_stride, int64_t lse_part_stride, const float* sinks, int32_t n_head, float* dst, "
            "float* lse_out, void* stream);") in hdr
    assert "int fattn_ext_sinks(const fattn_params* p, const float* sinks, void* stream);" in hdr
    P = fattn.FattnParams
    assert [f[0] for f in P._fields_][-1] == "head_first" and not any("lse" in f[0] for f in P._fields_)


SHAPES = {"config3": dict(), "config5": dict(NQ=64), "prefill": dict(NQ=4096), "nomask": dict(mask=False),
          "mla": dict(D=576, dk=576, dv=512, H=16, Hkv=1, N=416, kt=fattn.TYPE_F16)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_misaligned_lse_pointer_is_an_alignment_error(shape):
    """Checked beside sinks, before the workspace and before anything launches."""
    p = _params(**SHAPES[shape])
    L = fattn.lib()
    for off in (1, 2, 3, 5, 6, 7):
        assert L.fattn_ext_lse(C.byref(p), None, A + off, None) == ALIGNMENT, off
        assert L.fattn_ext_lse(C.byref(p), A, A + off, None) == ALIGNMENT, off
    assert L.fattn_ext_lse(C.byref(p), A + 2, A, None) == ALIGNMENT
    if fattn.workspace_size(p):
        assert L.fattn_ext_lse(C.byref(p), None, A, None) == WORKSPACE


BAD = [dict(D=72), dict(H=6, Hkv=4), dict(max_bias=-1.0), dict(logit_softcap=float("nan")), dict(ptr=(1 << 20) + 4),
       dict(n_head_total=16, head_first=0)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_invalid_params_win_over_a_bad_lse(bad):
    p = _params(**bad)
    L = fattn.lib()
    want = L.fattn_ext(C.byref(p), None)
    assert want != 0
    for lse in (None, A, A + 2):
        assert L.fattn_ext_lse(C.byref(p), None, lse, None) == want, lse


def _merge(outs=A, lses=A, n_parts=2, n_rows=8, dv=64, ostride=None, lstride=None, sinks=None, n_head=0, dst=2 * A, lse_out=None):
    ostride = n_rows * dv if ostride is None else ostride
    lstride = n_rows if lstride is None else lstride
    return fattn.lib().fattn_lse_merge(outs, lses, n_parts, n_rows, dv, ostride, lstride, sinks, n_head, dst, lse_out, None)


REFUSED = {
    "outs NULL": (dict(outs=None), INVALID_ARG), "lses NULL": (dict(lses=None), INVALID_ARG), "dst NULL": (dict(dst=None), INVALID_ARG),
    "n_parts 0": (dict(n_parts=0), INVALID_ARG), "n_parts 65": (dict(n_parts=65), INVALID_ARG),
    "n_rows 0": (dict(n_rows=0), INVALID_ARG), "n_rows 2^31": (dict(n_rows=1 << 31, dv=4), INVALID_ARG),
    "n_head 0 with sinks": (dict(sinks=A, n_head=0), INVALID_ARG),
    "dv 0": (dict(dv=0), HEAD_DIM), "dv 66": (dict(dv=66), HEAD_DIM), "dv 516": (dict(dv=516), HEAD_DIM),
    "out stride short": (dict(ostride=8 * 64 - 4), BAD_STRIDE), "out stride % 4": (dict(ostride=8 * 64 + 2), BAD_STRIDE),
    "lse stride short": (dict(lstride=7), BAD_STRIDE),
    "outs + 4": (dict(outs=A + 4), ALIGNMENT), "dst + 8": (dict(dst=2 * A + 8), ALIGNMENT), "lses + 2": (dict(lses=A + 2), ALIGNMENT),
    "lse_out + 1": (dict(lse_out=A + 1), ALIGNMENT), "sinks + 2": (dict(sinks=A + 2, n_head=4), ALIGNMENT),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_merge_refusals(what):
    """Each before anything launches (no device memory stands behind these pointers)."""
    kw, want = REFUSED[what]
    assert _merge(**kw) == want


FAMILY_PARAMS = {"split": dict(), "mq": dict(NQ=40, H=16, Hkv=4, N=320), "bd": dict(NQ=64, H=2, Hkv=2, N=800),
                 "pf": dict(NQ=4096, H=2, Hkv=2, N=4096), "mla": SHAPES["mla"]}


@pytest.mark.parametrize("family", list(FAMILY_PARAMS))
def test_plan_and_workspace_are_functions_of_the_params_alone(family):
    """What can be said on the host: describe and workspace_size have no lse
    argument to depend on, and a refused fattn_ext_lse leaves no state behind.
    That the lse LAUNCH runs the very plan describe(p) names, and leaves dst
    bit for bit, is what tests/test_gpu_lse.py checks on every case."""
    hdr = re.sub(r"[\s\*]+", " ", _header())
    assert "the workspace size and fattn_describe(p) stay functions of p alone" in hdr
    assert len(fattn.lib().fattn_describe.argtypes) == 3 and len(fattn.lib().fattn_workspace_size.argtypes) == 1
    p = _params(**FAMILY_PARAMS[family])
    d, ws = fattn.describe(p), fattn.workspace_size(p)
    fattn.lib().fattn_ext_lse(C.byref(p), None, A + 2, None)          # (returns before it would launch)
    assert fattn.describe(p) == d and fattn.workspace_size(p) == ws and "lse" not in d


def test_python_mirror_checks_lse():
    p = _params(H=32)
    with pytest.raises(ValueError):
        fattn.flash_attn_ext(p, stream=0, ev_begin=1, ev_end=2, lse=A)
    with pytest.raises(ValueError):
        fattn.flash_attn_ext(p, stream=0, ev_end=2, lse=A)
    with pytest.raises(fattn.FattnError) as e:                          # a pointer goes straight to the C ABI
        fattn.flash_attn_ext(p, stream=0, lse=A + 2)
    assert e.value.code == ALIGNMENT
    for bad in (torch.zeros(32, dtype=torch.float64), torch.zeros(64)[::2], torch.zeros(32), torch.zeros(31)):
        with pytest.raises(ValueError):                                 # dtype, contiguity, host tensor, count
            fattn.flash_attn_ext(p, stream=0, lse=bad)
    att = fattn.Attention.__new__(fattn.Attention)
    att.p, att.sinks, att.lse = p, None, A
    att.retarget(lse=None)
    assert att.lse == A
    att.retarget(lse=fattn.NO_LSE)
    assert att.lse is None


# ------------------------------------------------------------------ the references

def _f64_parts(o, ranges):
    """Per key range, float64 (out [S][NQ][H][D], lse [S][NQ][H]) of softmax(scores) . V over that range alone."""
    b = o.base
    V = op._decode(o.v).astype(np.float64)
    rk2, rk3 = b.H // b.Hkv, b.S // b.Skv
    outs = np.empty((len(ranges), b.S, b.NQ, b.H, b.D))
    lses = np.empty((len(ranges), b.S, b.NQ, b.H))
    for s, h, sc in ls.scores64(o):
        for i, (lo, hi) in enumerate(ranges):
            x = sc[:, lo:hi]
            with np.errstate(invalid="ignore", divide="ignore"):
                m = x.max(axis=1, keepdims=True)
                e = np.exp(x - m)                                       # (a range without a live key: NaN, as a launch leaves it)
                outs[i, s, :, h, :] = (e / e.sum(axis=1, keepdims=True)) @ V[s // rk3, h // rk2, lo:hi]
            lses[i, s, :, h] = sk.lse_rows(x)
    return outs, lses


@pytest.mark.parametrize("cuts", [(0, 320, 800), (0, 96, 512, 800)], ids=["320+480", "96+416+288"])
def test_merge_ref_over_key_ranges_is_the_unsharded_reference(cuts):
    spec = plans.OP_BY_ID["split_gqa_merge-D128-q8_0-q3h8kv2n800"]
    o = ls.spec_op(spec, ls.shard_mask(3, 800))
    ranges = list(zip(cuts[:-1], cuts[1:]))
    outs, lses = _f64_parts(o, ranges)
    assert np.isneginf(lses[-1]).any() and np.isnan(outs[-1]).any()     # rows the last range masks out entirely
    (full,), (full_lse,) = _f64_parts(o, [(0, 800)])
    got, got_lse = ls.merge_ref(outs, lses)
    assert not np.isnan(got).any()
    assert np.abs(got - full).max() <= 1e-12 * np.abs(full).max() and np.abs(got_lse - full_lse).max() <= 1e-12
    # with sinks at the merge: the factor form over the whole range
    s = ls.sink_values(8, 800).astype(np.float64)
    got_s, lse_s = ls.merge_ref(outs, lses, s)
    g = 1.0 / (1.0 + np.exp(s[None, None, :] - full_lse))
    assert np.abs(got_s - full * g[..., None]).max() <= 1e-12 and np.abs(lse_s - np.logaddexp(full_lse, s[None, None, :])).max() <= 1e-12


def test_merge_ref_edge_rows():
    outs = np.array([[[1.0, 2.0]], [[np.nan, np.nan]]])
    d, l = ls.merge_ref(outs, np.array([[0.5], [-np.inf]]))
    assert np.array_equal(d, [[1.0, 2.0]]) and l[0] == 0.5              # one part: a copy
    d, l = ls.merge_ref(outs, np.array([[-np.inf], [-np.inf]]))
    assert np.isnan(d).all() and np.isneginf(l[0])
    d, l = ls.merge_ref(outs, np.array([[-np.inf], [-np.inf]]), sinks=np.array([1.5]))
    assert (d == 0).all() and l[0] == 1.5


def test_lse_is_consistent_with_the_sink_factor():
    """g = 1 / (1 + exp(s - lse)) (include/fattn.h): the log-sum-exp with the sink is lse - ln g."""
    p = make_problem(D=128, NQ=3, H=6, Hkv=2, N=200, kv_type="q8_0", seed=22, mask="none")
    o = op.one_plane(p, op.random_mask(3, 200))
    s = np.linspace(2.0, 7.0, 6).astype(np.float32)
    plain, with_s = ls.lse_ref(o), ls.lse_ref(o, s)
    for h in range(6):
        g = sk.factor(plain[0, :, h], s[h]).astype(np.float64)
        assert np.abs(with_s[0, :, h] - (plain[0, :, h] - np.log(g))).max() <= 1e-6
    assert ls.ref_uncertainty(o) <= ls.REF_WORST
    assert ls.LSE_ATOL == 8 * ls.REF_WORST


# ------------------------------------------------------------------ shard helpers

def test_kv_ranges():
    assert shard.kv_ranges(800, 2) == [(0, 384), (384, 800)]
    assert shard.kv_ranges(800, 3) == [(0, 256), (256, 512), (512, 800)]
    assert shard.kv_ranges(384, 2, align=64) == [(0, 192), (192, 384)] and shard.kv_ranges(100, 1) == [(0, 100)]
    for N, world, align in ((4097, 8, 32), (1000, 3, 64), (96, 3, 32)):
        r = shard.kv_ranges(N, world, align)
        assert r[0][0] == 0 and r[-1][1] == N and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(lo % align == 0 and lo < hi for lo, hi in r)
    for bad in ((63, 2, 32), (100, 0, 32), (100, 2, 0)):
        with pytest.raises(ValueError):
            shard.kv_ranges(*bad)


def test_kv_views_arithmetic():
    rb = fattn.row_size(fattn.TYPE_Q8_0, 128)
    k = fattn.View(A, fattn.TYPE_Q8_0, (128, 800, 4, 1), (34, rb, rb * 800, rb * 3200))
    v = fattn.View(3 * A, fattn.TYPE_Q8_0, (128, 800, 4, 1), (34, rb * 4, rb, rb * 3200))       # "pos" layout
    m = fattn.View(5 * A, fattn.TYPE_F16, (832, 3, 1, 1), (2, 1664, 4992, 4992))
    kk, vv, mm = shard.kv_views(k, v, m, 320, 512)
    assert (kk.ptr, tuple(kk.ne), tuple(kk.nb)) == (A + 320 * rb, (128, 192, 4, 1), tuple(k.nb))
    assert (vv.ptr, tuple(vv.ne), tuple(vv.nb)) == (3 * A + 320 * rb * 4, (128, 192, 4, 1), tuple(v.nb))
    assert (mm.ptr, tuple(mm.ne), tuple(mm.nb)) == (5 * A + 640, (192, 3, 1, 1), tuple(m.nb))
    _, _, last = shard.kv_views(k, v, m, 512, 800)
    assert tuple(last.ne) == (320, 3, 1, 1)                              # the last range keeps the rows' padding
    assert shard.kv_views(k, v, None, 0, 32)[2] is None
    for lo, hi in ((-32, 64), (64, 64), (0, 801)):
        with pytest.raises(ValueError):
            shard.kv_views(k, v, m, lo, hi)
    # MLA: V is a view of K and stays one, at the same offset, in every range
    mk = fattn.kv_view(torch.zeros(1), fattn.TYPE_F16, fattn.MLA_DK, 416, 1)
    mv = fattn.mla_v_view(mk)
    assert mv.ptr - mk.ptr == 128
    for lo, hi in shard.kv_ranges(416, 3):
        kk, vv, _ = shard.kv_views(mk, mv, None, lo, hi)
        assert vv.ptr - kk.ptr == 128 and tuple(vv.nb) == tuple(kk.nb) and kk.ptr == mk.ptr + lo * 1152
        assert tuple(kk.ne) == (576, hi - lo, 1, 1) and tuple(vv.ne) == (512, hi - lo, 1, 1)
        p = fattn.ext_params(fattn.View(A, fattn.TYPE_F32, (576, 1, 16, 1), (4, 16 * 2304, 2304, 16 * 2304)),
                             fattn.View(A + kk.ptr - mk.ptr, kk.type, kk.ne, kk.nb), fattn.View(A + vv.ptr - mk.ptr, vv.type, vv.ne, vv.nb),
                             None, A, 0.07)
        assert "v=k+128" in fattn.describe(p)


# ------------------------------------------------------------------ two ranks

NQ_, H_, N_, D_ = 3, 4, 160, 16


def _toy():
    rng = np.random.default_rng(4)
    sc = rng.standard_normal((NQ_, H_, N_))
    sc[0, :, 64:] = -np.inf                                            # row 0 has no key in the second rank's range
    return sc, rng.standard_normal((N_, D_))


def _toy_part(sc, v, lo, hi):
    x = sc[..., lo:hi]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        out = (e / e.sum(axis=-1, keepdims=True)) @ v[lo:hi]
    return out, sk.lse_rows(x.reshape(-1, hi - lo)).reshape(NQ_, H_)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc, v = _toy()
        lo, hi = shard.kv_ranges(N_, world)[rank]
        out, lse = _toy_part(sc, v, lo, hi)
        outs, lses = shard.gather_parts(torch.from_numpy(out), torch.from_numpy(lse))
        assert outs.shape == (world, NQ_, H_, D_) and lses.shape == (world, NQ_, H_)
        if rank == 0:
            q.put((outs.numpy(), lses.numpy()))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_gather_and_merge_equals_single_process():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        outs, lses = q.get(timeout=120)
    finally:
        for p in procs:
            p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs)
    assert np.isnan(outs[1, 0]).all() and np.isneginf(lses[1, 0]).all()
    sc, v = _toy()
    full, full_lse = _toy_part(sc, v, 0, N_)
    got, got_lse = ls.merge_ref(outs, lses)
    assert np.abs(got - full).max() <= 1e-12 and np.abs(got_lse - full_lse).max() <= 1e-12


# ------------------------------------------------------------------ harness

@pytest.mark.parametrize("sinks", [False, True])
def test_harness_cpu_reference_has_the_lse(tmp_path, sinks):
    """kernel_test --lse --cpu-only against a float64 log-sum-exp over the
    harness's own inputs (the rand() stream in the order Q, K, V, mask; its mask
    stays f32).  f32 expf / logf over 96 keys: 1e-5."""
    H, Hkv, D, N, NQ = 10, 2, 64, 96, 2
    f = tmp_path / "out.bin"
    r = run_kernel_test(["--lse", "--cpu-only", "--heads", H, "--kv-heads", Hkv, "--head-dim", D, "--kv-size", N, "--n-q", NQ,
                         "--dump", f] + (["--sinks", "3"] if sinks else []))
    assert r.returncode == 0, r.stderr
    assert "Reference LSE" in r.stdout
    got = np.fromfile(str(f) + ".lse", dtype=np.float32).reshape(NQ, H)
    orc.srand(1)
    q = orc.random(D * H * NQ).reshape(NQ, H, D)
    k = orc.random(D * N * Hkv).reshape(Hkv, N, D)
    orc.random(D * N * Hkv)
    m = orc.random(N * NQ).reshape(NQ, N)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    for h in range(H):
        sc = orc.mulmat_f32(np.ascontiguousarray(q[:, h]), k[h // (H // Hkv)], None, NQ, N, D, float(scale), 1).reshape(NQ, N) + m
        want = sk.lse_rows(sc)
        if sinks:
            want = np.logaddexp(want, 3.0 + 0.25 * (h % 8))
        assert np.abs(got[:, h] - want).max() <= 1e-5, h


def test_harness_mla_cpu_path_prints_the_lse():
    r = run_kernel_test(["--lse", "--cpu-only", "--mla", "--heads", "4", "--kv-size", "64"])
    assert r.returncode == 0 and "Reference LSE" in r.stdout
