"""GPU: the row log-sum-exp of fattn_ext_lse on every plan and at every epilogue
that normalises into dst, and fattn_lse_merge over KV-sharded partials.

  every plan     tests/plans.py's OP_SPECS, the pf4 rows of PLANE_SPECS, five MLA
                 forms, a BF16 and a Q5_1 split row: describe() names the kernel,
                 dst is bit-equal to the launch without lse, lse is within the bar,
                 every guard band (lse's own included) is intact
  epilogues      the one-row and GQA split shapes under each split epilogue
  scalars        logit_softcap, max_bias, head / sequence mask planes, sinks (the
                 sink is a term of lse), a -inf sink, fully masked rows
  KV shards      the keys cut into two and three uneven ranges, each launched
                 without sinks, merged by fattn_lse_merge: the unsharded reference
                 under the suite's bars, lse_out within the LSE bar
  the merge      fattn_lse_merge alone against lse.merge_ref
  capture        two ranges plus the merge in one graph, replayed twice
  the harness    kernel_test --lse

The LSE bar is tests/lse.py's: |lse - ref| <= LSE_ATOL + 4 ulp_f32(|ref|), -inf
positions coinciding.  Every case prints an `LSE` line with its worst error
before it asserts (profiles/lse/errors.txt).
"""
import numpy as np
import pytest

import fattn
import lse as ls
import plans
from fattn import shard
from gpu_util import DST_GUARD_BYTES, SENTINEL, capture, check_bars, run_kernel_test

pytestmark = pytest.mark.gpu

_refs = {}


def _lse_ref(case):
    if case.id not in _refs:
        _refs[case.id] = case.lse_ref()
    return _refs[case.id]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _run(case, dev, tag=None):
    """The case with and without lse: (describe, dst, lse) after the common checks."""
    with fattn.options(dict(case.opts)):
        g = ls.LseLaunch.of(case.make(dev))
        d = g.describe()
        for w in case.want:
            assert w in d, (w, d)
        if "no" in case.extra:
            assert case.extra["no"] not in d, d
        assert "lse" not in d, d
        plain = g.run_without()
        assert np.isnan(g.lse_out()).all(), "the launch without lse wrote lse"
        got = g.run().copy()
        lse = g.lse_out()
    assert np.array_equal(_bits(got), _bits(plain)), f"{case.id}: dst differs from the launch without lse"
    ls.check_lse(lse, _lse_ref(case), f"{tag or case.id} | {d.split(' grid(')[0]}")
    assert g.guards_intact(), d
    return d, got, lse


# ------------------------------------------------------------------ every plan

EVERY = ls.every_plan()


@pytest.mark.parametrize("case", EVERY, ids=[c.id for c in EVERY])
def test_every_plan(dev, case):
    _run(case, dev)


# ------------------------------------------------------------------ split epilogues

EPI_SHAPES = [plans.OP_BY_ID[i] for i in ("split_row-D128-q8_0-q1h4kv4n256", "split_row_tail-D128-q8_0-q1h4kv4n200",
                                          "split_chunks-D128-q8_0-q2h8kv4n1500", "split_gqa_merge-D128-q8_0-q3h8kv2n800")]
W8 = (fattn.OPT_SPLIT_WAVES, 8)
# name -> (options, kv_chunk for the one-row shapes (0: the spec's), what describe() says where the epilogue is named)
EPILOGUES = {
    "wave-merge-1": ((), 64, ",4waves>"),                       # one-row tiles, several chunks: the last-arriving wave merges
    "wave-merge-2": ((W8,), 64, ",8waves>"),                    # ... wg_row_merge: one partial per workgroup
    "opt-wave-merge-1": (((fattn.OPT_SPLIT_WAVE_MERGE, 1),), 64, ",4waves>"),   # ... the workgroup-level merge of all other tiles
    "opt-split-merge-1": (((fattn.OPT_SPLIT_MERGE, 1),), 0, None),               # combine_tile
    "merge-in-kernel": (((fattn.OPT_MERGE_IN_KERNEL, 1),), 0, None),
    "part-f16-1": (((fattn.OPT_PART_F16, 1),), 0, None),
    "part-f16-2": (((fattn.OPT_PART_F16, 2),), 0, None),
    "8waves": ((W8,), 0, ",8waves>"),
}


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("spec", EPI_SHAPES, ids=[s.id for s in EPI_SHAPES])
def test_split_epilogues(dev, spec, epi):
    opts, row_chunk, says = EPILOGUES[epi]
    one_row = spec.shape[0] == 1
    case = ls.spec_case(spec, tag=f"-{epi}", opts=opts, kv_chunk=row_chunk if one_row and row_chunk else None)
    case.id = spec.id          # (one reference per shape)
    d, _, _ = _run(case, dev, tag=f"{spec.id} {epi}")
    if says and (one_row or epi == "8waves") and (",gran16," in d or "4waves" in says):
        assert says in d, d                                 # (8 waves: the 16-B row path only)
    if one_row and epi in ("wave-merge-1", "opt-wave-merge-1"):
        assert " grid(1," not in d, d                       # several chunks (8 waves: chunks of 256 keys, one here)
    if not one_row:
        merged = " + fattn_merge_kernel" in d or "(in-kernel merge)" in d
        if epi == "opt-split-merge-1":
            assert not merged, d
        if epi == "merge-in-kernel" and " grid(1," not in d:
            assert "(in-kernel merge)" in d or " + fattn_merge_kernel" not in d, d
        if epi == "part-f16-2" and " + fattn_merge_kernel" in d:
            assert "(f16 partials)" in d, d
        if epi == "part-f16-1":
            assert "(f16 partials)" not in d, d


def test_wg_row_merge_several_chunks(dev):
    """One-row tiles, 8 waves, four chunks of 256 keys: each workgroup publishes one
    row and the last one merges them (wg_row_merge -> merge_row_parts), config 3's
    own epilogue.  (At N = 256 / 200 the 8-wave cases above are one chunk.)"""
    d, _, _ = _run(ls.row_wg_case(), dev)
    assert ",8waves>" in d and " grid(4,4,1)" in d and " + fattn_merge_kernel" not in d, d


# ------------------------------------------------------------------ scalars and masks

SCALARS = [c for s in plans.FAMILIES for c in ls.scalar_cases(s)]


@pytest.mark.parametrize("case", SCALARS, ids=[c.id for c in SCALARS])
def test_scalars_and_masks(dev, case):
    d, got, lse = _run(case, dev)
    ref = _lse_ref(case)
    if case.id.endswith("-window"):
        assert np.isneginf(ref).any() and np.isneginf(lse[np.isneginf(ref)]).all()
        assert np.isnan(got[np.isneginf(ref)]).all()
    if case.id.endswith("-window-sinks"):
        dead = np.isneginf(ls.lse_ref(case.o))
        assert dead.any()
        want = np.broadcast_to(case.sinks[None, None, :], lse.shape)
        assert np.array_equal(_bits(lse[dead]), _bits(want[dead])), "a fully masked row's lse is its head's sink"
        assert (got[dead] == 0.0).all()
    if case.id.endswith("-sinks") and not case.id.endswith("-window-sinks"):
        assert (np.abs(ref - ls.lse_ref(case.o)) > 10 * ls.LSE_ATOL).all()   # (the sink moves every row's lse)


@pytest.mark.parametrize("spec", plans.FAMILIES, ids=[s.id for s in plans.FAMILIES])
def test_neg_inf_sink_is_no_sink(dev, spec):
    """sinks = -inf for every head: dst and lse bit-equal to the launch without sinks."""
    a = ls.spec_case(spec)
    b = ls.spec_case(spec, sinks=np.full(spec.shape[1], -np.inf, dtype=np.float32), tag="-neginf-sink")
    _, got_a, lse_a = _run(a, dev)
    b.id = a.id
    _, got_b, lse_b = _run(b, dev, tag=spec.id + " sinks -inf")
    assert np.array_equal(_bits(got_a), _bits(got_b)) and np.array_equal(_bits(lse_a), _bits(lse_b))


# ------------------------------------------------------------------ KV shards

def _view(t):
    return fattn.View(int(t.data), int(t.type), tuple(int(x) for x in t.ne), tuple(int(x) for x in t.nb))


class Shards:
    """The launch of a GuardedLaunch `g` cut into key ranges: range i writes part i of
    (outs, lses), each with a workspace of its own; merge() is fattn.lse_merge."""

    def __init__(self, g, ranges, dev, sinks=None):
        import torch
        p = g.p
        self.g = g
        dv = g.out_shape[-1]
        rows = g.n_out // dv
        P = len(ranges)
        nan = float("nan")
        self.outs = torch.full((P,) + tuple(g.out_shape), nan, dtype=torch.float32, device=dev)
        self.lses = torch.full((P,) + tuple(g.out_shape[:-1]), nan, dtype=torch.float32, device=dev)
        gd = DST_GUARD_BYTES // 4
        self.dst_all = torch.full((gd + rows * dv + gd,), SENTINEL, dtype=torch.int32, device=dev)
        self.dst = self.dst_all[gd:gd + rows * dv].view(torch.float32).view(g.out_shape)
        self.lse_all = torch.full((gd + rows + gd,), SENTINEL, dtype=torch.int32, device=dev)
        self.lse = self.lse_all[gd:gd + rows].view(torch.float32).view(g.out_shape[:-1])
        self.sinks = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks, dtype=np.float32)).to(dev)
        self.params, self.ws = [], []
        q, k, v = _view(p.q), _view(p.k), _view(p.v)
        m = _view(p.mask) if p.mask.data else None
        for i, (lo, hi) in enumerate(ranges):
            kk, vv, mm = shard.kv_views(k, v, m, lo, hi)
            pr = fattn.ext_params(q, kk, vv, mm, self.outs[i].data_ptr(), p.scale, 0, 0, p.kv_chunk, max_bias=p.max_bias,
                                  logit_softcap=p.logit_softcap, n_head_total=p.n_head_total, head_first=p.head_first)
            ws = torch.zeros(max(fattn.workspace_size(pr), 16), dtype=torch.uint8, device=dev)
            pr.workspace, pr.workspace_bytes = ws.data_ptr(), ws.numel()
            self.params.append(pr)
            self.ws.append(ws)

    def launch(self, stream=None):
        for i, pr in enumerate(self.params):
            fattn.flash_attn_ext(pr, stream, lse=self.lses[i])       # (never with sinks: they go to the merge)
        fattn.lse_merge(self.outs, self.lses, self.dst, sinks=self.sinks, lse_out=self.lse, stream=stream)

    def run(self):
        import torch
        self.dst.fill_(float("nan"))
        self.lse.fill_(float("nan"))
        self.launch()
        torch.cuda.synchronize()
        return self.dst.cpu().numpy(), self.lse.cpu().numpy()

    def guards_intact(self):
        gd = DST_GUARD_BYTES // 4
        return all(bool((b[:gd] == SENTINEL).all() and (b[-gd:] == SENTINEL).all())
                   for b in (self.dst_all.cpu().numpy().view(np.uint32), self.lse_all.cpu().numpy().view(np.uint32)))


def _cuts(N, align):
    """Two and three uneven ranges of [0, N), every boundary a multiple of `align`."""
    u = N // align
    a = max(1, (2 * u) // 5)
    b1, b2 = max(1, u // 8), max(2, u // 8 + (u * 13) // 25)
    two = [(0, a * align), (a * align, N)]
    three = [(0, b1 * align), (b1 * align, b2 * align), (b2 * align, N)]
    return {2: two, 3: three}


def _shard_cases():
    out = []
    for spec in plans.FAMILIES:
        NQ, H, Hkv, N = spec.shape
        c = ls.spec_case(spec, ls.shard_mask(NQ, N), tag="-shard")
        out.append((c, N, 64 if spec.family == "pf" else 32, lambda c=c: c.o.reference()))
    import mla
    mc = ls.shard_mla()
    out.append((ls.Case("mla-f16-view-decode-n160-shard", mc.ref, lambda dev: mla.MlaGpu(mc, dev=dev), ("fattn_mla_kernel<f16",)),
                160, 32, mc.reference))
    b = ls.kv_case("bf16")
    out.append((b, 256, 32, lambda: b.o.reference()))
    return out


SHARDS = _shard_cases()


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("entry", SHARDS, ids=[e[0].id for e in SHARDS])
def test_kv_shard_round_trip(dev, entry, parts):
    case, N, align, reference = entry
    ranges = _cuts(N, align)[parts]
    assert ranges[0][0] == 0 and ranges[-1][1] == N and all(lo % align == 0 and lo < hi for lo, hi in ranges)
    assert shard.kv_ranges(N, parts, align)[0][0] == 0
    key = ("shard-ref", case.id)
    if key not in _refs:
        _refs[key] = reference()
    ref = _refs[key]
    with fattn.options(dict(case.opts)):
        sh = Shards(case.make(dev), ranges, dev)
        got, lse = sh.run()
        partial = sh.outs.cpu().numpy()
    if case.o.base.NQ > 1:   # the early rows have no key in the last range: their partial rows are NaN there
        assert np.isnan(partial[-1]).any() and np.isneginf(sh.lses[-1].cpu().numpy()).any()
    assert not np.isnan(ref).any()
    check_bars(got, ref, lambda rel, el: f"LSE shard {case.id} {[hi - lo for lo, hi in ranges]}: merged->reference {rel:.3e} elem {el:.3f}")
    ls.check_lse(lse, _lse_ref(case), f"shard {case.id} x{parts} lse_out")
    assert sh.guards_intact()


def test_kv_shards_with_sinks_at_the_merge(dev):
    """Shard launches without sinks, the sinks given to the merge once: fattn_ext_sinks over the whole range."""
    import sinks as sk
    spec = plans.FAMILIES[0]
    NQ, H, Hkv, N = spec.shape
    s = ls.sink_values(H, N)
    plain = ls.spec_case(spec, ls.shard_mask(NQ, N), tag="-shard")
    full = ls.spec_case(spec, ls.shard_mask(NQ, N), sinks=s, tag="-shard-sinks")
    ref = sk.reference(sk.with_sinks(full.o, s))
    with fattn.options(dict(spec.opts)):
        _, whole, whole_lse = _run(full, dev)
        sh = Shards(plain.make(dev), _cuts(N, 32)[3], dev, sinks=s)
        got, lse = sh.run()
    check_bars(got, ref, lambda rel, el: f"LSE shard+sinks {spec.id}: merged->factor-form {rel:.3e} elem {el:.3f}")
    check_bars(got, whole, lambda rel, el: f"LSE shard+sinks {spec.id}: merged->fattn_ext_sinks {rel:.3e} elem {el:.3f}")
    ls.check_lse(lse, _lse_ref(full), "shard+sinks lse_out")
    assert sh.guards_intact()


# ------------------------------------------------------------------ the merge kernel alone

def _merge_inputs(P, rows, dv, seed, pad_o=8, pad_l=3):
    rng = np.random.default_rng(seed)
    outs = rng.standard_normal((P, rows, dv)).astype(np.float32)
    lses = (3.0 * rng.standard_normal((P, rows))).astype(np.float32)
    lses[rng.random((P, rows)) < 0.2] = -np.inf
    if rows > 2:
        lses[:, 2] = -np.inf                                   # a row no part has a key for
    outs[np.isneginf(lses)] = np.nan                            # what a launch leaves there
    return outs, lses


def _merge_gpu(outs, lses, dev, sinks=None, want_lse=True, pad_o=8, pad_l=3):
    import torch
    P, rows, dv = outs.shape
    ob = torch.full((P, rows * dv + pad_o), float("nan"), dtype=torch.float32, device=dev)
    lb = torch.full((P, rows + pad_l), float("nan"), dtype=torch.float32, device=dev)
    ob[:, :rows * dv] = torch.from_numpy(outs.reshape(P, -1)).to(dev)
    lb[:, :rows] = torch.from_numpy(lses).to(dev)
    gd = DST_GUARD_BYTES // 4
    dst_all = torch.full((gd + rows * dv + gd,), SENTINEL, dtype=torch.int32, device=dev)
    lse_all = torch.full((gd + rows + gd,), SENTINEL, dtype=torch.int32, device=dev)
    dst = dst_all[gd:gd + rows * dv].view(torch.float32).view(rows, dv)
    lse = lse_all[gd:gd + rows].view(torch.float32)
    st = None if sinks is None else torch.from_numpy(sinks).to(dev)
    fattn.lse_merge(ob[:, :rows * dv].view(P, rows, dv), lb[:, :rows], dst, sinks=st, lse_out=lse if want_lse else None)
    torch.cuda.synchronize()
    for b, n in ((dst_all, rows * dv), (lse_all, rows)):
        x = b.cpu().numpy().view(np.uint32)
        assert (x[:gd] == SENTINEL).all() and (x[gd + n:] == SENTINEL).all(), "guard band overwritten"
    if not want_lse:
        assert (lse_all.cpu().numpy().view(np.uint32) == SENTINEL).all(), "lse_out = NULL wrote something"
    return dst.cpu().numpy(), lse.cpu().numpy()


def _check_merge(outs, lses, got, got_lse, sinks, tag):
    """dst elementwise against merge_ref, relative to A = sum_p w_p |out_p| / L.
    The bound counts f32 roundings (eps = 2^-24 each, relative to A or to a
    term of it): a weight w_p carries v_exp_f32's ulp and one product (the
    kernel carries the rounding of the exponent's argument in a second float:
    left in, it would be |lse_p - M| log2e eps relative, 20 eps for every part
    under a sink 14 above them), the product w_p out_p one, the running sum one
    per part, L the same again and the division one: below (4 n_parts + 4) eps.
    Taken as (2 n_parts + 4) 2^-23.  What the count leaves out is the f32
    subtraction lse_p - M itself, half an ulp of the difference: |lse_p - M| eps
    relative in w_p, which matters only where every part lies far below a
    dominant sink (measured worst: 0.88 of the bound, one part 14 below its sink)."""
    P = outs.shape[0]
    ref, ref_lse = ls.merge_ref(outs, lses, sinks)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    l64 = lses.astype(np.float64)
    R = l64.shape[1]
    s = np.full(R, -np.inf) if sinks is None else sinks.astype(np.float64)[np.arange(R) % len(sinks)]
    M = np.maximum(l64.max(axis=0), s)
    Ms = np.where(np.isfinite(M), M, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(np.isneginf(l64), 0.0, np.exp(l64 - Ms))
        L = w.sum(axis=0) + np.where(np.isneginf(s), 0.0, np.exp(s - Ms))
        A = np.where((w > 0)[:, :, None], w[:, :, None] * np.abs(outs.astype(np.float64)), 0.0).sum(axis=0) / L[:, None]
    ok = ~np.isnan(ref)
    bound = (2 * P + 4) * 2.0 ** -23 * np.nan_to_num(A) + 1e-37    # (a row without a term: L = 0, zeros or NaN exactly)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"LSE merge {tag}: worst |dst - ref| / bound {worst:.3f}")
    assert worst <= 1.0, tag
    if got_lse is not None:
        ls.check_lse(got_lse, ref_lse, f"merge {tag} lse_out")


@pytest.mark.parametrize("rows", [1, 7, 130])
@pytest.mark.parametrize("dv", [64, 80, 512])
@pytest.mark.parametrize("P", [1, 2, 5, 64])
def test_merge_kernel(dev, P, dv, rows):
    outs, lses = _merge_inputs(P, rows, dv, seed=1000 * P + dv + rows)
    got, got_lse = _merge_gpu(outs, lses, dev)
    _check_merge(outs, lses, got, got_lse, None, f"P{P} dv{dv} rows{rows}")
    if rows > 2:
        assert np.isnan(got[2]).all() and np.isneginf(got_lse[2])
    sinks = np.array([0.5, -np.inf, 4.0, -3.0], dtype=np.float32)
    got_s, lse_s = _merge_gpu(outs, lses, dev, sinks=sinks)
    _check_merge(outs, lses, got_s, lse_s, sinks, f"P{P} dv{dv} rows{rows} sinks")
    if rows > 2:   # row 2 is head 2: zeros and the sink itself
        assert (got_s[2] == 0.0).all() and lse_s[2] == sinks[2]
    again, _ = _merge_gpu(outs, lses, dev, want_lse=False)
    assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("dv", [64, 80, 512])
def test_merge_of_one_part_is_a_copy(dev, dv):
    rng = np.random.default_rng(5)
    outs = rng.standard_normal((1, 130, dv)).astype(np.float32)
    outs[0, 3, :4] = [-0.0, 0.0, np.float32(1e-41), np.float32(-3e38)]
    lses = (5.0 * rng.standard_normal((1, 130))).astype(np.float32)
    got, got_lse = _merge_gpu(outs, lses, dev)
    assert np.array_equal(_bits(got), _bits(outs[0])) and np.array_equal(_bits(got_lse), _bits(lses[0]))


# ------------------------------------------------------------------ capture

def test_capture_two_ranges_and_the_merge(dev):
    import torch
    spec = plans.OP_BY_ID["split_chunks-D128-q8_0-q2h8kv4n1500"]
    case = ls.spec_case(spec, ls.shard_mask(2, 1500), tag="-capture")
    with fattn.options(dict(spec.opts)):
        sh = Shards(case.make(dev), [(0, 608), (608, 1500)], dev)
        eager, eager_lse = sh.run()
        g = capture(sh.launch)
        for _ in range(2):
            for t in (sh.outs, sh.lses, sh.dst, sh.lse):
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(sh.dst.cpu().numpy()), _bits(eager))
            assert np.array_equal(_bits(sh.lse.cpu().numpy()), _bits(eager_lse))
    ls.check_lse(eager_lse, case.lse_ref(), "capture lse_out")
    assert sh.guards_intact()


# ------------------------------------------------------------------ the harness

@pytest.mark.parametrize("args", [(), ("--mla", "--heads", "16", "--kv-size", "416", "--n-q", "2")], ids=["default", "mla"])
def test_kernel_test_harness(dev, args):
    r = run_kernel_test(["--lse", "--iters", "3"] + list(args))
    print(r.stdout[-800:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "lse max abs err" in r.stdout and "PASS" in r.stdout
