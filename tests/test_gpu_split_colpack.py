"""GPU: the column-packed V scales of the split kernel's one-row tiles
(fattn_split.h, col_packed: Q8_0 / Q4_0 V under the one-row epilogues).

On a one-row tile columns 0 .. D/32 - 1 of the 16 MFMA columns all carry the
tile's query row and column b folds the scales of V block b alone; block b's
dims are then read from column b in the magic-offset correction, the per-wave
publish (wave_merge_epilogue: 4 waves, D = 128, several chunks) and the LDS
merge (wg_row_merge: every other one-row plan, with its direct store into dst
when the tile has one chunk).  A miss at any of these is silent wrong output
for a quarter (or more) of a row, so every case asserts from describe() that
the intended kernel, wave count and chunk count ran -- nothing skips -- and is
held to the suite's bars against the CPU oracle: attn_rel_err <= RTOL and
attn_elem_err <= 1, NaN positions coinciding.  max_bias / logit_softcap and
sinks, which the frozen oracle does not have, go against the assembled
references of tests/op_params.py and tests/sinks.py, at the same bars.

Shapes: one query row, H = Hkv = 4, N <= 1024 -- N = 1024 is 8 chunks of 4
waves, 4 of 8, 2 of 16; N = 256 on 8 waves is one chunk.  N = 100 and 257 end a
slice in a partial step; a quantised cache of such an N plans the
dword-granular kernels (4 waves; not at D = 96, whose rows are no whole number
of dwords), so these cases cover those bodies too.  Quantised rows are whole blocks
of 32, so D = 80 exists as f16 only: its case shows that path unchanged.  The
GQA case (4 packed rows per tile) runs the multi-row epilogue, which is not
column-packed.
"""
import numpy as np
import pytest

import fattn
import op_params as op
import sinks as sk
import views
from gpu_util import check_bars, upload
from gpu_util import views as tensor_views
from problems import attn_elem_err, attn_rel_err, make_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-3

W, STEPS, LOADERS = fattn.OPT_SPLIT_WAVES, fattn.OPT_SPLIT_STEPS, fattn.OPT_SPLIT_LOADERS


def case(id, want, chunks, opts=None, **prob):
    """want: substrings of describe(); chunks: grid x (the tile's chunk count)."""
    prob = dict(dict(D=128, NQ=1, H=4, N=1024, kv_type="q8_0"), **prob)
    return pytest.param(prob, dict(opts or {}), (want,) if isinstance(want, str) else tuple(want), chunks, id=id)


def split(kt, vt, D, gran, mask, waves):
    return f"fattn_split_kernel<{kt},{vt},D{D},gran{gran},{mask},{waves}waves>"


def _cases():
    out = []
    # every head dim x type on the default plan (4 waves, 8 chunks: the per-wave publish at D = 128,
    # the LDS merge elsewhere) and on 8 and 16 waves (the LDS merge; D = 256 has no 16-wave body)
    for t in ("q8_0", "q4_0"):
        for D in (64, 96, 128, 256):
            out.append(case(f"{t}-D{D}-w4", split(t, t, D, 16, "mask", 4), 8, D=D, kv_type=t))
            out.append(case(f"{t}-D{D}-w8", split(t, t, D, 16, "mask", 8), 4, {W: 8}, D=D, kv_type=t))
            if D != 256:
                out.append(case(f"{t}-D{D}-w16", split(t, t, D, 16, "mask", 16), 2, {W: 16}, D=D, kv_type=t))
        # two steps per wave (two in flight): the rescale of o, l and corr between a wave's steps
        out.append(case(f"{t}-D128-w4-2steps", split(t, t, 128, 16, "mask", 4), 4, {STEPS: 2}, kv_type=t))
        # one chunk: wg_row_merge's direct store into dst
        out.append(case(f"{t}-one-chunk-w8", split(t, t, 128, 16, "mask", 8), 1, {W: 8}, N=256, kv_type=t))
        out.append(case(f"{t}-one-chunk-w16", split(t, t, 128, 16, "mask", 16), 1, {W: 16}, N=512, kv_type=t))
        # a slice ending in a partial step: N = 257 is 3 chunks, the last of one position; N = 100 one
        # chunk (4 waves, one chunk: the multi-row epilogue, not packed) whose wave 3 has 4 positions
        for D in (64, 128, 256):
            for mk in ("random", "none"):
                hm = "nomask" if mk == "none" else "mask"
                out.append(case(f"{t}-D{D}-N257-{hm}", split(t, t, D, 4, hm, 4), 3, D=D, N=257, kv_type=t, mask=mk))
        out.append(case(f"{t}-N100", split(t, t, 128, 4, "mask", 4), 1, N=100, kv_type=t))
        # hard inputs: many rescales of the running max (every rescale scales the one corr too)
        for w, ch in ((4, 8), (8, 4)):
            out.append(case(f"{t}-extreme-w{w}", split(t, t, 128, 16, "mask", w), ch, {W: w}, kv_type=t, extreme=True))
            out.append(case(f"{t}-ramp12-w{w}", split(t, t, 128, 16, "mask", w), ch, {W: w}, kv_type=t, ramp=12))
    # mixed K / V types: a quantised V is packed whatever K is; an f16 V is not
    for w, ch in ((4, 8), (8, 4)):
        out.append(case(f"k-f16-v-q8_0-w{w}", split("f16", "q8_0", 128, 16, "mask", w), ch, {W: w}, kv_type="f16",
                        v_type="q8_0"))
        out.append(case(f"k-q8_0-v-f16-w{w}", split("q8_0", "f16", 128, 16, "mask", w), ch, {W: w}, kv_type="q8_0",
                        v_type="f16"))
    # mask variants on both one-row epilogues
    for mk in ("none", "neginf_blocks", "tail"):
        hm = "nomask" if mk == "none" else "mask"
        out.append(case(f"mask-{mk}-w4", split("q8_0", "q8_0", 128, 16, hm, 4), 8, mask=mk))
        out.append(case(f"mask-{mk}-w8", split("q8_0", "q8_0", 128, 16, hm, 8), 4, {W: 8}, mask=mk))
        out.append(case(f"mask-{mk}-q4_0-D64", split("q4_0", "q4_0", 64, 16, hm, 4), 8, D=64, kv_type="q4_0", mask=mk))
    # D = 80: f16 rows only (not a whole number of ggml blocks) -- the unpacked path, unchanged
    out.append(case("f16-D80", split("f16", "f16", 80, 16, "mask", 4), 8, D=80, kv_type="f16"))
    # GQA: 4 packed rows per tile, the multi-row epilogue and its merge launch (not column-packed)
    out.append(case("gqa-H8-Hkv2", (split("q8_0", "q8_0", 128, 16, "mask", 4), "fattn_merge_kernel"), 8, H=8, Hkv=2))
    return out


def _launch(prob, opts, want, chunks, dev, seed=71, launches=1):
    p = make_problem(seed=seed, **prob)
    with fattn.options(opts):
        t = upload(p, dev)
        att = fattn.Attention(*tensor_views(p, t), t["dst"], p.scale)
        d = att.describe()
        for w in want:
            assert w in d, (w, d)
        assert f" grid({chunks}," in d, d
        outs = []
        for _ in range(launches):
            t["dst"].fill_(float("nan"))
            att()
            outs.append(t["dst"].cpu().numpy())
    return p, d, outs


def _check(tag, d, got, ref):
    check_bars(got, ref, lambda e_or, e_el: f"COLPACK {tag}: rel {e_or:.3e} elem {e_el:.3f} | {d.split(' lds ')[0]}")


@pytest.mark.parametrize("prob,opts,want,chunks", _cases())
def test_colpack_against_oracle(dev, request, prob, opts, want, chunks):
    p, d, (got,) = _launch(prob, opts, want, chunks, dev)
    _check(request.node.callspec.id, d, got, p.oracle())


@pytest.mark.parametrize("t,opts,waves,chunks", [("q8_0", {}, 4, 8), ("q8_0", {W: 8}, 8, 4), ("q4_0", {W: 16}, 16, 2),
                                                 ("q4_0", {W: 8}, 8, 1)])
def test_fully_masked_row_is_nan(dev, t, opts, waves, chunks):
    """Every key of the row at -inf: l = 0 on every part, the row is NaN as in the reference."""
    prob = dict(D=128, NQ=1, H=4, N=256 if chunks == 1 else 1024, kv_type=t)
    p = make_problem(seed=72, **prob)
    p.mask_bits[:] = 0xFC00  # f16 -inf
    with fattn.options(opts):
        tt = upload(p, dev)
        att = fattn.Attention(*tensor_views(p, tt), tt["dst"], p.scale)
        d = att.describe()
        assert split(t, t, 128, 16, "mask", waves) in d and f" grid({chunks}," in d, d
        tt["dst"].fill_(0.0)
        att()
        got = tt["dst"].cpu().numpy()
    ref = p.oracle()
    assert np.isnan(ref).all()
    assert np.isnan(got).all(), d
    assert attn_rel_err(got, ref) <= RTOL and attn_elem_err(got, ref) <= 1.0


@pytest.mark.parametrize("t,D,opts,waves,chunks", [("q8_0", 128, {}, 4, 8), ("q8_0", 128, {W: 8}, 8, 4),
                                                   ("q4_0", 64, {W: 16}, 16, 2), ("q4_0", 256, {}, 4, 8)])
def test_repeated_launches_equal_bits(dev, t, D, opts, waves, chunks):
    """Three launches on one workspace (the arrival words re-arm): the same bits, and the oracle's row."""
    prob = dict(D=D, NQ=1, H=4, N=1024, kv_type=t)
    p, d, outs = _launch(prob, opts, (split(t, t, D, 16, "mask", waves),), chunks, dev, seed=73, launches=3)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), d
    _check(f"repeat-{t}-D{D}-w{waves}", d, outs[2], p.oracle())


@pytest.mark.parametrize("t,D", [("q8_0", 128), ("q4_0", 128), ("q8_0", 64), ("q4_0", 64)])
def test_loader_waves_equal_the_8_wave_form(dev, t, D):
    """fattn_split_ld_kernel shares split_step and wg_row_merge: with the same chunks (two steps per
    wave) its rows equal the 8-wave split kernel's bit for bit, over three launches on one workspace."""
    prob = dict(D=D, NQ=1, H=4, N=1024, kv_type=t)
    p, d8, (base,) = _launch(prob, {W: 8, STEPS: 2}, (split(t, t, D, 16, "mask", 8),), 2, dev, seed=74)
    want = f"fattn_split_ld_kernel<{t},{t},D{D},gran16,mask,8waves+4loaders>"
    _, dl, outs = _launch(prob, {W: 8, STEPS: 2, LOADERS: 2}, (want,), 2, dev, seed=74, launches=3)
    for got in outs:
        assert np.array_equal(got, base), (d8, dl)
    _check(f"loaders-{t}-D{D}", dl, outs[2], p.oracle())


# ---- max_bias / logit_softcap / sinks (references: tests/op_params.py, tests/sinks.py)
_XF = {"alibi": dict(max_bias=8.0), "softcap": dict(logit_softcap=4.0)}


def _op_problem(t, seed, **kw):
    p = make_problem(D=128, NQ=1, H=4, N=1024, kv_type=t, mask="none", seed=seed)
    return op.one_plane(p, op.random_mask(1, 1024, seed), **kw)


@pytest.mark.parametrize("t", ["q8_0", "q4_0"])
@pytest.mark.parametrize("xf", sorted(_XF))
def test_score_transforms(dev, t, xf):
    """max_bias (every column of the packed row takes the row's head's slope) and logit_softcap: the
    4-wave bodies with the score transform, 8 chunks (the per-wave publish)."""
    o = _op_problem(t, 75, **_XF[xf])
    g = views.GpuView(o, dev)
    d = g.describe()
    assert split(t, t, 128, 16, "mask", 4) in d and " grid(8," in d and xf in d, d
    got = g.run()
    assert g.guards_intact(), d
    _check(f"{xf}-{t}", d, got, o.reference())


@pytest.mark.parametrize("t,opts,waves,chunks", [("q8_0", {}, 4, 8), ("q4_0", {W: 8}, 8, 4), ("q8_0", {W: 8}, 8, 1)])
def test_sinks(dev, t, opts, waves, chunks):
    """Sinks join the row where it is normalised: the per-wave merge, the chunk merge behind the LDS
    merge, and the LDS merge's direct store (one chunk)."""
    N = 256 if chunks == 1 else 1024
    p = make_problem(D=128, NQ=1, H=4, N=N, kv_type=t, mask="none", seed=76)
    sinks = (np.log(np.float64(N)) + np.array([1.0, -2.0, 3.0, 0.0])).astype(np.float32)
    sp = sk.with_sinks(op.one_plane(p, op.random_mask(1, N, 76)), sinks)
    with fattn.options(opts):
        g = sk.SinkGpuView(sp, dev)
        d = g.describe()
        assert split(t, t, 128, 16, "mask", waves) in d and f" grid({chunks}," in d, d
        got = g.run()
    assert g.guards_intact(), d
    _check(f"sinks-{t}-w{waves}-c{chunks}", d, got, sp.reference())
