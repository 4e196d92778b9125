"""GPU: the IQ4_NL KV-cache type.  Conversions and cache writes bit-exact against tests/iq4_nl.py; attention on
every plan of the type against the frozen oracle over F16 views of the dequantised cache (kv_types.reference_pair)
at the project's bars (1e-3 / 1), the shapes of tests/test_gpu_kv_types.py; the K-shift as test_gpu_k_shift.py's."""
import numpy as np
import pytest

import fattn
import iq4_nl as iq
import k_shift as ks
import kv_types as kt
import op_params as op
import sinks as sk
import views
from gpu_util import run_described, run_kernel_test
from test_gpu_k_shift import _launch as k_shift_launch, f32_twin

pytestmark = pytest.mark.gpu
NAME, T = iq.NAME, iq.TYPE_IQ4_NL


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_quantize_dequantize_bit_exact(dev):
    x = kt.conv_input(iq.KVT)
    want = iq.quantize(x)
    got = fattn.quantize(_dev(x, dev), T).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert got[65, 54:].tobytes().hex() == iq.KAT_HEX
    y = fattn.dequantize(_dev(want, dev), T, 128).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), iq.dequantize(want, 128).view(np.uint32))


def test_cpy_and_set_rows_into_pos_cache_view(dev):
    """22 tokens x 3 heads into a [N][Hkv][row] view from slot 7 on by both ops: numpy's bytes, every other byte untouched;
    set_rows' token 5 carries slot N and writes nothing."""
    import torch
    D, Hkv, N, p0 = 128, 3, 80, 7
    rb = fattn.row_size(T, D)
    cur = kt.conv_input(iq.KVT).reshape(-1, Hkv, D)
    ntok = len(cur)
    rows = iq.quantize(cur)
    cache0 = np.random.default_rng(3).integers(0, 256, size=N * Hkv * rb, dtype=np.uint8)
    slots = np.arange(p0, p0 + ntok, dtype=np.int64)
    slots[5] = N
    src, idx = _dev(cur, dev), _dev(slots, dev)
    for by_slot in (False, True):
        cache = _dev(cache0.copy(), dev)
        if by_slot:
            sv = fattn.View(src.data_ptr(), fattn.TYPE_F32, (D, ntok, Hkv, 1), (4, Hkv * D * 4, D * 4, ntok * Hkv * D * 4))
            dv = fattn.View(cache.data_ptr(), T, (D, N, Hkv, 1), (18, Hkv * rb, rb, N * Hkv * rb))
            fattn.set_rows(sv, fattn.View(idx.data_ptr(), fattn.TYPE_I64, (ntok, 1, 1, 1), (8, 8 * ntok, 8 * ntok, 8 * ntok)), dv)
        else:
            sv = fattn.View(src.data_ptr(), fattn.TYPE_F32, (D, Hkv, ntok, 1), (4, D * 4, Hkv * D * 4, ntok * Hkv * D * 4))
            dv = fattn.View(cache.data_ptr() + p0 * Hkv * rb, T, (D, Hkv, ntok, 1), (18, rb, Hkv * rb, N * Hkv * rb))
            fattn.cpy(sv, dv)
        torch.cuda.synchronize()
        want = cache0.copy().reshape(N, Hkv, rb)
        want[p0:p0 + ntok] = rows
        if by_slot:
            want[p0 + 5] = cache0.reshape(N, Hkv, rb)[p0 + 5]
        assert np.array_equal(cache.cpu().numpy().reshape(N, Hkv, rb), want), by_slot


W8 = {fattn.OPT_SPLIT_WAVES: 8}
# (id, describe() prefix after the types, kv_chunk, options, layout, what else describe() shows, the problem)
SPLIT = [(f"one_row-D{D}-{m}", f"D{D},gran16,{'nomask' if m == 'none' else 'mask'},4waves>", 128, {}, "head", "grid(5,4,1)",
          dict(D=D, NQ=1, H=4, N=544, mask=m, seed=21 + D)) for D in (64, 128, 256) for m in ("none", "random", "tail")]
SPLIT += [(f"one_row_8w-D{D}", f"D{D},gran16,mask,8waves>", 256, W8, "head", "grid(4,4,1)",
           dict(D=D, NQ=1, H=4, N=1024, mask="random", seed=17)) for D in (64, 128)]
SPLIT += [(f"{lay}-D{D}-N{N}", f"D{D},gran4,mask,4waves>", 0, {}, lay, "", dict(D=D, NQ=1, H=4, N=N, mask="random", seed=5 + N))
          for D in (64, 128, 256) for lay, N in (("pos", 77), ("padded", 96))]
SPLIT += [(f"gqa-D{D}", f"D{D},gran16,mask,", 0, {}, "head", "", dict(D=D, NQ=3, H=8, Hkv=2, N=288, S=2, Skv=1, mask="random", seed=9))
          for D in (64, 128, 256)]
SPLIT += [(f"merge_launch-{w or 4}w", f"D128,gran16,mask,{w or 4}waves> + fattn_merge_kernel", 256, {fattn.OPT_SPLIT_WAVES: w}, "head",
           "grid(8,2,1)", dict(D=128, NQ=1, H=8, Hkv=2, N=2048, mask="random", seed=13)) for w in (0, 8)]


@pytest.mark.parametrize("tag,prefix,kv_chunk,opts,layout,also,kw", SPLIT, ids=[c[0] for c in SPLIT])
def test_split_kernel(dev, tag, prefix, kv_chunk, opts, layout, also, kw):
    gpu, _, oracle, _ = kt.cached_pair(NAME, layout=layout, **kw)
    with fattn.options(opts):
        got, desc = run_described(gpu, dev, kv_chunk=kv_chunk)
    assert desc.startswith(f"fattn_split_kernel<{NAME},{NAME},{prefix}") and also in desc, desc
    kt.check(NAME, tag, desc, got, oracle)


@pytest.mark.parametrize("form", ["softcap", "alibi+sinks"])
def test_score_transform_body(dev, form):
    gpu, ref = kt.reference_pair(NAME, D=128, NQ=2, H=4, Hkv=2, N=544, mask="none", seed=31)
    sinks = None
    if form == "softcap":
        o = op.one_plane(ref, op.random_mask(2, 544, 1), logit_softcap=12.0)
        want = op.reference(o)
    else:
        o = sk.with_sinks(op.one_plane(ref, op.distance_mask(2, 544) / np.float32(64.0), max_bias=8.0),
                          np.array([0.5, -1.0, 2.0, -np.inf], dtype=np.float32))
        want, sinks = sk.reference(o), o.sinks
    gv = views.GpuView(views.swap_kv(o, gpu), dev, 128, sinks=sinks)
    desc = gv.describe()
    got = gv.run()
    assert gv.guards_intact(), desc
    assert desc.startswith(f"fattn_split_kernel<{NAME},{NAME},D128,gran16,mask,4waves>") and ("softcap 12" if sinks is None else "alibi 8") in desc, desc
    kt.check(NAME, form, desc, got, want)


@pytest.mark.parametrize("mask", ["causal", "zero"])
@pytest.mark.parametrize("D", [128, 64])
def test_prefill_staged(dev, D, mask):
    gpu, _, oracle, _ = kt.cached_pair(NAME, D=D, NQ=256, H=2, N=192, mask=mask, seed=41)
    with fattn.options({fattn.OPT_PF: 2}):
        got, desc = run_described(gpu, dev)
    assert f"kv_stage_f16<{NAME}>" in desc and f"<f16,D{D}" in desc, desc
    kt.check(NAME, f"prefill D{D} {mask}", desc, got, oracle)


@pytest.mark.parametrize("mode", ["neox", "norm"])
def test_k_shift(dev, mode):
    """A [Hkv][N][row] K cache, ne0 = 128, 8 heads, 53 slots, between guard bytes (NORMAL: n_dims = 64, blocks 2 and 3
    keep their bytes): the whole allocation equals the one before with quantize(Y) in the rotated blocks of the shifted rows."""
    ne0, n_slots, hkv = 128, 53, 8
    rng = np.random.default_rng(29)
    rows = iq.quantize((3.0 * (1.0 - 2.0 * rng.random((1, hkv, n_slots, ne0), dtype=np.float32))).astype(np.float32))
    guard = rng.integers(0, 256, size=64, dtype=np.uint8)
    alloc = np.concatenate([guard, rows.reshape(-1), guard])
    shift = ks.make_shift(n_slots, 1, seed=9)
    rope = ks.Rope(128, ks.NEOX) if mode == "neox" else ks.Rope(64, ks.NORMAL)
    y = f32_twin(dev, iq.dequantize(rows, ne0), shift, rope, None, f"iq4_nl {mode} f32 twin")
    want_rows = np.where((shift[0] != 0)[None, None, :, None] & (np.arange(72) < rope.n_dims // 32 * 18), iq.quantize(y), rows)
    assert (shift[0] == 0).any() and not np.array_equal(want_rows, rows)
    got = k_shift_launch(dev, alloc, 64, (18, 72, n_slots * 72, hkv * n_slots * 72), T, (ne0, n_slots, hkv, 1), shift, rope)
    assert np.array_equal(got, np.concatenate([guard, want_rows.reshape(-1), guard]))


def test_harness_kv_type(dev):
    r = run_kernel_test(["--iters", "3", "--no-kv-parallel", "--kv-type", NAME])
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
