"""GPU: fattn_k_shift (the K-shift: RoPE of a K cache in place, every cache type).

How a case is checked (run_case): the view sits in the middle of a larger
random-filled allocation and the WHOLE allocation is compared.
  1. X = dequantize(cache) goes up as a contiguous F32 view and is shifted on the
     GPU to Y.  Y must lie within k_shift.tol() -- the derived bound -- of
     rotate_f64(X) elementwise, and every F32 byte outside the rewritten elements
     must be unchanged.
  2. The typed cache is shifted with the same arguments.  Its allocation must
     equal, bit for bit, the one before with encode(Y) in every rewritten block:
     the requantisation is isolated from the trig ulps (the rotation is one
     function for all types, so both launches requantise the same f32 y), and
     zero-shift rows, blocks at or past n_dims, padding, guards and other planes
     are compared as bytes."""
import functools

import numpy as np
import pytest

import fattn
import k_shift as ks
import set_rows as sr
from gpu_util import capture, check_bars, run_kernel_test, upload, views as gpu_views
from problems import make_problem

pytestmark = pytest.mark.gpu
TYPED = ("f16", "bf16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1")


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)


def _shift_view(d_shift, n_slots, ns):
    return fattn.View(d_shift.data_ptr(), fattn.TYPE_I32, (n_slots, ns, 1, 1), (4, 4 * n_slots, 4 * n_slots * ns, 4 * n_slots * ns))


def _launch(dev, alloc, off, nb, typ, ne, shift, rope, ff=None):
    """One fattn_k_shift over the view; returns the whole allocation afterwards."""
    import torch
    d_alloc, d_shift = _dev(alloc, dev), _dev(shift.reshape(-1), dev)
    d_ff = None if ff is None else _dev(np.asarray(ff, dtype=np.float32), dev)
    fattn.k_shift(fattn.View(d_alloc.data_ptr() + off, typ, ne, nb), _shift_view(d_shift, ne[1], shift.shape[0]), rope.c(), d_ff)
    torch.cuda.synchronize()
    return d_alloc.cpu().numpy()


def _assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


def f32_twin(dev, x, shift, rope, ff, what):
    """Step 1: x f32 [S][Hkv][n_slots][ne0] as an F32 cache ("head" layout, guards),
    shifted on the GPU and checked against rotate_f64 within tol(); returns Y."""
    s, hkv, n_slots, ne0 = x.shape
    ne = (ne0, n_slots, hkv, s)
    alloc, off, nb = ks.make_cache(ks.TYPE_F32, ne0, n_slots, hkv, s, "head", values=x)
    got = _launch(dev, alloc, off, nb, ks.TYPE_F32, ne, shift, rope, ff)
    mask = ks.rewritten_mask(len(alloc), off, nb, ks.TYPE_F32, ne, shift, rope.n_dims)
    assert mask.any()
    _assert_same(got[~mask], alloc[~mask], (what, "f32 bytes outside the rewritten elements"))
    y = ks.cache_values(got, off, nb, ks.TYPE_F32, ne)
    p = np.broadcast_to(ks.shift_planes(shift, s), x.shape[:3])
    want, t = ks.rotate_f64(x, p, rope, ff), ks.tol(x, p, rope, ff)
    want[p == 0], t[p == 0] = x[p == 0], 0.0                  # (p == 0 is "not touched": no factor m either)
    err = np.abs(y.astype(np.float64) - want)
    worst = float((err / np.maximum(t, 1e-300))[t > 0].max())
    print(f"KSHIFT {what}: max |err| {err.max():.3e}, worst err / tol {worst:.3f}")
    assert (err <= t).all(), (what, worst, float(err.max()))
    return y


def run_case(dev, name, alloc, off, nb, ne, shift, rope, ff=None, what=""):
    """Steps 1 and 2 of the module docstring; returns the typed allocation after the shift."""
    typ = ks.TYPES[name]
    x = ks.cache_values(alloc, off, nb, typ, ne)
    y = f32_twin(dev, x, shift, rope, ff, f"{what} {name} f32 twin")
    want = ks.apply_rows(alloc, off, nb, typ, ne, shift, rope.n_dims, y)
    got = _launch(dev, alloc, off, nb, typ, ne, shift, rope, ff)
    assert not np.array_equal(want, alloc)
    _assert_same(got, want, (what, name))
    return got


# ------------------------------------------------------------------ (a) the rotation, F32 k

@pytest.mark.parametrize("case", sorted(ks.ROTATION_CASES))
def test_rotation_f32(dev, case):
    """Every parameter set: both modes, ne0 64 / 128 / 256, n_dims = ne0, 64 and 80 of
    128 (a straddled block), freq_factors, YaRN, shifts of +-100000 -- within the
    derived tolerance of float64, 150 slots x 3 heads in a [N][Hkv][row] F32 cache."""
    ne0, rope, ff, big = ks.ROTATION_CASES[case]
    n_slots, hkv = 150, 3
    alloc, off, nb = ks.make_cache(ks.TYPE_F32, ne0, n_slots, hkv, 1, "pos", seed=21)
    run_case(dev, "f32", alloc, off, nb, (ne0, n_slots, hkv, 1), ks.make_shift(n_slots, 1, seed=3, big=big), rope, ff, case)


# ------------------------------------------------------------------ (b) untouched bytes, every type

@pytest.mark.parametrize("mode", ["norm", "neox"])
@pytest.mark.parametrize("name", ("f32",) + TYPED)
def test_untouched_bytes(dev, name, mode):
    """A single-head view (head 1 of 3) of a padded [Hkv][N][row] cache, n_dims 64 of
    128: rows with p == 0, blocks at or past n_dims, the padding behind every
    row, the guards and the other heads' planes keep their bytes."""
    typ = ks.TYPES[name]
    ne0, n_slots, hkv = 128, 37, 3
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, 1, "head", seed=23, row_pad=12)
    shift = ks.make_shift(n_slots, 1, seed=5)
    rope = ks.Rope(64, ks.NEOX if mode == "neox" else ks.NORMAL)
    one = (ne0, n_slots, 1, 1)
    off1 = off + nb[2]
    got = run_case(dev, name, alloc, off1, nb, one, shift, rope, what=f"untouched {mode}")
    mask = ks.rewritten_mask(len(alloc), off1, nb, typ, one, shift, 64)
    assert mask.sum() == np.count_nonzero(shift) * ks.rewritten_bytes(typ, 64)
    _assert_same(got[~mask], alloc[~mask], (name, mode))
    for h in (0, 2):                                           # the other heads' planes, as a whole
        o = off + h * nb[2]
        assert np.array_equal(got[o:o + nb[2]], alloc[o:o + nb[2]])
    assert np.count_nonzero(got[mask] != alloc[mask]) > mask.sum() // 4


# ------------------------------------------------------------------ (c) requantisation, bit for bit

@pytest.mark.parametrize("mode", ["norm", "neox"])
@pytest.mark.parametrize("name", TYPED)
def test_requantisation(dev, name, mode):
    """A real rotation of mixed shifts over encoded data (every edge block of
    tests/set_rows.py among it): the typed cache holds encode(Y) bit for bit."""
    typ = ks.TYPES[name]
    ne0, n_slots, hkv = 128, 96, 2
    vals = sr.source_rows(hkv * n_slots, ne0, seed=6).reshape(1, hkv, n_slots, ne0)
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, 1, "pos", seed=25, values=vals)
    rope = ks.Rope(128, ks.NEOX if mode == "neox" else ks.NORMAL)
    run_case(dev, name, alloc, off, nb, (ne0, n_slots, hkv, 1), ks.make_shift(n_slots, 1, seed=7), rope, what=f"requant {mode}")


@pytest.mark.parametrize("name", TYPED)
def test_requantisation_tie_rules(dev, name):
    """The tie rules of quantize_row_*_ref: rows of raw codes (block types; their
    dequantised values tie for the largest |x| with opposite signs, and repeat
    their minima / maxima) and the encoded tie_blocks() rows, half of them with a
    shift of 0 -- untouched -- and the others under an EXACT rotation: p = 1 with
    freq_scale = 2^-100, so cos = 1 and |x sin| is far below half an ulp of any
    non-zero element: y == x there and every tie survives into the
    requantisation, which must reproduce encode(Y)."""
    typ = ks.TYPES[name]
    ne0, n_slots, hkv = 128, 44, 1
    vals = sr.source_rows(n_slots, ne0, seed=8).reshape(1, 1, n_slots, ne0)     # rows 0 .. 4: the 17 edge blocks
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, 1, "pos", seed=27, values=vals)
    ne = (ne0, n_slots, hkv, 1)
    if ks.is_block(typ):
        ks.rows_view(alloc, off, nb, typ, ne)[0, 0, 8:] = ks.raw_code_rows(typ, n_slots - 8, ne0)
    shift = np.ones((1, n_slots), dtype=np.int32)
    shift[0, 5::2] = 0                                         # (the edge-block rows 0 .. 4 all rotate)
    rope = ks.Rope(128, ks.NEOX, freq_scale=2.0 ** -100)
    got = run_case(dev, name, alloc, off, nb, ne, shift, rope, what="ties")
    if typ in ks.ELEM_BYTES:                                   # F16 / BF16: the exact rotation is the identity on non-zero values
        x, y = ks.cache_values(alloc, off, nb, typ, ne), ks.cache_values(got, off, nb, typ, ne)
        assert np.array_equal(y[x != 0], x[x != 0])


# ------------------------------------------------------------------ (d) layouts

@pytest.mark.parametrize("layout,row_pad", [("pos", 0), ("head", 0), ("head", 20)])
@pytest.mark.parametrize("name", ["f16", "q8_0", "q5_0", "q4_1"])
def test_layouts(dev, name, layout, row_pad):
    """[N][Hkv][row], [Hkv][N][row] and padded rows (20 bytes: no row base is 8-byte aligned), 8 heads, 53 slots."""
    typ = ks.TYPES[name]
    ne0, n_slots, hkv = 128, 53, 8
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, 1, layout, seed=29, row_pad=row_pad)
    run_case(dev, name, alloc, off, nb, (ne0, n_slots, hkv, 1), ks.make_shift(n_slots, 1, seed=9), ks.Rope(128, ks.NEOX),
             what=f"layout {layout}+{row_pad}")


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("name", ["bf16", "q4_0", "q5_1"])
def test_sequences(dev, name, ns):
    """S = 2: one shift plane for both sequences, and one each."""
    typ = ks.TYPES[name]
    ne0, n_slots, hkv, s = 128, 41, 2, 2
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, s, "pos", seed=31)
    shift = ks.make_shift(n_slots, ns, seed=11)
    if ns == 2:
        assert not np.array_equal(shift[0], shift[1])
    run_case(dev, name, alloc, off, nb, (ne0, n_slots, hkv, s), shift, ks.Rope(128, ks.NORMAL), what=f"S=2 ns={ns}")


@pytest.mark.parametrize("name,rb", [("f16", 1152), ("q8_0", 612)])
def test_mla_view(dev, name, rb):
    """The 64 RoPE dims of an MLA cache row (llama.cpp's order: they come first):
    ne0 = 64 over 576-element rows; the 512 latent dims keep their bytes."""
    typ = ks.TYPES[name]
    n_slots = 70
    full, off, nb = ks.make_cache(typ, 576, n_slots, 1, 1, "pos", seed=33)
    assert nb[1] == rb
    ne = (64, n_slots, 1, 1)
    shift = ks.make_shift(n_slots, 1, seed=13)
    _, rope, _, _ = ks.ROTATION_CASES["neox-64-mla"]
    got = run_case(dev, name, full, off, nb, ne, shift, rope, what="mla")
    lat = ks.row_bytes(typ, 64)
    rows_got = ks.rows_view(got, off, nb, typ, (576, n_slots, 1, 1))
    rows_was = ks.rows_view(full, off, nb, typ, (576, n_slots, 1, 1))
    assert np.array_equal(rows_got[..., lat:], rows_was[..., lat:])
    assert not np.array_equal(rows_got[..., :lat], rows_was[..., :lat])


@pytest.mark.parametrize("name", ["q8_0", "f16", "q5_1"])
@pytest.mark.parametrize("ne0,n_slots", [(256, 37), (128, 39), (64, 43), (96, 39), (32, 300)])
def test_rows_per_wave(dev, name, ne0, n_slots):
    """1, 2 and 4 rows per wave (ne0 256 / 128 / 64), two rows of three blocks with
    two idle lane groups (96), eight one-block rows (32); the last wave is
    part-filled every time (one row per wave: the last workgroup)."""
    typ = ks.TYPES[name]
    rpw = 8 // ((ne0 + 31) // 32)
    assert n_slots % rpw if rpw > 1 else n_slots % 4
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, 2, 1, "pos", seed=35)
    n_dims = ne0 if ne0 != 96 else 64
    run_case(dev, name, alloc, off, nb, (ne0, n_slots, 2, 1), ks.make_shift(n_slots, 1, seed=15), ks.Rope(n_dims, ks.NEOX),
             what=f"ne0={ne0}")


def test_elem_rows_of_partial_blocks(dev):
    """F32 / F16 / BF16 rows need no whole blocks: ne0 = 80 (the third block is half
    there) with n_dims 80 and 72."""
    for name in ("f32", "f16", "bf16"):
        typ = ks.TYPES[name]
        for n_dims, mode in ((80, ks.NEOX), (72, ks.NORMAL), (72, ks.NEOX)):
            alloc, off, nb = ks.make_cache(typ, 80, 45, 2, 1, "head", seed=37)
            run_case(dev, name, alloc, off, nb, (80, 45, 2, 1), ks.make_shift(45, 1, seed=17), ks.Rope(n_dims, mode),
                     what=f"ne0=80 n_dims={n_dims}")


def test_head_walk_and_head_grid_agree(dev):
    """Enough slots that one lane group walks all the heads with one set of angles
    (the launch fills the chip without spreading them over the grid): 8 heads of
    ne0 = 32 over 66000 slots, Q8_0; the same cache seen as 8 sequences of one
    head takes the other form and must write the same bytes."""
    import torch
    typ, ne0, n_slots, hkv = ks.TYPES["q8_0"], 32, 66000, 8
    rng = np.random.default_rng(39)
    vals = (3.0 * (1.0 - 2.0 * rng.random((1, hkv, n_slots, ne0), dtype=np.float32))).astype(np.float32)
    rows = ks.encode(vals, typ)                               # [1][Hkv][N][34]
    shift = ks.make_shift(n_slots, 1, seed=19)
    rb = 34
    nb = (34, rb, rb * n_slots, rb * n_slots * hkv)
    d_shift = _dev(shift.reshape(-1), dev)
    outs = []
    for ne, nbv in (((ne0, n_slots, hkv, 1), nb), ((ne0, n_slots, 1, hkv), (34, rb, rb * n_slots * hkv, rb * n_slots))):
        d = _dev(rows.reshape(-1), dev)
        fattn.k_shift(fattn.View(d.data_ptr(), typ, ne, nbv), _shift_view(d_shift, n_slots, 1), ks.Rope(32, ks.NEOX).c())
        torch.cuda.synchronize()
        outs.append(d.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    # and both are the shift: a sample of slots against the small-case machinery
    sl = slice(0, 64)
    sub = np.ascontiguousarray(rows[:, :, sl])
    sub_alloc = sub.reshape(-1)
    sub_nb = (34, rb, rb * 64, rb * 64 * hkv)
    want = run_case(dev, "q8_0", sub_alloc, 0, sub_nb, (ne0, 64, hkv, 1), shift[:, sl], ks.Rope(32, ks.NEOX), what="walk sample")
    got = outs[0].reshape(1, hkv, n_slots, rb)[:, :, sl].reshape(-1)
    _assert_same(got, want, "walk sample")


# ------------------------------------------------------------------ (e) a captured launch

@pytest.mark.parametrize("name", ["q5_1", "f16"])
def test_graph_replay_reads_new_shifts(dev, name):
    """One k_shift captured on a side stream; the shift tensor is then overwritten
    in place and the graph replayed: the cache moves by the NEW deltas (they are
    data, not launch arguments)."""
    import torch
    typ = ks.TYPES[name]
    ne0, n_slots, hkv = 128, 40, 2
    ne = (ne0, n_slots, hkv, 1)
    rope = ks.Rope(128, ks.NEOX)
    alloc, off, nb = ks.make_cache(typ, ne0, n_slots, hkv, 1, "pos", seed=41)
    sa, sb = ks.make_shift(n_slots, 1, seed=1), ks.make_shift(n_slots, 1, seed=2)
    assert not np.array_equal(sa, sb)
    d_alloc, d_shift = _dev(alloc, dev), _dev(sa.reshape(-1), dev)
    kv, sv, rp = fattn.View(d_alloc.data_ptr() + off, typ, ne, nb), _shift_view(d_shift, n_slots, 1), rope.c()
    g = capture(lambda stream: fattn.k_shift(kv, sv, rp, None, stream))
    after_a = d_alloc.cpu().numpy()                            # (capturing launched nothing: the eager launch's shift)
    _assert_same(after_a, run_case(dev, name, alloc, off, nb, ne, sa, rope, what="eager"), "eager")
    d_shift.copy_(_dev(sb.reshape(-1), dev))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_same(d_alloc.cpu().numpy(), run_case(dev, name, after_a, off, nb, ne, sb, rope, what="replay"), "replay")


# ------------------------------------------------------------------ (f) end to end

@functools.lru_cache(maxsize=None)
def _e2e_problem(name):
    return make_problem(D=128, NQ=1, H=4, Hkv=2, N=160, kv_type=name, seed=43)


@pytest.mark.parametrize("name", ["f16", "q8_0"])
def test_end_to_end(dev, name):
    """D = 128, N = 160: k_shift on the GPU, then fattn_ext over the shifted cache,
    against the frozen oracle over the numpy-shifted cache (k_shift_ref) -- the
    project's bars."""
    import dataclasses
    import torch
    p = _e2e_problem(name)
    shift = ks.make_shift(p.N, 1, seed=21)
    rope = ks.Rope(128, ks.NEOX)
    t = upload(p, dev)
    qv, kv, vv, mv = gpu_views(p, t)
    d_shift = _dev(shift.reshape(-1), dev)
    fattn.k_shift(kv, _shift_view(d_shift, p.N, 1), rope.c())
    att = fattn.Attention(qv, kv, vv, mv, t["dst"], p.scale)
    att()
    torch.cuda.synchronize()
    got = t["dst"].cpu().numpy()
    k_ref = ks.k_shift_ref(p.k_bytes, 0, p.k_nb, p.kv_type, p.kv_ne, shift, rope)
    assert not np.array_equal(k_ref, p.k_bytes)
    ref = dataclasses.replace(p, k_bytes=k_ref).oracle()
    unshifted = p.oracle()
    check_bars(got, ref, lambda rel, elem: f"KSHIFT e2e {name} rel={rel:.3e} elem={elem:.3f} | {att.describe()}")
    assert np.abs(ref - unshifted).max() > 1e-3               # (the shift matters to the output)


# ------------------------------------------------------------------ (g) the harness

@pytest.mark.parametrize("kv_type,mode", [("q8_0", "neox"), ("q5_1", "norm")])
def test_harness_k_shift(kv_type, mode):
    """kernel_test --k-shift: the cache shifted by fattn_k_shift, the host's own shift and reference; its max-diff check."""
    r = run_kernel_test(["--iters", "3", "--k-shift", "-256", "--kv-type", kv_type, "--rope-mode", mode, "--heads", "8",
                         "--kv-heads", "4", "--kv-size", "512"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and "k-shift" in r.stdout
