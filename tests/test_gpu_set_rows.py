"""GPU: fattn_set_rows (GGML_OP_SET_ROWS, the KV-cache write by slot index),
bit-exact against tests/set_rows.set_rows_ref.

In every case dst is a view into the middle of a larger random-filled
allocation (at least one slot's bytes of guard around every plane) and the
WHOLE allocation is compared: a missing bounds check, a truncated index or a
store past a row shows as changed guard bytes or a changed slot."""
import functools

import numpy as np
import pytest

import fattn
import set_rows as sr
from gpu_util import capture, run_kernel_test, upload, views as gpu_views
from oracle import oracle as orc
from problems import Problem, attn_elem_err, attn_rel_err

pytestmark = pytest.mark.gpu
ALL = ("f16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1")
IDX = {"i64": sr.TYPE_I64, "i32": sr.TYPE_I32}


@functools.lru_cache(maxsize=None)
def _src(ne3, ne2, nr, ne0, seed=5):
    x = sr.source_rows(ne3 * ne2 * nr, ne0, seed).reshape(ne3, ne2, nr, ne0)
    x.setflags(write=False)
    return x


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)     # (a copy: the shared sources are read-only)


def _launch(dev, typ, ityp, src, idx, n_slots, layout, *, token_major=False, base_off=0, row_pad=0, stride0=1):
    """Run one fattn_set_rows; returns (got, want, untouched): the whole
    allocation after the launch, what set_rows_ref says it must be, and the
    allocation before."""
    import torch
    ne3, ne2, nr, ne0 = src.shape
    cache, off, nb = sr.cache_alloc(typ, ne0, n_slots, ne2, ne3, layout)
    want = sr.set_rows_ref(cache, src, idx, typ, n_slots, off, nb)
    sflat, soff, snb = sr.place_src(src, token_major=token_major, base_off=base_off, row_pad=row_pad)
    iflat, ine, inb = sr.place_idx(idx, ityp, stride0)
    d_cache, d_src, d_idx = _dev(cache, dev), _dev(sflat, dev), _dev(iflat, dev)
    sv = fattn.View(d_src.data_ptr() + soff, fattn.TYPE_F32, (ne0, nr, ne2, ne3), snb)
    iv = fattn.View(d_idx.data_ptr(), ityp, ine, inb)
    dv = fattn.View(d_cache.data_ptr() + off, typ, (ne0, n_slots, ne2, ne3), nb)
    fattn.set_rows(sv, iv, dv)
    torch.cuda.synchronize()
    return d_cache.cpu().numpy(), want, cache


def _assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("iname", ["i64", "i32"])
@pytest.mark.parametrize("name", ALL)
def test_every_type_broadcast_index(dev, name, iname):
    """ne0 = 128, 22 rows x 3 heads (every edge block, then random rows) into an
    80-slot [N][Hkv][row] cache; one index row for all heads."""
    src = _src(1, 3, 22, 128)
    idx = sr.permuted_slots(80, (1, 1, 22))
    got, want, before = _launch(dev, sr.TYPES[name], IDX[iname], src, idx, 80, "pos")
    assert not np.array_equal(want, before)
    _assert_same(got, want, (name, iname))


@pytest.mark.parametrize("iname", ["i64", "i32"])
@pytest.mark.parametrize("name", ["q8_0", "q4_1", "f16"])
def test_per_head_indices(dev, name, iname):
    """idx.ne = [22, 3, 1]: other slots per head, indices two elements apart,
    a [Hkv][N][row] cache, the source token-major as llama.cpp's k_cur."""
    src = _src(1, 3, 22, 128)
    idx = sr.permuted_slots(80, (1, 3, 22), seed=4)
    assert not np.array_equal(idx[0, 0], idx[0, 1])
    got, want, _ = _launch(dev, sr.TYPES[name], IDX[iname], src, idx, 80, "head", token_major=True, stride0=2)
    _assert_same(got, want, (name, iname))


@pytest.mark.parametrize("ne12", [2, 1])
@pytest.mark.parametrize("name", ["q5_1", "q4_0", "f16"])
def test_streams(dev, name, ne12):
    """ne3 = 2 streams: an index plane per stream, and one shared by both."""
    src = _src(2, 3, 22, 128)
    idx = sr.permuted_slots(80, (ne12, 3, 22), seed=6)
    got, want, _ = _launch(dev, sr.TYPES[name], sr.TYPE_I64, src, idx, 80, "pos")
    _assert_same(got, want, (name, ne12))


@pytest.mark.parametrize("name,ne0", [(n, k) for n in ("q8_0", "q5_0") for k in (32, 96, 320, 1024)] +
                         [("f16", k) for k in (1, 80, 1028)])
def test_row_lengths(dev, name, ne0):
    """nr = 5: 34-B and 22-B blocks are never dword multiples; 320 crosses a
    wave, 32 leaves most of a wave to other rows; F16 with a partial last group
    of four (1028), a partial block (80) and a single element."""
    src = _src(1, 2, 5, ne0)
    idx = sr.permuted_slots(9, (1, 1, 5), seed=ne0)
    for layout in ("pos", "head"):
        got, want, _ = _launch(dev, sr.TYPES[name], sr.TYPE_I64, src, idx, 9, layout)
        _assert_same(got, want, (name, ne0, layout))


@pytest.mark.parametrize("name,ne0", [("q4_0", 128), ("f16", 128), ("f16", 1028), ("q4_0", 320)])
def test_dword_source_path(dev, name, ne0):
    """src base 4 bytes past a 16-B boundary and nb[1] = ne0 * 4 + 4: no row is
    16-B aligned, the kernel reads dwords."""
    src = _src(1, 3, 22, ne0)
    idx = sr.permuted_slots(80, (1, 1, 22), seed=8)
    got, want, _ = _launch(dev, sr.TYPES[name], sr.TYPE_I64, src, idx, 80, "pos", base_off=4, row_pad=4)
    _assert_same(got, want, (name, ne0))


@pytest.mark.parametrize("row_pad", [0, 8])
def test_f16_tail(dev, row_pad):
    """F16 rows of 70 elements: the last group of four is two elements, on the
    dword path (nb[1] = 280) and on the 16-B path (nb[1] = 288)."""
    src = _src(1, 2, 5, 70)
    idx = sr.permuted_slots(9, (1, 1, 5), seed=70)
    got, want, _ = _launch(dev, sr.TYPE_F16, sr.TYPE_I32, src, idx, 9, "head", row_pad=row_pad)
    _assert_same(got, want, row_pad)


@pytest.mark.parametrize("name", ["q8_0", "q5_1", "f16"])
def test_out_of_range_slots_are_skipped(dev, name):
    """-1, n_slots, n_slots + 5, 2^32 + 3 and INT64_MIN among valid slots: those
    rows write nothing (slot 3 is not otherwise written: a truncated 2^32 + 3
    would land there), every other row is written, guards intact."""
    n_slots = 40
    i64 = np.array([7, -1, 12, n_slots, 0, n_slots + 5, 39, 2 ** 32 + 3, 21, -2 ** 63, 5, 30], dtype=np.int64)
    src = _src(1, 2, len(i64), 128)
    typ = sr.TYPES[name]
    got, want, before = _launch(dev, typ, sr.TYPE_I64, src, i64.reshape(1, 1, -1), n_slots, "pos")
    _assert_same(got, want, name)
    _, off, nb = sr.cache_alloc(typ, 128, n_slots, 2, 1, "pos")
    rb = sr.row_bytes(typ, 128)
    o = off + 3 * nb[1]
    assert np.array_equal(got[o:o + 2 * rb], before[o:o + 2 * rb])          # slot 3, both heads
    assert np.count_nonzero(got != before) > 7 * 2 * rb // 2                 # the seven valid rows were written
    i32 = np.array([7, -1, 12, n_slots, 0, 39], dtype=np.int64)
    src = _src(1, 2, len(i32), 128)
    got, want, _ = _launch(dev, typ, sr.TYPE_I32, src, i32.reshape(1, 1, -1), n_slots, "head")
    _assert_same(got, want, name)


@pytest.mark.parametrize("ne0,ne2", [(1024, 1), (128, 8)])
@pytest.mark.parametrize("name", ["q8_0", "q4_0", "q5_0", "f16"])
def test_decode_shapes(dev, name, ne0, ne2):
    """One token: a whole n_embd_k_gqa row, and eight heads of 128."""
    src = _src(1, ne2, 1, ne0, seed=12)
    idx = np.array([[[5]]], dtype=np.int64)
    got, want, _ = _launch(dev, sr.TYPES[name], sr.TYPE_I64, src, idx, 9, "pos")
    _assert_same(got, want, (name, ne0, ne2))


@pytest.mark.parametrize("name,ne0,nr,dword", [(n, 4128, 1020, False) for n in ALL] +
                         [("q4_0", 4128, 1020, True), ("f16", 4102, 1021, True)])
def test_large_write_form(dev, name, ne0, nr, dword):
    """From 2^17 units (32-element blocks) on, a lane group takes four units with
    all its loads issued first: 129 units per row x 1020 (1021) rows is just past
    that, with a last workgroup that is partly empty; every edge block, invalid
    slots among the valid ones, the 16-B and the dword source path (F16 rows of
    4102 elements: a two-element tail)."""
    assert (ne0 + 31) // 32 * nr >= 1 << 17 and ((ne0 + 31) // 32 * nr) % 128
    src = _src(1, 1, nr, ne0, seed=40)
    idx = sr.permuted_slots(nr + 10, (1, 1, nr), seed=41)
    idx[0, 0, [3, 500, nr - 1]] = [-1, 2 ** 32 + 5, nr + 10]
    got, want, _ = _launch(dev, sr.TYPES[name], sr.TYPE_I64, src, idx, nr + 10, "pos",
                           base_off=4 if dword else 0, row_pad=0)
    _assert_same(got, want, (name, ne0, dword))


@pytest.mark.parametrize("name", ["q5_1", "f16"])
def test_graph_replay_reads_new_slots(dev, name):
    """One set_rows captured on a side stream; the index tensor and the source
    are then overwritten in place and the graph replayed: the rows land in the
    new slots with the new bytes (the slots are data, not launch arguments)."""
    import torch
    typ, ne0, nr, ne2, n_slots = sr.TYPES[name], 128, 6, 2, 40
    a, b = _src(1, ne2, nr, ne0, seed=21), _src(1, ne2, nr, ne0, seed=22)
    ia, ib = sr.permuted_slots(n_slots, (1, 1, nr), seed=1), sr.permuted_slots(n_slots, (1, 1, nr), seed=2)
    assert not np.array_equal(ia, ib)
    cache, off, nb = sr.cache_alloc(typ, ne0, n_slots, ne2, 1, "pos")
    d_cache, d_src, d_idx = _dev(cache, dev), _dev(a, dev), _dev(ia.reshape(-1), dev)
    sv = fattn.View(d_src.data_ptr(), fattn.TYPE_F32, (ne0, nr, ne2, 1), sr.place_src(a)[2])
    iv = fattn.View(d_idx.data_ptr(), fattn.TYPE_I64, (nr, 1, 1, 1), (8, 8 * nr, 8 * nr, 8 * nr))
    dv = fattn.View(d_cache.data_ptr() + off, typ, (ne0, n_slots, ne2, 1), nb)
    g = capture(lambda stream: fattn.set_rows(sv, iv, dv, stream))
    want = sr.set_rows_ref(cache, a, ia, typ, n_slots, off, nb)
    _assert_same(d_cache.cpu().numpy(), want, "eager")       # (capturing launched nothing: the eager launch's rows)
    d_src.copy_(_dev(b, dev))
    d_idx.copy_(_dev(ib.reshape(-1), dev))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = sr.set_rows_ref(want, b, ib, typ, n_slots, off, nb)
    _assert_same(d_cache.cpu().numpy(), want, "replay")


@pytest.mark.parametrize("name", ["q8_0", "f16"])
def test_end_to_end_decode(dev, name):
    """A 29-token prompt, then three decode steps at D = 128, Hkv = 2, H = 4 over
    a 96-slot cache: each step set_rows K and V into scattered slots, then
    fattn_ext with a mask that is -inf on unwritten slots.  The output is
    bit-equal to a launch over the cache built on the host, and within the
    project's bars of oracle.flash_attn_ext."""
    import torch
    typ = sr.TYPES[name]
    D, Hkv, H, N, NP = 128, 2, 4, 96, 128
    rb, eb = sr.row_bytes(typ, D), sr.elem_bytes(typ)
    nb = (eb, Hkv * rb, rb, N * Hkv * rb)                   # [N][Hkv][row]
    rng = np.random.default_rng(31)
    slots = rng.permutation(N)
    # (zeros, not random bytes: an unwritten f16 slot must not decode to NaN, whose product with weight 0 is NaN)
    host = {"k": np.zeros(N * Hkv * rb, dtype=np.uint8), "v": np.zeros(N * Hkv * rb, dtype=np.uint8)}
    devc = {n: _dev(c, dev) for n, c in host.items()}
    mask = np.full((1, NP), -np.inf, dtype=np.float32)
    written = 0
    for step, ntok in enumerate((29, 1, 1, 1)):
        cur = {n: (1.0 - 2.0 * rng.random((1, Hkv, ntok, D), dtype=np.float32)).astype(np.float32) for n in ("k", "v")}
        idx = slots[written:written + ntok].astype(np.int64).reshape(1, 1, ntok)
        d_idx = _dev(idx.reshape(-1), dev)
        iv = fattn.View(d_idx.data_ptr(), fattn.TYPE_I64, (ntok, 1, 1, 1), (8, 8 * ntok, 8 * ntok, 8 * ntok))
        keep = []
        for n in ("k", "v"):
            sflat, _, snb = sr.place_src(cur[n], token_major=True)
            d_src = _dev(sflat, dev)
            keep.append(d_src)
            fattn.set_rows(fattn.View(d_src.data_ptr(), fattn.TYPE_F32, (D, ntok, Hkv, 1), snb), iv,
                           fattn.View(devc[n].data_ptr(), typ, (D, N, Hkv, 1), nb))
            host[n] = sr.set_rows_ref(host[n], cur[n], idx, typ, N, 0, nb)
        mask[0, idx.reshape(-1)] = (1.0 - 2.0 * rng.random(ntok, dtype=np.float32)).astype(np.float32)
        written += ntok
        if step == 0:
            continue
        q = (1.0 - 2.0 * rng.random((1, 1, H, D), dtype=np.float32)).astype(np.float32)
        p = Problem(D, 1, H, Hkv, N, 1, 1, typ, "pos", float(np.float32(1.0 / np.sqrt(np.float32(D)))), q,
                    host["k"], host["v"], nb, nb, orc.f32_to_f16_bits(mask))
        t = upload(p, dev)                                    # the cache built on the host
        att = fattn.Attention(*gpu_views(p, t), t["dst"], p.scale)
        att()
        torch.cuda.synchronize()
        over_host = t["dst"].cpu().numpy().copy()
        t["dst"].fill_(float("nan"))
        att.retarget(k=devc["k"].data_ptr(), v=devc["v"].data_ptr())   # the cache set_rows wrote
        att()
        torch.cuda.synchronize()
        over_dev = t["dst"].cpu().numpy()
        for n in ("k", "v"):
            _assert_same(devc[n].cpu().numpy(), host[n], (name, step, n))
        assert np.array_equal(over_dev.view(np.uint32), over_host.view(np.uint32)), (name, step)
        ref = p.oracle()
        rel, elem = attn_rel_err(over_dev, ref), attn_elem_err(over_dev, ref)
        print(f"SETROWS e2e {name} step {step} written {written} rel={rel:.3e} elem={elem:.3f} | {att.describe()}")
        assert rel <= 1e-3, (rel, name, step)
        assert elem <= 1.0, (elem, name, step)


def test_harness_set_rows():
    """kernel_test --set-rows --kv-type q5_1: the caches written by fattn_set_rows
    through a seeded slot permutation; its own max-diff check."""
    r = run_kernel_test(["--iters", "3", "--set-rows", "--kv-type", "q5_1"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
