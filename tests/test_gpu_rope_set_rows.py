"""GPU: fattn_rope_set_rows.  Every dst is a view in the middle of a larger random-filled allocation and the
WHOLE allocation is compared.  The rotation is checked once per argument set, on an F32 dst (f32_y): Y within
k_shift.tol() -- the derived bound -- of rotate_f64, every byte outside the rows of valid slots unchanged.  A
typed dst must then hold encode(Y) bit for bit: the rotation is one function for all types."""
import dataclasses

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

import fattn
import iq4_nl
import k_shift as ks
import set_rows as sr
from gpu_util import capture, check_bars, run_kernel_test, upload, views as gpu_views
from problems import make_problem
from test_gpu_k_shift import _assert_same, _dev, _launch as k_shift_launch

pytestmark = pytest.mark.gpu
TYPES = dict(ks.TYPES, iq4_nl=iq4_nl.TYPE_IQ4_NL)
NR, NE2, N_SLOTS = 67, 3, 19
MODES = {"norm": ks.NORMAL, "neox": ks.NEOX}


def _encode(y, typ):
    return iq4_nl.quantize(y) if typ == iq4_nl.TYPE_IQ4_NL else ks.encode(y, typ)


def _rows_view(alloc, off, nb, typ, ne):
    return as_strided(alloc[off:], shape=(ne[3], ne[2], ne[1], fattn.row_size(typ, ne[0])), strides=(nb[3], nb[2], nb[1], 1))


def _x(ne3, ne2, nr, ne0, seed=5):
    rng = np.random.default_rng(seed)
    return (3.0 * (1.0 - 2.0 * rng.random((ne3, ne2, nr, ne0), dtype=np.float32))).astype(np.float32)


def _idx(n_slots, shape, seed=3, far=2 ** 32 + 3):
    """int64 [ne12][ne11][nr]: per row min(nr, n_slots) - 2 distinct valid slots, the rest -1, n_slots or 2^32 + 3."""
    rng = np.random.default_rng(seed)
    out = rng.choice(np.array([-1, n_slots, far], dtype=np.int64), size=shape)
    for row in out.reshape(-1, shape[2]):
        where = rng.permutation(shape[2])[:min(shape[2], n_slots) - 2]
        row[where] = rng.permutation(n_slots)[:len(where)]
    return out


class Part:
    """One of K / V: src f32 [ne3][ne2][nr][ne0] placed by set_rows.place_src, dst a fresh guarded allocation of typ."""
    def __init__(self, dev, src, typ, n_slots=N_SLOTS, layout="pos", **place):
        ne3, ne2, nr, ne0 = src.shape
        self.src, self.typ, self.ne = src, typ, (ne0, n_slots, ne2, ne3)
        alloc = ks.make_cache if typ == ks.TYPE_F32 else sr.cache_alloc       # (F32 guards are 4-byte multiples)
        self.alloc, self.off, self.nb = alloc(typ, ne0, n_slots, ne2, ne3, layout)
        flat, soff, snb = sr.place_src(src, **place)
        self.d_src, self.d_alloc = _dev(flat, dev), _dev(self.alloc, dev)
        self.sv = fattn.View(self.d_src.data_ptr() + soff, fattn.TYPE_F32, (ne0, nr, ne2, ne3), snb)
        self.dv = fattn.View(self.d_alloc.data_ptr() + self.off, typ, self.ne, self.nb)

    def got(self):
        return self.d_alloc.cpu().numpy()

    def slots(self, idx):
        s = idx[np.arange(self.ne[3])[:, None] % idx.shape[0], np.arange(self.ne[2])[None, :] % idx.shape[1]]
        return s, (s >= 0) & (s < self.ne[1])

    def want(self, idx, y):
        # the allocation with encode(y) in the rows of valid slots: set_rows_ref where it has the type
        if self.typ in sr.TYPES.values():
            return sr.set_rows_ref(self.alloc, y, idx, self.typ, self.ne[1], self.off, self.nb)
        out = self.alloc.copy()
        s, ok = self.slots(idx)
        i3, i2, _ = np.nonzero(ok)
        _rows_view(out, self.off, self.nb, self.typ, self.ne)[i3, i2, s[ok]] = _encode(y, self.typ)[ok]
        return out


def _launch(dev, k, idx, pos=None, rope=None, ff=None, v=None, ityp=sr.TYPE_I64, stride0=1, stream=None):
    import torch
    iflat, ine, inb = sr.place_idx(idx, ityp, stride0)
    d_idx = _dev(iflat, dev)
    d_pos = d_ff = pv = None
    if rope is not None:
        npl, nr = pos.shape
        d_pos = _dev(pos.reshape(-1), dev)
        pv = fattn.View(d_pos.data_ptr(), fattn.TYPE_I32, (nr, npl, 1, 1), (4, 4 * nr, 4 * nr * npl, 4 * nr * npl))
        d_ff = None if ff is None else _dev(np.asarray(ff, dtype=np.float32), dev)
    call = lambda st: fattn.rope_set_rows(k.sv, pv, fattn.View(d_idx.data_ptr(), ityp, ine, inb), k.dv, None if rope is None else rope.c(),
                                          d_ff, v and v.sv, v and v.dv, st)
    call(stream)
    torch.cuda.synchronize()
    return call, d_idx, d_pos


def f32_y(dev, x, idx, pos, rope, ff=None, what="", layout="pos", n_slots=N_SLOTS, **kw):
    # the module docstring's F32 launch: returns Y f32 like x (rows of invalid slots: zeros)
    k = Part(dev, x, ks.TYPE_F32, n_slots, layout, **{n: kw.pop(n) for n in ("token_major", "base_off", "row_pad") if n in kw})
    _launch(dev, k, idx, pos, rope, ff, **kw)
    got = k.got()
    s, ok = k.slots(idx)
    i3, i2 = np.indices(s.shape)[:2]
    y = np.where(ok[..., None], _rows_view(got, k.off, k.nb, k.typ, k.ne)[i3, i2, np.clip(s, 0, n_slots - 1)].view(np.float32), 0)
    _assert_same(got, k.want(idx, y), (what, "f32: bytes outside the written rows"))
    p = pos[np.arange(x.shape[0]) % pos.shape[0]][:, None, :]
    want, t = ks.rotate_f64(x, p, rope, ff), ks.tol(x, p, rope, ff)
    err = np.abs(y.astype(np.float64) - want)[ok]
    worst = float((err / np.maximum(t[ok], 1e-300))[t[ok] > 0].max())
    print(f"ROPESET {what}: {int(ok.sum())} rows, max |err| {err.max():.3e}, worst err / tol {worst:.3f}")
    assert ok.any() and not ok.all() and (err <= t[ok]).all(), (what, worst)
    return y.astype(np.float32)


@pytest.mark.parametrize("case", sorted(ks.ROTATION_CASES))
def test_rotation_f32(dev, case):
    ne0, rope, ff, big = ks.ROTATION_CASES[case]
    f32_y(dev, _x(1, NE2, NR, ne0), _idx(N_SLOTS, (1, 1, NR)), ks.make_shift(NR, 1, seed=3, big=big), rope, ff, case)


@pytest.mark.parametrize("ne0,nr", [(128, 67), (32, 67), (64, 5), (96, 5), (256, 67)])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(set(TYPES) - {"f32"}))
def test_every_type(dev, name, mode, ne0, nr):
    # a real rotation of random rows, then the EXACT one (p = 1, freq_scale = 2^-100) over set_rows.py's edge blocks
    edge = sr.source_rows(NE2 * nr, ne0, seed=6).reshape(1, NE2, nr, ne0)
    n = min(nr - 1, N_SLOTS - 2)                                # (the edge blocks fill the first rows of head 0: those get the slots)
    eidx = np.full((1, 1, nr), -1, dtype=np.int64)
    eidx[0, 0, :n] = np.random.default_rng(nr).permutation(N_SLOTS)[:n]
    for x, idx, pos, rope in ((_x(1, NE2, nr, ne0), _idx(N_SLOTS, (1, 1, nr), seed=nr), ks.make_shift(nr, 1, seed=7), ks.Rope(ne0, MODES[mode])),
                              (edge, eidx, np.ones((1, nr), dtype=np.int32), ks.Rope(ne0, MODES[mode], freq_scale=2.0 ** -100))):
        y = f32_y(dev, x, idx, pos, rope, what=f"{name} {mode} {ne0}")
        k = Part(dev, x, TYPES[name])
        _launch(dev, k, idx, pos, rope)
        _assert_same(k.got(), k.want(idx, y), (name, mode, ne0, nr))


@pytest.mark.parametrize("case", ["neox-128-yarn", "norm-128-ff", "neox-80of128", "neox-128-big"])
def test_same_y_as_k_shift(dev, case):
    ne0, rope, ff, big = ks.ROTATION_CASES[case]
    x, pos = _x(1, NE2, NR, ne0, seed=11), ks.make_shift(NR, 1, seed=5, big=big)
    idx = np.arange(-1, NR - 1, dtype=np.int64).reshape(1, 1, NR)   # token i into slot i - 1 (token 0 out of range)
    y = f32_y(dev, x, idx, pos, rope, ff, case, "head", NR)
    alloc, off, nb = ks.make_cache(ks.TYPE_F32, ne0, NR, NE2, 1, "head", values=x)
    ne = (ne0, NR, NE2, 1)
    shifted = ks.cache_values(k_shift_launch(dev, alloc, off, nb, ks.TYPE_F32, ne, pos, rope, ff), off, nb, ks.TYPE_F32, ne)
    sel = pos[0] != 0
    sel[0] = False
    assert sel.sum() > NR // 2
    assert np.array_equal(shifted[:, :, sel].view(np.uint32), y[:, :, sel].view(np.uint32))


def _set_rows(dev, part, idx, layout="pos"):
    import torch
    twin = Part(dev, part.src, part.typ, part.ne[1], layout)       # (fattn_set_rows over an identically initialised allocation)
    iflat, ine, inb = sr.place_idx(idx, sr.TYPE_I64)
    d_idx = _dev(iflat, dev)
    fattn.set_rows(twin.sv, fattn.View(d_idx.data_ptr(), sr.TYPE_I64, ine, inb), twin.dv)
    torch.cuda.synchronize()
    return twin.got()


@pytest.mark.parametrize("name,ne0", [(n, 320) for n in sorted(TYPES)] + [("f32", 70), ("bf16", 70), ("f16", 1)])
def test_no_rope(dev, name, ne0):
    x = sr.source_rows(NE2 * NR, ne0).reshape(1, NE2, NR, ne0)
    idx = _idx(N_SLOTS, (1, 1, NR), seed=ne0)
    k = Part(dev, x, TYPES[name])
    _launch(dev, k, idx)
    _assert_same(k.got(), k.want(idx, x) if name in ("f32", "bf16") else _set_rows(dev, k, idx), (name, ne0))


@pytest.mark.parametrize("ne0,ne0v", [(64, 128), (128, 320)])
@pytest.mark.parametrize("kname,vname", [("q8_0", "q4_0"), ("f16", "f16"), ("bf16", "bf16"), ("q5_1", "iq4_nl")])
def test_k_and_v(dev, kname, vname, ne0, ne0v):
    xk, xv = _x(1, NE2, NR, ne0, seed=13), sr.source_rows(4 * NR, ne0v, seed=14).reshape(1, 4, NR, ne0v)   # (ne2v = 4)
    idx, pos, rope = _idx(N_SLOTS, (1, 1, NR), seed=15), ks.make_shift(NR, 1, seed=15), ks.Rope(ne0, ks.NEOX)
    k, v, k_only = Part(dev, xk, TYPES[kname]), Part(dev, xv, TYPES[vname], layout="head"), Part(dev, xk, TYPES[kname])
    _launch(dev, k, idx, pos, rope, v=v)
    _launch(dev, k_only, idx, pos, rope)
    _assert_same(k.got(), k_only.got(), ("K", kname, vname))
    want = v.want(idx, xv) if vname == "bf16" else _set_rows(dev, v, idx, "head")
    _assert_same(v.got(), want, ("V", kname, vname))


VIEWS = {"head-cache": dict(layout="head"), "token-major": dict(token_major=True), "dword-source": dict(base_off=4, row_pad=4),
         "i32-strided": dict(ityp=sr.TYPE_I32, stride0=2), "per-head-idx": dict(ne11=NE2), "S2-one-plane": dict(ne3=2),
         "S2-two-planes": dict(ne3=2, npl=2, ne12=2)}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_views(dev, view):
    kw = dict(VIEWS[view])
    ne3, npl, ne11, ne12 = kw.pop("ne3", 1), kw.pop("npl", 1), kw.pop("ne11", 1), kw.pop("ne12", 1)
    x, xv = _x(ne3, NE2, NR, 128, seed=17), _x(ne3, NE2, NR, 128, seed=18)
    idx = _idx(N_SLOTS, (ne12, ne11, NR), 19, **({"far": 2 ** 31 - 1} if "ityp" in kw else {}))
    pos, rope = ks.make_shift(NR, npl, seed=19), ks.Rope(128, ks.NEOX)
    y = f32_y(dev, x, idx, pos, rope, what=view, **kw)
    layout = kw.pop("layout", "pos")
    place = {n: kw.pop(n) for n in ("token_major", "base_off", "row_pad") if n in kw}
    k, v = Part(dev, x, TYPES["q8_0"], N_SLOTS, layout, **place), Part(dev, xv, TYPES["q4_1"], N_SLOTS, layout, **place)
    _launch(dev, k, idx, pos, rope, v=v, **kw)
    _assert_same(k.got(), k.want(idx, y), (view, "K"))
    _assert_same(v.got(), v.want(idx, xv), (view, "V"))


def test_several_units_form(dev):
    """2051 tokens x 8 heads x 128, K and V: 131264 units, just past the threshold from which a lane group of a
    rope-less launch takes four; the last workgroup is partly empty.  With a rope: the one-unit form."""
    nr, n_slots = 2051, 2100
    x, xv = _x(1, 8, nr, 128, seed=21), _x(1, 8, nr, 128, seed=22)
    idx, pos, rope = _idx(n_slots, (1, 1, nr), seed=23), ks.make_shift(nr, 1, seed=23, big=True), ks.Rope(128, ks.NEOX)
    for y, args in ((f32_y(dev, x, idx, pos, rope, what="several units", n_slots=n_slots), (pos, rope)), (x, ())):
        k, v = Part(dev, x, TYPES["q8_0"], n_slots, "head"), Part(dev, xv, TYPES["q5_0"], n_slots, "head")
        _launch(dev, k, idx, *args, v=v)
        _assert_same(k.got(), k.want(idx, y), ("K", len(args)))
        _assert_same(v.got(), v.want(idx, xv), ("V", len(args)))


def test_head_walk_and_head_grid_agree(dev):
    # 66000 tokens of ne0 = 32 fill the chip: a lane group walks all 8 heads; as 8 sequences of one head it cannot
    nr, hkv = 66000, 8
    x, pos = _x(1, hkv, nr, 32, seed=25), ks.make_shift(nr, 1, seed=25)
    idx = np.random.default_rng(25).permutation(nr).astype(np.int64).reshape(1, 1, nr)
    idx[0, 0, ::97] = -1
    a, b = Part(dev, x, TYPES["q8_0"], nr, "head"), Part(dev, x, TYPES["q8_0"], nr, "head")
    swap = lambda view: fattn.View(view.ptr, view.type, (32, view.ne[1], 1, hkv), (view.nb[0], view.nb[1], view.nb[3], view.nb[2]))
    b.sv, b.dv = swap(b.sv), swap(b.dv)
    _launch(dev, a, idx, pos, ks.Rope(32, ks.NEOX))
    _launch(dev, b, idx, pos, ks.Rope(32, ks.NEOX))
    got = a.got()
    _assert_same(got, b.got(), "walk against grid")
    ok = idx[0, 0, :64] >= 0                                    # and both are the write: the first 64 tokens, slots of their own
    y = f32_y(dev, x[:, :, :64], np.where(ok, np.arange(64), -1).reshape(1, 1, 64), pos[:, :64], ks.Rope(32, ks.NEOX), what="walk sample", n_slots=64)
    assert np.array_equal(_rows_view(got, a.off, a.nb, a.typ, a.ne)[0][:, idx[0, 0, :64][ok]], _encode(y, a.typ)[0][:, ok])


def test_graph_replay_reads_new_inputs(dev):
    # pos, idx and both sources overwritten in place after the capture: every replay is the eager launch over the new data
    import torch
    rope = ks.Rope(128, ks.NEOX)
    xs = [(_x(1, NE2, NR, 128, seed=s), _x(1, NE2, NR, 128, seed=s + 1)) for s in (31, 41)]
    idxs, poss = [_idx(N_SLOTS, (1, 1, NR), seed=s) for s in (32, 42)], [ks.make_shift(NR, 1, seed=s) for s in (33, 43)]
    k, v = Part(dev, xs[0][0], TYPES["q5_1"]), Part(dev, xs[0][1], TYPES["f16"])
    call, d_idx, d_pos = _launch(dev, k, idxs[0], poss[0], rope, v=v)
    g = capture(call)
    eager_k, eager_v = Part(dev, xs[1][0], TYPES["q5_1"]), Part(dev, xs[1][1], TYPES["f16"])
    _launch(dev, eager_k, idxs[1], poss[1], rope, v=eager_v)
    for _ in range(3):
        for d, new in ((k.d_src, xs[1][0]), (v.d_src, xs[1][1]), (d_idx, idxs[1]), (d_pos, poss[1]), (k.d_alloc, k.alloc), (v.d_alloc, v.alloc)):
            d.copy_(_dev(new.reshape(-1), dev))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(k.got(), eager_k.got(), "replay K")
        _assert_same(v.got(), eager_v.got(), "replay V")


@pytest.mark.parametrize("name", ["f16", "q8_0"])
def test_end_to_end(dev, name):
    """Three decode steps (one token each, slots 157 .. 159) then fattn_ext: bit-equal to the launch over caches built
    on the host from the GPU's own Y, and within the project's bars of the oracle over the rotate_f64-built cache."""
    import torch
    p = make_problem(D=128, NQ=1, H=4, Hkv=2, N=160, kv_type=name, seed=43)
    rope, steps = ks.Rope(128, ks.NEOX), (157, 158, 159)
    xk, xv = _x(1, 2, 3, 128, seed=45), _x(1, 2, 3, 128, seed=46)
    pos, idx = np.array([steps], dtype=np.int32), np.array([[steps]], dtype=np.int64)
    y = f32_y(dev, np.concatenate([xk, xk[:, :, :1]], axis=2), np.array([[list(steps) + [-1]]]), np.array([list(steps) + [0]], dtype=np.int32),
              rope, what="e2e", n_slots=160)[:, :, :3]

    def attend(k_bytes, v_bytes, write):
        q = dataclasses.replace(p, k_bytes=k_bytes, v_bytes=v_bytes)
        t = upload(q, dev)
        qv, kv, vv, mv = gpu_views(q, t)
        if write:
            for i in range(3):
                d_k, d_v, d_pos, d_idx = (_dev(a, dev) for a in (xk[:, :, i:i + 1], xv[:, :, i:i + 1], pos[:, i], idx[0, :, i]))
                part = lambda d: fattn.View(d.data_ptr(), fattn.TYPE_F32, (128, 1, 2, 1), (4, 512, 512, 1024))
                fattn.rope_set_rows(part(d_k), fattn.View(d_pos.data_ptr(), fattn.TYPE_I32, (1, 1, 1, 1), (4, 4, 4, 4)),
                                    fattn.View(d_idx.data_ptr(), fattn.TYPE_I64, (1, 1, 1, 1), (8, 8, 8, 8)), kv, rope.c(), None, part(d_v), vv)
                torch.cuda.synchronize()                          # (the step's inputs are released with the loop variables)
        fattn.Attention(qv, kv, vv, mv, t["dst"], p.scale)()
        torch.cuda.synchronize()
        return t["dst"].cpu().numpy()

    def host_cache(yk):
        k, v = p.k_bytes.copy(), p.v_bytes.copy()
        _rows_view(k, 0, p.k_nb, p.kv_type, p.kv_ne)[0, :, 157:160] = ks.encode(yk, p.kv_type)[0]
        _rows_view(v, 0, p.v_nb, p.kv_type, p.kv_ne)[0, :, 157:160] = ks.encode(xv, p.kv_type)[0]
        return k, v

    got = attend(p.k_bytes, p.v_bytes, True)
    assert np.array_equal(got, attend(*host_cache(y), False))
    k64, v64 = host_cache(ks.rotate_f64(xk, pos[:, None, :], rope).astype(np.float32))
    ref = dataclasses.replace(p, k_bytes=k64, v_bytes=v64).oracle()
    check_bars(got, ref, lambda rel, elem: f"ROPESET e2e {name} rel={rel:.3e} elem={elem:.3f}")
    assert np.abs(ref - p.oracle()).max() > 1e-3                  # (the three new tokens matter to the output)


@pytest.mark.parametrize("kv_type,mode", [("q8_0", "neox"), ("q5_1", "norm")])
def test_harness_rope_set_rows(kv_type, mode):
    r = run_kernel_test(["--iters", "3", "--rope-set-rows", "--kv-type", kv_type, "--rope-mode", mode, "--heads", "8",
                         "--kv-heads", "4", "--kv-size", "512"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and "rope-set-rows" in r.stdout
