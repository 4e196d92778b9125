"""Host side of the big-view tests (tests/big_views.py): the layout function,
the planner's answer to every case of tests/test_gpu_big_views.py, the exact
span limits of K, V, the mask and Q on the generic and the MLA path, the
tail-tile rule, and the wrap witnesses that keep the GPU cases from testing
nothing.  Planning uses fake addresses: nothing here touches a GPU.
"""
import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

import big_views as bv
import fattn
import mla
from problems import make_problem

BAD_STRIDE = -4
SPAN_MAX = bv.SPAN_MAX


def _status(lay, kv_chunk=0, opts=()):
    with fattn.options(dict(opts)):
        try:
            return 0, fattn.describe(lay.params(kv_chunk=kv_chunk))
        except fattn.FattnError as e:
            return e.code, ""


# ------------------------------------------------------------------ the layout function

@pytest.mark.parametrize("case", bv.CASES, ids=[c.id for c in bv.CASES])
def test_layout_is_sound(case):
    """No two placed rows share a byte, everything (guards included) fits the
    arena, every view's ne / nb address exactly the rows placed, and no case
    holds more than the arena."""
    for lay in (bv.big_layout(case), bv.twin_layout(case)):
        assert lay.bytes <= bv.ARENA_BYTES
        assert not bv.overlaps(lay)
        for x in lay.t.values():
            assert x.base % 4 == 0 and x.base >= 0
            if x.shape is None:
                k = lay.t["k"]
                assert x.nb == k.nb and k.base <= x.base < k.base + k.row
                continue
            assert x.base + x.extent + bv.GUARD <= lay.bytes
            assert all(s > 0 for s in x.strides)
            n3, n2, n1 = x.shape[:3]
            if lay.lg.v_trans and x.name == "v":
                assert (x.ne[3], x.ne[2], x.ne[0]) == (n3, n2, n1) and (x.nb[3], x.nb[2], x.nb[0]) == x.strides[:3]
                assert x.nb[1] == 2 and x.row == 2 * x.ne[1]
            else:
                assert (x.ne[3], x.ne[2], x.ne[1]) == (n3, n2, n1) and (x.nb[3], x.nb[2], x.nb[1]) == x.strides[:3]
                eb = 4 if x.name == "q" else 2 if x.name == "mask" else bv.elem_bytes(x.type)
                per = 1 if x.name in ("q", "mask") or x.type in bv.ROW16 else 32
                assert x.nb[0] == eb and x.row == x.ne[0] // per * eb


@pytest.mark.parametrize("tag", ["A-split-q5_1", "A-split-vtrans", "A-mla-f16-own", "B-mla-q8_0-nb3", "C-mask-planes-split",
                                 "C-q-nb3-mla", "B-bdp-q8_0-nb3"])
def test_placement_round_trip(tag):
    """place() on a host tensor (the compact twin: the code path is the big
    view's): every tensor read back through its strides equals its rows, and
    every byte outside the rows is its region's poison."""
    import torch
    case = next(c for c in bv.CASES if c.tag == tag)
    lay = bv.twin_layout(case)
    raw = torch.zeros(lay.bytes + 4096, dtype=torch.uint8)
    off = (-raw.data_ptr()) % 4096
    arena = raw[off:off + lay.bytes]
    bv.place(lay, arena)
    a = arena.numpy()
    covered = np.zeros(lay.bytes, dtype=bool)
    for x in lay.t.values():
        if x.shape is None:
            continue
        assert np.array_equal(as_strided(a[x.base:], shape=x.shape, strides=x.strides), x.rows), x.name
        for s, e in x.intervals():
            covered[s:e] = True
    starts = sorted((x.base, x.poison) for x in lay.t.values() if x.shape is not None)
    for i, (s, poison) in enumerate(starts):
        e = starts[i + 1][0] if i + 1 < len(starts) else lay.bytes
        want = np.full((e - s) // 4, poison, dtype=np.uint32).view(np.uint8)
        hole = ~covered[s:e]
        assert np.array_equal(a[s:e][hole], want[hole]), (tag, s)


def test_wrap_witnesses_of_the_issue_view():
    """f16, D = 128, N = 77, nb[1] = 53 MiB: span 4 223 664 384; row 77 lies past
    it, row 78 wraps to byte 39 845 888 -- inside the descriptor, on poison."""
    case = next(c for c in bv.CASES if c.tag == "A-split-f16-asissue")
    lay = bv.big_layout(case)
    k = lay.t["k"]
    assert k.span == 4223664384
    w = bv.wraps(lay, "k", 32)
    assert [r for r, _, _ in w] == list(range(78, 96))
    assert w[0] == (78, 39845888, True)
    assert all(on_poison for _, _, on_poison in w)
    assert bv.wraps(lay, "v", 32)[0][:2] == (78, 39845888)


# ------------------------------------------------------------------ every GPU case, planned on the host

@pytest.mark.parametrize("case", bv.CASES, ids=[c.id for c in bv.CASES])
def test_case_plans(case):
    """The planner's status, the kernel family and the twin's plan; a
    near-limit, ragged case (Case.tile) has a wrap witness on poison -- or, where
    the planner rejects the view for it, that is what the case asserts."""
    lay = bv.big_layout(case)
    code, d = _status(lay, case.kv_chunk, case.opts)
    assert code == case.status, (code, d)
    if case.tile:
        w = bv.wraps(lay, "k", case.tile)
        assert any(on_poison for _, _, on_poison in w), "the case's last key tile wraps nowhere: it tests nothing"
    if case.status:
        return
    assert case.kernel in d and not (case.avoid and case.avoid in d), d
    code_t, d_t = _status(bv.twin_layout(case), case.kv_chunk, case.opts)
    assert code_t == 0
    if case.twin:
        assert d_t == d


def test_accepted_views_have_no_wrapping_tail_row():
    """The planner rule behind the near-limit cases: no accepted K / V view of
    the table has a row of its kernel's last key tile back inside the span --
    for the kernels that fetch such rows by offset alone (tail_tile())."""
    for case in bv.CASES:
        if case.status or case.kind in ("mla", "mlaq"):
            continue
        lay = bv.big_layout(case)
        _, d = _status(lay, case.kv_chunk, case.opts)
        tile = bv.tail_tile(d)
        for name in ("k", "v"):
            if not (name == "v" and lay.lg.v_trans):
                assert not bv.wraps(lay, name, tile), (case.tag, name, d)


# ------------------------------------------------------------------ the exact limits

def _generic(N=64, NQ=1, H=2, Hkv=2, kt="f16", D=128, **kw):
    return bv.from_problem(make_problem(D=D, NQ=NQ, H=H, Hkv=Hkv, N=N, kv_type=kt, seed=1, **kw))


def _blank(kt: str, N: int, D: int = 128, mla_v=None) -> bv.Logical:
    """A Logical of zeros, one head, one query row (planning reads no values).
    mla_v: None (generic), "view" (V inside K's rows) or "own"."""
    typ = fattn.TYPE_NAMES[kt]
    dq = fattn.MLA_DK if mla_v else D
    dv = fattn.MLA_DV if mla_v else D
    k = np.zeros((1, 1, N, bv.row_bytes(typ, dq)), dtype=np.uint8)
    v = None if mla_v == "view" else np.zeros((1, 1, N, bv.row_bytes(typ, dv)), dtype=np.uint8)
    v_off = (128 if kt == "f16" else 2 * bv.elem_bytes(typ)) if mla_v == "view" else 0
    return bv.Logical(np.zeros((1, 1, 1, dq), dtype=np.float32), typ, k, typ, v, dv, None, 0.125, False, v_off)


def _mla_f16(v_form, N=64, NQ=1, H=2):
    c, _ = mla.cached(mla.Shape(H=H, Hkv=1, NQ=NQ, N=N))
    return bv.from_mla(mla.MlaLaunch(c, "head", v_form))


def _limit_rows(row: int, align: int, tile: int = 32):
    """(N, nb1, exact) for a view of whole key tiles (N % tile == 0: the tail
    rule adds nothing) at the span limit: (N - 1) nb1 + row == SPAN_MAX where
    some N below 2^16 and nb1 % align == 0 allow it (exact), else N = tile with
    the largest such nb1 (the span then ends less than align (N - 1) bytes short)."""
    for n in range(tile, 1 << 16, tile):
        q, r = divmod(SPAN_MAX - row, n - 1)
        if r == 0 and q % align == 0:
            return n, q, True
    return tile, bv.nb1_for_span(SPAN_MAX, tile, row, align), False


def _accept_reject(build, step=16):
    """build(extra) -> Layout: plans at the limit, FATTN_ERR_BAD_STRIDE one stride step past it."""
    assert _status(build(0))[0] == 0
    assert _status(build(step))[0] == BAD_STRIDE


def _rows_limit(kt, name):
    """K's or V's rows on the generic path (the dword path: nb[1] % 4 == 0).  A
    row stride moves the span by nb[1]'s step times N - 1, so 16 bytes past the
    limit is not a view of whole key tiles; the pair is the limit itself (exact
    for Q4_0 and Q5_1 rows, as near as nb[1] % 4 allows for F16 and Q8_0) and
    the next stride."""
    row = bv.row_bytes(fattn.TYPE_NAMES[kt], 128)
    n, nb1, exact = _limit_rows(row, 4)
    lg = _blank(kt, n)

    def build(x):
        lay = bv.layout(lg, **{name + "_nb": (nb1 + x, None, None)})
        span = lay.t[name].span
        assert (span == SPAN_MAX + x * (n - 1)) if exact else (SPAN_MAX - 4 * (n - 1) < span - x * (n - 1) <= SPAN_MAX)
        return lay
    _accept_reject(build, 4)
    return exact


@pytest.mark.parametrize("kt", ["f16", "q8_0", "q4_0", "q5_1"])
def test_k_span_limit_generic(kt):
    assert _rows_limit(kt, "k") == (kt in ("q4_0", "q5_1"))


@pytest.mark.parametrize("kt", ["f16", "q8_0", "q4_0", "q5_1"])
def test_v_span_limit_generic(kt):
    assert _rows_limit(kt, "v") == (kt in ("q4_0", "q5_1"))


@pytest.mark.parametrize("kt", ["f16", "q8_0"])
def test_k_span_limit_mla(kt):
    """k_span = 0xFFFFFFF0 plans, 16 bytes more is FATTN_ERR_BAD_STRIDE (two
    rows; the MLA kernel guards the rows past N itself)."""
    lg = _blank(kt, 2, mla_v="view")
    row = lg.k_rows.shape[3]

    def build(x):
        lay = bv.layout(lg, k_nb=(SPAN_MAX - row + x, None, None))
        assert lay.t["k"].span == SPAN_MAX + x
        return lay
    _accept_reject(build)


def test_v_span_limit_mla_own():
    lg = _blank("f16", 2, mla_v="own")

    def build(x):
        lay = bv.layout(lg, k_nb=(SPAN_MAX - 1152, None, None), v_nb=(SPAN_MAX - 1024 + x, None, None), v_in_k=True)
        assert lay.t["v"].span == SPAN_MAX + x and lay.t["k"].span == SPAN_MAX
        return lay
    _accept_reject(build)


def test_v_span_limit_transposed():
    """(D - 1) nb[0] + 2 N == 0xFFFFFFF0 with N % 32 == 0 and nb[0] % 16 == 0
    plans; the next nb[0] is BAD_STRIDE."""
    nb0 = next(b for b in range(bv.down16(SPAN_MAX // 127), 0, -16) if (SPAN_MAX - 127 * b) % 64 == 0 and SPAN_MAX > 127 * b)
    n = (SPAN_MAX - 127 * nb0) // 2
    assert n > 0 and n % 32 == 0 and 127 * nb0 + 2 * n == SPAN_MAX
    lg = _generic(N=n, v_trans=True, mask="none")
    _accept_reject(lambda x: bv.layout(lg, v_nb0=nb0 + x, v_nb=(None, 4096, None)))


@pytest.mark.parametrize("path", ["generic", "mla"])
def test_mask_span_limit(path):
    """m_span = (n_q - 1) nb[1] + 2 ne[0] at the limit (two query rows)."""
    if path == "generic":
        lg = _generic(N=64, NQ=2)
    else:
        c = mla.make_case(mla.Shape(H=2, Hkv=1, NQ=2, N=64), mask="random")
        lg = bv.from_mla(mla.MlaLaunch(c, "head", "view128"))
        m = c.ref.mask
        lg.mask = np.ascontiguousarray(as_strided(m.data[m.off:].view(np.uint16), shape=(1, 1, m.ne[1], m.ne[0]),
                                                  strides=(0, 0, m.nb[1], 2)))
    row = lg.mask.shape[3] * 2

    def build(x):
        lay = bv.layout(lg, m_nb=(SPAN_MAX - row + x, None, None))
        assert lay.t["mask"].span == SPAN_MAX + x
        return lay
    _accept_reject(build)


@pytest.mark.parametrize("path", ["generic", "mla"])
def test_q_span_limit(path):
    """q_span = (n_q - 1) nb[1] + (H - 1) nb[2] + 4 D at the limit (one query row, two heads)."""
    lg = _generic(N=64, NQ=1, H=2, Hkv=1) if path == "generic" else _mla_f16("view128")
    row = lg.dq * 4
    _accept_reject(lambda x: bv.layout(lg, q_nb=(None, SPAN_MAX - row + x, None)))


def test_mask_head_plane_limit():
    """The split kernel's head-plane rule: m_span_h + m_span + 64 just inside the limit plans, just outside is BAD_STRIDE."""
    case = next(c for c in bv.CASES if c.tag == "C-mask-planes-split")
    lg = bv.logical(case)[0]
    nb2 = dict(case.big)["m_nb"][1]
    m_span = lg.mask.shape[3] * 2
    assert 3 * nb2 + 2 * m_span + 64 <= SPAN_MAX < 3 * (nb2 + 16) + 2 * m_span + 64
    assert _status(bv.layout(lg, m_nb=(None, nb2, None)))[0] == 0
    assert _status(bv.layout(lg, m_nb=(None, nb2 + 16, None)))[0] == BAD_STRIDE


# ------------------------------------------------------------------ the tail-tile rule

@pytest.mark.parametrize("kt,n", [("f16", 77), ("f16", 65), ("q8_0", 77), ("q5_1", 95), ("bf16", 1)])
def test_tail_tile_rule(kt, n):
    """The split kernel fetches whole 32-key steps and forms the offsets of the
    rows past N like any other: the planner holds the span of N ROUNDED UP to the
    step to the limit.  The largest such nb[1] plans and no row of the last step
    wraps; one stride step more is FATTN_ERR_BAD_STRIDE although k_span itself
    is then still (Nr - N) nb[1] bytes below the limit -- for K alone, V alone
    and both."""
    lg = _blank(kt, n)
    row = lg.k_rows.shape[3]
    nr = (n + 31) // 32 * 32
    al = 16 if kt in ("f16", "bf16") else 4
    nb1 = bv.nb1_for_span(SPAN_MAX, nr, row, al)
    for which in ("k", "v", "kv"):
        def lay(step):
            st = (nb1 + step, None, None)
            return bv.layout(lg, k_nb=st if "k" in which else None, v_nb=st if "v" in which else None, v_in_k="kv" == which)
        code, d = _status(lay(0))
        assert code == 0 and bv.tail_tile(d) == 32, d
        assert not bv.wraps(lay(0), which[0], 32)
        assert _status(lay(al))[0] == BAD_STRIDE
        assert lay(al).t[which[0]].span <= SPAN_MAX - (nr - n) * nb1 + al * n


def test_contiguous_quantised_rows_wrap_only_past_31_million():
    """Contiguous Q8_0 rows (the 16-byte path: nb[1] == row, N % 32 == 0) have no
    tail rows; on the dword path the rule needs N * 136 bytes near 4 GiB, about
    31.6 million rows -- planned here, not run."""
    n = SPAN_MAX // 136          # the most rows one plane holds: 31 580 641, one past a multiple of 32
    assert n % 32 == 1
    lg = bv.Logical(np.zeros((1, 1, 1, 128), dtype=np.float32), fattn.TYPE_Q8_0, np.zeros((1, 1, 1, 136), dtype=np.uint8),
                    fattn.TYPE_Q8_0, np.zeros((1, 1, 1, 136), dtype=np.uint8), 128, None, 0.125)

    def status(rows):
        lay = bv.layout(lg)
        for x in (lay.t["k"], lay.t["v"]):
            x.ne = (128, rows, 1, 1)
        return _status(lay)[0]
    assert (n - 1) * 136 + 136 <= SPAN_MAX < ((n + 31) // 32 * 32) * 136
    assert status(n) == BAD_STRIDE
    assert status(n - 1) == 0 and status(n - 28) == 0
