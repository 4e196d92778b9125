#!/usr/bin/env python3
"""fattn_rope_set_rows against what the library offered before it, timed.

The job: nr tokens x 8 KV heads x 128 of f32 k_cur / v_cur (token-major, as
llama.cpp has them) into [Hkv][N][row] caches of 4096 slots, K rotated (NEOX,
n_dims 128) by the tokens' positions.  Three contenders in one process:

    fused   one fattn_rope_set_rows
    (A)     fattn_set_rows K + fattn_set_rows V: two launches, NO rotation
    (B)     (A) + fattn_k_shift over the K cache with the positions as deltas
            (zeros on the slots not written): three launches, K quantised twice

in alternating rounds, all warmed up.  A round of one contender is a window of
at least --window seconds of back-to-back replays of a captured graph of --graph
repetitions between two device events.  Per case: the median time per
repetition over the rounds and the round-to-round range.  Gates: fused no slower
than (A) at nr = 1 and 64 (launch-bound: one launch against two), no slower than
(B) at nr = 4096 (the rotation is real work there, so the opponent rotates too);
the margin is the larger of the two ranges.  The ratio to (A) at 4096 is the
price of the rotation: reported, not gated.  At every timed size V's bytes are
compared with (A)'s and K's bytes of a rope-less fused launch with (A)'s K.

    python tools/bench_rope_set_rows.py [--out FILE] [--rounds 7] [--window 0.2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-cuda-experiments_amd"))

import fattn  # noqa: E402

HKV, D, N_SLOTS = 8, 128, 4096
NRS = (1, 64, 4096)
PAIRS = (("f16", "f16"), ("q8_0", "q8_0"), ("q4_0", "q4_0"), ("q5_1", "q5_1"), ("q8_0", "q4_0"))


class Seq:
    """A sequence of launches [(fn, args)]; window(n): ms per repetition over >= n of them, replayed from a graph."""

    def __init__(self, torch, steps, stream, graph_len):
        self.torch, self.steps, self.stream, self.graph_len = torch, steps, stream, graph_len
        self.launch()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=stream):
            for _ in range(graph_len):
                self.launch()
        torch.cuda.synchronize()

    def launch(self):
        for fn, args in self.steps:
            rc = fn(*args, self.stream.cuda_stream)
            if rc:
                raise fattn.FattnError(rc, fn.__name__)

    def window(self, n):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(1, -(-n // self.graph_len))
        with torch.cuda.stream(self.stream):
            e0.record(self.stream)
            for _ in range(reps):
                self.graph.replay()
            e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / (reps * self.graph_len)


def bench_case(torch, L, dev, stream, kname, vname, nr, rounds, window, graph_len):
    kt, vt = fattn.TYPE_NAMES[kname], fattn.TYPE_NAMES[vname]
    g = torch.Generator(device="cpu").manual_seed(nr)
    rnd = lambda: (3.0 * (1.0 - 2.0 * torch.rand((nr, HKV, D), generator=g, dtype=torch.float32))).to(dev)  # token-major
    k_cur, v_cur = rnd(), rnd()
    idx = torch.arange(nr, dtype=torch.int64, device=dev)
    pos = torch.arange(1000, 1000 + nr, dtype=torch.int32, device=dev)
    shift = torch.zeros(N_SLOTS, dtype=torch.int32, device=dev)
    shift[:nr] = pos

    def cache(typ):
        rb = fattn.row_size(typ, D)
        buf = torch.zeros(HKV * N_SLOTS * rb, dtype=torch.uint8, device=dev)
        return buf, fattn.View(buf.data_ptr(), typ, (D, N_SLOTS, HKV, 1), (fattn.elem_bytes(typ), rb, rb * N_SLOTS, rb * N_SLOTS * HKV)).c()

    src = lambda t: fattn.View(t.data_ptr(), fattn.TYPE_F32, (D, nr, HKV, 1), (4, HKV * D * 4, D * 4, nr * HKV * D * 4)).c()
    ks_, vs = src(k_cur), src(v_cur)
    iv = fattn.View(idx.data_ptr(), fattn.TYPE_I64, (nr, 1, 1, 1), (8, 8 * nr, 8 * nr, 8 * nr)).c()
    pv = fattn.View(pos.data_ptr(), fattn.TYPE_I32, (nr, 1, 1, 1), (4, 4 * nr, 4 * nr, 4 * nr)).c()
    sv = fattn.View(shift.data_ptr(), fattn.TYPE_I32, (N_SLOTS, 1, 1, 1), (4, 4 * N_SLOTS, 4 * N_SLOTS, 4 * N_SLOTS)).c()
    rope = fattn.rope_params(D, fattn.ROPE_NEOX)
    bufs = {n: (cache(kt), cache(vt)) for n in ("fused", "A", "B", "plain")}
    ref = C.byref
    fused = lambda n, rp: (L.fattn_rope_set_rows, (ref(ks_), ref(pv), ref(iv), ref(bufs[n][0][1]), None, rp, ref(vs), ref(bufs[n][1][1])))
    two = lambda n: [(L.fattn_set_rows, (ref(ks_), ref(iv), ref(bufs[n][0][1]))), (L.fattn_set_rows, (ref(vs), ref(iv), ref(bufs[n][1][1])))]
    with torch.cuda.stream(stream):
        seqs = {"fused": Seq(torch, [fused("fused", ref(rope))], stream, graph_len),
                "A": Seq(torch, two("A"), stream, graph_len),
                "B": Seq(torch, two("B") + [(L.fattn_k_shift, (ref(bufs["B"][0][1]), ref(sv), None, ref(rope)))], stream, graph_len)}
        Seq(torch, [fused("plain", None)], stream, 1)
    torch.cuda.synchronize()
    n = {}
    for k, s in seqs.items():          # warm up, and size the window
        s.window(50)
        n[k] = max(50, int(window * 1e3 / max(s.window(200), 1e-4)) + 1)
    t = {k: [] for k in seqs}
    for _ in range(rounds):
        for k, s in seqs.items():      # alternating
            t[k].append(s.window(n[k]))
    torch.cuda.synchronize()
    same = (torch.equal(bufs["fused"][1][0], bufs["A"][1][0]) and torch.equal(bufs["plain"][0][0], bufs["A"][0][0]) and
            torch.equal(bufs["plain"][1][0], bufs["A"][1][0]) and not torch.equal(bufs["fused"][0][0], bufs["A"][0][0]))
    out = {"same_bytes": bool(same)}
    for k in seqs:
        out[k] = {"median_us": statistics.median(t[k]) * 1e3, "min_us": min(t[k]) * 1e3, "max_us": max(t[k]) * 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--graph", type=int, default=20, help="repetitions per captured graph")
    ap.add_argument("--nrs", default=",".join(str(n) for n in NRS), help="token counts to time")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rope_set_rows: needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    L = fattn.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"fattn_rope_set_rows vs set_rows x 2 (A) and set_rows x 2 + k_shift (B) on {torch.cuda.get_device_name(0)}; "
        f"{L.fattn_version().decode()}")
    say(f"{HKV} heads x {D}, [Hkv][N][row] caches of {N_SLOTS} slots, NEOX n_dims {D}; rounds {a.rounds} (alternating), "
        f"window >= {a.window} s, graphs of {a.graph} repetitions; us per repetition, median [min .. max] over rounds")
    stream = torch.cuda.Stream()
    all_ok = True
    for nr in (int(n) for n in a.nrs.split(",")):
        opp = "B" if nr == 4096 else "A"
        say()
        say(f"== nr = {nr}: gated against ({opp})")
        for kname, vname in PAIRS:
            r = bench_case(torch, L, dev, stream, kname, vname, nr, a.rounds, a.window, a.graph)
            f, o = r["fused"], r[opp]
            spread = max(f["max_us"] - f["min_us"], o["max_us"] - o["min_us"])
            ok = f["median_us"] <= o["median_us"] + spread
            all_ok = all_ok and ok and r["same_bytes"]
            cell = lambda c: f"{c['median_us']:8.2f} [{c['min_us']:8.2f} .. {c['max_us']:8.2f}]"
            say(f"{kname + '/' + vname:11s} fused {cell(f)} | A {cell(r['A'])} | B {cell(r['B'])} | fused/A {f['median_us'] / r['A']['median_us']:.2f} "
                f"fused/B {f['median_us'] / r['B']['median_us']:.2f} | margin {spread:.2f} us {'no slower' if ok else 'SLOWER'} than {opp} | "
                f"bytes {'equal' if r['same_bytes'] else 'DIFFER'}")
    say()
    say("every gate met, outputs equal" if all_ok else "SOME CASE MISSED (see above)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
