#!/usr/bin/env python3
"""fattn_k_shift against the cast round trip the parent library could do: timed.

Nothing before fattn_k_shift performs the K-shift, so there is no pass / fail
time; the yardstick is fattn_dequantize followed by fattn_quantize over the same
contiguous rows -- llama.cpp's cast to f32 and back WITHOUT any rotation, through
an f32 temporary of the whole cache.  Shape: n_slots 32768, Hkv 8, ne0 = n_dims =
128, NEOX, every shift -256, a [Hkv][N][row] cache of Q8_0, F16 and Q5_1.

Three calls per type in one process, in alternating rounds, all replayed from
captured graphs: the round trip (two launches), fattn_k_shift over the view
[128, N, 8, 1] (its lane groups walk the 8 heads of a slot with one set of
angles) and fattn_k_shift over the same bytes seen as [128, N, 1, 8] (eight
sequences of one head sharing one shift plane: every lane group computes its
own angles) -- the form WITHOUT head sharing, measured without a build switch.
Per call: the median time per launch over the rounds with the round-to-round
range, and the model GB/s -- cache bytes read and written plus the shift words
(round trip: plus the f32 temporary written and read).  The copy ceiling is
tools/hbm_copy.hip's probe in the same run.

    python tools/bench_k_shift.py [--out FILE] [--rounds 7] [--window 0.2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-cuda-experiments_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fattn  # noqa: E402
from bench_set_rows import copy_ceiling  # noqa: E402

TYPES = ("q8_0", "f16", "q5_1")
N_SLOTS, HKV, NE0, SHIFT = 32768, 8, 128, -256


class Graph:
    """`launch(stream handle)` (one or more library calls) captured `graph_len` times; window(n): ms per launch."""

    def __init__(self, torch, launch, stream, graph_len):
        self.torch, self.stream, self.graph_len = torch, stream, graph_len
        with torch.cuda.stream(stream):
            launch(stream.cuda_stream)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=stream):
                for _ in range(graph_len):
                    launch(stream.cuda_stream)
        torch.cuda.synchronize()

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


def check(rc, what):
    if rc:
        raise fattn.FattnError(rc, what)


def bench_type(torch, L, dev, stream, tname, rounds, window, graph_len):
    typ = fattn.TYPE_NAMES[tname]
    rb, eb = fattn.row_size(typ, NE0), fattn.elem_bytes(typ)
    rows = N_SLOTS * HKV
    g = torch.Generator(device="cpu").manual_seed(7)
    x = (1.0 - 2.0 * torch.rand((rows, NE0), generator=g, dtype=torch.float32)).to(dev)
    cache0 = fattn.quantize(x, typ) if typ != fattn.TYPE_F16 else x.to(torch.float16).view(torch.uint8).reshape(rows, rb)
    caches = {k: cache0.clone() for k in ("round trip", "k_shift, heads walked", "k_shift, heads on the grid")}
    tmp = torch.empty((rows, NE0), dtype=torch.float32, device=dev)
    shift = torch.full((N_SLOTS,), SHIFT, dtype=torch.int32, device=dev)
    sv = fattn.View(shift.data_ptr(), fattn.TYPE_I32, (N_SLOTS, 1, 1, 1), (4, 4 * N_SLOTS, 4 * N_SLOTS, 4 * N_SLOTS)).c()
    rope = fattn.rope_params(NE0, fattn.ROPE_NEOX)
    plane = rb * N_SLOTS
    walked = fattn.View(caches["k_shift, heads walked"].data_ptr(), typ, (NE0, N_SLOTS, HKV, 1), (eb, rb, plane, plane * HKV)).c()
    on_grid = fattn.View(caches["k_shift, heads on the grid"].data_ptr(), typ, (NE0, N_SLOTS, 1, HKV), (eb, rb, plane * HKV, plane)).c()
    rt = caches["round trip"].data_ptr()

    def round_trip(s):
        check(L.fattn_dequantize(typ, rt, tmp.data_ptr(), NE0, rows, s), "fattn_dequantize")
        if typ == fattn.TYPE_F16:   # (fattn_quantize has no F16 form: the cast back is fattn_cpy)
            a = fattn.View(tmp.data_ptr(), fattn.TYPE_F32, (NE0, rows, 1, 1), (4, NE0 * 4, NE0 * 4 * rows, NE0 * 4 * rows)).c()
            b = fattn.View(rt, typ, (NE0, rows, 1, 1), (2, rb, rb * rows, rb * rows)).c()
            check(L.fattn_cpy(C.byref(a), C.byref(b), s), "fattn_cpy")
        else:
            check(L.fattn_quantize(typ, tmp.data_ptr(), rt, NE0, rows, s), "fattn_quantize")

    calls = {
        "round trip": Graph(torch, round_trip, stream, graph_len),
        "k_shift, heads walked": Graph(torch, lambda s: check(L.fattn_k_shift(C.byref(walked), C.byref(sv), None, C.byref(rope), s), "fattn_k_shift"), stream, graph_len),
        "k_shift, heads on the grid": Graph(torch, lambda s: check(L.fattn_k_shift(C.byref(on_grid), C.byref(sv), None, C.byref(rope), s), "fattn_k_shift"), stream, graph_len),
    }
    same = bool(torch.equal(caches["k_shift, heads walked"], caches["k_shift, heads on the grid"]))   # (one eager launch each)
    n = {}
    for k, c in calls.items():
        c.window(graph_len)
        n[k] = max(graph_len, int(window * 1e3 / max(c.window(2 * graph_len), 1e-4)) + 1)
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():      # alternating
            t[k].append(c.window(n[k]))
    torch.cuda.synchronize()
    cache_bytes = rows * rb
    model = {k: 2 * cache_bytes + 4 * N_SLOTS for k in calls}
    model["round trip"] = 2 * cache_bytes + 2 * rows * NE0 * 4
    out = {"same_bytes": same, "cache_bytes": cache_bytes}
    for k in calls:
        med = statistics.median(t[k])
        out[k] = {"median_us": med * 1e3, "min_us": min(t[k]) * 1e3, "max_us": max(t[k]) * 1e3,
                  "gbs": model[k] / (med * 1e-3) / 1e9, "model_bytes": model[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--graph", type=int, default=10, help="launches per captured graph")
    ap.add_argument("--types", default=",".join(TYPES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_k_shift: needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    L = fattn.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"fattn_k_shift vs fattn_dequantize + fattn_quantize on {torch.cuda.get_device_name(0)}; {L.fattn_version().decode()}")
    say(f"n_slots {N_SLOTS}, Hkv {HKV}, ne0 = n_dims = {NE0}, NEOX, every shift {SHIFT}, [Hkv][N][row]; rounds {a.rounds} "
        f"(alternating), window >= {a.window} s, graphs of {a.graph} launches; times per call, median [min .. max] over rounds")
    say("model bytes: cache read + written + shift words (round trip: + the f32 temporary written and read)")
    peak = copy_ceiling()
    say(f"copy ceiling (tools/hbm_copy.hip, dwordx4 copy of 1 GiB, read + written): {'%.0f GB/s' % peak if peak else 'not measured'}")
    stream = torch.cuda.Stream()
    all_ok = True
    for tname in a.types.split(","):
        r = bench_type(torch, L, dev, stream, tname, a.rounds, a.window, a.graph)
        say()
        say(f"== {tname}: cache {r['cache_bytes'] / 2 ** 20:.1f} MiB")
        for k in ("round trip", "k_shift, heads walked", "k_shift, heads on the grid"):
            c = r[k]
            say(f"  {k:27s} {c['median_us']:9.2f} us [{c['min_us']:9.2f} .. {c['max_us']:9.2f}]  {c['gbs']:8.1f} GB/s of "
                f"{c['model_bytes'] / 2 ** 20:.1f} MiB")
        rt, w, gr = r["round trip"], r["k_shift, heads walked"], r["k_shift, heads on the grid"]
        spread = max(x["max_us"] - x["min_us"] for x in (rt, w))
        ok = w["median_us"] <= rt["median_us"] + spread
        all_ok = all_ok and ok and r["same_bytes"]
        say(f"  fused (heads walked) vs round trip: x{rt['median_us'] / w['median_us']:.2f}, larger range {spread:.2f} us: "
            f"{'no slower' if ok else 'SLOWER'}; heads walked vs on the grid: x{gr['median_us'] / w['median_us']:.2f}; "
            f"the two forms' bytes {'equal' if r['same_bytes'] else 'DIFFER'}")
    say()
    say("the fused op is no slower than the two-launch round trip on every type" if all_ok else "SOME TYPE MISSED (see above)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
