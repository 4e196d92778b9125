#!/usr/bin/env python3
"""fattn_set_rows against fattn_cpy: the KV-cache write, timed.

Both calls convert the same f32 source into the same contiguous destination --
fattn_set_rows with slots arange(nr), fattn_cpy into the view of those slots --
in one process, in alternating rounds, both warmed up.  A round of one call is
a window of at least --window seconds of back-to-back launches between two
device events; the launches of a window are replayed from a captured graph of
--graph launches (--graph 0: plain launches from Python, whose enqueue cost
then bounds the small shapes).  Per case: the median time per launch of each
call over the rounds, the spread (min .. max over rounds), the achieved bytes/s
from the traffic model -- per row ne0 * 4 (+ the index for set_rows) read and
row_size written -- and whether set_rows is no slower than cpy by more than the
spread seen in this run.  The two outputs are compared byte for byte at the
timed sizes.  The copy ceiling is tools/hbm_copy.hip's probe on the same device.

    python tools/bench_set_rows.py [--out FILE] [--rounds 7] [--window 0.2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-cuda-experiments_amd"))

import fattn  # noqa: E402

# (name, nr, ne0, ne2, cache layout, gated): user sizes
CASES = (
    ("decode 1 x 1024", 1, 1024, 1, "pos", False),
    ("512 x 1024", 512, 1024, 1, "pos", True),
    ("4096 x 4096", 4096, 4096, 1, "pos", True),
    ("512 x 8 heads x 128 [Hkv][N][row]", 512, 128, 8, "head", True),
)
TYPES = ("f16", "q8_0", "q4_0", "q5_1")


def copy_ceiling():
    path = os.path.join(ROOT, "ggml-cuda-experiments_amd", "lib", "libhbmcopy.so")
    if not os.path.exists(path):
        return None
    L = C.CDLL(path)
    L.hbm_probe.restype = C.c_int
    L.hbm_probe.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    cp, rd = C.c_float(), C.c_float()
    if L.hbm_probe(1 << 30, 10, C.byref(cp), C.byref(rd)) != 0:
        return None
    return cp.value


class Call:
    """One of the two writes with its own destination; run(n) enqueues n launches."""

    def __init__(self, torch, fn, args, stream, graph_len):
        self.torch, self.fn, self.args, self.stream = torch, fn, args, stream
        self.graph, self.graph_len = None, graph_len
        self.launch()
        torch.cuda.synchronize()
        if graph_len:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=stream):
                for _ in range(graph_len):
                    self.launch()
            torch.cuda.synchronize()

    def launch(self):
        rc = self.fn(*self.args, self.stream.cuda_stream)
        if rc:
            raise fattn.FattnError(rc, self.fn.__name__)

    def window(self, n):
        """ms per launch over >= n launches between two events."""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record(self.stream)
            if self.graph is not None:
                reps = max(1, -(-n // self.graph_len))
                for _ in range(reps):
                    self.graph.replay()
                n = reps * self.graph_len
            else:
                for _ in range(n):
                    self.launch()
            e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n


def bench_case(torch, L, dev, stream, tname, nr, ne0, ne2, layout, rounds, window, graph_len):
    typ = fattn.TYPE_NAMES[tname]
    rb = fattn.row_size(typ, ne0)
    eb = 2 if typ == fattn.TYPE_F16 else fattn.BLOCK_BYTES[typ]
    g = torch.Generator(device="cpu").manual_seed(nr + ne0)
    src = (3.0 * (1.0 - 2.0 * torch.rand((nr, ne2, ne0), generator=g, dtype=torch.float32))).to(dev)  # k_cur: token-major
    idx = torch.arange(nr, dtype=torch.int64, device=dev)
    dsts = [torch.zeros(nr * ne2 * rb, dtype=torch.uint8, device=dev) for _ in range(2)]
    dnb = (eb, rb * ne2, rb, rb * ne2 * nr) if layout == "pos" else (eb, rb, rb * nr, rb * nr * ne2)
    sv = fattn.View(src.data_ptr(), fattn.TYPE_F32, (ne0, nr, ne2, 1), (4, ne2 * ne0 * 4, ne0 * 4, nr * ne2 * ne0 * 4)).c()
    iv = fattn.View(idx.data_ptr(), fattn.TYPE_I64, (nr, 1, 1, 1), (8, 8 * nr, 8 * nr, 8 * nr)).c()
    dv = [fattn.View(d.data_ptr(), typ, (ne0, nr, ne2, 1), dnb).c() for d in dsts]
    with torch.cuda.stream(stream):
        calls = {"cpy": Call(torch, L.fattn_cpy, (C.byref(sv), C.byref(dv[0])), stream, graph_len),
                 "set_rows": Call(torch, L.fattn_set_rows, (C.byref(sv), C.byref(iv), C.byref(dv[1])), stream, graph_len)}
    torch.cuda.synchronize()
    same = bool(torch.equal(dsts[0], dsts[1]))
    n = {}
    for k, c in calls.items():          # warm up, and size the window
        c.window(50)
        n[k] = max(50, int(window * 1e3 / max(c.window(200), 1e-4)) + 1)
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():      # alternating
            t[k].append(c.window(n[k]))
    torch.cuda.synchronize()
    same = same and bool(torch.equal(dsts[0], dsts[1]))
    rows = nr * ne2
    model = {"cpy": rows * (ne0 * 4 + rb), "set_rows": rows * (ne0 * 4 + 8 + rb)}
    out = {"same_bytes": same}
    for k in calls:
        med = statistics.median(t[k])
        out[k] = {"median_us": med * 1e3, "min_us": min(t[k]) * 1e3, "max_us": max(t[k]) * 1e3,
                  "gbs": model[k] / (med * 1e-3) / 1e9, "launches_per_window": n[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--graph", type=int, default=20, help="launches per captured graph; 0 = plain launches")
    ap.add_argument("--types", default=",".join(TYPES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_set_rows: needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    L = fattn.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"fattn_set_rows vs fattn_cpy on {torch.cuda.get_device_name(0)}; {fattn.lib().fattn_version().decode()}")
    say(f"rounds {a.rounds} (alternating), window >= {a.window} s, "
        f"{'graphs of %d launches' % a.graph if a.graph else 'plain launches from Python'}; times per launch, "
        "median [min .. max] over rounds")
    say("traffic model per row: ne0*4 (+8 index bytes, set_rows) read, row_size written")
    peak = copy_ceiling()
    say(f"copy ceiling (tools/hbm_copy.hip, dwordx4 copy of 1 GiB, read + written): "
        f"{'%.0f GB/s' % peak if peak else 'not measured'}")
    stream = torch.cuda.Stream()
    all_ok = True
    for cname, nr, ne0, ne2, layout, gated in CASES:
        say()
        say(f"== {cname}{'' if gated else '   (launch-bound: reported, not gated)'}")
        for tname in a.types.split(","):
            r = bench_case(torch, L, dev, stream, tname, nr, ne0, ne2, layout, a.rounds, a.window, a.graph)
            c, s = r["cpy"], r["set_rows"]
            spread = max(c["max_us"] - c["min_us"], s["max_us"] - s["min_us"])
            ok = s["median_us"] <= c["median_us"] + spread
            verdict = ("no slower" if ok else "SLOWER") if gated else "-"
            all_ok = all_ok and (ok or not gated) and r["same_bytes"]
            say(f"{tname:5s} cpy {c['median_us']:9.2f} us [{c['min_us']:9.2f} .. {c['max_us']:9.2f}] {c['gbs']:8.1f} GB/s | "
                f"set_rows {s['median_us']:9.2f} us [{s['min_us']:9.2f} .. {s['max_us']:9.2f}] {s['gbs']:8.1f} GB/s | "
                f"x{c['median_us'] / s['median_us']:.2f} spread {spread:.2f} us {verdict} | "
                f"bytes {'equal' if r['same_bytes'] else 'DIFFER'}")
    say()
    say("all gated cases no slower than fattn_cpy, outputs equal" if all_ok else "SOME CASE MISSED (see above)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
