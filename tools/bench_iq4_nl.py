#!/usr/bin/env python3
"""Split decode over an IQ4_NL cache against Q4_0 at BASELINE config 4's shape (H 32 over 8 KV heads, N 8192, D 128;
diagnostic).  R rotated K / V caches per type (>= 512 MB per pass) hold fattn.quantize of the same values; the types
alternate round by round in one process, `steps` launches per captured HIP graph, HIP events around the replay.

  python tools/bench_iq4_nl.py --rounds 9 --steps 55 --json profiles/kv_types/bench_iq4_nl.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ggml-cuda-experiments_amd"), ROOT]
H, HKV, N, D = 32, 8, 8192, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=55)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    import fattn
    from bench import hip_events
    dev = torch.device("cuda", 0)
    hip, evs = hip_events(2)
    gs = torch.cuda.Stream(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    types = {"q4_0": fattn.TYPE_Q4_0, "iq4_nl": fattn.TYPE_IQ4_NL}
    stored = 2 * HKV * N * fattn.row_size(fattn.TYPE_Q4_0, D)
    R = -(-(512 << 20) // stored)
    caches = {t: [] for t in types}
    for _ in range(R):
        k, v = (torch.randn((HKV * N, D), generator=g, device=dev) for _ in range(2))
        for t, ty in types.items():
            caches[t].append((fattn.quantize(k, ty), fattn.quantize(v, ty)))
    q = torch.randn((1, 1, H, D), generator=g, device=dev)
    mask = (torch.rand((1, N), generator=g, device=dev) * 2 - 1).to(torch.float16)
    outs = torch.empty((R, 1, 1, H, D), dtype=torch.float32, device=dev)
    graphs, us = {}, {t: [] for t in types}
    for t, ty in types.items():
        kv = caches[t]
        att = fattn.Attention(fattn.q_view(q), fattn.kv_view(kv[0][0], ty, D, N, HKV), fattn.kv_view(kv[0][1], ty, D, N, HKV),
                              fattn.mask_view(mask), outs[0], D ** -0.5)

        def step(i, att=att, kv=kv):
            att.retarget(k=kv[i % R][0].data_ptr(), v=kv[i % R][1].data_ptr(), dst=outs[i % R].data_ptr())
            att()

        gs.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(gs):
            for i in range(4):
                step(i)
        torch.cuda.synchronize()
        graphs[t] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[t], stream=gs):
            for i in range(args.steps):
                step(i)
        print(f"# {t}: {att.describe()}", flush=True)
    f = C.c_float()
    for r in range(args.rounds):
        for t, gr in graphs.items():
            with torch.cuda.stream(gs):
                gr.replay()
            torch.cuda.synchronize()
            hip.hipEventRecord(evs[0], gs.cuda_stream)
            with torch.cuda.stream(gs):
                gr.replay()
            hip.hipEventRecord(evs[1], gs.cuda_stream)
            torch.cuda.synchronize()
            hip.hipEventElapsedTime(C.byref(f), evs[0], evs[1])
            us[t].append(round(f.value * 1e3 / args.steps, 3))
    res = [dict(type=t, median_us=statistics.median(v), rounds_us=v, steps=args.steps, rotated_caches=R, stored_bytes=stored)
           for t, v in us.items()]
    for rec in res:
        print(json.dumps(rec), flush=True)
    print(f"iq4_nl / q4_0 = {res[1]['median_us'] / res[0]['median_us']:.3f}", flush=True)
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
