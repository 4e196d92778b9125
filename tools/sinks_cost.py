#!/usr/bin/env python3
"""What a live attention sink costs (diagnostic; profiles/sinks/cost.json).

fattn_ext_sinks has no events variant, so both variants of a shape -- off
(fattn_ext) and sinks (fattn_ext_sinks, ln N + U[-2, 3] per head) -- are timed
alike: torch events on the launch stream around --batch back-to-back launches
(every kernel of the plan, launch overhead included), per-launch average; the
variants alternate inside every round, so box drift hits them alike.  The
config-3 decode shape and the D = 128 f16 prefill shape.  Prints one JSON object.

  python tools/sinks_cost.py [--rounds 20] [--batch 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-cuda-experiments_amd"))
sys.path.insert(0, ROOT)

SHAPES = {
    "config3": dict(kv_type="q8_0", H=32, Hkv=32, N=4096, NQ=1, D=128),
    "prefill_f16": dict(kv_type="f16", H=32, Hkv=32, N=4096, NQ=4096, D=128),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    import torch
    import fattn

    dev = torch.device("cuda", 0)
    out = {"what": "torch events around --batch back-to-back launches, per-launch us, median over --rounds; off = fattn_ext, "
                   "sinks = fattn_ext_sinks with ln N + U[-2, 3] per head; variants alternating; random f16 mask",
           "rounds": args.rounds, "batch": args.batch, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, sh in SHAPES.items():
        D, H, Hkv, N, NQ = sh["D"], sh["H"], sh["Hkv"], sh["N"], sh["NQ"]
        typ = fattn.TYPE_NAMES[sh["kv_type"]]
        g = torch.Generator(device=dev)
        g.manual_seed(99)
        kv = []
        for _ in range(2):
            x = torch.rand((Hkv * N, D), generator=g, device=dev) * 2 - 1
            kv.append(x.to(torch.float16).view(torch.uint8).reshape(-1) if typ == fattn.TYPE_F16
                      else fattn.quantize(x, typ).reshape(-1))
        q = torch.rand((1, NQ, H, D), generator=g, device=dev) * 2 - 1
        mask = (torch.rand((NQ, (N + 63) // 64 * 64), generator=g, device=dev) * 2 - 1).to(torch.float16)
        sinks = math.log(N) + torch.rand((H,), generator=g, device=dev) * 5 - 2
        dst = torch.empty((1, NQ, H, D), dtype=torch.float32, device=dev)
        atts = {v: fattn.Attention(fattn.q_view(q), fattn.kv_view(kv[0], typ, D, N, Hkv), fattn.kv_view(kv[1], typ, D, N, Hkv),
                                   fattn.mask_view(mask), dst, 1.0 / D ** 0.5, sinks=s)
                for v, s in (("off", None), ("sinks", sinks))}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {v: [] for v in atts}
        for r in range(args.rounds + 3):
            for v, att in atts.items():
                e0.record()
                for _ in range(args.batch):
                    att()
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:                                    # (three warm-up rounds)
                    times[v].append(e0.elapsed_time(e1) * 1e3 / args.batch)
        out["shapes"][name] = {"shape": sh, "plan": atts["off"].describe(), "variants": {
            v: {"median_us": round(statistics.median(t), 3), "min_us": round(min(t), 3), "max_us": round(max(t), 3)}
            for v, t in times.items()}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
