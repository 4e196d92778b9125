#!/usr/bin/env python3
"""What max_bias / logit_softcap cost (diagnostic; profiles/op_params/cost.json).

fattn_ext_events medians -- HIP events around the main kernel, recorded by the
library on the launch stream -- on the config-3 decode shape and on the D = 128
f16 prefill shape, with both parameters off, with logit_softcap and with
max_bias.  The three variants of a shape alternate inside every round, so box
drift hits them alike.  Prints one JSON object.

  python tools/op_params_cost.py [--rounds 30]
"""
import argparse
import ctypes as C
import json
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
VARIANTS = {"off": {}, "softcap": dict(logit_softcap=30.0), "alibi": dict(max_bias=8.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    import torch
    import fattn
    from bench import hip_events

    dev = torch.device("cuda", 0)
    hip, evs = hip_events(2)
    f = C.c_float()
    out = {"what": "fattn_ext_events (main kernel, HIP events) median us over --rounds launches per variant, "
                   "variants alternating; random f16 mask; softcap = logit_softcap 30, alibi = max_bias 8",
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
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
        dst = torch.empty((1, NQ, H, D), dtype=torch.float32, device=dev)
        atts = {v: fattn.Attention(fattn.q_view(q), fattn.kv_view(kv[0], typ, D, N, Hkv), fattn.kv_view(kv[1], typ, D, N, Hkv),
                                   fattn.mask_view(mask), dst, 1.0 / D ** 0.5, **kw) for v, kw in VARIANTS.items()}
        times = {v: [] for v in VARIANTS}
        for r in range(args.rounds + 3):
            for v, att in atts.items():
                att(ev_begin=evs[0], ev_end=evs[1])
                torch.cuda.synchronize()
                hip.hipEventElapsedTime(C.byref(f), evs[0], evs[1])
                if r >= 3:                                    # (three warm-up rounds)
                    times[v].append(f.value * 1e3)
        out["shapes"][name] = {"shape": sh, "variants": {
            v: {"plan": atts[v].describe(), "median_us": round(statistics.median(t), 3), "min_us": round(min(t), 3),
                "max_us": round(max(t), 3)} for v, t in times.items()}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
