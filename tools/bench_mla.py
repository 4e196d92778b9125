#!/usr/bin/env python3
"""Timing of the MLA decode kernel (K dim 576, V dim 512; diagnostic).

For every shape the workload is built once -- R rotated f16 caches of
[S][N][576] rows (>= 512 MB per pass over them, so no launch finds its rows in
the Infinity Cache), one Q, one [1][N] mask -- and two forms of the same data
are timed in turn, round after round, in one process:

  view   V = the cache rows from byte 128 on (fattn.mla_v_view: each row read once)
  own    V = a separate [S][N][512] buffer holding the same values

K launches captured in one HIP graph, HIP events around the replay on the launch
stream, kernel (+ merge launch) time per step; median over the rounds with the
round-to-round range.  The roofline fractions are of 8 TB/s over the
algorithmic bytes (Q, the cache rows once, the mask, dst) and of 2.5 PFLOP/s
over 2 * S * H * N * (576 + 512) flops.

  python tools/bench_mla.py --rounds 7 --steps 50 --json profiles/mla/bench.json

--kv-type q8_0 / q4_0 (repeatable) times the f16 view form against the same
rows quantised (fattn.quantize; V the view two blocks in), alternating in the
same way, instead of view against own.  R then comes from the smallest cache
among the forms, every form rotates over the same R, and each record carries
`stored_bytes` (the cache rows as stored: 1152 / 612 / 324 B each) with its
fraction of 8 TB/s, `hbm_frac_stored`, next to the algorithmic figures.

  python tools/bench_mla.py --kv-type q8_0 --kv-type q4_0 --json profiles/mla_quant/bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-cuda-experiments_amd"))
sys.path.insert(0, ROOT)

SHAPES = {
    "v3_batch32": dict(H=128, N=4096, S=32),    # one decode step of 32 sequences
    "v3_single": dict(H=128, N=4096, S=1),      # the same, one sequence: latency-bound
    "lite_batch32": dict(H=16, N=4096, S=32),   # V2-Lite
    "lite_single": dict(H=16, N=4096, S=1),
}
HBM_BPS, MFMA_FLOPS = 8e12, 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default="")
    ap.add_argument("--kv-type", action="append", default=[], choices=["q8_0", "q4_0"])
    args = ap.parse_args()
    import ctypes as C
    import torch
    import fattn
    from bench import hip_events

    dev = torch.device("cuda", 0)
    DK, DV = fattn.MLA_DK, fattn.MLA_DV
    hip, evs = hip_events(2)
    gs = torch.cuda.Stream(dev)
    f = C.c_float()
    results = []
    for name in args.shape or list(SHAPES):
        H, N, S = SHAPES[name]["H"], SHAPES[name]["N"], SHAPES[name]["S"]
        g = torch.Generator(device=dev)
        g.manual_seed(4321)
        qtypes = {t: fattn.TYPE_NAMES[t] for t in args.kv_type}
        row_min = min([DK * 2] + [fattn.row_size(t, DK) for t in qtypes.values()])
        R = max(4, -(-(512 << 20) // (S * N * row_min)))
        caches, qcaches = [], {t: [] for t in qtypes}
        for _ in range(R):
            x = torch.randn((S * N, DK), generator=g, device=dev)
            caches.append(x.to(torch.float16))
            for t, ty in qtypes.items():
                qcaches[t].append(fattn.quantize(x, ty))
            del x
        owns = [] if qtypes else [c[:, DK - DV:].contiguous() for c in caches]
        q = torch.randn((S, 1, H, DK), generator=g, device=dev)
        npad = (N + 63) // 64 * 64
        mask = (torch.rand((1, npad), generator=g, device=dev) * 2 - 1).to(torch.float16)
        outs = torch.empty((R, S, 1, H, DV), dtype=torch.float32, device=dev)
        alg = S * (H * DK * 4 + H * DV * 4 + N * DK * 2) + N * 2
        flops = 2 * S * H * N * (DK + DV)
        scale = 1.0 / 192 ** 0.5
        kv0 = fattn.kv_view(caches[0], fattn.TYPE_F16, DK, N, 1, S)
        # form -> (K view, V view, K pointers, V pointers, bytes of a stored row)
        forms = {"view": (kv0, fattn.mla_v_view(kv0), [c.data_ptr() for c in caches],
                          [c.data_ptr() + 2 * (DK - DV) for c in caches], DK * 2)}
        if not qtypes:
            forms["own"] = (kv0, fattn.kv_view(owns[0], fattn.TYPE_F16, DV, N, 1, S), forms["view"][2],
                            [o.data_ptr() for o in owns], DK * 2)
        for t, ty in qtypes.items():
            kq = fattn.kv_view(qcaches[t][0], ty, DK, N, 1, S)
            voff = fattn.row_size(ty, DK - DV)
            forms[t] = (kq, fattn.mla_v_view(kq), [c.data_ptr() for c in qcaches[t]],
                        [c.data_ptr() + voff for c in qcaches[t]], fattn.row_size(ty, DK))
        graphs = {}
        for form, (kk, vv, kptrs, vptrs, _row) in forms.items():
            att = fattn.Attention(fattn.q_view(q), kk, vv, fattn.mask_view(mask), outs[0], scale)

            def step(i, att=att, kptrs=kptrs, vptrs=vptrs):
                att.retarget(k=kptrs[i % R], v=vptrs[i % R], dst=outs[i % R].data_ptr())
                att()

            gs.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(gs):
                for i in range(min(R, 4)):
                    step(i)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=gs):
                for i in range(args.steps):
                    step(i)
            graphs[form] = (gr, att.describe(), att)
            print(f"# {name} {form}: {att.describe()}", flush=True)
        # the two forms compute the same thing
        torch.cuda.synchronize()
        for form in graphs:
            with torch.cuda.stream(gs):
                graphs[form][0].replay()
            torch.cuda.synchronize()
            graphs[form] += (outs[0].clone(),)
        # (a quantised cache holds other values than the f16 one: no such comparison)
        same = bool(torch.equal(graphs["view"][3], graphs["own"][3])) if not qtypes else None
        us = {form: [] for form in graphs}
        for r in range(args.rounds):
            for form, (gr, *_rest) in graphs.items():
                with torch.cuda.stream(gs):
                    gr.replay()
                torch.cuda.synchronize()
                hip.hipEventRecord(evs[0], gs.cuda_stream)
                with torch.cuda.stream(gs):
                    gr.replay()
                hip.hipEventRecord(evs[1], gs.cuda_stream)
                torch.cuda.synchronize()
                hip.hipEventElapsedTime(C.byref(f), evs[0], evs[1])
                us[form].append(f.value * 1e3 / args.steps)
                print(f"round {r} {name} {form:5s} {us[form][-1]:8.3f} us/step", flush=True)
        for form, v in us.items():
            med = statistics.median(v)
            rec = dict(shape=name, H=H, N=N, S=S, form=form, plan=graphs[form][1], median_us=round(med, 3),
                       min_us=round(min(v), 3), max_us=round(max(v), 3), rounds=len(v), steps=args.steps, rotated_caches=R,
                       alg_bytes=alg, flops=flops, hbm_frac=round(alg / (med * 1e-6) / HBM_BPS, 4),
                       mfma_frac=round(flops / (med * 1e-6) / MFMA_FLOPS, 4), forms_bit_equal=same)
            if qtypes:
                stored = S * N * forms[form][4]
                rec.update(stored_bytes=stored, hbm_frac_stored=round(stored / (med * 1e-6) / HBM_BPS, 4))
            results.append(rec)
            print(json.dumps(rec), flush=True)
        del caches, qcaches, owns, outs, graphs
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
