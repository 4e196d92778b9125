"""The enumerated planner sweep behind tests/test_plan_golden.py: every
(option setting, head dim, K/V type pair) group's plans -- return code, the
fattn_describe text and fattn_workspace_size -- folded into one digest.  No GPU:
fattn_describe plans for 256 CUs when no device can be queried.

As a script it regenerates the fixture or dumps the full text for a diff:

    python tests/plan_sweep.py --write tests/golden/plan_digests.json
    python tests/plan_sweep.py --dump /tmp/new.txt [--setting NAME] [--group D128/q8_0/q8_0]

(FATTN_LIB=/path/to/other/libfattn.so dumps another build's plans.)"""
import ctypes as C
import dataclasses
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ggml-cuda-experiments_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fattn  # noqa: E402

F16, Q8, Q4 = fattn.TYPE_F16, fattn.TYPE_Q8_0, fattn.TYPE_Q4_0
Q41, Q50, Q51, BF16 = fattn.TYPE_Q4_1, fattn.TYPE_Q5_0, fattn.TYPE_Q5_1, fattn.TYPE_BF16
TYPE_NAME = {F16: "f16", Q8: "q8_0", Q4: "q4_0", Q41: "q4_1", Q50: "q5_0", Q51: "q5_1", BF16: "bf16"}
PTR = 1 << 20  # (alignment-only placeholder: nothing is launched)

HEAD_DIMS = (64, 80, 96, 128, 256)
TYPE_PAIRS = ((F16, F16), (Q8, Q8), (Q4, Q4), (Q8, F16), (F16, Q4), (Q8, Q4))
# the one-type caches of the split kernel (and the staged prefill), and a pair the
# library rejects: over SHAPES_1T at every head dim, the error codes of D = 80 / 96 included
TYPE_PAIRS_1T = ((Q41, Q41), (Q50, Q50), (Q51, Q51), (BF16, BF16), (Q50, F16))
# (NQ, H, Hkv, S, N): the BASELINE configs 2-5, their 2- / 4- / 8-rank head
# shards, prefill and batched shapes, and small awkward ones
SHAPES = (
    (1, 32, 32, 1, 2048),      # config 2
    (1, 32, 32, 1, 4096),      # config 3
    (1, 16, 16, 1, 4096),      # ... 2-rank shard
    (1, 4, 4, 1, 4096),        # ... 8-rank shard
    (1, 32, 8, 1, 8192),       # config 4
    (1, 8, 2, 1, 8192),        # ... 4-rank shard
    (64, 32, 32, 1, 4096),     # config 5
    (64, 16, 16, 1, 4096),     # ... 2-rank shard
    (64, 8, 8, 1, 4096),       # ... 4-rank shard
    (64, 4, 4, 1, 4096),       # ... 8-rank shard
    (4096, 32, 32, 1, 4096),   # prefill
    (512, 8, 8, 2, 1024),      # prefill, two sequences
    (256, 32, 8, 1, 4096),     # batched, GQA 4
    (256, 8, 8, 1, 1024),      # 256 rows per kv head, short KV: the multi-query kernel by default
    (16, 32, 8, 2, 2048),      # 64 packed rows per kv head
    (1, 8, 8, 1, 33),          # N = 33
    (7, 12, 2, 3, 1000),       # H / Hkv = 6, S = 3, N = 1000
    (1, 8, 8, 1, 131072),      # N = 131072
    (3, 6, 6, 2, 16384),       # few heads, long KV
)
# TYPE_PAIRS_1T: decode (configs 3 - 5), prefill (one and two sequences), 64
# packed rows, and the awkward ones
SHAPES_1T = tuple(SHAPES[i] for i in (1, 4, 6, 10, 11, 14, 15, 16, 17))
# MLA (K dim 576, V dim 512, one kv head): (H, NQ, N) over every V form of MLA_V
MLA_SHAPES = tuple((H, NQ, N) for H in (16, 128) for NQ in (1, 4) for N in (33, 4096, 131072))
# (K type, V: None of its own, else elements into the K row -- fattn.mla_v_view)
MLA_V = ((F16, 64), (F16, None), (Q8, 0), (Q8, 64), (Q4, 0), (Q4, 64))
MASKS = ("none", "one", "head", "seq")
XFORMS = (dict(), dict(logit_softcap=30.0), dict(max_bias=8.0))
KV_CHUNKS = (0, 1024)
LAYOUTS = ("head", "pos")

O = fattn
# every option at every legal non-default value (FATTN_OPT_SPLIT_STEPS and
# FATTN_OPT_MQ_MIN_ROWS: a spread of their ranges), one at a time ...
_SINGLE = (
    ("MQ_ROWS_PER_WAVE", O.OPT_MQ_ROWS_PER_WAVE, (16, 32)),
    ("MQ_DISABLE", O.OPT_MQ_DISABLE, (1,)),
    ("SPLIT_STEPS", O.OPT_SPLIT_STEPS, (1, 2, 3, 8, 64)),
    ("SPLIT_INFLIGHT", O.OPT_SPLIT_INFLIGHT, (1, 2, 3, 4)),
    ("PF", O.OPT_PF, (1, 2)),
    ("PF_STAGGER", O.OPT_PF_STAGGER, (0, 4, 6)),
    ("SPLIT_WAVE_MERGE", O.OPT_SPLIT_WAVE_MERGE, (1,)),
    ("SPLIT_PRIO", O.OPT_SPLIT_PRIO, (1, 2)),
    ("PF_SKIP", O.OPT_PF_SKIP, (1,)),
    ("MQ_MIN_ROWS", O.OPT_MQ_MIN_ROWS, (32, 64, 128, 1024)),
    ("SPLIT_WAVES", O.OPT_SPLIT_WAVES, (4, 8, 16)),
    ("SPLIT_SKIP", O.OPT_SPLIT_SKIP, (1,)),
    ("SPLIT_MERGE", O.OPT_SPLIT_MERGE, (1,)),
    ("BD", O.OPT_BD, (1, 2, 3)),
    ("MERGE_IN_KERNEL", O.OPT_MERGE_IN_KERNEL, (1,)),
    ("BD_XCD", O.OPT_BD_XCD, (1, 2)),
    ("SPLIT_XCD", O.OPT_SPLIT_XCD, (1, 2)),
    ("PF_STAGE", O.OPT_PF_STAGE, (1, 2)),
    ("PF_FORM", O.OPT_PF_FORM, (1, 4, 5, 6)),
    ("SPLIT_LOADERS", O.OPT_SPLIT_LOADERS, (1, 2)),
    ("MERGE_PLAIN", O.OPT_MERGE_PLAIN, (1, 2)),
    ("PART_F16", O.OPT_PART_F16, (1, 2)),
    ("GQA_UNPACK", O.OPT_GQA_UNPACK, (1, 2)),
)
# ... and combinations that reach plans no single option does
_COMBOS = (
    ("PF=1+BD=1", {O.OPT_PF: 1, O.OPT_BD: 1}),  # the multi-query kernel
    ("PF=1+BD=1+MQ_ROWS_PER_WAVE=16", {O.OPT_PF: 1, O.OPT_BD: 1, O.OPT_MQ_ROWS_PER_WAVE: 16}),
    ("PF=1+BD=1+MQ_ROWS_PER_WAVE=32", {O.OPT_PF: 1, O.OPT_BD: 1, O.OPT_MQ_ROWS_PER_WAVE: 32}),
    ("PF=1+BD=1+SPLIT_MERGE=1", {O.OPT_PF: 1, O.OPT_BD: 1, O.OPT_SPLIT_MERGE: 1}),
    ("PF=1+BD=1+PART_F16=1", {O.OPT_PF: 1, O.OPT_BD: 1, O.OPT_PART_F16: 1}),
    ("PF=1+BD=1+MQ_MIN_ROWS=32", {O.OPT_PF: 1, O.OPT_BD: 1, O.OPT_MQ_MIN_ROWS: 32}),
    ("PF=1+BD=2", {O.OPT_PF: 1, O.OPT_BD: 2}),
    ("BD=2+MERGE_IN_KERNEL=1", {O.OPT_BD: 2, O.OPT_MERGE_IN_KERNEL: 1}),
    ("BD=2+PART_F16=1+MERGE_PLAIN=2", {O.OPT_BD: 2, O.OPT_PART_F16: 1, O.OPT_MERGE_PLAIN: 2}),
    ("PART_F16=1+MERGE_PLAIN=2", {O.OPT_PART_F16: 1, O.OPT_MERGE_PLAIN: 2}),
    ("SPLIT_LOADERS=2+SPLIT_STEPS=3", {O.OPT_SPLIT_LOADERS: 2, O.OPT_SPLIT_STEPS: 3}),
    ("SPLIT_LOADERS=2+SPLIT_INFLIGHT=1", {O.OPT_SPLIT_LOADERS: 2, O.OPT_SPLIT_INFLIGHT: 1}),
    ("SPLIT_WAVES=16+SPLIT_STEPS=2", {O.OPT_SPLIT_WAVES: 16, O.OPT_SPLIT_STEPS: 2}),
    ("PF=2+PF_FORM=1+PF_STAGE=1", {O.OPT_PF: 2, O.OPT_PF_FORM: 1, O.OPT_PF_STAGE: 1}),
    ("MQ_DISABLE=1+GQA_UNPACK=2", {O.OPT_MQ_DISABLE: 1, O.OPT_GQA_UNPACK: 2}),
)


def settings():
    """[(name, {option: value})], the defaults first."""
    out = [("defaults", {})]
    for name, opt, values in _SINGLE:
        out += [(f"{name}={v}", {opt: v}) for v in values]
    return out + list(_COMBOS)


def _kv(t, D, N, Hkv, S, layout):
    rb = fattn.row_size(t, D)
    nb0 = fattn.elem_bytes(t)
    nb = (nb0, rb, rb * N, rb * N * Hkv) if layout == "head" else (nb0, rb * Hkv, rb, rb * N * Hkv)
    return fattn.View(PTR, t, (D, N, Hkv, S), nb)


def _mask(mode, NQ, H, S, N):
    if mode == "none":
        return None
    Np = N + (N & 1)
    ne2 = H if mode == "head" else 1
    ne3 = S if mode == "seq" else 1
    return fattn.View(PTR, F16, (Np, NQ, ne2, ne3), (2, Np * 2, Np * NQ * 2, Np * NQ * ne2 * 2))


def group_name(D, kt, vt):
    return f"D{D}/{TYPE_NAME[kt]}/{TYPE_NAME[vt]}"


def _variants(q, k, v, NQ, H, S, N):
    """(label suffix, FattnParams) of one (q, k, v) over the masks, score transforms and kv_chunk hints."""
    for mode in MASKS:
        m = _mask(mode, NQ, H, S, N)
        for xi, xf in enumerate(XFORMS):
            for chunk in KV_CHUNKS:
                yield f"mask:{mode} xf{xi} chunk{chunk}", fattn.ext_params(q, k, v, m, PTR, 0.088, kv_chunk=chunk, **xf)


def mla_group(kt):
    """The MLA cases of cache type kt: MLA_SHAPES x the type's V forms of MLA_V."""
    DK, DV = fattn.MLA_DK, fattn.MLA_DV
    cases = []
    for H, NQ, N in MLA_SHAPES:
        q = fattn.View(PTR, fattn.TYPE_F32, (DK, NQ, H, 1), (4, H * DK * 4, DK * 4, NQ * H * DK * 4))
        k = _kv(kt, DK, N, 1, 1, "head")
        for t, v_off in MLA_V:
            if t != kt:
                continue
            # (V of its own: another buffer, far from K's rows)
            v = fattn.mla_v_view(k, v_off) if v_off is not None else dataclasses.replace(_kv(kt, DV, N, 1, 1, "head"), ptr=PTR << 12)
            vname = "own" if v_off is None else f"k+{v_off}"
            cases += [(f"NQ{NQ} H{H}/1 S1 N{N} v:{vname} {label}", p) for label, p in _variants(q, k, v, NQ, H, 1, N)]
    return cases


def pair_cases(D, kt, vt, shapes):
    cases = []
    for NQ, H, Hkv, S, N in shapes:
        q = fattn.View(PTR, fattn.TYPE_F32, (D, NQ, H, S), (4, H * D * 4, D * 4, NQ * H * D * 4))
        for layout in LAYOUTS:
            k, v = _kv(kt, D, N, Hkv, S, layout), _kv(vt, D, N, Hkv, S, layout)
            cases += [(f"NQ{NQ} H{H}/{Hkv} S{S} N{N} {layout} {label}", p) for label, p in _variants(q, k, v, NQ, H, S, N)]
    return cases


def groups():
    """{group name: [(case label, FattnParams)]}, built once and planned under every setting.
    One group per (head dim, pair of TYPE_PAIRS); one per pair of TYPE_PAIRS_1T,
    its five head dims together (the fixture stays small); one per MLA cache type."""
    out = {}
    for D in HEAD_DIMS:
        for kt, vt in TYPE_PAIRS:
            out[group_name(D, kt, vt)] = pair_cases(D, kt, vt, SHAPES)
    for kt, vt in TYPE_PAIRS_1T:
        out[group_name("*", kt, vt)] = [(f"D{D} {label}", p) for D in HEAD_DIMS for label, p in pair_cases(D, kt, vt, SHAPES_1T)]
    for kt in (F16, Q8, Q4):
        out[f"D{fattn.MLA_DK}/mla/{TYPE_NAME[kt]}"] = mla_group(kt)
    return out


def plan_lines(cases):
    """One line per case: `label | rc | workspace size | describe text`."""
    L = fattn.lib()
    buf = C.create_string_buffer(512)
    for label, p in cases:
        ref = C.byref(p)
        rc = L.fattn_describe(ref, buf, len(buf))
        yield f"{label} | {rc} | {L.fattn_workspace_size(ref)} | {buf.value.decode() if rc == 0 else ''}"


def digest(cases):
    h = hashlib.sha256()
    for line in plan_lines(cases):
        h.update(line.encode())
        h.update(b"\n")
    return h.hexdigest()[:16]


def row_workspace_sizes():
    """fattn_row_workspace_size over a handful of (head dim, kv size, heads)."""
    L = fattn.lib()
    return {f"D{D} N{N} H{H}": int(L.fattn_row_workspace_size(D, N, H))
            for D in (64, 128, 256) for N in (33, 2048, 4096, 131072) for H in (1, 8, 32)}


def sweep(only_setting=None):
    """{setting name: {group name: digest}} with the library fattn loads."""
    G = groups()
    out = {}
    for name, opts in settings():
        if only_setting is not None and name != only_setting:
            continue
        with fattn.options(opts):
            out[name] = {g: digest(cases) for g, cases in G.items()}
    return out


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", metavar="JSON", help="write the digests of the loaded library as the fixture")
    ap.add_argument("--dump", metavar="TXT", help="write the full plan text (every case's line)")
    ap.add_argument("--setting", help="--dump: only this option setting (default: all)")
    ap.add_argument("--group", help="--dump: only this group, e.g. D128/q8_0/q8_0")
    a = ap.parse_args(argv)
    if a.write:
        G = groups()
        n = len(next(iter(G.values())))
        # (cases_per_group: the TYPE_PAIRS groups'; the others' counts by name)
        doc = {"cases_per_group": n, "cases_of_group": {g: len(c) for g, c in G.items() if len(c) != n},
               "row_workspace": row_workspace_sizes(), "digests": sweep()}
        with open(a.write, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"wrote {a.write}: {len(doc['digests'])} settings x {len(next(iter(doc['digests'].values())))} groups")
    if a.dump:
        G = groups()
        with open(a.dump, "w") as f:
            for name, opts in settings():
                if a.setting is not None and name != a.setting:
                    continue
                with fattn.options(opts):
                    for g, cases in G.items():
                        if a.group is None or g == a.group:
                            f.writelines(f"[{name}] {g} {line}\n" for line in plan_lines(cases))
        print(f"wrote {a.dump}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
