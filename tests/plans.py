"""The plan table of the GPU suites and host-only planning parameters.

A Spec is one plan at its smallest shape: the planner options that force it,
the kv_chunk, and what describe() must name.  ROWS are the plans every feature
suite walks; PLANE_SPECS (tests/test_gpu_mask_planes.py) and OP_SPECS
(tests/test_gpu_op_params.py, tests/test_gpu_sinks.py) add the rows only they
take.  tests/test_gpu_views.py generates its own, larger list of the same class.
CELLS / GQA_CELLS (below) are the cell table of tests/combos.py.

plan_params() builds fattn params over fake pointers: fattn.describe /
fattn.workspace_size plan on the host and nothing may launch.
"""
from dataclasses import dataclass

import fattn


@dataclass(frozen=True)
class Spec:
    plan: str                 # row of the plan table
    kernel: str               # what describe() must name (on a 16-B-aligned view, the suite's feature live)
    D: int
    kt: str
    shape: tuple              # (NQ, H, Hkv, N)
    opts: tuple = ()          # ((option, value), ...)
    kv_chunk: int = 0
    tag: str = ""             # distinguishes two specs of one plan / D / type
    vt: str = ""              # V type when it differs from K's
    variants: tuple = ()      # tests/views.py variants the row is laid out in
    mask: str = "random"      # tests/test_gpu_views.py: the problem's mask kind
    v_trans: bool = False     # f16 V stored transposed, [Hkv][D][N]

    @property
    def id(self):
        NQ, H, Hkv, N = self.shape
        return f"{self.plan}{self.tag}-D{self.D}-{self.kt}-q{NQ}h{H}kv{Hkv}n{N}"

    @property
    def rk2(self):
        return self.shape[1] // self.shape[2]

    @property
    def row(self):
        return self.plan + (f"_d{self.D}" if (self.plan, self.D) in (("mq", 256), ("pf", 80)) else "") + \
            ("_maskbody" if self.mask != "random" else "")

    @property
    def family(self):
        return self.plan.split("_")[0]      # split | mq | bd | bdp | pf | pf4


MQ = ((fattn.OPT_MQ_MIN_ROWS, 32), (fattn.OPT_BD, 1))
BD, BDP = ((fattn.OPT_BD, 2),), ((fattn.OPT_BD, 3),)
PF1 = ((fattn.OPT_PF, 2), (fattn.OPT_PF_FORM, 1))
PF4 = ((fattn.OPT_PF, 2),)
STAGED = "kv_stage_f16<q8_0> + pf_mask_flags] + "

ROWS = [
    Spec("split_row", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 256)),
    Spec("split_row", "fattn_split_kernel<", 128, "f16", (1, 4, 4, 256)),
    Spec("split_row_tail", "fattn_split_kernel<", 128, "q8_0", (1, 4, 4, 200)),
    Spec("split_chunks", "fattn_split_kernel<", 128, "q8_0", (2, 8, 4, 1500), kv_chunk=256),
    Spec("split_gqa_merge", "fattn_split_kernel<", 128, "q8_0", (3, 8, 2, 800), kv_chunk=256),
    Spec("split_d80", "fattn_split_kernel<", 80, "f16", (9, 8, 2, 300)),
    Spec("mq", "fattn_mq_kernel<", 128, "q8_0", (40, 16, 4, 320), MQ),
    Spec("mq", "fattn_mq_kernel<q8_0,D256,4waves", 256, "q8_0", (50, 2, 2, 320), MQ),
    Spec("bd", "fattn_bd_kernel<", 128, "f16", (40, 2, 2, 800), BD),
    Spec("bd", "fattn_bd_kernel<", 128, "q8_0", (40, 2, 2, 800), BD),
    Spec("bdp", "fattn_bdp_kernel<", 64, "q8_0", (64, 2, 2, 320), BDP),
    Spec("bdp", "fattn_bdp_kernel<", 128, "q8_0", (64, 2, 2, 320), BDP),
    Spec("pf", "fattn_pf_kernel<f16,D128", 128, "f16", (300, 2, 2, 384), PF1),
    Spec("pf", STAGED + "fattn_pf_kernel<f16,D128", 128, "q8_0", (300, 2, 2, 384), PF1, tag="_staged"),
    Spec("pf", "fattn_pf_kernel<q8_0,D128", 128, "q8_0", (300, 2, 2, 384), PF1 + ((fattn.OPT_PF_STAGE, 1),),
         tag="_inkernel"),
]
PLANE_SPECS = ROWS + [
    Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128", 128, "f16", (300, 2, 2, 384), PF4),
    Spec("pf4", STAGED + "fattn_pf4_kernel(lean)<f16,D128", 128, "q8_0", (300, 2, 2, 384), PF4, tag="_staged"),
]
OP_SPECS = ROWS + [
    # the shape and options that take fattn_pf4_kernel(lean) with max_bias and logit_softcap off
    Spec("pf4shape", "fattn_pf_kernel<f16,D128", 128, "f16", (300, 2, 2, 384), PF4),
    Spec("split_gran4", ",gran4,", 128, "q8_0", (1, 4, 4, 256), variants=("kv_offset4",)),
    Spec("split_mixed", "fattn_split_kernel<q8_0,f16,D128", 128, "q8_0", (1, 4, 4, 256), vt="f16"),
]
OP_BY_ID = {s.id: s for s in OP_SPECS}
# one row per kernel family
FAMILIES = [OP_BY_ID[i] for i in ("split_gqa_merge-D128-q8_0-q3h8kv2n800", "mq-D128-q8_0-q40h16kv4n320",
                                  "bd-D128-q8_0-q40h2kv2n800", "bdp-D128-q8_0-q64h2kv2n320",
                                  "pf_staged-D128-q8_0-q300h2kv2n384")]
# the rows of the "feature off is the launch without it" cases
IDENT = [OP_BY_ID[i] for i in ("split_row-D128-q8_0-q1h4kv4n256", "mq-D128-q8_0-q40h16kv4n320", "bd-D128-f16-q40h2kv2n800",
                               "pf4shape-D128-f16-q300h2kv2n384")]
# H = 8, Hkv = 4: what the head-shard cases cut into 2 and 4 ranks
SHARD = Spec("shard", "fattn_split_kernel<", 128, "q8_0", (2, 8, 4, 512))

# ------------------------------------------------------------------ the cell table
# CELLS: every (kernel family, K type, V type, head dim) that has_kernel
# (csrc/fattn_launch.h) admits, MLA apart, at the family's smallest forcing shape
# -- what tests/combos.py runs the op's features over, in pairs.  CELL_GROUPS
# keeps the rows of the table apart; tests/test_combos.py
# states their counts.
HEAD_DIMS = (64, 80, 96, 128, 256)
CORE, EXT = ("f16", "q8_0", "q4_0"), ("q4_1", "q5_0", "q5_1")
ROW5 = dict(shape=(1, 4, 4, 544), kv_chunk=128)       # a one-row decode over 5 chunks, the last one 32 keys
GQA_MERGE = dict(shape=(3, 8, 2, 800), kv_chunk=256)  # 12 packed rows per tile, the chunks merged in a second launch
PFSHAPE = (300, 2, 2, 384)
INKERNEL = PF1 + ((fattn.OPT_PF_STAGE, 1),)


def split_dims(kt):
    """The head dims of the split kernel over K and V of type kt (has_kernel, Kernel::Split)."""
    return HEAD_DIMS if kt == "f16" else (64, 96, 128, 256) if kt in CORE else (64, 128, 256)


def _cell_groups():
    g = {}
    g["split"] = [Spec(plan, f"fattn_split_kernel<{kt},{kt},D{D},", D, kt, **form)
                  for kt in CORE + EXT + ("bf16",) for D in split_dims(kt)
                  for plan, form in (("split_row5", ROW5), ("split_gqa_merge", GQA_MERGE))]
    g["split_vT"] = [Spec("split_gqa_merge", f"fattn_split_kernel<f16,f16T,D{D},", D, "f16", tag="_vT", v_trans=True, **GQA_MERGE)
                     for D in HEAD_DIMS]
    g["split_mixed"] = [Spec("split_gqa_merge", f"fattn_split_kernel<{kt},{vt},D{D},", D, kt, tag=f"_v{vt}", vt=vt, **GQA_MERGE)
                        for kt in CORE for vt in CORE if kt != vt for D in (64, 128, 256)]
    g["mq"] = [Spec("mq", f"fattn_mq_kernel<{kt},D{D},", D, kt, (50, 2, 2, 320) if D == 256 else (40, 16, 4, 320), MQ)
               for kt in ("q8_0", "q4_0") for D in (64, 128, 256)]
    # prefill, the 8-wave body: f16 rows; Q8_0 / Q4_0 rows converted in the kernel (FATTN_OPT_PF_STAGE = 1)
    g["pf"] = [Spec("pf", "fattn_pf_kernel<f16,D80,", 80, "f16", PFSHAPE, PF4)] + \
        [Spec("pf", f"fattn_pf_kernel<{kt},D{D},", D, kt, PFSHAPE, PF1 if kt == "f16" else INKERNEL,
              tag="" if kt == "f16" else "_inkernel") for kt in CORE for D in (64, 96, 128)]
    # ... over rows staged to f16 by the pre-pass: Q8_0 / Q4_0 (the default), Q4_1 / Q5_0 / Q5_1 (their only
    # prefill), and these three at D = 128 in the default body, fattn_pf4_kernel(lean)
    staged = lambda kt, body, D: f"kv_stage_f16<{kt}> + pf_mask_flags] + {body}<f16,D{D},"
    g["pf_staged"] = [Spec("pf", staged(kt, "fattn_pf_kernel", D), D, kt, PFSHAPE, PF1, tag="_staged")
                      for kt in ("q8_0", "q4_0") for D in (64, 96, 128)] + \
        [Spec("pf", staged(kt, "fattn_pf_kernel", D), D, kt, PFSHAPE, PF1, tag="_staged") for kt in EXT for D in (64, 128)] + \
        [Spec("pf4", staged(kt, "fattn_pf4_kernel(lean)", 128), 128, kt, PFSHAPE, PF4, tag="_staged") for kt in EXT]
    g["pf4"] = [Spec("pf4", "fattn_pf4_kernel(lean)<f16,D128,", 128, "f16", PFSHAPE, PF4)]
    g["bd"] = [Spec("bd", f"fattn_bd_kernel<{kt},D{D},", D, kt, (40, 2, 2, 800), BD)
               for kt, D in (("f16", 64), ("f16", 96), ("f16", 128), ("q8_0", 128), ("q4_0", 128))]
    g["bdp"] = [Spec("bdp", f"fattn_bdp_kernel<{kt},D{D},", D, kt, (64, 2, 2, 320), BDP)
                for kt in ("q8_0", "q4_0") for D in (64, 96, 128)]
    return g


CELL_GROUPS = _cell_groups()
CELLS = [s for specs in CELL_GROUPS.values() for s in specs]
# q heads per kv head that are no power of two (a tile's last rows stay empty) or above 16 (the split kernel's
# second head subtile is ragged), D = 128
GQA_CELLS = [
    Spec("split_gqa", "fattn_split_kernel<q8_0,q8_0,D128,", 128, "q8_0", (1, 12, 2, 544), kv_chunk=128, tag="_rk6"),
    Spec("split_gqa_merge", "fattn_split_kernel<q8_0,q8_0,D128,", 128, "q8_0", (3, 14, 2, 800), kv_chunk=256, tag="_rk7"),
    Spec("split_gqa", "fattn_split_kernel<q8_0,q8_0,D128,", 128, "q8_0", (1, 40, 2, 544), kv_chunk=128, tag="_rk20"),
    Spec("mq", "fattn_mq_kernel<q8_0,D128,", 128, "q8_0", (40, 24, 4, 320), MQ, tag="_rk6"),
    Spec("bd", "fattn_bd_kernel<f16,D128,", 128, "f16", (40, 12, 2, 800), BD, tag="_rk6"),
    Spec("bdp", "fattn_bdp_kernel<q8_0,D128,", 128, "q8_0", (64, 14, 2, 320), BDP, tag="_rk7"),
    Spec("pf", "kv_stage_f16<q8_0> + pf_mask_flags] + fattn_pf_kernel<f16,D128,", 128, "q8_0", (90, 12, 2, 384), PF1, tag="_staged_rk6"),
]


def plan_params(D=128, NQ=1, H=32, Hkv=32, N=4096, kt=fattn.TYPE_Q8_0, vt=None, ptr=1 << 20, mask=True, v_nb=None,
                dk=None, dv=None, **kw):
    """fattn params of a contiguous [Hkv][N][row] cache over the fake pointer
    `ptr`.  vt: V's type where it differs from K's; v_nb: V's strides; dk / dv:
    K's / V's row lengths where they differ from D (MLA); **kw: ext_params'
    keywords (kv_chunk, max_bias, ...)."""
    def view(t, d, nb=None):
        rb = fattn.row_size(t, d)
        eb = fattn.BLOCK_BYTES.get(t) or fattn.row_size(t, 1) or 4
        return fattn.View(ptr, t, (d, N, Hkv, 1), nb or (eb, rb, rb * N, rb * N * Hkv))
    q = fattn.View(ptr, fattn.TYPE_F32, (D, NQ, H, 1), (4, H * D * 4, D * 4, NQ * H * D * 4))
    m = fattn.View(ptr, fattn.TYPE_F16, (N, NQ, 1, 1), (2, N * 2, N * 2 * NQ, N * 2 * NQ)) if mask else None
    return fattn.ext_params(q, view(kt, dk or D), view(kt if vt is None else vt, dv or D, v_nb), m, ptr, 0.088, **kw)
