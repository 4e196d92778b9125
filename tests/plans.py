"""The plan table of the GPU suites and host-only planning parameters.

A Spec is one plan at its smallest shape: the planner options that force it,
the kv_chunk, and what describe() must name.  ROWS are the plans every feature
suite walks; PLANE_SPECS (tests/test_gpu_mask_planes.py) and OP_SPECS
(tests/test_gpu_op_params.py, tests/test_gpu_sinks.py) add the rows only they
take.  tests/test_gpu_views.py generates its own, larger list of the same class.

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
