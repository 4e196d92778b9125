"""Host-side mirror of the reference's attention interface, over libfattn.so.

The reference drives its kernels from C++ host code (src/kernel_test.h,
src/flash-matrix.cu) with ggml ne/nb views (src/flash-llama.h:7-32).  This
package is the Python face of the same boundary: it binds the C ABI declared
in include/fattn.h with ctypes and takes device pointers from torch tensors
(torch is plumbing here: device memory and the current HIP stream).

There is no fallback: if libfattn.so is missing or fails to load, every entry
point raises.  Nothing here imports the test oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_PKG_DIR, "..", "lib", os.environ.get("FATTN_LIB", "libfattn.so")))

# ggml_type numbering (include/fattn.h)
TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q8_0 = 0, 1, 2, 8
TYPE_Q4_1, TYPE_Q5_0, TYPE_Q5_1 = 3, 6, 7
TYPE_I32, TYPE_I64 = 26, 27   # index tensors of set_rows only
TYPE_BF16 = 30                # 2-byte elements: K / V of flash_attn_ext, dst of cpy / quantize (not of set_rows)
TYPE_NAMES = {"f32": TYPE_F32, "f16": TYPE_F16, "q4_0": TYPE_Q4_0, "q8_0": TYPE_Q8_0,
              "q4_1": TYPE_Q4_1, "q5_0": TYPE_Q5_0, "q5_1": TYPE_Q5_1, "bf16": TYPE_BF16}
BLOCK_TYPES = (TYPE_Q8_0, TYPE_Q4_0, TYPE_Q4_1, TYPE_Q5_0, TYPE_Q5_1)

FATTN_OK = 0
ERRORS = {
    -1: "FATTN_ERR_INVALID_ARG", -2: "FATTN_ERR_UNSUPPORTED_TYPE", -3: "FATTN_ERR_UNSUPPORTED_HEAD_DIM",
    -4: "FATTN_ERR_BAD_STRIDE", -5: "FATTN_ERR_WORKSPACE", -6: "FATTN_ERR_LAUNCH", -7: "FATTN_ERR_ALIGNMENT",
}

# every symbol include/fattn.h and include/fattn_debug.h declare
EXPORTS = (
    "fattn_workspace_size", "fattn_workspace_init", "fattn_ext", "fattn_ext_events", "fattn_ext_f16_launch", "fattn_row_workspace_size", "fattn_row",
    "fattn_dequantize", "fattn_quantize", "fattn_strerror", "fattn_row_size", "fattn_version", "fattn_set_option",
    "fattn_describe", "fattn_cpy", "fattn_ext_sinks", "fattn_set_rows", "fattn_ext_lse", "fattn_lse_merge",
    "fattn_k_shift",
)
ROPE_NORMAL, ROPE_NEOX = 0, 2   # fattn_rope.mode: ggml's GGML_ROPE_TYPE_NORMAL / GGML_ROPE_TYPE_NEOX
OPT_MQ_ROWS_PER_WAVE = 1
OPT_MQ_DISABLE = 2
OPT_SPLIT_STEPS = 3
OPT_SPLIT_INFLIGHT = 4
OPT_PF = 5
OPT_PF_STAGGER = 6
OPT_SPLIT_WAVE_MERGE = 10
OPT_SPLIT_PRIO = 11
OPT_PF_SKIP = 12
OPT_MQ_MIN_ROWS = 13
OPT_SPLIT_WAVES = 19
OPT_SPLIT_SKIP = 20
OPT_SPLIT_MERGE = 21
OPT_BD = 22
OPT_MERGE_IN_KERNEL = 24
OPT_BD_XCD = 25
OPT_SPLIT_XCD = 26
OPT_PF_STAGE = 28
OPT_PF_FORM = 29
OPT_SPLIT_LOADERS = 30
OPT_MERGE_PLAIN = 31
OPT_PART_F16 = 32
OPT_GQA_UNPACK = 33
# every option's default (include/fattn_debug.h): reset_options() restores them
OPTION_DEFAULTS = {
    OPT_MQ_ROWS_PER_WAVE: 0, OPT_MQ_DISABLE: 0, OPT_SPLIT_STEPS: 0, OPT_SPLIT_INFLIGHT: 0, OPT_PF: 0,
    OPT_PF_STAGGER: 2, OPT_SPLIT_WAVE_MERGE: 0, OPT_SPLIT_PRIO: 0, OPT_PF_SKIP: 0, OPT_MQ_MIN_ROWS: 0,
    OPT_SPLIT_WAVES: 0, OPT_SPLIT_SKIP: 0, OPT_SPLIT_MERGE: 0, OPT_BD: 0, OPT_MERGE_IN_KERNEL: 0, OPT_BD_XCD: 0, OPT_SPLIT_XCD: 0,
    OPT_PF_STAGE: 0, OPT_PF_FORM: 0, OPT_SPLIT_LOADERS: 0, OPT_MERGE_PLAIN: 0, OPT_PART_F16: 0, OPT_GQA_UNPACK: 0,
}


class FattnError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        super().__init__(f"{what}: {ERRORS.get(code, code)} ({code})")


class FattnTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("type", C.c_int32), ("pad_", C.c_int32),
                ("ne", C.c_int64 * 4), ("nb", C.c_int64 * 4)]


class FattnParams(C.Structure):
    _fields_ = [("q", FattnTensor), ("k", FattnTensor), ("v", FattnTensor), ("mask", FattnTensor),
                ("dst", C.c_void_p), ("scale", C.c_float), ("kv_chunk", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                # ggml's op_params[1], [2] and the global head numbering of the ALiBi slopes (zeros: off)
                ("max_bias", C.c_float), ("logit_softcap", C.c_float),
                ("n_head_total", C.c_int32), ("head_first", C.c_int32)]


class FattnRope(C.Structure):
    """ggml_rope_ext's parameters (include/fattn.h fattn_rope)."""
    _fields_ = [("n_dims", C.c_int32), ("mode", C.c_int32), ("n_ctx_orig", C.c_int32),
                ("freq_base", C.c_float), ("freq_scale", C.c_float), ("ext_factor", C.c_float),
                ("attn_factor", C.c_float), ("beta_fast", C.c_float), ("beta_slow", C.c_float)]


def rope_params(n_dims: int, mode: int = ROPE_NEOX, *, freq_base: float = 10000.0, freq_scale: float = 1.0,
                ext_factor: float = 0.0, attn_factor: float = 1.0, beta_fast: float = 32.0, beta_slow: float = 1.0,
                n_ctx_orig: int = 0) -> FattnRope:
    """A FattnRope with ggml's defaults for everything but n_dims."""
    return FattnRope(int(n_dims), int(mode), int(n_ctx_orig), float(freq_base), float(freq_scale), float(ext_factor),
                     float(attn_factor), float(beta_fast), float(beta_slow))


_lib = None


def lib() -> C.CDLL:
    """Load libfattn.so (fails loudly -- there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libfattn.so not built at {LIB_PATH}; run `make lib` (or __graft_entry__.build())")
        # torch's HIP runtime must be the process's one: libfattn.so's
        # libamdhip64.so.7 dependency then binds to it.  Loaded first, the
        # library would pull in /opt/rocm's runtime beside torch's and see no
        # device through it.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
        L.fattn_workspace_size.restype = sz
        L.fattn_workspace_size.argtypes = [C.POINTER(FattnParams)]
        L.fattn_set_option.restype = C.c_int
        L.fattn_set_option.argtypes = [C.c_int, C.c_int]
        L.fattn_workspace_init.restype = C.c_int
        L.fattn_workspace_init.argtypes = [vp, sz, vp]
        L.fattn_ext.restype = C.c_int
        L.fattn_ext.argtypes = [C.POINTER(FattnParams), vp]
        L.fattn_ext_sinks.restype = C.c_int
        L.fattn_ext_sinks.argtypes = [C.POINTER(FattnParams), vp, vp]
        L.fattn_ext_lse.restype = C.c_int
        L.fattn_ext_lse.argtypes = [C.POINTER(FattnParams), vp, vp, vp]
        L.fattn_lse_merge.restype = C.c_int
        L.fattn_lse_merge.argtypes = [vp, vp, C.c_int32, i64, C.c_int32, i64, i64, vp, C.c_int32, vp, vp, vp]
        L.fattn_ext_events.restype = C.c_int
        L.fattn_ext_events.argtypes = [C.POINTER(FattnParams), vp, vp, vp]
        L.fattn_ext_f16_launch.restype = C.c_int
        L.fattn_ext_f16_launch.argtypes = ([vp, vp, vp, vp, vp, C.c_float] + [C.c_int] * 20 +
                                           [C.c_int, C.c_int, vp, sz, vp])
        L.fattn_row_workspace_size.restype = sz
        L.fattn_row_workspace_size.argtypes = [C.c_int, C.c_int, C.c_int]
        L.fattn_row.restype = C.c_int
        L.fattn_row.argtypes = [vp, vp, vp, vp, vp, sz, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                vp]
        L.fattn_dequantize.restype = C.c_int
        L.fattn_dequantize.argtypes = [C.c_int, vp, vp, i64, i64, vp]
        L.fattn_quantize.restype = C.c_int
        L.fattn_quantize.argtypes = [C.c_int, vp, vp, i64, i64, vp]
        L.fattn_strerror.restype = C.c_char_p
        L.fattn_strerror.argtypes = [C.c_int]
        L.fattn_row_size.restype = sz
        L.fattn_row_size.argtypes = [C.c_int, i64]
        L.fattn_version.restype = C.c_char_p
        L.fattn_cpy.restype = C.c_int
        L.fattn_cpy.argtypes = [C.POINTER(FattnTensor), C.POINTER(FattnTensor), vp]
        L.fattn_set_rows.restype = C.c_int
        L.fattn_set_rows.argtypes = [C.POINTER(FattnTensor), C.POINTER(FattnTensor), C.POINTER(FattnTensor), vp]
        L.fattn_k_shift.restype = C.c_int
        L.fattn_k_shift.argtypes = [C.POINTER(FattnTensor), C.POINTER(FattnTensor), vp, C.POINTER(FattnRope), vp]
        L.fattn_describe.restype = C.c_int
        L.fattn_describe.argtypes = [C.POINTER(FattnParams), C.c_char_p, sz]
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != FATTN_OK:
        raise FattnError(rc, what)


def set_option(option: int, value: int):
    """Planner override (fattn_set_option): the OPT_* constants above mirror the
    FATTN_OPT_* enum of include/fattn_debug.h, which documents every option's
    values and effect.  Raises FattnError for an unknown option or an illegal value."""
    _check(lib().fattn_set_option(option, value), "fattn_set_option")


def reset_options():
    """Every planner override back to its default (the process-wide state of
    fattn_set_option; tests reset it after each case so a failing one cannot
    leak an override into the next)."""
    for opt, val in OPTION_DEFAULTS.items():
        set_option(opt, val)


class options:
    """Context manager: set planner overrides for a block, restore the defaults
    on exit (also when the block raises).  `with fattn.options({OPT_BD: 2}): ...`"""

    def __init__(self, opts: dict):
        self.opts = dict(opts)

    def __enter__(self):
        try:
            for opt, val in self.opts.items():
                set_option(opt, val)
        except Exception:
            reset_options()
            raise
        return self

    def __exit__(self, *exc):
        reset_options()
        return False


def row_size(typ: int, k: int) -> int:
    return int(lib().fattn_row_size(typ, k))


def elem_bytes(typ: int) -> int:
    """nb[0] of a contiguous row of typ: an element's bytes, or a ggml block's."""
    return row_size(typ, 1) or row_size(typ, 32)


def __getattr__(name):
    if name == "BLOCK_BYTES":   # {block type: bytes of a block}, as the library has them
        return {t: row_size(t, 32) for t in BLOCK_TYPES}
    raise AttributeError(name)


def strerror(code: int) -> str:
    return lib().fattn_strerror(code).decode()


@dataclass
class View:
    """A ggml tensor view: device pointer, ggml type, ne (elements), nb (bytes)."""
    ptr: int
    type: int
    ne: Sequence[int]
    nb: Sequence[int]

    def c(self) -> FattnTensor:
        t = FattnTensor()
        t.data = self.ptr
        t.type = self.type
        for i in range(4):
            t.ne[i] = int(self.ne[i])
            t.nb[i] = int(self.nb[i])
        return t


def _stream(stream) -> Optional[int]:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return int(stream)


def ext_params(q: View, k: View, v: View, mask: Optional[View], dst_ptr: int, scale: float,
               workspace_ptr: int = 0, workspace_bytes: int = 0, kv_chunk: int = 0, *, max_bias: float = 0.0,
               logit_softcap: float = 0.0, n_head_total: int = 0, head_first: int = 0) -> FattnParams:
    """max_bias / logit_softcap: ggml's op_params[1] / [2] (ALiBi slopes on the
    mask, cap * tanh(score / cap)); n_head_total / head_first: the unsharded
    head count and the global index of q head 0, for the slopes of a
    head-sharded launch (shard.HeadShard.slope_args()).  Zeros: off."""
    p = FattnParams()
    p.q, p.k, p.v = q.c(), k.c(), v.c()
    if mask is not None:
        p.mask = mask.c()
    p.dst = dst_ptr
    p.scale = float(scale)
    p.kv_chunk = int(kv_chunk)
    p.workspace = workspace_ptr or None
    p.workspace_bytes = int(workspace_bytes)
    p.max_bias = float(max_bias)
    p.logit_softcap = float(logit_softcap)
    p.n_head_total = int(n_head_total)
    p.head_first = int(head_first)
    return p


def workspace_size(p: FattnParams) -> int:
    return int(lib().fattn_workspace_size(C.byref(p)))


def describe(p: FattnParams) -> str:
    """The kernel(s) and plan fattn_ext would launch for these params (diagnostic)."""
    buf = C.create_string_buffer(512)
    _check(lib().fattn_describe(C.byref(p), buf, len(buf)), "fattn_describe")
    return buf.value.decode()


NO_SINKS = object()   # Attention.retarget(sinks=NO_SINKS): back to a launch without sinks
NO_LSE = object()     # Attention.retarget(lse=NO_LSE): back to a launch that writes no log-sum-exp


def _sinks_ptr(sinks, n_head: int) -> Optional[int]:
    """sinks: None, a raw device pointer (taken on trust), or a torch tensor:
    contiguous float32 on the GPU with exactly n_head = q.ne[2] values -- a host
    tensor or a short slice would be an illegal or out-of-bounds device read."""
    if sinks is None or isinstance(sinks, int):
        return sinks
    import torch
    if sinks.dtype != torch.float32 or not sinks.is_contiguous():
        raise ValueError("sinks: a contiguous float32 tensor, one value per q head of the launch")
    if not sinks.is_cuda:
        raise ValueError("sinks: a device tensor (this one is on the host)")
    if sinks.numel() != n_head:
        raise ValueError(f"sinks: {sinks.numel()} values for the launch's {n_head} q heads (q.ne[2])")
    return _tptr(sinks)


def _lse_ptr(lse, n_rows: int) -> Optional[int]:
    """lse: None, a raw device pointer (taken on trust), or a torch tensor:
    contiguous float32 on the GPU with exactly n_rows = S * n_q * H values -- a
    host tensor or a short one would be an illegal or out-of-bounds device write."""
    if lse is None or isinstance(lse, int):
        return lse
    import torch
    if lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("lse: a contiguous float32 tensor, one value per output row [S][n_q][H]")
    if not lse.is_cuda:
        raise ValueError("lse: a device tensor (this one is on the host)")
    if lse.numel() != n_rows:
        raise ValueError(f"lse: {lse.numel()} values for the launch's {n_rows} output rows (S * n_q * H)")
    return _tptr(lse)


def flash_attn_ext(p: FattnParams, stream=None, ev_begin=None, ev_end=None, sinks=None, lse=None):
    """GGML_OP_FLASH_ATTN_EXT on the GPU (replaces flash_attn_ext_f16, src/flash-llama.h:5-32).
    ev_begin/ev_end: optional raw hipEvent_t handles recorded around the main kernel.
    sinks: ggml's src[4], one raw f32 logit per q head of THIS launch that joins
    the softmax denominator (include/fattn.h, fattn_ext_sinks) -- a device pointer
    or a torch f32 tensor of p.q.ne[2] values (a head shard passes
    shard.HeadShard.sink_slice(sinks)); None is fattn_ext.  The plan, the
    workspace and describe(p) do not depend on it.  There is no events variant:
    sinks with ev_begin / ev_end raises ValueError.
    lse: where the rows' natural-log log-sum-exp goes (include/fattn.h,
    fattn_ext_lse) -- a device pointer or a contiguous torch f32 tensor of exactly
    S * n_q * H values, dst's layout without its last dim; with sinks the sink is
    one of its terms.  None writes none.  Like sinks it changes no plan and has no
    events variant (ValueError)."""
    if lse is not None:
        if ev_begin is not None or ev_end is not None:
            raise ValueError("flash_attn_ext: lse cannot be combined with ev_begin / ev_end")
        sptr = _sinks_ptr(sinks, int(p.q.ne[2]))
        lptr = _lse_ptr(lse, int(p.q.ne[1]) * int(p.q.ne[2]) * int(p.q.ne[3]))
        _check(lib().fattn_ext_lse(C.byref(p), sptr, lptr, _stream(stream)), "fattn_ext_lse")
    elif sinks is not None:
        if ev_begin is not None or ev_end is not None:
            raise ValueError("flash_attn_ext: sinks cannot be combined with ev_begin / ev_end")
        ptr = _sinks_ptr(sinks, int(p.q.ne[2]))
        _check(lib().fattn_ext_sinks(C.byref(p), ptr, _stream(stream)), "fattn_ext_sinks")
    elif ev_begin is None and ev_end is None:
        _check(lib().fattn_ext(C.byref(p), _stream(stream)), "fattn_ext")
    else:
        _check(lib().fattn_ext_events(C.byref(p), _stream(stream), ev_begin, ev_end), "fattn_ext_events")


def lse_merge(outs, lses, dst, sinks=None, lse_out=None, n_head=None, stream=None):
    """fattn_lse_merge (include/fattn.h): merge P normalised partial outputs of
    the same rows over disjoint key ranges by their log-sum-exps -- what
    flash_attn_ext(..., lse=) wrote on each range, e.g. after
    shard.gather_parts().  outs: f32 [P, ..., dv], lses: f32 [P, ...] (device
    tensors whose parts are contiguous; the part strides pass through, so a
    slice of a padded buffer works); dst: contiguous f32 [..., dv], not aliasing
    outs.  sinks: None, or a contiguous f32 tensor of n_head raw logits that join
    the merged denominator once (rows are in dst's [S][n_q][H] order: row r is
    head r % n_head; n_head defaults to sinks.numel()).  lse_out: None or a
    contiguous f32 tensor of one value per row.  Returns dst."""
    import torch
    for name, t in (("outs", outs), ("lses", lses), ("dst", dst)):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"lse_merge: {name} must be a float32 device tensor")
    if outs.dim() < 2 or lses.dim() < 1 or outs.shape[0] != lses.shape[0]:
        raise ValueError("lse_merge: outs is [P, ..., dv] and lses [P, ...] with the same P")
    P, dv = int(outs.shape[0]), int(outs.shape[-1])
    n_rows = outs[0].numel() // dv
    if not outs[0].is_contiguous() or not lses[0].is_contiguous() or not dst.is_contiguous():
        raise ValueError("lse_merge: every part of outs / lses, and dst, must be contiguous")
    if lses[0].numel() != n_rows or dst.numel() != n_rows * dv:
        raise ValueError("lse_merge: lses holds one value per row of outs, dst one part's shape")
    sptr = None
    if sinks is not None:
        if sinks.dtype != torch.float32 or not sinks.is_contiguous() or not sinks.is_cuda:
            raise ValueError("lse_merge: sinks must be a contiguous float32 device tensor")
        n_head = int(sinks.numel()) if n_head is None else int(n_head)
        if sinks.numel() != n_head or n_head < 1:
            raise ValueError("lse_merge: sinks holds n_head values")
        sptr = _tptr(sinks)
    lptr = _lse_ptr(lse_out, n_rows)
    _check(lib().fattn_lse_merge(_tptr(outs), _tptr(lses), P, n_rows, dv, int(outs.stride(0)) if P > 1 else n_rows * dv,
                                 int(lses.stride(0)) if P > 1 else n_rows, sptr, int(n_head or 0), _tptr(dst), lptr,
                                 _stream(stream)), "fattn_lse_merge")
    return dst


# ------------------------------------------------------------------ torch helpers

def _tptr(t) -> int:
    return int(t.data_ptr())


def kv_view(buf, typ: int, D: int, N: int, Hkv: int, S: int = 1, layout: str = "head") -> View:
    """View of a KV cache held in a byte (or f16) torch tensor; typ: TYPE_F16,
    TYPE_BF16 or a block type (Q8_0, Q4_0, Q4_1, Q5_0, Q5_1).

    layout "head": [S][Hkv][N][row]   (per-head contiguous; reference decode layout,
                   src/flash_row_float.h:19,58)
    layout "pos":  [S][N][Hkv][row]   (llama.cpp's KV cache: nb1 = Hkv * row)

    An MLA cache is kv_view(buf, TYPE_F16, MLA_DK, N, 1, S): 576-element rows; its
    V is mla_v_view() of that view (or a kv_view with D = MLA_DV over a buffer of
    its own).
    """
    rb = row_size(typ, D)
    nb0 = elem_bytes(typ)
    if layout == "head":
        nb = (nb0, rb, rb * N, rb * N * Hkv)
    elif layout == "pos":
        nb = (nb0, rb * Hkv, rb, rb * N * Hkv)
    else:
        raise ValueError(layout)
    return View(_tptr(buf), typ, (D, N, Hkv, S), nb)


MLA_DK, MLA_DV = 576, 512   # multi-head latent attention: K row (64 RoPE dims + the latent), V row (the latent)


def mla_v_view(k: View, v_off: int = MLA_DK - MLA_DV) -> View:
    """The V of an MLA call as a view of its K (include/fattn.h): the 512
    elements of every 576-element f16 cache row from element v_off on -- 64 when
    the RoPE dims come first (llama.cpp's order), 0 when the latent does.  Same
    strides as K, so fattn_ext reads each cache row once (describe: v=k+<bytes>).

    A Q8_0 / Q4_0 K view (18 blocks per row): v_off is 0, 32 or 64 elements --
    whole blocks -- and the pointer advances by row_size(type, v_off)."""
    if k.type in (TYPE_Q8_0, TYPE_Q4_0):
        if int(k.ne[0]) != MLA_DK or int(k.nb[0]) != elem_bytes(k.type):
            raise ValueError("mla_v_view: a quantised K must have 576-element rows of whole blocks")
        if v_off not in (0, 32, 64):
            raise ValueError("mla_v_view: v_off is 0, 32 or 64 elements (whole blocks) for a quantised K")
        return View(k.ptr + row_size(k.type, v_off), k.type, (MLA_DV,) + tuple(int(x) for x in k.ne[1:]), tuple(k.nb))
    if k.type != TYPE_F16 or int(k.ne[0]) != MLA_DK or int(k.nb[0]) != 2:
        raise ValueError("mla_v_view: K must be an f16 view with 576-element rows")
    if v_off % 8 or not 0 <= v_off <= MLA_DK - MLA_DV:
        raise ValueError("mla_v_view: v_off is 0 .. 64 elements, a multiple of 8 (16 bytes)")
    return View(k.ptr + 2 * v_off, TYPE_F16, (MLA_DV,) + tuple(int(x) for x in k.ne[1:]), tuple(k.nb))


def dst_shape(q: View, v: View) -> tuple:
    """Shape of the f32 output [S][n_q][H][V's row length]: dst's last dim is
    V's, which differs from Q's only for the MLA pair (576 / 512)."""
    return (int(q.ne[3]), int(q.ne[1]), int(q.ne[2]), int(v.ne[0]))


def q_view(q) -> View:
    """q: torch f32 contiguous [S][n_q][H][D] (ggml ne = [D, n_q, H, S] with
    nb1 = H*D*4: the permuted query of llama.cpp) -- or any tensor with the
    ggml strides supplied via q_view_strided."""
    S, NQ, H, D = q.shape
    return View(_tptr(q), TYPE_F32, (D, NQ, H, S), (4, H * D * 4, D * 4, NQ * H * D * 4))


def mask_view(mask) -> View:
    """mask: torch f16 [rows][N_padded] (ggml ne = [N, rows]): one plane for
    every head and sequence -- or contiguous [S'][H'][rows][N_padded] (ggml ne =
    [N, rows, H', S']): query head iq2 of sequence iq3 reads plane
    (iq2 % H', iq3 % S'); H' divides H, S' divides S (include/fattn.h)."""
    if mask.dim() == 4:
        if not mask.is_contiguous():
            raise ValueError("mask_view: a 4-D mask must be contiguous (build a View for other strides)")
        Sm, Hm, rows, Np = mask.shape
        return View(_tptr(mask), TYPE_F16, (Np, rows, Hm, Sm), (2, Np * 2, Np * rows * 2, Np * rows * Hm * 2))
    rows, Np = mask.shape
    return View(_tptr(mask), TYPE_F16, (Np, rows, 1, 1), (2, Np * 2, Np * rows * 2, Np * rows * 2))


class Attention:
    """Reusable FLASH_ATTN_EXT call: builds the params once, owns its workspace."""

    def __init__(self, q: View, k: View, v: View, mask: Optional[View], dst, scale: float, kv_chunk: int = 0, *,
                 max_bias: float = 0.0, logit_softcap: float = 0.0, n_head_total: int = 0, head_first: int = 0,
                 sinks=None, lse=None):
        import torch
        self.sinks = sinks   # ggml's src[4] (flash_attn_ext): a pointer, a torch f32 tensor (kept alive here) or None
        self.lse = lse       # where the rows' log-sum-exp goes (flash_attn_ext): a pointer, a torch f32 tensor or None
        self.p = ext_params(q, k, v, mask, _tptr(dst), scale, 0, 0, kv_chunk, max_bias=max_bias,
                            logit_softcap=logit_softcap, n_head_total=n_head_total, head_first=head_first)
        ws = workspace_size(self.p)
        # (zeroing is optional: each launch epoch-stamps the arrival words at its front)
        self.workspace = torch.zeros(max(ws, 16), dtype=torch.uint8, device=dst.device)
        self.p.workspace = _tptr(self.workspace)
        self.p.workspace_bytes = self.workspace.numel()
        self.dst = dst

    def retarget(self, q=None, k=None, v=None, dst=None, mask=None, sinks=None, lse=None):
        """Point the same call at other buffers with identical shapes/strides.
        None keeps what the call has.  sinks: another pointer or tensor of
        q.ne[2] f32 values, or fattn.NO_SINKS to launch without sinks again.
        lse: another pointer or tensor of S * n_q * H f32 values, or fattn.NO_LSE."""
        if lse is NO_LSE:
            self.lse = None
        elif lse is not None:
            self.lse = lse
        if sinks is NO_SINKS:
            self.sinks = None
        elif sinks is not None:
            self.sinks = sinks
        if mask is not None:
            self.p.mask.data = mask
        if q is not None:
            self.p.q.data = q
        if k is not None:
            self.p.k.data = k
        if v is not None:
            self.p.v.data = v
        if dst is not None:
            self.p.dst = dst

    def describe(self) -> str:
        return describe(self.p)

    def __call__(self, stream=None, ev_begin=None, ev_end=None):
        flash_attn_ext(self.p, stream, ev_begin, ev_end, sinks=self.sinks, lse=self.lse)
        return self.dst


def quantize(x, typ: int, stream=None):
    """f32 [rows, k] (cuda) -> ggml blocks uint8 [rows, k/32*bytes] (bit-exact ggml quantize_row_*_ref);
    TYPE_BF16: the bf16 bits, uint8 [rows, 2k] little endian (ggml_compute_fp32_to_bf16, any k)."""
    import torch
    assert x.dtype == torch.float32 and x.is_contiguous()
    k = x.shape[-1]
    rows = x.numel() // k
    out = torch.empty((rows, row_size(typ, k)), dtype=torch.uint8, device=x.device)
    _check(lib().fattn_quantize(typ, _tptr(x), _tptr(out), k, rows, _stream(stream)), "fattn_quantize")
    return out


def cpy(src: View, dst: View, stream=None):
    """GGML_OP_CPY f32 -> F16 / BF16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 into a strided view (the KV-cache
    write, include/fattn.h fattn_cpy); src/dst are ggml views of device memory."""
    s, d = src.c(), dst.c()
    _check(lib().fattn_cpy(C.byref(s), C.byref(d), _stream(stream)), "fattn_cpy")


def set_rows(src: View, idx: View, dst: View, stream=None):
    """GGML_OP_SET_ROWS f32 -> F16 / Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1: the KV-cache write by slot
    index (include/fattn.h fattn_set_rows).  src: f32 ne = [ne0, nr, ne2, ne3];
    idx: TYPE_I64 or TYPE_I32 ne = [nr, ne11, ne12, 1] in device memory; dst: the
    cache, ne = [ne0, n_slots, ne2, ne3].  Row i of plane (i2, i3) is converted
    into slot idx[i, i2 % ne11, i3 % ne12]; a slot outside [0, n_slots) writes
    nothing.  The slots are read on the device, so a captured graph replays with
    whatever the index tensor then holds."""
    s, i, d = src.c(), idx.c(), dst.c()
    _check(lib().fattn_set_rows(C.byref(s), C.byref(i), C.byref(d), _stream(stream)), "fattn_set_rows")


def k_shift(k: View, shift: View, rope: FattnRope, freq_factors=None, stream=None):
    """The K-shift (include/fattn.h fattn_k_shift): rotate the K cache view k, ne =
    [ne0 <= 256, n_slots, Hkv, S] of any row type, IN PLACE by the RoPE of the
    position deltas in shift (TYPE_I32, ne = [n_slots, ns, 1, 1], device memory;
    sequence i3 reads plane i3 % ns).  rope: a FattnRope (rope_params()).
    freq_factors: None, a raw device pointer, or a contiguous float32 device
    tensor of exactly rope.n_dims / 2 values.  Rows whose delta is 0 and blocks at
    or past n_dims keep their bytes.  The deltas are read on the device, so a
    captured graph replays with whatever the shift tensor then holds."""
    fptr = freq_factors
    if freq_factors is not None and not isinstance(freq_factors, int):
        import torch
        if freq_factors.dtype != torch.float32 or not freq_factors.is_contiguous() or not freq_factors.is_cuda:
            raise ValueError("k_shift: freq_factors must be a contiguous float32 device tensor")
        if freq_factors.numel() != int(rope.n_dims) // 2:
            raise ValueError(f"k_shift: {freq_factors.numel()} freq_factors for n_dims / 2 = {int(rope.n_dims) // 2} pairs")
        fptr = _tptr(freq_factors)
    kc, sc = k.c(), shift.c()
    _check(lib().fattn_k_shift(C.byref(kc), C.byref(sc), fptr, C.byref(rope), _stream(stream)), "fattn_k_shift")


def dequantize(blocks, typ: int, k: int, stream=None):
    """ggml blocks (or f16 / bf16 bits, in a tensor of any element size) -> f32 [rows, k]
    (bit-exact ggml dequantize_row_*; bf16: exact, the bits shifted up)."""
    import torch
    rows = blocks.numel() * (1 if typ not in (TYPE_F16, TYPE_BF16) else blocks.element_size()) // max(1, row_size(typ, k))
    out = torch.empty((rows, k), dtype=torch.float32, device=blocks.device)
    _check(lib().fattn_dequantize(typ, _tptr(blocks), _tptr(out), k, rows, _stream(stream)), "fattn_dequantize")
    return out


def row(query, key, value_t, mask, qkv, head_dim: int, kv_size: int, num_heads: int, scale: float,
        head_stride: int, r_kv_heads: int, tmp=None, stream=None):
    """flash_attn_row + fa_reduce (src/flash_row_float.h:4-6,415-416): key f16
    [Hkv][N][D], value f16 transposed [Hkv][D][N], mask f16 [N], qkv f32 [H][D]."""
    import torch
    need = int(lib().fattn_row_workspace_size(head_dim, kv_size, num_heads))
    if tmp is None:
        tmp = torch.zeros(max(need, 16), dtype=torch.uint8, device=qkv.device)
    _check(lib().fattn_row(_tptr(query), _tptr(key), _tptr(value_t), _tptr(mask) if mask is not None else None,
                           _tptr(tmp), tmp.numel() * tmp.element_size(), _tptr(qkv), head_dim, kv_size, num_heads,
                           float(scale), head_stride, r_kv_heads, _stream(stream)), "fattn_row")
    return qkv
