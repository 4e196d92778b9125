"""Heads x batch sharding across the GPUs of one node.

Heads (and ggml ne03 sequences) are independent attention problems: softmax
is per (sequence, head, query row) and the split-KV merge stays on one GPU,
so the path partitions with no collective on the data path.  A rank owns a
contiguous range of kv-heads together with their r = H/Hkv query heads (the
GQA broadcast ik2 = iq2 / r of src/flash-llama.h:128-140 never crosses a
shard), runs the unchanged single-GPU kernel on its slice, and the per-rank
outputs are collected with ONE all_gather (RCCL over xGMI on the GPU box,
gloo in the CPU tests) followed by a local permute into the ggml dst layout
[S][n_q][H][D] (src/flash-llama.h:434).
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class HeadShard:
    rank: int
    world: int
    kv0: int   # first kv-head owned
    kv1: int   # one past the last kv-head owned
    h0: int    # first q-head owned (= kv0 * r)
    h1: int
    H: int = 0  # q heads of the unsharded problem (0: unknown, a hand-built shard)

    @property
    def n_kv(self) -> int:
        return self.kv1 - self.kv0

    @property
    def n_heads(self) -> int:
        return self.h1 - self.h0

    def slope_args(self) -> dict:
        """What the rank's launch needs for the GLOBAL ALiBi slopes (max_bias):
        its slice's q head 0 is head h0 of H, so
        `fattn.ext_params(..., max_bias=b, **sh.slope_args())`.  Launched with
        the defaults instead, a slice would take the slopes of heads
        0 .. n_heads-1 of an n_heads-head model -- silently wrong."""
        if self.H <= 0:
            raise ValueError("HeadShard.H (the unsharded head count) is not set")
        return {"n_head_total": self.H, "head_first": self.h0}

    def sink_slice(self, sinks):
        """The rank's attention sinks: sinks[h0:h1] of the unsharded model's H
        values (a torch tensor or numpy array: a view).  fattn_ext_sinks indexes
        its array by the launch's LOCAL q head, so -- unlike the slopes, which
        come from a formula over the global head index -- a slice takes its own
        slice.  Passing the unsliced array would give every rank heads
        0 .. n_heads-1's sinks: silently wrong."""
        if self.H > 0 and len(sinks) != self.H:
            raise ValueError(f"sink_slice: {len(sinks)} sinks for {self.H} heads")
        return sinks[self.h0:self.h1]


def shard_heads(H: int, Hkv: int, world: int, rank: int) -> HeadShard:
    """Contiguous kv-head groups; every rank gets the same count (the gather
    needs equal slices), so world must divide Hkv."""
    if H % Hkv:
        raise ValueError(f"H={H} not a multiple of Hkv={Hkv}")
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    if Hkv % world:
        raise ValueError(f"Hkv={Hkv} kv-heads do not split evenly over {world} ranks")
    r = H // Hkv
    per = Hkv // world
    kv0 = rank * per
    return HeadShard(rank, world, kv0, kv0 + per, kv0 * r, (kv0 + per) * r, H)


def narrow(view, dim: int, start: int, count: int):
    """Zero-copy sub-view of a ggml view (fattn.View): elements [start, start+count)
    of ggml dimension `dim` -- the pointer moves by start * nb[dim], the
    strides stay.  `view.ptr` may be a device pointer or a byte offset."""
    from fattn import View
    if not 0 <= start <= start + count <= view.ne[dim]:
        raise ValueError(f"narrow dim {dim} [{start}, {start + count}) of {view.ne[dim]}")
    ne = list(view.ne)
    ne[dim] = count
    return View(view.ptr + start * view.nb[dim], view.type, tuple(ne), tuple(view.nb))


def head_views(q, k, v, sh: HeadShard):
    """The rank's FLASH_ATTN_EXT sub-problem, zero-copy: q heads [h0, h1) and
    kv heads [kv0, kv1) (ggml dim 2 of q / k / v).  The mask is shared by all
    heads (a row per query) and the rank's dst is its own contiguous
    [S][n_q][h1-h0][D] (with max_bias the slopes are per GLOBAL head: pass
    sh.slope_args() to ext_params / Attention); the GQA map ik2 = iq2 / r (src/flash-llama.h:128-140)
    holds inside the slice because h0 = kv0 * r."""
    return narrow(q, 2, sh.h0, sh.n_heads), narrow(k, 2, sh.kv0, sh.n_kv), narrow(v, 2, sh.kv0, sh.n_kv)


def assemble_heads(parts):
    """[world] x [..., S, n_q, H/world, D] per-rank outputs stacked on a leading
    axis -> [..., S, n_q, H, D] in the ggml dst layout (src/flash-llama.h:434):
    rank w holds heads [w*Hl, (w+1)*Hl).  Works on torch tensors and numpy."""
    world = parts.shape[0]
    *lead, S, NQ, Hl, D = parts.shape[1:]
    nl = len(lead)
    perm = tuple(range(1, 1 + nl)) + (1 + nl, 2 + nl, 0, 3 + nl, 4 + nl)
    x = parts.permute(*perm) if hasattr(parts, "permute") else parts.transpose(perm)
    return x.reshape(*lead, S, NQ, world * Hl, D)


def gather_heads(local, group=None, buf=None, out=None):
    """local: this rank's output [..., S, n_q, H/world, D] (contiguous).  Returns
    the full [..., S, n_q, H, D] on every rank via ONE all_gather_into_tensor
    (RCCL over xGMI on the GPU box, gloo on the CPU) and assemble_heads.
    `buf` ([world, *local.shape]) and `out` (the full shape), when given, are
    used instead of fresh allocations -- the form a captured HIP graph replays
    (the gather lands in `buf`, the permute writes `out`)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if buf is None:
        buf = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(buf.view(world * local.shape[0], *local.shape[1:]), local.contiguous(), group=group)
    if out is None:
        return assemble_heads(buf)
    # one strided copy: out seen as [..., S, n_q, world, H/world, D]
    *lead, S, NQ, Hl, D = buf.shape[1:]
    nl = len(lead)
    perm = tuple(range(1, 1 + nl)) + (1 + nl, 2 + nl, 0, 3 + nl, 4 + nl)
    out.view(*lead, S, NQ, world, Hl, D).copy_(buf.permute(*perm))
    return out


# ------------------------------------------------------------------ KV (context) sharding
# Heads do not split an MLA op (one kv head) or a cache too long for one GPU:
# there the KEYS split.  Each rank attends to its own contiguous key range
# and returns (out, lse) -- fattn.flash_attn_ext(..., lse=) -- and one
# all-gather plus fattn.lse_merge() give the exact result (include/fattn.h,
# fattn_lse_merge).  Sinks go to the merge, once, never to the shard launches.

def kv_ranges(N: int, world: int, align: int = 32):
    """[(lo, hi)] * world: contiguous key ranges that partition [0, N), every
    boundary a multiple of `align`, the last range taking the remainder.  align =
    32 keeps the 16-byte paths and whole ggml blocks; every range is non-empty,
    so N must hold at least `world` aligned pieces."""
    if world <= 0 or align <= 0:
        raise ValueError(f"kv_ranges: world {world}, align {align}")
    per = N // world // align * align
    if per <= 0:
        raise ValueError(f"kv_ranges: {N} keys do not give {world} ranges of a multiple of {align}")
    return [(w * per, (w + 1) * per if w + 1 < world else N) for w in range(world)]


def kv_views(k, v, mask, lo: int, hi: int):
    """The FLASH_ATTN_EXT sub-problem over keys [lo, hi), zero-copy: `narrow` on
    ggml dim 1 of K and V and on dim 0 of the mask (None stays None).  V moves
    by the same rows as K, so an MLA V that is a view of K (v = k + off, same
    strides) stays one.  The range that ends at the last key keeps the mask
    rows' padding past it (rows are read in dword pieces).  lo a multiple of 32
    keeps every alignment rule of the unsharded views."""
    N = int(k.ne[1])
    if not 0 <= lo < hi <= N:
        raise ValueError(f"kv_views: keys [{lo}, {hi}) of {N}")
    kk, vv = narrow(k, 1, lo, hi - lo), narrow(v, 1, lo, hi - lo)
    mm = None
    if mask is not None:
        mm = narrow(mask, 0, lo, (int(mask.ne[0]) if hi == N else hi) - lo)
    return kk, vv, mm


def gather_parts(out, lse, group=None):
    """out: this rank's [..., dv] output over its key range, lse: its [...]
    log-sum-exps (both contiguous).  Returns ([world, ..., dv], [world, ...]) on
    every rank by one all_gather_into_tensor each: fattn.lse_merge()'s inputs."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    outs = torch.empty((world,) + tuple(out.shape), dtype=out.dtype, device=out.device)
    lses = torch.empty((world,) + tuple(lse.shape), dtype=lse.dtype, device=lse.device)
    dist.all_gather_into_tensor(outs.view(-1), out.contiguous().view(-1), group=group)
    dist.all_gather_into_tensor(lses.view(-1), lse.contiguous().view(-1), group=group)
    return outs, lses
