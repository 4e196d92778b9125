"""The launch side of the suites: a tests/problems.Problem through the GPU path
(fattn -> libfattn.so), the guarded launcher that shows nothing is written
outside dst and the workspace, the error-bar check, graph capture and replay,
and the kernel_test harness."""
from __future__ import annotations

import os
import subprocess

import numpy as np

import fattn
from problems import Problem, attn_elem_err, attn_rel_err

RTOL = 1e-3
KERNEL_TEST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ggml-cuda-experiments_amd",
                           "bin", "kernel_test")


def upload(prob: Problem, dev="cuda"):
    import torch
    t = {
        "q": torch.from_numpy(np.ascontiguousarray(prob.q)).to(dev),
        "k": torch.from_numpy(prob.k_bytes).to(dev),
        "v": torch.from_numpy(prob.v_bytes).to(dev),
        "mask": (torch.from_numpy(np.ascontiguousarray(prob.mask_bits).view(np.int16)).to(dev)
                 if prob.mask_bits is not None else None),
        "dst": torch.full((prob.S, prob.NQ, prob.H, prob.D), float("nan"), dtype=torch.float32, device=dev),
    }
    return t


def views(prob: Problem, t):
    qv = fattn.View(t["q"].data_ptr(), fattn.TYPE_F32, prob.q_ne, prob.q_nb)
    kv = fattn.View(t["k"].data_ptr(), prob.kv_type, prob.kv_ne, prob.k_nb)
    vv = fattn.View(t["v"].data_ptr(), prob.v_type, prob.kv_ne, prob.v_nb)
    mv = fattn.View(t["mask"].data_ptr(), fattn.TYPE_F16, prob.mask_ne, prob.mask_nb) if t["mask"] is not None else None
    return qv, kv, vv, mv


def run_described(prob: Problem, dev="cuda", kv_chunk: int = 0):
    """(output, describe()) of prob through fattn.Attention."""
    import torch
    t = upload(prob, dev)
    att = fattn.Attention(*views(prob, t), t["dst"], prob.scale, kv_chunk=kv_chunk)
    desc = att.describe()
    att()
    torch.cuda.synchronize()
    return t["dst"].cpu().numpy(), desc


def run_gpu(prob: Problem, kv_chunk: int = 0, dev="cuda") -> np.ndarray:
    return run_described(prob, dev, kv_chunk)[0]


def check_bars(got, ref, line):
    """The suite's two bars: attn_rel_err <= 1e-3 and attn_elem_err <= 1 (NaN
    positions must coincide: both are inf otherwise).  line(rel, elem) is the
    caller's figure line, printed before anything is asserted."""
    rel, elem = attn_rel_err(got, ref), attn_elem_err(got, ref)
    text = line(rel, elem)
    print(text)
    assert rel <= RTOL, text
    assert elem <= 1.0, text
    return rel, elem


# ------------------------------------------------------------------ the guarded launcher

DST_GUARD_BYTES = 4096
SENTINEL = 0x5A5AA5A5   # a finite f32 (1.5e16), distinct from the NaN pre-fill
WS_TAIL_BYTES = 4096


class GuardedLaunch:
    """One fattn_ext launch that can show it wrote nowhere else: dst (f32
    [*out_shape], pre-filled with NaN) sits inside a larger tensor with 4 KiB of
    sentinel before and after it; the workspace is sized to exactly
    fattn.workspace_size() inside a larger buffer with a sentinel tail and is
    zeroed once -- or handed in (`ws`: a workspace shared with other launches;
    the 4 KiB behind this launch's share of it are what is compared).

    params_for(dst pointer) -> the fattn params, without a workspace; tensors:
    the launch's inputs by name, kept alive as .t; sinks: f32, one per q head."""

    def __init__(self, params_for, out_shape, tensors=None, dev="cuda", sinks=None, ws=None):
        import torch
        self.t = tensors
        self.out_shape = tuple(out_shape)
        self.n_out = int(np.prod(self.out_shape))
        g = DST_GUARD_BYTES // 4
        self.dst_all = torch.full((g + self.n_out + g,), SENTINEL, dtype=torch.int32, device=dev)
        self.dst = self.dst_all[g:g + self.n_out].view(torch.float32)
        self.dst.fill_(float("nan"))
        self.sinks_t = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks, dtype=np.float32)).to(dev)
        self.p = params_for(self.dst.data_ptr())
        self.ws_bytes = fattn.workspace_size(self.p)
        self.own_ws = ws is None
        if ws is None:
            ws = torch.full(((self.ws_bytes + 3) // 4 + WS_TAIL_BYTES // 4,), SENTINEL, dtype=torch.int32, device=dev)
            ws.view(torch.uint8)[:self.ws_bytes].zero_()
        self.ws_all = ws
        if self.ws_bytes:
            assert ws.numel() * 4 >= self.ws_bytes
            self.p.workspace = ws.data_ptr()
            self.p.workspace_bytes = self.ws_bytes

    def describe(self) -> str:
        return fattn.describe(self.p)

    def launch(self, stream=None):
        fattn.flash_attn_ext(self.p, stream, sinks=self.sinks_t)

    def run(self) -> np.ndarray:
        """The whole dst allocation, f32 [*out_shape]."""
        import torch
        self.dst.fill_(float("nan"))
        self.launch()
        torch.cuda.synchronize()
        return self.dst.cpu().numpy().reshape(self.out_shape)

    def guards_intact(self) -> bool:
        """dst's guard bands and the workspace tail still hold the sentinel."""
        import torch
        g = DST_GUARD_BYTES // 4
        d = self.dst_all.cpu().numpy().view(np.uint32)
        end = None if self.own_ws else self.ws_bytes + WS_TAIL_BYTES
        w = self.ws_all.view(torch.uint8)[self.ws_bytes:end].cpu().numpy()
        want = np.full(len(w) // 4 + 2, SENTINEL, dtype=np.uint32).view(np.uint8)[self.ws_bytes % 4:][:len(w)]
        return bool((d[:g] == SENTINEL).all() and (d[g + self.n_out:] == SENTINEL).all() and np.array_equal(w, want))


# ------------------------------------------------------------------ graph capture

def capture(launch):
    """launch(stream handle) run once on a side stream, then captured on it: the torch.cuda.CUDAGraph."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        launch(s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(s.cuda_stream)
    return g


def graph_replay(launch, dst, replays: int = 2):
    """capture(launch), then `replays` replays, each onto a NaN-filled dst:
    (the eager launch's output, [every replay's output])."""
    import torch
    g = capture(launch)
    eager = dst.cpu().numpy().copy()   # (capturing launched nothing: still the eager launch's)
    outs = []
    for _ in range(replays):
        dst.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        outs.append(dst.cpu().numpy().copy())
    return eager, outs


# ------------------------------------------------------------------ the kernel_test harness

def run_kernel_test(args, timeout=120):
    """kernel_test with args: the subprocess.CompletedProcess (text).  A missing binary fails the test."""
    import pytest
    if not os.path.exists(KERNEL_TEST):
        pytest.fail(f"{KERNEL_TEST} not built (make harness)")
    return subprocess.run([KERNEL_TEST] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
