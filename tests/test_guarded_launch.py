"""CPU: gpu_util.GuardedLaunch's own checks, on host tensors and fake input
pointers -- nothing launches.  One word written into dst's leading band, its
trailing band or the workspace tail must turn guards_intact() false."""
import numpy as np
import pytest
import torch

import fattn
from gpu_util import DST_GUARD_BYTES, SENTINEL, WS_TAIL_BYTES, GuardedLaunch
from plans import plan_params

SHAPE = (1, 1, 32, 128)     # plan_params' default: one-row tiles over several chunks, so a workspace


def _launch(ws=None):
    def params_for(dst):
        p = plan_params()
        p.dst = dst
        return p
    return GuardedLaunch(params_for, SHAPE, dev="cpu", ws=ws)


def test_untouched_guards_are_intact():
    g = _launch()
    assert (DST_GUARD_BYTES, WS_TAIL_BYTES, SENTINEL) == (4096, 4096, 0x5A5AA5A5)
    assert g.ws_bytes == fattn.workspace_size(g.p) > 0 and g.p.workspace_bytes == g.ws_bytes
    assert g.dst.shape == (int(np.prod(SHAPE)),) and torch.isnan(g.dst).all()
    assert g.dst_all.numel() == g.n_out + 2 * (DST_GUARD_BYTES // 4)
    assert (g.ws_all.view(torch.uint8)[:g.ws_bytes] == 0).all()
    assert g.ws_all.numel() * 4 - g.ws_bytes == WS_TAIL_BYTES + (-g.ws_bytes) % 4
    assert g.guards_intact()
    g.dst.fill_(1.0)                                     # what a launch may write: all of dst, all of the workspace
    g.ws_all.view(torch.uint8)[:g.ws_bytes].fill_(0xFF)
    assert g.guards_intact()


@pytest.mark.parametrize("where", ["lead_first", "lead_last", "trail_first", "trail_last", "ws_tail_first", "ws_tail_last"])
def test_one_word_outside_breaks_the_guards(where):
    g = _launch()
    n, band = g.n_out, DST_GUARD_BYTES // 4
    buf, i = {"lead_first": (g.dst_all, 0), "lead_last": (g.dst_all, band - 1), "trail_first": (g.dst_all, band + n),
              "trail_last": (g.dst_all, band + n + band - 1), "ws_tail_first": (g.ws_all, (g.ws_bytes + 3) // 4),
              "ws_tail_last": (g.ws_all, g.ws_all.numel() - 1)}[where]
    assert int(buf[i]) == SENTINEL
    buf[i] = 0
    assert not g.guards_intact()


def test_handed_in_workspace_compares_the_window_behind_its_share():
    probe = _launch()
    extra = 64
    ws = torch.full(((probe.ws_bytes + 3) // 4 + WS_TAIL_BYTES // 4 + extra,), SENTINEL, dtype=torch.int32)
    g = _launch(ws=ws)
    assert g.ws_all is ws and g.p.workspace == ws.data_ptr() and g.p.workspace_bytes == g.ws_bytes == probe.ws_bytes
    assert g.guards_intact()
    ws[-1] = 0                                           # behind the 4 KiB window: another launch's share
    assert g.guards_intact()
    ws[(g.ws_bytes + WS_TAIL_BYTES) // 4 - 1] = 0        # the window's last word
    assert not g.guards_intact()
