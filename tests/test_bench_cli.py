"""bench.py's command line: a plain `--gpus 1` run carries the value line only
(every other measurement is behind --full), and --dump-outputs writes the last
timed step's output, which is the attention of that step's inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from problems import attn_rel_err, oracle_of_dump as _oracle_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("strong_scaling_ref", "config5_seq64", "prefill", "prefill_random_mask", "prefill_inkernel_dequant",
             "cpu_baseline")


def test_full_and_dump_outputs_are_off_by_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs == "" and (a.steps, a.warmup) == (7, 3)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):  # --prefill-only times no decode step: nothing to dump
        bench.parse_args(["--prefill-only", "--dump-outputs", "d"])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step_output(tmp_path):
    npz, ddir = tmp_path / "in.npz", tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--rotate", "2",
           "--dump-out", str(npz), "--dump-outputs", str(ddir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step are the same measurement: bytes per step / time per step
    # (both rounded in the line: 5 decimals of a ms, 2 of a GB/s)
    assert line["value"] == pytest.approx(line["config"]["bytes_per_step"] / (line["ms_per_step"] * 1e-3) / 1e9,
                                          rel=5e-6 / line["ms_per_step"] + 1e-4)
    assert line["roofline"]["achieved"] > 0 and line["kernel_ms_avg"] > 0
    assert not [k for k in FULL_ONLY if k in line], "a plain run measures the value line only"
    assert line["kernel_ms_median"] is None and "peak_measured_copy" not in line["roofline"]
    assert sorted(os.listdir(ddir)) == ["out.npy"]
    out = np.load(ddir / "out.npy")
    d = np.load(npz)
    D, NQ, H, Hkv, N, typ, world = (int(x) for x in d["shape"])
    assert (D, NQ, H, Hkv, N, typ, world) == (128, 1, 32, 32, 4096, orc.TYPE_Q8_0, 1)
    assert out.dtype == np.float32 and out.shape == (1, NQ, H, D)
    assert np.array_equal(out, d["out"])  # the same buffer, read after the same (last) step
    ref = _oracle_of(d)
    assert attn_rel_err(out.reshape(ref.shape), ref) <= 1e-3
