"""CPU: the Q4_1 / Q5_0 / Q5_1 KV-cache types -- row sizes, the numpy
restatement of the formats (tests/kv_types.py) against the known-answer
blocks, the plans the planner picks for them, and what stays rejected."""
import json
import os

import numpy as np
import pytest

import fattn
import kv_types as kt
from plans import plan_params as _params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kv_types_kat.json")
NAMES = ("q4_1", "q5_0", "q5_1")


def test_constants():
    assert (fattn.TYPE_Q4_1, fattn.TYPE_Q5_0, fattn.TYPE_Q5_1) == (3, 6, 7)
    for n in NAMES:
        assert fattn.TYPE_NAMES[n] == kt.TYPES[n]
        assert fattn.BLOCK_BYTES[kt.TYPES[n]] == kt.BLOCK_BYTES[kt.TYPES[n]]


def test_row_size():
    assert fattn.row_size(fattn.TYPE_Q4_1, 128) == 80
    assert fattn.row_size(fattn.TYPE_Q5_0, 128) == 88
    assert fattn.row_size(fattn.TYPE_Q5_1, 128) == 96
    for t in kt.TYPES.values():
        assert fattn.row_size(t, 32) == kt.BLOCK_BYTES[t]
        assert fattn.row_size(t, 100) == 0
    assert fattn.row_size(5, 128) == 0   # (ggml's removed Q4_3 slot: not a type)


@pytest.mark.parametrize("name", NAMES)
def test_known_answer_blocks(name):
    """x[j] = (j - 10) * 0.25 through the numpy restatement: the bytes and the
    dequantised values of the committed known-answer file."""
    kat = json.load(open(GOLDEN))
    t = kt.TYPES[name]
    x = kt.kat_input()
    b = kt.quantize(x, t)
    assert b.shape == (kt.BLOCK_BYTES[t],)
    assert b.tobytes().hex() == kat[name]["bytes"]
    y = kt.dequantize(np.frombuffer(bytes.fromhex(kat[name]["bytes"]), dtype=np.uint8), t, 32)
    for j, want in kat[name]["y"].items():
        assert y[int(j)] == np.float32(want), (j, y[int(j)], want)
    if kat[name]["exact"]:
        assert np.array_equal(y, x)


def test_known_answer_values():
    """The values the formats' definition gives for the three blocks, spelled out."""
    kat = json.load(open(GOLDEN))
    assert kat["q4_1"]["bytes"] == "223800c180809191a2a2b3b3c4c4d5d5e6e6f7f7"
    assert kat["q5_0"]["bytes"] == "40b5ff070000b8b7a695858473625251403f2e2e1d0c"
    assert kat["q5_1"]["bytes"] == "003400c10000ffff00112233445566778899aabbccddeeff"
    assert kat["q4_1"]["y"] == {"0": -2.5, "17": 1.6328125, "31": 5.2490234375}
    assert kat["q5_0"]["y"] == {"0": -2.625, "17": 1.640625, "31": 5.25}


@pytest.mark.parametrize("name", NAMES)
def test_numpy_round_trip_bounds(name):
    """dequantize(quantize(x)) stays within half a code step of x (Q5_0: one
    step at the clamped end), and edge blocks quantise without NaN."""
    t = kt.TYPES[name]
    rng = np.random.default_rng(5)
    x = (1.0 - 2.0 * rng.random((64, 128), dtype=np.float32)).astype(np.float32)
    y = kt.dequantize(kt.quantize(x, t), t, 128)
    step = {"q4_1": 2.0 / 15, "q5_0": 1.0 / 16, "q5_1": 2.0 / 31}[name]
    assert np.abs(y - x).max() <= step * (1.01 if name == "q5_0" else 0.51) + 2e-3
    e = kt.edge_blocks()
    ye = kt.dequantize(kt.quantize(e, t), t, 32)
    assert np.isfinite(ye).all()
    assert np.all(ye[0] == 0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_decode_plans_are_the_split_kernel(name, D):
    d = fattn.describe(_params(D=D, kt=kt.TYPES[name]))
    assert d.startswith(f"fattn_split_kernel<{name},{name},D{D},"), d
    d = fattn.describe(_params(D=D, kt=kt.TYPES[name], H=32, Hkv=8, N=8192))   # GQA decode
    assert d.startswith(f"fattn_split_kernel<{name},{name},D{D},"), d


@pytest.mark.parametrize("name", NAMES)
def test_prefill_plans_stage_to_f16(name):
    t = kt.TYPES[name]
    with fattn.options({fattn.OPT_PF: 2}):
        d = fattn.describe(_params(NQ=256, H=2, Hkv=2, N=192, kt=t))
        assert f"kv_stage_f16<{name}>" in d and "fattn_pf4_kernel(lean)<f16,D128" in d, d
        d = fattn.describe(_params(D=64, NQ=256, H=2, Hkv=2, N=192, kt=t))
        assert f"kv_stage_f16<{name}>" in d and "fattn_pf_kernel<f16,D64" in d, d
        # D = 256 has no prefill body: the split kernel
        assert fattn.describe(_params(D=256, NQ=256, H=2, Hkv=2, N=192, kt=t)).startswith(f"fattn_split_kernel<{name},")
        # without the staging there is no prefill form of these types: the split kernel
        with fattn.options({fattn.OPT_PF: 2, fattn.OPT_PF_STAGE: 1}):
            assert fattn.describe(_params(NQ=256, H=2, Hkv=2, N=192, kt=t)).startswith(f"fattn_split_kernel<{name},")
    # the auto prefill shape
    assert f"kv_stage_f16<{name}>" in fattn.describe(_params(NQ=4096, kt=t))


@pytest.mark.parametrize("name", NAMES)
def test_batched_shapes_are_the_split_kernel(name):
    """No multi-query, batched-decode or role-form kernel takes these types (a known gap)."""
    t = kt.TYPES[name]
    for kw in (dict(NQ=64), dict(NQ=256), dict(NQ=64, D=64), dict(NQ=4096, D=256, H=16, Hkv=16)):
        d = fattn.describe(_params(kt=t, **kw))
        assert d.startswith(f"fattn_split_kernel<{name},{name},"), d
    with fattn.options({fattn.OPT_BD: 3}):
        assert fattn.describe(_params(NQ=64, kt=t)).startswith("fattn_split_kernel<")
    with fattn.options({fattn.OPT_SPLIT_LOADERS: 2}):
        assert fattn.describe(_params(kt=t)).startswith("fattn_split_kernel<")


def test_rejections():
    def status(**kw):
        with pytest.raises(Exception) as e:
            fattn.describe(_params(**kw))
        return str(e.value)
    for t in kt.TYPES.values():
        assert "UNSUPPORTED_HEAD_DIM" in status(D=96, kt=t)
        assert "UNSUPPORTED_HEAD_DIM" in status(D=80, kt=t)
        for other in (fattn.TYPE_Q8_0, fattn.TYPE_Q4_0, fattn.TYPE_F16):
            assert "UNSUPPORTED_TYPE" in status(kt=t, vt=other)
            assert "UNSUPPORTED_TYPE" in status(kt=other, vt=t)
    assert "UNSUPPORTED_TYPE" in status(kt=kt.TYPE_Q4_1, vt=kt.TYPE_Q5_1)
    assert "UNSUPPORTED_TYPE" in status(kt=5)
    assert "UNSUPPORTED_TYPE" in status(kt=fattn.TYPE_Q8_0, vt=5)
    assert "UNSUPPORTED_TYPE" in status(kt=4)


def test_existing_types_keep_their_plans():
    """The three types add no plan change: config 3 / 4 / 5 as tests/test_abi.py pins them."""
    assert "fattn_split_kernel<q8_0,q8_0,D128,gran16,mask,8waves>" in fattn.describe(_params())
    assert fattn.describe(_params(NQ=64)).startswith("fattn_bdp_kernel<q8_0")
    assert "kv_stage_f16<q4_0>" in fattn.describe(_params(NQ=4096, kt=fattn.TYPE_Q4_0))
