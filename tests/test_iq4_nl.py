"""CPU: the IQ4_NL KV-cache type -- constants, the known-answer block, its plans over fake pointers, the refusals."""
import numpy as np
import pytest

import fattn
import iq4_nl as iq
import kv_types as kt
from plans import plan_params as _params

T = iq.TYPE_IQ4_NL


def test_constants_and_known_answer_block():
    assert fattn.TYPE_IQ4_NL == 20 == T and fattn.TYPE_NAMES["iq4_nl"] == 20 and T in fattn.BLOCK_TYPES
    assert fattn.BLOCK_BYTES[T] == fattn.row_size(T, 32) == 18
    assert fattn.row_size(T, 128) == 72 and fattn.row_size(T, 100) == 0
    b = iq.quantize(kt.kat_input())                       # x[j] = (j - 10) * 0.25
    y = iq.dequantize(b, 32)
    assert b.tobytes().hex() == iq.KAT_HEX and float(b[:2].view(np.float16)[0]) == -0.0416259765625
    assert (y[0], y[17], y[31]) == (np.float32(-2.2061768), np.float32(2.0396729), np.float32(5.286499))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_plans(D):
    for kw in ({}, dict(H=32, Hkv=8, N=8192), dict(NQ=64)):
        d = fattn.describe(_params(D=D, kt=T, **kw))
        assert d.startswith(f"fattn_split_kernel<iq4_nl,iq4_nl,D{D},"), d
    with fattn.options({fattn.OPT_PF: 2}):
        d = fattn.describe(_params(D=D, NQ=256, H=2, Hkv=2, N=192, kt=T))
    assert ("kv_stage_f16<iq4_nl>" in d and f"<f16,D{D}" in d) if D < 256 else d.startswith("fattn_split_kernel<iq4_nl,"), d


def test_refusals():
    def status(**kw):
        with pytest.raises(Exception) as e:
            fattn.describe(_params(**kw))
        return str(e.value)
    for other in (fattn.TYPE_F16, fattn.TYPE_BF16, fattn.TYPE_Q8_0, fattn.TYPE_Q4_0, fattn.TYPE_Q5_0):
        assert "UNSUPPORTED_TYPE" in status(kt=T, vt=other) and "UNSUPPORTED_TYPE" in status(kt=other, vt=T)
    N = 4096
    assert "UNSUPPORTED_TYPE" in status(kt=T, vt=fattn.TYPE_F16, v_nb=(N * 2, 2, 128 * N * 2, 128 * N * 2 * 32))   # transposed V
    assert "UNSUPPORTED_TYPE" in status(kt=T, D=576, dk=576, dv=512, Hkv=1)                                          # the MLA pair
    assert "UNSUPPORTED_HEAD_DIM" in status(kt=T, D=80) and "UNSUPPORTED_HEAD_DIM" in status(kt=T, D=96)
