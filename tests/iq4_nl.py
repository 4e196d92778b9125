"""ggml's IQ4_NL block (Q4_0's 18 bytes f16 d; u8 qs[16]; x = h(d) * KV[q]) and its cache-write quantiser in numpy,
every f32 operation rounded on its own: d0 = (first element of largest |x|) / -127; q = the entry of KV nearest to
x / d0, a tie going up; d = sumqx / sumq2 (sequential sums over j = 0..15 of the terms (w v x)[j] + (w v x)[j + 16]
and (w v v)[j] + (w v v)[j + 16], w = x x, v = KV[q]) where sumq2 > 0, else d0.
Importing the module registers the type in kv_types.KV_TYPES (reference_pair / cached_pair / check serve it)."""
import numpy as np

import kv_types as kt

F, QK = np.float32, 32
TYPE_IQ4_NL, BLOCK_BYTES, NAME = 20, 18, "iq4_nl"
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=F)
KAT_HEX = "54a95c4c4c4b3b3a3a292928181717160605"     # quantize(kv_types.kat_input())


def best_index(v: np.ndarray) -> np.ndarray:
    m = np.clip(np.searchsorted(KV, v, side="right") - 1, 0, 14)     # KV[m] <= v < KV[m + 1] inside the table's range
    down = (v - KV[m]).astype(F) < (KV[m + 1] - v).astype(F)
    return np.where(v <= KV[0], 0, np.where(v >= KV[15], 15, np.where(down, m, m + 1)))


def quantize(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=F)
    xb = x.reshape(-1, QK)
    n = len(xb)
    a = np.abs(xb)
    vmax = np.where(a.max(axis=1) > 0, xb[np.arange(n), a.argmax(axis=1)], F(0.0)).astype(F)   # argmax: the first of the largest
    d0 = (vmax / F(-127.0)).astype(F)
    with np.errstate(divide="ignore"):
        idv = np.where(d0 != 0, F(1.0) / d0, F(0.0)).astype(F)
    q = best_index((xb * idv[:, None]).astype(F))
    v = KV[q]
    wv = ((xb * xb).astype(F) * v).astype(F)
    tx, t2 = (wv * xb).astype(F), (wv * v).astype(F)
    sumqx, sumq2 = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    for j in range(QK // 2):
        sumqx = (sumqx + (tx[:, j] + tx[:, j + 16]).astype(F)).astype(F)
        sumq2 = (sumq2 + (t2[:, j] + t2[:, j + 16]).astype(F)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(sumq2 > 0, sumqx / sumq2, d0).astype(F)
    out = np.zeros((n, BLOCK_BYTES), dtype=np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
    out[:, 2:] = (q[:, :16] | (q[:, 16:] << 4)).astype(np.uint8)
    return out.reshape(x.shape[:-1] + (x.shape[-1] // QK * BLOCK_BYTES,))


def dequantize(rows: np.ndarray, D: int) -> np.ndarray:
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    b = rows.reshape(-1, BLOCK_BYTES)
    d = np.ascontiguousarray(b[:, 0:2]).view(np.float16).reshape(-1).astype(F)
    q = np.concatenate([b[:, 2:] & 15, b[:, 2:] >> 4], axis=1)
    return (d[:, None] * KV[q]).astype(F).reshape(rows.shape[:-1] + (D,))


KVT = kt.KvType(NAME, TYPE_IQ4_NL, BLOCK_BYTES, lambda x: x, quantize, dequantize, lambda x: kt.edge_blocks().reshape(2, 128),
                "KVT " + NAME + " {tag} rel={rel:.3e} elem={elem:.3f} | {desc}", False)
kt.KV_TYPES[NAME] = KVT
