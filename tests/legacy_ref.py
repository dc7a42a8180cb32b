"""Shared helpers of the tests for weights in Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL: directly sampled blocks, a NumPy twin of
dequantize_row written from the layouts in include/ggml_abi.h, and twins of the Q8_0 / Q8_1 activation quantisers."""
import ctypes as C

import numpy as np

import harness as T
import llama_box_amd as L

FORMATS = (L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1, L.IQ4_NL)
ONE = (L.Q4_1, L.Q5_1)      # {d, m, ...}: value = level * d + m, activations quantised to Q8_1
FIVE = (L.Q5_0, L.Q5_1)     # a fifth bit per value in qh
IQ4NL = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int32)


def qs_off(qt):
    return 2 + (2 if qt in ONE else 0) + (4 if qt in FIVE else 0)


def make_blocks(qt, d, m, levels):
    """Blocks from f16-representable d [n], m [n] (ignored without an m field) and integer levels [n, 32] (0..15, or 0..31 with a fifth bit)."""
    levels = np.asarray(levels, dtype=np.uint32)
    n = levels.shape[0]
    out = np.zeros((n, L.TYPE_SIZE[qt]), dtype=np.uint8)
    out[:, 0:2] = np.asarray(d, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    if qt in ONE:
        out[:, 2:4] = np.asarray(m, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    if qt in FIVE:
        qh = np.zeros(n, dtype=np.uint32)
        for j in range(32):
            qh |= ((levels[:, j] >> 4) & 1) << j
        out[:, qs_off(qt) - 4:qs_off(qt)] = qh.view(np.uint8).reshape(n, 4)
    out[:, qs_off(qt):] = ((levels[:, :16] & 15) | ((levels[:, 16:] & 15) << 4)).astype(np.uint8)
    return out


def rand_blocks(qt, n, K, rng):
    s = (rng.uniform(0.5, 1.5, n) / np.sqrt(K)).astype(np.float32)
    std = 70.0 if qt == L.IQ4_NL else (9.2 if qt in FIVE else 4.6)
    d = s / std
    lev = rng.integers(0, 32 if qt in FIVE else 16, (n, 32))
    return make_blocks(qt, d, -d * (15.5 if qt in FIVE else 7.5), lev)


def rand_weight(qt, K, N, rng):
    return rand_blocks(qt, N * (K // 32), K, rng).reshape(N, (K // 32) * L.TYPE_SIZE[qt])


def np_dequant(qt, blocks):
    """dequantize_row_*: [n, block bytes] -> f32 [n, 32], one f32 rounding per operation."""
    b = np.asarray(blocks, dtype=np.uint8)
    n = b.shape[0]
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32).reshape(n, 1)
    qs = b[:, qs_off(qt):].astype(np.int32)
    lev = np.concatenate([qs & 15, qs >> 4], axis=1)
    if qt in FIVE:
        qh = b[:, qs_off(qt) - 4:qs_off(qt)].copy().view(np.uint32).reshape(n, 1)
        lev = lev | (((qh >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int32) << 4)
    if qt == L.IQ4_NL:
        return d * IQ4NL[lev].astype(np.float32)
    if qt in ONE:
        m = b[:, 2:4].copy().view(np.float16).astype(np.float32).reshape(n, 1)
        return (lev.astype(np.float32) * d).astype(np.float32) + m
    return (lev - (16 if qt in FIVE else 8)).astype(np.float32) * d


def oracle_dequant(qt, blocks):
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    out = np.empty(b.shape[0] * 32, dtype=np.float32)
    T.oracle().oracle_dequantize_row(qt, b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size)
    return out.reshape(b.shape[0], 32)


def quantize_act(x, q81):
    """quantize_row_q8_0_ref / _q8_1_ref per 32 values: (q int32 [nb, 32], d f32 through f16 [nb], s f32 through f16 [nb] or None).
    s = f16(sum(q) * d) with the UNROUNDED d = amax / 127."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 32)
    amax = np.max(np.abs(x), axis=1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
        v = (x * idv[:, None]).astype(np.float32)
    q = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int32)  # roundf: halves away from zero
    dh = d.astype(np.float16).astype(np.float32)
    s = (q.sum(axis=1).astype(np.float32) * d).astype(np.float32).astype(np.float16).astype(np.float32) if q81 else None
    return q, dh, s


def mul_mat(g, qt, W, X, K, N, M):
    w = g.new(qt, [K, N], W, name="w")
    x = g.new(L.F32, [K, M], X, name="x")
    return g.H.ggml_mul_mat(g.ctx, w, x)


def mul_mat_offset_view(g, qt, W, X, K, N, M):
    """The same product with the weight as a 2-D view ONE BLOCK into a 1-D parent (a junk block, then the rows): the row base is as little aligned as the format allows."""
    bs = L.TYPE_SIZE[qt]
    raw = np.concatenate([np.full(bs, 0xA5, dtype=np.uint8), np.ascontiguousarray(W).reshape(-1)])
    parent = g.new(qt, [32 * (N * (K // 32) + 1)], raw, name="parent")
    w = g.H.ggml_view_2d(g.ctx, parent, K, N, (K // 32) * bs, bs)
    x = g.new(L.F32, [K, M], X, name="x")
    return g.H.ggml_mul_mat(g.ctx, w, x)
