"""Helpers for the bf16-weight tests: the f32 -> bf16 rounding ggml-cpu applies (ggml_compute_fp32_to_bf16: nearest even, subnormals kept, NaN kept quiet) in NumPy,
random and constructed bf16 matrices, graph builders, and the model generator's draw for a bf16 tensor (host/llama_lite.cpp: synth_rows) restated value by value.
The REFERENCE of every product is the oracle (harness.run_case(..., "oracle")); nothing here computes one."""
import ctypes as C

import numpy as np

import llama_box_amd as L


def to_bf16(x):
    """float32 array -> uint16 array of bf16 bit patterns"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + (0x7FFF + ((u >> 16) & 1))) >> 16
    return np.where(nan, (u >> 16) | 64, rne).astype(np.uint16)


def from_bf16(h):
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rand_weight(K, N, rng):
    """bf16 bit patterns [N, K] of a matrix with rows of unit-order norm"""
    return to_bf16((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))


def g_mul_mat(g, W, X, K, N, M):
    """MUL_MAT node over a plain bf16 weight (W: uint16 [N, K]) and f32 activations (X: [M, K])"""
    return g.H.ggml_mul_mat(g.ctx, g.new(L.BF16, [K, N], W, name="w"), g.new(L.F32, [K, M], X, name="x"))


def g_mul_mat_offset_view(g, W, X, K, N, M):
    """The same product with the weight as a 2-D view ONE ELEMENT into a 1-D parent (a junk element, then the rows): rows 2-byte aligned and no more."""
    raw = np.concatenate([np.array([0x7FC0], dtype=np.uint16), np.ascontiguousarray(W).reshape(-1)])
    parent = g.new(L.BF16, [N * K + 1], raw, name="parent")
    w = g.H.ggml_view_2d(g.ctx, parent, K, N, K * 2, 2)
    return g.H.ggml_mul_mat(g.ctx, w, g.new(L.F32, [K, M], X, name="x"))


def host_rows(t):
    """uint16 [ne1, ne0] of a 2-D bf16 tensor in host memory"""
    assert t.type == L.BF16 and t.nb[0] == 2 and t.ne[2] == 1 and t.ne[3] == 1
    rows = [np.frombuffer((C.c_uint8 * (t.ne[0] * 2)).from_address(t.data + r * t.nb[1]), dtype=np.uint16).copy() for r in range(t.ne[1])]
    return np.stack(rows)


# ---------------------------------------------------------------------------------------------- the generator's draw
_M64 = (1 << 64) - 1


def _splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & _M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def synth_draw(seed, tensor_id, n_rows, K, gain):
    """float32 [n_rows, K]: what the F16 recipe of synth_rows draws for an unsharded [K, n_rows] matrix — lo + (hi - lo) u01 at the element's key — over the range a
    bf16 matrix gets (hi = gain sqrt(3 / K), lo = -hi), in the generator's float32 arithmetic"""
    hi = np.float32(gain) * np.sqrt(np.float32(3.0) / np.float32(K), dtype=np.float32)
    lo = np.float32(-hi)
    out = np.empty((n_rows, K), dtype=np.float32)
    base = seed ^ ((tensor_id * 0xD1B54A32D192ED03) & _M64)
    for r in range(n_rows):
        for i in range(K):
            u = np.float32((_splitmix64(base ^ (((r * K + i) * 0x9E3779B97F4A7C15) & _M64)) >> 40) * (1.0 / 16777216.0))
            out[r, i] = lo + np.float32(hi - lo) * u
    return out


# ---------------------------------------------------------------------------------------------- shared by the host and the GPU model tests
# activations whose rounding to bf16 tells the implementations apart: RNE ties with an even and an odd upper half, one ulp either side of a tie, -0.0, f32
# subnormals (kept, not flushed), values past f16's range (70000, 1e30: a conversion through f16 gives inf), below it (1e-30: f16 would flush) and the largest
# value that stays finite (0x7F7F0000; the next tie up rounds to inf)
READBACK_VALUES = np.concatenate([
    np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7F0000, 0xFF7F0000],
             dtype=np.uint32).view(np.float32),
    np.array([70000.0, -70000.0, 1e30, -1e30, 1e-30, -1e-30, 65504.0, 65520.0, 1.0, -2.5, 3.14159274, 0.0], dtype=np.float32)])
MODEL_SEED = 1234
PROMPT40 = [(7 * i + 3) % 512 for i in range(40)]
N_GEN = 17  # the prompt's last position + 16 batch-1 steps


def oracle_margins_and_yardstick(H, name, seed=MODEL_SEED):
    """top-2 margins of the oracle's greedy rows on `name` (soft-max path) and twice its own order sensitivity (tests/test_gpu_model.py)"""
    import harness as T
    from model_util import Context, Model, greedy, preset
    from test_gpu_model import _oracle_yardstick

    m = Model(preset(name), seed, H.ggml_backend_cpu_buffer_type())
    try:
        c = Context(m, compute=T.oracle_compute_fn(), flash_attn=0)
        _, rows = greedy(c, PROMPT40, N_GEN)
        c.free()
    finally:
        m.free()
    top2 = np.sort(np.stack(rows), axis=1)[:, -2:]
    return top2[:, 1] - top2[:, 0], 2.0 * _oracle_yardstick(H, name, PROMPT40, N_GEN)
