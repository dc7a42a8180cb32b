"""Reference for the tests of the gpt-oss expert block: a NumPy twin of MXFP4 weights, ADD_ID and SWIGLU_OAI written from the formats.

The oracle (oracle/ggml_cpu_ref.c) knows none of the three, so this module is the reference: sampled and edge blocks, dequantize_row, the integer vec_dot against
Q8_0 activation blocks (which DO come from the oracle: oracle_quantize_row_q8_0), MUL_MAT, MUL_MAT_ID, ADD_ID, SWIGLU_OAI (expf from libm.so.6 through ctypes, as
act_norm_ref does) and the gpt-oss expert block composed from them.

    block_mxfp4 (17 B):  u8 e | u8 qs[16]
    value j (j < 16) = table[qs[j] & 15], value j + 16 = table[qs[j] >> 4]         table = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12} (E2M1 doubled)
    scale = half of 2^(e - 127); as f32 bits: e < 2 ? 0x00200000 << e : (e - 1) << 23                   y = (float) table value * scale (one exact product)
    vec_dot against Q8_0 blocks (generic C): per block sumf += (dy * scale) * (float) sumi, sumi the int32 dot of the 32 table values with the activation's int8s

Nothing on the build machine pins this layout against ggml itself; tests/test_mxfp4_ref_host.py pins this twin with known-answer blocks.
"""
import ctypes as C
import functools

import numpy as np

import harness as T
import llama_box_amd as L

QT = L.MXFP4
BS = 17
f32 = np.float32
KVALUES = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], dtype=np.int32)
Q80 = np.dtype([("d", "<f2"), ("qs", "i1", 32)])
assert Q80.itemsize == 34


# ------------------------------------------------------------------------------------------ packing
def make_blocks(e, nibble):
    """e [n] in 0..255; nibble [n, 32] in 0..15 (table indices, value order) -> uint8 [n, 17]"""
    nibble = np.asarray(nibble, dtype=np.uint8)
    n = nibble.shape[0]
    out = np.zeros((n, BS), dtype=np.uint8)
    out[:, 0] = np.asarray(e, dtype=np.uint8).reshape(n)
    out[:, 1:] = nibble[:, :16] | (nibble[:, 16:] << 4)
    return out


def rand_blocks(n_blocks, K, rng):
    """Directly sampled blocks over every code, the exponent around the value that gives a row of K values a trained network's scale (rms of the table 5.85)."""
    e0 = 128 + int(np.round(np.log2(1.0 / (5.85 * np.sqrt(K)))))
    return make_blocks(rng.integers(e0 - 2, e0 + 2, n_blocks), rng.integers(0, 16, (n_blocks, 32)))


def rand_weight(K, N, rng):
    nb = K // 32
    return rand_blocks(N * nb, K, rng).reshape(N, nb * BS)


EDGE_E = (0, 1, 2, 3, 126, 127, 128, 129, 250)


def edge_blocks(n_blocks, rng):
    """Blocks drawn from a catalogue of extremes: e in EDGE_E (both subnormal scales, the smallest normal ones, around 1, a huge one — at or below 250: code 7 at
    e = 254 overflows f32 in the reference too) x codes all 0, all 7 (12), all 15 (-12), all 8 (the second zero), a ramp and its mirror."""
    ramp = np.arange(32)
    codes = np.stack([np.zeros(32), np.full(32, 7), np.full(32, 15), np.full(32, 8), ramp % 16, 15 - ramp % 16]).astype(np.uint8)
    cat = np.concatenate([make_blocks(np.full(len(codes), e), codes) for e in EDGE_E])
    return cat[rng.integers(0, len(cat), n_blocks)]


# ------------------------------------------------------------------------------------------ decoding
def scale_f32(e):
    e = np.asarray(e, dtype=np.uint32)
    bits = np.where(e < 2, np.uint32(0x00200000) << e, (np.maximum(e, 1) - 1).astype(np.uint32) << np.uint32(23)).astype(np.uint32)
    return bits.view(np.float32)


def unpack(raw, K):
    """raw [..., row bytes] -> dict of per-block arrays [R, nb, ...]: `nibble` [.., 32] (value order), `value` [.., 32] (table entries), float32 `scale` [..]"""
    nb = K // 32
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, nb, BS)
    qs = b[..., 1:].astype(np.int32)
    nibble = np.concatenate([qs & 15, qs >> 4], axis=-1)
    return dict(nibble=nibble, value=KVALUES[nibble], scale=scale_f32(b[..., 0]), e=b[..., 0].astype(np.int32))


def dequantize(raw, K):
    """dequantize_row_mxfp4: float32 [..., K]"""
    u = unpack(raw, K)
    y = (u["value"].astype(f32) * u["scale"][..., None]).astype(f32)
    return y.reshape(np.asarray(raw).shape[:-1] + (K,))


def quantize_q80(X):
    """X float32 [M, K] -> block_q8_0 records [M, K / 32] from the oracle's quantize_row_q8_0"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    M, K = X.shape
    out = np.zeros((M, K // 32), dtype=Q80)
    lib = T.oracle()
    for m in range(M):
        lib.oracle_quantize_row_q8_0(X[m].ctypes.data_as(C.c_void_p), out[m].ctypes.data_as(C.c_void_p), K)
    return out


def block_sums(u, y):
    """the int32 block sums of table value x q8: [M, R, nb] (float64 holds them exactly: |sum| <= 32 * 12 * 127)"""
    return np.einsum("mbi,rbi->mrb", y["qs"].astype(np.float64), u["value"].astype(np.float64))


def _dot(u, y):
    """u: unpack() of R rows; y: Q80 [M, nb] -> float32 [M, R] in the arithmetic of ggml_vec_dot_mxfp4_q8_0 (generic C): per block
    sumf += (dy * scale) * (float) sumi, in block order."""
    R, nb = u["value"].shape[:2]
    M = y.shape[0]
    sumi = block_sums(u, y).astype(f32)  # exact: below 2^24
    yd = y["d"].astype(f32)
    sumf = np.zeros((M, R), dtype=f32)
    with np.errstate(all="ignore"):
        for b in range(nb):
            d = (yd[:, b, None] * u["scale"][None, :, b]).astype(f32)
            sumf = (sumf + (d * sumi[:, :, b]).astype(f32)).astype(f32)
    return sumf


def dequantize_q80(y):
    return (y["d"].astype(f32)[..., None] * y["qs"].astype(f32)).astype(np.float64).reshape(y.shape[0], -1)


def mul_mat(W, X):
    """W [N, row bytes], X float32 [M, K] -> float32 [M, N]: every column quantised to Q8_0 on its own, one vec_dot per (row, column)"""
    X = np.asarray(X, dtype=np.float32)
    return _dot(unpack(W, X.shape[1]), quantize_q80(X))


def mul_mat_id(W, b, ids):
    """W [n_expert, N, row bytes], b [n_tok, rows, K], ids [n_tok, n_used] -> float32 [n_tok, n_used, N]; an id outside the experts gives a row of zeros"""
    n_tok, n_used = ids.shape
    out = np.zeros((n_tok, n_used, W.shape[1]), dtype=np.float32)
    for t in range(n_tok):
        for s in range(n_used):
            e = int(ids[t, s])
            if 0 <= e < W.shape[0]:
                out[t, s] = mul_mat(W[e], b[t, s if b.shape[1] > 1 else 0][None])[0]
    return out


def add_id(a, b, ids):
    """a [n_tok, n_used, n], b [n_expert, n], ids [n_tok, n_used] -> a + b[ids] in f32; an id outside the experts adds nothing"""
    a = np.asarray(a, dtype=f32)
    out = a.copy()
    ok = (ids >= 0) & (ids < b.shape[0])
    out[ok] = (a[ok] + np.asarray(b, dtype=f32)[ids[ok]]).astype(f32)
    return out


@functools.lru_cache(maxsize=None)
def _libm():
    m = C.CDLL("libm.so.6")
    m.expf.restype = C.c_float
    m.expf.argtypes = [C.c_float]
    return m


def expf(x):
    fn = _libm().expf
    x = np.asarray(x, dtype=f32)
    return np.array([fn(float(v)) for v in x.ravel()], dtype=f32).reshape(x.shape)


def swiglu_oai(g, u, alpha, limit):
    """ggml-cpu's scalar loop, every operation one f32 operation: x = min(g, limit), y = clamp(u, -limit, limit), out = (x / (1 + expf(alpha * -x))) * (y + 1).
    min and clamp are comparisons that hand a NaN operand through (std::min / std::clamp)."""
    g, u = np.asarray(g, dtype=f32), np.asarray(u, dtype=f32)
    alpha, limit = f32(alpha), f32(limit)
    with np.errstate(all="ignore"):
        x = np.where(limit < g, limit, g).astype(f32)
        y = np.where(u < -limit, -limit, np.where(limit < u, limit, u)).astype(f32)
        e = expf((alpha * (-x)).astype(f32))
        glu = (x / (f32(1.0) + e).astype(f32)).astype(f32)
        return (glu * (y + f32(1.0)).astype(f32)).astype(f32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


# ------------------------------------------------------------------------------------------ graphs
def g_mul_mat(g, W, X, K, N, M):
    return g.H.ggml_mul_mat(g.ctx, g.new(QT, [K, N], W, name="w"), g.new(L.F32, [K, M], X, name="x"))


def g_mul_mat_offset_view(g, W, X, K, N, M):
    """The same product with the weight as a 2-D view ONE BLOCK (17 bytes) into a 1-D parent: every row starts at an odd address."""
    raw = np.concatenate([np.full(BS, 0xA5, dtype=np.uint8), np.ascontiguousarray(W).reshape(-1)])
    parent = g.new(QT, [32 * (N * (K // 32) + 1)], raw, name="parent")
    w = g.H.ggml_view_2d(g.ctx, parent, K, N, (K // 32) * BS, BS)
    return g.H.ggml_mul_mat(g.ctx, w, g.new(L.F32, [K, M], X, name="x"))


def g_get_rows(g, W, idx, K, N):
    return g.H.ggml_get_rows(g.ctx, g.new(QT, [K, N], W, name="w"), g.new(L.I32, [len(idx)], np.asarray(idx, dtype=np.int32), name="idx"))


# ------------------------------------------------------------------------------------------ the gpt-oss expert block
ALPHA, LIMIT = 1.702, 7.0


class GptOssBlock:
    """One expert block in llama.cpp's order for gpt-oss (build_moe_ffn with biases, SOFTMAX_WEIGHT gating, SWIGLU_OAI): router MUL_MAT + ADD(bias); ARGSORT / top-k
    view; GET_ROWS of the LOGITS at the chosen experts, SOFT_MAX over the chosen; MUL_MAT_ID + ADD_ID for up and gate; SWIGLU_OAI(1.702, 7.0); MUL_MAT_ID + ADD_ID
    for down; MUL by the weights; slot views + ADD.  The router reads the logits off the first n_expert values of x (unit rows, as moe_ref.MoeBlock)."""

    def __init__(self, n_embd, n_ff, n_expert, n_used, seed):
        rng = np.random.default_rng(seed)
        self.n_embd, self.n_ff, self.n_expert, self.n_used = n_embd, n_ff, n_expert, n_used
        self.gate_inp = np.zeros((n_expert, n_embd), dtype=f32)
        self.gate_inp[np.arange(n_expert), np.arange(n_expert)] = 1.0
        self.gate_inp_b = (rng.integers(-2, 3, n_expert) * 2.0 ** -6).astype(f32)  # (small exact steps: the order of the logits stays the inputs')
        self.w_up = np.stack([rand_weight(n_embd, n_ff, rng) for _ in range(n_expert)])
        self.w_gate = np.stack([rand_weight(n_embd, n_ff, rng) for _ in range(n_expert)])
        self.w_down = np.stack([rand_weight(n_ff, n_embd, rng) for _ in range(n_expert)])
        self.b_up = rng.standard_normal((n_expert, n_ff)).astype(f32) * f32(0.5)
        self.b_gate = rng.standard_normal((n_expert, n_ff)).astype(f32) * f32(0.5)
        self.b_down = rng.standard_normal((n_expert, n_embd)).astype(f32) * f32(0.5)

    def router_inputs(self, n_tok, rng, step=0.25):
        """x [n_tok, n_embd]: logits (the first n_expert values) a fixed step apart in a random order per token, the rest N(0, 1)."""
        x = rng.standard_normal((n_tok, self.n_embd)).astype(f32)
        for t in range(n_tok):
            x[t, :self.n_expert] = (rng.permutation(self.n_expert) * step).astype(f32)
        return x

    def build(self, g, x):
        """The block on target g; returns (out [n_embd, n_tokens], selected ids as a contiguous copy)."""
        H, ctx = g.H, g.ctx
        n_tok, ne, nu, E, F = x.shape[0], self.n_expert, self.n_used, self.n_embd, self.n_ff
        cur = g.new(L.F32, [E, n_tok], x, "x")
        gi = g.new(L.F32, [E, ne], self.gate_inp, "ffn_gate_inp")
        gib = g.new(L.F32, [ne], self.gate_inp_b, "ffn_gate_inp_b")
        up = g.new(QT, [E, F, ne], self.w_up, "ffn_up_exps")
        gate = g.new(QT, [E, F, ne], self.w_gate, "ffn_gate_exps")
        down = g.new(QT, [F, E, ne], self.w_down, "ffn_down_exps")
        up_b = g.new(L.F32, [F, ne], self.b_up, "ffn_up_exps_b")
        gate_b = g.new(L.F32, [F, ne], self.b_gate, "ffn_gate_exps_b")
        down_b = g.new(L.F32, [E, ne], self.b_down, "ffn_down_exps_b")
        logits = H.ggml_add(ctx, H.ggml_mul_mat(ctx, gi, cur), gib)
        sel = H.ggml_top_k(ctx, logits, nu)
        w = H.ggml_get_rows(ctx, H.ggml_reshape_3d(ctx, logits, 1, ne, n_tok), sel)  # [1, n_used, n_tokens]
        w = H.ggml_soft_max(ctx, H.ggml_reshape_2d(ctx, w, nu, n_tok))
        w = H.ggml_reshape_3d(ctx, w, 1, nu, n_tok)
        cur3 = H.ggml_reshape_3d(ctx, cur, E, 1, n_tok)
        u = H.ggml_add_id(ctx, H.ggml_mul_mat_id(ctx, up, cur3, sel), up_b, sel)
        gt = H.ggml_add_id(ctx, H.ggml_mul_mat_id(ctx, gate, cur3, sel), gate_b, sel)
        act = H.ggml_swiglu_oai(ctx, gt, u, ALPHA, LIMIT)
        ex = H.ggml_add_id(ctx, H.ggml_mul_mat_id(ctx, down, act, sel), down_b, sel)
        ex = H.ggml_mul(ctx, ex, w)
        exc = ex.contents
        out = None
        for s in range(nu):
            v = H.ggml_view_2d(ctx, ex, E, n_tok, exc.nb[2], s * exc.nb[1])
            out = v if out is None else H.ggml_add(ctx, out, v)
        if nu == 1:
            out = H.ggml_cont(ctx, out)
        return out, H.ggml_cont(ctx, sel)

    def logits(self, x):
        return (x[:, :self.n_expert] + self.gate_inp_b[None, :]).astype(f32)  # (unit rows: every other term of the router product is an exact zero)

    def reference(self, x):
        """(out [n_tokens, n_embd], ids [n_tokens, n_used]) composed from this module's twins; the SOFT_MAX over the chosen logits comes from the oracle."""
        n_tok, nu = x.shape[0], self.n_used
        H = L.host()
        lg = self.logits(x)
        ids = np.argsort(-lg, axis=1, kind="stable")[:, :nu].astype(np.int32)
        chosen = np.take_along_axis(lg, ids, axis=1).astype(f32)
        w = T.run_case(lambda g: H.ggml_soft_max(g.ctx, g.new(L.F32, [nu, n_tok], chosen)), "oracle")[0].reshape(n_tok, nu)
        xb = x.reshape(n_tok, 1, self.n_embd)
        u = add_id(mul_mat_id(self.w_up, xb, ids), self.b_up, ids)
        gt = add_id(mul_mat_id(self.w_gate, xb, ids), self.b_gate, ids)
        act = swiglu_oai(gt, u, ALPHA, LIMIT)
        ex = add_id(mul_mat_id(self.w_down, act, ids), self.b_down, ids)
        ex = (ex * w[:, :, None]).astype(f32)
        out = ex[:, 0]
        for s in range(1, nu):
            out = (out + ex[:, s]).astype(f32)
        return out, ids

    def numpy_f64(self, x, ids):
        """The block in float64 on de-quantised weights and unquantised activations with the given routing (the floor of the reference itself)."""
        n_tok, nu = x.shape[0], self.n_used
        lg = np.take_along_axis(self.logits(x).astype(np.float64), ids.astype(np.int64), axis=1)
        w = np.exp(lg - lg.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        deq = lambda W, K: dequantize(W, K).astype(np.float64)  # noqa: E731
        wu, wg, wd = deq(self.w_up, self.n_embd), deq(self.w_gate, self.n_embd), deq(self.w_down, self.n_ff)
        out = np.zeros((n_tok, self.n_embd))
        for t in range(n_tok):
            for s in range(nu):
                e = int(ids[t, s])
                u = wu[e] @ x[t].astype(np.float64) + self.b_up[e]
                g = wg[e] @ x[t].astype(np.float64) + self.b_gate[e]
                xx, yy = np.minimum(g, LIMIT), np.clip(u, -LIMIT, LIMIT)
                act = xx / (1.0 + np.exp(ALPHA * -xx)) * (yy + 1.0)
                out[t] += w[t, s] * (wd[e] @ act + self.b_down[e])
        return out
