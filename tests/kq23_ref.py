"""Reference for the tests of Q2_K / Q3_K weights: a NumPy twin written from the layouts in include/ggml_abi.h.

The oracle (oracle/ggml_cpu_ref.c) does not know the two formats, so this module is the reference: sampled and edge blocks, dequantize_row, the integer
vec_dot against Q8_K activation blocks (which DO come from the oracle: oracle_quantize_row_q8_K), MUL_MAT, and a hybrid compute function for
model_util.Context that hands every node to the oracle except the MUL_MAT / GET_ROWS nodes whose src0 is Q2_K / Q3_K.

    block_q2_K (84 B):  scales[16] (scale | min << 4) | qs[64] | f16 d | f16 dmin        y = (d * sc) * level - dmin * m
    block_q3_K (110 B): hmask[32] | qs[64] | scales[12] | f16 d                          y = (d * (sc - 32)) * level
    value 128 n + 32 j + l (n < 2, j < 4, l < 32): low bits (qs[32 n + l] >> 2 j) & 3, sub-block 8 n + 2 j + l // 16; Q3_K subtracts 4 where bit
    4 n + j of hmask[l] is CLEAR.

Nothing on the build machine pins these layouts against ggml itself; tests/test_kq23_ref_host.py pins this twin with known-answer blocks.
"""
import ctypes as C

import numpy as np

import harness as T
import llama_box_amd as L

FORMATS = (L.Q2_K, L.Q3_K)
Q8K = np.dtype([("d", "<f4"), ("qs", "i1", 256), ("bsums", "<i2", 16)])
assert Q8K.itemsize == 292

_I = np.arange(256)
_N, _J, _LL = _I // 128, (_I // 32) % 4, _I % 32
SUB = 8 * _N + 2 * _J + _LL // 16   # sub-block of value i
QS_BYTE = 32 * _N + _LL             # byte of qs that holds value i, at bit 2 j


# ------------------------------------------------------------------------------------------ packing
def make_q2k(scale, mn, level, d, dmin):
    """scale, mn [n, 16] in 0..15; level [n, 256] in 0..3; d, dmin [n] (f16-representable) -> uint8 [n, 84]"""
    scale, mn, level = (np.asarray(a, dtype=np.uint8) for a in (scale, mn, level))
    n = level.shape[0]
    out = np.zeros((n, 84), dtype=np.uint8)
    out[:, 0:16] = scale | (mn << 4)
    for j in range(4):
        for h in range(2):
            out[:, 16 + 32 * h:48 + 32 * h] |= level[:, 128 * h + 32 * j:128 * h + 32 * j + 32] << (2 * j)
    out[:, 80:82] = np.asarray(d, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    out[:, 82:84] = np.asarray(dmin, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    return out


def make_q3k(scale6, level, d):
    """scale6 [n, 16] in 0..63 (used as scale6 - 32); level [n, 256] in -4..3; d [n] -> uint8 [n, 110]"""
    scale6, level = np.asarray(scale6, dtype=np.uint8), np.asarray(level, dtype=np.int64)
    n = level.shape[0]
    out = np.zeros((n, 110), dtype=np.uint8)
    low2, hbit = (level & 3).astype(np.uint8), (level >= 0).astype(np.uint8)
    for j in range(4):
        for h in range(2):
            sl = slice(128 * h + 32 * j, 128 * h + 32 * j + 32)
            out[:, 32 + 32 * h:64 + 32 * h] |= low2[:, sl] << (2 * j)
            out[:, 0:32] |= hbit[:, sl] << (4 * h + j)
    out[:, 96:104] = (scale6[:, 0:8] & 15) | ((scale6[:, 8:16] & 15) << 4)
    for k in range(4):
        out[:, 104 + k] = (scale6[:, k] >> 4) | ((scale6[:, k + 4] >> 4) << 2) | ((scale6[:, k + 8] >> 4) << 4) | ((scale6[:, k + 12] >> 4) << 6)
    out[:, 108:110] = np.asarray(d, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    return out


def rand_blocks(qtype, n_blocks, K, rng):
    """Directly sampled blocks over the whole range of every field, with d sized so that a row of K values has a trained network's scale."""
    s = (rng.uniform(0.5, 1.5, n_blocks) / np.sqrt(K)).astype(np.float32)
    if qtype == L.Q2_K:
        d = s / 11.2
        return make_q2k(rng.integers(0, 16, (n_blocks, 16)), rng.integers(0, 16, (n_blocks, 16)), rng.integers(0, 4, (n_blocks, 256)), d, 1.5 * d)
    if qtype == L.Q3_K:
        return make_q3k(rng.integers(0, 64, (n_blocks, 16)), rng.integers(-4, 4, (n_blocks, 256)), s / 48.5)
    raise ValueError(qtype)


def rand_weight(qtype, K, N, rng):
    nb = K // 256
    return rand_blocks(qtype, N * nb, K, rng).reshape(N, nb * L.TYPE_SIZE[qtype])


def edge_blocks(qtype, n_blocks, rng):
    """Blocks drawn from a catalogue of extremes: scales / mins all 0 and all at their maximum, levels all at either end (hmask all clear / all set), negative
    and zero d / dmin, an f16 subnormal d, and (Q3_K) -4 x -32 in every position."""
    ramp = np.arange(256)
    d = np.array([1.0, -0.5, 6e-8, 0.0, 0.25, 2e-3, -1.5, 1.0], dtype=np.float16)
    if qtype == L.Q2_K:
        dmin = np.array([0.5, 2.0, -0.25, 1.0, 0.0, -3.0, 0.125, 1.0], dtype=np.float16)
        nib = np.stack([np.zeros(16), np.full(16, 15), np.arange(16), np.arange(16)[::-1], np.full(16, 15), np.zeros(16), np.full(16, 7), np.full(16, 15)])
        mins = np.stack([np.zeros(16), np.full(16, 15), np.arange(16)[::-1], np.full(16, 15), np.zeros(16), np.arange(16), np.full(16, 15), np.zeros(16)])
        lev = np.stack([np.zeros(256), np.full(256, 3), ramp % 4, ramp[::-1] % 4, np.full(256, 3), np.zeros(256), (ramp // 16) % 4, np.full(256, 3)])
        cat = make_q2k(nib, mins, lev, d, dmin)
    elif qtype == L.Q3_K:
        sc = np.stack([np.zeros(16), np.full(16, 63), np.arange(16) * 4, 63 - np.arange(16) * 4, np.zeros(16), np.full(16, 63), np.full(16, 32), np.full(16, 31)])
        lev = np.stack([np.full(256, -4), np.full(256, 3), ramp % 8 - 4, ramp[::-1] % 8 - 4, np.full(256, 3), np.full(256, -4), np.full(256, -1), np.zeros(256)])
        cat = make_q3k(sc, lev, d)  # (block 0: hmask all clear, levels 0 -> -4 x -32 everywhere; 1: hmask all set, low bits all 3; 5: -4 x 31)
    else:
        raise ValueError(qtype)
    return cat[rng.integers(0, len(cat), n_blocks)]


# ------------------------------------------------------------------------------------------ decoding
def _f16(b):
    return np.ascontiguousarray(b).view(np.float16).astype(np.float32).reshape(b.shape[:-1])


def unpack(qtype, raw, K):
    """raw [..., row bytes] -> dict of per-block arrays [R, nb, ...] (R = product of the leading dims): integer `level` [.., 256], `scale` [.., 16]
    (Q3_K: already minus 32), `min` [.., 16] (Q2_K), float32 `d`, `dmin`."""
    bs, nb = L.TYPE_SIZE[qtype], K // 256
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, nb, bs)
    if qtype == L.Q2_K:
        sm = b[..., 0:16].astype(np.int32)
        qs = b[..., 16:80].astype(np.int32)
        level = (qs[..., QS_BYTE] >> (2 * _J)) & 3
        return dict(level=level, scale=sm & 15, min=sm >> 4, d=_f16(b[..., 80:82]), dmin=_f16(b[..., 82:84]))
    hm, qs, sc = b[..., 0:32].astype(np.int32), b[..., 32:96].astype(np.int32), b[..., 96:108].astype(np.int32)
    level = ((qs[..., QS_BYTE] >> (2 * _J)) & 3) - 4 * (1 - ((hm[..., _LL] >> (4 * _N + _J)) & 1))
    s = np.arange(16)
    low4 = np.where(s < 8, sc[..., s % 8] & 15, sc[..., s % 8] >> 4)
    scale = (low4 | (((sc[..., 8 + s % 4] >> (2 * (s // 4))) & 3) << 4)) - 32
    return dict(level=level, scale=scale, d=_f16(b[..., 108:110]))


def dequantize(qtype, raw, K):
    """dequantize_row_q2_K / _q3_K: float32 [..., K], every product and the difference rounded to float32 on its own."""
    u = unpack(qtype, raw, K)
    lev, sc = u["level"].astype(np.float32), u["scale"][..., SUB].astype(np.float32)
    dl = (u["d"][..., None] * sc).astype(np.float32)
    y = (dl * lev).astype(np.float32)
    if qtype == L.Q2_K:
        ml = (u["dmin"][..., None] * u["min"][..., SUB].astype(np.float32)).astype(np.float32)
        y = (y - ml).astype(np.float32)
    lead = np.asarray(raw).shape[:-1]
    return y.reshape(lead + (K,))


def quantize_q8k(X):
    """X float32 [M, K] -> block_q8_K records [M, K / 256] from the oracle's quantize_row_q8_K"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    M, K = X.shape
    out = np.zeros((M, K // 256), dtype=Q8K)
    lib = T.oracle()
    for m in range(M):
        lib.oracle_quantize_row_q8_K(X[m].ctypes.data_as(C.c_void_p), out[m].ctypes.data_as(C.c_void_p), K)
    return out


def _dot(qtype, u, y):
    """u: unpack() of R rows; y: Q8K [M, nb] -> float32 [M, R] in the arithmetic of ggml_vec_dot_q2_K_q8_K / _q3_K_q8_K (generic C)."""
    f32 = np.float32
    R, nb = u["level"].shape[:2]
    M = y.shape[0]
    wl = (u["level"] * u["scale"][..., SUB]).astype(np.float64)  # scale x level per position: |.| <= 128, sums over 256 x 127 exact in float64
    q8 = y["qs"].astype(np.float64)
    yd = y["d"].astype(f32)
    if qtype == L.Q2_K:
        sumf = np.zeros((M, R), dtype=f32)
        for b in range(nb):
            isum = (q8[:, b] @ wl[:, b].T).astype(f32)                                            # exact integers below 2^24
            summs = (y["bsums"][:, b].astype(np.float64) @ u["min"][:, b].T.astype(np.float64)).astype(f32)
            dall = (yd[:, b, None] * u["d"][None, :, b]).astype(f32)
            dmin = (yd[:, b, None] * u["dmin"][None, :, b]).astype(f32)
            sumf = (sumf + ((dall * isum).astype(f32) - (dmin * summs).astype(f32)).astype(f32)).astype(f32)
        return sumf
    lanes = np.zeros((M, R, 8), dtype=f32)  # eight float lanes: lane l sums the positions p with p % 8 == l
    for b in range(nb):
        aux = np.einsum("mki,rki->mri", q8[:, b].reshape(M, 32, 8), wl[:, b].reshape(R, 32, 8))   # int32 lanes, exact
        d = (u["d"][None, :, b] * yd[:, b, None]).astype(f32)
        lanes = (lanes + (d[..., None] * aux.astype(f32)).astype(f32)).astype(f32)
    sumf = np.zeros((M, R), dtype=f32)
    for l in range(8):
        sumf = (sumf + lanes[..., l]).astype(f32)
    return sumf


def vec_dot(qtype, raw, q8k_blocks):
    """One weight row (bytes) against one activation row (Q8K records [nb]) -> float32 scalar"""
    K = 256 * len(q8k_blocks)
    return _dot(qtype, unpack(qtype, np.asarray(raw).reshape(1, -1), K), np.asarray(q8k_blocks).reshape(1, -1))[0, 0]


def dequantize_q8k(y):
    return (y["d"][..., None] * y["qs"].astype(np.float32)).astype(np.float64).reshape(y.shape[0], -1)


def mul_mat(qtype, W, X):
    """W [N, row bytes], X float32 [M, K] -> float32 [M, N]: every column quantised to Q8_K on its own, one vec_dot per (row, column)"""
    X = np.asarray(X, dtype=np.float32)
    return _dot(qtype, unpack(qtype, W, X.shape[1]), quantize_q8k(X))


def mmid(qtype, W, b, ids):
    """moe_ref.mmid_numpy's job through the twin: W [n_expert, N, row bytes], b [n_tok, rows, K], ids [n_tok, n_used] -> float32 [n_tok, n_used, N]"""
    n_tok, n_used = ids.shape
    out = np.zeros((n_tok, n_used, W.shape[1]), dtype=np.float32)
    for t in range(n_tok):
        for s in range(n_used):
            out[t, s] = mul_mat(qtype, W[int(ids[t, s])], b[t, s if b.shape[1] > 1 else 0][None])[0]
    return out


# ------------------------------------------------------------------------------------------ graphs
def g_mul_mat(g, qt, W, X, K, N, M):
    return g.H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], W, name="w"), g.new(L.F32, [K, M], X, name="x"))


def g_mul_mat_offset_view(g, qt, W, X, K, N, M):
    """The same product with the weight as a 2-D view ONE BLOCK (84 / 110 bytes) into a 1-D parent: the row base is as little aligned as the format allows."""
    bs = L.TYPE_SIZE[qt]
    raw = np.concatenate([np.full(bs, 0xA5, dtype=np.uint8), np.ascontiguousarray(W).reshape(-1)])
    parent = g.new(qt, [256 * (N * (K // 256) + 1)], raw, name="parent")
    w = g.H.ggml_view_2d(g.ctx, parent, K, N, (K // 256) * bs, bs)
    return g.H.ggml_mul_mat(g.ctx, w, g.new(L.F32, [K, M], X, name="x"))


# ------------------------------------------------------------------------------------------ whole-model CPU reference
def _host_bytes(ptr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr))


def _rows(t, K):
    """the rows of a 2-D block-format tensor in host memory: uint8 [ne1, row bytes]"""
    rb = (K // 256) * L.TYPE_SIZE[t.type]
    assert t.ne[2] == 1 and t.ne[3] == 1 and t.nb[0] == L.TYPE_SIZE[t.type]
    return np.stack([_host_bytes(t.data + r * t.nb[1], rb) for r in range(t.ne[1])])


def hybrid_compute_fn(n_threads=4):
    """llm_compute_fn: the oracle node by node, except MUL_MAT / GET_ROWS over a Q2_K / Q3_K src0, which the twin computes straight into node->data.
    (keep the returned object alive while the context lives)"""
    lib = T.oracle()
    H = L.host()
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:  # the two op numbers, read off nodes built through the API
        w = H.ggml_new_tensor_2d(ctx, L.F32, 4, 4)
        GGML_OP_MUL_MAT = H.ggml_mul_mat(ctx, w, H.ggml_new_tensor_2d(ctx, L.F32, 4, 1)).contents.op
        GGML_OP_GET_ROWS = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 1)).contents.op
    finally:
        H.ggml_free(ctx)
    cache = {}  # weights do not change between steps: unpacked once per tensor

    def fn(graph, nth):
        g = graph.contents
        for i in range(g.n_nodes):
            node = g.nodes[i].contents
            a = node.src[0].contents if node.src[0] else None
            if a is not None and a.type in FORMATS and node.op in (GGML_OP_MUL_MAT, GGML_OP_GET_ROWS):
                K = a.ne[0]
                key = (a.data, a.type, K, a.ne[1])
                b = node.src[1].contents
                assert node.type == L.F32 and node.nb[0] == 4 and node.nb[1] == 4 * node.ne[0] and node.ne[2] == 1 and node.ne[3] == 1
                if node.op == GGML_OP_MUL_MAT:
                    if key not in cache:
                        cache[key] = unpack(a.type, _rows(a, K), K)
                    M = b.ne[1]
                    assert b.type == L.F32 and b.nb[0] == 4 and b.ne[2] == 1 and b.ne[3] == 1 and node.ne[0] == a.ne[1] and node.ne[1] == M
                    X = np.stack([_host_bytes(b.data + m * b.nb[1], 4 * K).view(np.float32) for m in range(M)]) if M else np.zeros((0, K), np.float32)
                    if M:
                        out = _dot(a.type, cache[key], quantize_q8k(X))
                        _host_bytes(node.data, 4 * M * node.ne[0]).view(np.float32)[:] = out.reshape(-1)
                else:
                    n = b.ne[0]
                    assert b.type == L.I32 and b.ne[1] == 1 and b.ne[2] == 1 and node.ne[0] == K and node.ne[1] == n
                    if n:
                        idx = _host_bytes(b.data, 4 * n).view(np.int32)
                        rows = np.stack([_host_bytes(a.data + int(r) * a.nb[1], (K // 256) * L.TYPE_SIZE[a.type]) for r in idx])
                        _host_bytes(node.data, 4 * n * K).view(np.float32)[:] = dequantize(a.type, rows, K).reshape(-1)
                continue
            st = lib.oracle_compute_node(g.nodes[i], nth if nth > 0 else n_threads)
            if st != 0:
                return st
        return 0

    return L.COMPUTE_FN(fn)
