"""Reference for the tests of IQ4_XS weights: a NumPy twin written from the layout in include/ggml_abi.h.

The oracle (oracle/ggml_cpu_ref.c) does not know the format, so this module is the reference: sampled and edge blocks, dequantize_row, the integer vec_dot
against Q8_K activation blocks (which DO come from the oracle: oracle_quantize_row_q8_K), MUL_MAT, MUL_MAT_ID, and a hybrid compute function for
model_util.Context that hands every node to the oracle except the MUL_MAT / GET_ROWS / MUL_MAT_ID nodes whose src0 is IQ4_XS.

    block_iq4_xs (136 B):  f16 d | u16 scales_h | u8 scales_l[4] | u8 qs[128]
    sub-block ib (0 .. 7) = values 32 ib .. 32 ib + 31, six-bit scale ls = nibble ib of scales_l | bit pair ib of scales_h << 4, used as ls - 32
    value 32 ib + j (j < 16) = table[qs[16 ib + j] & 15], value 32 ib + 16 + j = table[qs[16 ib + j] >> 4]            y = (d * (ls - 32)) * table value

Nothing on the build machine pins this layout against ggml itself; tests/test_iq4xs_ref_host.py pins this twin with known-answer blocks.
"""
import ctypes as C

import numpy as np

import harness as T
import llama_box_amd as L

QT = L.IQ4_XS
BS = 136
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int32)
Q8K = np.dtype([("d", "<f4"), ("qs", "i1", 256), ("bsums", "<i2", 16)])
assert Q8K.itemsize == 292

_I = np.arange(256)
SUB = _I // 32                          # sub-block of value i
QS_BYTE = 16 * SUB + _I % 16            # byte of qs that holds value i ...
QS_HIGH = (_I % 32) >= 16               # ... in its high nibble?


# ------------------------------------------------------------------------------------------ packing
def make_iq4xs(scale6, nibble, d):
    """scale6 [n, 8] in 0..63 (used as scale6 - 32); nibble [n, 256] in 0..15 (table indices, value order); d [n] (f16-representable) -> uint8 [n, 136]"""
    scale6, nibble = np.asarray(scale6, dtype=np.uint32), np.asarray(nibble, dtype=np.uint8)
    n = nibble.shape[0]
    out = np.zeros((n, BS), dtype=np.uint8)
    out[:, 0:2] = np.asarray(d, dtype=np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    sh = np.zeros(n, dtype=np.uint32)
    for ib in range(8):
        sh |= (scale6[:, ib] >> 4) << (2 * ib)
        out[:, 4 + ib // 2] |= ((scale6[:, ib] & 15) << (4 * (ib % 2))).astype(np.uint8)
    out[:, 2] = sh & 0xFF
    out[:, 3] = sh >> 8
    v = nibble.reshape(n, 8, 2, 16)
    out[:, 8:] = (v[:, :, 0, :] | (v[:, :, 1, :] << 4)).reshape(n, 128)
    return out


def rand_blocks(n_blocks, K, rng):
    """Directly sampled blocks over the whole range of every field, with d sized so that a row of K values has a trained network's scale
    (rms(ls - 32) = 18.5, rms(table) = 67.4)."""
    s = (rng.uniform(0.5, 1.5, n_blocks) / np.sqrt(K)).astype(np.float32)
    return make_iq4xs(rng.integers(0, 64, (n_blocks, 8)), rng.integers(0, 16, (n_blocks, 256)), s / 1246.0)


def rand_weight(K, N, rng):
    nb = K // 256
    return rand_blocks(N * nb, K, rng).reshape(N, nb * BS)


def edge_blocks(n_blocks, rng):
    """Blocks drawn from a catalogue of extremes: scales all 0 (-32) and all 63 (31), codes all at either end of the table, the largest products of both
    signs in every position, scale 32 (a zero block), ramps, negative and zero d, an f16 subnormal d."""
    ramp = np.arange(256)
    d = np.array([1.0, -0.5, 6e-8, 0.0, 0.25, 2e-3, -1.5, 1.0], dtype=np.float16)
    sc = np.stack([np.zeros(8), np.full(8, 63), np.arange(8) * 9, 63 - np.arange(8) * 9, np.zeros(8), np.full(8, 63), np.full(8, 32), np.full(8, 31)])
    nib = np.stack([np.zeros(256), np.full(256, 15), ramp % 16, ramp[::-1] % 16, np.full(256, 15), np.zeros(256), (ramp // 16) % 16, np.full(256, 8)])
    cat = make_iq4xs(sc, nib, d)  # (block 0: -32 x -127 everywhere; 1: 31 x 113; 4: -32 x 113; 5: 31 x -127)
    return cat[rng.integers(0, len(cat), n_blocks)]


# ------------------------------------------------------------------------------------------ decoding
def _f16(b):
    return np.ascontiguousarray(b).view(np.float16).astype(np.float32).reshape(b.shape[:-1])


def unpack(raw, K):
    """raw [..., row bytes] -> dict of per-block arrays [R, nb, ...] (R = product of the leading dims): integer `nibble` [.., 256] (value order), `value`
    [.., 256] (table entries), `scale` [.., 8] (already minus 32), float32 `d`."""
    nb = K // 256
    b = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, nb, BS)
    sh = b[..., 2].astype(np.int32) | (b[..., 3].astype(np.int32) << 8)
    sl = b[..., 4:8].astype(np.int32)
    ib = np.arange(8)
    scale = (((sl[..., ib // 2] >> (4 * (ib % 2))) & 15) | (((sh[..., None] >> (2 * ib)) & 3) << 4)) - 32
    qs = b[..., 8:].astype(np.int32)
    nibble = np.where(QS_HIGH, qs[..., QS_BYTE] >> 4, qs[..., QS_BYTE] & 15)
    return dict(nibble=nibble, value=KVALUES[nibble], scale=scale, d=_f16(b[..., 0:2]))


def dequantize(raw, K):
    """dequantize_row_iq4_xs: float32 [..., K]; dl = d * (ls - 32) and dl * table value are each rounded to float32 on their own."""
    u = unpack(raw, K)
    dl = (u["d"][..., None] * u["scale"].astype(np.float32)).astype(np.float32)
    y = (dl[..., SUB] * u["value"].astype(np.float32)).astype(np.float32)
    return y.reshape(np.asarray(raw).shape[:-1] + (K,))


def quantize_q8k(X):
    """X float32 [M, K] -> block_q8_K records [M, K / 256] from the oracle's quantize_row_q8_K"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    M, K = X.shape
    out = np.zeros((M, K // 256), dtype=Q8K)
    lib = T.oracle()
    for m in range(M):
        lib.oracle_quantize_row_q8_K(X[m].ctypes.data_as(C.c_void_p), out[m].ctypes.data_as(C.c_void_p), K)
    return out


def sub_sums(u, y):
    """the int32 sub-block sums of table value x q8: [M, R, nb, 8] (float64 holds them exactly: |sum| <= 32 * 127 * 127)"""
    R, nb = u["value"].shape[:2]
    M = y.shape[0]
    return np.einsum("mbsi,rbsi->mrbs", y["qs"].astype(np.float64).reshape(M, nb, 8, 32), u["value"].astype(np.float64).reshape(R, nb, 8, 32))


def _dot(u, y):
    """u: unpack() of R rows; y: Q8K [M, nb] -> float32 [M, R] in the arithmetic of ggml_vec_dot_iq4_xs_q8_K (generic C): per super-block
    d4d8 = d * y.d, per sub-block sumf += (d4d8 * (float) (ls - 32)) * (float) sumi, one after the other."""
    f32 = np.float32
    R, nb = u["value"].shape[:2]
    M = y.shape[0]
    sumi = sub_sums(u, y).astype(f32)  # exact: below 2^24
    yd = y["d"].astype(f32)
    sumf = np.zeros((M, R), dtype=f32)
    for b in range(nb):
        d4d8 = (u["d"][None, :, b] * yd[:, b, None]).astype(f32)
        for ib in range(8):
            dl = (d4d8 * u["scale"][None, :, b, ib].astype(f32)).astype(f32)
            sumf = (sumf + (dl * sumi[:, :, b, ib]).astype(f32)).astype(f32)
    return sumf


def vec_dot(raw, q8k_blocks):
    """One weight row (bytes) against one activation row (Q8K records [nb]) -> float32 scalar"""
    K = 256 * len(q8k_blocks)
    return _dot(unpack(np.asarray(raw).reshape(1, -1), K), np.asarray(q8k_blocks).reshape(1, -1))[0, 0]


def dequantize_q8k(y):
    return (y["d"][..., None] * y["qs"].astype(np.float32)).astype(np.float64).reshape(y.shape[0], -1)


def mul_mat(W, X):
    """W [N, row bytes], X float32 [M, K] -> float32 [M, N]: every column quantised to Q8_K on its own, one vec_dot per (row, column)"""
    X = np.asarray(X, dtype=np.float32)
    return _dot(unpack(W, X.shape[1]), quantize_q8k(X))


def mmid(W, b, ids):
    """W [n_expert, N, row bytes], b [n_tok, rows, K], ids [n_tok, n_used] -> float32 [n_tok, n_used, N]; an id outside the experts gives a row of zeros"""
    n_tok, n_used = ids.shape
    out = np.zeros((n_tok, n_used, W.shape[1]), dtype=np.float32)
    for t in range(n_tok):
        for s in range(n_used):
            e = int(ids[t, s])
            if 0 <= e < W.shape[0]:
                out[t, s] = mul_mat(W[e], b[t, s if b.shape[1] > 1 else 0][None])[0]
    return out


# ------------------------------------------------------------------------------------------ graphs
def g_mul_mat(g, W, X, K, N, M):
    return g.H.ggml_mul_mat(g.ctx, g.new(QT, [K, N], W, name="w"), g.new(L.F32, [K, M], X, name="x"))


def g_mul_mat_offset_view(g, W, X, K, N, M):
    """The same product with the weight as a 2-D view ONE BLOCK (136 bytes) into a 1-D parent: the row base is as little aligned as a whole-block view gets."""
    raw = np.concatenate([np.full(BS, 0xA5, dtype=np.uint8), np.ascontiguousarray(W).reshape(-1)])
    parent = g.new(QT, [256 * (N * (K // 256) + 1)], raw, name="parent")
    w = g.H.ggml_view_2d(g.ctx, parent, K, N, (K // 256) * BS, BS)
    return g.H.ggml_mul_mat(g.ctx, w, g.new(L.F32, [K, M], X, name="x"))


def g_get_rows(g, W, idx, K, N):
    return g.H.ggml_get_rows(g.ctx, g.new(QT, [K, N], W, name="w"), g.new(L.I32, [len(idx)], np.asarray(idx, dtype=np.int32), name="idx"))


# ------------------------------------------------------------------------------------------ whole-model CPU reference
def _host_bytes(ptr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr))


def _rows(t, K, e=0):
    """the rows of matrix e of a block-format tensor in host memory: uint8 [ne1, row bytes]"""
    rb = (K // 256) * BS
    assert t.ne[3] == 1 and t.nb[0] == BS
    return np.stack([_host_bytes(t.data + e * t.nb[2] + r * t.nb[1], rb) for r in range(t.ne[1])])


def hybrid_compute_fn(n_threads=4):
    """llm_compute_fn: the oracle node by node, except MUL_MAT / GET_ROWS / MUL_MAT_ID over an IQ4_XS src0, which the twin computes straight into node->data.
    (keep the returned object alive while the context lives)"""
    lib = T.oracle()
    H = L.host()
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:  # the op numbers, read off nodes built through the API
        w = H.ggml_new_tensor_2d(ctx, L.F32, 4, 4)
        GGML_OP_MUL_MAT = H.ggml_mul_mat(ctx, w, H.ggml_new_tensor_2d(ctx, L.F32, 4, 1)).contents.op
        GGML_OP_GET_ROWS = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 1)).contents.op
        w3 = H.ggml_new_tensor_3d(ctx, L.F32, 4, 4, 2)
        GGML_OP_MUL_MAT_ID = H.ggml_mul_mat_id(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 4, 1, 1), H.ggml_new_tensor_2d(ctx, L.I32, 1, 1)).contents.op
    finally:
        H.ggml_free(ctx)
    cache = {}  # weights do not change between steps: unpacked once per tensor

    def fn(graph, nth):
        g = graph.contents
        for i in range(g.n_nodes):
            node = g.nodes[i].contents
            a = node.src[0].contents if node.src[0] else None
            if a is not None and a.type == QT and node.op in (GGML_OP_MUL_MAT, GGML_OP_GET_ROWS, GGML_OP_MUL_MAT_ID):
                K = a.ne[0]
                b = node.src[1].contents
                assert node.type == L.F32 and node.nb[0] == 4 and node.nb[1] == 4 * node.ne[0] and node.ne[3] == 1
                if node.op == GGML_OP_MUL_MAT:
                    key = (a.data, K, a.ne[1])
                    if key not in cache:
                        cache[key] = unpack(_rows(a, K), K)
                    M = b.ne[1]
                    assert a.ne[2] == 1 and node.ne[2] == 1 and b.type == L.F32 and b.nb[0] == 4 and b.ne[2] == 1 and b.ne[3] == 1 and node.ne[0] == a.ne[1] and node.ne[1] == M
                    if M:
                        X = np.stack([_host_bytes(b.data + m * b.nb[1], 4 * K).view(np.float32) for m in range(M)])
                        _host_bytes(node.data, 4 * M * node.ne[0]).view(np.float32)[:] = _dot(cache[key], quantize_q8k(X)).reshape(-1)
                elif node.op == GGML_OP_GET_ROWS:
                    n = b.ne[0]
                    assert a.ne[2] == 1 and node.ne[2] == 1 and b.type == L.I32 and b.ne[1] == 1 and b.ne[2] == 1 and node.ne[0] == K and node.ne[1] == n
                    if n:
                        idx = _host_bytes(b.data, 4 * n).view(np.int32)
                        rows = np.stack([_host_bytes(a.data + int(r) * a.nb[1], (K // 256) * BS) for r in idx])
                        _host_bytes(node.data, 4 * n * K).view(np.float32)[:] = dequantize(rows, K).reshape(-1)
                else:
                    ids_t = node.src[2].contents
                    n_used, n_tok = ids_t.ne[0], ids_t.ne[1]
                    assert b.type == L.F32 and b.nb[0] == 4 and node.ne[1] == n_used and node.ne[2] == n_tok and node.nb[2] == node.nb[1] * n_used
                    W = np.stack([_rows(a, K, e) for e in range(a.ne[2])])
                    ids = np.stack([_host_bytes(ids_t.data + t * ids_t.nb[1], 4 * n_used).view(np.int32) for t in range(n_tok)])
                    X = np.stack([np.stack([_host_bytes(b.data + t * b.nb[2] + r * b.nb[1], 4 * K).view(np.float32) for r in range(b.ne[1])]) for t in range(n_tok)])
                    _host_bytes(node.data, 4 * n_tok * n_used * node.ne[0]).view(np.float32)[:] = mmid(W, X, ids).reshape(-1)
                continue
            st = lib.oracle_compute_node(g.nodes[i], nth if nth > 0 else n_threads)
            if st != 0:
                return st
        return 0

    return L.COMPUTE_FN(fn)
