"""GPU tests for weight matrices in IQ4_XS: acceptance, MUL_MAT on every kernel form of DESIGN.md 4g (streaming mat-vec, 2 .. 8-column mat-vec, the int8 tile
kernel from 9 columns), value edges, exact integers, column invariance, GET_ROWS, MUL_MAT_ID, the shared activation row and the test models.  The reference is the
NumPy twin of tests/iq4xs_ref.py (the oracle does not know the format; tests/test_iq4xs_ref_host.py pins the twin); the gates are the project's own: NMSE <= 1e-10
for a quantised MUL_MAT (tests/test_gpu_ops.py), 1e-3 for a model's logits (tests/test_gpu_model.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import harness as T
import iq4xs_ref as R
import legacy_ref as LR
import llama_box_amd as L
import moe_ref as MR
from model_util import Context, Model, greedy, preset

pytestmark = pytest.mark.gpu
GATE = 1e-10
QT = L.IQ4_XS
BS = 136
ALIGN = 8  # 136 = 8 * 17: the header is one aligned 8-byte load, the codes 16-byte loads at 8 mod 16


def _probe(H, backend, qt, K, N, M, buffer=None):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, qt, K, N)
        x = H.ggml_new_tensor_2d(ctx, L.F32, K, M)
        if buffer is not None:
            w.contents.buffer = buffer
        return bool(H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w, x)))
    finally:
        H.ggml_free(ctx)


# ---------------------------------------------------------------------------------------------- acceptance
def test_plain_2d_weight_is_accepted(H, backend):
    """What llama.cpp's loader asks: a plain 2-D tensor with a null buffer, for MUL_MAT, GET_ROWS and MUL_MAT_ID."""
    assert _probe(H, backend, QT, 256, 64, 1) and _probe(H, backend, QT, 4096, 33, 40)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        e = H.ggml_new_tensor_2d(ctx, QT, 512, 8)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, e, H.ggml_new_tensor_1d(ctx, L.I32, 3)))
        as_t = H.ggml_new_tensor_3d(ctx, QT, 256, 16, 4)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 5)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.I32, 2, 5)))
    finally:
        H.ggml_free(ctx)


def test_what_stays_refused(H, backend):
    """K % 256 != 0 (a 2-D view whose rows are 384 values of a 512-value parent stands for it), a base or a row stride below the block alignment, a 3-D
    weight in MUL_MAT; a view one block into its parent IS accepted."""
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, QT, 512, 8)
        x = H.ggml_new_tensor_2d(ctx, L.F32, 512, 1)
        mm = H.ggml_mul_mat(ctx, w, x)
        gr = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 3))
        assert H.ggml_backend_dev_supports_op(backend.dev, mm)
        for node in (mm, gr):
            for addr in (0x10000, 0x10000 + ALIGN, 0x10000 + BS):  # (+ BS: a view one block into its parent)
                w.contents.data = addr
                assert H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            for addr in (0x10001, 0x10002, 0x10000 + ALIGN // 2, 0x10000 + ALIGN + 1):
                w.contents.data = addr
                assert not H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            w.contents.data = 0x10000
            nb1 = w.contents.nb[1]
            for stride, ok in ((nb1 + BS, True), (nb1 + ALIGN // 2, False), (nb1 + 1, False)):
                w.contents.nb[1] = stride
                assert bool(H.ggml_backend_dev_supports_op(backend.dev, node)) == ok, stride
            w.contents.nb[1] = nb1
            w.contents.data = None
        w.contents.ne[0] = 384
        x.contents.ne[0] = 384
        assert not H.ggml_backend_dev_supports_op(backend.dev, mm)
        w3 = H.ggml_new_tensor_3d(ctx, QT, 256, 8, 2)
        assert not H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 2)))
        # the view itself, built through the API over a parent that has an address
        parent = H.ggml_new_tensor_1d(ctx, QT, 256 * 9)
        parent.contents.data = 0x20000
        v = H.ggml_view_2d(ctx, parent, 512, 4, 2 * BS, BS)
        assert v.contents.data == 0x20000 + BS
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, v, H.ggml_new_tensor_2d(ctx, L.F32, 512, 3)))
    finally:
        H.ggml_free(ctx)


def test_split_and_row_parallel_buffers_stay_refused(H, backend):
    addr = H.ggml_backend_reg_get_proc_address(backend.reg, b"ggml_backend_split_buffer_type")
    assert addr
    fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_float))(addr)
    split_buft = fn(0, (C.c_float * 16)(*([0.0] * 16)))
    assert split_buft
    buf = H.ggml_backend_buft_alloc_buffer(split_buft, 0)
    assert buf
    try:
        assert not _probe(H, backend, QT, 256, 64, 1, buffer=buf)
        assert _probe(H, backend, L.Q6_K, 256, 64, 1, buffer=buf)  # (what the split buffer serves today is unchanged)
    finally:
        H.ggml_backend_buffer_free(buf)
    rp = H.ggml_backend_buft_alloc_buffer(backend.rowpar_buft(), 1 << 16)
    assert rp
    try:
        assert not _probe(H, backend, QT, 256, 64, 1, buffer=rp)
        assert not _probe(H, backend, QT, 256, 64, 40, buffer=rp)
    finally:
        H.ggml_backend_buffer_free(rp)


# ---------------------------------------------------------------------------------------------- MUL_MAT
# (K, N, M): K {256: one super-block, 768: a partial wave, 4096: one full trip, 4352: a ragged second trip} x N {1, 3, 33, 257} x
# M {1, 2, 3, 8 | 9, 31, 33, 128, 160}: the streaming mat-vec (M 1), k_mmvq<T, 2 / 4 / 8> (M 2, 3, 8) and, from 9 columns, the int8 tile kernel in its
# 32-, 64- and 128-column forms (M 9 / 31, 33, 128 / 160), with and without a K split, on one and on several row panels
SHAPES = [(256, 1, 1), (768, 3, 1), (4096, 257, 1), (4352, 33, 1), (256, 33, 2), (4352, 3, 3), (768, 257, 8), (4096, 33, 8),
          (256, 1, 9), (768, 33, 9), (4352, 257, 31), (4096, 3, 33), (256, 257, 33), (768, 1, 128), (4096, 257, 128), (4352, 33, 160), (256, 3, 160)]
_REF = {}


def _case(K, N, M):
    """weights, activations and the twin's product for one shape: computed once, shared"""
    key = (K, N, M)
    if key not in _REF:
        rng = np.random.default_rng(23000 + K + N + M)
        W = R.rand_weight(K, N, rng)
        X = rng.standard_normal((M, K)).astype(np.float32)
        if K > 256 or M > 1:  # one activation super-block all zero (never the only one)
            X[M // 2, 256 * ((K // 256) // 2):256 * ((K // 256) // 2) + 256] = 0.0
        _REF[key] = (W, X, R.mul_mat(W, X))
    return _REF[key]


def _l1(W, X):
    """per output sum |x_i w_i| over the dequantised operands: the scale one wrong element is measured against"""
    K = X.shape[1]
    return np.abs(R.dequantize_q8k(R.quantize_q8k(X))) @ np.abs(R.dequantize(W, K).astype(np.float64)).T


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_n%d_m%d" % s)
def test_mul_mat_matches_the_twin(backend, plog, shape):
    K, N, M = shape
    W, X, ref = _case(K, N, M)
    k0, t0, s0, w0 = (backend.stat(k) for k in ("kernel_launches", "tiled_launches", "skinny_launches", "wide_launches"))
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    dk, dt = backend.stat("kernel_launches") - k0, backend.stat("tiled_launches") - t0
    e = T.nmse(got, ref)
    plog(f"iq4_xs mul_mat K={K} N={N} M={M} nmse={e:.3e} kernel_launches+{dk} tiled_launches+{dt}")
    assert np.any(ref != 0) and np.all(np.isfinite(got))
    assert e <= GATE, e
    # the form: one streaming launch with the f32 prologue (M 1); the Q8_K quantiser + ONE mat-vec pass (2 .. 8); the tile kernel, never mat-vec passes (9 and more)
    assert backend.stat("skinny_launches") == s0 and backend.stat("wide_launches") == w0
    if M == 1:
        assert (dk, dt) == (1, 0)
    elif M <= 8:
        assert (dk, dt) == (2, 0)
    else:
        assert dt == 1 and dk in (2, 3)  # (quantiser + tile kernel [+ the K split's reduction])


def test_batch_1_without_a_prologue_quantises_in_its_own_launch(backend, plog):
    """With the prologue option off (what the f32 prologue also falls back to when a result recycles its activation row's block) a batch-1 product is the Q8_K
    quantiser + the streaming kernel without prologue, and a gate / up / SwiGLU triple the quantiser + ONE two-matrix launch: same gates."""
    K, N = 768, 70
    rng = np.random.default_rng(623)
    Wg, Wu = R.rand_weight(K, N, rng), R.rand_weight(K, N, rng)
    X = rng.standard_normal((1, K)).astype(np.float32)
    H = L.host()

    def glu(g):
        x = g.new(L.F32, [K, 1], X)
        gate, up = (H.ggml_mul_mat(g.ctx, g.new(QT, [K, N], W), x) for W in (Wg, Wu))
        return H.ggml_swiglu_split(g.ctx, gate, up)

    backend.set_option("prologue", 0)
    try:
        k0 = backend.stat("kernel_launches")
        one = T.run_case(lambda g: R.g_mul_mat(g, Wg, X, K, N, 1), backend)[0].reshape(1, N)
        k1 = backend.stat("kernel_launches")
        both = T.run_case(glu, backend)[0].reshape(1, N)
        k2 = backend.stat("kernel_launches")
    finally:
        backend.set_option("prologue", 1)
    rg, ru = R.mul_mat(Wg, X).astype(np.float64), R.mul_mat(Wu, X).astype(np.float64)
    e1, e2 = T.nmse(one, rg), T.nmse(both, rg / (1.0 + np.exp(-rg)) * ru)
    plog(f"iq4_xs batch 1 without prologue: nmse={e1:.3e} (+{k1 - k0} launches), SwiGLU triple nmse={e2:.3e} (+{k2 - k1} launches)")
    assert (k1 - k0, k2 - k1) == (2, 2)
    assert e1 <= GATE and e2 <= GATE, (e1, e2)


def test_tile_kernel_on_128_row_panels(backend, plog):
    """The 128-row panel form of the tile kernel is chosen only for K >= 8192 on a full chip; the option mmq_bn = 128 asks for it at a test's size."""
    K, N, M = 4352, 257, 160
    W, X, ref = _case(K, N, M)
    backend.set_option("mmq_bn", 128)
    try:
        t0 = backend.stat("tiled_launches")
        got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
        assert backend.stat("tiled_launches") == t0 + 1
    finally:
        backend.set_option("mmq_bn", 0)
    e = T.nmse(got, ref)
    plog(f"iq4_xs mul_mat on 128-row panels K={K} N={N} M={M} nmse={e:.3e}")
    assert e <= GATE, e


def test_batch_with_the_tile_kernel_off_falls_to_mat_vec_passes(backend, plog):
    """Option mmq_i8 = 0: a 20-column batch is the quantiser + three passes of the multi-column mat-vec kernel (8 + 8 + 4), same gate."""
    K, N, M = 768, 33, 20
    W, X, ref = _case(K, N, M)
    backend.set_option("mmq_i8", 0)
    try:
        k0, t0 = backend.stat("kernel_launches"), backend.stat("tiled_launches")
        got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
        dk, dt = backend.stat("kernel_launches") - k0, backend.stat("tiled_launches") - t0
    finally:
        backend.set_option("mmq_i8", 1)
    e = T.nmse(got, ref)
    plog(f"iq4_xs mul_mat with mmq_i8 off K={K} N={N} M={M} nmse={e:.3e} kernel_launches+{dk}")
    assert (dk, dt) == (4, 0)
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- value edges
@pytest.mark.parametrize("M", [1, 2, 4, 8, 9, 33, 64, 130], ids=lambda m: f"m{m}")
def test_value_edges(backend, plog, M):
    """Scales all 0 (-32) and all 63, codes at either end of the table, the largest products of both signs, negative, zero and subnormal d — against activations
    that quantise to +-127 everywhere, one-hot rows, a zero super-block and ordinary rows.  The NMSE gate and, so that a single wrong element cannot hide in a
    large row, max |got - ref| <= 1e-6 of the row's sum |x_i w_i|."""
    K, N = 768, 40
    rng = np.random.default_rng(77 + QT)
    W = R.edge_blocks(N * 3, rng).reshape(N, -1)
    W[1] = np.tile(R.make_iq4xs(np.zeros((1, 8)), np.zeros((1, 256)), [1.0])[0], 3)  # row 1: -32 x -127 in every position
    rows = [np.where(rng.random(K) < 0.5, -3.0, 3.0), np.full(K, 5.0), np.full(K, -0.25), np.eye(1, K, 17)[0] * 2.0, np.eye(1, K, K - 1)[0] * -7.0,
            rng.standard_normal(K), rng.standard_normal(K) * 1e-3, rng.standard_normal(K) * 1e3]
    rows[5][256:512] = 0.0
    X = np.stack([rows[i % len(rows)] for i in range(M)]).astype(np.float32) if M > 1 else np.stack(rows[:1]).astype(np.float32)
    y = R.quantize_q8k(X)
    assert np.all(np.abs(y["qs"][0]) == 127)  # (row 0 quantises to +-127 in every position)
    ref = R.mul_mat(W, X)
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    l1 = _l1(W, X)
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / (l1 + 1e-30)))
    e = T.nmse(got, ref)
    plog(f"iq4_xs value edges M={M}: nmse={e:.3e} max |diff| / row L1 = {worst:.3e}")
    assert np.all(np.isfinite(got)) and np.any(ref != 0)
    assert e <= GATE, e
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * l1), worst


# ---------------------------------------------------------------------------------------------- exact integers
def _exact_case(K, N, M, seed):
    """Weights with d a power of two — row 0: -32 x -127 in every position, row 1: 31 x -127, the rest sampled over every field — and activations dy * q with dy a
    power of two, q one anchor of magnitude 127 per block and otherwise -1, 0, 1: every product, partial sum and scaled sum is an integer multiple of d * dy below
    2^24 of them, so float32 holds the result exactly whatever the order of additions."""
    rng = np.random.default_rng(seed)
    nb = K // 256
    sc, nib = rng.integers(0, 64, (N, nb, 8)), rng.integers(0, 16, (N, nb, 256))
    sc[0], nib[0] = 0, 0
    sc[1], nib[1] = 63, 0
    d = np.exp2(rng.integers(-1, 2, (N, nb))) * rng.choice([-1.0, 1.0], (N, nb))  # +-0.5, 1, 2
    d[0:2] = 1.0
    W = R.make_iq4xs(sc.reshape(-1, 8), nib.reshape(-1, 256), d.reshape(-1)).reshape(N, nb * BS)
    q = rng.integers(-1, 2, (M, nb, 256))
    q[np.arange(M)[:, None], np.arange(nb)[None, :], rng.integers(0, 256, (M, nb))] = rng.choice([-127, 127], (M, nb))
    dy = np.exp2(rng.integers(-4, 3, (M, 1, 1)))
    X = (q * dy).reshape(M, K).astype(np.float32)
    return W, X


@pytest.mark.parametrize("M", [1, 2, 4, 8, 9, 33, 130], ids=lambda m: f"m{m}")
def test_integer_products_are_exact(backend, M):
    """-32 x -127 = 4064 and 31 x -127 = -3937 in every position (neither fits an int8: the tile kernel splits them in two pieces), and sampled blocks, on the
    mat-vec (M 1, 4) and the three column-tile forms (M 9, 33, 130): bit-equal to the twin.  A wrong piece split, a swapped nibble half or a wrong scales_h
    shift changes integers, not roundings."""
    K, N = 768, 37
    W, X = _exact_case(K, N, M, 4064 + M)
    y = R.quantize_q8k(X)
    a = np.abs(y["qs"].astype(np.int32))
    assert np.all((a == 127).sum(axis=2) == 1) and np.all((a <= 1) | (a == 127))  # one anchor a block, otherwise -1, 0, 1
    dq = np.abs(y["d"])
    assert np.all(np.exp2(np.round(np.log2(dq))) == dq)  # powers of two
    u = R.unpack(W, K)
    # every partial sum stays below 2^24 units of (the smallest |d|) * dy: the sum over the row of |d| / 0.5 * |ls - 32| * |sub-block sum| bounds every order of
    # additions (dy is one power of two a row)
    bound = np.einsum("mrbs,rbs->mr", np.abs(R.sub_sums(u, y)), np.abs(u["scale"]) * (np.abs(u["d"]).astype(np.float64) / 0.5)[..., None])
    assert np.all(np.abs(u["d"]) >= 0.5) and float(bound.max()) < 2.0 ** 24, float(bound.max())
    ref = R.mul_mat(W, X)
    assert np.array_equal(ref.astype(np.float64), R.dequantize_q8k(y) @ R.dequantize(W, K).astype(np.float64).T)  # (the twin itself is exact here)
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------- column invariance
def test_multi_column_matvec_equals_single_columns(backend):
    K, N = 768, 37
    rng = np.random.default_rng(31 + QT)
    W = R.rand_weight(K, N, rng)
    Xall = rng.standard_normal((8, K)).astype(np.float32)
    ones = [T.run_case(lambda g: R.g_mul_mat(g, W, Xall[c:c + 1], K, N, 1), backend)[0].reshape(N) for c in range(8)]
    for M in range(2, 9):
        got = T.run_case(lambda g: R.g_mul_mat(g, W, Xall[:M], K, N, M), backend)[0].reshape(M, N)
        for c in range(M):
            assert np.array_equal(got[c].view(np.uint32), ones[c].view(np.uint32)), (M, c)


# ---------------------------------------------------------------------------------------------- GET_ROWS
@pytest.mark.parametrize("nblk", [1, 2, 3, 17], ids=lambda n: f"blocks{n}")
def test_get_rows_bit_equal(backend, nblk):
    K, N = 256 * nblk, 9
    rng = np.random.default_rng(9 + QT)
    W = np.concatenate([R.rand_weight(K, N - 2, rng), R.edge_blocks(2 * nblk, rng).reshape(2, -1)])
    idx = np.array([8, 0, 3, 3, 2, 8, 7, 1], dtype=np.int32)  # repeated and out of order
    got = T.run_case(lambda g: R.g_get_rows(g, W, idx, K, N), backend)[0].reshape(len(idx), K)
    want = R.dequantize(W, K)[idx]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- MUL_MAT over a view at the minimum alignment
@pytest.mark.parametrize("M", [1, 3, 8, 9, 33, 160], ids=lambda m: f"m{m}")
def test_mul_mat_over_a_view_one_block_into_its_parent(backend, plog, M):
    K, N = 512, 33
    rng = np.random.default_rng(500 * QT + M)
    W = R.rand_weight(K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    g = T.G(backend)
    try:
        out = R.g_mul_mat_offset_view(g, W, X, K, N, M)
        got = MR.compute_in_weights_buffer(g, [out])[0].reshape(M, N)
        w = out.contents.src[0].contents
        assert w.view_offs == BS and w.data % ALIGN == 0 and w.data % 16 == BS % 16, (w.view_offs, hex(w.data))
    finally:
        g.free()
    e = T.nmse(got, R.mul_mat(W, X))
    plog(f"iq4_xs mul_mat over an offset view M={M} base % 16 = {BS % 16} nmse={e:.3e}")
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- MUL_MAT_ID
@pytest.mark.parametrize("n_tokens", [1, 3, 8, 16, 32, 40], ids=lambda n: f"tokens{n}")
@pytest.mark.parametrize("per_slot", [False, True], ids=["shared_row", "per_slot"])
def test_mul_mat_id_matches_the_twin_and_the_backends_own_mat_vec(backend, plog, per_slot, n_tokens):
    """n_tokens 1, 3, 8, 16 (n_used * n_tokens <= 32), 32 and 40: NMSE <= 1e-10 against the twin, and up to 32 pairs every (slot, token) result is bit-equal to the
    backend's own one-column MUL_MAT over that expert's 2-D view (the contract of DESIGN.md 4b)."""
    K, N, n_expert, n_used = 512, 70, 4, 2
    rng = np.random.default_rng(3000 + 13 * QT + per_slot + 100 * n_tokens)
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    cases = []
    for n_tok in (n_tokens,):
        ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
        cases.append((rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32), ids))
    H = L.host()
    g = T.G(backend)
    try:
        as_t = g.new(QT, [K, N, n_expert], W)
        outs, cols = [], []
        for b, ids in cases:
            n_tok, rows = b.shape[0], b.shape[1]
            bt = g.new(L.F32, [K, rows, n_tok], b)
            outs.append(H.ggml_mul_mat_id(g.ctx, as_t, bt, MR.strided_ids(g, ids, n_expert)))
            if n_used * n_tok <= 32:
                for t in range(n_tok):
                    for s in range(n_used):
                        col = H.ggml_view_2d(g.ctx, bt, K, 1, K * 4, (t * rows + (s if rows > 1 else 0)) * K * 4)
                        cols.append(H.ggml_mul_mat(g.ctx, MR.expert_view(g, as_t, K, N, ids[t, s]), col))
        m0 = backend.stat("mmid_launches")
        res = MR.compute_in_weights_buffer(g, outs + cols)
        assert backend.stat("mmid_launches") - m0 == len(outs)
    finally:
        g.free()
    ci = 0
    for k, (b, ids) in enumerate(cases):
        n_tok = ids.shape[0]
        got = res[k].reshape(n_tok, n_used, N)
        T.compare(f"iq4_xs mul_mat_id n_tokens={n_tok}", got, R.mmid(W, b, ids), GATE, log=plog)
        if n_used * n_tok <= 32:
            for t in range(n_tok):
                for s in range(n_used):
                    own = res[len(outs) + ci].reshape(N)
                    ci += 1
                    assert np.array_equal(got[t, s].view(np.uint32), own.view(np.uint32)), f"n_tokens={n_tok}: (slot {s}, token {t}) differs from MUL_MAT over the expert's view"
    assert ci == len(cols)


def test_mul_mat_id_with_an_id_outside_the_experts_writes_zeros(backend):
    K, N, n_expert, n_used, n_tok = 256, 70, 4, 2, 4
    rng = np.random.default_rng(40 + QT)
    H = L.host()
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    b = rng.standard_normal((n_tok, n_used, K)).astype(np.float32)
    good = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    bad = good.copy()
    bad[1, 0] = n_expert
    bad[2, 1] = -1

    def build(g):
        as_t = g.new(QT, [K, N, n_expert], W)
        bt = g.new(L.F32, [K, n_used, n_tok], b)
        return [H.ggml_mul_mat_id(g.ctx, as_t, bt, MR.strided_ids(g, i, n_expert)) for i in (good, bad)]

    rg, rb = [r.reshape(n_tok, n_used, N) for r in T.run_case(build, backend)]
    assert np.count_nonzero(rg) > rg.size // 2
    assert T.nmse(rb, R.mmid(W, b, bad)) <= GATE
    for t in range(n_tok):
        for s in range(n_used):
            want = np.zeros(N, dtype=np.float32) if (t, s) in ((1, 0), (2, 1)) else rg[t, s]
            assert np.array_equal(rb[t, s].view(np.uint32), want.view(np.uint32)), (t, s)


# ---------------------------------------------------------------------------------------------- one norm output, three formats, two activation kinds
KINDS = (L.IQ4_XS, L.IQ4_NL, L.Q4_K)


def _mixed_layer(backend, order, Ws, nw, X, K, N, M):
    """cur = MUL(RMS_NORM(x), w) feeds an IQ4_XS, an IQ4_NL and a Q4_K matrix; the three MUL_MAT nodes enter the graph in `order`.  -> the products in KINDS order"""
    H = L.host()
    g = T.G(backend)
    try:
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X, "x"), 1e-5), g.new(L.F32, [K], nw, "norm"))
        mm = {qt: H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt], L.TYPE_NAME.get(qt, "q4_K")), cur) for qt in order}
        return g.compute([mm[qt] for qt in KINDS], expand_first=[mm[qt] for qt in order])
    finally:
        g.free()


def _quantiser_classes(backend):
    """{timing class: launches} of the activation quantisers since the last report"""
    return {c: n for c, (n, _ms, _b) in backend.timing_report().items() if n and "quantize" in c}


@pytest.mark.parametrize("M", [1, 2, 4, 9, 33], ids=lambda m: f"m{m}")
def test_iq4_xs_iq4_nl_and_q4_k_matrices_share_one_norm_output_in_every_node_order(backend, plog, M):
    """One norm output read by an IQ4_XS, an IQ4_NL and a Q4_K matrix — a Q8_K activation row serves the first and the last, a Q8_0 row the IQ4_NL matrix (two
    kinds keyed in the activation cache): every one of the six node orders gives the same bits, and those meet the gate against the twin (IQ4_NL, Q4_K: the
    oracle) over the oracle's norm output."""
    K, N = 512, 48
    rng = np.random.default_rng(70 + M + QT)
    Ws = {L.IQ4_XS: R.rand_weight(K, N, rng), L.IQ4_NL: LR.rand_weight(L.IQ4_NL, K, N, rng), L.Q4_K: T.rand_weight(L.Q4_K, K, N, rng)}
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    X = (rng.standard_normal((M, K)) + 0.3).astype(np.float32)
    H = L.host()

    def norm_and_oracle_formats(g):
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X), 1e-5), g.new(L.F32, [K], nw))
        return [cur] + [H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt]), cur) for qt in (L.IQ4_NL, L.Q4_K)]

    cur, refnl, ref4 = T.run_case(norm_and_oracle_formats, "oracle")
    ref = {L.IQ4_XS: R.mul_mat(Ws[L.IQ4_XS], cur.reshape(M, K)), L.IQ4_NL: refnl.reshape(M, N), L.Q4_K: ref4.reshape(M, N)}
    first = None
    for order in itertools.permutations(KINDS):
        backend.set_option("timing", 1)
        backend.timing_report()
        try:
            got = _mixed_layer(backend, order, Ws, nw, X, K, N, M)
            # the activation cache is one slot keyed by (tensor, kind, bytes): the Q8_0 row of the IQ4_NL matrix and the Q8_K row that IQ4_XS and Q4_K share are
            # two entries, so a batch costs one quantiser launch per change of kind along the node order: 2 when the Q8_K users are neighbours, 3 when the
            # IQ4_NL node sits between them; at M = 1 the Q8_K users quantise in their own prologue and only the Q8_0 row has a launch
            nq = sum(_quantiser_classes(backend).values())
            plog(f"iq4_xs shared norm output M={M} order {[L.TYPE_NAME.get(q, 'q4_K') for q in order]}: {nq} quantiser launches")
            assert nq == (1 if M == 1 else (3 if order[1] == L.IQ4_NL else 2)), (order, nq)
        finally:
            backend.set_option("timing", 0)
        if first is None:
            first = got
            for qt, a in zip(KINDS, got):
                e = T.nmse(a.reshape(M, N), ref[qt])
                plog(f"iq4_xs shared norm output M={M} type {L.TYPE_NAME.get(qt, 'q4_K')}: nmse={e:.3e}")
                assert e <= GATE, (qt, e)
        for qt, a, b in zip(KINDS, got, first):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (qt, order)


# ---------------------------------------------------------------------------------------------- model level
PROMPT40 = [(7 * i + 3) % 512 for i in range(40)]


def _accepted(H, backend, ctx):
    gf = H.llm_last_graph(ctx.c)
    for i in range(gf.contents.n_nodes):
        assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i]), gf.contents.nodes[i].contents.name


@pytest.mark.parametrize("fa", [0, 1], ids=["nofa", "fa"])
def test_iq4xs_model_runs_whole_on_the_device(H, backend, plog, fa):
    """test-llama-iq4xs (IQ4_XS embeddings, IQ4_XS / IQ4_NL / Q4_K / Q6_K layer matrices) on the peaked weight set (output rows tied to the embeddings, the
    project's tool for a decisive reference: llm_hparams::peaked): a 9- and a 40-token prompt batch, 16 batch-1 steps and a 4-sequence step against the hybrid
    (oracle + twin) reference, logits NMSE <= 1e-3 at each; every node accepted by the device.  Greedy ids: the device's own free-running greedy run equals the
    reference's at EVERY step, and so does the arg-max of every teacher-forced row.  That the reference is decisive is checked on the reference alone: its
    smallest top-2 margin is above 1 on logits spanning about 30 (2.9 at this seed, where its own soft-max and flash runs differ by 0.06 at most)."""
    hp = preset("test-llama-iq4xs")
    hp.peaked = 8
    mg, mc = Model(hp, 1234, backend.buft), Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=fa), Context(mc, compute=R.hybrid_compute_fn(), flash_attn=fa)
    n_gen = 16
    try:
        assert H.llm_model_tensor(mg.m, b"token_embd.weight").contents.type == QT and H.llm_model_tensor(mg.m, b"blk.0.ffn_up.weight").contents.type == QT
        t0 = backend.stat("tiled_launches")
        for n in (9, 40):
            cc.clear()
            cg.clear()
            rc, ref = cc.decode(PROMPT40[:n], range(n))
            rc2, got = cg.decode(PROMPT40[:n], range(n))
            assert rc == 0 and rc2 == 0
            _accepted(H, backend, cg)
            e = T.nmse(got, ref)
            plog(f"test-llama-iq4xs (peaked) fa={fa} {n}-token prompt logits: nmse={e:.3e}")
            assert e <= 1e-3
        assert backend.stat("tiled_launches") > t0
        cc.clear()
        cg.clear()
        ids_ref, rows_ref = greedy(cc, PROMPT40, n_gen)
        rows_ref = np.stack(rows_ref)
        top2 = np.sort(rows_ref, axis=1)
        margins = top2[:, -1] - top2[:, -2]
        assert float(margins.min()) > 1.0 and len(set(ids_ref)) > n_gen // 2, (margins, ids_ref)  # (the reference: decisive, and not one token repeated)
        ids_got, _ = greedy(cg, PROMPT40, n_gen)  # the device's own greedy run
        _accepted(H, backend, cg)
        assert ids_got == ids_ref, (ids_got, ids_ref)
        cg.clear()
        rc, lg = cg.decode(PROMPT40, range(40), want=[0] * 39 + [1])
        assert rc == 0
        rows_got = [lg[-1]]
        for i, t in enumerate(ids_ref[:-1]):
            rc, l1 = cg.decode([t], [40 + i])
            assert rc == 0
            rows_got.append(l1[0])
        _accepted(H, backend, cg)
        rows_got = np.stack(rows_got)
        e_dec = T.nmse(rows_got, rows_ref)
        agree = np.argmax(rows_got, axis=1) == np.array(ids_ref)
        plog(f"test-llama-iq4xs (peaked) fa={fa} teacher-forced decode x{n_gen}: nmse={e_dec:.3e} argmax agreement {int(agree.sum())}/{len(agree)}, "
             f"reference's min top-2 margin {margins.min():.3e}, max |d| {np.max(np.abs(rows_got - rows_ref)):.3e}")
        assert e_dec <= 1e-3
        assert bool(np.all(agree)), np.flatnonzero(~agree)
        cc.clear()
        cg.clear()
        seqs = [0, 1, 2, 3]
        out = []
        for c in (cg, cc):
            rc, l0 = c.decode([3, 11, 200, 45], [0] * 4, seq=seqs, want=[1] * 4)
            assert rc == 0
            rc, l1 = c.decode([5, 6, 7, 8], [1] * 4, seq=seqs, want=[1] * 4)
            assert rc == 0
            out.append(np.concatenate([l0, l1]))
        _accepted(H, backend, cg)
        e4 = T.nmse(out[0], out[1])
        plog(f"test-llama-iq4xs (peaked) fa={fa} 4-sequence steps: nmse={e4:.3e}")
        assert e4 <= 1e-3
    finally:
        for o in (cg, cc, mg, mc):
            o.free()


def test_iq4xs_decode_step_runs_in_a_captured_graph_and_replays_bit_identical_to_eager(backend, H, plog):
    mg = Model(preset("test-llama-iq4xs"), 99, backend.buft)
    outs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            c = Context(mg, backend=backend, flash_attn=1)
            l0 = backend.stat("graph_launches")
            ids, rows = greedy(c, PROMPT40[:20], 24)
            outs[mode] = (ids, np.stack(rows), backend.stat("graph_launches") - l0)
            c.free()
    finally:
        backend.set_option("graphs", 1)
        mg.free()
    plog(f"test-llama-iq4xs: hipGraph launches with graphs=1: {outs[1][2]}, with graphs=0: {outs[0][2]}")
    assert outs[1][2] >= 10 and outs[0][2] == 0
    assert outs[1][0] == outs[0][0]
    assert np.array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))


def test_single_format_model_runs_whole_on_the_device(H, backend, plog):
    """test-llama's shape as a *-IQ4_XS.gguf holds it (LLM_FTYPE_IQ4_XS = 17): gate and up share the base format in every layer, so the batch-1 step takes the SwiGLU
    form of the streaming mat-vec with the norm prologue (asserted by its timing class).  A 9-token prompt and 4 teacher-forced steps, logits NMSE <= 1e-3."""
    hp = preset("test-llama", ftype=17)
    mg, mc = Model(hp, 7, backend.buft), Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=1), Context(mc, compute=R.hybrid_compute_fn(), flash_attn=1)
    try:
        for n in (b"blk.0.ffn_gate.weight", b"blk.0.ffn_up.weight", b"token_embd.weight"):
            assert H.llm_model_tensor(mg.m, n).contents.type == QT
        ids_ref, rows_ref = greedy(cc, PROMPT40[:9], 5)
        rc, lg = cg.decode(PROMPT40[:9], range(9), want=[0] * 8 + [1])
        assert rc == 0
        _accepted(H, backend, cg)
        rows_got = [lg[-1]]
        backend.set_option("timing", 1)
        backend.timing_report()
        for i, t in enumerate(ids_ref[:-1]):
            rc, l1 = cg.decode([t], [9 + i])
            assert rc == 0
            rows_got.append(l1[0])
        classes = sorted(backend.timing_report())
        _accepted(H, backend, cg)
        e = T.nmse(np.stack(rows_got), np.stack(rows_ref))
        plog(f"test-llama in iq4_xs: prompt + 4 decode rows nmse={e:.3e}; mat-vec classes {[c for c in classes if c.startswith('mmvq_')]}")
        assert e <= 1e-3
        assert "mmvq_iq4_xs_glu_normpro" in classes, classes
    finally:
        backend.set_option("timing", 0)
        for o in (cg, cc, mg, mc):
            o.free()
