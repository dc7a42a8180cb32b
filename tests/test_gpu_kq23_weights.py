"""GPU tests for weight matrices in Q2_K / Q3_K: acceptance, MUL_MAT on every kernel form of DESIGN.md 4e (streaming mat-vec, 2 .. 8-column mat-vec, the
int8 tile kernel from 9 columns), value edges, column invariance, GET_ROWS, MUL_MAT_ID, the shared activation row and the test models.  The reference is the NumPy
twin of tests/kq23_ref.py (the oracle does not know the two formats; tests/test_kq23_ref_host.py pins the twin); the gates are the project's own: NMSE <= 1e-10 for a
quantised MUL_MAT (tests/test_gpu_ops.py), 1e-3 for a model's logits (tests/test_gpu_model.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import harness as T
import kq23_ref as R
import llama_box_amd as L
import moe_ref as MR
from model_util import Context, Model, greedy, preset

pytestmark = pytest.mark.gpu
GATE = 1e-10
IDS = lambda q: L.TYPE_NAME[q] if isinstance(q, int) and q in L.TYPE_NAME else str(q)  # noqa: E731
ALIGN = {L.Q2_K: 4, L.Q3_K: 2}  # 84-byte blocks are read as dwords, 110-byte blocks at 2 bytes


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
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_plain_2d_weight_is_accepted(H, backend, qt):
    """What llama.cpp's loader asks: a plain 2-D tensor with a null buffer, for MUL_MAT, GET_ROWS and MUL_MAT_ID."""
    assert _probe(H, backend, qt, 256, 64, 1) and _probe(H, backend, qt, 4096, 33, 40)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        e = H.ggml_new_tensor_2d(ctx, qt, 512, 8)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, e, H.ggml_new_tensor_1d(ctx, L.I32, 3)))
        as_t = H.ggml_new_tensor_3d(ctx, qt, 256, 16, 4)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 5)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.I32, 2, 5)))
    finally:
        H.ggml_free(ctx)


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_what_stays_refused(H, backend, qt):
    """K % 256 != 0 (a 2-D view whose rows are 384 values of a 512-value parent stands for it), a base or a row stride below the block alignment, a 3-D
    weight in MUL_MAT; a view one block into its parent IS accepted."""
    al, bs = ALIGN[qt], L.TYPE_SIZE[qt]
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, qt, 512, 8)
        x = H.ggml_new_tensor_2d(ctx, L.F32, 512, 1)
        mm = H.ggml_mul_mat(ctx, w, x)
        gr = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 3))
        assert H.ggml_backend_dev_supports_op(backend.dev, mm)
        for node in (mm, gr):
            for addr in (0x10000, 0x10000 + al, 0x10000 + bs):  # (+ bs: a view one block into its parent)
                w.contents.data = addr
                assert H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            for addr in (0x10001, 0x10000 + al // 2, 0x10000 + al + 1):
                w.contents.data = addr
                assert not H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            w.contents.data = 0x10000
            nb1 = w.contents.nb[1]
            for stride, ok in ((nb1 + bs, True), (nb1 + al // 2, False), (nb1 + 1, False)):
                w.contents.nb[1] = stride
                assert bool(H.ggml_backend_dev_supports_op(backend.dev, node)) == ok, stride
            w.contents.nb[1] = nb1
            w.contents.data = None
        w.contents.ne[0] = 384
        x.contents.ne[0] = 384
        assert not H.ggml_backend_dev_supports_op(backend.dev, mm)
        w3 = H.ggml_new_tensor_3d(ctx, qt, 256, 8, 2)
        assert not H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 2)))
        # the view itself, built through the API over a parent that has an address
        parent = H.ggml_new_tensor_1d(ctx, qt, 256 * 9)
        parent.contents.data = 0x20000
        v = H.ggml_view_2d(ctx, parent, 512, 4, 2 * bs, bs)
        assert v.contents.data == 0x20000 + bs
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, v, H.ggml_new_tensor_2d(ctx, L.F32, 512, 3)))
    finally:
        H.ggml_free(ctx)


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_split_buffer_weight_stays_refused(H, backend, qt):
    addr = H.ggml_backend_reg_get_proc_address(backend.reg, b"ggml_backend_split_buffer_type")
    assert addr
    fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_float))(addr)
    split_buft = fn(0, (C.c_float * 16)(*([0.0] * 16)))
    assert split_buft
    buf = H.ggml_backend_buft_alloc_buffer(split_buft, 0)
    assert buf
    try:
        assert not _probe(H, backend, qt, 256, 64, 1, buffer=buf)
        assert _probe(H, backend, L.Q6_K, 256, 64, 1, buffer=buf)  # (what the split buffer serves today is unchanged)
    finally:
        H.ggml_backend_buffer_free(buf)


# ---------------------------------------------------------------------------------------------- MUL_MAT
# (K, N, M): K {256: one super-block, 768: a partial wave, 4096: one full trip, 4352: a ragged second trip} x N {1, 3, 33, 257} x
# M {1, 2, 3, 8 | 9, 31, 33, 128, 160}: the streaming mat-vec (M 1), k_mmvq<T, 2 / 4 / 8> (M 2, 3, 8) and, from 9 columns, the int8 tile kernel in its
# 32-, 64- and 128-column forms (M 9 / 31, 33, 128 / 160), with and without a K split, on one and on several row panels
SHAPES = [(256, 1, 1), (768, 3, 1), (4096, 257, 1), (4352, 33, 1), (256, 33, 2), (4352, 3, 3), (768, 257, 8), (4096, 33, 8),
          (256, 1, 9), (768, 33, 9), (4352, 257, 31), (4096, 3, 33), (256, 257, 33), (768, 1, 128), (4096, 257, 128), (4352, 33, 160), (256, 3, 160)]
_REF = {}


def _case(qt, K, N, M):
    """weights, activations and the twin's product for one (format, shape): computed once, shared"""
    key = (qt, K, N, M)
    if key not in _REF:
        rng = np.random.default_rng(1000 * qt + K + N + M)
        W = R.rand_weight(qt, K, N, rng)
        X = rng.standard_normal((M, K)).astype(np.float32)
        if K > 256 or M > 1:  # one activation super-block all zero (never the only one)
            X[M // 2, 256 * ((K // 256) // 2):256 * ((K // 256) // 2) + 256] = 0.0
        _REF[key] = (W, X, R.mul_mat(qt, W, X))
    return _REF[key]


def _l1(qt, W, X):
    """per output sum |x_i w_i| over the dequantised operands: the scale one wrong element is measured against"""
    K = X.shape[1]
    return np.abs(R.dequantize_q8k(R.quantize_q8k(X))) @ np.abs(R.dequantize(qt, W, K).astype(np.float64)).T


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_n%d_m%d" % s)
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_matches_the_twin(backend, plog, qt, shape):
    K, N, M = shape
    W, X, ref = _case(qt, K, N, M)
    k0, t0, s0, w0 = (backend.stat(k) for k in ("kernel_launches", "tiled_launches", "skinny_launches", "wide_launches"))
    got = T.run_case(lambda g: R.g_mul_mat(g, qt, W, X, K, N, M), backend)[0].reshape(M, N)
    dk, dt = backend.stat("kernel_launches") - k0, backend.stat("tiled_launches") - t0
    e = T.nmse(got, ref)
    plog(f"kq23 mul_mat {L.TYPE_NAME[qt]} K={K} N={N} M={M} nmse={e:.3e} kernel_launches+{dk} tiled_launches+{dt}")
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


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_batch_1_without_a_prologue_quantises_in_its_own_launch(backend, plog, qt):
    """With the prologue option off (what the f32 prologue also falls back to when a result recycles its activation row's block) a batch-1 product is the Q8_K
    quantiser + the streaming kernel without prologue, and a gate / up / SwiGLU triple the quantiser + ONE two-matrix launch: same gates."""
    K, N = 768, 70
    rng = np.random.default_rng(600 + qt)
    Wg, Wu = R.rand_weight(qt, K, N, rng), R.rand_weight(qt, K, N, rng)
    X = rng.standard_normal((1, K)).astype(np.float32)
    H = L.host()

    def glu(g):
        x = g.new(L.F32, [K, 1], X)
        gate, up = (H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], W), x) for W in (Wg, Wu))
        return H.ggml_swiglu_split(g.ctx, gate, up)

    backend.set_option("prologue", 0)
    try:
        k0 = backend.stat("kernel_launches")
        one = T.run_case(lambda g: R.g_mul_mat(g, qt, Wg, X, K, N, 1), backend)[0].reshape(1, N)
        k1 = backend.stat("kernel_launches")
        both = T.run_case(glu, backend)[0].reshape(1, N)
        k2 = backend.stat("kernel_launches")
    finally:
        backend.set_option("prologue", 1)
    rg, ru = R.mul_mat(qt, Wg, X).astype(np.float64), R.mul_mat(qt, Wu, X).astype(np.float64)
    e1, e2 = T.nmse(one, rg), T.nmse(both, rg / (1.0 + np.exp(-rg)) * ru)
    plog(f"kq23 batch 1 without prologue {L.TYPE_NAME[qt]}: nmse={e1:.3e} (+{k1 - k0} launches), SwiGLU triple nmse={e2:.3e} (+{k2 - k1} launches)")
    assert (k1 - k0, k2 - k1) == (2, 2)
    assert e1 <= GATE and e2 <= GATE, (e1, e2)


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_tile_kernel_on_128_row_panels(backend, plog, qt):
    """The 128-row panel form of the tile kernel is chosen only for K >= 8192 on a full chip; the option mmq_bn = 128 asks for it at a test's size."""
    K, N, M = 4352, 257, 160
    W, X, ref = _case(qt, K, N, M)
    backend.set_option("mmq_bn", 128)
    try:
        t0 = backend.stat("tiled_launches")
        got = T.run_case(lambda g: R.g_mul_mat(g, qt, W, X, K, N, M), backend)[0].reshape(M, N)
        assert backend.stat("tiled_launches") == t0 + 1
    finally:
        backend.set_option("mmq_bn", 0)
    e = T.nmse(got, ref)
    plog(f"kq23 mul_mat on 128-row panels {L.TYPE_NAME[qt]} K={K} N={N} M={M} nmse={e:.3e}")
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- value edges
@pytest.mark.parametrize("M", [1, 33], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_value_edges(backend, plog, qt, M):
    """Scales / mins all 0 and all at their maximum, hmask all clear / all set, levels at either end, negative and zero d / dmin, the Q3_K block with -4 x -32 in
    every position — against activations that quantise to +-127 everywhere, one-hot rows, a zero super-block and ordinary rows.  The NMSE gate and, so that a
    single wrong element cannot hide in a large row, max |got - ref| <= 1e-6 of the row's sum |x_i w_i|."""
    K, N = 768, 40
    rng = np.random.default_rng(77 + qt)
    W = R.edge_blocks(qt, N * 3, rng).reshape(N, -1)
    # row 1: one extreme block three times — Q3_K: -4 x -32 in every position; Q2_K: every nibble 15, every level 3
    first = (R.make_q3k(np.zeros((1, 16)), np.full((1, 256), -4), [1.0]) if qt == L.Q3_K else
             R.make_q2k(np.full((1, 16), 15), np.full((1, 16), 15), np.full((1, 256), 3), [1.0], [0.5]))
    W[1] = np.tile(first[0], 3)
    rows = [np.where(rng.random(K) < 0.5, -3.0, 3.0), np.full(K, 5.0), np.full(K, -0.25), np.eye(1, K, 17)[0] * 2.0, np.eye(1, K, K - 1)[0] * -7.0,
            rng.standard_normal(K), rng.standard_normal(K) * 1e-3, rng.standard_normal(K) * 1e3]
    rows[5][256:512] = 0.0
    X = np.stack([rows[i % len(rows)] for i in range(M)]).astype(np.float32) if M > 1 else np.stack(rows[:1]).astype(np.float32)
    y = R.quantize_q8k(X)
    assert np.all(np.abs(y["qs"][0]) == 127)  # (row 0 quantises to +-127 in every position)
    ref = R.mul_mat(qt, W, X)
    got = T.run_case(lambda g: R.g_mul_mat(g, qt, W, X, K, N, M), backend)[0].reshape(M, N)
    l1 = _l1(qt, W, X)
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / (l1 + 1e-30)))
    e = T.nmse(got, ref)
    plog(f"kq23 value edges {L.TYPE_NAME[qt]} M={M}: nmse={e:.3e} max |diff| / row L1 = {worst:.3e}")
    assert np.all(np.isfinite(got)) and np.any(ref != 0)
    assert e <= GATE, e
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * l1), worst


def test_q3_k_minus_four_times_minus_thirty_two_in_every_position_is_exact(backend):
    """Every scale 0 (-32) and every hmask bit clear with low bits 0 (-4): the product +128 does not fit the tile kernel's int8 piece.  d = 1 and activations that
    quantise to small integers with d_act = 1 make every output an exactly representable integer: 128 x sum(q), bit for bit, on the mat-vec and on the tile kernel."""
    K, N = 512, 5
    W = np.tile(R.make_q3k(np.zeros((1, 16)), np.full((1, 256), -4), [1.0])[0], (N, 2))
    rng = np.random.default_rng(3)
    for M in (1, 8, 9, 33, 130):
        q = rng.integers(-126, 127, (M, K))
        q[:, 0] = 127
        q[:, 256] = 127  # amax = 127 in both super-blocks: d_act = 1, the quants are the values
        X = q.astype(np.float32)
        got = T.run_case(lambda g: R.g_mul_mat(g, L.Q3_K, W, X, K, N, M), backend)[0].reshape(M, N)
        want = np.repeat((128.0 * q.sum(axis=1))[:, None], N, axis=1).astype(np.float32)
        assert np.array_equal(got, want), (M, got[0], want[0])


# ---------------------------------------------------------------------------------------------- column invariance
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_multi_column_matvec_equals_single_columns(backend, qt):
    K, N = 768, 37
    rng = np.random.default_rng(31 + qt)
    W = R.rand_weight(qt, K, N, rng)
    Xall = rng.standard_normal((8, K)).astype(np.float32)
    ones = [T.run_case(lambda g: R.g_mul_mat(g, qt, W, Xall[c:c + 1], K, N, 1), backend)[0].reshape(N) for c in range(8)]
    for M in range(2, 9):
        got = T.run_case(lambda g: R.g_mul_mat(g, qt, W, Xall[:M], K, N, M), backend)[0].reshape(M, N)
        for c in range(M):
            assert np.array_equal(got[c].view(np.uint32), ones[c].view(np.uint32)), (M, c)


# ---------------------------------------------------------------------------------------------- GET_ROWS
@pytest.mark.parametrize("nblk", [1, 2, 17], ids=lambda n: f"blocks{n}")
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_get_rows_bit_equal(backend, qt, nblk):
    K, N = 256 * nblk, 9
    rng = np.random.default_rng(9 + qt)
    W = np.concatenate([R.rand_weight(qt, K, N - 2, rng), R.edge_blocks(qt, 2 * nblk, rng).reshape(2, -1)])
    idx = np.array([8, 0, 3, 3, 2, 8, 7, 1], dtype=np.int32)  # repeated and out of order

    def build(g):
        return g.H.ggml_get_rows(g.ctx, g.new(qt, [K, N], W), g.new(L.I32, [len(idx)], idx))

    got = T.run_case(build, backend)[0].reshape(len(idx), K)
    want = R.dequantize(qt, W, K)[idx]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- MUL_MAT over a view at the minimum alignment
@pytest.mark.parametrize("M", [1, 3, 9, 160], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_over_a_view_one_block_into_its_parent(backend, plog, qt, M):
    K, N = 512, 33
    rng = np.random.default_rng(500 * qt + M)
    W = R.rand_weight(qt, K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bs = L.TYPE_SIZE[qt]
    g = T.G(backend)
    try:
        out = R.g_mul_mat_offset_view(g, qt, W, X, K, N, M)
        got = MR.compute_in_weights_buffer(g, [out])[0].reshape(M, N)
        w = out.contents.src[0].contents
        assert w.view_offs == bs and w.data % ALIGN[qt] == 0 and w.data % 16 == bs % 16, (w.view_offs, hex(w.data))
    finally:
        g.free()
    e = T.nmse(got, R.mul_mat(qt, W, X))
    plog(f"kq23 mul_mat over an offset view {L.TYPE_NAME[qt]} M={M} base % 16 = {bs % 16} nmse={e:.3e}")
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- MUL_MAT_ID
@pytest.mark.parametrize("per_slot", [False, True], ids=["shared_row", "per_slot"])
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_id_matches_the_twin_and_the_backends_own_mat_vec(backend, plog, qt, per_slot):
    """Experts in both formats, n_tokens 1, 3, 16 (n_used * n_tokens <= 32) and 40: NMSE <= 1e-10 against the twin, and up to 32 pairs every (slot, token) result
    is bit-equal to the backend's own one-column MUL_MAT over that expert's 2-D view (the contract of DESIGN.md 4b)."""
    K, N, n_expert, n_used = 512, 70, 4, 2
    rng = np.random.default_rng(3000 + 13 * qt + per_slot)
    W = np.stack([R.rand_weight(qt, K, N, rng) for _ in range(n_expert)])
    cases = []
    for n_tok in (1, 3, 16, 40):
        ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
        cases.append((rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32), ids))
    H = L.host()
    g = T.G(backend)
    try:
        as_t = g.new(qt, [K, N, n_expert], W)
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
        T.compare(f"kq23 mul_mat_id {L.TYPE_NAME[qt]} n_tokens={n_tok}", got, R.mmid(qt, W, b, ids), GATE, log=plog)
        if n_used * n_tok <= 32:
            for t in range(n_tok):
                for s in range(n_used):
                    own = res[len(outs) + ci].reshape(N)
                    ci += 1
                    assert np.array_equal(got[t, s].view(np.uint32), own.view(np.uint32)), f"n_tokens={n_tok}: (slot {s}, token {t}) differs from MUL_MAT over the expert's view"
    assert ci == len(cols)


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_id_with_an_id_outside_the_experts_writes_zeros(backend, qt):
    K, N, n_expert, n_used, n_tok = 256, 70, 4, 2, 4
    rng = np.random.default_rng(40 + qt)
    H = L.host()
    W = np.stack([R.rand_weight(qt, K, N, rng) for _ in range(n_expert)])
    b = rng.standard_normal((n_tok, n_used, K)).astype(np.float32)
    good = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    bad = good.copy()
    bad[1, 0] = n_expert
    bad[2, 1] = -1

    def build(g):
        as_t = g.new(qt, [K, N, n_expert], W)
        bt = g.new(L.F32, [K, n_used, n_tok], b)
        return [H.ggml_mul_mat_id(g.ctx, as_t, bt, MR.strided_ids(g, i, n_expert)) for i in (good, bad)]

    rg, rb = [r.reshape(n_tok, n_used, N) for r in T.run_case(build, backend)]
    assert np.count_nonzero(rg) > rg.size // 2
    for t in range(n_tok):
        for s in range(n_used):
            want = np.zeros(N, dtype=np.float32) if (t, s) in ((1, 0), (2, 1)) else rg[t, s]
            assert np.array_equal(rb[t, s].view(np.uint32), want.view(np.uint32)), (t, s)


# ---------------------------------------------------------------------------------------------- one norm output, three formats
KINDS = (L.Q3_K, L.Q2_K, L.Q4_K)


def _mixed_layer(backend, order, Ws, nw, X, K, N, M):
    """cur = MUL(RMS_NORM(x), w) feeds a Q3_K, a Q2_K and a Q4_K matrix; the three MUL_MAT nodes enter the graph in `order`.  -> (cur, the products in KINDS order)"""
    H = L.host()
    g = T.G(backend)
    try:
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X, "x"), 1e-5), g.new(L.F32, [K], nw, "norm"))
        mm = {qt: H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt], L.TYPE_NAME.get(qt, "q4_K")), cur) for qt in order}
        return g.compute([mm[qt] for qt in KINDS], expand_first=[mm[qt] for qt in order])
    finally:
        g.free()


@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_q3_k_q2_k_and_q4_k_matrices_share_one_norm_output_in_every_node_order(backend, plog, M):
    """One norm output read by a Q3_K, a Q2_K and a Q4_K matrix — one Q8_K activation row serves all three (norm prologue, activation cache, or the quantise
    launch): every one of the six node orders gives the same bits, and those meet the gate against the twin (Q4_K: the oracle) over the oracle's norm output."""
    K, N = 512, 48
    rng = np.random.default_rng(70 + M)
    Ws = {L.Q3_K: R.rand_weight(L.Q3_K, K, N, rng), L.Q2_K: R.rand_weight(L.Q2_K, K, N, rng), L.Q4_K: T.rand_weight(L.Q4_K, K, N, rng)}
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    X = (rng.standard_normal((M, K)) + 0.3).astype(np.float32)
    H = L.host()

    def norm_and_q4(g):
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X), 1e-5), g.new(L.F32, [K], nw))
        return [cur, H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [K, N], Ws[L.Q4_K]), cur)]

    cur, ref4 = T.run_case(norm_and_q4, "oracle")
    ref = {L.Q3_K: R.mul_mat(L.Q3_K, Ws[L.Q3_K], cur.reshape(M, K)), L.Q2_K: R.mul_mat(L.Q2_K, Ws[L.Q2_K], cur.reshape(M, K)), L.Q4_K: ref4.reshape(M, N)}
    first = None
    for order in itertools.permutations(KINDS):
        got = _mixed_layer(backend, order, Ws, nw, X, K, N, M)
        if first is None:
            first = got
            for qt, a in zip(KINDS, got):
                e = T.nmse(a.reshape(M, N), ref[qt])
                plog(f"kq23 shared norm output M={M} type {qt}: nmse={e:.3e}")
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
def test_kq23_model_runs_whole_on_the_device(H, backend, plog, fa):
    """test-llama-kq23 (Q3_K embeddings, Q2_K output matrix, Q2_K / Q3_K / Q4_K / Q6_K layer matrices): a 40-token prompt batch, 16 batch-1 steps teacher-forced
    on the reference's tokens and a 4-sequence step against the hybrid (oracle + twin) reference, logits NMSE <= 1e-3 at each; every node accepted by the device."""
    hp = preset("test-llama-kq23")
    mg, mc = Model(hp, 1234, backend.buft), Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=fa), Context(mc, compute=R.hybrid_compute_fn(), flash_attn=fa)
    n_gen = 16
    try:
        assert H.llm_model_tensor(mg.m, b"token_embd.weight").contents.type == L.Q3_K and H.llm_model_tensor(mg.m, b"output.weight").contents.type == L.Q2_K
        t0 = backend.stat("tiled_launches")
        rc, ref = cc.decode(PROMPT40, range(40))
        rc2, got = cg.decode(PROMPT40, range(40))
        assert rc == 0 and rc2 == 0
        _accepted(H, backend, cg)
        assert backend.stat("tiled_launches") > t0
        e = T.nmse(got, ref)
        plog(f"test-llama-kq23 fa={fa} 40-token prompt logits: nmse={e:.3e}")
        assert e <= 1e-3
        cc.clear()
        cg.clear()
        ids_ref, rows_ref = greedy(cc, PROMPT40, n_gen)
        rows_ref = np.stack(rows_ref)
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
        plog(f"test-llama-kq23 fa={fa} teacher-forced decode x{n_gen}: nmse={e_dec:.3e} argmax agreement {int(agree.sum())}/{len(agree)}")
        assert e_dec <= 1e-3
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
        plog(f"test-llama-kq23 fa={fa} 4-sequence steps: nmse={e4:.3e}")
        assert e4 <= 1e-3
    finally:
        for o in (cg, cc, mg, mc):
            o.free()


def test_kq23_decode_step_runs_in_a_captured_graph_and_replays_bit_identical_to_eager(backend, H, plog):
    mg = Model(preset("test-llama-kq23"), 99, backend.buft)
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
    plog(f"test-llama-kq23: hipGraph launches with graphs=1: {outs[1][2]}, with graphs=0: {outs[0][2]}")
    assert outs[1][2] >= 10 and outs[0][2] == 0
    assert outs[1][0] == outs[0][0]
    assert np.array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))


FTYPES = {"q3_k_s": (14, L.Q3_K, "q3_K"), "q2_k": (13, L.Q2_K, "q2_K")}  # LLM_FTYPE_Q3_K_S, LLM_FTYPE_Q2_K (host/llama_lite.h)


@pytest.mark.parametrize("ft", sorted(FTYPES))
def test_single_format_model_runs_whole_on_the_device(H, backend, plog, ft):
    """test-llama's shape as a *-Q3_K_S.gguf / *-Q2_K.gguf holds it: gate and up share the base format in every layer, so the batch-1 step takes the SwiGLU form of
    the streaming mat-vec with the norm prologue (asserted by its timing class).  A 9-token prompt and 4 teacher-forced steps, logits NMSE <= 1e-3."""
    ftype, base, tag = FTYPES[ft]
    hp = preset("test-llama", ftype=ftype)
    mg, mc = Model(hp, 7, backend.buft), Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=1), Context(mc, compute=R.hybrid_compute_fn(), flash_attn=1)
    try:
        for n in (b"blk.0.ffn_gate.weight", b"blk.0.ffn_up.weight", b"token_embd.weight"):
            assert H.llm_model_tensor(mg.m, n).contents.type == base
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
        plog(f"test-llama in {ft}: prompt + 4 decode rows nmse={e:.3e}; mat-vec classes {[c for c in classes if c.startswith('mmvq_')]}")
        assert e <= 1e-3
        assert f"mmvq_{tag}_glu_normpro" in classes, classes
    finally:
        backend.set_option("timing", 0)
        for o in (cg, cc, mg, mc):
            o.free()
