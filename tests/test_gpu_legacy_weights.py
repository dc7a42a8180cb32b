"""GPU tests for weight matrices in Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL: acceptance, MUL_MAT on every kernel form (streaming mat-vec, 2 .. 8-column
mat-vec, the weight-streaming and the tiled matrix-core forms, the K % 128 != 0 fallback), value edges from sampled blocks, exact read-back of
the Q8_0 / Q8_1 activation quantisers, column invariance, GET_ROWS, MUL_MAT_ID, the activation cache's kind key and the legacy test models.  Every comparison is against the oracle through
harness.run_case; the gate is the project's own for quantised MUL_MAT, NMSE <= 1e-10 (tests/test_gpu_ops.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import harness as T
import legacy_ref as R
import llama_box_amd as L
import moe_ref as MR
import probes as P
from model_util import Context, Model, greedy, preset
from test_gpu_model import _oracle_yardstick  # (the yardstick of the greedy-id gate is the one test-llama is held to, not a copy of it)

pytestmark = pytest.mark.gpu
GATE = 1e-10
IDS = lambda q: L.TYPE_NAME[q] if isinstance(q, int) and q in L.TYPE_NAME else str(q)  # noqa: E731


def _both(build, backend):
    return T.run_case(build, backend)[0], T.run_case(build, "oracle")[0]


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
    assert _probe(H, backend, qt, 256, 64, 1) and _probe(H, backend, qt, 4096, 33, 40)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:  # K % 32 != 0 cannot be built as a tensor of whole blocks: a 2-D view whose row is 48 values of a 64-value parent stands for it
        w = H.ggml_new_tensor_2d(ctx, qt, 64, 8)
        x = H.ggml_new_tensor_2d(ctx, L.F32, 64, 1)
        mm = H.ggml_mul_mat(ctx, w, x)
        assert H.ggml_backend_dev_supports_op(backend.dev, mm)
        w.contents.ne[0] = 48
        x.contents.ne[0] = 48
        assert not H.ggml_backend_dev_supports_op(backend.dev, mm)
        # GET_ROWS takes the format as `a` (token_embd)
        e = H.ggml_new_tensor_2d(ctx, qt, 64, 8)
        i = H.ggml_new_tensor_1d(ctx, L.I32, 3)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, e, i))
    finally:
        H.ggml_free(ctx)


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_split_buffer_weight_stays_refused(H, backend, qt):
    addr = H.ggml_backend_reg_get_proc_address(backend.reg, b"ggml_backend_split_buffer_type")
    assert addr
    fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_float))(addr)
    split_buft = fn(0, (C.c_float * 16)(*([0.0] * 16)))
    assert split_buft
    # llama.cpp's weight_buft_supported: the probe tensor's buffer is a dummy buffer of the type under test
    buf = H.ggml_backend_buft_alloc_buffer(split_buft, 0)
    assert buf
    try:
        assert not _probe(H, backend, qt, 256, 64, 1, buffer=buf)
        assert _probe(H, backend, L.Q8_0, 256, 64, 1, buffer=buf)  # (what the split buffer serves today is unchanged)
    finally:
        H.ggml_backend_buffer_free(buf)


# ---------------------------------------------------------------------------------------------- MUL_MAT
# (K, N, M): a cross-section of K {32, 96, 128, 160, 4096, 4128} x N {1, 3, 33, 130, 257} x M {1, 2, 3, 8, 9, 31, 32, 33, 128, 160}; every kernel form at
# its smallest and at a ragged shape: streaming mat-vec (M 1), k_mmvq<T, 2 / 4 / 8> (M 2, 3, 8), the K % 128 != 0 fallback at 9+ columns (K 96, 160, 4128),
# the weight-streaming matrix-core form (M 9 .. 128, K % 128 == 0) and the tiled one (M 129 and more)
SHAPES = [(32, 1, 1), (96, 3, 2), (128, 33, 3), (160, 130, 8), (4096, 257, 1), (4128, 33, 1), (4096, 130, 8),
          (128, 1, 9), (128, 33, 31), (4096, 257, 32), (4096, 33, 33), (128, 130, 128), (128, 3, 160), (4096, 257, 160),
          (96, 33, 9), (160, 3, 33), (4128, 130, 160)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_n%d_m%d" % s)
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_matches_oracle(backend, plog, qt, shape):
    K, N, M = shape
    rng = np.random.default_rng(1000 * qt + K + N + M)
    W = R.rand_weight(qt, K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    if K > 32 or M > 1:  # one activation block all zero (never the only one: a product of nothing but zeros would pass whatever the kernel decodes)
        X[M // 2, 32 * ((K // 32) // 2):32 * ((K // 32) // 2) + 32] = 0.0
    got, ref = _both(lambda g: R.mul_mat(g, qt, W, X, K, N, M), backend)
    e = T.nmse(got, ref)
    plog(f"legacy mul_mat {L.TYPE_NAME[qt]} K={K} N={N} M={M} nmse={e:.3e}")
    assert np.any(ref != 0) and np.all(np.isfinite(got[np.isfinite(ref)]))
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- value edges
def _edge_weight(qt, K, N, rng):
    n5 = 31 if qt in R.FIVE else 15
    nb = K // 32
    d = np.array([1.0, -0.5, 6e-8, 0.0, 0.25, 2e-3, -1.5, 1.0], dtype=np.float16)     # negative d, an f16 subnormal, zero
    m = np.array([0.0, -3.0, 1.0, 2.0, 512.0, -0.125, 7.0, -64.0], dtype=np.float16)  # negative m, m large against d
    lev = np.stack([np.zeros(32), np.full(32, 15), np.full(32, n5), np.full(32, 16 if qt in R.FIVE else 0), np.arange(32) % (n5 + 1),
                    np.arange(32)[::-1] % (n5 + 1), np.full(32, n5), np.zeros(32)]).astype(np.int64)  # all nibbles 0 / 15, qh all ones
    pick = rng.integers(0, 8, N * nb)
    return R.make_blocks(qt, d[pick], m[pick], lev[pick]).reshape(N, nb * L.TYPE_SIZE[qt])


@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_value_edges(backend, qt, M):
    K, N = 256, 40
    rng = np.random.default_rng(77 + qt)
    W = _edge_weight(qt, K, N, rng)
    cat, names = P.edge_activations("q8_0", K, rng)  # the catalogue of tests/probes.py, its subnormal row included
    sub = [i for i, n in enumerate(names) if "subnormal" in n]
    assert sub and len(names) <= 33
    X = np.ascontiguousarray(cat[sub[:1]]) if M == 1 else P.tile_rows(np.roll(cat, -sub[0], axis=0), M)  # (the subnormal row leads: M = 4 holds it too)
    got, ref = _both(lambda g: R.mul_mat(g, qt, W, X, K, N, M), backend)
    assert np.all(np.isfinite(got[np.isfinite(ref)]))
    assert T.nmse(got, ref) <= GATE


# ---------------------------------------------------------------------------------------------- exact read-back of the quantisers
@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_q4_0_readout_returns_d_act_times_q_act(backend, M):
    """Row j of the matrix has d = 1 and level 9 (value +1) at column j, 8 (value 0) elsewhere: the product is d_act * q_act[j], bit for bit."""
    K = 64
    rng = np.random.default_rng(5)
    lev = np.full((K, K // 32, 32), 8)
    for j in range(K):
        lev[j, j // 32, j % 32] = 9
    W = R.make_blocks(L.Q4_0, np.ones(K * (K // 32)), None, lev.reshape(-1, 32)).reshape(K, -1)
    X = (rng.standard_normal((M, K)) * rng.uniform(0.01, 30.0, (M, 1))).astype(np.float32)
    got = T.run_case(lambda g: R.mul_mat(g, L.Q4_0, W, X, K, K, M), backend)[0].reshape(M, K)
    q, d, _ = R.quantize_act(X, False)
    want = (q.astype(np.float32) * d[:, None]).astype(np.float32).reshape(M, K)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_q4_1_readout_returns_block_q8_1_s(backend, M):
    """Row r has d = 0 everywhere and m = 1 in block r only: the product is block_q8_1.s of activation block r = f16(sum(q) * d) with the UNROUNDED
    d = amax / 127 — a quantiser that builds s from the stored, f16-rounded d fails here."""
    K, nb = 128, 4
    rng = np.random.default_rng(6)
    m = np.zeros((nb, nb))
    m[np.arange(nb), np.arange(nb)] = 1.0
    W = R.make_blocks(L.Q4_1, np.zeros(nb * nb), m.reshape(-1), rng.integers(0, 16, (nb * nb, 32))).reshape(nb, -1)
    X = (rng.standard_normal((M, K)) * rng.uniform(0.01, 30.0, (M, 1)) + 0.3).astype(np.float32)
    got = T.run_case(lambda g: R.mul_mat(g, L.Q4_1, W, X, K, nb, M), backend)[0].reshape(M, nb)
    _, d, s = R.quantize_act(X, True)
    q, _, _ = R.quantize_act(X, True)
    rounded = (q.sum(axis=1).astype(np.float32) * d).astype(np.float16).astype(np.float32)
    assert not np.array_equal(rounded, s), "the inputs must tell the unrounded d from the rounded one"
    assert np.array_equal(got.view(np.uint32), s.reshape(M, nb).view(np.uint32))


def double_rounding_blocks(n, rng):
    """n activation blocks whose f32 product sum(q) * d lies exactly on an f16 tie although the exact product does not: rounding the product once,
    straight to f16 (a fused multiply-convert), gives the other neighbour than quantize_row_q8_1_ref's two roundings."""
    found = []
    for _ in range(40):
        x = (rng.standard_normal((1 << 16, 32)) * rng.uniform(0.05, 20.0, (1 << 16, 1)) + 0.4).astype(np.float32)
        q, _, s = R.quantize_act(x, True)
        d = (np.max(np.abs(x), axis=1) / np.float32(127.0)).astype(np.float32)
        with np.errstate(over="ignore"):
            once = (q.sum(axis=1).astype(np.float64) * d.astype(np.float64)).astype(np.float16).astype(np.float32)
        found.extend(x[(once != s) & np.isfinite(s)])
        if len(found) >= n:
            return np.stack(found[:n])
    raise AssertionError("no double-rounding blocks found")


_DR = []


def _dr_blocks():  # searched once, shared by the cases below
    if not _DR:
        _DR.append(double_rounding_blocks(33 * 4, np.random.default_rng(88)))
    return _DR[0]


@pytest.mark.parametrize("M", [1, 5, 33], ids=lambda m: f"m{m}")
def test_q4_1_readout_where_one_rounding_differs_from_two(backend, M):
    """The read-out above on activation blocks chosen so that f16(f32(sum * d)) != f16(sum * d): s must be the reference's, rounded twice."""
    K, nb = 128, 4
    rng = np.random.default_rng(8)
    m = np.zeros((nb, nb))
    m[np.arange(nb), np.arange(nb)] = 1.0
    W = R.make_blocks(L.Q4_1, np.zeros(nb * nb), m.reshape(-1), rng.integers(0, 16, (nb * nb, 32))).reshape(nb, -1)
    X = _dr_blocks()[:M * nb].reshape(M, K)
    got = T.run_case(lambda g: R.mul_mat(g, L.Q4_1, W, X, K, nb, M), backend)[0].reshape(M, nb)
    ref = T.run_case(lambda g: R.mul_mat(g, L.Q4_1, W, X, K, nb, M), "oracle")[0].reshape(M, nb)
    _, _, s = R.quantize_act(X, True)
    assert np.array_equal(ref.view(np.uint32), s.reshape(M, nb).view(np.uint32))  # (the twin is the oracle's)
    assert np.array_equal(got.view(np.uint32), s.reshape(M, nb).view(np.uint32))


# ---------------------------------------------------------------------------------------------- column invariance
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_multi_column_matvec_equals_single_columns(backend, qt):
    K, N, M = 160, 37, 7  # 4 + 2 + 1 columns of the multi-column form
    rng = np.random.default_rng(31 + qt)
    W = R.rand_weight(qt, K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    got = T.run_case(lambda g: R.mul_mat(g, qt, W, X, K, N, M), backend)[0].reshape(M, N)
    for c in range(M):
        one = T.run_case(lambda g: R.mul_mat(g, qt, W, X[c:c + 1], K, N, 1), backend)[0].reshape(N)
        assert np.array_equal(got[c].view(np.uint32), one.view(np.uint32)), c


# ---------------------------------------------------------------------------------------------- GET_ROWS
@pytest.mark.parametrize("nblk", [1, 129], ids=lambda n: f"blocks{n}")
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_get_rows_bit_equal(backend, qt, nblk):
    K, N = 32 * nblk, 9
    rng = np.random.default_rng(9 + qt)
    W = R.rand_weight(qt, K, N, rng)
    idx = np.array([[8, 0, 3, 3], [2, 8, 0, 1]], dtype=np.int32)  # 2-D indices, repeated and out of order

    def build(g):
        a = g.new(qt, [K, N, 2], np.stack([W, W[::-1]]))
        i = g.new(L.I32, [4, 2], idx)
        return g.H.ggml_get_rows(g.ctx, a, i)

    got, ref = _both(build, backend)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------- acceptance: alignment, cache views
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_block_alignment_is_a_condition_of_acceptance(H, backend, qt):
    """Blocks are 18 / 22 bytes (2-byte aligned and no more) or 20 / 24 bytes (4-byte aligned): a row base below that is refused, at it accepted."""
    al = 4 if qt in R.ONE else 2
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, qt, 64, 8)
        mm = H.ggml_mul_mat(ctx, w, H.ggml_new_tensor_2d(ctx, L.F32, 64, 1))
        gr = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 3))
        for node in (mm, gr):
            for addr in (0x10000, 0x10000 + al, 0x10000 + 3 * al):
                w.contents.data = addr
                assert H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            for addr in (0x10001, 0x10000 + al // 2, 0x10000 + al + 1):
                w.contents.data = addr
                assert not H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
    finally:
        H.ggml_free(ctx)


def test_q4_0_cache_view_keeps_the_f16_image_route(H, backend, plog):
    """A view into a q4_0 K cache (2-D for one KV head, 3-D for two) is accepted as before and served through its f16 image (stat kv_image_nodes), within
    the 1e-3 that tests/test_gpu_kv_types.py holds that route to; the SAME 2-D view in a weights buffer is a weight matrix: no image, the integer-dot gate."""
    HD, nkv, NCTX, nq = 128, 40, 64, 3
    rng = np.random.default_rng(21)
    cache1, cache2 = R.rand_weight(L.Q4_0, HD, NCTX, rng), R.rand_weight(L.Q4_0, 2 * HD, NCTX, rng)
    q1, q2 = rng.standard_normal((nq, HD)).astype(np.float32), rng.standard_normal((2, nq, HD)).astype(np.float32)
    rb = (HD // 32) * L.TYPE_SIZE[L.Q4_0]

    def view2(g):
        k = H.ggml_view_2d(g.ctx, g.new(L.Q4_0, [HD, NCTX], cache1), HD, nkv, rb, 0)
        return H.ggml_mul_mat(g.ctx, k, g.new(L.F32, [HD, nq], q1))

    def view3(g):
        k = H.ggml_view_3d(g.ctx, g.new(L.Q4_0, [2 * HD, NCTX], cache2), HD, nkv, 2, 2 * rb, rb, 0)
        return H.ggml_mul_mat(g.ctx, k, g.new(L.F32, [HD, nq, 2], q2))

    for name, build in (("2-D", view2), ("3-D", view3)):
        img0 = backend.stat("kv_image_nodes")
        got, ref = _both(build, backend)
        e = T.nmse(got, ref)
        plog(f"q4_0 cache view {name}: image nodes {backend.stat('kv_image_nodes') - img0}, nmse={e:.3e}")
        assert backend.stat("kv_image_nodes") == img0 + 1, name
        assert e <= 1e-3
    g = T.G(backend)
    try:
        img0 = backend.stat("kv_image_nodes")
        got = MR.compute_in_weights_buffer(g, [view2(g)])[0]
        assert backend.stat("kv_image_nodes") == img0
    finally:
        g.free()
    assert T.nmse(got, T.run_case(view2, "oracle")[0]) <= GATE


# ---------------------------------------------------------------------------------------------- MUL_MAT at the minimum alignment
# every kernel form over the view: streaming mat-vec, 2 / 4-column mat-vec, the fallback (K % 128 != 0, 9+ columns), the weight-streaming and the tiled matrix-core forms
VIEW_SHAPES = [(128, 33, 1), (96, 5, 3), (96, 5, 9), (128, 33, 9), (128, 33, 160)]


@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=lambda s: "k%d_n%d_m%d" % s)
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_over_a_view_one_block_into_its_parent(backend, plog, qt, shape):
    """The weight is a 2-D view ONE BLOCK (18 / 20 / 22 / 24 bytes) into its parent, in a weights buffer: its row base has the minimum alignment supports_op
    admits (an 18- or 22-byte offset leaves 2 bytes and no more), and it is served by the block kernels, not through an f16 image."""
    K, N, M = shape
    rng = np.random.default_rng(500 * qt + K + N + M)
    W = R.rand_weight(qt, K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bs = L.TYPE_SIZE[qt]
    ref = T.run_case(lambda g: R.mul_mat_offset_view(g, qt, W, X, K, N, M), "oracle")[0]
    g = T.G(backend)
    try:
        out = R.mul_mat_offset_view(g, qt, W, X, K, N, M)
        img0 = backend.stat("kv_image_nodes")
        got = MR.compute_in_weights_buffer(g, [out])[0]
        w = out.contents.src[0].contents
        assert w.view_offs == bs and w.data % (4 if qt in R.ONE else 2) == 0 and w.data % 16 == bs % 16, (w.view_offs, hex(w.data))
        assert backend.stat("kv_image_nodes") == img0
    finally:
        g.free()
    e = T.nmse(got, ref)
    plog(f"legacy mul_mat over an offset view {L.TYPE_NAME[qt]} K={K} N={N} M={M} base % 16 = {bs % 16} nmse={e:.3e}")
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- MUL_MAT_ID
@pytest.mark.parametrize("K,N,per_slot", [(256, 70, False), (96, 5, True)], ids=["k256_n70", "k96_n5_per_slot"])
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_mul_mat_id_matches_the_reference_and_the_backends_own_mat_vec(backend, plog, qt, K, N, per_slot):
    """Experts in each format, n_tokens 1, 3, 16 (n_used * n_tokens <= 32) and 40: NMSE <= 1e-10 against the composite oracle reference of tests/moe_ref.py, and up
    to 32 pairs every (slot, token) result is bit-equal to the backend's own one-column MUL_MAT over that expert's 2-D view (the contract of DESIGN.md 4b)."""
    n_expert, n_used = 4, 2
    rng = np.random.default_rng(3000 + 13 * qt + K)
    W = np.stack([R.rand_weight(qt, K, N, rng) for _ in range(n_expert)])
    cases = []
    for n_tok in (1, 3, 16, 40):
        ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
        cases.append((rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32), ids))
    ref = MR.mmid_reference(qt, W, K, N, cases)
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
        T.compare(f"mul_mat_id {L.TYPE_NAME[qt]} K={K} N={N} n_tokens={n_tok}", got, ref[k], 1e-10, log=plog)
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


# ---------------------------------------------------------------------------------------------- the activation cache's kind key
KINDS = (L.Q4_0, L.Q4_1, L.Q8_0)


def _mixed_layer(target, order, Ws, nw, X, K, N, M):
    """cur = MUL(RMS_NORM(x), w) feeds a Q4_0, a Q4_1 and a Q8_0 matrix; the three MUL_MAT nodes enter the graph in `order`.  -> the products in KINDS order"""
    H = L.host()
    g = T.G(target)
    try:
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X, "x"), 1e-5), g.new(L.F32, [K], nw, "norm"))
        mm = {qt: H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt], L.TYPE_NAME[qt]), cur) for qt in order}
        return g.compute([mm[qt] for qt in KINDS], expand_first=[mm[qt] for qt in order])
    finally:
        g.free()


@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_q4_0_q4_1_and_q8_0_matrices_share_one_norm_output_in_every_node_order(backend, plog, M):
    """One norm output read by a Q4_0, a Q4_1 and a Q8_0 matrix: same data pointer, same byte count — only the kind of the activation cache's key tells the Q8_1
    row the Q4_1 matrix needs from the Q8_0 row the other two share.  Every one of the six node orders gives the same bits, and those meet the oracle gate."""
    K, N = 256, 48
    rng = np.random.default_rng(70 + M)
    Ws = {L.Q4_0: R.rand_weight(L.Q4_0, K, N, rng), L.Q4_1: R.rand_weight(L.Q4_1, K, N, rng), L.Q8_0: T.rand_weight(L.Q8_0, K, N, rng)}
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    X = (rng.standard_normal((M, K)) + 0.3).astype(np.float32)
    ref = _mixed_layer("oracle", KINDS, Ws, nw, X, K, N, M)
    first = None
    for order in itertools.permutations(KINDS):
        got = _mixed_layer(backend, order, Ws, nw, X, K, N, M)
        if first is None:
            first = got
            for qt, a, b in zip(KINDS, got, ref):
                e = T.nmse(a, b)
                plog(f"mixed kinds M={M} {L.TYPE_NAME[qt]}: nmse={e:.3e}")
                assert e <= GATE, (L.TYPE_NAME[qt], e)
        for qt, a, b in zip(KINDS, got, first):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (L.TYPE_NAME[qt], [L.TYPE_NAME[o] for o in order])


# ---------------------------------------------------------------------------------------------- model level
PROMPT40 = [(7 * i + 3) % 512 for i in range(40)]


def _accepted(H, backend, ctx):
    gf = H.llm_last_graph(ctx.c)
    for i in range(gf.contents.n_nodes):
        assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i]), gf.contents.nodes[i].contents.name


@pytest.mark.parametrize("fa", [0, 1], ids=["nofa", "fa"])
@pytest.mark.parametrize("name", ["test-llama-legacy", "test-qwen2-legacy"])
def test_legacy_model_runs_whole_on_the_device(H, backend, plog, name, fa):
    """A 40-token prompt batch, batch-1 greedy decode teacher-forced on the oracle's tokens and a 4-sequence step, under the gates tests/test_gpu_model.py holds
    test-llama to: logits NMSE <= 1e-3 at every step kind and, on the soft-max path, greedy ids equal to the oracle's wherever the top-2 margin exceeds twice the
    oracle's own sensitivity to one-ulp changes of its arithmetic.  Every node of every graph is accepted by the device."""
    hp = preset(name)
    assert max(PROMPT40) < hp.n_vocab
    mg, mc = Model(hp, 1234, backend.buft), Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=fa), Context(mc, compute=T.oracle_compute_fn(), flash_attn=fa)
    n_gen = 16
    try:
        rc, ref = cc.decode(PROMPT40, range(40))
        rc2, got = cg.decode(PROMPT40, range(40))
        assert rc == 0 and rc2 == 0
        _accepted(H, backend, cg)
        e = T.nmse(got, ref)
        plog(f"{name} fa={fa} 40-token prompt logits: nmse={e:.3e}")
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
        top2 = np.sort(rows_ref, axis=1)
        margins = top2[:, -1] - top2[:, -2]
        agree = np.argmax(rows_got, axis=1) == np.array(ids_ref)
        plog(f"{name} fa={fa} teacher-forced decode x{n_gen}: nmse={e_dec:.3e} argmax agreement {int(agree.sum())}/{len(agree)} min margin {margins.min():.3e}")
        assert e_dec <= 1e-3
        if not fa:  # (as in tests/test_gpu_model.py: the yardstick is taken on the soft-max path)
            yard = 2.0 * _oracle_yardstick(H, name, PROMPT40, n_gen)
            decisive = margins > yard
            plog(f"{name}: oracle-vs-oracle yardstick {yard:.3e}; {int(decisive.sum())}/{len(margins)} decode positions decisive")
            assert bool(np.all(agree[decisive])), "greedy token differs where the margin exceeds the oracle's own order sensitivity"
        # a 4-sequence step
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
        assert T.nmse(out[0], out[1]) <= 1e-3
    finally:
        for o in (cg, cc, mg, mc):
            o.free()


@pytest.mark.parametrize("name", ["test-llama-legacy", "test-qwen2-legacy"])
def test_legacy_decode_step_runs_in_a_captured_graph_and_replays_bit_identical_to_eager(backend, H, plog, name):
    """The same greedy run with hipGraph capture on and off: with it the batch-1 steps are replays (stat graph_launches), without it none is, and ids and logits are
    the same bits — the streaming mat-vec launches of the five formats sit inside the captured decode graph."""
    mg = Model(preset(name), 99, backend.buft)
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
    plog(f"{name}: hipGraph launches with graphs=1: {outs[1][2]}, with graphs=0: {outs[0][2]}")
    assert outs[1][2] >= 10 and outs[0][2] == 0
    assert outs[1][0] == outs[0][0]
    assert np.array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))


FTYPES = {"q4_0": 6, "q4_1": 7, "q5_0": 8, "q5_1": 9, "iq4_nl": 10}  # LLM_FTYPE_Q4_0 .. LLM_FTYPE_IQ4_NL (host/llama_lite.h)


@pytest.mark.parametrize("ft", sorted(FTYPES))
def test_single_format_model_runs_whole_on_the_device(H, backend, plog, ft):
    """A model as llama.cpp writes a *-Q4_0.gguf ...: every layer matrix and token_embd in the base format, output.weight in Q6_K — gate and up share the format, so the
    batch-1 step takes the SwiGLU form of the streaming mat-vec in that format.  A 9-token prompt and 4 teacher-forced steps, logits NMSE <= 1e-3, every node accepted."""
    hp = preset("test-llama", ftype=FTYPES[ft])
    mg, mc = Model(hp, 7, backend.buft), Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=1), Context(mc, compute=T.oracle_compute_fn(), flash_attn=1)
    try:
        base = {v: k for k, v in L.TYPE_NAME.items()}[ft]
        assert H.llm_model_tensor(mg.m, b"blk.0.ffn_gate.weight").contents.type == base and H.llm_model_tensor(mg.m, b"token_embd.weight").contents.type == base
        ids_ref, rows_ref = greedy(cc, PROMPT40[:9], 5)
        rc, lg = cg.decode(PROMPT40[:9], range(9), want=[0] * 8 + [1])
        assert rc == 0
        _accepted(H, backend, cg)
        rows_got = [lg[-1]]
        for i, t in enumerate(ids_ref[:-1]):
            rc, l1 = cg.decode([t], [9 + i])
            assert rc == 0
            rows_got.append(l1[0])
        _accepted(H, backend, cg)
        e = T.nmse(np.stack(rows_got), np.stack(rows_ref))
        plog(f"test-llama in {ft}: prompt + 4 decode rows nmse={e:.3e}")
        assert e <= 1e-3
    finally:
        for o in (cg, cc, mg, mc):
            o.free()
