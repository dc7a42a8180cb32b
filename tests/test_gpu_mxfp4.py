"""GPU tests for the gpt-oss expert block: MXFP4 weight matrices (MUL_MAT, MUL_MAT_ID, GET_ROWS), ADD_ID on its own and in the MUL_MAT_ID store, SWIGLU_OAI, and the
block as a whole, eager and captured.  The reference is the NumPy twin of tests/mxfp4_ref.py (the oracle knows none of the three; tests/test_mxfp4_ref_host.py pins
the twin); the gate for products is the project's own for a quantised MUL_MAT: NMSE <= 1e-10."""
import ctypes as C
import struct

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as MR
import mxfp4_ref as R
import probes as P

pytestmark = pytest.mark.gpu
GATE = 1e-10
QT = L.MXFP4
BS = 17
f32 = np.float32


def _f32_param(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _probe(H, backend, K, N, M, buffer=None):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, QT, K, N)
        x = H.ggml_new_tensor_2d(ctx, L.F32, K, M)
        if buffer is not None:
            w.contents.buffer = buffer
        return bool(H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w, x)))
    finally:
        H.ggml_free(ctx)


# ---------------------------------------------------------------------------------------------- acceptance
def test_plain_2d_and_3d_expert_tensors_are_accepted(H, backend):
    """What llama.cpp's loader asks: plain tensors with a null buffer, for MUL_MAT, GET_ROWS and MUL_MAT_ID."""
    assert _probe(H, backend, 32, 3, 1) and _probe(H, backend, 2880, 33, 40)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        e = H.ggml_new_tensor_2d(ctx, QT, 96, 8)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, e, H.ggml_new_tensor_1d(ctx, L.I32, 3)))
        as_t = H.ggml_new_tensor_3d(ctx, QT, 2880, 16, 4)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 2880, 1, 5)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.I32, 2, 5)))
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, as_t, H.ggml_new_tensor_2d(ctx, L.I32, 3, 4)))
    finally:
        H.ggml_free(ctx)


def test_what_stays_refused(H, backend):
    """K % 32 != 0 (a view whose rows are 48 values of a 64-value parent stands for it) and a 3-D weight in MUL_MAT; a block at ANY byte address is accepted."""
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        w = H.ggml_new_tensor_2d(ctx, QT, 64, 8)
        x = H.ggml_new_tensor_2d(ctx, L.F32, 64, 1)
        mm = H.ggml_mul_mat(ctx, w, x)
        gr = H.ggml_get_rows(ctx, w, H.ggml_new_tensor_1d(ctx, L.I32, 3))
        as_t = H.ggml_new_tensor_3d(ctx, QT, 64, 8, 4)
        b3 = H.ggml_new_tensor_3d(ctx, L.F32, 64, 1, 5)
        mmid = H.ggml_mul_mat_id(ctx, as_t, b3, H.ggml_new_tensor_2d(ctx, L.I32, 2, 5))
        for node in (mm, gr):
            for addr in (0x10000, 0x10001, 0x10002, 0x10000 + BS):
                w.contents.data = addr
                assert H.ggml_backend_dev_supports_op(backend.dev, node), hex(addr)
            w.contents.data = None
        assert H.ggml_backend_dev_supports_op(backend.dev, mmid)
        w.contents.ne[0] = 48
        x.contents.ne[0] = 48
        as_t.contents.ne[0] = 48
        b3.contents.ne[0] = 48
        for node in (mm, gr, mmid):
            assert not H.ggml_backend_dev_supports_op(backend.dev, node)
        w3 = H.ggml_new_tensor_3d(ctx, QT, 64, 8, 2)
        assert not H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 64, 1, 2)))
        assert not H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 64, 3, 4)))
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
        assert not _probe(H, backend, 256, 64, 1, buffer=buf)
    finally:
        H.ggml_backend_buffer_free(buf)
    rp = H.ggml_backend_buft_alloc_buffer(backend.rowpar_buft(), 1 << 16)
    assert rp
    try:
        assert not _probe(H, backend, 256, 64, 1, buffer=rp)
        assert not _probe(H, backend, 256, 64, 40, buffer=rp)
    finally:
        H.ggml_backend_buffer_free(rp)


def test_add_id_is_accepted(H, backend):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        a = H.ggml_new_tensor_3d(ctx, L.F32, 2880, 4, 5)
        b = H.ggml_new_tensor_2d(ctx, L.F32, 2880, 32)
        ids = H.ggml_new_tensor_2d(ctx, L.I32, 4, 5)
        node = H.ggml_add_id(ctx, a, b, ids)
        assert H.ggml_op_name(node.contents.op) == b"ADD_ID"
        assert H.ggml_backend_dev_supports_op(backend.dev, node)
        ids.contents.type = L.F32
        assert not H.ggml_backend_dev_supports_op(backend.dev, node)
    finally:
        H.ggml_free(ctx)


def test_swiglu_oai_is_accepted_with_a_models_parameters_only(H, backend):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        a = H.ggml_new_tensor_3d(ctx, L.F32, 2880, 4, 5)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 2880, 4, 5)
        node = H.ggml_swiglu_oai(ctx, a, b, R.ALPHA, R.LIMIT)
        assert H.ggml_backend_dev_supports_op(backend.dev, node)
        for limit in (0.0, -1.0, float("inf"), float("nan")):
            node.contents.op_params[3] = _f32_param(limit)
            assert not H.ggml_backend_dev_supports_op(backend.dev, node), limit
        node.contents.op_params[3] = _f32_param(R.LIMIT)
        node.contents.op_params[2] = _f32_param(float("nan"))
        assert not H.ggml_backend_dev_supports_op(backend.dev, node)
    finally:
        H.ggml_free(ctx)


# ---------------------------------------------------------------------------------------------- MUL_MAT
# (K, N, M): (32, 3, 1) rows at odd addresses; (2880, 33, 1) 90 blocks, the second lane trip partial; M 9 and 33: passes of the mat-vec kernel
SHAPES = [(32, 3, 1), (96, 33, 2), (160, 130, 8), (2880, 33, 1), (4128, 5, 3), (128, 3, 9), (2880, 7, 33)]
_REF = {}


def _case(K, N, M):
    key = (K, N, M)
    if key not in _REF:
        rng = np.random.default_rng(39000 + K + N + M)
        W = R.rand_weight(K, N, rng)
        X = rng.standard_normal((M, K)).astype(f32)
        if K > 32:  # one activation block all zero (never the only one)
            X[M // 2, 32 * ((K // 32) // 2):32 * ((K // 32) // 2) + 32] = 0.0
        _REF[key] = (W, X, R.mul_mat(W, X))
    return _REF[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_n%d_m%d" % s)
def test_mul_mat_matches_the_twin(backend, plog, shape):
    K, N, M = shape
    W, X, ref = _case(K, N, M)
    k0, t0, s0, w0 = (backend.stat(k) for k in ("kernel_launches", "tiled_launches", "skinny_launches", "wide_launches"))
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    dk = backend.stat("kernel_launches") - k0
    e = T.nmse(got, ref)
    plog(f"mxfp4 mul_mat K={K} N={N} M={M} nmse={e:.3e} kernel_launches+{dk}")
    print(f"mxfp4 mul_mat K={K} N={N} M={M} nmse={e:.3e} kernel_launches+{dk}")
    assert np.any(ref != 0) and np.all(np.isfinite(got))
    assert e <= GATE, e
    # the form: the Q8_0 quantiser + passes of the mat-vec kernel over up to 8 columns each; never a matrix-core kernel
    assert (backend.stat("tiled_launches"), backend.stat("skinny_launches"), backend.stat("wide_launches")) == (t0, s0, w0)
    assert dk == 1 + (M + 7) // 8


@pytest.mark.parametrize("M", [1, 3, 9], ids=lambda m: f"m{m}")
def test_mul_mat_over_a_view_one_block_into_its_parent(backend, plog, M):
    K, N = 160, 33
    rng = np.random.default_rng(500 * QT + M)
    W = R.rand_weight(K, N, rng)
    X = rng.standard_normal((M, K)).astype(f32)
    g = T.G(backend)
    try:
        out = R.g_mul_mat_offset_view(g, W, X, K, N, M)
        got = MR.compute_in_weights_buffer(g, [out])[0].reshape(M, N)
        w = out.contents.src[0].contents
        assert w.view_offs == BS and w.data % 2 == 1, (w.view_offs, hex(w.data))
    finally:
        g.free()
    e = T.nmse(got, R.mul_mat(W, X))
    plog(f"mxfp4 mul_mat over an offset view M={M} nmse={e:.3e}")
    assert e <= GATE, e


def test_multi_column_matvec_equals_single_columns(backend):
    K, N = 2880, 37
    rng = np.random.default_rng(31 + QT)
    W = R.rand_weight(K, N, rng)
    Xall = rng.standard_normal((9, K)).astype(f32)
    ones = [T.run_case(lambda g: R.g_mul_mat(g, W, Xall[c:c + 1], K, N, 1), backend)[0].reshape(N) for c in range(9)]
    for M in (2, 3, 4, 5, 8, 9):
        got = T.run_case(lambda g: R.g_mul_mat(g, W, Xall[:M], K, N, M), backend)[0].reshape(M, N)
        for c in range(M):
            assert np.array_equal(got[c].view(np.uint32), ones[c].view(np.uint32)), (M, c)


# ---------------------------------------------------------------------------------------------- the dense fusions a quantised 2-D matrix takes
def _fusion_on_off(backend, build):
    """-> {mode: (outputs, launches, fused nodes)} of the same graph with option fusion 1 and 0"""
    res = {}
    try:
        for mode in (1, 0):
            backend.set_option("fusion", mode)
            s0 = {k: backend.stat(k) for k in ("kernel_launches", "fused_nodes")}
            outs = T.run_case(build, backend)
            res[mode] = (outs, backend.stat("kernel_launches") - s0["kernel_launches"], backend.stat("fused_nodes") - s0["fused_nodes"])
    finally:
        backend.set_option("fusion", 1)
    return res


@pytest.mark.parametrize("M", [1, 2], ids=lambda m: f"m{m}")  # (option mmvq_max_cols, default 2: the widest batch that takes the mat-vec fusions)
def test_gate_up_swiglu_over_mxfp4_is_one_launch_and_bit_equal_to_the_separate_nodes(backend, plog, M):
    """MUL_MAT(gate) MUL_MAT(up) SWIGLU over two MXFP4 matrices: the two-matrix form of the mat-vec kernel (the streaming kernel at one column, k_mmvq<T, 2> at two)"""
    K, N = 2880, 70
    rng = np.random.default_rng(1530 + M)
    Wg, Wu = R.rand_weight(K, N, rng), R.rand_weight(K, N, rng)
    X = rng.standard_normal((M, K)).astype(f32)
    H = L.host()

    def glu(g):
        x = g.new(L.F32, [K, M], X)
        gate, up = (H.ggml_mul_mat(g.ctx, g.new(QT, [K, N], W), x) for W in (Wg, Wu))
        return H.ggml_swiglu_split(g.ctx, gate, up)

    res = _fusion_on_off(backend, glu)
    (on, k_on, f_on), (off, k_off, f_off) = res[1], res[0]
    plog(f"mxfp4 gate / up / SwiGLU M={M}: fusion on +{k_on} launches, off +{k_off}")
    assert (k_on, f_on) == (2, 2) and (k_off, f_off) == (4, 0)  # the quantiser + one launch, against the quantiser + two products + SwiGLU
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    rg, ru = R.mul_mat(Wg, X).astype(np.float64), R.mul_mat(Wu, X).astype(np.float64)
    e = T.nmse(on[0].reshape(M, N), rg / (1.0 + np.exp(-rg)) * ru)
    assert e <= GATE, e


@pytest.mark.parametrize("M", [1, 2], ids=lambda m: f"m{m}")
def test_mul_mat_add_add_over_mxfp4_rides_in_the_store_and_is_bit_equal_to_the_separate_nodes(backend, plog, M):
    """MUL_MAT -> ADD(bias row) -> ADD(residual) over an MXFP4 matrix: both addends in the mat-vec kernel's store"""
    K, N = 2880, 70
    rng = np.random.default_rng(1700 + M)
    W = R.rand_weight(K, N, rng)
    X = rng.standard_normal((M, K)).astype(f32)
    bias, resid = rng.standard_normal(N).astype(f32), rng.standard_normal((M, N)).astype(f32)
    H = L.host()

    def chain(g):
        mm = R.g_mul_mat(g, W, X, K, N, M)
        return H.ggml_add(g.ctx, H.ggml_add(g.ctx, mm, g.new(L.F32, [N], bias)), g.new(L.F32, [N, M], resid))

    res = _fusion_on_off(backend, chain)
    (on, k_on, f_on), (off, k_off, f_off) = res[1], res[0]
    plog(f"mxfp4 mul_mat + add + add M={M}: fusion on +{k_on} launches, off +{k_off}")
    assert (k_on, f_on) == (2, 2) and (k_off, f_off) == (4, 0)
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    want = ((R.mul_mat(W, X) + bias[None, :]).astype(f32) + resid).astype(f32)
    assert T.nmse(on[0].reshape(M, N), want) <= GATE


# ---------------------------------------------------------------------------------------------- exact integers
def _exact_case(K, N, M, seed):
    """Weights with e in {127, 128, 129} (scale 0.5, 1, 2) — row 0: code 7 (12) in every position, row 1: code 15 (-12), the rest sampled over every code — and
    activations dy * q with dy a power of two, q one anchor of magnitude 127 per block and otherwise -1, 0, 1: every product, partial sum and scaled sum is an
    integer multiple of 0.5 * dy below 2^24 of them, so float32 holds the result exactly whatever the order of additions."""
    rng = np.random.default_rng(seed)
    nb = K // 32
    nib = rng.integers(0, 16, (N, nb, 32))
    nib[0], nib[1] = 7, 15
    e = rng.integers(127, 130, (N, nb))
    W = R.make_blocks(e.reshape(-1), nib.reshape(-1, 32)).reshape(N, nb * BS)
    q = rng.integers(-1, 2, (M, nb, 32))
    q[np.arange(M)[:, None], np.arange(nb)[None, :], rng.integers(0, 32, (M, nb))] = rng.choice([-127, 127], (M, nb))
    dy = np.exp2(rng.integers(-4, 3, (M, 1, 1)))
    return W, (q * dy).reshape(M, K).astype(f32)


@pytest.mark.parametrize("M", [1, 4, 9], ids=lambda m: f"m{m}")
def test_integer_products_are_exact(backend, M):
    K, N = 2880, 19
    W, X = _exact_case(K, N, M, 1200 + M)
    y = R.quantize_q80(X)
    a = np.abs(y["qs"].astype(np.int32))
    assert np.all((a == 127).sum(axis=2) == 1) and np.all((a <= 1) | (a == 127))  # one anchor a block, otherwise -1, 0, 1
    dq = y["d"].astype(f32)
    assert np.all(np.exp2(np.round(np.log2(dq))) == dq)  # powers of two
    u = R.unpack(W, K)
    bound = np.einsum("mrb,rb->mr", np.abs(R.block_sums(u, y)), u["scale"].astype(np.float64) / 0.5)  # in units of 0.5 * dy: bounds every order of additions
    assert float(bound.max()) < 2.0 ** 24, float(bound.max())
    ref = R.mul_mat(W, X)
    assert np.array_equal(ref.astype(np.float64), R.dequantize_q80(y) @ R.dequantize(W, K).astype(np.float64).T)  # (the twin itself is exact here)
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("M", [1, 5, 19], ids=lambda m: f"m{m}")
def test_readout_returns_the_q8_0_quantiser_exactly(backend, M):
    """Row j has e = 128 (scale 1) and code 2 (table value 2) at column j, code 0 elsewhere: output (m, j) = 2 * d_act * q_act[j], one non-zero term — the
    activation quantiser read back through the MXFP4 kernels, against the NumPy twin of quantize_row_q8_0 over the edge catalogue of tests/probes.py."""
    K = 96
    nib = np.zeros((K, K // 32, 32), dtype=np.uint8)
    for j in range(K):
        nib[j, j // 32, j % 32] = 2
    W = R.make_blocks(np.full(K * (K // 32), 128), nib.reshape(-1, 32)).reshape(K, (K // 32) * BS)
    assert np.array_equal(R.dequantize(W, K), 2.0 * np.eye(K, dtype=f32))
    cat, _ = P.edge_activations("q8_0", K, np.random.default_rng(96))
    X = P.tile_rows(cat, M)
    with np.errstate(all="ignore"):
        want = (f32(2.0) * P.expected_readout("q8_0", X)).astype(f32)
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, K, M), backend)[0].reshape(M, K)
    bad = np.argwhere(P.bits(got) != P.bits(want))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------- value edges
@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_value_edges(backend, plog, M):
    """Every e of the catalogue (both subnormal scales, 2^-126, 2^-125, around 1, 2^122) x codes all 0 / 7 / 15 / 8 and ramps, one e a row, against the activation
    catalogue of tests/probes.py: finite wherever the twin is finite, and the gate over those elements."""
    K = 96
    cat = np.concatenate([R.make_blocks(np.full(6, e), np.stack([np.zeros(32), np.full(32, 7), np.full(32, 15), np.full(32, 8), np.arange(32) % 16, 15 - np.arange(32) % 16]))
                          for e in R.EDGE_E])
    rng = np.random.default_rng(77 + QT + M)
    per_e = len(cat) // len(R.EDGE_E)
    rows = []
    for ei in range(len(R.EDGE_E)):  # eight rows an exponent: the six codes in three rotations, then two random mixtures of them
        for r in range(8):
            pick = [(r + b) % per_e for b in range(3)] if r < 6 else rng.integers(0, per_e, 3)
            rows.append(np.concatenate([cat[ei * per_e + p] for p in pick]))
    W = np.stack(rows)
    N = W.shape[0]
    acts, _ = P.edge_activations("q8_0", K, rng)
    X = P.tile_rows(acts, M)
    ref = R.mul_mat(W, X)
    got = T.run_case(lambda g: R.g_mul_mat(g, W, X, K, N, M), backend)[0].reshape(M, N)
    fin = np.isfinite(ref)
    assert fin.mean() > 0.8 and np.any(ref[fin] != 0)
    assert np.all(np.isfinite(got[fin])), np.argwhere(fin & ~np.isfinite(got))[:4].tolist()
    e = T.nmse(got[fin], ref[fin])
    plog(f"mxfp4 value edges M={M}: nmse={e:.3e} over {int(fin.sum())}/{fin.size} finite reference elements")
    print(f"mxfp4 value edges M={M}: nmse={e:.3e} over {int(fin.sum())}/{fin.size} finite reference elements")
    assert e <= GATE, e
    # per exponent, so that the small scales cannot hide behind the large ones
    for ei, ex in enumerate(R.EDGE_E):
        sl = slice(8 * ei, 8 * ei + 8)
        f = fin[:, sl]
        if np.any(ref[:, sl][f] != 0):
            ee = T.nmse(got[:, sl][f], ref[:, sl][f])
            assert ee <= GATE, (ex, ee)


# ---------------------------------------------------------------------------------------------- GET_ROWS
@pytest.mark.parametrize("nblk", [1, 2, 3, 17], ids=lambda n: f"blocks{n}")
def test_get_rows_bit_equal(backend, nblk):
    K, N = 32 * nblk, 9
    rng = np.random.default_rng(9 + QT)
    W = np.concatenate([R.rand_weight(K, N - 4, rng), R.edge_blocks(4 * nblk, rng).reshape(4, -1)])
    idx = np.array([8, 0, 3, 3, 2, 8, 7, 1, 6, 5], dtype=np.int32)  # repeated and out of order
    got = T.run_case(lambda g: R.g_get_rows(g, W, idx, K, N), backend)[0].reshape(len(idx), K)
    want = R.dequantize(W, K)[idx]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- MUL_MAT_ID
def _mmid_and_own_columns(backend, W, b, ids, K, N, own=True):
    """-> (MUL_MAT_ID result [n_tok, n_used, N], the backend's own one-column MUL_MAT per (token, slot) over the expert's 2-D view, mmid launches)"""
    H = L.host()
    n_expert, (n_tok, n_used), rows = W.shape[0], ids.shape, b.shape[1]
    g = T.G(backend)
    try:
        as_t = g.new(QT, [K, N, n_expert], W)
        bt = g.new(L.F32, [K, rows, n_tok], b)
        out = H.ggml_mul_mat_id(g.ctx, as_t, bt, MR.strided_ids(g, ids, max(n_expert, n_used)))
        cols = []
        if own:
            for t in range(n_tok):
                for s in range(n_used):
                    col = H.ggml_view_2d(g.ctx, bt, K, 1, K * 4, (t * rows + (s if rows > 1 else 0)) * K * 4)
                    cols.append(H.ggml_mul_mat(g.ctx, MR.expert_view(g, as_t, K, N, ids[t, s]), col))
        m0 = backend.stat("mmid_launches")
        res = MR.compute_in_weights_buffer(g, [out] + cols)
        return res[0].reshape(n_tok, n_used, N), [r.reshape(N) for r in res[1:]], backend.stat("mmid_launches") - m0
    finally:
        g.free()


@pytest.mark.parametrize("K", [160, 2880], ids=lambda k: f"k{k}")
@pytest.mark.parametrize("n_tokens", [1, 3, 8, 40], ids=lambda n: f"tokens{n}")
@pytest.mark.parametrize("per_slot", [False, True], ids=["shared_row", "per_slot"])
def test_mul_mat_id_matches_the_twin_and_the_backends_own_mat_vec(backend, plog, per_slot, n_tokens, K):
    N, n_expert, n_used = 33, 4, 2
    rng = np.random.default_rng(3000 + 13 * QT + per_slot + 100 * n_tokens + K)
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tokens)]).astype(np.int32)
    b = rng.standard_normal((n_tokens, n_used if per_slot else 1, K)).astype(f32)
    got, own, nl = _mmid_and_own_columns(backend, W, b, ids, K, N)
    assert nl == 1
    T.compare(f"mxfp4 mul_mat_id K={K} n_tokens={n_tokens} per_slot={per_slot}", got, R.mul_mat_id(W, b, ids), GATE, log=plog)
    ci = 0
    for t in range(n_tokens):
        for s in range(n_used):
            assert np.array_equal(got[t, s].view(np.uint32), own[ci].view(np.uint32)), f"(slot {s}, token {t}) differs from MUL_MAT over the expert's view"
            ci += 1


def test_mul_mat_id_two_rows_a_wave(backend, plog):
    """N * pairs >= 16384: the form in which a wave computes two rows (N = 512, 2 slots x 16 tokens); N odd by one so that the last wave's second row is clamped"""
    lim = MR.mmid_limits()
    K, N, n_expert, n_used, n_tok = 160, 513, 4, 2, 16
    assert N * n_used * n_tok >= lim["r2_min"] > 33 * 80
    rng = np.random.default_rng(512)
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    b = rng.standard_normal((n_tok, 1, K)).astype(f32)
    got, _, _ = _mmid_and_own_columns(backend, W, b, ids, K, N, own=False)
    T.compare("mxfp4 mul_mat_id two rows a wave", got, R.mul_mat_id(W, b, ids), GATE, log=plog)


def test_mul_mat_id_with_the_activation_row_past_the_lds_budget(backend, plog):
    """A K whose Q8_0 activation row no longer fits 64 KB of LDS: the form that reads the activations from global memory (N = 5, one pair)"""
    lim = MR.mmid_limits()
    K = (lim["lds_max"] // lim["act_bytes"]["q8_0"] + 1) * 32
    assert (K // 32) * lim["act_bytes"]["q8_0"] > lim["lds_max"] >= (K // 32 - 1) * lim["act_bytes"]["q8_0"]
    N, n_expert = 5, 3
    rng = np.random.default_rng(K)
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    ids = np.array([[2]], dtype=np.int32)
    b = rng.standard_normal((1, 1, K)).astype(f32)
    got, _, _ = _mmid_and_own_columns(backend, W, b, ids, K, N, own=False)
    T.compare(f"mxfp4 mul_mat_id K={K} (no LDS)", got, R.mul_mat_id(W, b, ids), GATE, log=plog)


def test_mul_mat_id_with_an_id_outside_the_experts_writes_zeros(backend):
    K, N, n_expert, n_used, n_tok = 160, 33, 4, 2, 4
    rng = np.random.default_rng(40 + QT)
    H = L.host()
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)])
    b = rng.standard_normal((n_tok, n_used, K)).astype(f32)
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
    for t in range(n_tok):
        for s in range(n_used):
            want = np.zeros(N, dtype=f32) if (t, s) in ((1, 0), (2, 1)) else rg[t, s]
            assert np.array_equal(rb[t, s].view(np.uint32), want.view(np.uint32)), (t, s)


# ---------------------------------------------------------------------------------------------- ADD_ID
@pytest.mark.parametrize("n_tok", [1, 5], ids=lambda n: f"tokens{n}")
@pytest.mark.parametrize("n_used", [1, 4], ids=lambda n: f"used{n}")
@pytest.mark.parametrize("n", [1, 33, 2880], ids=lambda n: f"n{n}")
def test_add_id_on_its_own_is_bit_equal(backend, n, n_used, n_tok):
    """ids as the strided view ggml_top_k hands out, `a` with a padded row stride (a view of rows three values longer), one id outside the experts"""
    n_expert, pad = 6, 3
    rng = np.random.default_rng(n + 10 * n_used + n_tok)
    a = rng.standard_normal((n_tok, n_used, n)).astype(f32)
    bias = rng.standard_normal((n_expert, n)).astype(f32)
    ids = rng.integers(0, n_expert, (n_tok, n_used)).astype(np.int32)
    if n_tok > 1:
        ids[n_tok - 1, 0] = n_expert + 2
    H = L.host()

    def build(g):
        wide = np.full((n_tok, n_used, n + pad), 1e30, dtype=f32)
        wide[:, :, :n] = a
        parent = g.new(L.F32, [n + pad, n_used, n_tok], wide)
        av = H.ggml_view_3d(g.ctx, parent, n, n_used, n_tok, (n + pad) * 4, (n + pad) * 4 * n_used, 0)
        dense = g.new(L.F32, [n, n_used, n_tok], a)
        bt = g.new(L.F32, [n, n_expert], bias)
        return [H.ggml_add_id(g.ctx, av, bt, MR.strided_ids(g, ids, n_expert + 1)), H.ggml_add_id(g.ctx, dense, bt, MR.strided_ids(g, ids, n_expert + 1))]

    k0 = backend.stat("kernel_launches")
    outs = T.run_case(build, backend)
    assert backend.stat("kernel_launches") - k0 == 2
    want = R.add_id(a, bias, ids)
    for o in outs:
        assert np.array_equal(o.reshape(n_tok, n_used, n).view(np.uint32), want.view(np.uint32))


def _expert_weights(qt, K, N, n_expert, rng):
    return np.stack([R.rand_weight(K, N, rng) for _ in range(n_expert)]) if qt == QT else MR.expert_weights(qt, K, N, n_expert, rng)


def _bias_graph(backend, qt, W, b, bias, ids, K, N, variant):
    """MUL_MAT_ID -> ADD_ID under mmid_bias 1 and 0 -> {mode: (result [n_tok, n_used, N], launches, fused nodes)}.  variant: "pair" (the fusible pair, twice, the
    second pair per slot), "second_reader" (a SCALE also reads the MUL_MAT_ID result), "other_ids" (the ADD_ID takes another ids tensor)"""
    H = L.host()
    n_expert, (n_tok, n_used) = W.shape[0], ids.shape
    other = (ids + 1) % n_expert
    res = {}
    try:
        for mode in (1, 0):
            backend.set_option("mmid_bias", mode)
            g = T.G(backend)
            try:
                as_t = g.new(qt, [K, N, n_expert], W)
                bt = g.new(L.F32, [K, 1, n_tok], b)
                bias_t = g.new(L.F32, [N, n_expert], bias)
                sel = MR.strided_ids(g, ids, n_expert)
                mm = H.ggml_mul_mat_id(g.ctx, as_t, bt, sel)
                outs = [H.ggml_add_id(g.ctx, mm, bias_t, MR.strided_ids(g, other, n_expert) if variant == "other_ids" else sel)]
                if variant == "second_reader":
                    outs.append(H.ggml_scale(g.ctx, mm, 2.0))
                if variant == "pair":
                    outs.append(H.ggml_add_id(g.ctx, H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, n_used, n_tok], np.repeat(b, n_used, axis=1) * f32(0.5)), sel), bias_t, sel))
                s0 = {k: backend.stat(k) for k in ("kernel_launches", "fused_nodes", "mmid_launches")}
                r = MR.compute_in_weights_buffer(g, outs)
                res[mode] = ([x.reshape(n_tok, n_used, N) for x in r], {k: backend.stat(k) - v for k, v in s0.items()})
            finally:
                g.free()
    finally:
        backend.set_option("mmid_bias", 1)
    return res, other


@pytest.mark.parametrize("qt", [L.MXFP4, L.F16], ids=["mxfp4", "f16"])
def test_add_id_rides_in_the_mul_mat_id_store(backend, plog, qt):
    K, N, n_expert, n_used, n_tok = 160, 33, 4, 2, 5
    rng = np.random.default_rng(160 + qt)
    W = _expert_weights(qt, K, N, n_expert, rng)
    b = rng.standard_normal((n_tok, 1, K)).astype(f32)
    bias = rng.standard_normal((n_expert, N)).astype(f32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    ids[3, 1] = n_expert  # (an id outside the experts: zeros from both forms)
    res, _ = _bias_graph(backend, qt, W, b, bias, ids, K, N, "pair")
    (on, s_on), (off, s_off) = res[1], res[0]
    plog(f"add_id in the store ({L.TYPE_NAME[qt]}): mmid_bias=1 {s_on}, mmid_bias=0 {s_off}")
    assert s_off["kernel_launches"] - s_on["kernel_launches"] == 2 and s_on["fused_nodes"] - s_off["fused_nodes"] == 2  # one a pair
    assert s_on["mmid_launches"] == s_off["mmid_launches"] == 2
    for x, y in zip(on, off):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not on[0][3, 1].any() and on[0][0].any()
    if qt == QT:
        for x, bb in zip(on, (b, np.repeat(b, n_used, axis=1) * f32(0.5))):
            want = R.add_id(R.mul_mat_id(W, bb, ids), bias, ids)
            assert T.nmse(x, want) <= GATE


@pytest.mark.parametrize("variant", ["second_reader", "other_ids"])
def test_add_id_stays_a_launch_of_its_own_when_the_store_cannot_take_it(backend, variant):
    K, N, n_expert, n_used, n_tok = 160, 33, 4, 2, 3
    rng = np.random.default_rng(len(variant))
    W = _expert_weights(QT, K, N, n_expert, rng)
    b = rng.standard_normal((n_tok, 1, K)).astype(f32)
    bias = rng.standard_normal((n_expert, N)).astype(f32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    res, other = _bias_graph(backend, QT, W, b, bias, ids, K, N, variant)
    (on, s_on), (off, s_off) = res[1], res[0]
    assert s_on == s_off, (s_on, s_off)
    for x, y in zip(on, off):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    mm = R.mul_mat_id(W, b, ids)
    assert T.nmse(on[0], R.add_id(mm, bias, other if variant == "other_ids" else ids)) <= GATE
    if variant == "second_reader":
        assert T.nmse(on[1], mm * f32(2.0)) <= GATE


# ---------------------------------------------------------------------------------------------- SWIGLU_OAI
def _oai_operands(rows, n, rng):
    """gate / up values around both clamps, with the clamps themselves, +-inf, large negative gates (expf overflows) and a NaN planted where the row is long enough"""
    g = (rng.standard_normal((rows, n)) * 5).astype(f32)
    u = (rng.standard_normal((rows, n)) * 6).astype(f32)
    plant_g = [7.0, 7.5, -7.0, 100.0, -60.0, -100.0, np.inf, -np.inf, np.nan, 1.0, 0.0, -0.0]
    plant_u = [8.0, -8.0, 7.0, -7.0, 0.5, 1.0, 2.0, 3.0, 1.0, np.nan, np.inf, -np.inf]
    for r in range(rows):
        k = min(n, len(plant_g))
        at = rng.permutation(n)[:k]
        g[r, at], u[r, at] = plant_g[:k], plant_u[:k]
    return g, u


def _same_bits_or_both_nan(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("n", [1, 33, 1024, 2880], ids=lambda n: f"n{n}")
def test_swiglu_oai_is_bit_equal_in_every_form(backend, n):
    H = L.host()
    rng = np.random.default_rng(1702 + n)
    n_used, n_tok = 2, 3
    rows = n_used * n_tok
    g_, u_ = _oai_operands(rows, n, rng)
    want = R.swiglu_oai(g_, u_, R.ALPHA, R.LIMIT)
    assert np.isnan(want).any() == (n >= 9) and np.isfinite(want).any()

    def one_tensor(g, halves, swapped):
        node = H.ggml_swiglu(g.ctx, g.new(L.F32, [2 * n, rows], np.concatenate(halves, axis=1)))
        node.contents.op_params[0] = 3  # GGML_GLU_OP_SWIGLU_OAI
        node.contents.op_params[1] = swapped
        node.contents.op_params[2], node.contents.op_params[3] = _f32_param(R.ALPHA), _f32_param(R.LIMIT)
        return node

    def build(g):
        return [H.ggml_swiglu_oai(g.ctx, g.new(L.F32, [n, rows], g_), g.new(L.F32, [n, rows], u_), R.ALPHA, R.LIMIT),                  # split, 2-D
                H.ggml_swiglu_oai(g.ctx, g.new(L.F32, [n, n_used, n_tok], g_), g.new(L.F32, [n, n_used, n_tok], u_), R.ALPHA, R.LIMIT),  # split, dense 3-D
                one_tensor(g, (g_, u_), 0), one_tensor(g, (u_, g_), 1)]

    k0 = backend.stat("kernel_launches")
    outs = T.run_case(build, backend)
    assert backend.stat("kernel_launches") - k0 == 4
    for form, o in zip(("split 2-D", "split 3-D", "one tensor", "swapped"), outs):
        assert _same_bits_or_both_nan(o.reshape(rows, n), want), form


def test_swiglu_oai_with_other_parameters(backend):
    H = L.host()
    rng = np.random.default_rng(5)
    g_, u_ = _oai_operands(4, 40, rng)
    for alpha, limit in ((1.0, 3.5), (-0.5, 100.0)):
        got = T.run_case(lambda g: H.ggml_swiglu_oai(g.ctx, g.new(L.F32, [40, 4], g_), g.new(L.F32, [40, 4], u_), alpha, limit), backend)[0].reshape(4, 40)
        assert _same_bits_or_both_nan(got, R.swiglu_oai(g_, u_, alpha, limit)), (alpha, limit)


# ---------------------------------------------------------------------------------------------- the gpt-oss expert block, whole
_BLK = {}


def _block():
    if "b" not in _BLK:
        _BLK["b"] = R.GptOssBlock(160, 96, 8, 2, seed=2880)
    return _BLK["b"]


@pytest.mark.parametrize("n_tok", [1, 5], ids=lambda n: f"tokens{n}")
def test_whole_expert_block_matches_the_composed_twin(backend, plog, n_tok):
    """Every node passes supports_op (the harness raises otherwise); the selected ids equal the twin's; the three ADD_IDs ride in their MUL_MAT_ID launches.
    Gate: the products' own, NMSE <= 1e-10 against the composed twin.  Every stage is bit-equal to its twin or within that gate, and the inputs are fixed, so the
    run is deterministic; the twin's distance from the block in float64 on de-quantised weights (what the 8-bit activations cost, ~1e-4) is printed, not used."""
    blk = _block()
    x = blk.router_inputs(n_tok, np.random.default_rng(100 + n_tok))
    ref, ids_ref = blk.reference(x)
    floor = T.nmse(ref, blk.numpy_f64(x, ids_ref))
    s0 = {k: backend.stat(k) for k in ("mmid_launches", "fused_nodes")}
    out, ids = T.run_case(lambda g: blk.build(g, x), backend)
    assert backend.stat("mmid_launches") - s0["mmid_launches"] == 3 and backend.stat("fused_nodes") - s0["fused_nodes"] >= 3
    e = T.nmse(out.reshape(ref.shape), ref)
    print(f"gpt-oss block n_tokens={n_tok}: twin vs f64 = {floor:.3e}, gate = {GATE:.1e}, gpu nmse = {e:.3e}")
    assert np.array_equal(ids.reshape(n_tok, blk.n_used), ids_ref)
    T.compare(f"gpt-oss block n_tokens={n_tok}", out.reshape(ref.shape), ref, GATE, log=plog)


def _stepper(backend, blk, xs):
    """One batch-1 graph of the block, computed once per row of xs with the input replaced in between; returns (outputs, ids) per step."""
    H = L.host()
    g = T.G(backend)
    try:
        out, ids = blk.build(g, xs[0][None, :])
        x_t = g.inputs[0][0]
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in (out, ids):
            H.ggml_set_output(o)
            H.ggml_build_forward_expand(gf, o)
        for i in range(gf.contents.n_nodes):
            assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i]), gf.contents.nodes[i].contents.name
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        res = []
        for x in xs:
            raw = np.ascontiguousarray(x, dtype=f32)
            H.ggml_backend_tensor_set(x_t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(out).copy(), g.read(ids).copy()))
        return res
    finally:
        g.free()


def test_a_decode_step_with_the_block_is_captured_and_replays_follow_the_routing(backend, plog):
    """The one-token graph computed three times with the router input changed in between: steps two and three launch the captured hipGraph although other experts
    are selected each time — MUL_MAT_ID and ADD_ID read the ids on the device — and every result is bit-equal to an eager run on the same inputs."""
    blk = _block()
    xs = blk.router_inputs(3, np.random.default_rng(77))
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures", "mmid_launches")}
            runs[mode] = (_stepper(backend, blk, xs), {k: backend.stat(k) - v for k, v in s0.items()})
    finally:
        backend.set_option("graphs", 1)
    plog(f"gpt-oss block capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["mmid_launches"] == 9, runs[0][1]
    sel = [tuple(sorted(r[1].ravel().tolist())) for r in runs[0][0]]
    assert len(set(sel)) == 3, f"the three steps were meant to select different experts: {sel}"
    for k, ((o1, i1), (o0, i0)) in enumerate(zip(runs[1][0], runs[0][0])):
        assert np.array_equal(i1, i0)
        assert np.array_equal(o1.view(np.uint32), o0.view(np.uint32)), k
        ref, ids_ref = blk.reference(xs[k][None, :])
        assert np.array_equal(i0.ravel(), ids_ref.ravel())
