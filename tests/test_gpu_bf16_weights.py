"""GPU tests for weight matrices kept in bf16: acceptance and what stays refused, MUL_MAT on every kernel form of csrc/mmbf.hip (the streaming
mat-vec, its multi-column form, 16 x 16 and 32 x 32 matrix-core tiles, the dot kernel's vector and scalar paths), bit-equal sums of one matrix stored as f16 and as bf16 on the kernels the two formats share, exact integer products, a read-back of the
activation rounding, weight value edges, GET_ROWS, MUL_MAT_ID, a norm output shared with quantised matrices, and the bf16 test models.

The reference is the CPU oracle (vec_dot_type(BF16) = BF16: activations rounded by fp32_to_bf16, products summed in double).  Gates are the project's own: NMSE <= 1e-11
for a 16-bit src0 (tests/test_gpu_ops.py::test_mul_mat_f — products of two bf16 values are exact in f32, only the f32 summation order differs), 1e-10 for a quantised
product, 1e-3 for a model's logits.  A kernel form is asserted through its timing class (option timing = 1)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bf16_ref as B
import harness as T
import llama_box_amd as L
import moe_ref as MR
from model_util import Context, Model, greedy, preset

pytestmark = pytest.mark.gpu
GATE = 1e-11
DOT, MMV, MMV_COLS, MMA16, MMA = 0, 1, 2, 3, 4  # MI_BF16_* of csrc/kernels.h (option bf16_form; -1 = routed)
CLASS_OF = {DOT: "mul_mat_bf16_dot", MMA16: "mul_mat_bf16_mma16", MMA: "mul_mat_bf16_mma"}


def _mmv_class(M):
    return "mmv_bf16_nc1" if M == 1 else "mmv_bf16_nc2" if M == 2 else "mmv_bf16_nc4" if M <= 4 else "mmv_bf16_nc8"


def _run_timed(backend, build, form=-1, weights_buffer=False):
    """-> (outputs, timing classes of the run) with the form option set for the run"""
    backend.set_option("bf16_form", form)
    backend.set_option("timing", 1)
    try:
        backend.timing_report()
        if weights_buffer:
            g = T.G(backend)
            try:
                outs = build(g)
                res = MR.compute_in_weights_buffer(g, list(outs) if isinstance(outs, (list, tuple)) else [outs])
            finally:
                g.free()
        else:
            res = T.run_case(build, backend)
        return res, sorted(backend.timing_report())
    finally:
        backend.set_option("timing", 0)
        backend.set_option("bf16_form", -1)


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
def test_plain_2d_bf16_weight_is_accepted(H, backend):
    """What llama.cpp's loader asks: a plain 2-D tensor with a null buffer, for MUL_MAT (any K), GET_ROWS and MUL_MAT_ID."""
    for K, N, M in ((256, 64, 1), (4096, 33, 40), (7, 5, 2)):
        assert _probe(H, backend, L.BF16, K, N, M), (K, N, M)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        e = H.ggml_new_tensor_2d(ctx, L.BF16, 512, 8)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_get_rows(ctx, e, H.ggml_new_tensor_1d(ctx, L.I32, 3)))
        as_t = H.ggml_new_tensor_3d(ctx, L.BF16, 256, 16, 4)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 5)
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.I32, 2, 5)))
    finally:
        H.ggml_free(ctx)


def test_view_in_a_weights_buffer_is_accepted_and_a_3d_weight_is_not(H, backend):
    """A 2-D view one row into a parent that lives in a WEIGHTS buffer is a weight; a 3-D bf16 tensor there is no MUL_MAT operand of this backend (unchanged)."""
    buf = H.ggml_backend_buft_alloc_buffer(backend.buft, 1 << 16)
    assert buf
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        H.ggml_backend_buffer_set_usage(buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
        base = H.ggml_backend_buffer_get_base(buf)
        parent = H.ggml_new_tensor_2d(ctx, L.BF16, 256, 9)
        parent.contents.buffer = buf
        parent.contents.data = base
        v = H.ggml_view_2d(ctx, parent, 256, 8, 512, 512)
        assert v.contents.data == base + 512
        assert H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, v, H.ggml_new_tensor_2d(ctx, L.F32, 256, 3)))
        w3 = H.ggml_new_tensor_3d(ctx, L.BF16, 256, 8, 2)
        w3.contents.buffer = buf
        w3.contents.data = base
        assert not H.ggml_backend_dev_supports_op(backend.dev, H.ggml_mul_mat(ctx, w3, H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 2)))
    finally:
        H.ggml_free(ctx)
        H.ggml_backend_buffer_free(buf)


def test_split_and_row_parallel_buffers_stay_refused(H, backend):
    addr = H.ggml_backend_reg_get_proc_address(backend.reg, b"ggml_backend_split_buffer_type")
    assert addr
    fn = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_float))(addr)
    split_buft = fn(0, (C.c_float * 16)(*([0.0] * 16)))
    assert split_buft
    buf = H.ggml_backend_buft_alloc_buffer(split_buft, 0)
    assert buf
    try:
        assert not _probe(H, backend, L.BF16, 256, 64, 1, buffer=buf)
        assert _probe(H, backend, L.Q8_0, 256, 64, 1, buffer=buf)  # (what the split buffer serves today is unchanged)
    finally:
        H.ggml_backend_buffer_free(buf)
    rp = H.ggml_backend_buft_alloc_buffer(backend.rowpar_buft(), 1 << 16)
    assert rp
    try:
        assert not _probe(H, backend, L.BF16, 256, 64, 1, buffer=rp)
        assert not _probe(H, backend, L.BF16, 256, 64, 40, buffer=rp)
    finally:
        H.ggml_backend_buffer_free(rp)


def test_bf16_k_cache_view_keeps_the_f16_image_route(H, backend, plog):
    """K.q over a bf16 cache view [128, n_kv, n_head_kv] outside a weights buffer: served through the f16 image as before (stat kv_image_nodes), not by the
    weight kernels."""
    HD, NKV, NH, nkv, nq = 128, 2, 4, 96, 3
    rng = np.random.default_rng(11)
    kf = B.to_bf16(rng.standard_normal((nkv, NKV * HD)).astype(np.float32))
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)

    def build(g):
        ks = g.new(L.BF16, [NKV * HD, nkv], kf)
        k = H.ggml_view_3d(g.ctx, ks, HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        return H.ggml_mul_mat(g.ctx, k, g.new(L.F32, [HD, nq, NH], q))

    ref = T.run_case(build, "oracle")[0]
    img0 = backend.stat("kv_image_nodes")
    (got,), classes = _run_timed(backend, build)
    assert backend.stat("kv_image_nodes") == img0 + 1
    assert "mul_mat_f_kv_image" in classes and not any("bf16" in c for c in classes), classes
    T.compare("bf16 K-cache view through its f16 image", got, ref, max_nmse=1e-3, log=plog)


# ---------------------------------------------------------------------------------------------- MUL_MAT: every form at its smallest and at a ragged shape
_REF = {}


def _case(K, N, M, seed=0):
    """weights, activations and the oracle's product for one shape: computed once, shared"""
    key = (K, N, M, seed)
    if key not in _REF:
        rng = np.random.default_rng(1000 * seed + K + 7 * N + 31 * M)
        W = B.rand_weight(K, N, rng)
        X = rng.standard_normal((M, K)).astype(np.float32)
        if K > 32:  # one activation block of 32 zeros in a middle column
            X[M // 2, 32 * ((K // 32) // 2):32 * ((K // 32) // 2) + 32] = 0.0
        ref = T.run_case(lambda g: B.g_mul_mat(g, W, X, K, N, M), "oracle")[0].reshape(M, N)
        _REF[key] = (W, X, ref)
    return _REF[key]


# (K, N, M) per form.  Streaming: K 8 = one lane's unit, 520 = one partial trip, 4104 = a partial second round; N 5 / 33 / 257: no multiple of the rows a workgroup owns.
# Tiles: K 136 and 2056 are 8 mod 16 (the second k-group of the last step is past the end).  5 columns route to the 16 x 16 tiles below 8192 rows (the measured
# hand-over), so (1032, 17, 5) stands as the issue lists it; the forms are forced per case, so that every shape runs on the form it is listed under.  (200, 17, 1) meets the vector conditions (K % 8 == 0, 400-byte rows), so the dot kernel serves it on
# its vector path, with half of its lanes past the row's end; (7, 5, 2) is the scalar path.
FORM_SHAPES = [
    (MMV, (8, 1, 1)), (MMV, (64, 3, 1)), (MMV, (520, 5, 1)), (MMV, (4096, 257, 1)), (MMV, (4104, 33, 1)),
    (MMV_COLS, (64, 3, 2)), (MMV_COLS, (520, 33, 3)), (MMV_COLS, (4096, 130, 8)), (MMV_COLS, (4104, 5, 5)),
    (MMA16, (128, 33, 9)), (MMA16, (4096, 16, 15)), (MMA16, (1032, 17, 5)), (MMA16, (1032, 17, 9)),
    (MMA, (128, 33, 16)), (MMA, (136, 65, 33)), (MMA, (2056, 130, 64)), (MMA, (4096, 257, 160)),
    (DOT, (7, 5, 2)), (DOT, (200, 17, 1)), (DOT, (4096, 33, 1)), (DOT, (520, 5, 3)),
]


@pytest.mark.parametrize("form,shape", FORM_SHAPES, ids=lambda v: "k%d_n%d_m%d" % v if isinstance(v, tuple) else ("dot", "mmv", "mmvcols", "mma16", "mma")[v])
def test_mul_mat_on_every_form(backend, plog, form, shape):
    K, N, M = shape
    W, X, ref = _case(K, N, M)
    k0 = backend.stat("kernel_launches")
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M), form)
    got = got.reshape(M, N)
    e = T.nmse(got, ref)
    plog(f"bf16 mul_mat K={K} N={N} M={M} form {form}: nmse={e:.3e} classes {classes} kernel_launches+{backend.stat('kernel_launches') - k0}")
    want = _mmv_class(M) if form in (MMV, MMV_COLS) else CLASS_OF[form]
    assert classes == [want], classes
    assert np.any(ref != 0) and np.all(np.isfinite(got))
    assert e <= GATE, e


@pytest.mark.parametrize("shape,want", [((4096, 64, 1), "mmv_bf16_nc1"), ((4096, 64, 2), "mmv_bf16_nc2"), ((4096, 64, 3), "mmv_bf16_nc4"), ((4096, 64, 4), "mmv_bf16_nc4"),
                                        ((4096, 64, 5), "mul_mat_bf16_mma16"), ((4096, 64, 8), "mul_mat_bf16_mma16"), ((4096, 8192, 5), "mmv_bf16_nc8"),
                                        ((4096, 8192, 8), "mmv_bf16_nc8"), ((14336, 8, 2), "mmv_bf16_nc2"), ((14336, 8, 3), "mul_mat_bf16_mma16"),
                                        ((8200, 8, 3), "mul_mat_bf16_mma16"), ((5120, 8192, 5), "mul_mat_bf16_mma16"), ((4096, 64, 9), "mul_mat_bf16_mma16"),
                                        ((4096, 64, 15), "mul_mat_bf16_mma16"), ((128, 64, 16), "mul_mat_bf16_mma"), ((4096, 64, 16), "mul_mat_bf16_mma16"), ((1024, 520, 33), "mul_mat_bf16_mma16"),
                                        ((1024, 8200, 64), "mul_mat_bf16_mma"),
                                        ((7, 5, 2), "mul_mat_bf16_dot"), ((204, 17, 1), "mul_mat_bf16_dot"), ((200, 17, 1), "mmv_bf16_nc1"), ((200, 17, 40), "mul_mat_bf16_mma")],
                         ids=lambda v: "k%d_n%d_m%d" % v if isinstance(v, tuple) else v)
def test_routing_table(backend, plog, shape, want):
    """The routed form (option bf16_form = -1) per batch width: DESIGN.md 4f's table — the streaming kernel up to 4 columns (up to 8 from 8192 rows on, and only
    while the 1 / 2 / 4 / 8 columns the kernel stages fit one launch's LDS — 3 columns at K = 8200 and 5 at K = 5120 do not), 16 x 16 tiles below 16 columns or below 512 32 x 32 tiles over rows of 1024 and more, 32 x 32 tiles beyond.  K = 7 and K = 204 (K % 8 != 0; 408-byte rows) take the dot kernel's scalar
    path; K = 200 is a multiple of 8 with 400-byte rows, which ARE 16-byte aligned: one column takes the streaming kernel, a batch of 40 the tiles."""
    K, N, M = shape
    W, X, ref = _case(K, N, M, seed=1)
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M))
    e = T.nmse(got.reshape(M, N), ref)
    plog(f"bf16 routing K={K} N={N} M={M}: {classes} nmse={e:.3e}")
    assert classes == [want], classes
    assert e <= GATE, e


@pytest.mark.parametrize("M", [1, 3, 9, 40], ids=lambda m: f"m{m}")
def test_scalar_path_over_a_view_one_element_into_its_parent(backend, plog, M):
    """Rows that start 2 bytes into a parent (a weights buffer): 2-byte aligned and no more — every batch width takes the dot kernel's scalar path."""
    K, N = 256, 9
    rng = np.random.default_rng(50 + M)
    W = B.rand_weight(K, N, rng)
    X = rng.standard_normal((M, K)).astype(np.float32)
    X[M // 2, 96:128] = 0.0
    ref = T.run_case(lambda g: B.g_mul_mat_offset_view(g, W, X, K, N, M), "oracle")[0].reshape(M, N)
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat_offset_view(g, W, X, K, N, M), weights_buffer=True)
    e = T.nmse(got.reshape(M, N), ref)
    plog(f"bf16 mul_mat over a view one element into its parent M={M}: nmse={e:.3e} {classes}")
    assert classes == ["mul_mat_bf16_dot"], classes
    assert e <= GATE, e


# ---------------------------------------------------------------------------------------------- batches with src1 rounded once into scratch
@pytest.mark.parametrize("shape", [(2056, 130, 64), (4096, 257, 160), (136, 65, 72)], ids=lambda s: "k%d_n%d_m%d" % s)
def test_tiles_over_prerounded_columns(backend, plog, shape):
    """Option bf16_preround (on by default): the 32 x 32 tile form reads src1 from a bf16 copy made by one launch ahead of it (64 columns and more).  The same arithmetic: the
    result equals the in-loop conversion's bit for bit, and meets the gate."""
    K, N, M = shape
    W, X, ref = _case(K, N, M)
    backend.set_option("bf16_preround", 0)
    try:
        (plain,), _ = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M), MMA)
    finally:
        backend.set_option("bf16_preround", 1)
    k0 = backend.stat("kernel_launches")
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M), MMA)
    dk = backend.stat("kernel_launches") - k0
    e = T.nmse(got.reshape(M, N), ref)
    plog(f"bf16 tiles over pre-rounded columns K={K} N={N} M={M}: nmse={e:.3e} kernel_launches+{dk}")
    assert classes == ["mul_mat_bf16_mma"] and dk == 2, (classes, dk)
    assert e <= GATE, e
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the f16 and bf16 forms are one kernel
def _both_formats_exact(shape, rng):
    """float32 values exact in f16 AND bf16: at most 8 significant bits (bf16's width), exponents 2^-6 .. 2^4 (well inside f16's range), random signs"""
    return (rng.integers(128, 256, shape) * np.exp2(rng.integers(-13, -2, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


# (K, N, M), the bf16 form to force (-1: routed).  K = 136 ends in the 8-mod-16 tail, N = 65 leaves a one-row edge tile; the f16 side routes itself: (136, 40, 1)
# falls through to the dot kernel (fewer than 64 rows), K = 7 fails the vector conditions, 4 columns take the 16 x 16 tiles and 33 the 32 x 32 ones
TWINS = [("dot_vector", (136, 40, 1), DOT), ("dot_scalar", (7, 65, 3), -1), ("mma16", (136, 65, 4), MMA16), ("mma", (136, 65, 33), -1)]


@pytest.mark.parametrize("pair,shape,form", TWINS, ids=[t[0] for t in TWINS])
def test_f16_and_bf16_forms_sum_in_the_same_order(backend, plog, pair, shape, form):
    """One matrix stored as F16 and as BF16, its values and the activations exact in both formats (so both roundings are the identity): the twin kernels share
    their addressing, loop and reduction, hence the f32 summation order — the two products are equal bit for bit.  The exponent spread makes the f32 sums inexact,
    so a different order WOULD show: at least one output differs from the double-precision sum rounded to f32."""
    K, N, M = shape
    rng = np.random.default_rng(4000 + K + 7 * N + 31 * M)
    Wf, X = _both_formats_exact((N, K), rng), _both_formats_exact((M, K), rng)
    W16, Wbf = Wf.astype(np.float16), B.to_bf16(Wf)
    for v in (Wf, X):  # both conversions round-trip the inputs
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v) and np.array_equal(B.from_bf16(B.to_bf16(v)), v)
    H = L.host()
    (g16,), c16 = _run_timed(backend, lambda g: H.ggml_mul_mat(g.ctx, g.new(L.F16, [K, N], W16, name="w"), g.new(L.F32, [K, M], X, name="x")))
    (gbf,), cbf = _run_timed(backend, lambda g: B.g_mul_mat(g, Wbf, X, K, N, M), form)
    exact = (X.astype(np.float64) @ Wf.astype(np.float64).T).astype(np.float32)
    g16, gbf = g16.reshape(M, N), gbf.reshape(M, N)
    n_inexact = int(np.count_nonzero(g16 != exact))
    n_diff = int(np.count_nonzero(g16.view(np.uint32) != gbf.view(np.uint32)))
    plog(f"f16 / bf16 twins {pair} K={K} N={N} M={M}: {c16} / {cbf}; {n_diff} of {g16.size} outputs differ between the formats, {n_inexact} differ from the exact sum rounded")
    assert c16 == ["mul_mat_f"] and cbf == [{"dot_vector": "mul_mat_bf16_dot", "dot_scalar": "mul_mat_bf16_dot", "mma16": "mul_mat_bf16_mma16", "mma": "mul_mat_bf16_mma"}[pair]], (c16, cbf)
    assert n_inexact > 0
    assert n_diff == 0, np.argwhere(g16.view(np.uint32) != gbf.view(np.uint32))[:4]


# ---------------------------------------------------------------------------------------------- exact on small integers
EXACT =[(1, -1), (2, -1), (3, -1), (8, -1), (8, MMV_COLS), (12, -1), (40, -1), (40, MMA), (12, MMA16), (3, DOT), (3, MMA16), (1, DOT)]


@pytest.mark.parametrize("M,form", EXACT, ids=lambda v: str(v))
def test_integer_products_are_exact(backend, M, form):
    """Weights {-4 .. 4} 2^e (e per row from {-3, 0, 5}), activations integers in -16 .. 16, K = 4096: every partial sum in any order is an integer multiple of 2^e
    below 2^24 of them, so the result equals the integer product bit for bit — a lane-map or layout error cannot hide behind a tolerance."""
    K, N = 4096, 67
    rng = np.random.default_rng(900 + M)
    lev = rng.integers(-4, 5, (N, K))
    e = np.array([-3, 0, 5])[rng.integers(0, 3, N)]
    Wf = (lev * np.exp2(e)[:, None]).astype(np.float32)
    W = B.to_bf16(Wf)
    assert np.array_equal(B.from_bf16(W), Wf)
    xi = rng.integers(-16, 17, (M, K))
    X = xi.astype(np.float32)
    want = ((xi @ lev.T) * np.exp2(e)[None, :]).astype(np.float32)
    assert np.max(np.abs(xi @ lev.T)) < 2 ** 24
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M), form)
    got = got.reshape(M, N)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (classes, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])


# ---------------------------------------------------------------------------------------------- read-back of the activation rounding
@pytest.mark.parametrize("M,form", [(1, -1), (2, -1), (4, -1), (8, MMV_COLS), (12, -1), (33, -1), (1, DOT), (4, DOT)], ids=lambda v: str(v))
def test_activation_rounding_read_back(backend, plog, M, form):
    """W = the 64 x 64 identity in bf16: row j returns bf16(x[j]) — RNE ties, their neighbours, f32 subnormals, values outside f16's range, the largest finite
    value.  Bit-equal to oracle_fp32_to_bf16 shifted up (a -0.0 comes back as +0.0: the sum starts from +0.0, in the oracle too)."""
    K = 64
    W = B.to_bf16(np.eye(K, dtype=np.float32))
    rng = np.random.default_rng(M)
    base = np.concatenate([B.READBACK_VALUES, rng.standard_normal(K - len(B.READBACK_VALUES)).astype(np.float32)])
    X = np.stack([np.roll(base, 5 * c) for c in range(M)])
    lib = T.oracle()
    want = (np.array([[lib.oracle_fp32_to_bf16(C.c_float(float(v))) for v in row] for row in X], dtype=np.uint32) << 16)
    want = np.where(want == 0x80000000, 0, want).astype(np.uint32)
    ref = T.run_case(lambda g: B.g_mul_mat(g, W, X, K, K, M), "oracle")[0].reshape(M, K)
    assert np.array_equal(ref.view(np.uint32), want)  # (the oracle's product IS the rounding)
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, K, M), form)
    got = got.reshape(M, K).view(np.uint32)
    bad = np.argwhere(got != want)
    plog(f"bf16 activation read-back M={M} {classes}: {len(bad)} of {got.size} differ" + "".join(f"; x={X[i, j]!r} got {got[i, j]:08x} want {want[i, j]:08x}" for i, j in bad[:6]))
    assert len(bad) == 0, [(float(X[i, j]), hex(got[i, j]), hex(want[i, j])) for i, j in bad[:6]]


# ---------------------------------------------------------------------------------------------- weight value edges
@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_weight_value_edges(backend, plog, M):
    """bf16 subnormals, +-0, +-0x7F7F (the largest finite weights) against activations of 2^-120, alternating-sign cancellation rows.  Finite where the oracle is;
    NMSE <= 1e-11 over the outputs above 1e-30; sums that live in the f32-subnormal range may be off by K 2^-126 (one flushed product a term: what a matrix core
    that flushes subnormals would do — the log line records what is observed)."""
    K, N = 256, 40
    rng = np.random.default_rng(300 + M)
    W = B.rand_weight(K, N, rng)
    W[0] = rng.integers(1, 0x80, K).astype(np.uint16) | (rng.integers(0, 2, K).astype(np.uint16) << 15)  # subnormals of either sign
    W[1] = np.where(np.arange(K) % 2 == 0, 0x0000, 0x8000).astype(np.uint16)                              # +0 / -0
    W[2] = np.where(np.arange(K) % 2 == 0, 0x7F7F, 0xFF7F).astype(np.uint16)                              # +-max, alternating: cancels against a constant row
    W[3] = np.full(K, 0x7F7F, dtype=np.uint16)
    W[4] = np.where(np.arange(K) % 2 == 0, 0x3F80, 0xBF80).astype(np.uint16)                              # +1 / -1
    W[5] = np.full(K, 0x0001, dtype=np.uint16)                                                            # the smallest subnormal
    # (every activation is small enough that a row of +-0x7F7F weights cannot overflow an f32 partial sum the oracle's double sum would survive)
    rows = [np.full(K, 2.0 ** -120), rng.standard_normal(K) * 2.0 ** -10, np.where(np.arange(K) % 2 == 0, 1.0, -1.0) * 2.0 ** -120,
            rng.integers(-8, 9, K) * 2.0 ** -120, rng.standard_normal(K) * 2.0 ** -126]
    X = np.stack([rows[i % len(rows)] for i in range(M)]).astype(np.float32)
    ref = T.run_case(lambda g: B.g_mul_mat(g, W, X, K, N, M), "oracle")[0].reshape(M, N)
    (got,), classes = _run_timed(backend, lambda g: B.g_mul_mat(g, W, X, K, N, M))
    got = got.reshape(M, N)
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(got[fin])), np.argwhere(fin & ~np.isfinite(got))[:4]
    big = fin & (np.abs(ref) > 1e-30)
    tiny = fin & ~big
    e = T.nmse(got[big], ref[big])
    d_tiny = float(np.max(np.abs(got[tiny].astype(np.float64) - ref[tiny]))) if tiny.any() else 0.0
    flushed = int(np.count_nonzero((got[tiny] == 0) & (ref[tiny] != 0)))
    plog(f"bf16 weight value edges M={M} {classes}: nmse over {int(big.sum())} outputs {e:.3e}; {int(tiny.sum())} outputs in the subnormal range: max |diff| {d_tiny:.3e}, "
         f"{flushed} zero where the oracle's is not")
    assert e <= GATE, e
    assert d_tiny <= K * 2.0 ** -126, d_tiny


# ---------------------------------------------------------------------------------------------- GET_ROWS
@pytest.mark.parametrize("K", [1, 7, 64, 4104], ids=lambda k: f"k{k}")
def test_get_rows_bit_equal(backend, K):
    N = 9
    rng = np.random.default_rng(9 + K)
    W = B.rand_weight(K, N, rng)
    W[0, 0], W[N - 1, K - 1] = 0x0001, 0xFF7F
    idx = np.array([8, 0, 3, 3, 2, 8, 7, 1], dtype=np.int32)  # row 0, the last row, repeats, out of order

    def build(g):
        return g.H.ggml_get_rows(g.ctx, g.new(L.BF16, [K, N], W), g.new(L.I32, [len(idx)], idx))

    got = T.run_case(build, backend)[0].reshape(len(idx), K)
    ref = T.run_case(build, "oracle")[0].reshape(len(idx), K)
    want = B.from_bf16(W)[idx]
    assert np.array_equal(ref.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_get_rows_with_a_3d_index_tensor(backend):
    K, N = 72, 6
    rng = np.random.default_rng(77)
    W = B.to_bf16(rng.standard_normal((2, 3, N, K)).astype(np.float32))
    idx = rng.integers(0, N, (2, 3, 4)).astype(np.int32)
    idx[0, 0, 0], idx[1, 2, 3] = 0, N - 1

    def build(g):
        return g.H.ggml_get_rows(g.ctx, g.new(L.BF16, [K, N, 3, 2], W), g.new(L.I32, [4, 3, 2], idx))

    got = T.run_case(build, backend)[0].reshape(2, 3, 4, K)
    want = np.stack([np.stack([B.from_bf16(W[a, b])[idx[a, b]] for b in range(3)]) for a in range(2)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- MUL_MAT_ID
@pytest.mark.parametrize("K", [64, 72, 7], ids=lambda k: f"k{k}")
@pytest.mark.parametrize("per_slot", [False, True], ids=["shared_row", "per_slot"])
def test_mul_mat_id_matches_the_oracle(backend, plog, per_slot, K):
    N, n_expert, n_used = 37, 4, 2
    rng = np.random.default_rng(3000 + K + per_slot)
    W = np.stack([B.rand_weight(K, N, rng) for _ in range(n_expert)])
    cases = []
    for n_tok in (1, 5):
        ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
        cases.append((rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32), ids))
    refs = MR.mmid_reference(L.BF16, W, K, N, cases)
    H = L.host()

    def build(g):
        as_t = g.new(L.BF16, [K, N, n_expert], W)
        return [H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, b.shape[1], b.shape[0]], b), MR.strided_ids(g, ids, n_expert)) for b, ids in cases]

    m0 = backend.stat("mmid_launches")
    res, classes = _run_timed(backend, build)
    assert backend.stat("mmid_launches") - m0 == len(cases) and classes == ["mmid_bf16"], classes
    for (b, ids), got, ref in zip(cases, res, refs):
        T.compare(f"bf16 mul_mat_id K={K} n_tokens={ids.shape[0]} per_slot={per_slot}", got.reshape(ref.shape), ref, GATE, log=plog)
        assert np.any(ref != 0)


def test_mul_mat_id_with_an_id_outside_the_experts_writes_zeros(backend):
    K, N, n_expert, n_used, n_tok = 72, 37, 4, 2, 4
    rng = np.random.default_rng(41)
    H = L.host()
    W = np.stack([B.rand_weight(K, N, rng) for _ in range(n_expert)])
    b = rng.standard_normal((n_tok, n_used, K)).astype(np.float32)
    good = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    bad = good.copy()
    bad[1, 0] = n_expert
    bad[2, 1] = -1

    def build(g):
        as_t = g.new(L.BF16, [K, N, n_expert], W)
        bt = g.new(L.F32, [K, n_used, n_tok], b)
        return [H.ggml_mul_mat_id(g.ctx, as_t, bt, MR.strided_ids(g, i, n_expert)) for i in (good, bad)]

    rg, rb = [r.reshape(n_tok, n_used, N) for r in T.run_case(build, backend)]
    assert np.count_nonzero(rg) > rg.size // 2
    for t in range(n_tok):
        for s in range(n_used):
            want = np.zeros(N, dtype=np.float32) if (t, s) in ((1, 0), (2, 1)) else rg[t, s]
            assert np.array_equal(rb[t, s].view(np.uint32), want.view(np.uint32)), (t, s)


# ---------------------------------------------------------------------------------------------- one norm output, three formats
KINDS = (L.BF16, L.Q4_K, L.Q8_0)


def _mixed_layer(backend, order, Ws, nw, X, K, N, M):
    """cur = MUL(RMS_NORM(x), w) feeds a bf16, a Q4_K and a Q8_0 matrix; the three MUL_MAT nodes enter the graph in `order`.  -> the products in KINDS order"""
    H = L.host()
    g = T.G(backend)
    try:
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X, "x"), 1e-5), g.new(L.F32, [K], nw, "norm"))
        mm = {qt: H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt], L.TYPE_NAME.get(qt, "q4_K")), cur) for qt in order}
        return g.compute([mm[qt] for qt in KINDS], expand_first=[mm[qt] for qt in order])
    finally:
        g.free()


@pytest.mark.parametrize("M", [1, 4, 33], ids=lambda m: f"m{m}")
def test_bf16_q4_k_and_q8_0_matrices_share_one_norm_output_in_every_node_order(backend, plog, M):
    """The bf16 matrix needs the norm output in f32: a prologue fusion or a producer that leaves only quantised blocks for the Q4_K / Q8_0 readers must not swallow
    it.  Every node order: the bf16 product within 1e-11 of the oracle, the quantised ones within their 1e-10."""
    K, N = 512, 48
    rng = np.random.default_rng(70 + M)
    Ws = {L.BF16: B.rand_weight(K, N, rng), L.Q4_K: T.rand_weight(L.Q4_K, K, N, rng), L.Q8_0: T.rand_weight(L.Q8_0, K, N, rng)}
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    X = (rng.standard_normal((M, K)) + 0.3).astype(np.float32)
    H = L.host()

    def reference(g):
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], X), 1e-5), g.new(L.F32, [K], nw))
        return [H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], Ws[qt]), cur) for qt in KINDS]

    ref = dict(zip(KINDS, T.run_case(reference, "oracle")))
    gate = {L.BF16: GATE, L.Q4_K: 1e-10, L.Q8_0: 1e-10}
    for order in itertools.permutations(KINDS):
        got = _mixed_layer(backend, order, Ws, nw, X, K, N, M)
        for qt, a in zip(KINDS, got):
            e = T.nmse(a, ref[qt])
            plog(f"bf16 shared norm output M={M} order {[L.TYPE_NAME.get(q, 'q4_K') for q in order]} type {L.TYPE_NAME.get(qt, 'q4_K')}: nmse={e:.3e}")
            assert e <= gate[qt], (qt, order, e)


# ---------------------------------------------------------------------------------------------- model level
def _accepted(H, backend, ctx):
    gf = H.llm_last_graph(ctx.c)
    for i in range(gf.contents.n_nodes):
        assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i]), gf.contents.nodes[i].contents.name


@pytest.mark.parametrize("name,fa", [("test-llama-bf16", 0), ("test-llama-bf16", 1), ("test-qwen2-bf16", 0), ("test-qwen2-bf16", 1)],
                         ids=["llama_nofa", "llama_fa", "qwen2_nofa", "qwen2_fa"])
def test_bf16_model_runs_whole_on_the_device(H, backend, plog, name, fa):
    """A 40-token prompt batch, 16 batch-1 steps teacher-forced on the oracle's tokens and a 4-sequence step: logits NMSE <= 1e-3 at each, greedy ids equal to the
    oracle's wherever the top-2 margin exceeds twice the oracle's own order sensitivity (at least half of the positions: tests/test_bf16_ref_host.py), every node
    accepted by the device, the batch-1 steps on the streaming kernel."""
    hp = preset(name)
    mg, mc = Model(hp, B.MODEL_SEED, backend.buft), Model(hp, B.MODEL_SEED, H.ggml_backend_cpu_buffer_type())
    cg, cc = Context(mg, backend=backend, flash_attn=fa), Context(mc, compute=T.oracle_compute_fn(), flash_attn=fa)
    try:
        assert H.llm_model_tensor(mg.m, b"token_embd.weight").contents.type == L.BF16 and H.llm_model_tensor(mg.m, b"output.weight").contents.type == L.BF16
        rc, ref = cc.decode(B.PROMPT40, range(40))
        rc2, got = cg.decode(B.PROMPT40, range(40))
        assert rc == 0 and rc2 == 0
        _accepted(H, backend, cg)
        e = T.nmse(got, ref)
        plog(f"{name} fa={fa} 40-token prompt logits: nmse={e:.3e}")
        assert e <= 1e-3
        cc.clear()
        cg.clear()
        ids_ref, rows_ref = greedy(cc, B.PROMPT40, B.N_GEN)
        rows_ref = np.stack(rows_ref)
        rc, lg = cg.decode(B.PROMPT40, range(40), want=[0] * 39 + [1])
        assert rc == 0
        rows_got = [lg[-1]]
        backend.set_option("timing", 1)
        backend.timing_report()
        for i, t in enumerate(ids_ref[:-1]):
            rc, l1 = cg.decode([t], [40 + i])
            assert rc == 0
            rows_got.append(l1[0])
        classes = sorted(backend.timing_report())
        backend.set_option("timing", 0)
        _accepted(H, backend, cg)
        rows_got = np.stack(rows_got)
        e_dec = T.nmse(rows_got, rows_ref)
        agree = np.argmax(rows_got, axis=1) == np.array(ids_ref)
        top2 = np.sort(rows_ref, axis=1)[:, -2:]
        margins = top2[:, 1] - top2[:, 0]
        plog(f"{name} fa={fa} teacher-forced decode x{len(ids_ref)}: nmse={e_dec:.3e} argmax agreement {int(agree.sum())}/{len(agree)} min margin {margins.min():.3e}; "
             f"bf16 classes {[c for c in classes if 'bf16' in c]}")
        assert e_dec <= 1e-3
        assert "mmv_bf16_nc1" in classes and not any(c.startswith("mul_mat_bf16") for c in classes), classes
        if fa == 0:  # (the yardstick is the oracle's on the soft-max path, as for test-llama)
            from test_gpu_model import _oracle_yardstick
            yard = 2.0 * _oracle_yardstick(H, name, B.PROMPT40, B.N_GEN)
            decisive = margins > yard
            plog(f"{name}: oracle-vs-oracle yardstick {yard:.3e}; {int(decisive.sum())}/{len(margins)} decode positions decisive")
            assert 2 * int(decisive.sum()) >= len(margins)
            assert bool(np.all(agree[decisive])), "greedy token differs where the margin exceeds the oracle's own order sensitivity"
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
        plog(f"{name} fa={fa} 4-sequence steps: nmse={e4:.3e}")
        assert e4 <= 1e-3
    finally:
        backend.set_option("timing", 0)
        for o in (cg, cc, mg, mc):
            o.free()


def test_bf16_decode_step_runs_in_a_captured_graph_and_replays_bit_identical_to_eager(backend, H, plog):
    mg = Model(preset("test-llama-bf16"), 99, backend.buft)
    outs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            c = Context(mg, backend=backend, flash_attn=1)
            l0 = backend.stat("graph_launches")
            ids, rows = greedy(c, B.PROMPT40[:20], 24)
            outs[mode] = (ids, np.stack(rows), backend.stat("graph_launches") - l0)
            c.free()
    finally:
        backend.set_option("graphs", 1)
        mg.free()
    plog(f"test-llama-bf16: hipGraph launches with graphs=1: {outs[1][2]}, with graphs=0: {outs[0][2]}")
    assert outs[1][2] >= 10 and outs[0][2] == 0
    assert outs[1][0] == outs[0][0]
    assert np.array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))
