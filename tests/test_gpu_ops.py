"""GPU parity tests, op level: every case is evaluated by the CPU oracle and by the MI355X backend THROUGH THE C-ABI
(ggml_backend_init -> reg -> device -> backend vtables; tests/harness.py), on the same seeded inputs.

Gates (written per case):
  * integer / byte / index results and pure data movement ............ bit-exact
  * element-wise f32 ops with one rounding per operation ............. bit-exact (kernels built with -ffp-contract=off)
  * quantised MUL_MAT: integer block sums are exact, only the f32 scale-accumulate ORDER differs -> NMSE <= 1e-10
  * reductions / transcendental ops (rms_norm, rope, soft_max) ....... NMSE <= 1e-12 .. 1e-10
  * FLASH_ATTN_EXT: the CPU accumulates V in f16 (noise grows with n_kv), the kernel in f32 -> NMSE <= 1e-4 (upstream's gate for this op is 5e-4)
"""
import numpy as np
import pytest

import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu

QTYPES = [L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0]
QNAME = {L.Q4_K: "q4_K", L.Q5_K: "q5_K", L.Q6_K: "q6_K", L.Q8_0: "q8_0", L.F16: "f16", L.F32: "f32"}


def both(build, backend):
    return T.run_case(build, "oracle"), T.run_case(build, backend)


# ------------------------------------------------------------------------------------------------ MUL_MAT (quantised)
MM_SHAPES = [  # (K, N, M)
    (256, 8, 1), (512, 33, 1), (4096, 64, 1), (4096, 257, 1), (14336, 16, 1), (2048, 40, 1),
    (1024, 48, 2), (1024, 48, 3), (512, 64, 4), (512, 20, 5), (768, 32, 8), (512, 24, 9), (512, 16, 19),
    # M >= 3 takes the matrix-core path for K-quants: full tiles, ragged rows/columns, several super-blocks
    (512, 128, 128), (1024, 200, 300), (4096, 256, 160), (256, 130, 33), (2048, 384, 512),
]


@pytest.mark.parametrize("qt", QTYPES)
@pytest.mark.parametrize("K,N,M", MM_SHAPES)
def test_mul_mat_q(backend, H, plog, qt, K, N, M):
    rng = np.random.default_rng(K * 131 + N * 7 + M + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    if M > 1:
        x[0, :256] = 0.0  # an all-zero activation block (d = 0 branch)

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))

    ref, got = both(build, backend)
    T.compare(f"mul_mat {QNAME[qt]} K={K} N={N} M={M}", got[0], ref[0], max_nmse=1e-10, log=plog)


@pytest.mark.parametrize("qt", QTYPES)
@pytest.mark.parametrize("K,N,M", [(1024, 48, 3), (512, 64, 4), (512, 20, 5), (768, 32, 8), (4096, 130, 7)])
def test_mul_mat_q_multi_column_mat_vec(backend, H, plog, qt, K, N, M):
    """3..8 columns on the multi-column mat-vec kernels (k_mmvq<T, NC>): the route taken when the matrix-core path is switched
    off (mmq_min_cols above the batch) and, for Q8_0 weights, always below 33 columns."""
    rng = np.random.default_rng(K + N + M + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))

    backend.set_option("mmq_min_cols", 9)
    try:
        ref, got = both(build, backend)
    finally:
        backend.set_option("mmq_min_cols", 3)
    T.compare(f"mul_mat multi-column mat-vec {QNAME[qt]} K={K} N={N} M={M}", got[0], ref[0], max_nmse=1e-10, log=plog)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K,N,M", [(2048, 70, 32), (2048, 33, 24), (5632, 40, 32), (4096, 64, 13), (4096, 48, 20), (11008, 20, 32), (256, 19, 12), (2048, 2050, 31), (128, 7, 9), (14336, 96, 32),
                                   (2080, 33, 24), (1056, 40, 32), (4128, 16, 13), (11040, 20, 32), (2048, 70, 48), (4096, 64, 64), (2048, 40, 33), (5632, 33, 57), (2048, 64, 128), (1024, 33, 97)])
def test_mul_mat_q8_0_9_to_32_columns(backend, H, plog, K, N, M, bias):
    """Q8_0 weights, 9 .. 32 columns (a -np decode step of a Q8_0 model; round 6; 33 .. 128 columns as passes of 32).  K a multiple of 128: the weight-streaming matrix-core kernel (mmq_q80.hip:
    k_mmq_q80_skinny — 32-row panels, K split over eight waves, one MFMA per block, f32 scale-accumulate in ggml-cpu's expression).  Other K (whole Q8_0 blocks only):
    16 or 32 columns in ONE pass of the multi-column mat-vec kernel when their blocks fit the LDS — bit-equal to the same columns computed 8 at a time (same dot
    products per column, same f32 order).  Both against the oracle; bias / residual ADD folded into the store."""
    rng = np.random.default_rng(K + 3 * N + M)
    w = T.rand_weight(L.Q8_0, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    x[1, :32] = 0.0
    b = rng.standard_normal(N).astype(np.float32)

    def build_cols(c0, c1):
        def build(g):
            r = H.ggml_mul_mat(g.ctx, g.new(L.Q8_0, [K, N], w), g.new(L.F32, [K, c1 - c0], x[c0:c1]))
            return H.ggml_add(g.ctx, r, g.new(L.F32, [N], b)) if bias else r
        return build

    s0 = backend.stat("skinny_launches")
    ref, got = both(build_cols(0, M), backend)
    served = backend.stat("skinny_launches") - s0
    T.compare(f"mul_mat q8_0 K={K} N={N} M={M} bias={bias} ({'matrix cores' if served else 'wide mat-vec passes'})", got[0], ref[0], max_nmse=1e-10, log=plog)
    assert served == (1 if K % 128 == 0 else 0)
    if not served:
        by8 = np.concatenate([T.run_case(build_cols(c, min(M, c + 8)), backend)[0].reshape(-1, N) for c in range(0, M, 8)])
        assert np.array_equal(got[0].reshape(-1, N).view(np.uint32), by8.view(np.uint32))


@pytest.mark.parametrize("M,bias", [(32, False), (12, True), (64, True), (9, False)])
def test_q8_0_sibling_mul_mats_share_a_launch(backend, H, plog, M, bias):
    """wq / wk / wv of a Q8_0 model's batch multiply the same activations: ONE launch of the 9 .. 128-column matrix-core kernel over the concatenated 32-row panels
    (graph.cpp: try_merge_q80_skinny), bias ADDs folded into the store — equal to the oracle, and bit-equal to the one-by-one execution (same kernel, same tiles)."""
    rng = np.random.default_rng(M * 11 + 1)
    K, NQ, NK = 1024, 512, 96
    wq, wk, wv = T.rand_weight(L.Q8_0, K, NQ, rng), T.rand_weight(L.Q8_0, K, NK, rng), T.rand_weight(L.Q8_0, K, NK, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) for n in (NQ, NK, NK))

    def build(g):
        cur = g.new(L.F32, [K, M], x)
        outs = []
        for w, n, b in ((wq, NQ, bq), (wk, NK, bk), (wv, NK, bv)):
            r = H.ggml_mul_mat(g.ctx, g.new(L.Q8_0, [K, n], w), cur)
            if bias:
                r = H.ggml_add(g.ctx, r, g.new(L.F32, [n], b))
            outs.append(r)
        return outs

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("mm_merge", 0)
    try:
        k1 = backend.stat("kernel_launches")
        plain = T.run_case(build, backend)
        launches_plain = backend.stat("kernel_launches") - k1
    finally:
        backend.set_option("mm_merge", 1)
    plog(f"    Q8_0 sibling mat-muls M={M} bias={bias}: {launches} launches merged, {launches_plain} one by one")
    assert launches == 2 and launches < launches_plain  # quantise + one matrix-core launch (M = 64: two passes inside the launcher count as one)
    for name, a, b, c in zip("qkv", got, ref, plain):
        T.compare(f"Q8_0 sibling mat-muls M={M} bias={bias} {name}", a, b, max_nmse=1e-10, log=plog)
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(c).view(np.uint32))


@pytest.mark.parametrize("i8,bn", [(1, 64), (1, 128), (0, 0)])
@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K, L.Q6_K])
@pytest.mark.parametrize("K,N,M", [(512, 128, 128), (1024, 200, 300), (2048, 384, 512), (256, 130, 33), (4096, 256, 24), (512, 200, 64), (1024, 96, 9), (2048, 384, 40), (4096, 1024, 32)])
def test_mul_mat_q_matrix_core_variants(backend, H, plog, qt, K, N, M, i8, bn):
    """K-quant batches: the int8-MFMA GEMM with 64- and 128-row panels and 32 / 64 / 128-column tiles (mmq_i8.hip) and the
    f16-MFMA kernel (mmq.hip)."""
    rng = np.random.default_rng(K * 31 + N * 7 + M + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    x[1, 256:512] = 0.0

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))

    backend.set_option("mmq_i8", i8)
    backend.set_option("mmq_bn", bn)
    try:
        ref, got = both(build, backend)
    finally:
        backend.set_option("mmq_i8", 1)
        backend.set_option("mmq_bn", 0)
    T.compare(f"mul_mat {QNAME[qt]} K={K} N={N} M={M} i8={i8} bn={bn}", got[0], ref[0], max_nmse=1e-10, log=plog)


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K, L.Q6_K])
def test_f16_tiles_leave_a_bias_add_to_the_mat_vec_passes(backend, H, plog, qt):
    """Options mmq_i8 = 0 and mmvq_max_cols = 9, nine columns (the narrowest batch the f16-MFMA tile kernel takes, admitted to the mat-vec fusions by the second
    option): that kernel has no addend in its store, so MUL_MAT -> ADD(bias) runs as passes of the mat-vec kernel with the bias folded in, while the bare MUL_MAT
    takes the tiles."""
    K, N, M = 256, 64, 9
    rng = np.random.default_rng(300 + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)

    def build(bias):
        def f(g):
            r = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))
            return H.ggml_add(g.ctx, r, g.new(L.F32, [N], b)) if bias else r
        return f

    backend.set_option("mmq_i8", 0)
    backend.set_option("mmvq_max_cols", 9)
    backend.set_option("timing", 1)
    try:
        for bias, prefix in ((True, "mmvq_"), (False, "mmq_")):
            ref = T.run_case(build(bias), "oracle")
            backend.timing_report()
            f0 = backend.stat("fused_nodes")
            got = T.run_case(build(bias), backend)
            classes = sorted(backend.timing_report())
            mmc = [c for c in classes if c.startswith(("mmvq_", "mmq_"))]
            assert len(mmc) == 1 and mmc[0].startswith(prefix + QNAME[qt]), (bias, classes)
            assert backend.stat("fused_nodes") - f0 == (1 if bias else 0), (bias, classes)
            T.compare(f"mul_mat {QNAME[qt]} M={M} mmq_i8=0 bias={bias}", got[0], ref[0], max_nmse=1e-10, log=plog)
    finally:
        backend.set_option("mmq_i8", 1)
        backend.set_option("mmvq_max_cols", 2)
        backend.set_option("timing", 0)


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K, L.Q6_K])
@pytest.mark.parametrize("M,bias", [(32, False), (12, True), (64, True), (300, False), (512, True)])
def test_sibling_mul_mats_share_a_launch(backend, H, plog, qt, M, bias):
    """wq / wk / wv (and gate / up) of a batch multiply the same activations: one matrix-core launch over the concatenated row
    panels (+ one split-K pass when the K range is split), bias ADDs folded into the store — equal to the oracle and to the
    one-by-one execution bit for bit (same kernel, same tiles)."""
    rng = np.random.default_rng(M * 7 + qt)
    K, NQ, NK = 1024, 512, 128
    wq, wk, wv = T.rand_weight(qt, K, NQ, rng), T.rand_weight(qt, K, NK, rng), T.rand_weight(qt, K, NK, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) for n in (NQ, NK, NK))

    def build(g):
        cur = g.new(L.F32, [K, M], x)
        outs = []
        for w, n, b in ((wq, NQ, bq), (wk, NK, bk), (wv, NK, bv)):
            r = H.ggml_mul_mat(g.ctx, g.new(qt, [K, n], w), cur)
            if bias:
                r = H.ggml_add(g.ctx, r, g.new(L.F32, [n], b))
            outs.append(r)
        return outs

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("mm_merge", 0)
    try:
        k1 = backend.stat("kernel_launches")
        plain = T.run_case(build, backend)
        launches_plain = backend.stat("kernel_launches") - k1
    finally:
        backend.set_option("mm_merge", 1)
    plog(f"    sibling mat-muls {QNAME[qt]} M={M} bias={bias}: {launches} launches merged, {launches_plain} one by one")
    assert launches <= 3 and launches < launches_plain  # quantise + GEMM (+ split-K pass)
    for name, a, b, c in zip("qkv", got, ref, plain):
        T.compare(f"sibling mat-muls {QNAME[qt]} M={M} bias={bias} {name}", a, b, max_nmse=1e-10, log=plog)
        T.compare(f"sibling mat-muls {QNAME[qt]} M={M} bias={bias} {name} vs one by one", a, c, max_nmse=1e-12, log=plog)


@pytest.mark.parametrize("tq,tv", [(L.Q4_K, L.Q6_K), (L.Q5_K, L.Q6_K)])
@pytest.mark.parametrize("M,K,bias", [(32, 4096, False), (5, 4096, True), (17, 1024, False)])
def test_sibling_mul_mats_of_two_formats_share_a_launch(backend, H, plog, tq, tv, M, K, bias):
    """2..32 columns: wq / wk in one K-quant format and wv in another (Q4_K_M / Q5_K_M keep wv as Q6_K in half the layers) multiply the
    same activations in ONE skinny launch — a pass per format over the workgroup's items — here WITHOUT the rope epilogue (the results
    are graph outputs), so also with a K split and its reduce pass where the tiles alone do not fill the chip (K = 4096: four K slices).
    Equal to the oracle; against the separate launches (skinny_mix = 0) only the order of the K slices' partial sums may differ."""
    rng = np.random.default_rng(M * 11 + tq + K)
    NQ, NK = 1024, 256
    wq, wk, wv = T.rand_weight(tq, K, NQ, rng), T.rand_weight(tq, K, NK, rng), T.rand_weight(tv, K, NK, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) for n in (NQ, NK, NK))

    def build(g):
        cur = g.new(L.F32, [K, M], x)
        outs = []
        for t, w, n, b in ((tq, wq, NQ, bq), (tq, wk, NK, bk), (tv, wv, NK, bv)):
            r = H.ggml_mul_mat(g.ctx, g.new(t, [K, n], w), cur)
            if bias:
                r = H.ggml_add(g.ctx, r, g.new(L.F32, [n], b))
            outs.append(r)
        return outs

    ref = T.run_case(build, "oracle")
    k0, s0 = backend.stat("kernel_launches"), backend.stat("skinny_launches")
    got = T.run_case(build, backend)
    launches, served = backend.stat("kernel_launches") - k0, backend.stat("skinny_launches") - s0
    backend.set_option("skinny_mix", 0)
    try:
        k1 = backend.stat("kernel_launches")
        apart = T.run_case(build, backend)
        launches_apart = backend.stat("kernel_launches") - k1
    finally:
        backend.set_option("skinny_mix", 1)
    plog(f"    sibling mat-muls {QNAME[tq]}/{QNAME[tv]} M={M} K={K} bias={bias}: {launches} launches in two formats at once, {launches_apart} apart")
    assert served == 1 and launches <= 3 and launches < launches_apart, (served, launches, launches_apart)  # quantise + mat-mul (+ split-K pass)
    for name, a, b, c in zip("qkv", got, ref, apart):
        T.compare(f"two-format siblings {QNAME[tq]}/{QNAME[tv]} M={M} K={K} bias={bias} {name}", a, b, max_nmse=1e-10, log=plog)
        T.compare(f"two-format siblings {QNAME[tq]}/{QNAME[tv]} M={M} K={K} bias={bias} {name} vs apart", a, c, max_nmse=1e-12, log=plog)


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K, L.Q6_K])
@pytest.mark.parametrize("K,N,M,epi", [
    (512, 32, 3, "none"), (512, 64, 32, "bias"), (1024, 96, 9, "res"), (4096, 512, 32, "res"), (4096, 512, 17, "none"),
    (14336, 128, 32, "res"), (2048, 4096, 32, "bias"), (2048, 4096, 5, "none"), (3584, 608, 31, "res"), (8192, 256, 32, "none"),
    # enough 128-row groups to occupy the chip: the tile-parallel form (four tiles of a super-block share its activations, LDS-DMA rings)
    (512, 24576, 32, "res"), (1024, 28672, 7, "none"), (256, 32768, 19, "bias"), (2048, 24704, 32, "none"),
    # more groups than CUs: workgroups serve two items (the request rings run across the item boundary); Q4_K with K % 512 == 0 takes
    # the eight-wave form (two waves per tile, even / odd super-blocks)
    (1024, 49152, 32, "res"), (1536, 40960, 13, "none"),
])
def test_mul_mat_q_skinny_batches(backend, H, plog, qt, K, N, M, epi):
    """2..32 columns (a decode step of `-np` parallel sequences): the weight-streaming matrix-core kernel (mmq_skinny.hip) —
    one workgroup per 32-row tile, eight waves over the super-blocks, K split across workgroups when the tiles alone do not
    fill the chip (N = 4096 at K = 2048: two K halves, summed by the reduce pass).  Same integer block sums as ggml-cpu's
    vec_dot_q*_K_q8_K; the gate is the per-op one.  Also against the tiled GEMM it replaces (mmq_skinny = 0)."""
    rng = np.random.default_rng(K * 31 + N * 7 + M + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    x[M - 1, :256] = 0.0
    addend = rng.standard_normal((M, N) if epi == "res" else (N,)).astype(np.float32)

    def build(g):
        r = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))
        if epi == "bias":
            r = H.ggml_add(g.ctx, r, g.new(L.F32, [N], addend))
        elif epi == "res":
            r = H.ggml_add(g.ctx, r, g.new(L.F32, [N, M], addend))
        return r

    ref = T.run_case(build, "oracle")
    s0 = backend.stat("skinny_launches")
    got = T.run_case(build, backend)
    served = backend.stat("skinny_launches") - s0
    expect = 0 if (qt == L.Q6_K and (K // 256) % 2) else 1  # Q6_K rows of an odd number of 210-byte blocks are not dword-aligned
    assert served == expect, f"skinny kernel served {served} launches, expected {expect}"
    T.compare(f"mul_mat skinny {QNAME[qt]} K={K} N={N} M={M} {epi}", got[0], ref[0], max_nmse=1e-10, log=plog)
    backend.set_option("mmq_skinny", 0)
    try:
        tiled = T.run_case(build, backend)
    finally:
        backend.set_option("mmq_skinny", 1)
    T.compare(f"mul_mat skinny {QNAME[qt]} K={K} N={N} M={M} {epi} vs tiled GEMM", got[0], tiled[0], max_nmse=1e-12, log=plog)


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K])
@pytest.mark.parametrize("K,N,M,epi,served", [
    (512, 4096, 512, "res", 1), (1024, 8192, 300, "bias", 1), (256, 12288, 130, "none", 1), (2048, 16384, 33, "none", 1), (4096, 16384, 64, "res", 1),
    (512, 28672, 128, "none", 1), (1024, 16384, 200, "bias", 1),  # many row groups, ragged columns
    (2048, 4096, 100, "none", 0),  # too few (row group, token tile) pairs to fill the chip: the tiled GEMM keeps it
])
def test_mul_mat_q_wide_batches(backend, H, plog, qt, K, N, M, epi, served):
    """Prompt batches (33 columns and up) on the wide form of the skinny unit (mmq_skinny.hip, k_mmq_wide): four row tiles x two
    token tiles per workgroup + two loader waves, weights converted once per super-block in registers, both operands by LDS-DMA.  Ragged column
    counts (the last token-tile group is fetched whole and stored partly), residual / bias in the store; same integers as
    ggml-cpu's vec_dot_q*_K_q8_K.  Also against the tiled GEMM it replaces (mmq_skinny = 0)."""
    rng = np.random.default_rng(K * 31 + N * 7 + M + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    x[M - 1, :256] = 0.0
    addend = rng.standard_normal((M, N) if epi == "res" else (N,)).astype(np.float32)

    def build(g):
        r = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))
        if epi == "bias":
            r = H.ggml_add(g.ctx, r, g.new(L.F32, [N], addend))
        elif epi == "res":
            r = H.ggml_add(g.ctx, r, g.new(L.F32, [N, M], addend))
        return r

    ref = T.run_case(build, "oracle", T.host_threads(32))
    s0 = backend.stat("wide_launches")
    got = T.run_case(build, backend)
    assert backend.stat("wide_launches") - s0 == served
    T.compare(f"mul_mat wide {QNAME[qt]} K={K} N={N} M={M} {epi}", got[0], ref[0], max_nmse=1e-10, log=plog)
    backend.set_option("mmq_skinny", 0)
    try:
        tiled = T.run_case(build, backend)
    finally:
        backend.set_option("mmq_skinny", 1)
    T.compare(f"mul_mat wide {QNAME[qt]} K={K} N={N} M={M} {epi} vs tiled GEMM", got[0], tiled[0], max_nmse=1e-12, log=plog)


def _random_mm_shapes():
    rng = np.random.default_rng(2024)
    out = []
    for i in range(40):
        qt = QTYPES[i % 4]
        K = int(rng.choice([256, 512, 768, 1024, 2048, 3584, 4096]))
        N = int(rng.integers(1, 700))
        M = int(rng.choice([1, 2, 3, 5, 7, 8, 9, 10, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 100, 127, 128, 129, 200, 300]))
        out.append((qt, K, N, M))
    return out


@pytest.mark.parametrize("qt,K,N,M", _random_mm_shapes())
def test_mul_mat_q_random_shapes(backend, H, plog, qt, K, N, M):
    """Seeded sweep over ragged shapes: every row count (panel tails, odd N), every column-count regime (mat-vec passes, 32 / 64 /
    128-column matrix-core tiles and their tails) and K lengths that give uneven K splits — all formats."""
    rng = np.random.default_rng(K * 7 + N * 13 + M * 17 + qt)
    w = T.rand_weight(qt, K, N, rng)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)

    def build(g):
        r = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))
        return H.ggml_add(g.ctx, r, g.new(L.F32, [N], bias)) if (N + M) % 2 else r

    ref, got = both(build, backend)
    T.compare(f"mul_mat random {QNAME[qt]} K={K} N={N} M={M}", got[0], ref[0], max_nmse=1e-10, log=plog)


@pytest.mark.parametrize("qt", QTYPES)
def test_mul_mat_q_3d_src1(backend, H, plog, qt):
    """src1 with ne12 > 1 (all rows of src1 are columns of the product) and a strided (permuted) src1."""
    rng = np.random.default_rng(77 + qt)
    K, N = 512, 40
    w = T.rand_weight(qt, K, N, rng)
    x = rng.standard_normal((2, 3, K)).astype(np.float32)  # ggml [K, 3, 2]

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), g.new(L.F32, [K, 3, 2], x))

    ref, got = both(build, backend)
    T.compare(f"mul_mat {QNAME[qt]} 3d", got[0], ref[0], max_nmse=1e-10, log=plog)

    def build_perm(g):
        a = g.new(L.F32, [K, 2, 3], np.ascontiguousarray(x.transpose(1, 0, 2)))
        return H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], w), H.ggml_permute(g.ctx, a, 0, 2, 1, 3))

    ref2, got2 = both(build_perm, backend)
    T.compare(f"mul_mat {QNAME[qt]} permuted src1", got2[0], ref2[0], max_nmse=1e-10, log=plog)
    assert T.nmse(ref2[0], ref[0]) < 1e-12


# ------------------------------------------------------------------------------------------------ MUL_MAT (f16/f32)
@pytest.mark.parametrize("wt", [L.F16, L.F32])
@pytest.mark.parametrize("K,N,M,B0,B1", [(128, 96, 1, 2, 8), (64, 33, 3, 1, 4), (200, 17, 2, 1, 1), (2048, 128, 1, 2, 4), (7, 5, 2, 1, 1),
                                          # batches of columns (a prompt chunk on the non-flash path): the f16 matrix-core kernel, ragged tiles, K = 8 mod 16
                                          # one column, grouped heads (a decode step on the non-flash path): short rows (K.q) and long rows (V^T.p), ragged
                                          (128, 300, 1, 2, 8), (64, 1000, 1, 4, 4), (80, 77, 1, 1, 8), (512, 65, 1, 3, 6), (2304, 128, 1, 8, 32), (1000, 66, 1, 1, 2), (520, 64, 1, 2, 2),
                                          # few tiles over long rows (V^T.p of a -np decode batch) and 2..15 columns: 16x16 tiles, K split over the workgroup's waves
                                          (7304, 128, 32, 2, 8), (3000, 40, 20, 1, 2), (128, 300, 8, 2, 8), (1032, 16, 5, 1, 3),
                                          (4096, 96, 40, 2, 4), (2056, 128, 64, 1, 3), (4104, 160, 8, 1, 2),
                                          # short rows, many of them, against a batch (K.Q): columns of 4 / 2 / 1 grouped heads resident in registers
                                          (128, 3000, 32, 2, 8), (128, 700, 70, 2, 4), (64, 513, 16, 3, 3), (120, 300, 33, 1, 2), (72, 260, 20, 2, 14),
                                          (128, 96, 40, 2, 8), (64, 130, 33, 1, 4), (200, 70, 16, 1, 1), (2048, 128, 100, 2, 4), (136, 50, 64, 1, 2), (128, 512, 512, 8, 32)])
def test_mul_mat_f(backend, H, plog, wt, K, N, M, B0, B1):
    rng = np.random.default_rng(K + N + M)
    w = rng.standard_normal((B0, N, K)).astype(np.float16 if wt == L.F16 else np.float32)
    x = rng.standard_normal((B1, M, K)).astype(np.float32)

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(wt, [K, N, B0], w), g.new(L.F32, [K, M, B1], x))

    ref, got = both(build, backend)
    T.compare(f"mul_mat {QNAME[wt]} K={K} N={N} M={M} bc={B0}->{B1}", got[0], ref[0], max_nmse=1e-11, log=plog)


def test_mul_mat_f16_kv_views(backend, H, plog):
    """The non-flash attention products exactly as llama_lite builds them: K view (strided f16) x permuted Q, then
    transposed-V view x soft-max output."""
    rng = np.random.default_rng(3)
    HD, NKV, NH, T_, NCTX, NKVLEN = 64, 2, 4, 3, 512, 256
    kc = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    q = rng.standard_normal((T_, NH, HD)).astype(np.float32)
    p = rng.uniform(0, 1, (NH, T_, NKVLEN)).astype(np.float32)

    def build(g):
        k_cache = g.new(L.F16, [NKV * HD, NCTX], kc)
        v_cache = g.new(L.F16, [NCTX, NKV * HD], vc)
        tq = g.new(L.F32, [HD, NH, T_], q)
        tp = g.new(L.F32, [NKVLEN, T_, NH], p)
        qp = H.ggml_permute(g.ctx, tq, 0, 2, 1, 3)
        k = H.ggml_view_3d(g.ctx, k_cache, HD, NKVLEN, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, v_cache, NKVLEN, HD, NKV, NCTX * 2, NCTX * 2 * HD, 0)
        return [H.ggml_mul_mat(g.ctx, k, qp), H.ggml_mul_mat(g.ctx, v, tp)]

    ref, got = both(build, backend)
    T.compare("kq (strided K view x permuted Q)", got[0], ref[0], max_nmse=1e-11, log=plog)
    T.compare("kqv (transposed V view x P)", got[1], ref[1], max_nmse=1e-11, log=plog)


@pytest.mark.parametrize("NKVLEN", [256, 2304])
def test_mul_mat_f16_kv_views_decode(backend, H, plog, NKVLEN):
    """One token against the cache views with 4 query heads per KV head: the grouped-head mat-vec kernels."""
    rng = np.random.default_rng(5 + NKVLEN)
    HD, NKV, NH, NCTX = 128, 2, 8, 4096
    kc = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    q = rng.standard_normal((1, NH, HD)).astype(np.float32)
    p = rng.uniform(0, 1, (NH, 1, NKVLEN)).astype(np.float32)

    def build(g):
        k_cache = g.new(L.F16, [NKV * HD, NCTX], kc)
        v_cache = g.new(L.F16, [NCTX, NKV * HD], vc)
        tq = g.new(L.F32, [HD, NH, 1], q)
        tp = g.new(L.F32, [NKVLEN, 1, NH], p)
        qp = H.ggml_permute(g.ctx, tq, 0, 2, 1, 3)
        k = H.ggml_view_3d(g.ctx, k_cache, HD, NKVLEN, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, v_cache, NKVLEN, HD, NKV, NCTX * 2, NCTX * 2 * HD, 0)
        return [H.ggml_mul_mat(g.ctx, k, qp), H.ggml_mul_mat(g.ctx, v, tp)]

    ref, got = both(build, backend)
    T.compare(f"kq decode n_kv={NKVLEN}", got[0], ref[0], max_nmse=1e-11, log=plog)
    T.compare(f"kqv decode n_kv={NKVLEN}", got[1], ref[1], max_nmse=1e-11, log=plog)


@pytest.mark.parametrize("NH,NKV,NKVLEN,mask_t", [(8, 2, 256, L.F16), (8, 2, 2304, L.F16), (32, 8, 2304, L.F32), (4, 4, 4104, L.F16), (7, 1, 1000, L.F16),
                                                  (16, 2, 5000, None), (6, 2, 9000, L.F16), (8, 8, 64, L.F32)])
def test_soft_max_folded_into_vt_p(backend, H, plog, NH, NKV, NKVLEN, mask_t):
    """Decode on the non-flash path: SOFT_MAX(K.q, mask, scale) -> MUL_MAT(V^T view, p) runs as one launch (mmf.hip) and equals the oracle and the two
    separate launches (the probabilities and their f16 rounding are the same numbers; only the partition of the double sum differs)."""
    rng = np.random.default_rng(11 + NKVLEN + NH)
    HD, NCTX = 128, ((NKVLEN + 255) // 256) * 256
    vc = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    kq = (rng.standard_normal((NH, 1, NKVLEN)) * 20).astype(np.float32)
    mask = np.zeros((64, NKVLEN), np.float32)
    mask[:, int(NKVLEN * 0.8):] = -np.inf  # the cells past this sequence
    mask[:, 3] = -np.inf

    def build(g):
        v_cache = g.new(L.F16, [NCTX, NKV * HD], vc)
        tkq = g.new(L.F32, [NKVLEN, 1, NH], kq)
        tm = None if mask_t is None else g.new(mask_t, [NKVLEN, 64], mask.astype(np.float16) if mask_t == L.F16 else mask)
        p = H.ggml_soft_max_ext(g.ctx, tkq, tm, 0.0883883, 0.0)
        v = H.ggml_view_3d(g.ctx, v_cache, NKVLEN, HD, NKV, NCTX * 2, NCTX * 2 * HD, 0)
        return [H.ggml_mul_mat(g.ctx, v, p)]

    ref = T.run_case(build, "oracle")
    f0, k0 = backend.stat("fused_nodes"), backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    fused, launches = backend.stat("fused_nodes") - f0, backend.stat("kernel_launches") - k0
    backend.set_option("softmax_mm", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("softmax_mm", 1)
    assert fused == 1 and launches == 1, (fused, launches)
    T.compare(f"soft_max+V^T.p NH={NH} NKV={NKV} n_kv={NKVLEN} mask={mask_t}", got[0], ref[0], max_nmse=1e-11, log=plog)
    # the separate soft_max splits the double sum over threads differently and its mat-vec adds in another order: f32 rounding level
    assert T.nmse(got[0], plain[0]) < 1e-11


# ------------------------------------------------------------------------------------------------ element-wise & norm
@pytest.mark.parametrize("ne", [(4096, 1), (256, 7), (3584, 3), (100, 5, 2)])
def test_rms_norm_and_mul(backend, H, plog, ne):
    rng = np.random.default_rng(sum(ne))
    x = (rng.standard_normal(ne[::-1]) * 3).astype(np.float32)
    w = rng.uniform(0.5, 1.5, ne[0]).astype(np.float32)

    def build(g):
        n = H.ggml_rms_norm(g.ctx, g.new(L.F32, ne, x), 1e-5)
        return [H.ggml_mul(g.ctx, n, g.new(L.F32, [ne[0]], w))]

    def build_keep(g):  # norm output has two consumers -> must NOT be fused away
        n = H.ggml_rms_norm(g.ctx, g.new(L.F32, ne, x), 1e-5)
        return [H.ggml_mul(g.ctx, n, g.new(L.F32, [ne[0]], w)), H.ggml_scale(g.ctx, n, 2.0)]

    ref, got = both(build, backend)
    T.compare(f"rms_norm*w {ne}", got[0], ref[0], max_nmse=1e-13, max_abs=2e-6, log=plog)
    ref, got = both(build_keep, backend)
    T.compare(f"rms_norm*w (shared) {ne}", got[0], ref[0], max_nmse=1e-13, log=plog)
    T.compare(f"rms_norm*2 (shared) {ne}", got[1], ref[1], max_nmse=1e-13, log=plog)


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div"])
def test_binary_broadcast(backend, H, plog, op):
    rng = np.random.default_rng(11)
    a = rng.standard_normal((2, 3, 5, 64)).astype(np.float32)
    cases = {"same": (64, 5, 3, 2), "row": (64, 1, 1, 1), "col": (1, 5, 3, 1), "batch": (64, 5, 1, 1)}
    fn = getattr(H, "ggml_" + op)
    for name, ne in cases.items():
        b = (rng.standard_normal(ne[::-1]) + 3.0).astype(np.float32)

        def build(g):
            return fn(g.ctx, g.new(L.F32, [64, 5, 3, 2], a), g.new(L.F32, ne, b))

        ref, got = both(build, backend)
        T.compare(f"{op} bcast={name}", got[0], ref[0], max_nmse=0.0, log=plog)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


def test_scale_unary_glu(backend, H, plog):
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((6, 512)) * 4).astype(np.float32)
    y = rng.standard_normal((6, 512)).astype(np.float32)

    def build(g):
        tx = g.new(L.F32, [512, 6], x)
        ty = g.new(L.F32, [512, 6], y)
        return [H.ggml_scale_bias(g.ctx, tx, 0.37, -1.25), H.ggml_silu(g.ctx, tx), H.ggml_swiglu_split(g.ctx, tx, ty), H.ggml_swiglu(g.ctx, tx)]

    ref, got = both(build, backend)
    T.compare("scale_bias", got[0], ref[0], max_nmse=0.0, log=plog)
    T.compare("silu", got[1], ref[1], max_nmse=1e-13, log=plog)
    T.compare("swiglu_split", got[2], ref[2], max_nmse=1e-13, log=plog)
    T.compare("swiglu (halves)", got[3], ref[3], max_nmse=1e-13, log=plog)


def test_cpy_cont_cast(backend, H, plog):
    rng = np.random.default_rng(13)
    x = (rng.standard_normal((3, 4, 5, 64)) * 100).astype(np.float32)

    def build(g):
        tx = g.new(L.F32, [64, 5, 4, 3], x)
        perm = H.ggml_permute(g.ctx, tx, 0, 2, 1, 3)
        h = H.ggml_cast(g.ctx, tx, L.F16)
        return [H.ggml_cont(g.ctx, perm), h, H.ggml_cast(g.ctx, h, L.F32), H.ggml_cont_2d(g.ctx, perm, 64 * 4, 15), H.ggml_cont(g.ctx, H.ggml_transpose(g.ctx, tx))]

    ref, got = both(build, backend)
    for i, nm in enumerate(["cont(permute)", "cast f32->f16", "cast f16->f32", "cont_2d", "cont(transpose)"]):
        T.compare(nm, got[i].view(np.uint16 if got[i].dtype == np.float16 else np.uint32), ref[i].view(np.uint16 if ref[i].dtype == np.float16 else np.uint32), max_nmse=0.0, log=plog)


@pytest.mark.parametrize("qt", QTYPES + [L.F16, L.F32])
def test_get_rows(backend, H, plog, qt):
    rng = np.random.default_rng(14 + qt)
    K, N = 512, 50
    w = T.rand_weight(qt, K, N, rng)
    idx = np.array([0, 49, 7, 7, 13], dtype=np.int32)

    def build(g):
        return H.ggml_get_rows(g.ctx, g.new(qt, [K, N], w), g.new(L.I32, [5], idx))

    ref, got = both(build, backend)
    T.compare(f"get_rows {QNAME[qt]}", got[0].view(np.uint32), ref[0].view(np.uint32), max_nmse=0.0, log=plog)


def test_get_rows_golden(backend, H, plog):
    """Dequantisation of the COMMITTED golden blocks on the device == the NumPy golden (three-way pin)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "quant_golden.npz"))
    for name, qt in (("q8_0", L.Q8_0), ("q4_K", L.Q4_K), ("q5_K", L.Q5_K), ("q6_K", L.Q6_K)):
        blocks = np.ascontiguousarray(gold[name + "_blocks"])
        nbk = 512 // L.TYPE_BLCK[qt]
        rows = blocks.shape[0] // nbk
        idx = np.arange(rows, dtype=np.int32)

        def build(g):
            return H.ggml_get_rows(g.ctx, g.new(qt, [512, rows], blocks), g.new(L.I32, [rows], idx))

        got = T.run_case(build, backend)[0].reshape(-1)
        ref = gold[name + "_dequant"].reshape(-1)
        T.compare(f"golden dequant {name}", got.view(np.uint32), ref.view(np.uint32), max_nmse=0.0, log=plog)


def test_mul_mat_golden(backend, H, plog):
    """Quantised mat-vec on the committed golden blocks/activations == the float64 golden dot products."""
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "quant_golden.npz"))
    for name, qt in (("q8_0", L.Q8_0), ("q4_K", L.Q4_K), ("q5_K", L.Q5_K), ("q6_K", L.Q6_K)):
        blocks = np.ascontiguousarray(gold[name + "_blocks"])
        x = np.ascontiguousarray(gold[name + "_x"])
        rows = x.shape[0]

        def build(g):
            return H.ggml_mul_mat(g.ctx, g.new(qt, [512, rows], blocks), g.new(L.F32, [512, rows], x))

        got = T.run_case(build, backend)[0].reshape(rows, rows)
        ref = gold[name + "_dot"]
        T.compare(f"golden mat-vec {name}", np.diag(got).astype(np.float64), ref, max_nmse=1e-10, log=plog)


def test_set_rows(backend, H, plog):
    rng = np.random.default_rng(15)
    src = (rng.standard_normal((7, 256)) * 50).astype(np.float32)
    idx = np.array([3, 0, 19, 5, 6, 31, 12], dtype=np.int64)
    for dt, npdt in ((L.F16, np.float16), (L.F32, np.float32)):
        base = rng.standard_normal((32, 256)).astype(npdt)

        def build(g):
            dst = g.new(dt, [256, 32], base)
            r = H.ggml_set_rows(g.ctx, dst, g.new(L.F32, [256, 7], src), g.new(L.I64, [7], idx))
            g.keep.append(dst)
            return [r, H.ggml_cont(g.ctx, dst)] if False else [r]

        # read back the whole destination through a second graph output: CONT of the destination after the scatter
        def build2(g):
            dst = g.new(dt, [256, 32], base)
            r = H.ggml_set_rows(g.ctx, dst, g.new(L.F32, [256, 7], src), g.new(L.I64, [7], idx))
            return [H.ggml_cont(g.ctx, r)]

        ref, got = both(build2, backend)
        bits = np.uint16 if dt == L.F16 else np.uint32
        T.compare(f"set_rows -> {QNAME[dt]}", got[0].view(bits), ref[0].view(bits), max_nmse=0.0, log=plog)
    # element scatter (transposed V cache): rows of one element
    vals = rng.standard_normal(40).astype(np.float32)
    eidx = rng.permutation(512)[:40].astype(np.int64)
    base = np.zeros((512, 1), np.float16)

    def build3(g):
        dst = g.new(L.F16, [1, 512], base)
        r = H.ggml_set_rows(g.ctx, dst, g.new(L.F32, [1, 40], vals.reshape(40, 1)), g.new(L.I64, [40], eidx))
        return [H.ggml_cont(g.ctx, r)]

    ref, got = both(build3, backend)
    T.compare("set_rows element scatter", got[0].view(np.uint16), ref[0].view(np.uint16), max_nmse=0.0, log=plog)


def test_cpy_q8_0_f32_roundtrip_for_k_shift(backend, H, plog):
    """K-shift of a quantised cache (llama.cpp build_rope_shift): cast(q8_0 view -> f32), in-place rope, cpy back (re-quantise)."""
    rng = np.random.default_rng(21)
    HD, NKV, NCTX = 128, 2, 40
    kc = T.rand_weight(L.Q8_0, NKV * HD, NCTX, rng)
    shift = rng.integers(-9, 3, NCTX).astype(np.int32)
    shift[::3] = 0

    def build(g):
        cache = g.new(L.Q8_0, [NKV * HD, NCTX], kc)
        k = H.ggml_view_3d(g.ctx, cache, HD, NKV, NCTX, HD // 32 * 34, NKV * HD // 32 * 34, 0)
        f = H.ggml_cast(g.ctx, k, L.F32)
        r = H.ggml_rope_ext_inplace(g.ctx, f, g.new(L.I32, [NCTX], shift), None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        return [H.ggml_cpy(g.ctx, r, k)]

    def build_cast_only(g):
        cache = g.new(L.Q8_0, [NKV * HD, NCTX], kc)
        k = H.ggml_view_3d(g.ctx, cache, HD, NKV, NCTX, HD // 32 * 34, NKV * HD // 32 * 34, 0)
        return [H.ggml_cast(g.ctx, k, L.F32)]

    ref, got = both(build_cast_only, backend)
    T.compare("cpy q8_0 -> f32", got[0].view(np.uint32), ref[0].view(np.uint32), max_nmse=0.0, log=plog)
    ref, got = both(build, backend)

    def deq(raw):
        blk = np.asarray(raw).reshape(-1, 34)
        return blk[:, :2].copy().view(np.float16).astype(np.float32) * blk[:, 2:].copy().view(np.int8).astype(np.float32)
    same = np.count_nonzero(np.asarray(got[0]) == np.asarray(ref[0]))
    plog(f"  q8_0 K-shift round trip: {same}/{np.asarray(ref[0]).size} bytes equal")
    # sin/cos differ from libm in the last bit here and there: a re-quantised code may then flip by one
    T.compare("cpy q8_0 -> f32 -> rope -> q8_0", deq(got[0]), deq(ref[0]), max_nmse=1e-5, log=plog)
    assert same >= 0.995 * np.asarray(ref[0]).size
    # cells with a zero shift are rotated by the identity: their re-quantised rows are pure integer work and match the oracle's
    rows0, rows0_ref = (np.asarray(t).reshape(NCTX, -1)[shift == 0] for t in (got[0], ref[0]))
    assert np.array_equal(rows0, rows0_ref)


def test_argmax(backend, H, plog):
    rng = np.random.default_rng(16)
    x = rng.standard_normal((5, 128256)).astype(np.float32)
    x[2, 77] = x[2, 90000] = 99.0  # tie -> first index

    def build(g):
        return H.ggml_argmax(g.ctx, g.new(L.F32, [128256, 5], x))

    ref, got = both(build, backend)
    T.compare("argmax", got[0], ref[0], max_nmse=0.0, log=plog)
    assert int(got[0].reshape(-1)[2]) == 77


# ------------------------------------------------------------------------------------------------ ROPE
@pytest.mark.parametrize("mode", [0, L.ROPE_NEOX])
@pytest.mark.parametrize("variant", ["plain", "freq_factors", "yarn", "partial"])
def test_rope(backend, H, plog, mode, variant):
    rng = np.random.default_rng(17 + mode)
    HD, NH, T_ = 128, 6, 9
    x = rng.standard_normal((T_, NH, HD)).astype(np.float32)
    pos = np.array([0, 1, 2, 3, 100, 2047, 4096, 8191, 30000], dtype=np.int32)
    ff = rng.uniform(1.0, 8.0, HD // 2).astype(np.float32)
    n_dims = 64 if variant == "partial" else HD
    ext, fscale, attn = (1.0, 0.25, 1.1) if variant == "yarn" else (0.0, 1.0, 1.0)

    def build(g):
        tx = g.new(L.F32, [HD, NH, T_], x)
        tp = g.new(L.I32, [T_], pos)
        tf = g.new(L.F32, [HD // 2], ff) if variant == "freq_factors" else None
        return H.ggml_rope_ext(g.ctx, tx, tp, tf, n_dims, mode, 8192, 500000.0, fscale, ext, attn, 32.0, 1.0)

    ref, got = both(build, backend)
    T.compare(f"rope mode={mode} {variant}", got[0], ref[0], max_nmse=1e-12, max_abs=5e-6, log=plog)


@pytest.mark.parametrize("dt", [L.F32, L.F16])
@pytest.mark.parametrize("case", ["mrope", "mrope_partial_ff", "vision", "vision_uneven", "mrope_empty_first"])
def test_rope_multi(backend, H, plog, case, dt):
    """ggml_rope_multi (llama-box/patches/llama.cpp/mrope.patch:5-41): Qwen2-VL style multimodal sections and the vision-tower
    mode with independently restarting sections; corner cases of the reference recurrence included."""
    import ctypes as C
    rng = np.random.default_rng(23)
    NH, NT = 3, 7
    HD, n_dims, sections, mode, ff = {
        "mrope": (128, 128, [16, 24, 24, 0], L.ROPE_MROPE, False),
        "mrope_partial_ff": (128, 96, [8, 12, 12, 4], L.ROPE_MROPE, True),       # rotated part < row, freq factors, 4th stream
        "vision": (80, 40, [20, 20, 20, 20], L.ROPE_VISION, False),
        "vision_uneven": (64, 32, [5, 9, 7, 3], L.ROPE_VISION, True),            # cycle of 24 pairs: sections repeat, angles restart
        "mrope_empty_first": (64, 64, [0, 10, 0, 6], L.ROPE_MROPE, False),
    }[case]
    npdt = np.float16 if dt == L.F16 else np.float32
    x = rng.standard_normal((NT, NH, HD)).astype(npdt)
    pos4 = rng.integers(0, 3000, 4 * NT).astype(np.int32)
    ffv = rng.uniform(0.8, 4.0, HD // 2).astype(np.float32)

    def build(g):
        sec = (C.c_int * 4)(*sections)
        return H.ggml_rope_multi(g.ctx, g.new(dt, [HD, NH, NT], x), g.new(L.I32, [4 * NT], pos4), g.new(L.F32, [HD // 2], ffv) if ff else None,
                                 n_dims, sec, mode, 32768, 1000000.0, 1.0, 0.0, 1.0, 32.0, 1.0)

    ref, got = both(build, backend)
    T.compare(f"rope_multi {case} {QNAME[dt]}", got[0].astype(np.float32), ref[0].astype(np.float32), max_nmse=1e-7 if dt == L.F16 else 1e-9, log=plog)


def test_rope_f16_kshift(backend, H, plog):
    """K-shift form: in-place-shaped rope on f16 data (llama-box context shift, httpserver.hpp:3453-3537)."""
    rng = np.random.default_rng(18)
    x = rng.standard_normal((5, 2, 128)).astype(np.float16)
    pos = np.array([-3, -3, 7, 0, 100], dtype=np.int32)

    def build(g):
        return H.ggml_rope_ext(g.ctx, g.new(L.F16, [128, 2, 5], x), g.new(L.I32, [5], pos), None, 128, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)

    ref, got = both(build, backend)
    g32, r32 = got[0].astype(np.float32), ref[0].astype(np.float32)
    T.compare("rope f16 (k-shift)", g32, r32, max_nmse=1e-7, log=plog)  # at most 1 f16 ulp where sin/cos differ in the last bit


# ------------------------------------------------------------------------------------------------ SOFT_MAX
@pytest.mark.parametrize("mask_t", [None, L.F16, L.F32])
@pytest.mark.parametrize("n,rows,heads", [(256, 3, 4), (1000, 1, 8), (8192, 2, 2), (33, 5, 12), (2304, 1, 32), (3000, 2, 2), (8200, 1, 3)])
def test_soft_max(backend, H, plog, mask_t, n, rows, heads):
    rng = np.random.default_rng(n + rows)
    x = (rng.standard_normal((heads, rows, n)) * 5).astype(np.float32)
    mask = np.where(rng.uniform(size=(64, n)) < 0.3, -np.inf, 0.0).astype(np.float32)
    mask[:, 0] = 0.0
    max_bias = 8.0 if (mask_t is not None and heads == 12) else 0.0

    def build(g):
        tx = g.new(L.F32, [n, rows, heads], x)
        tm = None
        if mask_t is not None:
            tm = g.new(mask_t, [n, 64], mask.astype(np.float16) if mask_t == L.F16 else mask)
        return H.ggml_soft_max_ext(g.ctx, tx, tm, 0.125, max_bias)

    ref, got = both(build, backend)
    T.compare(f"soft_max n={n} mask={mask_t} alibi={max_bias}", got[0], ref[0], max_nmse=1e-12, max_abs=1e-6, log=plog)


def test_soft_max_sinks_and_fully_masked(backend, H, plog):
    rng = np.random.default_rng(19)
    x = rng.standard_normal((4, 2, 128)).astype(np.float32)
    sinks = rng.standard_normal(4).astype(np.float32)
    mask = np.zeros((64, 128), np.float32)
    mask[1, :] = -np.inf  # a fully masked row: llama-box's patched soft_max must not abort (ggml-cpu.patch:5-15)

    def build(g):
        r = H.ggml_soft_max_ext(g.ctx, g.new(L.F32, [128, 2, 4], x), g.new(L.F32, [128, 64], mask), 1.0, 0.0)
        H.ggml_soft_max_add_sinks(r, g.new(L.F32, [4], sinks))
        return r

    ref, got = both(build, backend)
    T.compare("soft_max sinks + masked row", got[0], ref[0], max_nmse=1e-12, log=plog)


# ------------------------------------------------------------------------------------------------ FLASH_ATTN_EXT
FA_CASES = [  # (HD, NH, NKV, n_q, n_kv, splits, softcap, alibi, sinks)
    (128, 32, 8, 1, 256, 0, 0.0, 0.0, False),
    (128, 32, 8, 1, 2048, 0, 0.0, 0.0, False),
    (128, 28, 4, 1, 1024, 0, 0.0, 0.0, False),
    (64, 32, 4, 1, 512, 0, 0.0, 0.0, False),
    (128, 8, 8, 3, 256, 1, 0.0, 0.0, False),
    (128, 8, 2, 5, 512, 4, 30.0, 0.0, False),
    (64, 4, 2, 2, 256, 2, 0.0, 8.0, False),
    (128, 16, 2, 1, 768, 3, 0.0, 0.0, True),
    (64, 2, 1, 7, 256, 0, 0.0, 0.0, False),
    # lane-parallel decode kernel (head_dim 128, G = 2 / 4 / 7 / 8): several trips per split, ragged split ends, sinks
    (128, 8, 4, 2, 512, 0, 0.0, 0.0, False),
    (128, 32, 8, 1, 2048, 2, 0.0, 0.0, False),
    (128, 32, 8, 3, 1000, 3, 0.0, 0.0, True),
    (128, 28, 4, 2, 1024, 5, 0.0, 0.0, False),
    (128, 16, 2, 4, 300, 1, 0.0, 0.0, True),
    # the same kernel on head_dim 64 (eight-lane K / V rows; G = 4 / 8; TinyLlama, Llama-3.2-1B shapes): one split on four waves, several on eight, ragged ends, sinks
    (64, 32, 4, 1, 600, 1, 0.0, 0.0, False),
    (64, 32, 4, 1, 2048, 5, 0.0, 0.0, True),
    (64, 32, 4, 1, 4096, 0, 0.0, 0.0, False),
    (64, 32, 8, 1, 1000, 3, 0.0, 0.0, False),
    (64, 16, 4, 1, 300, 1, 0.0, 0.0, True),
    (64, 32, 8, 1, 3072, 0, 0.0, 0.0, False),  # (longer random caches leave the 1e-4 gate on the ORACLE side: its f16 V accumulator, 1.7e-4 at 8192 cells with either kernel)
    (64, 8, 2, 1, 68, 2, 0.0, 0.0, False),
    # query heads per KV head other than 2 / 4 / 7 / 8 (round 6; until then FLASH_ATTN_EXT of such models stayed on the CPU backend): 3 (Llama-3.2-3B: 24 / 8), 5, 6
    # (Qwen2.5-1.5B: 12 / 2) on the lane-parallel kernel in the next power of two's form, at both head sizes; soft-capped / ALiBi on the generic kernel; a prompt batch
    (128, 32, 32, 1, 1024, 0, 0.0, 0.0, False),   # multi-head attention (Llama-2-7B): the two-head template with one real head
    (64, 16, 16, 1, 512, 2, 0.0, 0.0, True),
    (128, 8, 8, 5, 300, 3, 0.0, 0.0, False),
    (128, 24, 8, 1, 1024, 0, 0.0, 0.0, False),
    (128, 12, 2, 1, 700, 3, 0.0, 0.0, True),
    (128, 20, 4, 3, 512, 2, 0.0, 0.0, False),
    (128, 24, 8, 1, 333, 1, 0.0, 0.0, False),
    (128, 24, 8, 2, 256, 2, 30.0, 0.0, False),
    (128, 12, 2, 4, 300, 0, 0.0, 8.0, False),
    (128, 24, 8, 64, 512, 0, 0.0, 0.0, False),
    (64, 14, 2, 1, 900, 0, 0.0, 0.0, False),
    (64, 24, 8, 1, 600, 2, 0.0, 0.0, True),
    (64, 8, 4, 1, 300, 1, 0.0, 0.0, False),
    (64, 12, 2, 1, 2048, 0, 0.0, 0.0, False),
    (64, 24, 8, 3, 256, 2, 20.0, 0.0, False),
    (64, 20, 4, 40, 256, 0, 0.0, 0.0, False),
    # >= 32 query tokens: the matrix-core kernel (fattn_mma.hip); ragged query tiles, fully-masked KV tiles, KV tails
    (128, 32, 8, 64, 512, 0, 0.0, 0.0, False),
    (128, 8, 2, 200, 256, 0, 0.0, 0.0, False),
    (128, 4, 4, 33, 260, 0, 0.0, 0.0, False),
    (64, 4, 2, 96, 256, 0, 0.0, 0.0, False),
    (64, 8, 1, 130, 1024, 0, 0.0, 0.0, False),
    (128, 4, 2, 40, 256, 2, 20.0, 0.0, False),  # softcap -> falls back to the split-KV kernel
    # matrix-core kernel with the KV range split over workgroups (+ combine): -np 32 style batches over a long unified cache
    (128, 32, 8, 32, 2048, 4, 0.0, 0.0, False),
    (128, 8, 2, 40, 1024, 0, 0.0, 0.0, False),
    (64, 4, 2, 96, 512, 3, 0.0, 0.0, False),
    (128, 16, 4, 33, 1100, 5, 0.0, 0.0, False),
    # ... with >= 2048 (token, head) rows: the row-parallel combine pass of prompt micro-batches (k_fattn_combine_rows, 4- and 8-split forms)
    (128, 32, 8, 64, 1024, 4, 0.0, 0.0, False),
    (128, 32, 4, 80, 768, 6, 0.0, 0.0, False),
]


@pytest.mark.parametrize("HD,NH,NKV,nq,nkv,splits,softcap,alibi,sinks", FA_CASES)
def test_flash_attn(backend, H, plog, HD, NH, NKV, nq, nkv, splits, softcap, alibi, sinks):
    rng = np.random.default_rng(HD + NH + nkv)
    NCTX = nkv + 256
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)
    kc = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    MR = (max(nq, 1) + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nq):
        mask[t, : nkv - nq + t + 1 - 17] = 0  # causal-ish with a masked tail (padding cells)
        mask[t, 5] = -np.inf                  # a hole (cell of another sequence)
    sk = rng.standard_normal(NH).astype(np.float32)
    backend.set_option("fa_splits", splits)

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        k_cache = g.new(L.F16, [NKV * HD, NCTX], kc)
        v_cache = g.new(L.F16, [NKV * HD, NCTX], vc)
        k = H.ggml_view_3d(g.ctx, k_cache, HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, v_cache, HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), alibi, softcap)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        if sinks:
            H.ggml_flash_attn_ext_add_sinks(r, g.new(L.F32, [NH], sk))
        return r

    try:
        ref, got = both(build, backend)
    finally:
        backend.set_option("fa_splits", 0)
    T.compare(f"flash_attn D={HD} H={NH}/{NKV} nq={nq} nkv={nkv} splits={splits} cap={softcap} alibi={alibi} sinks={sinks}", got[0], ref[0], max_nmse=1e-4, log=plog)
    # and against exact (float64) attention: the f32-accumulating kernel must be CLOSER to it than the f16-accumulating CPU path
    kf = kc[:nkv].astype(np.float64).reshape(nkv, NKV, HD)
    vf = vc[:nkv].astype(np.float64).reshape(nkv, NKV, HD)
    exact = np.zeros((nq, NH, HD))
    n2 = 1 << int(np.floor(np.log2(NH)))
    for h in range(NH):
        slope = 1.0
        if alibi > 0:
            slope = (2.0 ** (-alibi / n2)) ** (h + 1) if h < n2 else (2.0 ** (-alibi / 2 / n2)) ** (2 * (h - n2) + 1)
        for t in range(nq):
            s = kf[:, h // (NH // NKV)] @ q[h, t].astype(np.float16).astype(np.float64) / np.sqrt(HD)
            if softcap:
                s = softcap * np.tanh(s / softcap)
            s = s + slope * mask[t].astype(np.float64)
            m = s.max()
            if sinks:
                m = max(m, float(sk[h]))
            p = np.exp(s - m)
            den = p.sum() + (np.exp(float(sk[h]) - m) if sinks else 0.0)
            exact[t, h] = (p @ vf[:, h // (NH // NKV)]) / den
    e_gpu, e_cpu = T.nmse(got[0].reshape(nq, NH, HD), exact), T.nmse(ref[0].reshape(nq, NH, HD), exact)
    plog(f"    vs exact attention: kernel nmse={e_gpu:.3e}  cpu-oracle nmse={e_cpu:.3e}")
    # (the matrix-core kernel rounds P to f16 once per element; the CPU path rounds the whole V accumulator every step)
    assert e_gpu <= (1e-9 if nq < 32 or softcap else 3e-7) and e_gpu <= e_cpu * 1.01 + 1e-12


def _random_fa_cases():
    rng = np.random.default_rng(77)
    heads = [(32, 8), (28, 4), (8, 2), (16, 2), (8, 8), (4, 2)]
    out = []
    for i in range(28):
        NH, NKV = heads[int(rng.integers(len(heads)))]
        nq = int(rng.choice([1, 2, 3, 5, 8, 16, 31, 32, 33, 48, 64, 65, 130]))
        nkv = int(rng.integers(8, 700)) * 4
        nseq = int(rng.choice([1, 1, 2, 4, 8]))
        out.append((128, NH, NKV, nq, nkv, nseq, i))
    # round 6: head_dim 64 and every number of query heads per KV head from 1 to 8, at both head sizes (own generator: the 28 cases above stay what they were)
    rng = np.random.default_rng(78)
    heads = [(32, 4), (32, 8), (24, 8), (12, 2), (20, 4), (14, 2), (8, 8), (6, 1), (16, 8)]
    for i in range(28, 64):
        NH, NKV = heads[int(rng.integers(len(heads)))]
        HD = int(rng.choice([64, 64, 128]))
        nq = int(rng.choice([1, 1, 2, 3, 5, 8, 16, 31, 32, 33, 48, 65]))
        nkv = int(rng.integers(8, 700)) * 4
        nseq = int(rng.choice([1, 1, 2, 4, 8]))
        out.append((HD, NH, NKV, nq, nkv, nseq, i))
    return out


@pytest.mark.parametrize("HD,NH,NKV,nq,nkv,nseq,case", _random_fa_cases())
def test_flash_attn_random_masks(backend, H, plog, HD, NH, NKV, nq, nkv, nseq, case):
    """Seeded sweep at head_dim 128 (and, round 6, 64; 1 .. 8 query heads per KV head): query counts on both sides of every kernel boundary (1 / 2..32 position
    lists / >= 33 matrix cores), ragged cache lengths, one or several sequences in a unified cache (each query sees a random causal prefix of its own
    sequence's scattered cells — whole tiles and whole splits with nothing visible) — against the oracle."""
    rng = np.random.default_rng(1000 + case)
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    MR = (nq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    owner = rng.integers(0, nseq, nkv)               # which sequence a cell belongs to
    if nseq > 1:                                      # contiguous runs, like a unified cache after several prompts
        owner = np.sort(owner)
    for t in range(nq):
        cells = np.flatnonzero(owner == (t % nseq))
        if cells.size == 0:
            cells = np.arange(min(4, nkv))
        n_vis = int(rng.integers(1, cells.size + 1))
        mask[t, cells[:n_vis]] = 0
    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], vc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    ref, got = both(build, backend)
    T.compare(f"flash_attn random D={HD} H={NH}/{NKV} nq={nq} nkv={nkv} nseq={nseq}", got[0], ref[0], max_nmse=1e-4, log=plog)


# quantised KV cache (-ctk q8_0 -ctv q8_0): SET_ROWS quantises f32 rows into block_q8_0, FLASH_ATTN_EXT reads the blocks
FA_Q8_CASES = [  # (NH, NKV, n_q, n_kv, splits, sinks)
    (32, 8, 1, 256, 0, False),
    (32, 8, 1, 2048, 0, False),
    (32, 8, 1, 1000, 3, True),
    (28, 4, 1, 1024, 0, False),
    (28, 4, 2, 700, 5, False),
    (16, 2, 1, 768, 0, True),
    (16, 2, 4, 300, 1, False),
    (8, 4, 3, 512, 2, False),
    (8, 8, 1, 512, 0, False),     # 1 (multi-head attention), 3, 6, 5 query heads per KV head (round 6)
    (16, 16, 3, 400, 2, True),
    (24, 8, 1, 1024, 0, False),
    (12, 2, 2, 600, 3, True),
    (20, 4, 1, 333, 1, False),
    # prompt batches (>= 32 query tokens): the cells are expanded to f16 and the matrix-core kernel runs on that image
    (32, 8, 40, 512, 0, False),
    (32, 8, 200, 1024, 0, False),
    (28, 4, 33, 260, 3, False),
    (8, 2, 64, 2048, 4, False),
    (16, 2, 40, 300, 0, True),    # sinks: not a matrix-core case -> per-token lane-parallel passes over the blocks
]


@pytest.mark.parametrize("NH,NKV,nq,nkv,splits,sinks", FA_Q8_CASES)
def test_flash_attn_q8_0_kv(backend, H, plog, NH, NKV, nq, nkv, splits, sinks):
    HD = 128
    rng = np.random.default_rng(NH * 3 + nkv + nq)
    NCTX = nkv + 64
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)
    kf = (rng.standard_normal((nkv, NKV * HD)) * rng.uniform(0.3, 2.0, (nkv, 1))).astype(np.float32)
    vf = (rng.standard_normal((nkv, NKV * HD)) * rng.uniform(0.3, 2.0, (nkv, 1))).astype(np.float32)
    kf[3, :64] = 0.0  # all-zero blocks: d = 0
    rows = rng.permutation(NCTX)[:nkv].astype(np.int64)
    rows.sort()
    rows[: nkv] = np.arange(nkv)  # the view reads cells [0, nkv)
    MR = (nq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nq):
        mask[t, : nkv - nq + t + 1 - 9] = 0
        mask[t, 5] = -np.inf
    sk = rng.standard_normal(NH).astype(np.float32)
    rb = NKV * HD // 32 * 34  # bytes per cache row
    backend.set_option("fa_splits", splits)

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        k_cache = g.new(L.Q8_0, [NKV * HD, NCTX])
        v_cache = g.new(L.Q8_0, [NKV * HD, NCTX])
        idx = g.new(L.I64, [nkv], rows)
        ks = H.ggml_set_rows(g.ctx, k_cache, g.new(L.F32, [NKV * HD, nkv], kf), idx)
        vs = H.ggml_set_rows(g.ctx, v_cache, g.new(L.F32, [NKV * HD, nkv], vf), idx)
        k = H.ggml_view_3d(g.ctx, ks, HD, nkv, NKV, rb, HD // 32 * 34, 0)
        v = H.ggml_view_3d(g.ctx, vs, HD, nkv, NKV, rb, HD // 32 * 34, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        if sinks:
            H.ggml_flash_attn_ext_add_sinks(r, g.new(L.F32, [NH], sk))
        return [r, ks, vs]

    try:
        ref, got = both(build, backend)
    finally:
        backend.set_option("fa_splits", 0)
    # the cache contents are integer work: byte-exact (rows [0, nkv) were written, the rest stays zero)
    for name, i in (("K", 1), ("V", 2)):
        assert np.array_equal(got[i], ref[i]), f"set_rows -> q8_0 {name} cache differs in {np.count_nonzero(got[i] != ref[i])} bytes"
    plog(f"  set_rows -> q8_0 cache {NKV * HD}x{nkv}: byte-exact")
    name = f"flash_attn q8_0 KV H={NH}/{NKV} nq={nq} nkv={nkv} splits={splits} sinks={sinks}"
    if nq < 32 or sinks:
        # same arithmetic as the CPU: queries quantised to Q8_0, integer block dots, f32 softmax / V accumulation
        T.compare(name, got[0], ref[0], max_nmse=1e-6, log=plog)
        return
    # matrix-core path: f16 queries against the dequantised cells.  The CPU's 8-bit queries are the larger approximation, so
    # the gate is exact (float64) attention over the dequantised cache: the kernel must be at least as close to it as the CPU
    def deq(raw):
        blk = np.asarray(raw).reshape(-1, 34)
        return (blk[:, :2].copy().view(np.float16).astype(np.float64) * blk[:, 2:].copy().view(np.int8).astype(np.float64)).reshape(NCTX, NKV, HD)
    kd, vd = deq(ref[1])[:nkv], deq(ref[2])[:nkv]
    exact = np.zeros((nq, NH, HD))
    for h in range(NH):
        kh, vh = kd[:, h // (NH // NKV)], vd[:, h // (NH // NKV)]
        sc = (q[h].astype(np.float64) @ kh.T) / np.sqrt(HD) + mask[:nq].astype(np.float64)
        sc -= sc.max(axis=1, keepdims=True)
        pr = np.exp(sc)
        exact[:, h] = (pr @ vh) / pr.sum(axis=1, keepdims=True)
    e_gpu, e_cpu = T.nmse(got[0].reshape(nq, NH, HD), exact), T.nmse(ref[0].reshape(nq, NH, HD), exact)
    T.compare(name, got[0], ref[0], max_nmse=1e-3, log=plog)
    plog(f"    vs exact attention over the dequantised cache: kernel nmse={e_gpu:.3e}  cpu-oracle nmse={e_cpu:.3e}")
    assert e_gpu <= 6e-7 and e_gpu <= e_cpu * 1.01 + 1e-12  # (f16 rounding of P: ~3e-7)


@pytest.mark.parametrize("HD,NH,NKV,nseq,per_seq", [(128, 32, 8, 32, 64), (128, 8, 2, 12, 100), (128, 28, 4, 5, 300), (128, 16, 2, 48, 48), (64, 8, 2, 16, 64), (64, 32, 4, 32, 40), (64, 32, 8, 12, 100),
                                                    (64, 32, 4, 5, 700), (128, 24, 8, 16, 64), (64, 24, 8, 16, 64), (128, 12, 2, 9, 120), (64, 14, 2, 32, 30), (128, 8, 8, 16, 64), (64, 8, 8, 12, 50)])
def test_flash_attn_continuous_batching_mask(backend, H, plog, HD, NH, NKV, nseq, per_seq):
    """-np style decode batch: token i belongs to sequence i and sees only that sequence's cells of the unified cache (a block-diagonal
    mask).  The decode kernel reads the mask of its split first and skips KV trips no position of which is visible."""
    rng = np.random.default_rng(HD + NH + nseq + per_seq)
    nkv = (nseq * per_seq + 255) // 256 * 256
    q = rng.standard_normal((NH, nseq, HD)).astype(np.float32)
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    MR = (nseq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nseq):
        mask[t, t * per_seq: t * per_seq + per_seq - (t % 7)] = 0  # ragged sequence lengths

    def build(g):
        tq = g.new(L.F32, [HD, nseq, NH], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], vc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    s0 = backend.stat("fa_list_launches")
    ref, got = both(build, backend)
    T.compare(f"flash_attn block-diagonal D={HD} H={NH}/{NKV} nseq={nseq} per_seq={per_seq}", got[0], ref[0], max_nmse=1e-4, log=plog)
    if nseq <= 32:  # 2 .. 32 tokens walk position lists — at head_dim 64 (G = 4 / 8) too since round 6
        assert backend.stat("fa_list_launches") > s0


@pytest.mark.parametrize("upstream_cast", [False, True])
def test_flash_attn_draft_batch_over_a_large_unified_cache_walks_position_lists(backend, H, plog, upstream_cast):
    """upstream_cast: the graph llama.cpp emits — KQ_mask is an F32 input and FLASH_ATTN_EXT reads ggml_cast(KQ_mask, F16), a CPY node's output that never
    passed through set_tensor; the statistics are found through the cast's source (VERDICT r04 weak #3 / ADVICE r04).
    32 sequences x 5 positions (sampled token + 4 drafts: llama-box's verification batch) over a 10 k-cell unified cache: the mask — 192 rows
    x 10 240 cells, 3.9 MB, named KQ_mask as in llama.cpp's graphs — is sparse, its statistics are taken when it is uploaded, and the batch
    walks per-token position lists instead of multiplying every tile through the whole cache (round 4's first cut stopped looking at 2 MiB
    and lost exactly the bench's `--np 32 --draft 4` line)."""
    HD, NH, NKV, nseq, T1, per_seq = 128, 32, 8, 32, 5, 300
    nq, nkv = nseq * T1, 10240
    rng = np.random.default_rng(4242)
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    MR = (nq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for sq in range(nseq):
        for j in range(T1):
            mask[sq * T1 + j, sq * per_seq: sq * per_seq + per_seq - 8 + j] = 0  # the sequence's cells up to this position
    assert mask.nbytes > (2 << 20)

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], vc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        if upstream_cast:
            m = H.ggml_cast(g.ctx, g.new(L.F32, [nkv, MR], mask.astype(np.float32), name="KQ_mask"), L.F16)
        else:
            m = g.new(L.F16, [nkv, MR], mask, name="KQ_mask")
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    n0 = backend.stat("fa_list_launches")
    ref, got = both(build, backend)
    assert backend.stat("fa_list_launches") == n0 + 1
    T.compare(f"flash_attn draft batch 32 x 5 over 10240 cells{' (F32 mask + cast, as llama.cpp builds it)' if upstream_cast else ''}", got[0], ref[0], max_nmse=1e-4, log=plog)


@pytest.mark.parametrize("nseq,per_seq,nkv_dec", [(32, 64, 0), (5, 300, 0), (1, 0, 2100), (1, 0, 8192)])
def test_flash_attn_self_merging_splits(backend, H, plog, nseq, per_seq, nkv_dec):
    """Option fa_self_merge (off by default — measured slower for one token, +1 % for -np 32): the last split workgroup of a
    (token, kv head) merges the partial records itself (arrival counter, agent-scope record stores / loads) instead of a combine
    launch.  Same result as the two-launch form, the counters are back at zero afterwards (the second run checks that)."""
    HD, NH, NKV = 128, 32, 8
    rng = np.random.default_rng(nseq * 7 + per_seq + nkv_dec)
    nkv = nkv_dec if nseq == 1 else (nseq * per_seq + 255) // 256 * 256
    q = rng.standard_normal((NH, nseq, HD)).astype(np.float32)
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    MR = (nseq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nseq):
        if nseq == 1:
            mask[0, : nkv - 37] = 0
        else:
            mask[t, t * per_seq: t * per_seq + per_seq - (t % 7)] = 0

    def build(g):
        tq = g.new(L.F32, [HD, nseq, NH], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], vc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    ref = T.run_case(build, "oracle")
    two = T.run_case(build, backend)
    backend.set_option("fa_self_merge", 1)
    try:
        k0 = backend.stat("kernel_launches")
        one = T.run_case(build, backend)
        launches = backend.stat("kernel_launches") - k0
        again = T.run_case(build, backend)
    finally:
        backend.set_option("fa_self_merge", 0)
    # (8192 cells: the CPU's f16 accumulation of V alone is ~1.7e-4 away from exact attention — test_flash_attn_head_dim_128_at_8192)
    T.compare(f"flash_attn self-merging splits nseq={nseq} nkv={nkv}", one[0], ref[0], max_nmse=1e-4 if nkv <= 4096 else 3e-4, log=plog)
    T.compare(f"flash_attn self-merging splits nseq={nseq} nkv={nkv} vs combine launch", one[0], two[0], max_nmse=1e-12, log=plog)
    assert np.array_equal(one[0], again[0])
    plog(f"    self-merging attention nseq={nseq} nkv={nkv}: {launches} launches")


@pytest.mark.parametrize("nseq,per_seq,splits", [(32, 64, 0), (32, 192, 1), (32, 192, 3), (12, 100, 0), (5, 700, 0)])
def test_flash_attn_feeds_quantised_wo(backend, H, plog, nseq, per_seq, splits):
    """-np decode: attention over a unified cache whose only reader is the quantised wo mat-mul.  The attention kernel leaves Q8_K
    blocks (two heads each) instead of f32 — from its single pass when the position lists are short (no combine launch), from the
    combine pass otherwise — and the skinny mat-mul reads them.  Equal to the oracle's f32 attention -> quantise -> mat-mul within
    the attention gate (the quantisation sees values a few 1e-7 apart: a Q8 code may flip, worth ~1e-5 of the mat-mul's output)."""
    HD, NH, NKV, E = 128, 32, 8, 4096
    rng = np.random.default_rng(nseq * 13 + per_seq + splits)
    nkv = (nseq * per_seq + 255) // 256 * 256
    q = rng.standard_normal((NH, nseq, HD)).astype(np.float32)
    kc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    vc = rng.standard_normal((nkv, NKV * HD)).astype(np.float16)
    MR = (nseq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nseq):
        cells = rng.choice(nkv, per_seq - (t % 7), replace=False)  # scattered, as the decode cells of interleaved sequences are
        mask[t, cells] = 0
    wo = T.rand_weight(L.Q4_K, E, 512, rng)

    def build(g):
        tq = g.new(L.F32, [HD, nseq, NH], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], kc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * HD, nkv], vc), HD, nkv, NKV, NKV * HD * 2, HD * 2, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [E, 512], wo), H.ggml_reshape_2d(g.ctx, r, E, nseq))

    ref = T.run_case(build, "oracle", T.host_threads(16))
    backend.set_option("fa_splits", splits)
    try:
        k0 = backend.stat("kernel_launches")
        got = T.run_case(build, backend)
        launches = backend.stat("kernel_launches") - k0
    finally:
        backend.set_option("fa_splits", 0)
    plog(f"    attention -> wo nseq={nseq} per_seq={per_seq} splits={splits}: {launches} launches")
    T.compare(f"flash_attn -> q8 -> wo nseq={nseq} per_seq={per_seq} splits={splits}", got[0], ref[0], max_nmse=1e-4, log=plog)


# ------------------------------------------------------------------------------------------------ fused Q/K/V
@pytest.mark.parametrize("tq,tv,bias", [(L.Q4_K, L.Q4_K, False), (L.Q4_K, L.Q6_K, False), (L.Q5_K, L.Q6_K, True), (L.Q6_K, L.Q6_K, True), (L.Q4_K, L.Q5_K, False), (L.Q8_0, L.Q8_0, False), (L.Q8_0, L.Q8_0, True)])
@pytest.mark.parametrize("kvt", [L.F16, L.Q8_0])
def test_fused_qkv_rope_store(backend, H, plog, tq, tv, bias, kvt):
    """One decode token through norm -> {wq, wk, wv} -> (+bias) -> rope(q, k) -> KV-cache store, the node pattern of
    llama_lite / llm_build_llama.  wq/wk in one K-quant format and wv in another take ONE launch (qkv.hip gives each
    format its own workgroups); result must equal the oracle and the unfused execution."""
    rng = np.random.default_rng(5 + tq * 7 + tv)
    E, HD, NH, NKV, NCTX, slot, pos = 1024, 128, 8, 2, 32, 11, 7
    x = rng.standard_normal((1, E)).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, E).astype(np.float32)
    wq, wk, wv = T.rand_weight(tq, E, NH * HD, rng), T.rand_weight(tq, E, NKV * HD, rng), T.rand_weight(tv, E, NKV * HD, rng)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) for n in (NH * HD, NKV * HD, NKV * HD))
    if kvt == L.F16:
        kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
        vc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    else:  # quantised KV cache: the launch assembles block_q8_0 rows (16 row pairs of a workgroup = one block)
        kc0 = T.rand_weight(L.Q8_0, NKV * HD, NCTX, rng)
        vc0 = T.rand_weight(L.Q8_0, NKV * HD, NCTX, rng)

    def deq(t):
        if kvt == L.F16:
            return np.asarray(t).astype(np.float32)
        if np.asarray(t).dtype != np.uint8:
            return np.asarray(t).astype(np.float32)
        blk = np.asarray(t).reshape(-1, 34)
        return blk[:, :2].copy().view(np.float16).astype(np.float32) * blk[:, 2:].copy().view(np.int8).astype(np.float32)

    def build(g):
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [E, 1], x), 1e-5), g.new(L.F32, [E], nw))
        q = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NH * HD], wq), cur)
        k = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NKV * HD], wk), cur)
        v = H.ggml_mul_mat(g.ctx, g.new(tv, [E, NKV * HD], wv), cur)
        if bias:
            q = H.ggml_add(g.ctx, q, g.new(L.F32, [NH * HD], bq))
            k = H.ggml_add(g.ctx, k, g.new(L.F32, [NKV * HD], bk))
            v = H.ggml_add(g.ctx, v, g.new(L.F32, [NKV * HD], bv))
        tp = g.new(L.I32, [1], np.array([pos], np.int32))
        idx = g.new(L.I64, [1], np.array([slot], np.int64))
        q = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, q, HD, NH, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, k, HD, NKV, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        v = H.ggml_reshape_3d(g.ctx, v, HD, NKV, 1)
        ks = H.ggml_set_rows(g.ctx, g.new(kvt, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, k, NKV * HD, 1), idx)
        vs = H.ggml_set_rows(g.ctx, g.new(kvt, [NKV * HD, NCTX], vc0), H.ggml_reshape_2d(g.ctx, v, NKV * HD, 1), idx)
        return [q, ks, vs]

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("fusion", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("fusion", 1)
    plog(f"    fused qkv {QNAME[tq]}/{QNAME[tv]} bias={bias} cache={QNAME[kvt]}: {launches} kernel launch(es)")
    assert launches == 2, launches  # the token's (cos, sin) table — once per graph run, shared by all layers — and the fused launch
    # (a Q8_0 cache row: one rounding flip of a code is 1/127 of the block's range, hence the looser bound against the oracle;
    # fused and unfused GPU paths do the same arithmetic and must agree byte for byte)
    tol_cache = 1e-6 if kvt == L.F16 else 1e-4
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache"), got, ref, plain):
        a32, b32, c32 = deq(a), deq(b), deq(c)
        T.compare(f"fused qkv {QNAME[tq]}/{QNAME[tv]} {name}", a32, b32, max_nmse=tol_cache if name != "q_rope" else 1e-10, log=plog)
        T.compare(f"fused qkv {QNAME[tq]}/{QNAME[tv]} {name} vs unfused", a32, c32, max_nmse=tol_cache if name != "q_rope" else 1e-10, log=plog)
        if kvt == L.Q8_0 and name != "q_rope":
            assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: fused and unfused q8_0 cache rows differ"


@pytest.mark.parametrize("tq,tv", [(L.Q4_K, L.Q4_K), (L.Q4_K, L.Q6_K), (L.Q5_K, L.Q6_K)])
def test_fused_qkv_transposed_v_store(backend, H, plog, tq, tv):
    """The non-flash path keeps V transposed: llama.cpp views the projection as n_embd_v rows of ONE element and scatters them with an
    index per element (j * n_ctx + cell).  The fused decode launch does that scatter in its epilogue: still one launch, same bytes."""
    rng = np.random.default_rng(9 + tq * 7 + tv)
    E, HD, NH, NKV, NCTX, slot, pos = 1024, 128, 8, 2, 64, 37, 7
    x = rng.standard_normal((1, E)).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, E).astype(np.float32)
    wq, wk, wv = T.rand_weight(tq, E, NH * HD, rng), T.rand_weight(tq, E, NKV * HD, rng), T.rand_weight(tv, E, NKV * HD, rng)
    kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc0 = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    v_idx = (np.arange(NKV * HD, dtype=np.int64) * NCTX + slot)

    def build(g):
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [E, 1], x), 1e-5), g.new(L.F32, [E], nw))
        q = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NH * HD], wq), cur)
        k = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NKV * HD], wk), cur)
        v = H.ggml_mul_mat(g.ctx, g.new(tv, [E, NKV * HD], wv), cur)
        tp = g.new(L.I32, [1], np.array([pos], np.int32))
        idx = g.new(L.I64, [1], np.array([slot], np.int64))
        vidx = g.new(L.I64, [NKV * HD], v_idx)
        q = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, q, HD, NH, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, k, HD, NKV, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        v = H.ggml_reshape_3d(g.ctx, v, HD, NKV, 1)
        ks = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, k, NKV * HD, 1), idx)
        v_view = H.ggml_reshape_2d(g.ctx, g.new(L.F16, [NCTX, NKV * HD], vc0), 1, NCTX * NKV * HD)
        vs = H.ggml_set_rows(g.ctx, v_view, H.ggml_reshape_2d(g.ctx, v, 1, NKV * HD), vidx)
        return [q, ks, vs]

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("fusion", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("fusion", 1)
    plog(f"    fused qkv {QNAME[tq]}/{QNAME[tv]} with the transposed V cache: {launches} kernel launch(es)")
    assert launches == 2, launches  # the token's (cos, sin) table (once per graph run) + the fused launch
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache_T"), got, ref, plain):
        a32, b32, c32 = (np.asarray(t).astype(np.float32) for t in (a, b, c))
        T.compare(f"fused qkv {QNAME[tq]}/{QNAME[tv]} transposed V: {name}", a32, b32, max_nmse=1e-10 if name == "q_rope" else 1e-6, log=plog)
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: fused and node-by-node execution differ"
    vt = np.asarray(got[2]).reshape(NKV * HD, NCTX)
    assert np.array_equal(np.delete(vt, slot, axis=1), np.delete(vc0, slot, axis=1)), "cells of other tokens were touched"


@pytest.mark.parametrize("tq,tv,M,n_dims,bias", [(L.Q4_K, L.Q4_K, 32, 128, False), (L.Q4_K, L.Q6_K, 32, 128, False), (L.Q4_K, L.Q6_K, 7, 128, True),
                                                  (L.Q5_K, L.Q5_K, 19, 64, False), (L.Q6_K, L.Q6_K, 32, 128, True), (L.Q5_K, L.Q6_K, 32, 128, False), (L.Q5_K, L.Q6_K, 3, 64, True)])
def test_np_batch_qkv_rope_store_in_the_gemm_epilogue(backend, H, plog, tq, tv, M, n_dims, bias):
    """-np decode step (3..32 tokens): wq / wk / wv -> (+bias) -> rope(q, k) -> KV-cache stores.  ONE skinny launch — also when wv is
    stored in another K-quant format than wq / wk (Q4_K_M: Q6_K in half the layers; the kernel serves two formats in two passes) —
    rotates and stores in its epilogue: no rope launch, the f32 projections are never written.  Equal to the oracle, and to the
    unfused execution bit for bit (same mat-mul arithmetic per tile, same rope arithmetic element for element)."""
    rng = np.random.default_rng(77 + tq * 7 + tv + M)
    E, HD, NH, NKV, NCTX = 1024, 128, 8, 2, 300
    x = rng.standard_normal((M, E)).astype(np.float32)
    wq, wk, wv = T.rand_weight(tq, E, NH * HD, rng), T.rand_weight(tq, E, NKV * HD, rng), T.rand_weight(tv, E, NKV * HD, rng)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) for n in (NH * HD, NKV * HD, NKV * HD))
    kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    pos = rng.integers(0, 5000, M).astype(np.int32)
    rows = rng.permutation(NCTX)[:M].astype(np.int64)

    def build(g):
        cur = g.new(L.F32, [E, M], x)
        q = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NH * HD], wq), cur)
        k = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NKV * HD], wk), cur)
        v = H.ggml_mul_mat(g.ctx, g.new(tv, [E, NKV * HD], wv), cur)
        if bias:
            q = H.ggml_add(g.ctx, q, g.new(L.F32, [NH * HD], bq))
            k = H.ggml_add(g.ctx, k, g.new(L.F32, [NKV * HD], bk))
            v = H.ggml_add(g.ctx, v, g.new(L.F32, [NKV * HD], bv))
        tp = g.new(L.I32, [M], pos)
        idx = g.new(L.I64, [M], rows)
        q = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, q, HD, NH, M), tp, None, n_dims, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, k, HD, NKV, M), tp, None, n_dims, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        ks = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, k, NKV * HD, M), idx)
        vs = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], vc0), v, idx)
        return [q, ks, vs]

    ref = T.run_case(build, "oracle", expand_first=())
    e0, k0 = backend.stat("rope_epilogues"), backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    epilogues, launches = backend.stat("rope_epilogues") - e0, backend.stat("kernel_launches") - k0
    backend.set_option("skinny_rope", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("skinny_rope", 1)
    plog(f"    np batch qkv {QNAME[tq]}/{QNAME[tv]} M={M} n_dims={n_dims} bias={bias}: {launches} launches, {epilogues} rope epilogue(s)")
    assert epilogues == 1, epilogues
    assert launches == 3, launches  # the activations' quantiser + the (cos, sin) table of the batch (once per graph run) + the one mat-mul launch
    if tq != tv:  # the two-format launch against the one-format launches it replaces (wq / wk together, wv alone, rope + stores)
        backend.set_option("skinny_mix", 0)
        try:
            k1 = backend.stat("kernel_launches")
            apart = T.run_case(build, backend)
            launches_apart = backend.stat("kernel_launches") - k1
        finally:
            backend.set_option("skinny_mix", 1)
        assert launches_apart > launches, (launches_apart, launches)
        for name, a, c in zip(("q_rope", "k_cache", "v_cache"), got, apart):
            assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: two-format launch and separate launches differ"
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache"), got, ref, plain):
        a32, b32, c32 = (np.asarray(t).astype(np.float32) for t in (a, b, c))
        T.compare(f"np batch qkv {QNAME[tq]}/{QNAME[tv]} M={M} {name}", a32, b32, max_nmse=1e-10 if name == "q_rope" else 1e-6, log=plog)
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: epilogue and separate rope launch differ"


@pytest.mark.parametrize("mode,n_dims,T_", [(0, 128, 32), (L.ROPE_NEOX, 128, 5), (0, 64, 130), (0, 128, 64), (L.ROPE_NEOX, 128, 200), (0, 128, 513)])
def test_batch_rope_and_cache_stores_one_launch(backend, H, plog, mode, n_dims, T_):
    """A batch's ROPE(q), ROPE(k), SET_ROWS(k cache), SET_ROWS(v cache) run as one launch (k_rope_qk_store; from 33 tokens with whole heads
    rotated: the vectorised k_rope_qk_store_vec over the per-run (cos, sin) table, + the table's launch) and equal both the oracle and the
    node-by-node execution bit for bit."""
    rng = np.random.default_rng(41 + T_)
    HD, NH, NKV, NCTX = 128, 8, 2, max(300, T_ + 40)
    q = rng.standard_normal((T_, NH, HD)).astype(np.float32)
    k = rng.standard_normal((T_, NKV, HD)).astype(np.float32)
    v = rng.standard_normal((T_, NKV * HD)).astype(np.float32)
    pos = rng.integers(0, 5000, T_).astype(np.int32)
    rows = rng.permutation(NCTX)[:T_].astype(np.int64)
    kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)

    def build(g):
        tp = g.new(L.I32, [T_], pos)
        idx = g.new(L.I64, [T_], rows)
        # (the reshapes stand where llm_build_* has them: the projections come out 2-D)
        q3 = H.ggml_reshape_3d(g.ctx, g.new(L.F32, [NH * HD, T_], q), HD, NH, T_)
        k3 = H.ggml_reshape_3d(g.ctx, g.new(L.F32, [NKV * HD, T_], k), HD, NKV, T_)
        qr = H.ggml_rope_ext(g.ctx, q3, tp, None, n_dims, mode, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        kr = H.ggml_rope_ext(g.ctx, k3, tp, None, n_dims, mode, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        ks = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, kr, NKV * HD, T_), idx)
        vs = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], vc0), g.new(L.F32, [NKV * HD, T_], v), idx)
        return [qr, ks, vs]

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("fusion", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("fusion", 1)
    assert launches == (2 if T_ >= 33 and n_dims == HD else 1), launches
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache"), got, ref, plain):
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: fused and unfused differ"
        T.compare(f"batch rope+store T={T_} mode={mode} n_dims={n_dims} {name}", np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32),
                  max_nmse=1e-6 if name != "q_rope" else 1e-10, log=plog)


@pytest.mark.parametrize("T_", [32, 130, 512])
def test_batch_rope_and_transposed_v_store_one_launch(backend, H, plog, T_):
    """The same window on the non-flash path: the V store is a scatter of single elements into the transposed cache (an index per element)."""
    rng = np.random.default_rng(43 + T_)
    HD, NH, NKV, NCTX = 128, 8, 2, max(300, T_ + 40)
    q = rng.standard_normal((T_, NH, HD)).astype(np.float32)
    k = rng.standard_normal((T_, NKV, HD)).astype(np.float32)
    v = rng.standard_normal((T_, NKV * HD)).astype(np.float32)
    pos = rng.integers(0, 5000, T_).astype(np.int32)
    rows = rng.permutation(NCTX)[:T_].astype(np.int64)
    kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc0 = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    v_idx = (np.arange(NKV * HD, dtype=np.int64)[None, :] * NCTX + rows[:, None]).reshape(-1)

    def build(g):
        tp = g.new(L.I32, [T_], pos)
        idx = g.new(L.I64, [T_], rows)
        vidx = g.new(L.I64, [T_ * NKV * HD], v_idx)
        q3 = H.ggml_reshape_3d(g.ctx, g.new(L.F32, [NH * HD, T_], q), HD, NH, T_)
        k3 = H.ggml_reshape_3d(g.ctx, g.new(L.F32, [NKV * HD, T_], k), HD, NKV, T_)
        qr = H.ggml_rope_ext(g.ctx, q3, tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        kr = H.ggml_rope_ext(g.ctx, k3, tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        ks = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, kr, NKV * HD, T_), idx)
        v_view = H.ggml_reshape_2d(g.ctx, g.new(L.F16, [NCTX, NKV * HD], vc0), 1, NCTX * NKV * HD)
        vs = H.ggml_set_rows(g.ctx, v_view, H.ggml_reshape_2d(g.ctx, g.new(L.F32, [NKV * HD, T_], v), 1, T_ * NKV * HD), vidx)
        return [qr, ks, vs]

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("kernel_launches")
    got = T.run_case(build, backend)
    launches = backend.stat("kernel_launches") - k0
    backend.set_option("fusion", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("fusion", 1)
    assert launches == (2 if T_ >= 33 else 1), launches  # (from 33 tokens: the vectorised store + the (cos, sin) table's launch)
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache_T"), got, ref, plain):
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: fused and unfused differ"
        T.compare(f"batch rope + transposed V store T={T_} {name}", np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32),
                  max_nmse=1e-6 if name != "q_rope" else 1e-10, log=plog)


@pytest.mark.parametrize("tq,tv,M", [(L.Q4_K, L.Q4_K, 32), (L.Q4_K, L.Q6_K, 32), (L.Q4_K, L.Q6_K, 5)])
def test_np_batch_qkv_rope_store_epilogue_with_the_transposed_v_cache(backend, H, plog, tq, tv, M):
    """The same step on the NON-flash path (llama-box's default): V lives transposed in its cache, llama.cpp stores it with one index per
    ELEMENT.  The skinny launch's epilogue scatters the V values there itself (kind 4) — no rope + store launch on this path either.
    Equal to the oracle and bit for bit to the execution with the separate launch."""
    rng = np.random.default_rng(311 + tq + tv + M)
    E, HD, NH, NKV, NCTX = 1024, 128, 8, 2, 300
    x = rng.standard_normal((M, E)).astype(np.float32)
    wq, wk, wv = T.rand_weight(tq, E, NH * HD, rng), T.rand_weight(tq, E, NKV * HD, rng), T.rand_weight(tv, E, NKV * HD, rng)
    kc0 = rng.standard_normal((NCTX, NKV * HD)).astype(np.float16)
    vc0 = rng.standard_normal((NKV * HD, NCTX)).astype(np.float16)
    pos = rng.integers(0, 5000, M).astype(np.int32)
    rows = rng.permutation(NCTX)[:M].astype(np.int64)
    v_idx = (np.arange(NKV * HD, dtype=np.int64)[None, :] * NCTX + rows[:, None]).reshape(-1)

    def build(g):
        cur = g.new(L.F32, [E, M], x)
        q = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NH * HD], wq), cur)
        k = H.ggml_mul_mat(g.ctx, g.new(tq, [E, NKV * HD], wk), cur)
        v = H.ggml_mul_mat(g.ctx, g.new(tv, [E, NKV * HD], wv), cur)
        tp = g.new(L.I32, [M], pos)
        idx = g.new(L.I64, [M], rows)
        vidx = g.new(L.I64, [M * NKV * HD], v_idx)
        q = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, q, HD, NH, M), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, k, HD, NKV, M), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        ks = H.ggml_set_rows(g.ctx, g.new(L.F16, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, k, NKV * HD, M), idx)
        v_view = H.ggml_reshape_2d(g.ctx, g.new(L.F16, [NCTX, NKV * HD], vc0), 1, NCTX * NKV * HD)
        vs = H.ggml_set_rows(g.ctx, v_view, H.ggml_reshape_2d(g.ctx, v, 1, M * NKV * HD), vidx)
        return [q, ks, vs]

    ref = T.run_case(build, "oracle", expand_first=())
    e0 = backend.stat("rope_epilogues")
    got = T.run_case(build, backend)
    epilogues = backend.stat("rope_epilogues") - e0
    backend.set_option("skinny_rope", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("skinny_rope", 1)
    assert epilogues == 1, epilogues
    for name, a, b, c in zip(("q_rope", "k_cache", "v_cache_T"), got, ref, plain):
        a32, b32 = (np.asarray(t).astype(np.float32) for t in (a, b))
        T.compare(f"np batch qkv (transposed V) {QNAME[tq]}/{QNAME[tv]} M={M} {name}", a32, b32, max_nmse=1e-10 if name == "q_rope" else 1e-6, log=plog)
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"{name}: epilogue and separate rope launch differ"
    vt = np.asarray(got[2]).reshape(NKV * HD, NCTX)
    assert np.array_equal(np.delete(vt, rows, axis=1), np.delete(vc0, rows, axis=1)), "cells of other tokens were touched"


# ------------------------------------------------------------------------------------------------ fused chains
@pytest.mark.parametrize("qt", QTYPES)
@pytest.mark.parametrize("M", [1, 4, 32, 130])
def test_fused_chains_equal_unfused(backend, H, plog, qt, M):
    """norm->mul->{gate,up}->swiglu->down->+bias->+residual with fusion on == fusion off == oracle."""
    rng = np.random.default_rng(21 + qt + M)
    E, FF = 512, 1024
    x = rng.standard_normal((M, E)).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, E).astype(np.float32)
    wg, wu, wd = T.rand_weight(qt, E, FF, rng), T.rand_weight(qt, E, FF, rng), T.rand_weight(qt, FF, E, rng)
    bias = rng.standard_normal(E).astype(np.float32)

    def build(g):
        tx = g.new(L.F32, [E, M], x)
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, tx, 1e-5), g.new(L.F32, [E], nw))
        gate = H.ggml_mul_mat(g.ctx, g.new(qt, [E, FF], wg), cur)
        up = H.ggml_mul_mat(g.ctx, g.new(qt, [E, FF], wu), cur)
        act = H.ggml_swiglu_split(g.ctx, gate, up)
        down = H.ggml_mul_mat(g.ctx, g.new(qt, [FF, E], wd), act)
        down = H.ggml_add(g.ctx, down, g.new(L.F32, [E], bias))
        return H.ggml_add(g.ctx, down, tx)

    ref = T.run_case(build, "oracle")
    k0 = backend.stat("fused_nodes")
    backend.set_option("fusion", 1)
    fused = T.run_case(build, backend)
    assert backend.stat("fused_nodes") > k0, "fusion did not trigger"
    backend.set_option("fusion", 0)
    try:
        plain = T.run_case(build, backend)
    finally:
        backend.set_option("fusion", 1)
    # vs the oracle the gate allows for ONE activation-rounding flip: silu's expf differs by an ulp between libm and
    # the device, and an ulp can move one Q8 activation across a rounding boundary (worth ~5e-7 NMSE on this shape)
    T.compare(f"ffn chain fused {QNAME[qt]} M={M}", fused[0], ref[0], max_nmse=2e-6, log=plog)
    T.compare(f"ffn chain unfused {QNAME[qt]} M={M}", plain[0], ref[0], max_nmse=2e-6, log=plog)
    T.compare(f"ffn chain fused-vs-unfused {QNAME[qt]} M={M}", fused[0], plain[0], max_nmse=1e-12, log=plog)
