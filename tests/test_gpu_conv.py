"""GPU: csrc/conv.hip through the C-ABI — IM2COL, POOL_2D / POOL_1D, PAD and UPSCALE bit for bit against the f32 twins of tests/conv_ref.py (the CPU oracle has
none of the ops), MUL_MAT f16 x f16 against the float64 twin at the project's gate for this arithmetic in both of its forms, then a vision and an audio front end
over persistent buffers, eager and as a replayed hipGraph.

Every value test here fails on a backend without these ops: harness.G.compute raises supports_op=false at the first new node; the acceptance test fails outright.
"""
import ctypes as C
import math

import numpy as np
import pytest

import conv_ref as R
import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu
F32, F16, BF16, Q8_0 = L.F32, L.F16, L.BF16, L.Q8_0
f16, f32, f64 = np.float16, np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == f16 else np.uint32)


def _run(target, build):
    """build(g) -> the tensors to read after one compute of all of them."""
    g = T.G(target)
    try:
        outs = build(g)
        g.compute(list(outs))
        return [g.read(t) for t in outs]
    finally:
        g.free()


def _strided(g, x, extra):
    """x [n3, n2, n1, n0] uploaded inside a larger tensor (extra = elements added to dims 1, 2, 3) and returned as a view of x's extents: dim 0 stays contiguous,
    every other stride exceeds the dense one."""
    n3, n2, n1, n0 = x.shape
    big = np.random.default_rng(99).standard_normal((n3 + extra[2], n2 + extra[1], n1 + extra[0], n0)).astype(f32)
    big[:n3, :n2, :n1, :] = x
    t = g.new(F32, list(big.shape[::-1]), big)
    nb1 = n0 * 4
    nb2 = nb1 * big.shape[2]
    nb3 = nb2 * big.shape[1]
    return g.H.ggml_view_4d(g.ctx, t, n0, n1, n2, n3, nb1, nb2, nb3, 0)


def _im2col_node(g, x, KH, KW, s0, s1, p0, p1, d0, d1, dt, two_d=True, view=None):
    """x [N, IC, IH, IW] (2-D) or [N, IC, 1, IW] (1-D: data [IW, IC, N])."""
    H, ctx = g.H, g.ctx
    N, IC, IH, IW = x.shape
    if two_d:
        kern = g.new(F16, [KW, KH, IC, 2])
        data = view if view is not None else g.new(F32, [IW, IH, IC, N], x)
        return H.ggml_im2col(ctx, kern, data, s0, s1, p0, p1, d0, d1, True, dt)
    kern = g.new(F16, [KW, IC, 2])
    return H.ggml_im2col(ctx, kern, g.new(F32, [IW, IC, N], x), s0, 0, p0, 0, d0, 0, False, dt)


# ------------------------------------------------------------------------------------------------ 1. acceptance, 2. refusals
def _mm(H, ctx, ta, tb, K, na, nb, batch_a=1, batch_b=1):
    return H.ggml_mul_mat(ctx, H.ggml_new_tensor_3d(ctx, ta, K, na, batch_a), H.ggml_new_tensor_3d(ctx, tb, K, nb, batch_b))


def test_supports_op_accepts_the_tower_ops(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        # tower shapes: a 448 x 448 image under 14 x 14 patches (Qwen2-VL / SigLIP style), a Whisper stem over 3000 mel frames
        patch = H.ggml_new_tensor_4d(ctx, F16, 14, 14, 3, 1280)
        image = H.ggml_new_tensor_4d(ctx, F32, 448, 448, 3, 1)
        for dt in (F16, F32):
            assert ok(H.ggml_im2col(ctx, patch, image, 14, 14, 0, 0, 1, 1, True, dt)), dt
        stem = H.ggml_new_tensor_3d(ctx, F16, 3, 128, 1280)
        mel = H.ggml_new_tensor_3d(ctx, F32, 3000, 128, 1)
        assert ok(H.ggml_im2col(ctx, stem, mel, 1, 0, 1, 0, 1, 0, False, F16))
        assert ok(H.ggml_im2col(ctx, H.ggml_new_tensor_3d(ctx, F16, 3, 1280, 1280), H.ggml_new_tensor_3d(ctx, F32, 3000, 1280, 1), 2, 0, 1, 0, 1, 0, False, F16))
        assert ok(_mm(H, ctx, F16, F16, 588, 1024, 1280)) and ok(_mm(H, ctx, F16, F16, 588, 729, 1152)) and ok(_mm(H, ctx, F16, F16, 384, 3000, 1280))
        assert ok(H.ggml_pool_2d(ctx, H.ggml_new_tensor_4d(ctx, F32, 64, 64, 1152, 1), L.POOL_AVG, 4, 4, 4, 4, 0.0, 0.0))
        assert ok(H.ggml_pool_1d(ctx, H.ggml_new_tensor_2d(ctx, F32, 1500, 1280), L.POOL_AVG, 2, 2, 0))
        assert ok(H.ggml_pad(ctx, H.ggml_new_tensor_3d(ctx, F32, 1280, 749, 1), 0, 3, 0, 0))
        pos = H.ggml_new_tensor_3d(ctx, F32, 27, 27, 1152)
        for mode in (L.SCALE_NEAREST, L.SCALE_BILINEAR):
            assert ok(H.ggml_interpolate(ctx, pos, 32, 20, 1152, 1, mode)), mode
        # tiny ones, both whole graphs of the builders included
        kern = H.ggml_new_tensor_4d(ctx, F16, 3, 3, 2, 4)
        img = H.ggml_new_tensor_4d(ctx, F32, 5, 7, 2, 1)
        assert ok(H.ggml_im2col(ctx, kern, img, 1, 1, 1, 1, 1, 1, True, F16)) and ok(H.ggml_im2col(ctx, kern, img, 2, 1, 0, 2, 1, 2, True, F32))
        assert ok(_mm(H, ctx, F16, F16, 9, 5, 3)) and ok(_mm(H, ctx, F16, F16, 1, 1, 1)) and ok(_mm(H, ctx, F16, F16, 24, 7, 3, 2, 4))
        for op in (L.POOL_MAX, L.POOL_AVG):
            assert ok(H.ggml_pool_2d(ctx, img, op, 3, 2, 2, 1, 1.0, 0.0)) and ok(H.ggml_pool_1d(ctx, img, op, 2, 2, 0))
        assert ok(H.ggml_pad(ctx, img, 0, 0, 0, 0)) and ok(H.ggml_pad(ctx, img, 1, 2, 3, 4))
        assert ok(H.ggml_upscale(ctx, img, 2, L.SCALE_NEAREST)) and ok(H.ggml_interpolate(ctx, img, 3, 9, 2, 1, L.SCALE_BILINEAR))
        c2 = H.ggml_conv_2d(ctx, kern, img, 1, 1, 1, 1, 1, 1)
        c1 = H.ggml_conv_1d(ctx, H.ggml_new_tensor_3d(ctx, F16, 3, 8, 16), H.ggml_new_tensor_3d(ctx, F32, 30, 8, 2), 2, 1, 1)
        for t in (c2, c1):
            while t:  # down the chain of first sources to the IM2COL
                assert ok(t), H.ggml_op_name(t.contents.op)
                t = t.contents.src[0] if t.contents.op != 0 and t.contents.src[0] else None
    finally:
        g.free()


def test_supports_op_refuses_what_is_outside_the_contract(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        x = H.ggml_new_tensor_4d(ctx, F32, 8, 6, 2, 1)
        assert ok(H.ggml_interpolate(ctx, x, 16, 12, 2, 1, L.SCALE_BILINEAR))
        assert not ok(H.ggml_interpolate(ctx, x, 16, 12, 2, 1, L.SCALE_BICUBIC))
        for mode in (L.SCALE_NEAREST, L.SCALE_BILINEAR):
            assert not ok(H.ggml_interpolate(ctx, x, 16, 12, 2, 1, mode | L.SCALE_ALIGN_CORNERS)), mode
        assert not ok(H.ggml_interpolate(ctx, x, 16, 12, 2, 1, L.SCALE_BILINEAR | (1 << 9)))  # some other bit
        assert not ok(H.ggml_interpolate(ctx, H.ggml_new_tensor_4d(ctx, F16, 8, 6, 2, 1), 16, 12, 2, 1, L.SCALE_NEAREST))
        # POOL_1D computes only k0 == s0, p0 == 0
        assert ok(H.ggml_pool_1d(ctx, x, L.POOL_AVG, 2, 2, 0))
        assert not ok(H.ggml_pool_1d(ctx, x, L.POOL_AVG, 3, 2, 0)) and not ok(H.ggml_pool_1d(ctx, x, L.POOL_AVG, 2, 1, 0)) and not ok(H.ggml_pool_1d(ctx, x, L.POOL_MAX, 2, 2, 1))
        assert not ok(H.ggml_pool_2d(ctx, H.ggml_new_tensor_4d(ctx, F16, 8, 6, 2, 1), L.POOL_AVG, 2, 2, 2, 2, 0.0, 0.0))
        node = H.ggml_pool_2d(ctx, x, L.POOL_AVG, 2, 2, 2, 2, 0.0, 0.0)
        node.contents.op_params[0] = 2  # no such pool op
        assert not ok(node)
        assert not ok(H.ggml_pool_2d(ctx, H.ggml_transpose(ctx, x), L.POOL_MAX, 2, 2, 2, 2, 0.0, 0.0))  # source elements not contiguous
        # PAD: a left pad of a later ggml version
        for i in (0, 2, 4, 6):
            node = H.ggml_pad(ctx, x, 1, 1, 0, 0)
            assert ok(node)
            node.contents.op_params[i] = 1
            assert not ok(node), i
        assert not ok(H.ggml_pad(ctx, H.ggml_new_tensor_4d(ctx, F16, 8, 6, 2, 1), 1, 0, 0, 0))
        node = H.ggml_pad(ctx, x, 1, 0, 0, 0)
        node.contents.ne[1] -= 1  # a result smaller than its source
        assert not ok(node)
        # IM2COL
        kern = H.ggml_new_tensor_4d(ctx, F16, 3, 3, 2, 4)
        assert ok(H.ggml_im2col(ctx, kern, x, 1, 1, 1, 1, 1, 1, True, F16))
        wide = H.ggml_new_tensor_4d(ctx, F32, 10, 6, 2, 1)
        padded_rows = H.ggml_view_4d(ctx, wide, 8, 6, 2, 1, 10 * 4, 10 * 6 * 4, 10 * 6 * 2 * 4, 0)
        assert not ok(H.ggml_im2col(ctx, kern, padded_rows, 1, 1, 1, 1, 1, 1, True, F16))
        assert not ok(H.ggml_im2col(ctx, kern, H.ggml_new_tensor_4d(ctx, F16, 8, 6, 2, 1), 1, 1, 1, 1, 1, 1, True, F16))
        node = H.ggml_im2col(ctx, kern, x, 1, 1, 1, 1, 1, 1, True, F16)
        node.contents.ne[1] -= 1  # a result one column short
        assert not ok(node)
        for i, v in ((0, 0), (1, -1), (2, -1), (3, -1), (4, 0), (5, 0)):  # strides <= 0, negative padding, dilations <= 0
            node = H.ggml_im2col(ctx, kern, x, 1, 1, 1, 1, 1, 1, True, F16)
            node.contents.op_params[i] = v
            assert not ok(node), (i, v)
        assert not ok(H.ggml_im2col(ctx, kern, x, 1, 1, 1, 1, 1, 1, True, BF16))
        # MUL_MAT: only f16 x f16 joins f32 activations
        assert ok(_mm(H, ctx, F16, F16, 64, 8, 4))
        assert not ok(_mm(H, ctx, F32, F16, 64, 8, 4)) and not ok(_mm(H, ctx, Q8_0, F16, 64, 8, 4)) and not ok(_mm(H, ctx, F16, BF16, 64, 8, 4))
        assert not ok(_mm(H, ctx, BF16, F16, 64, 8, 4)) and not ok(_mm(H, ctx, L.Q4_K, F16, 256, 8, 4))
        assert not ok(H.ggml_mul_mat(ctx, H.ggml_new_tensor_2d(ctx, F16, 64, 8), H.ggml_transpose(ctx, H.ggml_new_tensor_2d(ctx, F16, 4, 64))))  # src1 elements not contiguous
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ 3. IM2COL
IM2COL_2D = [  # (N, IC, IH, IW), KH, KW, s0, s1, p0, p1, d0, d1
    ((2, 3, 28, 28), 14, 14, 14, 14, 0, 0, 1, 1),   # K = 588, the patch case
    ((1, 2, 7, 5), 3, 3, 1, 1, 1, 1, 1, 1),
    ((1, 3, 6, 8), 3, 3, 2, 2, 1, 1, 1, 1),
    ((1, 1, 9, 9), 3, 3, 1, 1, 2, 2, 2, 2),         # K = 9: odd rows
    ((1, 2, 5, 6), 3, 1, 2, 1, 0, 1, 1, 1),         # a 1 x 3 kernel (KW 1, KH 3), strides (2, 1), pads (0, 1)
    ((1, 3, 64, 64), 16, 16, 16, 16, 0, 0, 1, 1),   # more than one workgroup
]


@pytest.mark.parametrize("dt", [F16, F32])
def test_im2col_bit_exact(backend, dt):
    npdt = f16 if dt == F16 else f32
    rng = np.random.default_rng(11)
    xs = [(rng.standard_normal(c[0]) * 3).astype(f32) for c in IM2COL_2D]
    x1 = (rng.standard_normal((2, 8, 1, 30)) * 3).astype(f32)

    def build(g):
        outs = [_im2col_node(g, x, *c[1:], dt) for x, c in zip(xs, IM2COL_2D)]
        outs.append(_im2col_node(g, xs[1], *IM2COL_2D[1][1:], dt, view=_strided(g, xs[1], (1, 1, 1))))  # dense rows; channel and batch strides beyond the dense ones
        outs += [_im2col_node(g, x1, 1, 3, s0, 1, 1, 0, 1, 1, dt, two_d=False) for s0 in (1, 2)]
        return outs

    got = _run(backend, build)
    want = [R.im2col(x, *c[1:], npdt) for x, c in zip(xs, IM2COL_2D)]
    want.append(want[1])
    want += [R.im2col(x1, 1, 3, s0, 1, 1, 0, 1, 1, npdt).reshape(1, 2, -1, 24) for s0 in (1, 2)]
    assert want[0].shape[-1] == 588 and want[3].shape[-1] == 9 and want[5].size > 256 * 8
    for k, (r, w) in enumerate(zip(got, want)):
        assert r.dtype == npdt and r.shape == w.shape and np.array_equal(_bits(r), _bits(w)), k


# ------------------------------------------------------------------------------------------------ 4. MUL_MAT f16 x f16
# (K, src0 rows, src1 rows): 8-byte rows, 4-byte rows, odd K, 16-byte rows, a K below one trip, one column; then the two sides of the routed threshold
MM_SHAPES = [(588, 40, 33), (590, 33, 65), (9, 5, 3), (768, 64, 64), (24, 70, 33), (1176, 8, 1), (588, 224, 128), (588, 256, 128)]
MM_MIN_TILES = 32  # kernels.h MI_CONV_MMA_MIN_TILES: conv_mma 1 takes the matrix cores from this many 32 x 32 result tiles on


def _mm_form(mode, K, na, nb, batches=1):
    """The form that serves an uploaded (16-byte-aligned) pair: conv_mma 0 never the matrix cores, 2 wherever K is even, 1 routed by the tile count."""
    if mode == 0 or K % 2:
        return "dot"
    return "mma" if mode == 2 or -(-na // 32) * -(-nb // 32) * batches >= MM_MIN_TILES else "dot"


def _mm_inputs():
    rng = np.random.default_rng(12)
    cases = [(rng.standard_normal((na, K)).astype(f16), rng.standard_normal((nb, K)).astype(f16)) for K, na, nb in MM_SHAPES]
    cases.append((rng.standard_normal((1, 40, 588)).astype(f16), rng.standard_normal((2, 33, 588)).astype(f16)))  # src0 broadcast over two src1 batches
    return cases


@pytest.fixture(scope="module")
def mm_cases():
    cases = _mm_inputs()
    return cases, [R.mul_mat64(a, b) for a, b in cases]


@pytest.mark.parametrize("mma", [2, 1, 0])
def test_mul_mat_f16_f16_within_the_gate_and_deterministic(backend, H, plog, mm_cases, mma):
    cases, wants = mm_cases
    img = (np.random.default_rng(13).standard_normal((4, 3, 28, 28)) * 2).astype(f32)  # 16 patches
    kern = np.random.default_rng(14).standard_normal((32, 588)).astype(f16)

    def build(g):
        outs = []
        for a, b in cases:
            for _ in range(2):  # the same node twice: bit-equal
                outs.append(H.ggml_mul_mat(g.ctx, g.new(F16, list(a.shape[::-1]), a), g.new(F16, list(b.shape[::-1]), b)))
        cols = _im2col_node(g, img, 14, 14, 14, 14, 0, 0, 1, 1, F16)  # src0 a reshaped IM2COL result
        outs.append(H.ggml_mul_mat(g.ctx, H.ggml_reshape_2d(g.ctx, cols, 588, 16), g.new(F16, [588, 32], kern)))
        return outs

    try:
        backend.set_option("conv_mma", mma)
        backend.set_option("timing", 1)
        backend.timing_report()
        got = _run(backend, build)
        classes = backend.timing_report()
    finally:
        backend.set_option("timing", 0)
        backend.set_option("conv_mma", 1)
    # which form ran: every node's form follows from the switch and its shape (the batch: 588 x 40 x 33 twice over; the IM2COL product: 588 x 16 x 32)
    forms = [_mm_form(mma, *s) for s in MM_SHAPES] + [_mm_form(mma, 588, 40, 33, 2)]
    n_mma = 2 * forms.count("mma") + (_mm_form(mma, 588, 16, 32) == "mma")
    assert n_mma == {2: 17, 1: 2, 0: 0}[mma]  # forced: seven even-K shapes and the batch twice each, and the IM2COL product; routed: the one 32-tile shape, twice
    assert classes.get("mul_mat_f16x_mma", (0,))[0] == n_mma and classes.get("mul_mat_f16x_dot", (0,))[0] == 2 * len(cases) + 1 - n_mma, classes
    wants = wants + [R.mul_mat64(R.im2col(img, 14, 14, 14, 14, 0, 0, 1, 1, f16).reshape(16, 588), kern)]
    for k, want in enumerate(wants):
        r = got[2 * k] if k < len(cases) else got[-1]
        e = R.nmse(r.reshape(want.shape), want)
        plog(f"  mul_mat f16 x f16 conv_mma={mma} case {k} {want.shape}: nmse {e:.3e} (gate {R.MM_NMSE_GATE:.0e})")
        assert r.dtype == f32 and e <= R.MM_NMSE_GATE, (k, e)
        if k < len(cases):
            assert np.array_equal(_bits(got[2 * k]), _bits(got[2 * k + 1])), k


# ------------------------------------------------------------------------------------------------ 5. POOL_2D / POOL_1D
POOL_2D = [  # (N3, N2, H, W), k0, k1, s0, s1, p0, p1
    ((1, 1, 4, 4), 2, 2, 2, 2, 0, 0), ((1, 1, 5, 7), 3, 3, 2, 2, 1, 1), ((1, 2, 6, 6), 1, 1, 1, 1, 0, 0), ((1, 1, 7, 6), 2, 3, 1, 2, 0, 0),
]


@pytest.mark.parametrize("op", [R.MAX, R.AVG])
def test_pool_bit_exact(backend, H, op):
    rng = np.random.default_rng(15)
    xs = [rng.standard_normal(c[0]).astype(f32) - (2 if op == R.MAX else 0) for c in POOL_2D]  # (MAX over negatives: padding must not be read as zero)
    xv = rng.standard_normal((2, 3, 9, 8)).astype(f32)  # 3 planes x 2 batches through a strided view
    rows9, rows8 = rng.standard_normal((3, 9)).astype(f32), rng.standard_normal((2, 2, 8)).astype(f32)

    def build(g):
        outs = [H.ggml_pool_2d(g.ctx, g.new(F32, list(x.shape[::-1]), x), op, c[1], c[2], c[3], c[4], float(c[5]), float(c[6])) for x, c in zip(xs, POOL_2D)]
        outs.append(H.ggml_pool_2d(g.ctx, _strided(g, xv, (2, 1, 1)), op, 3, 3, 2, 2, 1.0, 1.0))
        outs.append(H.ggml_pool_1d(g.ctx, g.new(F32, [9, 3], rows9), op, 2, 2, 0))  # the ninth sample is dropped
        outs.append(H.ggml_pool_1d(g.ctx, g.new(F32, [8, 2, 2], rows8), op, 4, 4, 0))
        return outs

    got = _run(backend, build)
    want = [R.pool2d(x, op, *c[1:]) for x, c in zip(xs, POOL_2D)] + [R.pool2d(xv, op, 3, 3, 2, 2, 1, 1), R.pool1d(rows9, op, 2), R.pool1d(rows8, op, 4)]
    assert want[-2].shape == (3, 4) and want[-1].shape == (2, 2, 2)
    for k, (r, w) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(r.reshape(w.shape)), _bits(w)), (op, k)


# ------------------------------------------------------------------------------------------------ 6. PAD
def test_pad_bit_exact(backend, H):
    rng = np.random.default_rng(16)
    x = rng.standard_normal((2, 3, 4, 5)).astype(f32)
    x[0, 0, 0, 0] = -0.0
    pads = [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (3, 1, 2, 2), (0, 0, 0, 0)]
    big = rng.standard_normal((1, 1, 3, 300)).astype(f32)  # more than one workgroup

    def build(g):
        t = g.new(F32, [5, 4, 3, 2], x)
        outs = [H.ggml_pad(g.ctx, t, *p) for p in pads]
        outs.append(H.ggml_pad(g.ctx, H.ggml_permute(g.ctx, t, 0, 2, 1, 3), 1, 1, 0, 1))  # a permuted source: dims 1 and 2 swapped
        outs.append(H.ggml_pad(g.ctx, g.new(F32, [300, 3], big), 5, 1, 0, 0))
        return outs

    got = _run(backend, build)
    want = [R.pad(x, (2 + p[3], 3 + p[2], 4 + p[1], 5 + p[0])) for p in pads]
    want.append(R.pad(np.ascontiguousarray(x.transpose(0, 2, 1, 3)), (3, 4, 4, 6)))
    want.append(R.pad(big, (1, 1, 4, 305)))
    for k, (r, w) in enumerate(zip(got, want)):
        assert r.shape == w.shape and np.array_equal(_bits(r), _bits(w)), k


# ------------------------------------------------------------------------------------------------ 7. UPSCALE
def test_upscale_bit_exact(backend, H):
    rng = np.random.default_rng(17)
    near = [((5, 4), (10, 8)), ((5, 4), (15, 12)), ((3, 3), (7, 7)), ((1, 1), (4, 4))]                     # (H, W) -> (H, W): x 2, x 3, 3 -> 7
    lin = [((2, 2), (5, 3)), ((16, 16), (11, 27)), ((1, 1), (4, 4)), ((2, 2), (4, 4))]                    # W 2 -> 3, H 2 -> 5; 16 x 16 -> 27 wide, 11 high
    xs_n = [rng.standard_normal((1, 2) + s).astype(f32) for s, _ in near]
    xs_l = [rng.standard_normal((1, 2) + s).astype(f32) for s, _ in lin]
    deep = rng.standard_normal((2, 2, 3, 3)).astype(f32)  # dims 2 and 3 scaled too: nearest there in both modes

    def build(g):
        outs = [H.ggml_interpolate(g.ctx, g.new(F32, list(x.shape[::-1]), x), d[1], d[0], 2, 1, L.SCALE_NEAREST) for x, (_, d) in zip(xs_n, near)]
        outs += [H.ggml_interpolate(g.ctx, g.new(F32, list(x.shape[::-1]), x), d[1], d[0], 2, 1, L.SCALE_BILINEAR) for x, (_, d) in zip(xs_l, lin)]
        outs += [H.ggml_interpolate(g.ctx, g.new(F32, [3, 3, 2, 2], deep), 5, 4, 3, 4, m) for m in (L.SCALE_NEAREST, L.SCALE_BILINEAR)]
        outs.append(H.ggml_upscale(g.ctx, g.new(F32, [4, 5, 2, 1], xs_n[0]), 2, L.SCALE_NEAREST))
        return outs

    got = _run(backend, build)
    want = [R.upscale_nearest(x, (1, 2) + d) for x, (_, d) in zip(xs_n, near)] + [R.upscale_bilinear(x, (1, 2) + d) for x, (_, d) in zip(xs_l, lin)]
    want += [R.upscale_nearest(deep, (4, 3, 4, 5)), R.upscale_bilinear(deep, (4, 3, 4, 5)), R.upscale_nearest(xs_n[0], (1, 2, 10, 8))]
    for k, (r, w) in enumerate(zip(got, want)):
        assert r.shape == w.shape and np.array_equal(_bits(r), _bits(w)), k


# ------------------------------------------------------------------------------------------------ 8. two front ends over persistent buffers
_erf = np.vectorize(math.erf)


def _gelu_erf(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


class Vision:
    """conv_2d patch 14 on a 28 x 42 x 3 image -> 32 channels; + bias; + a 2 x 2 position grid resized bilinearly to the 2 x 3 patch grid; NORM; 2 x 2 AVG POOL_2D
    over the patch grid (clip.cpp's order: the convolution's [OW, OH, C] is flattened and transposed to [C, patches])."""
    EPS = 1e-6
    mid = None

    def __init__(self):
        rng = np.random.default_rng(80)
        self.kern = (rng.standard_normal((32, 3, 14, 14)) / 24).astype(f16)
        self.bias = rng.standard_normal(32).astype(f32)
        self.pos = rng.standard_normal((32, 2, 2)).astype(f32)  # [W 2, H 2, C 32]
        self.steps = [rng.standard_normal((1, 3, 42, 28)).astype(f32) for _ in range(3)]

    def graph(self, g):
        H, ctx = g.H, g.ctx
        x = g.new(F32, [28, 42, 3, 1])
        c = H.ggml_conv_2d(ctx, g.new(F16, [14, 14, 3, 32], self.kern), x, 14, 14, 0, 0, 1, 1)     # [2, 3, 32, 1]
        c = H.ggml_cont(ctx, H.ggml_transpose(ctx, H.ggml_reshape_2d(ctx, c, 6, 32)))                # [32, 6]
        c = H.ggml_add(ctx, c, g.new(F32, [32], self.bias))
        p = H.ggml_interpolate(ctx, g.new(F32, [2, 2, 32], self.pos), 2, 3, 32, 1, L.SCALE_BILINEAR)  # [2, 3, 32]
        c = H.ggml_add(ctx, c, H.ggml_cont(ctx, H.ggml_transpose(ctx, H.ggml_reshape_2d(ctx, p, 6, 32))))
        c = H.ggml_norm(ctx, c, self.EPS)
        c = H.ggml_reshape_3d(ctx, H.ggml_cont(ctx, H.ggml_transpose(ctx, c)), 2, 3, 32)             # [2, 3, 32]
        return x, H.ggml_pool_2d(ctx, c, L.POOL_AVG, 2, 2, 2, 2, 0.0, 0.0)                          # [1, 1, 32]

    def twin(self, x, mid=None):
        cols = R.im2col(x, 14, 14, 14, 14, 0, 0, 1, 1, f16).reshape(6, 588)
        c = R.mul_mat64(cols, self.kern.reshape(32, 588))[0, 0].T                                    # [patch, channel]
        c = c + self.bias.astype(f64)
        c = c + R.upscale_bilinear(self.pos[None], (1, 32, 3, 2), f64).reshape(32, 6).T
        m = c.mean(-1, keepdims=True)
        c = (c - m) / np.sqrt(((c - m) ** 2).mean(-1, keepdims=True) + self.EPS)
        return R.pool2d(c.T.reshape(1, 32, 3, 2), R.AVG, 2, 2, 2, 2, 0, 0, f64).reshape(32)


class Audio:
    """conv_1d k 3 p 1; + bias; GELU_ERF; conv_1d k 3 s 2 p 1; + bias; GELU_ERF; transpose and CONT; AVG POOL_1D of 2 (a Whisper-style stem: 30 frames of 8 mel
    bins -> 16 channels, biases stored [1, C] as clip.cpp keeps them)."""

    def __init__(self):
        rng = np.random.default_rng(81)
        self.k1 = (rng.standard_normal((16, 8, 3)) / 5).astype(f16)
        self.k2 = (rng.standard_normal((16, 16, 3)) / 7).astype(f16)
        self.b1, self.b2 = rng.standard_normal(16).astype(f32), rng.standard_normal(16).astype(f32)
        self.steps = [rng.standard_normal((1, 8, 1, 30)).astype(f32) for _ in range(3)]

    def graph(self, g):
        H, ctx = g.H, g.ctx
        x = g.new(F32, [30, 8, 1])
        c = H.ggml_conv_1d(ctx, g.new(F16, [3, 8, 16], self.k1), x, 1, 1, 1)                         # [30, 16, 1]
        c = self.mid = H.ggml_gelu_erf(ctx, H.ggml_add(ctx, c, g.new(F32, [1, 16], self.b1)))
        c = H.ggml_conv_1d(ctx, g.new(F16, [3, 16, 16], self.k2), c, 2, 1, 1)                        # [15, 16, 1]
        c = H.ggml_gelu_erf(ctx, H.ggml_add(ctx, c, g.new(F32, [1, 16], self.b2)))
        c = H.ggml_cont(ctx, H.ggml_transpose(ctx, c))                                               # [16, 15]
        return x, H.ggml_pool_1d(ctx, c, L.POOL_AVG, 2, 2, 0)                                        # [8, 15]

    @staticmethod
    def _conv(v, k, s0):
        """v f32 [C_in, T] -> float64 [C_out, T']: the im2col rounds to the kernel's f16, as the node does."""
        cols = R.im2col(v.reshape(1, v.shape[0], 1, v.shape[1]), 1, 3, s0, 1, 1, 0, 1, 1, f16)[0, 0]
        return R.mul_mat64(cols, k.reshape(k.shape[0], -1))[0, 0]

    def twin_mid(self, x):
        """The first leg: the activations the second IM2COL reads, [16, 30]."""
        return _gelu_erf(self._conv(x[0, :, 0, :], self.k1, 1) + self.b1.astype(f64)[:, None])

    def twin(self, x, mid=None):
        """The second leg starts from the f32 activations the GPU itself fed its second IM2COL (`mid`): that node rounds them to f16, and a twin that rounded its own
        float64 activations instead would now and then land on the other side of an f16 rounding boundary — an error of 2^-11 in an operand, far above the gate, that
        says nothing about any kernel.  The first leg is held to the gate on its own (twin_mid)."""
        c = _gelu_erf(self._conv(mid.reshape(16, 30), self.k2, 2) + self.b2.astype(f64)[:, None])
        return R.pool1d(c.T, R.AVG, 2, f64)                                                          # [15, 8]


def _run_chain(backend, chain):
    """Three steps of the ONE graph on the same buffers -> (per-step results, the counters' change)."""
    H = L.host()
    g = T.G(backend)
    try:
        x, out = chain.graph(g)
        gf = H.ggml_new_graph_custom(g.ctx, 256, False)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        ops = set()
        for i in range(gf.contents.n_nodes):  # the path the scheduler would cut: no node may be refused
            node = gf.contents.nodes[i]
            assert H.ggml_backend_dev_supports_op(backend.dev, node), (i, H.ggml_op_name(node.contents.op), node.contents.name)
            ops.add(H.ggml_op_name(node.contents.op).decode())
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures")}
        res = []
        for step in chain.steps:
            raw = np.ascontiguousarray(step)
            H.ggml_backend_tensor_set(x, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(out).copy(), g.read(chain.mid).copy() if chain.mid else None))
        return res, {k: backend.stat(k) - v for k, v in s0.items()}, ops
    finally:
        g.free()


@pytest.mark.parametrize("chain_cls", [Vision, Audio])
def test_front_end_eager_and_replayed(backend, plog, chain_cls):
    """Every node accepted; each step against the float64 twin chain at the mat-mul gate; the second sighting is captured, the third replayed (graph_launches 2, one
    capture), bit-equal at every step to a backend with graphs off."""
    chain = chain_cls()
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            runs[mode] = _run_chain(backend, chain)
    finally:
        backend.set_option("graphs", 1)
    ops = runs[0][2]
    assert {"IM2COL", "MUL_MAT"} <= ops and (({"UPSCALE", "POOL_2D", "NORM"} <= ops) if chain_cls is Vision else ("POOL_1D" in ops)), ops
    plog(f"  {chain_cls.__name__} front end: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["graph_captures"] == 0, runs[0][1]
    for k, ((a, a_mid), (b, b_mid), x) in enumerate(zip(runs[1][0], runs[0][0], chain.steps)):
        assert np.array_equal(_bits(a), _bits(b)), k
        if b_mid is not None:
            assert np.array_equal(_bits(a_mid), _bits(b_mid)), k
            want = chain.twin_mid(x)
            e = R.nmse(b_mid.reshape(want.shape), want)
            plog(f"  {chain_cls.__name__} front end step {k}, first leg: nmse {e:.3e}")
            assert e <= R.MM_NMSE_GATE, (k, e)
        want = chain.twin(x, b_mid)
        e = R.nmse(b.reshape(want.shape), want)
        plog(f"  {chain_cls.__name__} front end step {k}: nmse {e:.3e} (gate {R.MM_NMSE_GATE:.0e})")
        assert e <= R.MM_NMSE_GATE, (k, e)
    assert not np.array_equal(runs[0][0][0][0], runs[0][0][1][0])
