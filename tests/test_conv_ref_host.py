"""CPU tests of the tower ops' ground work: the twins of tests/conv_ref.py against hand-computed vectors and against each other (the f32 twins inside the bounds
derived in conv_ref's docstring, deliberately wrong twins far outside them), and the ggml_lite builders (result shapes, op numbers, op_params)."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as R
import llama_box_amd as L

f16, f32, f64 = np.float16, np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == f16 else np.uint32 if a.dtype == f32 else np.uint64)


# ------------------------------------------------------------------------------------------------ known answers, worked by hand
def test_im2col_3x3_image_2x2_kernel_padding_1():
    """Row (oh, ow) is [x[oh-1, ow-1], x[oh-1, ow], x[oh, ow-1], x[oh, ow]] with zeros outside: OW = OH = (3 + 2 - 1 - 1) / 1 + 1 = 4."""
    x = np.arange(1, 10, dtype=f32).reshape(1, 1, 3, 3)
    want = [[[0, 0, 0, 1], [0, 0, 1, 2], [0, 0, 2, 3], [0, 0, 3, 0]],
            [[0, 1, 0, 4], [1, 2, 4, 5], [2, 3, 5, 6], [3, 0, 6, 0]],
            [[0, 4, 0, 7], [4, 5, 7, 8], [5, 6, 8, 9], [6, 0, 9, 0]],
            [[0, 7, 0, 0], [7, 8, 0, 0], [8, 9, 0, 0], [9, 0, 0, 0]]]
    for dt in (f16, f32, f64):
        got = R.im2col(x, 2, 2, 1, 1, 1, 1, 1, 1, dt)
        assert got.dtype == dt and got.shape == (1, 4, 4, 4) and np.array_equal(got[0], np.array(want, dtype=dt))


def test_conv_1d_window_of_four_samples():
    """Two channels of four samples, K 3, padding 1: row ow is [x0[ow-1 .. ow+1], x1[ow-1 .. ow+1]]; against the kernel [1, 0, -1 | 0.5, 0.5, 0.5] the convolution
    is (x0[ow-1] - x0[ow+1]) + (x1[ow-1] + x1[ow] + x1[ow+1]) / 2."""
    x = np.array([[1, 2, 3, 4], [10, 20, 30, 40]], dtype=f32).reshape(1, 2, 1, 4)
    cols = R.im2col(x, 1, 3, 1, 1, 1, 0, 1, 1, f16)
    want = [[0, 1, 2, 0, 10, 20], [1, 2, 3, 10, 20, 30], [2, 3, 4, 20, 30, 40], [3, 4, 0, 30, 40, 0]]
    assert cols.shape == (1, 1, 4, 6) and np.array_equal(cols[0, 0], np.array(want, dtype=f16))
    kernel = np.array([[1, 0, -1, 0.5, 0.5, 0.5]], dtype=f16)
    for mm in (R.mul_mat64, R.mul_mat32):
        assert np.array_equal(mm(cols[0, 0], kernel).reshape(4), [-2 + 15, -2 + 30, -2 + 45, 3 + 35])
    # stride 2: every other window
    assert np.array_equal(R.im2col(x, 1, 3, 2, 1, 1, 0, 1, 1, f32)[0, 0], np.array(want, dtype=f32)[::2])


def test_mul_mat_known_answer_and_broadcast():
    a = np.array([[1, 2, 3]], dtype=f16)
    b = np.array([[4, 5, 6], [0.5, 0, -1]], dtype=f16)
    assert np.array_equal(R.mul_mat64(a, b).reshape(2, 1), [[32], [-2.5]])
    a2 = np.stack([a, 2 * a])[None]                      # [1, 2, 1, 3]: two src0 batches
    b4 = np.stack([b, b, b, b]).reshape(1, 4, 2, 3)      # four src1 batches: batch i2 reads src0 batch i2 // 2
    got = R.mul_mat32(a2, b4)
    assert got.shape == (1, 4, 2, 1) and np.array_equal(got[0, :, 0, 0], [32, 32, 64, 64])


def test_pool_avg_window_over_the_border():
    """3 x 3 image, k 2 s 2 p 1: the windows hold {1}, {2, 3}, {4, 7}, {5, 6, 8, 9}; AVG divides every one of them by 4."""
    x = np.arange(1, 10, dtype=f32).reshape(1, 1, 3, 3)
    assert np.array_equal(R.pool2d(x, R.AVG, 2, 2, 2, 2, 1, 1)[0, 0], [[0.25, 1.25], [2.75, 7.0]])
    assert np.array_equal(R.pool2d(x, R.MAX, 2, 2, 2, 2, 1, 1)[0, 0], [[1, 3], [7, 9]])
    assert np.array_equal(R.pool2d(x, R.AVG, 2, 2, 2, 2, 1, 1, wrong="valid_divisor")[0, 0], [[1, 2.5], [5.5, 7.0]])
    assert np.array_equal(R.pool2d(-x, R.MAX, 3, 3, 1, 1, 1, 1)[0, 0, 0], [-1, -1, -2])  # (MAX over negatives: the padding is skipped, not read as zero)
    assert np.array_equal(R.pool1d(np.arange(9, dtype=f32), R.AVG, 2), [0.5, 2.5, 4.5, 6.5])  # the ninth sample is dropped
    assert np.array_equal(R.pool1d(np.arange(8, dtype=f32), R.MAX, 4), [3, 7])


def test_pad_known_answer():
    x = np.array([[1, 2], [3, 4]], dtype=f32).reshape(1, 1, 2, 2)
    assert np.array_equal(R.pad(x, (1, 1, 3, 3))[0, 0], [[1, 2, 0], [3, 4, 0], [0, 0, 0]])
    assert np.array_equal(R.pad(x, (2, 1, 2, 2))[1], np.zeros((1, 2, 2)))


def test_upscale_known_answers():
    """2 x 2 -> 4 x 4 bilinear: along an axis the samples sit at -0.25, 0.25, 0.75, 1.25, so a row [p, q] becomes [p, .75 p + .25 q, .25 p + .75 q, q] — the two
    outer samples are clamped to the edge pixel, which the plain linear extension (p - .25 (q - p)) would not give.  Every number below is exact in binary."""
    x = np.array([[0, 4], [8, 12]], dtype=f32).reshape(1, 1, 2, 2)
    want = [[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]]
    for f in (f32, f64):
        got = R.upscale_bilinear(x, (1, 1, 4, 4), f)
        assert got.dtype == f and np.array_equal(got[0, 0], want)
    assert want[0][0] != 0 - 0.25 * 4 - 0.25 * 8  # (the unclamped extension would be -3)
    # nearest 3 -> 7: (int) (i / (7 / 3)) = 0 0 0 1 1 2 2; x 2 repeats every pixel
    row = np.array([10, 20, 30], dtype=f32).reshape(1, 1, 1, 3)
    assert np.array_equal(R.upscale_nearest(row, (1, 1, 1, 7)).ravel(), [10, 10, 10, 20, 20, 30, 30])
    assert np.array_equal(R.upscale_nearest(x, (1, 1, 4, 4))[0, 0], [[0, 0, 4, 4], [0, 0, 4, 4], [8, 8, 12, 12], [8, 8, 12, 12]])
    one = np.array([7.5], dtype=f32).reshape(1, 1, 1, 1)
    assert np.array_equal(R.upscale_bilinear(one, (1, 1, 4, 4)), np.full((1, 1, 4, 4), 7.5, dtype=f32))


# ------------------------------------------------------------------------------------------------ f32 twins against float64 twins; wrong twins far outside
IM2COL_CASES = [  # (N, IC, IH, IW), KH, KW, s0, s1, p0, p1, d0, d1
    ((2, 3, 28, 28), 14, 14, 14, 14, 0, 0, 1, 1), ((1, 2, 7, 5), 3, 3, 1, 1, 1, 1, 1, 1), ((1, 3, 6, 8), 3, 3, 2, 2, 1, 1, 1, 1),
    ((1, 1, 9, 9), 3, 3, 1, 1, 2, 2, 2, 2), ((1, 2, 5, 6), 3, 1, 2, 1, 0, 1, 1, 1), ((2, 8, 1, 30), 1, 3, 2, 1, 1, 0, 1, 1),
]


@pytest.mark.parametrize("case", IM2COL_CASES)
def test_im2col_twins_and_wrong_twins(case):
    shape, *par = case
    x = (np.random.default_rng(1).standard_normal(shape) * 3).astype(f32)
    want = R.im2col(x, *par, f64)
    for dt in (f16, f32):
        got = R.im2col(x, *par, dt)
        assert np.all(np.abs(got.astype(f64) - want) <= R.im2col_gate(want, dt))
    KH, KW, d0, d1 = par[0], par[1], par[6], par[7]
    gate = R.im2col_gate(want, f16)
    if KH > 1 and KW > 1:
        bad = R.im2col(x, *par, f16, wrong="swap_khkw")
        assert np.max(np.abs(bad.astype(f64) - want) / gate) > 100
    if d0 > 1 or d1 > 1:
        bad = R.im2col(x, *par, f16, wrong="no_dilation")
        assert np.max(np.abs(bad.astype(f64) - want) / gate) > 100


@pytest.mark.parametrize("K, na, nb", [(588, 40, 33), (590, 33, 65), (9, 5, 3), (768, 64, 64), (24, 70, 33), (1176, 8, 1)])
def test_mul_mat_f32_twin_inside_the_gate_and_a_rounded_twin_outside(K, na, nb):
    rng = np.random.default_rng(K)
    a, b = rng.standard_normal((na, K)).astype(f16), rng.standard_normal((nb, K)).astype(f16)
    want = R.mul_mat64(a, b)
    assert want.shape == (1, 1, nb, na)
    e = R.nmse(R.mul_mat32(a, b), want)
    assert e <= R.MM_NMSE_GATE and e <= 10 * U2 * K, (e, K)  # (the random-walk estimate u^2 K / 6, with room)
    assert R.nmse(R.mul_mat32(a, b, wrong="round_bf16"), want) > 1000 * R.MM_NMSE_GATE


U2 = R.U * R.U

POOL_CASES = [((1, 1, 4, 4), 2, 2, 2, 2, 0, 0), ((1, 1, 5, 7), 3, 3, 2, 2, 1, 1), ((1, 2, 6, 6), 1, 1, 1, 1, 0, 0), ((1, 1, 7, 6), 2, 3, 1, 2, 0, 0), ((2, 3, 9, 8), 3, 3, 2, 2, 1, 1)]


@pytest.mark.parametrize("case", POOL_CASES)
def test_pool_twins_and_wrong_twin(case):
    shape, *par = case
    x = (np.random.default_rng(2).standard_normal(shape) + 3).astype(f32)
    want = R.pool2d(x, R.AVG, *par, f64)
    got = R.pool2d(x, R.AVG, *par, f32)
    gate = R.pool_avg_gate(x, *par)
    assert got.dtype == f32 and np.all(np.abs(got.astype(f64) - want) <= gate)
    assert np.array_equal(R.pool2d(x, R.MAX, *par, f32).astype(f64), R.pool2d(x, R.MAX, *par, f64))
    if par[4] or par[5]:  # padding: the divisor that leaves it out is far off at the border
        bad = R.pool2d(x, R.AVG, *par, f32, wrong="valid_divisor")
        assert np.max(np.abs(bad.astype(f64) - want) / gate) > 1e5


@pytest.mark.parametrize("src, dst", [((2, 2), (3, 5)), ((16, 16), (27, 11)), ((1, 1), (4, 4)), ((2, 2), (4, 4)), ((5, 3), (10, 9))])
def test_upscale_bilinear_twins_and_wrong_twins(src, dst):
    x = np.random.default_rng(3).standard_normal((1, 2) + src).astype(f32)
    ne = (1, 2) + dst
    want = R.upscale_bilinear(x, ne, f64)
    got = R.upscale_bilinear(x, ne, f32)
    gate = R.upscale_bilinear_gate(x)
    assert got.dtype == f32 and got.shape == ne and np.max(np.abs(got.astype(f64) - want)) <= gate
    if src != (1, 1):
        for wrong in ("no_half_pixel", "nearest"):
            bad = R.upscale_bilinear(x, ne, f32, wrong=wrong)
            assert np.max(np.abs(bad.astype(f64) - want)) > 1000 * gate, wrong


# ------------------------------------------------------------------------------------------------ the builders
def _op_number(H, name):
    for i in range(128):
        if H.ggml_op_name(i) == name.encode():
            return i
    raise KeyError(name)


def _ne(t):
    return list(t.contents.ne)


def _params(t, n):
    return list(t.contents.op_params[:n])


def _same(p, t):
    return C.addressof(p.contents) == C.addressof(t.contents)


def _contig(t):
    tt, exp = t.contents, L.TYPE_SIZE[t.contents.type]
    for d in range(4):
        if tt.nb[d] != exp:
            return False
        exp *= tt.ne[d]
    return True


def test_tower_builders_give_the_stated_shapes_op_numbers_and_op_params(H):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        # IM2COL, 2-D and 1-D
        kern = H.ggml_new_tensor_4d(ctx, L.F16, 14, 14, 3, 32)
        img = H.ggml_new_tensor_4d(ctx, L.F32, 28, 42, 3, 2)
        for dt in (L.F16, L.F32):
            t = H.ggml_im2col(ctx, kern, img, 14, 14, 0, 0, 1, 1, True, dt)
            assert t.contents.op == _op_number(H, "IM2COL") and t.contents.type == dt and _ne(t) == [588, 2, 3, 2] and _contig(t)
            assert _params(t, 7) == [14, 14, 0, 0, 1, 1, 1] and _same(t.contents.src[0], kern) and _same(t.contents.src[1], img)
        t = H.ggml_im2col(ctx, H.ggml_new_tensor_4d(ctx, L.F16, 3, 3, 2, 4), H.ggml_new_tensor_4d(ctx, L.F32, 9, 7, 2, 1), 2, 1, 1, 2, 2, 1, True, L.F16)
        assert _ne(t) == [18, (9 + 2 - 2 * 2 - 1) // 2 + 1, (7 + 4 - 2 - 1) // 1 + 1, 1] and _params(t, 7) == [2, 1, 1, 2, 2, 1, 1]
        k1 = H.ggml_new_tensor_3d(ctx, L.F16, 3, 8, 16)
        wav = H.ggml_new_tensor_3d(ctx, L.F32, 30, 8, 2)
        t = H.ggml_im2col(ctx, k1, wav, 2, 0, 1, 0, 1, 0, False, L.F16)
        assert _ne(t) == [24, 15, 2, 1] and _params(t, 7) == [2, 0, 1, 0, 1, 0, 0]
        # conv_1d: reshape(mul_mat(reshape(im2col), reshape(kernel)))
        c1 = H.ggml_conv_1d(ctx, k1, wav, 2, 1, 1)
        assert c1.contents.op == _op_number(H, "RESHAPE") and _ne(c1) == [15, 16, 2, 1]
        mm = c1.contents.src[0]
        assert mm.contents.op == _op_number(H, "MUL_MAT") and mm.contents.type == L.F32 and _ne(mm) == [30, 16, 1, 1]
        s0, s1 = mm.contents.src[0], mm.contents.src[1]
        assert s0.contents.type == L.F16 and _ne(s0) == [24, 30, 1, 1] and s0.contents.src[0].contents.op == _op_number(H, "IM2COL") and _params(s0.contents.src[0], 7) == [2, 0, 1, 0, 1, 0, 0]
        assert s1.contents.type == L.F16 and _ne(s1) == [24, 16, 1, 1] and _same(s1.contents.src[0], k1)
        # conv_2d: ... and cont(permute(0, 1, 3, 2))
        c2 = H.ggml_conv_2d(ctx, kern, img, 14, 14, 0, 0, 1, 1)
        assert c2.contents.op == _op_number(H, "CONT") and c2.contents.type == L.F32 and _ne(c2) == [2, 3, 32, 2] and _contig(c2)
        pm = c2.contents.src[0]
        assert pm.contents.op == _op_number(H, "PERMUTE") and _params(pm, 4) == [0, 1, 3, 2] and _ne(pm) == [2, 3, 32, 2]
        rs = pm.contents.src[0]
        assert rs.contents.op == _op_number(H, "RESHAPE") and _ne(rs) == [2, 3, 2, 32]
        mm = rs.contents.src[0]
        assert mm.contents.op == _op_number(H, "MUL_MAT") and _ne(mm) == [12, 32, 1, 1]
        assert _ne(mm.contents.src[0]) == [588, 12, 1, 1] and mm.contents.src[0].contents.type == L.F16 and _ne(mm.contents.src[1]) == [588, 32, 1, 1]
        # an f32 kernel gives an f32 im2col
        c3 = H.ggml_conv_1d(ctx, H.ggml_new_tensor_3d(ctx, L.F32, 3, 8, 16), wav, 1, 1, 1)
        assert c3.contents.src[0].contents.src[0].contents.type == L.F32
        # pools
        x = H.ggml_new_tensor_4d(ctx, L.F32, 7, 5, 3, 2)
        for op in (L.POOL_MAX, L.POOL_AVG):
            t = H.ggml_pool_2d(ctx, x, op, 3, 2, 2, 1, 1.0, 0.0)
            assert t.contents.op == _op_number(H, "POOL_2D") and t.contents.type == L.F32 and _ne(t) == [(7 + 2 - 3) // 2 + 1, (5 - 2) // 1 + 1, 3, 2] and _contig(t)
            assert _params(t, 7) == [op, 3, 2, 2, 1, 1, 0] and _same(t.contents.src[0], x)
            t = H.ggml_pool_1d(ctx, H.ggml_new_tensor_2d(ctx, L.F32, 9, 4), op, 2, 2, 0)
            assert t.contents.op == _op_number(H, "POOL_1D") and _ne(t) == [4, 4, 1, 1] and _params(t, 4) == [op, 2, 2, 0]
        assert (L.POOL_MAX, L.POOL_AVG) == (0, 1)
        # pad: no parameters at this snapshot
        t = H.ggml_pad(ctx, x, 1, 0, 2, 3)
        assert t.contents.op == _op_number(H, "PAD") and t.contents.type == L.F32 and _ne(t) == [8, 5, 5, 5] and _params(t, 8) == [0] * 8 and _same(t.contents.src[0], x)
        # upscale / interpolate
        t = H.ggml_upscale(ctx, x, 2, L.SCALE_NEAREST)
        assert t.contents.op == _op_number(H, "UPSCALE") and _ne(t) == [14, 10, 3, 2] and _params(t, 1) == [0]
        t = H.ggml_interpolate(ctx, x, 27, 11, 3, 2, L.SCALE_BILINEAR)
        assert t.contents.op == _op_number(H, "UPSCALE") and t.contents.type == L.F32 and _ne(t) == [27, 11, 3, 2] and _params(t, 1) == [1] and _contig(t)
        t = H.ggml_interpolate(ctx, x, 14, 10, 3, 2, L.SCALE_BILINEAR | L.SCALE_ALIGN_CORNERS)
        assert _params(t, 1) == [257]
        assert (L.SCALE_NEAREST, L.SCALE_BILINEAR, L.SCALE_BICUBIC, L.SCALE_ALIGN_CORNERS) == (0, 1, 2, 256)
        # the op numbers the backend switches on are the header's
        hdr = _header_ops()
        for n in ("IM2COL", "POOL_1D", "POOL_2D", "UPSCALE", "PAD"):
            assert _op_number(H, n) == hdr[n], n
    finally:
        H.ggml_free(ctx)


def _header_ops():
    import os
    ops, on = [], False
    with open(os.path.join(L.REPO, "include", "ggml_abi.h")) as f:
        for line in f:
            s = line.strip()
            if s.startswith("enum ggml_op {"):
                on = True
            elif on and s.startswith("}"):
                break
            elif on and s.startswith("GGML_OP_"):
                ops.append(s.split(",")[0].split("=")[0].strip()[len("GGML_OP_"):])
    return {n: i for i, n in enumerate(ops)}
