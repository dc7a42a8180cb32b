"""CPU: the NumPy twins of tests/diffusion_ref.py (GROUP_NORM, TIMESTEP_EMBEDDING, DIAG_MASK_INF, LEAKY_RELU) on known answers, the ceil rule of the channel
groups on hand-made cases, the host mirror's new builders, and the two constants the edge shapes follow against csrc/kernels.h.  No GPU, no oracle (it has none
of these ops)."""
import ctypes as C
import math

import numpy as np
import pytest

import act_norm_ref as A
import diffusion_ref as R
import llama_box_amd as L

f32 = np.float32


def test_constants_follow_the_source():
    src = R.source_constants()
    assert R.GN_CHUNK == src["MI_GN_CHUNK"] and R.GN_RESIDENT_MAX == src["MI_GN_RESIDENT_MAX"], src
    assert src["MI_GN_ROUTED_MAX"] <= src["MI_GN_RESIDENT_MAX"] and src["MI_GN_RESIDENT_MAX"] == 1024 * 40 and src["MI_GN_CHUNK"] % 1024 == 0, src


@pytest.mark.parametrize("C_,G,want", [
    (8, 4, [(0, 2), (2, 4), (4, 6), (6, 8)]),
    (7, 4, [(0, 2), (2, 4), (4, 6), (6, 7)]),          # a shorter last group
    (10, 4, [(0, 3), (3, 6), (6, 9), (9, 10)]),
    (4, 1, [(0, 4)]), (4, 4, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    (320, 32, [(10 * g, 10 * g + 10) for g in range(32)]),
    (5, 4, None),                                      # cpg 2: the fourth group would start at channel 6
    (9, 4, None),                                      # cpg 3: the fourth group would start at channel 9
    (3, 4, None), (4, 0, None), (4, -1, None),
])
def test_ceil_rule(C_, G, want):
    assert R.group_ranges(C_, G) == want


def test_group_norm_twin_against_float64():
    rng = np.random.default_rng(3)
    for shape, G in (((2, 8, 3, 5), 4), ((1, 7, 4, 4), 4), ((1, 6, 2, 3), 1), ((2, 4, 5, 5), 4)):
        x = (rng.standard_normal(shape) * 3 + 1.5).astype(f32)
        y, ref = R.group_norm(x, G, 1e-6), R.group_norm64(x, G, 1e-6)
        for n, c0, c1 in R._groups(x, G):
            d = R.row_distance(y[n, c0:c1].reshape(1, -1), ref[n, c0:c1].reshape(1, -1))[0]
            assert d <= 4 * A.U24 + A.norm_extra(x[n, c0:c1].reshape(1, -1)), (shape, G, n, c0, d)  # the twin's own f32 steps: the mean's rounding and v's
    # the groups are what the ceil rule says: a twin that normalised whole channels or the whole tensor is far outside
    x = (rng.standard_normal((1, 7, 4, 4)) * np.arange(1, 8).reshape(1, 7, 1, 1)).astype(f32)
    assert np.max(np.abs(R.group_norm(x, 4, 1e-6) - R.group_norm64(x, 7, 1e-6))) > 1e-2
    assert np.max(np.abs(R.group_norm(x, 4, 1e-6) - R.group_norm64(x, 1, 1e-6))) > 1e-2
    # groups of one value: 0 with eps, 0 * inf = NaN without; a constant group alike
    one = rng.standard_normal((1, 4, 1, 1)).astype(f32)
    assert np.all(R.group_norm(one, 4, 1e-6) == 0) and np.all(np.isnan(R.group_norm(one, 4, 0.0)))
    const = np.full((1, 4, 3, 3), 2.5, f32)
    assert np.all(R.group_norm(const, 2, 1e-6) == 0) and np.all(np.isnan(R.group_norm(const, 2, 0.0)))
    # the excess is in units of the gate
    x = rng.standard_normal((2, 8, 3, 5)).astype(f32)
    want = R.group_norm(x, 4, 1e-6)
    assert R.group_norm_excess(want.astype(f32), x, 4, 1e-6)[0] <= 1.0
    off = want.copy()
    off[1, 2, 0, 0] += 40 * A.U24 * np.max(np.abs(want[1, 2:4]))
    assert R.group_norm_excess(off.astype(f32), x, 4, 1e-6)[0] > 1.0
    w = rng.standard_normal(8).astype(f32)
    assert np.array_equal(R.channel_binary("mul", x, w)[1, 3], x[1, 3] * w[3]) and np.array_equal(R.channel_binary("add", x, w)[0, 7], x[0, 7] + w[7])


def test_diag_mask_inf_twin():
    x = np.arange(1, 13, dtype=f32).reshape(1, 3, 4)  # 3 rows (j) of 4 columns (i)
    ninf = -np.inf
    assert R.diag_mask_inf(x, 0)[0].tolist() == [[1, ninf, ninf, ninf], [5, 6, ninf, ninf], [9, 10, 11, ninf]]
    assert R.diag_mask_inf(x, 2)[0].tolist() == [[1, 2, 3, ninf], [5, 6, 7, 8], [9, 10, 11, 12]]
    assert np.array_equal(R.diag_mask_inf(x, 3), x) and x[0, 0, 1] == 2  # (the argument is not written)


def test_leaky_relu_twin():
    sub = f32(2.0 ** -149)
    x = np.array([2.0, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub], f32)
    y = R.leaky_relu(x, 0.2)
    assert y[0] == 2.0 and y[1] == f32(0.2) * f32(-2.0) and y[4] == np.inf and y[5] == -np.inf and y[7] == sub
    assert [bool(np.signbit(v)) for v in y[2:4]] == [False, False] and y[2] == 0 and y[3] == 0 and y[6] == 0  # +0 + -0 = +0; a NaN gives way to the zeros
    assert y[8] == f32(0.2) * -sub  # 0.2 of the smallest subnormal rounds to -0
    y0 = R.leaky_relu(x, 0.0)
    assert y0[1] == 0 and y0[3] == 0 and np.isnan(y0[5]) and not np.signbit(y0[1])  # 0 * -inf
    assert R.leaky_relu(x, -0.5)[1] == 1.0 and R.leaky_relu(x, -0.5)[5] == np.inf


def test_timestep_embedding_twin():
    y, a = R.timestep_embedding([0.0, 1.0, 999.0], 4, 10000)
    assert y.shape == (3, 4) and y[0].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert y[1].tolist() == pytest.approx([math.cos(1.0), math.cos(0.01), math.sin(1.0), math.sin(0.01)], abs=1e-15)
    assert a[2].tolist() == pytest.approx([999.0, 9.99, 999.0, 9.99])
    y5, a5 = R.timestep_embedding([0.5], 5, 10000)
    assert y5.shape == (1, 6) and y5[0, 4] == 0 and y5[0, 5] == 0 and a5[0, 4] == 0
    assert R.timestep_embedding([3.0], 2, 100)[0][0].tolist() == pytest.approx([math.cos(3.0), math.sin(3.0)], abs=1e-15)
    assert R.te_rel(10000) == pytest.approx((4 * math.log(10000) + 4) * 2.0 ** -23)
    good = y.astype(f32)
    assert np.all(R.timestep_excess(good, [0.0, 1.0, 999.0], 4, 10000) <= 1.0)
    bad = good.copy()
    bad[1, 0] += f32(64 * 2.0 ** -23)
    assert R.timestep_excess(bad, [0.0, 1.0, 999.0], 4, 10000)[1, 0] > 1.0
    nz = y5.astype(f32)
    nz[0, 5] = 1e-30
    assert R.timestep_excess(nz, [0.5], 5, 10000)[0, 5] == np.inf


def test_builders(built, H):
    names = (R.OP_GROUP_NORM, R.OP_DIAG_MASK_INF, R.OP_DIAG_MASK_ZERO, R.OP_TIMESTEP_EMBEDDING, R.OP_LEAKY_RELU)
    assert tuple(H.ggml_op_name(o) for o in names) == (b"GROUP_NORM", b"DIAG_MASK_INF", b"DIAG_MASK_ZERO", b"TIMESTEP_EMBEDDING", b"LEAKY_RELU")
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        def same(p, q):
            return C.addressof(p.contents) == C.addressof(q.contents)

        def as_f32(v):
            return np.int32(v).view(f32)

        a = H.ggml_new_tensor_4d(ctx, L.F32, 6, 5, 8, 2)
        for fn, view in ((H.ggml_group_norm, False), (H.ggml_group_norm_inplace, True)):
            n = fn(ctx, a, 4, 1e-6).contents
            assert n.op == R.OP_GROUP_NORM and n.op_params[0] == 4 and as_f32(n.op_params[1]) == f32(1e-6) and same(n.src[0], a) and not n.src[1]
            assert list(n.ne) == [6, 5, 8, 2] and list(n.nb) == list(a.contents.nb) and n.type == L.F32
            assert (bool(n.view_src) and same(n.view_src, a)) if view else not n.view_src
        for dim, width in ((2, 2), (5, 6), (320, 320)):
            t = H.ggml_new_tensor_1d(ctx, L.F32, 3)
            e = H.ggml_timestep_embedding(ctx, t, dim, 10000).contents
            assert e.op == R.OP_TIMESTEP_EMBEDDING and e.op_params[0] == dim and e.op_params[1] == 10000 and same(e.src[0], t) and not e.view_src
            assert list(e.ne) == [width, 3, 1, 1] and e.type == L.F32
        kq = H.ggml_new_tensor_3d(ctx, L.F32, 7, 5, 3)
        for fn, view in ((H.ggml_diag_mask_inf, False), (H.ggml_diag_mask_inf_inplace, True)):
            m = fn(ctx, kq, 2).contents
            assert m.op == R.OP_DIAG_MASK_INF and m.op_params[0] == 2 and same(m.src[0], kq) and list(m.ne) == [7, 5, 3, 1] and m.type == L.F32
            assert (bool(m.view_src) and same(m.view_src, kq)) if view else not m.view_src
        wide = H.ggml_new_tensor_3d(ctx, L.F32, 9, 5, 3)
        sv = H.ggml_view_3d(ctx, wide, 7, 5, 3, 9 * 4, 9 * 5 * 4, 4)
        m = H.ggml_diag_mask_inf_inplace(ctx, sv, 0).contents  # a view of a view: the root is the leaf, the strides and the offset are the view's
        assert same(m.view_src, wide) and m.view_offs == 4 and list(m.nb) == [4, 36, 180, 540]
        m = H.ggml_diag_mask_inf(ctx, sv, 0).contents          # out of place: a dense result
        assert not m.view_src and list(m.nb) == [4, 28, 140, 420]
        for inplace in (False, True):
            r = H.ggml_leaky_relu(ctx, a, 0.2, inplace).contents
            assert r.op == R.OP_LEAKY_RELU and as_f32(r.op_params[0]) == f32(0.2) and same(r.src[0], a) and list(r.ne) == [6, 5, 8, 2]
            assert (bool(r.view_src) and same(r.view_src, a)) if inplace else not r.view_src
    finally:
        H.ggml_free(ctx)
