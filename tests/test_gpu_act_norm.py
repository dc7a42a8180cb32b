"""GPU: csrc/ops_act.hip through the C-ABI — NORM (+ the fused MUL / ADD), GELU / GELU_QUICK / GELU_ERF and the gated units REGLU / GEGLU / GEGLU_QUICK /
GEGLU_ERF — against the NumPy twins of tests/act_norm_ref.py (the CPU oracle has none of these ops).

  * GELU, GELU_QUICK, REGLU, GEGLU, GEGLU_QUICK: bit equality (NaN by isnan).  The kernels look the same two tables up that the twin builds from this
    process's libm; after the lookup comes at most one f32 product.
  * GELU_ERF, GEGLU_ERF: absolute error <= 16 * 2^-24 |x| |g| + 1 ulp of the result (act_norm_ref.ERF_K, reasoned there).
  * NORM: error over the row's largest |y| <= 2 * 2^-23 + 2^-23 |mean| / max |x - mean| (act_norm_ref.NORM_GATE and norm_extra, reasoned there).

Every test here fails on a backend without these ops: harness.G.compute raises supports_op=false at the first new node.
"""
import itertools

import numpy as np
import pytest

import act_norm_ref as A
import harness as T
import llama_box_amd as L
import ops_ref as R

pytestmark = pytest.mark.gpu


def _run(target, build):
    """build(g) -> (outs, reads); the arrays of the reads after one compute."""
    g = T.G(target)
    try:
        outs, reads = build(g)
        g.compute(list(outs))
        return [g.read(t) for t in reads]
    finally:
        g.free()


def _assert_bits(cid, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (cid, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(A.bits(got).reshape(-1) != A.bits(want).reshape(-1))
    assert bad.size == 0, f"{cid}: kernel and twin differ in {bad.size} of {got.size} elements, first at {bad[:5]}: kernel {got.reshape(-1)[bad[:5]]} twin {want.reshape(-1)[bad[:5]]}"


def _glu_node(g, op, form, tx, tg=None):
    fn = getattr(g.H, f"ggml_{A.GLU_BUILDER[op]}{form}")
    return fn(g.ctx, tx, tg) if form == "_split" else fn(g.ctx, tx)


# ------------------------------------------------------------------------------------------------ 1. supports_op
def test_supports_op(backend, H):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        a, b = H.ggml_new_tensor_2d(ctx, L.F32, 64, 3), H.ggml_new_tensor_2d(ctx, L.F32, 64, 3)
        a3, b3 = H.ggml_new_tensor_3d(ctx, L.F32, 64, 2, 3), H.ggml_new_tensor_3d(ctx, L.F32, 64, 2, 3)
        h, h2 = H.ggml_new_tensor_2d(ctx, L.F16, 64, 3), H.ggml_new_tensor_2d(ctx, L.F16, 64, 3)
        assert ok(H.ggml_norm(ctx, a, 1e-5)) and ok(H.ggml_norm(ctx, a3, 1e-5))
        assert ok(H.ggml_norm(ctx, H.ggml_view_2d(ctx, a, 32, 3, 64 * 4, 4), 1e-5))  # strided rows at an odd offset
        for fn in (H.ggml_gelu, H.ggml_gelu_quick, H.ggml_gelu_erf):
            assert ok(fn(ctx, a)) and not ok(fn(ctx, h)) and not ok(fn(ctx, H.ggml_transpose(ctx, a)))
        for stem in A.GLU_BUILDER.values():
            one, swp, spl = (getattr(H, f"ggml_{stem}{form}") for form in ("", "_swapped", "_split"))
            assert ok(one(ctx, a)) and ok(swp(ctx, a)) and ok(spl(ctx, a, b)), stem
            assert ok(spl(ctx, a3, b3)), stem  # dense 3-D rows
            assert not ok(spl(ctx, h, h2)) and not ok(one(ctx, h)), stem  # f16 operands
            assert not ok(one(ctx, H.ggml_transpose(ctx, a))), stem  # nb[0] != 4
            wide = H.ggml_new_tensor_3d(ctx, L.F32, 64, 3, 3)
            sparse = H.ggml_view_3d(ctx, wide, 64, 2, 3, 64 * 4, 64 * 4 * 3, 0)  # two of three rows of every matrix: not one row stride apart
            assert not ok(spl(ctx, sparse, b3)) and not ok(spl(ctx, a3, sparse)), stem
            assert not ok(one(ctx, a3)), stem  # the one-tensor form is 2-D only
        oai = H.ggml_swiglu_split(ctx, a, b)
        assert ok(oai)
        oai.contents.op_params[0] = A.GLU["SWIGLU_OAI"]
        assert not ok(oai)
        assert not ok(H.ggml_norm(ctx, h, 1e-5)) and not ok(H.ggml_norm(ctx, H.ggml_transpose(ctx, a), 1e-5))
    finally:
        H.ggml_free(ctx)


# ------------------------------------------------------------------------------------------------ 2. GELU, GELU_QUICK
@pytest.mark.parametrize("name", ["GELU", "GELU_QUICK"])
def test_gelu_tables_bit_exact(backend, H, plog, name):
    x = A.gelu_input()
    fn = {"GELU": H.ggml_gelu, "GELU_QUICK": H.ggml_gelu_quick}[name]

    def build(g):
        r = fn(g.ctx, g.new(L.F32, [A.GELU_N], x))
        return [r], [r]

    got = _run(backend, build)[0]
    want = {"GELU": A.gelu, "GELU_QUICK": A.gelu_quick}[name](x).reshape(1, 1, 1, -1)
    plog(f"  act {name}: {got.size} values, {int(np.count_nonzero(A.bits(got) != A.bits(want)))} differ from the twin")
    _assert_bits(name, got, want)


# ------------------------------------------------------------------------------------------------ 3. GELU_ERF, GEGLU_ERF
def test_gelu_erf_within_the_absolute_gate(backend, H, plog):
    x = A.gelu_input()

    def build(g):
        r = H.ggml_gelu_erf(g.ctx, g.new(L.F32, [A.GELU_N], x))
        return [r], [r]

    got = _run(backend, build)[0].reshape(-1)
    e = A.erf_excess(got, x)
    k = int(np.argmax(e))
    plog(f"  act GELU_ERF: worst {float(e[k]):.4g} of the gate (16 * 2^-24 |x| + 1 ulp) at x = {x[k]!r}: kernel {got[k]!r}, float64 twin {float(A.gelu_erf64(x[k])):.9g}")
    assert float(e[k]) <= 1.0, f"GELU_ERF: {float(e[k]):.6g} of the gate at x = {x[k]!r}: kernel {got[k]!r}"


@pytest.mark.parametrize("form", ["_split", "", "_swapped"])
def test_geglu_erf_within_the_absolute_gate(backend, H, plog, form):
    nc, rows = A.GLU_NC[2], 3
    x, gm = A.glu_operands(nc, rows, 8300)
    # (a subnormal x: 0.5f * x is rounded on f32's ABSOLUTE grid, 2^-150 off, and g multiplies that — the definition's own step, which the gate's one ulp of the
    # result holds only for |g| <= 1)
    gm = np.where(np.abs(x) < R.FLT_MIN, np.clip(gm, -1.0, 1.0), gm).astype(np.float32)
    # (x < -5: 1.0f + erff(.) is exactly 0 in f32 where float64 still holds 1e-7 and less — an infinite g makes that NaN against -inf, again the definition's own)
    gm = np.where(np.isinf(gm) & (x < -5.0), np.sign(gm), gm).astype(np.float32)

    def build(g):
        if form == "_split":
            r = _glu_node(g, "GEGLU_ERF", form, g.new(L.F32, [nc, rows], x), g.new(L.F32, [nc, rows], gm))
        else:
            r = _glu_node(g, "GEGLU_ERF", form, g.new(L.F32, [2 * nc, rows], np.concatenate([gm, x] if form == "_swapped" else [x, gm], axis=1)))
        return [r], [r]

    got = _run(backend, build)[0].reshape(rows, nc)
    e = A.erf_excess(got, x, gm)
    k = np.unravel_index(int(np.argmax(e)), e.shape)
    plog(f"  act GEGLU_ERF{form}: worst {float(e[k]):.4g} of the gate (16 * 2^-24 |x| |g| + 1 ulp) at x = {x[k]!r}, g = {gm[k]!r}")
    assert float(e[k]) <= 1.0, f"GEGLU_ERF{form}: {float(e[k]):.6g} of the gate at x = {x[k]!r}, g = {gm[k]!r}: kernel {got[k]!r}"


# ------------------------------------------------------------------------------------------------ 4. GLU, bit-exact
GLU_BITS = ("REGLU", "GEGLU", "GEGLU_QUICK")


@pytest.mark.parametrize("op,form,nc", list(itertools.product(GLU_BITS, ["_split", "", "_swapped"], A.GLU_NC)), ids=lambda v: str(v) or "halves")
def test_glu_bit_exact(backend, H, plog, op, form, nc):
    for rows in (1, 3):
        x, gm = A.glu_operands(nc, rows, 8400 + nc + rows)

        def build(g):
            if form == "_split":
                r = _glu_node(g, op, form, g.new(L.F32, [nc, rows], x), g.new(L.F32, [nc, rows], gm))
            else:
                r = _glu_node(g, op, form, g.new(L.F32, [2 * nc, rows], np.concatenate([gm, x] if form == "_swapped" else [x, gm], axis=1)))
            return [r], [r]

        _assert_bits(f"{op}{form} nc={nc} rows={rows}", _run(backend, build)[0], A.glu(op, x, gm).reshape(1, 1, rows, nc))


@pytest.mark.parametrize("op", GLU_BITS)
def test_glu_layouts_bit_exact(backend, H, plog, op):
    nc = A.GLU_NC[2]  # chunk + 4: a second, partial chunk
    # dense 3-D split [nc, 2, 3]
    x, gm = A.glu_operands(nc, 6, 8500)

    def build_3d(g):
        r = _glu_node(g, op, "_split", g.new(L.F32, [nc, 2, 3], x), g.new(L.F32, [nc, 2, 3], gm))
        return [r], [r]

    _assert_bits(f"{op} dense 3-D", _run(backend, build_3d)[0], A.glu(op, x, gm).reshape(1, 3, 2, nc))
    # g starts 4 bytes off 16-byte alignment (nc % 4 == 0 all the same): the scalar path
    x, gm = A.glu_operands(nc, 3, 8501)
    base = np.full((3, nc + 4), 1000.0, np.float32)
    base[:, 1:nc + 1] = gm

    def build_off(g):
        tg = H.ggml_view_2d(g.ctx, g.new(L.F32, [nc + 4, 3], base), nc, 3, (nc + 4) * 4, 4)
        r = _glu_node(g, op, "_split", g.new(L.F32, [nc, 3], x), tg)
        return [r], [r]

    _assert_bits(f"{op} g off alignment", _run(backend, build_off)[0], A.glu(op, x, gm).reshape(1, 1, 3, nc))
    # padded row strides on both operands (aligned: the float4 path over strided rows)
    bx, bg = np.full((3, nc + 8), -1000.0, np.float32), np.full((3, nc + 8), 1000.0, np.float32)
    bx[:, :nc], bg[:, :nc] = x, gm

    def build_pad(g):
        tx = H.ggml_view_2d(g.ctx, g.new(L.F32, [nc + 8, 3], bx), nc, 3, (nc + 8) * 4, 0)
        tg = H.ggml_view_2d(g.ctx, g.new(L.F32, [nc + 8, 3], bg), nc, 3, (nc + 8) * 4, 0)
        r = _glu_node(g, op, "_split", tx, tg)
        return [r], [r]

    _assert_bits(f"{op} padded rows", _run(backend, build_pad)[0], A.glu(op, x, gm).reshape(1, 1, 3, nc))


def test_geglu_both_sides_of_ten(backend, H, plog):
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    ten = np.float32(10.0)
    x = np.array([10.0, np.nextafter(ten, dn), np.nextafter(ten, up), 9.99, 10.01, 12.5, 100.0, 65520.0, 1e30,
                  -10.0, np.nextafter(-ten, up), np.nextafter(-ten, dn), -9.99, -10.01, -12.5, -100.0, -65520.0, -1e30], np.float32)
    gm = np.full_like(x, 3.0)

    def build(g):
        r = _glu_node(g, "GEGLU", "_split", g.new(L.F32, [len(x), 1], x), g.new(L.F32, [len(x), 1], gm))
        return [r], [r]

    got = _run(backend, build)[0]
    _assert_bits("GEGLU at +-10", got, A.glu("GEGLU", x, gm).reshape(1, 1, 1, -1))
    assert got.reshape(-1)[5] == np.float32(37.5) and got.reshape(-1)[14] == 0  # x >= 10: x * g; x <= -10: +0 * g


# ------------------------------------------------------------------------------------------------ 5. NORM
def _norm_case(cid, x, eps, build, expect_x=None):
    xe = x if expect_x is None else expect_x
    return A.Case(cid, "norm", build, lambda: [A.norm(xe, eps).reshape((1,) * (4 - xe.ndim) + xe.shape)], "row", extra=A.norm_extra(xe))


def _norm_cases():
    out = []
    for ne0, rows, eps in itertools.product(A.NORM_NE0, (1, 3), (1e-5, 0.0)):
        rng = np.random.default_rng(9000 + ne0 + rows)
        x = (rng.standard_normal((rows, ne0)) * rng.uniform(0.5, 30.0, (rows, 1)) + rng.uniform(-2.0, 2.0, (rows, 1))).astype(np.float32)

        def build(g, x=x, ne0=ne0, rows=rows, eps=eps):
            r = g.H.ggml_norm(g.ctx, g.new(L.F32, [ne0, rows], x), eps)
            return [r], [r]

        out.append(_norm_case(f"norm-{ne0}x{rows}-eps{eps:g}", x, eps, build))
    trip = A.NORM_NE0[3]
    # a 4-D strided view: rows of trip + 4 values inside rows of trip + 12, two of three rows, two of two matrices, two batches
    ne0, pad = trip + 4, 8
    rng = np.random.default_rng(9100)
    base = (rng.standard_normal((2, 2, 3, ne0 + pad)) * 5 + 1).astype(np.float32)
    base[..., ne0:] = 1000.0

    def build_4d(g):
        rb = (ne0 + pad) * 4
        v = g.H.ggml_view_4d(g.ctx, g.new(L.F32, [ne0 + pad, 3, 2, 2], base), ne0, 2, 2, 2, rb, rb * 3, rb * 6, 0)
        r = g.H.ggml_norm(g.ctx, v, 1e-5)
        return [r], [r]

    out.append(_norm_case("norm-4d-strided-view", base, 1e-5, build_4d, np.ascontiguousarray(base[:, :, :2, :ne0])))
    # row starts 4 bytes off 16-byte alignment: the scalar path although ne0 % 4 == 0
    for ne0 in (trip, 2 * trip):
        rng = np.random.default_rng(9110 + ne0)
        b2 = (rng.standard_normal((3, ne0 + 4)) * 3 - 0.5).astype(np.float32)
        b2[:, 0] = -1000.0
        b2[:, ne0 + 1:] = 1000.0

        def build_off(g, b2=b2, ne0=ne0):
            v = g.H.ggml_view_2d(g.ctx, g.new(L.F32, [ne0 + 4, 3], b2), ne0, 3, (ne0 + 4) * 4, 4)
            r = g.H.ggml_norm(g.ctx, v, 1e-5)
            return [r], [r]

        out.append(_norm_case(f"norm-view-offset4-{ne0}", b2, 1e-5, build_off, np.ascontiguousarray(b2[:, 1:ne0 + 1])))
    # in place (ggml_norm_inplace): scalar path, register path, the re-reading path
    for ne0 in (100, trip, 2 * trip):
        rng = np.random.default_rng(9120 + ne0)
        xi = (rng.standard_normal((3, ne0)) * 7 + 0.25).astype(np.float32)

        def build_inplace(g, xi=xi, ne0=ne0):
            a = g.new(L.F32, [ne0, 3], xi)
            r = A._as_view(g.H.ggml_norm(g.ctx, a, 1e-5), a, [4, 4 * ne0, 12 * ne0, 12 * ne0], 0)
            return [r], [r]

        out.append(_norm_case(f"norm-inplace-{ne0}", xi, 1e-5, build_inplace))
    # constant rows: 0 with eps, NaN (0 * inf) without; on the scalar and both float4 paths
    for ne0, eps in itertools.product((100, trip, trip + 4), (1e-5, 0.0)):
        xc = np.repeat(np.array([[3.25], [-1e20], [0.0]], np.float32), ne0, axis=1)

        def build_c(g, xc=xc, ne0=ne0, eps=eps):
            r = g.H.ggml_norm(g.ctx, g.new(L.F32, [ne0, 3], xc), eps)
            return [r], [r]

        out.append(_norm_case(f"norm-constant-{ne0}-eps{eps:g}", xc, eps, build_c))
    # a mean 1000 times the spread: the case's own term carries the gate
    rng = np.random.default_rng(9130)
    xm = (1000.0 + rng.uniform(-1.0, 1.0, (3, trip))).astype(np.float32)

    def build_m(g):
        r = g.H.ggml_norm(g.ctx, g.new(L.F32, [trip, 3], xm), 1e-5)
        return [r], [r]

    out.append(_norm_case("norm-mean-1000x-spread", xm, 1e-5, build_m))
    return out


@pytest.mark.parametrize("case", _norm_cases(), ids=repr)
def test_norm_within_the_gate(backend, H, plog, case):
    got, want = _run(backend, case.build)[0], case.expect()[0]
    assert got.shape == want.shape, (case.id, got.shape, want.shape)
    gate = A.NORM_GATE + case.extra
    d = float(np.max(A.row_distance(got, want)))
    plog(f"  act {case.id}: kernel {d:.4g} of the row's maximum from the float64 twin, gate {gate:.4g} (2 * 2^-23 + {case.extra:.3g})")
    assert d <= gate, f"{case.id}: kernel is {d:.6g} of the row's maximum from the twin, the gate is {gate:.6g}"
    if "constant" in case.id:
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(got[~np.isnan(got)] == 0)


# ------------------------------------------------------------------------------------------------ 6. fusion
def _launches(backend, build, fusion):
    """(arrays of the reads, kernel launches, fused nodes) of one graph at option fusion = 0 / 1."""
    backend.set_option("fusion", fusion)
    try:
        k0, f0 = backend.stat("kernel_launches"), backend.stat("fused_nodes")
        got = _run(backend, build)
        return got, backend.stat("kernel_launches") - k0, backend.stat("fused_nodes") - f0
    finally:
        backend.set_option("fusion", 1)


@pytest.mark.parametrize("ne0,rows,w_left,b_left,bias", [(100, 3, False, False, True), (4096, 1, False, True, True), (4100, 1, True, False, True), (4096, 1, True, True, True),
                                                         (8192, 3, False, False, False), (100, 1, True, False, False)])
def test_norm_affine_fusion(backend, H, plog, ne0, rows, w_left, b_left, bias):
    rng = np.random.default_rng(9200 + ne0 + rows)
    x = (rng.standard_normal((rows, ne0)) * 4 + 0.5).astype(np.float32)
    w, b = rng.uniform(0.5, 1.5, ne0).astype(np.float32), rng.standard_normal(ne0).astype(np.float32)

    def build(g):  # (w or b on the left: a single row — ggml's broadcast rule wants the right operand to repeat into the left)
        n = H.ggml_norm(g.ctx, g.new(L.F32, [ne0, rows], x), 1e-5)
        tw = g.new(L.F32, [ne0], w)
        r = H.ggml_mul(g.ctx, tw, n) if w_left else H.ggml_mul(g.ctx, n, tw)
        if bias:
            tb = g.new(L.F32, [ne0], b)
            r = H.ggml_add(g.ctx, tb, r) if b_left else H.ggml_add(g.ctx, r, tb)
        return [r], [r]

    def build_plain(g):
        r = H.ggml_norm(g.ctx, g.new(L.F32, [ne0, rows], x), 1e-5)
        return [r], [r]

    plain = _run(backend, build_plain)[0]
    want = R.binary("mul", plain, w)
    want = R.binary("add", want, b) if bias else want
    fused, k1, f1 = _launches(backend, build, 1)
    unfused, k0, f0 = _launches(backend, build, 0)
    plog(f"  act norm-affine ne0={ne0} rows={rows} w_left={w_left} b_left={b_left} bias={bias}: launches fused {k1} / unfused {k0}, fused nodes {f1} / {f0}")
    assert (k1, f1) == (1, 2 if bias else 1) and (k0, f0) == (3 if bias else 2, 0)
    _assert_bits("norm-affine fused vs unfused", fused[0], unfused[0])
    _assert_bits("norm-affine vs the MUL / ADD of the kernel's own NORM", fused[0], want.reshape(fused[0].shape))


def test_norm_with_a_second_reader_is_not_fused(backend, H, plog):
    ne0, rows = 4096, 3
    rng = np.random.default_rng(9300)
    x = (rng.standard_normal((rows, ne0)) * 4 + 0.5).astype(np.float32)
    w, b = rng.uniform(0.5, 1.5, ne0).astype(np.float32), rng.standard_normal(ne0).astype(np.float32)

    def build(g):
        n = H.ggml_norm(g.ctx, g.new(L.F32, [ne0, rows], x), 1e-5)
        r = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, n, g.new(L.F32, [ne0], w)), g.new(L.F32, [ne0], b))
        s = H.ggml_scale(g.ctx, n, 2.0)
        return [r, s], [r, s]

    def build_plain(g):
        r = H.ggml_norm(g.ctx, g.new(L.F32, [ne0, rows], x), 1e-5)
        return [r], [r]

    plain = _run(backend, build_plain)[0]
    (r, s), k, f = _launches(backend, build, 1)
    assert (k, f) == (4, 0), (k, f)
    _assert_bits("second reader: affine", r, R.binary("add", R.binary("mul", plain, w), b).reshape(r.shape))
    _assert_bits("second reader: scale", s, R.scale(plain, 2.0).reshape(s.shape))


# ------------------------------------------------------------------------------------------------ 7. chains
K_, N_ = 256, 512


def _four_times(backend, g, outs, reads):
    """One graph computed four times on one backend: the arrays of the first run; every later run must repeat them bit for bit, and the replay path
    (a captured hipGraph, which carries the GELU tables' address) must have run."""
    H = g.H
    gl0 = backend.stat("graph_launches")
    g.compute(list(outs))
    first = [g.read(t) for t in reads]
    for k in range(3):
        assert H.ggml_backend_graph_compute(backend.backend, g.gf) == 0
        for t, f in zip(reads, first):
            _assert_bits(f"run {k + 2} against run 1", g.read(t), f)
    assert backend.stat("graph_launches") > gl0, "no replayed hipGraph among four computes of one graph"
    return first


def _oracle_mm(qt, wbytes, Kd, Nd, act, bias=None):
    def build(g):
        r = g.H.ggml_mul_mat(g.ctx, g.new(qt, [Kd, Nd], wbytes), g.new(L.F32, [Kd, act.shape[-2]], act))
        if bias is not None:
            r = g.H.ggml_add(g.ctx, r, g.new(L.F32, [Nd], bias))
        return [r], [r]

    return _run("oracle", build)[0]


@pytest.mark.parametrize("cols", [1, 5, 33])
def test_encoder_ffn_chain(backend, H, plog, cols):
    """MUL_MAT(q8_0) + b -> GELU -> MUL_MAT(q8_0) + b -> ADD(residual) -> NORM * w + b"""
    rng = np.random.default_rng(9400 + cols)
    x = (rng.standard_normal((cols, K_)) * 2).astype(np.float32)
    w1, w2 = T.rand_weight(L.Q8_0, K_, N_, rng), T.rand_weight(L.Q8_0, N_, K_, rng)
    b1, b2 = (rng.standard_normal(N_) * 0.5).astype(np.float32), (rng.standard_normal(K_) * 0.5).astype(np.float32)
    nw, nb = rng.uniform(0.5, 1.5, K_).astype(np.float32), rng.standard_normal(K_).astype(np.float32)
    g = T.G(backend)
    try:
        tx = g.new(L.F32, [K_, cols], x)
        h1 = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(L.Q8_0, [K_, N_], w1), tx), g.new(L.F32, [N_], b1))
        ge = H.ggml_gelu(g.ctx, h1)
        h2 = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(L.Q8_0, [N_, K_], w2), ge), g.new(L.F32, [K_], b2))
        res = H.ggml_add(g.ctx, h2, tx)
        nn = H.ggml_norm(g.ctx, res, 1e-5)
        y = H.ggml_add(g.ctx, H.ggml_mul(g.ctx, nn, g.new(L.F32, [K_], nw)), g.new(L.F32, [K_], nb))
        reads = [h1, ge, h2, res, nn, y]
        h1_g, ge_g, h2_g, res_g, nn_g, y_g = _four_times(backend, g, reads, reads)
    finally:
        g.free()
    _assert_bits(f"encoder chain cols={cols}: GELU of the kernel's own input", ge_g, A.gelu(h1_g))
    d, gate = float(np.max(A.row_distance(nn_g, A.norm(res_g, 1e-5)))), A.NORM_GATE + A.norm_extra(res_g)
    plog(f"  act encoder chain cols={cols}: NORM {d:.4g} of the row's maximum from the twin on the kernel's own input, gate {gate:.4g}")
    assert d <= gate
    _assert_bits(f"encoder chain cols={cols}: NORM * w + b", y_g, R.binary("add", R.binary("mul", nn_g, nw), nb))
    T.compare(f"act encoder chain cols={cols}: MUL_MAT(q8_0)(GELU) + b vs the oracle on the kernel's own activation", h2_g, _oracle_mm(L.Q8_0, w2, N_, K_, ge_g.reshape(cols, N_), b2), max_nmse=1e-10, log=plog)


@pytest.mark.parametrize("cols", [1, 5, 33])
def test_gemma_ffn_chain(backend, H, plog, cols):
    """RMS_NORM * w -> gate, up (Q4_K) -> geglu_split -> down (Q4_K) -> RMS_NORM * w -> ADD(residual)   (Gemma 2's FFN with its post-norm)"""
    rng = np.random.default_rng(9500 + cols)
    x = (rng.standard_normal((cols, K_)) * 2).astype(np.float32)
    wg, wu, wd = T.rand_weight(L.Q4_K, K_, N_, rng), T.rand_weight(L.Q4_K, K_, N_, rng), T.rand_weight(L.Q4_K, N_, K_, rng)
    n1, n2 = rng.uniform(0.5, 1.5, K_).astype(np.float32), rng.uniform(0.5, 1.5, K_).astype(np.float32)
    g = T.G(backend)
    try:
        tx = g.new(L.F32, [K_, cols], x)
        cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, tx, 1e-6), g.new(L.F32, [K_], n1))
        gate = H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [K_, N_], wg), cur)
        up = H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [K_, N_], wu), cur)
        act = H.ggml_geglu_split(g.ctx, gate, up)
        down = H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [N_, K_], wd), act)
        post = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, down, 1e-6), g.new(L.F32, [K_], n2))
        out = H.ggml_add(g.ctx, post, tx)
        reads = [gate, up, act, down, out]
        gate_g, up_g, act_g, down_g, _ = _four_times(backend, g, reads, reads)
    finally:
        g.free()
    _assert_bits(f"gemma chain cols={cols}: GEGLU of the kernel's own inputs", act_g, A.glu("GEGLU", gate_g, up_g))
    T.compare(f"act gemma chain cols={cols}: down (Q4_K) vs the oracle on the kernel's own activation", down_g, _oracle_mm(L.Q4_K, wd, N_, K_, act_g.reshape(cols, N_)), max_nmse=1e-10, log=plog)
