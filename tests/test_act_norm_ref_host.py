"""CPU: the NumPy twins of tests/act_norm_ref.py (NORM, the GELU tables, the gated units) on known answers, the sanity of the two tables the process's libm
gives, the host mirror's new builders, and the edge shapes against the constants parsed from csrc/ops_act.hip.  No GPU, no oracle (it has none of these ops)."""
import numpy as np
import pytest

import act_norm_ref as A
import llama_box_amd as L


def _idx(v):
    return int(np.float16(v).view(np.uint16))


def test_edge_shapes_follow_the_launcher_constants():
    want = A.shapes_from(A.act_limits())
    assert A.GELU_N == want["GELU_N"] and A.NORM_NE0 == want["NORM_NE0"] and A.GLU_NC == want["GLU_NC"], want


# entries far from any f16 rounding boundary: the f32 evaluation, the float64 one and any correct tanhf / expf agree on them
KNOWN = [(1.0, 0x3ABB, 0x3AC4), (-1.0, 0xB115, 0xB0EF), (0.5, 0x3588, 0x359B), (3.0, 0x41FE, 0x41F7), (-3.0, 0x9B73, 0xA4A0)]


@pytest.mark.parametrize("x,tg,tq", KNOWN)
def test_table_known_answers(x, tg, tq):
    g, q = A.tables()
    g64, q64 = A.tables_f64()
    assert (int(g[_idx(x)]), int(q[_idx(x)])) == (tg, tq)
    assert (int(g64[_idx(x)]), int(q64[_idx(x)])) == (tg, tq)


def test_table_ends():
    g, q = A.tables()
    gv, qv = g.view(np.float16), q.view(np.float16)
    assert gv[0x7C00] == np.inf and np.isnan(gv[0xFC00])          # 0.5 inf (1 + 1); 0.5 -inf (1 + -1) = -inf * 0
    assert qv[0x7C00] == np.inf and np.isnan(qv[0xFC00])          # inf / (1 + 0); -inf * (1 / inf)
    assert g[0] == 0 and g[0x8000] == 0x8000 and q[0] == 0 and q[0x8000] == 0x8000  # zeros keep their sign


def test_tables_against_float64(capsys):
    """A condition, not a pin: the libm tables may differ from the float64 ones (f32 cancellation in 1 + tanhf(.) for negative arguments) in at most 2 % of
    the entries, and never in WHERE the NaNs are.  The table's bytes belong to the libm in use and are not asserted."""
    for name, t, t64, v64 in zip(("gelu", "gelu_quick"), A.tables(), A.tables_f64(), A.functions_f64()):
        nan, nan64 = np.isnan(t.view(np.float16)), np.isnan(t64.view(np.float16))
        assert np.array_equal(nan, nan64), name
        differ = (t != t64) & ~nan
        with np.errstate(all="ignore"):  # (how far the libm entry is from the float64 VALUE, in f16 steps at that value)
            far = differ & ~(np.abs(t.view(np.float16).astype(np.float64) - v64) <= np.spacing(np.abs(t64.view(np.float16))).astype(np.float64))
        with capsys.disabled():
            print(f"\n  {name}: {int(differ.sum())} of 65536 entries differ from the float64 table ({100.0 * differ.mean():.2f} %), {int(far.sum())} lie more than one f16 step from the float64 value")
        assert differ.mean() <= 0.02, name


def test_gelu_twin_branches():
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    x = np.array([-10.0, np.nextafter(np.float32(-10), up), 10.0, np.nextafter(np.float32(10), dn), 1e30, -1e30, np.nan, 1.0, -0.0], np.float32)
    y = A.gelu(x)
    t = A.tables()[0].view(np.float16)
    assert y[0] == 0 and not np.signbit(y[0]) and y[2] == 10.0 and y[4] == np.float32(1e30) and y[5] == 0 and np.isnan(y[6])
    assert y[1] == np.float32(t[_idx(-10.0)]) and y[3] == np.float32(t[_idx(10.0)])  # the neighbours of +-10 round to +-10 in f16 and take the table
    assert y[7] == np.float32(np.uint16(0x3ABB).view(np.float16)) and y[8] == 0 and np.signbit(y[8])
    q = A.gelu_quick(np.array([65519.996, 65520.0, -65520.0, 1e30], np.float32))
    assert np.isfinite(q[0]) and q[1] == np.inf and np.isnan(q[2]) and q[3] == np.inf
    # GEGLU's x >= 10 branch: x * g
    assert A.glu("GEGLU", np.float32([12.5, -12.5]), np.float32([3.0, 3.0])).tolist() == [37.5, 0.0]
    assert A.glu("REGLU", np.float32([2.0, -2.0, -0.0]), np.float32([3.0, 3.0, 3.0])).tolist() == [6.0, 0.0, 0.0]
    assert abs(A.gelu_erf64(np.float32(1.0)) - 0.8413447460685429) < 1e-7


def test_norm_twin():
    rng = np.random.default_rng(5)
    for ne0 in (1, 3, 100, 4100):
        x = (rng.standard_normal((3, ne0)) * 4 + 1.5).astype(np.float32)
        y, ref = A.norm(x, 1e-5), A.layer_norm64(x, 1e-5)
        if ne0 == 1:
            assert np.all(y == 0)  # a single value is its own mean
            continue
        d = A.row_distance(y, ref)
        assert np.all(d <= 4 * A.U24 + A.norm_extra(x)), (ne0, d)  # the twin's own f32 steps: the mean's rounding and v's
    const = np.full((2, 64), 3.25, np.float32)
    assert np.all(A.norm(const, 1e-5) == 0)
    assert np.all(np.isnan(A.norm(const, 0.0)))
    w, b = rng.uniform(0.5, 1.5, 100).astype(np.float32), rng.standard_normal(100).astype(np.float32)
    x = rng.standard_normal((2, 100)).astype(np.float32)
    assert np.allclose(A.norm(x, 1e-5, w, b), A.norm(x, 1e-5) * w + b, rtol=1e-14, atol=0)
    assert A.norm_extra(np.float32([[1000.0, 1001.0, 999.0]])) == pytest.approx(1000.0 * A.U23)


def test_erf_excess_measures_in_units_of_the_gate():
    x, g = np.float32([1.0, -3.0]), np.float32([2.0, 0.5])
    ref = A.gelu_erf64(x) * g.astype(np.float64)
    assert np.all(A.erf_excess(ref.astype(np.float32), x, g) <= 1.0)
    off = (ref + 40 * A.U24 * np.abs(x) * np.abs(g)).astype(np.float32)
    assert np.all(A.erf_excess(off, x, g) > 1.0)
    assert A.erf_excess(np.float32([np.nan]), np.float32([np.nan]))[0] == 0 and A.erf_excess(np.float32([np.nan]), np.float32([1.0]))[0] == np.inf


def test_builders(built, H):
    assert (H.ggml_op_name(A.OP_NORM), H.ggml_op_name(A.OP_UNARY), H.ggml_op_name(A.OP_GLU)) == (b"NORM", b"UNARY", b"GLU")
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        a = H.ggml_new_tensor_4d(ctx, L.F32, 12, 3, 2, 1)
        b = H.ggml_new_tensor_4d(ctx, L.F32, 12, 3, 2, 1)

        def same(p, q):
            import ctypes as C
            return C.addressof(p.contents) == C.addressof(q.contents)

        n = H.ggml_norm(ctx, a, 1e-6).contents
        assert n.op == A.OP_NORM and np.int32(n.op_params[0]).view(np.float32) == np.float32(1e-6) and same(n.src[0], a) and not n.src[1]
        assert list(n.ne) == [12, 3, 2, 1] and n.type == L.F32
        for name, fn in (("GELU", H.ggml_gelu), ("GELU_QUICK", H.ggml_gelu_quick), ("GELU_ERF", H.ggml_gelu_erf)):
            u = fn(ctx, a).contents
            assert u.op == A.OP_UNARY and u.op_params[0] == A.UNARY[name] and u.op_params[1] == 0 and same(u.src[0], a) and not u.src[1] and list(u.ne) == [12, 3, 2, 1]
        for name, stem in A.GLU_BUILDER.items():
            for form, swapped, split in (("", 0, False), ("_swapped", 1, False), ("_split", 0, True)):
                fn = getattr(H, f"ggml_{stem}{form}")
                r = (fn(ctx, a, b) if split else fn(ctx, a)).contents
                assert r.op == A.OP_GLU and r.op_params[0] == A.GLU[name] and r.op_params[1] == swapped, (name, form)
                assert same(r.src[0], a) and (same(r.src[1], b) if split else not r.src[1]), (name, form)
                assert list(r.ne) == [12 if split else 6, 3, 2, 1] and r.type == L.F32, (name, form)
    finally:
        H.ggml_free(ctx)
