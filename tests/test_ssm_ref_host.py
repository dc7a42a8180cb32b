"""CPU: the host mirror's builders for CONCAT / SSM_CONV / SSM_SCAN and the NumPy twins and gates of tests/ssm_ref.py that tests/test_gpu_ssm.py holds the
kernels to — known answers worked out by hand, the f32 twin against the gate, and six wrong twins that the gate must catch on the GPU tests' own inputs."""
import numpy as np
import pytest

import llama_box_amd as L
import ssm_ref as S


# ------------------------------------------------------------------------------------------------ builders
def _ne(t):
    return list(t.contents.ne)


def test_builders_shapes_op_src_and_params(H):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        a, b = H.ggml_new_tensor_4d(ctx, L.F32, 5, 3, 2, 2), H.ggml_new_tensor_4d(ctx, L.F32, 7, 3, 2, 2)
        r = H.ggml_concat(ctx, a, b, 0)
        assert H.ggml_op_name(r.contents.op) == b"CONCAT" and _ne(r) == [12, 3, 2, 2] and r.contents.op_params[0] == 0 and r.contents.type == L.F32
        assert C_addr(r.contents.src[0]) == C_addr(a) and C_addr(r.contents.src[1]) == C_addr(b) and not r.contents.src[2]
        for dim in (1, 2, 3):
            ne = [5, 3, 2, 2]
            ne[dim] += 4
            o = H.ggml_new_tensor_4d(ctx, L.F32, *[4 if d == dim else v for d, v in enumerate([5, 3, 2, 2])])
            r = H.ggml_concat(ctx, a, o, dim)
            assert _ne(r) == ne and r.contents.op_params[0] == dim
        # the Mamba shape: the conv state in front of the transposed activations
        x = H.ggml_new_tensor_3d(ctx, L.F32, 70, 5, 2)
        r = H.ggml_concat(ctx, H.ggml_new_tensor_3d(ctx, L.F32, 3, 70, 2), H.ggml_transpose(ctx, x), 0)
        assert _ne(r) == [8, 70, 2, 1] and list(r.contents.nb) == [4, 32, 32 * 70, 32 * 70 * 2]

        sx, c = H.ggml_new_tensor_3d(ctx, L.F32, 3 + 5, 70, 2), H.ggml_new_tensor_2d(ctx, L.F32, 4, 70)
        r = H.ggml_ssm_conv(ctx, sx, c)
        assert H.ggml_op_name(r.contents.op) == b"SSM_CONV" and _ne(r) == [70, 5, 2, 1] and r.contents.type == L.F32
        assert C_addr(r.contents.src[0]) == C_addr(sx) and C_addr(r.contents.src[1]) == C_addr(c)

        d_state, head_dim, n_head, n_t, n_s, n_rs = 128, 64, 3, 7, 2, 4
        s = H.ggml_new_tensor_4d(ctx, L.F32, d_state, head_dim, n_head, n_rs)
        xs = H.ggml_new_tensor_4d(ctx, L.F32, head_dim, n_head, n_t, n_s)
        dt = H.ggml_new_tensor_3d(ctx, L.F32, n_head, n_t, n_s)
        B, Cc = (H.ggml_new_tensor_4d(ctx, L.F32, d_state, 1, n_t, n_s) for _ in range(2))
        ids = H.ggml_new_tensor_1d(ctx, L.I32, n_s)
        for A in (H.ggml_new_tensor_2d(ctx, L.F32, 1, n_head), H.ggml_new_tensor_2d(ctx, L.F32, d_state, n_head)):
            r = H.ggml_ssm_scan(ctx, s, xs, dt, A, B, Cc, ids)
            assert H.ggml_op_name(r.contents.op) == b"SSM_SCAN" and r.contents.type == L.F32
            assert _ne(r) == [head_dim * n_head * n_t * n_s + d_state * head_dim * n_head * n_s, 1, 1, 1]
            assert [C_addr(r.contents.src[k]) for k in range(7)] == [C_addr(t) for t in (s, xs, dt, A, B, Cc, ids)] and not r.contents.src[7]
    finally:
        H.ggml_free(ctx)


def C_addr(p):
    import ctypes

    return ctypes.addressof(p.contents)


# ------------------------------------------------------------------------------------------------ known answers
def test_concat_along_each_dim():
    a = np.arange(2 * 2 * 3 * 5, dtype=np.float32).reshape(2, 2, 3, 5)  # ne = [5, 3, 2, 2]
    for dim, ne in ((0, [7, 3, 2, 2]), (1, [5, 4, 2, 2]), (2, [5, 3, 1, 2]), (3, [5, 3, 2, 3])):
        b = -np.arange(int(np.prod(ne)), dtype=np.float32).reshape(ne[::-1])
        r = S.concat(a, b, dim)
        assert list(r.shape[::-1]) == [a.shape[3 - d] + (ne[d] if d == dim else 0) for d in range(4)]
        idx = [0, 0, 0, 0]
        assert r[tuple(idx)] == a[tuple(idx)]  # element 0 comes from a
        idx[3 - dim] = a.shape[3 - dim]        # the first index past a's extent comes from b at 0
        assert r[tuple(idx)] == b[0, 0, 0, 0]
        idx[3 - dim] = r.shape[3 - dim] - 1
        last_b = [0, 0, 0, 0]
        last_b[3 - dim] = b.shape[3 - dim] - 1
        assert r[tuple(idx)] == b[tuple(last_b)]


def test_conv_d_conv_2_by_hand():
    """d_conv 2, d_inner 2, three tokens: channel 0 has taps (1, 2) over 1 2 3 4 -> 1 + 4, 2 + 6, 3 + 8; channel 1 taps (-1, 0.5) over 4 0 -2 8 -> -4, -1, 6."""
    sx = np.array([[[1, 2, 3, 4], [4, 0, -2, 8]]], dtype=np.float32)
    c = np.array([[1, 2], [-1, 0.5]], dtype=np.float32)
    want = np.array([[[5, -4], [8, -1], [11, 6]]], dtype=np.float64)
    got, env = S.conv64(sx, c)
    assert np.array_equal(got, want)
    assert np.array_equal(env, np.array([[[5, 4], [8, 1], [11, 6]]], dtype=np.float64))
    assert np.array_equal(S.conv32(sx, c), want.astype(np.float32))
    assert np.array_equal(S.conv_gate(sx, c), 3 * S.U * env)


def _tiny_scan():
    """Two state elements, one row, two tokens, by hand.  A = -ln 2 / 25, dt above the threshold so that dtp = dt:
        token 0: dt 25 -> dA = 1/2;  x 0.04 -> xdt = 1;  state = (1, 2) / 2 + (1, -1) = (1.5, 0);      C = (1, 1)   -> y = 1.5
        token 1: dt 50 -> dA = 1/4;  x 0.02 -> xdt = 1;  state = (1.5, 0) / 4 + (0, 1) = (0.375, 1);   C = (2, -1)  -> y = -0.25
    The start state is row 1 of a cache of two rows (ids = [1]); row 0 holds (100, 100)."""
    return {
        "s": np.array([[[[100, 100]]], [[[1, 2]]]], dtype=np.float32),
        "x": np.array([[[[0.04]], [[0.02]]]], dtype=np.float32),
        "dt": np.array([[[25], [50]]], dtype=np.float32),
        "A": np.array([[-np.log(2.0) / 25.0]], dtype=np.float32),
        "B": np.array([[[[1, -1]], [[0, 1]]]], dtype=np.float32),
        "C": np.array([[[[1, 1]], [[2, -1]]]], dtype=np.float32),
        "ids": np.array([1], dtype=np.int32),
    }


def test_scan_two_states_two_tokens_by_hand():
    inp = _tiny_scan()
    ref = S.scan64(inp)
    assert np.allclose(ref["y"].ravel(), [1.5, -0.25], rtol=0, atol=2e-7)
    assert np.allclose(ref["st"].ravel(), [0.375, 1.0], rtol=0, atol=2e-7)
    # the envelope: |prev| dA + |B xdt| -> (1.5, 2) then (0.375, 1.5); sum E |C| -> 3.5 then 2.25
    assert np.allclose(ref["Es"].ravel(), [0.375, 1.5], atol=2e-7) and np.allclose(ref["Ey"].ravel(), [3.5, 2.25], atol=2e-7)
    y32, st32 = S.scan32(inp)
    assert np.allclose(y32.ravel(), [1.5, -0.25], atol=1e-6) and np.allclose(st32.ravel(), [0.375, 1.0], atol=1e-6)
    # below the threshold dtp = ln(1 + e^dt): dt = 0 gives ln 2, and A = 0 keeps the state: state = 1 + 1 * (2 * ln 2)
    one = {"s": np.ones((1, 1, 1, 1), np.float32), "x": np.full((1, 1, 1, 1), 2, np.float32), "dt": np.zeros((1, 1, 1), np.float32),
           "A": np.zeros((1, 1), np.float32), "B": np.ones((1, 1, 1, 1), np.float32), "C": np.ones((1, 1, 1, 1), np.float32), "ids": np.zeros(1, np.int32)}
    assert abs(S.scan64(one)["y"].item() - (1 + 2 * np.log(2.0))) < 1e-15


def test_wrong_twins_differ_on_the_tiny_scan_where_they_can():
    inp = _tiny_scan()
    ref = S.scan64(inp)
    assert not np.allclose(S.scan64(inp, "prev_not_carried")["y"], ref["y"])      # token 1 restarts from (1, 2)
    assert not np.allclose(S.scan64(inp, "ids_ignored")["y"], ref["y"])           # starts from (100, 100)
    assert not np.allclose(S.scan64(inp, "b_c_swapped")["y"], ref["y"])
    assert np.all(S.scan64(inp, "states_stored_at_ids")["st"] == 0)               # ids[0] = 1 names no block of a one-sequence result


# ------------------------------------------------------------------------------------------------ the gate on the GPU tests' inputs
CASES = sorted(S.SCAN_CASES)


def test_inputs_hold_what_the_gpu_tests_promise():
    for name in CASES:
        d_state, head_dim, n_head, n_group, n_t, n_s, m1, dup, xbc = S.SCAN_CASES[name]
        inp = S.scan_inputs(name)
        ids = inp["ids"].tolist()
        assert inp["s"].shape[0] == n_s + 2 and all(0 <= i < n_s + 2 and i != k for k, i in enumerate(ids)), name  # no sequence starts from the row of its index
        assert (len(set(ids)) < len(ids)) == dup, name
        dt = inp["dt"].ravel()
        for v in S.DT_SPECIAL:
            assert np.any(dt == np.float32(v)), (name, v)
        assert np.any(dt < 20) and np.any(dt > 20) and np.float32(S.DT_SPECIAL[1]) > np.float32(20.0)
        assert np.all(inp["s"][ids] != 0) and inp["A"].shape == (n_head, d_state if m1 else 1) and np.all(inp["A"] < 0), name
        assert n_group in (1, n_head)
    assert any(S.SCAN_CASES[n][7] for n in CASES) and any(S.SCAN_CASES[n][8] for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_f32_twin_is_inside_the_gate_with_room_and_the_gate_is_reachable(name):
    """The f32 twin with this libm stays inside the a-priori bound for functions one ulp off, e(2, 2) u — so the analysis holds and R is no free parameter — and
    therefore inside the gate (R e(0,0) + e(4,4) - e(0,0) ...) with the margin of the two further ulps.  The gate is not vacuous: relative to the envelope it is
    below 2^-10 everywhere, so an error of one part in a thousand of any term fails it."""
    inp = S.scan_inputs(name)
    ref, R, gates = S.scan_reference(name)
    y32, st32 = S.scan32(inp)
    for got, want, e22 in ((y32, ref["y"], ref["ey"][(2, 2)]), (st32, ref["st"], ref["es"][(2, 2)])):
        assert np.all(np.abs(got.astype(np.float64) - want) <= S.U * e22 * S.SECOND_ORDER + S.FLOOR * (1 + ref["d_state"])), name
    ey, es = S.scan_excess(ref, gates, y32, st32)
    assert 0 < R < 2.0 and ey <= 1.0 and es <= 1.0, (name, R, ey, es)
    # room: wherever a function's error reaches the element at all (e(4,4) > e(0,0): some dt on its way was at or below the threshold, or a decay factor took
    # part), the gate stands clear of the twin.  Elsewhere — a state that is B x dt alone — twin and kernel do the same two roundings and the gate is R e(0,0)
    for got, want, g, e0, e4 in ((y32, ref["y"], gates[0], ref["ey"][(0, 0)], ref["ey"][(4, 4)]), (st32, ref["st"], gates[1], ref["es"][(0, 0)], ref["es"][(4, 4)])):
        m = e4 > 1.5 * e0
        assert (np.any(m) or got is y32) and np.all(np.abs(got.astype(np.float64) - want)[m] < 0.75 * g[m]), name  # (y's bound is mostly its reduction's)
    for g, E in ((gates[0], ref["Ey"]), (gates[1], ref["Es"])):
        m = E > 0
        assert np.all(g[m] / E[m] < 2.0 ** -10), (name, float(np.max(g[m] / E[m])))


def _applies(name, wrong):
    d_state, head_dim, n_head, n_group, n_t, n_s, m1, dup, xbc = S.SCAN_CASES[name]
    if wrong == "prev_not_carried":
        return n_t >= 2
    if wrong == "a_per_head":
        return m1
    if wrong == "b_c_swapped":
        return True
    return True


@pytest.mark.parametrize("wrong", S.WRONG)
def test_each_wrong_twin_fails_the_gate_on_every_case_it_applies_to(wrong):
    hit = 0
    for name in CASES:
        if not _applies(name, wrong):
            continue
        ref, R, gates = S.scan_reference(name)
        bad = S.scan64(S.scan_inputs(name), wrong)
        ey, es = S.scan_excess(ref, gates, bad["y"], bad["st"])
        if wrong == "states_stored_at_ids":
            assert es > 1.0, (name, wrong, es)  # (y is untouched by where the states go)
        else:
            assert ey > 1.0, (name, wrong, ey, es)
        hit += 1
    assert hit >= 4, (wrong, hit)


def test_conv_twins_agree_within_the_conv_gate():
    rng = np.random.default_rng(3)
    sx = rng.standard_normal((3, 70, 3 + 33)).astype(np.float32)
    c = rng.standard_normal((70, 4)).astype(np.float32)
    ref, env = S.conv64(sx, c)
    err = np.abs(S.conv32(sx, c).astype(np.float64) - ref)
    assert np.all(err <= S.conv_gate(sx, c)) and np.max(err / (S.U * env)) < 3.0
    shifted = S.conv64(np.roll(sx, 1, axis=-1), c)[0]  # a window one column off fails it
    assert np.max(np.abs(shifted - ref) / S.conv_gate(sx, c)) > 1e3
