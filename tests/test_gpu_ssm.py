"""GPU: csrc/ssm.hip through the C-ABI — CONCAT, SSM_CONV (alone and with the bias ADD and SILU folded in) and SSM_SCAN in its Mamba-1 and Mamba-2 forms, then
a whole Mamba layer and a whole Mamba-2 layer over a persistent state cache — against the NumPy twins of tests/ssm_ref.py (the CPU oracle has none of the ops).

  * CONCAT: bit equality.
  * SSM_CONV: |got - f64| <= (d_conv + 1) 2^-24 sum |sx c| (ssm_ref.conv_gate); fused and unfused launches bit-equal.
  * SSM_SCAN: y and the final states inside ssm_ref.scan_gates — the f32 twin's measured error plus two ulps each of expf and log1pf and a reordered reduction.
  * the layers: the bound stated at LAYER_K.

Every test here fails on a backend without these ops: harness.G.compute raises supports_op=false at the first new node.
"""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import ssm_ref as S

pytestmark = pytest.mark.gpu
F32, F16, I32 = L.F32, L.F16, L.I32


def _run(target, build):
    """build(g) -> (outs, reads); the arrays of the reads after one compute."""
    g = T.G(target)
    try:
        outs, reads = build(g)
        g.compute(list(outs))
        return [g.read(t) for t in reads]
    finally:
        g.free()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _np_permute(arr, axes):
    """ggml_permute(a, *axes) as an array: source dimension i becomes dimension axes[i] (NumPy axis = 3 - ggml dimension)."""
    perm = [0] * 4
    for i, ax in enumerate(axes):
        perm[3 - ax] = 3 - i
    return np.transpose(arr, perm)


# ------------------------------------------------------------------------------------------------ scan operands as graph tensors
def _scan_node(g, inp, xbc=False, strided=False):
    """The SSM_SCAN node over the arrays of a ssm_ref case.  xbc: x, B and C are views into one [d_inner + 2 n_group d_state, n_t, n_s] buffer, Mamba-2's strides;
    strided: each is a view of a wider tensor of its own (rows further apart than their length)."""
    H, ctx = g.H, g.ctx
    n_rs, n_head, head_dim, d_state = inp["s"].shape
    n_s, n_t = inp["x"].shape[:2]
    n_group = inp["B"].shape[2]
    s = g.new(F32, [d_state, head_dim, n_head, n_rs], inp["s"])
    dt = g.new(F32, [n_head, n_t, n_s], inp["dt"])
    A = g.new(F32, [inp["A"].shape[1], n_head], inp["A"])
    ids = g.new(I32, [n_s], inp["ids"])
    d_inner, gd = head_dim * n_head, n_group * d_state
    if xbc:
        w = d_inner + 2 * gd
        buf = np.concatenate([inp["x"].reshape(n_s, n_t, d_inner), inp["B"].reshape(n_s, n_t, gd), inp["C"].reshape(n_s, n_t, gd)], axis=2)
        t = g.new(F32, [w, n_t, n_s], buf)
        x = H.ggml_view_4d(ctx, t, head_dim, n_head, n_t, n_s, head_dim * 4, w * 4, w * 4 * n_t, 0)
        B = H.ggml_view_4d(ctx, t, d_state, n_group, n_t, n_s, d_state * 4, w * 4, w * 4 * n_t, d_inner * 4)
        Cc = H.ggml_view_4d(ctx, t, d_state, n_group, n_t, n_s, d_state * 4, w * 4, w * 4 * n_t, (d_inner + gd) * 4)
    elif strided:
        def wide(arr, row, pad):
            full = np.zeros((n_s, n_t, row + pad), dtype=np.float32)
            full[:, :, :row] = arr.reshape(n_s, n_t, row)
            return g.new(F32, [row + pad, n_t, n_s], full), (row + pad) * 4
        tx, sx_ = wide(inp["x"], d_inner, 4)
        tb, sb = wide(inp["B"], gd, 8)
        tc, sc = wide(inp["C"], gd, 12)
        x = H.ggml_view_4d(ctx, tx, head_dim, n_head, n_t, n_s, head_dim * 4, sx_, sx_ * n_t, 0)
        B = H.ggml_view_4d(ctx, tb, d_state, n_group, n_t, n_s, d_state * 4, sb, sb * n_t, 0)
        Cc = H.ggml_view_4d(ctx, tc, d_state, n_group, n_t, n_s, d_state * 4, sc, sc * n_t, 0)
    else:
        x = g.new(F32, [head_dim, n_head, n_t, n_s], inp["x"])
        B = g.new(F32, [d_state, n_group, n_t, n_s], inp["B"])
        Cc = g.new(F32, [d_state, n_group, n_t, n_s], inp["C"])
    return H.ggml_ssm_scan(ctx, s, x, dt, A, B, Cc, ids)


def _split_scan(flat, inp):
    n_rs, n_head, head_dim, d_state = inp["s"].shape
    n_s, n_t = inp["x"].shape[:2]
    flat = flat.reshape(-1)
    ny = n_s * n_t * n_head * head_dim
    assert flat.size == ny + n_s * n_head * head_dim * d_state
    return flat[:ny].reshape(n_s, n_t, n_head, head_dim), flat[ny:].reshape(n_s, n_head, head_dim, d_state)


# ------------------------------------------------------------------------------------------------ 1. supports_op
def test_supports_op(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        m1, m2 = S.scan_inputs("m1-h70-t2-s3"), S.scan_inputs("m2-d128-hd48-h3-g3-t2-s3")
        g1 = S.scan_inputs("m2-d128-hd64-h3-g1-t1-s3")
        assert ok(_scan_node(g, m1)) and ok(_scan_node(g, m2)) and ok(_scan_node(g, g1))          # both forms; n_group 1 and n_head
        assert ok(_scan_node(g, m2, xbc=True)) and ok(_scan_node(g, g1, strided=True))              # strided x / B / C
        # two groups over four heads: refused (which heads share a group is not pinned); f16 operands: refused
        n_t, n_s = 2, 1
        s = H.ggml_new_tensor_4d(ctx, F32, 64, 16, 4, 3)
        x = H.ggml_new_tensor_4d(ctx, F32, 16, 4, n_t, n_s)
        dt, A, ids = H.ggml_new_tensor_3d(ctx, F32, 4, n_t, n_s), H.ggml_new_tensor_2d(ctx, F32, 1, 4), H.ggml_new_tensor_1d(ctx, I32, n_s)
        for n_group, want in ((1, True), (4, True), (2, False)):
            B, Cc = (H.ggml_new_tensor_4d(ctx, F32, 64, n_group, n_t, n_s) for _ in range(2))
            assert ok(H.ggml_ssm_scan(ctx, s, x, dt, A, B, Cc, ids)) == want, n_group
        B, Cc = (H.ggml_new_tensor_4d(ctx, F32, 64, 1, n_t, n_s) for _ in range(2))
        assert not ok(H.ggml_ssm_scan(ctx, s, H.ggml_new_tensor_4d(ctx, F16, 16, 4, n_t, n_s), dt, A, B, Cc, ids))
        assert not ok(H.ggml_ssm_scan(ctx, s, x, dt, A, H.ggml_new_tensor_4d(ctx, F16, 64, 1, n_t, n_s), H.ggml_new_tensor_4d(ctx, F16, 64, 1, n_t, n_s), ids))
        x0, dt0 = H.ggml_new_tensor_4d(ctx, F32, 16, 4, 0, n_s), H.ggml_new_tensor_3d(ctx, F32, 4, 0, n_s)  # no token but a sequence: its state area would stay unwritten
        B0, C0 = (H.ggml_new_tensor_4d(ctx, F32, 64, 1, 0, n_s) for _ in range(2))
        assert not ok(H.ggml_ssm_scan(ctx, s, x0, dt0, A, B0, C0, ids))
        s32 = H.ggml_new_tensor_4d(ctx, F32, 32, 16, 4, 3)  # a d_state no kernel form serves
        B32, C32 = (H.ggml_new_tensor_4d(ctx, F32, 32, 1, n_t, n_s) for _ in range(2))
        assert not ok(H.ggml_ssm_scan(ctx, s32, x, dt, A, B32, C32, ids))

        # SSM_CONV: dense rows, nb[2] free; padded rows and f16 refused; d_conv 2 .. 8
        c4 = H.ggml_new_tensor_2d(ctx, F32, 4, 70)
        assert ok(H.ggml_ssm_conv(ctx, H.ggml_new_tensor_3d(ctx, F32, 3 + 5, 70, 2), c4))
        big = H.ggml_new_tensor_3d(ctx, F32, 8, 75, 2)
        assert ok(H.ggml_ssm_conv(ctx, H.ggml_view_3d(ctx, big, 8, 70, 2, 8 * 4, 8 * 4 * 75, 0), c4))           # nb[2] larger than a matrix
        padded = H.ggml_new_tensor_3d(ctx, F32, 10, 70, 2)
        assert not ok(H.ggml_ssm_conv(ctx, H.ggml_view_3d(ctx, padded, 8, 70, 2, 10 * 4, 10 * 4 * 70, 0), c4))  # rows padded: nb[1] != ne[0] * 4
        assert not ok(H.ggml_ssm_conv(ctx, H.ggml_new_tensor_3d(ctx, F16, 8, 70, 2), H.ggml_new_tensor_2d(ctx, F16, 4, 70)))
        assert ok(H.ggml_ssm_conv(ctx, H.ggml_new_tensor_3d(ctx, F32, 8, 70, 2), H.ggml_new_tensor_2d(ctx, F32, 8, 70)))
        assert not ok(H.ggml_ssm_conv(ctx, H.ggml_new_tensor_3d(ctx, F32, 9, 70, 2), H.ggml_new_tensor_2d(ctx, F32, 9, 70)))

        # CONCAT: a transposed source, every dim, f16 / i32; mixed types cannot be built (the builder asserts)
        st, xt = H.ggml_new_tensor_3d(ctx, F32, 3, 70, 2), H.ggml_new_tensor_3d(ctx, F32, 70, 5, 2)
        assert ok(H.ggml_concat(ctx, st, H.ggml_transpose(ctx, xt), 0))
        for t in (F32, F16, I32):
            for dim in range(4):
                assert ok(H.ggml_concat(ctx, H.ggml_new_tensor_4d(ctx, t, 5, 3, 2, 2), H.ggml_new_tensor_4d(ctx, t, 5, 3, 2, 2), dim)), (t, dim)
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ 2. CONCAT
def test_concat_bit_exact(backend, H):
    rng = np.random.default_rng(1)

    def plain(t=F32):
        return (lambda g, arr: g.new(t, list(arr.shape[::-1]), arr)), (lambda arr: arr)

    # a tensor maker and the array the tensor stands for
    transposed = (lambda g, arr: H.ggml_transpose(g.ctx, plain()[0](g, arr))), (lambda arr: np.swapaxes(arr, 2, 3))
    permuted = (lambda g, arr: H.ggml_permute(g.ctx, plain()[0](g, arr), 1, 2, 0, 3)), (lambda arr: _np_permute(arr, (1, 2, 0, 3)))
    f = np.float32
    cases = []  # (a array, how a is made and seen, b array, how b is made and seen, dim)
    for dim, ne_b in ((0, [7, 3, 2, 2]), (1, [5, 4, 2, 2]), (2, [5, 3, 3, 2]), (3, [5, 3, 2, 1])):  # 4-D, odd extents, every dim
        cases.append((rng.standard_normal((2, 2, 3, 5)).astype(f), plain(), rng.standard_normal(ne_b[::-1]).astype(f), plain(), dim))
    # the Mamba shape: [3, 70, 2] + transpose([70, 5, 2])
    cases.append((rng.standard_normal((1, 2, 70, 3)).astype(f), plain(), rng.standard_normal((1, 2, 5, 70)).astype(f), transposed, 0))
    # a permuted source: [4, 6, 3, 2] permuted (1, 2, 0, 3) -> [3, 4, 6, 2], behind a plain [3, 4, 5, 2] along dim 2
    cases.append((rng.standard_normal((2, 5, 4, 3)).astype(f), plain(), rng.standard_normal((2, 3, 6, 4)).astype(f), permuted, 2))
    # a transposed first source, more than one workgroup; f16; i32
    cases.append((rng.standard_normal((1, 1, 300, 33)).astype(f), transposed, rng.standard_normal((1, 1, 33, 17)).astype(f), plain(), 0))
    cases.append((rng.standard_normal((1, 3, 5, 9)).astype(np.float16), plain(F16), rng.standard_normal((1, 3, 2, 9)).astype(np.float16), plain(F16), 1))
    cases.append((rng.integers(-2 ** 31, 2 ** 31 - 1, (1, 1, 4, 11), dtype=np.int32), plain(I32), rng.integers(-2 ** 31, 2 ** 31 - 1, (1, 1, 4, 6), dtype=np.int32), plain(I32), 0))

    def build(g):
        outs = [H.ggml_concat(g.ctx, ma[0](g, a), mb[0](g, b), dim) for a, ma, b, mb, dim in cases]
        return outs, outs

    got = _run(backend, build)
    for k, ((a, ma, b, mb, dim), r) in enumerate(zip(cases, got)):
        want = S.concat(ma[1](a), mb[1](b), dim)
        assert r.shape == want.shape and np.array_equal(_bits(r), _bits(want)), (k, dim, r.shape, want.shape)


# ------------------------------------------------------------------------------------------------ 3. SSM_CONV
@pytest.mark.parametrize("d_conv,d_inner", [(2, 64), (2, 70), (4, 64), (4, 70)])
def test_ssm_conv_within_the_gate(backend, H, plog, d_conv, d_inner):
    rng = np.random.default_rng(d_conv * 100 + d_inner)
    shapes = [(n_t, n_s) for n_t in (1, 5, 33) for n_s in (1, 3)]
    sxs = [rng.standard_normal((n_s, d_inner, d_conv - 1 + n_t)).astype(np.float32) for n_t, n_s in shapes]
    sxv = rng.standard_normal((3, d_inner + 5, d_conv - 1 + 33)).astype(np.float32)  # read through a view: nb[2] larger than a matrix
    c = rng.standard_normal((d_inner, d_conv)).astype(np.float32)

    def build(g):
        ct = g.new(F32, [d_conv, d_inner], c)
        outs = [H.ggml_ssm_conv(g.ctx, g.new(F32, list(sx.shape[::-1]), sx), ct) for sx in sxs]
        tv = g.new(F32, list(sxv.shape[::-1]), sxv)
        ncs = sxv.shape[2]
        outs.append(H.ggml_ssm_conv(g.ctx, H.ggml_view_3d(g.ctx, tv, ncs, d_inner, 3, ncs * 4, ncs * 4 * (d_inner + 5), 0), ct))
        return outs, outs

    got = _run(backend, build)
    worst = 0.0
    for sx, r in zip(sxs + [sxv[:, :d_inner, :]], got):
        ref, _ = S.conv64(sx, c)
        r = r.reshape(ref.shape)
        ex = float(np.max(np.abs(r.astype(np.float64) - ref) / S.conv_gate(sx, c)))
        worst = max(worst, ex)
        assert ex <= 1.0, (sx.shape, ex)
    plog(f"  ssm_conv d_conv {d_conv} d_inner {d_inner}: worst error {worst:.3f} of the gate ((d_conv + 1) 2^-24 sum |sx c|)")


def _conv_chain_graph(g, H, sx, c, b, second_reader):
    ct, bt = g.new(F32, list(c.shape[::-1]), c), g.new(F32, [c.shape[0]], b)
    outs = []
    for a in sx:
        conv = H.ggml_ssm_conv(g.ctx, g.new(F32, list(a.shape[::-1]), a), ct)
        outs.append(H.ggml_silu(g.ctx, H.ggml_add(g.ctx, conv, bt)))
        if second_reader:
            outs.append(H.ggml_scale(g.ctx, conv, 2.0))
    return outs, outs


@pytest.mark.parametrize("second_reader", [False, True])
def test_conv_bias_silu_fusion_is_bit_equal_and_counted(backend, H, plog, second_reader):
    """SSM_CONV -> ADD(bias) -> SILU with single readers is one launch (two chains: kernel_launches differs by four between ssm_fuse 1 and 0, fused_nodes by four)
    with the bits of the three launches; a conv output that a second node reads is not fused."""
    rng = np.random.default_rng(9)
    d_conv, d_inner = 4, 70
    sx = [rng.standard_normal((n_s, d_inner, d_conv - 1 + n_t)).astype(np.float32) * 3 for n_t, n_s in ((1, 3), (33, 2))]
    c, b = rng.standard_normal((d_inner, d_conv)).astype(np.float32), rng.standard_normal(d_inner).astype(np.float32)
    runs = {}
    try:
        for fuse in (1, 0):
            backend.set_option("ssm_fuse", fuse)
            s0 = {k: backend.stat(k) for k in ("kernel_launches", "fused_nodes")}
            res = _run(backend, lambda g: _conv_chain_graph(g, H, sx, c, b, second_reader))
            runs[fuse] = (res, {k: backend.stat(k) - v for k, v in s0.items()})
    finally:
        backend.set_option("ssm_fuse", 1)
    plog(f"  ssm_conv chain (second reader: {second_reader}): ssm_fuse=1 {runs[1][1]}, ssm_fuse=0 {runs[0][1]}")
    for r1, r0 in zip(runs[1][0], runs[0][0]):
        assert np.array_equal(_bits(r1), _bits(r0))
    d = {k: runs[0][1][k] - runs[1][1][k] for k in runs[0][1]}
    assert d == ({"kernel_launches": 0, "fused_nodes": 0} if second_reader else {"kernel_launches": 4, "fused_nodes": -4}), (runs[0][1], runs[1][1])
    assert runs[0][1]["kernel_launches"] == (8 if second_reader else 6)
    # and against the twin: silu(conv + b), the conv inside its gate carried through the ADD and silu's slope (<= 1.1) with a rounding each and expf's two ulps
    for a, r in zip(sx, runs[1][0][::2] if second_reader else runs[1][0]):
        ref, env = S.conv64(a, c)
        want = S.silu64(ref + b.astype(np.float64))
        bound = 1.1 * (S.conv_gate(a, c) + S.U * np.abs(ref + b)) + 8 * S.U * np.abs(want) + 2.0 ** -120
        assert np.all(np.abs(r.reshape(ref.shape).astype(np.float64) - want) <= bound)


# ------------------------------------------------------------------------------------------------ 4. SSM_SCAN
def _scan_case(backend, plog, name):
    d_state, head_dim, n_head, n_group, n_t, n_s, m1, dup, xbc = S.SCAN_CASES[name]
    inp = S.scan_inputs(name)
    ref, R, gates = S.scan_reference(name)

    def build(g):
        r = _scan_node(g, inp, xbc=xbc)
        return [r], [r]

    y, st = _split_scan(_run(backend, build)[0], inp)
    ey, es = S.scan_excess(ref, gates, y, st)
    ky = float(np.max(np.abs(y.astype(np.float64) - ref["y"]) / (S.U * ref["ey"][(0, 0)])))
    ks = float(np.max(np.abs(st.astype(np.float64) - ref["st"]) / (S.U * ref["es"][(0, 0)])))
    plog(f"  ssm_scan {name}: f32 twin R = {R:.3f} of the roundings-only bound; kernel y {ky:.3f}, states {ks:.3f} of it; of the gate: y {ey:.3f}, states {es:.3f}")
    assert ey <= 1.0 and es <= 1.0, (name, ey, es)


@pytest.mark.parametrize("name", [n for n in sorted(S.SCAN_CASES) if S.SCAN_CASES[n][6]])
def test_ssm_scan_mamba1_form(backend, plog, name):
    _scan_case(backend, plog, name)


@pytest.mark.parametrize("name", [n for n in sorted(S.SCAN_CASES) if not S.SCAN_CASES[n][6]])
def test_ssm_scan_mamba2_form(backend, plog, name):
    _scan_case(backend, plog, name)


# ------------------------------------------------------------------------------------------------ 5. a layer
N_EMBD, D_INNER, D_CONV, N_S, N_RS, EPS = 64, 128, 4, 2, 4, 1e-5
# The layer's bound.  Every stage is an f32 evaluation whose error is at most (terms + 2) 2^-24 of the stage's absolute-value envelope, and every stage's map is
# Lipschitz with a constant of order one on these inputs (silu's slope <= 1.1, softplus's <= 1, the scan's dependence on dt through exp(dtp A) with |dtp A| of
# order one to ten, the group norm's 1 / rms), so a stage's error reaches the output as about that share of the output's own envelope sum |W_out| |v|.  The stage
# widths, in units of 2^-24: ssm_in 64 + 2; the conv, its bias and silu 4 + 1 + 8; ssm_x (Mamba-1) 128 + 2 and ssm_dt 4 + 2; the scan over 7 tokens 7 * 12 for the
# recurrence plus d_state + 1 (up to 128 + 1) for y; y + x D and SwiGLU 3; the group norm (Mamba-2) 128 + 2; ssm_out 128 + 2 — 691 together — and a factor four for
# the Lipschitz constants and the envelopes' ratios: LAYER_K = 4 * 691 units of 2^-24 of the output's envelope, 1.6e-4 of it, where a mistake in an op is of order one.
LAYER_K = 4 * 691


class Layer:
    """One Mamba (kind 1) or Mamba-2 (kind 2) layer: F32 weights, the node sequence of llama.cpp's build_mamba_layer / build_mamba2_layer, and its float64 twin
    over the same persistent caches (conv states [d_conv - 1, conv_dim] and scan states [d_state, head_dim, n_head] per cache row)."""

    def __init__(self, kind, seed):
        rng = np.random.default_rng(seed)
        self.kind = kind
        f = np.float32
        if kind == 1:
            self.d_state, self.head_dim, self.n_head, self.n_group, self.dt_rank = 16, 1, D_INNER, 1, 4
            self.conv_dim = D_INNER
            self.d_in = 2 * D_INNER
            self.w_x = (rng.standard_normal((self.dt_rank + 2 * self.d_state, D_INNER)) / np.sqrt(D_INNER)).astype(f)
            self.w_dt = (rng.standard_normal((D_INNER, self.dt_rank)) / np.sqrt(self.dt_rank)).astype(f)
            self.dt_b = rng.uniform(-2.0, 1.0, D_INNER).astype(f)
            self.A = (-(np.arange(1, self.d_state + 1))[None, :] * rng.uniform(0.05, 0.2, (D_INNER, 1))).astype(f)
            self.D = rng.standard_normal(D_INNER).astype(f)
        else:
            self.d_state, self.head_dim, self.n_head, self.n_group = 128, 64, 2, 1
            self.conv_dim = D_INNER + 2 * self.n_group * self.d_state
            self.d_in = 2 * D_INNER + 2 * self.n_group * self.d_state + self.n_head
            self.dt_b = rng.uniform(-2.0, 1.0, self.n_head).astype(f)
            self.A = (-rng.uniform(0.1, 1.0, (self.n_head, 1))).astype(f)
            self.D = rng.standard_normal((self.n_head, 1)).astype(f)
            self.norm_w = rng.uniform(0.5, 1.5, D_INNER).astype(f)
        self.w_in = (rng.standard_normal((self.d_in, N_EMBD)) / np.sqrt(N_EMBD)).astype(f)
        self.conv_w = (rng.standard_normal((self.conv_dim, D_CONV)) / 2).astype(f)
        self.conv_b = rng.standard_normal(self.conv_dim).astype(f) / 4
        self.w_out = (rng.standard_normal((N_EMBD, D_INNER)) / np.sqrt(D_INNER)).astype(f)
        self.conv0 = rng.standard_normal((N_RS, self.conv_dim, D_CONV - 1)).astype(f)
        self.ssm0 = rng.standard_normal((N_RS, self.n_head, self.head_dim, self.d_state)).astype(f)

    # -------------------------------------------------------------------------------------------- graph
    def tensors(self, g):
        """Weights and the two caches, once per context."""
        t = {}
        t["w_in"] = g.new(F32, [N_EMBD, self.d_in], self.w_in)
        t["conv_w"] = g.new(F32, [D_CONV, self.conv_dim], self.conv_w)
        t["conv_b"] = g.new(F32, [self.conv_dim], self.conv_b)
        t["w_out"] = g.new(F32, [D_INNER, N_EMBD], self.w_out)
        t["A"] = g.new(F32, [self.A.shape[1], self.n_head], self.A)
        t["dt_b"] = g.new(F32, [self.dt_b.size], self.dt_b)
        if self.kind == 1:
            t["w_x"] = g.new(F32, [D_INNER, self.dt_rank + 2 * self.d_state], self.w_x)
            t["w_dt"] = g.new(F32, [self.dt_rank, D_INNER], self.w_dt)
            t["D"] = g.new(F32, [D_INNER], self.D)
        else:
            t["D"] = g.new(F32, [1, self.n_head], self.D)
            t["norm_w"] = g.new(F32, [D_INNER // self.n_group, self.n_group], self.norm_w)
        t["conv_all"] = g.new(F32, [(D_CONV - 1) * self.conv_dim, N_RS], self.conv0)
        t["ssm_all"] = g.new(F32, [self.d_state * D_INNER, N_RS], self.ssm0)
        return t

    def graph(self, g, t, n_t, head):
        """The layer over [n_embd, n_t, N_S] tokens writing the states of its sequences to cache rows head, head + 1; returns (gf, x_in, ids, out)."""
        H, ctx = g.H, g.ctx
        ds, hd, nh, ng, cd = self.d_state, self.head_dim, self.n_head, self.n_group, self.conv_dim
        x_in, ids = g.new(F32, [N_EMBD, n_t, N_S]), g.new(I32, [N_S])
        gf = H.ggml_new_graph_custom(ctx, 512, False)
        # the state bookkeeping of build_rs for a batch that clears no state and has no extra cells: three nodes over zero elements
        n_r = (D_CONV - 1) * cd
        none = g.new(I32, [0])
        H.ggml_build_forward_expand(gf, H.ggml_scale(ctx, H.ggml_view_2d(ctx, t["conv_all"], n_r, 0, n_r * 4, 0), 0.0))
        extra = H.ggml_get_rows(ctx, t["conv_all"], none)
        H.ggml_build_forward_expand(gf, H.ggml_cpy(ctx, extra, H.ggml_view_1d(ctx, t["conv_all"], 0, 0)))
        conv = H.ggml_reshape_3d(ctx, H.ggml_get_rows(ctx, t["conv_all"], ids), D_CONV - 1, cd, N_S)
        proj = H.ggml_mul_mat(ctx, t["w_in"], x_in)  # [d_in, n_t, N_S]
        nb1, nb2 = self.d_in * 4, self.d_in * 4 * n_t
        if self.kind == 1:
            xc = H.ggml_view_3d(ctx, proj, D_INNER, n_t, N_S, nb1, nb2, 0)
            z = H.ggml_view_3d(ctx, proj, D_INNER, n_t, N_S, nb1, nb2, D_INNER * 4)
        else:
            z = H.ggml_view_4d(ctx, proj, hd, nh, n_t, N_S, hd * 4, nb1, nb2, 0)
            xc = H.ggml_view_3d(ctx, proj, cd, n_t, N_S, nb1, nb2, D_INNER * 4)
            dt = H.ggml_view_3d(ctx, proj, nh, n_t, N_S, nb1, nb2, (D_INNER + cd) * 4)
        conv_x = H.ggml_concat(ctx, conv, H.ggml_transpose(ctx, xc), 0)  # [d_conv - 1 + n_t, conv_dim, N_S]
        ncs = D_CONV - 1 + n_t
        last = H.ggml_view_3d(ctx, conv_x, D_CONV - 1, cd, N_S, ncs * 4, ncs * 4 * cd, n_t * 4)
        H.ggml_build_forward_expand(gf, H.ggml_cpy(ctx, last, H.ggml_view_1d(ctx, t["conv_all"], n_r * N_S, head * n_r * 4)))
        xa = H.ggml_silu(ctx, H.ggml_add(ctx, H.ggml_ssm_conv(ctx, conv_x, t["conv_w"]), t["conv_b"]))  # [conv_dim, n_t, N_S]
        if self.kind == 1:
            w = self.dt_rank + 2 * ds
            x_db = H.ggml_mul_mat(ctx, t["w_x"], xa)  # [dt_rank + 2 d_state, n_t, N_S]
            dtr = H.ggml_view_3d(ctx, x_db, self.dt_rank, n_t, N_S, w * 4, w * 4 * n_t, 0)
            B = H.ggml_view_4d(ctx, x_db, ds, 1, n_t, N_S, ds * 4, w * 4, w * 4 * n_t, self.dt_rank * 4)
            Cc = H.ggml_view_4d(ctx, x_db, ds, 1, n_t, N_S, ds * 4, w * 4, w * 4 * n_t, (self.dt_rank + ds) * 4)
            dt = H.ggml_add(ctx, H.ggml_mul_mat(ctx, t["w_dt"], dtr), t["dt_b"])  # [d_inner, n_t, N_S]
            x = H.ggml_reshape_4d(ctx, xa, 1, D_INNER, n_t, N_S)
        else:
            x = H.ggml_view_4d(ctx, xa, hd, nh, n_t, N_S, hd * 4, cd * 4, cd * 4 * n_t, 0)
            B = H.ggml_view_4d(ctx, xa, ds, ng, n_t, N_S, ds * 4, cd * 4, cd * 4 * n_t, D_INNER * 4)
            Cc = H.ggml_view_4d(ctx, xa, ds, ng, n_t, N_S, ds * 4, cd * 4, cd * 4 * n_t, (D_INNER + ng * ds) * 4)
            dt = H.ggml_add(ctx, H.ggml_cont(ctx, dt), t["dt_b"])  # [n_head, n_t, N_S]
        ssm = H.ggml_reshape_4d(ctx, t["ssm_all"], ds, hd, nh, N_RS)
        y_ssm = H.ggml_ssm_scan(ctx, ssm, x, dt, t["A"], B, Cc, ids)
        n_y, n_st = D_INNER * n_t * N_S, ds * D_INNER
        H.ggml_build_forward_expand(gf, H.ggml_cpy(ctx, H.ggml_view_1d(ctx, y_ssm, n_st * N_S, n_y * 4), H.ggml_view_1d(ctx, t["ssm_all"], n_st * N_S, head * n_st * 4)))
        if self.kind == 1:
            y = H.ggml_view_3d(ctx, y_ssm, D_INNER, n_t, N_S, D_INNER * 4, D_INNER * 4 * n_t, 0)
            y = H.ggml_add(ctx, y, H.ggml_mul(ctx, xa, t["D"]))
            y = H.ggml_swiglu_split(ctx, H.ggml_cont(ctx, z), y)
        else:
            y = H.ggml_view_4d(ctx, y_ssm, hd, nh, n_t, N_S, hd * 4, D_INNER * 4, D_INNER * 4 * n_t, 0)
            y = H.ggml_add(ctx, y, H.ggml_mul(ctx, x, t["D"]))
            y = H.ggml_swiglu_split(ctx, H.ggml_cont(ctx, z), y)
            y = H.ggml_reshape_4d(ctx, y, D_INNER // ng, ng, n_t, N_S)
            y = H.ggml_mul(ctx, H.ggml_rms_norm(ctx, y, EPS), t["norm_w"])
            y = H.ggml_reshape_3d(ctx, y, D_INNER, n_t, N_S)
        out = H.ggml_mul_mat(ctx, t["w_out"], y)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        return gf, x_in, ids, out

    # -------------------------------------------------------------------------------------------- float64 twin
    def twin(self, conv_all, ssm_all, x_in, ids, head):
        """One step on float64 caches (updated in place): x_in (N_S, n_t, n_embd) -> (out (N_S, n_t, n_embd), envelope sum |W_out| |v|)."""
        n_t = x_in.shape[1]
        ds, hd, nh, ng, cd = self.d_state, self.head_dim, self.n_head, self.n_group, self.conv_dim
        proj = x_in.astype(np.float64) @ self.w_in.astype(np.float64).T  # (N_S, n_t, d_in)
        if self.kind == 1:
            xc, z = proj[..., :D_INNER], proj[..., D_INNER:]
        else:
            z, xc, dt = proj[..., :D_INNER], proj[..., D_INNER:D_INNER + cd], proj[..., D_INNER + cd:]
        conv_x = np.concatenate([conv_all[ids], xc.transpose(0, 2, 1)], axis=2)  # (N_S, conv_dim, d_conv - 1 + n_t)
        new_conv = conv_x[:, :, n_t:].copy()
        w = np.stack([conv_x[..., k:k + n_t] for k in range(D_CONV)], axis=-1)
        xa = S.silu64((w * self.conv_w.astype(np.float64)[None, :, None, :]).sum(-1).transpose(0, 2, 1) + self.conv_b.astype(np.float64))  # (N_S, n_t, conv_dim)
        if self.kind == 1:
            x_db = xa @ self.w_x.astype(np.float64).T
            dt = x_db[..., :self.dt_rank] @ self.w_dt.astype(np.float64).T + self.dt_b.astype(np.float64)
            B, Cc = x_db[..., self.dt_rank:self.dt_rank + ds], x_db[..., self.dt_rank + ds:]
            x = xa
        else:
            x, B, Cc = xa[..., :D_INNER], xa[..., D_INNER:D_INNER + ng * ds], xa[..., D_INNER + ng * ds:]
            dt = dt + self.dt_b.astype(np.float64)
        dtp = np.where(dt <= 20.0, np.log1p(np.exp(np.minimum(dt, 20.0))), dt)  # (N_S, n_t, n_head)
        x4 = x.reshape(N_S, n_t, nh, hd)
        B4, C4 = B.reshape(N_S, n_t, ng, ds), Cc.reshape(N_S, n_t, ng, ds)
        gi = np.zeros(nh, dtype=np.int64) if ng == 1 else np.arange(nh)
        y = np.zeros((N_S, n_t, nh, hd))
        new_ssm = np.zeros((N_S, nh, hd, ds))
        A = self.A.astype(np.float64)
        for i3 in range(N_S):
            state = ssm_all[ids[i3]].copy()
            for i2 in range(n_t):
                a = np.exp(dtp[i3, i2][:, None] * A)[:, None, :]
                state = state * a + B4[i3, i2][gi][:, None, :] * (x4[i3, i2] * dtp[i3, i2][:, None])[:, :, None]
                y[i3, i2] = (state * C4[i3, i2][gi][:, None, :]).sum(-1)
            new_ssm[i3] = state
        conv_all[head:head + N_S] = new_conv
        ssm_all[head:head + N_S] = new_ssm
        y = y + x4 * self.D.astype(np.float64).reshape(nh, -1)
        v = S.silu64(z) * y.reshape(N_S, n_t, D_INNER)
        if self.kind == 2:
            vg = v.reshape(N_S, n_t, ng, D_INNER // ng)
            vg = vg / np.sqrt((vg * vg).mean(-1, keepdims=True) + EPS)
            v = vg.reshape(N_S, n_t, D_INNER) * self.norm_w.astype(np.float64)
        wo = self.w_out.astype(np.float64)
        return v @ wo.T, np.abs(v) @ np.abs(wo).T


def _layer_inputs(kind):
    rng = np.random.default_rng(40 + kind)
    prompt = (rng.standard_normal((N_S, 7, N_EMBD)).astype(np.float32), np.array([2, 3], dtype=np.int32), 0)
    # the decode graph writes rows 2, 3; every step starts from the rows the step before wrote, the second with the sequences swapped
    steps = [(rng.standard_normal((N_S, 1, N_EMBD)).astype(np.float32), np.array(i, dtype=np.int32), 2) for i in ([0, 1], [3, 2], [2, 3])]
    return prompt, steps


def _run_layer(backend, lay):
    """The prompt graph once, then the ONE decode graph three times, on the same buffers: per step (out, conv cache, scan cache) and the stat deltas of the decode steps."""
    H = L.host()
    g = T.G(backend)
    prompt, steps = _layer_inputs(lay.kind)
    try:
        t = lay.tensors(g)
        gp = lay.graph(g, t, 7, prompt[2])
        gd = lay.graph(g, t, 1, steps[0][2])
        for gf in (gp[0], gd[0]):
            for i in range(gf.contents.n_nodes):
                node = gf.contents.nodes[i]
                assert H.ggml_backend_dev_supports_op(backend.dev, node), (i, H.ggml_op_name(node.contents.op), node.contents.name)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        res = []

        def step(graph, x, ids):
            gf, x_t, ids_t, out = graph
            for tt, raw in ((x_t, np.ascontiguousarray(x)), (ids_t, np.ascontiguousarray(ids))):
                H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(out).copy(), g.read(t["conv_all"]).copy(), g.read(t["ssm_all"]).copy()))

        step(gp, prompt[0], prompt[1])
        s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures", "eager_graphs", "kernel_launches", "fused_nodes")}
        for x, ids, _ in steps:
            step(gd, x, ids)
        return res, {k: backend.stat(k) - v for k, v in s0.items()}
    finally:
        g.free()


@pytest.mark.parametrize("kind", [1, 2])
def test_layer_prompt_then_decode_steps_against_the_float64_twin(backend, plog, kind):
    lay = Layer(kind, 100 + kind)
    res, stats = _run_layer(backend, lay)
    prompt, steps = _layer_inputs(kind)
    conv_all, ssm_all = lay.conv0.astype(np.float64), lay.ssm0.astype(np.float64)
    worst = 0.0
    for k, ((x, ids, head), (out, conv_g, ssm_g)) in enumerate(zip([prompt] + steps, res)):
        want, env = lay.twin(conv_all, ssm_all, x, ids, head)
        ex = float(np.max(np.abs(out.reshape(want.shape).astype(np.float64) - want) / (LAYER_K * S.U * env)))
        worst = max(worst, ex)
        assert ex <= 1.0, (kind, k, ex)
        # the caches carry: what the step wrote is what the twin's step wrote, to the same relative bound of each cache's largest value
        for got, ref in ((conv_g, conv_all), (ssm_g, ssm_all)):
            assert float(np.max(np.abs(got.reshape(ref.shape).astype(np.float64) - ref))) <= LAYER_K * S.U * float(np.max(np.abs(ref))), (kind, k)
    plog(f"  mamba{'' if kind == 1 else '-2'} layer: worst output error {worst:.4f} of LAYER_K 2^-24 sum |W_out| |v| over a 7-token prompt and three decode steps; decode stats {stats}")


@pytest.mark.parametrize("kind", [1, 2])
def test_layer_decode_graph_is_captured_and_replays_follow_the_ids(backend, plog, kind):
    """The decode-step graph computed three times with other inputs and permuted ids: steps two and three launch the captured hipGraph (graph_launches rises by two,
    one capture), the ids are read on the device, the state cache carries from step to step — all bit-equal to a backend with graphs off."""
    lay = Layer(kind, 100 + kind)
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            runs[mode] = _run_layer(backend, lay)
    finally:
        backend.set_option("graphs", 1)
    plog(f"  mamba{'' if kind == 1 else '-2'} layer capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["graph_captures"] == 0, runs[0][1]
    for a, b in zip(runs[1][0], runs[0][0]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
    # the cache carried: the rows the decode graph writes differ after every step, and the other rows never change behind the prompt step
    caches = [r[2].reshape(N_RS, -1) for r in runs[0][0]]
    for k in (1, 2, 3):
        assert not np.array_equal(caches[k][2:], caches[k - 1][2:]) and np.array_equal(caches[k][:2], caches[0][:2])
