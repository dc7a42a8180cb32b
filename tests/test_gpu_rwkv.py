"""GPU: csrc/rwkv.hip through the C-ABI — RWKV_WKV6, GATED_LINEAR_ATTN and RWKV_WKV7 against the gates of tests/rwkv_ref.py (the CPU oracle has none of the ops),
L2_NORM against its gate, SQR and REPEAT bit for bit, then an RWKV-6 layer, an RWKV-7 layer and a QRWKV6 time mix over persistent state buffers, eager and as a
replayed hipGraph.

Every value test here fails on a backend without these ops: harness.G.compute raises supports_op=false at the first new node; the acceptance test fails outright.
"""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import rwkv_ref as R

pytestmark = pytest.mark.gpu
F32, F16, I32, Q8_0 = L.F32, L.F16, L.I32, L.Q8_0
NEG, TANH, RELU, SIGMOID, SILU, EXP = 2, 4, 6, 7, 10, 13  # ggml_unary_op
# the kernels' token chunks as built (rwkv.hip: wkv6_geom / wkv7_geom): WKV6 and GLA 1024 / S, WKV7 512 / S
CHUNK = {("wkv6", 64): 16, ("wkv6", 128): 8, ("gla", 64): 16, ("gla", 128): 8, ("wkv7", 64): 8, ("wkv7", 128): 4}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(target, build):
    """build(g) -> the tensors to read after one compute of all of them."""
    g = T.G(target)
    try:
        outs = build(g)
        g.compute(list(outs))
        return [g.read(t) for t in outs]
    finally:
        g.free()


def _np_permute(arr, axes):
    """ggml_permute(a, *axes) as an array: source dimension i becomes dimension axes[i] (NumPy axis = 3 - ggml dimension)."""
    perm = [0] * 4
    for i, ax in enumerate(axes):
        perm[3 - ax] = 3 - i
    return np.transpose(arr, perm)


def _wkv_node(g, op, inp):
    """The recurrent node over the arrays of a rwkv_ref case; the state is the [S S H, n_seqs] matrix llama.cpp's build_rs hands over."""
    H, ctx = g.H, g.ctx
    n_seqs, nh, S, _ = inp["state"].shape
    Tn = inp["k"].shape[0]
    t = {n: g.new(F32, [S, nh, Tn], inp[n]) for n in R.N_SRC[op] if n not in ("tf", "state")}
    state = g.new(F32, [S * S * nh, n_seqs], inp["state"])
    if op == "wkv6":
        return H.ggml_rwkv_wkv6(ctx, t["k"], t["v"], t["r"], g.new(F32, [S, nh], inp["tf"]), t["td"], state)
    if op == "gla":
        return H.ggml_gated_linear_attn(ctx, t["k"], t["v"], t["q"], t["g"], state, float(inp["scale"]))
    return H.ggml_rwkv_wkv7(ctx, t["r"], t["w"], t["k"], t["v"], t["a"], t["b"], state)


def _empty_wkv(H, ctx, op, S, nh, Tn, n_seqs, typ=F32):
    x = [H.ggml_new_tensor_3d(ctx, typ, S, nh, Tn) for _ in range(6)]
    state = H.ggml_new_tensor_2d(ctx, F32, S * S * nh, n_seqs)
    if op == "wkv6":
        return H.ggml_rwkv_wkv6(ctx, x[0], x[1], x[2], H.ggml_new_tensor_2d(ctx, typ, S, nh), x[3], state)
    if op == "gla":
        return H.ggml_gated_linear_attn(ctx, x[0], x[1], x[2], x[3], state, 0.125)
    return H.ggml_rwkv_wkv7(ctx, x[0], x[1], x[2], x[3], x[4], x[5], state)


# ------------------------------------------------------------------------------------------------ 1. acceptance, 2. refusals
def test_supports_op_accepts_the_six_ops(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        for op in R.OPS:
            for S in (64, 128):
                for nh, Tn, n_seqs in ((1, 1, 1), (3, 6, 3), (64, 32, 32), (40, 512, 1)):
                    assert ok(_empty_wkv(H, ctx, op, S, nh, Tn, n_seqs)), (op, S, nh, Tn, n_seqs)
        assert ok(H.ggml_l2_norm(ctx, H.ggml_new_tensor_3d(ctx, F32, 64, 40, 7), 1e-12))
        big = H.ggml_new_tensor_3d(ctx, F32, 70, 5, 3)
        assert ok(H.ggml_l2_norm(ctx, H.ggml_view_3d(ctx, big, 64, 5, 3, 70 * 4, 70 * 5 * 4, 0), 1e-12))
        assert ok(H.ggml_sqr(ctx, H.ggml_new_tensor_2d(ctx, F32, 448, 7)))
        sx = H.ggml_new_tensor_4d(ctx, F32, 128, 2, 3, 1)
        assert ok(H.ggml_repeat(ctx, sx, H.ggml_new_tensor_4d(ctx, F32, 128, 2, 3, 6)))
        assert ok(H.ggml_repeat(ctx, H.ggml_permute(ctx, H.ggml_new_tensor_4d(ctx, F32, 4, 3, 2, 1), 1, 0, 2, 3), H.ggml_new_tensor_4d(ctx, F32, 6, 4, 4, 2)))
    finally:
        g.free()


def test_supports_op_refuses_what_is_outside_the_contract(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        for op in R.OPS:
            n_src = len(R.N_SRC[op])
            for S in (32, 96, 256):
                assert not ok(_empty_wkv(H, ctx, op, S, 2, 4, 2)), (op, S)
            assert not ok(_empty_wkv(H, ctx, op, 64, 2, 5, 2)), op                  # T % n_seqs != 0
            assert not ok(_empty_wkv(H, ctx, op, 64, 2, 4, 2, typ=F16)), op         # f16 operands
            def patched(i, src):  # a node of the contract's shape (accepted) with source i replaced
                node = _empty_wkv(H, ctx, op, 64, 2, 4, 2)
                assert ok(node)
                node.contents.src[i] = src
                return node

            assert not ok(patched(1, H.ggml_new_tensor_3d(ctx, F16, 64, 2, 4))), op   # one f16 operand among f32 ones
            wide = H.ggml_new_tensor_3d(ctx, F32, 80, 2, 4)                            # src[0] with rows further apart than their length
            assert not ok(patched(0, H.ggml_view_3d(ctx, wide, 64, 2, 4, 80 * 4, 80 * 2 * 4, 0))), op
            assert not ok(patched(n_src - 1, H.ggml_new_tensor_2d(ctx, F32, 64 * 64 * 2 // 2, 2))), op  # a state with one sequence's elements missing
            node = _empty_wkv(H, ctx, op, 64, 2, 4, 2)
            node.contents.ne[1] -= 1                                                   # a dst one row short
            assert not ok(node), op
        rep = H.ggml_repeat(ctx, H.ggml_new_tensor_2d(ctx, F32, 4, 3), H.ggml_new_tensor_2d(ctx, F32, 8, 6))
        rep.contents.src[0] = H.ggml_new_tensor_2d(ctx, F32, 3, 3)                  # 8 is no whole multiple of 3 (the builder itself refuses to build this)
        assert not ok(rep)
        assert not ok(H.ggml_repeat(ctx, H.ggml_new_tensor_2d(ctx, F16, 4, 3), H.ggml_new_tensor_2d(ctx, F16, 8, 6)))
        assert not ok(H.ggml_sqr(ctx, H.ggml_transpose(ctx, H.ggml_new_tensor_2d(ctx, F32, 8, 6))))  # a non-contiguous source
        assert not ok(H.ggml_sqr(ctx, H.ggml_new_tensor_2d(ctx, F16, 8, 6)))
        assert not ok(H.ggml_l2_norm(ctx, H.ggml_new_tensor_2d(ctx, F16, 64, 6), 1e-12))
        assert not ok(H.ggml_l2_norm(ctx, H.ggml_transpose(ctx, H.ggml_new_tensor_2d(ctx, F32, 8, 6)), 1e-12))
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ 3. the recurrences against their gates
def _cases(op, S):
    """(H, n_seqs, n_t, kind): the grid, one token beside each side of the kernel's chunk boundary and the boundary itself, and the three special inputs."""
    c = [(nh, n_seqs, n_t, "rand") for nh in (1, 3) for n_seqs in (1, 3) for n_t in (1, 2, 5)]
    tc = CHUNK[(op, S)]
    c += [(1, 1, tc - 1, "rand"), (1, 3, tc, "rand"), (3, 1, tc + 1, "rand"), (1, 1, 2 * tc + 1, "rand")]
    c += [(3, 3, 5, kind) for kind in ("indicator", "zero_decay", "unit_decay")]
    return c


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("op", R.OPS)
def test_recurrence_within_the_gate(backend, plog, op, S):
    cases = _cases(op, S)
    inps = [R.inputs(op, S, nh, n_seqs, n_t, kind) for nh, n_seqs, n_t, kind in cases]
    got = _run(backend, lambda g: [_wkv_node(g, op, inp) for inp in inps])
    worst = (0.0, 0.0)
    for case, inp, flat in zip(cases, inps, got):
        ref = R.twin64(op, inp)
        y, st = R.split(flat, inp)
        ey, es = R.excess(ref, y, st)
        worst = (max(worst[0], ey), max(worst[1], es))
        assert ey <= 1.0 and es <= 1.0, (op, S, case, ey, es)
        if case[3] == "zero_decay" and op != "wkv7":  # the state is forgotten: what is left is the last token's outer product, exactly (WKV7 keeps sa b)
            assert np.array_equal(_bits(st[-1]), _bits(inp["k"][-1][:, :, None] * inp["v"][-1][:, None, :]))
        if case[3] == "indicator" and case[2] == 5:
            nz = np.count_nonzero(st)
            assert 0 < nz <= st.shape[0] * st.shape[1] * 5, nz  # at most one cell per token and head
    plog(f"  {op} S {S}: {len(cases)} cases, worst error y {worst[0]:.3f}, states {worst[1]:.3f} of the gate")


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("op", R.OPS)
def test_launches_are_deterministic_and_sequences_independent(backend, op):
    for S, n_t in ((64, CHUNK[(op, 64)] + 1), (128, 2)):
        inp = R.inputs(op, S, 3, 3, n_t)
        alone = [R.one_sequence(op, inp, s) for s in range(3)]
        got = _run(backend, lambda g: [_wkv_node(g, op, inp), _wkv_node(g, op, inp)] + [_wkv_node(g, op, a) for a in alone])
        assert np.array_equal(_bits(got[0]), _bits(got[1]))
        y, st = R.split(got[0], inp)
        for s in range(3):
            y1, st1 = R.split(got[2 + s], alone[s])
            assert np.array_equal(_bits(y1), _bits(y[s * n_t:(s + 1) * n_t])) and np.array_equal(_bits(st1[0]), _bits(st[s])), (op, S, s)


# ------------------------------------------------------------------------------------------------ 5. L2_NORM
def test_l2_norm_within_the_gate(backend, H, plog):
    rng = np.random.default_rng(5)
    eps = 1e-6
    xs = []
    for ne0 in (1, 63, 64, 65, 128, 4096):
        x = rng.standard_normal((2, 3, ne0)).astype(np.float32)
        x[0, 1] = 0.0          # an all-zero row: the eps path, 0 / eps
        x[1, 2] *= 1e-9        # a norm below eps: x / eps
        xs.append(x)
    wide = rng.standard_normal((3, 5, 70)).astype(np.float32)  # a 3-D source whose rows are 70 floats apart and 64 long
    wide[2, 4] = 0.0
    heads = rng.standard_normal((40, 2, 64)).astype(np.float32)  # RWKV-7's use: one row a head and token, eps 1e-12

    def build(g):
        outs = [H.ggml_l2_norm(g.ctx, g.new(F32, list(x.shape[::-1]), x), eps) for x in xs]
        tw = g.new(F32, [70, 5, 3], wide)
        outs.append(H.ggml_l2_norm(g.ctx, H.ggml_view_3d(g.ctx, tw, 64, 5, 3, 70 * 4, 70 * 5 * 4, 0), eps))
        outs.append(H.ggml_l2_norm(g.ctx, g.new(F32, [64, 2, 40], heads), 1e-12))
        return outs

    got = _run(backend, build)
    worst = 0.0
    for x, r in zip(xs + [wide[:, :, :64]], got):
        want = R.l2_norm64(x, eps)
        r = r.reshape(want.shape).astype(np.float64)
        gate = R.l2_norm_gate(x, eps)
        assert np.all(np.abs(r - want) <= gate), x.shape
        nz = gate > 0
        worst = max(worst, float(np.max(np.abs(r - want)[nz] / gate[nz])))
        small = np.sqrt((x.astype(np.float64) ** 2).sum(-1)) < eps
        assert small.any() and np.all(np.abs(r[small] - x[small].astype(np.float64) / eps) <= 4 * R.U * np.abs(x[small].astype(np.float64) / eps))
    n = np.sqrt((got[-1].astype(np.float64) ** 2).sum(-1))
    assert np.all(np.abs(n - 1.0) <= 70 * R.U)  # RWKV-7's use: unit rows
    plog(f"  l2_norm: worst error {worst:.3f} of (ne0 + 4) 2^-24 |y|")


# ------------------------------------------------------------------------------------------------ 6. SQR, 7. REPEAT
def test_sqr_bit_exact(backend, H):
    rng = np.random.default_rng(6)
    xs = [(rng.standard_normal(n) * 100).astype(np.float32) for n in (1, 255, 256, 257, 4097)]
    xs.append((rng.standard_normal((3, 7, 448))).astype(np.float32))  # the channel mix's shape: relu(W_k x) of a batch
    got = _run(backend, lambda g: [H.ggml_sqr(g.ctx, g.new(F32, list(x.shape[::-1]), x)) for x in xs])
    for x, r in zip(xs, got):
        assert np.array_equal(_bits(r.reshape(x.shape)), _bits(R.sqr(x))), x.shape


def test_repeat_bit_exact(backend, H):
    rng = np.random.default_rng(7)
    f = np.float32
    sx = rng.standard_normal((1, 3, 2, 128)).astype(f)        # RWKV-7: [n_embd, n_t, n_s, 1] -> [.., 6]
    every = rng.standard_normal((2, 3, 1, 5)).astype(f)       # every dimension at once: [5, 1, 3, 2] -> [10, 4, 9, 4]
    perm = rng.standard_normal((1, 2, 3, 4)).astype(f)        # [4, 3, 2, 1] permuted (1, 0, 2, 3) -> [3, 4, 2, 1], repeated to [6, 4, 4, 2]
    row = rng.standard_normal((1, 1, 1, 1)).astype(f)         # one element to more than one workgroup

    def build(g):
        def rep(a, ne):
            return H.ggml_repeat(g.ctx, a, g.new(F32, ne))
        return [rep(g.new(F32, [128, 2, 3, 1], sx), [128, 2, 3, 6]), rep(g.new(F32, [5, 1, 3, 2], every), [10, 4, 9, 4]),
                rep(H.ggml_permute(g.ctx, g.new(F32, [4, 3, 2, 1], perm), 1, 0, 2, 3), [6, 4, 4, 2]), rep(g.new(F32, [1, 1, 1, 1], row), [33, 5, 2, 2])]

    got = _run(backend, build)
    want = [R.repeat(sx, [128, 2, 3, 6]), R.repeat(every, [10, 4, 9, 4]), R.repeat(_np_permute(perm, (1, 0, 2, 3)), [6, 4, 4, 2]), R.repeat(row, [33, 5, 2, 2])]
    for k, (r, w) in enumerate(zip(got, want)):
        assert r.shape == w.shape and np.array_equal(_bits(r), _bits(w)), k


# ------------------------------------------------------------------------------------------------ 8. whole layers
N_EMBD, N_HEAD, HS, LORA, N_FF, N_S, N_T, NORM_EPS = 128, 2, 64, 32, 256, 2, 2, 64e-5
N_TOK = N_S * N_T


def _q8_rows(x):
    """ggml's quantize_row_q8_0 over the last axis: (q (.., K / 32, 32) f32 integers, d (.., K / 32) f32 through f16)."""
    xb = np.asarray(x, dtype=np.float32).reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    d = (np.abs(xb).max(-1) / np.float32(127.0)).astype(np.float32)
    inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    v = xb * inv[..., None]
    q = np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))  # roundf: halves away from zero
    return q.astype(np.float32), d.astype(np.float16).astype(np.float32)


class Weights:
    """Named weights of a layer: Q8_0 projection matrices (raw blocks for the device, scales and quants for the twins) and f32 tensors."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.q8, self.f32, self.ne = {}, {}, {}

    def add_q8(self, name, K, N):
        raw = T.rand_weight(Q8_0, K, N, self.rng)
        blk = raw.reshape(N, K // 32, 34)
        d = np.ascontiguousarray(blk[:, :, :2]).view(np.float16).astype(np.float32)[..., 0]
        q = np.ascontiguousarray(blk[:, :, 2:]).view(np.int8).astype(np.float32)
        self.q8[name] = (raw, d, q, K, N)

    def add(self, name, ne, arr):
        arr = np.asarray(arr, dtype=np.float32)
        assert arr.size == int(np.prod(ne))
        self.f32[name], self.ne[name] = arr, list(ne)

    def mat(self, name, K, N, gain=1.0):
        self.add(name, [K, N], self.rng.standard_normal((N, K)) * gain / np.sqrt(K))

    def tensors(self, g):
        t = {n: g.new(Q8_0, [K, N], raw) for n, (raw, d, q, K, N) in self.q8.items()}
        t.update({n: g.new(F32, self.ne[n], a) for n, a in self.f32.items()})
        return t

    def mm(self, name, x, f):
        """x (.., K) -> (.., N).  float64: the dequantised weights, exact activations.  f32: ggml's arithmetic — the activations quantised to Q8_0 per block of 32,
        integer block sums, f32 products with the two scales — for the Q8_0 matrices, an f32 product for the others."""
        if name in self.f32:
            return np.asarray(x, dtype=f) @ self.f32[name].astype(f).T
        raw, d, q, K, N = self.q8[name]
        if f == np.float64:
            return np.asarray(x, dtype=f) @ (d[:, :, None].astype(f) * q.astype(f)).reshape(N, K).T
        qa, da = _q8_rows(x)
        isum = np.einsum("...bk,nbk->...nb", qa, q).astype(np.float32)  # (integers below 2^24: exact)
        return np.add.accumulate(isum * (da[..., None, :] * d), axis=-1, dtype=np.float32)[..., -1]


def _sig(x):
    return 1 / (1 + np.exp(-x))


def _head_norm(y, w, b, f):
    """ggml_norm over each head's S values, then * w + b."""
    yh = y.reshape(y.shape[:-1] + (N_HEAD, HS))
    m = yh.mean(-1, keepdims=True)
    c = yh - m
    yh = c / np.sqrt((c * c).mean(-1, keepdims=True) + f(NORM_EPS))
    return yh.reshape(y.shape) * w.astype(f) + b.astype(f)


class Layer:
    """arch 6: an RWKV-6 time mix and channel mix; 7: an RWKV-7 time mix (second-layer form, with v_first) and channel mix; 62: a QRWKV6 time mix with
    GATED_LINEAR_ATTN.  The node sequences are llama.cpp's build_rwkv6_time_mix / build_rwkv7_time_mix / build_rwkv*_channel_mix, over a persistent token-shift
    buffer [2 n_embd, n_seqs] and a persistent state buffer [S S H, n_seqs], both read through GET_ROWS and written back with CPY as build_rs does."""

    def __init__(self, arch, seed):
        self.arch = arch
        self.op = {6: "wkv6", 7: "wkv7", 62: "gla"}[arch]
        W = self.W = Weights(seed)
        rng = W.rng
        E = N_EMBD
        for n in ("receptance", "key", "value", "output") + (("gate",) if arch != 7 else ()):
            W.add_q8(n, E, E)
        if arch != 62:
            W.add_q8("cm_key", E, N_FF)
            W.add_q8("cm_value", N_FF, E)
            W.add("cm_lerp_k", [E], rng.uniform(0, 1, E))
        if arch == 6:
            W.add_q8("cm_receptance", E, E)
            W.add("cm_lerp_r", [E], rng.uniform(0, 1, E))
        if arch in (6, 62):
            W.add("lerp_x", [E], rng.uniform(0, 1, E))
            W.mat("w1", E, 5 * LORA)
            W.add("w2", [LORA, E, 5], rng.standard_normal((5, E, LORA)) / np.sqrt(LORA))
            for c in "wkvrg":
                W.add("lerp_" + c, [E], rng.uniform(0, 1, E))
            W.mat("decay_w1", E, LORA)
            W.mat("decay_w2", LORA, E)
            W.add("decay", [E], rng.uniform(-3.0, 0.5, E))
            if arch == 6:
                W.add("first", [HS, N_HEAD], rng.standard_normal((N_HEAD, HS)) * 0.5)
        else:
            W.add("lerp_fused", [E, 1, 1, 6], rng.uniform(0, 1, (6, E)))
            for c in "wavg":
                W.mat(c + "1", E, LORA)
                W.mat(c + "2", LORA, E)
            W.add("w0", [E], rng.uniform(-2.0, 2.0, E))
            W.add("a0", [E], rng.standard_normal(E))
            W.add("v0", [E], rng.standard_normal(E))
            W.add("k_k", [E], rng.uniform(0.5, 1.5, E))
            W.add("k_a", [E], rng.uniform(0.5, 1.5, E))
            W.add("r_k", [HS, N_HEAD], rng.standard_normal((N_HEAD, HS)) * 0.5)
        if arch != 62:
            W.add("ln_w", [E], rng.uniform(0.5, 1.5, E))
            W.add("ln_b", [E], rng.standard_normal(E) * 0.1)
        self.shift0 = rng.standard_normal((N_S, 2, E)).astype(np.float32)
        self.state0 = (rng.standard_normal((N_S, N_HEAD, HS, HS)) * 0.5).astype(np.float32)

    # -------------------------------------------------------------------------------------------- graph
    def graph(self, g):
        """Returns a dict: gf, the inputs x / v_first / ids, out, the caches, and the recurrent node `rec`."""
        H, ctx, E = g.H, g.ctx, N_EMBD
        t = self.W.tensors(g)
        u = lambda a, op: H.ggml_unary(ctx, a, op)
        mm = lambda n, a: H.ggml_mul_mat(ctx, t[n], a)
        add, sub, mul = (lambda a, b: H.ggml_add(ctx, a, b)), (lambda a, b: H.ggml_sub(ctx, a, b)), (lambda a, b: H.ggml_mul(ctx, a, b))
        r = {"shift_all": g.new(F32, [2 * E, N_S], self.shift0), "state_all": g.new(F32, [HS * HS * N_HEAD, N_S], self.state0)}
        r["x"], r["ids"] = g.new(F32, [E, N_T, N_S]), g.new(I32, [N_S])
        gf = r["gf"] = H.ggml_new_graph_custom(ctx, 1024, False)
        x3 = r["x"]
        shift = H.ggml_reshape_3d(ctx, H.ggml_get_rows(ctx, r["shift_all"], r["ids"]), E, 2, N_S)
        state = H.ggml_get_rows(ctx, r["state_all"], r["ids"])  # [S S H, n_seqs]

        def prev_of(cur3, slot):
            sh = H.ggml_view_3d(ctx, shift, E, 1, N_S, shift.contents.nb[1], shift.contents.nb[2], slot * E * 4)
            return H.ggml_concat(ctx, sh, H.ggml_view_3d(ctx, cur3, E, N_T - 1, N_S, cur3.contents.nb[1], cur3.contents.nb[2], 0), 1)

        def flat(a):
            return H.ggml_reshape_2d(ctx, a, E, N_TOK)

        def heads(a):
            return H.ggml_reshape_3d(ctx, a, HS, N_HEAD, N_TOK)

        cur = flat(x3)
        if self.arch in (6, 62):
            sx = flat(sub(prev_of(x3, 0), x3))
            xxx = add(mul(sx, t["lerp_x"]), cur)
            xxx = H.ggml_reshape_4d(ctx, u(mm("w1", xxx), TANH), LORA, 1, 5, N_TOK)
            xxx = H.ggml_cont(ctx, H.ggml_permute(ctx, xxx, 0, 1, 3, 2))
            xxx = H.ggml_mul_mat(ctx, H.ggml_reshape_4d(ctx, t["w2"], LORA, E, 1, 5), xxx)  # [n_embd, 1, n_tok, 5]
            mix = {c: H.ggml_view_2d(ctx, xxx, E, N_TOK, xxx.contents.nb[1], k * E * N_TOK * 4) for k, c in enumerate("wkvrg")}
            xs = {c: add(mul(add(mix[c], t["lerp_" + c]), sx), cur) for c in "wkvrg"}
            rr, k, v = mm("receptance", xs["r"]), mm("key", xs["k"]), mm("value", xs["v"])
            gate = u(mm("gate", xs["g"]), SIGMOID if self.arch == 62 else SILU)
            w = add(mm("decay_w2", u(mm("decay_w1", xs["w"]), TANH)), t["decay"])
            w = u(u(u(w, EXP), NEG), EXP)
            if self.arch == 62:
                k = sub(k, mul(k, w))  # k * (1 - w)
                rec = H.ggml_gated_linear_attn(ctx, heads(k), heads(v), heads(rr), heads(w), state, float(HS) ** -0.5)
            else:
                rec = H.ggml_rwkv_wkv6(ctx, heads(k), heads(v), heads(rr), t["first"], heads(w), state)
        else:
            r["v_first"] = g.new(F32, [E, N_TOK])
            sx = H.ggml_repeat(ctx, sub(prev_of(x3, 0), x3), g.new(F32, [E, N_T, N_S, 6]))
            xxx = add(mul(sx, t["lerp_fused"]), x3)
            xs = {c: H.ggml_view_2d(ctx, xxx, E, N_TOK, xxx.contents.nb[1], k * E * N_TOK * 4) for k, c in enumerate("rwkvag")}
            rr = mm("receptance", xs["r"])
            w = add(mm("w2", u(mm("w1", xs["w"]), TANH)), t["w0"])
            w = u(H.ggml_scale(ctx, u(w, SIGMOID), -0.606531), EXP)
            k, v = mm("key", xs["k"]), mm("value", xs["v"])
            v = add(v, mul(sub(r["v_first"], v), u(add(mm("v2", mm("v1", xs["v"])), t["v0"]), SIGMOID)))
            gate = mm("g2", u(mm("g1", xs["g"]), SIGMOID))
            a = u(add(mm("a2", mm("a1", xs["a"])), t["a0"]), SIGMOID)
            kk = H.ggml_l2_norm(ctx, heads(mul(k, t["k_k"])), 1e-12)
            ka = mul(k, t["k_a"])
            k = add(k, sub(mul(a, ka), ka))
            rec = H.ggml_rwkv_wkv7(ctx, heads(rr), heads(w), heads(k), heads(v), u(kk, NEG), mul(kk, heads(a)), state)
        r["rec"] = rec
        y = H.ggml_view_1d(ctx, rec, E * N_TOK, 0)
        n_st = HS * HS * N_HEAD * N_S
        H.ggml_build_forward_expand(gf, H.ggml_cpy(ctx, H.ggml_view_1d(ctx, rec, n_st, E * N_TOK * 4), H.ggml_view_1d(ctx, r["state_all"], n_st, 0)))
        if self.arch != 62:
            y = H.ggml_norm(ctx, H.ggml_reshape_3d(ctx, y, HS, N_HEAD, N_TOK), NORM_EPS)
            y = add(mul(flat(y), t["ln_w"]), t["ln_b"])
        else:
            y = flat(y)
        if self.arch == 7:
            rk = H.ggml_sum_rows(ctx, mul(mul(heads(k), heads(rr)), t["r_k"]))  # [1, H, n_tok]
            y = add(y, flat(mul(heads(v), rk)))
        att = mm("output", mul(y, gate))
        if self.arch == 62:
            out = att
            ffn_in3 = x3
        else:
            ffn_in = add(att, cur)
            ffn_in3 = H.ggml_reshape_3d(ctx, ffn_in, E, N_T, N_S)
            sx = flat(sub(prev_of(ffn_in3, 1), ffn_in3))
            kx = u(mm("cm_key", add(mul(sx, t["cm_lerp_k"]), ffn_in)), RELU)
            ffn = mm("cm_value", H.ggml_sqr(ctx, kx))
            if self.arch == 6:
                ffn = mul(u(mm("cm_receptance", add(mul(sx, t["cm_lerp_r"]), ffn_in)), SIGMOID), ffn)
            out = add(ffn, ffn_in)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        # the new token shifts: the last token of each sequence, of the layer input and of the channel mix's input
        last = lambda a3: H.ggml_view_3d(ctx, a3, E, 1, N_S, a3.contents.nb[1], a3.contents.nb[2], (N_T - 1) * a3.contents.nb[1])
        new_shift = H.ggml_concat(ctx, last(x3), last(ffn_in3), 1)  # [n_embd, 2, n_seqs]
        H.ggml_build_forward_expand(gf, H.ggml_cpy(ctx, new_shift, H.ggml_view_1d(ctx, r["shift_all"], 2 * E * N_S, 0)))
        r["out"] = out
        return r

    # -------------------------------------------------------------------------------------------- twins
    def rec_inputs(self, srcs):
        """The rwkv_ref input dict of the recurrent node from its sources in op order (arrays as read back: ggml dimensions reversed)."""
        names = R.N_SRC[self.op]
        inp = {}
        for n, a in zip(names, srcs):
            a = np.asarray(a, dtype=np.float32)
            inp[n] = a.reshape(N_S, N_HEAD, HS, HS) if n == "state" else a.reshape(N_HEAD, HS) if n == "tf" else a.reshape(N_TOK, N_HEAD, HS)
        if self.op == "gla":
            inp["scale"] = np.float32(float(HS) ** -0.5)
        return inp

    def twin(self, f, x, v_first, shift, state):
        """One step in dtype f (float64: exact activations; float32: ggml's arithmetic, see Weights.mm) on caches updated in place: x (N_S, N_T, E) -> out."""
        W, E = self.W, N_EMBD
        p = lambda n: W.f32[n].astype(f)
        mm = lambda n, a: W.mm(n, a, f)
        x = x.astype(f)

        def prev_of(cur, slot):
            return np.concatenate([shift[:, slot:slot + 1, :], cur[:, :-1, :]], axis=1)

        sx = prev_of(x, 0) - x
        if self.arch in (6, 62):
            xxx = sx * p("lerp_x") + x
            lo = np.tanh(mm("w1", xxx)).reshape(N_S, N_T, 5, LORA)
            w2 = p("w2").reshape(5, E, LORA)
            xs = {c: ((lo[:, :, k, :] @ w2[k].T) + p("lerp_" + c)) * sx + x for k, c in enumerate("wkvrg")}
            rr, k, v = mm("receptance", xs["r"]), mm("key", xs["k"]), mm("value", xs["v"])
            gg = mm("gate", xs["g"])
            gate = _sig(gg) if self.arch == 62 else gg * _sig(gg)
            w = mm("decay_w2", np.tanh(mm("decay_w1", xs["w"]))) + p("decay")
            w = np.exp(-np.exp(w))
            hd = lambda a: a.reshape(N_TOK, N_HEAD, HS)
            if self.arch == 62:
                k = k - k * w
                inp = {"k": hd(k), "v": hd(v), "q": hd(rr), "g": hd(w), "state": state, "scale": np.float32(float(HS) ** -0.5)}
            else:
                inp = {"k": hd(k), "v": hd(v), "r": hd(rr), "tf": p("first").reshape(N_HEAD, HS), "td": hd(w), "state": state}
        else:
            lf = p("lerp_fused").reshape(6, E)
            xs = {c: sx * lf[k] + x for k, c in enumerate("rwkvag")}
            rr = mm("receptance", xs["r"])
            w = mm("w2", np.tanh(mm("w1", xs["w"]))) + p("w0")
            w = np.exp(_sig(w) * f(np.float32(-0.606531)))
            k, v = mm("key", xs["k"]), mm("value", xs["v"])
            v = v + (v_first.astype(f).reshape(v.shape) - v) * _sig(mm("v2", mm("v1", xs["v"])) + p("v0"))
            gate = mm("g2", _sig(mm("g1", xs["g"])))
            a = _sig(mm("a2", mm("a1", xs["a"])) + p("a0"))
            hd = lambda z: z.reshape(N_TOK, N_HEAD, HS)
            kk = hd(k * p("k_k"))
            kk = kk / np.maximum(np.sqrt((kk * kk).sum(-1, keepdims=True)), f(1e-12))
            ka = k * p("k_a")
            k = k + (a * ka - ka)
            inp = {"r": hd(rr), "w": hd(w), "k": hd(k), "v": hd(v), "a": -kk, "b": kk * hd(a), "state": state}
        if f == np.float64:
            ref = R.twin64(self.op, inp)
            y, st = ref["y"], ref["st"]
        else:
            assert all(np.asarray(z).dtype == np.float32 for z in inp.values()), {n: np.asarray(z).dtype for n, z in inp.items()}
            y, st = R.twin32(self.op, inp)
        state[:] = st
        y = y.reshape(N_S, N_T, E)
        if self.arch != 62:
            y = _head_norm(y, p("ln_w"), p("ln_b"), f)
        if self.arch == 7:
            rk = ((hd(k) * hd(rr)) * p("r_k").reshape(N_HEAD, HS)).sum(-1, keepdims=True)
            y = y + (hd(v) * rk).reshape(y.shape)
        att = mm("output", y * gate)
        if self.arch == 62:
            out, ffn_in = att, x
        else:
            ffn_in = att + x
            sx = prev_of(ffn_in, 1) - ffn_in
            kx = np.maximum(mm("cm_key", sx * p("cm_lerp_k") + ffn_in), 0)
            ffn = mm("cm_value", kx * kx)
            if self.arch == 6:
                ffn = _sig(mm("cm_receptance", sx * p("cm_lerp_r") + ffn_in)) * ffn
            out = ffn + ffn_in
        shift[:, 0, :], shift[:, 1, :] = x[:, -1, :], ffn_in[:, -1, :]
        assert out.dtype == f
        return out


def _layer_steps(arch):
    rng = np.random.default_rng(70 + arch)
    return [(rng.standard_normal((N_S, N_T, N_EMBD)).astype(np.float32), rng.standard_normal((N_TOK, N_EMBD)).astype(np.float32)) for _ in range(3)]


def _run_layer(backend, lay, read_rec):
    """Three consecutive steps of the ONE graph on the same buffers: per step (out, shift cache, state cache[, the recurrent node's sources and result])."""
    H = L.host()
    g = T.G(backend)
    try:
        r = lay.graph(g)
        gf = r["gf"]
        for i in range(gf.contents.n_nodes):
            node = gf.contents.nodes[i]
            assert H.ggml_backend_dev_supports_op(backend.dev, node), (i, H.ggml_op_name(node.contents.op), node.contents.name)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        ids = np.arange(N_S, dtype=np.int32)
        res = []
        s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures", "eager_graphs")}
        for x, v_first in _layer_steps(lay.arch):
            sets = [(r["x"], x), (r["ids"], ids)] + ([(r["v_first"], v_first)] if "v_first" in r else [])
            for tt, raw in sets:
                raw = np.ascontiguousarray(raw)
                H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            step = [g.read(r["out"]).copy(), g.read(r["shift_all"]).copy(), g.read(r["state_all"]).copy()]
            if read_rec:
                rec = r["rec"].contents
                step.append([g.read(rec.src[i]).copy() for i in range(len(R.N_SRC[lay.op]))])
                step.append(g.read(r["rec"]).copy())
            res.append(step)
        return res, {k: backend.stat(k) - v for k, v in s0.items()}
    finally:
        g.free()


@pytest.mark.parametrize("arch", [6, 7, 62])
def test_layer_three_steps_against_the_twins(backend, plog, arch):
    """Every node accepted; the recurrent node inside its op gate on the inputs the GPU itself fed it; the layer output against the float64 twin at four times
    the f32 twin's own error against float64 on the same inputs (the base is computed here from the two twins, never from the GPU's result)."""
    lay = Layer(arch, 600 + arch)
    try:
        backend.set_option("graphs", 0)
        res, _ = _run_layer(backend, lay, True)
    finally:
        backend.set_option("graphs", 1)
    c64 = (lay.shift0.astype(np.float64), lay.state0.astype(np.float64))
    c32 = (lay.shift0.copy(), lay.state0.copy())
    for k, ((x, v_first), (out, shift_g, state_g, srcs, rec)) in enumerate(zip(_layer_steps(arch), res)):
        inp = lay.rec_inputs(srcs)
        ey, es = R.excess(R.twin64(lay.op, inp), *R.split(rec, inp))
        want = lay.twin(np.float64, x, v_first, *c64)
        near = lay.twin(np.float32, x, v_first, *c32)
        base = float(np.max(np.abs(near.astype(np.float64) - want)))
        err = float(np.max(np.abs(out.reshape(want.shape).astype(np.float64) - want)))
        plog(f"  rwkv layer arch {arch} step {k}: {lay.op} node y {ey:.3f}, states {es:.3f} of its gate; output max error {err:.3e}, f32 twin's {base:.3e} "
             f"(x 4 = the bound), output max {float(np.max(np.abs(want))):.3e}")
        assert ey <= 1.0 and es <= 1.0, (arch, k, ey, es)
        assert base > 0.0 and err <= 4.0 * base, (arch, k, err, base)
        # the caches carry: the step's token shifts and states are the float64 twin's, each to four times the f32 twin's own error in that cache
        for got, ref, near_c in ((shift_g, c64[0], c32[0]), (state_g, c64[1], c32[1])):
            assert float(np.max(np.abs(got.reshape(ref.shape).astype(np.float64) - ref))) <= 4.0 * float(np.max(np.abs(near_c.astype(np.float64) - ref))), (arch, k)


@pytest.mark.parametrize("arch", [6, 7, 62])
def test_layer_step_is_captured_and_replays_bit_equal(backend, plog, arch):
    """The step's graph computed three times on persistent buffers: the second sighting captures it, the third replays it (graph_launches 2, one capture), bit-equal
    at every step to a backend with graphs off."""
    lay = Layer(arch, 600 + arch)
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            runs[mode] = _run_layer(backend, lay, False)
    finally:
        backend.set_option("graphs", 1)
    plog(f"  rwkv layer arch {arch} capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["graph_captures"] == 0, runs[0][1]
    for a, b in zip(runs[1][0], runs[0][0]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
    states = [r[2] for r in runs[0][0]]
    assert not np.array_equal(states[1], states[0]) and not np.array_equal(states[2], states[1])
