"""GPU: csrc/diffusion.hip through the C-ABI — GROUP_NORM in both of its forms against the float64 twin at NORM's gate, group by group, its fusion with the MUL, ADD
and SILU nodes behind it, DIAG_MASK_INF and LEAKY_RELU bit for bit against their f32 twins, TIMESTEP_EMBEDDING against the float64 twin at the absolute gate
tests/diffusion_ref.py derives, then a UNet block and a CLIP layer over persistent buffers, eager and as a replayed hipGraph, every node checked against its twin
on the GPU's own read-back input (the CPU oracle has none of the four ops).

Every value test here fails on a backend without these ops: harness.G.compute raises supports_op=false at the first new node; the acceptance test fails outright.
"""
import ctypes as C

import numpy as np
import pytest

import act_norm_ref as A
import conv_ref as CR
import diffusion_ref as R
import harness as T
import llama_box_amd as L
import ops_ref as O

pytestmark = pytest.mark.gpu
F32, F16 = L.F32, L.F16
f16, f32, f64 = np.float16, np.float32, np.float64
CHUNK, RES_MAX = R.GN_CHUNK, R.GN_RESIDENT_MAX


def _assert_bits(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(O.bits(got).ravel() != O.bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


def _run(backend, build):
    """build(g) -> the tensors to read after one compute of all of them."""
    g = T.G(backend)
    try:
        outs = build(g)
        g.compute(list(outs))
        return [g.read(t) for t in outs]
    finally:
        g.free()


def _counted(backend, build, fusion=1):
    """(arrays of the reads, kernel launches, fused nodes) of one graph."""
    backend.set_option("fusion", fusion)
    try:
        k0, f0 = backend.stat("kernel_launches"), backend.stat("fused_nodes")
        got = _run(backend, build)
        return got, backend.stat("kernel_launches") - k0, backend.stat("fused_nodes") - f0
    finally:
        backend.set_option("fusion", 1)


@pytest.fixture
def gn_form(backend):
    def set_form(v):
        backend.set_option("gn_form", v)
    yield set_form
    backend.set_option("gn_form", 0)


def _gn_launches(form, n_full):
    """Launches of one GROUP_NORM node whose full group holds n_full values: 1 resident, 3 split."""
    routed_max = R.source_constants()["MI_GN_ROUTED_MAX"]
    resident = form != 2 and n_full <= RES_MAX and (form == 1 or n_full <= routed_max)
    return 1 if resident else 3


# ------------------------------------------------------------------------------------------------ 1. acceptance, 2. refusals
def test_supports_op_accepts_the_image_generation_ops(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        # SD shapes: a UNet ResBlock at 64 x 64 x 320, the VAE decoder at 512 x 512 x 128, the UNet's timestep head, CLIP's causal mask
        for ne, G in (([64, 64, 320, 1], 32), ([512, 512, 128, 1], 32), ([8, 8, 1280, 2], 32)):
            x = H.ggml_new_tensor_4d(ctx, F32, *ne)
            assert ok(H.ggml_group_norm(ctx, x, G, 1e-6)) and ok(H.ggml_group_norm_inplace(ctx, x, G, 1e-6)), ne
        assert ok(H.ggml_timestep_embedding(ctx, H.ggml_new_tensor_1d(ctx, F32, 1), 320, 10000))
        kq = H.ggml_new_tensor_3d(ctx, F32, 77, 77, 12)
        assert ok(H.ggml_diag_mask_inf(ctx, kq, 0)) and ok(H.ggml_diag_mask_inf_inplace(ctx, kq, 0))
        assert ok(H.ggml_leaky_relu(ctx, H.ggml_new_tensor_4d(ctx, F32, 128, 128, 64, 1), 0.2, True))
        # tiny ones
        for ne, G in (([5, 3, 8, 2], 4), ([4, 4, 7, 1], 4), ([1, 1, 4, 1], 4), ([3, 2, 6, 1], 1), ([1, 1, 1, 1], 1)):
            assert ok(H.ggml_group_norm(ctx, H.ggml_new_tensor_4d(ctx, F32, *ne), G, 0.0)), ne
        for dim in (2, 3, 5):
            assert ok(H.ggml_timestep_embedding(ctx, H.ggml_new_tensor_1d(ctx, F32, 3), dim, 1)), dim
        small = H.ggml_new_tensor_3d(ctx, F32, 7, 5, 3)
        assert ok(H.ggml_diag_mask_inf(ctx, small, 9)) and ok(H.ggml_diag_mask_inf(ctx, H.ggml_new_tensor_1d(ctx, F32, 1), 0))
        wide = H.ggml_new_tensor_3d(ctx, F32, 9, 6, 3)
        view = H.ggml_view_3d(ctx, wide, 7, 5, 3, 9 * 4, 9 * 6 * 4, 4)
        assert ok(H.ggml_diag_mask_inf(ctx, view, 0)) and ok(H.ggml_diag_mask_inf_inplace(ctx, view, 0))
        assert ok(H.ggml_leaky_relu(ctx, small, -0.5, False)) and ok(H.ggml_leaky_relu(ctx, small, 0.0, True))
    finally:
        g.free()


def test_supports_op_refuses_what_is_outside_the_contract(backend, H):
    g = T.G(backend)
    ctx = g.ctx
    try:
        def ok(node):
            return bool(H.ggml_backend_dev_supports_op(backend.dev, node))

        x = H.ggml_new_tensor_4d(ctx, F32, 6, 5, 8, 2)
        assert ok(H.ggml_group_norm(ctx, x, 4, 1e-6))
        assert not ok(H.ggml_group_norm(ctx, H.ggml_new_tensor_4d(ctx, F32, 6, 5, 5, 1), 4, 1e-6))  # C = 5, G = 4: cpg 2, the fourth group is empty
        assert not ok(H.ggml_group_norm(ctx, H.ggml_new_tensor_4d(ctx, F32, 6, 5, 9, 1), 4, 1e-6))  # C = 9, G = 4: cpg 3, the fourth group is empty
        assert not ok(H.ggml_group_norm(ctx, H.ggml_new_tensor_4d(ctx, F16, 6, 5, 8, 2), 4, 1e-6))
        assert not ok(H.ggml_group_norm(ctx, H.ggml_permute(ctx, x, 1, 0, 2, 3), 4, 1e-6))          # a non-contiguous source
        assert not ok(H.ggml_group_norm_inplace(ctx, H.ggml_permute(ctx, x, 1, 0, 2, 3), 4, 1e-6))
        for G in (0, -1, 9):
            assert not ok(H.ggml_group_norm(ctx, x, G, 1e-6)), G
        node = H.ggml_group_norm(ctx, x, 4, 1e-6)
        node.contents.ne[0] -= 1  # a result of another shape
        assert not ok(node)
        # DIAG_MASK_ZERO; a negative n_past; f16; rows that are not contiguous
        kq = H.ggml_new_tensor_3d(ctx, F32, 7, 5, 3)
        node = H.ggml_diag_mask_inf(ctx, kq, 0)
        assert ok(node)
        node.contents.op = R.OP_DIAG_MASK_ZERO
        assert not ok(node)
        assert not ok(H.ggml_diag_mask_inf(ctx, kq, -1))
        assert not ok(H.ggml_diag_mask_inf(ctx, H.ggml_new_tensor_3d(ctx, F16, 7, 5, 3), 0))
        assert not ok(H.ggml_diag_mask_inf_inplace(ctx, H.ggml_transpose(ctx, kq), 0))
        # TIMESTEP_EMBEDDING: dim < 2, max_period < 1, f16 timesteps, a 2-D timestep tensor
        t = H.ggml_new_tensor_1d(ctx, F32, 3)
        assert ok(H.ggml_timestep_embedding(ctx, t, 2, 10000))
        for dim in (1, 0, -2):
            assert not ok(H.ggml_timestep_embedding(ctx, t, dim, 10000)), dim
        assert not ok(H.ggml_timestep_embedding(ctx, t, 8, 0))
        assert not ok(H.ggml_timestep_embedding(ctx, H.ggml_new_tensor_1d(ctx, F16, 3), 8, 10000))
        assert not ok(H.ggml_timestep_embedding(ctx, H.ggml_new_tensor_2d(ctx, F32, 3, 2), 8, 10000))
        # LEAKY_RELU: f16, a non-contiguous source
        assert not ok(H.ggml_leaky_relu(ctx, H.ggml_new_tensor_1d(ctx, F16, 8), 0.2, False))
        assert not ok(H.ggml_leaky_relu(ctx, H.ggml_transpose(ctx, kq), 0.2, False))
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ 3. GROUP_NORM against the twin
def _gn_cases():
    """(id, x [N, C, H, W], G, eps, in place)"""
    rng = np.random.default_rng(4100)

    def rnd(*shape):
        return (rng.standard_normal(shape) * 3 + 0.75).astype(f32)

    out = [("30-values-unaligned-two-batches", rnd(2, 8, 3, 5), 4, 1e-6, False),   # [5, 3, 8, 2] / 4: groups of 30 values, most of them off 16 bytes
           ("shorter-last-group", rnd(1, 7, 4, 4), 4, 1e-6, False),                # [4, 4, 7, 1] / 4: 32, 32, 32, 16 values
           ("one-group", rnd(2, 6, 2, 3), 1, 1e-5, False),
           ("a-group-a-channel", rnd(2, 4, 5, 5), 4, 1e-6, False),
           ("groups-of-one-value", rnd(1, 4, 1, 1), 4, 1e-6, False),               # [1, 1, 4, 1] / 4: 0
           ("groups-of-one-value-eps0", rnd(1, 4, 1, 1), 4, 0.0, False),           # ... 0 * inf = NaN
           ("in-place", rnd(2, 8, 3, 5), 4, 1e-6, True)]
    const = rnd(1, 4, 3, 3)
    const[0, 0:2] = 2.5  # the first group is constant: 0, and NaN without eps
    out += [("constant-group", const, 2, 1e-6, False), ("constant-group-eps0", const, 2, 0.0, False)]
    out.append(("mean-1000x-spread", (rng.standard_normal((1, 4, 6, 6)) + 1000.0).astype(f32), 2, 1e-6, False))
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):  # two groups, two batch entries; only the first start is 16-byte aligned when n is odd
        out.append((f"group-of-{n}", rnd(2, 2, 1, n), 2, 1e-6, False))
    out.append(("in-place-three-chunks", rnd(1, 4, 50, 61), 2, 1e-6, True))          # groups of 6100 values, W H = 3050
    return out


@pytest.fixture(scope="module")
def gn_cases():
    return _gn_cases()


@pytest.mark.parametrize("form", [1, 2])
def test_group_norm_within_the_gate(backend, H, plog, gn_form, gn_cases, form):
    def build(g):
        outs = []
        for _, x, G, eps, inplace in gn_cases:
            t = g.new(F32, list(x.shape[::-1]), x)
            outs.append((H.ggml_group_norm_inplace if inplace else H.ggml_group_norm)(g.ctx, t, G, eps))
        return outs

    gn_form(form)
    got, launches, fused = _counted(backend, build)
    want_launches = sum(_gn_launches(form, x.shape[2] * x.shape[3] * -(-x.shape[1] // G)) for _, x, G, _, _ in gn_cases)
    assert launches == want_launches == len(gn_cases) * (1 if form == 1 else 3) and fused == 0, (launches, want_launches, fused)
    for (cid, x, G, eps, _), r in zip(gn_cases, got):
        assert r.shape == x.shape and r.dtype == f32, cid
        want = R.group_norm(x, G, eps)
        assert np.array_equal(np.isnan(r), np.isnan(want)), cid
        frac, d, gate = R.group_norm_excess(r, x, G, eps)
        plog(f"  group_norm form {form} {cid} {list(x.shape[::-1])} / {G}: worst group {d:.4g} of its maximum from the twin, {frac:.3f} of its gate {gate:.4g}")
        assert frac <= 1.0, f"{cid}: a group is {d:.6g} of its maximum from the twin, its gate is {gate:.6g}"
        if "one-value" in cid or "constant" in cid:
            flat = r.reshape(-1) if "one-value" in cid else r[0, 0:2].reshape(-1)
            assert np.all(np.isnan(flat)) if eps == 0.0 else np.all(flat == 0), cid


@pytest.mark.parametrize("form", [0, 1])
def test_group_norm_at_the_resident_bound(backend, H, plog, gn_form, form):
    """A group of MI_GN_RESIDENT_MAX values is the last the resident form holds; one value more takes the split form under gn_form 1 and, routed, under 0."""
    rng = np.random.default_rng(4200)
    gn_form(form)
    for n in (RES_MAX, RES_MAX + 1):
        x = (rng.standard_normal((1, 2, 1, n)) * 2 - 0.5).astype(f32)
        (r,), launches, _ = _counted(backend, lambda g: [H.ggml_group_norm(g.ctx, g.new(F32, [n, 1, 2, 1], x), 2, 1e-6)])
        assert launches == _gn_launches(form, n) and (launches == 3 if n > RES_MAX else form == 0 or launches == 1), (form, n, launches)
        frac, d, gate = R.group_norm_excess(r, x, 2, 1e-6)
        plog(f"  group_norm form {form} group of {n}: {launches} launch(es), {frac:.3f} of the gate {gate:.4g}")
        assert frac <= 1.0, (form, n, d, gate)


@pytest.mark.parametrize("form", [1, 2])
def test_group_norm_is_deterministic(backend, H, gn_form, form):
    x = (np.random.default_rng(4300).standard_normal((2, 4, 50, 50)) * 5).astype(f32)  # groups of 5000 values: two chunks in the split form

    def build(g):
        return [H.ggml_group_norm(g.ctx, g.new(F32, [50, 50, 4, 2], x), 2, 1e-6) for _ in range(2)]

    gn_form(form)
    a, b = _run(backend, build), _run(backend, build)
    for r in (a[1], b[0], b[1]):
        _assert_bits(f"group_norm form {form}, a repeat", r, a[0])


# ------------------------------------------------------------------------------------------------ 4. fusion
FUSE_X = (1, 4, 41, 61)  # [61, 41, 4, 1] / 2: W H = 2501 (a vector crosses channels), groups of 5002 values (two chunks, the second cut short)


def _fuse_inputs():
    rng = np.random.default_rng(4400)
    return (rng.standard_normal(FUSE_X) * 2 + 0.3).astype(f32), rng.uniform(0.5, 1.5, FUSE_X[1]).astype(f32), rng.standard_normal(FUSE_X[1]).astype(f32)


def _fuse_chain(H, g, x, w, b, prefix, second_reader=None):
    C_ = x.shape[1]
    nodes = [H.ggml_group_norm(g.ctx, g.new(F32, list(x.shape[::-1]), x), 2, 1e-6)]
    if prefix >= 1:
        nodes.append(H.ggml_mul(g.ctx, nodes[-1], g.new(F32, [1, 1, C_, 1], w)))
    if prefix >= 2:
        nodes.append(H.ggml_add(g.ctx, nodes[-1], g.new(F32, [1, 1, C_, 1], b)))
    if prefix >= 3:
        nodes.append(H.ggml_silu(g.ctx, nodes[-1]))
    outs = [nodes[-1]]
    if second_reader is not None:
        outs.append(H.ggml_scale(g.ctx, nodes[second_reader], 2.0))
    return outs


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("prefix", [1, 2, 3])
def test_group_norm_affine_fusion(backend, H, plog, gn_form, prefix, form):
    x, w, b = _fuse_inputs()
    gn_form(form)
    base = _gn_launches(form, 2 * 41 * 61)
    assert base == (1 if form == 1 else 3)
    plain = _run(backend, lambda g: _fuse_chain(H, g, x, w, b, 0))[0]
    fused, k1, f1 = _counted(backend, lambda g: _fuse_chain(H, g, x, w, b, prefix), 1)
    unfused, k0, f0 = _counted(backend, lambda g: _fuse_chain(H, g, x, w, b, prefix), 0)
    plog(f"  group_norm affine form {form} prefix {prefix}: launches fused {k1} / unfused {k0}, fused nodes {f1} / {f0}")
    assert (k1, f1) == (base, prefix) and (k0, f0) == (base + prefix, 0), (k1, f1, k0, f0)
    _assert_bits("group_norm affine fused vs unfused", fused[0], unfused[0])
    want = R.channel_binary("mul", plain, w)
    want = R.channel_binary("add", want, b) if prefix >= 2 else want
    if prefix < 3:
        _assert_bits("group_norm affine vs the MUL / ADD of the kernel's own GROUP_NORM", fused[0], want)
    else:  # SILU's twin is float64: the gate of tests/test_gpu_ops.py's unary family
        gate = O.oracle_baseline("silu") + O.ALLOWANCE["silu"]
        d = float(np.max(O.ulp_distance(fused[0], O.unary("SILU", want))))
        plog(f"  group_norm affine form {form}: SILU of the kernel's own affine {d:.3g} ulp from the twin, gate {gate:.3g}")
        assert d <= gate, (d, gate)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("reader_of", [0, 1, 2])
def test_group_norm_chain_stops_at_a_second_reader(backend, H, gn_form, reader_of, form):
    """A second reader of the GROUP_NORM, of the MUL or of the ADD: the chain absorbs the nodes in front of it and no more."""
    x, w, b = _fuse_inputs()
    gn_form(form)
    base = _gn_launches(form, 2 * 41 * 61)
    (r, s), k, f = _counted(backend, lambda g: _fuse_chain(H, g, x, w, b, 3, second_reader=reader_of), 1)
    assert (k, f) == (base + (3 - reader_of) + 1, reader_of), (k, f)
    (r0, s0), _, _ = _counted(backend, lambda g: _fuse_chain(H, g, x, w, b, 3, second_reader=reader_of), 0)
    _assert_bits("second reader: the chain", r, r0)
    _assert_bits("second reader: the reader", s, s0)
    plain = _run(backend, lambda g: _fuse_chain(H, g, x, w, b, 0))[0]
    stages = [plain, R.channel_binary("mul", plain, w)]
    stages.append(R.channel_binary("add", stages[1], b))
    _assert_bits("second reader: the scale of the node it reads", s, O.scale(stages[reader_of], 2.0))


# ------------------------------------------------------------------------------------------------ 5. DIAG_MASK_INF
@pytest.mark.parametrize("n_past", [0, 2, 9])
def test_diag_mask_inf_bit_exact(backend, H, n_past):
    rng = np.random.default_rng(4500)
    x = rng.standard_normal((3, 5, 7)).astype(f32)       # [7, 5, 3]
    big = rng.standard_normal((3, 6, 9)).astype(f32)     # [9, 6, 3]: the view [7, 5, 3] one element in keeps rows of 9 and planes of 6 rows

    def build(g):
        t = g.new(F32, [7, 5, 3], x)
        t2 = g.new(F32, [7, 5, 3], x)
        b1, b2 = g.new(F32, [9, 6, 3], big), g.new(F32, [9, 6, 3], big)
        v1 = H.ggml_view_3d(g.ctx, b1, 7, 5, 3, 9 * 4, 9 * 6 * 4, 4)
        v2 = H.ggml_view_3d(g.ctx, b2, 7, 5, 3, 9 * 4, 9 * 6 * 4, 4)
        g.keep += [b1, b2, t2]
        outs = [H.ggml_diag_mask_inf(g.ctx, t, n_past), H.ggml_diag_mask_inf_inplace(g.ctx, t2, n_past), H.ggml_diag_mask_inf(g.ctx, v1, n_past),
                H.ggml_diag_mask_inf_inplace(g.ctx, v2, n_past)]
        g.roots = (t, t2, b1, b2)
        return outs

    g = T.G(backend)
    try:
        outs = build(g)
        g.compute(list(outs))
        out_of_place, in_place, from_view = g.read(outs[0]), g.read(outs[1]), g.read(outs[2])
        src, src_ip, root_oop, root_ip = (g.read(t) for t in g.roots)
    finally:
        g.free()
    want = R.diag_mask_inf(x, n_past)
    assert (n_past == 9) == np.array_equal(want, x)  # (9 masks nothing)
    _assert_bits("diag_mask_inf", out_of_place, want.reshape(out_of_place.shape))
    _assert_bits("diag_mask_inf: the source is left alone", src, x.reshape(src.shape))
    _assert_bits("diag_mask_inf in place", in_place, want.reshape(in_place.shape))
    _assert_bits("diag_mask_inf in place: the source holds the result", src_ip, want.reshape(src_ip.shape))
    vwant = R.diag_mask_inf(big[:, :5, 1:8], n_past)
    _assert_bits("diag_mask_inf of a strided view", from_view, vwant.reshape(from_view.shape))
    _assert_bits("diag_mask_inf of a strided view: the root is left alone", root_oop, big.reshape(root_oop.shape))
    bwant = big.copy()
    bwant[:, :5, 1:8] = vwant
    _assert_bits("diag_mask_inf in place on a strided view: the masked cells and nothing else", root_ip, bwant.reshape(root_ip.shape))


# ------------------------------------------------------------------------------------------------ 6. LEAKY_RELU
@pytest.mark.parametrize("slope", [0.2, 0.0, -0.5])
def test_leaky_relu_bit_exact(backend, H, slope):
    rng = np.random.default_rng(4600)
    sub = f32(2.0 ** -149)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 5 * sub, -5 * sub, f32(1e-39), f32(-1e-39)], f32)
    x = np.concatenate([edge, O.catalogue(), O.seeded(rng, 2048 * 256 + 257 - len(edge) - len(O.catalogue()))]).astype(f32)  # a second, partial stride; no multiple of 4
    small = np.concatenate([edge, O.seeded(rng, 1027 - len(edge))]).astype(f32)
    assert x.size % 4 and small.size % 4

    def build(g):
        return [H.ggml_leaky_relu(g.ctx, g.new(F32, [x.size], x), slope, False), H.ggml_leaky_relu(g.ctx, g.new(F32, [x.size], x), slope, True),
                H.ggml_leaky_relu(g.ctx, g.new(F32, [13, 79], small), slope, False)]

    got = _run(backend, build)
    want = R.leaky_relu(x, slope)
    _assert_bits("leaky_relu", got[0].reshape(-1), want)
    _assert_bits("leaky_relu in place", got[1].reshape(-1), want)
    _assert_bits("leaky_relu 2-D", got[2].reshape(-1), R.leaky_relu(small, slope))


# ------------------------------------------------------------------------------------------------ 7. TIMESTEP_EMBEDDING
@pytest.mark.parametrize("dim", [2, 5, 320])
def test_timestep_embedding_within_the_gate(backend, H, plog, dim):
    steps = [np.array([999.0], f32), np.array([0.0, 0.5, 1.0], f32), np.array([1.0, 999.0, 0.5], f32)]
    got = _run(backend, lambda g: [H.ggml_timestep_embedding(g.ctx, g.new(F32, [len(t)], t), dim, 10000) for t in steps])
    for t, r in zip(steps, got):
        assert r.reshape(len(t), -1).shape == (len(t), dim + (dim & 1))
        e = R.timestep_excess(r, t, dim, 10000)
        plog(f"  timestep_embedding dim {dim} t {t.tolist()}: worst {float(np.max(e)):.3f} of the gate ({R.TE_ABS:.3g} + {R.te_rel(10000):.3g} |arg|)")
        assert np.max(e) <= 1.0, (dim, t, float(np.max(e)))
        if dim & 1:
            assert np.all(r.reshape(len(t), -1)[:, dim - 1:] == 0)
    assert np.array_equal(got[1].reshape(3, -1)[2], got[2].reshape(3, -1)[0])  # t = 1 in either batch


# ------------------------------------------------------------------------------------------------ 8. two chains over persistent buffers
def _logical(g, t):
    """The tensor as an array [ne3, ne2, ne1, ne0] whatever its strides: the bytes it spans, read back and walked with its nb[]."""
    H, tt = g.H, t.contents
    n = H.ggml_nbytes(t)
    raw = np.empty(n, np.uint8)
    H.ggml_backend_tensor_get(t, raw.ctypes.data_as(C.c_void_p), 0, n)
    dt = {F32: f32, F16: f16}[tt.type]
    return np.lib.stride_tricks.as_strided(raw.view(dt), shape=tuple(tt.ne[i] for i in (3, 2, 1, 0)), strides=tuple(tt.nb[i] for i in (3, 2, 1, 0))).copy()


def _op_f32(node, i):
    return float(np.int32(node.op_params[i]).view(f32))


def _check_nodes(g, gf, plog, tag):
    """Every node of the graph that ran unfused against its twin on the GPU's own read-back sources, at that op's gate: the new ops at theirs (diffusion_ref), the others at
    the gate their own test file uses.  Returns the op names seen.  A cell that a later in-place DIAG_MASK_INF overwrote with -inf is left out of its producer's check."""
    H = g.H
    silu_gate = O.oracle_baseline("silu") + O.ALLOWANCE["silu"]
    softmax_gate = O.oracle_baseline("soft_max") + O.ALLOWANCE["soft_max"]
    worst, seen = {}, set()

    def note(name, v, gate):
        worst[name] = max(worst.get(name, 0.0), v / gate if gate else v)

    for i in range(gf.contents.n_nodes):
        t = gf.contents.nodes[i]
        n = t.contents
        name = H.ggml_op_name(n.op).decode()
        if name in ("NONE", "VIEW", "RESHAPE", "PERMUTE", "TRANSPOSE"):
            continue
        seen.add(name)
        out = _logical(g, t)
        a = _logical(g, n.src[0]) if n.src[0] else None
        b = _logical(g, n.src[1]) if n.src[1] else None
        keep = np.ones(out.shape, bool) if out.dtype != f32 else ~np.isneginf(out) | (name in ("DIAG_MASK_INF", "SOFT_MAX"))
        what = f"{tag} node {i} {name} '{n.name.decode()}'"
        if name == "GROUP_NORM":
            frac, d, gate = R.group_norm_excess(out, a, n.op_params[0], _op_f32(n, 1))
            assert frac <= 1.0, (what, d, gate)
            note(name, frac, 1.0)
        elif name == "TIMESTEP_EMBEDDING":
            e = float(np.max(R.timestep_excess(out, a.reshape(-1), n.op_params[0], n.op_params[1])))
            assert e <= 1.0, (what, e)
            note(name, e, 1.0)
        elif name == "DIAG_MASK_INF":
            _assert_bits(what, out, R.diag_mask_inf(a, n.op_params[0]))
            assert np.all(np.isfinite(out[~np.isneginf(R.diag_mask_inf(np.zeros(out.shape, f32), n.op_params[0]))]))
        elif name == "MUL_MAT":
            b64 = (b.astype(f16) if (a.dtype == f16 and b.dtype == f32) else b).astype(f64)  # (an f16 src0 takes src1 rounded to f16: ggml-cpu's vec_dot_type)
            a64 = a.astype(f64)
            rep = (b64.shape[0] // a64.shape[0], b64.shape[1] // a64.shape[1], 1, 1)
            want = np.matmul(b64, np.swapaxes(np.tile(a64, rep), -1, -2))
            e = CR.nmse(out[keep], want[keep])
            assert out.shape == want.shape and e <= CR.MM_NMSE_GATE, (what, e)
            note(name, e, CR.MM_NMSE_GATE)
        elif name in ("ADD", "MUL"):
            _assert_bits(what, out[keep], O.binary(name.lower(), a, b)[keep])
        elif name == "SCALE":
            _assert_bits(what, out[keep], O.scale(a, _op_f32(n, 0), _op_f32(n, 1))[keep])
        elif name == "CONT":
            _assert_bits(what, out, a.reshape(out.shape))
        elif name == "IM2COL":
            q = n.op_params
            kn = n.src[0].contents
            want = CR.im2col(b, kn.ne[1], kn.ne[0], q[0], q[1], q[2], q[3], q[4], q[5], out.dtype.type)
            assert q[6] == 1
            _assert_bits(what, out, want.reshape(out.shape))
        elif name == "NORM":
            d = float(np.max(O.row_distance(out, A.norm(a, _op_f32(n, 0)))))
            gate = A.NORM_GATE + A.norm_extra(a)
            assert d <= gate, (what, d, gate)
            note(name, d, gate)
        elif name == "SOFT_MAX":
            assert not n.src[1]
            d = float(np.max(O.row_distance(out, O.soft_max(a, None, _op_f32(n, 0), 0.0))))
            assert d <= softmax_gate, (what, d, softmax_gate)
            note(name, d, softmax_gate)
        elif name == "UNARY":
            if n.op_params[0] == O.UNARY["SILU"]:
                d = float(np.max(O.ulp_distance(out, O.unary("SILU", a))))
                assert d <= silu_gate, (what, d, silu_gate)
                note("SILU", d, silu_gate)
            else:
                assert n.op_params[0] == A.UNARY["GELU_QUICK"], what
                _assert_bits(what, out, A.gelu_quick(a))
        else:
            raise AssertionError(f"{what}: no twin for this op in the chain test")
    plog(f"  {tag}: worst fraction of its gate per op " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    return seen


class UNetBlock:
    """[8, 8, 16, 1]: timestep embedding (32) -> linear -> SILU -> linear; GROUP_NORM / 4 * w + b -> SILU -> conv 3 x 3 (f16 kernel, pad 1) + bias -> + temb [1, 1, C] ->
    GROUP_NORM -> SILU -> conv 3 x 3 -> + skip; then GROUP_NORM -> 1 x 1 conv -> tokens -> NORM -> two-head attention (MUL_MAT, SCALE, SOFT_MAX, MUL_MAT) -> back, + the
    residual."""
    NEW = {"GROUP_NORM", "TIMESTEP_EMBEDDING"}
    OLD = {"MUL_MAT", "ADD", "MUL", "UNARY", "IM2COL", "CONT", "NORM", "SCALE", "SOFT_MAX"}

    def __init__(self):
        rng = np.random.default_rng(90)
        self.w1, self.b1 = (rng.standard_normal((64, 32)) / 5).astype(f32), rng.standard_normal(64).astype(f32)
        self.w2, self.b2 = (rng.standard_normal((16, 64)) / 8).astype(f32), rng.standard_normal(16).astype(f32)
        self.gw, self.gb = rng.uniform(0.5, 1.5, 16).astype(f32), rng.standard_normal(16).astype(f32)
        self.k1 = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(f16)
        self.k2 = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(f16)
        self.kb = rng.standard_normal(16).astype(f32)
        self.k3 = (rng.standard_normal((16, 16, 1, 1)) / 4).astype(f16)
        self.steps = [(rng.standard_normal((1, 16, 8, 8)).astype(f32), np.array([t], f32)) for t in (999.0, 500.0, 1.0)]

    def graph(self, g):
        H, ctx = g.H, g.ctx
        x, t = g.new(F32, [8, 8, 16, 1]), g.new(F32, [1])
        e = H.ggml_timestep_embedding(ctx, t, 32, 10000)                                              # [32, 1]
        e = H.ggml_silu(ctx, H.ggml_add(ctx, H.ggml_mul_mat(ctx, g.new(F32, [32, 64], self.w1), e), g.new(F32, [64], self.b1)))
        e = H.ggml_add(ctx, H.ggml_mul_mat(ctx, g.new(F32, [64, 16], self.w2), e), g.new(F32, [16], self.b2))  # [16, 1]
        h = H.ggml_add(ctx, H.ggml_mul(ctx, H.ggml_group_norm(ctx, x, 4, 1e-6), g.new(F32, [1, 1, 16, 1], self.gw)), g.new(F32, [1, 1, 16, 1], self.gb))
        h = H.ggml_conv_2d(ctx, g.new(F16, [3, 3, 16, 16], self.k1), H.ggml_silu(ctx, h), 1, 1, 1, 1, 1, 1)
        h = H.ggml_add(ctx, h, g.new(F32, [1, 1, 16, 1], self.kb))
        h = H.ggml_add(ctx, h, H.ggml_reshape_4d(ctx, e, 1, 1, 16, 1))
        h = H.ggml_conv_2d(ctx, g.new(F16, [3, 3, 16, 16], self.k2), H.ggml_silu(ctx, H.ggml_group_norm(ctx, h, 4, 1e-6)), 1, 1, 1, 1, 1, 1)
        h = H.ggml_add(ctx, h, x)
        a = H.ggml_conv_2d(ctx, g.new(F16, [1, 1, 16, 16], self.k3), H.ggml_group_norm(ctx, h, 4, 1e-6), 1, 1, 0, 0, 1, 1)  # [8, 8, 16, 1]
        tok = H.ggml_norm(ctx, H.ggml_cont(ctx, H.ggml_transpose(ctx, H.ggml_reshape_2d(ctx, a, 64, 16))), 1e-5)           # [16, 64]
        qk = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_reshape_3d(ctx, tok, 8, 2, 64), 0, 2, 1, 3))                       # [8, 64, 2]
        v = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_reshape_3d(ctx, tok, 8, 2, 64), 1, 2, 0, 3))                        # [64, 8, 2]
        kq = H.ggml_soft_max(ctx, H.ggml_scale(ctx, H.ggml_mul_mat(ctx, qk, qk), 8.0 ** -0.5))                               # [64, 64, 2]
        o = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_mul_mat(ctx, v, kq), 0, 2, 1, 3))                                   # [8, 64, 2] -> [8, 2, 64]
        o = H.ggml_cont(ctx, H.ggml_transpose(ctx, H.ggml_reshape_2d(ctx, o, 16, 64)))                                      # [64, 16]
        return (x, t), H.ggml_add(ctx, H.ggml_reshape_4d(ctx, o, 8, 8, 16, 1), h)


class ClipLayer:
    """7 tokens x 16 x 2 heads: NORM * w + b -> q, k, v (f16 weights, + bias) -> K.Q -> SCALE -> diag_mask_inf_inplace(kq, 0) -> SOFT_MAX -> .V -> projection, + the
    residual; NORM * w + b -> a GELU_QUICK MLP, + the residual."""
    NEW = {"DIAG_MASK_INF"}
    OLD = {"MUL_MAT", "ADD", "MUL", "UNARY", "CONT", "NORM", "SCALE", "SOFT_MAX"}

    def __init__(self):
        rng = np.random.default_rng(91)
        self.lin = {k: ((rng.standard_normal((o, i)) / np.sqrt(i)).astype(f16), (rng.standard_normal(o) / 4).astype(f32))
                    for k, (i, o) in {"q": (16, 16), "k": (16, 16), "v": (16, 16), "o": (16, 16), "fc1": (16, 32), "fc2": (32, 16)}.items()}
        self.ln = [(rng.uniform(0.5, 1.5, 16).astype(f32), rng.standard_normal(16).astype(f32)) for _ in range(2)]
        self.steps = [(rng.standard_normal((7, 16)).astype(f32),) for _ in range(3)]

    def graph(self, g):
        H, ctx = g.H, g.ctx

        def linear(name, v):
            w, b = self.lin[name]
            return H.ggml_add(ctx, H.ggml_mul_mat(ctx, g.new(F16, list(w.shape[::-1]), w), v), g.new(F32, [len(b)], b))

        def ln(k, v):
            w, b = self.ln[k]
            return H.ggml_add(ctx, H.ggml_mul(ctx, H.ggml_norm(ctx, v, 1e-5), g.new(F32, [16], w)), g.new(F32, [16], b))

        x = g.new(F32, [16, 7])
        h = ln(0, x)
        q = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_reshape_3d(ctx, linear("q", h), 8, 2, 7), 0, 2, 1, 3))   # [8, 7, 2]
        k = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_reshape_3d(ctx, linear("k", h), 8, 2, 7), 0, 2, 1, 3))   # [8, 7, 2]
        v = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_reshape_3d(ctx, linear("v", h), 8, 2, 7), 1, 2, 0, 3))   # [7, 8, 2]
        kq = H.ggml_scale(ctx, H.ggml_mul_mat(ctx, k, q), 8.0 ** -0.5)                                           # [7, 7, 2]
        kq = H.ggml_soft_max(ctx, H.ggml_diag_mask_inf_inplace(ctx, kq, 0))
        o = H.ggml_cont(ctx, H.ggml_permute(ctx, H.ggml_mul_mat(ctx, v, kq), 0, 2, 1, 3))                       # [8, 7, 2] -> [8, 2, 7]
        x1 = H.ggml_add(ctx, linear("o", H.ggml_reshape_2d(ctx, o, 16, 7)), x)
        m = linear("fc2", H.ggml_gelu_quick(ctx, linear("fc1", ln(1, x1))))
        return (x,), H.ggml_add(ctx, m, x1)


def _run_chain(backend, chain, plog=None, check=False):
    """Three steps of the ONE graph on the same buffers -> (per-step results, the counters' change, the ops seen by the node check)."""
    H = L.host()
    g = T.G(backend)
    try:
        ins, out = chain.graph(g)
        gf = H.ggml_new_graph_custom(g.ctx, 512, False)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        for i in range(gf.contents.n_nodes):  # no node may be refused: sd.cpp hands the whole graph to the one backend
            node = gf.contents.nodes[i]
            assert H.ggml_backend_dev_supports_op(backend.dev, node), (i, H.ggml_op_name(node.contents.op), node.contents.name)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures")}
        res, seen = [], set()
        for k, step in enumerate(chain.steps):
            for tt, arr in zip(ins, step):
                raw = np.ascontiguousarray(arr)
                H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append(g.read(out).copy())
            if check:
                seen |= _check_nodes(g, gf, plog, f"{type(chain).__name__} step {k}")
        return res, {k: backend.stat(k) - v for k, v in s0.items()}, seen
    finally:
        g.free()


@pytest.mark.parametrize("chain_cls", [UNetBlock, ClipLayer])
def test_chain_eager_and_replayed(backend, plog, chain_cls):
    """Every node accepted.  With fusion off every node is written: each is held to its own gate on its own read-back input.  With fusion on, the second sighting is
    captured and the third replayed (graph_launches 2, one capture), bit-equal at every step to a backend with graphs off, and within the mat-mul gate of the unfused
    run (the fusions are the unfused arithmetic; the gate only allows for a fused store the existing ops may round otherwise)."""
    chain = chain_cls()
    runs = {}
    try:
        for graphs, fusion in ((1, 1), (0, 1), (0, 0)):
            backend.set_option("graphs", graphs)
            backend.set_option("fusion", fusion)
            runs[(graphs, fusion)] = _run_chain(backend, chain, plog, check=(fusion == 0))
    finally:
        backend.set_option("graphs", 1)
        backend.set_option("fusion", 1)
    seen = runs[(0, 0)][2]
    assert chain.NEW <= seen and seen <= chain.NEW | chain.OLD, seen
    plog(f"  {chain_cls.__name__}: graphs=1 {runs[(1, 1)][1]}, graphs=0 {runs[(0, 1)][1]}, ops {sorted(seen)}")
    assert runs[(1, 1)][1] == {"graph_launches": 2, "graph_captures": 1}, runs[(1, 1)][1]
    assert runs[(0, 1)][1] == {"graph_launches": 0, "graph_captures": 0}, runs[(0, 1)][1]
    for k, (a, b, c) in enumerate(zip(runs[(1, 1)][0], runs[(0, 1)][0], runs[(0, 0)][0])):
        _assert_bits(f"{chain_cls.__name__} step {k}: replayed vs eager", a, b)
        e = CR.nmse(b, c)
        plog(f"  {chain_cls.__name__} step {k}: fused vs unfused nmse {e:.3e}, bit-equal {np.array_equal(O.bits(b), O.bits(c))}")
        assert e <= CR.MM_NMSE_GATE, (k, e)
    assert not np.array_equal(runs[(0, 0)][0][0], runs[(0, 0)][0][1])
