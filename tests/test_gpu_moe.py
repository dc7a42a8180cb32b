"""Mixture-of-experts FFN blocks on the MI355X: MUL_MAT_ID (csrc/mmid.hip), the router ops ARGSORT / SUM_ROWS / CLAMP, batched GET_ROWS, the 3-D split
SwiGLU, the whole build_moe_ffn sequence, its hipGraph capture, out-of-range ids, and a guard on the dense paths.  References: tests/moe_ref.py.
The edge cases — the kernel forms these model shapes never select, strided and offset operands, the exact read-back of the quantiser in front of MUL_MAT_ID and a layer
with a shared expert — live in tests/test_gpu_moe_edges.py."""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as M
from model_util import Context, Model, preset

pytestmark = pytest.mark.gpu

QUANT = (L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0)
TYPES = {"q4_K": L.Q4_K, "q5_K": L.Q5_K, "q6_K": L.Q6_K, "q8_0": L.Q8_0, "f16": L.F16}
# (K, N, n_expert, n_used, one activation row per slot)
SHAPES = {
    "mixtral-up": (4096, 14336, 8, 2, False),
    "mixtral-down": (14336, 4096, 8, 2, True),
    "qwen3-up": (2048, 768, 128, 8, False),
    "qwen3-down": (768, 2048, 128, 8, True),
}


def _routing(rng, n_tok, n_used, n_expert, one_expert):
    """ids [n_tok, n_used], distinct within a token.  The last two experts are selected by nobody; token 1 repeats token 0's list; with `one_expert`
    slot 0 of EVERY token is expert 1 (all tokens on one expert)."""
    pool = np.arange(n_expert - 2)
    ids = np.stack([rng.permutation(pool)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    if one_expert:
        for t in range(n_tok):
            rest = [e for e in ids[t] if e != 1][:n_used - 1]
            ids[t] = [1] + rest
    if n_tok >= 2:
        ids[1] = ids[0]
    return ids


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("tname", sorted(TYPES))
def test_mul_mat_id_matches_the_composite_reference_and_the_backends_own_mat_vec(backend, plog, tname, shape):
    """MUL_MAT_ID per expert type and model shape, n_tokens 1 .. 77 (512 for the Qwen3 shapes), ids as the strided top-k view and as a contiguous tensor.
    Gates: NMSE <= 1e-10 against the composite oracle reference (the quantised MUL_MAT gate of tests/test_gpu_ops.py); for n_used * n_tokens <= 32 and the
    mat-vec formats (Q4_K / Q5_K / Q6_K / Q8_0: the route the bit-equality is promised for — f16 experts run a plain f16 dot, not the mat-vec route)
    every (slot, token) column is bit-equal to the backend's own one-column MUL_MAT over that expert's 2-D view; one launch per node."""
    qtype = TYPES[tname]
    K, N, n_expert, n_used, per_slot = SHAPES[shape]
    rng = np.random.default_rng(1000 + 17 * qtype + len(shape))
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    toks = [1, 2, 4, 5, 32, 77] + ([512] if shape.startswith("qwen3") else [])
    cases = []
    for n_tok in toks:
        ids = _routing(rng, n_tok, n_used, n_expert, one_expert=n_tok in (4, 32, 512))
        b = rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32)
        cases.append((b, ids))
    assert not np.isin(np.concatenate([c[1].ravel() for c in cases]), [n_expert - 2, n_expert - 1]).any()
    ref = M.mmid_reference(qtype, W, K, N, cases)

    H = L.host()
    g = T.G(backend)
    try:
        as_t = g.new(qtype, [K, N, n_expert], W)
        outs, cols = [], []
        for b, ids in cases:
            n_tok, rows = b.shape[0], b.shape[1]
            bt = g.new(L.F32, [K, rows, n_tok], b)
            outs.append(H.ggml_mul_mat_id(g.ctx, as_t, bt, M.strided_ids(g, ids, n_expert)))
            outs.append(H.ggml_mul_mat_id(g.ctx, as_t, bt, g.new(L.I32, [n_used, n_tok], ids)))
            if qtype in QUANT and n_used * n_tok <= 32:
                for t in range(n_tok):
                    for s in range(n_used):
                        col = H.ggml_view_2d(g.ctx, bt, K, 1, K * 4, (t * rows + (s if rows > 1 else 0)) * K * 4)
                        cols.append(H.ggml_mul_mat(g.ctx, M.expert_view(g, as_t, K, N, ids[t, s]), col))
        m0 = backend.stat("mmid_launches")
        res = M.compute_in_weights_buffer(g, outs + cols)
        launches = backend.stat("mmid_launches") - m0
    finally:
        g.free()
    assert launches == len(outs), f"{launches} MUL_MAT_ID launches for {len(outs)} nodes"
    ci = 0
    for k, (b, ids) in enumerate(cases):
        n_tok = ids.shape[0]
        strided = res[2 * k].reshape(n_tok, n_used, N)
        contig = res[2 * k + 1].reshape(n_tok, n_used, N)
        T.compare(f"mul_mat_id {tname} {shape} n_tokens={n_tok} strided ids", strided, ref[k], 1e-10, log=plog)
        T.compare(f"mul_mat_id {tname} {shape} n_tokens={n_tok} contiguous ids", contig, ref[k], 1e-10, log=plog)
        assert np.array_equal(strided.view(np.uint32), contig.view(np.uint32))
        if qtype in QUANT and n_used * n_tok <= 32:
            for t in range(n_tok):
                for s in range(n_used):
                    own = res[len(outs) + ci].reshape(N)
                    ci += 1
                    assert np.array_equal(strided[t, s].view(np.uint32), own.view(np.uint32)), f"{tname} {shape} n_tokens={n_tok}: (slot {s}, token {t}) differs from MUL_MAT over the expert's view"
    assert ci == len(cols)


@pytest.mark.parametrize("ncols", [1, 2, 8, 60, 64, 128, 160, 256, 1000, 1024])
@pytest.mark.parametrize("order", [L.SORT_ORDER_ASC, L.SORT_ORDER_DESC], ids=["asc", "desc"])
def test_argsort_equals_numpy_and_keeps_index_order_among_equal_values(backend, order, ncols):
    rng = np.random.default_rng(ncols * 2 + order)
    H = L.host()
    data = []
    for rows in (1, 5, 512):
        distinct = (rng.permutation(rows * ncols).astype(np.float32) - rows * ncols / 2).reshape(rows, ncols)
        assert all(len(np.unique(r)) == ncols for r in distinct)
        ties = rng.integers(0, max(2, ncols // 4), (rows, ncols)).astype(np.float32) - 1.0
        data += [distinct, ties]

    def build(g):
        return [H.ggml_argsort(g.ctx, g.new(L.F32, [ncols, x.shape[0]], x), order) for x in data]

    res = T.run_case(build, backend)
    for x, r in zip(data, res):
        got = r.reshape(x.shape)
        key = -x if order == L.SORT_ORDER_DESC else x
        assert np.array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(ncols), x.shape)), "not a permutation"
        v = np.take_along_axis(key, got.astype(np.int64), axis=1)
        assert np.all(v[:, 1:] >= v[:, :-1]), "gathered values are not sorted"
        same = v[:, 1:] == v[:, :-1]
        assert np.all(got[:, 1:][same] > got[:, :-1][same]), "equal values are not in index order"
        assert np.array_equal(got, np.argsort(key, axis=1, kind="stable"))


def test_sum_rows_is_within_4_ulp_of_the_float64_sum(backend):
    rng = np.random.default_rng(3)
    H = L.host()
    shapes = [(1, 1, 1), (8, 5, 1), (60, 3, 2), (128, 200, 1), (1000, 7, 1), (1024, 512, 1), (8, 2, 77)]
    data = [(rng.standard_normal((n2, n1, n0)) * rng.uniform(0.01, 100.0)).astype(np.float32) for n0, n1, n2 in shapes]

    def build(g):
        return [H.ggml_sum_rows(g.ctx, g.new(L.F32, [x.shape[2], x.shape[1], x.shape[0]], x)) for x in data]

    for x, r in zip(data, T.run_case(build, backend)):
        ref = x.astype(np.float64).sum(axis=2).astype(np.float32)
        got = r.reshape(ref.shape)
        ulp = np.spacing(np.abs(ref))
        print(f"sum_rows {x.shape}: max |d| / ulp = {float(np.max(np.abs(got.astype(np.float64) - ref) / ulp)):.2f}")
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 4 * ulp)


def test_clamp_is_exact(backend):
    rng = np.random.default_rng(4)
    H = L.host()
    x = (rng.standard_normal((3, 5, 257)) * 4).astype(np.float32)
    x[0, 0, :4] = [0.0, -0.0, 6.103515625e-5, 1e-30]
    bounds = [(-1.0, 1.0), (6.103515625e-5, float("inf")), (float("-inf"), 0.5), (0.25, 0.25)]

    def build(g):
        return [H.ggml_clamp(g.ctx, g.new(L.F32, [257, 5, 3], x), lo, hi) for lo, hi in bounds]

    for (lo, hi), r in zip(bounds, T.run_case(build, backend)):
        ref = np.maximum(np.minimum(x, np.float32(hi)), np.float32(lo))
        assert np.array_equal(r.reshape(x.shape).view(np.uint32), ref.view(np.uint32)), (lo, hi)


@pytest.mark.parametrize("n_expert,n_used,n_tok", [(8, 2, 1), (8, 2, 77), (128, 8, 4), (128, 8, 512)])
def test_batched_get_rows_of_the_router_weights_is_exact(backend, n_expert, n_used, n_tok):
    """GET_ROWS(a = [1, n_expert, n_tokens], b = the strided top-k view [n_used, n_tokens]) against the oracle's 2-D GET_ROWS of the same elements."""
    rng = np.random.default_rng(n_tok)
    H = L.host()
    probs = rng.uniform(0.0, 1.0, (n_tok, n_expert)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)

    def gpu(g):
        a = g.new(L.F32, [1, n_expert, n_tok], probs)
        return H.ggml_get_rows(g.ctx, a, M.strided_ids(g, ids, n_expert))

    def ref(g):
        flat = (ids + n_expert * np.arange(n_tok, dtype=np.int32)[:, None]).astype(np.int32)
        return H.ggml_get_rows(g.ctx, g.new(L.F32, [1, n_expert * n_tok], probs), g.new(L.I32, [n_used * n_tok], flat))

    got = T.run_case(gpu, backend)[0]
    assert list(got.shape) == [1, n_tok, n_used, 1]
    want = T.run_case(ref, "oracle")[0]
    assert np.array_equal(got.reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(got.reshape(n_tok, n_used), np.take_along_axis(probs, ids.astype(np.int64), axis=1))


GLU_SHAPES = [(14336, 2, 5), (14336, 2, 32), (768, 8, 4), (768, 8, 77), (100, 3, 7), (4, 1, 2)]


def _glu_runs(backend, n_ff, n_used, n_tok):
    rng = np.random.default_rng(n_ff + n_tok)
    H = L.host()
    a = rng.standard_normal((n_tok, n_used, n_ff)).astype(np.float32) * 3
    b = rng.standard_normal((n_tok, n_used, n_ff)).astype(np.float32)
    a.ravel()[:6] = [0.0, -0.0, 87.0, -87.5, 95.0, -110.0]  # silu's expf at the ends of its range
    d3 = T.run_case(lambda g: H.ggml_swiglu_split(g.ctx, g.new(L.F32, [n_ff, n_used, n_tok], a), g.new(L.F32, [n_ff, n_used, n_tok], b)), backend)[0]
    flat = lambda g: H.ggml_swiglu_split(g.ctx, g.new(L.F32, [n_ff, n_used * n_tok], a), g.new(L.F32, [n_ff, n_used * n_tok], b))  # noqa: E731
    d2 = T.run_case(flat, backend)[0]
    want = T.run_case(flat, "oracle")[0]
    assert list(d3.shape) == [1, n_tok, n_used, n_ff]
    return d3.reshape(-1), d2.reshape(-1), want.reshape(-1)


@pytest.mark.parametrize("n_ff,n_used,n_tok", GLU_SHAPES)
def test_split_swiglu_over_the_3d_intermediate_is_exact(backend, plog, n_ff, n_used, n_tok):
    """The 3-D split SwiGLU ([n_ff, n_used, n_tokens], n_tokens > 1) is bit-equal to the ORACLE's GLU of the operands reshaped to 2-D.  silu(x) = x / (1 + expf(-x))
    is the same formula on both sides; the device library's expf differs from libm's in the last place for a few per cent of the arguments (733 of 28 672 elements,
    up to 3 ulp of the product, on [14336, 2, 1] before), so the 3-D form computes expf the way libm does (csrc/ops.hip: expf_libm)."""
    d3, _, want = _glu_runs(backend, n_ff, n_used, n_tok)
    diff = np.abs(d3.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    msg = f"swiglu_split 3-D [{n_ff}, {n_used}, {n_tok}] vs oracle: {int(np.count_nonzero(diff))} of {diff.size} elements differ, max {int(diff.max())} ulp, nmse {T.nmse(d3, want):.3e}"
    plog(msg)
    print(msg)
    assert np.array_equal(d3.view(np.uint32), want.view(np.uint32)), msg


@pytest.mark.parametrize("n_ff,n_used", [(14336, 2), (768, 8)])
def test_split_swiglu_of_one_token_is_the_dense_2d_form(backend, plog, n_ff, n_used):
    """With ONE token the intermediate [n_ff, n_used, 1] IS a 2-D tensor: it takes the dense split GLU's path, unchanged — bit-equal to the backend's GLU of the
    2-D operands, and within the dense form's gate against the oracle (tests/test_gpu_ops.py: NMSE <= 1e-13; that path keeps the device library's expf, so that
    dense graphs compute what they computed and the fused and unfused FFN chains stay equal)."""
    d3, d2, want = _glu_runs(backend, n_ff, n_used, 1)
    assert np.array_equal(d3.view(np.uint32), d2.view(np.uint32))
    T.compare(f"swiglu_split [{n_ff}, {n_used}, 1]", d3, want, max_nmse=1e-13, log=plog)


BLOCKS = {
    # n_embd, n_ff, n_expert, n_used, up / gate type, down type, CLAMP of the weight sum
    "mixtral-like": (1024, 3584, 8, 2, L.Q4_K, L.Q6_K, False),
    "qwen3-moe-like": (1024, 768, 128, 8, L.Q4_K, L.Q6_K, True),
}
_blocks = {}


def _block(name):
    if name not in _blocks:
        _blocks[name] = M.MoeBlock(*BLOCKS[name], seed=len(name))
    return _blocks[name]


@pytest.mark.parametrize("n_tok", [1, 4, 32, 200])
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_whole_moe_block_matches_the_composite_reference(backend, plog, name, n_tok):
    """llama.cpp's build_moe_ffn sequence end to end on the device (softmax router, top-k, normalised weights — with the CLAMP for the Qwen3-like block —,
    up / gate / down MUL_MAT_ID, split SwiGLU, weighting, sum over the slots); every node passes supports_op (the harness raises otherwise).
    Gates: the selected ids equal the reference's exactly — the margin between the n_used-th and the next probability is asserted on the ORACLE's
    probabilities (> 0.1 % of the probability; the f32 noise of the router product is ~1e-7) —; block output NMSE against the composite reference <= 1e-9,
    or 3 x the reference's own floor where that is larger.  The floor is the composite reference against the block in float64 on de-quantised weights
    with unquantised activations, measured on the CPU: 1.1e-4 .. 4.3e-4 for these blocks (mixtral-like 4.34e-4 / 3.84e-4 / 2.67e-4 / 2.62e-4 and qwen3-moe-like
    1.29e-4 / 1.15e-4 / 1.15e-4 / 1.17e-4 at 1 / 4 / 32 / 200 tokens) — far above 1e-9, because three products chain through 8-bit activation quantisation,
    which is discontinuous: two correct implementations one ulp apart in the intermediate round some activations to neighbouring int8 values.  The floor is
    re-measured by the test and printed."""
    blk = _block(name)
    x = blk.router_inputs(n_tok, np.random.default_rng(100 + n_tok))
    ref, ids_ref, probs = blk.reference(x)
    srt = np.sort(probs, axis=1)[:, ::-1]
    k = blk.n_used
    assert np.all(srt[:, k - 1] - srt[:, k] > 1e-3 * srt[:, k - 1]), "router margin too small for an exact id comparison"
    floor = T.nmse(ref, blk.numpy_f64(x, ids_ref))
    gate = 1e-9 if floor <= 1e-9 else 3.0 * floor
    m0 = backend.stat("mmid_launches")
    out, ids, _ = T.run_case(lambda g: blk.build(g, x), backend)
    assert backend.stat("mmid_launches") - m0 == 3
    plog(f"moe block {name} n_tokens={n_tok}: reference floor vs f64 = {floor:.3e}, gate = {gate:.3e}")
    print(f"moe block {name} n_tokens={n_tok}: reference floor vs f64 = {floor:.3e}, gate = {gate:.3e}, gpu nmse = {T.nmse(out.reshape(ref.shape), ref):.3e}")
    assert np.array_equal(ids.reshape(n_tok, k), ids_ref)
    T.compare(f"moe block {name} n_tokens={n_tok}", out.reshape(ref.shape), ref, gate, log=plog)


def _stepper(backend, blk, xs):
    """One batch-1 graph of the block, computed once per row of xs with the input replaced in between; returns (outputs, ids) per step."""
    H = L.host()
    g = T.G(backend)
    try:
        out, ids, _ = blk.build(g, xs[0][None, :])
        x_t = g.inputs[0][0]
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in (out, ids):
            H.ggml_set_output(o)
            H.ggml_build_forward_expand(gf, o)
        for i in range(gf.contents.n_nodes):
            assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i])
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        res = []
        for x in xs:
            raw = np.ascontiguousarray(x, dtype=np.float32)
            H.ggml_backend_tensor_set(x_t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(out).copy(), g.read(ids).copy()))
        return res
    finally:
        g.free()


def test_a_decode_step_with_the_block_is_captured_and_replays_follow_the_routing(backend, plog):
    """A batch-1 graph holding the block, computed three times with different router inputs: steps two and three launch the captured hipGraph (stat
    graph_launches, as test_hipgraph_replay_is_bit_identical_to_eager counts replays) although other experts are selected each time — the ids are read by the
    kernels, nothing on the host depends on them — and every result is bit-equal to an eager run on the same inputs.  (The backend exposes no stream-synchronise
    or device-to-host copy counters; the MUL_MAT_ID path holds no such call, and a capture would fail on one.)"""
    blk = _block("mixtral-like")
    rng = np.random.default_rng(77)
    xs = blk.router_inputs(3, rng)
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures", "eager_graphs", "mmid_launches")}
            runs[mode] = (_stepper(backend, blk, xs), {k: backend.stat(k) - v for k, v in s0.items()})
    finally:
        backend.set_option("graphs", 1)
    plog(f"moe block capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["mmid_launches"] == 9, runs[0][1]
    sel = [tuple(sorted(r[1].ravel().tolist())) for r in runs[0][0]]
    assert len(set(sel)) == 3, f"the three steps were meant to select different experts: {sel}"
    for (o1, i1), (o0, i0) in zip(runs[1][0], runs[0][0]):
        assert np.array_equal(i1, i0)
        assert np.array_equal(o1.view(np.uint32), o0.view(np.uint32))


@pytest.mark.parametrize("tname", ["q4_K", "q6_K", "q8_0", "f16"])
def test_an_id_outside_the_experts_gives_a_zero_slot_and_leaves_the_others_alone(backend, tname):
    """ggml-cpu asserts on an id outside [0, n_expert); the kernel's bounds check is the behaviour under test: that slot reads nothing of `as` and is written
    as zeros, every other slot is bit-equal to the run without the bad ids."""
    qtype = TYPES[tname]
    K, N, n_expert, n_used, n_tok = 512, 300, 8, 2, 4
    rng = np.random.default_rng(5)
    H = L.host()
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    b = rng.standard_normal((n_tok, n_used, K)).astype(np.float32)
    good = _routing(rng, n_tok, n_used, n_expert, False)
    bad = good.copy()
    bad[1, 0] = n_expert
    bad[2, 1] = -1

    def build(g):
        as_t = g.new(qtype, [K, N, n_expert], W)
        bt = g.new(L.F32, [K, n_used, n_tok], b)
        return [H.ggml_mul_mat_id(g.ctx, as_t, bt, M.strided_ids(g, i, n_expert)) for i in (good, bad)]

    rg, rb = [r.reshape(n_tok, n_used, N) for r in T.run_case(build, backend)]
    assert np.count_nonzero(rg) > rg.size // 2
    for t in range(n_tok):
        for s in range(n_used):
            if (t, s) in ((1, 0), (2, 1)):
                assert np.array_equal(rb[t, s].view(np.uint32), np.zeros(N, dtype=np.uint32)), (t, s)
            else:
                assert np.array_equal(rb[t, s].view(np.uint32), rg[t, s].view(np.uint32)), (t, s)


# kernel launches of the body below on the commit before MUL_MAT_ID and the router ops existed (measured there on an MI355X)
DENSE_LAUNCHES_BEFORE = 139


def _dense_body(backend):
    """A dense Llama model (test-llama: GET_ROWS of the embeddings, fused and plain SwiGLU paths) run eagerly: an 8-token prompt, then three single-token
    steps; plus a plain 2-D split GLU and a plain GET_ROWS graph.  Returns the kernel launches it took."""
    H = L.host()
    hp = preset("test-llama")
    mg = Model(hp, 7, backend.buft)
    backend.set_option("graphs", 0)
    try:
        k0 = backend.stat("kernel_launches")
        c = Context(mg, backend=backend, flash_attn=1)
        rc, _ = c.decode([1, 5, 9, 300, 17, 42, 99, 7], list(range(8)))
        assert rc == 0
        for i, tok in enumerate((11, 12, 13)):
            rc, _ = c.decode([tok], [8 + i])
            assert rc == 0
        c.free()
        rng = np.random.default_rng(1)
        a = rng.standard_normal((5, 512)).astype(np.float32)
        emb = rng.standard_normal((64, 256)).astype(np.float32)
        T.run_case(lambda g: H.ggml_swiglu_split(g.ctx, g.new(L.F32, [512, 5], a), g.new(L.F32, [512, 5], a)), backend)
        T.run_case(lambda g: H.ggml_swiglu(g.ctx, g.new(L.F32, [512, 5], a)), backend)
        T.run_case(lambda g: H.ggml_get_rows(g.ctx, g.new(L.F32, [256, 64], emb), g.new(L.I32, [3], np.array([5, 0, 63], dtype=np.int32))), backend)
        return backend.stat("kernel_launches") - k0
    finally:
        backend.set_option("graphs", 1)
        mg.free()


def test_dense_glu_and_get_rows_paths_launch_what_they_launched_before(backend, plog):
    n = _dense_body(backend)
    plog(f"dense regression guard: kernel_launches = {n} (before: {DENSE_LAUNCHES_BEFORE})")
    print(f"dense regression guard: kernel_launches = {n}")
    assert n == DENSE_LAUNCHES_BEFORE
