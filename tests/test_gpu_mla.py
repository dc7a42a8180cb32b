"""MUL_MAT over a 3-D quantised weight (one matrix per head: the absorbed MLA matrices wk_b / wv_b of llama.cpp's deepseek2 graph) on the GPU — csrc/mmb.hip,
csrc/graph.cpp: mm_batched_q_ok, DESIGN.md 4j — and one whole non-flash MLA attention block.  Helpers and references: tests/mla_ref.py (checked on the CPU by
tests/test_mla_ref_host.py).

Gates.  (a) NMSE <= 1e-10 against the oracle's op_mul_mat on the same 3-D tensors: the quantised MUL_MAT gate of tests/test_gpu_ops.py.  (b) every (head, column) bit-equal
to the backend's own one-column 2-D MUL_MAT over that head's view, the promise k_mmid makes.  The block: NMSE <= 1e-9 against the staged oracle reference (the block gate
of tests/test_gpu_moe.py), and at one token bit-equal to the same block with each batched node replaced by per-head 2-D nodes + CONCAT.

The block's shapes are the ones the feature was specified with (3 heads, qk_nope 64, qk_rope 32, kv_lora 256, v_head 64, 40 cells, M in {1, 5}, wk_b Q8_0, wv_b Q4_K),
except one: wo was to be Q4_K, whose rows are whole blocks of 256 values, and 3 heads x 64 = 192 is none.  The 3-head block therefore carries a Q8_0 wo, and a 4-head
block (256 = one Q4_K block) with a Q4_K wo runs beside it.
"""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import mla_ref as R

pytestmark = pytest.mark.gpu

GATE = 1e-10
BLOCK_GATE = 1e-9
IDS = [R.NAMES[t] for t in R.TYPES]
H3 = 3
MS = (1, 2, 3, 5, 8, 9, 33)  # every column-block width (1, 2, 4, 8) and every tail: 3 = 4 - 1, 5 = 8 - 3, 9 = 8 + 1, 33 = 4 x 8 + 1
NS = (1, 70)                 # 70: no multiple of the 4, 16, 32 or 64 rows a workgroup computes


def _ks(qt):
    """The K of the full N x M sweep: 4 and 8 (block, chunk) pairs a row — the kernel's row groups of W = 4 and W = 8 lanes (launch_mmb_nc)."""
    return (256, 512) if qt in R.KQUANTS else (128, 256)


def _wide_ks(qt):
    """... and of the reduced sweep: 16 pairs (W = 16, e.g. a Q8_0 wv_b with kv_lora 512) and more than 64 (the whole wave, W = 64, with a ragged second trip of
    its pair loop and its look-ahead load: 72 pairs, K-quants 68)."""
    return (1024, 4352) if qt in R.KQUANTS else (512, 2304)


def _lds_free_k(qt):
    """The smallest K whose quantised activation row no longer fits the kernel's 64 KiB LDS budget even for one column: k_mmb<T, 1, 64, false>."""
    act = 320 if qt in R.KQUANTS else (40 if qt in (L.Q4_1, L.Q5_1) else 36)  # sizeof(q8k_dev) per 256 values, q81_dev / q80_dev per 32 (csrc/common.h)
    return (64 * 1024 // act + 1) * L.TYPE_BLCK[qt]


def _probe(H, backend, qt, a_ne=(256, 8, 3), b_ne=(256, 2, 3, 1), buffer=None, edit=None, b_type=L.F32):
    """supports_op for MUL_MAT(a, b) over bare tensors (as llama.cpp's loader probes), `edit(a, b, mm)` applied first."""
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        a = H.ggml_new_tensor_3d(ctx, qt, *a_ne)
        b = H.ggml_new_tensor_4d(ctx, b_type, *b_ne)
        mm = H.ggml_mul_mat(ctx, a, b)
        if buffer is not None:
            a.contents.buffer = buffer
            a.contents.data = 0x100000
        if edit:
            edit(a, b, mm)
        return bool(H.ggml_backend_dev_supports_op(backend.dev, mm))
    finally:
        H.ggml_free(ctx)


@pytest.fixture(scope="module")
def weights_buffer(H, backend):
    buf = H.ggml_backend_buft_alloc_buffer(backend.buft, 1 << 16)
    assert buf
    H.ggml_backend_buffer_set_usage(buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
    yield buf
    H.ggml_backend_buffer_free(buf)


# ---------------------------------------------------------------------------------------------- supports_op
@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_supports_op_accepts_the_nine_formats(H, backend, weights_buffer, qt):
    K = 256 if qt in R.KQUANTS else 128
    for buf in (None, weights_buffer):  # a plain tensor (the loader's probe) and a tensor in a WEIGHTS buffer
        assert _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf)
        assert _probe(H, backend, qt, (K, 8, 3), (K, 5, 6, 1), buf), "r2 = 2"
        assert _probe(H, backend, qt, (K, 8, 3), (K, 5, 3, 2), buf), "E = 2"
        assert _probe(H, backend, qt, (K, 8, 3), (K, 1, 3, 7), buf), "the flash path's [K, 1, H, n_tokens]"

        def permuted(a, b, mm):  # ggml_permute(., 0, 2, 1, 3) of a [K + 32, 3, 2] view: nb[1] > nb[2], rows further apart than K
            b.contents.nb[1], b.contents.nb[2] = (K + 32) * 4 * 3, (K + 32) * 4

        assert _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, permuted)


@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_supports_op_refusals(H, backend, weights_buffer, qt):
    K = 256 if qt in R.KQUANTS else 128
    bs, blck = L.TYPE_SIZE[qt], L.TYPE_BLCK[qt]
    buf = weights_buffer
    def b_f16(a, b, mm):
        b.contents.type = L.F16
        for i in range(4):
            b.contents.nb[i] //= 2

    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, b_f16), "b f16"

    def dst_strided(a, b, mm):
        mm.contents.nb[1] += 4
        mm.contents.nb[2] = mm.contents.nb[1] * mm.contents.ne[1]
        mm.contents.nb[3] = mm.contents.nb[2] * mm.contents.ne[2]

    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, dst_strided), "a non-contiguous dst"

    def short_k(a, b, mm):  # rows of K - blck / 2 values of a parent with K: no whole number of blocks
        a.contents.ne[0] = b.contents.ne[0] = K - blck // 2

    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, short_k), "K not a whole number of blocks"
    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, lambda a, b, mm: a.contents.ne.__setitem__(3, 2)), "a->ne[3] = 2"
    def four_heads(a, b, mm):  # (edited in: the graph API itself asserts the broadcast rule)
        b.contents.ne[2] = mm.contents.ne[2] = 4
        b.contents.nb[3], mm.contents.nb[3] = b.contents.nb[2] * 4, mm.contents.nb[2] * 4

    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, four_heads), "b->ne[2] no multiple of H"
    assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, lambda a, b, mm: b.contents.nb.__setitem__(2, b.contents.nb[2] + 2)), "a b stride off the element grid"
    if qt in (L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1, L.IQ4_NL):  # the aligned formats: every matrix starts on the block alignment (2 bytes; 4 for the offset formats)
        al = 4 if qt in (L.Q4_1, L.Q5_1) else 2
        assert _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, lambda a, b, mm: a.contents.nb.__setitem__(2, a.contents.nb[2] + bs))
        assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), buf, lambda a, b, mm: a.contents.nb.__setitem__(2, a.contents.nb[2] + al // 2)), "a block-misaligned nb[2]"
    # a buffer that is no WEIGHTS buffer: what the f16 image of a KV-cache view does not take (dim 3 of b broadcast; a K-quant) stays refused, as before the batched node
    plain = H.ggml_backend_buft_alloc_buffer(backend.buft, 1 << 16)
    assert plain
    try:
        assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 2), plain), "E = 2 outside a WEIGHTS buffer"
        assert _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), plain) == (qt not in R.KQUANTS), "outside a WEIGHTS buffer: the image route or nothing"
    finally:
        H.ggml_backend_buffer_free(plain)
    # the split (-sm row) and row-parallel buffer types
    addr =H.ggml_backend_reg_get_proc_address(backend.reg, b"ggml_backend_split_buffer_type")
    assert addr
    split_buft = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_float))(addr)(0, (C.c_float * 16)(*([0.0] * 16)))
    rowpar = H.ggml_backend_buft_alloc_buffer(backend.rowpar_buft(), 1 << 16)
    assert rowpar
    H.ggml_backend_buffer_set_usage(rowpar, 1)  # (as the loader marks every buffer of a model: outside a WEIGHTS buffer a block-format batch is a KV-cache view)
    for other in (H.ggml_backend_buft_alloc_buffer(split_buft, 0), rowpar):
        assert other
        try:
            assert not _probe(H, backend, qt, (K, 8, 3), (K, 2, 3, 1), other)
        finally:
            H.ggml_backend_buffer_free(other)


@pytest.mark.parametrize("qt", (L.Q2_K, L.Q3_K, L.IQ4_XS, L.BF16), ids=["q2_K", "q3_K", "iq4_xs", "bf16"])
def test_the_pinned_formats_stay_refused(H, backend, weights_buffer, qt):
    """Restated from tests/test_gpu_kq23_weights.py, test_gpu_iq4xs_weights.py and test_gpu_bf16_weights.py: a 3-D weight in these formats stays on the CPU backend
    (bf16: in a WEIGHTS buffer, as that test pins it — outside one a bf16 batch is a KV-cache view on its f16 image, as before)."""
    for buf in ((weights_buffer,) if qt == L.BF16 else (None, weights_buffer)):
        assert not _probe(H, backend, qt, (256, 8, 2), (256, 1, 2, 1), buf)
        assert not _probe(H, backend, qt, (256, 8, 3), (256, 5, 3, 1), buf)


# ---------------------------------------------------------------------------------------------- values
_REF = {}


def _case(qt, K, N, ms=MS):
    """Weights [H3, N, .], activations [1, H3, max(ms), K] (the cases of fewer columns take the first M) and the oracle's batched products for every M: computed once, shared."""
    key = (qt, K, N, ms)
    if key not in _REF:
        rng = np.random.default_rng(9000 + 131 * qt + K + N)
        W = R.head_weights(qt, K, N, H3, rng)
        X = rng.standard_normal((1, H3, max(ms), K)).astype(np.float32)
        X[0, 1, 0, :L.TYPE_BLCK[qt]] = 0.0  # one activation block all zero
        g = T.G("oracle")
        try:
            a = g.new(qt, [K, N, H3], W)
            outs = [g.H.ggml_mul_mat(g.ctx, a, R.make_b(g, X[:, :, :M], "contig")) for M in ms]
            ref = {M: r.reshape(1, H3, M, N) for M, r in zip(ms, g.compute(outs, T.host_threads()))}
        finally:
            g.free()
        _REF[key] = (W, X, ref)
    return _REF[key]


def _sweep(backend, qt, ks, ns, ms):
    """type x K x N x H = 3 x M: gate (a) against the oracle, gate (b) bit-equality with the backend's own one-column 2-D MUL_MATs (one graph per (K, N): the batched
    nodes, and one 2-D node per (head, column) of the widest b, whose first M columns are the smaller cases' b).  -> the worst NMSE"""
    worst = 0.0
    for K in ks:
        for N in ns:
            W, X, ref = _case(qt, K, N, ms)
            g = T.G(backend)
            try:
                a = g.new(qt, [K, N, H3], W, "w_b")
                bs = {M: R.make_b(g, X[:, :, :M], "contig") for M in ms}
                outs = [g.H.ggml_mul_mat(g.ctx, a, bs[M]) for M in ms]
                ph = R.per_head_nodes(g, a, bs[max(ms)], one_column=True)
                i0 = backend.stat("kv_image_nodes")
                res = R.compute_in_weights_buffer(g, outs + [n for _, n in ph])
                assert backend.stat("kv_image_nodes") == i0, "a node ran on an f16 image of the weight"
            finally:
                g.free()
            twin = R.assemble([w for w, _ in ph], res[len(ms):], 1, H3, max(ms), N)
            for M, got in zip(ms, res):
                got = got.reshape(1, H3, M, N)
                e = T.nmse(got, ref[M])
                worst = max(worst, e)
                print(f"  {R.NAMES[qt]} K={K} N={N} M={M}: nmse vs oracle {e:.3e}, bit-equal to the one-column twin {int(np.count_nonzero(R.bits(got) == R.bits(twin[:, :, :M])))}/{got.size}")
                assert e <= GATE, (R.NAMES[qt], K, N, M, e)
                assert np.array_equal(R.bits(got), R.bits(twin[:, :, :M])), (R.NAMES[qt], K, N, M)
    return worst


@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_values_every_column_block_and_tail(backend, plog, qt):
    """type x K (4 and 8 pairs a row: row groups of 4 and 8 lanes) x N in {1, 70} x H = 3 x M in {1, 2, 3, 5, 8, 9, 33}: gates (a) and (b)."""
    worst = _sweep(backend, qt, _ks(qt), NS, MS)
    plog(f"mla batched mul_mat {R.NAMES[qt]}: worst nmse vs oracle {worst:.3e} over K {_ks(qt)} x N {NS} x M {MS}")


@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_values_row_groups_of_16_lanes_and_the_whole_wave(backend, plog, qt):
    """The other two row-group widths under the same gates, N = 70, M in {1, 3, 9} (column blocks of 1, 4 with a dead column, 8 + a tail of 1): 16 pairs a row
    (group_sum<16>) and 68 / 72 pairs (one row a wave, two trips of the pair loop, the second ragged)."""
    worst = _sweep(backend, qt, _wide_ks(qt), (70,), (1, 3, 9))
    plog(f"mla batched mul_mat {R.NAMES[qt]}: worst nmse vs oracle {worst:.3e} over K {_wide_ks(qt)} x N 70 x M (1, 3, 9)")


@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_values_rows_beyond_the_lds_budget(backend, plog, qt):
    """k_mmb<T, 1, 64, false>: the first K whose quantised activation row exceeds 64 KiB, so that no column block fits the LDS and the rows are read from global
    memory one column a workgroup (M = 2: two column blocks).  N = 3 (fewer rows than the workgroup's four waves).  Same gates."""
    K = _lds_free_k(qt)
    worst = _sweep(backend, qt, (K,), (3,), (1, 2))
    plog(f"mla batched mul_mat {R.NAMES[qt]}: worst nmse vs oracle {worst:.3e} at K {K} (no LDS staging)")


@pytest.mark.parametrize("layout,r2,E", [("permuted", 1, 1), ("strided", 1, 1), ("mla", 1, 1), ("contig", 2, 1), ("contig", 1, 2), ("mla", 2, 2)])
@pytest.mark.parametrize("qt", R.TYPES, ids=IDS)
def test_values_broadcast_and_strided_b(backend, qt, layout, r2, E):
    """r2 = 2, E = 2, the permuted b with nb[1] > nb[2] and a b whose rows sit further apart than K (the strided layouts hold 1e3 between the rows)."""
    K, N, H, M = _ks(qt)[0], 70, 2, 5
    rng = np.random.default_rng(9500 + 17 * qt + 3 * r2 + E + len(layout))
    W = R.head_weights(qt, K, N, H, rng)
    X = rng.standard_normal((E, H * r2, M, K)).astype(np.float32)

    def run(target):
        g = T.G(target)
        try:
            node, a, b = R.batched_node(g, qt, W, X, layout)
            assert b.contents.nb[0] == 4 and (layout not in ("permuted", "mla") or b.contents.nb[1] > b.contents.nb[2])
            if target == "oracle":
                return g.compute([node], T.host_threads()), None
            ph = R.per_head_nodes(g, a, b, one_column=True)
            res = R.compute_in_weights_buffer(g, [node] + [n for _, n in ph])
            return res, R.assemble([w for w, _ in ph], res[1:], E, H * r2, M, N)
        finally:
            g.free()

    ref = run("oracle")[0][0].reshape(E, H * r2, M, N)
    res, twin = run(backend)
    got = res[0].reshape(E, H * r2, M, N)
    e = T.nmse(got, ref)
    print(f"  {R.NAMES[qt]} {layout} r2={r2} E={E}: nmse vs oracle {e:.3e}")
    assert e <= GATE, e
    assert np.array_equal(R.bits(got), R.bits(twin))


@pytest.mark.parametrize("M", [1, 9, 33])
@pytest.mark.parametrize("qt", (L.Q8_0, L.Q4_1, L.Q4_K), ids=["q8_0", "q4_1", "q4_K"])
def test_one_launch_and_one_quantise_launch_per_node(backend, qt, M):
    K, N = _ks(qt)[0], 70
    W, X, ref = _case(qt, K, N)
    backend.set_option("graphs", 0)
    try:
        g = T.G(backend)
        try:
            node, _, _ = R.batched_node(g, qt, W, X[:, :, :M], "permuted")
            k0 = backend.stat("kernel_launches")
            got = R.compute_in_weights_buffer(g, [node])[0]
            launches = backend.stat("kernel_launches") - k0
        finally:
            g.free()
    finally:
        backend.set_option("graphs", 1)
    assert launches == 2, f"{launches} launches for one batched node of {M} columns (expected: the quantiser and the mat-mul)"
    assert T.nmse(got.reshape(ref[M].shape), ref[M]) <= GATE


# ---------------------------------------------------------------------------------------------- the activation cache
@pytest.mark.parametrize("order", ["tensor_first", "permuted_first"])
@pytest.mark.parametrize("qt", (L.Q8_0, L.Q4_K), ids=["q8_0", "q4_K"])
def test_quantised_activation_cache_tells_a_tensor_from_its_permutation(backend, qt, order):
    """Two batched nodes in one graph whose b share data and nbytes but not strides: a tensor t [K, 3, 3] and ggml_permute(t, 0, 2, 1, 3) (ne[1] == ne[2]).  The
    quantised rows of the one are not the rows of the other in another order of nodes either."""
    K, N, H = _ks(qt)[0], 70, 3
    rng = np.random.default_rng(9900 + qt)
    W = R.head_weights(qt, K, N, H, rng)
    X = rng.standard_normal((1, H, H, K)).astype(np.float32)  # t in ggml order [K, 3, 3]: X[0, i2, i1]

    def build(g):
        a = g.new(qt, [K, N, H], W, "w_b")
        t = g.new(L.F32, [K, H, H], X)
        p = g.H.ggml_permute(g.ctx, t, 0, 2, 1, 3)
        assert p.contents.data == t.contents.data and g.H.ggml_nbytes(p) == g.H.ggml_nbytes(t)
        n_t, n_p = g.H.ggml_mul_mat(g.ctx, a, t), g.H.ggml_mul_mat(g.ctx, a, p)
        return [n_t, n_p] if order == "tensor_first" else [n_p, n_t]

    g = T.G("oracle")
    try:
        ref = g.compute(build(g), 2)
    finally:
        g.free()
    g = T.G(backend)
    try:
        got = R.compute_in_weights_buffer(g, build(g))
    finally:
        g.free()
    assert T.nmse(ref[0], ref[1]) > 0.1, "the two products were meant to differ"
    for k in (0, 1):
        assert T.nmse(got[k], ref[k]) <= GATE, (order, k, T.nmse(got[k], ref[k]))


# ---------------------------------------------------------------------------------------------- a whole MLA attention block
BLOCKS = {"3heads-q8_0-wo": dict(n_head=3, t_o=L.Q8_0), "4heads-q4_K-wo": dict(n_head=4, t_o=L.Q4_K)}


def _block(name, M):
    key = ("block", name, M)
    if key not in _REF:
        blk = R.MlaBlock(seed=7 + BLOCKS[name]["n_head"], **BLOCKS[name])
        q, kvpe = blk.inputs(M, np.random.default_rng(70 + M))
        ref = blk.reference(q, kvpe)
        _REF[key] = (blk, q, kvpe, ref, T.nmse(ref, blk.numpy_f64(q, kvpe)))
    return _REF[key]


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("name", list(BLOCKS))
def test_mla_block_against_the_staged_oracle(backend, plog, name, M):
    blk, q, kvpe, ref, floor = _block(name, M)
    res, stats, n_nodes = R.run_block(backend, blk, [(q, kvpe)])
    e = T.nmse(res[0][0], ref)
    msg = f"mla block {name} M={M}: {n_nodes} nodes, gpu nmse vs staged oracle {e:.3e} (gate {BLOCK_GATE:.0e}); oracle vs float64 floor {floor:.3e}; {stats}"
    plog(msg)
    print("  " + msg)
    assert stats["kv_image_nodes"] == 0, "a batched node ran on an f16 image of its weight"
    assert e <= BLOCK_GATE, msg
    if M == 1:  # ... and bit-equal to the block whose batched nodes are per-head 2-D nodes + CONCAT along dim 2, on the same backend
        twin, _, n_twin = R.run_block(backend, blk, [(q, kvpe)], per_head=True)
        assert n_twin > n_nodes
        for k, what in enumerate(("out", "wk_b product", "wv_b product")):
            assert np.array_equal(R.bits(res[0][k]), R.bits(twin[0][k])), what


def test_mla_block_decode_graph_is_captured_and_replayed(backend, plog):
    """The one-token block computed three times with fresh inputs: one capture, two replays, bit-equal to a backend with graphs off."""
    blk = _block("3heads-q8_0-wo", 1)[0]
    rng = np.random.default_rng(77)
    steps = [blk.inputs(1, rng) for _ in range(3)]
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            runs[mode] = R.run_block(backend, blk, steps)
    finally:
        backend.set_option("graphs", 1)
    plog(f"mla block capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_captures"] == 1 and runs[1][1]["graph_launches"] == 2, runs[1][1]
    assert runs[0][1]["graph_captures"] == 0 and runs[0][1]["graph_launches"] == 0, runs[0][1]
    for a, b in zip(runs[1][0], runs[0][0]):
        for x, y in zip(a, b):
            assert np.array_equal(R.bits(x), R.bits(y))
    assert not np.array_equal(runs[0][0][0][0], runs[0][0][1][0]), "the steps were meant to differ"
