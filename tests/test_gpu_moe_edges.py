"""MUL_MAT_ID at the shapes, layouts and graph neighbourhoods the model shapes of tests/test_gpu_moe.py never reach.

Every threshold below is READ from the source by moe_ref.mmid_limits (launch_mmid_t, launch_mmid, mm_id_ok) — LIM — and the shapes are derived from it; if an
expression there is rewritten, the pattern in mmid_limits that names it is the one line to edit.

    kernel form (csrc/mmid.hip)                         selected by                                         reached by
    k_mmid<T, 2, true>, ragged last row tile            N * n_used * n_tokens >= LIM[r2_min], N % 8 != 0    test_two_rows_a_wave_with_a_ragged_last_tile
    k_mmid<T, 1, true>, N in {1, 2, 3, 5}               below r2_min; waves with row0 >= N                  test_one_row_a_wave_with_fewer_rows_than_waves
    k_mmid<T, 1, true>, 4 / 8 / 68 (lane, chunk) pairs  K of 1, 2, 17 K-quant blocks; 1, 2, 65 Q8_0 blocks  test_rows_of_one_block_and_pairs_around_one_wave
    k_mmid<T, 1, false> (no LDS staging)                K >= moe_ref.lds_free_k(T): row > LIM[lds_max]      test_the_lds_free_form
    k_mmid_f<false> (f32 experts), vector branch        type f32, K % LIM[vec_k] == 0, 16-byte aligned      test_f32_experts
    k_mmid_f<true / false>, scalar branch               K % LIM[vec_k] != 0, or b 4 bytes into its parent   test_the_scalar_branch_of_the_float_kernel
    grid.y = LIM[pair_max]                              n_used * n_tokens == LIM[pair_max]                  test_the_pair_limit_runs, test_above_the_pair_limit_is_refused
    (k_mmid<T, 2, false> needs N * pairs >= r2_min at K >= 52 480: a weight tensor of several hundred MB; the LDSA switch is orthogonal to R in the kernel text
     and both values of each are launched above.)

    operand layouts mm_id_ok accepts                                                                        test_operand_layouts[b_padded_per_slot / b_padded_per_token / as_view]
    quantiser site launch_quantize_act on a 3-D b -> k_mmid, read back exactly                              test_quantiser_read_back_through_mul_mat_id
    routed experts + dense shared expert on one norm output (the activation scratch and its cache key)      test_shared_expert_layer, test_shared_expert_decode_step_is_captured

The kernel variants cannot be told apart from outside — the timing class is mmid_<type> and the counter mmid_launches for all of them — so the forms are pinned
by shape against the thresholds read from the source, and each test asserts that its shape is on the intended side.
"""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as M
import probes as P

pytestmark = pytest.mark.gpu

QUANT = (L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0)
TYPES = {"q4_K": L.Q4_K, "q5_K": L.Q5_K, "q6_K": L.Q6_K, "q8_0": L.Q8_0, "f16": L.F16, "f32": L.F32}
QNAMES = ["q4_K", "q5_K", "q6_K", "q8_0"]
LIM = M.mmid_limits()
# f16 experts: the gate of tests/test_gpu_moe.py; f32 experts: the gate test_mul_mat_f (tests/test_gpu_ops.py) applies to f32 weights
GATE = {t: 1e-10 for t in TYPES.values()}
GATE[L.F32] = 1e-11
SENTINEL = np.float32(-1234.5)
GUARD = 64
JUNK = np.float32(3.0e6)


def _routing(rng, n_tok, n_used, n_expert):
    return np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)


def _acts(rng, n_tok, rows, K):
    return rng.standard_normal((n_tok, rows, K)).astype(np.float32)


# ---- how `b` reaches the node: -> (b tensor, column(t, r) = the [K, 1] view of one activation row)
def b_contiguous(g, b):
    n_tok, rows, K = b.shape
    bt = g.new(L.F32, [K, rows, n_tok], b)
    return bt, lambda t, r: g.H.ggml_view_2d(g.ctx, bt, K, 1, K * 4, (t * rows + r) * K * 4)


def b_padded(g, b):
    """A view [K, rows, n_tokens] at element offset (32, 1, 1) of a parent [K + 32, rows + 1, n_tokens + 1] that holds large junk everywhere else."""
    n_tok, rows, K = b.shape
    full = np.full((n_tok + 1, rows + 1, K + 32), JUNK, np.float32)
    full[::2] *= -1
    full[1:, 1:, 32:] = b
    pt = g.new(L.F32, [K + 32, rows + 1, n_tok + 1], full)
    nb1 = (K + 32) * 4
    nb2 = nb1 * (rows + 1)
    off = 32 * 4 + nb1 + nb2
    bt = g.H.ggml_view_3d(g.ctx, pt, K, rows, n_tok, nb1, nb2, off)
    return bt, lambda t, r: g.H.ggml_view_2d(g.ctx, pt, K, 1, nb1, off + t * nb2 + r * nb1)


def b_four_bytes_in(g, b):
    """A contiguous view that starts 4 bytes into its parent: the base is 4-byte but not 16-byte aligned."""
    n_tok, rows, K = b.shape
    flat = np.concatenate([np.array([JUNK], np.float32), b.ravel(), np.full(3, JUNK, np.float32)])
    pt = g.new(L.F32, [flat.size], flat)
    bt = g.H.ggml_view_3d(g.ctx, pt, K, rows, n_tok, K * 4, K * rows * 4, 4)
    return bt, lambda t, r: g.H.ggml_view_2d(g.ctx, pt, K, 1, K * 4, 4 + (t * rows + r) * K * 4)


def _into_guard(g, node):
    """Makes the node's result a view GUARD floats into a larger tensor filled with SENTINEL (what ggml's in-place builders do with view_src)."""
    n = int(g.H.ggml_nelements(node))
    parent = g.new(L.F32, [n + 2 * GUARD], np.full(n + 2 * GUARD, SENTINEL, np.float32))
    node.contents.view_src = parent
    node.contents.view_offs = GUARD * 4
    return parent


def run_cases(backend, plog, tag, qtype, K, N, W, cases, b_make=b_contiguous, as_range=None, guard=False, own=True):
    """The harness of test_mul_mat_id_matches_the_composite_reference_and_the_backends_own_mat_vec with its gates: every case (b [n_tokens, rows, K], ids) once
    with the strided top-k ids and once with contiguous ids; NMSE <= GATE against moe_ref.mmid_reference; both bit-equal; for the block formats every (slot, token)
    column bit-equal to the backend's own one-column MUL_MAT over the expert's 2-D view (n_used * n_tokens <= 32); one mmid launch per node.
    as_range (lo, n): `as` is the view of experts lo .. lo + n - 1 and the ids are relative to it; an id outside the view must give a zero slot.
    guard: every result is a view into a SENTINEL-filled tensor, which must keep the sentinel in front of and behind the result."""
    H = L.host()
    lo, ne = as_range or (0, W.shape[0])
    ref_cases = [(b, np.where((ids >= 0) & (ids < ne), ids, 0).astype(np.int32)) for b, ids in cases]
    ref = M.mmid_reference(qtype, W[lo:lo + ne], K, N, ref_cases)
    for (b, ids), r in zip(cases, ref):
        r[(ids < 0) | (ids >= ne)] = 0.0
    g = T.G(backend)
    try:
        as_t = g.new(qtype, [K, N, W.shape[0]], W)
        full = as_t
        if as_range:
            tt = as_t.contents
            as_t = H.ggml_view_3d(g.ctx, full, K, N, ne, tt.nb[1], tt.nb[2], lo * tt.nb[2])
        outs, cols, parents = [], [], []
        for b, ids in cases:
            n_tok, n_used = ids.shape
            rows = b.shape[1]
            bt, column = b_make(g, b)
            for idt in (M.strided_ids(g, ids, max(ne, n_used + 3)), g.new(L.I32, [n_used, n_tok], ids)):
                node = H.ggml_mul_mat_id(g.ctx, as_t, bt, idt)
                if guard:
                    parents.append(_into_guard(g, node))
                outs.append(node)
            if own and qtype in QUANT and n_used * n_tok <= 32:
                for t in range(n_tok):
                    for s in range(n_used):
                        if 0 <= ids[t, s] < ne:
                            cols.append(H.ggml_mul_mat(g.ctx, M.expert_view(g, full, K, N, lo + ids[t, s]), column(t, s if rows > 1 else 0)))
        m0 = backend.stat("mmid_launches")
        res = M.compute_in_weights_buffer(g, outs + cols)
        launches = backend.stat("mmid_launches") - m0
        guards = [g.read(p).reshape(-1) for p in parents]
    finally:
        g.free()
    assert launches == len(outs), f"{tag}: {launches} MUL_MAT_ID launches for {len(outs)} nodes"
    ci = 0
    for k, (b, ids) in enumerate(cases):
        n_tok, n_used = ids.shape
        strided, contig = (res[2 * k + j].reshape(n_tok, n_used, N) for j in (0, 1))
        T.compare(f"{tag} n_tokens={n_tok} rows={b.shape[1]} strided ids", strided, ref[k], GATE[qtype], log=plog)
        T.compare(f"{tag} n_tokens={n_tok} rows={b.shape[1]} contiguous ids", contig, ref[k], GATE[qtype], log=plog)
        assert np.array_equal(strided.view(np.uint32), contig.view(np.uint32)), f"{tag} n_tokens={n_tok}: strided and contiguous ids differ"
        for t in range(n_tok):
            for s in range(n_used):
                if not 0 <= ids[t, s] < ne:
                    assert not strided[t, s].view(np.uint32).any(), f"{tag}: id {ids[t, s]} outside the view did not give a zero slot"
                elif own and qtype in QUANT and n_used * n_tok <= 32:
                    mine = res[len(outs) + ci].reshape(N)
                    ci += 1
                    assert np.array_equal(strided[t, s].view(np.uint32), mine.view(np.uint32)), f"{tag} n_tokens={n_tok}: (slot {s}, token {t}) differs from MUL_MAT over the expert's view"
        for j in (0, 1):
            if guard:
                gd = guards[2 * k + j]
                inner = gd[GUARD:-GUARD].reshape(n_tok, n_used, N)
                assert np.array_equal(inner.view(np.uint32), res[2 * k + j].reshape(inner.shape).view(np.uint32))
                touched = np.nonzero(np.concatenate([gd[:GUARD], gd[-GUARD:]]).view(np.uint32) != SENTINEL.view(np.uint32))[0]
                assert touched.size == 0, f"{tag} n_tokens={n_tok}: guard floats {touched.tolist()} (front 0..{GUARD - 1}, behind {GUARD}..) were written"
    assert ci == len(cols)


# ------------------------------------------------------------------------------------------------ 1. every kernel form
def _blk(qtype):
    return L.TYPE_BLCK[qtype]


RAGGED = [(1, 1), (1, 5), (1, 7), (8, 7)]  # (n_tokens, rows past the last multiple of 8): N = 8193, 8197, 8199 at one token, 1031 at eight (r2_min 16384, n_used 2)


@pytest.mark.parametrize("n_tok,extra", RAGGED, ids=[f"tok{t}-N+{e}" for t, e in RAGGED])
@pytest.mark.parametrize("tname", QNAMES)
def test_two_rows_a_wave_with_a_ragged_last_tile(backend, plog, tname, n_tok, extra):
    """k_mmid<T, 2, true> with N % 8 != 0: N = LIM[r2_min] / (n_used * n_tokens) + {1, 5, 7} (8193, 8197, 8199 at one token; 1031 at eight tokens), K one block.
    The second row of the last wave is clamped for the loads (min(row0 + r, N - 1)) and must not be stored; whole waves have row0 >= N behind the barrier.
    Every result lives inside a sentinel-filled tensor that must stay untouched around it."""
    qtype, n_used, n_expert = TYPES[tname], 2, 4
    K = _blk(qtype)
    N = LIM["r2_min"] // (n_used * n_tok) + extra
    assert N * n_used * n_tok >= LIM["r2_min"] and N % 8 != 0 and (N - extra) * n_used * n_tok == LIM["r2_min"]
    rng = np.random.default_rng(N + qtype)
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    run_cases(backend, plog, f"mmid R=2 ragged {tname} K={K} N={N}", qtype, K, N, W, [(_acts(rng, n_tok, n_used, K), _routing(rng, n_tok, n_used, n_expert))], guard=True)


@pytest.mark.parametrize("N", [1, 2, 3, 5])
@pytest.mark.parametrize("tname", QNAMES)
def test_one_row_a_wave_with_fewer_rows_than_waves(backend, plog, tname, N):
    """k_mmid<T, 1, true> with N in {1, 2, 3, 5} at 1 and 3 tokens: waves whose row0 >= N take part in the LDS staging and leave; one workgroup holds 4 rows."""
    qtype, n_used, n_expert = TYPES[tname], 2, 4
    K = 2 * _blk(qtype)
    rng = np.random.default_rng(100 + N + qtype)
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    cases = [(_acts(rng, n_tok, n_used, K), _routing(rng, n_tok, n_used, n_expert)) for n_tok in (1, 3)]
    assert all(N * n_used * n_tok < LIM["r2_min"] for n_tok in (1, 3))
    run_cases(backend, plog, f"mmid R=1 {tname} K={K} N={N}", qtype, K, N, W, cases, guard=True)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["one-block", "two-blocks", "above-one-wave"])
@pytest.mark.parametrize("tname", QNAMES)
def test_rows_of_one_block_and_pairs_around_one_wave(backend, plog, tname, which):
    """Rows of 1, 2 and 17 K-quant super-blocks (K = 256, 512, 4352: 4, 8 and 68 (block, chunk) pairs — below and just above the 64 a wave strides by, so lanes
    >= npairs hold no weight and the loop body runs zero, one or two times) and of 1, 2 and 65 Q8_0 blocks (K = 32, 64, 2080: 1, 2 and 65 pairs)."""
    qtype, n_used, n_expert, N = TYPES[tname], 2, 4, 40
    blocks = ((1, 2, 65) if qtype == L.Q8_0 else (1, 2, 17))[which]
    K = blocks * _blk(qtype)
    rng = np.random.default_rng(200 + blocks + qtype)
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    cases = [(_acts(rng, n_tok, n_used, K), _routing(rng, n_tok, n_used, n_expert)) for n_tok in (1, 3)]
    run_cases(backend, plog, f"mmid short rows {tname} K={K}", qtype, K, N, W, cases)


@pytest.mark.parametrize("tname", QNAMES)
def test_the_lds_free_form(backend, plog, tname):
    """k_mmid<T, 1, false>: the first K whose quantised activation row exceeds LIM[lds_max] (moe_ref.lds_free_k: 52 480 for Q8_K activations of 320 bytes per
    256 values, 58 272 for Q8_0 activations of 36 bytes per 32), N = 12, two experts, 1 and 3 tokens, b with one row per slot and with one row per token.
    The variant cannot be told apart from outside (class mmid_<type>, counter mmid_launches for every form): the K threshold is read from launch_mmid_t."""
    qtype, n_used, n_expert, N = TYPES[tname], 2, 2, 12
    K = M.lds_free_k(qtype, LIM)
    rng = np.random.default_rng(300 + qtype)
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    cases = [(_acts(rng, n_tok, rows, K), _routing(rng, n_tok, n_used, n_expert)) for n_tok in (1, 3) for rows in (n_used, 1)]
    run_cases(backend, plog, f"mmid no-LDS {tname} K={K}", qtype, K, N, W, cases)


@pytest.mark.parametrize("n_used,per_slot", [(2, False), (2, True), (4, False), (4, True)], ids=["used2-per-token", "used2-per-slot", "used4-per-token", "used4-per-slot"])
def test_f32_experts(backend, plog, n_used, per_slot):
    """k_mmid_f<false>, vector branch (K % LIM[vec_k] == 0, everything 16-byte aligned): the up / down layouts of the model shapes at K 512, N 300, 8 experts,
    1 / 5 / 32 tokens.  Gate: the NMSE <= 1e-11 that test_mul_mat_f applies to f32 weights."""
    K, N, n_expert = 512, 300, 8
    assert K % LIM["vec_k"] == 0 and (K * 4) % LIM["vec_align"] == 0
    rng = np.random.default_rng(400 + n_used + per_slot)
    W = M.expert_weights(L.F32, K, N, n_expert, rng)
    cases = [(_acts(rng, n_tok, n_used if per_slot else 1, K), _routing(rng, n_tok, n_used, n_expert)) for n_tok in (1, 5, 32)]
    run_cases(backend, plog, f"mmid f32 experts n_used={n_used} per_slot={per_slot}", L.F32, K, N, W, cases)


@pytest.mark.parametrize("how", ["K100", "K7", "K1", "K512-b-4-bytes-in"])
@pytest.mark.parametrize("tname", ["f16", "f32"])
def test_the_scalar_branch_of_the_float_kernel(backend, plog, tname, how):
    """k_mmid_f<W16>'s scalar branch (vec_ok == 0): K % LIM[vec_k] != 0 (K = 100, 7, 1; N = 9), and K = 512 with b a view that starts 4 bytes into its parent
    (4-byte, not LIM[vec_align]-byte aligned).  The vector and scalar branches sum in different orders, so neither is compared with the other: both are
    gated against the reference (f16 1e-10, f32 the 1e-11 of test_mul_mat_f)."""
    qtype, n_used, n_expert, N = TYPES[tname], 2, 4, 9
    K = 512 if how.startswith("K512") else int(how[1:])
    assert (K % LIM["vec_k"] != 0) != how.startswith("K512") and 4 % LIM["vec_align"] != 0
    rng = np.random.default_rng(500 + K + qtype)
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    cases = [(_acts(rng, n_tok, rows, K), _routing(rng, n_tok, n_used, n_expert)) for n_tok in (1, 3) for rows in (n_used, 1)]
    run_cases(backend, plog, f"mmid scalar {tname} {how}", qtype, K, N, W, cases, b_make=b_four_bytes_in if how.startswith("K512") else b_contiguous)


def test_the_pair_limit_runs(backend, plog):
    """n_used 5 x n_tokens 13 107 = LIM[pair_max] = 65 535 (slot, token) pairs — grid.y at its limit —, K 256, N 5, Q4_K, 8 experts.  The reference is eight
    grouped oracle MUL_MATs."""
    n_used, n_expert, K, N = 5, 8, 256, 5
    n_tok = LIM["pair_max"] // n_used
    assert n_used * n_tok == LIM["pair_max"]
    rng = np.random.default_rng(600)
    W = M.expert_weights(L.Q4_K, K, N, n_expert, rng)
    run_cases(backend, plog, f"mmid {n_used} x {n_tok} pairs", L.Q4_K, K, N, W, [(_acts(rng, n_tok, n_used, K), _routing(rng, n_tok, n_used, n_expert))])


def test_above_the_pair_limit_is_refused(backend):
    """n_used 8 x n_tokens 8 192 > LIM[pair_max]: supports_op answers false (a query: nothing is launched); one token fewer than the limit's quotient is accepted."""
    H = L.host()
    n_used, K, N, n_expert = 8, 256, 5, 8
    over = LIM["pair_max"] // n_used + 1
    assert over == 8192
    g = T.G(backend)
    try:
        as_t = g.new(L.Q4_K, [K, N, n_expert])
        ans = {}
        for n_tok in (over, over - 1):
            node = H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, 1, n_tok]), g.new(L.I32, [n_used, n_tok]))
            ans[n_tok] = node
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        m0 = backend.stat("mmid_launches")
        assert not H.ggml_backend_dev_supports_op(backend.dev, ans[over])
        assert H.ggml_backend_dev_supports_op(backend.dev, ans[over - 1])
        assert backend.stat("mmid_launches") == m0
    finally:
        g.free()


# ------------------------------------------------------------------------------------------------ 2. operand layouts
@pytest.mark.parametrize("layout", ["b_padded_per_slot", "b_padded_per_token", "as_view"])
@pytest.mark.parametrize("tname", ["q4_K", "q8_0", "f16"])
def test_operand_layouts(backend, plog, tname, layout):
    """Layouts mm_id_ok accepts — an accepted op gives the right answer.  K 512, N 40, 6 experts, n_used 2, 1 and 5 tokens.
    b_padded_*: b is the view [K, n_used | 1, n_tokens] at element offset (32, 1, 1) of a parent [K + 32, rows + 1, n_tokens + 1] full of large junk: the
    quantiser (launch_quantize_act over TD(b)) must walk nb[1] / nb[2] and leave the rows in the flat order (tok * b_rows + slot) k_mmid indexes.
    as_view: `as` is the view of experts 2 .. 4 (byte offset 2 * nb[2], ne[2] = 3); ids are relative to the view and an id of 3 gives a zero slot."""
    qtype, K, N, n_expert, n_used = TYPES[tname], 512, 40, 6, 2
    rng = np.random.default_rng(700 + qtype + len(layout))
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    rows = 1 if layout == "b_padded_per_token" else n_used
    cases = []
    for n_tok in (1, 5):
        ids = _routing(rng, n_tok, n_used, 3 if layout == "as_view" else n_expert)
        if layout == "as_view" and n_tok == 5:
            ids[2, 1] = 3  # expert 5 of the parent: outside the view
            ids[4, 0] = -1
        cases.append((_acts(rng, n_tok, rows, K), ids))
    run_cases(backend, plog, f"mmid layout {layout} {tname}", qtype, K, N, W, cases, b_make=b_contiguous if layout == "as_view" else b_padded, as_range=(2, 3) if layout == "as_view" else None)


# ------------------------------------------------------------------------------------------------ 3. exact read-back of the quantiser
@pytest.mark.parametrize("K", [512, 1536])
@pytest.mark.parametrize("tname", QNAMES)
def test_quantiser_read_back_through_mul_mat_id(backend, plog, tname, K):
    """The quantiser site launch_quantize_act on a 3-D b -> k_mmid (the table of tests/test_gpu_value_edges.py lists the 2-D sites): the read-out weights of
    tests/probes.py stacked as experts, each rotated by its own shift, over the edge-activation catalogue as the rows of b — one row per (slot, token) and one
    row per token, 1 / 3 / 32 tokens, K = 512 and six super-blocks.  Gate: got == NumPy twin as uint32 (+-0 equal, NaN where the twin has NaN); that the
    composite oracle equals the twin on the same cases is asserted on the CPU (tests/test_moe_host.py)."""
    qtype = TYPES[tname]
    H = L.host()
    n = 0
    for what in ("values", "bsums") if qtype in (L.Q4_K, L.Q5_K) else ("values",):
        cases = [M.readout_case(qtype, K, n_tok, per_slot, what) for per_slot in (True, False) for n_tok in (1, 3, 32)]
        W = cases[0][0]

        def build(g):
            as_t = g.new(qtype, [K, W.shape[1], W.shape[0]], W)
            return [H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, b.shape[1], b.shape[0]], b), M.strided_ids(g, ids, W.shape[0] + 3)) for _, b, ids, _ in cases]

        m0 = backend.stat("mmid_launches")
        res = T.run_case(build, backend)
        assert backend.stat("mmid_launches") - m0 == len(cases)
        for (_, b, ids, want), r in zip(cases, res):
            got = r.reshape(want.shape)
            bad = P.bits(got) != P.bits(want)
            assert not bad.any(), (f"read-back {tname} K={K} [{what}] n_tokens={ids.shape[0]} rows={b.shape[1]}: {int(bad.sum())}/{bad.size} outputs differ from the NumPy twin; "
                                   f"first at (token, slot, output) {np.argwhere(bad)[0].tolist()}: {got[tuple(np.argwhere(bad)[0])]!r} != {want[tuple(np.argwhere(bad)[0])]!r}")
            n += 1
    plog(f"quantiser read-back through MUL_MAT_ID {tname} K={K}: {n} nodes bit-equal to the NumPy twin")


# ------------------------------------------------------------------------------------------------ 4. the shared-expert layer
LAYERS = {
    # routed up / gate, routed down, shared up / gate, shared down
    "q4_K+q6_K": (L.Q4_K, L.Q6_K, L.Q4_K, L.Q6_K),
    "q8_0": (L.Q8_0, L.Q8_0, L.Q8_0, L.Q8_0),
    "routed-q4_K-shared-q8_0": (L.Q4_K, L.Q4_K, L.Q8_0, L.Q8_0),
}
_layers = {}


def _layer(name):
    if name not in _layers:
        _layers[name] = M.SharedExpertLayer(512, 768, 1024, 8, 2, *LAYERS[name], seed=len(name))
    return _layers[name]


def _run_layer(backend, lay, x, order, routed_only=False):
    """-> ([out, ids, up, gate, down] as arrays, mmid launches, node ops)."""
    g = T.G(backend)
    try:
        out, sel, _, prods, first = lay.build(g, x, order, routed_only=routed_only)
        outs = [out, sel] + prods
        ops = M.node_ops(g, outs, first)
        m0 = backend.stat("mmid_launches")
        res = g.compute(outs, expand_first=first)
        return res, backend.stat("mmid_launches") - m0, ops
    finally:
        g.free()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("n_tok", [1, 2, 8, 9, 32, 40])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_shared_expert_layer(backend, plog, name, n_tok):
    """Routed experts plus a dense shared expert on ONE norm output (moe_ref.SharedExpertLayer: n_embd 512, routed n_ff 768, shared n_ff 1024, 8 experts, 2 used):
    the f32 router MUL_MAT, the routed MUL_MAT_IDs (through a reshape with the same data pointer and nbytes) and the dense quantised chain read the same tensor,
    and dense and expert mat-muls interleave in node order — in both orders, and in a third (shared_up_gate_first) that puts a MUL_MAT_ID on `cur` directly
    behind a dense quantised MUL_MAT on `cur`: there only the `kind` of quantized_src1's key separates the two quantisations when the formats differ.  1 / 2 / 8 / 9 / 32 / 40 tokens take the dense chain through the batch-1
    prologues, the multi-column mat-vec, the skinny kernels, the 9 .. 32-column Q8_0 panel kernel and the wide forms.
    Gates: ids equal the reference's (router margin asserted on the oracle's probabilities); output NMSE <= max(1e-9, 3 x floor), the floor being the
    reference against float64 on de-quantised weights (a property of the reference; measured here and printed: 6e-5 .. 4e-4 at these sizes); the two node orders
    bit-equal; fusion 1 against fusion 0 NMSE <= 1e-12 — what test_fused_chains_equal_unfused promises for the dense chain, no more —; the three MUL_MAT_ID
    results bit-equal to the same nodes of a graph holding the routed branch alone; mmid_launches + 3 per run.
    The order gate found a route that depended on the neighbourhood: [q4_K+q6_K-2] differed by an ulp in 430 of 1024 outputs between the orders (NMSE 4.6e-15) — with
    the routed branch first the shared expert's Q6_K down product is directly followed by both ADDs, took them into one mat-vec launch (mmvq_q6_K_nc2), and with the
    shared expert first it ran on the matrix-core kernel (mmq_q6_K_n512_k1024).  csrc/graph.cpp now keeps two columns of a Q4_K / Q6_K matrix on the matrix-core
    kernel with the first ADD in its store and leaves the second ADD a node of its own."""
    lay = _layer(name)
    x = lay.inputs(n_tok, np.random.default_rng(100 + n_tok))
    ref, ids_ref, probs, _ = lay.reference(x)
    srt = np.sort(probs, axis=1)[:, ::-1]
    k = lay.n_used
    assert np.all(srt[:, k - 1] - srt[:, k] > 1e-3 * srt[:, k - 1]), "router margin too small for an exact id comparison"
    floor = T.nmse(ref, lay.numpy_f64(x, ids_ref))
    gate = 1e-9 if floor <= 1e-9 else 3.0 * floor
    runs = {}
    for order in lay.ORDERS:
        runs[order] = _run_layer(backend, lay, x, order)
    backend.set_option("fusion", 0)
    try:
        plain = _run_layer(backend, lay, x, lay.ORDERS[0])
        plain_b = _run_layer(backend, lay, x, lay.ORDERS[1])
    finally:
        backend.set_option("fusion", 1)
    alone = _run_layer(backend, lay, x, lay.ORDERS[0], routed_only=True)
    (ra, la, opa), (rb, lb, opb), (rc, lc, opc) = (runs[o] for o in lay.ORDERS)
    msg = (f"shared-expert layer {name} n_tokens={n_tok}: reference floor vs f64 = {floor:.3e}, gate = {gate:.3e}, gpu nmse = {T.nmse(ra[0].reshape(ref.shape), ref):.3e} / "
           f"{T.nmse(rb[0].reshape(ref.shape), ref):.3e}, fused vs unfused = {T.nmse(ra[0], plain[0][0]):.3e}")
    plog(msg)
    print(msg)
    assert opa != opb and sorted(opa) == sorted(opb), "the two orders were meant to interleave the dense and the expert nodes differently"
    assert opc not in (opa, opb) and sorted(opc) == sorted(opa)
    assert la == 3 and lb == 3 and lc == 3 and plain[1] == 3 and alone[1] == 3
    for tag, r in (("routed first", ra), ("shared first", rb), ("shared up / gate first", rc), ("fusion 0", plain[0])):
        assert np.array_equal(r[1].reshape(n_tok, k), ids_ref), tag
        T.compare(f"shared-expert layer {name} n_tokens={n_tok} {tag}", r[0].reshape(ref.shape), ref, gate, log=plog)
    for j, what in enumerate(("up", "gate", "down")):
        for tag, r in (("routed first", ra), ("shared first", rb), ("shared up / gate first", rc)):
            assert _same(r[2 + j], alone[0][2 + j]), f"{name} n_tokens={n_tok} {tag}: MUL_MAT_ID {what} differs from the routed branch computed alone (nmse {T.nmse(r[2 + j], alone[0][2 + j]):.3e})"
    T.compare(f"shared-expert layer {name} n_tokens={n_tok} fused vs unfused", ra[0], plain[0][0], 1e-12, log=plog)
    assert _same(plain[0][0], plain_b[0][0]), f"{name} n_tokens={n_tok}: the two node orders differ with fusion 0 (nmse {T.nmse(plain[0][0], plain_b[0][0]):.3e})"
    assert _same(ra[0], rb[0]), f"{name} n_tokens={n_tok}: the two node orders differ (nmse {T.nmse(ra[0], rb[0]):.3e})"


def _stepper(backend, lay, xs, order):
    """One batch-1 graph of the layer, computed once per row of xs with the input replaced in between."""
    H = L.host()
    g = T.G(backend)
    try:
        out, ids, _, _, first = lay.build(g, xs[0][None, :], order)
        x_t = g.inputs[0][0]
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in first:
            H.ggml_build_forward_expand(gf, o)
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


@pytest.mark.parametrize("order", M.SharedExpertLayer.ORDERS)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_shared_expert_decode_step_is_captured(backend, plog, name, order):
    """The one-token layer computed three times with different inputs (as test_a_decode_step_with_the_block_is_captured_and_replays_follow_the_routing):
    steps two and three replay the captured hipGraph, and all three are bit-equal to graphs = 0."""
    lay = _layer(name)
    xs = lay.inputs(3, np.random.default_rng(83))
    runs = {}
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures", "eager_graphs", "mmid_launches")}
            runs[mode] = (_stepper(backend, lay, xs, order), {k: backend.stat(k) - v for k, v in s0.items()})
    finally:
        backend.set_option("graphs", 1)
    plog(f"shared-expert layer {name} {order} capture: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["mmid_launches"] == 9, runs[0][1]
    sel = [tuple(sorted(r[1].ravel().tolist())) for r in runs[0][0]]
    assert len(set(sel)) == 3, f"the three steps were meant to select different experts: {sel}"
    for (o1, i1), (o0, i0) in zip(runs[1][0], runs[0][0]):
        assert np.array_equal(i1, i0)
        assert _same(o1, o0)
