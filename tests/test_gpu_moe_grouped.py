"""MUL_MAT_ID, the grouped matrix-core form (csrc/mmid_group.hip): the pairs ordered by expert on the device, every expert's pairs as the columns of the integer
matrix-core unit.  Against the composite reference of tests/moe_ref.py with the form forced on (mmid_group 2), batch invariance to the bit, the routing of the
default (mmid_group 1: MI_MMID_GROUP_MIN_PAIRS of csrc/kernels.h), and a captured graph replayed over new ids.  The form is recognised by its timing class."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as M

pytestmark = pytest.mark.gpu

TYPES = {"q4_K": L.Q4_K, "q5_K": L.Q5_K, "q6_K": L.Q6_K}
N_EXPERT, N_USED, N_TOK = 6, 2, 40


def _routing(rng):
    """ids [40, 2] over 6 experts: expert 0 in slot 0 of every token (40 columns: a full tile and a tile of 8); slot 1: expert 1 for exactly 32 tokens, expert 2
    for exactly one, expert 3 for nobody, experts 4 / 5 at random for five, and the ids -1 and n_expert for the last two; the tokens shuffled."""
    ids = np.zeros((N_TOK, N_USED), np.int32)
    ids[:32, 1], ids[32, 1], ids[33:38, 1], ids[38, 1], ids[39, 1] = 1, 2, rng.integers(4, 6, 5), -1, N_EXPERT
    return ids[rng.permutation(N_TOK)]


def _k_for(qtype, K):
    return K + 256 if qtype == L.Q6_K and (K // 256) % 2 else K


def _compute(backend, build, group, graphs=1):
    """(results, timing classes) of one graph computed in a weights buffer under mmid_group = group."""
    g = T.G(backend)
    try:
        backend.set_option("mmid_group", group)
        backend.set_option("graphs", graphs)
        backend.set_option("timing", 1)
        backend.timing_report()
        res = M.compute_in_weights_buffer(g, build(g))
        return res, backend.timing_report()
    finally:
        backend.set_option("timing", 0)
        backend.set_option("graphs", 1)
        backend.set_option("mmid_group", 1)
        g.free()


def _count(classes, name):
    return classes.get(name, (0,))[0]


# (2304, 64): nine super-blocks, a wave takes two; (768, 96): fewer super-blocks than waves; (256, 32): one super-block, one panel.  Q6_K rows are 210 bytes a
# super-block and the form wants them dword-aligned — an even number of super-blocks: K 256, 768 and 2304 would be refused and run the pair form, so Q6_K
# takes one super-block more (_k_for): 512 (its smallest shape), 1024, 2560 (ten super-blocks: two waves take two)
@pytest.mark.parametrize("per_slot", [False, True], ids=["one-row", "row-per-slot"])
@pytest.mark.parametrize("K,N", [(256, 32), (768, 96), (2304, 64)])
@pytest.mark.parametrize("tname", sorted(TYPES))
def test_grouped_form_matches_the_composite_reference(backend, plog, tname, K, N, per_slot):
    qtype = TYPES[tname]
    K = _k_for(qtype, K)
    rng = np.random.default_rng(K + N + qtype)
    W = M.expert_weights(qtype, K, N, N_EXPERT, rng)
    b = rng.standard_normal((N_TOK, N_USED if per_slot else 1, K)).astype(np.float32)
    ids = _routing(rng)
    bad = (ids < 0) | (ids >= N_EXPERT)
    assert bad.sum() == 2 and [int((ids == e).sum()) for e in range(4)] == [40, 32, 1, 0]
    ref = M.mmid_reference(qtype, W, K, N, [(b, np.where(bad, 4, ids).astype(np.int32))])[0]
    H = L.host()

    def build(g):
        as_t, bt = g.new(qtype, [K, N, N_EXPERT], W), g.new(L.F32, [K, b.shape[1], N_TOK], b)
        return [H.ggml_mul_mat_id(g.ctx, as_t, bt, M.strided_ids(g, ids, N_EXPERT)), H.ggml_mul_mat_id(g.ctx, as_t, bt, g.new(L.I32, [N_USED, N_TOK], ids))]

    (strided, contig), classes = _compute(backend, build, 2)
    strided, contig = strided.reshape(N_TOK, N_USED, N), contig.reshape(N_TOK, N_USED, N)
    assert _count(classes, f"mmid_grp_{tname}") == 2 and _count(classes, f"mmid_{tname}") == 0, classes
    assert np.array_equal(strided.view(np.uint32), contig.view(np.uint32))
    assert not strided[bad].any() and np.count_nonzero(strided[~bad]) > strided[~bad].size // 2
    T.compare(f"mul_mat_id grouped {tname} K={K} N={N} per_slot={per_slot}", strided[~bad], ref[~bad], 1e-10, log=plog)


@pytest.mark.parametrize("tname", sorted(TYPES))
def test_a_pairs_result_does_not_depend_on_the_batch(backend, tname):
    """The 40-token node, a node over its first five tokens (10 pairs: other tiles) and one with the tokens reversed: every shared (slot, token) column is bit-equal."""
    qtype, N = TYPES[tname], 64
    K = _k_for(qtype, 2304)
    rng = np.random.default_rng(7 + qtype)
    W = M.expert_weights(qtype, K, N, N_EXPERT, rng)
    b = rng.standard_normal((N_TOK, N_USED, K)).astype(np.float32)
    ids = _routing(rng)
    H = L.host()

    def build(g):
        as_t = g.new(qtype, [K, N, N_EXPERT], W)
        return [H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, N_USED, len(i)], np.ascontiguousarray(x)), M.strided_ids(g, np.ascontiguousarray(i), N_EXPERT))
                for x, i in ((b, ids), (b[:5], ids[:5]), (b[::-1], ids[::-1]))]

    (full, head, rev), classes = _compute(backend, build, 2)
    assert _count(classes, f"mmid_grp_{tname}") == 3, classes
    full = full.reshape(N_TOK, N_USED, N).view(np.uint32)
    assert np.array_equal(head.reshape(5, N_USED, N).view(np.uint32), full[:5])
    assert np.array_equal(rev.reshape(N_TOK, N_USED, N).view(np.uint32), full[::-1])


@pytest.mark.parametrize("tname", sorted(TYPES))
def test_add_id_rides_in_the_grouped_store(backend, tname):
    """MUL_MAT_ID -> ADD_ID under mmid_group 2: with mmid_bias 1 the bias is added in the grouped kernel's store (one fused node), bit-equal to the grouped product
    followed by the ADD_ID launch (mmid_bias 0); the two pairs outside the experts are zeros either way."""
    qtype, K, N = TYPES[tname], 1024, 96
    rng = np.random.default_rng(31 + qtype)
    W = M.expert_weights(qtype, K, N, N_EXPERT, rng)
    b = rng.standard_normal((N_TOK, 1, K)).astype(np.float32)
    bias = rng.standard_normal((N_EXPERT, N)).astype(np.float32)
    ids = _routing(rng)
    H = L.host()

    def build(g):
        sel = M.strided_ids(g, ids, N_EXPERT)
        mm = H.ggml_mul_mat_id(g.ctx, g.new(qtype, [K, N, N_EXPERT], W), g.new(L.F32, [K, 1, N_TOK], b), sel)
        return [H.ggml_add_id(g.ctx, mm, g.new(L.F32, [N, N_EXPERT], bias), sel)]

    res = {}
    try:
        for mode in (1, 0):
            backend.set_option("mmid_bias", mode)
            f0 = backend.stat("fused_nodes")
            (r,), classes = _compute(backend, build, 2)
            assert _count(classes, f"mmid_grp_{tname}") == 1 and _count(classes, "add_id") == 1 - mode, classes
            res[mode] = (r.reshape(N_TOK, N_USED, N), backend.stat("fused_nodes") - f0)
    finally:
        backend.set_option("mmid_bias", 1)
    assert res[1][1] - res[0][1] == 1
    assert np.array_equal(res[1][0].view(np.uint32), res[0][0].view(np.uint32))
    bad = (ids < 0) | (ids >= N_EXPERT)
    assert not res[1][0][bad].any() and res[1][0][~bad].all()


def _min_pairs():
    with open(os.path.join(L.REPO, "llama_box_amd", "csrc", "kernels.h")) as f:
        (v,) = re.findall(r"#define MI_MMID_GROUP_MIN_PAIRS (\d+)", f.read())
    return int(v)


@pytest.mark.parametrize("tname", sorted(TYPES))
def test_the_default_routes_by_pair_count_and_format(backend, tname):
    """mmid_group 1: 32 pairs keep the pair form, MI_MMID_GROUP_MIN_PAIRS pairs take the grouped one, Q8_0 experts never do; mmid_group 0: nobody does."""
    K, N, big = 512, 64, _min_pairs()
    assert big >= 33
    rng = np.random.default_rng(11)
    H = L.host()

    def node(qtype, n_tok):
        W = M.expert_weights(qtype, K, N, N_EXPERT, rng)
        b = rng.standard_normal((n_tok, 1, K)).astype(np.float32)
        ids = rng.integers(0, N_EXPERT, (n_tok, 1)).astype(np.int32)
        return lambda g: [H.ggml_mul_mat_id(g.ctx, g.new(qtype, [K, N, N_EXPERT], W), g.new(L.F32, [K, 1, n_tok], b), M.strided_ids(g, ids, N_EXPERT))]

    for group, qtype, n_tok, want in ((1, TYPES[tname], 32, f"mmid_{tname}"), (1, TYPES[tname], big, f"mmid_grp_{tname}"), (1, L.Q8_0, big, "mmid_q8_0"), (0, TYPES[tname], big, f"mmid_{tname}")):
        _, classes = _compute(backend, node(qtype, n_tok), group)
        assert {k: v[0] for k, v in classes.items() if k.startswith("mmid")} == {want: 1}, (group, n_tok, classes)


def test_a_captured_graph_follows_new_ids_on_replay(backend):
    """The forced-form node computed three times with other ids uploaded in between: computes two and three are replays of the captured hipGraph (graph_launches),
    each bit-equal to an eager run over the same ids."""
    qtype, K, N = L.Q4_K, 768, 96
    rng = np.random.default_rng(21)
    W = M.expert_weights(qtype, K, N, N_EXPERT, rng)
    b = rng.standard_normal((N_TOK, 1, K)).astype(np.float32)
    idss = [_routing(rng) for _ in range(3)]
    H = L.host()
    runs = {}
    for graphs in (1, 0):
        g = T.G(backend)
        try:
            backend.set_option("mmid_group", 2)
            backend.set_option("graphs", graphs)
            idt = g.new(L.I32, [N_USED, N_TOK], idss[0])
            as_t, bt = g.new(qtype, [K, N, N_EXPERT], W), g.new(L.F32, [K, 1, N_TOK], b)
            out = H.ggml_mul_mat_id(g.ctx, as_t, bt, idt)
            for _ in range(4):  # (graphs of fewer than eight nodes are not captured: five products and four sums)
                out = H.ggml_add(g.ctx, out, H.ggml_mul_mat_id(g.ctx, as_t, bt, idt))
            gf = H.ggml_new_graph_custom(g.ctx, 64, False)
            H.ggml_set_output(out)
            H.ggml_build_forward_expand(gf, out)
            g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
            assert g.buf
            for t, raw in g.inputs:
                H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            n0, res = backend.stat("graph_launches"), []
            for ids in idss:
                H.ggml_backend_tensor_set(idt, ids.ctypes.data_as(C.c_void_p), 0, ids.nbytes)
                assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
                res.append(g.read(out).copy())
            runs[graphs] = (res, backend.stat("graph_launches") - n0)
        finally:
            backend.set_option("graphs", 1)
            backend.set_option("mmid_group", 1)
            g.free()
    assert runs[1][1] == 2 and runs[0][1] == 0, (runs[1][1], runs[0][1])
    assert not np.array_equal(runs[0][0][0], runs[0][0][1])
    for r1, r0 in zip(runs[1][0], runs[0][0]):
        assert np.array_equal(r1.view(np.uint32), r0.view(np.uint32))
