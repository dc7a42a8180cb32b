"""MUL_MAT_ID over MXFP4 experts, the grouped matrix-core form (csrc/mmid_group_mxfp4.hip), recognised by its timing class: against the twin of tests/mxfp4_ref.py, exact
products, batch invariance, ADD_ID in the store, the default's routing and a captured graph.  The routing is test_gpu_moe_grouped.py's: 40 tokens x 2 slots over 6 experts."""
import ctypes as C
import re

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as M
import mxfp4_ref as R

pytestmark = pytest.mark.gpu
N_EXPERT, N_USED, N_TOK, GRP, PAIR = 6, 2, 40, "mmid_grp_mxfp4", "mmid_mxfp4"


def _routing(rng):
    ids = np.zeros((N_TOK, N_USED), np.int32)
    ids[:32, 1], ids[32, 1], ids[33:38, 1], ids[38, 1], ids[39, 1] = 1, 2, rng.integers(4, 6, 5), -1, N_EXPERT
    return ids[rng.permutation(N_TOK)]


def _set(backend, **opts):
    for k, v in opts.items():
        backend.set_option(k, v)


def _compute(backend, build, group, mmid_bias=1):
    g = T.G(backend)
    try:
        _set(backend, mmid_group=group, timing=1, mmid_bias=mmid_bias)
        backend.timing_report()
        res = M.compute_in_weights_buffer(g, build(g))
        return res, {k: v[0] for k, v in backend.timing_report().items() if v[0] and (k.startswith("mmid") or k == "add_id")}
    finally:
        _set(backend, timing=0, mmid_group=1, mmid_bias=1)
        g.free()


def _node(g, W, b, ids, strided=True):
    idt = M.strided_ids(g, ids, N_EXPERT) if strided else g.new(L.I32, list(ids.shape[::-1]), ids)
    return g.H.ggml_mul_mat_id(g.ctx, g.new(R.QT, [b.shape[2], W.shape[1], W.shape[0]], W), g.new(L.F32, list(b.shape[::-1]), np.ascontiguousarray(b)), idt), idt


def _experts(K, N, rng, e=None):
    W = np.stack([R.rand_weight(K, N, rng) for _ in range(N_EXPERT)])
    if e is not None:  # (the block scales in a band of powers of two)
        W.reshape(N_EXPERT, N, K // 32, R.BS)[..., 0] = rng.integers(e[0], e[1] + 1, (N_EXPERT, N, K // 32))
    return W


# (32, 32): one block, seven waves without one, rows at 17-byte steps; (160, 96): five blocks, 85-byte rows at odd addresses; (2880, 64): 90 blocks, an uneven split.  exact: scales
# 1/2 and 1, integer activations with 127 in every block (Q8_0 exact, d = 1): every partial sum is a multiple of 1/2 below 90 * 32 * 12 * 127 < 2^23: any order gives the twin's bits
@pytest.mark.parametrize("K,N,per_slot,exact", [(k, n, p, x) for k, n in ((32, 32), (160, 96), (2880, 64)) for p in (False, True) for x in (False, True)])
def test_grouped_form_matches_the_twin(backend, plog, K, N, per_slot, exact):
    rng = np.random.default_rng(K + N + per_slot)
    W = _experts(K, N, rng, (127, 128) if exact else None)
    b = (rng.integers(-127, 128, (N_TOK, 1 + per_slot, K)) if exact else rng.standard_normal((N_TOK, 1 + per_slot, K))).astype(np.float32)
    if exact:
        b[..., ::32] = 127.0
        y = R.quantize_q80(b.reshape(-1, K))
        assert (y["d"] == 1).all() and np.array_equal(y["qs"].reshape(b.shape), b) and (K // 32) * 32 * 12 * 127 < 2 ** 23
    bad = ((ids := _routing(rng)) < 0) | (ids >= N_EXPERT)
    assert bad.sum() == 2 and [int((ids == e).sum()) for e in range(4)] == [40, 32, 1, 0]
    (strided, contig), classes = _compute(backend, lambda g: [_node(g, W, b, ids)[0], _node(g, W, b, ids, strided=False)[0]], 2)
    strided, contig = strided.reshape(N_TOK, N_USED, N), contig.reshape(N_TOK, N_USED, N)
    assert classes == {GRP: 2} and np.array_equal(R.bits(strided), R.bits(contig)), classes
    T.compare(f"mul_mat_id grouped mxfp4 K={K} N={N} per_slot={per_slot} exact={exact}", strided[~bad], (ref := R.mul_mat_id(W, b, ids))[~bad], 1e-10, log=plog)
    assert not strided[bad].any() and np.count_nonzero(strided[~bad]) > strided[~bad].size // 2 and (not exact or np.array_equal(R.bits(strided), R.bits(ref)))


def test_a_pairs_result_does_not_depend_on_the_batch(backend):
    """The 40-token node, a node over its first five tokens (10 pairs: other tiles) and one with the tokens reversed: every shared (slot, token) column is bit-equal."""
    K, N, rng = 2880, 64, np.random.default_rng(7)
    W, b, ids = _experts(K, N, rng), rng.standard_normal((N_TOK, N_USED, K)).astype(np.float32), _routing(rng)
    (full, head, rev), classes = _compute(backend, lambda g: [_node(g, W, x, np.ascontiguousarray(i))[0] for x, i in ((b, ids), (b[:5], ids[:5]), (b[::-1], ids[::-1]))], 2)
    assert classes == {GRP: 3}, classes
    assert np.array_equal(R.bits(head.reshape(5, N_USED, N)), (full := R.bits(full.reshape(N_TOK, N_USED, N)))[:5]) and np.array_equal(R.bits(rev.reshape(N_TOK, N_USED, N)), full[::-1])


def test_add_id_rides_in_the_grouped_store(backend):
    """mmid_group 2: with mmid_bias 1 the bias is added in the grouped store (one fused node more, no add_id launch), bit-equal to mmid_bias 0; bad-id pairs are zeros."""
    N, rng = 96, np.random.default_rng(31)
    W, b, ids, bias = _experts(160, N, rng), rng.standard_normal((N_TOK, 1, 160)).astype(np.float32), _routing(rng), rng.standard_normal((N_EXPERT, N)).astype(np.float32)

    def build(g):
        mm, sel = _node(g, W, b, ids)
        return [g.H.ggml_add_id(g.ctx, mm, g.new(L.F32, [N, N_EXPERT], bias), sel)]

    res = {}
    for mode in (1, 0):
        f0 = backend.stat("fused_nodes")
        (r,), classes = _compute(backend, build, 2, mmid_bias=mode)
        assert classes == ({GRP: 1} if mode else {GRP: 1, "add_id": 1}), classes
        res[mode] = (r.reshape(N_TOK, N_USED, N), backend.stat("fused_nodes") - f0)
    assert res[1][1] - res[0][1] == 1 and np.array_equal(R.bits(res[1][0]), R.bits(res[0][0]))
    assert not res[1][0][(ids < 0) | (ids >= N_EXPERT)].any() and res[1][0][(ids >= 0) & (ids < N_EXPERT)].all()


def test_the_default_routes_by_pair_count(backend):
    """mmid_group 1: 32 pairs keep the pair form, MI_MMID_GROUP_MXFP4_MIN_PAIRS pairs take the grouped one; mmid_group 0: nobody does; mmid_group 2: N = 33 keeps the pair form."""
    with open(L.REPO + "/llama_box_amd/csrc/kernels.h") as f:
        (big,) = map(int, re.findall(r"#define MI_MMID_GROUP_MXFP4_MIN_PAIRS (\d+)", f.read()))
    assert big >= 128
    rng = np.random.default_rng(11)
    for group, n_tok, N, want in ((1, 32, 64, PAIR), (1, big, 64, GRP), (0, big, 64, PAIR), (2, big, 33, PAIR)):
        W, b, ids = _experts(160, N, rng), rng.standard_normal((n_tok, 1, 160)).astype(np.float32), rng.integers(0, N_EXPERT, (n_tok, 1)).astype(np.int32)
        _, classes = _compute(backend, lambda g: [_node(g, W, b, ids)[0]], group)
        assert classes == {want: 1}, (group, n_tok, N, classes)


def test_a_captured_graph_follows_new_ids_on_replay(backend):
    """The forced-form node computed three times, other ids uploaded in between: computes two and three replay the captured hipGraph, bit-equal to eager runs over the same ids."""
    rng = np.random.default_rng(21)
    W, b, idss, H, runs = _experts(160, 96, rng), rng.standard_normal((N_TOK, 1, 160)).astype(np.float32), [_routing(rng) for _ in range(3)], L.host(), {}
    for graphs in (1, 0):
        g = T.G(backend)
        try:
            _set(backend, mmid_group=2, graphs=graphs)
            idt, as_t, bt = g.new(L.I32, [N_USED, N_TOK], idss[0]), g.new(R.QT, [160, 96, N_EXPERT], W), g.new(L.F32, [160, 1, N_TOK], b)
            out = H.ggml_mul_mat_id(g.ctx, as_t, bt, idt)
            for _ in range(4):  # (graphs of fewer than eight nodes are not captured: five products and four sums)
                out = H.ggml_add(g.ctx, out, H.ggml_mul_mat_id(g.ctx, as_t, bt, idt))
            n0, res = backend.stat("graph_launches"), [g.compute([out])[0].copy()]
            for ids in idss[1:]:
                H.ggml_backend_tensor_set(idt, ids.ctypes.data_as(C.c_void_p), 0, ids.nbytes)
                assert H.ggml_backend_graph_compute(backend.backend, g.gf) == 0
                res.append(g.read(out).copy())
            runs[graphs] = (res, backend.stat("graph_launches") - n0)
        finally:
            _set(backend, graphs=1, mmid_group=1)
            g.free()
    assert runs[1][1] == 2 and runs[0][1] == 0 and not np.array_equal(runs[0][0][0], runs[0][0][1]), (runs[1][1], runs[0][1])
    assert all(np.array_equal(R.bits(r1), R.bits(r0)) for r1, r0 in zip(runs[1][0], runs[0][0]))
