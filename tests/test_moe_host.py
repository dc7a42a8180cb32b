"""CPU tests of the mixture-of-experts ground work: the ggml_lite builders of the router / expert ops (upstream's result shapes, strides, op_params and
operand asserts) and the composite reference of tests/moe_ref.py against a direct NumPy de-quantise-and-multiply."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import moe_ref as M


def _op_number(H, name):
    for i in range(128):
        if H.ggml_op_name(i) == name.encode():
            return i
    raise KeyError(name)


def _f32(t, i):
    return np.array([t.contents.op_params[i]], dtype=np.int32).view(np.float32)[0]


def _ne(t):
    return list(t.contents.ne)


def _nb(t):
    return list(t.contents.nb)


def test_router_and_expert_builders_give_upstream_shapes_strides_and_op_params(H):
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        n_expert, n_used, n_tok, K, N = 8, 2, 5, 256, 512
        probs = H.ggml_new_tensor_2d(ctx, L.F32, n_expert, n_tok)
        for order in (L.SORT_ORDER_ASC, L.SORT_ORDER_DESC):
            s = H.ggml_argsort(ctx, probs, order)
            assert s.contents.op == _op_number(H, "ARGSORT") and s.contents.type == L.I32
            assert _ne(s) == [n_expert, n_tok, 1, 1] and _nb(s) == [4, 4 * n_expert, 4 * n_expert * n_tok, 4 * n_expert * n_tok]
            assert s.contents.op_params[0] == order
            assert C.addressof(s.contents.src[0].contents) == C.addressof(probs.contents)
        assert (L.SORT_ORDER_ASC, L.SORT_ORDER_DESC) == (0, 1)

        sel = H.ggml_top_k(ctx, probs, n_used)
        assert sel.contents.op == _op_number(H, "VIEW") and sel.contents.type == L.I32
        assert _ne(sel) == [n_used, n_tok, 1, 1]
        assert _nb(sel)[0] == 4 and _nb(sel)[1] == n_expert * 4, "the top-k view keeps the stride of ARGSORT's rows"
        srt = sel.contents.view_src
        assert srt.contents.op == _op_number(H, "ARGSORT") and srt.contents.op_params[0] == L.SORT_ORDER_DESC and sel.contents.view_offs == 0

        sm = H.ggml_sum_rows(ctx, probs)
        assert sm.contents.op == _op_number(H, "SUM_ROWS") and sm.contents.type == L.F32 and _ne(sm) == [1, n_tok, 1, 1]

        cl = H.ggml_clamp(ctx, sm, 6.103515625e-5, float("inf"))
        assert cl.contents.op == _op_number(H, "CLAMP") and _ne(cl) == _ne(sm) and _nb(cl) == _nb(sm)
        assert C.addressof(cl.contents.view_src.contents) == C.addressof(sm.contents), "ggml_clamp works in place (a view of its operand)"
        assert _f32(cl, 0) == np.float32(6.103515625e-5) and np.isinf(_f32(cl, 1))

        for qt in (L.Q4_K, L.Q8_0, L.F16):
            as_t = H.ggml_new_tensor_3d(ctx, qt, K, N, n_expert)
            for rows in (1, n_used):
                b = H.ggml_new_tensor_3d(ctx, L.F32, K, rows, n_tok)
                r = H.ggml_mul_mat_id(ctx, as_t, b, sel)
                assert r.contents.op == _op_number(H, "MUL_MAT_ID") and r.contents.type == L.F32
                assert _ne(r) == [N, n_used, n_tok, 1] and _nb(r) == [4, 4 * N, 4 * N * n_used, 4 * N * n_used * n_tok]
                for k, t in enumerate((as_t, b, sel)):
                    assert C.addressof(r.contents.src[k].contents) == C.addressof(t.contents)
        # the op numbers the backend switches on are the header's
        assert [_op_number(H, n) for n in ("SUM_ROWS", "MUL_MAT_ID", "CLAMP", "ARGSORT")] == [H_OP[n] for n in ("SUM_ROWS", "MUL_MAT_ID", "CLAMP", "ARGSORT")]
    finally:
        H.ggml_free(ctx)


def _header_ops():
    ops, on = [], False
    with open(os.path.join(L.REPO, "include", "ggml_abi.h")) as f:
        for line in f:
            s = line.strip()
            if s.startswith("enum ggml_op {"):
                on = True
            elif on and s.startswith("}"):
                break
            elif on and s.startswith("GGML_OP_"):
                ops.append(s.split(",")[0].split("=")[0].strip()[len("GGML_OP_"):])
    return {n: i for i, n in enumerate(ops)}


H_OP = _header_ops()

_MALFORMED = {
    "ids_not_i32": "H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.F32, 2, 5))",
    "as_4d": "H.ggml_mul_mat_id(ctx, H.ggml_new_tensor_4d(ctx, L.F16, 256, 64, 8, 2), b, ids)",
    "b_4d": "H.ggml_mul_mat_id(ctx, as_t, H.ggml_new_tensor_4d(ctx, L.F32, 256, 1, 5, 2), ids)",
    "ids_3d": "H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_3d(ctx, L.I32, 2, 5, 2))",
    "token_count": "H.ggml_mul_mat_id(ctx, as_t, b, H.ggml_new_tensor_2d(ctx, L.I32, 2, 4))",
    "inner_dim": "H.ggml_mul_mat_id(ctx, as_t, H.ggml_new_tensor_3d(ctx, L.F32, 512, 1, 5), ids)",
    "slot_broadcast": "H.ggml_mul_mat_id(ctx, as_t, H.ggml_new_tensor_3d(ctx, L.F32, 256, 3, 5), H.ggml_new_tensor_2d(ctx, L.I32, 4, 5))",
    "as_transposed": "H.ggml_mul_mat_id(ctx, H.ggml_transpose(ctx, H.ggml_new_tensor_3d(ctx, L.F32, 64, 256, 8)), b, ids)",
    "top_k_too_wide": "H.ggml_top_k(ctx, H.ggml_new_tensor_2d(ctx, L.F32, 8, 5), 9)",
    "sort_order": "H.ggml_argsort(ctx, H.ggml_new_tensor_2d(ctx, L.F32, 8, 5), 2)",
}


@pytest.mark.parametrize("case", sorted(_MALFORMED))
def test_builders_refuse_malformed_operands(built, case):
    """The builders assert like upstream's (an abort with the failed condition on stderr): checked in a child process."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {L.REPO!r})
        import llama_box_amd as L
        H = L.host()
        ctx = H.ggml_init(L.InitParams(0, None, True))
        as_t = H.ggml_new_tensor_3d(ctx, L.F16, 256, 64, 8)
        b = H.ggml_new_tensor_3d(ctx, L.F32, 256, 1, 5)
        ids = H.ggml_new_tensor_2d(ctx, L.I32, 2, 5)
        ok = H.ggml_mul_mat_id(ctx, as_t, b, ids)
        print("well-formed ok", flush=True)
        {_MALFORMED[case]}
        print("malformed accepted", flush=True)
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "well-formed ok" in r.stdout, r.stderr
    assert "malformed accepted" not in r.stdout and r.returncode != 0, (r.returncode, r.stdout)
    assert "assertion failed" in r.stderr, r.stderr


def _routing(rng, n_tok, n_used, n_expert):
    return np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)


@pytest.mark.parametrize("qtype", [L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0, L.F16], ids=["q4_K", "q5_K", "q6_K", "q8_0", "f16"])
@pytest.mark.parametrize("rows_per_slot", [False, True], ids=["broadcast", "per-slot"])
def test_composite_reference_matches_numpy_dequantise_and_multiply(built, qtype, rows_per_slot):
    """The composite reference (oracle MUL_MATs over 2-D expert views, ids from NumPy) against float64 products of the de-quantised experts with the
    UNQUANTISED activations.  Distance, not bits: the oracle quantises the activations to 8 bits — a step of amax / 127 per block, amax ~ 3 sigma for N(0, 1) rows, so an NMSE
    of (3 / 127)^2 / 12 ~ 4.6e-5 (measured 2.7e-5 .. 5.9e-5); the bound is ten times that.  f16 experts round the activations to f16 on both sides, leaving the f32 result rounding."""
    rng = np.random.default_rng(11)
    K, N, n_expert, n_used, n_tok = 512, 96, 6, 2, 7
    W = M.expert_weights(qtype, K, N, n_expert, rng)
    ids = _routing(rng, n_tok, n_used, n_expert)
    b = rng.standard_normal((n_tok, n_used if rows_per_slot else 1, K)).astype(np.float32)
    ref = M.mmid_reference(qtype, W, K, N, [(b, ids)], 4)[0]
    f64 = M.mmid_numpy(qtype, W, K, b, ids)
    e = T.nmse(ref, f64)
    print(f"composite reference vs NumPy f64: nmse={e:.3e}")
    assert e <= (1e-12 if qtype == L.F16 else 5e-4)
    # one MUL_MAT per expert over its pairs' columns is, column by column, the one-column product per (slot, token)
    lit = M.mmid_reference(qtype, W, K, N, [(b, ids)], 4, grouped=False)[0]
    assert np.array_equal(ref.view(np.uint32), lit.view(np.uint32))


def test_composite_block_reference_matches_numpy_f64(built):
    """The whole-block reference against the block in float64 on de-quantised weights with the same routing: the floor the GPU gate (NMSE <= 1e-9
    against the COMPOSITE reference) is not allowed to hide behind — this distance is the 8-bit activation quantisation of three chained products."""
    blk = M.MoeBlock(256, 512, 8, 2, L.Q4_K, L.Q6_K, False, 5)
    x = blk.router_inputs(6, np.random.default_rng(2))
    out, ids, probs = blk.reference(x, 4)
    srt = np.sort(probs, axis=1)[:, ::-1]
    assert np.all(srt[:, 1] - srt[:, 2] > 1e-3 * srt[:, 1])
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-5)
    f64 = blk.numpy_f64(x, ids)
    e = T.nmse(out, f64)
    print(f"block reference vs NumPy f64: nmse={e:.3e}")
    assert e <= 5e-3


# ------------------------------------------------------------------------------------------------ helpers of tests/test_gpu_moe_edges.py
def test_kernel_selection_thresholds_are_read_from_the_source(built):
    """moe_ref.mmid_limits parses every threshold out of launch_mmid / launch_mmid_t / mm_id_ok; the shapes derived from them sit on the right side of each."""
    lim = M.mmid_limits()
    print(f"mmid limits: {lim}")
    assert lim["r2_min"] > 0 and lim["pair_max"] > 0 and lim["vec_align"] in (4, 8, 16, 32) and lim["vec_k"] >= 2
    for qt in (L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0):
        K = M.lds_free_k(qt, lim)
        per = lim["act_bytes"]["q8_0" if qt == L.Q8_0 else "q8_K"]
        nblk = K // L.TYPE_BLCK[qt]
        print(f"  type {qt}: the LDS-free form starts at K = {K} ({nblk} activation blocks of {per} bytes)")
        assert K % L.TYPE_BLCK[qt] == 0 and nblk * per > lim["lds_max"] >= (nblk - 1) * per


@pytest.mark.parametrize("qtype", [L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0], ids=["q4_K", "q5_K", "q6_K", "q8_0"])
@pytest.mark.parametrize("K", [512, 1536])
def test_readout_experts_oracle_equals_the_numpy_twin(built, qtype, K):
    """The CPU half of the exact read-back through MUL_MAT_ID: the composite oracle over the stacked, rotated read-out experts equals the NumPy twin of the
    activation quantiser bit for bit (+-0 equal, NaN where the twin has NaN) — one row per (slot, token) and one row per token, 1 / 3 / 32 tokens."""
    import probes as P
    for what in ("values", "bsums") if qtype in (L.Q4_K, L.Q5_K) else ("values",):
        for per_slot in (True, False):
            cases = [M.readout_case(qtype, K, n_tok, per_slot, what) for n_tok in (1, 3, 32)]
            W = cases[0][0]
            ref = M.mmid_reference(qtype, W, K, W.shape[1], [(b, ids) for _, b, ids, _ in cases], 4)
            for (_, b, ids, want), r in zip(cases, ref):
                bad = P.bits(r) != P.bits(want)
                assert not bad.any(), f"{what} per_slot={per_slot} n_tokens={ids.shape[0]}: {int(bad.sum())}/{bad.size} outputs differ; first at {np.argwhere(bad)[0].tolist()}"
    # the rotation tells the experts apart: another expert's read-out of the same row is a different vector
    W, b, ids, want = M.readout_case(qtype, K, 3, True)
    _, shifts = M.readout_experts(qtype, K, 4)
    wrong = M.expected_expert_readout(qtype, b, (ids + 1) % 4, shifts)
    assert all((P.bits(wrong[t, s]) != P.bits(want[t, s])).any() for t in range(3) for s in range(2))


SHARED_LAYERS = {
    # routed up / gate, routed down, shared up / gate, shared down
    "q4_K+q6_K": (L.Q4_K, L.Q6_K, L.Q4_K, L.Q6_K),
    "q8_0": (L.Q8_0, L.Q8_0, L.Q8_0, L.Q8_0),
    "routed-q4_K-shared-q8_0": (L.Q4_K, L.Q4_K, L.Q8_0, L.Q8_0),
}


@pytest.mark.parametrize("name", sorted(SHARED_LAYERS))
def test_shared_expert_layer_reference_matches_numpy_f64_and_its_two_orders_differ(built, name):
    """SharedExpertLayer.reference (oracle ops + NumPy glue) against the layer in float64 on de-quantised weights; and the two build orders give
    different node lists with the same multiset of ops."""
    tu, td, su, sd = SHARED_LAYERS[name]
    lay = M.SharedExpertLayer(512, 768, 1024, 8, 2, tu, td, su, sd, seed=3)
    x = lay.inputs(5, np.random.default_rng(9))
    out, ids, probs, prods = lay.reference(x, 4)
    srt = np.sort(probs, axis=1)[:, ::-1]
    assert np.all(srt[:, 1] - srt[:, 2] > 1e-3 * srt[:, 1])
    e = T.nmse(out, lay.numpy_f64(x, ids))
    print(f"shared-expert layer {name}: reference vs NumPy f64 nmse = {e:.3e}")
    assert e <= 5e-3
    assert [p.shape for p in prods] == [(5, 2, 768), (5, 2, 768), (5, 2, 512)]
    ops = {}
    for order in lay.ORDERS:
        g = T.G("oracle")
        try:
            o, sel, _, _, first = lay.build(g, x, order)
            ops[order] = M.node_ops(g, [o, sel], first)
        finally:
            g.free()
    a, b, c = (ops[o] for o in lay.ORDERS)
    mm, mmid = _op_number(L.host(), "MUL_MAT"), _op_number(L.host(), "MUL_MAT_ID")
    assert a != b and sorted(a) == sorted(b)
    first_of = lambda seq, op: seq.index(op)  # noqa: E731
    # routed_first: the router MUL_MAT, then the three MUL_MAT_IDs, then the dense chain; shared_first: the three dense MUL_MATs before the first MUL_MAT_ID
    assert [o for o in a if o in (mm, mmid)] == [mm, mmid, mmid, mmid, mm, mm, mm]
    assert [o for o in b if o in (mm, mmid)] == [mm, mm, mm, mm, mmid, mmid, mmid]
    # shared_up_gate_first: the dense gate and up products, the router, the MUL_MAT_IDs directly behind it, the dense down product last
    assert [o for o in c if o in (mm, mmid)] == [mm, mm, mm, mmid, mmid, mmid, mm] and sorted(c) == sorted(a)
    assert first_of(a, mmid) < len(a) and first_of(b, mmid) > first_of(b, mm)
