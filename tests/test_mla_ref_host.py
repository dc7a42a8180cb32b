"""The references of the MLA tests, checked on the CPU alone (tests/mla_ref.py; the GPU side is tests/test_gpu_mla.py).

 * the oracle's batched MUL_MAT over a 3-D quantised weight is bit-equal to its own per-head 2-D MUL_MATs — for the nine served formats, with r2 in {1, 2}, E in {1, 2}
   and b contiguous, permuted and as llama.cpp's permuted strided view: the per-head twin is a valid reference for what a backend computes head by head;
 * a WRONG twin (head hb % H in place of hb / r2; b's dims 1 and 2 taken for each other) misses the batched gate, NMSE <= 1e-10, by far more than 10 x: the gate can
   tell a wrong head or a wrong column from the right one;
 * the staged oracle reference of the whole block agrees with a float64 evaluation on de-quantised weights to the error of the 8-bit activation rows.
"""
import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import mla_ref as R

GATE = 1e-10  # the quantised MUL_MAT gate of tests/test_gpu_ops.py, which tests/test_gpu_mla.py applies to the batched node


def _shape(qt):
    return (256 if qt in R.KQUANTS else 64), 5, 2, 3  # K, N, H, M


def _oracle_pair(qt, r2, E, layout, **twin):
    """(batched result [E, Hb, M, N], per-head twin assembled the same way) from ONE oracle graph over the same tensors."""
    K, N, H, M = _shape(qt)
    if twin.get("swap"):
        M = H * r2  # (the swapped twin reads M columns along the head stride: inside b only when there are as many heads)
    rng = np.random.default_rng(1000 + 37 * qt + 5 * r2 + E + len(layout))
    W = R.head_weights(qt, K, N, H, rng)
    X = rng.standard_normal((E, H * r2, M, K)).astype(np.float32)
    g = T.G("oracle")
    try:
        node, a, b = R.batched_node(g, qt, W, X, layout)
        ph = R.per_head_nodes(g, a, b, **twin)
        res = g.compute([node] + [n for _, n in ph], 2)
    finally:
        g.free()
    return res[0].reshape(E, H * r2, M, N), R.assemble([w for w, _ in ph], res[1:], E, H * r2, M, N), (W, X)


@pytest.mark.parametrize("qt", R.TYPES, ids=[R.NAMES[t] for t in R.TYPES])
def test_oracle_batched_mul_mat_is_bit_equal_to_its_per_head_2d_mul_mats(qt):
    for r2 in (1, 2):
        for E in (1, 2):
            for layout in ("contig", "permuted", "mla"):
                got, twin, (W, X) = _oracle_pair(qt, r2, E, layout)
                assert np.array_equal(R.bits(got), R.bits(twin)), (R.NAMES[qt], r2, E, layout)
                # ... and means what the contract says: close to the float64 product on de-quantised weights (8-bit activation rows: NMSE ~ 1e-4 at most)
                assert T.nmse(got, R.numpy_f64(qt, W, X, r2)) < 1e-3, (R.NAMES[qt], r2, E, layout)


@pytest.mark.parametrize("qt", (L.Q8_0, L.Q5_1, L.Q4_K), ids=["q8_0", "q5_1", "q4_K"])
def test_oracle_one_column_twin_is_bit_equal_too(qt):
    """A column's result does not depend on its neighbours: one node per (head, column) gives the same bits (the form of the GPU test's gate (b))."""
    got, twin, _ = _oracle_pair(qt, 2, 1, "mla", one_column=True)
    assert np.array_equal(R.bits(got), R.bits(twin))


@pytest.mark.parametrize("qt", (L.Q8_0, L.Q4_1, L.Q6_K), ids=["q8_0", "q4_1", "q6_K"])
def test_a_wrong_twin_misses_the_gate_by_more_than_ten_times(qt):
    r2 = 2
    H = _shape(qt)[2]
    wrong_head = _oracle_pair(qt, r2, 1, "contig", head_of=lambda hb: hb % H)
    swapped = _oracle_pair(qt, r2, 1, "contig", swap=True)
    for name, (got, twin, _) in (("head hb % H", wrong_head), ("columns and heads swapped", swapped)):
        e = T.nmse(twin, got)
        print(f"  {R.NAMES[qt]} wrong twin ({name}): NMSE {e:.3e} against the gate {GATE:.0e}")
        assert e >= 10 * GATE, (name, e)
    # (the right twin of the same tensors, for the record)
    got, twin, _ = _oracle_pair(qt, r2, 1, "contig")
    assert T.nmse(twin, got) == 0.0


# The floor of the block reference.  Every quantised product rounds its activation rows to 8 bits: a Q8_0 block of 32 N(0, s) values has amax ~ 2.5 s and a step of
# amax / 127, so a uniform rounding error of variance step^2 / 12 ~ 3e-5 s^2 (Q8_K, 256 values: amax ~ 3.3 s, 6e-5 s^2) — an NMSE of that size per product, three
# products in a chain (wk_b, wv_b, wo), the first of them through a soft-max whose logits have unit scale (a relative error of 0.6 % in a logit is 0.6 % in a
# probability), plus the f16 rounding of q in K.q (2^-11 relative: nothing beside it).  Together ~2e-4; the bound leaves a factor of five.
BLOCK_FLOOR = 1e-3


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("n_head,t_o", [(3, L.Q8_0), (4, L.Q4_K)], ids=["3heads-q8_0-wo", "4heads-q4_K-wo"])
def test_block_reference_against_float64(n_head, t_o, M):
    blk = R.MlaBlock(n_head=n_head, t_o=t_o, seed=7 + n_head)
    q, kvpe = blk.inputs(M, np.random.default_rng(70 + M))
    ref = blk.reference(q, kvpe, 2)
    f64 = blk.numpy_f64(q, kvpe)
    e = T.nmse(ref, f64)
    print(f"  MLA block, {n_head} heads, M = {M}: staged oracle reference against float64 NMSE {e:.3e} (bound {BLOCK_FLOOR:.0e})")
    assert np.all(np.isfinite(ref)) and e <= BLOCK_FLOOR, e
