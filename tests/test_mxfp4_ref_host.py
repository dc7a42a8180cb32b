"""CPU-side tests for the gpt-oss expert block's references: the NumPy twin of tests/mxfp4_ref.py against known-answer blocks written out by hand from the format
(a byte pattern and the values it must decode to, no code shared with the twin), its integer vec_dot against the float64 dot of the dequantised operands, and
add_id / swiglu_oai against per-element restatements."""
import math
import os
import re
import struct

import numpy as np
import pytest

import llama_box_amd as L
import mxfp4_ref as R

f32 = np.float32


def _bits(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def test_type_tables_know_the_layout():
    H = L.host()
    assert L.MXFP4 == 39 and L.TYPE_NAME[L.MXFP4] == "mxfp4"
    assert (L.TYPE_BLCK[L.MXFP4], L.TYPE_SIZE[L.MXFP4]) == (32, 17)
    assert H.ggml_row_size(L.MXFP4, 2880) == 90 * 17 == 1530  # (ggml_abi.h's tables, through the host library)
    src = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "ggml_abi.h")).read()
    assert re.search(r"case GGML_TYPE_MXFP4: return 17;", src) and re.search(r"GGML_TYPE_MXFP4 = 39", src)
    ctx = H.ggml_init(L.InitParams(0, None, True))
    try:
        t = H.ggml_new_tensor_3d(ctx, L.MXFP4, 64, 3, 2)
        assert H.ggml_nbytes(t) == 2 * 3 * 2 * 17 and t.contents.nb[1] == 34 and t.contents.nb[2] == 102
    finally:
        H.ggml_free(ctx)


# (e, the byte every qs[j] holds, values 0 .. 15, values 16 .. 31) — worked out by hand: low nibble first, table {0,1,2,3,4,6,8,12 | 0,-1,-2,-3,-4,-6,-8,-12},
# scale = 2^(e - 128)
KNOWN = [
    (127, 0x71, 0.5, 6.0),                         # codes 1 / 7 at scale 0.5: 1 * 0.5, 12 * 0.5
    (128, 0xF9, -1.0, -12.0),                      # codes 9 / 15 at scale 1
    (126, 0x2A, -0.5, 0.5),                        # codes 10 (-2) / 2 at scale 0.25
    (0, 0x21, _bits(0x00200000), _bits(0x00400000)),   # codes 1 / 2 at the smaller subnormal scale 2^-128: 2^-128 and 2^-127
]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: f"e{c[0]}_qs{c[1]:02x}")
def test_twin_dequantize_matches_known_answer_block(case):
    e, byte, lo, hi = case
    raw = np.array([e] + [byte] * 16, dtype=np.uint8)
    got = R.dequantize(raw[None], 32)[0]
    want = np.array([lo] * 16 + [hi] * 16, dtype=f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_scale_bits_at_the_bottom_of_the_range():
    assert R.scale_f32(np.array([0, 1, 2, 3, 127, 128, 254])).view(np.uint32).tolist() == [0x00200000, 0x00400000, 0x00800000, 0x01000000, 126 << 23, 127 << 23, 253 << 23]
    assert R.scale_f32(np.array([127]))[0] == 0.5 and R.scale_f32(np.array([128]))[0] == 1.0 and R.scale_f32(np.array([2]))[0] == 2.0 ** -126


def test_code_8_decodes_to_positive_zero():
    got = R.dequantize(np.array([130] + [0x88] * 16, dtype=np.uint8)[None], 32)[0]
    assert np.array_equal(got.view(np.uint32), np.zeros(32, dtype=np.uint32))


def test_ramp_block_checks_the_nibble_order():
    """qs[j] = j | (15 - j) << 4: values 0 .. 15 are table[j], values 16 .. 31 table[15 - j]"""
    raw = np.array([128] + [j | ((15 - j) << 4) for j in range(16)], dtype=np.uint8)
    table = [0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12]
    want = np.array([table[j] for j in range(16)] + [table[15 - j] for j in range(16)], dtype=f32)
    assert np.array_equal(R.dequantize(raw[None], 32)[0], want)
    u = R.unpack(raw[None], 32)
    assert u["nibble"][0, 0].tolist() == list(range(16)) + list(range(15, -1, -1))


def test_packer_is_inverted_by_the_twin():
    rng = np.random.default_rng(39)
    nib, e = rng.integers(0, 16, (50, 32)), rng.integers(0, 256, 50)
    u = R.unpack(R.make_blocks(e, nib), 32)
    assert np.array_equal(u["nibble"][:, 0], nib) and np.array_equal(u["e"][:, 0], e) and np.array_equal(u["value"][:, 0], R.KVALUES[nib])
    full = R.unpack(R.rand_weight(2880, 4, rng), 2880)
    assert set(full["nibble"].reshape(-1).tolist()) == set(range(16)) and full["nibble"].shape == (4, 90, 32)
    edge = R.unpack(R.edge_blocks(600, rng), 32)
    assert set(edge["e"].reshape(-1).tolist()) == set(R.EDGE_E) and max(R.EDGE_E) <= 250


@pytest.mark.parametrize("K", [32, 160, 2880])
def test_vec_dot_equals_the_float64_dot_of_the_dequantised_operands(K):
    """The twin's MUL_MAT is the f64 dot of dequantize(W) with the dequantised Q8_0 activations up to f32 rounding of the block terms (NMSE ~1e-14)."""
    rng = np.random.default_rng(K)
    W = R.rand_weight(K, 7, rng)
    X = rng.standard_normal((3, K)).astype(f32)
    got = R.mul_mat(W, X)
    want = R.dequantize_q80(R.quantize_q80(X)) @ R.dequantize(W, K).astype(np.float64).T
    assert got.shape == (3, 7) and np.any(want != 0)
    assert float(np.sum((got - want) ** 2) / np.sum(want ** 2)) <= 1e-12


def test_vec_dot_on_a_hand_block():
    """e = 128 (scale 1), code 2 (value 2) at column 5, everything else code 0, against x = 127 at column 5 (d_act = 1, q = 127): 2 * 127"""
    nib = np.zeros((1, 32), dtype=np.uint8)
    nib[0, 5] = 2
    x = np.zeros((1, 32), dtype=f32)
    x[0, 5] = 127.0
    assert R.mul_mat(R.make_blocks([128], nib), x)[0, 0] == 254.0


def test_mul_mat_id_picks_the_expert_and_zeroes_unknown_ids():
    rng = np.random.default_rng(5)
    W = np.stack([R.rand_weight(64, 5, rng) for _ in range(3)])
    b = rng.standard_normal((2, 1, 64)).astype(f32)
    ids = np.array([[2, 0], [3, -1]], dtype=np.int32)
    out = R.mul_mat_id(W, b, ids)
    assert np.array_equal(out[0, 0], R.mul_mat(W[2], b[0])[0]) and np.array_equal(out[0, 1], R.mul_mat(W[0], b[0])[0])
    assert not out[1].any()


def test_add_id_against_a_per_element_restatement():
    rng = np.random.default_rng(6)
    a = rng.standard_normal((3, 2, 5)).astype(f32)
    b = rng.standard_normal((4, 5)).astype(f32)
    ids = np.array([[0, 3], [2, 2], [4, -1]], dtype=np.int32)
    got = R.add_id(a, b, ids)
    for t in range(3):
        for s in range(2):
            for i in range(5):
                e = int(ids[t, s])
                want = f32(a[t, s, i] + b[e, i]) if 0 <= e < 4 else a[t, s, i]
                assert got[t, s, i] == want
    assert np.array_equal(got[2], a[2])  # (ids outside the experts add nothing)


def _oai_scalar(g, u, alpha, limit):
    """ggml-cpu's loop in Python floats rounded to f32 after every operation"""
    expf = R._libm().expf
    g, u, alpha, limit = float(f32(g)), float(f32(u)), float(f32(alpha)), float(f32(limit))
    x = limit if limit < g else g
    y = -limit if u < -limit else (limit if limit < u else u)
    with np.errstate(all="ignore"):
        e = f32(expf(float(f32(alpha) * f32(-x))))
        glu = f32(x) / f32(f32(1.0) + e)
        return f32(f32(glu) * f32(f32(y) + f32(1.0)))


def test_swiglu_oai_against_a_per_element_restatement():
    rng = np.random.default_rng(7)
    g = np.concatenate([rng.standard_normal(200) * 4, [7.0, 7.5, 100.0, -7.0, -30.0, -60.0, -100.0, np.inf, -np.inf, 0.0, -0.0]]).astype(f32)
    u = np.concatenate([rng.standard_normal(200) * 6, [8.0, -8.0, 7.0, -7.0, 0.0, 1.0, 2.0, 3.0, 4.0, np.inf, -np.inf]]).astype(f32)
    got = R.swiglu_oai(g, u, R.ALPHA, R.LIMIT)
    want = np.array([_oai_scalar(a, b, R.ALPHA, R.LIMIT) for a, b in zip(g, u)], dtype=f32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    # the named corners
    one = lambda a, b: R.swiglu_oai(np.array([a], f32), np.array([b], f32), R.ALPHA, R.LIMIT)[0]  # noqa: E731
    assert one(100.0, 1.0) == one(7.0, 1.0) and one(7.5, 1.0) == one(7.0, 1.0)          # g > limit
    assert one(1.0, 100.0) == one(1.0, 7.0) and one(1.0, -100.0) == one(1.0, -7.0)      # |u| > limit
    assert one(np.inf, 1.0) == one(7.0, 1.0) and math.isnan(one(-np.inf, 1.0))          # g = +-inf: the clamp; -inf / inf
    z = one(-100.0, 1.0)                                                               # expf overflows: -100 / inf = -0.0
    assert z == 0.0 and np.signbit(z)
    assert math.isnan(one(np.nan, 1.0)) and math.isnan(one(1.0, np.nan))
    assert one(1.0, 0.0) == f32(f32(1.0) / f32(f32(1.0) + f32(R._libm().expf(float(f32(R.ALPHA) * f32(-1.0))))))


def test_block_reference_against_its_float64_floor():
    """The composed twin of the gpt-oss expert block against the same block in float64 on de-quantised weights: what the 8-bit activations cost, nothing more."""
    blk = R.GptOssBlock(160, 96, 8, 2, seed=11)
    x = blk.router_inputs(5, np.random.default_rng(12))
    out, ids = blk.reference(x)
    assert out.shape == (5, 160) and ids.shape == (5, 2) and np.all(np.isfinite(out))
    floor = float(np.sum((out - blk.numpy_f64(x, ids)) ** 2) / np.sum(blk.numpy_f64(x, ids) ** 2))
    assert floor <= 5e-3, floor
