"""CPU: the NumPy twins of tests/ops_ref.py against the C oracle, on the inputs of tests/test_gpu_ops_edges.py — the two references are pinned to each
other before either judges a kernel.  Bit-exact ops: twin == oracle as uint32 / uint16 (NaNs by isnan).  Distance ops: the oracle's largest distance
from the float64 twin is the BASELINE the GPU gates start from (ops_ref.gate); here it is printed and held against what f32 arithmetic and a libm
within one ulp can be from the exact value.  And the launcher constants the edge shapes are derived from are still the ones in csrc/ops.hip."""
import numpy as np
import pytest

import ops_ref as R

CASES = R.all_cases()
# What the ORACLE itself may be from the float64 twin: the operations of each definition, half an ulp apiece where they are correctly rounded, one ulp for
# a libm call, a relative error r counted as r / 2^-24 ulps of the result (ops_ref.U24).
#   rms_norm  mean, mean + eps, sqrtf (halved), reciprocal, x * scale, * w: <= 0.5 + 0.5 + 0.25 + 0.5 + 0.5 + 0.5 = 2.75 relative half-steps of 2^-23 -> 5.5 ulps
#   exp       one libm call, under 1 ulp
#   tanh      glibc's own ulps table gives tanhf 2 (from the correctly rounded value): 2.5 from the exact one
#   sigmoid / silu   expf (2 * 2^-24), 1 + e and the quotient (2^-24 each): 4 ulps; swiglu one more product: 5 ulps
#   soft_max  expf, the f32 reciprocal of the sum and the product: 2^-23 + 2^-24 + 2^-24 = 2^-22 of the row's maximum
#   rope      libm cos / sin (2^-23 of mscale each, times up to max|x| each), two products and a sum: (2 + 1.5) * 2^-23 of the row's largest |x|;
#             f16 data: half an f16 ulp of a result that may reach sqrt(2) times the largest |x|, sqrt(2) * 2^-11, on top
ORACLE_OWN = {"rms_norm": 5.5, "exp": 1.0, "tanh": 2.5, "sigmoid": 4.0, "silu": 4.0, "swiglu": 5.0, "soft_max": 2.0 ** -22, "rope": 3.5 * 2.0 ** -23, "rope_f16": 2.0 ** -10.5 + 3.5 * 2.0 ** -23,
              "rope_yarn": 4.5 * 2.0 ** -23}


@pytest.fixture(scope="module")
def oracle_built(built):
    return built


def test_edge_shapes_follow_the_launcher_constants():
    lim = R.ops_limits()
    want = R.shapes_from(lim)
    assert R.SOFTMAX_N == want["SOFTMAX_N"], f"launch_soft_max hands over at {lim['softmax_reg']}: SOFTMAX_N is stale"
    assert all(R.STRIDE_N == n for n in want["STRIDE_N"].values()), f"grid caps {lim['grid_cap']}: STRIDE_N no longer takes a second, partial stride"
    assert R.CPY_STRIDE_N == want["CPY_STRIDE_N"], f"launch_cpy's grid cap is {lim['grid_cap']['cpy']}: CPY_STRIDE_N is stale"
    assert R.RMS_NE0 == want["RMS_NE0"], f"a float4 trip of k_rms_norm covers {lim['vec_trip']} values: RMS_NE0 is stale"
    assert R.GLU_NC == want["GLU_NC"], f"a k_swiglu chunk is {lim['glu_chunk']} values: GLU_NC is stale"
    assert R.SET_ROWS_NC == want["SET_ROWS_NC"], f"a float4 trip of k_set_rows covers {lim['vec_trip']} values: SET_ROWS_NC is stale"


def test_ulp_distance_and_catalogue():
    f = np.float32
    one = f(1.0)
    assert R.ulp_distance(np.nextafter(one, f(2)), 1.0) == 1.0 and R.ulp_distance(np.nextafter(one, f(0)), 1.0) == 0.5
    assert R.ulp_distance(f(0.0), 2.0 ** -149) == 1.0 and R.ulp_distance(f(2.0 ** -149), 0.0) == 1.0 and R.ulp_distance(f(-3.7e-42), -0.0) > 2000
    assert R.ulp_distance(f(1e-7), 0.0) > 1e37 and R.ulp_distance(f(0.0), 0.0) == 0.0 and R.ulp_distance(f(-0.0), -0.0) == 0.0
    assert R.ulp_distance(f(-0.0), 0.0) == np.inf and R.ulp_distance(f(0.0), -0.0) == np.inf  # the sign of an exact zero counts
    assert R.ulp_distance(f(-0.0), 1e-60) < 1e-10  # (an underflowed reference is not an exact zero)
    assert R.ulp_distance(f(np.inf), 1e39) == 0.0 and R.ulp_distance(f(np.nan), np.nan) == 0.0
    assert R.ulp_distance(f(np.inf), 1.0) == np.inf and R.ulp_distance(f(1.0), np.nan) == np.inf and R.ulp_distance(f(np.nan), 1.0) == np.inf
    cat = R.catalogue()
    h = R.cast(cat, np.float16)
    for v, bits in ((65504.0, 0x7BFF), (65520.0, 0x7C00), (2.0 ** -25, 0x0000), (1.5 * 2.0 ** -24, 0x0002), (2.5 * 2.0 ** -24, 0x0002), (1.0 + 2.0 ** -11, 0x3C00)):
        i = int(np.flatnonzero(cat == f(v))[0])
        assert int(h[i:i + 1].view(np.uint16)[0]) == bits, (v, hex(int(h[i:i + 1].view(np.uint16)[0])))
    below = int(np.flatnonzero(cat == np.nextafter(f(65520.0), f(0)))[0])
    assert int(h[below:below + 1].view(np.uint16)[0]) == 0x7BFF
    assert np.isnan(cat).sum() == 1 and np.isinf(cat).sum() == 2 and (np.abs(cat[cat != 0]) < R.FLT_MIN).sum() >= 4


def test_twins_on_known_answers():
    """Hand-computed values, so a twin that is wrong the way the oracle is wrong does not pass by agreement."""
    assert R.argmax(np.array([[1, 5, 5, 2], [np.nan, -1, -1, np.nan], [-np.inf] * 4], np.float32)).tolist() == [1, 1, 0]
    y = R.rms_norm(np.array([[3.0, 4.0]], np.float32), 0.0)
    assert np.allclose(y, [[3.0 / np.sqrt(12.5), 4.0 / np.sqrt(12.5)]], rtol=1e-15)
    assert np.all(R.rms_norm(np.full((1, 8), 1e20, np.float32), 1e-5) == 0.0)  # f32 squares overflow: infinite mean
    p = R.soft_max(np.array([[[[0.0, np.log(3.0)]]]], np.float32))
    assert np.allclose(p, [[[[0.25, 0.75]]]], rtol=1e-7)
    # a fully masked row: max = -inf, -inf - -inf = NaN, the sum is NaN and the guard makes it -inf — the row is NaN (what the guard prevents is the abort), a zero sum gives zeros
    assert np.all(np.isnan(R.soft_max(np.zeros((1, 1, 1, 4), np.float32), np.full((1, 4), -np.inf, np.float32))))
    s = R.alibi_slopes(6, 8.0)
    assert np.allclose(s, [0.25, 0.0625, 0.015625, 0.00390625, 0.5, 0.125], rtol=1e-7)
    r = R.rope(np.array([[[[1.0, 0.0, 1.0, 0.0]]]], np.float32), np.array([1], np.int32), 4, 0, 10000.0)
    assert np.allclose(r, [[[[np.cos(1.0), np.sin(1.0), np.cos(0.01), np.sin(0.01)]]]], rtol=1e-6)
    r = R.rope(np.array([[[[1.0, 1.0, 0.0, 0.0, 7.0]]]], np.float32), np.array([1], np.int32), 4, 1, 10000.0)
    assert np.allclose(r, [[[[np.cos(1.0), np.cos(0.01), np.sin(1.0), np.sin(0.01), 7.0]]]], rtol=1e-6)
    assert R.unary("SILU", np.float32(-100.0)) == 0.0 and np.signbit(R.unary("SILU", np.float32(-100.0)))  # expf overflows in f32: -100 / inf
    assert R.bits(R.clamp(np.array([np.nan, -5, 5, -0.0], np.float32), -1.0, 2.0)).tolist() == R.bits(np.array([2, -1, 2, -0.0], np.float32)).tolist()
    assert R.get_rows(np.arange(12, dtype=np.float32).reshape(2, 3, 2), np.array([[2, 0], [1, 1]], np.int32)).reshape(-1).tolist() == [4, 5, 0, 1, 8, 9, 8, 9]
    d = R.set_rows(np.zeros((1, 2, 3, 1), np.float32), np.array([1, 2, 3, 4], np.float32).reshape(1, 2, 2, 1), np.array([[2, 0]], np.int64).reshape(1, 1, 2))
    assert d.reshape(-1).tolist() == [2, 0, 1, 4, 0, 3]
    assert R.permute(np.zeros((2, 3, 4, 5)), (0, 2, 1, 3)).shape == (2, 4, 3, 5) and R.permute(np.zeros((2, 3, 4, 5)), (1, 0, 2, 3)).shape == (2, 3, 5, 4)


@pytest.mark.parametrize("case", [c for c in CASES if c.metric == "bits"], ids=repr)
def test_twin_equals_oracle_bit_for_bit(oracle_built, case):
    got, ref = R.run(case, "oracle"), case.expect()
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype, (g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero(R.bits(g).reshape(-1) != R.bits(r).reshape(-1))
        assert bad.size == 0, f"{case.id}: oracle and twin differ in {bad.size} of {g.size} elements, first at {bad[:5]}: oracle {g.reshape(-1)[bad[:5]]} twin {r.reshape(-1)[bad[:5]]}"


@pytest.mark.parametrize("case", [c for c in CASES if c.metric != "bits"], ids=repr)
def test_oracle_within_its_own_arithmetic_of_the_twin(oracle_built, case, capsys):
    got, ref = R.run(case, "oracle"), case.expect()
    for g, r in zip(got, ref):
        assert g.shape == r.shape, (g.shape, r.shape)
        d = R.distance(case, g, r)
        with capsys.disabled():
            print(f"\n    {case.id}: oracle is {d:.3g} {'ulp' if case.metric == 'ulp' else 'of the row maximum'} from the float64 twin (bound {ORACLE_OWN[case.family]:.3g})", end="")
        assert d <= ORACLE_OWN[case.family], f"{case.id}: oracle {d} from the twin, its own arithmetic accounts for {ORACLE_OWN[case.family]}"


def test_baselines(oracle_built, capsys):
    """The numbers the GPU gates are set from: baseline + ops_ref.ALLOWANCE[family]."""
    fams = sorted({c.family for c in CASES if c.metric != "bits"})
    with capsys.disabled():
        for f in fams:
            b = R.oracle_baseline(f)
            print(f"\n    baseline {f}: {b:.4g}  allowance {R.ALLOWANCE[f]:.4g}  gate {b + R.ALLOWANCE[f]:.4g}", end="")
            assert np.isfinite(b) and b <= ORACLE_OWN[f]
