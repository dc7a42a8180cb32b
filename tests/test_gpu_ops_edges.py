"""GPU: the generic kernels of csrc/ops.hip (element-wise, norm, soft-max, rope, row ops) at their edges — the branches no friendly shape reaches:
second and partial trips of the grid-stride and float4 loops, scalar paths forced by shape or alignment, strided views, the hand-over points between
kernels, broadcast indices, ties, and the value catalogue of tests/ops_ref.py (zeros of both signs, subnormals, the f16 overflow boundary and ties,
expf's range ends, inf, NaN).  Every case is one small graph of tests/ops_ref.py: all_cases(), run through the C-ABI.

  * plain IEEE f32 / data movement (binary, scale, RELU, NEG, clamp, cpy / cast, get_rows, set_rows, argmax): kernel == oracle == NumPy twin as
    uint32 / uint16, NaNs by isnan; destinations that a view writes into are read back WHOLE against their sentinel pattern.
  * rms_norm, silu / exp / tanh / sigmoid, swiglu: f32 ulps from the float64 twin; soft_max, rope: error over the row's largest magnitude.  The gate
    is the ORACLE's largest distance on the same inputs plus what the kernel's own functions account for (ops_ref.ALLOWANCE, reasoned there) —
    no NMSE: one wrong element in half a million must fail.

ARGMAX pins what kernel and oracle do (first maximum, NaN never wins, 0 for a row without a maximum); upstream's rule is unpinned.
"""
import numpy as np
import pytest

import ops_ref as R

pytestmark = pytest.mark.gpu

CASES = R.all_cases()


def _first_bad(a, b):
    bad = np.flatnonzero(R.bits(a).reshape(-1) != R.bits(b).reshape(-1))
    return bad.size, bad[:5]


@pytest.mark.parametrize("case", [c for c in CASES if c.metric == "bits"], ids=repr)
def test_bit_exact(backend, H, plog, case):
    got, ora, twin = R.run(case, backend), R.run(case, "oracle"), case.expect()
    assert len(got) == len(ora) == len(twin)
    for g, o, t in zip(got, ora, twin):
        assert g.shape == t.shape == o.shape and g.dtype == t.dtype == o.dtype, (case.id, g.shape, o.shape, t.shape, g.dtype, o.dtype, t.dtype)
        n_t, at_t = _first_bad(g, t)
        n_o, at_o = _first_bad(g, o)
        plog(f"  edges {case.id}: {g.size} values, {n_t} differ from the twin, {n_o} from the oracle")
        assert n_t == 0, f"{case.id}: kernel and twin differ in {n_t} of {g.size} elements, first at {at_t}: kernel {g.reshape(-1)[at_t]} twin {t.reshape(-1)[at_t]}"
        assert n_o == 0, f"{case.id}: kernel and oracle differ in {n_o} of {g.size} elements, first at {at_o}: kernel {g.reshape(-1)[at_o]} oracle {o.reshape(-1)[at_o]}"


@pytest.mark.parametrize("case", [c for c in CASES if c.metric != "bits"], ids=repr)
def test_within_the_gate_of_the_float64_twin(backend, H, plog, case):
    got, twin = R.run(case, backend), case.expect()
    base, gate = R.oracle_baseline(case.family), R.gate(case)
    unit = "ulp" if case.metric == "ulp" else "of the row's maximum"
    assert len(got) == len(twin)
    for k, (g, t) in enumerate(zip(got, twin)):
        assert g.shape == t.shape, (case.id, g.shape, t.shape)
        d = R.distance(case, g, t)
        plog(f"  edges {case.id}[{k}]: kernel {d:.4g} {unit} from the float64 twin; oracle baseline of '{case.family}' {base:.4g}, gate {gate:.4g}")
        assert d <= gate, f"{case.id}[{k}]: kernel is {d:.6g} {unit} from the twin, the gate is {gate:.6g} (oracle baseline {base:.6g})"


def test_rope_f16_results_are_f16_roundings_of_a_close_f32_value(backend, H, plog):
    """The f16 forms round ONE f32 result: apart from elements where the f32 value sits within the rope gate of a rounding boundary, the bits equal the
    twin's value rounded to f16 — so an error hides neither in the half f16 ulp of the distance gate nor in the pass-through tail, which is exact."""
    for case in (c for c in CASES if c.family == "rope_f16"):
        g, t = R.run(case, backend)[0], case.expect()[0]
        t16 = R.cast(t, np.float16)
        differ = R.bits(g) != R.bits(t16)
        # a differing element must be a neighbouring f16 whose boundary the float64 value all but touches
        gap = np.abs(np.abs(g.astype(np.float64) - t) - np.abs(t16.astype(np.float64) - t))
        tol = R.ALLOWANCE["rope"] * np.broadcast_to(np.asarray(case.scale)[..., None], t.shape) * 2
        plog(f"  edges {case.id}: {int(differ.sum())} of {g.size} f16 values on the other side of a rounding boundary")
        assert np.all(gap[differ] <= tol[differ]), f"{case.id}: {int((gap[differ] > tol[differ]).sum())} f16 results are not a rounding of the expected value"
        assert differ.mean() <= 0.01
