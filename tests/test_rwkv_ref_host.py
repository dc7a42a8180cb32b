"""CPU: the NumPy twins and gates of tests/rwkv_ref.py, which the GPU tests of csrc/rwkv.hip rest on — the f32 twin in the contract's order lies inside the
float64 twin's a-priori bound, every wrong twin lies outside the kernels' gate by at least 10 x, the generators are reproducible, the result layout holds."""
import numpy as np
import pytest

import rwkv_ref as R

# (op, S, H, n_seqs, n_t): both head sizes, an odd head count, more than one sequence, more than one token
SHAPES = [(64, 3, 3, 5), (128, 1, 3, 2), (64, 1, 1, 17)]


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("S,H,n_seqs,n_t", SHAPES)
def test_f32_twin_inside_the_contract_order_bound(op, S, H, n_seqs, n_t):
    inp = R.inputs(op, S, H, n_seqs, n_t)
    ref = R.twin64(op, inp, reordered=False)
    ey, es = R.excess(ref, *R.twin32(op, inp))
    assert ey <= 1.0 and es <= 1.0, (op, ey, es)
    # the kernels' gate differs by the second S roundings of each reduction and by nothing else: for WKV6 / GLA, whose states hold no reduction, S Ey exactly
    wide = R.twin64(op, inp)
    assert np.all(wide["ey"] >= ref["ey"]) and np.all(wide["es"] >= ref["es"])
    if op != "wkv7":
        assert np.allclose(wide["ey"] - ref["ey"], S * ref["Ey"], rtol=1e-9) and np.array_equal(wide["es"], ref["es"])


@pytest.mark.parametrize("kind", ["indicator", "zero_decay", "unit_decay"])
@pytest.mark.parametrize("op", R.OPS)
def test_f32_twin_inside_the_bound_on_the_edge_inputs(op, kind):
    inp = R.inputs(op, 64, 3, 3, 5, kind)
    ey, es = R.excess(R.twin64(op, inp, reordered=False), *R.twin32(op, inp))
    assert ey <= 1.0 and es <= 1.0, (op, kind, ey, es)


@pytest.mark.parametrize("wrong,op", [(w, op) for w in sorted(R.WRONG) for op in R.WRONG[w]])
def test_wrong_twins_miss_the_gate_by_ten(wrong, op):
    """State, decay and bonus all of order one (the plain generator), three sequences of three tokens: each mistake is of order one where the gate is 1e-5."""
    inp = R.inputs(op, 64, 3, 3, 3)
    ref = R.twin64(op, inp)
    bad = R.twin64(op, inp, wrong=wrong)
    ey, es = R.excess(ref, bad["y"], bad["st"])
    assert max(ey, es) >= 10.0, (wrong, op, ey, es)


def test_generators_are_reproducible_and_cover_the_decay_edges():
    for op in R.OPS:
        a, b = R.inputs(op, 64, 3, 3, 5), R.inputs(op, 64, 3, 3, 5)
        assert a.keys() == b.keys() and all(np.array_equal(a[n], b[n]) for n in a)
        d = a[{"wkv6": "td", "gla": "g", "wkv7": "w"}[op]]
        assert d.min() > 0.0 and d.max() < 1.0 and d.min() <= 2.0 ** -10 and d.max() >= 1.0 - 2.0 ** -10
        assert np.all(a["state"] != 0.0) and (a["k"] < 0).any() and (a["k"] > 0).any() and (a["v"] < 0).any()
        other = R.inputs(op, 64, 3, 3, 5, seed=1)
        assert not np.array_equal(a["k"], other["k"])


@pytest.mark.parametrize("op", R.OPS)
def test_result_layout_y_first_then_states_per_sequence(op):
    inp = R.inputs(op, 64, 3, 3, 2)
    y, st = R.twin32(op, inp)
    flat = R.join(y, st)
    C, T, S, n_seqs = 3 * 64, 6, 64, 3
    assert flat.size == C * (T + S * n_seqs)
    y2, st2 = R.split(flat, inp)
    assert np.array_equal(y2, y) and np.array_equal(st2, st)
    assert np.array_equal(flat[:C * T], y.reshape(-1)) and np.array_equal(flat[C * T + S * C:C * T + 2 * S * C], st[1].reshape(-1))
    # a sequence run alone is its rows of the joint run (the twins share nothing between sequences)
    for s in range(n_seqs):
        y1, st1 = R.twin32(op, R.one_sequence(op, inp, s))
        assert np.array_equal(y1, y[2 * s:2 * s + 2]) and np.array_equal(st1[0], st[s])


def test_indicator_lands_in_one_cell():
    for op in R.OPS:
        inp = R.inputs(op, 64, 3, 1, 1, "indicator")
        _, st = R.twin32(op, inp)
        for h in range(3):
            i, j = np.nonzero(st[0, h])
            ki, vj = (3 + 11 * h) % 64, (1 + 13 * h) % 64
            # WKV6 / GLA: state [i, j] = k[i] v[j]; WKV7: state [i, j] = v[i] k[j]
            assert (list(i), list(j)) == (([vj], [ki]) if op == "wkv7" else ([ki], [vj])), (op, h, i, j)


def test_l2_norm_sqr_repeat_twins():
    rng = np.random.default_rng(3)
    for ne0 in (1, 63, 64, 65, 128, 4096):
        x = rng.standard_normal((5, ne0)).astype(np.float32)
        x[2] = 0.0
        x[3] *= 1e-9  # below eps: x / eps
        eps = 1e-6
        want = R.l2_norm64(x, eps)
        assert np.all(np.abs(R.l2_norm32(x, eps).astype(np.float64) - want) <= R.l2_norm_gate(x, eps))
        assert np.array_equal(want[2], np.zeros(ne0)) and np.allclose(want[3], x[3].astype(np.float64) / eps, rtol=1e-12)
    a = rng.standard_normal((1, 3, 2, 5)).astype(np.float32)
    r = R.repeat(a, [10, 2, 9, 4])
    assert r.shape == (4, 9, 2, 10) and r[3, 7, 1, 8] == a[0, 1, 1, 3]
    assert np.array_equal(R.sqr(np.float32([3, -2])), np.float32([9, 4]))
