"""CPU checks of tests/placed_ref.py: every case's placement is one an allocator could have produced, the checker rejects the case once its placed node runs before
its victim's last reader, and the oracle computes the same bits on the placed graph as on the graph with every tensor in its own block — so the oracle on the
placed graph is the reference of tests/test_gpu_placed.py."""
import numpy as np
import pytest

import placed_ref as P
from ops_ref import bits

CASES = list(P.CASES.values())
PLACED = [c for c in CASES if c.placed_node]


@pytest.fixture(scope="module", autouse=True)
def _libs(built):
    return built


def test_the_table_has_the_cases_the_gpu_module_runs():
    assert [c.id for c in CASES if not c.placed_node] == ["B3", "C3-q4_K", "C3-q8_0"]  # the guards of these three are about order, not about bytes
    # NORM, GROUP_NORM, SSM_CONV, MUL_MAT_ID and ADD_ID are no ops of the oracle: judged against their families' references on the GPU
    assert [c.id for c in CASES if not c.oracle] == ["D1", "D2", "D3", "D4", "D5", "E-f16", "E-q4_K"]
    assert {c.family for c in CASES} == set("ABCDEF") and all(c.kind in ("deterministic", "race") for c in CASES)
    assert [c.id for c in CASES if c.family == "F"] == ["F1-list", "F2-list", "F1-mma", "F2-mma", "F3"]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_placement_is_legal(case):
    for control in (False, True):
        with P.graph(case, True, control) as gf:
            assert P.violations(gf) == []
            assert P.legal(gf)
    with P.graph(case, True) as gf:
        assert (P.victim_reader(gf) is not None) == case.placed_node


@pytest.mark.parametrize("case", PLACED, ids=repr)
def test_checker_rejects_the_placed_node_in_front_of_its_victims_last_reader(case):
    with P.graph(case, True) as gf:
        j, r = P.move_before_reader(gf)
        assert r < j
        bad = P.violations(gf)
        assert bad and not P.legal(gf), (case.id, j, r)
        assert all("overwrites" in b for b in bad), bad


@pytest.mark.parametrize("case", [c for c in CASES if c.oracle], ids=repr)
def test_oracle_on_the_placed_graph_equals_the_oracle_with_every_tensor_in_its_own_block(case):
    placed, _ = P.run(case, "oracle", True, n_threads=1)  # (one thread: the reference's own threading must not race on the shared bytes)
    apart, _ = P.run(case, "oracle", False)
    assert len(placed) == len(apart)
    for a, b in zip(placed, apart):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), case.id


def test_checker_rejects_what_the_issue_lists_as_unreachable():
    """A single MUL_MAT over its own activation row (A1's first form; A4 and A6 are the same shape of problem): the operand's last reader is the node itself, and
    MUL_MAT is not an op that runs in place."""
    import harness as T
    import llama_box_amd as L

    rng = np.random.default_rng(1)
    w, x = T.rand_weight(L.Q4_K, 512, 64, rng), rng.standard_normal((1, 512)).astype(np.float32)

    def build(g, placed=True, control=False):
        xt = g.new(L.F32, [512], x, "x")
        return P.Built([P.place(g, g.H.ggml_mul_mat(g.ctx, g.new(L.Q4_K, [512, 64], w), xt), xt)])

    with P.graph(P.Case("A1-mm", "A", build, "race")) as gf:
        assert not P.legal(gf) and "still reads" in P.violations(gf)[0]
