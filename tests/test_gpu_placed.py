"""Fused and reordered launches when a result lies over a tensor the graph read before it — the layouts a graph allocator produces and tests/harness.py alone never
does.  The cases, their placement and the legality rule are in tests/placed_ref.py; tests/test_placed_ref_host.py shows on the CPU that the oracle on a placed graph
equals the oracle on the graph with every tensor in its own block, which makes it the reference here.

Every case: the placement is legal; the placed GPU result is compared with the oracle on the placed graph (harness.compare, the gate of the chain's own test:
max_nmse 1e-10 for the quantised mat-muls, test_gpu_ops.py); with option fusion 0 the placed and the unplaced GPU run are bit-equal (same kernels: placement alone
changes nothing); the statistic that shows which branch ran is asserted, after the control graph has shown that the fused form IS taken next door.  The
attention chains of family F are held to nf_ref.RANDOM_GATE, their own tests' gate against the oracle.  NORM, GROUP_NORM, SSM_CONV, MUL_MAT_ID and ADD_ID are no
ops of the oracle: D1-D4 are held to the bits of the unfused kernels, to the f32 MUL / ADD of the kernel's own norm and that norm to its float64 twin at
act_norm_ref's gate (what test_gpu_act_norm.py / test_gpu_diffusion.py pin for the chains); D5 to test_gpu_ssm.py's bound from the twin; E to moe_ref's composite
oracle reference at test_gpu_moe.py's gate.

What a pass shows.  Deterministic cases (A2, A3, A5, B1-B3, C1-C3, D1, D3, F1): a missing guard runs a launch early or reads a stale key and gives a wrong value
on every run.  Race cases (A1, D2, D4, D5, E, F2, F3): the unguarded launch would have workgroups write what others still read; a pass shows that the guarded
branch is taken (the statistic) and computes the right values — it cannot show that the race is absent, and no case is repeated to hunt for one.

Two cases pin less than the guard they are filed under.  A5: the hand-over compares the recorded tensor with the RMS_NORM's source by pointer, and the in-place
SCALE is another tensor — the case pins that comparison, and stays green without the record's invalidation by range in run_nodes.  C2: a node that lies between
the siblings and is read there also overlaps an operand of a node in between, so find_mm_siblings' operand test declines the layout before its result test is
asked; the result test alone is never the deciding one.
"""
import numpy as np
import pytest

import act_norm_ref as A
import diffusion_ref as DR
import harness as T
import llama_box_amd as L
import moe_ref as MR
import mxfp4_ref as XR
import nf_ref as NF
import ops_ref as R
import placed_ref as P
import ssm_ref as S

pytestmark = pytest.mark.gpu

STATS = ("kernel_launches", "fused_nodes", "ss_handoffs", "nf_list_chains", "nf_mma_chains")
MM_GATE = 1e-10  # test_gpu_ops.py: quantised MUL_MAT
QTS = [L.Q4_K, L.Q8_0]


def gpu(backend, case, placed=True, control=False, **options):
    """(outs, probes, stat deltas) of one run with the given options set for its duration.  Only options whose default is 1 are taken: that is what the finally
    puts back (the backend has no getter)."""
    assert set(options) <= {"fusion", "mm_merge"}, options
    try:
        for k, v in options.items():
            backend.set_option(k, v)
        s0 = {k: backend.stat(k) for k in STATS}
        outs, probes = P.run(case, backend, placed, control)
        return outs, probes, {k: backend.stat(k) - v for k, v in s0.items()}
    finally:
        for k in options:
            backend.set_option(k, 1)


def assert_bits(name, a, b):
    assert a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b)), f"{name}: {int(np.count_nonzero(R.bits(a) != R.bits(b)))} of {a.size} values differ"


def common(backend, plog, case, gate=MM_GATE):
    """The assertions every case shares; returns (outs, probes, stat deltas) of the placed run with fusion on.  gate: the NMSE gate against the oracle on the placed
    graph (rows that are NaN in the oracle — a token that sees nothing — must be NaN and are left out: nf_ref.nmse_rows)."""
    for control in (False, True):
        with P.graph(case, True, control) as gf:
            assert P.violations(gf) == []
    outs, probes, d = gpu(backend, case)
    plog(f"  placed {case.id}: {d}")
    if case.oracle:
        ref, _ = P.run(case, "oracle", True, n_threads=1)
        for k, (a, b) in enumerate(zip(outs, ref)):
            if np.isnan(b).any():
                e = NF.nmse_rows(a, b)
                plog(f"placed {case.id} out {k}: nmse {e:.3e} over the rows that are not NaN, gate {gate:.1e}")
                assert e <= gate, (case.id, e)
            else:
                T.compare(f"placed {case.id} out {k}", a, b, max_nmse=gate, log=plog)
    plain_placed, _, _ = gpu(backend, case, True, fusion=0)
    plain_apart, _, _ = gpu(backend, case, False, fusion=0)
    for k, (a, b) in enumerate(zip(plain_placed, plain_apart)):
        assert_bits(f"{case.id} out {k}, fusion 0: placed vs every tensor in its own block", a, b)
    return outs, probes, d


# ------------------------------------------------------------------------------------------------ A. batch-1 mat-vec prologues
@pytest.mark.parametrize("qt", QTS)
def test_a1_glu_over_the_activation_row_takes_no_f32_prologue(backend, plog, qt):
    case = P.CASES[f"A1-glu-{P.QNAME[qt]}"]
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["kernel_launches"] == 1 and ctl["fused_nodes"] == 2, ctl  # the row is quantised in the launch's prologue
    _, _, d = common(backend, plog, case)
    assert d["kernel_launches"] == 2 and d["fused_nodes"] == 2, d  # the quantiser, then the launch without prologue


@pytest.mark.parametrize("qt", QTS)
def test_a2_deferred_norm_with_the_mul_in_place_over_x(backend, plog, qt):
    case = P.CASES[f"A2-{P.QNAME[qt]}"]
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 2 and ctl["kernel_launches"] == 2, ctl
    _, probes, d = common(backend, plog, case)
    assert d["fused_nodes"] == 2 and d["kernel_launches"] == 2, d  # still deferred: one launch per consumer
    assert_bits("A2: x after the run (the MUL node stays unwritten)", probes[0].reshape(-1), case.build.inputs[0].reshape(-1))


@pytest.mark.parametrize("qt", QTS)
def test_a3_first_consumer_over_x_keeps_the_norm_from_being_deferred(backend, plog, qt):
    case = P.CASES[f"A3-{P.QNAME[qt]}"]
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 2, ctl
    _, _, d = common(backend, plog, case)
    assert d["fused_nodes"] == 1 and d["kernel_launches"] == 3, d  # RMS_NORM -> MUL as one launch of its own, then the two mat-vecs


def test_a5_in_place_scale_drops_the_sum_of_squares_record(backend, plog):
    case = P.CASES["A5-q4_K"]
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["ss_handoffs"] == 1, ctl
    _, _, d = common(backend, plog, case)
    assert d["ss_handoffs"] == 0, d


# ------------------------------------------------------------------------------------------------ B. the quantised-activation area
@pytest.mark.parametrize("cid", ["B1", "B2"])
def test_b_activation_cache_is_dropped_when_its_source_is_overwritten(backend, plog, cid):
    _, _, d = common(backend, plog, P.CASES[cid])
    if cid == "B2":
        assert d["fused_nodes"] >= 1, d  # the ADD over X rode in a mat-mul's store


def test_b3_intruder_in_the_activation_area_keeps_the_f32_rows(backend, plog):
    case = P.CASES["B3"]
    backend.set_option("timing", 1)
    try:
        backend.timing_report()
        gpu(backend, case, control=True)
        ctl = backend.timing_report()
        common(backend, plog, case)
        got = backend.timing_report()
    finally:
        backend.set_option("timing", 0)
    assert ctl.get("rms_norm_mul_quantize", (0,))[0] == 1, sorted(ctl)
    assert "rms_norm_mul_quantize" not in got, sorted(got)


# ------------------------------------------------------------------------------------------------ C. sibling merges
@pytest.mark.parametrize("qt", QTS)
@pytest.mark.parametrize("which", ["C1", "C2", "C3"])
def test_c_sibling_merge_leaves_out_what_cannot_run_early(backend, plog, which, qt):
    case = P.CASES[f"{which}-{P.QNAME[qt]}"]
    _, _, ctl = gpu(backend, case, control=True)
    _, _, ctl_plain = gpu(backend, case, control=True, mm_merge=0)
    assert ctl["kernel_launches"] < ctl_plain["kernel_launches"], (ctl, ctl_plain)  # the three siblings alone do merge
    outs, probes, d = common(backend, plog, case)
    one_by_one, probes1, d1 = gpu(backend, case, mm_merge=0)
    plog(f"  placed {case.id}: control {ctl['kernel_launches']} / {ctl_plain['kernel_launches']} launches merged / one by one, case {d['kernel_launches']} / {d1['kernel_launches']}")
    for k, (a, b) in enumerate(zip(list(outs) + list(probes), list(one_by_one) + list(probes1))):
        assert_bits(f"{case.id} out {k}: merged vs mm_merge 0", a, b)
    saved, saved_ctl = d1["kernel_launches"] - d["kernel_launches"], ctl_plain["kernel_launches"] - ctl["kernel_launches"]
    if which == "C3":  # (the third sibling may ride along without its ADD: no more is saved than by the three alone)
        assert 0 <= saved <= saved_ctl, (saved, saved_ctl)
    else:  # the first two siblings still share a launch, the third is left out
        assert 0 < saved < saved_ctl, (saved, saved_ctl)
    if which == "C3":
        ref, ref_probes = P.run(case, "oracle", True, n_threads=1)
        T.compare(f"placed {case.id} first sibling", probes[0], ref_probes[0], max_nmse=MM_GATE, log=plog)


# ------------------------------------------------------------------------------------------------ D. chains that write a later node's memory
def _gpu_norm(backend, x):
    def build(g, placed=True, control=False):
        return P.Built([g.H.ggml_norm(g.ctx, g.new(L.F32, list(x.shape[::-1]), x), P.EPS)])

    return P.run(P.Case("norm", "D", build, "race"), backend)[0][0]


@pytest.mark.parametrize("cid,absorbed", [("D1", 2), ("D2", 1)])
def test_d_norm_affine_chain_over_x(backend, plog, cid, absorbed):
    case = P.CASES[cid]
    x, w, b = case.build.inputs
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 2 and ctl["kernel_launches"] == 1, ctl
    outs, _, d = common(backend, plog, case)
    # D1: in place, the same rows — the chain stays one launch.  D2: the ADD's rows are x's, one row on — the launch stops at the MUL
    assert d["fused_nodes"] == absorbed and d["kernel_launches"] == 3 - absorbed, d
    apart, _, _ = gpu(backend, case, False, fusion=0)
    assert_bits(f"{cid}: placed and fused vs apart and unfused", outs[0], apart[0])
    # the independent reference: the kernel's NORM inside act_norm_ref's gate from the float64 twin, and the result the f32 MUL and ADD of exactly that NORM
    # (the fused launch rounds as the nodes it stands for: test_gpu_act_norm.py's test_norm_affine_fusion pins the same two equalities)
    nn = _gpu_norm(backend, x)
    dist, gate = float(np.max(R.row_distance(nn.reshape(x.shape), A.norm(x, P.EPS)))), A.NORM_GATE + A.norm_extra(x)
    plog(f"  placed {cid}: NORM {dist:.4g} of the row's maximum from the float64 twin, gate {gate:.4g}")
    assert dist <= gate, (dist, gate)
    want = R.binary("add", R.binary("mul", nn, w), b)
    assert_bits(f"{cid}: vs the MUL / ADD of the kernel's own NORM", outs[0], want.reshape(outs[0].shape))


@pytest.mark.parametrize("cid,absorbed", [("D3", 3), ("D4", 2)])
def test_d_group_norm_affine_silu_chain_over_x(backend, plog, cid, absorbed):
    case = P.CASES[cid]
    x, w, b = case.build.inputs
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 3 and ctl["kernel_launches"] == 1, ctl
    outs, _, d = common(backend, plog, case)
    # D3: in place, the same bytes — the chain stays one launch.  D4: the SILU's bytes are x's, one row on — the launch stops at the ADD
    assert d["fused_nodes"] == absorbed and d["kernel_launches"] == 4 - absorbed, d
    apart, _, _ = gpu(backend, case, False, fusion=0)
    assert_bits(f"{cid}: placed and fused vs apart and unfused", outs[0], apart[0])
    # the independent reference, as test_gpu_diffusion.py's test_group_norm_affine_fusion has it: the kernel's GROUP_NORM inside its gate from the float64
    # twin, group by group; the f32 MUL and ADD of exactly that; SILU at the unary family's gate from its float64 twin
    def build_gn(g, placed=True, control=False):
        return P.Built([g.H.ggml_group_norm(g.ctx, g.new(L.F32, P.GN_NE, x), P.GN_GROUPS, P.GN_EPS)])

    gn = P.run(P.Case("group_norm", "D", build_gn, "race"), backend)[0][0].reshape(x.shape)
    frac, dist, gate = DR.group_norm_excess(gn, x, P.GN_GROUPS, P.GN_EPS)
    plog(f"  placed {cid}: GROUP_NORM worst group {dist:.4g} of its maximum from the twin, {frac:.3f} of its gate {gate:.4g}")
    assert frac <= 1.0, (dist, gate)
    affine = DR.channel_binary("add", DR.channel_binary("mul", gn, w), b)
    silu_gate = R.oracle_baseline("silu") + R.ALLOWANCE["silu"]
    ulp = float(np.max(R.ulp_distance(outs[0].reshape(x.shape), R.unary("SILU", affine))))
    plog(f"  placed {cid}: SILU of the kernel's own affine {ulp:.3g} ulp from the twin, gate {silu_gate:.3g}")
    assert ulp <= silu_gate, (ulp, silu_gate)


def test_d5_ssm_conv_chain_with_the_silu_over_the_conv_input(backend, plog):
    case = P.CASES["D5"]
    sx, c, b = case.build.inputs
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 2 and ctl["kernel_launches"] == 1, ctl
    outs, _, d = common(backend, plog, case)
    assert d["fused_nodes"] == 0 and d["kernel_launches"] == 3, d
    apart, _, _ = gpu(backend, case, False, fusion=0)
    assert_bits("D5: placed vs apart and unfused", outs[0], apart[0])
    ref, _ = S.conv64(sx, c)  # test_gpu_ssm.py's bound for silu(conv + b)
    want = S.silu64(ref + b.astype(np.float64))
    bound = 1.1 * (S.conv_gate(sx, c) + S.U * np.abs(ref + b)) + 8 * S.U * np.abs(want) + 2.0 ** -120
    assert np.all(np.abs(outs[0].reshape(ref.shape).astype(np.float64) - want) <= bound)


# ------------------------------------------------------------------------------------------------ E. MUL_MAT_ID -> ADD_ID
@pytest.mark.parametrize("tname", ["f16", "q4_K"])
def test_e_add_id_over_b_does_not_ride_in_the_store(backend, plog, tname):
    case = P.CASES[f"E-{tname}"]
    qt, W, K, N, b, bias, ids = case.build.inputs
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 1, ctl  # in a block of its own the bias rides in the product's store
    outs, _, d = common(backend, plog, case)
    assert d["fused_nodes"] == 0 and d["kernel_launches"] == ctl["kernel_launches"] + 1, (d, ctl)  # the ADD_ID is a launch of its own
    # MUL_MAT_ID and ADD_ID are no ops of the oracle: moe_ref's composite reference (one-column oracle MUL_MATs per pair) and the f32 add of the expert's bias,
    # at test_gpu_moe.py's gate
    want = XR.add_id(MR.mmid_reference(qt, W, K, N, [(b, ids)])[0], bias, ids)
    T.compare(f"placed {case.id}", outs[0].reshape(want.shape), want, max_nmse=MM_GATE, log=plog)
    apart, _, _ = gpu(backend, case, False, fusion=0)
    assert_bits(f"{case.id}: placed vs apart and unfused", outs[0], apart[0])


# ------------------------------------------------------------------------------------------------ F. the non-flash attention chain, SOFT_MAX -> V^T.p
@pytest.mark.parametrize("form", ["list", "mma"])
@pytest.mark.parametrize("which,absorbed", [("F1", 3), ("F2", 2)])
def test_f_attention_chain_with_the_copy_over_q(backend, plog, which, absorbed, form):
    case = P.CASES[f"{which}-{form}"]
    chains = "nf_list_chains" if form == "list" else "nf_mma_chains"
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl[chains] == 1 and ctl["fused_nodes"] == 3, ctl  # SOFT_MAX, V^T.p and the CONT copy are the K.q launch's
    _, _, d = common(backend, plog, case, gate=NF.RANDOM_GATE)
    # F1: the same rows — the copy stays the launch's target.  F2: other rows of q's block — the launch writes the product's own tensor, the CONT follows
    assert d[chains] == 1 and d["fused_nodes"] == absorbed and d["kernel_launches"] == ctl["kernel_launches"] + 3 - absorbed, (d, ctl)


def test_f3_product_over_the_logits_keeps_the_soft_max_out_of_it(backend, plog):
    case = P.CASES["F3"]
    _, _, ctl = gpu(backend, case, control=True)
    assert ctl["fused_nodes"] == 1 and ctl["kernel_launches"] == 2, ctl  # K.q, then SOFT_MAX inside V^T.p
    _, _, d = common(backend, plog, case, gate=NF.RANDOM_GATE)
    assert d["fused_nodes"] == 0 and d["kernel_launches"] == 3, d
