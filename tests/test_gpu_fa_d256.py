"""FLASH_ATTN_EXT at head size 256 on the GPU (Gemma 1 / 2 / 3): supports_op, the generic split kernel k_fattn_split<256, G> for 1 .. 32 query tokens, the
matrix-core kernel k_fattn_mma<256, NW> (soft-capped or not) for prompt batches, the f16 image of a q8_0 / q4_0 cache, and the cell accounting of fa_ref's
probes on one form of each kernel.  Every test asserts supports_op on its node before anything is computed; every computed node states the kernel form it
expects (stat "fa_form").  Specs, twin and gates: tests/fa_d256.py (proved on the CPU by test_fa_d256_ref_host.py)."""
import numpy as np
import pytest

import fa_d256 as F2
import fa_ref as FR
import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu

S = F2.Spec


def _require(backend, H, spec):
    assert F2.supported(backend, H, F2.builder(spec, None, H)), f"{spec.id}: supports_op refuses FLASH_ATTN_EXT at head size {spec.HD} ({L.TYPE_NAME[spec.tk]} / {L.TYPE_NAME[spec.tv]}, {spec.NH}/{spec.NKV} heads)"


def _compute(backend, H, spec, x):
    backend.set_option("fa_splits", spec.splits)
    try:
        got = F2.run_node(spec, x, backend, H)
        ran = backend.stat("fa_form")
    finally:
        backend.set_option("fa_splits", 0)
    assert ran == spec.form, f"{spec.id}: expected form [{F2.form_name(spec.form)}], ran [{F2.form_name(ran)}]"
    return got


def _gates(spec, x, got, ref, plog):
    exact = F2.twin_of(spec, x)
    e_ref, e_gpu, e_cpu = T.nmse(got, ref), T.nmse(got, exact), T.nmse(ref, exact)
    plog(f"fa_d256 {spec.id} [{F2.form_name(spec.form)}]: vs oracle {e_ref:.3e}  vs twin {e_gpu:.3e}  oracle vs twin {e_cpu:.3e}")
    assert not np.isnan(got).any()
    assert e_ref <= (F2.ORACLE_IMAGE if spec.imaged else F2.ORACLE_F16), f"{spec.id}: nmse {e_ref:.3e} against the oracle"
    assert e_gpu <= (F2.TWIN_MMA if spec.kernel == "MMA" else F2.TWIN_SPLIT), f"{spec.id}: nmse {e_gpu:.3e} against the float64 twin"
    assert e_gpu <= e_cpu * 1.01 + 1e-12, f"{spec.id}: further from the twin ({e_gpu:.3e}) than the oracle is ({e_cpu:.3e})"


# ------------------------------------------------------------------------------------------ 1. supports_op
ACCEPTED = [S("f16", "SPLIT", 4, 2, 1, 64)] + [S(f"{L.TYPE_NAME[t]}", "SPLIT", 4, 2, 1, 64, tk=t, tv=t) for t in (L.Q8_0, L.Q4_0, L.BF16)] + [
    S("q8_0_f16", "SPLIT", 4, 2, 1, 64, tk=L.Q8_0, tv=L.F16)] + [S(f"g{g}", "SPLIT", g, 1, 1, 64) for g in (1, 2, 3, 4, 8)] + [
    S("batch_f16", "MMA", 4, 2, 40, 64), S("batch_q4_0_cap", "MMA", 4, 2, 40, 64, cap=50.0, tk=L.Q4_0, tv=L.Q4_0)]


@pytest.mark.parametrize("spec", ACCEPTED, ids=lambda s: s.id)
def test_supports_op_accepts(backend, H, spec):
    _require(backend, H, spec)


def test_supports_op_still_refuses(backend, H):
    _require(backend, H, S("f16", "SPLIT", 4, 2, 1, 64))  # (on a tree without head size 256 nothing below says anything)
    for hd in (96, 512):
        assert not F2.supported(backend, H, F2.builder(S(f"hd{hd}", "SPLIT", 4, 2, 1, 64, HD=hd), None, H)), hd
    assert not F2.supported(backend, H, F2.builder(S("g16", "SPLIT", 16, 1, 1, 64), None, H))

    def k192_v128(g):
        tq = g.new(L.F32, [192, 1, 4])
        k = g.new(L.F16, [192, 64, 2])
        v = g.new(L.F16, [128, 64, 2])
        return H.ggml_flash_attn_ext(g.ctx, tq, k, v, None, 1.0 / np.sqrt(192), 0.0, 0.0)

    assert not F2.supported(backend, H, k192_v128)


def test_soft_capped_batch_at_128_keeps_the_split_kernel(backend, H, plog):
    """Soft-capping reaches the matrix cores at head size 256 only: 40 capped tokens at 128 run k_fattn_split as before."""
    _require(backend, H, S("f16", "SPLIT", 4, 2, 1, 64))
    spec = S("cap_d128_40", "SPLIT", 4, 2, 40, 260, splits=2, cap=30.0, HD=128)
    assert spec.form == FR.form("SPLIT", 0, 4, "F16", 128, "COMBINE")
    _require(backend, H, spec)
    x = F2.make_inputs(spec)
    got = _compute(backend, H, spec, x)
    assert T.nmse(got, F2.twin_of(spec, x)) <= F2.TWIN_SPLIT


# ------------------------------------------------------------------------------------------ 2. / 3. / 5. the kernels on random data
@pytest.mark.parametrize("spec", F2.SPLIT_SPECS + F2.MMA_SPECS, ids=lambda s: s.id)
def test_flash_attn_d256(backend, H, plog, spec):
    _require(backend, H, spec)
    x = F2.make_inputs(spec)
    ref = F2.run_node(spec, x, "oracle", H)
    got = _compute(backend, H, spec, x)
    _gates(spec, x, got, ref, plog)


@pytest.mark.parametrize("spec", F2.IMAGE_SPECS, ids=lambda s: s.id)
def test_flash_attn_d256_through_the_image(backend, H, plog, spec):
    _require(backend, H, spec)
    x = F2.make_inputs(spec)
    ref = F2.run_node(spec, x, "oracle", H)
    img0, nat0 = backend.stat("kv_image_nodes"), backend.stat("kv_native_nodes")
    got = _compute(backend, H, spec, x)
    assert (backend.stat("kv_image_nodes") - img0, backend.stat("kv_native_nodes") - nat0) == (1, 0)
    _gates(spec, x, got, ref, plog)


# ------------------------------------------------------------------------------------------ 4. cell accounting
@pytest.mark.parametrize("spec", [F2.SPLIT_SPECS[6], F2.MMA_SPECS[0]], ids=lambda s: s.id)
def test_fa_cells_d256(backend, H, plog, spec):
    """fa_ref's indicator, witness and pair probes (one wrong cell is an order-one error) at their own gates, on a split case with two splits and sinks and on
    the matrix-core form with tile states."""
    assert spec.id in ("split_sinks_g4", "mma_33_tile_states") and (spec.kernel == "MMA" or spec.n_splits >= 2)
    _require(backend, H, spec)
    case = F2.fr_case(spec)
    assert case.trip == (FR.fa_constants()["bkv"] if spec.kernel == "MMA" else 32) and case.n_splits == spec.n_splits
    bad, worst = [], {}
    backend.set_option("fa_splits", spec.splits)
    try:
        probes = FR.indicator_probes(case) + FR.witness_probes(case, False) + FR.witness_probes(case, True)
        assert any(p.name.startswith("indicator") for p in probes) and any(p.name.startswith("witness") for p in probes)
        for p in probes:
            got = FR.run_probe(case, p, backend, H)
            ran = backend.stat("fa_form")
            if ran != spec.form:
                bad.append(f"{p.name}: expected form [{F2.form_name(spec.form)}], ran [{F2.form_name(ran)}]")
            try:
                kind = p.name.split("_")[0]
                worst[kind] = max(worst.get(kind, 0.0), FR.check_probe(case, p, got))
            except AssertionError as e:
                bad.append(str(e))
    finally:
        backend.set_option("fa_splits", 0)
    plog(f"fa_cells_d256 {spec.id}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" (gates: indicator {FR.INDICATOR_GATE}, witness {FR.WITNESS_GATE} x max|V|)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])
