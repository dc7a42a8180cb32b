"""CPU checks of tests/fa_d256.py: its form-code helper against kernels.h (no code of a head-size-64 / -128 form moved when the 256 flag was added), and its
float64 twin — soft-capped or not — against the CPU oracle at head size 256 on the shapes test_gpu_fa_d256.py runs, at that file's gates: the gates can be met
by the reference alone, so a GPU failure there is the kernels'."""
import re

import numpy as np
import pytest

import fa_d256 as F2
import fa_ref as FR
import harness as T
import llama_box_amd as L

# the codes of fa_ref.CASES as they were before head size 256 had a flag (kernel | mode << 4 | waves << 6 | cache kind << 10 | (D == 128) << 12 | tail << 13)
CODES_BEFORE = {
    "split_d128_alibi": 12545, "split_d64_nomask": 257, "plain4_d128_g2_nomask": 4354, "plain4_q8_0": 13570, "plain4_q4_0": 14594, "wide8_d128_g2": 12802,
    "wide8_d64_g8_chooser": 8706, "fat_one_trip_splits": 45570, "list_d128_g3_one": 4386, "list_d64_g4_one": 290, "skip_d128_g3_sinks": 12562,
    "mma_d128_33": 4243, "mma_d64_40_splits": 8339, "mma_d128_264_nomask": 4355, "mma_d128_rows": 20627, "mma_q8_0_image": 15507, "merge2_wide8": 37378,
    "self_merge_list_g1": 28962,
}


def test_form_codes_of_the_other_head_sizes_are_unchanged():
    by = {c.id: c for c in FR.CASES}
    for cid, code in CODES_BEFORE.items():
        assert by[cid].form == code, f"{cid}: {by[cid].form} != {code}"
    bit = F2.d256_bit()
    for c in FR.CASES:  # ... and none of them uses the new bit; the helper agrees with fa_ref on them
        assert c.form & bit == 0 and c.form < bit, c.id
        kvf = c.kvform or {L.F16: "F16", L.Q8_0: "Q8_0", L.Q4_0: "BLOCK"}[c.kv]
        assert F2.form(c.kernel, c.mode, c.waves, kvf, c.HD, c.tail) == c.form


def test_form_code_helper_matches_kernels_h():
    """fa_form_code as kernels.h writes it, evaluated here: the 256 flag is one bit above the tail field, and the three head sizes give three different codes."""
    kh = FR._src("kernels.h")
    f = FR.fa_constants()["form"]
    assert f["FA_FORM_D256_BIT"] == 16 and max(v for k, v in f.items() if k.startswith("FA_FORM_TAIL_")) < 8  # tail: bits 13 .. 15
    body = FR._one(kh, r"static inline int fa_form_code\(int kernel, int mode, int waves, int kv, int D, int tail\) \{\n((?:.*\n)*?)\}", "fa_form_code")
    assert re.sub(r"\s+", " ", body).strip() == ("if (D == 256) kernel |= 1 << FA_FORM_D256_BIT; "
                                                 "return kernel | (mode << 4) | (waves << 6) | (kv << 10) | ((D == 128 ? 1 : 0) << 12) | (tail << 13);")

    def code(kernel, mode, waves, kv, D, tail):
        if D == 256:
            kernel |= 1 << f["FA_FORM_D256_BIT"]
        return kernel | (mode << 4) | (waves << 6) | (kv << 10) | ((1 if D == 128 else 0) << 12) | (tail << 13)

    for kern in ("SPLIT", "MMA"):
        for mode in (0, 1):
            for waves in (2, 4):
                for tail in ("NONE", "COMBINE"):
                    codes = [F2.form(kern, mode, waves, "F16", D, tail) for D in (64, 128, 256)]
                    assert codes == [code(f["FA_FORM_K_" + kern], mode, waves, f["FA_FORM_KV_F16"], D, f["FA_FORM_TAIL_" + tail]) for D in (64, 128, 256)]
                    assert len(set(codes)) == 3
                    assert [F2.form_name(c).split("D=")[1].split()[0] for c in codes] == ["64", "128", "256"]


def test_spec_geometry():
    trip = FR.trip_len(256, 1, 4, "split")
    assert trip == 32  # a row is 32 lanes: two rows per wave-instruction, NG x 4 waves x 2
    ns = sorted(s.nkv for s in F2.SPLIT_SPECS if s.id.startswith("split_one_token"))
    assert {1, trip - 1, trip, trip + 1} <= set(ns) and max(ns) > 2 * trip
    assert {s.G for s in F2.SPLIT_SPECS} >= {1, 2, 3, 4, 5, 7, 8}
    by = {s.id: s for s in F2.SPLIT_SPECS + F2.MMA_SPECS + F2.IMAGE_SPECS}
    assert by["split_alibi_g8"].n_splits == 2 and by["split_five_cells_chooser"].n_splits == 1 and by["split_g7"].n_splits == 1
    assert by["split_more_splits_than_cells"].n_splits > by["split_more_splits_than_cells"].nkv
    c = FR.fa_constants()
    assert by["mma_33_tile_states"].nq == c["mma_min_q"] and by["mma_264_nomask"].nq >= c["wg128_min_q"] and by["mma_ragged_cache"].nkv % c["bkv"] == 4
    assert by["mma_ragged_cache"].n_splits == 1 and by["mma_gemma2_cap_splits"].n_splits == 3
    m = F2.mask_of(by["mma_causal_hidden_and_diagonal"])[:64] == 0
    B = c["bkv"]
    states = [[("hidden" if not m[32 * qt:32 * qt + 32, B * kt:B * kt + B].any() else "open" if m[32 * qt:32 * qt + 32, B * kt:B * kt + B].all() else "diagonal") for kt in range(5)] for qt in range(2)]
    assert states == [["open", "diagonal", "hidden", "hidden", "hidden"]] * 2, states  # (kv tiles 2 .. 4 are hidden from the whole workgroup: it skips them)
    for s in F2.MMA_SPECS + F2.IMAGE_SPECS:
        assert s.nkv % 4 == 0 or s.nq < c["mma_min_q"], s.id


@pytest.mark.parametrize("spec", F2.SPLIT_SPECS + F2.MMA_SPECS, ids=lambda s: s.id)
def test_twin_against_the_oracle(H, spec):
    x = F2.make_inputs(spec)
    ref = F2.run_node(spec, x, "oracle", H)
    exact = F2.twin_of(spec, x)
    assert not np.isnan(exact).any()
    e = T.nmse(ref, exact)
    # the oracle rounds its V accumulator to f16 at every cell (2^-11 relative per step): what the GPU gate against the oracle has to leave room for
    assert e <= F2.ORACLE_F16, f"{spec.id}: oracle vs twin nmse {e:.3e}"


def test_twin_cap_is_the_ops_soft_capping(H):
    """A cap small enough to matter (scores of +-8 against a cap of 5): without the tanh the twin is far from the oracle, with it as close as uncapped."""
    spec = F2.Spec("cap_matters", "SPLIT", 4, 2, 3, 100, cap=5.0)
    x = F2.make_inputs(spec)
    x.q *= 8.0
    ref = F2.run_node(spec, x, "oracle", H)
    capped = F2.twin_of(spec, x)
    uncapped = np.stack([F2.twin(x.q[0], x.Kd, x.Vd, x.mask, 1.0 / np.sqrt(spec.HD))])
    assert T.nmse(ref, capped) <= F2.ORACLE_F16 and T.nmse(ref, uncapped) > 100 * F2.ORACLE_F16
