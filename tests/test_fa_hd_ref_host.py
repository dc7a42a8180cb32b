"""CPU checks of tests/fa_hd.py: the head-size field of the form code against kernels.h (no earlier code moved), the padded geometry the specs are laid out for, and
the float64 twin against the CPU oracle at every shape and in every layout test_gpu_fa_hd.py runs, at that file's oracle gate: the reference alone stays inside it, so
a GPU failure there is the kernels'.  The gap layout's NaN never reaches the oracle's result either: it reads what the view describes."""
import numpy as np
import pytest

import fa_d256 as F2
import fa_hd as FH
import fa_ref as FR
import harness as T
import llama_box_amd as L
from test_fa_d256_ref_host import CODES_BEFORE


def test_form_codes_are_distinct_and_none_moved():
    f = FR.fa_constants()["form"]
    shift = f["FA_FORM_HD_SHIFT"]
    assert shift == 17 and shift > f["FA_FORM_D256_BIT"]  # above the tail field (bits 13..15, which fa_form_tail rewrites) and the 256 bit
    vals = [f[f"FA_FORM_HD_{D}"] for D in FH.SIZES]
    assert len(set(vals)) == 4 and all(1 <= v <= 7 for v in vals)
    by = {c.id: c for c in FR.CASES}
    for cid, code in CODES_BEFORE.items():
        assert by[cid].form == code, cid
    old = {c.form for c in FR.CASES} | {s.form for s in F2.SPLIT_SPECS + F2.MMA_SPECS + F2.IMAGE_SPECS}
    assert all(c & FH.hd_mask() == 0 and c < (1 << shift) for c in old)
    new = {}
    for kern in ("SPLIT", "MMA"):
        for mode in (0, 1):
            for waves in (2, 4):
                for tail in ("NONE", "COMBINE"):
                    codes = [FH.form(kern, mode, waves, D, tail) for D in FH.SIZES]
                    assert len(set(codes)) == 4 and not set(codes) & old
                    for D, c in zip(FH.SIZES, codes):
                        assert c & ~FH.hd_mask() == FR.form(kern, mode, waves, "F16", 64, tail)  # the head-size-64 code with the field ORed on
                        assert FH.form_name(c).split("D=")[1].split()[0] == str(D)
                        new[c] = (kern, mode, waves, D, tail)
    assert len(new) == 2 * 2 * 2 * 2 * 4
    assert FH.form_name(by["mma_d128_33"].form) == FR.form_name(by["mma_d128_33"].form)


def test_spec_geometry():
    c = FR.fa_constants()
    assert FH.TRIP == c["split_ng"] * 4 * (c["wave"] // FH.ROW_LANES) == 64
    for D in FH.SIZES:
        assert D % 8 == 0 and D % 32 != 0 and D // 8 < FH.ROW_LANES and FH.PADDED[D] % 32 == 0 and 0 < FH.PADDED[D] - D < 32
        assert ((FH.PADDED[D] + 8) * 2 // 16) % 2 == 1  # the K tile's row stride stays an odd multiple of 16 bytes
        ns = {s.nkv for s in FH.SPLIT_ALL if s.HD == D and "one_token" in s.id}
        assert {1, FH.TRIP - 1, FH.TRIP, FH.TRIP + 1} <= ns and max(ns) > 2 * FH.TRIP
        assert sum(1 for s in FH.SPLIT_ONE if s.HD == D) >= 2
    assert (72 // 8) % 2 == 1 and (88 // 8) % 2 == 1  # a half-live last k-step of 16 dims
    assert {s.G for s in FH.SPLIT_ALL + FH.SPLIT_ONE} >= {1, 3, 5, 7, 8}
    by = {s.id: s for s in FH.RANDOM_SPECS + FH.CELL_SPECS + [FH.HIPGRAPH_SPEC]}
    assert len(by) == len(FH.RANDOM_SPECS) + len(FH.CELL_SPECS) + 1
    assert by["d72_more_splits_than_cells"].n_splits > by["d72_more_splits_than_cells"].nkv
    assert by["d112_32_tokens"].nq == c["mma_min_q"] - 1 and by["d112_32_tokens"].n_splits == 2
    assert by["d80_sinks_five_tokens"].n_splits == 2 and by["d112_cap50_three_splits"].n_splits == 3 and by["d80_two_batches"].nb == 2
    for D in FH.SIZES:
        assert by[f"d{D}_mma_33_tile_states"].nq == c["mma_min_q"] and by[f"d{D}_mma_264_nomask"].nq >= c["wg128_min_q"]
        assert by[f"d{D}_holes_g2_three_splits"].n_splits == 3
        case = FH.fr_case(by[f"d{D}_cells_split_sinks_g4"])
        assert case.trip == FH.TRIP and case.per(case.nkv) == 130 and {63, 64, 65, 129, 130, 131, 259} <= set(FR.edges_of(case, 0))
        case = FH.fr_case(by[f"d{D}_cells_mma_33"])
        assert case.trip == c["bkv"] and {63, 64, 65, 255, 256, 259} <= set(FR.edges_of(case, 0))
    assert by["d72_mma_ragged_cache"].nkv % c["bkv"] == 4 and by["d80_mma_40_three_splits"].n_splits == 3
    assert by["d72_kv_262_keeps_split"].nkv % 4 != 0 and by["d72_kv_262_keeps_split"].nq >= c["mma_min_q"] and by["d72_kv_262_keeps_split"].kernel == "SPLIT"
    assert by["d112_cap_40_tokens_keep_split"].cap != 0 and by["d112_cap_40_tokens_keep_split"].kernel == "SPLIT"
    m = F2.mask_of(by["d88_mma_causal_hidden_and_diagonal"])[:64] == 0
    B = c["bkv"]
    states = [[("hidden" if not m[32 * qt:32 * qt + 32, B * kt:B * kt + B].any() else "open" if m[32 * qt:32 * qt + 32, B * kt:B * kt + B].all() else "diagonal") for kt in range(5)] for qt in range(2)]
    assert states == [["open", "diagonal", "hidden", "hidden", "hidden"]] * 2, states
    for s in FH.RANDOM_SPECS + FH.CELL_SPECS:
        if s.kernel == "MMA":
            assert s.nkv % 4 == 0 and s.nq >= c["mma_min_q"] and s.cap == 0 and not s.sinks and s.alibi == 0, s.id
            assert (s.form >> 6) & 15 == (c["nw_big"] if s.nq >= c["wg128_min_q"] else c["nw_small"])
        assert (s.form & 15) == c["form"]["FA_FORM_K_" + s.kernel] and s.form & FH.hd_mask() == FH.hd_field(s.HD)
    assert {(s.HD, s.layout) for s in FH.LAYOUT_SPECS} == {(72, "tower"), (88, "tower"), (72, "gap"), (112, "gap")}


@pytest.mark.parametrize("spec", FH.RANDOM_SPECS + [FH.HIPGRAPH_SPEC], ids=lambda s: s.id)
def test_twin_against_the_oracle(H, spec):
    x, ref, exact = FH.reference(spec, H)
    assert not np.isnan(exact).any() and not np.isnan(ref).any()
    e = T.nmse(ref, exact)
    assert e <= F2.ORACLE_F16, f"{spec.id}: oracle vs twin nmse {e:.3e}"


def test_layouts_describe_the_same_attention(H):
    """The tower and gap builders hand the oracle the values of the cache layout: the three results agree bit for bit (the oracle's arithmetic does not depend on strides)."""
    for spec in FH.LAYOUT_SPECS:
        x, ref, _ = FH.reference(spec, H)
        same = FH.Spec(**{**{k: getattr(spec, k) for k in spec.__dataclass_fields__}, "layout": "cache"})
        assert np.array_equal(F2.run_node(same, x, "oracle", H).view(np.uint32), ref.view(np.uint32)), spec.id


def test_refused_nodes_can_be_built(H):
    """The nodes test_gpu_fa_hd.py asserts refused are well-formed graphs (built on the CPU side here; nothing is computed)."""
    builds = FH.refused_builders(H)
    assert len(builds) == 6 + 3 + 4 * 6
    for name, build in builds:
        g = T.G("oracle")
        try:
            r = build(g)
            assert r.contents.ne[0] > 0, name
        finally:
            g.free()
