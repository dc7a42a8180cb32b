"""CPU checks of tests/fa_ref.py: the constants parsed from the attention kernels still give the edge table the cases were laid out for, every generated
probe input meets the conditions its gate was derived under, and the CPU oracle passes every probe of every case at the gates the GPU file uses — which
proves inputs, twin and expectations without a GPU."""
import dataclasses

import numpy as np
import pytest

import fa_ref as FR
import harness as T
import llama_box_amd as L

# what the cases of fa_ref.CASES were laid out for; a constant that moves in the kernels fails here, next to the name of what moved
EDGE_TABLE = {
    "dims_per_lane": 8, "wave": 64, "split_ng": 4, "bkv": 64, "scan_q": 32, "wg128_min_q": 256, "nw_big": 4, "nw_small": 2, "q_per_wave": 32,
    "pos_scan_pass": 1024, "mma_min_q": 33, "rows_min": 2048, "rows_splits": (2, 8), "skip_trips": 32, "skip_round": 64, "fat_trip": 32, "fat_max": 12,
    "dec_want": 768, "dec_len": 86, "dec_cap": 256, "mma_want": 512, "mma_max": 64, "mma_tiles_per": 4,
}
TRIPS = {  # (head size, query heads per KV head, waves, kernel) -> cells per trip
    (128, 1, 4, "dec"): 128, (128, 2, 4, "dec"): 128, (128, 3, 4, "dec"): 64, (128, 4, 4, "dec"): 64, (128, 8, 4, "dec"): 32, (128, 2, 8, "dec"): 256, (128, 8, 8, "dec"): 64,
    (64, 1, 4, "dec"): 128, (64, 2, 4, "dec"): 128, (64, 3, 4, "dec"): 64, (64, 3, 8, "dec"): 128, (64, 4, 4, "dec"): 64, (64, 8, 4, "dec"): 32, (64, 8, 8, "dec"): 64, (128, 2, 4, "split"): 64, (64, 2, 4, "split"): 128,
}


def test_parsed_constants_match_the_edge_table():
    c = FR.fa_constants()
    for k, v in EDGE_TABLE.items():
        assert c[k] == v, f"{k}: the kernels say {c[k]}, the edge table of tests/fa_ref.py was laid out for {v}"
    for (D, G, wv, kern), t in TRIPS.items():
        assert FR.trip_len(D, G, wv, kern) == t, (D, G, wv, kern)
    f = c["form"]
    assert len(set(v for k, v in f.items() if k.startswith("FA_FORM_TAIL_"))) == 6 and f["FA_FORM_K_MMA"] == 3


def test_split_choosers_and_case_geometry():
    by = {c.id: c for c in FR.CASES}
    assert len(by) == len(FR.CASES)
    assert by["wide8_d64_g8_chooser"].n_splits == 47 and by["wide8_d64_g8_chooser"].per() == 88
    assert by["mma_d64_264_chooser"].n_splits == 16 and by["mma_d64_264_chooser"].per() == 5 * 64
    assert (by["fat_one_trip_splits"].n_splits, by["fat_one_trip_splits"].per()) == (9, 228)   # nine trips of 256 -> nine splits
    assert (by["fat_two_trip_splits"].n_splits, by["fat_two_trip_splits"].per()) == (9, 456)   # 17 trips -> 9 splits of two
    assert by["skip_d128_g3_sinks"].per() == 384 and by["skip_d128_g3_sinks"].per() <= FR.fa_constants()["skip_trips"] * by["skip_d128_g3_sinks"].trip
    c = FR.fa_constants()
    rows = by["mma_d128_rows"]
    assert rows.nq * rows.NH >= c["rows_min"] and c["rows_splits"][0] <= rows.n_splits <= c["rows_splits"][1]
    assert by["mma_d128_264_nomask"].nq >= c["wg128_min_q"] and by["mma_d128_264_nomask"].nq % (c["nw_big"] * c["q_per_wave"]) != 0  # a ragged second 128-query tile
    assert by["mma_d128_33"].nq == c["mma_min_q"] and by["list_d128_g8_splits"].nq == c["mma_min_q"] - 1
    for case in FR.CASES:  # the edge set of every case holds both sides of a trip end and, with splits, of a split boundary
        for t in (0, case.nq - 1):
            ed, n = FR.edges_of(case, t), len(FR.token_cells(case, t))
            assert {0, n - 1} <= set(ed) and all(0 <= e < n for e in ed)
            if case.trip + 1 < n:
                assert {case.trip - 1, case.trip} <= set(ed), case.id
            per = case.per(n)
            if case.n_splits > 1 and per < n:
                assert {per - 1, per} <= set(ed), case.id
        if case.kernel == "DEC" and case.mode in (1, 2) or case.kernel == "MMA":
            assert case.nkv % 4 == 0, case.id
    # G from {1, 2, 3, 4, 8} at both head sizes, and a group smaller than its template (1 -> 2, 3 -> 4) in plain, wide, list, skip and self-merging forms
    for HD in (64, 128):
        assert {1, 2, 3, 4, 8} <= {c.G for c in FR.CASES if c.HD == HD}, HD
    short = {(c.HD, c.mode, c.waves, c.tail) for c in FR.CASES if c.kernel == "DEC" and c.G < FR.gg(c.G)}
    assert {(64, 0, 4, "NONE"), (64, 0, 8, "COMBINE"), (64, 2, 4, "NONE"), (64, 2, 4, "COMBINE"), (128, 2, 4, "NONE"), (128, 1, 4, "COMBINE"), (128, 2, 4, "SELF_MERGE")} <= short, short
    kinds = {(c.kernel, c.mode, c.waves, c.tail, c.HD, c.kv, c.kvform) for c in FR.CASES}
    assert len(kinds) >= 25  # distinct kernel forms in the table


def test_twin_is_the_expression_of_test_flash_attn():
    """The twin against a per-row restatement with sinks, grouped heads, ALiBi slopes and finite mask values."""
    rng = np.random.default_rng(5)
    NH, NKV, nq, nkv, HD = 6, 2, 3, 37, 64
    q = rng.standard_normal((NH, nq, HD)).astype(np.float32)
    K, V = rng.standard_normal((nkv, NKV, HD)), rng.standard_normal((nkv, NKV, HD))
    mask = rng.choice(np.array([0.0, -np.inf, -1.5, 0.75], np.float16), (64, nkv))
    mask[:, 0] = 0
    sk = rng.standard_normal(NH).astype(np.float32)
    out, den, _ = FR.twin(q, K, V, mask, 0.125, sk, alibi=8.0)
    n2 = 4
    for h in range(NH):
        slope = (2.0 ** (-8.0 / n2)) ** (h + 1) if h < n2 else (2.0 ** (-8.0 / 2 / n2)) ** (2 * (h - n2) + 1)
        for t in range(nq):
            s = K[:, h // 3] @ q[h, t].astype(np.float16).astype(np.float64) * 0.125 + slope * mask[t].astype(np.float64)
            m = max(s.max(), float(sk[h]))
            p = np.exp(s - m)
            d = p.sum() + np.exp(float(sk[h]) - m)
            assert np.allclose(out[t, h], p @ V[:, h // 3] / d, rtol=1e-13, atol=1e-15) and np.isclose(den[t, h], d, rtol=1e-13)


def test_gates_catch_one_cell():
    """One dropped, one doubled and one neighbouring cell, applied to the twin itself, fail the indicator gate; a dropped witness fails the witness gate."""
    case = next(c for c in FR.CASES if c.id == "list_d128_g3_one")
    p = next(x for x in FR.indicator_probes(case) if x.name == "indicator_A_interleaved")
    FR.check_probe(case, p, p.expect.astype(np.float32))
    vis = np.isfinite(p.mask[: case.nq].astype(np.float32))
    for what in ("drop", "double", "neighbour"):
        w = vis.astype(np.float64)
        c = np.flatnonzero(vis[2])[-1]
        if what == "drop":
            w[2, c] = 0
        elif what == "double":
            w[2, c] = 2
        else:
            w[2, c], w[2, c - 1] = 0, w[2, c - 1] + 1
        bad = np.stack([(w @ p.Vd[:, h // case.G]) / w.sum(axis=1, keepdims=True) for h in range(case.NH)], axis=1)
        with pytest.raises(AssertionError):
            FR.check_probe(case, p, bad.astype(np.float32))
    wp = FR.witness_probes(case)[0]
    bad = wp.expect.copy()
    bad[1, 0] = wp.Vd[0, 0]
    with pytest.raises(AssertionError):
        FR.check_probe(case, wp, bad.astype(np.float32))


@pytest.mark.parametrize("case", FR.CASES, ids=lambda c: c.id)
def test_oracle_passes_every_probe(H, case):
    """Inputs, twin and expectations are right if the CPU oracle — another implementation, f16 accumulation of V and all — passes the gates; the conditions the
    gates were derived under are asserted on every generated input.  (Quantised caches: the oracle quantises the query as the lane kernels do, so its pass
    shows that the 60-nat margin survives the 8-bit query.)"""
    nth = T.host_threads(8)
    if case.kvform == "Q8_IMAGE":  # the oracle reads the blocks themselves, not their f16 image: same inputs, expectations without the image's rounding
        case = dataclasses.replace(case, kvform="")
    n = 0
    for p in FR.indicator_probes(case):
        FR.check_probe(case, p, FR.run_probe(case, p, "oracle", H, nth), quant_step=case.wo)
        n += 1
    assert n >= (1 if not case.masked else 4)
    for pair in (False, True):
        if pair and case.n_splits == 1 and case.trip >= case.nkv:
            continue
        own = set()
        for p in FR.witness_probes(case, pair):
            assert p.margin >= FR.MARGIN_NATS and p.residual <= 1e-9, (p.name, p.margin, p.residual)
            own.update(p.own)
            FR.check_probe(case, p, FR.run_probe(case, p, "oracle", H, nth), quant_step=case.wo)
        # every edge of the case's edge set is probed at its own position (a pair that collides with another token's falls back to token 0's: never for all its tokens)
        assert own == set(range(len(FR.edges_of(case, 0)))), (case.id, pair, sorted(own))
    p = FR.random_probe(case)
    got = FR.run_probe(case, p, "oracle", H, nth)
    if not case.wo:  # (the oracle's own distance from exact attention: its f16 V accumulator, and the 8-bit query over a quantised cache)
        assert T.nmse(got, p.expect) <= (1e-4 if case.kv == L.F16 else 1e-3)
