"""CPU checks of tests/nf_ref.py (the role test_fa_ref_host.py has for fa_ref.py): the constants parsed from attn_nf.hip / fattn_mma.hip / graph.cpp are the ones the
cases were laid out for, the case table reaches every path the kernels have, the float64 twin agrees with the CPU oracle, every generated probe meets the conditions
its gate was derived under — and the probes have teeth: a twin that drops, doubles or moves by one cell the entry at an edge slot is rejected by at least 10 x the gate."""
import time

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import nf_ref as NR

# what NR.CASES were laid out for; a constant that moves in the sources fails here, next to the name of what moved
EDGE_TABLE = {
    "cap": 1024, "threads": 256, "group_max": 512, "group": 8, "dq_max": 8, "dq_wgs": 192, "scratch_trip": 16, "t_min": 2, "t_max": 32, "g_max": 8,
    "rb": (4, 64, 16, 32, 8, 4), "named_row_max": 1024, "bkv": 64, "scan_q": 32, "mma_min_q": 33, "pick_qt": (256, 128, 64), "pick_want": 512, "pick_max": 64,
    "pick_tiles_per": 4, "rows": (2, 8, 2048),
}
TEETH = 10.0  # a mutation must miss its gate by this factor


def test_parsed_constants_match_the_edge_table():
    c = NR.nf_constants()
    for k, v in EDGE_TABLE.items():
        assert c[k] == v, f"{k}: the sources say {c[k]}, the cases of tests/nf_ref.py were laid out for {v}"
    assert [NR.dq_of(t, n) for t, n in ((24, 8), (32, 8), (12, 8), (23, 8), (6, 8), (11, 8), (5, 8), (2, 2), (2, 1))] == [1, 1, 2, 2, 4, 4, 8, 8, 8]
    assert [NR.rb_of(g, d) for g, d in ((4, 1), (5, 1), (4, 2), (5, 2), (1, 4), (8, 4), (1, 8), (8, 8))] == [16, 8, 16, 8, 8, 8, 4, 4]
    assert [NR.path_of(n, 1) for n in (0, 1, 512, 513, 1024, 1025)] == ["nan", "group", "group", "vtp", "vtp", "scratch"]
    assert [NR.path_of(n, 2) for n in (1, 512, 1024, 1025)] == ["vtp", "vtp", "vtp", "scratch"]


def _group_kinds(cells):
    """k_attn_nf_list's classification of the full groups of eight list entries: True = a run (one 16-byte load)."""
    g = NR.nf_constants()["group"]
    return [bool(cells[i + g - 1] == cells[i] + g - 1 and cells[i] % 2 == 0) for i in range(0, len(cells) - g + 1, g)]


def test_case_table_reaches_every_path():
    c = NR.nf_constants()
    by = {x.id: x for x in NR.CASES}
    assert len(by) == len(NR.CASES)
    lists = [x for x in NR.CASES if x.form == "LIST"]
    assert all(x.HD == 128 and x.nkv % 4 == 0 and x.nkv <= 4096 and x.nkv <= c["cap"] * x.T and c["t_min"] <= x.T <= c["t_max"] for x in lists)
    assert {x.G for x in lists} == set(range(1, 9))
    assert {x.dq for x in lists} == {1, 2, 4, 8}
    # V^T.p with 16, 8 and 4 rows per wave and block, on both sides of the G <= 4 choice; both mask types
    vtp = {(NR.rb_of(x.G, x.dq), x.G <= 4) for x in lists for f in x.families for n in [len(NR.list_cells(x, f, t)) for t in range(x.T)] if NR.path_of(n, x.dq) == "vtp"}
    assert vtp >= {(16, True), (8, False), (8, True), (4, True), (4, False)}, vtp
    assert {x.mtype for x in lists} == {L.F16, L.F32}
    # every rung of the count ladder, in every slice class, on the path the rung stands for
    for dq in (1, 2, 4, 8):
        rungs = {}
        for x in lists:
            if x.dq == dq and x.id.startswith("ladder"):
                for t in range(x.T):
                    n = len(NR.list_cells(x, x.families[0], t))
                    rungs[n] = NR.path_of(n, dq)
        assert set(NR.LADDER) <= set(rungs), (dq, sorted(set(NR.LADDER) - set(rungs)))
        assert {rungs[n] for n in (1500, 2100, 1025)} == {"scratch"} and rungs[0] == "nan" and rungs[1024] == "vtp" and rungs[513] == "vtp"
        assert rungs[512] == ("group" if dq == 1 else "vtp")
    # masks with a row above 1024 cells are anonymous (a mask called KQ_mask with such a row is refused)
    assert all(not x.mask_name for x in lists)
    # the layout families of the group form: what the kernel's classification makes of them
    for cid in NR.GROUP_CASES:
        x = by[cid]
        assert x.dq == 1 and set(x.families) == set(NR.LAYOUTS)
        cells = {f: [NR.list_cells(x, f, t) for t in range(x.T)] for f in x.families}
        assert all(1 <= len(cl) <= c["group_max"] and np.all(np.diff(cl) > 0) and cl[-1] < x.nkv for f in cells for cl in cells[f])
        assert all(all(_group_kinds(cl)) and len(cl) % 8 == 0 and cl[0] % 8 == 0 for cl in cells["run_aligned"])
        assert all(not any(_group_kinds(cl)) and cl[0] % 2 == 1 and cl[-1] - cl[0] == len(cl) - 1 for cl in cells["run_odd"])
        assert all(all(_group_kinds(cl)) and cl[0] % 8 in (2, 4, 6) for cl in cells["run_shift"]) and {cl[0] % 8 for cl in cells["run_shift"]} == {2, 4, 6}
        assert all(not any(_group_kinds(cl)) for cl in cells["stride"])
        assert all(any(_group_kinds(cl)) and not all(_group_kinds(cl)) for cl in cells["np"])
        assert all(len(cl) % 8 != 0 for cl in cells["partial"]) and any(len(cl) < 8 for cl in cells["partial"]) and any(len(cl) > 64 for cl in cells["partial"])
        assert all(len(cl) == c["group_max"] for cl in cells["groups64"]) and {tuple(set(_group_kinds(cl))) for cl in cells["groups64"]} == {(True,), (False,), (False, True)}
        assert all(cl[-1] == x.nkv - 1 for cl in cells["run_to_end"]) and any(all(_group_kinds(cl)) for cl in cells["run_to_end"]) and any(cl[0] % 2 for cl in cells["run_to_end"])
        assert all(cl[0] == 0 for cl in cells["run_from_zero"])
    # destinations: the copy, kqv itself, and Q8_K blocks (G even at dq = 1) or f32 rows + quantiser (G odd; dq > 1)
    assert {x.dest for x in lists} == {"copy", "kqv", "wo"}
    wo = {(x.G % 2, x.dq, x.q8_out) for x in lists if x.dest == "wo"}
    assert {(0, 1, True), (1, 1, False), (0, 2, False)} <= wo, wo
    assert any(x.scale and abs(x.scale - 1 / np.sqrt(128)) > 0.01 for x in lists)
    assert any(x.T == 2 and x.NKV in (1, 2) for x in lists) and any(x.T == 32 for x in lists) and any(x.T == 6 for x in lists)
    # refused shapes, each for its own reason
    ref = {x.id: x for x in NR.CASES if x.form == "DENSE"}
    assert ref["refused_g16"].G == 16 and ref["refused_d64"].HD == 64 and ref["refused_nkv_mod4"].nkv % 4 != 0
    assert ref["refused_average_row"].nkv > c["cap"] * ref["refused_average_row"].T and ref["refused_average_row"].nkv % 4 == 0
    x = ref["refused_named_long_row"]
    assert x.mask_name == "KQ_mask" and max(len(NR.list_cells(x, x.families[0], t)) for t in range(x.T)) > c["named_row_max"] and x.nkv <= c["cap"] * x.T
    assert ref["refused_mma_f16_mask"].T >= c["mma_min_q"] and ref["refused_mma_f16_mask"].mtype == L.F16
    # the matrix-core form
    mma = [x for x in NR.CASES if x.form == "MMA"]
    assert all(x.T <= 160 and x.nkv <= 1600 and x.nkv % 8 == 0 and x.NH in (8, 16) and x.mtype == L.F32 and x.T >= c["mma_min_q"] for x in mma)
    assert {x.T for x in mma} >= {33, 64, 65, 128, 129, 160} and {x.nkv for x in mma} == {64, 72, 256, 520, 1032, 1600} and {x.G for x in mma} == {1, 2, 4, 8}
    for x in mma:  # fa_ref.mma_splits is fattn_mma_pick_splits
        assert x.n_splits == NR.pick_splits(x.T, x.NH, x.nkv), x.id
    B = c["bkv"]
    assert any(x.n_splits == 1 for x in mma)
    assert any(x.n_splits > 1 and (x.n_splits - 1) * x.per >= x.nkv for x in mma), "no case leaves a split without a tile"
    assert by["mma_t33_kv1600_g8_kqv"].n_splits == 6 and by["mma_t33_kv1600_g8_kqv"].per == 5 * B
    assert any(x.n_splits > 1 and 0 < x.nkv - (x.n_splits - 1) * x.per < x.per - B for x in mma), "no short last split"
    assert any(x.nkv % B for x in mma)
    assert {x.dest for x in mma} == {"copy", "kqv", "wo"} and {x.q8_out for x in mma if x.dest == "wo"} == {True, False}
    for x in mma:  # every tile state occurs in the tile_states family, next to a token that sees nothing
        vis, vals = NR.family_vis(x, "tile_states")
        st = set()
        for qt in range(0, x.T, c["scan_q"]):
            for kt in range(0, x.nkv, B):
                blk = vis[qt:qt + c["scan_q"], kt:kt + B]
                zero = blk.all() and kt + B <= x.nkv and not np.signbit(vals[qt:qt + c["scan_q"], kt:kt + B]).any()
                st.add(0 if not blk.any() else (2 if zero else 1))
        assert st == {0, 1, 2} if x.nkv >= 3 * B else 1 in st, (x.id, st)  # (one or two tiles cannot show all three)
        assert (not vis[5].any()) == (x.dest != "wo")
    # edge sets: both sides of what the issue names
    e = NR.list_edges(2100)
    assert {0, 2099, 7, 8, 15, 16, 255, 256, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2095, 2096} <= set(e)
    assert {1007, 1008, 1015, 1016} <= set(NR.list_edges(1020))  # the last trip of 16 and the last group of eight
    assert NR.list_edges(1) == [0] and NR.list_edges(9) == [0, 1, 7, 8]
    e = NR.mma_edges(by["mma_t33_kv1600_g8_kqv"])
    assert {0, 1599, 63, 64, 1535, 1536, 319, 320, 1279, 1280} <= set(e)


def test_twin_is_the_chain_written_out():
    """The twin (dense and list paths) against a per-row restatement of ggml-cpu's steps, finite mask values and an empty row included."""
    rng = np.random.default_rng(5)
    NH, NKV, T_, nkv, D = 6, 2, 5, 40, 128
    q = rng.standard_normal((T_, NH, D)).astype(np.float32)
    K, V = rng.standard_normal((nkv, NKV, D)), rng.standard_normal((nkv, NKV, D))
    mask = rng.choice(np.array([0.0, -np.inf, -1.5, 0.75, -0.0], np.float16), (64, nkv))
    mask[3] = -np.inf
    out, den = NR.twin(q, K, V, mask, 0.07)
    lists = [np.flatnonzero(mask[t] != -np.inf) for t in range(T_)]
    out_l, den_l = NR.twin_lists(q, K, V, lists, [mask[t, lists[t]] for t in range(T_)], 0.07)
    assert np.isnan(out[3]).all() and np.isnan(out_l[3]).all() and np.isnan(den[3]).all()
    for t in (0, 1, 2, 4):
        for h in range(NH):
            s = K[:, h // 3] @ q[t, h].astype(np.float16).astype(np.float64) * 0.07 + mask[t].astype(np.float64)
            e = np.exp(s - s.max())
            p = (e / e.sum()).astype(np.float16).astype(np.float64)
            assert np.allclose(out[t, h], p @ V[:, h // 3], rtol=1e-12, atol=1e-14) and np.isclose(den[t, h], e.sum(), rtol=1e-13)
            assert np.allclose(out_l[t, h], out[t, h], rtol=1e-12, atol=1e-14) and np.isclose(den_l[t, h], den[t, h], rtol=1e-13)


HOST_CASES = [
    NR.Case("host_list_f32", "LIST", 8, 2, 4, 256, ("np", NR._counts([0, 1, 9, 130]))),
    NR.Case("host_list_f16", "LIST", 6, 2, 3, 512, (NR._counts([300, 64, 7]),), mtype=L.F16, dest="kqv"),
    NR.Case("host_mma_f32", "MMA", 8, 4, 40, 136, ("full", "tile_states", "causal_end")),
    NR.Case("host_dense_f16", "DENSE", 8, 4, 33, 128, ("full", "causal_end"), mtype=L.F16),
    NR.Case("host_list_wo", "LIST", 4, 2, 4, 256, ("np",), dest="wo"),
]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.id)
def test_twin_agrees_with_the_oracle(H, plog, case):
    """One small case per form and mask type: the oracle passes every probe at the gates the GPU file uses, and random data is within the chain's gate of the twin."""
    nth = T.host_threads(8)
    wo = case.dest == "wo"
    for p in NR.indicator_probes(case) + NR.witness_probes(case) + NR.witness_probes(case, True):
        NR.check_probe(case, p, NR.run_probe(case, p, "oracle", H, nth), quant_step=wo)
    p = NR.random_probe(case)
    got = NR.run_probe(case, p, "oracle", H, nth)
    if wo:  # read through the Q8_K activation: half a quantisation step of each 256-value block, plus 1e-4 of the block maximum for the f32 arithmetic (test_fa_cells' rule)
        amax = np.abs(p.expect.reshape(-1, 256)).max(axis=1)
        over = float(((np.abs(got.astype(np.float64) - p.expect).reshape(-1, 256) - (amax / 254)[:, None]) / amax[:, None]).max())
        plog(f"nf_ref twin against the oracle, {case.id}: random, {over:.3e} of the block maximum beyond half a quantisation step")
        assert over <= 1e-4, over
        return
    e = NR.nmse_rows(got, p.expect)
    plog(f"nf_ref twin against the oracle, {case.id}: random nmse={e:.3e}")
    assert e <= NR.RANDOM_GATE, e


def _entry(cells, cell):
    i = int(np.searchsorted(cells, cell))
    assert cells[i] == cell
    return i


def _mutants(cells, e, nkv, double=True):
    """The list with entry e dropped, doubled, and moved to the neighbouring cell."""
    nb = cells[e] + 1 if cells[e] + 1 < nkv else cells[e] - 1
    moved = cells.copy()
    moved[e] = nb
    out = {"drop": np.delete(cells, e), "shift": moved}
    if double:
        out["double"] = np.append(cells, cells[e])
    return out


def _figure(case, p, t, cells, h=None):
    """max |mutated twin - expectation| of token t (indicator: its first KV head, times the denominator; otherwise head h; NaN counts as infinite), in the probe's own units."""
    if h is None:
        hs, ks = slice(0, case.G), slice(0, 1)
    else:
        hs, ks = slice(h, h + 1), slice(h // case.G, h // case.G + 1)
    sc = p.scores[t:t + 1, hs] if getattr(p, "scores", None) is not None else None
    out, _ = NR.twin_lists(p.q[t:t + 1, hs], p.Kd[:, ks], p.Vd[:, ks], [cells], [np.zeros(len(cells))], case.sc, sc)
    dev = np.abs(out[0] - p.expect[t, hs])
    if p.name.startswith("indicator"):
        dev = dev * p.den[t, hs, None]
        if case.dest == "wo":  # the half quantisation step check_probe allows, in the same units
            dev = dev - np.abs(p.expect[t, hs]).max() / 254 * p.den[t, hs, None]
    return float(np.where(np.isnan(dev), np.inf, dev).max())


@pytest.mark.parametrize("case", NR.CASES, ids=lambda c: c.id)
def test_probes_pass_on_the_twin_and_have_teeth(case, plog):
    t0 = time.time()
    wo = case.dest == "wo"
    ind = NR.indicator_probes(case)
    assert {p.name.split("_", 2)[2] for p in ind} == set(case.families)
    for p in ind:
        assert NR.check_probe(case, p, p.expect.astype(np.float32), quant_step=wo) <= 1e-3  # (f32 rounding of the expectation itself)
    # indicator: mutate every edge slot of the longest, the shortest and a middle list of the edge family
    p = ind[0]
    lists = NR.token_lists(case)
    order = [t for t in np.argsort([len(x) for x in lists]) if len(lists[t])]
    n_mut = 0
    for t in sorted({order[0], order[len(order) // 2], order[-1]}):
        cells = lists[t]
        slots = NR.edges_of(case, len(cells)) if case.form != "MMA" else [_entry(cells, c) for c in NR.mma_edges(case) if c in set(cells)]
        for e in slots:
            for what, mut in _mutants(cells, e, case.nkv, double=len(cells) > 1).items():
                f = _figure(case, p, t, mut)
                assert f >= TEETH * NR.INDICATOR_GATE, f"{case.id} {p.name}: {what} of entry {e} of token {t} ({len(cells)} cells) moves the figure by {f:.3e} only"
                n_mut += 1
    # witness and pair probes: the conditions of their gate, then the same mutations at the witness' own entry (a doubled witness still weighs 1.0: the pair probe sees
    # that one).  Every head of a token carries another slot; in the matrix-core form every token has the same edge set, so three tokens reach all of it.
    owned = {False: set(), True: set()}
    for pair in (False, True):
        for p in NR.witness_probes(case, pair):
            assert p.margin >= NR.MARGIN_NATS and p.residual <= 1e-9, (p.name, p.margin, p.residual)
            NR.check_probe(case, p, p.expect.astype(np.float32), quant_step=wo)
            mid = "_mid_" in p.name
            if mid:
                owned[pair].update(p.own)
            wit, part = p.witness
            vis = np.asarray(p.mask[: case.T], np.float32) != -np.inf
            toks = sorted({t for t, _ in p.own})
            if case.form == "MMA":
                toks = sorted({toks[0], toks[len(toks) // 2], toks[-1]})
            done = set()
            for t in toks:
                cells = np.flatnonzero(vis[t])
                for h in range(case.NH) if mid and not pair else (0,):
                    for c in (wit[t, h], part[t]) if pair else (wit[t, h],):
                        if (t, c) in done:
                            continue
                        done.add((t, c))
                        for what, mut in _mutants(cells, _entry(cells, c), case.nkv, double=pair).items():
                            f = _figure(case, p, t, mut, h)
                            assert f >= TEETH * NR.WITNESS_GATE * p.vmax, f"{case.id} {p.name}: {what} of cell {c} of token {t} moves the result by {f:.3e} only"
                            n_mut += 1
    # every entry of every token's edge set is some head's witness, every boundary some token's own pair
    assert owned[False] == {(t, s) for t in range(case.T) for s in range(len(NR.edges_of(case, len(lists[t]))))}, case.id
    assert owned[True] == {(t, s) for t in range(case.T) for s in range(len(NR.pair_ends_of(case, len(lists[t]))))}, case.id
    p = NR.random_probe(case)
    assert np.isfinite(p.expect[~np.isnan(p.den).any(axis=1)]).all()
    plog(f"nf_ref host {case.id}: {len(ind)} indicator probes, {n_mut} mutations rejected ({time.time() - t0:.1f} s)")
