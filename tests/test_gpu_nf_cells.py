"""Cell accounting of the non-flash attention chain on the GPU: every case of tests/nf_ref.py — every template form G = 1 .. 8 and slice count of k_attn_nf_list, every
rung of the count ladder (empty list, group form, the three V^T.p forms, the scratch path), the list layouts of the group form, the three destinations; k_attn_nf_mma with
one split, a short last split and a split without a tile, part-filled query tiles and every tile state — runs the indicator probe over every visibility family, a witness
sweep over its edge set, pair probes across its boundaries and one random-data probe, and states the form it expects: a case whose form did not run (counters
nf_list_chains / nf_mma_chains) fails.  Inputs, expectations and gates come from tests/nf_ref.py (derivations there; test_nf_ref_host.py proves them on the CPU)."""
import dataclasses
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import harness as T
import nf_ref as NR

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(case, p, H):
    """The CPU oracle's result of a case's random probe: computed once."""
    if case.id not in _ORACLE:
        _ORACLE[case.id] = NR.run_probe(case, p, "oracle", H, T.host_threads(8))
    return _ORACLE[case.id]


def _run(backend, H, case, p, bad):
    try:
        got, wrong = NR.run_counted(case, p, backend, H)
    except AssertionError as e:
        bad.append(str(e))
        return None
    if wrong:
        bad.append(wrong)
    return got


def _gate(case, p, got, bad, worst):
    if got is None:
        return
    try:
        w = NR.check_probe(case, p, got, quant_step=case.dest == "wo")
        kind = p.name.split("_")[0]
        worst[kind] = max(worst.get(kind, 0.0), w)
    except AssertionError as e:
        bad.append(str(e))


def _random(backend, H, case, bad, worst):
    p = NR.random_probe(case)
    got = _run(backend, H, case, p, bad)
    if got is None:
        return p, got
    lim = NR.RANDOM_GATE_WO if case.dest == "wo" else NR.RANDOM_GATE
    try:
        worst["random"] = NR.nmse_rows(got, _oracle(case, p, H))
        if not worst["random"] <= lim:
            bad.append(f"{case.id} random: nmse {worst['random']:.3e} against the oracle > {lim}")
    except AssertionError as e:
        bad.append(f"{case.id} random: {e}")
    return p, got


def _sweep(backend, H, case, bad, worst, keep=None):
    """Every probe of the case; keep: a dict that receives name -> result."""
    for p in NR.indicator_probes(case):
        got = _run(backend, H, case, p, bad)
        _gate(case, p, got, bad, worst)
        if keep is not None:
            keep[p.name] = got
    for pair in (False, True):
        for p in NR.witness_probes(case, pair):
            got = _run(backend, H, case, p, bad)
            _gate(case, p, got, bad, worst)
            if keep is not None:
                keep[p.name] = got
    p, got = _random(backend, H, case, bad, worst)
    if keep is not None:
        keep[p.name] = got


@pytest.mark.parametrize("case", [c for c in NR.CASES if c.form != "DENSE"], ids=lambda c: c.id)
def test_nf_cells(backend, H, plog, case):
    t0 = time.time()
    bad, worst, keep = [], {}, {}
    _sweep(backend, H, case, bad, worst, keep)
    if case.dest == "wo" and case.form == "LIST":
        # as test_non_flash_attention_chain_into_wo asserts: the Q8_K blocks written by the launch and the f32 rows + quantiser launch (prologue = 0) give the same bits
        backend.set_option("prologue", 0)
        try:
            for p in (NR.indicator_probes(case, case.families[:1])[0], NR.witness_probes(case)[0], NR.random_probe(case)):
                plain = _run(backend, H, case, p, bad)
                if plain is not None and keep[p.name] is not None and not np.array_equal(plain.view(np.uint32), keep[p.name].view(np.uint32)):
                    bad.append(f"{case.id} {p.name}: prologue = 1 and prologue = 0 differ in {np.count_nonzero(plain != keep[p.name])} values")
        finally:
            backend.set_option("prologue", 1)
    plog(f"nf_cells {case.id} [{case.form} G={case.G} dq={case.dq} splits={case.n_splits} dest={case.dest}{' q8' if case.q8_out else ''}]: "
         + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" ({len(keep)} probes, {time.time() - t0:.1f} s)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("form", ["LIST", "MMA"])
def test_nf_token_that_sees_nothing(backend, H, plog, form):
    """A token whose mask row is all -inf: the CPU's row is expf(-inf - -inf) = NaN throughout; the other tokens' rows stay finite and in gate.  List form: empty lists
    in the group form's batch (dq = 1) and with slices of the head dimensions; matrix-core form: one token inside a query tile, and a whole 32-query tile."""
    if form == "LIST":
        cases = [NR.Case("nothing_list_dq1", "LIST", 32, 8, 24, 1024, (NR._counts([0, 40, 0] + [8 * t for t in range(3, 23)] + [0]),)),
                 NR.Case("nothing_list_dq8", "LIST", 6, 2, 3, 1024, (NR._counts([600, 0, 9]),), mtype=NR.L.F16)]
    else:
        cases = [next(c for c in NR.CASES if c.id == "mma_t65_kv256_g4")]
    for case in cases:
        probes = NR.indicator_probes(case, ("tile_states",) if form == "MMA" else None)[:1]
        if form == "MMA":  # ... and every token of the second query tile
            p = probes[0]
            mask = p.mask.copy()
            mask[32:64] = -np.inf
            exp, den = NR.twin(p.q, p.Kd, p.Vd, mask, case.sc)
            probes.append(dataclasses.replace(p, name="indicator_A_tile_states_empty_query_tile", mask=mask, expect=exp, den=den))
        for p in probes:
            nan_rows = np.isnan(p.expect).all(axis=(1, 2))
            assert nan_rows.any() and not nan_rows.all()
            ref = NR.run_probe(case, p, "oracle", H)
            assert np.array_equal(np.isnan(ref).all(axis=(1, 2)), nan_rows) and np.isnan(ref[nan_rows]).all()
            bad = []
            got = _run(backend, H, case, p, bad)
            assert not bad, bad
            assert np.isnan(got[nan_rows]).all() and not np.isnan(got[~nan_rows]).any()
            w = NR.check_probe(case, p, got)
            plog(f"nf_cells {case.id} {p.name}: {int(nan_rows.sum())} NaN rows as the oracle's, the others at {w:.2e}")


@pytest.mark.parametrize("case", [c for c in NR.CASES if c.form == "DENSE"], ids=lambda c: c.id)
def test_nf_refused_shapes_take_the_dense_kernels(backend, H, plog, case):
    """Shapes neither form serves: the counters stay, and the dense kernels give the chain's result — the witness and pair probes (exact whatever the order of the sums)
    and random data against the oracle."""
    t0 = time.time()
    bad, worst = [], {}
    for pair in (False, True):
        for p in NR.witness_probes(case, pair):
            _gate(case, p, _run(backend, H, case, p, bad), bad, worst)
    _random(backend, H, case, bad, worst)
    plog(f"nf_cells {case.id} [dense kernels]: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" ({time.time() - t0:.1f} s)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


def test_nf_group_form_against_the_gather_form(backend, H, plog):
    """GGML_MI355X_NF_GROUPS=0 (read once per process: a fresh child) sends the lists of the group form through the gather form of V^T.p.  Indicator, witness and pair
    results are exact in any order of the sums (k * p and 0.5 * V on their grids): bit-equal between the two; the child's random data is gated against the oracle."""
    assert os.environ.get("GGML_MI355X_NF_GROUPS", "1") != "0", "this process must run the group form"
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "gather.npz")
        env = dict(os.environ, GGML_MI355X_NF_GROUPS="0")
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "nf_groups_worker.py"), out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("NF_GROUPS_JSON "))
        info = json.loads(line[len("NF_GROUPS_JSON "):])
        child = dict(np.load(out))
    assert info["env"] == "0" and info["bad"] == [], info
    bad, n = [], 0
    for cid in NR.GROUP_CASES:
        case = next(c for c in NR.CASES if c.id == cid)
        mine, worst = {}, {}
        _sweep(backend, H, case, bad, worst, mine)
        for name, got in mine.items():
            other = child[f"{cid}|{name}"]
            n += 1
            if name == "random":
                e = NR.nmse_rows(other, _oracle(case, NR.random_probe(case), H))
                if not e <= NR.RANDOM_GATE:
                    bad.append(f"{cid} random in the gather form: nmse {e:.3e} against the oracle")
            elif got is None or not np.array_equal(got.view(np.uint32), other.view(np.uint32)):
                bad.append(f"{cid} {name}: group form and gather form differ in {np.count_nonzero(got != other) if got is not None else 'all'} values")
    plog(f"nf_cells group form against the gather form: {n} probes compared ({time.time() - t0:.1f} s)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])
