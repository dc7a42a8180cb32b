"""FLASH_ATTN_EXT cell accounting on the GPU: every kernel form of fattn.hip / fattn_mma.hip that can be reached in process runs the indicator probe over every
mask family its shape admits, a witness sweep over its edge set (both sides of a trip end, of the first and the last split boundary, the cache ends; list forms: entry indices
into scattered lists), a pair probe across trips / splits, and one random-data case — and states the form it expects, read back through stat "fa_form".  A case
whose expected form did not run fails.  Inputs, expectations and gates come from tests/fa_ref.py (derivations there; test_fa_ref_host.py proves them on the CPU).
"""
import dataclasses
import time

import numpy as np
import pytest

import fa_ref as FR
import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu


def _options(backend, case, self_merge=None):
    backend.set_option("fa_splits", case.splits)
    backend.set_option("fa_self_merge", int(case.self_merge if self_merge is None else self_merge))
    backend.set_option("fa_wo", int(case.wo))


def _reset(backend):
    backend.set_option("fa_splits", 0)
    backend.set_option("fa_self_merge", 0)
    backend.set_option("fa_wo", 0)


def _run(backend, H, case, p, want_form, bad):
    got = FR.run_probe(case, p, backend, H)
    ran = backend.stat("fa_form")
    if ran != want_form:
        bad.append(f"{case.id} {p.name}: expected form [{FR.form_name(want_form)}], ran [{FR.form_name(ran)}]")
    return got


@pytest.mark.parametrize("case", FR.CASES, ids=lambda c: c.id)
def test_fa_cells(backend, H, plog, case):
    t0 = time.time()
    bad, worst = [], {}

    def gate(p, got):
        try:
            w = FR.check_probe(case, p, got, quant_step=case.wo)
            kind = p.name.split("_")[0]
            worst[kind] = max(worst.get(kind, 0.0), w)
        except AssertionError as e:
            bad.append(str(e))

    _options(backend, case)
    try:
        for p in FR.indicator_probes(case):
            gate(p, _run(backend, H, case, p, case.form, bad))
        pairs = []
        for pair in (False, True):
            if pair and case.n_splits == 1 and case.trip >= case.nkv:
                continue  # (one trip, one split: nothing to merge)
            for p in FR.witness_probes(case, pair):
                got = _run(backend, H, case, p, case.form, bad)
                gate(p, got)
                if pair:
                    pairs.append((p, got))
        p = FR.random_probe(case)
        got = _run(backend, H, case, p, case.form, bad)
        if case.wo:
            # through the Q8_K activation of the read-out mat-vec: half a quantisation step, plus 1e-4 of the block maximum for the f32 arithmetic in front of it
            amax = np.abs(p.expect.reshape(-1, 256)).max(axis=1)
            over = (np.abs(got.astype(np.float64) - p.expect).reshape(-1, 256) - (amax / 254)[:, None]) / amax[:, None]
            worst["random"] = float(over.max())
            if not over.max() <= 1e-4:
                bad.append(f"{case.id} random: {over.max():.3e} of the block maximum beyond half a quantisation step")
        elif case.kv != L.F16 and case.kernel == "DEC":
            # the lane kernels over a quantised cache ask with ggml-cpu's 8-bit query: the oracle is the reference, at test_flash_attn_q8_0_kv's gate
            ref = FR.run_probe(case, p, "oracle", H, T.host_threads(8))
            worst["random"] = T.nmse(got, ref)
            if not worst["random"] <= 1e-6:
                bad.append(f"{case.id} random: nmse {worst['random']:.3e} against the oracle > 1e-6")
        else:
            lim = 3e-7 if case.kernel == "MMA" else 1e-9  # (the matrix-core kernel rounds P to f16 once per element: test_flash_attn's gates)
            worst["random"] = T.nmse(got, p.expect)
            if not worst["random"] <= lim:
                bad.append(f"{case.id} random: nmse {worst['random']:.3e} against the float64 twin > {lim}")
        if case.self_merge:  # the same records merged by a combine launch: bit-equal on the pair probe (weights of exactly one half)
            two = dataclasses.replace(case, self_merge=False, tail="COMBINE")
            _options(backend, two)
            for p, one in pairs:
                got = _run(backend, H, two, p, two.form, bad)
                if not np.array_equal(got, one):
                    bad.append(f"{case.id} {p.name}: self-merged result differs from the combine launch's in {np.count_nonzero(got != one)} values")
    finally:
        _reset(backend)
    plog(f"fa_cells {case.id} [{FR.form_name(case.form)}]: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" ({time.time() - t0:.1f} s)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


def test_fa_list_token_that_sees_nothing(backend, H, plog):
    """List mode, one split: a token whose mask row is all -inf has an empty list and no combine pass to say so — the kernel writes the CPU's NaN row itself."""
    case = next(c for c in FR.CASES if c.id == "list_d128_g3_one")
    p = next(x for x in FR.indicator_probes(case) if x.name == "indicator_A_blockdiag")
    mask = p.mask.copy()
    mask[2] = -np.inf
    p = dataclasses.replace(p, mask=mask)
    ref = FR.run_probe(case, p, "oracle", H)
    _options(backend, case)
    try:
        got = FR.run_probe(case, p, backend, H)
        assert backend.stat("fa_form") == case.form, FR.form_name(backend.stat("fa_form"))
    finally:
        _reset(backend)
    assert np.isnan(ref[2]).all() and np.isnan(got[2]).all()
    rows = [0, 1, 3, 4]
    dev = np.abs(got[rows].astype(np.float64) - p.expect[rows]) * p.den[rows][:, :, None]
    assert dev.max() <= FR.INDICATOR_GATE and not np.isnan(got[rows]).any()
