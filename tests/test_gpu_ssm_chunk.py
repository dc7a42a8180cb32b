"""GPU: csrc/ssm_chunk.hip — SSM_SCAN's chunked matrix-core form (Mamba-2 prompts) through the C-ABI against ssm_ref.scan64, the float64 twin, at the smallest
shapes that reach a partial-only chunk (5 tokens), an exact chunk (64), a chunk plus one token (65), two chunks plus a tail (130), a head_dim tail (48) and both
group mappings.  On a backend without the form set_option("ssm_chunk", ..) is refused and every test here fails.

The gate: y and the final states finite and within G u Ey / G u Es of the twin, Ey / Es the twin's absolute-value envelopes, u = 2^-24, with
    G = 5 c_S + D + Q + 13 = 6325,    c_S = K + Q + 12 = 1224,    K = 11 * 104 + 4 = 1148,    Q = 64 tokens a chunk,    D = 128 state elements.
In units of u, relative to a term's own share of the envelope (expf and log1pf taken as two ulps = 4 u each, as ssm_ref's P = (4, 4)):
  * dtp 8; a = dtp A and x dtp 9 each.  The prefix sums are two-float: their own error is second order.  A decay's argument (hi_t - hi_s) + (lo_t - lo_s) adds two
    roundings: 11 |arg|, which expf turns into the decay's relative error 11 |arg| + 4.  A decay is 0 in f32 once its argument is below -104, so K bounds every decay
    that is not 0.  (The serial kernel multiplies per-token decays: 9 |arg| + 6 a token, below K + 6 n_t as well.)
  * the state after a chunk: the old part K + 1, a new term K + 9 + 2, the Q + 1 partial sums of the accumulation one each: at most c_S more than before the chunk.
  * y in the chunk behind c_S-steps of state: the state's error, then K + (D + 1) + 1 for exp(cum_t) (S0 C_t); the terms inside the chunk (D + 1) for C_t . B_s,
    K + 1 for the decay and its product, 9 + 1 for x dtp and its product, Q partial sums: K + D + Q + 13 on top of the state's.
  * the longest run here is three chunks and two serial steps (each within c_S): five steps.
The bound is a worst case and is carried by the 11 * 104 of a decay at the edge of underflow; on the CPU a NumPy f32 restatement of the chunked order (sequential f32
sums along each product's K) stays at 0.0007 of the gate for y and 0.0015 for the states at worst over every case below — where ssm_ref.scan32, the serial order's
f32 twin, stands too (0.0007 / 0.0016).  G was fixed before any GPU run.
"""
import functools
import itertools

import numpy as np
import pytest

import harness as T
import ssm_ref as S
import test_gpu_ssm as TS

pytestmark = pytest.mark.gpu
G_GATE = 6325.0
MIN_TOKENS = 128  # kernels.h MI_SSM_CHUNK_MIN_TOKENS
N_HEAD = 3
CASES = [c + (False,) for c in itertools.product((128, 64), (64, 48), (1, 3), (5, 64, 65, 130), (1, 3))] + [(128, 64, 1, 130, 3, True)]


@functools.lru_cache(maxsize=None)
def _inputs(d_state, head_dim, n_group, n_t, n_s):
    """Drawn as ssm_ref.scan_inputs draws them; with three sequences the ids are permuted and two sequences start from one state row."""
    rng = np.random.default_rng(d_state * 1009 + head_dim * 101 + n_group * 31 + n_t * 7 + n_s)
    f = np.float32
    inp = {
        "s": rng.standard_normal((n_s + 2, N_HEAD, head_dim, d_state)).astype(f),
        "x": rng.standard_normal((n_s, n_t, N_HEAD, head_dim)).astype(f),
        "B": rng.standard_normal((n_s, n_t, n_group, d_state)).astype(f),
        "C": rng.standard_normal((n_s, n_t, n_group, d_state)).astype(f),
        "ids": np.array({1: [2], 3: [4, 2, 4]}[n_s], dtype=np.int32),
        "A": (-rng.uniform(0.05, 1.5, (N_HEAD, 1))).astype(f),
    }
    dt = rng.uniform(-3.0, 3.0, (n_s, n_t, N_HEAD)).astype(f)
    flat = dt.reshape(-1)
    for k, v in enumerate(S.DT_SPECIAL):
        flat[(k * flat.size) // len(S.DT_SPECIAL) + flat.size // (2 * len(S.DT_SPECIAL))] = v
    inp["dt"] = dt
    return inp, S.scan64(inp)


def _scan(backend, inp, mode, xbc=False, timing=False):
    """(y, states[, timing classes]) of the node under ssm_chunk = mode."""
    def build(g):
        r = TS._scan_node(g, inp, xbc=xbc)
        return [r], [r]

    try:
        backend.set_option("ssm_chunk", mode)
        if timing:
            backend.set_option("timing", 1)
            backend.timing_report()
        out = TS._split_scan(TS._run(backend, build)[0], inp)
        return out + (backend.timing_report(),) if timing else out
    finally:
        backend.set_option("timing", 0)
        backend.set_option("ssm_chunk", 1)


def _excess(ref, y, st):
    """Worst |got - twin| over the gate, for y and for the states (inf for a value that is not finite)."""
    return S.scan_excess(ref, (G_GATE * S.U * ref["Ey"], G_GATE * S.U * ref["Es"]), y, st)


@pytest.mark.parametrize("d_state,head_dim,n_group,n_t,n_s,xbc", CASES)
def test_chunked_and_serial_within_the_gate(backend, plog, d_state, head_dim, n_group, n_t, n_s, xbc):
    inp, ref = _inputs(d_state, head_dim, n_group, n_t, n_s)
    for mode in (2, 0):
        ey, es = _excess(ref, *_scan(backend, inp, mode, xbc=xbc))
        plog(f"  ssm_scan d{d_state} hd{head_dim} g{n_group} t{n_t} s{n_s} xbc={xbc} ssm_chunk={mode}: y {ey:.5f}, states {es:.5f} of G u E")
        assert ey <= 1.0 and es <= 1.0, (mode, ey, es)


@pytest.mark.parametrize("mode,n_t,chunked", [(2, 5, True), (0, MIN_TOKENS, False), (1, 65, False), (1, MIN_TOKENS, True)])
def test_the_form_that_ran(backend, mode, n_t, chunked):
    inp, _ = _inputs(128, 64, 1, n_t, 1)
    classes = _scan(backend, inp, mode, timing=True)[2]
    got = {k: classes.get(k, (0,))[0] for k in ("ssm_scan_chunk", "ssm_scan")}
    assert got == {"ssm_scan_chunk": int(chunked), "ssm_scan": int(not chunked)}, classes


def test_deterministic_and_the_state_carries_into_serial_steps(backend, plog):
    """Two chunked runs bit-equal; a 130-token prompt in the chunked form, then two one-token steps of the serial kernel on the states it wrote, against the twin
    over all 132 tokens."""
    inp, ref = _inputs(128, 48, 3, 132, 3)
    cut = lambda a, b, s, ids: dict(inp, x=inp["x"][:, a:b], dt=inp["dt"][:, a:b], B=inp["B"][:, a:b], C=inp["C"][:, a:b], s=s, ids=ids)
    prompt = cut(0, 130, inp["s"], inp["ids"])
    y, st = _scan(backend, prompt, 2)
    y2, st2 = _scan(backend, prompt, 2)
    assert np.array_equal(TS._bits(y), TS._bits(y2)) and np.array_equal(TS._bits(st), TS._bits(st2))
    ys = [y]
    for t in (130, 131):
        y1, st = _scan(backend, cut(t, t + 1, st.copy(), np.arange(3, dtype=np.int32)), 0)
        ys.append(y1)
    ey, es = _excess(ref, np.concatenate(ys, axis=1), st)
    plog(f"  ssm_scan 130 chunked tokens + 2 serial steps: y {ey:.5f}, states {es:.5f} of G u E")
    assert ey <= 1.0 and es <= 1.0, (ey, es)
