"""GPU: csrc/wkv7_chunk.hip — the chunked matrix-core form of RWKV_WKV7 through the C-ABI against rwkv_ref.twin64, under the gate the serial kernel answers to
(R.excess <= 1, unchanged), at the smallest shapes that reach a partial-only chunk (5 tokens), an exact one (Q), a chunk plus one token and three chunks with a
tail.  On a backend without the form the timing class rwkv_wkv7_chunk does not exist and wkv_chunk = 2 runs the serial kernel: test_the_form_that_ran fails.

Why factor 1 (DESIGN.md 4k holds the table; counted for the kernel as written, before any GPU run; units of u relative to a term's own share of the envelope; Q = 16):
  * state, granted 3 a token step on everything carried, 3 on v k and e_sa |b| + 2 Esa |b| on sa b at entry.  Spent: P0_Q is Q - 1 roundings (the first factor
    multiplies 1) and its product with S0 one; K~[s] and B~[s] are Q - 1 - s each (running products that start from k_s, b_s); every outer product is added by its OWN
    K = 1 MFMA step, token ascending, v k before sa b: one product and one sum a step.  Old state Q + 2 Q = 3 Q; v k of token s (Q - 1 - s) + 1 + 2 (Q - s) = 3 (Q - s);
    sa b of token s (Q - 1 - s) + 1 + 2 (Q - s) - 1 = 2 + 3 (Q - 1 - s) beside sa_s's own error: the grant, to the unit.
  * sa_t, granted e carried (3 t on the old state, 3 (t - s) on v k and 2 + 3 (t - 1 - s) on sa b of token s < t) and 1 + N on Esa, N = 2 S.  Products: old state t
    (a~) + 1 <= 3 t + 1; v k term (t - 1 - s) + 1 (a . kp) + 1 (A v) = t - s + 1 <= 3 (t - s) + 1; sa b term t - s + 1 <= 3 (t - s).  Partial sums: the G accumulator
    takes S / 4 + 4 K = 4 steps of at most 4 additions, the substitution at most 15 more, an element of A at most S / 16 + 3: 1.0625 S + 34 <= 2 S.
  * y_t, granted e_t carried and 1 + N on Ey.  Products: old state t + 2 <= 3 (t + 1) + 1; v k of s <= t: t - s + 2 <= 3 (t - s) + 4; sa b: t - s + 2 <= 3 (t - s) + 3.
    Partial sums: S / 4 + 8 K = 4 steps and an element of A: 1.0625 S + 35 <= 2 S.
"""
import functools

import numpy as np
import pytest

import rwkv_ref as R
import test_gpu_rwkv as TR

pytestmark = pytest.mark.gpu
Q = 16            # wkv7_chunk.hip: W7Q
MIN_TOKENS = 128  # kernels.h: MI_WKV7_CHUNK_MIN_TOKENS
OP = "wkv7"


@functools.lru_cache(maxsize=None)
def _case(S, H, n_seqs, n_t, kind="rand"):
    inp = R.inputs(OP, S, H, n_seqs, n_t, kind)
    return inp, R.twin64(OP, inp)


def _wkv(backend, inps, mode, timing=False):
    """[(y, states)] of the nodes under wkv_chunk = mode [, the timing classes]."""
    try:
        backend.set_option("wkv_chunk", mode)
        if timing:
            backend.set_option("timing", 1)
            backend.timing_report()
        out = [R.split(flat, inp) for flat, inp in zip(TR._run(backend, lambda g: [TR._wkv_node(g, OP, inp) for inp in inps]), inps)]
        return (out, backend.timing_report()) if timing else out
    finally:
        backend.set_option("timing", 0)
        backend.set_option("wkv_chunk", 1)


@pytest.mark.parametrize("n_t", [5, Q, Q + 1, 3 * Q + 1])
@pytest.mark.parametrize("H,n_seqs", [(1, 1), (3, 3)])
@pytest.mark.parametrize("S", [64, 128])
def test_chunked_and_serial_within_the_gate(backend, plog, S, H, n_seqs, n_t):
    inp, ref = _case(S, H, n_seqs, n_t)
    for mode in (2, 0):
        ey, es = R.excess(ref, *_wkv(backend, [inp], mode)[0])
        plog(f"  wkv7 S {S} H {H} seqs {n_seqs} n_t {n_t} wkv_chunk={mode}: y {ey:.3f}, states {es:.3f} of the gate")
        assert ey <= 1.0 and es <= 1.0, (mode, ey, es)


@pytest.mark.parametrize("kind", ["indicator", "zero_decay", "unit_decay"])
@pytest.mark.parametrize("S", [64, 128])
def test_special_inputs_chunked(backend, plog, S, kind):
    inp, ref = _case(S, 3, 3, 2 * Q + 1, kind)
    y, st = _wkv(backend, [inp], 2)[0]
    ey, es = R.excess(ref, y, st)
    plog(f"  wkv7 S {S} {kind}: y {ey:.3f}, states {es:.3f} of the gate")
    assert ey <= 1.0 and es <= 1.0, (ey, es)
    if kind == "zero_decay":  # nothing became inf or NaN (sa b stays in the state: no equality with the last outer product here)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(st))
    if kind == "indicator":
        assert 0 < np.count_nonzero(st) <= st.shape[0] * st.shape[1] * (2 * Q + 1)  # at most one cell per token and head


@pytest.mark.parametrize("mode,n_t,chunked", [(2, 5, True), (0, MIN_TOKENS, False), (1, MIN_TOKENS - 1, False), (1, MIN_TOKENS, True)])
def test_the_form_that_ran(backend, mode, n_t, chunked):
    classes = _wkv(backend, [R.inputs(OP, 64, 1, 1, n_t)], mode, timing=True)[1]
    got = {k: classes.get(k, (0,))[0] for k in ("rwkv_wkv7_chunk", "rwkv_wkv7")}
    assert got == {"rwkv_wkv7_chunk": int(chunked), "rwkv_wkv7": int(not chunked)}, classes


def test_deterministic_independent_and_the_state_carries(backend, plog):
    """Two chunked runs bit-equal, each sequence alone the same bits; a 3 Q + 1 token prompt in the chunked form, then two one-token steps of the serial kernel on the
    states it wrote, against the twin over all 3 Q + 3 tokens."""
    n_t = 3 * Q + 1
    inp, ref = _case(64, 3, 3, n_t + 2)
    per_tok = [n for n in inp if n != "state"]

    def cut(a, b, state):
        return dict(inp, state=state, **{n: np.concatenate([inp[n][s * (n_t + 2) + a:s * (n_t + 2) + b] for s in range(3)]) for n in per_tok})

    prompt = cut(0, n_t, inp["state"])
    alone = [R.one_sequence(OP, prompt, s) for s in range(3)]
    got = _wkv(backend, [prompt, prompt] + alone, 2)
    (y, st), (y2, st2) = got[0], got[1]
    assert np.array_equal(TR._bits(y), TR._bits(y2)) and np.array_equal(TR._bits(st), TR._bits(st2))
    for s in range(3):
        y1, st1 = got[2 + s]
        assert np.array_equal(TR._bits(y1), TR._bits(y[s * n_t:(s + 1) * n_t])) and np.array_equal(TR._bits(st1[0]), TR._bits(st[s])), s
    ys = [y.reshape(3, n_t, 3, 64)]
    for t in (n_t, n_t + 1):
        y1, st = _wkv(backend, [cut(t, t + 1, st.copy())], 0)[0]
        ys.append(y1.reshape(3, 1, 3, 64))
    ey, es = R.excess(ref, np.concatenate(ys, axis=1), st)
    plog(f"  wkv7: {n_t} chunked tokens + 2 serial steps: y {ey:.3f}, states {es:.3f} of the gate")
    assert ey <= 1.0 and es <= 1.0, (ey, es)
