"""GPU: csrc/wkv_chunk.hip — the chunked matrix-core form of RWKV_WKV6 and GATED_LINEAR_ATTN through the C-ABI against rwkv_ref.twin64, under the gate the serial
kernel answers to (R.excess <= 1, unchanged), at the smallest shapes that reach a partial-only chunk (5 tokens), an exact one (Q), a chunk plus one token and three
chunks with a tail.  On a backend without the form set_option("wkv_chunk", ..) is refused and every test here fails.

Why factor 1 (counted for the kernel as written, before any GPU run; units of u relative to a term's own share of the envelope; Q = 16):
  * state, granted 2 a token step on everything carried: 2 Q on the old state, 2 (Q - s) on token s's term.  Spent: P0_Q is Q - 1 roundings (the first factor multiplies
    1) and its product with S0 one; K~[s] = k_s P_(Q,s) is Q - 1 - s (a running product that starts from k_s); each token is added by its OWN K = 1 MFMA step, in ascending
    order, onto the decayed old state: one product and one sum a step (one rounding if the unit fuses them), the partial sum after token s no larger than the envelope
    of the terms so far.  Old state Q + Q, token s (Q - 1 - s) + 1 + (Q - s): within the grant whatever order a K = 4 step would sum its four products in — none is used here.
  * y, granted 4 + N (GLA 2 + N), N = 2 S, beside what the state carries (2 t on the old state, 2 (t - s) on token s at WKV6's y_t; one step more for GLA).  Products:
    WKV6 old state t + 1, token s < t: t - s + 1, bonus 3; GLA (qs's own rounding included) t + 3 and t - s + 3.  Partial sums: the Y accumulator takes S / 4 + 4 K = 4
    steps, at most 4 additions each in any order: S + 16; an element of A at most S / 4 + 2 (lane-local run, two DPP adds, three cross-wave adds): 1.25 S + 18 <= 2 S.
"""
import functools

import numpy as np
import pytest

import rwkv_ref as R
import test_gpu_rwkv as TR

pytestmark = pytest.mark.gpu
Q = 16            # wkv_chunk.hip: WQ
MIN_TOKENS = 128  # kernels.h: MI_WKV_CHUNK_MIN_TOKENS
CLASS = {"wkv6": "rwkv_wkv6", "gla": "gated_linear_attn"}
OPS = ("wkv6", "gla")


@functools.lru_cache(maxsize=None)
def _case(op, S, H, n_seqs, n_t, kind="rand"):
    inp = R.inputs(op, S, H, n_seqs, n_t, kind)
    return inp, R.twin64(op, inp)


def _wkv(backend, op, inps, mode, timing=False):
    """[(y, states)] of the nodes under wkv_chunk = mode [, the timing classes]."""
    try:
        backend.set_option("wkv_chunk", mode)
        if timing:
            backend.set_option("timing", 1)
            backend.timing_report()
        out = [R.split(flat, inp) for flat, inp in zip(TR._run(backend, lambda g: [TR._wkv_node(g, op, inp) for inp in inps]), inps)]
        return (out, backend.timing_report()) if timing else out
    finally:
        backend.set_option("timing", 0)
        backend.set_option("wkv_chunk", 1)


@pytest.mark.parametrize("n_t", [5, Q, Q + 1, 3 * Q + 1])
@pytest.mark.parametrize("H,n_seqs", [(1, 1), (3, 3)])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("op", OPS)
def test_chunked_and_serial_within_the_gate(backend, plog, op, S, H, n_seqs, n_t):
    inp, ref = _case(op, S, H, n_seqs, n_t)
    for mode in (2, 0):
        ey, es = R.excess(ref, *_wkv(backend, op, [inp], mode)[0])
        plog(f"  {op} S {S} H {H} seqs {n_seqs} n_t {n_t} wkv_chunk={mode}: y {ey:.3f}, states {es:.3f} of the gate")
        assert ey <= 1.0 and es <= 1.0, (mode, ey, es)


@pytest.mark.parametrize("kind", ["indicator", "zero_decay", "unit_decay"])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("op", OPS)
def test_special_inputs_chunked(backend, op, S, kind):
    inp, ref = _case(op, S, 3, 3, 2 * Q + 1, kind)
    y, st = _wkv(backend, op, [inp], 2)[0]
    ey, es = R.excess(ref, y, st)
    assert ey <= 1.0 and es <= 1.0, (ey, es)
    if kind == "zero_decay":  # nothing became inf or NaN, and what is left is the last token's outer product, exactly
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(st))
        assert np.array_equal(TR._bits(st[-1]), TR._bits(inp["k"][-1][:, :, None] * inp["v"][-1][:, None, :]))
    if kind == "indicator":
        assert 0 < np.count_nonzero(st) <= st.shape[0] * st.shape[1] * (2 * Q + 1)  # at most one cell per token and head


@pytest.mark.parametrize("mode,n_t,chunked", [(2, 5, True), (0, MIN_TOKENS, False), (1, MIN_TOKENS - 1, False), (1, MIN_TOKENS, True)])
@pytest.mark.parametrize("op", OPS)
def test_the_form_that_ran(backend, op, mode, n_t, chunked):
    classes = _wkv(backend, op, [R.inputs(op, 64, 1, 1, n_t)], mode, timing=True)[1]
    got = {k: classes.get(k, (0,))[0] for k in (CLASS[op] + "_chunk", CLASS[op])}
    assert got == {CLASS[op] + "_chunk": int(chunked), CLASS[op]: int(not chunked)}, classes


@pytest.mark.parametrize("op", OPS)
def test_deterministic_independent_and_the_state_carries(backend, plog, op):
    """Two chunked runs bit-equal, each sequence alone the same bits; a 3 Q + 1 token prompt in the chunked form, then two one-token steps of the serial kernel on the
    states it wrote, against the twin over all 3 Q + 3 tokens."""
    n_t = 3 * Q + 1
    inp, ref = _case(op, 64, 3, 3, n_t + 2)
    per_tok = [n for n in inp if n not in ("state", "tf", "scale")]

    def cut(a, b, state):
        return dict(inp, state=state, **{n: np.concatenate([inp[n][s * (n_t + 2) + a:s * (n_t + 2) + b] for s in range(3)]) for n in per_tok})

    prompt = cut(0, n_t, inp["state"])
    alone = [R.one_sequence(op, prompt, s) for s in range(3)]
    got = _wkv(backend, op, [prompt, prompt] + alone, 2)
    (y, st), (y2, st2) = got[0], got[1]
    assert np.array_equal(TR._bits(y), TR._bits(y2)) and np.array_equal(TR._bits(st), TR._bits(st2))
    for s in range(3):
        y1, st1 = got[2 + s]
        assert np.array_equal(TR._bits(y1), TR._bits(y[s * n_t:(s + 1) * n_t])) and np.array_equal(TR._bits(st1[0]), TR._bits(st[s])), s
    ys = [y.reshape(3, n_t, 3, 64)]
    for t in (n_t, n_t + 1):
        y1, st = _wkv(backend, op, [cut(t, t + 1, st.copy())], 0)[0]
        ys.append(y1.reshape(3, 1, 3, 64))
    ey, es = R.excess(ref, np.concatenate(ys, axis=1), st)
    plog(f"  {op}: {n_t} chunked tokens + 2 serial steps: y {ey:.3f}, states {es:.3f} of the gate")
    assert ey <= 1.0 and es <= 1.0, (ey, es)
