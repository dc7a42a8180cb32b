"""CPU: the read-out weights and the edge-activation catalogue of tests/probes.py, checked before any GPU test relies on them.

  * the one-hot blocks de-quantise to the identity (the bsums blocks to -1 on their sub-block) through the C oracle;
  * the oracle's mat-mul over the read-out weights equals the NumPy twins' d_act * q_act bit for bit on every edge row;
  * the catalogue has teeth: each way a device quantiser could be subtly wrong (a mutant of the NumPy twin) changes at least one
    expected output on it.  Two of the mutants one might list cannot be seen through ANY mat-mul, and the test proves that instead:
      - "last index instead of first on a tie for max|x|": the tied elements differ in sign only, so iscale, every quant and d all flip
        sign together (rint is symmetric) and d * q, d * bsums are unchanged bit for bit.  The mutant does change the Q8_K block (asserted).
      - "clamp removed": with iscale = -127 / max no product iscale * x exceeds 127 by more than an ulp, so min(127, .) never acts.
"""
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import probes as P
from probes import MG

TYPES = [("q8_0", L.Q8_0), ("q4_K", L.Q4_K), ("q5_K", L.Q5_K), ("q6_K", L.Q6_K)]
K = 512


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _dequant(qt, raw, n):
    y = np.empty(n, np.float32)
    raw = np.ascontiguousarray(raw)
    T.oracle().oracle_dequantize_row(qt, _ptr(raw), _ptr(y), n)
    return y


@pytest.mark.parametrize("name,qt", TYPES)
def test_readout_weight_dequantises_to_identity(built, name, qt):
    w = P.readout_weight(qt, K)
    y = _dequant(qt, w, K * K).reshape(K, K)
    assert np.array_equal(y, np.eye(K, dtype=np.float32)), name
    assert np.array_equal(MG.dequant(qt, w.reshape(-1, L.TYPE_SIZE[qt])).reshape(K, K), np.eye(K, dtype=np.float32)), name + " (NumPy twin)"


@pytest.mark.parametrize("name,qt", TYPES[1:3])
def test_bsums_readout_weight_dequantises_to_minus_one_on_its_sub_block(built, name, qt):
    w = P.bsums_readout_weight(qt, K)
    y = _dequant(qt, w, (K // 32) * K).reshape(K // 32, K)
    ref = np.zeros((K // 32, K), np.float32)
    for r in range(K // 32):
        ref[r, 32 * r:32 * r + 32] = -1.0
    assert np.array_equal(y, ref), name


@pytest.mark.parametrize("name,qt", TYPES)
def test_oracle_quantisers_equal_the_numpy_twins_on_the_catalogue(built, name, qt):
    kind = P.act_kind(qt)
    x, names = P.edge_activations(kind, K, np.random.default_rng(7))
    d, q, bs = P.quantize(kind, x)
    o = T.oracle()
    for i, row in enumerate(x):
        row = np.ascontiguousarray(row)
        if kind == "q8_K":
            raw = np.zeros((K // 256, 292), np.uint8)
            o.oracle_quantize_row_q8_K(_ptr(row), _ptr(raw), K)
            od = raw[:, 0:4].copy().view(np.float32).reshape(-1)
            oq = raw[:, 4:260].copy().view(np.int8).astype(np.int32)
            obs = raw[:, 260:292].copy().view(np.int16).astype(np.int32)
            live = od != 0  # (d = 0: the quants are multiplied by zero; the reference leaves what a float -> int conversion of inf gives)
            assert np.array_equal(P.bits(od), P.bits(d[i])), names[i]
            assert np.array_equal(oq[live], q[i][live]) and np.array_equal(obs[live], bs[i][live]), names[i]
        else:
            raw = np.zeros((K // 32, 34), np.uint8)
            o.oracle_quantize_row_q8_0(_ptr(row), _ptr(raw), K)
            od = raw[:, 0:2].copy().view(np.float16).astype(np.float32).reshape(-1)
            oq = raw[:, 2:34].copy().view(np.int8).astype(np.int32)
            live = od != 0
            assert np.array_equal(P.bits(od), P.bits(d[i])), names[i]
            assert np.array_equal(oq[live], q[i][live]), names[i]


def _oracle_mul_mat(qt, w, n_out, x):
    H = L.host()

    def build(g):
        return H.ggml_mul_mat(g.ctx, g.new(qt, [x.shape[1], n_out], w), g.new(L.F32, [x.shape[1], x.shape[0]], x))

    return T.run_case(build, "oracle")[0].reshape(x.shape[0], n_out)


@pytest.mark.parametrize("name,qt", TYPES)
def test_oracle_vec_dot_over_readout_rows_is_the_quantiser(built, name, qt):
    kind = P.act_kind(qt)
    x, names = P.edge_activations(kind, K, np.random.default_rng(11))
    got = _oracle_mul_mat(qt, P.readout_weight(qt, K), K, x)
    ref = P.expected_readout(kind, x)
    bad = P.bits(got) != P.bits(ref)
    assert not bad.any(), f"{name}: rows {[names[i] for i in np.nonzero(bad.any(axis=1))[0]]}"
    # and the block dot called directly, one edge row against a few read-out rows
    o = T.oracle()
    w = P.readout_weight(qt, K)
    fn = getattr(o, f"oracle_vec_dot_{name}_{kind}")
    for i in range(0, len(x), 5):
        row = np.ascontiguousarray(x[i])
        act = np.zeros(K // 256 * 292 if kind == "q8_K" else K // 32 * 34, np.uint8)
        (o.oracle_quantize_row_q8_K if kind == "q8_K" else o.oracle_quantize_row_q8_0)(_ptr(row), _ptr(act), K)
        for j in (0, 1, 31, 32, 255, 256, 300, K - 1):
            wr = np.ascontiguousarray(w[j])
            v = np.float32(fn(K, _ptr(wr), _ptr(act)))
            assert P.bits(v) == P.bits(ref[i, j]), (name, names[i], j)


@pytest.mark.parametrize("name,qt", TYPES[1:3])
def test_oracle_vec_dot_over_bsums_rows_is_the_bsums_field(built, name, qt):
    x, names = P.edge_activations("q8_K", K, np.random.default_rng(13))
    got = _oracle_mul_mat(qt, P.bsums_readout_weight(qt, K), K // 32, x)
    ref = P.expected_bsums_readout(x)
    bad = P.bits(got) != P.bits(ref)
    assert not bad.any(), f"{name}: rows {[names[i] for i in np.nonzero(bad.any(axis=1))[0]]}"
    i = [n.split("@")[0] for n in names].index("const_neg")
    at = int(names[i].split("@")[1])
    d, q, bs = P.quantize("q8_K", x)
    assert (q[i, at] == -127).all() and (bs[i, at] == -2032).all()  # the extreme the f16 / int16 bsums fields must hold


# ------------------------------------------------------------------------------------------------ mutants of the NumPy twins
def _q8K_mutant(rounding="even", tie="first", num=-127.0, clamp=True, bsums_slip=False):
    def quantize_q8_K(x):
        x = x.astype(np.float32)
        ax = np.abs(x)
        idx = np.argmax(ax, axis=1) if tie == "first" else x.shape[1] - 1 - np.argmax(ax[:, ::-1], axis=1)
        mx = x[np.arange(x.shape[0]), idx]
        d = np.zeros(x.shape[0], np.float32)
        qs = np.zeros(x.shape, np.int8)
        nz = mx != 0
        iscale = np.zeros_like(mx)
        iscale[nz] = (np.float32(num) / mx[nz]).astype(np.float32)
        t = (iscale[:, None] * x).astype(np.float32)
        r = np.rint(t) if rounding == "even" else np.where(t >= 0, np.floor(t + np.float32(0.5)), np.ceil(t - np.float32(0.5)))
        v = r.astype(np.int32)
        if clamp:
            v = np.minimum(127, v)
        qs[nz] = v[nz].astype(np.int8)
        d[nz] = (np.float32(1.0) / iscale[nz]).astype(np.float32)
        src = qs.astype(np.int32)
        bsums = src.reshape(-1, 16, 16).sum(axis=2)
        if bsums_slip:  # entry 5 of every block summed over values 72 .. 87 instead of 80 .. 95
            bsums[:, 5] = src[:, 72:88].sum(axis=1)
        return d, qs, bsums.astype(np.int16)

    return quantize_q8_K


def _q80_mutant(rounding="away", d_f16=True, divide=False):
    def quantize_q8_0(x):
        x = x.astype(np.float32)
        amax = np.max(np.abs(x), axis=1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        if divide:  # q = round(x / d_f16) instead of x * (1 / d)
            dh = d.astype(np.float16).astype(np.float32)
            t = np.where(dh[:, None] != 0, x / np.where(dh != 0, dh, 1)[:, None], 0).astype(np.float32)
        else:
            inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, 1), 0).astype(np.float32)
            t = (x * inv[:, None]).astype(np.float32)
        r = np.rint(t) if rounding == "even" else np.where(t >= 0, np.floor(t + np.float32(0.5)), np.ceil(t - np.float32(0.5)))
        return (d.astype(np.float16) if d_f16 else d), r.astype(np.int32).astype(np.int8)

    return quantize_q8_0


def test_mutant_builders_restate_the_twins(built):
    """With no mutation switched on the builders above ARE the twins (so a mutant differs from the reference by its one change only)."""
    for kind, twin in (("q8_K", {"q8K": _q8K_mutant()}), ("q8_0", {"q80": _q80_mutant()})):
        x, _ = P.edge_activations(kind, K, np.random.default_rng(3))
        assert np.array_equal(P.bits(P.expected_readout(kind, x)), P.bits(P.expected_readout(kind, x, **twin)))
    x, _ = P.edge_activations("q8_K", K, np.random.default_rng(3))
    assert np.array_equal(P.bits(P.expected_bsums_readout(x)), P.bits(P.expected_bsums_readout(x, q8K=_q8K_mutant())))


MUTANTS = [
    ("q8_K", "half away from zero instead of half to even", {"q8K": _q8K_mutant(rounding="away")}, "halfway"),
    ("q8_K", "iscale = -128 / max", {"q8K": _q8K_mutant(num=-128.0)}, None),
    ("q8_K", "one bsums entry summed over the wrong 16 values", {"q8K": _q8K_mutant(bsums_slip=True)}, None),
    ("q8_0", "half to even instead of half away from zero", {"q80": _q80_mutant(rounding="even")}, "halfway"),
    ("q8_0", "d not rounded through f16", {"q80": _q80_mutant(d_f16=False)}, None),
    ("q8_0", "q = round(x / d_f16) instead of x * (1 / d)", {"q80": _q80_mutant(divide=True)}, None),
]


@pytest.mark.parametrize("kind,what,twin,row", MUTANTS, ids=[m[1].replace(" ", "_") for m in MUTANTS])
def test_catalogue_catches_mutant(built, kind, what, twin, row):
    x, names = P.edge_activations(kind, K, np.random.default_rng(17))
    diff = P.bits(P.expected_readout(kind, x)) != P.bits(P.expected_readout(kind, x, **twin))
    if kind == "q8_K":
        diff = np.concatenate([diff, P.bits(P.expected_bsums_readout(x)) != P.bits(P.expected_bsums_readout(x, **twin))], axis=1)
    hit = [names[i] for i in np.nonzero(diff.any(axis=1))[0]]
    assert hit, f"mutant '{what}' changes no expected output on the catalogue"
    if row:  # the row built for this property catches it, on many elements (about half of its ~250 / 31 exact ties)
        rows = [i for i, n in enumerate(names) if n.startswith(row)]
        B = 256 if kind == "q8_K" else 32
        for i in rows:
            at = int(names[i].split("@")[1])
            n = int(diff[i, at * B:(at + 1) * B].sum())
            assert n >= B // 4, (what, names[i], n)


def test_tie_order_and_clamp_cannot_be_seen_through_a_mat_mul(built):
    """See the module docstring: both mutants leave d * q and d * bsums unchanged; the tie mutant does change the block."""
    x, names = P.edge_activations("q8_K", K, np.random.default_rng(17))
    ref, refb = P.bits(P.expected_readout("q8_K", x)), P.bits(P.expected_bsums_readout(x))
    for twin in ({"q8K": _q8K_mutant(tie="last")}, {"q8K": _q8K_mutant(clamp=False)}):
        assert np.array_equal(ref, P.bits(P.expected_readout("q8_K", x, **twin)))
        assert np.array_equal(refb, P.bits(P.expected_bsums_readout(x, **twin)))
    d0, q0, _ = P.quantize("q8_K", x)
    d1, q1, _ = P.quantize("q8_K", x, q8K=_q8K_mutant(tie="last"))
    for i, n in enumerate(names):
        if n.startswith("tie_"):
            at = int(n.split("@")[1])
            assert d1[i, at] == -d0[i, at] and np.array_equal(q1[i, at], -q0[i, at]), n
            assert q0[i, at].max() == 127  # the tied partner of the maximum sits on +127, the value min(127, .) guards
