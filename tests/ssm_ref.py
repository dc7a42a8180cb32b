"""NumPy twins of the three ops a state-space layer adds — CONCAT, SSM_CONV, SSM_SCAN — with the gates the GPU tests hold csrc/ssm.hip to (the CPU oracle has
none of these ops), and the inputs those tests run on.  The operand contracts are DESIGN.md §4i's.

Arrays are in NumPy order, ggml's dimensions reversed:
    s  (n_rs, n_head, head_dim, d_state)     x (n_s, n_t, n_head, head_dim)     dt (n_s, n_t, n_head)     A (n_head, d_state | 1)
    B, C (n_s, n_t, n_group, d_state)        ids (n_s,)                          sx (n_s, d_inner, d_conv - 1 + n_t)   c (d_inner, d_conv)

u = 2^-24 is the unit roundoff of f32: a correctly rounded operation is off by at most u relative, a function that is N ulps off by at most 2 N u.

SSM_CONV gate.  out = sum of d_conv products.  Each product rounds once (u), each of the d_conv additions rounds a partial sum whose magnitude is at most the sum
of the |products| (u each, the first addition to 0 is exact), a contraction into an fma only removes roundings:  |got - f64| <= (d_conv + 1) u sum |sx c|.

SSM_SCAN gate.  Per state element and token, with a = exp(dtp A), the f32 evaluation is
    dtp   = log1pf(expf(dt))           relative error  c_dtp = P_e + P_l   (d/dv log1p(v) v / log1p(v) <= 1: expf's error is not amplified); 0 above the threshold
    xdt   = x dtp                      c_dtp + 1
    arg   = dtp A                      c_dtp + 1, which exp() turns into the relative error |arg| (c_dtp + 1) of a, plus expf's own P_e
    state = prev a + B xdt             one rounding per product, one for the sum
where P_e and P_l are the errors of expf and log1pf in units of u.  To first order the error bound e_t (in units of u) of a state element obeys
    e_t = e_(t-1) a + [ |arg| (c_dtp + 1) + P_e + 1 ] |prev| a + [ c_dtp + 2 ] |B xdt| + E_t,        E_t = E_(t-1) a + |B xdt|,  E_0 = |s|,  e_0 = 0
E being the absolute-value envelope of the recurrence: the bound grows with the token index and forgets what a small `a` wipes out, as the error itself does.
y = sum over the state of state C adds a rounding per product and at most d_state roundings of partial sums no larger than E_y = sum E |C|, in any order:
    e_y = sum e |C| + (1 + d_state) E_y.
scan64() returns e for P = (0, 0): the roundings alone; for (2, 2): functions one ulp off; and for (4, 4).

The constants of the device's expf / log1pf are not assumed.  scan32() is the f32 twin in the contract's order with this process's libm; its worst error over
e(0, 0) on a case's inputs, R, is measured on the CPU (it carries the libm's true function error).  The gate allows the kernel that, plus what two further ulps of
expf and of log1pf can add (e(4, 4) - e(0, 0): the same propagation), plus — for y — a reduction in another order (d_state E_y), and nothing else:
    |got - f64| <= u [ R e(0,0) + e(4,4) - e(0,0) + (y only) d_state E_y ]
(The bounds e are first-order.  Where the a-priori bound e(2, 2) itself is checked — the host test of the f32 twin — it carries a factor 1 + 2^-10 for the
second-order terms and FLOOR (1 + d_state), FLOOR = 2^-120, for results that underflow, where a rounding is absolute instead of relative; the gate has neither.)
"""
import ctypes
import ctypes.util
import functools

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -120
SECOND_ORDER = 1.0 + 2.0 ** -10

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "log1pf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_expf_o = np.frompyfunc(lambda v: _libm.expf(float(v)), 1, 1)
_log1pf_o = np.frompyfunc(lambda v: _libm.log1pf(float(v)), 1, 1)


def expf(a):
    """This process's expf, element by element."""
    return _expf_o(np.asarray(a, dtype=np.float32)).astype(np.float32)


def log1pf(a):
    return _log1pf_o(np.asarray(a, dtype=np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CONCAT
def concat(a, b, dim):
    """ggml_concat along ggml dimension `dim` of two arrays of equal rank (NumPy order)."""
    return np.concatenate([a, b], axis=a.ndim - 1 - dim)


# ------------------------------------------------------------------------------------------------ SSM_CONV
def _windows(sx, d_conv):
    n_t = sx.shape[-1] - d_conv + 1
    return np.stack([sx[..., k:k + n_t] for k in range(d_conv)], axis=-1)  # (n_s, d_inner, n_t, d_conv)


def conv64(sx, c):
    """float64 result (n_s, n_t, d_inner) and the envelope sum |sx c|."""
    w = _windows(sx.astype(np.float64), c.shape[1])
    p = w * c.astype(np.float64)[None, :, None, :]
    return p.sum(-1).transpose(0, 2, 1), np.abs(p).sum(-1).transpose(0, 2, 1)


def conv32(sx, c):
    """f32, the contract's order: sum = 0, sum += sx c with i0 ascending, every product and sum rounded."""
    w = _windows(sx.astype(np.float32), c.shape[1])
    p = (w * c.astype(np.float32)[None, :, None, :]).astype(np.float32)
    return np.add.accumulate(p, axis=-1, dtype=np.float32)[..., -1].transpose(0, 2, 1)


def conv_gate(sx, c):
    return (c.shape[1] + 1) * U * conv64(sx, c)[1]


def silu64(v):
    """x / (1 + exp(-x)) in float64: the reference for ops.hip's silu_f (fused and unfused launches are compared bit for bit; this is for the float64 twins)."""
    v = np.asarray(v, dtype=np.float64)
    return v / (1.0 + np.exp(-v))


# ------------------------------------------------------------------------------------------------ SSM_SCAN
WRONG = ("softplus_threshold_dropped", "prev_not_carried", "ids_ignored", "states_stored_at_ids", "a_per_head", "b_c_swapped")
P_SETS = ((0, 0), (2, 2), (4, 4))


def _group_index(n_head, n_group):
    assert n_group in (1, n_head), "which heads share a group between the two is not pinned (DESIGN.md 4i)"
    return np.zeros(n_head, dtype=np.int64) if n_group == 1 else np.arange(n_head)


def scan64(inp, wrong=None):
    """float64 twin.  Returns a dict: y (n_s, n_t, n_head, head_dim), st (n_s, n_head, head_dim, d_state), their envelopes Ey / Es and, per P of P_SETS, the
    error bounds ey[P] / es[P] in units of u.  wrong: one of WRONG — a twin with that mistake (the sensitivity tests)."""
    s, x, dt, A, B, C, ids = (inp[k] for k in ("s", "x", "dt", "A", "B", "C", "ids"))
    n_rs, n_head, head_dim, d_state = s.shape
    n_s, n_t = x.shape[:2]
    if wrong == "b_c_swapped":
        B, C = C, B
    gi = _group_index(n_head, B.shape[2])
    s64, x64, A64 = s.astype(np.float64), x.astype(np.float64), A.astype(np.float64)
    if wrong == "a_per_head":
        A64 = np.repeat(A64[:, :1], A64.shape[1], axis=1)
    y = np.zeros((n_s, n_t, n_head, head_dim))
    st = np.zeros((n_s, n_head, head_dim, d_state))
    Ey = np.zeros_like(y)
    Es = np.zeros_like(st)
    ey = {P: np.zeros_like(y) for P in P_SETS}
    es = {P: np.zeros_like(st) for P in P_SETS}
    for i3 in range(n_s):
        row = i3 if wrong == "ids_ignored" else int(ids[i3])
        start = s64[row]
        state, E = start.copy(), np.abs(start)
        e = {P: np.zeros_like(state) for P in P_SETS}
        for i2 in range(n_t):
            d32 = dt[i3, i2].astype(np.float32)
            below = d32 <= np.float32(20.0)
            if wrong == "softplus_threshold_dropped":  # the f32 evaluation without the branch: expf overflows above 88.7
                with np.errstate(over="ignore"):
                    dtp = np.log1p(np.exp(d32)).astype(np.float64)
                below = np.ones_like(below)
            else:
                d64 = d32.astype(np.float64)
                dtp = np.where(below, np.log1p(np.exp(np.minimum(d64, 20.0))), d64)
            Bt, Ct = B[i3, i2].astype(np.float64)[gi], C[i3, i2].astype(np.float64)[gi]  # (n_head, d_state)
            xdt = x64[i3, i2] * dtp[:, None]  # (n_head, head_dim)
            with np.errstate(invalid="ignore", over="ignore"):
                arg = dtp[:, None] * A64  # (n_head, d_state | 1)
                a = np.exp(arg)[:, None, :]
                bx = Bt[:, None, :] * xdt[:, :, None]
                prev = start if (wrong == "prev_not_carried" and i2 > 0) else state
                for P in P_SETS:
                    c_dtp = np.where(below, P[0] + P[1], 0.0)[:, None]
                    k_prev = (np.abs(arg) * (c_dtp + 1.0) + P[0] + 1.0)[:, None, :]
                    e[P] = e[P] * a + k_prev * E * a + (c_dtp + 2.0)[:, :, None] * np.abs(bx) + (E * a + np.abs(bx))
                E = E * a + np.abs(bx)
                state = prev * a + bx
                y[i3, i2] = (state * Ct[:, None, :]).sum(-1)
            Ey[i3, i2] = (E * np.abs(Ct)[:, None, :]).sum(-1)
            for P in P_SETS:
                ey[P][i3, i2] = (e[P] * np.abs(Ct)[:, None, :]).sum(-1) + (1 + d_state) * Ey[i3, i2]
        if wrong == "states_stored_at_ids":
            if int(ids[i3]) < n_s:
                st[int(ids[i3])] = state
        else:
            st[i3] = state
        Es[i3] = E
        for P in P_SETS:
            es[P][i3] = e[P]
    return {"y": y, "st": st, "Ey": Ey, "Es": Es, "ey": ey, "es": es, "d_state": d_state}


def scan32(inp):
    """f32 twin in the contract's order, expf / log1pf from this process's libm: (y, st)."""
    s, x, dt, A, B, C, ids = (inp[k] for k in ("s", "x", "dt", "A", "B", "C", "ids"))
    n_rs, n_head, head_dim, d_state = s.shape
    n_s, n_t = x.shape[:2]
    gi = _group_index(n_head, B.shape[2])
    f = np.float32
    y = np.zeros((n_s, n_t, n_head, head_dim), dtype=f)
    st = np.zeros((n_s, n_head, head_dim, d_state), dtype=f)
    d = dt.astype(f)
    dtp_all = np.where(d <= f(20.0), log1pf(expf(np.minimum(d, f(20.0)))), d).astype(f)
    with np.errstate(under="ignore"):
        dA_all = expf((dtp_all[..., None] * A.astype(f)[None, None]).astype(f))  # (n_s, n_t, n_head, d_state | 1)
    for i3 in range(n_s):
        state = s[int(ids[i3])].astype(f).copy()
        for i2 in range(n_t):
            xdt = (x[i3, i2].astype(f) * dtp_all[i3, i2][:, None]).astype(f)
            Bt, Ct = B[i3, i2].astype(f)[gi], C[i3, i2].astype(f)[gi]
            with np.errstate(under="ignore"):
                state = ((state * dA_all[i3, i2][:, None, :]).astype(f) + (Bt[:, None, :] * xdt[:, :, None]).astype(f)).astype(f)
                p = (state * Ct[:, None, :]).astype(f)
            y[i3, i2] = np.add.accumulate(p, axis=-1, dtype=f)[..., -1]
        st[i3] = state
    return y, st


def twin_ratio(ref, y32, st32):
    """R: the f32 twin's worst error over the bound of the roundings alone, e(0, 0) u."""
    r = 0.0
    for got, want, e in ((y32, ref["y"], ref["ey"][(0, 0)]), (st32, ref["st"], ref["es"][(0, 0)])):
        err = np.abs(got.astype(np.float64) - want)
        m = e > 0
        if np.any(m):
            r = max(r, float(np.max(err[m] / (U * e[m]))))
        assert np.all(err[~m] == 0.0)
    return r


def scan_gates(ref, R):
    """(gate for y, gate for the final states): absolute bounds on |got - float64 twin| (module docstring)."""
    n = ref["d_state"]
    gy = U * (R * ref["ey"][(0, 0)] + (ref["ey"][(4, 4)] - ref["ey"][(0, 0)]) + n * ref["Ey"])
    gs = U * (R * ref["es"][(0, 0)] + (ref["es"][(4, 4)] - ref["es"][(0, 0)]))
    return gy, gs


def scan_excess(ref, gates, y, st):
    """Worst |got - f64| / gate over y and over the states (inf for a value that is not finite): <= 1 passes."""
    out = []
    for got, want, g in ((y, ref["y"], gates[0]), (st, ref["st"], gates[1])):
        got = np.asarray(got, dtype=np.float64).reshape(want.shape)
        with np.errstate(invalid="ignore"):
            ex = np.abs(got - want) / g
        out.append(float("inf") if not np.all(np.isfinite(got)) else float(np.max(ex)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the inputs of the scan tests
DT_SPECIAL = (20.0, float(np.nextafter(np.float32(20.0), np.float32(np.inf))), -30.0, 100.0, 19.5, 25.0)
# name: (d_state, head_dim, n_head, n_group, n_t, n_s, mamba1, duplicate start row, operands as views of one xBC buffer)
SCAN_CASES = {
    # Mamba-1 form: head_dim 1, A per state element; every n_head x n_t x n_s; two sequences start from one row in the h64-t7-s3 case
    "m1-h64-t1-s1": (16, 1, 64, 1, 1, 1, True, False, False),
    "m1-h64-t1-s3": (16, 1, 64, 1, 1, 3, True, False, False),
    "m1-h64-t2-s1": (16, 1, 64, 1, 2, 1, True, False, False),
    "m1-h64-t2-s3": (16, 1, 64, 1, 2, 3, True, False, False),
    "m1-h64-t7-s1": (16, 1, 64, 1, 7, 1, True, False, False),
    "m1-h64-t7-s3": (16, 1, 64, 1, 7, 3, True, True, False),
    "m1-h64-t65-s1": (16, 1, 64, 1, 65, 1, True, False, False),
    "m1-h64-t65-s3": (16, 1, 64, 1, 65, 3, True, False, False),
    "m1-h70-t1-s1": (16, 1, 70, 1, 1, 1, True, False, False),
    "m1-h70-t1-s3": (16, 1, 70, 1, 1, 3, True, False, False),
    "m1-h70-t2-s1": (16, 1, 70, 1, 2, 1, True, False, False),
    "m1-h70-t2-s3": (16, 1, 70, 1, 2, 3, True, False, False),
    "m1-h70-t7-s1": (16, 1, 70, 1, 7, 1, True, False, False),
    "m1-h70-t7-s3": (16, 1, 70, 1, 7, 3, True, False, False),
    "m1-h70-t65-s1": (16, 1, 70, 1, 65, 1, True, False, False),
    "m1-h70-t65-s3": (16, 1, 70, 1, 65, 3, True, False, False),
    # A per state element at the wider states (no model ships these, but supports_op accepts them): k_ssm_scan<64 / 128 / 256, per-element A>
    "m1-d64-hd48-h3-g1-t7-s3": (64, 48, 3, 1, 7, 3, True, False, False),
    "m1-d128-hd5-h3-g3-t65-s1": (128, 5, 3, 3, 65, 1, True, False, False),
    "m1-d256-hd64-h1-g1-t2-s3": (256, 64, 1, 1, 2, 3, True, False, False),
    # Mamba-2 form: A per head
    "m2-d128-hd64-h3-g1-t1-s3": (128, 64, 3, 1, 1, 3, False, False, False),
    "m2-d128-hd64-h3-g3-t7-s1": (128, 64, 3, 3, 7, 1, False, False, False),
    "m2-d128-hd48-h3-g1-t65-s1": (128, 48, 3, 1, 65, 1, False, False, False),
    "m2-d128-hd48-h3-g3-t2-s3": (128, 48, 3, 3, 2, 3, False, True, False),
    "m2-d64-hd64-h1-g1-t7-s3": (64, 64, 1, 1, 7, 3, False, False, False),
    "m2-d64-hd48-h3-g3-t65-s1": (64, 48, 3, 3, 65, 1, False, False, False),
    "m2-d64-hd48-h3-g1-t2-s3": (64, 48, 3, 1, 2, 3, False, False, False),
    "m2-d256-hd64-h3-g1-t2-s3": (256, 64, 3, 1, 2, 3, False, False, False),
    "m2-d256-hd48-h1-g1-t65-s1": (256, 48, 1, 1, 65, 1, False, False, False),
    "m2-d256-hd48-h3-g3-t7-s3": (256, 48, 3, 3, 7, 3, False, False, False),
    "m2-d16-hd5-h3-g1-t7-s3": (16, 5, 3, 1, 7, 3, False, False, False),     # A per head at d_state 16, rows that straddle heads inside a wave
    "m2-d128-hd64-h3-g1-t7-s3-xbc": (128, 64, 3, 1, 7, 3, False, False, True),
    "m2-d128-hd48-h3-g3-t7-s3-xbc": (128, 48, 3, 3, 7, 3, False, False, True),
}


@functools.lru_cache(maxsize=None)
def scan_inputs(name):
    d_state, head_dim, n_head, n_group, n_t, n_s, m1, dup, xbc = SCAN_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + 11)
    n_rs = n_s + 2
    f = np.float32
    ids = {1: [2], 3: [4, 2, 3]}[n_s]  # a permutation into the cache that sends no sequence to the row of its own index
    if dup:
        ids = [4, 2, 4]  # two sequences start from one row
    inp = {
        "s": rng.standard_normal((n_rs, n_head, head_dim, d_state)).astype(f),
        "x": rng.standard_normal((n_s, n_t, n_head, head_dim)).astype(f),
        "B": rng.standard_normal((n_s, n_t, n_group, d_state)).astype(f),
        "C": rng.standard_normal((n_s, n_t, n_group, d_state)).astype(f),
        "ids": np.array(ids, dtype=np.int32),
    }
    # softplus(dt) around 0.05 .. 3 as a trained dt_proj gives, with the values of DT_SPECIAL spread over heads, tokens and sequences
    dt = rng.uniform(-3.0, 3.0, (n_s, n_t, n_head)).astype(f)
    flat = dt.reshape(-1)
    assert flat.size >= len(DT_SPECIAL), name
    for k, v in enumerate(DT_SPECIAL):
        flat[(k * flat.size) // len(DT_SPECIAL) + flat.size // (2 * len(DT_SPECIAL))] = v  # (half a step in: token 0 of a long case keeps its start state)
    inp["dt"] = dt
    if m1:  # A = -(1 .. d_state) scaled per head, as Mamba-1's S4D-real initialisation
        inp["A"] = (-(np.arange(1, d_state + 1, dtype=np.float64))[None, :] * (16.0 / d_state) * rng.uniform(0.05, 0.2, (n_head, 1))).astype(f)
    else:
        inp["A"] = (-rng.uniform(0.05, 1.5, (n_head, 1))).astype(f)
    return inp


@functools.lru_cache(maxsize=None)
def scan_reference(name):
    """(float64 twin with envelopes and bounds, R of the f32 twin, (gate y, gate states)) of a case: computed once, shared."""
    inp = scan_inputs(name)
    ref = scan64(inp)
    R = twin_ratio(ref, *scan32(inp))
    return ref, R, scan_gates(ref, R)
