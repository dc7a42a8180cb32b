"""NumPy twins of the ops a linear-attention recurrent layer adds — RWKV_WKV6, GATED_LINEAR_ATTN, RWKV_WKV7, L2_NORM, SQR, REPEAT — with the gates the GPU tests
hold csrc/rwkv.hip to (the CPU oracle has none of these ops), and the inputs those tests run on.  The operand contracts are DESIGN.md §4k's.

Arrays are in NumPy order, ggml's dimensions reversed.  S = head size, H = heads, T = n_seqs * n_t tokens, the tokens of sequence s being [s n_t, (s + 1) n_t):
    k, v, r, td (g, q, w, a, b)  (T, H, S)        tf (H, S)        state (n_seqs, H, S, S) with element [s, h, i, j]
    result: y (T, H, S), then the new states (n_seqs, H, S, S) — `split` takes the op's flat result apart.

u = 2^-24 is the unit roundoff of f32.  These ops hold products and sums only — no libm call — so a bound needs no function constant: every operation is correctly
rounded, off by at most u of its own result, and a result is at most its absolute-value envelope — the same recurrence run over |operands|, E below.  To first
order the bound e (in units of u) of a state element follows the recurrence itself, one term per operation.  N counts the roundings of partial sums allowed to a
reduction over S terms: a sum of S terms taken in ANY order has at most S - 1 additions, each of a partial sum no larger than the envelope of the whole sum, so
N = S bounds the contract's order (the f32 twin is checked against that); the kernels reduce in another order (lane-local runs, then a DPP tree) and the gate
allows them a second S: N = 2 S.  No measured constant enters.

RWKV_WKV6, per token, head and state element [i, j] (kv = v[j] k[i]; prev, cur the state before and after the token):
    kv                         one rounding:                                                u |kv|
    cur = prev td[i] + kv      the product, the sum, kv's rounding, prev's error carried:   e_t = e_(t-1) |td| + 2 E_(t-1) |td| + 2 |kv|,   E_t = E_(t-1) |td| + |kv|
    term = (kv tf[i] + prev) r[i]   roundings of kv, kv tf, the sum, the product with r:    e_(t-1) |r| + (4 |kv tf| + 2 E_(t-1)) |r|   <=  e_(t-1) |r| + 4 Ty,
                                                                                            Ty = (|kv tf| + E_(t-1)) |r|
    y[j] = sum over i of term                                                               e_y = sum_i e_(t-1) |r| + (4 + N) Ey,   Ey = sum_i Ty
GATED_LINEAR_ATTN: tmp = prev g[i] + kv is WKV6's cur (same e_t, E_t with g for td); qs = q[i] scale rounds once, term = tmp qs once more:
    e_y = sum_i e_t |qs| + (2 + N) Ey,   Ey = sum_i E_t |qs|
RWKV_WKV7, per token, head and state element [i, j] (j is reduced):
    sa = sum over j of a[j] prev[i, j]         e_sa = sum_j e_(t-1) |a| + (1 + N) Esa,   Esa = sum_j |a| E_(t-1)
    cur = (prev w[j] + v[i] k[j]) + sa b[j]    three products, two sums:   e_t = e_(t-1) |w| + e_sa |b| + 3 E_(t-1) |w| + 3 |v k| + 2 Esa |b|,
                                                                           E_t = E_(t-1) |w| + |v k| + Esa |b|
    y[i] = sum over j of cur r[j]              e_y = sum_j e_t |r| + (1 + N) Ey,   Ey = sum_j E_t |r|
The gate of a result is  u e SECOND_ORDER + FLOOR (S + 1):  SECOND_ORDER = 1 + 2^-10 for the terms in u^2 the recurrences drop, FLOOR = 2^-120 for results that
underflow (decays within 2^-10 of zero are among the inputs), where a rounding is absolute instead of relative.

L2_NORM: y = x / max(sqrt(sum x^2), eps).  ne0 roundings of the squares and ne0 of the partial sums are each at most u of sum x^2 and reach sqrt halved:
ne0 u |y| together; sqrt, the reciprocal and the product round once each, and the conversion of a double sum to f32 once: (ne0 + 4) u |y| against float64.
Rows with sqrt(sum x^2) < eps are x / eps.   SQR and REPEAT: bit-equal to NumPy's f32.
"""
import zlib

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -120
SECOND_ORDER = 1.0 + 2.0 ** -10

OPS = ("wkv6", "gla", "wkv7")
N_SRC = {"wkv6": ("k", "v", "r", "tf", "td", "state"), "gla": ("k", "v", "q", "g", "state"), "wkv7": ("r", "w", "k", "v", "a", "b", "state")}
# mistakes the gate must reject, and the ops each can be made in
WRONG = {
    "state_not_carried": OPS, "seq_state_offset_ignored": OPS, "state_transposed": OPS,
    "bonus_into_state": ("wkv6",), "decay_per_head": ("wkv6", "gla"), "scale_dropped": ("gla",),
    "sa_from_updated_state": ("wkv7",), "a_b_swapped": ("wkv7",), "y_before_update": ("wkv7",),
}


def dims(op, inp):
    n_seqs, H, S, _ = inp["state"].shape
    T = inp["k"].shape[0]
    assert T % n_seqs == 0
    return S, H, T, n_seqs, T // n_seqs


# ------------------------------------------------------------------------------------------------ float64 twins with envelopes and bounds
def _wkv6_64(inp, gla, wrong, N):
    S, H, T, n_seqs, n_t = dims("wkv6", inp)
    f = np.float64
    k, v, state = inp["k"].astype(f), inp["v"].astype(f), inp["state"].astype(f)
    r = inp["q" if gla else "r"].astype(f)
    td = inp["g" if gla else "td"].astype(f)
    if gla:
        scale = 1.0 if wrong == "scale_dropped" else float(inp["scale"])
        # (the f32 product q * scale is an operation of the contract; the float64 twin takes it exactly)
        r = r * scale
    else:
        tf = inp["tf"].astype(f)[:, :, None]
    if wrong == "decay_per_head":
        td = np.repeat(td[:, :, :1], S, axis=2)
    y, Ey, ey = (np.zeros((T, H, S)) for _ in range(3))
    st, Es, es = (np.zeros((n_seqs, H, S, S)) for _ in range(3))
    for s in range(n_seqs):
        first = state[0 if wrong == "seq_state_offset_ignored" else s]
        if wrong == "state_transposed":
            first = first.transpose(0, 2, 1)
        prev, E, e = first.copy(), np.abs(first), np.zeros_like(first)
        for t in range(s * n_t, (s + 1) * n_t):
            if wrong == "state_not_carried":
                prev, E, e = first.copy(), np.abs(first), np.zeros_like(first)
            kv = k[t][:, :, None] * v[t][:, None, :]  # [h, i, j]
            akv = np.abs(kv)
            rt, dt = r[t][:, :, None], td[t][:, :, None]
            art, adt = np.abs(rt), np.abs(dt)
            cur = prev * dt + kv
            e_cur = e * adt + 2.0 * E * adt + 2.0 * akv
            E_cur = E * adt + akv
            if gla:
                y[t] = (cur * rt).sum(1)
                Ey[t] = (E_cur * art).sum(1)
                ey[t] = (e_cur * art).sum(1) + (2.0 + N) * Ey[t]
            else:
                y[t] = ((kv * tf + prev) * rt).sum(1)
                Ey[t] = ((akv * np.abs(tf) + E) * art).sum(1)
                ey[t] = (e * art).sum(1) + (4.0 + N) * Ey[t]
                if wrong == "bonus_into_state":
                    cur = kv * tf + prev
            prev, E, e = cur, E_cur, e_cur
        st[s], Es[s], es[s] = prev, E, e
    return {"y": y, "st": st, "Ey": Ey, "Es": Es, "ey": ey, "es": es}


def _wkv7_64(inp, wrong, N):
    S, H, T, n_seqs, n_t = dims("wkv7", inp)
    f = np.float64
    r, w, k, v, a, b, state = (inp[n].astype(f) for n in N_SRC["wkv7"])
    if wrong == "a_b_swapped":
        a, b = b, a
    y, Ey, ey = (np.zeros((T, H, S)) for _ in range(3))
    st, Es, es = (np.zeros((n_seqs, H, S, S)) for _ in range(3))
    for s in range(n_seqs):
        first = state[0 if wrong == "seq_state_offset_ignored" else s]
        if wrong == "state_transposed":
            first = first.transpose(0, 2, 1)
        prev, E, e = first.copy(), np.abs(first), np.zeros_like(first)
        for t in range(s * n_t, (s + 1) * n_t):
            if wrong == "state_not_carried":
                prev, E, e = first.copy(), np.abs(first), np.zeros_like(first)
            at, bt, wt, rt, kt = (x[t][:, None, :] for x in (a, b, w, r, k))  # [h, 1, j]
            vk = v[t][:, :, None] * kt                                        # [h, i, j]
            base = prev * wt + vk if wrong == "sa_from_updated_state" else prev
            sa = (at * base).sum(2, keepdims=True)
            Esa = (np.abs(at) * E).sum(2, keepdims=True)
            e_sa = (np.abs(at) * e).sum(2, keepdims=True) + (1.0 + N) * Esa
            cur = (prev * wt + vk) + sa * bt
            E_cur = E * np.abs(wt) + np.abs(vk) + Esa * np.abs(bt)
            e_cur = e * np.abs(wt) + e_sa * np.abs(bt) + 3.0 * E * np.abs(wt) + 3.0 * np.abs(vk) + 2.0 * Esa * np.abs(bt)
            y[t] = ((prev if wrong == "y_before_update" else cur) * rt).sum(2)
            Ey[t] = (E_cur * np.abs(rt)).sum(2)
            ey[t] = (e_cur * np.abs(rt)).sum(2) + (1.0 + N) * Ey[t]
            prev, E, e = cur, E_cur, e_cur
        st[s], Es[s], es[s] = prev, E, e
    return {"y": y, "st": st, "Ey": Ey, "Es": Es, "ey": ey, "es": es}


def twin64(op, inp, wrong=None, reordered=True):
    """float64 twin of `op` on `inp`: y, st, the envelopes Ey / Es and the first-order bounds ey / es in units of u — for a reduction in any order twice over
    (reordered: N = 2 S, the kernels' gate) or in the contract's order (N = S, what the f32 twin is held to).  wrong: one of WRONG — a twin with that mistake."""
    assert wrong is None or op in WRONG[wrong], (op, wrong)
    S = inp["state"].shape[2]
    N = (2.0 if reordered else 1.0) * S
    return _wkv7_64(inp, wrong, N) if op == "wkv7" else _wkv6_64(inp, op == "gla", wrong, N)


# ------------------------------------------------------------------------------------------------ f32 twins, the contract's order
def twin32(op, inp):
    """f32, every product and sum rounded, in the contract's order (the reductions ascending from the first term)."""
    S, H, T, n_seqs, n_t = dims(op, inp)
    f = np.float32
    y = np.zeros((T, H, S), dtype=f)
    st = np.zeros((n_seqs, H, S, S), dtype=f)
    x = {n: np.asarray(inp[n], dtype=f) for n in N_SRC[op]}
    for s in range(n_seqs):
        prev = x["state"][s].copy()
        for t in range(s * n_t, (s + 1) * n_t):
            if op == "wkv7":
                at, bt, wt, rt, kt = (x[n][t][:, None, :] for n in ("a", "b", "w", "r", "k"))
                vk = x["v"][t][:, :, None] * kt
                sa = np.add.accumulate(at * prev, axis=2, dtype=f)[:, :, -1:]
                cur = (prev * wt + vk) + sa * bt
                y[t] = np.add.accumulate(cur * rt, axis=2, dtype=f)[:, :, -1]
            else:
                kv = x["k"][t][:, :, None] * x["v"][t][:, None, :]
                if op == "gla":
                    qs = (x["q"][t] * f(inp["scale"]))[:, :, None]
                    cur = prev * x["g"][t][:, :, None] + kv
                    term = cur * qs
                else:
                    term = (kv * x["tf"][:, :, None] + prev) * x["r"][t][:, :, None]
                    cur = prev * x["td"][t][:, :, None] + kv
                y[t] = np.add.accumulate(term, axis=1, dtype=f)[:, -1, :]
            assert cur.dtype == f
            prev = cur
        st[s] = prev
    return y, st


def gates(ref):
    """(gate of y, gate of the states) of a twin64 result, element by element."""
    S = ref["st"].shape[2]
    return U * ref["ey"] * SECOND_ORDER + FLOOR * (S + 1), U * ref["es"] * SECOND_ORDER + FLOOR * (S + 1)


def excess(ref, y, st):
    """The largest |got - float64| over its gate, for y and for the states: <= 1 passes."""
    gy, gs = gates(ref)
    return (float(np.max(np.abs(np.asarray(y, dtype=np.float64).reshape(ref["y"].shape) - ref["y"]) / gy)),
            float(np.max(np.abs(np.asarray(st, dtype=np.float64).reshape(ref["st"].shape) - ref["st"]) / gs)))


def split(flat, inp):
    """The op's result [C, T + S n_seqs] taken apart: y (T, H, S) first, then the states per sequence (n_seqs, H, S, S)."""
    n_seqs, H, S, _ = inp["state"].shape
    T = inp["k"].shape[0]
    flat = np.asarray(flat).reshape(-1)
    assert flat.size == H * S * (T + S * n_seqs)
    return flat[:T * H * S].reshape(T, H, S), flat[T * H * S:].reshape(n_seqs, H, S, S)


def join(y, st):
    return np.concatenate([np.asarray(y).reshape(-1), np.asarray(st).reshape(-1)])


def one_sequence(op, inp, s):
    """The inputs of sequence s alone, as a launch with n_seqs = 1."""
    S, H, T, n_seqs, n_t = dims(op, inp)
    out = {}
    for n, a in inp.items():
        if n == "state":
            out[n] = a[s:s + 1].copy()
        elif n in ("tf", "scale"):
            out[n] = a
        else:
            out[n] = a[s * n_t:(s + 1) * n_t].copy()
    return out


# ------------------------------------------------------------------------------------------------ inputs
def decays(rng, shape):
    """Decays in (0, 1), among them values within 2^-10 of 0 and of 1."""
    d = rng.uniform(0.05, 0.999, shape).astype(np.float32)
    flat = d.reshape(-1)
    flat[::7] = np.float32(2.0 ** -11)
    flat[3::11] = np.float32(1.0 - 2.0 ** -12)
    return d


def inputs(op, S, H, n_seqs, n_t, kind="rand", seed=None):
    """Signed operands, non-zero initial states, decays per `decays`.  kind: rand | indicator (one non-zero k and v element per head and token, the state zero:
    a misplaced index lands in a wrong cell exactly) | zero_decay (the state is forgotten) | unit_decay."""
    if seed is None:
        seed = zlib.crc32(f"{op}-{S}-{H}-{n_seqs}-{n_t}-{kind}".encode())
    rng = np.random.default_rng(seed)
    T = n_seqs * n_t
    f = np.float32

    def tok(scale=1.0):
        return (rng.standard_normal((T, H, S)) * scale).astype(f)

    inp = {"state": rng.standard_normal((n_seqs, H, S, S)).astype(f)}
    dec = decays(rng, (T, H, S))
    if kind == "zero_decay":
        dec[:] = 0.0
    elif kind == "unit_decay":
        dec[:] = 1.0
    if op == "wkv7":
        inp.update(r=tok(), w=dec, k=tok(0.5), v=tok(), a=tok(0.5 / np.sqrt(S)), b=tok(0.5 / np.sqrt(S)))
    elif op == "gla":
        inp.update(k=tok(0.5), v=tok(), q=tok(), g=dec, scale=f(0.37))
    else:
        inp.update(k=tok(0.5), v=tok(), r=tok(), tf=(rng.standard_normal((H, S)) * 0.5).astype(f), td=dec)
    if kind == "indicator":
        inp["state"][:] = 0.0
        for n in ("k", "v"):
            inp[n][:] = 0.0
        for t in range(T):
            for h in range(H):
                inp["k"][t, h, (5 * t + 11 * h + 3) % S] = 1.0 + h
                inp["v"][t, h, (7 * t + 13 * h + 1) % S] = 2.0 + t
        if op == "wkv7":  # (a and b would spread the one cell over its row)
            inp["a"][:] = 0.0
            inp["b"][:] = 0.0
    return inp


# ------------------------------------------------------------------------------------------------ L2_NORM, SQR, REPEAT
def l2_norm64(x, eps):
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return x / np.maximum(n, eps)


def l2_norm32(x, eps):
    """ggml-cpu's order: the squares f32 products, their sum in double, sqrtf, the reciprocal, the product."""
    x = np.asarray(x, dtype=np.float32)
    s = (x * x).astype(np.float64).sum(-1, keepdims=True)
    scale = np.float32(1.0) / np.maximum(np.sqrt(s.astype(np.float32)), np.float32(eps))
    return (x * scale).astype(np.float32)


def l2_norm_gate(x, eps):
    return (np.asarray(x).shape[-1] + 4) * U * np.abs(l2_norm64(x, eps))


def sqr(x):
    x = np.asarray(x, dtype=np.float32)
    return x * x


def repeat(a, ne):
    """ggml_repeat of a (NumPy order, 4-D) to the ggml extents ne."""
    a = np.asarray(a)
    reps = [n // s for n, s in zip(ne[::-1], a.shape)]
    assert all(n % s == 0 for n, s in zip(ne[::-1], a.shape))
    return np.tile(a, reps)
