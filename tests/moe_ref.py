"""Helpers for the mixture-of-experts tests: graph builders for llama.cpp's build_moe_ffn sequence and its COMPOSITE reference.

The oracle has no MUL_MAT_ID / ARGSORT / SUM_ROWS (and had no CLAMP when this was written), so the reference is composed from what it has.  ggml-cpu's mul_mat_id is
one vec_dot per (row, slot, token) over that pair's quantised activation row; the oracle's MUL_MAT is the same vec_dot per (row, column),
each column quantised on its own (oracle/ggml_cpu_ref.c: op_mul_mat) — so the product of a (slot, token) pair is a ONE-column MUL_MAT of
the selected expert's 2-D slice (`ggml_view_2d(as, K, N, nb1, id * nb2)`) with that pair's activation row, the ids taken from NumPy.
`mmid_reference` hands the oracle the one-column products of all pairs that chose the same expert as the columns of one MUL_MAT node
(`grouped=True`: a column's result does not depend on its neighbours) or literally one node per pair (`grouped=False`);
tests/test_moe_host.py asserts that both give the same bits.  The rest of the block is oracle ops (SOFT_MAX, GLU, MUL, ADD, DIV) with
NumPy doing argsort, gather, sum and clamp in float32.
"""
import ctypes as C

import numpy as np

import harness as T
import llama_box_amd as L


def expert_weights(qtype, K, N, n_expert, rng):
    """Raw bytes of an `as` tensor [K, N, n_expert]: array [n_expert, N, row bytes] (uint8) or [n_expert, N, K] (f16 / f32)."""
    return np.stack([T.rand_weight(qtype, K, N, rng) for _ in range(n_expert)])


def dequantize(qtype, raw, K):
    """float32 [..., K] of raw rows (the oracle's dequantize_row for block formats)."""
    if qtype in (L.F32, L.F16):
        return raw.astype(np.float32)
    rows = np.ascontiguousarray(raw.reshape(-1, raw.shape[-1]))
    out = np.empty((rows.shape[0], K), dtype=np.float32)
    lib = T.oracle()
    for i in range(rows.shape[0]):
        lib.oracle_dequantize_row(qtype, rows[i].ctypes.data_as(C.c_void_p), out[i].ctypes.data_as(C.c_void_p), K)
    return out.reshape(raw.shape[:-1] + (K,))


def strided_ids(g, ids, n_expert, junk=-7):
    """ids [n_tokens, n_used] as ggml_top_k leaves them: a view of the first n_used columns of an I32 [n_expert, n_tokens] tensor
    (nb[1] = n_expert * 4).  The columns behind the view hold `junk`: a kernel that ignored nb[1] would read it."""
    n_tok, n_used = ids.shape
    full = np.full((n_tok, n_expert), junk, dtype=np.int32)
    full[:, :n_used] = ids
    t = g.new(L.I32, [n_expert, n_tok], full)
    return g.H.ggml_view_2d(g.ctx, t, n_used, n_tok, n_expert * 4, 0)


def expert_view(g, as_t, K, N, e):
    tt = as_t.contents
    return g.H.ggml_view_2d(g.ctx, as_t, K, N, tt.nb[1], int(e) * tt.nb[2])


def compute_in_weights_buffer(g, outs):
    """G.compute for a backend target with the graph's buffer marked as a WEIGHTS buffer first, as a loaded model's expert tensors are: the backend then serves a
    MUL_MAT over a 2-D view of a Q8_0 expert with the quantised mat-vec kernels (a Q8_0 view outside a weights buffer is taken for a KV-cache view and goes
    through an f16 image instead: csrc/graph.cpp, mm_cache_image_ok)."""
    H = g.H
    gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
    for o in outs:
        H.ggml_set_output(o)
        H.ggml_build_forward_expand(gf, o)
    for i in range(gf.contents.n_nodes):
        node = gf.contents.nodes[i]
        if not H.ggml_backend_dev_supports_op(g.target.dev, node):
            raise RuntimeError(f"backend reports supports_op=false for node {i} op={node.contents.op} '{node.contents.name.decode()}'")
    g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, g.target.buft)
    assert g.buf, "buffer allocation failed"
    H.ggml_backend_buffer_clear(g.buf, 0)
    H.ggml_backend_buffer_set_usage(g.buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
    for t, raw in g.inputs:
        H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
    st = H.ggml_backend_graph_compute(g.target.backend, gf)
    if st != 0:
        raise RuntimeError(f"graph compute failed with status {st}")
    return [g.read(o) for o in outs]


def mmid_reference(qtype, W, K, N, cases, n_threads=None, grouped=True):
    """cases: list of (b [n_tokens, rows, K] float32 with rows in (1, n_used), ids [n_tokens, n_used] int) over the same experts W.
    Returns one float32 [n_tokens, n_used, N] per case, from ONE oracle graph of plain MUL_MATs over 2-D expert views."""
    n_threads = n_threads or T.host_threads()
    n_expert = W.shape[0]
    g = T.G("oracle")
    try:
        as_t = g.new(qtype, [K, N, n_expert], W)
        outs, where = [], []
        for ci, (b, ids) in enumerate(cases):
            n_tok, n_used = ids.shape
            assert b.shape[0] == n_tok and b.shape[1] in (1, n_used) and b.shape[2] == K
            assert ids.min() >= 0 and ids.max() < n_expert, "the reference has no expert for this id"
            pairs = [(t, s) for t in range(n_tok) for s in range(n_used)]
            groups = {}
            for t, s in pairs:
                groups.setdefault((int(ids[t, s]),) if grouped else (int(ids[t, s]), t, s), []).append((t, s))
            for key, cols in groups.items():
                be = np.stack([b[t, s if b.shape[1] > 1 else 0] for t, s in cols]).astype(np.float32)
                bt = g.new(L.F32, [K, len(cols)], be)
                outs.append(g.H.ggml_mul_mat(g.ctx, expert_view(g, as_t, K, N, key[0]), bt))
                where.append((ci, cols))
        res = g.compute(outs, n_threads)
    finally:
        g.free()
    ref = [np.zeros((ids.shape[0], ids.shape[1], N), dtype=np.float32) for _, ids in cases]
    for r, (ci, cols) in zip(res, where):
        r = r.reshape(len(cols), N)
        for j, (t, s) in enumerate(cols):
            ref[ci][t, s] = r[j]
    return ref


def mmid_numpy(qtype, W, K, b, ids):
    """The same product on de-quantised weights and unquantised activations, in float64 (the yardstick of the reference itself)."""
    n_tok, n_used = ids.shape
    out = np.zeros((n_tok, n_used, W.shape[1]), dtype=np.float64)
    deq = {}
    for t in range(n_tok):
        for s in range(n_used):
            e = int(ids[t, s])
            if e not in deq:
                deq[e] = dequantize(qtype, W[e], K).astype(np.float64)
            x = b[t, s if b.shape[1] > 1 else 0].astype(np.float64)
            if qtype == L.F16:
                x = x.astype(np.float16).astype(np.float64)
            out[t, s] = deq[e] @ x
    return out


def _oracle(build, n_threads=None):
    return T.run_case(build, "oracle", n_threads or T.host_threads())


class MoeBlock:
    """One expert FFN block in llama.cpp's build_moe_ffn order: softmax router, top-k, weights gathered (and normalised: SUM_ROWS, optional CLAMP, DIV),
    up / gate / down MUL_MAT_ID with a split SwiGLU, MUL by the weights, VIEW + ADD over the slots."""

    def __init__(self, n_embd, n_ff, n_expert, n_used, t_up, t_down, clamp, seed):
        rng = np.random.default_rng(seed)
        self.n_embd, self.n_ff, self.n_expert, self.n_used, self.t_up, self.t_down, self.clamp = n_embd, n_ff, n_expert, n_used, t_up, t_down, clamp
        assert n_embd >= n_expert
        # the router reads the logits off the first n_expert values of x: rows of `gate_inp` are unit vectors, so logit e of a token IS x[e] —
        # the test data sets the margin between the n_used-th and the next probability by construction (router_inputs)
        self.gate_inp = np.zeros((n_expert, n_embd), dtype=np.float32)
        self.gate_inp[np.arange(n_expert), np.arange(n_expert)] = 1.0
        self.w_up = expert_weights(t_up, n_embd, n_ff, n_expert, rng)
        self.w_gate = expert_weights(t_up, n_embd, n_ff, n_expert, rng)
        self.w_down = expert_weights(t_down, n_ff, n_embd, n_expert, rng)

    def router_inputs(self, n_tok, rng, step=None):
        """x [n_tok, n_embd]: logits (the first n_expert values) a fixed step apart in a random order per token, the rest N(0, 1)."""
        step = step or (0.25 if self.n_expert <= 16 else 0.05)
        x = rng.standard_normal((n_tok, self.n_embd)).astype(np.float32)
        for t in range(n_tok):
            x[t, :self.n_expert] = (rng.permutation(self.n_expert) * step).astype(np.float32)
        return x

    def build(self, g, x):
        """The block on target g; returns (out [n_embd, n_tokens], selected ids as a contiguous copy, every node for supports_op)."""
        H, ctx = g.H, g.ctx
        n_tok = x.shape[0]
        ne, nu = self.n_expert, self.n_used
        cur = g.new(L.F32, [self.n_embd, n_tok], x, "x")
        gi = g.new(L.F32, [self.n_embd, ne], self.gate_inp, "ffn_gate_inp")
        up = g.new(self.t_up, [self.n_embd, self.n_ff, ne], self.w_up, "ffn_up_exps")
        gate = g.new(self.t_up, [self.n_embd, self.n_ff, ne], self.w_gate, "ffn_gate_exps")
        down = g.new(self.t_down, [self.n_ff, self.n_embd, ne], self.w_down, "ffn_down_exps")
        logits = H.ggml_mul_mat(ctx, gi, cur)
        probs = H.ggml_soft_max(ctx, logits)
        sel = H.ggml_top_k(ctx, probs, nu)
        w = H.ggml_get_rows(ctx, H.ggml_reshape_3d(ctx, probs, 1, ne, n_tok), sel)  # [1, n_used, n_tokens]
        w = H.ggml_reshape_2d(ctx, w, nu, n_tok)
        wsum = H.ggml_sum_rows(ctx, w)
        if self.clamp:
            wsum = H.ggml_clamp(ctx, wsum, 6.103515625e-5, float("inf"))
        w = H.ggml_div(ctx, w, wsum)
        w = H.ggml_reshape_3d(ctx, w, 1, nu, n_tok)
        cur3 = H.ggml_reshape_3d(ctx, cur, self.n_embd, 1, n_tok)
        u = H.ggml_mul_mat_id(ctx, up, cur3, sel)
        gt = H.ggml_mul_mat_id(ctx, gate, cur3, sel)
        act = H.ggml_swiglu_split(ctx, gt, u)
        ex = H.ggml_mul_mat_id(ctx, down, act, sel)
        ex = H.ggml_mul(ctx, ex, w)
        exc = ex.contents
        out = None
        for s in range(nu):
            v = H.ggml_view_2d(ctx, ex, self.n_embd, n_tok, exc.nb[2], s * exc.nb[1])
            out = v if out is None else H.ggml_add(ctx, out, v)
        if nu == 1:
            out = H.ggml_cont(ctx, out)
        return out, H.ggml_cont(ctx, sel), probs

    def reference(self, x, n_threads=None, products=False):
        """(out [n_tokens, n_embd], ids [n_tokens, n_used], probs [n_tokens, n_expert]) from oracle ops + NumPy glue; with `products` also the (up, gate, down)
        MUL_MAT_ID results [n_tokens, n_used, .]."""
        n_tok = x.shape[0]
        ne, nu = self.n_expert, self.n_used
        H = L.host()

        def router(g):
            cur = g.new(L.F32, [self.n_embd, n_tok], x)
            gi = g.new(L.F32, [self.n_embd, ne], self.gate_inp)
            return H.ggml_soft_max(g.ctx, H.ggml_mul_mat(g.ctx, gi, cur))

        probs = _oracle(router, n_threads)[0].reshape(n_tok, ne)
        ids = np.argsort(-probs, axis=1, kind="stable")[:, :nu].astype(np.int32)
        w = np.take_along_axis(probs, ids, axis=1).astype(np.float32)
        wsum = np.sum(w, axis=1, keepdims=True, dtype=np.float32)
        if self.clamp:
            wsum = np.maximum(wsum, np.float32(6.103515625e-5))
        wn = _oracle(lambda g: H.ggml_div(g.ctx, g.new(L.F32, [nu, n_tok], w), g.new(L.F32, [1, n_tok], wsum)), n_threads)[0].reshape(n_tok, nu)
        xb = x.reshape(n_tok, 1, self.n_embd)
        u = mmid_reference(self.t_up, self.w_up, self.n_embd, self.n_ff, [(xb, ids)], n_threads)[0]
        gt = mmid_reference(self.t_up, self.w_gate, self.n_embd, self.n_ff, [(xb, ids)], n_threads)[0]
        act = _oracle(lambda g: H.ggml_swiglu_split(g.ctx, g.new(L.F32, [self.n_ff, nu * n_tok], gt), g.new(L.F32, [self.n_ff, nu * n_tok], u)), n_threads)[0].reshape(n_tok, nu, self.n_ff)
        ex = mmid_reference(self.t_down, self.w_down, self.n_ff, self.n_embd, [(act, ids)], n_threads)[0]

        def tail(g):
            e = g.new(L.F32, [self.n_embd, nu, n_tok], ex)
            m = H.ggml_mul(g.ctx, e, g.new(L.F32, [1, nu, n_tok], wn))
            mc = m.contents
            out = None
            for s in range(nu):
                v = H.ggml_view_2d(g.ctx, m, self.n_embd, n_tok, mc.nb[2], s * mc.nb[1])
                out = v if out is None else H.ggml_add(g.ctx, out, v)
            return out if nu > 1 else H.ggml_cont(g.ctx, out)

        out = _oracle(tail, n_threads)[0].reshape(n_tok, self.n_embd)
        if products:
            return out, ids, probs, (u, gt, ex)
        return out, ids, probs

    def numpy_f64(self, x, ids):
        """The block in float64 on de-quantised weights and unquantised activations, with the given routing (the floor of the reference itself)."""
        n_tok = x.shape[0]
        logits = x[:, :self.n_expert].astype(np.float64)
        p = np.exp(logits - logits.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        w = np.take_along_axis(p, ids.astype(np.int64), axis=1)
        s = w.sum(axis=1, keepdims=True)
        if self.clamp:
            s = np.maximum(s, 6.103515625e-5)
        w = w / s
        xb = x.reshape(n_tok, 1, self.n_embd)
        u = mmid_numpy(self.t_up, self.w_up, self.n_embd, xb, ids)
        gt = mmid_numpy(self.t_up, self.w_gate, self.n_embd, xb, ids)
        act = gt / (1.0 + np.exp(-gt)) * u
        ex = mmid_numpy(self.t_down, self.w_down, self.n_ff, act, ids)
        return (ex * w[:, :, None]).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the kernel-selection thresholds, read from the source
def mmid_limits():
    """The constants that decide which k_mmid / k_mmid_f form a MUL_MAT_ID node gets, parsed from the expressions in csrc/mmid.hip (launch_mmid_t, launch_mmid),
    csrc/graph.cpp (mm_id_ok) and csrc/common.h (the activation block sizes) — so a changed threshold moves the shapes of tests/test_gpu_moe_edges.py with it.
    If an expression is rewritten, the one pattern below that names it is the line to edit.
      r2_min      N * n_used * n_tokens from which a wave computes two rows            `a.N * npair >= 16384`
      lds_max     bytes of one quantised activation row up to which it is staged in LDS `lds <= 64 * 1024`
      pair_max    n_used * n_tokens the launch (and supports_op) accepts                `a.n_used * a.n_tokens > 65535`, `ids->ne[0] * ids->ne[1] > 65535`
      vec_k       K % vec_k == 0 and ...                                                `(a.K % 8) == 0`
      vec_align   ... every base pointer and stride a multiple of vec_align: the vector branch of k_mmid_f   `& 15) == 0`
      act_bytes   {"q8_K": sizeof(q8k_dev), "q8_0": sizeof(q80_dev)}"""
    import os
    import re

    def src(name):
        with open(os.path.join(L.REPO, "llama_box_amd", "csrc", name)) as f:
            return f.read()

    def one(text, pattern, what):
        m = re.findall(pattern, text)
        assert len(m) == 1, f"{what}: pattern {pattern!r} matches {len(m)} times — the expression moved, edit tests/moe_ref.py: mmid_limits"
        return m[0]

    mm, gr, co = src("mmid.hip"), src("graph.cpp"), src("common.h")
    lim = {
        "r2_min": int(one(mm, r"a\.N \* npair >= (\d+)", "two rows a wave")),
        "lds_max": int(one(mm, r"lds <= (\d+) \* 1024", "LDS budget")) * 1024,
        "pair_max": int(one(mm, r"a\.n_used \* a\.n_tokens > (\d+)", "pair limit of launch_mmid")),
        "vec_k": int(one(mm, r"\(a\.K % (\d+)\) == 0", "vector branch, K")),
        "vec_align": int(one(mm, r"& (\d+)\) == 0;", "vector branch, alignment")) + 1,
        "act_bytes": {"q8_K": int(one(co, r"static_assert\(sizeof\(q8k_dev\) == (\d+)", "q8k_dev")), "q8_0": int(one(co, r"static_assert\(sizeof\(q80_dev\) == (\d+)", "q80_dev"))},
    }
    assert int(one(gr, r"ids->ne\[0\] \* ids->ne\[1\] > (\d+)", "pair limit of mm_id_ok")) == lim["pair_max"], "mm_id_ok and launch_mmid disagree on the pair limit"
    return lim


def lds_free_k(qtype, lim=None):
    """The smallest K whose quantised activation row no longer fits the LDS budget: k_mmid<T, R, false>."""
    lim = lim or mmid_limits()
    kind = "q8_0" if qtype == L.Q8_0 else "q8_K"
    return (lim["lds_max"] // lim["act_bytes"][kind] + 1) * L.TYPE_BLCK[qtype]


# ------------------------------------------------------------------------------------------------ read-out experts
def readout_experts(qtype, K, n_expert, what="values"):
    """The read-out weights of tests/probes.py stacked as the experts of an `as` tensor, expert e's rows rotated by shift(e) = 37 * e (values; e for the K / 32
    rows of the bsums read-out): row j of expert e reads element (j + shift) % rows — reading the wrong expert, or the right expert over the wrong activation
    row, changes the bits.  -> (raw [n_expert, rows, row bytes], shifts)"""
    import probes as P
    base = P.readout_weight(qtype, K) if what == "values" else P.bsums_readout_weight(qtype, K)
    rows = base.shape[0]
    shifts = [(37 * e if what == "values" else e) % rows for e in range(n_expert)]
    assert len(set(shifts)) == n_expert
    return np.stack([np.roll(base, -s, axis=0) for s in shifts]), shifts


def expected_expert_readout(qtype, b, ids, shifts, what="values"):
    """What MUL_MAT_ID(readout_experts, b, ids) must return, from the NumPy twins of the quantisers: [n_tokens, n_used, rows]."""
    import probes as P
    kind = P.act_kind(qtype)
    n_tok, n_used = ids.shape
    flat = b.reshape(-1, b.shape[-1])
    full = (P.expected_readout(kind, flat) if what == "values" else P.expected_bsums_readout(flat)).reshape(n_tok, b.shape[1], -1)
    out = np.empty((n_tok, n_used, full.shape[-1]), np.float32)
    for t in range(n_tok):
        for s in range(n_used):
            out[t, s] = np.roll(full[t, s if b.shape[1] > 1 else 0], -shifts[int(ids[t, s])])
    return out


# ------------------------------------------------------------------------------------------------ routed experts + a dense shared expert
class SharedExpertLayer:
    """One FFN layer of a model with a shared expert (Qwen2-MoE, DeepSeek, Llama-4, GLM-4.5):
        cur = MUL(RMS_NORM(x), w);  routed = build_moe_ffn(cur) — MUL_MAT_IDs on RESHAPE(cur, [K, 1, n_tokens]);  shared = down(swiglu_split(gate(cur), up(cur))) (dense);
        out = ADD(ADD(routed, shared), x).
    One norm output feeds the f32 router MUL_MAT, the routed MUL_MAT_IDs (same data pointer, same nbytes) and the dense quantised chain.
    `order`: "routed_first" / "shared_first" — which branch ggml_build_forward_expand reaches first (build() names the tensors to expand before the sum) —, and
    "shared_up_gate_first": the shared expert's gate and up products, then the whole routed branch, then the rest of the shared expert — the one order in which a
    dense quantised MUL_MAT on `cur` is DIRECTLY followed by a MUL_MAT_ID on the same data pointer and nbytes, so that with routed and shared experts of different
    activation formats (Q8_K / Q8_0) only the `kind` of the activation cache key tells the two quantisations apart."""

    ORDERS = ("routed_first", "shared_first", "shared_up_gate_first")

    def __init__(self, n_embd, n_ff, n_ff_shared, n_expert, n_used, t_up, t_down, ts_up, ts_down, seed):
        self.blk = MoeBlock(n_embd, n_ff, n_expert, n_used, t_up, t_down, False, seed)
        rng = np.random.default_rng(seed + 1000)
        self.n_embd, self.n_ff_shared, self.n_expert, self.n_used, self.ts_up, self.ts_down = n_embd, n_ff_shared, n_expert, n_used, ts_up, ts_down
        self.eps = 1e-5
        # the norm weight is 1 on the router's logit columns and the inputs give those columns mean square ~1 by construction (inputs()),
        # so the logits keep their fixed steps up to the common factor 1 / rms(x)
        self.nw = rng.uniform(0.5, 1.5, n_embd).astype(np.float32)
        self.nw[:n_expert] = 1.0
        self.ws_gate = T.rand_weight(ts_up, n_embd, n_ff_shared, rng)
        self.ws_up = T.rand_weight(ts_up, n_embd, n_ff_shared, rng)
        self.ws_down = T.rand_weight(ts_down, n_ff_shared, n_embd, rng)

    def inputs(self, n_tok, rng):
        """x [n_tok, n_embd]: MoeBlock.router_inputs with the logit step doubled (the norm divides every logit by rms(x), 1 .. 1.3 here)."""
        return self.blk.router_inputs(n_tok, rng, step=0.5)

    def build(self, g, x, order="routed_first", routed_only=False):
        """-> (out [n_embd, n_tokens], ids (contiguous copy), probs, [up, gate, down MUL_MAT_ID nodes], the tensors to expand first — for G.compute(expand_first=...)).
        routed_only: the graph holds the norm and the routed branch alone (out = the routed branch's sum)."""
        assert order in self.ORDERS
        H, ctx, b = g.H, g.ctx, self.blk
        n_tok, ne, nu, E = x.shape[0], self.n_expert, self.n_used, self.n_embd
        tx = g.new(L.F32, [E, n_tok], x, "x")
        cur = H.ggml_mul(ctx, H.ggml_rms_norm(ctx, tx, self.eps), g.new(L.F32, [E], self.nw, "ffn_norm"))

        def routed():
            gi = g.new(L.F32, [E, ne], b.gate_inp, "ffn_gate_inp")
            up = g.new(b.t_up, [E, b.n_ff, ne], b.w_up, "ffn_up_exps")
            gate = g.new(b.t_up, [E, b.n_ff, ne], b.w_gate, "ffn_gate_exps")
            down = g.new(b.t_down, [b.n_ff, E, ne], b.w_down, "ffn_down_exps")
            probs = H.ggml_soft_max(ctx, H.ggml_mul_mat(ctx, gi, cur))
            sel = H.ggml_top_k(ctx, probs, nu)
            w = H.ggml_get_rows(ctx, H.ggml_reshape_3d(ctx, probs, 1, ne, n_tok), sel)
            w = H.ggml_reshape_2d(ctx, w, nu, n_tok)
            w = H.ggml_div(ctx, w, H.ggml_sum_rows(ctx, w))
            w = H.ggml_reshape_3d(ctx, w, 1, nu, n_tok)
            cur3 = H.ggml_reshape_3d(ctx, cur, E, 1, n_tok)
            u = H.ggml_mul_mat_id(ctx, up, cur3, sel)
            gt = H.ggml_mul_mat_id(ctx, gate, cur3, sel)
            dn = H.ggml_mul_mat_id(ctx, down, H.ggml_swiglu_split(ctx, gt, u), sel)
            ex = H.ggml_mul(ctx, dn, w)
            exc = ex.contents
            out = None
            for s in range(nu):
                v = H.ggml_view_2d(ctx, ex, E, n_tok, exc.nb[2], s * exc.nb[1])
                out = v if out is None else H.ggml_add(ctx, out, v)
            if nu == 1:
                out = H.ggml_cont(ctx, out)
            return out, sel, probs, [u, gt, dn]

        def shared_up_gate():
            gt = H.ggml_mul_mat(ctx, g.new(self.ts_up, [E, self.n_ff_shared], self.ws_gate, "ffn_gate_shexp"), cur)
            u = H.ggml_mul_mat(ctx, g.new(self.ts_up, [E, self.n_ff_shared], self.ws_up, "ffn_up_shexp"), cur)
            return gt, u

        def shared(gt_u=None):
            gt, u = gt_u or shared_up_gate()
            return H.ggml_mul_mat(ctx, g.new(self.ts_down, [self.n_ff_shared, E], self.ws_down, "ffn_down_shexp"), H.ggml_swiglu_split(ctx, gt, u))

        if routed_only:
            r, sel, probs, ids3 = routed()
            return r, H.ggml_cont(ctx, sel), probs, ids3, [r]
        if order == "routed_first":
            (r, sel, probs, ids3), sh = routed(), shared()
            first = [r]
        elif order == "shared_first":
            sh = shared()
            r, sel, probs, ids3 = routed()
            first = [sh]
        else:
            gt_u = shared_up_gate()
            r, sel, probs, ids3 = routed()
            sh = shared(gt_u)
            first = [gt_u[0], gt_u[1], r]
        out = H.ggml_add(ctx, H.ggml_add(ctx, r, sh), tx)
        return out, H.ggml_cont(ctx, sel), probs, ids3, first

    def _cur(self, x, n_threads):
        H = L.host()
        return _oracle(lambda g: H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [self.n_embd, x.shape[0]], x), self.eps), g.new(L.F32, [self.n_embd], self.nw)), n_threads)[0].reshape(x.shape)

    def reference(self, x, n_threads=None):
        """(out [n_tokens, n_embd], ids, probs, (up, gate, down) routed products [n_tokens, n_used, .]) from oracle ops + NumPy glue."""
        H = L.host()
        n_tok, E, FS = x.shape[0], self.n_embd, self.n_ff_shared
        cur = self._cur(x, n_threads)
        routed, ids, probs, prods = self.blk.reference(cur, n_threads, products=True)

        def dense(g):
            c = g.new(L.F32, [E, n_tok], cur)
            gt = H.ggml_mul_mat(g.ctx, g.new(self.ts_up, [E, FS], self.ws_gate), c)
            u = H.ggml_mul_mat(g.ctx, g.new(self.ts_up, [E, FS], self.ws_up), c)
            sh = H.ggml_mul_mat(g.ctx, g.new(self.ts_down, [FS, E], self.ws_down), H.ggml_swiglu_split(g.ctx, gt, u))
            return H.ggml_add(g.ctx, H.ggml_add(g.ctx, g.new(L.F32, [E, n_tok], routed), sh), g.new(L.F32, [E, n_tok], x))

        out = _oracle(dense, n_threads)[0].reshape(n_tok, E)
        return out, ids, probs, prods

    def numpy_f64(self, x, ids):
        """The layer in float64 on de-quantised weights and unquantised activations with the given routing."""
        x64 = x.astype(np.float64)
        cur = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + self.eps) * self.nw.astype(np.float64)
        routed = self.blk.numpy_f64(cur, ids)
        wg, wu, wd = (dequantize(t, w, k).astype(np.float64) for t, w, k in ((self.ts_up, self.ws_gate, self.n_embd), (self.ts_up, self.ws_up, self.n_embd), (self.ts_down, self.ws_down, self.n_ff_shared)))
        gt, u = cur @ wg.T, cur @ wu.T
        return routed + (gt / (1.0 + np.exp(-gt)) * u) @ wd.T + x64


def node_ops(g, outs, expand_first=()):
    """[(op, name of src0's root)] of the graph G.compute would hand to the backend for `outs` (nothing is allocated or computed)."""
    H = g.H
    gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
    for o in list(expand_first) + list(outs):
        H.ggml_build_forward_expand(gf, o)
    return [int(gf.contents.nodes[i].contents.op) for i in range(gf.contents.n_nodes)]


def readout_case(qtype, K, n_tok, per_slot, what="values", n_expert=4, n_used=2):
    """One exact read-back case of the quantiser in front of MUL_MAT_ID: -> (W raw experts, b [n_tokens, rows, K] from the edge catalogue, ids, want [n_tokens, n_used, rows])."""
    import probes as P
    rng = np.random.default_rng(5000 + 31 * qtype + K + 7 * n_tok + (1 if per_slot else 0))
    W, shifts = readout_experts(qtype, K, n_expert, what)
    cat, _ = P.edge_activations(P.act_kind(qtype), K, rng)
    rows = n_used if per_slot else 1
    b = np.ascontiguousarray(P.tile_rows(np.roll(cat, -int(rng.integers(0, len(cat))), axis=0), n_tok * rows).reshape(n_tok, rows, K))
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    return W, b, ids, expected_expert_readout(qtype, b, ids, shifts, what)
