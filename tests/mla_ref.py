"""Helpers for the multi-head-latent-attention (MLA) tests: the batched MUL_MAT over a 3-D quantised weight (one matrix per head: llama.cpp's absorbed wk_b / wv_b
of the deepseek2 graph), its per-head 2-D twin, and one whole non-flash MLA attention block with its staged oracle reference and a float64 evaluation.

The contract (csrc/graph.cpp: mm_batched_q_ok; oracle/ggml_cpu_ref.c: op_mul_mat):
    a [K, N, H] quantised,  b [K, M, H * r2, E] f32 at any element-aligned strides,  dst [N, M, H * r2, E]:  dst(:, m, h, e) = a(:, :, h / r2) . q(b(:, m, h, e))
GPU graphs go through moe_ref.compute_in_weights_buffer: outside a WEIGHTS buffer a Q8_0 / 4-5-bit 3-D src0 is taken for a KV-cache view and runs on an f16 image.
"""
import ctypes as C

import numpy as np

import harness as T
import legacy_ref as LG
import llama_box_amd as L
from moe_ref import compute_in_weights_buffer, dequantize  # noqa: F401  (re-exported for the tests)

KQUANTS = (L.Q4_K, L.Q5_K, L.Q6_K)
TYPES = (L.Q8_0,) + LG.FORMATS + KQUANTS  # the nine served formats
NAMES = {L.Q8_0: "q8_0", L.Q4_0: "q4_0", L.Q4_1: "q4_1", L.Q5_0: "q5_0", L.Q5_1: "q5_1", L.IQ4_NL: "iq4_nl", L.Q4_K: "q4_K", L.Q5_K: "q5_K", L.Q6_K: "q6_K"}
LAYOUTS = ("contig", "permuted", "strided", "mla")
PAD = 32      # floats behind every row of the strided layouts
JUNK = 1.0e3  # what they hold: a kernel that ignored a stride would read it


def rand_weight(qt, K, N, rng):
    return LG.rand_weight(qt, K, N, rng) if qt in LG.FORMATS else T.rand_weight(qt, K, N, rng)


def head_weights(qt, K, N, H, rng):
    """Raw bytes of a [K, N, H]: array [H, N, row bytes]."""
    return np.stack([rand_weight(qt, K, N, rng) for _ in range(H)])


def make_b(g, X, layout):
    """The tensor b [K, M, Hb, E] holding X (float32 [E, Hb, M, K], b's logical order) in one of four layouts:
      contig    a plain tensor
      permuted  ggml_permute(p, 0, 2, 1, 3) of a plain p [K, Hb, M, E]: nb[1] > nb[2]
      strided   the first K of every row of a plain [K + PAD, M, Hb, E]: rows further apart than K
      mla       llama.cpp's q_nope: a strided view [K, Hb, M, E] of q [K + PAD, Hb, M, E], permuted (0, 2, 1, 3)"""
    H, ctx = g.H, g.ctx
    X = np.ascontiguousarray(X, dtype=np.float32)
    E, Hb, M, K = X.shape
    if layout == "contig":
        return g.new(L.F32, [K, M, Hb, E], X)
    if layout == "permuted":
        return H.ggml_permute(ctx, g.new(L.F32, [K, Hb, M, E], X.transpose(0, 2, 1, 3)), 0, 2, 1, 3)
    wide = np.full((E, Hb, M, K + PAD), JUNK, dtype=np.float32)
    wide[..., :K] = X
    if layout == "strided":
        p = g.new(L.F32, [K + PAD, M, Hb, E], wide)
        nb = p.contents.nb
        return H.ggml_view_4d(ctx, p, K, M, Hb, E, nb[1], nb[2], nb[3], 0)
    assert layout == "mla", layout
    p = g.new(L.F32, [K + PAD, Hb, M, E], wide.transpose(0, 2, 1, 3))
    nb = p.contents.nb
    return H.ggml_permute(ctx, H.ggml_view_4d(ctx, p, K, Hb, M, E, nb[1], nb[2], nb[3], 0), 0, 2, 1, 3)


def batched_node(g, qt, W, X, layout="contig", name="w_b"):
    """-> (MUL_MAT(a, b), a, b) with a = W [H, N, row bytes] as one [K, N, H] tensor and b = make_b(X)."""
    a = g.new(qt, [X.shape[-1], W.shape[1], W.shape[0]], W, name)
    b = make_b(g, X, layout)
    return g.H.ggml_mul_mat(g.ctx, a, b), a, b


def head_view(g, a, h):
    t = a.contents
    return g.H.ggml_view_2d(g.ctx, a, t.ne[0], t.ne[1], t.nb[1], int(h) * t.nb[2])


def per_head_nodes(g, a, b, one_column=False, head_of=None, swap=False):
    """The same product from 2-D MUL_MATs over ggml_view_2d of each head's matrix: one node per (e, hb) over b's [K, M] slice, or one per (e, hb, m) over one column.
    -> [((e, hb, m0, columns), node)].  head_of(hb): the matrix head hb reads (default hb // r2); swap: the WRONG twin that takes b's dims 1 and 2 for each other."""
    H, ctx = g.H, g.ctx
    ta, tb = a.contents, b.contents
    K, M, Hb, E = tb.ne[0], tb.ne[1], tb.ne[2], tb.ne[3]
    r2 = Hb // ta.ne[2]
    head_of = head_of or (lambda hb: hb // r2)
    s1, s2 = (tb.nb[2], tb.nb[1]) if swap else (tb.nb[1], tb.nb[2])
    out = []
    for e in range(E):
        for hb in range(Hb):
            w = head_view(g, a, head_of(hb))
            if one_column:
                for m in range(M):
                    out.append(((e, hb, m, 1), H.ggml_mul_mat(ctx, w, H.ggml_view_2d(ctx, b, K, 1, s1, m * s1 + hb * s2 + e * tb.nb[3]))))
            else:
                out.append(((e, hb, 0, M), H.ggml_mul_mat(ctx, w, H.ggml_view_2d(ctx, b, K, M, s1, hb * s2 + e * tb.nb[3]))))
    return out


def assemble(where, results, E, Hb, M, N):
    """The per-head results as the batched node's [E, Hb, M, N]."""
    out = np.zeros((E, Hb, M, N), dtype=np.float32)
    for (e, hb, m0, nc), r in zip(where, results):
        out[e, hb, m0:m0 + nc] = np.asarray(r).reshape(nc, N)
    return out


def numpy_f64(qt, W, X, r2):
    """The product on de-quantised weights and unquantised activations in float64: [E, Hb, M, N]."""
    K = X.shape[-1]
    D = dequantize(qt, W, K).astype(np.float64)  # [H, N, K]
    return np.stack([np.stack([X[e, hb].astype(np.float64) @ D[hb // r2].T for hb in range(X.shape[1])]) for e in range(X.shape[0])])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ one MLA attention block
EPS = 1e-6
ROPE_BASE = 10000.0


def rope_f64(x, pos, n_dims):
    """ggml's ROPE in its default (pair (2i, 2i + 1)) mode on x [M, heads, n_dims] float64 at positions pos [M]."""
    i = np.arange(n_dims // 2)
    th = pos.astype(np.float64)[:, None, None] * (ROPE_BASE ** (-2.0 * i / n_dims))[None, None, :]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = x0 * np.cos(th) - x1 * np.sin(th)
    out[..., 1::2] = x0 * np.sin(th) + x1 * np.cos(th)
    return out


class MlaBlock:
    """The attention of one deepseek2 layer without flash attention, from q and the compressed kv row to the output projection, in llama.cpp's order:
        q_nope / q_pe: strided views of q [qk_nope + qk_rope, n_head, M];  kv_cmpr / k_pe: views of kv_cmpr_pe [kv_lora + qk_rope, M]
        q_pe, k_pe = ROPE(views);  kv_cmpr = MUL(RMS_NORM(kv_cmpr), w)
        q_abs = permute(MUL_MAT(wk_b, permute(q_nope, 0, 2, 1, 3)), 0, 2, 1, 3);  Qcur = CONCAT(q_abs, q_pe, 0);  Kcur = CONCAT(kv_cmpr, k_pe, 0)
        CPY Kcur into the f16 K cache [kv_lora + qk_rope, n_kv], CPY transpose(kv_cmpr) into the transposed f16 V cache [n_kv, kv_lora]
        kq = soft_max_ext(MUL_MAT(K [., n_kv, 1], permute(Qcur, 0, 2, 1, 3)), f16 mask, 1 / sqrt(qk_nope + qk_rope))
        kqv = MUL_MAT(wv_b, MUL_MAT(V^T [n_kv, kv_lora, 1], kq));  out = MUL_MAT(wo, cont_2d(permute(kqv, 0, 2, 1, 3)))
    The new tokens take the last M of the n_kv cells; the cells before them hold a random past."""

    def __init__(self, n_head=3, qk_nope=64, qk_rope=32, kv_lora=256, v_head=64, n_kv=40, n_embd=80, t_kb=L.Q8_0, t_vb=L.Q4_K, t_o=L.Q8_0, seed=0):
        rng = np.random.default_rng(seed)
        self.n_head, self.qk_nope, self.qk_rope, self.kv_lora, self.v_head, self.n_kv, self.n_embd = n_head, qk_nope, qk_rope, kv_lora, v_head, n_kv, n_embd
        self.t_kb, self.t_vb, self.t_o = t_kb, t_vb, t_o
        self.wk_b = head_weights(t_kb, qk_nope, kv_lora, n_head, rng)
        self.wv_b = head_weights(t_vb, kv_lora, v_head, n_head, rng)
        self.wo = rand_weight(t_o, n_head * v_head, n_embd, rng)
        self.kv_norm = rng.uniform(0.5, 1.5, kv_lora).astype(np.float32)
        self.scale = float(1.0 / np.sqrt(qk_nope + qk_rope))
        self.kc0 = (rng.standard_normal((n_kv, kv_lora + qk_rope)) * 0.5).astype(np.float16)
        self.vt0 = (rng.standard_normal((kv_lora, n_kv)) * 0.5).astype(np.float16)

    def inputs(self, M, rng):
        """(q [M, n_head, qk_nope + qk_rope], kv_cmpr_pe [M, kv_lora + qk_rope])"""
        return rng.standard_normal((M, self.n_head, self.qk_nope + self.qk_rope)).astype(np.float32), rng.standard_normal((M, self.kv_lora + self.qk_rope)).astype(np.float32)

    def mask(self, M):
        m = np.full((64, self.n_kv), -np.inf, dtype=np.float16)  # [n_kv, 64] in ggml order: the rows are padded as llama.cpp pads them
        head = self.n_kv - M
        for t in range(M):
            m[t, :head + t + 1] = 0
        return m

    # -------------------------------------------------------------------------------------------- graph pieces
    def _mm(self, g, a, b, per_head):
        """MUL_MAT(a, b) as the batched node, or as per-head 2-D nodes joined by CONCAT along dim 2 (one column a head: M = 1)."""
        H, ctx = g.H, g.ctx
        if not per_head:
            return H.ggml_mul_mat(ctx, a, b)
        assert b.contents.ne[1] == 1 and b.contents.ne[3] == 1
        out = None
        for _, node in per_head_nodes(g, a, b):
            node = H.ggml_reshape_3d(ctx, node, a.contents.ne[1], 1, 1)
            out = node if out is None else H.ggml_concat(ctx, out, node, 2)
        return out

    def front(self, g, q, kvpe, per_head=False):
        """q, kv_cmpr_pe -> (q_abs [kv_lora, n_head, M] (a permuted view), q_pe [qk_rope, n_head, M], kv_cmpr [kv_lora, M], k_pe [qk_rope, 1, M], wk_b's MUL_MAT)."""
        H, ctx = g.H, g.ctx
        M, nh, dn, dr, dl = q.shape[0], self.n_head, self.qk_nope, self.qk_rope, self.kv_lora
        tq = g.new(L.F32, [dn + dr, nh, M], q, "q")
        tkv = g.new(L.F32, [dl + dr, M], kvpe, "kv_cmpr_pe")
        pos = g.new(L.I32, [M], np.arange(self.n_kv - M, self.n_kv, dtype=np.int32), "pos")
        qnb, knb = tq.contents.nb, tkv.contents.nb
        q_nope = H.ggml_view_3d(ctx, tq, dn, nh, M, qnb[1], qnb[2], 0)
        q_pe = H.ggml_view_3d(ctx, tq, dr, nh, M, qnb[1], qnb[2], dn * 4)
        kv_cmpr = H.ggml_view_2d(ctx, tkv, dl, M, knb[1], 0)
        k_pe = H.ggml_view_3d(ctx, tkv, dr, 1, M, knb[1], knb[1], dl * 4)
        rope = lambda t: H.ggml_rope_ext(ctx, t, pos, None, dr, 0, 4096, ROPE_BASE, 1.0, 0.0, 1.0, 32.0, 1.0)  # noqa: E731
        q_pe, k_pe = rope(q_pe), rope(k_pe)
        kv_cmpr = H.ggml_mul(ctx, H.ggml_rms_norm(ctx, kv_cmpr, EPS), g.new(L.F32, [dl], self.kv_norm, "attn_kv_a_norm"))
        wk_b = g.new(self.t_kb, [dn, dl, nh], self.wk_b, "wk_b")
        mm = self._mm(g, wk_b, H.ggml_permute(ctx, q_nope, 0, 2, 1, 3), per_head)  # [kv_lora, M, n_head]
        return H.ggml_permute(ctx, mm, 0, 2, 1, 3), q_pe, kv_cmpr, k_pe, mm

    def back(self, g, Qcur, kc, vt, M, per_head=False):
        """Qcur [kv_lora + qk_rope, n_head, M] and the caches (already holding the new tokens) -> (out [n_embd, M], wv_b's MUL_MAT)."""
        H, ctx = g.H, g.ctx
        nh, dl, dk, n_kv = self.n_head, self.kv_lora, self.kv_lora + self.qk_rope, self.n_kv
        k = H.ggml_view_3d(ctx, kc, dk, n_kv, 1, dk * 2, dk * 2 * n_kv, 0)
        v = H.ggml_view_3d(ctx, vt, n_kv, dl, 1, n_kv * 2, n_kv * 2 * dl, 0)
        kq = H.ggml_mul_mat(ctx, k, H.ggml_permute(ctx, Qcur, 0, 2, 1, 3))  # [n_kv, M, n_head]
        kq = H.ggml_soft_max_ext(ctx, kq, g.new(L.F16, [n_kv, 64], self.mask(M), "kq_mask"), self.scale, 0.0)
        kqv = H.ggml_mul_mat(ctx, v, kq)  # [kv_lora, M, n_head]
        wv_b = g.new(self.t_vb, [dl, self.v_head, nh], self.wv_b, "wv_b")
        mm = self._mm(g, wv_b, kqv, per_head)  # [v_head, M, n_head]
        cur = H.ggml_cont_2d(ctx, H.ggml_permute(ctx, mm, 0, 2, 1, 3), self.v_head * nh, M)
        return H.ggml_mul_mat(ctx, g.new(self.t_o, [self.v_head * nh, self.n_embd], self.wo, "wo"), cur), mm

    def build(self, g, q, kvpe, per_head=False):
        """The whole block on g -> (out, the cache stores to expand first, {name: tensor} of q / kv_cmpr_pe / the two batched products)."""
        H, ctx = g.H, g.ctx
        M, dl, dk, n_kv = q.shape[0], self.kv_lora, self.kv_lora + self.qk_rope, self.n_kv
        head = n_kv - M
        q_abs, q_pe, kv_cmpr, k_pe, mm_k = self.front(g, q, kvpe, per_head)
        Qcur = H.ggml_concat(ctx, q_abs, q_pe, 0)
        Kcur = H.ggml_concat(ctx, H.ggml_reshape_3d(ctx, kv_cmpr, dl, 1, M), k_pe, 0)  # [kv_lora + qk_rope, 1, M]
        kc = g.new(L.F16, [dk, n_kv], self.kc0, "cache_k")
        vt = g.new(L.F16, [n_kv, dl], self.vt0, "cache_v_t")
        ks = H.ggml_cpy(ctx, H.ggml_reshape_2d(ctx, Kcur, dk, M), H.ggml_view_2d(ctx, kc, dk, M, dk * 2, head * dk * 2))
        vs = H.ggml_cpy(ctx, H.ggml_transpose(ctx, kv_cmpr), H.ggml_view_2d(ctx, vt, M, dl, n_kv * 2, head * 2))
        out, mm_v = self.back(g, Qcur, kc, vt, M, per_head)
        return out, [ks, vs], {"wk_b": mm_k, "wv_b": mm_v, "q": g.inputs[0][0], "kvpe": g.inputs[1][0]}

    # -------------------------------------------------------------------------------------------- references
    def reference(self, q, kvpe, n_threads=None):
        """out [M, n_embd] from the oracle run in two stages; the two CONCATs (copies: the oracle has none) and the two cache stores (f32 -> f16 casts) in NumPy."""
        n_threads = n_threads or T.host_threads()
        M, nh, dl, dr = q.shape[0], self.n_head, self.kv_lora, self.qk_rope
        head = self.n_kv - M

        def stage1(g):
            q_abs, q_pe, kv_cmpr, k_pe, _ = self.front(g, q, kvpe)
            return [g.H.ggml_cont(g.ctx, q_abs), q_pe, kv_cmpr, k_pe]

        q_abs, q_pe, kv_cmpr, k_pe = T.run_case(stage1, "oracle", n_threads)
        Qcur = np.concatenate([q_abs.reshape(M, nh, dl), q_pe.reshape(M, nh, dr)], axis=2)
        Kcur = np.concatenate([kv_cmpr.reshape(M, dl), k_pe.reshape(M, dr)], axis=1)
        kc, vt = self.kc0.copy(), self.vt0.copy()
        kc[head:] = Kcur.astype(np.float16)
        vt[:, head:] = kv_cmpr.reshape(M, dl).astype(np.float16).T

        def stage2(g):
            tq = g.new(L.F32, [dl + dr, nh, M], Qcur)
            return self.back(g, tq, g.new(L.F16, [dl + dr, self.n_kv], kc), g.new(L.F16, [self.n_kv, dl], vt), M)[0]

        return T.run_case(stage2, "oracle", n_threads)[0].reshape(M, self.n_embd)

    def numpy_f64(self, q, kvpe):
        """The block in float64 on de-quantised weights and unquantised activations (the cache entries rounded to f16, as stored): the floor of the reference itself."""
        M, nh, dn, dl = q.shape[0], self.n_head, self.qk_nope, self.kv_lora
        head = self.n_kv - M
        pos = np.arange(head, self.n_kv)
        q64, kv64 = q.astype(np.float64), kvpe.astype(np.float64)
        q_pe = rope_f64(q64[..., dn:], pos, self.qk_rope)
        k_pe = rope_f64(kv64[:, None, dl:], pos, self.qk_rope)[:, 0]
        kv = kv64[:, :dl]
        kv = kv / np.sqrt((kv * kv).mean(axis=1, keepdims=True) + EPS) * self.kv_norm.astype(np.float64)
        Wk = dequantize(self.t_kb, self.wk_b, dn).astype(np.float64)       # [n_head, kv_lora, qk_nope]
        Wv = dequantize(self.t_vb, self.wv_b, dl).astype(np.float64)       # [n_head, v_head, kv_lora]
        Wo = dequantize(self.t_o, self.wo, nh * self.v_head).astype(np.float64)
        q_abs = np.einsum("hlk,mhk->mhl", Wk, q64[..., :dn])
        Q = np.concatenate([q_abs, q_pe], axis=2)                          # [M, n_head, kv_lora + qk_rope]
        kc, vt = self.kc0.astype(np.float64), self.vt0.astype(np.float64)
        kc[head:] = np.concatenate([kv, k_pe], axis=1).astype(np.float16).astype(np.float64)
        vt[:, head:] = kv.astype(np.float16).astype(np.float64).T
        s = np.einsum("ck,mhk->hmc", kc, Q) * self.scale + self.mask(M)[:M].astype(np.float64)[None]
        p = np.exp(s - s.max(axis=2, keepdims=True))
        p /= p.sum(axis=2, keepdims=True)
        kqv = np.einsum("hmc,lc->hml", p, vt)
        o = np.einsum("hvl,hml->mhv", Wv, kqv)
        return o.reshape(M, nh * self.v_head) @ Wo.T


def run_block(backend, blk, steps, per_head=False):
    """The block's graph built ONCE on `backend` in a WEIGHTS buffer and computed for every (q, kv_cmpr_pe) of `steps` (equal M).
    -> ([(out [M, n_embd], wk_b product, wv_b product)], stat deltas over the steps, node count)."""
    H = L.host()
    g = T.G(backend)
    try:
        out, first, t = blk.build(g, steps[0][0], steps[0][1], per_head)
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in first:
            H.ggml_build_forward_expand(gf, o)
        for o in (t["wk_b"], t["wv_b"], out):
            H.ggml_set_output(o)
        H.ggml_build_forward_expand(gf, out)
        for i in range(gf.contents.n_nodes):
            node = gf.contents.nodes[i]
            assert H.ggml_backend_dev_supports_op(backend.dev, node), (i, H.ggml_op_name(node.contents.op), node.contents.name)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        H.ggml_backend_buffer_set_usage(g.buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        keys = ("graph_launches", "graph_captures", "eager_graphs", "kernel_launches", "kv_image_nodes")
        s0 = {k: backend.stat(k) for k in keys}
        res = []
        for q, kvpe in steps:
            for tt, raw in ((t["q"], np.ascontiguousarray(q)), (t["kvpe"], np.ascontiguousarray(kvpe))):
                H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(out).reshape(q.shape[0], blk.n_embd).copy(), g.read(t["wk_b"]).copy(), g.read(t["wv_b"]).copy()))
        return res, {k: backend.stat(k) - v for k, v in s0.items()}, gf.contents.n_nodes
    finally:
        g.free()
