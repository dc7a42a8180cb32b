"""Batch-1 MUL_MAT_ID launches (up / gate and down nodes of the Mixtral and Qwen3-30B-A3B expert shapes) next to the dense one-column mat-vec of a 2-D
matrix of the same type and the same byte count (n_used * N rows).  Run it under `rocprofv3 --kernel-trace --stats -d DIR -o mmid -- python
scripts/ubench/mmid_bench.py [type] [n_tokens]` and read the trace with `scripts/trace_by_grid.py DIR/.../mmid_kernel_trace.csv k_mm` (every configuration has a
grid size of its own); `--group 0,2` times the node under each value of the backend's mmid_group switch (0: the pair form, 2: the grouped matrix-core form forced on), `--windows 5` takes
five windows per cell (median, lowest, highest);
with n_tokens > 1 (the larger-batch form: the same launch over more pairs) the dense yardstick is the batch mat-mul of that matrix
with n_tokens columns.  Type `mxfp4` times the gpt-oss expert shapes instead (K = N = 2880, 4 of 32 and 4 of 128 experts, one activation row a token and one a
slot), each node with its ADD_ID riding in the store as gpt-oss runs it, and no dense yardstick (no gpt-oss file has a dense MXFP4 matrix).  The script itself prints the hipEvent-bracketed class times of the backend's timing option as a cross-check."""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402

SHAPES = {"mixtral-up": (4096, 14336, 8, 2, False), "mixtral-down": (14336, 4096, 8, 2, True),
          "qwen3-up": (2048, 768, 128, 8, False), "qwen3-down": (768, 2048, 128, 8, True)}
GPTOSS_SHAPES = {"oss20b-up": (2880, 2880, 32, 4, False), "oss20b-down": (2880, 2880, 32, 4, True),
                 "oss120b-up": (2880, 2880, 128, 4, False), "oss120b-down": (2880, 2880, 128, 4, True)}
TYPES = {"q4_K": L.Q4_K, "q5_K": L.Q5_K, "q6_K": L.Q6_K, "q8_0": L.Q8_0, "mxfp4": L.MXFP4}


def mxfp4_experts(K, N, n_expert, rng):
    """[n_expert, N, K / 32 * 17] random codes, the block exponents around the value that gives a row a trained network's scale (tests/mxfp4_ref.py: rand_blocks)"""
    W = rng.integers(0, 256, (n_expert, N, K // 32, 17), dtype=np.uint8)
    e0 = 128 + int(np.round(np.log2(1.0 / (5.85 * np.sqrt(K)))))
    W[..., 0] = rng.integers(e0 - 2, e0 + 2, W.shape[:3], dtype=np.uint8)
    return W.reshape(n_expert, N, -1)


def run(be, build, reps):
    H = L.host()
    g = T.G(be)
    try:
        out = build(g)
        gf = H.ggml_new_graph_custom(g.ctx, 64, False)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        for _ in range(reps):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
    finally:
        g.free()


def take(flag, default):
    if flag not in sys.argv:
        return default
    i = sys.argv.index(flag)
    v = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return v


def main():
    """mmid_bench.py [type] [n_tokens[,n_tokens..]] [--group G[,G..]] [--windows W]: every shape's weights are made once and serve all token counts and forms;
    a cell is the median over W windows (default 1) of the mean of `reps` launches, printed with the windows' lowest and highest mean."""
    groups = [None if g == "" else int(g) for g in take("--group", "").split(",")]
    windows = int(take("--windows", "1"))
    tname = sys.argv[1] if len(sys.argv) > 1 else "q4_K"
    qtype = TYPES[tname]
    toks = [int(t) for t in (sys.argv[2] if len(sys.argv) > 2 else "1").split(",")]
    be = L.Backend(0)
    be.set_option("graphs", 0)
    be.set_option("timing", 1)
    H = L.host()
    rng = np.random.default_rng(0)
    mx = qtype == L.MXFP4
    for name, (K, N, n_expert, n_used, per_slot) in (GPTOSS_SHAPES if mx else SHAPES).items():
        row_bytes = K // L.TYPE_BLCK[qtype] * L.TYPE_SIZE[qtype]
        W = mxfp4_experts(K, N, n_expert, rng) if mx else np.stack([T.rand_weight(qtype, K, N, rng) for _ in range(n_expert)])
        bias = rng.standard_normal((n_expert, N)).astype(np.float32)
        for n_tok in toks:
            reps = 50 if n_tok == 1 else 10
            ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
            b = rng.standard_normal((n_tok, n_used if per_slot else 1, K)).astype(np.float32)
            full = np.zeros((n_tok, n_expert), dtype=np.int32)
            full[:, :n_used] = ids

            def moe(g):
                as_t = g.new(qtype, [K, N, n_expert], W)
                idt = H.ggml_view_2d(g.ctx, g.new(L.I32, [n_expert, n_tok], full), n_used, n_tok, n_expert * 4, 0)
                mm = H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, b.shape[1], n_tok], b), idt)
                return H.ggml_add_id(g.ctx, mm, g.new(L.F32, [N, n_expert], bias), idt) if mx else mm

            def dense(g):
                w = g.new(qtype, [K, n_used * N], W[:n_used].reshape(n_used * N, -1))
                return H.ggml_mul_mat(g.ctx, w, g.new(L.F32, [K, n_tok], np.ascontiguousarray(b[:, 0])))

            for kind, fn, grp in [("mul_mat_id", moe, g) for g in groups] + ([] if mx else [("dense", dense, None)]):
                if grp is not None:
                    be.set_option("mmid_group", grp)
                per = {}
                for _ in range(windows):
                    be.timing_report(reset=True)
                    run(be, fn, reps)
                    for cls, (cnt, ms, _) in be.timing_report(reset=True).items():
                        if cnt and (cls.startswith("mmid") or cls == "add_id" or cls.startswith("mmvq") or cls.startswith("mmq")):
                            per.setdefault(cls, []).append(ms * 1e3 / cnt)
                nbytes = n_used * N * row_bytes
                for cls, v in sorted(per.items()):
                    us = float(np.median(v))
                    print(f"{tname} n_tokens={n_tok} {name:13s} {kind:10s} group={grp} {cls:28s} windows={len(v)} {us:8.2f} us/launch (min {min(v):.2f} max {max(v):.2f}) {nbytes / 1e6:7.1f} MB {nbytes / us / 1e6:7.3f} TB/s", flush=True)
    be.close()


if __name__ == "__main__":
    main()
