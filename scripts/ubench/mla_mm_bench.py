"""The two batched MUL_MATs of an MLA layer (csrc/mmb.hip) at DeepSeek-V3 and V2-Lite shapes, against the same product built from what the backend
served before the batched node: H separate 2-D MUL_MAT nodes over ggml_view_2d of each head's matrix, in one graph, in a WEIGHTS buffer.

    python scripts/ubench/mla_mm_bench.py [NODE ...]         every node (or the named ones) x M in {1, 8, 32, 512} x {warm, cold} x {batched, per-head}

Graphs are ON, as in the product: after the warm-up a graph_compute is one hipGraph replay, of 2 kernels (batched: quantiser + mat-mul) or of H x (1 or 2) kernels
(per head).  Time: host clock around a synchronised window of replays, over the window's graph_computes and operand sets; the two forms alternate, two windows each,
the faster one is quoted (both are printed).
warm: one operand set, replayed again and again (9 MB of wk_b stay in the 256 MiB Infinity Cache).  cold: `copies` operand sets of more than 300 MB together in one
graph, one node (or H nodes) each, so that no node finds its weights in a cache.
Bytes a node has to move: the weights once, b in, dst out — over the time, as a share of 8 TB/s.  At M = 512 the per-head graph runs matrix-core kernels; the batched
kernel is a mat-vec form and is not expected to keep up there.
Gate: at M = 1 the batched node must not be slower than the per-head graph, warm and cold — the script exits non-zero otherwise.  M = 8, 32 and 512 are recorded only.
Reads nothing outside the tree; inputs come from a seed."""
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402
import mla_ref as R  # noqa: E402

PEAK = 8.0e12  # bytes / s
# (weight type, K, N, heads)
NODES = {
    "v3-wk_b": (L.Q8_0, 128, 512, 128),
    "v3-wv_b": (L.Q4_K, 512, 128, 128),
    "v2lite-wk_b": (L.Q8_0, 128, 512, 16),
    "v2lite-wv_b": (L.Q4_K, 512, 128, 16),
}
MS = (1, 8, 32, 512)


def node_bytes(qt, K, N, Hh, M):
    return Hh * (N * (K // L.TYPE_BLCK[qt]) * L.TYPE_SIZE[qt] + 4 * M * (K + N))


def run_form(be, qt, K, N, Hh, M, W, X, copies, per_head):
    """-> (graph handle pieces to time, first operand set's result [Hh, M, N])"""
    H = L.host()
    g = T.G(be)
    gf = H.ggml_new_graph_custom(g.ctx, 1 << 15, False)
    firsts = []
    for c in range(copies):
        a = g.new(qt, [K, N, Hh], W)
        b = g.new(L.F32, [K, M, Hh], X)
        nodes = [n for _, n in R.per_head_nodes(g, a, b)] if per_head else [H.ggml_mul_mat(g.ctx, a, b)]
        for n in nodes:
            H.ggml_set_output(n)
            H.ggml_build_forward_expand(gf, n)
        if c == 0:
            firsts = nodes
    g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
    assert g.buf
    H.ggml_backend_buffer_set_usage(g.buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
    for t, raw in g.inputs:
        H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
    return g, gf, firsts


def window(be, gf, reps):
    H = L.host()
    t0 = time.perf_counter()
    for _ in range(reps):
        assert H.ggml_backend_graph_compute(be.backend, gf) == 0
    be.synchronize()
    return time.perf_counter() - t0


def measure(be, name, M, mode):
    qt, K, N, Hh = NODES[name]
    nbytes = node_bytes(qt, K, N, Hh, M)
    copies = 1 if mode == "warm" else max(2, -(-300_000_000 // nbytes))
    rng = np.random.default_rng(0)
    W = R.head_weights(qt, K, N, Hh, rng)
    X = rng.standard_normal((Hh, M, K)).astype(np.float32)
    forms, out, launches = {}, {}, {}
    try:
        for per_head in (False, True):
            g, gf, firsts = run_form(be, qt, K, N, Hh, M, W, X, copies, per_head)
            forms[per_head] = (g, gf)
            l0 = be.stat("kernel_launches")
            window(be, gf, 1)  # (eager: counts the launches of one graph_compute)
            launches[per_head] = (be.stat("kernel_launches") - l0) // copies
            window(be, gf, 4)  # warm-up: capture, code objects, clocks
            out[per_head] = np.concatenate([g.read(n).ravel() for n in firsts]).reshape(Hh, M, N)  # (one [N, M, Hh] tensor, or Hh of [N, M])
        err = T.nmse(out[False], out[True])
        same = bool(np.array_equal(R.bits(out[False]), R.bits(out[True])))
        times = {False: [], True: []}
        for per_head in (False, True):  # size the windows: at least 0.2 s each
            est = window(be, forms[per_head][1], 3) / 3
            times[per_head].append(max(5, min(3000, int(0.2 / max(est, 1e-6)))))
        for _ in range(2):
            for per_head in (False, True):
                reps = times[per_head][0]
                times[per_head].append(window(be, forms[per_head][1], reps) / (reps * copies) * 1e6)
        tb, tp = min(times[False][1:]), min(times[True][1:])
        print(f"{name:12s} M={M:3d} {mode:4s} copies={copies:3d} {nbytes / 1e6:7.2f} MB/node | batched {launches[False]:3d} launches {tb:9.2f} us ({nbytes / tb / 1e6 / (PEAK / 1e12) * 100:5.1f} % of 8 TB/s; "
              f"windows {times[False][1]:.2f} {times[False][2]:.2f}) | per-head {launches[True]:3d} launches {tp:9.2f} us ({nbytes / tp / 1e6 / (PEAK / 1e12) * 100:5.1f} %; windows {times[True][1]:.2f} {times[True][2]:.2f}) | "
              f"per-head / batched = {tp / tb:6.2f} | results {'bit-equal' if same else f'nmse {err:.1e}'}", flush=True)
        # the gate: at one token the batched node replaces H launches (or 2 H) by two and must not be slower than the graph it replaces, warm or cold.
        # Larger M are recorded, not gated: the per-head graph runs matrix-core kernels there
        return M != 1 or tb <= tp
    finally:
        for g, _ in forms.values():
            g.free()


def main():
    be = L.Backend(0)
    names = sys.argv[1:] or list(NODES)
    lost = []
    for name in names:
        for M in MS:
            for mode in ("warm", "cold"):
                if not measure(be, name, M, mode):
                    lost.append(f"{name} M={M} {mode}")
    be.close()
    if lost:
        sys.exit("GATE FAILED: the batched node is slower than the per-head graph at one token: " + ", ".join(lost))
    print("gate: at M = 1 the batched node is not slower than the per-head graph, warm and cold, on every node measured")


if __name__ == "__main__":
    main()
