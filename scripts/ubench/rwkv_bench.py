"""RWKV_WKV6, GATED_LINEAR_ATTN and RWKV_WKV7 at model shapes (csrc/rwkv.hip): device time per launch, the state bytes the launch moves (read plus
write) and that over the time as a share of 8 TB/s.

    python scripts/ubench/rwkv_bench.py                 every op, model and shape: one child process per (op, model, shape) under its own `timeout`, warm then
                                                        cold; the run ends at the first child that fails or runs out of time
    python scripts/ubench/rwkv_bench.py OP MODEL SHAPE  that one case in this process

warm: one operand set, launched again and again (a one-sequence state of 1 - 2.6 MB stays in the L2 / the 256 MiB Infinity Cache).  cold: `copies` operand sets of
more than 512 MiB together, one launch each per graph, so that no launch finds its state in a cache.  Every case is warmed up before its timed window; a
window is at least a few hundred launches.  Times: the host clock around a synchronised window, then the backend's hipEvent class times.  There is no pass mark:
the nodes had no GPU form before.  Reads nothing outside the tree; inputs come from a seed."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402

PEAK = 8.0e12  # bytes / s
MODELS = {"rwkv6-7b": (64, 64), "rwkv7-2.9b": (40, 64), "qrwkv6-32b": (40, 128)}  # (heads, head size)
SHAPES = {"decode-s1": (1, 1), "decode-s32": (32, 1), "prompt-512": (1, 512)}    # (n_seqs, n_t)
OPS = {"wkv6": "rwkv_wkv6", "gla": "gated_linear_attn", "wkv7": "rwkv_wkv7"}      # the backend's timing class
CHILD_TIMEOUT_S = 120


def build(g, rng, op, nh, S, n_seqs, n_t):
    H, f = g.H, np.float32
    Tn = n_seqs * n_t

    def tok(scale=1.0):
        return g.new(L.F32, [S, nh, Tn], (rng.standard_normal((Tn, nh, S)) * scale).astype(f))

    def decay():
        return g.new(L.F32, [S, nh, Tn], rng.uniform(0.05, 0.999, (Tn, nh, S)).astype(f))

    state = g.new(L.F32, [S * S * nh, n_seqs], rng.standard_normal((n_seqs, nh * S * S)).astype(f))
    if op == "wkv6":
        return H.ggml_rwkv_wkv6(g.ctx, tok(0.5), tok(), tok(), g.new(L.F32, [S, nh], rng.standard_normal((nh, S)).astype(f)), decay(), state)
    if op == "gla":
        return H.ggml_gated_linear_attn(g.ctx, tok(0.5), tok(), tok(), decay(), state, float(S) ** -0.5)
    r, w, k, v = tok(), decay(), tok(0.5), tok()
    return H.ggml_rwkv_wkv7(g.ctx, r, w, k, v, tok(0.5 / np.sqrt(S)), tok(0.5 / np.sqrt(S)), state)


def measure(be, op, model, shape, mode):
    H = L.host()
    nh, S = MODELS[model]
    n_seqs, n_t = SHAPES[shape]
    nbytes = 2 * 4 * S * S * nh * n_seqs  # the states, read once and written once
    footprint = nbytes + 4 * S * nh * n_seqs * n_t * (7 if op == "wkv7" else 5)  # ... and the per-token operands and y: what a copy keeps out of the caches
    copies = 1 if mode == "warm" else max(2, min(256, -(-(512 << 20) // footprint)))
    reps = max(8, (2000 if n_t == 1 else 200) // copies)
    rng = np.random.default_rng(0)
    g = T.G(be)
    try:
        outs = [build(g, rng, op, nh, S, n_seqs, n_t) for _ in range(copies)]
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in outs:
            H.ggml_set_output(o)
            H.ggml_build_forward_expand(gf, o)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        assert g.buf
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        for _ in range(max(3, 40 // copies)):  # warm-up: code objects, clocks
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        wall_us = (time.perf_counter() - t0) * 1e6 / (reps * copies)
        line = (f"{op:5s} {model:11s} {shape:11s} {mode:4s} copies={copies:3d} launches={reps * copies:5d} state {nbytes / 1e6:8.2f} MB/launch  "
                f"host clock {wall_us:9.2f} us/launch ({nbytes / wall_us / 1e6 / (PEAK / 1e12) * 100:5.1f} % of 8 TB/s)")
        be.set_option("timing", 1)
        be.timing_report(reset=True)
        for _ in range(max(2, reps // 4)):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        for cls, (cnt, ms, _) in sorted(be.timing_report(reset=True).items()):
            if cnt and cls == OPS[op]:
                us = ms * 1e3 / cnt
                line += f" | events n={cnt} {us:9.2f} us ({nbytes / us / 1e6 / (PEAK / 1e12) * 100:5.1f} %)"
        be.set_option("timing", 0)
        print(line, flush=True)
    finally:
        g.free()


def main():
    if len(sys.argv) == 4:
        be = L.Backend(0)
        be.set_option("graphs", 0)
        for mode in ("warm", "cold"):
            measure(be, sys.argv[1], sys.argv[2], sys.argv[3], mode)
        be.close()
        return 0
    for op, model in (("wkv6", "rwkv6-7b"), ("gla", "rwkv6-7b"), ("wkv7", "rwkv7-2.9b"), ("wkv6", "qrwkv6-32b"), ("gla", "qrwkv6-32b"), ("wkv7", "qrwkv6-32b"),
                      ("wkv6", "rwkv7-2.9b"), ("gla", "rwkv7-2.9b"), ("wkv7", "rwkv6-7b")):
        for shape in SHAPES:
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), op, model, shape]).returncode
            if rc != 0:
                print(f"{op} {model} {shape}: exit status {rc}; stopping here", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
