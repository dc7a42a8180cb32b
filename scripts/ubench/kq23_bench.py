"""MUL_MAT over Q2_K / Q3_K weights next to the same shape in Q4_K (block layout, a plain buffer: no decode copy), per format:

  batch 1     (K 4096, N 14336), (K 14336, N 4096), (K 4096, N 4096): the mat-vec launch, its bytes per second and both as ratios to the Q4_K launch.
              Q3_K holds 0.76 and Q2_K 0.58 of Q4_K's bytes: a launch LONGER than Q4_K's is marked `MISSES`.
  batches     32 and 512 columns at (K 4096, N 4096): the int8 tile kernel against Q4_K's batch launch, and against the same batch as passes of the 8-column
              mat-vec (measured at 8 columns, times ceil(M / 8)): a tile launch slower than those passes is marked `KILL`.
  --e2e       batch-1 tokens/s of llama3-8b-q3_k_m through llm_decode_steps, next to llama3-8b-q4_k_m, in this run.

`python scripts/ubench/kq23_bench.py [--e2e] [--layers L] [--out FILE]` prints the hipEvent-bracketed class times of the backend's timing option (graphs off: one
class per launch kind; the activation quantisation is a class of its own and is listed beside the product).  For the kernel-trace view run it under
`rocprofv3 --kernel-trace --stats -d DIR -o kq23 -- python scripts/ubench/kq23_bench.py` and read DIR/.../kq23_kernel_stats.csv: the rows named k_mmvq*,
k_mmq_i8* and k_quantize* are the launches timed here."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import kq23_ref as R  # noqa: E402
import llama_box_amd as L  # noqa: E402
from model_util import Context, Model, preset  # noqa: E402

FORMATS = (L.Q4_K,) + R.FORMATS
NAME = {L.Q4_K: "q4_K", L.Q2_K: "q2_K", L.Q3_K: "q3_K"}
MATVEC = [(4096, 14336), (14336, 4096), (4096, 4096)]
BATCH = (4096, 4096)
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def weight(qt, K, N, rng):
    """N rows cut from 64 random ones: the kernels' time does not depend on the values, the host's does on how many it draws."""
    base = (T.rand_weight if qt == L.Q4_K else R.rand_weight)(qt, K, 64, rng)
    return np.ascontiguousarray(np.tile(base, ((N + 63) // 64, 1))[:N])


def timed(be, qt, K, N, M, W, rng, reps):
    """-> ({class: us per launch} of the product's classes, us per graph of the activation quantisation, launches per graph)"""
    H = L.host()
    X = rng.standard_normal((M, K)).astype(np.float32)
    g = T.G(be)
    try:
        out = H.ggml_mul_mat(g.ctx, g.new(qt, [K, N], W), g.new(L.F32, [K, M], X))
        gf = H.ggml_new_graph_custom(g.ctx, 64, False)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        for _ in range(3):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        be.timing_report(reset=True)
        k0 = be.stat("kernel_launches")
        for _ in range(reps):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        launches = (be.stat("kernel_launches") - k0) / reps
        rep = be.timing_report(reset=True)
    finally:
        g.free()
    prod = {c: ms * 1e3 / reps for c, (n, ms, _) in rep.items() if n and (c.startswith("mmvq") or c.startswith("mmq"))}
    quant = sum(ms * 1e3 / reps for c, (n, ms, _) in rep.items() if n and c.startswith("quantize"))
    return prod, quant, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--layers", type=int, default=0, help="layers of the end-to-end models (0: all 32)")
    ap.add_argument("--vocab", type=int, default=0, help="vocabulary rows of the end-to-end models (0: all 128256; the host draws every block)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    be = L.Backend(0)
    be.set_option("graphs", 0)
    be.set_option("timing", 1)
    rng = np.random.default_rng(0)
    say("# batch 1: us per graph of the product's launches (class), of the activation quantisation beside it, MB of weights, TB/s of the product; ratios to q4_K")
    for K, N in MATVEC:
        base = None
        for qt in FORMATS:
            W = weight(qt, K, N, rng)
            prod, quant, launches = timed(be, qt, K, N, 1, W, rng, 50)
            us = sum(prod.values())
            rate = W.nbytes / us / 1e6
            if qt == L.Q4_K:
                base = (us, rate)
            verdict = "" if qt == L.Q4_K else ("  ok" if us <= base[0] else "  MISSES (longer than the q4_K launch)")
            say(f"K={K:5d} N={N:5d} M=1 {NAME[qt]:6s} {'+'.join(sorted(prod)):24s} {us:8.2f} us  quantise {quant:6.2f} us  launches {launches:.0f}  {W.nbytes / 1e6:6.1f} MB {rate:6.3f} TB/s  "
                f"time x{us / base[0]:.2f}  rate x{rate / base[1]:.2f}{verdict}")
    K, N = BATCH
    say("# batches at K 4096, N 4096: the int8 tile kernel, q4_K's batch launch, and the batch as passes of the 8-column mat-vec (8 columns timed, times ceil(M / 8))")
    for M in (32, 512):
        base = None
        for qt in FORMATS:
            W = weight(qt, K, N, rng)
            prod, quant, launches = timed(be, qt, K, N, M, W, rng, 20)
            us = sum(prod.values())
            if qt == L.Q4_K:
                base = us
                say(f"K={K} N={N} M={M:3d} q4_K   {'+'.join(sorted(prod)):24s} {us:8.2f} us  quantise {quant:6.2f} us  launches {launches:.0f}")
                continue
            p8, _, _ = timed(be, qt, K, N, 8, W, rng, 20)
            passes = sum(p8.values()) * ((M + 7) // 8)
            verdict = "ok" if us <= passes else "KILL (slower than the mat-vec passes)"
            say(f"K={K} N={N} M={M:3d} {NAME[qt]:6s} {'+'.join(sorted(prod)):24s} {us:8.2f} us  quantise {quant:6.2f} us  launches {launches:.0f}  x{us / base:.2f} of q4_K  "
                f"mat-vec passes {passes:9.2f} us ({'+'.join(sorted(p8))})  {verdict}")
    if args.e2e:
        be.set_option("timing", 0)
        be.set_option("graphs", 1)
        say(f"# end to end: batch-1 decode through llm_decode_steps, {args.steps} timed steps after 8, 64-token prompt" + (f", {args.layers} layers" if args.layers else ""))
        for name in ("llama3-8b-q3_k_m", "llama3-8b-q4_k_m"):
            hp = preset(name)
            if args.layers:
                hp.n_layer = args.layers
            if args.vocab:
                hp.n_vocab = args.vocab
            m = Model(hp, 1, be.buft)
            c = Context(m, backend=be, flash_attn=1, n_ctx=512)
            toks = rng.integers(0, hp.n_vocab, 64 + 8 + args.steps).tolist()
            rc, _ = c.decode(toks[:64], range(64), want=[0] * 63 + [1])
            assert rc == 0
            assert c.decode_steps([[t] for t in toks[64:72]], 1, 64) == 0
            be.synchronize()
            t0 = time.perf_counter()
            assert c.decode_steps([[t] for t in toks[72:]], 1, 72) == 0
            be.synchronize()
            dt = time.perf_counter() - t0
            say(f"{name:18s} {m.stream_bytes() / 1e9:6.2f} GB streamed per token  {dt / args.steps * 1e3:7.3f} ms/step  {args.steps / dt:7.1f} tok/s")
            c.free()
            m.free()
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
