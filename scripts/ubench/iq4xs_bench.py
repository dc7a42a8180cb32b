"""MUL_MAT over IQ4_XS weights next to the same shape in Q4_K (block layout, a plain buffer: no decode copy) and in IQ4_NL:

  batch 1     (K 4096, N 14336), (K 14336, N 4096), (K 4096, N 4096): the mat-vec launch, its bytes per second and both as ratios to the Q4_K launch.
              IQ4_XS holds 136 / 144 of Q4_K's bytes and has no mins term: a launch LONGER than Q4_K's is marked `MISSES`.
  batches     32 and 512 columns at the same three shapes: the int8 tile kernel against Q4_K's and IQ4_NL's batch launches, and against the same batch as
              passes of the 8-column mat-vec (measured at 8 columns, times ceil(M / 8)): a tile launch slower than those passes is marked `KILL`.

`python scripts/ubench/iq4xs_bench.py [--out FILE]` prints the hipEvent-bracketed class times of the backend's timing option (graphs off: one class per launch
kind; the activation quantisation is a class of its own and is listed beside the product) on one MI355X.  End to end: `bench.py --preset llama3-8b-iq4_xs` and
`--preset llama3-8b-q4_k_m` in the same session.  For the kernel-trace view run it under
`rocprofv3 --kernel-trace --stats -d DIR -o iq4xs -- python scripts/ubench/iq4xs_bench.py` and read DIR/.../iq4xs_kernel_stats.csv: the rows named k_mmvq*,
k_mmq_i8* and k_quantize* are the launches timed here."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import iq4xs_ref as R  # noqa: E402
import legacy_ref as LR  # noqa: E402
import llama_box_amd as L  # noqa: E402

FORMATS = (L.Q4_K, L.IQ4_NL, L.IQ4_XS)
NAME = {L.Q4_K: "q4_K", L.IQ4_NL: "iq4_nl", L.IQ4_XS: "iq4_xs"}
SHAPES = [(4096, 14336), (14336, 4096), (4096, 4096)]
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def weight(qt, K, N, rng):
    """N rows cut from 64 random ones: the kernels' time does not depend on the values, the host's does on how many it draws."""
    base = T.rand_weight(qt, K, 64, rng) if qt == L.Q4_K else (LR.rand_weight(qt, K, 64, rng) if qt == L.IQ4_NL else R.rand_weight(K, 64, rng))
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    be = L.Backend(0)
    be.set_option("graphs", 0)
    be.set_option("timing", 1)
    rng = np.random.default_rng(0)
    say("# batch 1: us per graph of the product's launches (class), of the activation quantisation beside it, MB of weights, TB/s of the product; ratios to q4_K")
    for K, N in SHAPES:
        base = None
        for qt in FORMATS:
            W = weight(qt, K, N, rng)
            prod, quant, launches = timed(be, qt, K, N, 1, W, rng, 50)
            us = sum(prod.values())
            rate = W.nbytes / us / 1e6
            if qt == L.Q4_K:
                base = (us, rate)
            verdict = "" if qt != L.IQ4_XS else ("  ok" if us <= base[0] else "  MISSES (longer than the q4_K launch)")
            say(f"K={K:5d} N={N:5d} M=1 {NAME[qt]:6s} {'+'.join(sorted(prod)):24s} {us:8.2f} us  quantise {quant:6.2f} us  launches {launches:.0f}  {W.nbytes / 1e6:6.1f} MB {rate:6.3f} TB/s  "
                f"time x{us / base[0]:.2f}  rate x{rate / base[1]:.2f}{verdict}")
    say("# batches: the batch launch per format, and for iq4_xs the batch as passes of the 8-column mat-vec (8 columns timed, times ceil(M / 8))")
    for K, N in SHAPES:
        for M in (32, 512):
            base = None
            for qt in FORMATS:
                W = weight(qt, K, N, rng)
                prod, quant, launches = timed(be, qt, K, N, M, W, rng, 20)
                us = sum(prod.values())
                if qt == L.Q4_K:
                    base = us
                line = f"K={K:5d} N={N:5d} M={M:3d} {NAME[qt]:6s} {'+'.join(sorted(prod)):26s} {us:8.2f} us  quantise {quant:6.2f} us  launches {launches:.0f}  x{us / base:.2f} of q4_K"
                if qt == L.IQ4_XS:
                    p8, _, _ = timed(be, qt, K, N, 8, W, rng, 20)
                    passes = sum(p8.values()) * ((M + 7) // 8)
                    line += f"  mat-vec passes {passes:9.2f} us ({'+'.join(sorted(p8))})  {'ok' if us <= passes else 'KILL (slower than the mat-vec passes)'}"
                say(line)
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
