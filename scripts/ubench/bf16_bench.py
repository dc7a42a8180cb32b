"""MUL_MAT over bf16 weights at the Llama-3-8B shapes, every candidate form of csrc/mmbf.hip per batch width, next to three yardsticks that are not the code under
test: the same shape as F16 through the existing launch_mul_mat_f (what a 16-bit matrix gets today), the same shape as Q8_0 through its own kernels scaled by bytes,
and bytes / 8 TB/s.

  shapes      (K 4096, N 4096), (4096, 1024), (4096, 14336), (14336, 4096), (4096, 128256)
  batches     M = 1, 2, 4, 8, 9, 16, 64, 512, 2048
  candidates  option bf16_form: the dot kernel (M <= 9), the streaming mat-vec in chunks of <= 8 columns (M <= 16), 16 x 16 tiles, 32 x 32 tiles (M >= 2), the 32 x 32 tiles over src1 rounded
              to bf16 once into scratch (option bf16_preround, M >= 64); at M = 1 the
              streaming kernel with and without non-temporal loads (back-to-back replays of ONE launch: the load policy is decided by the end-to-end lines, not here)
  --e2e       llama3-8b-bf16 through llm_decode_steps: batch-1 tokens/s with bf16_nt on and off, a 2048-token prefill, and -np 32 steps

`python scripts/ubench/bf16_bench.py [--e2e] [--layers L] [--vocab V] [--shapes i,j] [--out FILE]` prints the hipEvent-bracketed class times of the backend's timing option
(graphs off).  The routing condition of DESIGN.md 4f is checkable from the output: at every M = 1 shape the streaming kernel must be no slower than the dot kernel
(lines marked `MISSES` otherwise), and a hand-over sits where the faster candidate changes."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bf16_ref as B  # noqa: E402
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402
from model_util import Context, Model, preset  # noqa: E402

SHAPES = [(4096, 4096), (4096, 1024), (4096, 14336), (14336, 4096), (4096, 128256)]
BATCHES = (1, 2, 4, 8, 9, 16, 64, 512, 2048)
FORMS = {"dot": 0, "mmv": 1, "mma16": 3, "mma": 4}
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def weight(qt, K, N, rng):
    """N rows cut from 64 random ones: the kernels' time does not depend on the values, the host's does on how many it draws."""
    base = B.rand_weight(K, 64, rng) if qt == L.BF16 else T.rand_weight(qt, K, 64, rng)
    return np.ascontiguousarray(np.tile(base, ((N + 63) // 64, 1))[:N])


class Case:
    """one weight matrix on the device and one activation batch per M, graphs built on demand"""

    def __init__(self, be, qt, K, N, rng):
        self.be, self.qt, self.K, self.N = be, qt, K, N
        self.W = weight(qt, K, N, rng)
        self.rng = rng

    def timed(self, M, reps, prefixes):
        """-> ({class: us per graph} of the classes that start with one of `prefixes`, launches per graph)"""
        H, be = L.host(), self.be
        X = self.rng.standard_normal((M, self.K)).astype(np.float32)
        g = T.G(be)
        try:
            out = H.ggml_mul_mat(g.ctx, g.new(self.qt, [self.K, self.N], self.W), g.new(L.F32, [self.K, M], X))
            gf = H.ggml_new_graph_custom(g.ctx, 64, False)
            H.ggml_set_output(out)
            H.ggml_build_forward_expand(gf, out)
            g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
            assert g.buf
            for t, raw in g.inputs:
                H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            for _ in range(2):
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
        return {c: ms * 1e3 / reps for c, (n, ms, _) in rep.items() if n and c.startswith(prefixes)}, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-micro", action="store_true")
    ap.add_argument("--layers", type=int, default=0, help="layers of the end-to-end model (0: all 32)")
    ap.add_argument("--vocab", type=int, default=0, help="vocabulary rows of the end-to-end model (0: all 128256)")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--shapes", default="", help="comma-separated indices into the shape list (default: all)")
    ap.add_argument("--max-m", type=int, default=2048)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    be = L.Backend(0)
    be.set_option("graphs", 0)
    rng = np.random.default_rng(0)
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else SHAPES
    if not args.no_micro:
        be.set_option("timing", 1)
        say("# us per graph of the product's launches; bf16 candidates by option bf16_form, then the yardsticks: f16 (launch_mul_mat_f), q8_0 (its kernels + the activation "
            "quantisation beside them, and the product scaled by bf16 / q8_0 bytes), bytes / 8 TB/s")
        for K, N in shapes:
            cb, cf, cq = Case(be, L.BF16, K, N, rng), Case(be, L.F16, K, N, rng), Case(be, L.Q8_0, K, N, rng)
            floor = cb.W.nbytes / 8e12 * 1e6
            for M in [m for m in BATCHES if m <= args.max_m]:
                reps = 20 if M <= 16 else (5 if M <= 512 else 3)
                cand = {}
                for name, form in FORMS.items():
                    if (name == "dot" and M > 9) or (name == "mmv" and M > 16) or (name in ("mma16", "mma") and M < 2):
                        continue
                    be.set_option("bf16_form", form)
                    be.set_option("bf16_preround", 0)  # ("mma": src1 converted in the loop; "mma_pre" below is what the backend runs from 64 columns on)
                    prod, _ = cb.timed(M, reps, ("mmv_bf16", "mul_mat_bf16"))
                    be.set_option("bf16_preround", 1)
                    cand[name + "[" + "+".join(sorted(prod)) + "]"] = sum(prod.values())
                if M >= 64:  # the 32 x 32 tiles over src1 rounded to bf16 once into scratch (the rounding launch is part of the class's time)
                    be.set_option("bf16_form", 4)
                    be.set_option("bf16_preround", 1)
                    prod, _ = cb.timed(M, reps, ("mul_mat_bf16",))
                    cand["mma_pre[" + "+".join(sorted(prod)) + "]"] = sum(prod.values())
                if M == 1:
                    be.set_option("bf16_form", 1)
                    be.set_option("bf16_nt", 0)
                    prod, _ = cb.timed(M, reps, ("mmv_bf16",))
                    cand["mmv_nt0[" + "+".join(sorted(prod)) + "]"] = sum(prod.values())
                    be.set_option("bf16_nt", 1)
                be.set_option("bf16_form", -1)
                routed, _ = cb.timed(M, reps, ("mmv_bf16", "mul_mat_bf16"))
                f16, _ = cf.timed(M, reps, ("mul_mat_f",))
                q80, _ = cq.timed(M, reps, ("mmvq", "mmq", "quantize"))
                q_prod = sum(v for c, v in q80.items() if not c.startswith("quantize"))
                q_quant = sum(v for c, v in q80.items() if c.startswith("quantize"))
                best = min(cand, key=cand.get)
                note = ""
                if M == 1:
                    dot = [v for c, v in cand.items() if c.startswith("dot")][0]
                    mmv = [v for c, v in cand.items() if c.startswith("mmv[")][0]
                    note = "  ok (streaming <= dot)" if mmv <= dot else "  MISSES (the streaming kernel is slower than the dot kernel)"
                say(f"K={K:5d} N={N:6d} M={M:4d} " + "  ".join(f"{c} {v:9.2f}" for c, v in cand.items()) + f"  | routed {'+'.join(sorted(routed))} {sum(routed.values()):9.2f}  best {best.split('[')[0]}"
                    f"  | f16 {sum(f16.values()):9.2f}  q8_0 {q_prod:9.2f} (+ quantise {q_quant:6.2f}; x bytes {q_prod * cb.W.nbytes / cq.W.nbytes:9.2f})  floor {floor:8.2f}"
                    f"  | {cb.W.nbytes / 1e6:7.1f} MB, routed {cb.W.nbytes / max(sum(routed.values()), 1e-9) / 1e6:6.3f} TB/s{note}")
            del cb, cf, cq
        be.set_option("timing", 0)
    if args.e2e:
        be.set_option("graphs", 1)
        hp = preset("llama3-8b-bf16")
        if args.layers:
            hp.n_layer = args.layers
        if args.vocab:
            hp.n_vocab = args.vocab
        say(f"# end to end: llama3-8b-bf16 ({hp.n_layer} layers, {hp.n_vocab} vocabulary rows) through llm_decode / llm_decode_steps, flash attention on")
        m = Model(hp, 1, be.buft)
        say(f"{m.stream_bytes() / 1e9:6.2f} GB streamed per token")
        toks = rng.integers(0, hp.n_vocab, 4096).tolist()
        for nt in (1, 0, 1, 0):
            be.set_option("bf16_nt", nt)
            c = Context(m, backend=be, flash_attn=1, n_ctx=512)
            rc, _ = c.decode(toks[:64], range(64), want=[0] * 63 + [1])
            assert rc == 0
            assert c.decode_steps([[t] for t in toks[64:72]], 1, 64) == 0
            be.synchronize()
            t0 = time.perf_counter()
            assert c.decode_steps([[t] for t in toks[72:72 + args.steps]], 1, 72) == 0
            be.synchronize()
            dt = time.perf_counter() - t0
            say(f"batch-1 decode bf16_nt={nt}: {dt / args.steps * 1e3:7.3f} ms/step  {args.steps / dt:7.1f} tok/s  {m.stream_bytes() / (dt / args.steps) / 1e12:5.2f} TB/s")
            c.free()
        be.set_option("bf16_nt", 1)
        c = Context(m, backend=be, flash_attn=1, n_ctx=4096, n_ubatch=512)
        for rnd in range(2):
            c.clear()
            be.synchronize()
            t0 = time.perf_counter()
            rc, _ = c.decode(toks[:2048], range(2048), want=[0] * 2047 + [1])
            be.synchronize()
            dt = time.perf_counter() - t0
            assert rc == 0
            say(f"2048-token prefill (n_ubatch 512), run {rnd}: {dt * 1e3:8.2f} ms  {2048 / dt:8.1f} tok/s")
        c.free()
        c = Context(m, backend=be, flash_attn=1, n_ctx=32 * 128)
        seq = [s for s in range(32) for _ in range(16)]
        pos = [p for _ in range(32) for p in range(16)]
        rc, _ = c.decode(toks[:512], pos, seq=seq, want=[0] * 511 + [1])
        assert rc == 0
        assert c.decode_steps([toks[600 + 32 * i:632 + 32 * i] for i in range(4)], 32, 16) == 0
        be.synchronize()
        n = 16
        t0 = time.perf_counter()
        assert c.decode_steps([toks[1000 + 32 * i:1032 + 32 * i] for i in range(n)], 32, 20) == 0
        be.synchronize()
        dt = time.perf_counter() - t0
        say(f"-np 32 decode: {dt / n * 1e3:7.3f} ms/step  {32 * n / dt:8.1f} tok/s")
        c.free()
        m.free()
    be.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
