"""SSM_SCAN and the fused SSM_CONV + bias + SILU launch at model shapes (csrc/ssm.hip): device time per launch and the bytes the op has to move
over that time, as a share of 8 TB/s.

    python scripts/ubench/ssm_bench.py                       every shape, warm and cold: host clock around synchronised windows, then the hipEvent class times
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ssm -- python scripts/ubench/ssm_bench.py SHAPE MODE
                                                             one shape in one mode (warm | cold), no events: kernel times are the trace's (scripts/trace_by_grid.py)

warm: one operand set, launched again and again (a decode state of 2.6 MB stays in the L2 / the 256 MiB Infinity Cache).  cold: `copies` operand sets of more than
512 MiB together, one launch each per graph, so that no launch finds its states in a cache.  Every shape is warmed up before its timed window; a window is at
least a few hundred launches.  Bytes: the states read and written once, x, dt, B, C read and y written once (scan); sx, c, bias read and the result written (conv).
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

PEAK = 8.0e12  # bytes / s
# scan: (d_state, head_dim, n_head, n_group, n_t, n_s, A per state element)
SCAN = {
    "m2-decode-s1": (128, 64, 80, 1, 1, 1, False),
    "m2-decode-s32": (128, 64, 80, 1, 1, 32, False),
    "m2-prompt-512": (128, 64, 80, 1, 512, 1, False),
    "m1-decode-s1": (16, 1, 5120, 1, 1, 1, True),
    "m1-decode-s32": (16, 1, 5120, 1, 1, 32, True),
    "m1-prompt-512": (16, 1, 5120, 1, 512, 1, True),
}
# fused conv: (d_conv, conv_dim, n_t, n_s) — Mamba-2's xBC width at d_inner 5120, one group of 128 states
CONV = {"conv-silu-s1": (4, 5376, 1, 1), "conv-silu-s32": (4, 5376, 1, 32)}


def scan_bytes(d_state, head_dim, n_head, n_group, n_t, n_s, m1):
    rows = head_dim * n_head
    return 4 * (2 * n_s * rows * d_state + 2 * rows * n_t * n_s + n_head * n_t * n_s + 2 * n_group * d_state * n_t * n_s)


def conv_bytes(d_conv, cd, n_t, n_s):
    return 4 * ((d_conv - 1 + n_t) * cd * n_s + d_conv * cd + cd + cd * n_t * n_s)


def build_scan(g, rng, d_state, head_dim, n_head, n_group, n_t, n_s, m1):
    H, f = g.H, np.float32
    s = g.new(L.F32, [d_state, head_dim, n_head, n_s], rng.standard_normal((n_s, n_head, head_dim, d_state)).astype(f))
    x = g.new(L.F32, [head_dim, n_head, n_t, n_s], rng.standard_normal((n_s, n_t, n_head, head_dim)).astype(f))
    dt = g.new(L.F32, [n_head, n_t, n_s], rng.uniform(-3, 3, (n_s, n_t, n_head)).astype(f))
    A = g.new(L.F32, [d_state if m1 else 1, n_head], (-rng.uniform(0.05, 1.5, (n_head, d_state if m1 else 1))).astype(f))
    B, Cc = (g.new(L.F32, [d_state, n_group, n_t, n_s], rng.standard_normal((n_s, n_t, n_group, d_state)).astype(f)) for _ in range(2))
    ids = g.new(L.I32, [n_s], rng.permutation(n_s).astype(np.int32))
    return H.ggml_ssm_scan(g.ctx, s, x, dt, A, B, Cc, ids)


def build_conv(g, rng, d_conv, cd, n_t, n_s):
    H, f = g.H, np.float32
    sx = g.new(L.F32, [d_conv - 1 + n_t, cd, n_s], rng.standard_normal((n_s, cd, d_conv - 1 + n_t)).astype(f))
    c = g.new(L.F32, [d_conv, cd], rng.standard_normal((cd, d_conv)).astype(f))
    b = g.new(L.F32, [cd], rng.standard_normal(cd).astype(f))
    return H.ggml_silu(g.ctx, H.ggml_add(g.ctx, H.ggml_ssm_conv(g.ctx, sx, c), b))


def measure(be, name, mode, events):
    H = L.host()
    scan = name in SCAN
    shape = SCAN[name] if scan else CONV[name]
    nbytes = scan_bytes(*shape) if scan else conv_bytes(*shape)
    copies = 1 if mode == "warm" else max(2, min(256, -(-(512 << 20) // nbytes)))
    reps = max(8, (2000 if nbytes < (64 << 20) else 300) // copies)
    rng = np.random.default_rng(0)
    g = T.G(be)
    try:
        outs = [(build_scan if scan else build_conv)(g, rng, *shape) for _ in range(copies)]
        gf = H.ggml_new_graph_custom(g.ctx, 4096, False)
        for o in outs:
            H.ggml_set_output(o)
            H.ggml_build_forward_expand(gf, o)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        assert g.buf
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        l0 = be.stat("kernel_launches")
        for _ in range(max(3, 40 // copies)):  # warm-up: code objects, clocks
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        per_graph = (be.stat("kernel_launches") - l0) // max(3, 40 // copies)
        assert per_graph == copies, (per_graph, copies)  # one launch an operand set (the conv chain fused)
        t0 = time.perf_counter()
        for _ in range(reps):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        wall_us = (time.perf_counter() - t0) * 1e6 / (reps * copies)
        line = f"{name:15s} {mode:4s} copies={copies:3d} launches={reps * copies:5d} {nbytes / 1e6:8.2f} MB/launch  host clock {wall_us:8.2f} us/launch ({nbytes / wall_us / 1e6 / (PEAK / 1e12) * 100:5.1f} % of 8 TB/s)"
        if events:
            be.set_option("timing", 1)
            be.timing_report(reset=True)
            for _ in range(max(2, reps // 4)):
                assert H.ggml_backend_graph_compute(be.backend, gf) == 0
            be.synchronize()
            for cls, (cnt, ms, _) in sorted(be.timing_report(reset=True).items()):
                if cnt and cls.startswith("ssm_"):
                    us = ms * 1e3 / cnt
                    line += f" | events {cls} n={cnt} {us:8.2f} us ({nbytes / us / 1e6 / (PEAK / 1e12) * 100:5.1f} %)"
            be.set_option("timing", 0)
        print(line, flush=True)
    finally:
        g.free()


def main():
    be = L.Backend(0)
    be.set_option("graphs", 0)
    if len(sys.argv) > 2:
        measure(be, sys.argv[1], sys.argv[2], events=False)
    else:
        for name in list(SCAN) + list(CONV):
            for mode in ("warm", "cold"):
                measure(be, name, mode, events=True)
    be.close()


if __name__ == "__main__":
    main()
