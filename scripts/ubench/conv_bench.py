"""IM2COL and the f16 x f16 MUL_MAT behind it at tower shapes (csrc/conv.hip): device time per launch from the backend's hipEvent classes.

    python scripts/ubench/conv_bench.py              every case: one child process per (case, shape) under its own `timeout`; the run ends at the first child that
                                                     fails or runs out of time
    python scripts/ubench/conv_bench.py CASE SHAPE   that one case in this process

Cases:
  im2col    the f16 IM2COL launch of a 14 x 14 x 3 patch embedding: us, and bytes moved (the f32 image read once, the f16 patch matrix written once) against 8 TB/s
  mma       MUL_MAT f16 x f16 [K, patches] x [K, outputs] with conv_mma 2: the matrix-core form whatever the shape
  dot       the same node with conv_mma 0: the dot form
  ref_f32   the yardstick that is NOT under test: the f16 x f32 product the backend has always served (mmf.hip's 32 x 32 tiles), at K = 592 — the nearest K its
            16-byte loads can take — and otherwise the same extents
Every case is measured in WINDOWS windows of `reps` launches after a warm-up; a line gives the windows' minimum, median and maximum and the spread (max - min) /
median: a difference between two forms counts only when it exceeds the spreads beside it.  The operands of a shape (19 MB + 1.5 MB in, 84 MB out at the largest) pass
through the 4 MB L2 but not out of the 256 MiB Infinity Cache between launches; nothing is flushed.  Reads nothing outside the tree; inputs come from a seed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402

PEAK = 8.0e12  # bytes / s
# (patch grid w, h, outputs): 16 384 and 729 patches of K = 588 at model widths, then the small end, where the routed threshold (MI_CONV_MMA_MIN_TILES result tiles of
# 32 x 32) lies: 2, 16, 32 and 64 tiles
SHAPES = {"qwen2vl": (128, 128, 1280), "siglip": (27, 27, 1152), "t2": (8, 8, 32), "t16": (8, 8, 256), "t32": (16, 8, 256), "t64": (16, 16, 256)}
CASES = {"im2col": "im2col", "mma": "mul_mat_f16x_mma", "dot": "mul_mat_f16x_dot", "ref_f32": "mul_mat_f"}  # the backend's timing class
WINDOWS = 5
CHILD_TIMEOUT_S = 150


def measure(be, case, shape):
    H = L.host()
    pw, ph, n_out = SHAPES[shape]
    n_patch, K = pw * ph, 588
    rng = np.random.default_rng(0)
    g = T.G(be)
    try:
        if case == "im2col":
            img = g.new(L.F32, [14 * pw, 14 * ph, 3, 1], rng.standard_normal((1, 3, 14 * ph, 14 * pw)).astype(np.float32))
            node = H.ggml_im2col(g.ctx, g.new(L.F16, [14, 14, 3, n_out]), img, 14, 14, 0, 0, 1, 1, True, L.F16)
            work, unit = 4 * 588 * n_patch + 2 * 588 * n_patch, "GB/s"
        else:
            if case == "ref_f32":
                K = 592
            a = g.new(L.F16, [K, n_patch], rng.standard_normal((n_patch, K)).astype(np.float16))
            bt = L.F32 if case == "ref_f32" else L.F16
            b = g.new(bt, [K, n_out], rng.standard_normal((n_out, K)).astype(np.float32 if case == "ref_f32" else np.float16))
            node = H.ggml_mul_mat(g.ctx, a, b)
            work, unit = 2.0 * K * n_patch * n_out, "TFLOP/s"
        gf = H.ggml_new_graph_custom(g.ctx, 64, False)
        H.ggml_set_output(node)
        H.ggml_build_forward_expand(gf, node)
        assert H.ggml_backend_dev_supports_op(be.dev, node)
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        assert g.buf
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        be.set_option("conv_mma", 0 if case == "dot" else 2)
        be.set_option("timing", 1)
        # a first launch sizes the windows: about 0.2 s of device time each, 3 .. 200 launches
        assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        be.timing_report(reset=True)
        for _ in range(3):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        rep = be.timing_report(reset=True)
        assert CASES[case] in rep and rep[CASES[case]][0] == 3, (case, rep)
        us0 = rep[CASES[case]][1] * 1e3 / 3
        reps = int(max(3, min(200, 2e5 / max(us0, 1.0))))
        times = []
        for _ in range(WINDOWS):
            for _ in range(reps):
                assert H.ggml_backend_graph_compute(be.backend, gf) == 0
            be.synchronize()
            cnt, ms, _ = be.timing_report(reset=True)[CASES[case]]
            assert cnt == reps
            times.append(ms * 1e3 / cnt)
        times.sort()
        lo, med, hi = times[0], times[len(times) // 2], times[-1]
        rate = work / (med * 1e-6)
        share = f" = {rate / PEAK * 100:5.1f} % of 8 TB/s" if unit == "GB/s" else ""
        print(f"{case:8s} {shape:8s} patches {n_patch:6d} K {K:4d} outputs {n_out:5d}  {WINDOWS} x {reps:3d} launches: min {lo:10.2f}  median {med:10.2f}  max {hi:10.2f} us  "
              f"spread {(hi - lo) / med * 100:5.1f} %  {rate / (1e9 if unit == 'GB/s' else 1e12):8.2f} {unit}{share}", flush=True)
        be.set_option("timing", 0)
        be.set_option("conv_mma", 1)
    finally:
        g.free()


def main():
    if len(sys.argv) == 3:
        be = L.Backend(0)
        be.set_option("graphs", 0)
        measure(be, sys.argv[1], sys.argv[2])
        be.close()
        return 0
    for shape in SHAPES:
        for case in CASES:
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), case, shape]).returncode
            if rc != 0:
                print(f"{case} {shape}: exit status {rc}; stopping here", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
