"""GROUP_NORM at Stable Diffusion shapes (csrc/diffusion.hip): device time per node from the backend's hipEvent classes, both forms, alone, with the
`* w`, `+ b` and SILU nodes behind it fused into the writing pass, and as the unfused chain of four nodes.

    python scripts/ubench/diffusion_bench.py          every shape: one child process per shape under its own `timeout`; the run ends at the first child that
                                                      fails or runs out of time
    python scripts/ubench/diffusion_bench.py SHAPE    that one shape in this process

Cases of a shape (32 groups, one batch entry, as every GroupNorm32 of the UNet and the VAE is):
  res          GROUP_NORM alone, gn_form 1: the resident form (only where a group fits MI_GN_RESIDENT_MAX values)
  split        GROUP_NORM alone, gn_form 2: the split form's three launches
  res_fused    GROUP_NORM -> MUL(w) -> ADD(b) -> SILU with fusion on: one launch
  split_fused  ... the same chain in the split form: three launches
  chain        the same chain with fusion off, routed form: the GROUP_NORM's launches, two k_binary launches and one k_unary launch, their device times added up
Every case is measured in WINDOWS windows of `reps` graph computes after a warm-up; a line gives the windows' minimum, median and maximum per node (or chain) and the
spread (max - min) / median: a difference between two forms counts only when it exceeds the spreads beside it.  "of 8 TB/s" is the bytes the node HAS to move (the
tensor read once and written once) over the median time, as a share of the HBM peak; the split form itself reads the tensor three times.  Nothing is flushed between
launches: tensors up to 128 MiB may be served from the 256 MiB Infinity Cache.  Reads nothing outside the tree; inputs come from a seed."""
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
RESIDENT_MAX = 40960  # kernels.h MI_GN_RESIDENT_MAX
SHAPES = {"unet64": (64, 64, 320), "unet32": (32, 32, 640), "unet16": (16, 16, 1280), "unet8": (8, 8, 1280), "vae512": (512, 512, 128), "vae256": (256, 256, 256),
          "vae64": (64, 64, 512)}
N_GROUPS = 32
WINDOWS = 5
CHILD_TIMEOUT_S = 240
# case -> (gn_form, fusion, the chain behind the node?)
CASES = {"res": (1, 1, False), "split": (2, 1, False), "res_fused": (1, 1, True), "split_fused": (2, 1, True), "chain": (0, 0, True)}


def _classes(rep):
    """(device ms, launches-bearing node count) of the GROUP_NORM classes plus, for the unfused chain, binary and unary."""
    ms = sum(v[1] for k, v in rep.items() if k.startswith("group_norm") or k in ("binary", "unary"))
    return ms, {k: v[0] for k, v in rep.items()}


def measure(be, shape):
    H = L.host()
    W, Hh, Cc = SHAPES[shape]
    group = W * Hh * (Cc // N_GROUPS)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, Cc, Hh, W), dtype=np.float32)
    w, b = rng.uniform(0.5, 1.5, Cc).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)
    nbytes = 2.0 * x.nbytes
    for case, (form, fusion, chain) in CASES.items():
        if form == 1 and group > RESIDENT_MAX:
            print(f"{case:11s} {shape:7s} [{W}, {Hh}, {Cc}] group {group:8d}: does not fit the resident form", flush=True)
            continue
        g = T.G(be)
        try:
            node = H.ggml_group_norm(g.ctx, g.new(L.F32, [W, Hh, Cc, 1], x), N_GROUPS, 1e-6)
            if chain:
                node = H.ggml_mul(g.ctx, node, g.new(L.F32, [1, 1, Cc, 1], w))
                node = H.ggml_add(g.ctx, node, g.new(L.F32, [1, 1, Cc, 1], b))
                node = H.ggml_silu(g.ctx, node)
            gf = H.ggml_new_graph_custom(g.ctx, 64, False)
            H.ggml_set_output(node)
            H.ggml_build_forward_expand(gf, node)
            for i in range(gf.contents.n_nodes):
                assert H.ggml_backend_dev_supports_op(be.dev, gf.contents.nodes[i]), i
            g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
            assert g.buf
            for t, raw in g.inputs:
                H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
            be.set_option("gn_form", form)
            be.set_option("fusion", fusion)
            be.set_option("timing", 1)
            k0 = be.stat("kernel_launches")
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
            be.synchronize()
            launches = be.stat("kernel_launches") - k0
            be.timing_report(reset=True)
            for _ in range(3):  # a first window sizes the others: about 0.1 s of device time each, 3 .. 300 computes
                assert H.ggml_backend_graph_compute(be.backend, gf) == 0
            be.synchronize()
            ms0, counts = _classes(be.timing_report(reset=True))
            reps = int(max(3, min(300, 1e5 / max(ms0 * 1e3 / 3, 1.0))))
            times = []
            for _ in range(WINDOWS):
                for _ in range(reps):
                    assert H.ggml_backend_graph_compute(be.backend, gf) == 0
                be.synchronize()
                ms, _ = _classes(be.timing_report(reset=True))
                times.append(ms * 1e3 / reps)
            times.sort()
            lo, med, hi = times[0], times[len(times) // 2], times[-1]
            print(f"{case:11s} {shape:7s} [{W}, {Hh}, {Cc}] group {group:8d}  launches {launches}  {WINDOWS} x {reps:3d} computes: min {lo:9.2f}  median {med:9.2f}  max {hi:9.2f} us  "
                  f"spread {(hi - lo) / med * 100:5.1f} %  {nbytes / (med * 1e-6) / 1e9:8.1f} GB/s = {nbytes / (med * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s  classes {sorted(counts)}", flush=True)
        finally:
            be.set_option("timing", 0)
            be.set_option("fusion", 1)
            be.set_option("gn_form", 0)
            g.free()


def main():
    if len(sys.argv) == 2:
        be = L.Backend(0)
        be.set_option("graphs", 0)
        measure(be, sys.argv[1])
        be.close()
        return 0
    for shape in SHAPES:
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), shape]).returncode
        if rc != 0:
            print(f"{shape}: exit status {rc}; stopping here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
