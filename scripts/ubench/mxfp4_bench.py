"""One MUL_MAT_ID -> ADD_ID pair at gpt-oss expert shapes (K = N = 2880; 32 and 128 experts, 4 used; 1 / 8 / 32 tokens) over MXFP4 experts and, in the same run,
over IQ4_NL experts of the same shape (17 against 18 bytes a block: the nearest format with the same lane mapping), with the bias in the MUL_MAT_ID store
(mmid_bias 1) and as a launch of its own (mmid_bias 0).  Prints the hipEvent-bracketed class times of the backend's timing option, three back-to-back loops a configuration (one process, one allocation: loop-to-loop
spread, not process-to-process),
and the MXFP4 : IQ4_NL launch-time ratio next to the byte ratio 17 / 18.  `python scripts/ubench/mxfp4_bench.py > profiles/mxfp4_ubench.txt`"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402

K = N = 2880
N_USED = 4
TYPES = {"mxfp4": L.MXFP4, "iq4_nl": L.IQ4_NL}


def experts(qtype, n_expert, rng):
    """random code bytes under a fixed sane scale (the kernels' time does not depend on the values): [n_expert, N, row bytes]"""
    bs = L.TYPE_SIZE[qtype]
    raw = rng.integers(0, 256, (n_expert * N * (K // 32), bs), dtype=np.uint8)
    if qtype == L.MXFP4:
        raw[:, 0] = 120
    else:
        raw[:, 0:2] = np.array([2e-4], np.float16).view(np.uint8)
    return raw.reshape(n_expert, N, (K // 32) * bs)


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
        times = []
        for _ in range(3):
            be.timing_report(reset=True)
            for _ in range(reps):
                assert H.ggml_backend_graph_compute(be.backend, gf) == 0
            be.synchronize()
            rep = be.timing_report(reset=True)
            times.append({cls: ms * 1e3 / cnt for cls, (cnt, ms, _) in rep.items() if cnt and (cls.startswith("mmid") or cls == "add_id" or cls == "quantize_act")})
        return times
    finally:
        g.free()


def main():
    be = L.Backend(0)
    be.set_option("graphs", 0)
    be.set_option("timing", 1)
    H = L.host()
    rng = np.random.default_rng(0)
    med = {}
    for n_expert in (32, 128):
        W = {t: experts(q, n_expert, rng) for t, q in TYPES.items()}
        bias = rng.standard_normal((n_expert, N)).astype(np.float32)
        for n_tok in (1, 8, 32):
            ids = np.stack([rng.permutation(n_expert)[:N_USED] for _ in range(n_tok)]).astype(np.int32)
            full = np.zeros((n_tok, n_expert), dtype=np.int32)
            full[:, :N_USED] = ids
            b = rng.standard_normal((n_tok, 1, K)).astype(np.float32)
            for tname, qtype in TYPES.items():
                nbytes = N_USED * n_tok * N * (K // 32) * L.TYPE_SIZE[qtype]
                for bias_on in (1, 0):
                    be.set_option("mmid_bias", bias_on)

                    def pair(g):
                        as_t = g.new(qtype, [K, N, n_expert], W[tname])
                        idt = H.ggml_view_2d(g.ctx, g.new(L.I32, [n_expert, n_tok], full), N_USED, n_tok, n_expert * 4, 0)
                        mm = H.ggml_mul_mat_id(g.ctx, as_t, g.new(L.F32, [K, 1, n_tok], b), idt)
                        return H.ggml_add_id(g.ctx, mm, g.new(L.F32, [N, n_expert], bias), idt)

                    times = run(be, pair, 50 if n_tok == 1 else 20)
                    mm = sorted(t[f"mmid_{tname}"] for t in times)
                    ad = sorted(t.get("add_id", 0.0) for t in times)
                    med[(n_expert, n_tok, tname, bias_on)] = mm[1]
                    print(f"experts={n_expert:3d} n_tokens={n_tok:2d} {tname:6s} mmid_bias={bias_on} mmid {mm[0]:7.2f} {mm[1]:7.2f} {mm[2]:7.2f} us/launch (3 loops, sorted)  add_id {ad[1]:5.2f} us  "
                          f"{nbytes / 1e6:7.1f} MB {nbytes / mm[1] / 1e6:6.3f} TB/s", flush=True)
    be.set_option("mmid_bias", 1)
    print(f"byte ratio mxfp4 : iq4_nl = {17 / 18:.3f}")
    for n_expert in (32, 128):
        for n_tok in (1, 8, 32):
            for bias_on in (1, 0):
                r = med[(n_expert, n_tok, "mxfp4", bias_on)] / med[(n_expert, n_tok, "iq4_nl", bias_on)]
                print(f"experts={n_expert:3d} n_tokens={n_tok:2d} mmid_bias={bias_on} launch-time ratio mxfp4 : iq4_nl (medians) = {r:.3f}")
    be.close()


if __name__ == "__main__":
    main()
