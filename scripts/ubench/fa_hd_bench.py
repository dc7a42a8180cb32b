"""FLASH_ATTN_EXT at head sizes 72 / 80 / 88 / 112 (csrc/fattn_hd.hip): device time of single attention nodes from the backend's hipEvent classes.

    python scripts/ubench/fa_hd_bench.py [--out FILE]     every case: one child process per case under its own `timeout` (the forced rows need an environment
                                                          variable the backend reads once); the run ends at the first child that fails or runs out of time
    python scripts/ubench/fa_hd_bench.py CASE             that one case in this process: prints its JSON line

Shapes: a decoder layer (32 / 32 heads, f16 cache, 2048 cells, causal mask at the end of the context) at 80 and 112; a vision tower (16 / 16 heads, no mask, as many
cells as tokens, K / V contiguous per head and Q permuted, as clip builds them) at 72 / 80 / 88.  Per shape: one token; a batch (512 tokens, towers 1024) on the
padded matrix-core form; the same batch forced onto the split kernel (GGML_MI355X_FA_MMA_MIN_Q=1000; 2000 for a tower's 1024 tokens); the non-flash chain MUL_MAT K.q -> SOFT_MAX -> MUL_MAT V^T.p
(+ the permuting copy) for the same attention on the same build — the only GPU path these models had before; towers also 729 x 729, which keeps the split kernel
(n_kv % 4 != 0).  Every launch is bracketed by hipEvents (backend option timing=1, eager launches): 3 warm-up + 20 timed graph runs per case; us per node by class.
A chain node the backend refuses makes the row UNMEASURED and names the op.  Reads nothing outside the tree; inputs come from a seed."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fa_hd as FH  # noqa: E402
import harness as T  # noqa: E402
import llama_box_amd as L  # noqa: E402

WARM, RUNS = 3, 20
CHILD_TIMEOUT_S = 120


def _cases():
    out = {}
    for D in (80, 112):
        for nq in (1, 512):
            out[f"decoder D={D} flash nq={nq}"] = dict(D=D, shape="decoder", nq=nq, nkv=2048, kind="flash")
            out[f"decoder D={D} non-flash chain nq={nq}"] = dict(D=D, shape="decoder", nq=nq, nkv=2048, kind="chain")
        out[f"decoder D={D} flash nq=512 forced onto the split kernel"] = dict(D=D, shape="decoder", nq=512, nkv=2048, kind="flash", forced=1000)
    for D in (72, 80, 88):
        for nq, nkv in ((1, 1024), (1024, 1024), (729, 729)):
            out[f"tower D={D} flash nq={nq} nkv={nkv}"] = dict(D=D, shape="tower", nq=nq, nkv=nkv, kind="flash")
            out[f"tower D={D} non-flash chain nq={nq} nkv={nkv}"] = dict(D=D, shape="tower", nq=nq, nkv=nkv, kind="chain")
        out[f"tower D={D} flash nq=1024 nkv=1024 forced onto the split kernel"] = dict(D=D, shape="tower", nq=1024, nkv=1024, kind="flash", forced=2000)
    return out


CASES = _cases()


def _graph(g, H, c):
    """-> the output node of the case's attention."""
    D, nq, nkv = c["D"], c["nq"], c["nkv"]
    NH = NKV = 32 if c["shape"] == "decoder" else 16
    rng = np.random.default_rng(D * 1000 + nq)
    q = rng.standard_normal((nq, NH, D)).astype(np.float32)
    kx = rng.standard_normal((NKV, nkv, D)).astype(np.float16)
    vx = rng.standard_normal((NKV, nkv, D)).astype(np.float16)
    scale = 1.0 / np.sqrt(D)
    tq = H.ggml_permute(g.ctx, g.new(L.F32, [D, NH, nq], q), 0, 2, 1, 3)  # [D, nq, NH]: llama.cpp's and clip's query
    causal = None
    if c["shape"] == "decoder":  # token t of the batch sits at the end of the context: it sees cells 0 .. nkv - nq + t
        MR = (nq + 63) // 64 * 64
        causal = np.full((MR, nkv), -np.inf, np.float32)
        for t in range(nq):
            causal[t, : nkv - nq + t + 1] = 0
    if c["kind"] == "flash":
        if c["shape"] == "decoder":  # views into the cache: a cell's heads side by side
            kc = g.new(L.F16, [NKV * D, nkv], np.ascontiguousarray(kx.transpose(1, 0, 2)))
            vc = g.new(L.F16, [NKV * D, nkv], np.ascontiguousarray(vx.transpose(1, 0, 2)))
            k = H.ggml_view_3d(g.ctx, kc, D, nkv, NKV, NKV * D * 2, D * 2, 0)
            v = H.ggml_view_3d(g.ctx, vc, D, nkv, NKV, NKV * D * 2, D * 2, 0)
        else:
            k, v = g.new(L.F16, [D, nkv, NKV], kx), g.new(L.F16, [D, nkv, NKV], vx)
        m = g.new(L.F16, [nkv, causal.shape[0]], causal.astype(np.float16)) if causal is not None else None
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, scale, 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r
    # the non-flash chain as llama.cpp / clip build it: K [D, nkv, NKV], V transposed [nkv, D, NKV], an f32 mask (clip: none)
    k = g.new(L.F16, [D, nkv, NKV], kx)
    vt = g.new(L.F16, [nkv, D, NKV], np.ascontiguousarray(vx.transpose(0, 2, 1)))
    kq = H.ggml_mul_mat(g.ctx, k, tq)
    m = g.new(L.F32, [nkv, causal.shape[0]], causal) if causal is not None else None
    sm = H.ggml_soft_max_ext(g.ctx, kq, m, float(scale), 0.0)
    kqv = H.ggml_mul_mat(g.ctx, vt, sm)
    return H.ggml_cont_2d(g.ctx, H.ggml_permute(g.ctx, kqv, 0, 2, 1, 3), D * NH, nq)


def measure(name):
    c = CASES[name]
    be = L.Backend(0)
    be.set_option("graphs", 0)
    H = L.host()
    g = T.G(be)
    row = {"case": name}
    try:
        node = _graph(g, H, c)
        gf = H.ggml_new_graph_custom(g.ctx, 64, False)
        H.ggml_set_output(node)
        H.ggml_build_forward_expand(gf, node)
        refused = [H.ggml_op_name(gf.contents.nodes[i].contents.op).decode() for i in range(gf.contents.n_nodes) if not H.ggml_backend_dev_supports_op(be.dev, gf.contents.nodes[i])]
        if refused:
            row.update(us_total="UNMEASURED", refused=refused)
            return row
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, be.buft)
        assert g.buf
        for t, raw in g.inputs:
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        be.set_option("timing", 1)
        for _ in range(WARM):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        be.timing_report(reset=True)
        for _ in range(RUNS):
            assert H.ggml_backend_graph_compute(be.backend, gf) == 0
        be.synchronize()
        rep = be.timing_report(reset=True)
        by = {cls: round(ms * 1e3 / RUNS, 2) for cls, (cnt, ms, _) in sorted(rep.items()) if cnt}
        form = int(be.stat("fa_form"))
        row.update(us_per_node_by_class=by, us_total=round(sum(by.values()), 2), fa_form=form, form=FH.form_name(form) if form else "-")
        be.set_option("timing", 0)
        return row
    finally:
        g.free()
        be.close()


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        args = [a for i, a in enumerate(args) if a != "--out" and (i == 0 or args[i - 1] != "--out")]
    if args:
        print(json.dumps(measure(args[0])), flush=True)
        return 0
    lines = ["# FLASH_ATTN_EXT at head sizes 72 / 80 / 88 / 112: single attention nodes, MI355X.  us per node by kernel class: hipEvents around every launch (backend option",
             f"# timing=1), {WARM} warm-up + {RUNS} timed graph runs per case, eager launches, one process per case.  decoder: 32/32 heads, f16 cache, 2048 cells, causal mask at the end",
             "# of the context; tower: 16/16 heads, no mask, K / V contiguous per head.  The forced rows ran with GGML_MI355X_FA_MMA_MIN_Q=1000 (towers: 2000).  The non-flash chain (MUL_MAT K.q ->",
             "# SOFT_MAX -> MUL_MAT V^T.p -> permuting copy) is the only GPU path such a model had before."]
    for name, c in CASES.items():
        env = dict(os.environ)
        if c.get("forced"):
            env["GGML_MI355X_FA_MMA_MIN_Q"] = str(c["forced"])
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"# {name}: exit status {r.returncode}; stopped here — the remaining cases are UNMEASURED")
            print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
            break
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0 if not lines[-1].startswith("#") else 1


if __name__ == "__main__":
    sys.exit(main())
