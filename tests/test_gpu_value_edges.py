"""GPU: exact read-back of the on-device activation quantisers, and the Q8_0 cache writers on edge values.

(a) MUL_MAT(read-out weight, edge rows) — tests/probes.py: output (m, j) = d_act * q_act[j], one non-zero term, so the f32 result is
    the same bits whatever the summation order, tiling, K split or MFMA shape.  Gate, everywhere in (a): got == oracle == NumPy twin as
    uint32 (+-0 equal, NaN where the oracle has NaN).  Every case switches `timing` on and asserts the kernel classes / counters of the
    route it means to take.

    quantiser site                                               reached by
    k_quantize_q8_K -> k_mmvq<T, NC>                             test_standalone_quantiser_then_mat_vec
    k_quantize_q8_0<false> -> k_mmvq<Q8_0, NC>, 16/32-col pass   test_standalone_quantiser_then_mat_vec, test_q8_0_batch_routes[wide_mat_vec-*]
    k_mmvq / k_mmvq_stream f32 prologue (block layout, copy)     test_batch1_prologues[f32pro-*]
    k_mmvq / k_mmvq_stream RMS_NORM prologue                     test_batch1_prologues[normpro-*]
    k_swiglu_q8_K                                                test_k_quant_batch_routes[swiglu-*]
    k_rms_norm_mul_q8_K<false> -> skinny / tiled / f16 GEMM      test_k_quant_batch_routes[norm-*]
    k_quantize_q8_K -> k_mmq_wide                                test_k_quant_wide_form
    k_quantize_q8_0<PANEL> -> k_mmq_q80_skinny                   test_q8_0_batch_routes[skinny-*]
    k_quantize_q8_0 -> k_mmq_q80 (block and panel order)         test_q8_0_batch_routes[gemm-*]
    Q8_0 panel producers after RMS_NORM and SwiGLU (ops.hip)     test_q8_0_batch_routes[norm_panel-*], [swiglu_panel-*]

    attention -> wo: fa_wo prologue (flash_attn_fat + attnpro)   test_attention_hands_its_result_to_wo_quantised[fa_wo_prologue-*]
    attention -> wo: Q8_K blocks from the single pass / combine  test_attention_hands_its_result_to_wo_quantised[q8out_single_pass-*], [q8out_combine-*]
    per-block indexing over six super-blocks (K = 1536)          test_block_indexing_over_six_super_blocks
    launch_quantize_act on a 3-D b -> k_mmid (MUL_MAT_ID)        tests/test_gpu_moe_edges.py: test_quantiser_read_back_through_mul_mat_id
    (k_mmq_wide serves Q4_K / Q5_K only — mmq_skinny.hip — hence no Q6_K case of test_k_quant_wide_form.)

    Left out, with the reason (two routes):
      * k_rms_norm_mul_q8_K<true> (rows assembled from split-K partial products) and the GLU mat-vec's own prologue: the quantiser's input is there the
        OUTPUT of another kernel in the same launch chain (a split-K mat-mul; silu(gate) * up whose expf differs by an ulp between libm and the device),
        so no chosen edge row reaches it exactly.  Both call dev_util.h wave_quantize_q8_K, which every K-quant case above runs.

    What no read-out can see: a device Q8_K quantiser that took the LAST maximum on a tie for max|x|.  The tied elements differ in sign only, so iscale,
    every quant and d flip sign together and d * q, d * bsums are the same bits (tests/test_readout_probes.py proves it): the stored block's sign convention
    is unobservable through a mat-mul, and equally harmless to one.

(b) The Q8_0 cache writers — SET_ROWS (2-D, 3-D with a broadcast index), CPY f32 -> Q8_0 and the cast back, the fused Q/K/V store —
    byte-exact against the oracle on the Q8_0 edge catalogue.  One exception inside a block: where the block's scale d is zero although
    values are not (f32 subnormals: 1 / d overflows to inf), the reference converts inf / NaN to int8 — undefined in C, and multiplied by
    d = 0 afterwards; there the scale bytes are compared and the quants are not.  The mask is computed from the inputs (q80_dead) and every test asserts
    that it holds exactly the one block the catalogue plants for it.
    The 8-bit query of the in-place decode attention cannot be observed from outside: test_q8_0_query_rows_from_the_catalogue keeps
    test_flash_attn_q8_0_kv's NMSE <= 1e-6 gate.

(c) Weight-value edges (test_weight_value_edges): see its docstring for the cases and the gate pair.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import harness as T
import llama_box_amd as L
import probes as P

pytestmark = pytest.mark.gpu

QNAME = {L.Q4_K: "q4_K", L.Q5_K: "q5_K", L.Q6_K: "q6_K", L.Q8_0: "q8_0"}
QTYPES = [L.Q4_K, L.Q5_K, L.Q6_K, L.Q8_0]
DEFAULTS = {"fa_wo": 0, "fa_splits": 0, "fusion": 1, "prologue": 1, "mmq_min_cols": 3, "mmq_i8": 1, "mmq_bn": 0, "mmq_skinny": 1, "decode_copy": 1, "qkv": 1, "timing": 0}
K0 = 512


@contextlib.contextmanager
def options(backend, **kw):
    try:
        for k, v in kw.items():
            backend.set_option(k, v)
        yield
    finally:
        for k in kw:
            backend.set_option(k, DEFAULTS[k])


class Weights:
    """Weight matrices in a buffer of their own (usage WEIGHTS: the backend then keeps its second copies — decode planes, Q8_0 panels)."""

    def __init__(self, H, buft, specs, usage_weights=True):
        self.H = H
        self.ctx = H.ggml_init(L.InitParams(0, None, True))
        self.t = [H.ggml_new_tensor_2d(self.ctx, qt, K, N) for qt, K, N, _ in specs]
        self.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(self.ctx, buft)
        assert self.buf
        if usage_weights:
            H.ggml_backend_buffer_set_usage(self.buf, 1)  # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
        for t, (_, _, _, raw) in zip(self.t, specs):
            raw = np.ascontiguousarray(raw)
            assert raw.nbytes == H.ggml_nbytes(t)
            H.ggml_backend_tensor_set(t, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)

    def free(self):
        self.H.ggml_backend_buffer_free(self.buf)
        self.H.ggml_free(self.ctx)


def act_node(H, g, form, vals, K):
    """The graph producing the activation rows `vals` [M, K] exactly, and the values the quantiser then sees."""
    M = (vals[0] if form == "norm" else vals).shape[0]
    if form == "plain":
        return g.new(L.F32, [K, M], vals)
    if form == "norm":  # RMS_NORM(x in {+-1}, eps = 0) is x exactly (mean of squares 1, scale 1 / sqrt(1) = 1); times w = +-w
        signs, w = vals
        return H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [K, M], signs), 0.0), g.new(L.F32, [K], w))
    if form == "swiglu":  # silu(64) = 64 / (1 + expf(-64)) = 64 exactly for any expf (expf(-64) ~ 1.6e-28 vanishes against 1); 64 * (v / 64)
        return H.ggml_swiglu_split(g.ctx, g.new(L.F32, [K, M], np.full((M, K), 64.0, np.float32)), g.new(L.F32, [K, M], vals))
    raise ValueError(form)


def form_inputs(form, rows, M, rng):
    """Per graph run: (what act_node takes, the f32 values that reach the quantiser [M, K]).  `rows`: the catalogue."""
    runs = []
    if form == "norm":  # one edge row per run; the M columns carry it under different sign patterns (column 0: the row itself)
        for r in rows:
            signs = np.where(rng.integers(0, 2, (M, r.size)) == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
            signs[0] = 1.0
            runs.append(((signs, r), (signs * r[None, :]).astype(np.float32)))
        return runs
    n = len(rows)
    for c0 in range(0, n, M):
        v = P.tile_rows(np.roll(rows, -c0, axis=0), M) if c0 + M > n else np.ascontiguousarray(rows[c0:c0 + M])
        if form == "swiglu":
            with np.errstate(all="ignore"):
                up = (v / np.float32(64.0)).astype(np.float32)  # (exact but for f32 subnormals, which lose their last bits here)
                v = (np.float32(64.0) * up).astype(np.float32)
            runs.append((up, v))
        else:
            runs.append((v, v))
    return runs


def readout(backend, H, plog, tag, qt, form, M, opts=None, weights="graph", K=K0, reps=1, mm=None, quant=None, no_quant_launch=False, stats=None, seed=0):
    """Runs the catalogue through MUL_MAT(read-out weight [K, reps * K], activations [K, M]) (and the bsums read-out for Q4_K / Q5_K) on the oracle and the
    backend; asserts got == oracle == NumPy twin as uint32 and the route: every mat-mul kernel class starts with `mm`, the class `quant` ran (or, with
    no_quant_launch, no stand-alone quantiser did), the counters in `stats` moved by the given amounts per graph run (a callable takes the delta)."""
    kind = P.act_kind(qt)
    rng = np.random.default_rng(1000 + seed + qt)
    rows, names = P.edge_activations(kind, K, rng)
    mats = [("values", np.tile(P.readout_weight(qt, K), (reps, 1)), reps * K, lambda v: np.tile(P.expected_readout(kind, v), (1, reps)))]
    if qt in (L.Q4_K, L.Q5_K):
        rb = 2 if reps == 1 else reps * 32  # (K / 32 rows each: stacked to whole 32-row tiles, and for the wide form to the rows of the value read-out)
        mats.append(("bsums", np.tile(P.bsums_readout_weight(qt, K), (rb, 1)), rb * K // 32, lambda v: np.tile(P.expected_bsums_readout(v), (1, rb))))
    n_runs = 0
    with options(backend, timing=1, **(opts or {})):
        for what, w, N, expect in mats:
            wd = Weights(H, backend.buft, [(qt, K, N, w)]) if weights == "weights" else None
            wh = Weights(H, H.ggml_backend_cpu_buffer_type(), [(qt, K, N, w)], False) if weights == "weights" else None
            try:
                for inp, vals in form_inputs(form, rows, M, rng):
                    def build(g, held=None):
                        wt = held.t[0] if held else g.new(qt, [K, N], w)
                        return H.ggml_mul_mat(g.ctx, wt, act_node(H, g, form, inp, K))

                    ref = T.run_case(lambda g: build(g, wh), "oracle")[0].reshape(M, N)
                    backend.timing_report()
                    s0 = {k: backend.stat(k) for k in (stats or {})}
                    got = T.run_case(lambda g: build(g, wd), backend)[0].reshape(M, N)
                    classes = sorted(backend.timing_report())
                    n_runs += 1
                    want = expect(vals)
                    for a, b, nm in ((got, ref, "oracle"), (ref, want, "NumPy twin (oracle against it)")):
                        bad = P.bits(a) != P.bits(b)
                        if bad.any():
                            m, j = (int(v) for v in np.argwhere(bad)[0])
                            which = names[int(np.argmax([np.array_equal(vals[m], r) or np.array_equal(np.abs(vals[m]), np.abs(r)) for r in rows]))]
                            raise AssertionError(f"{tag} [{what}] differs from the {nm} in {int(bad.sum())}/{bad.size} outputs; first: column {m} ('{which}') output {j}: "
                                                 f"{a[m, j]!r} != {b[m, j]!r}; classes {classes}")
                    mmc = [c for c in classes if c.startswith(("mmvq_", "mmq_"))]
                    assert mmc and all(c.startswith(mm) for c in mmc), f"{tag}: mat-mul classes {mmc}, expected {mm}*"
                    if quant:
                        assert quant in classes, f"{tag}: quantiser class {quant} did not run: {classes}"
                    if no_quant_launch:
                        assert not [c for c in classes if "quantize" in c], f"{tag}: a stand-alone quantiser ran: {classes}"
                    for k, d in (stats or {}).items():
                        delta = backend.stat(k) - s0[k]
                        assert d(delta) if callable(d) else delta == d, f"{tag}: counter {k} moved by {delta}; classes {classes}"
            finally:
                for o in (wd, wh):
                    if o:
                        o.free()
    plog(f"{tag}: {n_runs} graph runs bit-equal to the oracle and the NumPy twin")


# ------------------------------------------------------------------------------------------------ (a) read-out through every route
@pytest.mark.parametrize("qt", QTYPES, ids=lambda q: QNAME[q])
@pytest.mark.parametrize("M,opts", [(1, {"fusion": 0}), (2, {"fusion": 0}), (3, {"mmq_min_cols": 9}), (5, {"mmq_min_cols": 9, "fusion": 0}), (8, {"mmq_min_cols": 9})],
                         ids=["M1-fusion0", "M2-fusion0", "M3-min9", "M5-min9-fusion0", "M8-min9"])
def test_standalone_quantiser_then_mat_vec(backend, H, plog, qt, M, opts):
    """k_quantize_q8_K / k_quantize_q8_0 in a launch of their own, read by the 1 .. 8-column mat-vec kernels."""
    if qt != L.Q8_0 and M == 2:
        opts = dict(opts, mmq_min_cols=9)  # (two columns of a K-quant would take the skinny matrix-core kernel)
    readout(backend, H, plog, f"quantize -> mat-vec {QNAME[qt]} M={M}", qt, "plain", M, opts, mm=f"mmvq_{QNAME[qt]}_nc{M}", quant="quantize_act", seed=M)


@pytest.mark.parametrize("qt", QTYPES, ids=lambda q: QNAME[q])
@pytest.mark.parametrize("weights,copy", [("graph", 1), ("weights", 1), ("weights", 0)], ids=["block_layout", "decode_copy", "decode_copy_off"])
@pytest.mark.parametrize("form,cls", [("plain", "f32pro"), ("norm", "normpro")], ids=["f32pro", "normpro"])
def test_batch1_prologues(backend, H, plog, qt, form, cls, weights, copy):
    """Batch 1: the mat-vec launch quantises its own activation row (k_mmvq / k_mmvq_stream prologues: plain f32 and RMS_NORM * w), over the block
    layout and over the decode copy of a WEIGHTS buffer.  No stand-alone quantiser may run."""
    streamed = weights == "weights" and copy == 1  # (Q8_0: the counter is left alone — the class and the absent quantiser launch pin its route)
    readout(backend, H, plog, f"{cls} {QNAME[qt]} {weights} decode_copy={copy}", qt, form, 1, {"decode_copy": copy}, weights, mm=f"mmvq_{QNAME[qt]}_{cls}", no_quant_launch=True,
            stats={} if qt == L.Q8_0 else {"decode_copy_launches": 1 if streamed else 0}, seed=copy)


KQ_BATCH = [(9, {}), (32, {}), (32, {"mmq_skinny": 0}), (33, {"mmq_skinny": 0, "mmq_bn": 64}), (33, {"mmq_i8": 0}), (130, {"mmq_skinny": 0, "mmq_bn": 128}), (130, {"mmq_i8": 0}), (512, {"mmq_skinny": 0})]


# (the SwiGLU producer is read through the 9-, 32- and 130-column consumers; 33 / 512 columns add no quantiser path to it)
KQ_CASES = [("norm", "rms_norm_mul_quantize", m, o) for m, o in KQ_BATCH] + [("swiglu", "swiglu_quantize", m, o) for m, o in KQ_BATCH if m not in (33, 512)]


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K, L.Q6_K], ids=lambda q: QNAME[q])
@pytest.mark.parametrize("form,quant,M,opts", KQ_CASES, ids=[f"{f}-M{m}-" + ("-".join(f"{k}{v}" for k, v in o.items()) or "default") for f, _, m, o in KQ_CASES])
def test_k_quant_batch_routes(backend, H, plog, qt, form, quant, M, opts):
    """Batches: k_rms_norm_mul_q8_K<false> and k_swiglu_q8_K write the Q8_K blocks; read by the skinny matrix-core kernel (2 .. 32 columns), the tiled
    int8 GEMM with 64- / 128-row panels, and the f16-MFMA kernel (mmq_i8 0)."""
    stats = {}
    if opts.get("mmq_i8", 1):
        sk = opts.get("mmq_skinny", 1) and M <= 32
        stats = {"skinny_launches": 1 if sk else 0, "tiled_launches": 0 if sk else 1, "wide_launches": 0}
    readout(backend, H, plog, f"{quant} -> {QNAME[qt]} M={M} {opts}", qt, form, M, opts, mm=f"mmq_{QNAME[qt]}_n", quant=quant, stats=stats, seed=M)


@pytest.mark.parametrize("qt", [L.Q4_K, L.Q5_K], ids=lambda q: QNAME[q])
def test_k_quant_wide_form(backend, H, plog, qt):
    """k_quantize_q8_K -> the wide form of the skinny unit (k_mmq_wide: prompt batches over many row groups): the read-out stacked eight times, 512 columns."""
    readout(backend, H, plog, f"quantize -> wide {QNAME[qt]}", qt, "plain", 512, {}, reps=8, mm=f"mmq_{QNAME[qt]}_n", quant="quantize_act", stats={"wide_launches": 1, "skinny_launches": 0})


Q80_BATCH = [
    ("wide_mat_vec", "plain", 16, 288, "graph", "mmvq_q8_0_nc8", "quantize_act", 0),
    ("wide_mat_vec", "plain", 32, 288, "graph", "mmvq_q8_0_nc8", "quantize_act", 0),
    ("skinny", "plain", 9, 512, "graph", "mmq_q8_0_skinny", "quantize_act", 1),
    ("skinny", "plain", 32, 512, "weights", "mmq_q8_0_skinny", "quantize_act", 1),
    ("skinny", "plain", 97, 512, "graph", "mmq_q8_0_skinny", "quantize_act", 1),
    ("skinny", "plain", 128, 512, "weights", "mmq_q8_0_skinny", "quantize_act", 1),
    ("gemm", "plain", 130, 512, "graph", "mmq_q8_0", "quantize_act", 0),
    ("gemm", "plain", 130, 512, "weights", "mmq_q8_0", "quantize_act", 0),
    ("gemm", "plain", 300, 512, "weights", "mmq_q8_0", "quantize_act", 0),
    ("norm_panel", "norm", 9, 512, "graph", "mmq_q8_0_skinny", "rms_norm_mul_quantize_q8_0", 1),
    ("norm_panel", "norm", 32, 512, "weights", "mmq_q8_0_skinny", "rms_norm_mul_quantize_q8_0", 1),
    ("norm_panel", "norm", 100, 512, "weights", "mmq_q8_0_skinny", "rms_norm_mul_quantize_q8_0", 1),
    ("swiglu_panel", "swiglu", 9, 512, "graph", "mmq_q8_0_skinny", "swiglu_quantize_q8_0", 1),
    ("swiglu_panel", "swiglu", 64, 512, "weights", "mmq_q8_0_skinny", "swiglu_quantize_q8_0", 1),
]


@pytest.mark.parametrize("route,form,M,K,weights,mm,quant,skinny", Q80_BATCH, ids=[f"{c[0]}-M{c[2]}-K{c[3]}-{c[4]}" for c in Q80_BATCH])
def test_q8_0_batch_routes(backend, H, plog, route, form, M, K, weights, mm, quant, skinny):
    """Q8_0 weights: 16 / 32 columns in one pass of the mat-vec kernel (K not a multiple of 128), k_quantize_q8_0<PANEL> -> k_mmq_q80_skinny (9 .. 128
    columns), k_mmq_q80 (block order without a panel copy of the weights, panel order with one), and the panel producers after RMS_NORM and SwiGLU."""
    readout(backend, H, plog, f"q8_0 {route} M={M} K={K} {weights}", L.Q8_0, form, M, {}, weights, K=K, mm=mm, quant=quant, stats={"skinny_launches": skinny}, seed=M)


# ------------------------------------------------------------------------------------------------ (b) Q8_0 cache writers
def q80_dead(x):
    """Blocks of the f32 rows x whose 1 / d overflows to inf (the maximum an f32 subnormal): the reference's float -> int8 conversion is undefined there."""
    amax = np.abs(np.asarray(x, np.float32).reshape(-1, 32)).max(axis=1)
    with np.errstate(all="ignore"):
        d = (amax / np.float32(127.0)).astype(np.float32)
        return (d != 0) & np.isinf(np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)))


def q80_same(got, ref, what, x=None):
    """Byte equality of Q8_0 rows quantised from the f32 rows x; in the blocks q80_dead(x) marks only the scale is compared (module docstring).  The mask
    comes from the inputs alone, and the callers assert that it holds exactly the blocks the catalogue plants for it."""
    g, r = np.asarray(got).reshape(-1, 34), np.asarray(ref).reshape(-1, 34)
    live = ~q80_dead(x) if x is not None else np.ones(len(r), bool)
    assert np.array_equal(g[:, :2], r[:, :2]), f"{what}: {int((g[:, :2] != r[:, :2]).any(axis=1).sum())} block scales differ"
    bad = np.nonzero((g[live] != r[live]).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} blocks differ; first: oracle {r[live][bad[0]].tolist()} gpu {g[live][bad[0]].tolist()}"


def test_set_rows_into_q8_0_on_the_catalogue(backend, H, plog):
    rng = np.random.default_rng(41)
    W = 1024
    x, names = P.edge_activations("q8_0", W, rng)
    n, NCTX = len(x), 48
    rows = rng.permutation(NCTX)[:n].astype(np.int64)

    def build(g):
        return [H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [W, NCTX]), g.new(L.F32, [W, n], x), g.new(L.I64, [n], rows))]

    ref, got = T.run_case(build, "oracle"), T.run_case(build, backend)
    assert int(q80_dead(x).sum()) == 1 and q80_dead(x).reshape(n, -1).any(axis=1)[[nm.startswith("subnormal@") for nm in names].index(True)]  # the one planted block
    for i, r in enumerate(rows):
        q80_same(np.asarray(got[0]).reshape(NCTX, -1)[r], np.asarray(ref[0]).reshape(NCTX, -1)[r], f"set_rows -> q8_0 row '{names[i]}'", x[i])
    rest = np.setdiff1d(np.arange(NCTX), rows)
    q80_same(np.asarray(got[0]).reshape(NCTX, -1)[rest], np.asarray(ref[0]).reshape(NCTX, -1)[rest], "set_rows -> q8_0, rows not written")
    # the 3-D form (K of one micro-batch: [head_dim, n_head_kv, n_tokens] viewed as rows) with a broadcast index tensor
    x3, _ = P.edge_activations("q8_0", 256, rng)
    x3 = np.ascontiguousarray(x3[:20].reshape(2, 10, 256))
    idx3 = rng.permutation(16)[:10].astype(np.int64).reshape(1, 10)

    def build3(g):
        return [H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [256, 16, 2]), g.new(L.F32, [256, 10, 2], x3), g.new(L.I64, [10, 1], idx3))]

    ref, got = T.run_case(build3, "oracle"), T.run_case(build3, backend)
    full3 = np.zeros((2, 16, 256), np.float32)
    full3[:, idx3[0]] = x3
    assert int(q80_dead(full3).sum()) == 1
    q80_same(got[0], ref[0], "3-D set_rows -> q8_0 with a broadcast index", full3)
    plog(f"  set_rows f32 -> q8_0 on {n} catalogue rows of {W} and the 3-D form: byte-equal")


def test_cpy_f32_to_q8_0_and_back_on_the_catalogue(backend, H, plog):
    rng = np.random.default_rng(43)
    HD, NKV = 128, 2
    x, names = P.edge_activations("q8_0", NKV * HD, rng)
    NCTX = len(x)
    rb = NKV * HD // 32 * 34

    def build_back(g):
        k = H.ggml_view_3d(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX]), HD, NKV, NCTX, HD // 32 * 34, rb, 0)
        return [H.ggml_cpy(g.ctx, g.new(L.F32, [HD, NKV, NCTX], x), k)]

    ref, got = T.run_case(build_back, "oracle"), T.run_case(build_back, backend)
    for i in range(NCTX):
        q80_same(np.asarray(got[0]).reshape(NCTX, -1)[i], np.asarray(ref[0]).reshape(NCTX, -1)[i], f"cpy f32 -> q8_0 row '{names[i]}'", x[i])
    assert int(q80_dead(x).sum()) == 1
    cache = np.asarray(ref[0]).reshape(NCTX, rb)

    def build_cast(g):
        k = H.ggml_view_3d(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX], cache), HD, NKV, NCTX, HD // 32 * 34, rb, 0)
        return [H.ggml_cast(g.ctx, k, L.F32)]

    ref, got = T.run_case(build_cast, "oracle"), T.run_case(build_cast, backend)
    assert np.array_equal(P.bits(got[0]), P.bits(ref[0])), "cast q8_0 -> f32 is not bit-exact"


@pytest.mark.parametrize("qkv", [1, 0])
@pytest.mark.parametrize("wt", [L.Q4_K, L.Q8_0], ids=lambda q: QNAME[q])
def test_fused_qkv_store_into_a_q8_0_cache_on_the_catalogue(backend, H, plog, wt, qkv):
    """One decode token through norm -> {wq, wk, wv} -> +bias -> rope -> SET_ROWS into Q8_0 caches, as test_fused_qkv_rope_store builds it — with an all-zero
    token (every projection is an exact 0) and the biases carrying the catalogue rows, at position 0 (cos = 1, sin = 0: x * 1 - y * 0 = x), so the values
    the store quantises are the edge rows bit for bit.  K row and V row byte-equal to the oracle, from the fused launch (qkv 1) and from SET_ROWS (qkv 0)."""
    rng = np.random.default_rng(47 + wt)
    E, HD, NH, NKV, NCTX, slot = 1024, 128, 8, 2, 32, 11
    nw = rng.uniform(0.5, 1.5, E).astype(np.float32)
    wq, wk, wv = T.rand_weight(wt, E, NH * HD, rng), T.rand_weight(wt, E, NKV * HD, rng), T.rand_weight(wt, E, NKV * HD, rng)
    cat, names = P.edge_activations("q8_0", NKV * HD, rng)
    bq = rng.standard_normal(NH * HD).astype(np.float32)
    kc0, vc0 = T.rand_weight(L.Q8_0, NKV * HD, NCTX, rng), T.rand_weight(L.Q8_0, NKV * HD, NCTX, rng)
    launches = []
    assert int(q80_dead(cat).sum()) == 1
    with options(backend, qkv=qkv):
        for i in range(len(cat)):
            bk, bv = cat[i], cat[(i + 7) % len(cat)]

            def build(g):
                cur = H.ggml_mul(g.ctx, H.ggml_rms_norm(g.ctx, g.new(L.F32, [E, 1], np.zeros((1, E), np.float32)), 1e-5), g.new(L.F32, [E], nw))
                q = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(wt, [E, NH * HD], wq), cur), g.new(L.F32, [NH * HD], bq))
                k = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(wt, [E, NKV * HD], wk), cur), g.new(L.F32, [NKV * HD], bk))
                v = H.ggml_add(g.ctx, H.ggml_mul_mat(g.ctx, g.new(wt, [E, NKV * HD], wv), cur), g.new(L.F32, [NKV * HD], bv))
                tp = g.new(L.I32, [1], np.array([0], np.int32))
                idx = g.new(L.I64, [1], np.array([slot], np.int64))
                q = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, q, HD, NH, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
                k = H.ggml_rope_ext(g.ctx, H.ggml_reshape_3d(g.ctx, k, HD, NKV, 1), tp, None, HD, 0, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
                v = H.ggml_reshape_3d(g.ctx, v, HD, NKV, 1)
                ks = H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX], kc0), H.ggml_reshape_2d(g.ctx, k, NKV * HD, 1), idx)
                vs = H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX], vc0), H.ggml_reshape_2d(g.ctx, v, NKV * HD, 1), idx)
                return [q, ks, vs]

            ref = T.run_case(build, "oracle")
            k0 = backend.stat("kernel_launches")
            got = T.run_case(build, backend)
            launches.append(backend.stat("kernel_launches") - k0)
            assert np.array_equal(P.bits(got[0]), P.bits(ref[0])), "q = 0 + bias, rotated by the identity"
            for o, xrow, nm in ((1, bk, f"K cache, row '{names[i]}'"), (2, bv, f"V cache, row '{names[(i + 7) % len(cat)]}'")):
                g2, r2 = np.asarray(got[o]).reshape(NCTX, -1), np.asarray(ref[o]).reshape(NCTX, -1)
                q80_same(g2[slot], r2[slot], f"{nm} (qkv {qkv})", xrow)
                q80_same(np.delete(g2, slot, axis=0), np.delete(r2, slot, axis=0), f"{nm} (qkv {qkv}): cells of other tokens")
    plog(f"  Q/K/V store into q8_0 caches ({QNAME[wt]} weights, qkv {qkv}): {len(cat)} catalogue rows byte-equal; kernel launches per token {sorted(set(launches))}")
    # the route: (cos, sin) table + ONE fused launch, or the separate kernels (a run replayed as a captured graph counts no launches)
    assert (max(launches) == 2) if qkv else (max(launches) > 2), launches


@pytest.mark.parametrize("NH,NKV,nq,nkv,splits", [(32, 8, 1, 1024, 0), (16, 2, 4, 300, 1), (28, 4, 2, 700, 5)])
def test_q8_0_query_rows_from_the_catalogue(backend, H, plog, NH, NKV, nq, nkv, splits):
    """The 8-bit query of the in-place decode attention over a Q8_0 cache (fattn.hip): test_flash_attn_q8_0_kv's set-up with the query rows taken from the
    Q8_0 edge catalogue.  The query's quantised bytes are not observable from outside, so this one site keeps that test's NMSE <= 1e-6 gate against the oracle
    instead of equality.  (Catalogue rows whose scale overflows nothing: the logits stay finite; the half-way rows reach |q| = 127.)"""
    HD = 128
    rng = np.random.default_rng(NH * 3 + nkv + nq)
    NCTX = nkv + 64
    cat, _ = P.edge_activations("q8_0", HD, rng)
    q = P.tile_rows(cat, NH * nq).reshape(NH, nq, HD)
    kf = (rng.standard_normal((nkv, NKV * HD)) * rng.uniform(0.3, 2.0, (nkv, 1))).astype(np.float32)
    vf = (rng.standard_normal((nkv, NKV * HD)) * rng.uniform(0.3, 2.0, (nkv, 1))).astype(np.float32)
    kf[3, :64] = 0.0
    rows = np.arange(nkv, dtype=np.int64)
    MR = (nq + 63) // 64 * 64
    mask = np.full((MR, nkv), -np.inf, np.float16)
    for t in range(nq):
        mask[t, : nkv - nq + t + 1 - 9] = 0
        mask[t, 5] = -np.inf
    rb = NKV * HD // 32 * 34

    def build(g):
        tq = g.new(L.F32, [HD, nq, NH], q)
        idx = g.new(L.I64, [nkv], rows)
        ks = H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX]), g.new(L.F32, [NKV * HD, nkv], kf), idx)
        vs = H.ggml_set_rows(g.ctx, g.new(L.Q8_0, [NKV * HD, NCTX]), g.new(L.F32, [NKV * HD, nkv], vf), idx)
        k = H.ggml_view_3d(g.ctx, ks, HD, nkv, NKV, rb, HD // 32 * 34, 0)
        v = H.ggml_view_3d(g.ctx, vs, HD, nkv, NKV, rb, HD // 32 * 34, 0)
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, g.new(L.F16, [nkv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return [r, ks, vs]

    backend.set_option("fa_splits", splits)
    try:
        ref, got = T.run_case(build, "oracle"), T.run_case(build, backend)
    finally:
        backend.set_option("fa_splits", 0)
    for i in (1, 2):
        assert np.array_equal(got[i], ref[i])
    T.compare(f"flash_attn q8_0 KV, catalogue queries H={NH}/{NKV} nq={nq} nkv={nkv} splits={splits}", got[0], ref[0], max_nmse=1e-6, log=plog)


# ------------------------------------------------------------------------------------------------ (a) attention -> wo hand-off
def attn_wo_case(H, qt, NH, NKV, seed=0):
    """FLASH_ATTN_EXT -> reshape -> MUL_MAT(read-out wo) where every query token sees exactly ONE cache cell: its softmax weight is exp(0) / 1 = 1, so
    the attention row is that cell's V row bit for bit (f16 values, exact in f32) whatever q and K hold.  Cell t of the V cache holds catalogue row t
    rounded to f16 (rows that overflow f16 — the 1e30 row — are left out); with grouped heads every 128-value slice repeats per query head of its group.
    -> (build(g, cells) for the tokens that see `cells`, the f32 rows the quantiser sees [n, NH * 128], names)"""
    HD = 128
    E, EK = NH * HD, NKV * HD
    kind = P.act_kind(qt)
    rng = np.random.default_rng(7000 + seed + qt)
    rows, names = P.edge_activations(kind, EK, rng)
    with np.errstate(over="ignore"):
        v16 = rows.astype(np.float16)
    keep = np.isfinite(v16.astype(np.float32)).all(axis=1)
    v16, names = v16[keep], [nm for nm, k in zip(names, keep) if k]
    n, n_kv = len(v16), 256
    vc = (rng.standard_normal((n_kv, EK)) * 0.5).astype(np.float16)
    cell_of = rng.permutation(n_kv)[:n]
    vc[cell_of] = v16
    kc = (rng.standard_normal((n_kv, EK)) * 0.5).astype(np.float16)
    G = NH // NKV
    vals = np.concatenate([v16.astype(np.float32).reshape(n, NKV, HD)[:, h // G] for h in range(NH)], axis=1)
    w = P.readout_weight(qt, E)

    def build(g, toks):
        nq = len(toks)
        q = np.random.default_rng(toks[0] + nq).standard_normal((NH, nq, HD)).astype(np.float32)
        MR = (nq + 63) // 64 * 64
        mask = np.full((MR, n_kv), -np.inf, np.float16)
        for i, t in enumerate(toks):
            mask[i, cell_of[t]] = 0
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [EK, n_kv], kc), HD, n_kv, NKV, EK * 2, HD * 2, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [EK, n_kv], vc), HD, n_kv, NKV, EK * 2, HD * 2, 0)
        fa = H.ggml_flash_attn_ext(g.ctx, g.new(L.F32, [HD, nq, NH], q), k, v, g.new(L.F16, [n_kv, MR], mask), 1.0 / np.sqrt(HD), 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(fa, 10)
        return H.ggml_mul_mat(g.ctx, g.new(qt, [E, E], w), H.ggml_reshape_2d(g.ctx, fa, E, nq))

    return build, vals, names


ATTN_WO = [("fa_wo_prologue", 4, 4, 1, {"fa_wo": 1}), ("fa_wo_prologue", 8, 4, 1, {"fa_wo": 1}), ("q8out_single_pass", 8, 4, 0, {}), ("q8out_combine", 4, 4, 0, {"fa_splits": 3}),
           ("q8out_combine", 8, 4, 0, {"fa_splits": 2})]


# (the batch hand-off leaves Q8_K blocks: K-quant wo only — graph.cpp quant_consumers_only; the one-token prologue serves Q8_0 too)
ATTN_WO_CASES = [(qt,) + c for c in ATTN_WO for qt in QTYPES if qt != L.Q8_0 or c[0] == "fa_wo_prologue"]


@pytest.mark.parametrize("qt,route,NH,NKV,per_graph,opts", ATTN_WO_CASES, ids=[f"{c[1]}-H{c[2]}over{c[3]}-{QNAME[c[0]]}" for c in ATTN_WO_CASES])
def test_attention_hands_its_result_to_wo_quantised(backend, H, plog, qt, route, NH, NKV, per_graph, opts):
    """The quantisers inside the attention kernels: one decode token whose split records are merged and quantised in the wo mat-vec's prologue (option fa_wo:
    class mmvq_<type>_attnpro after flash_attn_fat), and a batch whose attention leaves Q8_K blocks for wo — from its single pass (an even number of query
    heads per KV head) or from the combine pass over splits (Q8OUT) — so that NO stand-alone quantiser runs before the mat-mul.  Same equality gate."""
    build, vals, names = attn_wo_case(H, qt, NH, NKV)
    kind = P.act_kind(qt)
    n = len(vals)
    groups = [[t] for t in range(n)] if per_graph == 1 else [list(range(n))]
    with options(backend, timing=1, **opts):
        for toks in groups:
            ref = T.run_case(lambda g: build(g, toks), "oracle")[0].reshape(len(toks), -1)
            backend.timing_report()
            got = T.run_case(lambda g: build(g, toks), backend)[0].reshape(len(toks), -1)
            classes = sorted(backend.timing_report())
            want = P.expected_readout(kind, vals[toks])
            for a, b, nm in ((got, ref, "oracle"), (ref, want, "NumPy twin (oracle against it)")):
                bad = P.bits(a) != P.bits(b)
                assert not bad.any(), (f"attention -> wo {route} {QNAME[qt]}: differs from the {nm} in {int(bad.sum())}/{bad.size} outputs; rows "
                                       f"{[names[toks[i]] for i in np.nonzero(bad.any(axis=1))[0]][:6]}; classes {classes}")
            assert not [c for c in classes if "quantize" in c], f"a stand-alone quantiser ran: {classes}"
            if route == "fa_wo_prologue":
                assert f"mmvq_{QNAME[qt]}_attnpro" in classes and "flash_attn_fat" in classes, classes
            else:
                assert "flash_attn" in classes and [c for c in classes if c.startswith(f"mmq_{QNAME[qt]}_n")], classes
    plog(f"attention -> wo {route} {QNAME[qt]} heads {NH}/{NKV}: {n} catalogue rows bit-equal")


@pytest.mark.parametrize("qt", QTYPES, ids=lambda q: QNAME[q])
@pytest.mark.parametrize("form,M,mm,quant", [("plain", 1, "mmvq_{}_f32pro", None), ("norm", 1, "mmvq_{}_normpro", None), ("plain", 5, "mmvq_{}_nc5", "quantize_act"), ("norm", 32, "mmq_{}", None)],
                         ids=["f32pro", "normpro", "mat_vec5", "norm32"])
def test_block_indexing_over_six_super_blocks(backend, H, plog, qt, form, M, mm, quant):
    """K = 1536: six Q8_K blocks (48 Q8_0 blocks) a row, the planted block at a different index in every catalogue row (K = 512 alternates between two)."""
    opts = {"mmq_min_cols": 9} if M == 5 else {}
    if M == 32:
        quant = "rms_norm_mul_quantize_q8_0" if qt == L.Q8_0 else "rms_norm_mul_quantize"
    readout(backend, H, plog, f"K=1536 {form} M={M} {QNAME[qt]}", qt, form, M, opts, K=1536, mm=mm.format(QNAME[qt]), quant=quant, no_quant_launch=M == 1, seed=M)


# ------------------------------------------------------------------------------------------------ (c) weight-value edges
WEIGHT_EDGES = ["d_neg", "dmin_neg", "d_subnormal", "d_zero", "d_max", "quants_m128", "all_max", "all_min"]
_D_OFF = {L.Q8_0: 0, L.Q4_K: 0, L.Q5_K: 0, L.Q6_K: 208}


def edge_weight(qt, case, K, N, rng):
    """harness.rand_blocks with one property of real files that it never draws; None where the format has no such field."""
    nb = K // L.TYPE_BLCK[qt]
    b = T.rand_blocks(qt, N * nb, K, rng)
    o = _D_OFF[qt]
    k45 = qt in (L.Q4_K, L.Q5_K)
    if case == "d_neg":  # Q6_K: d = 1 / iscale with iscale = -128 / max_scale — negative in real files all the time
        b[:, o + 1] |= 0x80
    elif case == "dmin_neg":
        if not k45:
            return None
        b[:, 3] |= 0x80
    elif case == "d_subnormal":  # 6e-8 .. 6e-5: f16 bit patterns 1 .. 0x3FF
        b[:, o:o + 2] = rng.integers(1, 0x400, N * nb).astype(np.uint16).view(np.uint8).reshape(-1, 2)
    elif case == "d_zero":
        b[:, o:o + 2] = 0
        b[::2, o + 1] = 0x80  # every other block -0.0
    elif case == "d_max":  # 65504
        b[:, o:o + 2] = np.array([0x7BFF], np.uint16).view(np.uint8)
    elif case == "quants_m128":
        if qt != L.Q8_0:
            return None
        b[:, 2:] = 0x80
    elif case in ("all_max", "all_min"):
        hi = case == "all_max"
        if qt == L.Q8_0:
            b[:, 2:] = 0x7F if hi else 0x80
        elif k45:
            b[:, 4:] = 0xFF if hi else 0x00  # six-bit scales and mins 63 / 0, quants 15 (31) / 0
        else:
            b[:, 0:192] = 0xFF if hi else 0x00  # quants 63 - 32 = 31 / 0 - 32 = -32
            b[:, 192:208] = 0x7F if hi else 0x80  # scales 127 / -128
    else:
        raise ValueError(case)
    return np.ascontiguousarray(b.reshape(N, nb * L.TYPE_SIZE[qt]))


def exact_activations(qt, K, M, rng):
    """Small integers times a power of two with one +-127 * 2^k element per block: they quantise with no rounding in play (d_act = 2^k exactly)."""
    B = 256 if qt != L.Q8_0 else 32
    x = rng.integers(-100, 101, (M, K // B, B)).astype(np.float32)
    at = rng.integers(0, B, (M, K // B))
    np.put_along_axis(x, at[:, :, None], np.where(rng.integers(0, 2, (M, K // B, 1)) == 0, 127.0, -127.0).astype(np.float32), axis=2)
    x *= np.exp2(rng.integers(-6, 5, (M, K // B, 1))).astype(np.float32)
    return np.ascontiguousarray(x.reshape(M, K))


def exact_terms(qt, w, x):
    """float64 value of MUL_MAT(w, x) [M, N] under the CPU semantics (integer sub-block sums exact, scales in float64) and the largest |term| among the
    per-block products that are summed in f32 (for Q4_K / Q5_K the scale term and the mins term separately)."""
    K = x.shape[1]
    N = w.shape[0]
    blk = w.reshape(-1, L.TYPE_SIZE[qt])
    wq = P.MG.unpack_q(qt, blk).astype(np.float64)
    d8, q8, bs = P.quantize(P.act_kind(qt), x)
    d8 = d8.astype(np.float64)
    if qt == L.Q8_0:
        nb = K // 32
        S = np.einsum("mbi,nbi->mnb", q8.astype(np.float64), wq.reshape(N, nb, 32))
        terms = [S * P.MG.f16(blk[:, 0:2]).astype(np.float64).reshape(1, N, nb) * d8[:, None, :]]
    elif qt == L.Q6_K:
        nb = K // 256
        S = np.einsum("mbgi,nbgi->mnbg", q8.reshape(-1, nb, 16, 16).astype(np.float64), wq.reshape(N, nb, 16, 16))
        sc = blk[:, 192:208].view(np.int8).astype(np.float64).reshape(1, N, nb, 16)
        terms = [(S * sc).sum(axis=3) * P.MG.f16(blk[:, 208:210]).astype(np.float64).reshape(1, N, nb) * d8[:, None, :]]
    else:
        nb = K // 256
        S = np.einsum("mbgi,nbgi->mnbg", q8.reshape(-1, nb, 8, 32).astype(np.float64), wq.reshape(N, nb, 8, 32))
        sc, mn = P.MG.scale_min_k4(blk[:, 4:16])
        sc, mn = sc.astype(np.float64).reshape(1, N, nb, 8), mn.astype(np.float64).reshape(1, N, nb, 8)
        b32 = bs.reshape(-1, nb, 8, 2).sum(axis=3).astype(np.float64)[:, None, :, :]
        d, dmin = (P.MG.f16(blk[:, c:c + 2]).astype(np.float64).reshape(1, N, nb) for c in (0, 2))
        terms = [(S * sc).sum(axis=3) * d * d8[:, None, :], -(b32 * mn).sum(axis=3) * dmin * d8[:, None, :]]
    exact = sum(t.sum(axis=2) for t in terms)
    return exact, max(float(np.abs(t).max()) for t in terms)


# max |f32 result - float64 value| in ulps of the largest |term|.  Measured on the CPU, the oracle against exact_terms over every case below (all formats, all
# weight cases, K = 256 and 512, 1 .. 300 columns): at most 8.5 (Q4_K, every field at its maximum, K = 256: the scale term and the mins term are both huge and
# cancel, and the oracle adds eight rounded lane sums; next Q6_K all-max 7.5, Q8_0 all-max 4.0; every other case below 3.2).  The gate is twice the measured value.
ULP_MEASURED = 8.5
ULP_GATE = 2.0 * ULP_MEASURED

WEIGHT_EDGE_CASES = [(qt, case, K) for qt in QTYPES for case in WEIGHT_EDGES for K in (256, 512) if not ((case == "dmin_neg" and qt not in (L.Q4_K, L.Q5_K)) or (case == "quants_m128" and qt != L.Q8_0))]


@pytest.mark.parametrize("qt,case,K", WEIGHT_EDGE_CASES, ids=[f"{QNAME[q]}-{c}-K{k}" for q, c, k in WEIGHT_EDGE_CASES])
def test_weight_value_edges(backend, H, plog, qt, case, K):
    """Weights rand_blocks never draws — negative d (and dmin), f16-subnormal d, d = +-0, the largest finite f16 d, Q8_0 quants of -128, every scale / min /
    quant at its maximum and at its minimum (Q6_K: scales -128 over quants -32) — under activations that quantise exactly, through 1 column (block layout and
    the decode copy of a WEIGHTS buffer), 4, 16, 64 and 300 columns.  Gate: NMSE <= 1e-10 against the oracle AND max |got - float64 value| <= ULP_GATE ulps
    of the largest |term| (the oracle's own distance from float64, measured on the CPU, doubled), so one wrong row cannot hide in the norm.
    No bit-equality gate at K = 256: the oracle's expression has no single rounding sequence there either — Q8_0 adds eight block products in f32,
    Q6_K (like Q4_K / Q5_K) keeps eight lane sums that it adds at the end — so any other summation order is equally valid; bit_equal is logged."""
    N = 64
    rng = np.random.default_rng(K + qt * 7 + WEIGHT_EDGES.index(case))
    w = edge_weight(qt, case, K, N, rng)
    for M, held in ((1, False), (1, True), (4, False), (16, False), (64, False), (300, False)):
        x = exact_activations(qt, K, M, rng)
        wd = Weights(H, backend.buft, [(qt, K, N, w)]) if held else None
        wh = Weights(H, H.ggml_backend_cpu_buffer_type(), [(qt, K, N, w)], False) if held else None
        try:
            def build(g, hw=None):
                return H.ggml_mul_mat(g.ctx, hw.t[0] if hw else g.new(qt, [K, N], w), g.new(L.F32, [K, M], x))

            ref = T.run_case(lambda g: build(g, wh), "oracle")[0].reshape(M, N)
            s0 = backend.stat("decode_copy_launches")
            got = T.run_case(lambda g: build(g, wd), backend)[0].reshape(M, N)
            if qt != L.Q8_0:
                assert backend.stat("decode_copy_launches") - s0 == (1 if held else 0)
        finally:
            for o in (wd, wh):
                if o:
                    o.free()
        exact, top = exact_terms(qt, w, x)
        ulp = float(np.spacing(np.float32(top))) if top > 0 else 0.0
        e_gpu, e_cpu = float(np.abs(got.astype(np.float64) - exact).max()), float(np.abs(ref.astype(np.float64) - exact).max())
        tag = f"weight edge {QNAME[qt]} {case} K={K} M={M}{' decode copy' if held else ''}"
        plog(f"{tag}: max |gpu - f64| = {e_gpu / ulp if ulp else 0:.3f} ulp of the largest term, oracle {e_cpu / ulp if ulp else 0:.3f}")
        T.compare(tag, got, ref, max_nmse=1e-10, log=plog)
        assert e_gpu <= ULP_GATE * ulp, f"{tag}: {e_gpu / ulp if ulp else np.inf:.3f} ulp from the float64 value (gate {ULP_GATE})"
