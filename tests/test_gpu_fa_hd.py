"""FLASH_ATTN_EXT at head sizes 72 / 80 / 88 / 112 on the GPU (csrc/fattn_hd.hip): supports_op, the split kernel on 16-lane rows for 1 .. 32 tokens (and for
every soft-capped / ALiBi / sink batch), the matrix cores at the padded sizes 96 / 128 for prompt batches, the tower and gap layouts, fa_ref's cell accounting, a
replayed hipGraph, and what stays refused.  Every test asserts supports_op on its node before anything is computed (on a tree without these sizes it fails there and
launches nothing); every computed node states the kernel form it expects (stat "fa_form").  Specs, layouts and gates: tests/fa_hd.py (proved on the CPU by
test_fa_hd_ref_host.py)."""
import ctypes as C

import numpy as np
import pytest

import fa_d256 as F2
import fa_hd as FH
import fa_ref as FR
import harness as T
import llama_box_amd as L

pytestmark = pytest.mark.gpu

_WORST = {}


def _require(backend, H, spec):
    assert F2.supported(backend, H, FH.builder(spec, None, H)), f"{spec.id}: supports_op refuses FLASH_ATTN_EXT at head size {spec.HD} ({spec.NH}/{spec.NKV} heads, {spec.layout} layout)"


def _compute(backend, H, spec, x):
    backend.set_option("fa_splits", spec.splits)
    try:
        got = FH.run_node(spec, x, backend, H)
        ran = backend.stat("fa_form")
    finally:
        backend.set_option("fa_splits", 0)
    assert ran == spec.form, f"{spec.id}: expected form [{FH.form_name(spec.form)}], ran [{FH.form_name(ran)}]"
    return got


def _gates(spec, got, ref, exact, plog):
    e_ref, e_gpu, e_cpu = T.nmse(got, ref), T.nmse(got, exact), T.nmse(ref, exact)
    key = f"{spec.kernel} D={spec.HD}"
    w = _WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_ref), max(w[1], e_gpu)
    plog(f"fa_hd {spec.id} [{FH.form_name(spec.form)}]: vs oracle {e_ref:.3e}  vs twin {e_gpu:.3e}  oracle vs twin {e_cpu:.3e} | worst so far of {key}: vs oracle {w[0]:.3e}  vs twin {w[1]:.3e}")
    assert not np.isnan(got).any(), f"{spec.id}: NaN in the result"
    assert e_ref <= F2.ORACLE_F16, f"{spec.id}: nmse {e_ref:.3e} against the oracle"
    assert e_gpu <= (F2.TWIN_MMA if spec.kernel == "MMA" else F2.TWIN_SPLIT), f"{spec.id}: nmse {e_gpu:.3e} against the float64 twin"
    assert e_gpu <= e_cpu * 1.01 + 1e-12, f"{spec.id}: further from the twin ({e_gpu:.3e}) than the oracle is ({e_cpu:.3e})"


# ------------------------------------------------------------------------------------------ the kernels on random data, every layout
@pytest.mark.parametrize("spec", FH.RANDOM_SPECS, ids=lambda s: s.id)
def test_flash_attn_hd(backend, H, plog, spec):
    _require(backend, H, spec)
    x, ref, exact = FH.reference(spec, H)
    got = _compute(backend, H, spec, x)
    _gates(spec, got, ref, exact, plog)


# ------------------------------------------------------------------------------------------ cell accounting
@pytest.mark.parametrize("spec", FH.CELL_SPECS, ids=lambda s: s.id)
def test_fa_cells_hd(backend, H, plog, spec):
    """fa_ref's indicator, witness and pair probes (one wrong cell is an order-one error) at their own gates: edges at the trip (63 | 64), the split boundary, the
    64-cell tile and the cache end."""
    _require(backend, H, spec)
    case = FH.fr_case(spec)
    assert case.trip == 64 and case.n_splits == spec.n_splits and (spec.kernel == "MMA" or spec.n_splits >= 2)
    assert {0, 63, 64, 65, case.nkv - 1} <= set(FR.edges_of(case, 0))
    bad, worst = [], {}
    backend.set_option("fa_splits", spec.splits)
    try:
        probes = FR.indicator_probes(case) + FR.witness_probes(case, False) + FR.witness_probes(case, True)
        assert any(p.name.startswith("indicator") for p in probes) and any(p.name.startswith("witness") for p in probes) and any(p.name.startswith("pair") for p in probes)
        for p in probes:
            got = FR.run_probe(case, p, backend, H)
            ran = backend.stat("fa_form")
            if ran != spec.form:
                bad.append(f"{p.name}: expected form [{FH.form_name(spec.form)}], ran [{FH.form_name(ran)}]")
            try:
                kind = p.name.split("_")[0]
                worst[kind] = max(worst.get(kind, 0.0), FR.check_probe(case, p, got))
            except AssertionError as e:
                bad.append(str(e))
    finally:
        backend.set_option("fa_splits", 0)
    plog(f"fa_cells_hd {spec.id}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" (gates: indicator {FR.INDICATOR_GATE}, witness {FR.WITNESS_GATE} x max|V|)")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------------------------------ one walk: the padded form against the full form
def _node(H, D, NH, NKV, q, K, V, mask, scale):
    """-> build(g): FLASH_ATTN_EXT over q [1, NH, nq, D] f32, K / V [nkv, NKV, D] f16 and an f16 mask (or None) with an EXPLICIT scale."""
    nq, nkv = q.shape[2], K.shape[0]

    def build(g):
        tq = g.new(L.F32, [D, nq, NH, 1], q)
        k = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * D, nkv], K), D, nkv, NKV, 2 * NKV * D, 2 * D, 0)
        v = H.ggml_view_3d(g.ctx, g.new(L.F16, [NKV * D, nkv], V), D, nkv, NKV, 2 * NKV * D, 2 * D, 0)
        m = g.new(L.F16, [nkv, mask.shape[0]], mask) if mask is not None else None
        r = H.ggml_flash_attn_ext(g.ctx, tq, k, v, m, scale, 0.0, 0.0)
        H.ggml_flash_attn_ext_set_prec(r, 10)
        return r

    return build


@pytest.mark.parametrize("nq,nkv,NH,NKV,masked", [(33, 68, 4, 2, True), (264, 132, 2, 1, False)], ids=["nw2_causal_at_end", "nw4_nomask"])
def test_padded_form_equals_full_form_on_zero_padded_operands(backend, H, plog, nq, nkv, NH, NKV, masked):
    """Head size 112 runs k_fattn_mma's PAD form at 128 columns; a head-size-128 node whose Q, K and V are the 112-wide ones with columns 112 .. 127 zero runs the
    full form.  Same mask, the same explicit scale 1 / sqrt(112), one split (no combine pass: the two sizes merge records with different kernels).  The pad products
    add exact zeros in the same matrix-core order, so the first 112 output columns are EQUAL as float values (-0 == +0); the pad columns of the 128 node are
    compared with the float64 twin only (exact zeros there).  The masked shape (33 tokens at the end of 68 cells, two query tiles x two cell tiles) walks a diagonal
    tile, a plainly visible one (the last token over cells 0 .. 63, no mask read) and the ragged four-cell tail under both query tiles; a causal mask at the cache's end
    hides no tile at this shape."""
    D, DP = 112, 128
    scale = float(1.0 / np.sqrt(D))
    rng = np.random.default_rng(112 * nq + nkv)
    q = np.zeros((1, NH, nq, DP), np.float32)
    K = np.zeros((nkv, NKV, DP), np.float16)
    V = np.zeros((nkv, NKV, DP), np.float16)
    q[..., :D] = rng.standard_normal((1, NH, nq, D)).astype(np.float32)
    K[..., :D] = rng.standard_normal((nkv, NKV, D)).astype(np.float16)
    V[..., :D] = rng.standard_normal((nkv, NKV, D)).astype(np.float16)
    mask = None
    if masked:  # causal at the cache's end: the last token sees every cell
        mask = np.full(((nq + 63) // 64 * 64, nkv), -np.inf, np.float16)
        for t in range(nq):
            mask[t, : nkv - nq + t + 1] = 0
    c = FR.fa_constants()
    waves = c["nw_big"] if nq >= c["wg128_min_q"] else c["nw_small"]
    mode = 1 if masked else 0
    nodes = {
        D: (_node(H, D, NH, NKV, np.ascontiguousarray(q[..., :D]), np.ascontiguousarray(K[..., :D]), np.ascontiguousarray(V[..., :D]), mask, scale), FH.form("MMA", mode, waves, D, "NONE")),
        DP: (_node(H, DP, NH, NKV, q, K, V, mask, scale), FR.form("MMA", mode, waves, "F16", DP, "NONE")),
    }
    got = {}
    backend.set_option("fa_splits", 1)
    try:
        for d, (build, form) in nodes.items():
            assert F2.supported(backend, H, build), d
            got[d] = np.asarray(T.run_case(build, backend)[0], np.float32).reshape(nq, NH, d)
            ran = backend.stat("fa_form")
            assert ran == form, f"head size {d}: expected form [{FH.form_name(form)}], ran [{FH.form_name(ran)}]"
    finally:
        backend.set_option("fa_splits", 0)
    assert nodes[DP][1] & FH.hd_mask() == 0 and nodes[D][1] & FH.hd_mask() == FH.hd_field(D)
    exact = F2.twin(q[0], K.astype(np.float64), V.astype(np.float64), mask, scale)  # [nq, NH, 128]
    differ = np.argwhere(got[D] != got[DP][..., :D])
    plog(f"fa_hd padded vs full nq={nq} nkv={nkv} waves={waves}: {len(differ)} of {got[D].size} values differ" + (f", first at {differ[0].tolist()}" if len(differ) else "")
         + f"; vs twin: padded {T.nmse(got[D], exact[..., :D]):.3e}  full {T.nmse(got[DP], exact):.3e}")
    assert not np.isnan(got[D]).any() and not np.isnan(got[DP]).any()
    assert np.array_equal(got[D], got[DP][..., :D]), f"{len(differ)} values differ, columns {sorted(set(differ[:, 2].tolist()))[:16]}"
    assert T.nmse(got[DP], exact) <= F2.TWIN_MMA
    assert np.array_equal(got[DP][..., D:], exact[..., D:].astype(np.float32))


# ------------------------------------------------------------------------------------------ hipGraph
def _three_steps(backend, H, spec, x):
    """The node followed by eight SCALE nodes (a graph of nine nodes: the backend replays graphs of eight and more), computed three times on the same buffers."""
    g = T.G(backend)
    try:
        r = FH.builder(spec, x, H)(g)
        out = r
        for _ in range(8):
            out = H.ggml_scale(g.ctx, out, 1.0)
        gf = H.ggml_new_graph_custom(g.ctx, 64, False)
        H.ggml_set_output(r)
        H.ggml_set_output(out)
        H.ggml_build_forward_expand(gf, out)
        assert gf.contents.n_nodes >= 9
        for i in range(gf.contents.n_nodes):
            assert H.ggml_backend_dev_supports_op(backend.dev, gf.contents.nodes[i]), i
        g.buf = H.ggml_backend_alloc_ctx_tensors_from_buft(g.ctx, backend.buft)
        assert g.buf
        H.ggml_backend_buffer_clear(g.buf, 0)
        for tt, raw in g.inputs:
            H.ggml_backend_tensor_set(tt, raw.ctypes.data_as(C.c_void_p), 0, raw.nbytes)
        s0 = {k: backend.stat(k) for k in ("graph_launches", "graph_captures")}
        res = []
        for _ in range(3):
            assert H.ggml_backend_graph_compute(backend.backend, gf) == 0
            res.append((g.read(r).copy(), backend.stat("fa_form")))
        return res, {k: backend.stat(k) - v for k, v in s0.items()}
    finally:
        g.free()


def test_hipgraph_replay_is_bit_identical_to_eager(backend, H, plog):
    """A decode-shaped node at head size 80 (one token, 8 / 2 heads, 333 cells, three splits + combine): eager, captured, replayed — and the same three steps with
    graphs off: every step gives the same bits and reports the same form."""
    spec = FH.HIPGRAPH_SPEC
    _require(backend, H, spec)
    x, ref, exact = FH.reference(spec, H)
    runs = {}
    backend.set_option("fa_splits", spec.splits)
    try:
        for mode in (1, 0):
            backend.set_option("graphs", mode)
            runs[mode] = _three_steps(backend, H, spec, x)
    finally:
        backend.set_option("graphs", 1)
        backend.set_option("fa_splits", 0)
    plog(f"fa_hd hipGraph {spec.id}: graphs=1 {runs[1][1]}, graphs=0 {runs[0][1]}")
    assert runs[1][1]["graph_launches"] == 2 and runs[1][1]["graph_captures"] == 1, runs[1][1]
    assert runs[0][1]["graph_launches"] == 0 and runs[0][1]["graph_captures"] == 0, runs[0][1]
    for (a, fa), (b, fb) in zip(runs[1][0], runs[0][0]):
        assert fa == spec.form and fb == spec.form, (FH.form_name(fa), FH.form_name(fb))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    got = runs[1][0][2][0].reshape(spec.nb, spec.nq, spec.NH, spec.HD)
    _gates(spec, got, ref, exact, plog)


# ------------------------------------------------------------------------------------------ what stays refused; what the other sizes still run
def test_supports_op_refusals(backend, H):
    for D in FH.SIZES:  # (on a tree without these sizes nothing below says anything)
        _require(backend, H, FH.Spec(f"d{D}_f16", "SPLIT", 4, 2, 1, 64, HD=D))
        for g in (1, 2, 3, 4, 5, 6, 7, 8):
            _require(backend, H, FH.Spec(f"d{D}_g{g}", "SPLIT", g, 1, 1, 64, HD=D))
        _require(backend, H, FH.Spec(f"d{D}_cap_alibi_sinks_nb2", "SPLIT", 4, 2, 3, 64, HD=D, cap=30.0, alibi=4.0, sinks=True, nb=2))
    for name, build in FH.refused_builders(H):
        assert not F2.supported(backend, H, build), name


def test_other_head_sizes_keep_their_forms(backend, H, plog):
    """64 / 128 / 256 nodes report the forms they reported: two of fa_ref.CASES and one head-size-256 spec (none carries a head-size field)."""
    _require(backend, H, FH.Spec("d80_f16", "SPLIT", 4, 2, 1, 64, HD=80))
    by = {c.id: c for c in FR.CASES}
    for cid in ("split_d64_nomask", "mma_d128_33"):
        case = by[cid]
        p = FR.random_probe(case)
        backend.set_option("fa_splits", case.splits)
        try:
            got = FR.run_probe(case, p, backend, H)
            ran = backend.stat("fa_form")
        finally:
            backend.set_option("fa_splits", 0)
        assert ran == case.form and ran & FH.hd_mask() == 0, f"{cid}: [{FH.form_name(ran)}]"
        assert T.nmse(got, p.expect) <= (F2.TWIN_MMA if case.kernel == "MMA" else F2.TWIN_SPLIT), cid
    spec = F2.SPLIT_SPECS[5]
    assert spec.id == "split_gemma2_decode_cap" and spec.HD == 256
    x = F2.make_inputs(spec)
    backend.set_option("fa_splits", spec.splits)
    try:
        got = F2.run_node(spec, x, backend, H)
        ran = backend.stat("fa_form")
    finally:
        backend.set_option("fa_splits", 0)
    assert ran == spec.form and ran & FH.hd_mask() == 0, f"{spec.id}: [{FH.form_name(ran)}]"
    assert T.nmse(got, F2.twin_of(spec, x)) <= F2.TWIN_SPLIT
