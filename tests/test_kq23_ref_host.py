"""CPU-side tests for Q2_K / Q3_K: the NumPy twin of tests/kq23_ref.py against known-answer blocks (tests/golden/kq23_blocks.json, written value by value by
tests/golden/make_kq23_golden.py, which shares no code with the twin), its integer vec_dot against the float64 dot of the dequantised operands, and the model
generator's new file types, presets and loader with the hybrid (oracle + twin) compute function."""
import json
import os

import numpy as np
import pytest

import kq23_ref as R
import llama_box_amd as L
from model_util import Context, Model, greedy, preset

IDS = lambda q: L.TYPE_NAME[q]  # noqa: E731
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kq23_blocks.json")) as _f:
    GOLDEN = json.load(_f)


def test_type_tables_know_the_two_layouts():
    H = L.host()
    assert (L.Q2_K, L.Q3_K) == (10, 11)
    assert (L.TYPE_BLCK[L.Q2_K], L.TYPE_SIZE[L.Q2_K], L.TYPE_BLCK[L.Q3_K], L.TYPE_SIZE[L.Q3_K]) == (256, 84, 256, 110)
    assert H.ggml_row_size(L.Q2_K, 4096) == 16 * 84 and H.ggml_row_size(L.Q3_K, 4096) == 16 * 110


def test_golden_file_has_three_blocks_per_format():
    for t in ("q2_K", "q3_K"):
        names = [b["name"] for b in GOLDEN if b["type"] == t]
        assert len(names) >= 3 and any("minimum" in n for n in names) and any("maximum" in n for n in names) and any("different scale" in n for n in names)


@pytest.mark.parametrize("blk", GOLDEN, ids=lambda b: b["name"].replace(" ", "_"))
def test_twin_dequantize_matches_known_answer_block(blk):
    qt = {"q2_K": L.Q2_K, "q3_K": L.Q3_K}[blk["type"]]
    raw = np.array(blk["bytes"], dtype=np.uint8)
    want = np.array(blk["values"], dtype=np.float32)
    assert raw.size == L.TYPE_SIZE[qt] and want.size == 256
    assert np.array_equal(want.astype(np.float64), np.array(blk["values"]))  # (the worksheet's values are exact in float32)
    got = R.dequantize(qt, raw[None], 256)[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
    if "different scale" in blk["name"]:  # a permuted scale unpack cannot pass: sixteen sub-blocks, sixteen different |scale|
        sc = R.unpack(qt, raw[None], 256)["scale"][0, 0]
        assert len(set(sc.tolist())) == 16


@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_packers_are_inverted_by_the_twin(qt):
    """make_q2k / make_q3k (what the GPU tests build their weights with) against unpack: every field comes back."""
    rng = np.random.default_rng(qt)
    n = 40
    lev = rng.integers(0, 4, (n, 256)) if qt == L.Q2_K else rng.integers(-4, 4, (n, 256))
    sc = rng.integers(0, 16 if qt == L.Q2_K else 64, (n, 16))
    mn = rng.integers(0, 16, (n, 16))
    d = rng.uniform(-2, 2, n).astype(np.float16)
    raw = R.make_q2k(sc, mn, lev, d, -d) if qt == L.Q2_K else R.make_q3k(sc, lev, d)
    u = R.unpack(qt, raw, 256)
    assert np.array_equal(u["level"][:, 0], lev) and np.array_equal(u["scale"][:, 0], sc if qt == L.Q2_K else sc - 32)
    assert np.array_equal(u["d"][:, 0], d.astype(np.float32))
    if qt == L.Q2_K:
        assert np.array_equal(u["min"][:, 0], mn) and np.array_equal(u["dmin"][:, 0], (-d).astype(np.float32))


@pytest.mark.parametrize("edge", [False, True], ids=["sampled", "edges"])
@pytest.mark.parametrize("qt", R.FORMATS, ids=IDS)
def test_integer_vec_dot_equals_the_float64_dot_of_the_dequantised_operands(qt, edge):
    K, N, M = 1024, 24, 5
    rng = np.random.default_rng(100 + qt)
    W = (R.edge_blocks(qt, N * 4, rng) if edge else R.rand_blocks(qt, N * 4, K, rng)).reshape(N, -1)
    X = (rng.standard_normal((M, K)) * rng.uniform(0.1, 10.0, (M, 1))).astype(np.float32)
    y = R.quantize_q8k(X)
    assert np.array_equal(y["bsums"], y["qs"].reshape(M, K // 256, 16, 16).sum(axis=3))  # (the Q8_K blocks are the oracle's; their bsums feed both offset terms)
    got = R.mul_mat(qt, W, X).astype(np.float64)
    want = R.dequantize_q8k(y) @ R.dequantize(qt, W, K).astype(np.float64).T
    l1 = np.abs(R.dequantize_q8k(y)) @ np.abs(R.dequantize(qt, W, K).astype(np.float64)).T  # sum |x_i w_i|: the scale a float32 accumulation error is relative to
    # 1e-6 relative, twice: of the whole result in the 2-norm, and of every element against sum |x_i w_i| (the dot itself is float32 arithmetic — one rounding per
    # super-block term at 6e-8 — so an element that cancels to a tenth of its terms cannot hold 1e-6 of its own value: measured up to 6.4e-6 there)
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
    assert np.all(np.abs(got - want) <= 1e-6 * l1 + 1e-30), float(np.max(np.abs(got - want) / (l1 + 1e-30)))
    one = R.vec_dot(qt, W[3], y[2])
    assert np.float32(one).view(np.uint32) == np.float32(got[2, 3]).view(np.uint32)


def test_new_presets_and_file_types():
    k, t = preset("test-llama-kq23"), preset("test-llama")
    assert k.ftype == 15
    for f in ("n_layer", "n_embd", "n_head", "n_head_kv", "n_embd_head", "n_ff", "n_vocab", "qkv_bias", "rope_type"):
        assert getattr(k, f) == getattr(t, f), f
    a, b = preset("llama3-8b-q3_k_m"), preset("llama3-70b-q2_k")
    assert (a.ftype, a.n_layer, a.n_embd, a.n_ff, a.n_vocab) == (12, 32, 4096, 14336, 128256)
    assert (b.ftype, b.n_layer, b.n_embd, b.n_ff, b.n_vocab) == (13, 80, 8192, 28672, 128256)
    assert preset("test-llama-legacy").ftype == 11 and preset("test-llama").ftype == 5  # (earlier values stay)


WEIGHTS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def _types(H, m, hp):
    out = {n: H.llm_model_tensor(m.m, n.encode()).contents for n in ("token_embd.weight", "output.weight")}
    for il in range(hp.n_layer):
        for w in WEIGHTS:
            out[f"blk.{il}.{w}.weight"] = H.llm_model_tensor(m.m, f"blk.{il}.{w}.weight".encode()).contents
    return out


def test_kq23_model_loads_with_the_expected_types_and_byte_counts_and_decodes_on_the_hybrid_reference():
    H = L.host()
    hp = preset("test-llama-kq23")
    m = Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    try:
        ts = _types(H, m, hp)
        assert {t.type for t in ts.values()} == {L.Q2_K, L.Q3_K, L.Q4_K, L.Q6_K}
        # the recipe's draw (host/llama_lite.cpp: pick_type): the embeddings are Q3_K, the output matrix Q2_K, layer 0's gate and up share Q3_K
        assert ts["token_embd.weight"].type == L.Q3_K and ts["output.weight"].type == L.Q2_K
        assert ts["blk.0.ffn_gate.weight"].type == L.Q3_K and ts["blk.0.ffn_up.weight"].type == L.Q3_K and ts["blk.2.ffn_down.weight"].type == L.Q2_K
        for n, t in ts.items():
            assert t.nb[0] == L.TYPE_SIZE[t.type] and t.nb[1] == (t.ne[0] // 256) * L.TYPE_SIZE[t.type], n
            assert H.ggml_nbytes(H.llm_model_tensor(m.m, n.encode())) == t.ne[1] * (t.ne[0] // 256) * L.TYPE_SIZE[t.type], n
        # the synthetic blocks decode to weights of a trained network's scale: rows of unit-order norm (the embeddings carry a sqrt(n_embd) gain)
        for n in ("blk.0.attn_k.weight", "blk.0.ffn_gate.weight"):
            t = ts[n]
            w = R.dequantize(t.type, R._rows(t, t.ne[0]), t.ne[0])
            rms = float(np.sqrt(np.mean(w.astype(np.float64) ** 2)) * np.sqrt(t.ne[0]))
            assert 0.5 < rms < 2.0 and abs(float(np.mean(w))) * np.sqrt(t.ne[0]) < 0.2, (n, rms, float(np.mean(w)))
        prompt = [1, 5, 9, 300, 17, 42, 99, 7]
        runs = []
        for _ in range(2):
            c = Context(m, compute=R.hybrid_compute_fn(), flash_attn=0)
            ids, rows = greedy(c, prompt, 3)
            runs.append((ids, np.stack(rows)))
            c.free()
        assert np.all(np.isfinite(runs[0][1])) and float(np.std(runs[0][1])) > 0
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    finally:
        m.free()


@pytest.mark.parametrize("ft,base,others", [(14, "Q3_K", {}), (13, "Q2_K", {"attn_v": "Q3_K", "attn_output": "Q3_K", "ffn_down": "Q3_K"}),
                                            (12, "Q3_K", {"attn_output": "Q4_K"})], ids=["q3_k_s", "q2_k", "q3_k_m"])
def test_file_type_mixes(ft, base, others):
    H = L.host()
    hp = preset("test-llama", ftype=ft)
    m = Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    try:
        ts = _types(H, m, hp)
        assert ts["output.weight"].type == L.Q6_K and ts["token_embd.weight"].type == getattr(L, base)
        for il in range(hp.n_layer):
            for w in WEIGHTS:
                t = ts[f"blk.{il}.{w}.weight"].type
                if ft == 12 and w in ("attn_v", "ffn_down"):
                    assert t in (L.Q4_K, L.Q5_K), (il, w, t)
                else:
                    assert t == getattr(L, others.get(w, base)), (il, w, t)
    finally:
        m.free()
