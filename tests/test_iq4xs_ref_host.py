"""CPU-side tests for IQ4_XS: the NumPy twin of tests/iq4xs_ref.py against known-answer blocks (tests/golden/iq4xs_blocks.json, written value by value by
tests/golden/make_iq4xs_golden.py, which shares no code with the twin), its integer vec_dot against the float64 dot of the dequantised operands, and the model
generator's block recipe, file types, presets and loader with the hybrid (oracle + twin) compute function."""
import json
import os
import re

import numpy as np
import pytest

import iq4xs_ref as R
import llama_box_amd as L
from model_util import Context, Model, greedy, preset

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iq4xs_blocks.json")) as _f:
    GOLDEN = json.load(_f)


def test_type_tables_know_the_layout():
    H = L.host()
    assert L.IQ4_XS == 23 and L.TYPE_NAME[L.IQ4_XS] == "iq4_xs"
    assert (L.TYPE_BLCK[L.IQ4_XS], L.TYPE_SIZE[L.IQ4_XS]) == (256, 136)
    assert H.ggml_row_size(L.IQ4_XS, 4096) == 16 * 136  # (ggml_abi.h's tables, through the host library)
    src = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "ggml_abi.h")).read()
    assert re.search(r"sizeof\(block_iq4_xs\) == 136", src) and re.search(r"case GGML_TYPE_IQ4_XS: return 136;", src)


def test_golden_file_covers_the_six_cases():
    names = [b["name"] for b in GOLDEN]
    assert len(names) >= 6 and all(b["type"] == "iq4_xs" for b in GOLDEN)
    for word in ("minimum", "maximum", "different scale", "ramp", "negative d", "subnormal"):
        assert any(word in n for n in names), word


@pytest.mark.parametrize("blk", GOLDEN, ids=lambda b: b["name"].replace(" ", "_"))
def test_twin_dequantize_matches_known_answer_block(blk):
    raw = np.array(blk["bytes"], dtype=np.uint8)
    want = np.array(blk["values"], dtype=np.float32)
    assert raw.size == 136 and want.size == 256
    assert np.array_equal(want.astype(np.float64), np.array(blk["values"]))  # (the worksheet's values are exact in float32)
    got = R.dequantize(raw[None], 256)[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
    if "different scale" in blk["name"]:  # a permuted scale unpack cannot pass: eight sub-blocks, eight different scales, low nibbles and neighbouring bit pairs differ
        sc = R.unpack(raw[None], 256)["scale"][0, 0] + 32
        assert len(set(sc.tolist())) == 8 and len(set((sc & 15).tolist())) == 8 and all((sc[i] >> 4) != (sc[i + 1] >> 4) for i in range(7))


def test_packer_is_inverted_by_the_twin():
    """make_iq4xs (what the GPU tests build their weights with) against unpack: every field comes back."""
    rng = np.random.default_rng(23)
    n = 40
    nib, sc = rng.integers(0, 16, (n, 256)), rng.integers(0, 64, (n, 8))
    d = rng.uniform(-2, 2, n).astype(np.float16)
    u = R.unpack(R.make_iq4xs(sc, nib, d), 256)
    assert np.array_equal(u["nibble"][:, 0], nib) and np.array_equal(u["scale"][:, 0], sc - 32) and np.array_equal(u["d"][:, 0], d.astype(np.float32))
    assert np.array_equal(u["value"][:, 0], R.KVALUES[nib])
    # ... over the whole range of every field
    full = R.unpack(R.rand_blocks(400, 256, rng), 256)
    assert set(full["scale"].reshape(-1).tolist()) == set(range(-32, 32)) and set(full["nibble"].reshape(-1).tolist()) == set(range(16))


@pytest.mark.parametrize("edge", [False, True], ids=["sampled", "edges"])
def test_integer_vec_dot_equals_the_float64_dot_of_the_dequantised_operands(edge):
    K, N, M = 1024, 24, 5
    rng = np.random.default_rng(123)
    W = (R.edge_blocks(N * 4, rng) if edge else R.rand_blocks(N * 4, K, rng)).reshape(N, -1)
    X = (rng.standard_normal((M, K)) * rng.uniform(0.1, 10.0, (M, 1))).astype(np.float32)
    y = R.quantize_q8k(X)
    got = R.mul_mat(W, X).astype(np.float64)
    want = R.dequantize_q8k(y) @ R.dequantize(W, K).astype(np.float64).T
    l1 = np.abs(R.dequantize_q8k(y)) @ np.abs(R.dequantize(W, K).astype(np.float64)).T  # sum |x_i w_i|: the scale a float32 accumulation error is relative to
    # float32 arithmetic: three roundings a sub-block term (d4d8, times the scale, times the sum) and one per addition, 32 terms at K = 1024, each at 6e-8 of a
    # partial sum bounded by sum |x_i w_i| — 1e-6 of the 2-norm of the result and 2e-6 of sum |x_i w_i| per element
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
    assert np.all(np.abs(got - want) <= 2e-6 * l1 + 1e-30), float(np.max(np.abs(got - want) / (l1 + 1e-30)))
    one = R.vec_dot(W[3], y[2])
    assert np.float32(one).view(np.uint32) == np.float32(got[2, 3]).view(np.uint32)


def test_new_presets_and_file_types():
    k, t = preset("test-llama-iq4xs"), preset("test-llama-kq23")
    assert k.ftype == 18
    for f in ("n_layer", "n_embd", "n_head", "n_head_kv", "n_embd_head", "n_ff", "n_vocab", "qkv_bias", "rope_type"):
        assert getattr(k, f) == getattr(t, f), f
    a = preset("llama3-8b-iq4_xs")
    assert (a.ftype, a.n_layer, a.n_embd, a.n_ff, a.n_vocab) == (17, 32, 4096, 14336, 128256)
    assert preset("test-llama-kq23").ftype == 15 and preset("test-llama-bf16").ftype == 16  # (earlier values stay)


WEIGHTS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def _types(H, m, hp):
    out = {n: H.llm_model_tensor(m.m, n.encode()).contents for n in ("token_embd.weight", "output.weight")}
    for il in range(hp.n_layer):
        for w in WEIGHTS:
            out[f"blk.{il}.{w}.weight"] = H.llm_model_tensor(m.m, f"blk.{il}.{w}.weight".encode()).contents
    return out


def test_iq4xs_model_loads_with_the_expected_types_and_blocks_and_decodes_on_the_hybrid_reference():
    H = L.host()
    hp = preset("test-llama-iq4xs")
    m = Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    try:
        ts = _types(H, m, hp)
        assert {t.type for t in ts.values()} == {L.IQ4_XS, L.IQ4_NL, L.Q4_K, L.Q6_K}
        # the recipe (host/llama_lite.cpp: pick_type): the embeddings are IQ4_XS, layer 0's gate and up share IQ4_XS, the other layers' gate and up differ
        assert ts["token_embd.weight"].type == L.IQ4_XS and ts["output.weight"].type == L.Q6_K
        assert ts["blk.0.ffn_gate.weight"].type == L.IQ4_XS and ts["blk.0.ffn_up.weight"].type == L.IQ4_XS
        assert all(ts[f"blk.{il}.ffn_gate.weight"].type != ts[f"blk.{il}.ffn_up.weight"].type for il in (1, 2))
        assert {w for w in WEIGHTS for il in range(3) if ts[f"blk.{il}.{w}.weight"].type == L.IQ4_XS} == set(WEIGHTS) - {"attn_k"}
        for n, t in ts.items():
            per = L.TYPE_BLCK[t.type]
            assert t.nb[0] == L.TYPE_SIZE[t.type] and t.nb[1] == (t.ne[0] // per) * L.TYPE_SIZE[t.type], n
            assert H.ggml_nbytes(H.llm_model_tensor(m.m, n.encode())) == t.ne[1] * (t.ne[0] // per) * L.TYPE_SIZE[t.type], n
        # the synthetic blocks: every field over its whole range, and weights of a trained network's scale — rows of unit-order norm
        for n in ("blk.0.attn_q.weight", "blk.0.ffn_gate.weight"):
            t = ts[n]
            assert t.type == L.IQ4_XS
            raw = R._rows(t, t.ne[0])
            u = R.unpack(raw, t.ne[0])
            assert set(u["scale"].reshape(-1).tolist()) == set(range(-32, 32)) and set(u["nibble"].reshape(-1).tolist()) == set(range(16))
            w = R.dequantize(raw, t.ne[0])
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


def _pack_q6_K(x):
    """llama_lite.cpp's pack_q6_K (the generator's plain absmax encoder, float32 arithmetic) -> uint8 [n, 210]: x float32 [n, 256]"""
    f32 = np.float32
    n = x.shape[0]
    sub = (np.abs(x).reshape(n, 16, 16).max(axis=2) / f32(31.0)).astype(f32)
    smax = sub.max(axis=1)
    d16 = (smax / f32(127.0)).astype(f32).astype(np.float16)
    d = d16.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.clip(np.rint((sub / d[:, None]).astype(f32)), 1, 127).astype(np.int32)
        step = (d[:, None] * sc.astype(f32)).astype(f32)
        q = np.clip(np.rint((x.reshape(n, 16, 16) / step[:, :, None]).astype(f32)), -32, 31).astype(np.int32).reshape(n, 256) + 32
    out = np.zeros((n, 210), dtype=np.uint8)
    for h in range(2):
        q1, q2, q3, q4 = (q[:, 128 * h + 32 * k:128 * h + 32 * k + 32] for k in range(4))
        out[:, 64 * h:64 * h + 32] = (q1 & 15) | ((q3 & 15) << 4)
        out[:, 64 * h + 32:64 * h + 64] = (q2 & 15) | ((q4 & 15) << 4)
        out[:, 128 + 32 * h:160 + 32 * h] = (q1 >> 4) | ((q2 >> 4) << 2) | ((q3 >> 4) << 4) | ((q4 >> 4) << 6)
    out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, 208:210] = d16.view(np.uint8).reshape(n, 2)
    out[smax == 0] = 0
    return out


def test_block_values_of_the_model_generator_agree_with_the_twin():
    """A fully peaked model ties every output block to token_embd's: llama_lite's block_values of the IQ4_XS block, times the gain ratio 1 / sqrt(n_embd), packed
    as Q6_K by the generator's own encoder.  The twin's values through a NumPy restatement of that encoder must give the output rows BYTE for byte: a single
    wrong code or scale in block_values moves a Q6_K level or sub-scale of its block."""
    H = L.host()
    hp = preset("test-llama", ftype=17)
    hp.peaked = 8
    m = Model(hp, 99, H.ggml_backend_cpu_buffer_type())
    try:
        te, out = H.llm_model_tensor(m.m, b"token_embd.weight").contents, H.llm_model_tensor(m.m, b"output.weight").contents
        assert te.type == L.IQ4_XS and out.type == L.Q6_K
        K, n = te.ne[0], 64
        src = [(r * 7919 + 13) % hp.n_vocab for r in range(n)]  # (output row r repeats token_embd's row (7919 r + 13) mod n_vocab: llama_lite.cpp)
        gain = np.float32(1.0) / np.sqrt(np.float32(hp.n_embd))  # the output matrix's gain over the embeddings'
        vals = (R.dequantize(R._rows(te, K)[src], K) * gain).astype(np.float32)
        want = _pack_q6_K(vals.reshape(-1, 256)).reshape(n, -1)
        got = np.stack([R._host_bytes(out.data + r * out.nb[1], (K // 256) * 210) for r in range(n)])
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        # ... and the encoder restated here is not vacuous: one code changed in one block changes that block's bytes
        bad = vals.copy().reshape(-1, 256)
        bad[0, 5] = -bad[0, 5] if bad[0, 5] != 0 else 1.0
        assert not np.array_equal(_pack_q6_K(bad[:1]), want.reshape(-1, 210)[:1])
    finally:
        m.free()


def test_file_type_mix():
    H = L.host()
    hp = preset("test-llama", ftype=17)
    m = Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    try:
        ts = _types(H, m, hp)
        assert ts["output.weight"].type == L.Q6_K and ts["token_embd.weight"].type == L.IQ4_XS
        for il in range(hp.n_layer):
            for w in WEIGHTS:
                t = ts[f"blk.{il}.{w}.weight"].type
                assert t in ((L.IQ4_XS, L.Q5_K) if w in ("attn_v", "ffn_down") else (L.IQ4_XS,)), (il, w, t)
        assert any(ts[f"blk.{il}.attn_v.weight"].type == L.Q5_K for il in range(hp.n_layer))
    finally:
        m.free()
