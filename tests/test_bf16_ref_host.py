"""CPU-side tests for models stored in bf16: the NumPy rounding of tests/bf16_ref.py against the oracle's, the model generator's new file type, presets and
bf16 recipe, the oracle on test-llama-bf16 end to end, and the decisiveness of the greedy-id gate tests/test_gpu_bf16_weights.py applies with the same seed."""
import ctypes as C

import numpy as np
import pytest

import bf16_ref as B
import harness as T
import llama_box_amd as L
from model_util import Context, Model, greedy, preset

WEIGHTS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def _oracle_bf16(x):
    lib = T.oracle()
    return np.array([lib.oracle_fp32_to_bf16(C.c_float(float(v))) for v in x], dtype=np.uint16)


def test_to_bf16_equals_the_oracles_rounding():
    x = B.READBACK_VALUES
    assert np.array_equal(B.to_bf16(x), _oracle_bf16(x))
    rng = np.random.default_rng(5)
    u = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]  # NaNs excluded (a float passed by value may not keep a signalling NaN's bits)
    x = u.view(np.float32)
    assert x.size > 99000
    assert np.array_equal(B.to_bf16(x), _oracle_bf16(x))
    assert np.array_equal(B.from_bf16(B.to_bf16(x[:1000])), np.array([T.oracle().oracle_bf16_to_fp32(int(h)) for h in B.to_bf16(x[:1000])], dtype=np.float32))
    # ties go to the even upper half, one ulp either side of a tie goes to the nearer one, NaN stays a quiet NaN
    t = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7FC00001, 0xFF800001], dtype=np.uint32).view(np.float32)
    assert B.to_bf16(t).tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x7FC0, 0xFFC0]


def test_new_presets_and_file_type():
    assert L.LLM_FTYPE_BF16 == 16
    for name, like in (("test-llama-bf16", "test-llama"), ("test-qwen2-bf16", "test-qwen2")):
        k, t = preset(name), preset(like)
        assert k.ftype == 16
        for f in ("n_layer", "n_embd", "n_head", "n_head_kv", "n_embd_head", "n_ff", "n_vocab", "qkv_bias", "rope_type"):
            assert getattr(k, f) == getattr(t, f), (name, f)
    a, b = preset("tinyllama-1.1b-bf16"), preset("llama3-8b-bf16")
    assert (a.ftype, a.n_layer, a.n_embd, a.n_ff, a.n_vocab) == (16, 22, 2048, 5632, 32000)
    assert (b.ftype, b.n_layer, b.n_embd, b.n_ff, b.n_vocab, b.n_head_kv) == (16, 32, 4096, 14336, 128256, 8)
    assert preset("test-llama-kq23").ftype == 15 and preset("test-llama").ftype == 5 and preset("test-qwen2").ftype == 5  # (earlier values stay)


def test_every_matrix_of_the_bf16_model_is_bf16_and_the_recipe_is_the_rounded_f16_draw():
    H = L.host()
    hp = preset("test-llama-bf16")
    m, m2 = Model(hp, B.MODEL_SEED, H.ggml_backend_cpu_buffer_type()), Model(hp, B.MODEL_SEED, H.ggml_backend_cpu_buffer_type())
    try:
        names = ["token_embd.weight", "output.weight"] + [f"blk.{il}.{w}.weight" for il in range(hp.n_layer) for w in WEIGHTS]
        for n in names:
            t, t2 = (H.llm_model_tensor(x.m, n.encode()).contents for x in (m, m2))
            assert t.type == L.BF16 and t.nb[0] == 2 and t.nb[1] == 2 * t.ne[0], n
            assert np.array_equal(B.host_rows(t), B.host_rows(t2)), n  # deterministic
        for il in range(hp.n_layer):
            for n in ("attn_norm", "ffn_norm"):
                assert H.llm_model_tensor(m.m, f"blk.{il}.{n}.weight".encode()).contents.type == L.F32
        # tensor ids in plan order: token_embd 0; layer il: attn_norm 1 + 9 il, then q, k, v, attn_output, ffn_norm, gate, up, down
        for name, tid, gain in (("token_embd.weight", 0, np.sqrt(np.float32(hp.n_embd))), ("blk.0.attn_q.weight", 2, 1.0), ("blk.1.ffn_down.weight", 1 + 9 + 8, 0.25)):
            t = H.llm_model_tensor(m.m, name.encode()).contents
            rows = B.host_rows(t)[:3]
            draw = B.synth_draw(B.MODEL_SEED, tid, 3, t.ne[0], gain)
            assert np.array_equal(rows, B.to_bf16(draw)), name
            assert np.any(rows != (draw.view(np.uint32) >> 16).astype(np.uint16))  # (rounded: some values differ from their truncation)
        # rows of unit-order norm (the embeddings carry a sqrt(n_embd) gain)
        w = B.from_bf16(B.host_rows(H.llm_model_tensor(m.m, b"blk.0.ffn_gate.weight").contents)).astype(np.float64)
        rms = float(np.sqrt(np.mean(w ** 2)) * np.sqrt(w.shape[1]))
        assert 0.8 < rms < 1.2 and abs(float(np.mean(w))) * np.sqrt(w.shape[1]) < 0.2, rms
    finally:
        m.free()
        m2.free()


def test_a_peaked_bf16_output_matrix_ties_groups_of_32_to_the_embeddings():
    """The "-damped" weight set of a bf16 model (what the benchmark runs): 3 of every 8 groups of 32 values of output row r are token_embd's row
    (7919 r + 13) mod n_vocab scaled by 1 / sqrt(n_embd), up to the bf16 rounding."""
    H = L.host()
    hp = preset("test-llama-bf16-damped")
    assert hp.peaked == 3 and hp.ftype == 16
    m = Model(hp, 7, H.ggml_backend_cpu_buffer_type())
    try:
        emb = B.from_bf16(B.host_rows(H.llm_model_tensor(m.m, b"token_embd.weight").contents))
        out = B.from_bf16(B.host_rows(H.llm_model_tensor(m.m, b"output.weight").contents))
        E, V = hp.n_embd, hp.n_vocab
        tied = 0
        for r in range(0, V, 37):
            src = emb[(r * 7919 + 13) % V] / np.sqrt(np.float32(E))
            for g in range(E // 32):
                a, b = out[r, 32 * g:32 * g + 32], src[32 * g:32 * g + 32]
                tied += bool(np.all(np.abs(a - b) <= np.abs(b) * 2.0 ** -7 + 1e-30))
        n = len(range(0, V, 37)) * (E // 32)
        assert 0.25 * n < tied < 0.5 * n, (tied, n)
    finally:
        m.free()


def test_oracle_runs_the_bf16_model_end_to_end():
    H = L.host()
    m = Model(preset("test-llama-bf16"), B.MODEL_SEED, H.ggml_backend_cpu_buffer_type())
    try:
        runs = []
        for fa in (0, 1):
            c = Context(m, compute=T.oracle_compute_fn(), flash_attn=fa)
            ids, rows = greedy(c, B.PROMPT40[:8], 3)
            runs.append((ids, np.stack(rows)))
            c.free()
        assert np.all(np.isfinite(runs[0][1])) and float(np.std(runs[0][1])) > 0
        assert T.nmse(runs[1][1], runs[0][1]) < 1e-3  # (flash attention and the soft-max path agree as far as two summation orders do)
    finally:
        m.free()


@pytest.mark.parametrize("name", ["test-llama-bf16", "test-qwen2-bf16"])
def test_at_least_half_of_the_decode_positions_are_decisive_under_the_oracles_own_yardstick(name):
    """The greedy-id gate of the GPU model test binds only where the oracle's top-2 margin exceeds twice its own order sensitivity: with the seed that test uses,
    at least half of the 16 + 1 positions must be such — decided on the oracle alone."""
    H = L.host()
    margins, yard = B.oracle_margins_and_yardstick(H, name)
    decisive = int(np.sum(margins > yard))
    print(f"{name}: yardstick {yard:.3e}, margins {np.sort(margins)}, decisive {decisive}/{len(margins)}")
    assert len(margins) == B.N_GEN == 17
    assert 2 * decisive >= len(margins), (decisive, yard, margins)
