"""CPU-side tests for models stored in Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL: the layouts (a NumPy twin of dequantize_row against the oracle),
the model generator's new file types and presets, and one legacy model decoded with the oracle as compute function."""
import numpy as np
import pytest

import harness as T
import legacy_ref as R
import llama_box_amd as L
from model_util import Context, Model, greedy, preset


@pytest.mark.parametrize("qt", R.FORMATS, ids=lambda q: L.TYPE_NAME[q])
def test_numpy_twin_matches_oracle_dequantize(qt):
    rng = np.random.default_rng(qt)
    b = R.rand_blocks(qt, 64, 256, rng)
    # ... and the corners: all nibbles 0 / 15, qh all ones, negative d, subnormal d, d = 0, negative and large m
    n5 = 31 if qt in R.FIVE else 15
    d = np.array([1.0, -0.5, 6e-8, 0.0, 0.25, 1e-3], dtype=np.float16)
    m = np.array([0.0, -3.0, 1.0, 2.0, 1000.0, -0.125], dtype=np.float16)
    lev = np.stack([np.zeros(32), np.full(32, 15), np.full(32, n5), np.arange(32) % (n5 + 1), np.full(32, 16 if qt in R.FIVE else 8), np.arange(32)[::-1] % (n5 + 1)]).astype(np.int64)
    b = np.concatenate([b, R.make_blocks(qt, d, m, lev)])
    assert np.array_equal(R.np_dequant(qt, b).view(np.uint32), R.oracle_dequant(qt, b).view(np.uint32))


def test_new_presets_resolve_and_old_ftype_values_stay():
    old = {"tinyllama-1.1b-q8_0": 0, "llama3-8b-q4_k_m": 1, "qwen2-7b-q5_k_m": 2, "test-llama": 5, "test-qwen2": 5}
    for name, ft in old.items():
        assert preset(name).ftype == ft, name
    a, b, c = preset("test-llama-legacy"), preset("test-qwen2-legacy"), preset("llama2-7b-q4_0")
    assert a.ftype == 11 and b.ftype == 11 and c.ftype == 6
    ta, tb = preset("test-llama"), preset("test-qwen2")
    for f in ("n_layer", "n_embd", "n_head", "n_head_kv", "n_embd_head", "n_ff", "n_vocab", "qkv_bias", "rope_type"):
        assert getattr(a, f) == getattr(ta, f) and getattr(b, f) == getattr(tb, f), f
    assert (c.n_layer, c.n_embd, c.n_ff, c.n_vocab) == (32, 4096, 11008, 32000)


def test_legacy_model_holds_every_format_and_decodes_on_the_oracle():
    H = L.host()
    hp = preset("test-llama-legacy")
    m = Model(hp, 1234, H.ggml_backend_cpu_buffer_type())
    names = ["token_embd.weight", "output.weight"] + [f"blk.{il}.{w}.weight" for il in range(hp.n_layer) for w in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")]
    types = {H.llm_model_tensor(m.m, n.encode()).contents.type for n in names}
    assert types == set(R.FORMATS) | {L.Q8_0}, types
    prompt = [1, 5, 9, 300, 17, 42, 99, 7]
    runs = []
    for _ in range(2):
        c = Context(m, compute=T.oracle_compute_fn(), flash_attn=0)
        ids, rows = greedy(c, prompt, 4)
        runs.append((ids, np.stack(rows)))
        c.free()
    m.free()
    assert np.all(np.isfinite(runs[0][1]))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    m2 = Model(hp, 1235, H.ggml_backend_cpu_buffer_type())
    c2 = Context(m2, compute=T.oracle_compute_fn(), flash_attn=0)
    _, rows2 = greedy(c2, prompt, 1)
    c2.free()
    m2.free()
    assert not np.array_equal(np.stack(rows2)[0], runs[0][1][0])  # another seed, another model


def test_gguf_file_in_the_legacy_formats_loads_as_the_in_memory_model(tmp_path):
    """llm_model_load takes the five types from a GGUF file: same tensor types, same logits as the model synthesised in memory."""
    H = L.host()
    hp = preset("test-llama-legacy")
    path = str(tmp_path / "legacy.gguf")
    assert H.llm_synth_gguf(hp, 4321, path.encode()) == 0
    m1 = Model(path=path, buft=H.ggml_backend_cpu_buffer_type())
    m2 = Model(hp, 4321, H.ggml_backend_cpu_buffer_type())
    try:
        for n in ("token_embd.weight", "blk.0.attn_q.weight", "blk.1.ffn_down.weight", "output.weight"):
            assert H.llm_model_tensor(m1.m, n.encode()).contents.type == H.llm_model_tensor(m2.m, n.encode()).contents.type, n
        rows = []
        for m in (m1, m2):
            c = Context(m, compute=T.oracle_compute_fn(), flash_attn=0)
            rc, lg = c.decode([1, 5, 9, 300, 17], range(5))
            assert rc == 0
            rows.append(lg)
            c.free()
        assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
    finally:
        m1.free()
        m2.free()
