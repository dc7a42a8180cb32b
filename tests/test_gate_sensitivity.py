"""CPU-only: does the full-depth parity gate of tests/test_gpu_full_depth.py (north_star's bar as written: max|d| <= 1e-3 of the logit range on the damped + peaked weight
sets) trip when it should — and pass when it should?  The oracle is run against ITSELF with a known fault injected (oracle_set_variant 5 / 6, oracle/ggml_cpu_ref.c):

  * the logits scaled by 1 + 4e-3 (an error in the output path)  ->  the gate's metric must exceed the bar;
  * another f32 summation order (what any second correct implementation is) ->  the metric must stay inside the bar, at Llama-3-8B's layer shapes and damped gain;
  * every layer's FFN branch scaled by 1 + 1e-2 ->  logged: on a damped set the layers carry a small share of the logit spread, so THIS gate does not see a 1 % error
    inside the layers (DESIGN.md section 2 says so; the per-op and per-layer teacher-forced gates do) — the test pins that the statement is true, not that it is good.
"""
import ctypes as C

import numpy as np

import harness as T
import llama_box_amd as L
from model_util import Context, Model, preset


def _rows(mc, prompt, fast, variant):
    lib = T.oracle()
    lib.oracle_set_fast.restype = C.c_int
    lib.oracle_set_fast(fast)
    lib.oracle_set_variant(variant)
    try:
        c = Context(mc, compute=T.oracle_compute_fn(T.host_threads(16)), flash_attn=1, n_ctx=256, n_threads=T.host_threads(16))
        try:
            rc, lg = c.decode(prompt, range(len(prompt)), want=[1] * len(prompt))
            assert rc == 0
            return lg
        finally:
            c.free()
    finally:
        lib.oracle_set_variant(0)
        lib.oracle_set_fast(0)


def test_the_bar_as_written_trips_on_an_output_path_error_and_passes_a_correct_second_implementation(built):
    H = L.host()
    hp = preset("llama3-8b-q4_k_m-damped", n_layer=4, n_vocab=8192)  # Llama-3-8B's layer shapes, formats and damped branch gain (0.01); 4 layers, 8 k vocabulary: ~1 GB
    rng = np.random.default_rng(5)
    prompt = rng.integers(3, hp.n_vocab, 12).tolist()
    mc = Model(hp, 11, H.ggml_backend_cpu_buffer_type())
    try:
        ref = _rows(mc, prompt, 0, 0)
        other_order = _rows(mc, prompt, 1, 2) if int(T.oracle().oracle_set_fast(1)) else _rows(mc, prompt, 0, 1)
        T.oracle().oracle_set_fast(0)
        out_fault = _rows(mc, prompt, 0, 5)
        ffn_fault = _rows(mc, prompt, 0, 6)
    finally:
        mc.free()
    span = float(ref.max() - ref.min())
    rel = lambda a: float(np.max(np.abs(a - ref))) / span
    top2 = np.sort(ref, axis=1)
    margin = top2[:, -1] - top2[:, -2]
    print(f"logit range {span:.1f}; max|d| / range: another summation order {rel(other_order):.2e}, logits x 1.004 {rel(out_fault):.2e}, every FFN branch x 1.01 {rel(ffn_fault):.2e}; "
          f"min / median top-2 margin {margin.min():.2f} / {np.median(margin):.2f}")
    assert rel(other_order) <= 1e-3, "a correct second implementation (another f32 summation order) fails the bar on the damped set"
    assert rel(out_fault) > 1e-3, "a 4e-3 error of the logits passes the bar: the gate has no teeth in the output path"
    assert np.array_equal(np.argmax(other_order, axis=1), np.argmax(ref, axis=1))
    # the documented limit: a 1 % error inside every layer stays below this gate on a damped set
    assert rel(ffn_fault) < rel(out_fault)
