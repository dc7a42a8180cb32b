"""The keys hosts pass to ggml_backend_mi355x_set_option / _get_stat, as the hand-written arms of backend.cpp spelled them before options and counters
became tables (csrc/options.h).  Written out here on purpose: a key that disappears from the tables must fail this file."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

# key -> default.  Left out: tp_p2p, tp_p2p_reset and clear_failure, which act on state instead of storing a value.
OPTION_DEFAULTS = {
    "graphs": 1, "fusion": 1, "prologue": 1, "qkv": 1, "mmvq_max_cols": 2, "mmq_min_cols": 3, "mmq_i8": 1, "mm_merge": 1, "mmq_bn": 0,
    "bf16_form": -1, "bf16_mmv_max_cols": 8, "bf16_nt": 1, "bf16_preround": 1, "mmq_skinny": 1, "skinny_rope": 1, "skinny_mix": 1,
    "softmax_mm": 1, "attn_nf": 1, "fa_self_merge": 0, "ss_partials": 1, "fa_splits": 0, "fa_wo": 0, "small_uploads": 1, "small_downloads": 1,
    "timing": 0, "exec_update": 1, "shadow_capture": 1, "q80_min_cols": 33, "decode_copy": 1, "decode_copy_headroom_gib": 2, "staged_upload": 0,
}
STAT_KEYS = [
    "graph_launches", "graph_captures", "eager_graphs", "kernel_launches", "fused_nodes", "allreduces", "ss_handoffs", "fa_list_launches", "fa_form",
    "nf_mma_chains", "nf_list_chains", "p2p_allreduces", "p2p_timeouts", "step_heads", "elided_conts", "decode_copy_tensors", "decode_copy_bytes", "decode_copy_launches",
    "graph_exec_update_failures", "graph_evictions", "graph_cache_size", "graph_launch_host_ns", "kernel_downloads", "kv_image_nodes", "kv_native_nodes",
    "graph_key_host_ns", "graph_compute_host_ns", "graph_key_fast_hits", "graph_key_collisions", "graph_early_captures", "graph_shadow_captures",
    "graph_capture_walk_ns", "graph_exec_update_ns", "graph_shadow_eager_ns", "graph_exec_updates", "skinny_launches", "mmid_launches", "wide_launches",
    "tiled_launches", "rope_epilogues", "staged_upload_bytes", "staged_upload_us",
    # the ip_ prefix (the in-process tensor-parallel engine's counters): 0 on a backend that has no engine
    "ip_graphs", "ip_declined", "ip_plans", "ip_input_copies", "ip_output_copies", "ip_kv_gathers", "ip_kv_scatters", "ip_devices", "ip_worker_kernel_launches",
]
# keys that answer -1 on a single-device backend: none (p2p_timeouts is 0 without a group, every ip_ key 0 without an engine)
STAT_MINUS_ONE = []


def test_every_option_key_is_accepted(backend):
    fn = backend.proc("ggml_backend_mi355x_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p])
    try:
        for key, default in OPTION_DEFAULTS.items():
            assert fn(backend.backend, key.encode(), str(default).encode()) == 0, key
        for key in ("no_such_option", "", "GRAPHS", "graphs "):
            assert fn(backend.backend, key.encode(), b"1") == -1, key
    finally:
        for key, default in OPTION_DEFAULTS.items():
            fn(backend.backend, key.encode(), str(default).encode())


def test_every_stat_key_is_known(backend):
    for key in STAT_KEYS:
        v = backend.stat(key)
        assert (v == -1) if key in STAT_MINUS_ONE else (v != -1), (key, v)
    for key in ("no_such_stat", "", "ip_no_such_stat", "GRAPH_LAUNCHES"):
        assert backend.stat(key) == -1, key
