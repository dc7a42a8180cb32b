// options.h — the backend's run-time switches and counters, each written once.  Standard library only (no HIP): tests/options_probe.cpp includes it from a plain C++ program.
//   MI_OPTIONS: the per-backend options (backend_ctx::opt).  A row gives the field, its default, how set_option stores a value and whether init_backend reads an
//               environment variable for it; struct options, options_from_env, options_set and operator== are generated from the rows.
//   MI_STATS:   the counters (backend_ctx::st) behind get_stat: struct stats and stats_find.
//   env_flag / env_int / env_present: the process-wide knobs, each read where it is used into a `static const` (once per process, not settable at run time).
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace mi355x {

#define MI_BF16_MMV_MAX_COLS 8  // default hand-over from the bf16 streaming kernel's multi-column form to the 16 x 16 tiles (option bf16_mmv_max_cols)
#define MI_BF16_NT 1            // default load policy of the bf16 streaming kernel: non-temporal (option bf16_nt / GGML_MI355X_BF16_NT)
#define MI_BF16_PREROUND 1      // default of option bf16_preround: on (measured 1.25 - 1.45 x faster at 512 and 2048 columns: profiles/r09_bf16_bench.txt)

// X(type, name, default, flag, env)
//   name: the field of struct options and the set_option key
//   flag: 1 = a write stores value != 0, 0 = the value as given
//   env:  1 = init_backend reads GGML_MI355X_<NAME in upper case>, 0 = no environment variable
#define MI_OPTIONS(X)                                                                                                                                                    \
    X(bool, graphs, true, 1, 1)        /* hipGraph capture + replay of repeated graphs */                                                                                \
    X(bool, fusion, true, 1, 1)        /* node fusion (norm+mul, mul_mat+add, ...) */                                                                                    \
    X(bool, prologue, true, 1, 1)      /* fold RMS_NORM / activation quantisation into the mat-vec prologue */                                                           \
    X(bool, qkv, true, 1, 1)           /* fused Q/K/V + rope + cache store launch */                                                                                     \
    X(int, mmvq_max_cols, 2, 0, 1)     /* widest batch that takes the mat-vec fusions (gate/up/SwiGLU, +bias +residual in one launch); from three columns on the
                                          skinny matrix-core kernel + its separate SwiGLU launch is faster (-np 8 step 4.06 -> 3.45 ms, -np 3 3.77 -> 3.35) */         \
    X(int, mmq_min_cols, 3, 0, 1)      /* batches at least this wide run on the matrix cores (measured, ms/step matrix cores vs multi-column mat-vec: 3 columns 4.1 / 4.4, 4: 3.9 / 4.2, 8: 4.4 / 5.7; 2 columns: 3.6 / 3.1) */ \
    X(bool, mmq_i8, true, 1, 1)        /* Q4_K/Q5_K batches on the int8 matrix cores (mmq_i8.hip) instead of the f16 variant (mmq.hip) */                                \
    X(bool, mm_merge, true, 1, 1)      /* batches: sibling mat-muls over the same activations (wq/wk/wv, gate/up) as one launch */                                       \
    X(bool, ss_partials, true, 1, 1)   /* residual-stream mat-vecs leave the sum of squares of their result for the next RMS_NORM prologue (GGML_MI355X_SS_PARTIALS=0: off) */ \
    X(bool, fa_self_merge, false, 1, 1) /* split attention (decode): the last split workgroup merges the partial records, no combine launch.  Off: measured
                                          one token, n_kv 2100: 16.5 us against 7.6 + 5.0 for split + combine (record write-through, counter and re-read are a longer
                                          dependent chain than a launch); -np 32: 18.3 against 19.6 us per layer (4.45 vs 4.49 ms per step) */                          \
    X(bool, attn_nf, true, 1, 1)       /* -np decode steps on the non-flash path: K.q -> SOFT_MAX -> V^T.p as one launch over the tokens' visible-cell lists (attn_nf.hip) */ \
    X(bool, softmax_mm, true, 1, 1)    /* decode on the non-flash path: SOFT_MAX folded into the V^T.p product that reads it (mmf.hip) */                                \
    X(bool, skinny_rope, true, 1, 1)   /* -np decode steps: ROPE(q), ROPE(k) and both KV-cache stores in the epilogue of the skinny QKV launch(es) */                    \
    X(bool, skinny_mix, true, 1, 1)    /* -np decode steps: sibling mat-muls stored in two K-quant formats (Q4_K wq / wk + Q6_K wv) share one skinny launch */           \
    X(bool, mmq_skinny, true, 1, 1)    /* 2..32 columns: weight-streaming matrix-core kernel (mmq_skinny.hip) instead of the tiled GEMM */                               \
    X(int, mmq_bn, 0, 0, 1)            /* force the weight-panel height of mmq_i8 (64 / 128); 0 = pick by grid size */                                                   \
    /* bf16 weight matrices (mmbf.hip) */                                                                                                                  \
    X(int, bf16_form, -1, 0, 1)        /* -1: routed; MI_BF16_DOT .. MI_BF16_MMA: that form wherever it can serve the operands (measurements and tests) */               \
    X(int, bf16_mmv_max_cols, MI_BF16_MMV_MAX_COLS, 0, 1) /* widest batch on the streaming kernel; wider ones go to the matrix cores */                                  \
    X(int, bf16_nt, MI_BF16_NT, 1, 1)  /* non-temporal weight loads in the streaming kernel */                                                                           \
    X(int, bf16_preround, MI_BF16_PREROUND, 1, 1) /* batches on the 32 x 32 tiles: src1 rounded to bf16 once into scratch instead of in every workgroup's loop */        \
    X(int, fa_splits, 0, 0, 1)         /* 0 = auto */                                                                                                                    \
    X(bool, fa_wo, false, 1, 1)        /* decode: attention as few fat splits whose merge is the wo mat-vec's prologue (no combine launch).  Correct and
                                          tested, OFF by default: a KV trip of the lane-parallel kernel is a ~4 us dependent chain, so 9 splits of 2
                                          trips (12.0 us) + the merging prologue (wo 6.8 -> 10.4 us) lose to 36 one-trip splits + combine (13.6 + 6.8) */               \
    X(bool, small_uploads, true, 1, 1) /* set_tensor_async of <= 64 KiB: pinned ring + copy kernel instead of a blit */                                                  \
    X(bool, small_downloads, true, 1, 1) /* get_tensor_async of <= 8 MiB into this backend's pinned host buffer type: a copy kernel instead of a blit */                 \
    X(bool, timing, false, 1, 0)       /* hipEvent-bracket kernel classes (bench only; disables graphs) */                                                               \
    X(int, decode_copy_headroom_gib, 2, 0, 0) /* a buffer's decode copy is made only while this much device memory stays free beside it (tests raise it to force the fallback) */ \
    X(bool, decode_copy, true, 1, 1)   /* batch-1 mat-vecs read the plane-layout copy of their weights */                                                                \
    X(int, exec_update, 1, 0, 1)       /* patch the predecessor's executable graph at a capture at
                                          first sighting (graph.cpp); 2 = run the update and treat it as failed (tests) */                                               \
    X(int, shadow_capture, 1, 0, 1)    /* a capture at first sighting runs BEHIND the step's own eager launches */                                                       \
    X(int, q80_min_cols, 33, 0, 1)     /* Q8_0 weights: batches of at least this many columns take the matrix-core GEMM (mmq_q80.hip), smaller ones 8-column mat-vec passes */

// One per-backend switch is kept beside the table: ssm_fuse (backend_ctx::ssm_fuse, default on, GGML_MI355X_SSM_FUSE, set_option("ssm_fuse", 0 / 1)): SSM_CONV ->
// ADD(bias) -> SILU as one launch.  tests/test_options_host.py holds the table's rows as a written-down contract that is extended on purpose, in a change of its own;
// until then the switch is no row: backend.cpp reads the variable and stores the value next to the keys that are no field of c->opt.
// mmid_bias (backend_ctx::mmid_bias, default on, GGML_MI355X_MMID_BIAS, set_option("mmid_bias", 0 / 1)) is kept the same way: MUL_MAT_ID -> ADD_ID as one launch, the bias
// added in the store (graph.cpp, mmid.hip).
// conv_mma (backend_ctx::conv_mma, default 1, GGML_MI355X_CONV_MMA, set_option("conv_mma", 0 / 1 / 2)) likewise: MUL_MAT f16 x f16, the product behind an IM2COL.
// 1: on the matrix cores where the shape is routed there; 0: the dot form everywhere; 2: the matrix cores wherever the operands allow (A/B runs, tests; conv.hip).
// gn_form (backend_ctx::gn_form, default 0, GGML_MI355X_GN_FORM, set_option("gn_form", 0 / 1 / 2)) likewise: which of GROUP_NORM's two forms serves a node.
// 0: routed by the group's length; 1: the resident form wherever a group fits it; 2: the split form everywhere (A/B runs, tests; diffusion.hip).

struct options {
#define MI_X(type, name, def, flag, env) type name = def;
    MI_OPTIONS(MI_X)
#undef MI_X
};
inline bool operator==(const options & a, const options & b) {
#define MI_X(type, name, def, flag, env) &&a.name == b.name
    return true MI_OPTIONS(MI_X);
#undef MI_X
}
// set_option: false = no option of that name (nothing changed)
inline bool options_set(options & o, const char * key, int value) {
#define MI_X(type, name, def, flag, env) \
    if (strcmp(key, #name) == 0) { o.name = flag ? (type) (value != 0) : (type) value; return true; }
    MI_OPTIONS(MI_X)
#undef MI_X
    return false;
}
inline std::string option_env_name(const char * key) {
    std::string s = "GGML_MI355X_";
    for (; *key; ++key) s += (char) toupper((unsigned char) *key);
    return s;
}
// init_backend: the environment over the defaults, parsed as set_option parses its value
inline void options_from_env(options & o) {
#define MI_X(type, name, def, flag, env) \
    if (env) if (const char * e = getenv(option_env_name(#name).c_str())) options_set(o, #name, atoi(e));
    MI_OPTIONS(MI_X)
#undef MI_X
}

// X(name): an int64_t counter, zero at init_backend; the name is the get_stat key
#define MI_STATS(X)                                                                                                                                                      \
    X(graph_launches) X(graph_captures) X(eager_graphs) X(kernel_launches) X(fused_nodes) X(allreduces)                                                                  \
    X(p2p_allreduces)             /* row-parallel sums served by the one-shot peer-to-peer kernel (tp_p2p.hip) instead of RCCL */                                        \
    X(ss_handoffs)                /* RMS_NORM prologues that took the sum of squares from the producing mat-vec's partial sums */                                        \
    X(skinny_launches)            /* mat-muls of 2..32 columns served by the weight-streaming matrix-core kernel */                                                      \
    X(mmid_launches)              /* MUL_MAT_ID nodes served by the expert mat-vec launch (mmid.hip), one launch a node */                                               \
    X(wide_launches)              /* prompt-batch mat-muls served by its wide form */                                                                                    \
    X(tiled_launches)             /* batch mat-muls served by the LDS-tiled int8 GEMM (mmq_i8.hip) */                                                                    \
    X(nf_mma_chains)              /* non-flash K.q -> SOFT_MAX -> V^T.p chains of a prompt micro-batch served by the two-pass matrix-core kernel (round 4) */            \
    X(nf_list_chains)             /* ... and those of a 2..32-token batch served by the one-launch list kernel (attn_nf.hip) */                                          \
    X(fa_form)                    /* kernels.h fa_form_code of the last FLASH_ATTN_EXT node of the graph computed last (0: it had none) */                               \
    X(fa_list_launches)           /* FLASH_ATTN_EXT nodes served over per-token position lists (2..32 tokens; 33..256 when the mask is known to be sparse) */            \
    X(rope_epilogues)             /* batches whose rope + KV-cache stores rode in the skinny QKV launches */                                                             \
    X(graph_launch_host_ns)       /* host time spent inside hipGraphLaunch (replays only) */                                                                             \
    X(graph_key_host_ns)          /* replays only: host time from entering graph_compute to calling hipGraphLaunch (recognising the graph) */                            \
    X(graph_compute_host_ns)      /* host time inside graph_compute, all paths */                                                                                        \
    X(graph_key_fast_hits)        /* replays recognised by comparing against the graph replayed last (no key built, no hash) */                                          \
    X(kv_native_nodes)            /* ... and those whose K / V in such a type were read in place by the lane-parallel kernel's DQ form */                                \
    X(kv_image_nodes)             /* FLASH_ATTN_EXT nodes whose K / V (kept in q4_0, q4_1, q5_0, q5_1, iq4_nl, bf16, f32 ...) were read through an f16 image */          \
    X(kernel_downloads)           /* get_tensor_async calls served by a copy kernel writing mapped pinned memory */                                                      \
    X(graph_early_captures)       /* graphs captured at their FIRST sighting (same step as the one replayed last, over a grown cache) */                                 \
    X(graph_shadow_captures)      /* ... of which the capture ran behind the step's own eager launches (the GPU busy meanwhile) and serves the NEXT step */              \
    X(graph_capture_walk_ns) X(graph_exec_update_ns) X(graph_shadow_eager_ns) /* host time of: the walk into a capture (begin..end), hipGraphExecUpdate / instantiate, a shadow capture's eager walk */ \
    X(graph_exec_updates)         /* ... of them, served by patching the predecessor's executable graph (hipGraphExecUpdate) instead of instantiating */                 \
    X(decode_copy_tensors)        /* weight matrices repacked into the decode copy by this backend instance ... */                                                       \
    X(decode_copy_bytes)          /* ... and their bytes */                                                                                                              \
    X(decode_copy_launches)       /* mat-vec / fused Q/K/V launches that streamed a decode copy */                                                                       \
    X(elided_conts)               /* cont(permute(kqv)) copies of a one-token non-flash attention whose bytes the producing launch wrote in place (round 6) */           \
    X(step_heads)                 /* decode-step heads served by one launch: GET_ROWS + mask cast + rotary table (ops.hip: k_step_head) */                               \
    X(graph_exec_update_failures) /* ... and updates that failed: the predecessor's (possibly half-patched) executable graph is destroyed, both entries start over */    \
    X(graph_evictions)            /* cache entries dropped because they had not been used for 256 graphs */                                                              \
    X(graph_key_collisions)       /* two different graph keys with one hash (each keeps its own entry) */

struct stats {
#define MI_X(name) int64_t name = 0;
    MI_STATS(MI_X)
#undef MI_X
};
// get_stat: the counter of that name, or nullptr
inline const int64_t * stats_find(const stats & s, const char * key) {
#define MI_X(name) if (strcmp(key, #name) == 0) return &s.name;
    MI_STATS(MI_X)
#undef MI_X
    return nullptr;
}

// Process-wide knobs: GGML_MI355X_* variables that are no backend option.
inline bool env_flag(const char * name, bool dflt) { const char * e = getenv(name); return e ? atoi(e) != 0 : dflt; }  // unset: dflt; otherwise its number != 0
inline int env_int(const char * name, int dflt) { const char * e = getenv(name); return e ? atoi(e) : dflt; }
inline bool env_present(const char * name) { return getenv(name) != nullptr; }  // set to anything, "0" and "" included (the DBG_* switches)

}  // namespace mi355x
