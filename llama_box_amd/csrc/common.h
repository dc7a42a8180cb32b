// common.h — internal declarations shared by the backend's translation units (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ggml_mi355x.h"
#include "options.h"  // struct options, struct stats, env_flag / env_int / env_present

#define MI_LOG(level, ...)                                    \
    do {                                                      \
        if ((level) <= mi355x::log_level()) {                 \
            fprintf(stderr, "ggml-mi355x: " __VA_ARGS__);     \
            fprintf(stderr, "\n");                            \
        }                                                     \
    } while (0)
#define MI_ERR(...) MI_LOG(0, __VA_ARGS__)
#define MI_INFO(...) MI_LOG(1, __VA_ARGS__)
#define MI_DBG(...) MI_LOG(2, __VA_ARGS__)

// abort-on-error, the convention of every ggml backend for non-graph entry points (SURVEY.md §8b "Error conventions")
#define HIP_CHECK(expr)                                                                                         \
    do {                                                                                                        \
        hipError_t err_ = (expr);                                                                               \
        if (err_ != hipSuccess) {                                                                               \
            fprintf(stderr, "ggml-mi355x: HIP error %d (%s) at %s:%d: %s\n", (int) err_, hipGetErrorString(err_), __FILE__, __LINE__, #expr); \
            abort();                                                                                            \
        }                                                                                                       \
    } while (0)

// Entry points of the ggml interface that return no status (set_tensor, get_tensor, memset, cpy, clear, synchronize, events, free): upstream's
// backends abort() there.  llama-box is a server: a failed copy must not take every other request down with it.  The failure is logged,
// cleared and REMEMBERED (mi355x::hip_failed()): from then on every graph_compute of this process's backends returns GGML_STATUS_FAILED ->
// llama_decode rc < 0 -> the engine fails the affected requests (llama-box/httpserver.hpp:3541-3545) and the operator sees the log.
#define HIP_SOFT(expr)                                                                                          \
    do {                                                                                                        \
        hipError_t err_ = (expr);                                                                               \
        if (err_ != hipSuccess) {                                                                               \
            (void) hipGetLastError();                                                                           \
            fprintf(stderr, "ggml-mi355x: HIP error %d (%s) at %s:%d: %s — graph_compute will report failure from here on\n", (int) err_, \
                    hipGetErrorString(err_), __FILE__, __LINE__, #expr);                                        \
            mi355x::note_hip_failure();                                                                         \
        }                                                                                                       \
    } while (0)

// Bookkeeping calls that move no tensor data (event create / destroy / elapsed time of the bench's timing, frees in teardown, memory and property
// queries): a failure there is logged and cleared and NOTHING else — it must not brick inference for the rest of the process.
#define HIP_NOTE(expr)                                                                                          \
    do {                                                                                                        \
        hipError_t err_ = (expr);                                                                               \
        if (err_ != hipSuccess) {                                                                               \
            (void) hipGetLastError();                                                                           \
            fprintf(stderr, "ggml-mi355x: HIP error %d (%s) at %s:%d: %s (ignored: no tensor data involved)\n", (int) err_, hipGetErrorString(err_), __FILE__, __LINE__, #expr); \
        }                                                                                                       \
    } while (0)

// inside graph execution a HIP failure must fail ONE llama_decode (GGML_STATUS_FAILED -> rc -2, llama-box/httpserver.hpp:3541-3545),
// not the whole llama-box process: log, clear the sticky error, hand `ret` to the caller
#define HIP_TRY(expr, ret)                                                                                      \
    do {                                                                                                        \
        hipError_t err_ = (expr);                                                                               \
        if (err_ != hipSuccess) {                                                                               \
            (void) hipGetLastError();                                                                           \
            fprintf(stderr, "ggml-mi355x: HIP error %d (%s) at %s:%d: %s\n", (int) err_, hipGetErrorString(err_), __FILE__, __LINE__, #expr); \
            return ret;                                                                                         \
        }                                                                                                       \
    } while (0)

namespace mi355x {

int log_level();
void note_hip_failure();  // backend.cpp: a data-path HIP call failed outside graph execution (HIP_SOFT)
bool hip_failed();
void clear_hip_failure();  // set_option("clear_failure", 1): the operator's way back without a restart (the log says what failed)

// device-side layout of a Q8_K-quantised activation block (the ggml block_q8_K fields, 16-byte aligned:
// qs | bsums | d) — produced by quantize kernels, consumed by the K-quant matvec / GEMM kernels
// small host -> device uploads batched into one launch (ops.hip: k_upload_multi)
struct upload_seg { char * dst; const char * src; size_t n; };
struct upload_batch { upload_seg seg[8]; int n; };

struct q8k_dev {
    int8_t qs[256];
    uint16_t bsums[16]; // block_q8_K.bsums (sums over 16 values, |.| <= 2032) stored as IEEE f16 — exact — because their only
                        // readers are the matrix-core GEMMs, which feed them to an f16 MFMA as they are
    int16_t bs32[8];    // sums over 32 values (what the Q4_K/Q5_K mins term needs per sub-block)
    float d;
    float pad[3];
};
static_assert(sizeof(q8k_dev) == 320, "q8k_dev");
// Q8_0-quantised activation block for Q8_0 weights: d already rounded through fp16 (as block_q8_0.d is)
struct q80_dev {
    int8_t qs[32];
    float d;
};
static_assert(sizeof(q80_dev) == 36, "q80_dev");
// Q8_1-quantised activation block for Q4_1 / Q5_1 weights: a q80_dev plus block_q8_1.s = f16(sum(qs) * d) taken with the UNROUNDED d = amax / 127, as
// quantize_row_q8_1_ref does — it cannot be rebuilt from the stored (f16-rounded) d, so the quantiser emits it
struct q81_dev {
    int8_t qs[32];
    float d;
    float s;
};
static_assert(sizeof(q81_dev) == 40, "q81_dev");

struct backend_ctx;

struct tp_state;      // tp.cpp
struct split_helper;  // split.cpp
struct ip_engine;     // tp_inproc.cpp

struct cached_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int seen = 0;
    uint64_t last_use = 0;
    int64_t allreduces = 0;  // reductions / collectives recorded in the graph (counted again at every replay: stats::allreduces)
    int n_nodes = 0;
    int fa_form = 0;  // stats::fa_form as the capture walk left it (reported again at every replay)
    bool early_failed = false;  // a capture at first sighting was tried and failed (graph.cpp)
    std::vector<uint64_t> key;  // the graph this entry stands for, word by word (graph.cpp: walk_key) — an entry is used only when these are equal
};

struct timing_slot {
    double total_ms = 0;
    int64_t count = 0;
};

struct backend_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string name;
    options opt;
    stats st;
    // scratch (quantised activations, attention partials); grown outside capture only
    void * ws = nullptr;
    size_t ws_size = 0;
    // activation-quantisation cache: which src1 tensor the q8 scratch currently holds
    const void * q8_src = nullptr;
    int q8_kind = 0;
    size_t q8_bytes = 0;
    uint64_t q8_epoch = 0;
    // hipGraph cache
    std::unordered_map<uint64_t, cached_graph> graphs;
    cached_graph * last_graph = nullptr;  // the entry looked up last: compared first, in place (graph.cpp: key_equals)
    std::vector<uint64_t> key_scratch;
    uint64_t tick = 0;
    uint64_t decode_epoch = 0;  // decode_copy_epoch() the cached graphs were captured under
    bool capturing = false;
    bool ssm_fuse = true;      // SSM_CONV -> ADD(bias) -> SILU as one launch (set_option "ssm_fuse" / GGML_MI355X_SSM_FUSE; options.h says why it is no row of MI_OPTIONS)
    int conv_mma = 1;          // MUL_MAT f16 x f16 (the product behind an IM2COL): 1 = the matrix cores where the shape is routed there, 0 = the dot form everywhere, 2 = the matrix cores wherever the operands allow (set_option "conv_mma" / GGML_MI355X_CONV_MMA; beside the table as ssm_fuse is)
    int gn_form = 0;           // GROUP_NORM: 0 = routed (diffusion.hip: group_norm_runs_resident), 1 = the resident form wherever a group fits it, 2 = the split form everywhere (set_option "gn_form" / GGML_MI355X_GN_FORM; beside the table as ssm_fuse is)
    bool mmid_bias = true;     // MUL_MAT_ID -> ADD_ID as one launch, the bias in the store (set_option "mmid_bias" / GGML_MI355X_MMID_BIAS; kept beside the table as ssm_fuse is)
    bool mm_q5_major = false;  // the graph being planned / run holds more Q5_K than Q4_K weight bytes (graph.cpp: mmq_min_cols_for)
    // tensor parallel
    tp_state * tp = nullptr;
    ip_engine * ip = nullptr;  // -sm row served as in-process tensor parallelism (tp_inproc.cpp); owned by the main device's backend
    // -sm row: per owning device a stream / scratch / event for the slices of row-split weights (split.cpp), created on first use
    std::vector<split_helper *> split_helpers;
    hipEvent_t split_ready = nullptr;  // "the activations of this split mat-mul exist on the main stream"
    // small host->device uploads (token ids, positions, cache indices, one mask row): staged in a pinned ring and moved by a
    // tiny kernel — a blit through hipMemcpyAsync costs ~25 us of stream time per copy, five of them per decode step
    char * up_ring = nullptr;
    size_t up_cap = 0, up_head = 0;
    upload_batch up_pending{};  // staged in the ring, not yet launched: flushed as ONE kernel before anything else enters the stream
    // attention over a unified cache with a few query tokens: per-token lists of visible tiles (fattn.hip, k_fattn_tile_scan),
    // built once per graph execution and shared by the attention nodes of all layers
    double * ss_buf = nullptr;       // 256 partial sums of squares: from the mat-vec that writes a residual stream to the norm prologue that reads it (mmvq_args::ss_out)
    unsigned * fa_arrive = nullptr;  // arrival counters of the self-merging attention splits (zero between launches)
    static constexpr int fa_arrive_slots = 16384;
    float * rope_tab = nullptr;   // (cos, sin) per (token, rotation pair) of a small batch: written once per graph run, read by every layer's QKV epilogue
    static constexpr int rope_tab_floats = 4096 * 256;  // (cos, sin) of up to 4096 tokens x 128 pairs (round 4: prompt micro-batches use the table too)
    uint16_t * act_tab = nullptr;  // T_gelu[65536] then T_quick[65536], f16 bits: ggml-cpu's GELU / GELU_QUICK tables, built on the host and uploaded before the first graph that needs them (graph.cpp: ensure_act_tables)
    int * fa_lists = nullptr;
    size_t fa_lists_bytes = 0;
    // per-class kernel timing (bench)
    std::map<std::string, timing_slot> timing;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> pending_events;
};

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (kernel, DEVICE) pair: llama-box's usual multi-GPU mode is one process
// driving several MI355X, so "raised once per process" would leave every device but the first at the 64 KB default and its launches
// failing.  `done` is one bit per device ordinal, owned by the launcher of that kernel instantiation.
inline bool ensure_dyn_lds(const void * kernel, size_t bytes, std::atomic<uint32_t> & done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 0;
    const uint32_t bit = 1u << dev;
    if (done.load(std::memory_order_acquire) & bit) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes) != hipSuccess) {
        (void) hipGetLastError();
        MI_ERR("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %zu) failed on device %d", bytes, dev);
        return false;
    }
    done.fetch_or(bit, std::memory_order_release);
    return true;
}

void flush_uploads(backend_ctx * c);  // launches the small uploads staged by set_tensor_async (backend.cpp)

// ---- buffers (backend.cpp) ----
struct buffer_ctx {
    int device = 0;
    void * base = nullptr;
    size_t size = 0;
    bool rowpar = false;  // tensor-parallel reducing buffer type
    // THE DECODE COPY (round 6; repack.hip, mmvq_types.h): a weights buffer's K-quant matrices a second time, in the plane layout the batch-1 mat-vec kernels stream
    // with non-temporal loads — same size, a tensor's copy sits at the tensor's own offset.  Allocated at the first use by a graph (never for buffers that are not
    // usage WEIGHTS), a tensor's copy written then too; anything that writes into the buffer afterwards drops the copies it overlaps (and every captured graph).
    void * shadow = nullptr;
    bool shadow_failed = false;
    std::mutex sh_mtx;
    std::unordered_map<size_t, size_t> sh_valid;  // offset of a repacked tensor -> its bytes
};
// the plane-layout copy of weight matrix w for the batch-1 mat-vec kernels, or nullptr (no copy: views, split / row-parallel buffers, option off,
// allocation failed, or asked during a capture for a tensor not yet repacked)
const uint8_t * decode_copy(backend_ctx * c, const ggml_tensor * w);
const uint8_t * q80_panel_copy(backend_ctx * c, const ggml_tensor * w);  // a Q8_0 matrix's panel copy (mmq_q80.hip: the 9 .. 32-column kernel), or nullptr
uint64_t decode_copy_epoch();  // bumped whenever a copy was dropped: graphs captured before hold pointers to it
bool buffer_is_ours(ggml_backend_buffer_t b);
bool buffer_is_rowpar(ggml_backend_buffer_t b);
ggml_backend_buffer_t make_backend_buffer(ggml_backend_buffer_type_t buft, const ggml_backend_buffer_i & iface, void * context, size_t size);
int logical_device_count();                 // devices of the registration (GGML_MI355X_FAKE_DEVICES multiplies them for tests)
int logical_device_ordinal(int i);          // HIP ordinal behind logical device i
ggml_backend_dev_t logical_device(int i);

// ---- row-split weight buffers, -sm row (split.cpp) ----
struct split_tensor_info {
    int n_dev;
    int kind;                                   // 0: cut by ROWS (output features: wq / wk / wv / ffn_gate / ffn_up / output — "column-parallel"),
                                                // 1: cut along K (input features, whole 256-value super-blocks: attn_output / ffn_down — "row-parallel":
                                                //    every device holds all rows of its K range and produces a partial sum)
    int64_t row0[GGML_MI355X_MAX_DEVICES + 1];  // kind 0: device d owns rows [row0[d], row0[d + 1]); kind 1: VALUES [row0[d], row0[d + 1]) of every row
    void * slice[GGML_MI355X_MAX_DEVICES];      // its part, GGUF bytes verbatim (kind 1: rows of (row0[d+1] - row0[d]) / blck blocks), in device d's memory
    size_t row_bytes;                           // bytes of a FULL row
    size_t slice_row_bytes[GGML_MI355X_MAX_DEVICES];  // bytes of a row of device d's slice (kind 0: = row_bytes)
};
void split_rows(int64_t nrows, const float * tensor_split, int n_dev, int64_t granule, int64_t * row0);
ggml_backend_buffer_type_t split_buffer_type(int main_device, const float * tensor_split);
bool buft_is_split(ggml_backend_buffer_type_t buft);
int split_buft_main_device(ggml_backend_buffer_type_t buft);
bool buffer_is_split(ggml_backend_buffer_t b);
const split_tensor_info * split_info(const ggml_tensor * t);
bool split_mul_mat_supported(const ggml_tensor * op);
bool run_split_mul_mat(backend_ctx * c, const ggml_tensor * w, const ggml_tensor * b, ggml_tensor * dst);
// row-parallel weight (kind 1): scatter b's K ranges, per-device partial products, in-stream sum on the main device (+ optional addend)
bool run_split_rowpar(backend_ctx * c, const ggml_tensor * w, const ggml_tensor * b, ggml_tensor * dst, const ggml_tensor * add);
// the whole FFN on sharded weights: broadcast x once, gate / up / SwiGLU / down on every device's own rows of the hidden layer, ONE sum
bool split_ffn_applies(const ggml_tensor * wg, const ggml_tensor * wu, const ggml_tensor * wd);
bool run_split_ffn(backend_ctx * c, const ggml_tensor * wg, const ggml_tensor * wu, const ggml_tensor * wd, const ggml_tensor * x, ggml_tensor * dst, const ggml_tensor * add);
void free_split_helpers(backend_ctx * c);

// ---- graph execution (graph.cpp) ----
bool supports_op(const ggml_tensor * op);
bool mm_batched_q_ok(const ggml_tensor * op);  // MUL_MAT over a 3-D quantised weight, one matrix per head (mmb.hip): the whole operand contract
enum ggml_status graph_compute(backend_ctx * ctx, ggml_cgraph * g);
void free_graph_cache(backend_ctx * ctx);
bool graph_key_equals(const ggml_cgraph * g, const std::vector<uint64_t> & key);  // the graph-key words (graph.cpp: walk_key), compared in place ...
void graph_key_build(const ggml_cgraph * g, std::vector<uint64_t> & key);         // ... or materialised

// ---- in-process tensor parallel over the devices of a row-split model, -sm row (tp_inproc.cpp) ----
struct ip_engine;
// handled = false: the graph is not one the engine takes (no split weights, or a shape it declines): the caller goes on as before
enum ggml_status ip_graph_compute(backend_ctx * ctx, ggml_cgraph * g, bool * handled);
void ip_free(backend_ctx * ctx);
int64_t ip_stat(const backend_ctx * ctx, const char * key);  // -1: unknown key
// the host is about to read / has written memory of `b` behind the engine's back (get_tensor, set_tensor, copies, a graph the engine does not take):
// the per-device KV shards are gathered into / re-scattered from the host's cache tensors lazily
void ip_host_access(ggml_backend_buffer_t b, bool write);
void ip_host_buffer_freed(ggml_backend_buffer_t b);  // the host frees a buffer the engine mirrors
bool ip_any();

// ---- internal buffer objects for tensors the backend creates itself (backend.cpp) ----
struct buffer_ctx;
void make_internal_buffer(ggml_backend_buffer * out, buffer_ctx * bc, int device_ordinal, bool rowpar);
ggml_backend_t internal_backend(int logical_device);  // a second backend instance on a device of the registration (its own stream and scratch)

// ---- host-side shadow of what the engine uploads as attention masks (backend.cpp) ----
// llama.cpp fills the KQ mask on the host and hands it over with set_tensor(_async) before every graph: while the bytes pass through, the
// backend notes how many cells the batch's tokens can see.  graph_compute reads that to choose kernels whose cost depends on the mask's
// CONTENT (position lists against the dense matrix-core kernel for 33+ tokens; the list form of the non-flash chain only when no token's
// list exceeds its capacity) — decisions a captured graph cannot take from device memory.  Unknown mask (never uploaded through this
// backend, or too large to be worth scanning): callers keep their shape-only rules.
struct mask_stats {
    int rows = 0;          // rows with at least one visible cell
    int max_visible = 0;   // the longest row
    float density = 1.0f;  // visible cells / (rows x row length)
};
void note_mask_upload(const ggml_tensor * t, const void * host, size_t offset, size_t size);
bool lookup_mask_stats(const void * dev_ptr, mask_stats * out);
void forget_mask_stats(const void * dev_ptr, size_t nbytes);  // a device-side write landed there
void copy_mask_stats(const ggml_tensor * src, const ggml_tensor * dst, size_t nbytes);  // ... unless it was a whole-tensor copy of a tensor on record: the record follows the bytes
// 1: the mask at dev_ptr is known and sparse enough (<= a quarter visible) that per-token position lists beat a dense tile kernel
int mask_sparse_hint(const void * dev_ptr);

// ---- tensor parallel (tp.cpp) ----
int tp_init(backend_ctx * ctx, int rank, int world, const void * uid, size_t uid_size);
int tp_get_unique_id(void * out, size_t size);
bool tp_active(const backend_ctx * ctx);
int tp_p2p_export(backend_ctx * ctx, int rank, int world, void * handle_out, size_t size);  // -> this rank's mailbox as a hipIpcMemHandle_t (64 bytes)
int tp_p2p_attach(backend_ctx * ctx, const void * handles, size_t size);                    // world handles in rank order, own slot ignored
int64_t tp_p2p_timeouts(backend_ctx * ctx);
int tp_attach_local(backend_ctx * const * ctxs, int n);  // the devices of this process as one group (ranks = array order); 0 or < 0
bool tp_p2p_enable(backend_ctx * ctx, bool on);  // false: refused (switching the only transport of a group off)
bool tp_p2p_reset(backend_ctx * ctx);           // forget a time-out (every rank, all idle)
bool tp_check(backend_ctx * ctx);               // false: an all-reduce of an earlier graph timed out — the caller fails its graph_compute
// in-stream sum all-reduce of n floats at ptr (capturable)
bool tp_all_reduce(backend_ctx * ctx, float * ptr, size_t n);
// the same with the residual ADD that follows folded in: out[i] = sum_ranks(ptr[i]) + add[i] (add: n values), and the sum of squares of `out`
// left as partial sums (ss_out, *ss_n of them) — served by ONE peer-to-peer launch; returns false (nothing done) when that form does not apply
bool tp_all_reduce_fused(backend_ctx * ctx, float * ptr, size_t n, const float * add, float * out, double * ss_out, int * ss_n);
void tp_free(backend_ctx * ctx);

}  // namespace mi355x
