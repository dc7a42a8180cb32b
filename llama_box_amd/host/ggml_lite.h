/*
 * ggml_lite.h — host-side mirror of the slice of the ggml public API that the hot path's callers use.
 *
 * The reference (llama-box -> llama.cpp) builds a ggml_cgraph with ggml.h's constructors and hands it
 * to the backend through ggml-backend.h (llama-box/rpcserver.hpp:1339-1393 rebuilds such a graph from
 * the wire and calls ggml_backend_graph_compute; llama-box/httpserver.hpp:3591 reaches it through
 * llama_decode).  ggml itself is absent from /root/reference (un-vendored submodule), so this file
 * provides our OWN implementation of the same entry points — same names, argument meaning and error
 * behaviour — so that (1) the backend .so can be exercised exactly the way ggml would exercise it and
 * (2) the parity tests read like upstream's test-backend-ops.  It is a driver/test harness: the
 * product is the backend library (csrc/), which depends on none of this.
 */
#ifndef GGML_LITE_H
#define GGML_LITE_H
#include "../../include/ggml_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct ggml_context;
struct ggml_init_params {
    size_t mem_size;   /* ignored: tensors are heap objects owned by the context */
    void * mem_buffer; /* ignored */
    bool no_alloc;     /* always treated as true: data is placed by the backend allocators below */
};

struct ggml_context * ggml_init(struct ggml_init_params params);
void ggml_free(struct ggml_context * ctx);

/* type helpers */
size_t ggml_type_size(enum ggml_type type);
int64_t ggml_blck_size(enum ggml_type type);
size_t ggml_row_size(enum ggml_type type, int64_t ne);
const char * ggml_type_name(enum ggml_type type);
const char * ggml_op_name(enum ggml_op op);
size_t ggml_nbytes(const struct ggml_tensor * t);
int64_t ggml_nelements(const struct ggml_tensor * t);
int64_t ggml_nrows(const struct ggml_tensor * t);
bool ggml_is_contiguous(const struct ggml_tensor * t);
bool ggml_is_quantized(enum ggml_type type);

/* tensors */
struct ggml_tensor * ggml_new_tensor(struct ggml_context * ctx, enum ggml_type type, int n_dims, const int64_t * ne);
struct ggml_tensor * ggml_new_tensor_1d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0);
struct ggml_tensor * ggml_new_tensor_2d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1);
struct ggml_tensor * ggml_new_tensor_3d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1, int64_t ne2);
struct ggml_tensor * ggml_new_tensor_4d(struct ggml_context * ctx, enum ggml_type type, int64_t ne0, int64_t ne1, int64_t ne2, int64_t ne3);
struct ggml_tensor * ggml_set_name(struct ggml_tensor * t, const char * name);
void ggml_set_input(struct ggml_tensor * t);
void ggml_set_output(struct ggml_tensor * t);
struct ggml_tensor * ggml_get_first_tensor(const struct ggml_context * ctx);
struct ggml_tensor * ggml_get_next_tensor(const struct ggml_context * ctx, struct ggml_tensor * t);
struct ggml_tensor * ggml_get_tensor(struct ggml_context * ctx, const char * name);

/* views (metadata only) */
struct ggml_tensor * ggml_view_1d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, size_t offset);
struct ggml_tensor * ggml_view_2d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, size_t nb1, size_t offset);
struct ggml_tensor * ggml_view_3d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, int64_t ne2, size_t nb1, size_t nb2, size_t offset);
struct ggml_tensor * ggml_view_4d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, int64_t ne2, int64_t ne3, size_t nb1, size_t nb2, size_t nb3, size_t offset);
struct ggml_tensor * ggml_reshape_1d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0);
struct ggml_tensor * ggml_reshape_2d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1);
struct ggml_tensor * ggml_reshape_3d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, int64_t ne2);
struct ggml_tensor * ggml_reshape_4d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, int64_t ne2, int64_t ne3);
struct ggml_tensor * ggml_permute(struct ggml_context * ctx, struct ggml_tensor * a, int axis0, int axis1, int axis2, int axis3);
struct ggml_tensor * ggml_transpose(struct ggml_context * ctx, struct ggml_tensor * a);

/* ops */
struct ggml_tensor * ggml_dup(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_cont(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_cont_2d(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1);
struct ggml_tensor * ggml_cpy(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_cast(struct ggml_context * ctx, struct ggml_tensor * a, enum ggml_type type);
struct ggml_tensor * ggml_add(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_sub(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_mul(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_div(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_scale(struct ggml_context * ctx, struct ggml_tensor * a, float s);
struct ggml_tensor * ggml_scale_bias(struct ggml_context * ctx, struct ggml_tensor * a, float s, float b);
struct ggml_tensor * ggml_rms_norm(struct ggml_context * ctx, struct ggml_tensor * a, float eps);
struct ggml_tensor * ggml_norm(struct ggml_context * ctx, struct ggml_tensor * a, float eps);
struct ggml_tensor * ggml_mul_mat(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
void ggml_mul_mat_set_prec(struct ggml_tensor * a, enum ggml_prec prec);
struct ggml_tensor * ggml_get_rows(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_set_rows(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * c);
struct ggml_tensor * ggml_silu(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_unary(struct ggml_context * ctx, struct ggml_tensor * a, enum ggml_unary_op op);
struct ggml_tensor * ggml_swiglu(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_swiglu_split(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_swiglu_oai(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, float alpha, float limit);
struct ggml_tensor * ggml_gelu(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_gelu_quick(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_gelu_erf(struct ggml_context * ctx, struct ggml_tensor * a);
/* REGLU / GEGLU / GEGLU_ERF / GEGLU_QUICK: act(x) * g over the halves of a row (x first; _swapped: g first) or over two tensors (_split: a is x, b is g) */
struct ggml_tensor * ggml_reglu(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_reglu_swapped(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_reglu_split(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_geglu(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_swapped(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_split(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_geglu_erf(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_erf_swapped(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_erf_split(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_geglu_quick(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_quick_swapped(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_geglu_quick_split(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);
struct ggml_tensor * ggml_soft_max(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_soft_max_ext(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * mask, float scale, float max_bias);
void ggml_soft_max_add_sinks(struct ggml_tensor * a, struct ggml_tensor * sinks);
struct ggml_tensor * ggml_rope_ext(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * c,
                                   int n_dims, int mode, int n_ctx_orig, float freq_base, float freq_scale, float ext_factor,
                                   float attn_factor, float beta_fast, float beta_slow);
struct ggml_tensor * ggml_rope_multi(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * c,
                                     int n_dims, int sections[4], int mode, int n_ctx_orig, float freq_base, float freq_scale,
                                     float ext_factor, float attn_factor, float beta_fast, float beta_slow);
struct ggml_tensor * ggml_rope_ext_inplace(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * c,
                                   int n_dims, int mode, int n_ctx_orig, float freq_base, float freq_scale, float ext_factor,
                                   float attn_factor, float beta_fast, float beta_slow);
struct ggml_tensor * ggml_flash_attn_ext(struct ggml_context * ctx, struct ggml_tensor * q, struct ggml_tensor * k, struct ggml_tensor * v,
                                         struct ggml_tensor * mask, float scale, float max_bias, float logit_softcap);
void ggml_flash_attn_ext_set_prec(struct ggml_tensor * a, enum ggml_prec prec);
void ggml_flash_attn_ext_add_sinks(struct ggml_tensor * a, struct ggml_tensor * sinks);
struct ggml_tensor * ggml_argmax(struct ggml_context * ctx, struct ggml_tensor * a);
/* mixture-of-experts FFN (llama.cpp build_moe_ffn): the router's top-k, its weight normalisation, and the expert mat-muls */
struct ggml_tensor * ggml_argsort(struct ggml_context * ctx, struct ggml_tensor * a, enum ggml_sort_order order);
struct ggml_tensor * ggml_top_k(struct ggml_context * ctx, struct ggml_tensor * a, int k);  /* ARGSORT (descending) + a view of its first k columns */
struct ggml_tensor * ggml_sum_rows(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_clamp(struct ggml_context * ctx, struct ggml_tensor * a, float min, float max);  /* in place: a view of a */
/* as [K, N, n_expert], b [K, n_used | 1, n_tokens] f32, ids [n_used, n_tokens] i32 -> [N, n_used, n_tokens] */
struct ggml_tensor * ggml_mul_mat_id(struct ggml_context * ctx, struct ggml_tensor * as, struct ggml_tensor * b, struct ggml_tensor * ids);
struct ggml_tensor * ggml_add_id(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * ids);
/* state-space layers (llama.cpp build_mamba_layer / build_mamba2_layer; DESIGN.md §4i states the three contracts) */
struct ggml_tensor * ggml_concat(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, int dim);
/* sx [d_conv - 1 + n_t, d_inner, n_s], c [d_conv, d_inner] -> [d_inner, n_t, n_s] */
struct ggml_tensor * ggml_ssm_conv(struct ggml_context * ctx, struct ggml_tensor * sx, struct ggml_tensor * c);
/* s [d_state, head_dim, n_head, n_rs], x [head_dim, n_head, n_t, n_s], dt [n_head, n_t, n_s], A [d_state | 1, n_head], B / C [d_state, n_group, n_t, n_s],
 * ids i32 [n_s] -> one f32 vector: y [head_dim, n_head, n_t, n_s], then the final states [d_state, head_dim, n_head, n_s] */
struct ggml_tensor * ggml_ssm_scan(struct ggml_context * ctx, struct ggml_tensor * s, struct ggml_tensor * x, struct ggml_tensor * dt, struct ggml_tensor * A,
                                   struct ggml_tensor * B, struct ggml_tensor * C, struct ggml_tensor * ids);
/* linear-attention recurrent layers (llama.cpp rwkv6 / rwkv6qwen2 / rwkv7 / arwkv7; DESIGN.md §4k states the contracts) */
struct ggml_tensor * ggml_sqr(struct ggml_context * ctx, struct ggml_tensor * a);
struct ggml_tensor * ggml_repeat(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b);  /* a repeated to b's shape */
struct ggml_tensor * ggml_l2_norm(struct ggml_context * ctx, struct ggml_tensor * a, float eps);
/* k, v, r, td (and q, g, w, a, b) [S, H, n_tokens], tf [S, H], state S * S * H floats for each of its ne[1] sequences -> [S * H, n_tokens + S * n_seqs]:
 * y [S * H, n_tokens], then the new states */
struct ggml_tensor * ggml_rwkv_wkv6(struct ggml_context * ctx, struct ggml_tensor * k, struct ggml_tensor * v, struct ggml_tensor * r, struct ggml_tensor * tf,
                                    struct ggml_tensor * td, struct ggml_tensor * state);
struct ggml_tensor * ggml_rwkv_wkv7(struct ggml_context * ctx, struct ggml_tensor * r, struct ggml_tensor * w, struct ggml_tensor * k, struct ggml_tensor * v,
                                    struct ggml_tensor * a, struct ggml_tensor * b, struct ggml_tensor * state);
struct ggml_tensor * ggml_gated_linear_attn(struct ggml_context * ctx, struct ggml_tensor * k, struct ggml_tensor * v, struct ggml_tensor * q, struct ggml_tensor * g,
                                            struct ggml_tensor * state, float scale);
/* vision / audio towers (ggml_conv_2d patch embeddings, Whisper-style ggml_conv_1d stems, pooled projectors; DESIGN.md §4m states the contracts) */
enum ggml_op_pool { GGML_OP_POOL_MAX, GGML_OP_POOL_AVG, GGML_OP_POOL_COUNT };
enum ggml_scale_mode { GGML_SCALE_MODE_NEAREST = 0, GGML_SCALE_MODE_BILINEAR = 1, GGML_SCALE_MODE_BICUBIC = 2 };
enum ggml_scale_flag { GGML_SCALE_FLAG_ALIGN_CORNERS = 1 << 8 };
/* a: the convolution kernel [KW, KH, IC, OC] (1-D: [KW, IC, OC]), read for its extents; b: the data f32 [IW, IH, IC, N] (1-D: [IW, IC, N])
 * -> dst_type [IC * KH * KW, OW, OH, N] (1-D: [IC * KW, OW, N]); op_params {s0, s1, p0, p1, d0, d1, is_2D} */
struct ggml_tensor * ggml_im2col(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, int s0, int s1, int p0, int p1, int d0, int d1, bool is_2D,
                                 enum ggml_type dst_type);
/* im2col in the kernel's type, MUL_MAT(im2col, kernel), reshaped: 1-D -> [OL, OC, N]; 2-D -> cont(permute(0, 1, 3, 2)) = [OW, OH, OC, N] */
struct ggml_tensor * ggml_conv_1d(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, int s0, int p0, int d0);
struct ggml_tensor * ggml_conv_2d(struct ggml_context * ctx, struct ggml_tensor * a, struct ggml_tensor * b, int s0, int s1, int p0, int p1, int d0, int d1);
/* op_params {op, k0, s0, p0} -> [(W + 2 p0 - k0) / s0 + 1, ne1, ne2, ne3]; {op, k0, k1, s0, s1, p0, p1} -> [(W + 2 p0 - k0) / s0 + 1, (H + 2 p1 - k1) / s1 + 1, ne2, ne3] */
struct ggml_tensor * ggml_pool_1d(struct ggml_context * ctx, struct ggml_tensor * a, enum ggml_op_pool op, int k0, int s0, int p0);
struct ggml_tensor * ggml_pool_2d(struct ggml_context * ctx, struct ggml_tensor * a, enum ggml_op_pool op, int k0, int k1, int s0, int s1, float p0, float p1);
/* zeros appended at the high end of every dimension; no op_params at this ABI snapshot */
struct ggml_tensor * ggml_pad(struct ggml_context * ctx, struct ggml_tensor * a, int p0, int p1, int p2, int p3);
/* mode: a ggml_scale_mode, optionally | GGML_SCALE_FLAG_ALIGN_CORNERS, in op_params[0]; ggml_upscale multiplies dims 0 and 1 by scale_factor */
struct ggml_tensor * ggml_upscale(struct ggml_context * ctx, struct ggml_tensor * a, int scale_factor, enum ggml_scale_mode mode);
struct ggml_tensor * ggml_interpolate(struct ggml_context * ctx, struct ggml_tensor * a, int64_t ne0, int64_t ne1, int64_t ne2, int64_t ne3, uint32_t mode);
/* image generation (stable-diffusion.cpp's UNet, VAE, CLIP and ESRGAN graphs; DESIGN.md §4n states the contracts) */
/* op_params {n_groups, eps as f32}; a [W, H, C, N]; the _inplace form is a view of a */
struct ggml_tensor * ggml_group_norm(struct ggml_context * ctx, struct ggml_tensor * a, int n_groups, float eps);
struct ggml_tensor * ggml_group_norm_inplace(struct ggml_context * ctx, struct ggml_tensor * a, int n_groups, float eps);
/* op_params {dim, max_period}; timesteps f32 [N] -> f32 [dim rounded up to even, N] */
struct ggml_tensor * ggml_timestep_embedding(struct ggml_context * ctx, struct ggml_tensor * timesteps, int dim, int max_period);
/* op_params {n_past}; the _inplace form is a view of a */
struct ggml_tensor * ggml_diag_mask_inf(struct ggml_context * ctx, struct ggml_tensor * a, int n_past);
struct ggml_tensor * ggml_diag_mask_inf_inplace(struct ggml_context * ctx, struct ggml_tensor * a, int n_past);
/* op_params {negative_slope as f32}; inplace: a view of a */
struct ggml_tensor * ggml_leaky_relu(struct ggml_context * ctx, struct ggml_tensor * a, float negative_slope, bool inplace);

/* graphs */
struct ggml_cgraph * ggml_new_graph(struct ggml_context * ctx);
struct ggml_cgraph * ggml_new_graph_custom(struct ggml_context * ctx, size_t size, bool grads);
void ggml_build_forward_expand(struct ggml_cgraph * cgraph, struct ggml_tensor * tensor);
void ggml_lite_set_no_reuse(int on);  // harness only: graph allocator keeps every intermediate (per-node comparisons)
struct ggml_cgraph ggml_graph_view(struct ggml_cgraph * cgraph, int i0, int i1);  // shares the parent's hash set + use counts
int ggml_graph_n_nodes(struct ggml_cgraph * cgraph);
struct ggml_tensor * ggml_graph_node(struct ggml_cgraph * cgraph, int i);

/* ------------------------- ggml-backend.h mirror (generic wrappers over the vtables) ------------------------- */
/* dlopen()s a backend library and calls its ggml_backend_init(); NULL (with a message on stderr) on failure:
 * missing symbol, api_version mismatch (same checks as ggml_backend_load in ggml-backend-reg.cpp). */
ggml_backend_reg_t ggml_backend_load(const char * path);
const char * ggml_backend_reg_name(ggml_backend_reg_t reg);
size_t ggml_backend_reg_dev_count(ggml_backend_reg_t reg);
ggml_backend_dev_t ggml_backend_reg_dev_get(ggml_backend_reg_t reg, size_t index);
void * ggml_backend_reg_get_proc_address(ggml_backend_reg_t reg, const char * name);
const char * ggml_backend_dev_name(ggml_backend_dev_t dev);
const char * ggml_backend_dev_description(ggml_backend_dev_t dev);
void ggml_backend_dev_memory(ggml_backend_dev_t dev, size_t * free, size_t * total);
enum ggml_backend_dev_type ggml_backend_dev_type(ggml_backend_dev_t dev);
void ggml_backend_dev_get_props(ggml_backend_dev_t dev, struct ggml_backend_dev_props * props);
ggml_backend_t ggml_backend_dev_init(ggml_backend_dev_t dev, const char * params);
ggml_backend_buffer_type_t ggml_backend_dev_buffer_type(ggml_backend_dev_t dev);
ggml_backend_buffer_type_t ggml_backend_dev_host_buffer_type(ggml_backend_dev_t dev);
bool ggml_backend_dev_supports_op(ggml_backend_dev_t dev, const struct ggml_tensor * op);
bool ggml_backend_dev_supports_buft(ggml_backend_dev_t dev, ggml_backend_buffer_type_t buft);

const char * ggml_backend_buft_name(ggml_backend_buffer_type_t buft);
ggml_backend_buffer_t ggml_backend_buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size);
size_t ggml_backend_buft_get_alignment(ggml_backend_buffer_type_t buft);
size_t ggml_backend_buft_get_alloc_size(ggml_backend_buffer_type_t buft, const struct ggml_tensor * tensor);
bool ggml_backend_buft_is_host(ggml_backend_buffer_type_t buft);

/* what libggml-base provides to backends; exported here so the backend .so (which looks it up with
 * dlsym(RTLD_DEFAULT)) behaves exactly as it would inside a real ggml host */
ggml_backend_buffer_t ggml_backend_buffer_init(ggml_backend_buffer_type_t buft, struct ggml_backend_buffer_i iface, void * context, size_t size);
void ggml_backend_buffer_free(ggml_backend_buffer_t buffer);
void * ggml_backend_buffer_get_base(ggml_backend_buffer_t buffer);
size_t ggml_backend_buffer_get_size(ggml_backend_buffer_t buffer);
void ggml_backend_buffer_clear(ggml_backend_buffer_t buffer, uint8_t value);
void ggml_backend_buffer_set_usage(ggml_backend_buffer_t buffer, enum ggml_backend_buffer_usage usage);
bool ggml_backend_buffer_is_host(ggml_backend_buffer_t buffer);

const char * ggml_backend_name(ggml_backend_t backend);
void ggml_backend_free(ggml_backend_t backend);
void ggml_backend_tensor_set(struct ggml_tensor * tensor, const void * data, size_t offset, size_t size);
void ggml_backend_tensor_get(const struct ggml_tensor * tensor, void * data, size_t offset, size_t size);
void ggml_backend_tensor_memset(struct ggml_tensor * tensor, uint8_t value, size_t offset, size_t size);
void ggml_backend_tensor_set_async(ggml_backend_t backend, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size);
void ggml_backend_tensor_get_async(ggml_backend_t backend, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size);
void ggml_backend_synchronize(ggml_backend_t backend);
enum ggml_status ggml_backend_graph_compute(ggml_backend_t backend, struct ggml_cgraph * cgraph);
enum ggml_status ggml_backend_graph_compute_async(ggml_backend_t backend, struct ggml_cgraph * cgraph);
bool ggml_backend_supports_op(ggml_backend_t backend, const struct ggml_tensor * op);
/* copies between backends and events (ggml-backend.h): what ggml_backend_sched issues between the devices of a layer split */
void ggml_backend_tensor_copy(struct ggml_tensor * src, struct ggml_tensor * dst);
void ggml_backend_tensor_copy_async(ggml_backend_t backend_src, ggml_backend_t backend_dst, struct ggml_tensor * src, struct ggml_tensor * dst);
ggml_backend_event_t ggml_backend_event_new(ggml_backend_dev_t device);
void ggml_backend_event_free(ggml_backend_event_t event);
void ggml_backend_event_record(ggml_backend_event_t event, ggml_backend_t backend);
void ggml_backend_event_synchronize(ggml_backend_event_t event);
void ggml_backend_event_wait(ggml_backend_t backend, ggml_backend_event_t event);

/* plain host-memory buffer type (the role ggml_backend_cpu_buffer_type() plays upstream) */
ggml_backend_buffer_type_t ggml_backend_cpu_buffer_type(void);

/* ggml-alloc.h mirror */
/* allocates every tensor of ctx that has no data yet (views follow their view_src) in ONE buffer of buft */
ggml_backend_buffer_t ggml_backend_alloc_ctx_tensors_from_buft(struct ggml_context * ctx, ggml_backend_buffer_type_t buft);
typedef struct ggml_gallocr * ggml_gallocr_t;
ggml_gallocr_t ggml_gallocr_new(ggml_backend_buffer_type_t buft);
void ggml_gallocr_free(ggml_gallocr_t galloc);
/* sizes the compute buffer for `graph` (liveness-based reuse) without touching tensors */
bool ggml_gallocr_reserve(ggml_gallocr_t galloc, struct ggml_cgraph * graph);
/* places graph inputs and node outputs; re-uses the reserved buffer when it is large enough */
bool ggml_gallocr_alloc_graph(ggml_gallocr_t galloc, struct ggml_cgraph * graph);
size_t ggml_gallocr_get_buffer_size(ggml_gallocr_t galloc, int buffer_id);

#ifdef __cplusplus
}
#endif
#endif
