// mmid.hip — MUL_MAT_ID: the expert mat-vecs of a mixture-of-experts FFN (llama.cpp build_moe_ffn: up / gate / down).
//
//   dst[N, n_used, n_tokens] : dst(:, slot, token) = as(:, :, ids(slot, token)) · b(:, slot or 0, token)
//
// ggml-cpu's mul_mat_id is one vec_dot per (row, slot, token) over the quantised activation row; this is the same product with the
// expert chosen ON THE DEVICE: the ids (a strided view of ARGSORT's result) are read by the kernel, never by the host, so the launch
// geometry depends on shapes only — the node is captured into a hipGraph like a dense mat-vec and a replay follows whatever routing
// the ids hold then.
//
// Form: one launch per node, grid = (row tiles) x (slot, token) pairs.  A workgroup loads its pair's id (the only dependency ahead of
// the weight loads), resolves the expert's base address, issues the first weight loads, stages the pair's Q8_K / Q8_0 activation row
// in LDS and then runs k_mmvq's single-column loop: the block decoders and integer dots of mmvq_types.h, lanes over (super-block,
// chunk) pairs in the same order, the same 6-step butterfly — so a (slot, token) result is bit-equal to the backend's own one-column
// MUL_MAT over that expert's 2-D view.  An id outside [0, n_expert) reads nothing of `as` and writes zeros (ggml-cpu asserts there).
// Larger batches are the same launch with more pairs: each pair streams its expert matrix again (out of L2 / MALL when experts repeat).
//
// ADD_ID (the per-expert bias gpt-oss puts behind each MUL_MAT_ID): dst(:, slot, token) = a(:, slot, token) + b(:, ids(slot, token)), ids read on the device as
// above; an id outside [0, n_expert) adds nothing.  k_add_id is the node on its own; when it directly follows its MUL_MAT_ID (graph.cpp decides), the bias rides in
// that launch's store instead (mmid_args::bias): acc + b[id][row] is the same single f32 addition, so both forms give the same bits, and an id outside the experts
// stores the zeros the unfused pair would.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "mm_dense.h"
#include "mmvq_types.h"

namespace mi355x {

// LDSA: the activation row is staged in LDS (else read from global / L2: rows beyond the LDS budget)
template <typename T, int R, bool LDSA>
__global__ void __launch_bounds__(256) k_mmid(const mmid_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename T::act act;
    constexpr int WAVES = 4, NT = WAVES * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = a.K / T::BLK;
    const int npairs = nblk * T::PPB;
    const int row0 = (blockIdx.x * WAVES + wave) * R;
    const int pair = blockIdx.y, tok = pair / a.n_used, slot = pair - tok * a.n_used;
    float * dcol = a.dst + (size_t) tok * a.dst_nb2 + (size_t) slot * a.dst_nb1;

    const int id = *(const int32_t *) (a.ids + (size_t) tok * a.ids_nb1 + (size_t) slot * 4);
    if ((unsigned) id >= (unsigned) a.n_expert) {  // (uniform over the workgroup) no expert: nothing of `as` is read
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (lane == 0 && row0 + r < a.N) dcol[row0 + r] = 0.0f;
        return;
    }
    const uint8_t * W = a.W + (size_t) id * a.w_nb2;
    const float * bias = a.bias ? (const float *) (a.bias + (size_t) id * a.bias_nb1) : nullptr;  // (ADD_ID in the store)

    // the first weight loads go out before the activations are touched (as k_mmvq)
    const uint8_t * rows[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = W + (size_t) min(row0 + r, a.N - 1) * a.w_nb1;
    typename T::raw w[R];
    int p = lane;
    if (p < npairs) {
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = T::load(rows[r], p, nblk);
    }

    const act * y = (const act *) a.act + (size_t) (tok * a.b_rows + (a.b_rows == 1 ? 0 : slot)) * nblk;
    if constexpr (LDSA) {
        const int nwords = (int) ((size_t) nblk * sizeof(act) / 4);
        const uint32_t * src = (const uint32_t *) y;
        uint32_t * dst = (uint32_t *) smem;
        for (int i = tid; i < nwords; i += NT) dst[i] = src[i];
        __syncthreads();
        y = (const act *) smem;
    }
    if (row0 >= a.N) return;

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    while (p < npairs) {
        typename T::raw nw[R];
        const int pn = p + 64;
        if (pn < npairs) {
#pragma unroll
            for (int r = 0; r < R; ++r) nw[r] = T::load(rows[r], pn, nblk);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) T::template dot<1>(w[r], p, y, nblk, &acc[r]);
        if (pn < npairs) {
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = nw[r];
        }
        p = pn;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0 && row0 + r < a.N) dcol[row0 + r] = bias ? v + bias[row0 + r] : v;
    }
}

// f16 / bf16 / f32 experts: the dot kernel's product (mm_dense.h: f32 activations rounded to the weights' 16-bit format first — f16, or bf16 through f2bf as
// ggml-cpu's from_float does —, f32 fmaf accumulation), one wave per row.  WT: 0 f32, 1 f16, 2 bf16
template <int WT>
__global__ void __launch_bounds__(256) k_mmid_f(const mmid_args a, const int vec_ok) {
    typedef std::conditional_t<WT == 1, elem_f16, std::conditional_t<WT == 2, elem_bf16, elem_f32>> E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    const int pair = blockIdx.y, tok = pair / a.n_used, slot = pair - tok * a.n_used;
    if (row >= a.N) return;
    float * out = a.dst + (size_t) tok * a.dst_nb2 + (size_t) slot * a.dst_nb1 + row;
    const int id = *(const int32_t *) (a.ids + (size_t) tok * a.ids_nb1 + (size_t) slot * 4);
    if ((unsigned) id >= (unsigned) a.n_expert) {
        if (lane == 0) *out = 0.0f;
        return;
    }
    const char * wrow = (const char *) a.W + (size_t) id * a.w_nb2 + (size_t) row * a.w_nb1;
    const char * xcol = a.x + (size_t) tok * a.x_nb2 + (size_t) (a.b_rows == 1 ? 0 : slot) * a.x_nb1;
    const int K = a.K;
    float acc = 0.0f;
    if (vec_ok) {
        for (int k = lane * 8; k < K; k += 64 * 8) {
            float w[8], x[8];
            if constexpr (E::SIZE == 2) {  // (E::load8, written out: filled through a reference, the bf16 instantiation's FMAs are scheduled differently)
                const uint4 t = *(const uint4 *) (wrow + (size_t) k * 2);
                const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    w[2 * i] = E::cvt1((uint16_t) (u[i] & 0xFFFF));
                    w[2 * i + 1] = E::cvt1((uint16_t) (u[i] >> 16));
                }
            } else E::load8(wrow + (size_t) k * E::SIZE, w);
            elem_f32::load8(xcol + (size_t) k * 4, x);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fmaf(w[i], E::round1(x[i]), acc);
        }
    } else {
        for (int k = lane; k < K; k += 64) {
            const float wv = E::load1(wrow + (size_t) k * E::SIZE);
            const float xv = E::round1(*(const float *) (xcol + (size_t) k * 4));
            acc = fmaf(wv, xv, acc);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) *out = a.bias ? acc + ((const float *) (a.bias + (size_t) id * a.bias_nb1))[row] : acc;
}

// ADD_ID on its own: one workgroup per (slot, token) row of a; every thread reads its own elements before it writes them (dst may be a's block)
__global__ void __launch_bounds__(256) k_add_id(const tdesc a, const tdesc b, const tdesc ids, const tdesc d) {
    const int64_t pair = blockIdx.x, tok = pair / a.ne[1], slot = pair - tok * a.ne[1];
    const float * x = (const float *) (a.data + slot * a.nb[1] + tok * a.nb[2]);
    float * y = (float *) (d.data + slot * d.nb[1] + tok * d.nb[2]);
    const int id = *(const int32_t *) (ids.data + tok * ids.nb[1] + slot * 4);
    const bool in = (unsigned) id < (unsigned) b.ne[1];
    const float * br = (const float *) (b.data + (in ? (int64_t) id : 0) * b.nb[1]);
    for (int64_t i = (int64_t) blockIdx.y * 256 + threadIdx.x; i < a.ne[0]; i += (int64_t) gridDim.y * 256) y[i] = in ? x[i] + br[i] : x[i];
}
void launch_add_id(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & ids, const tdesc & d) {
    const int64_t pairs = a.ne[1] * a.ne[2];
    if (pairs < 1 || a.ne[0] < 1) return;
    const unsigned chunks = (unsigned) std::min<int64_t>(64, (a.ne[0] + 1023) / 1024);
    hipLaunchKernelGGL(k_add_id, dim3((unsigned) pairs, chunks), dim3(256), 0, s, a, b, ids, d);
}

template <typename T> static void launch_mmid_t(hipStream_t s, const mmid_args & a) {
    const int nblk = a.K / T::BLK;
    const size_t lds = (size_t) nblk * sizeof(typename T::act);
    const int npair = a.n_used * a.n_tokens;
    // two rows a wave where that still leaves every CU several workgroups
    const bool r2 = (int64_t) a.N * npair >= 16384;
    const int rpb = 4 * (r2 ? 2 : 1);
    const dim3 grid((unsigned) ((a.N + rpb - 1) / rpb), (unsigned) npair);
    if (lds <= 64 * 1024) {
        if (r2) hipLaunchKernelGGL((k_mmid<T, 2, true>), grid, dim3(256), lds, s, a);
        else    hipLaunchKernelGGL((k_mmid<T, 1, true>), grid, dim3(256), lds, s, a);
    } else {
        if (r2) hipLaunchKernelGGL((k_mmid<T, 2, false>), grid, dim3(256), 0, s, a);
        else    hipLaunchKernelGGL((k_mmid<T, 1, false>), grid, dim3(256), 0, s, a);
    }
}

void launch_mmid(hipStream_t s, const mmid_args & a) {
    if (a.n_used < 1 || a.n_tokens < 1 || (int64_t) a.n_used * a.n_tokens > 65535 || (a.b_rows != 1 && a.b_rows != a.n_used)) {
        MI_ERR("launch_mmid: %d slots x %d tokens, %d activation rows a token", a.n_used, a.n_tokens, a.b_rows);
        abort();
    }
    switch (a.type) {
        case GGML_TYPE_Q2_K: launch_mmid_t<T_Q2K>(s, a); break;
        case GGML_TYPE_Q3_K: launch_mmid_t<T_Q3K>(s, a); break;
        case GGML_TYPE_Q4_K: launch_mmid_t<T_Q4K>(s, a); break;
        case GGML_TYPE_Q5_K: launch_mmid_t<T_Q5K>(s, a); break;
        case GGML_TYPE_Q6_K: launch_mmid_t<T_Q6K>(s, a); break;
        case GGML_TYPE_Q8_0: launch_mmid_t<T_Q80>(s, a); break;
        case GGML_TYPE_Q4_0: launch_mmid_t<T_Q40>(s, a); break;
        case GGML_TYPE_Q4_1: launch_mmid_t<T_Q41>(s, a); break;
        case GGML_TYPE_Q5_0: launch_mmid_t<T_Q50>(s, a); break;
        case GGML_TYPE_Q5_1: launch_mmid_t<T_Q51>(s, a); break;
        case GGML_TYPE_IQ4_NL: launch_mmid_t<T_IQ4NL>(s, a); break;
        case GGML_TYPE_IQ4_XS: launch_mmid_t<T_IQ4XS>(s, a); break;
        case GGML_TYPE_MXFP4: launch_mmid_t<T_MXFP4>(s, a); break;
        case GGML_TYPE_F16: case GGML_TYPE_BF16: case GGML_TYPE_F32: {
            const bool w16 = a.type == GGML_TYPE_F16;
            const bool vec_ok = (a.K % 8) == 0 && ((((uintptr_t) a.W) | ((uintptr_t) a.x) | (uintptr_t) a.w_nb1 | (uintptr_t) a.w_nb2 | (uintptr_t) a.x_nb1 | (uintptr_t) a.x_nb2) & 15) == 0;
            const dim3 grid((unsigned) ((a.N + 3) / 4), (unsigned) (a.n_used * a.n_tokens));
            if (w16) hipLaunchKernelGGL(k_mmid_f<1>, grid, dim3(256), 0, s, a, vec_ok ? 1 : 0);
            else if (a.type == GGML_TYPE_BF16) hipLaunchKernelGGL(k_mmid_f<2>, grid, dim3(256), 0, s, a, vec_ok ? 1 : 0);
            else hipLaunchKernelGGL(k_mmid_f<0>, grid, dim3(256), 0, s, a, vec_ok ? 1 : 0);
            break;
        }
        default: MI_ERR("launch_mmid: unsupported expert type %d", a.type); abort();
    }
}

MI_TU_TOUCH(mmid)

}  // namespace mi355x
