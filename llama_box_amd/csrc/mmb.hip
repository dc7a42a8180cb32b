// mmb.hip — batched MUL_MAT over a 3-D quantised weight, one matrix per head (llama.cpp's deepseek2 graph: the absorbed MLA matrices wk_b and wv_b).
//
//   a [K, N, H] quantised, b [K, M, H * r2, E] f32, dst [N, M, H * r2, E] f32 :  dst(:, m, h, e) = a(:, :, h / r2) · q(b(:, m, h, e))
//
// ggml-cpu's mul_mat with broadcasting (oracle/ggml_cpu_ref.c: op_mul_mat): one vec_dot per (row, column) over the column's quantised row.  b arrives already
// quantised (quantize.hip, rows in (i11, i12, i13) order), so the NC columns of one (head, e) that a workgroup serves are NC consecutive rows of the scratch.
//
// Form: k_mmid without the id load, one launch per node for any M.  grid = (row tiles, column blocks, heads x e) — columns and heads never share a grid axis: 512
// tokens x 128 heads is past the 65535 of y and z.  Two things go beyond k_mmid:
//   * column blocking: a workgroup computes NC (1, 2, 4, 8) columns of its head per pass over the weights (T::dot<NC> of mmvq_types.h keeps one sum per column), so a
//     prompt batch reads a head's matrix M / NC times instead of M.  The last block of a node may hold fewer live columns: its dead columns repeat the last live
//     activation row and are not stored.
//   * short rows: wk_b has K = 128 — four Q8_0 blocks, four (block, chunk) pairs for 64 lanes.  A wave is cut into row groups of W = 4, 8 or 16 lanes when a row's
//     pairs fit one group (64 / W rows a wave, 16 .. 64 rows a workgroup), so a wave's loads are 64 consecutive pairs of consecutive rows and no lane idles for
//     W = npairs.
// Summation order: lane s of a row's group owns pair p = s (p = lane, lane + 64, ... for W = 64), as k_mmvq's one-column loop gives lane p of a whole wave; the group
// is reduced by the steps of wave_sum that involve its lanes, in wave_sum's order.  In k_mmvq the other lanes hold +0.0 (a sum that starts at +0.0 never becomes
// -0.0) and adding +0.0 changes nothing, so every (head, column) is bit-equal to the backend's one-column MUL_MAT over that head's 2-D view — k_mmid's promise.
//   wave_sum, lane 0:  rows of 16 by rotations of 8, 4, 2, 1, then ((r0 + r16) + r32) + r48.  With values in lanes 0 .. W - 1 only, lane 0 ends with
//   W = 16: row16_sum itself;  W = 8: [(v0 + v4) + (v2 + v6)] + [(v1 + v5) + (v3 + v7)];  W = 4: (v0 + v2) + (v1 + v3)   (f32 addition commutes: either rotation
//   direction gives these trees) — the xor steps W / 2, ..., 2, 1 below.
#include <hip/hip_runtime.h>

#include "mmvq_types.h"

namespace mi355x {

template <int W> __device__ __forceinline__ float mmb_group_sum(float v) {
    if constexpr (W == 16) return row16_sum(v);
    if constexpr (W == 8) v += __shfl_xor(v, 4, 64);
    v += dpp_f32<MI_DPP_QUAD_XOR2>(v);
    v += dpp_f32<MI_DPP_QUAD_XOR1>(v);
    return v;
}

// W: lanes per row (64: one row a wave); LDSA: the block's NC activation rows are staged in LDS (else read from global / L2: rows beyond the LDS budget)
template <typename T, int NC, int W, bool LDSA>
__global__ void __launch_bounds__(256) k_mmb(const mmb_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename T::act act;
    constexpr int WAVES = 4, NT = WAVES * 64, RW = 64 / W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = a.K / T::BLK;
    const int npairs = nblk * T::PPB;
    const int sub = lane & (W - 1);
    const int row = (blockIdx.x * WAVES + wave) * RW + (lane / W);
    const int hb = (int) blockIdx.z % a.Hb, e = (int) blockIdx.z / a.Hb;
    const int c0 = (int) blockIdx.y * NC, live = min(NC, a.M - c0);

    // the first weight loads go out before the activations are touched (as k_mmvq)
    const uint8_t * wrow = a.W + (size_t) (hb / a.r2) * a.w_nb2 + (size_t) min(row, a.N - 1) * a.w_nb1;
    typename T::raw w;
    int p = sub;
    if (p < npairs) w = T::load(wrow, p, nblk);

    // the block's activation rows: NC consecutive rows of the scratch, [E][Hb][M][K / blk]
    const size_t col0 = ((size_t) e * a.Hb + hb) * (size_t) a.M + c0;
    const act * y = (const act *) a.act + col0 * nblk;
    if constexpr (LDSA) {
        const int wpr = (int) ((size_t) nblk * sizeof(act) / 4);  // dwords of one row
        const uint32_t * src = (const uint32_t *) y;
        uint32_t * dst = (uint32_t *) smem;
        if (live == NC) {
            for (int i = tid; i < NC * wpr; i += NT) dst[i] = src[i];
        } else {
            for (int i = tid; i < NC * wpr; i += NT) {
                const int col = i / wpr;
                dst[i] = src[i - (col - min(col, live - 1)) * wpr];
            }
        }
        __syncthreads();
        y = (const act *) smem;
    }  // (unstaged rows — beyond the LDS budget even for one column — come with NC = 1: no dead columns)

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
    while (p < npairs) {
        typename T::raw nw;
        const int pn = p + W;
        if (pn < npairs) nw = T::load(wrow, pn, nblk);
        T::template dot<NC>(w, p, y, nblk, acc);
        if (pn < npairs) w = nw;
        p = pn;
    }
    float * out = a.dst + (col0 * (size_t) a.N + (size_t) row);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float v;
        if constexpr (W == 64) v = wave_sum(acc[c]);
        else v = mmb_group_sum<W>(acc[c]);
        if (sub == 0 && row < a.N && c < live) out[(size_t) c * a.N] = v;
    }
}

template <typename T, int NC, int W> static void launch_mmb_w(hipStream_t s, const mmb_args & a) {
    const int nblk = a.K / T::BLK;
    const size_t lds = (size_t) NC * nblk * sizeof(typename T::act);
    const int rpb = 4 * (64 / W);
    const dim3 grid((unsigned) ((a.N + rpb - 1) / rpb), (unsigned) ((a.M + NC - 1) / NC), (unsigned) (a.Hb * a.E));
    if (lds <= 64 * 1024) hipLaunchKernelGGL((k_mmb<T, NC, W, true>), grid, dim3(256), lds, s, a);
    else if constexpr (NC == 1) hipLaunchKernelGGL((k_mmb<T, 1, W, false>), grid, dim3(256), 0, s, a);
    else { MI_ERR("launch_mmb: %d columns of K = %d do not fit the LDS budget", NC, a.K); abort(); }  // (launch_mmb_t narrows the block first)
}
template <typename T, int NC> static void launch_mmb_nc(hipStream_t s, const mmb_args & a) {
    const int npairs = a.K / T::BLK * T::PPB;
    // a group of W lanes keeps k_mmvq's order only while every lane owns at most one pair
    if (npairs <= 4) launch_mmb_w<T, NC, 4>(s, a);
    else if (npairs <= 8) launch_mmb_w<T, NC, 8>(s, a);
    else if (npairs <= 16) launch_mmb_w<T, NC, 16>(s, a);
    else launch_mmb_w<T, NC, 64>(s, a);
}
template <typename T> static void launch_mmb_t(hipStream_t s, const mmb_args & a) {
    // the widest block the node fills at least once; activation rows too long for the LDS budget at that width take a narrower block that fits
    int nc = a.M >= 5 ? 8 : a.M >= 3 ? 4 : a.M >= 2 ? 2 : 1;
    const size_t row_bytes = (size_t) (a.K / T::BLK) * sizeof(typename T::act);
    while (nc > 1 && (size_t) nc * row_bytes > 64 * 1024) nc >>= 1;
    switch (nc) {
        case 8: launch_mmb_nc<T, 8>(s, a); break;
        case 4: launch_mmb_nc<T, 4>(s, a); break;
        case 2: launch_mmb_nc<T, 2>(s, a); break;
        default: launch_mmb_nc<T, 1>(s, a); break;
    }
}

void launch_mmb(hipStream_t s, const mmb_args & a) {
    if (a.M < 1 || a.Hb < 1 || a.E < 1 || a.r2 < 1 || (a.Hb % a.r2) != 0 || (int64_t) a.Hb * a.E > 65535 || a.M > 65535) {  // (grid y and z; graph.cpp: mm_batched_q_ok)
        MI_ERR("launch_mmb: %d columns x %d heads x %d, %d heads a matrix", a.M, a.Hb, a.E, a.r2);
        abort();
    }
    switch (a.type) {
        case GGML_TYPE_Q4_K: launch_mmb_t<T_Q4K>(s, a); break;
        case GGML_TYPE_Q5_K: launch_mmb_t<T_Q5K>(s, a); break;
        case GGML_TYPE_Q6_K: launch_mmb_t<T_Q6K>(s, a); break;
        case GGML_TYPE_Q8_0: launch_mmb_t<T_Q80>(s, a); break;
        case GGML_TYPE_Q4_0: launch_mmb_t<T_Q40>(s, a); break;
        case GGML_TYPE_Q4_1: launch_mmb_t<T_Q41>(s, a); break;
        case GGML_TYPE_Q5_0: launch_mmb_t<T_Q50>(s, a); break;
        case GGML_TYPE_Q5_1: launch_mmb_t<T_Q51>(s, a); break;
        case GGML_TYPE_IQ4_NL: launch_mmb_t<T_IQ4NL>(s, a); break;
        default: MI_ERR("launch_mmb: unsupported weight type %d", a.type); abort();
    }
}

MI_TU_TOUCH(mmb)

}  // namespace mi355x
