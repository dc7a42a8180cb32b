// mmf.hip — mat-mul with f16 / f32 src0 (K·Q and V·softmax on the non-flash path, small dense tensors).
//
// Restates ggml_compute_forward_mul_mat for vec_dot_type F16 / F32: when src0 is f16 the
// f32 activations are FIRST rounded to f16 (that is what ggml-cpu's from_float does to src1) and the products are
// accumulated in f32.  ggml broadcasting: src0 dims 2/3 repeat over src1's.
//
// The dot kernel, the 32 x 32 and the 16 x 16 tile kernels are mm_dense.h's templates (shared with the bf16 weights of mmbf.hip), instantiated here for
// elem_f16 (the dot kernel for elem_f32 too); this file keeps the forms only the f16 attention operands have — columns resident, K split over workgroups,
// grouped queries, SOFT_MAX folded in — and the routing.  Every conversion is a member of elem_f16.
#include "mm_dense.h"

namespace mi355x {

// ---- short rows against a batch (K.Q on the non-flash path: K = head size, rows = cells): the 32 x 32 tile kernel of mm_dense.h fetches 16 KB of src1
// and 8 KB of src0 per 32 x 32 tile — 205 MB through the L2 for the 32 x 32 x 7300 logits of a -np 32 step, 39 us.  Here a wave
// keeps its 32 columns of GH heads that share the src0 rows (grouped queries) in registers as f16 A operands — the whole K, at most
// 16 NK — and walks RT row tiles: 8 KB of src0 per tile feed GH x NK MFMAs, the next tile's rows are requested before the current
// one is multiplied.
template <int GH, int NK>
__global__ void __launch_bounds__(256, 2) k_mul_mat_f16_mma_xres(const tdesc a, const tdesc b, const tdesc d, const int RT) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, g = lane >> 5;
    const int64_t K = a.ne[0], col0 = (int64_t) blockIdx.y * 32;
    const int64_t hg = blockIdx.z % (b.ne[2] / GH), i13 = blockIdx.z / (b.ne[2] / GH);  // group of GH src1 heads with one src0 head
    const int64_t i02 = hg * GH / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t tile0 = ((int64_t) blockIdx.x * 4 + wave) * RT, n_tiles = (a.ne[1] + 31) / 32;
    if (tile0 >= n_tiles) return;
    // k-group g of step s: elements 16 s + 8 g ..; past K: the first group is fetched instead and masked to zeros
    elem_f16::vec8 xs[GH][NK];
#pragma unroll
    for (int h = 0; h < GH; ++h) {
        const char * xcol = b.data + std::min<int64_t>(col0 + r32, b.ne[1] - 1) * b.nb[1] + (hg * GH + h) * b.nb[2] + i13 * b.nb[3];
#pragma unroll
        for (int st = 0; st < NK; ++st) {
            const int64_t kk = 16 * st + 8 * g;
            const bool in = kk < K;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            uint4 p0 = *(const uint4 *) (xcol + (in ? kk : 0) * 4), p1 = *(const uint4 *) (xcol + (in ? kk : 0) * 4 + 16);
            p0.x &= keep; p0.y &= keep; p0.z &= keep; p0.w &= keep; p1.x &= keep; p1.y &= keep; p1.z &= keep; p1.w &= keep;
            xs[h][st] = elem_f16::round8(p0, p1);
        }
    }
    const char * abase = a.data + i02 * a.nb[2] + i03 * a.nb[3];
    auto fetch = [&](const int64_t tile, uint4 (&w)[NK]) {
        const char * wrow = abase + std::min<int64_t>(tile * 32 + r32, a.ne[1] - 1) * a.nb[1];
#pragma unroll
        for (int st = 0; st < NK; ++st) {
            const int64_t kk = 16 * st + 8 * g;
            const bool in = kk < K;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            w[st] = *(const uint4 *) (wrow + (in ? kk : 0) * 2);
            w[st].x &= keep; w[st].y &= keep; w[st].z &= keep; w[st].w &= keep;
        }
    };
    uint4 w[NK], wn[NK];
    fetch(tile0, w);
    const int64_t tile_end = std::min<int64_t>(n_tiles, tile0 + RT);
    for (int64_t tile = tile0; tile < tile_end; ++tile) {
        if (tile + 1 < tile_end) fetch(tile + 1, wn);
        const int64_t row = tile * 32 + r32;
#pragma unroll
        for (int h = 0; h < GH; ++h) {
            mm_float16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int st = 0; st < NK; ++st) acc = elem_f16::mfma32(xs[h][st], w[st], acc);
            if (row < a.ne[1]) {
                char * out = d.data + row * d.nb[0] + (hg * GH + h) * d.nb[2] + i13 * d.nb[3];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t col = col0 + (i & 3) + 8 * (i >> 2) + 4 * g;
                    if (col < b.ne[1]) *(float *) (out + col * d.nb[1]) = acc[i];
                }
            }
        }
#pragma unroll
        for (int st = 0; st < NK; ++st) w[st] = wn[st];
    }
}
template <int GH> static void launch_xres_t(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d) {
    const int64_t n_tiles = (a.ne[1] + 31) / 32, ct = (b.ne[1] + 31) / 32, nz = (b.ne[2] / GH) * b.ne[3];
    const int RT = (int) std::max<int64_t>(1, std::min<int64_t>(8, n_tiles * ct * nz / 512));
    dim3 grid((unsigned) ((n_tiles + 4 * RT - 1) / (4 * RT)), (unsigned) ct, (unsigned) nz);
    if (a.ne[0] <= 64) hipLaunchKernelGGL((k_mul_mat_f16_mma_xres<GH, 4>), grid, dim3(256), 0, s, a, b, d, RT);
    else hipLaunchKernelGGL((k_mul_mat_f16_mma_xres<GH, 8>), grid, dim3(256), 0, s, a, b, d, RT);
}

// ---- few columns, at most 128 rows, long rows (V^T.p of a -np decode batch) when scratch is at hand: the 16 x 16 tiles of mm_dense.h fetch
// every probability 8 times and every V^T element twice — 360 MB through the L2 for a 15 MB cache, 45 us.  Here a workgroup's four
// waves cover ALL rows (32 each) of one head over a slice of K, so the probabilities of the slice cross the L2 once (the waves read
// the same lines together), K is cut over workgroups, the partial tiles go to scratch ([slice][batch][column][row]) and
// launch_splitk_reduce adds them in slice order.
template <int NCT>
__global__ void __launch_bounds__(256) k_mul_mat_f16_mma_ksplit(const tdesc a, const tdesc b, float * __restrict__ part, const int64_t Kc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t) wave * 32;
    if (row0 >= a.ne[1]) return;
    const int64_t i12 = blockIdx.y % b.ne[2], i13 = blockIdx.y / b.ne[2];
    const int64_t i02 = i12 / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t kb = (int64_t) blockIdx.x * Kc, ke = std::min<int64_t>(a.ne[0], kb + Kc);
    const char * wrow = a.data + std::min<int64_t>(row0 + r32, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2] + i03 * a.nb[3] + g * 16;
    const char * xcol[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) xcol[ct] = b.data + std::min<int64_t>(ct * 32 + r32, b.ne[1] - 1) * b.nb[1] + i12 * b.nb[2] + i13 * b.nb[3] + g * 32;
    mm_float16 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = (mm_float16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = kb; k < ke; k += 64) {
        uint4 w[4], x0[4][NCT], x1[4][NCT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t kk = k + 16 * u;
            const bool in = kk + 8 * g < ke;
            const int64_t kc = in ? kk : -8 * g;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            w[u] = *(const uint4 *) (wrow + kc * 2);
            w[u].x &= keep; w[u].y &= keep; w[u].z &= keep; w[u].w &= keep;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                x0[u][ct] = *(const uint4 *) (xcol[ct] + kc * 4);
                x1[u][ct] = *(const uint4 *) (xcol[ct] + kc * 4 + 16);
                x0[u][ct].x &= keep; x0[u][ct].y &= keep; x0[u][ct].z &= keep; x0[u][ct].w &= keep;
                x1[u][ct].x &= keep; x1[u][ct].y &= keep; x1[u][ct].z &= keep; x1[u][ct].w &= keep;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = elem_f16::mfma32(elem_f16::round8(x0[u][ct], x1[u][ct]), w[u], acc[ct]);
    }
    const int64_t row = row0 + r32;
    if (row >= a.ne[1]) return;
    float * out = part + ((int64_t) blockIdx.x * gridDim.y + blockIdx.y) * b.ne[1] * a.ne[1] + row;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t col = ct * 32 + (i & 3) + 8 * (i >> 2) + 4 * g;
            if (col < b.ne[1]) out[col * a.ne[1]] = acc[ct][i];
        }
}
// slices of K for the form above (0: the form does not apply)
static int mmf_ksplit_slices(const tdesc & a, const tdesc & b, int64_t * Kc_out) {
    const int64_t K = a.ne[0], nbatch = b.ne[2] * b.ne[3];
    if (a.type != GGML_TYPE_F16 || b.ne[1] < 2 || b.ne[1] > 64 || a.ne[1] > 128 || (a.ne[1] % 4) != 0 || K < 2048 || b.ne[2] % a.ne[2] != 0 || b.ne[3] % a.ne[3] != 0) return 0;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(K / 256, 512 / std::max<int64_t>(1, nbatch)));
    const int64_t Kc = ((K + want - 1) / want + 63) / 64 * 64;
    if (Kc_out) *Kc_out = Kc;
    return (int) ((K + Kc - 1) / Kc);
}
size_t mul_mat_f_workspace_bytes(const tdesc & a, const tdesc & b) {
    const int ks = mmf_ksplit_slices(a, b, nullptr);
    return ks <= 1 ? 0 : (size_t) ks * (size_t) (b.ne[2] * b.ne[3] * b.ne[1] * a.ne[1]) * sizeof(float);
}

// ---- one column against an f16 src0 that G heads of src1 share (K.q and V^T.p of a decode step on the non-flash path with grouped
// queries: a.ne[2] KV heads, b.ne[2] = G a.ne[2] query heads).  The dot kernel above runs one workgroup per (rows, query head): every
// src0 row is fetched G times and each wave waits out one or two dependent loads — 10 us per call at 2k cells, for 4.7 MB.  Here a
// row owner fetches its slice of the row ONCE and feeds G accumulators (src1 is rounded to f16 first, as from_float does), with
// several rows' loads in flight:
//   short rows (K <= 512, K.q: rows = cells): LPR lanes own a row, 4 rows per owner, 64 x 4 / LPR rows per wave;
//   long rows (V^T.p: K = cells): a wave owns 4 rows, the 4 waves of the workgroup take K in interleaved 512-element slices and
//   add up through LDS.
// f32 accumulation in a different order than the dot kernel (and the CPU); same NMSE gate (tests/test_gpu_ops.py::test_mul_mat_f).
// sum over each group of LPR consecutive lanes, on the DPP path (the 64 ds_bpermute a shuffle butterfly needs here — 16 sums, 4
// dependent steps each — were 3.7 of the kernel's 7.8 us: scripts/ubench/attn_probe.hip)
template <int LPR> __device__ __forceinline__ float mmf_group_sum(float v) {
    if (LPR == 64) return wave_sum(v);
    if (LPR >= 16) {
        v = row16_sum(v);
        if (LPR == 32) v += __shfl_xor(v, 16, 64);
        return v;
    }
    v += dpp_f32<MI_DPP_QUAD_XOR1>(v);
    v += dpp_f32<MI_DPP_QUAD_XOR2>(v);
    v += dpp_f32<MI_DPP_HALF_MIRROR>(v);
    return v;
}
template <int G, int LPR>
__global__ void __launch_bounds__(256) k_mul_mat_f16_gqa_short(const tdesc a, const tdesc b, const tdesc d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int lpr = LPR;
    const int rpw = 64 / lpr, sub = lane / lpr, sl = lane % lpr;
    const int64_t i02 = blockIdx.y, K = a.ne[0];
    const int64_t base = (int64_t) blockIdx.x * 16 * rpw + wave * rpw + sub;  // owner's rows: base + 4 rpw r
    const bool kin = (int64_t) sl * 8 < K;
    float x[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (kin) elem_f16::x8(b.data + (i02 * G + g) * b.nb[2] + (int64_t) sl * 32, x[g]);
        else
#pragma unroll
            for (int i = 0; i < 8; ++i) x[g][i] = 0.0f;
    }
    float w[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = std::min<int64_t>(base + 4 * rpw * r, a.ne[1] - 1);
        if (kin) elem_f16::load8(a.data + row * a.nb[1] + i02 * a.nb[2] + (int64_t) sl * 16, w[r]);
        else
#pragma unroll
            for (int i = 0; i < 8; ++i) w[r][i] = 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = base + 4 * rpw * r;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fmaf(w[r][i], x[g][i], acc);
            acc = mmf_group_sum<LPR>(acc);
            if (sl == 0 && row < a.ne[1]) *(float *) (d.data + row * d.nb[0] + (i02 * G + g) * d.nb[2]) = acc;
        }
    }
}
template <int G>
__global__ void __launch_bounds__(256) k_mul_mat_f16_gqa_long(const tdesc a, const tdesc b, const tdesc d) {
    __shared__ float part[4][4 * G];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i02 = blockIdx.y, K = a.ne[0], row0 = (int64_t) blockIdx.x * 4;
    const char * wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = a.data + std::min<int64_t>(row0 + r, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2];
    float acc[4][G];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[r][g] = 0.0f;
    for (int64_t k = (int64_t) wave * 512 + lane * 8; k < K; k += 2048) {
        float w[4][8], x[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) elem_f16::load8(wr[r] + k * 2, w[r]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            elem_f16::x8(b.data + (i02 * G + g) * b.nb[2] + k * 4, x);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[r][g] = fmaf(w[r][i], x[i], acc[r][g]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = wave_sum(acc[r][g]);
            if (lane == 0) part[wave][r * G + g] = v;
        }
    __syncthreads();
    if (threadIdx.x < 4 * G) {
        const int r = threadIdx.x / G, g = threadIdx.x % G;
        const float v = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        if (row0 + r < a.ne[1]) *(float *) (d.data + (row0 + r) * d.nb[0] + (i02 * G + g) * d.nb[2]) = v;
    }
}
// ---- SOFT_MAX(K.q) folded into V^T.p (a decode step on the non-flash path): the long-row layout above with 8 waves, whose 512 threads
// x 8 cells tile the whole row.  The workgroup first turns its slices of the G logit rows into probabilities —
// ggml_compute_forward_soft_max_f32 as ops.hip restates it: w = x scale + mask, max, e = expf(w - max), sum in double, llama-box's
// zero-sum guard, p = e (1 / sum) — and feeds them (rounded to f16, as from_float would) to the products.  One launch and one round
// trip of the probabilities less; every row group of a KV head repeats the G rows' exponentials (32 x for 128 dims / 4), so the work
// per thread is kept to one or two 8-cell slices, the logits / exponentials stay in registers between the passes when the row is
// short enough (NIT slices of 4096 cells; NIT = 0: re-read and recomputed), and the V^T slices are requested before the statistics
// are made.  The per-thread partial sums cover other cells than soft_max's own kernel; they are doubles, the float reciprocal is
// the same in all but freak cases.  scripts/ubench/attn_probe.hip: 6.7 + 5.6 us as two launches at 2304 cells.
#define SMM_NW 8
template <int G, int NIT>
__global__ void __launch_bounds__(64 * SMM_NW) k_soft_max_mul_mat_f16(const tdesc a, const tdesc kq, const tdesc m, const int has_mask, const tdesc d, const float scale) {
    __shared__ float shm[SMM_NW][G];
    __shared__ double shs[SMM_NW][G];
    __shared__ float part[SMM_NW][4 * G];
    constexpr int64_t STEP = 512 * SMM_NW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i02 = blockIdx.y, K = a.ne[0], row0 = (int64_t) blockIdx.x * 4;
    const bool m16 = m.type == GGML_TYPE_F16;
    const int64_t k0 = (int64_t) wave * 512 + lane * 8;
    auto logits = [&](const int g, const int64_t k, float (&w)[8]) {
        const int64_t h = i02 * G + g;
        const char * xp = kq.data + h * kq.nb[2] + k * 4;
        float t[8];
        elem_f32::load8(xp, t);
        if (has_mask) {
            const char * mp = m.data + (h % m.ne[2]) * m.nb[2];
            float mv[8];
            if (m16) elem_f16::load8(mp + k * 2, mv);
            else elem_f32::load8(mp + k * 4, mv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float v = t[i] * scale;
                v += mv[i];
                w[i] = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = t[i] * scale;
        }
    };
    const char * wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = a.data + std::min<int64_t>(row0 + r, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2];
    constexpr int NC = NIT > 0 ? NIT : 1;
    uint4 vq[NC][4];  // this thread's slices of the 4 V^T rows (NIT > 0)
    if (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NC; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) vq[it][r] = k0 + STEP * it < K ? *(const uint4 *) (wr[r] + (k0 + STEP * it) * 2) : make_uint4(0, 0, 0, 0);
    }
    float e[NC][G][8];  // logits, then exponentials (NIT > 0)
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) mx[g] = -INFINITY;
    if (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NC; ++it)
            if (k0 + STEP * it < K)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    logits(g, k0 + STEP * it, e[it][g]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) mx[g] = fmaxf(mx[g], e[it][g][i]);
                }
    } else {
        for (int64_t k = k0; k < K; k += STEP)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float w[8];
                logits(g, k, w);
#pragma unroll
                for (int i = 0; i < 8; ++i) mx[g] = fmaxf(mx[g], w[i]);
            }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float v = wave_max(mx[g]);
        if (lane == 0) shm[wave][g] = v;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float v = shm[0][g];
#pragma unroll
        for (int w = 1; w < SMM_NW; ++w) v = fmaxf(v, shm[w][g]);
        mx[g] = v;
    }
    double sum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0;
    if (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NC; ++it)
            if (k0 + STEP * it < K)
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        e[it][g][i] = expf(e[it][g][i] - mx[g]);
                        sum[g] += (double) e[it][g][i];
                    }
    } else {
        for (int64_t k = k0; k < K; k += STEP)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float w[8];
                logits(g, k, w);
#pragma unroll
                for (int i = 0; i < 8; ++i) sum[g] += (double) expf(w[i] - mx[g]);
            }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double v = wave_sum_d(sum[g]);
        if (lane == 0) shs[wave][g] = v;
    }
    __syncthreads();
    float inv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double t = shs[0][g];
#pragma unroll
        for (int w = 1; w < SMM_NW; ++w) t += shs[w][g];
        if (isnan(t) || t == 0.0) t = -INFINITY;
        inv[g] = (float) (1.0 / t);
    }
    float acc[4][G];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[r][g] = 0.0f;
    auto product = [&](const int64_t k, const int it) {
        float w[4][8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (NIT > 0) elem_f16::unpack8(vq[it][r], w[r]);
            else elem_f16::load8(wr[r] + k * 2, w[r]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float x[8];
            if (NIT > 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = elem_f16::round1(e[it][g][i] * inv[g]);
            } else {
                logits(g, k, x);
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = elem_f16::round1(expf(x[i] - mx[g]) * inv[g]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[r][g] = fmaf(w[r][i], x[i], acc[r][g]);
        }
    };
    if (NIT > 0) {
#pragma unroll
        for (int it = 0; it < NC; ++it)
            if (k0 + STEP * it < K) product(k0 + STEP * it, it);
    } else {
        for (int64_t k = k0; k < K; k += STEP) product(k, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = wave_sum(acc[r][g]);
            if (lane == 0) part[wave][r * G + g] = v;
        }
    __syncthreads();
    if (threadIdx.x < 4 * G) {
        const int r = threadIdx.x / G, g = threadIdx.x % G;
        float v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SMM_NW; ++w) v += part[w][threadIdx.x];
        if (row0 + r < a.ne[1]) *(float *) (d.data + (row0 + r) * d.nb[0] + (i02 * G + g) * d.nb[2]) = v;
    }
}
template <int G, int MAXC>
static void launch_smm_t(hipStream_t s, dim3 grid, int nit, const tdesc & a, const tdesc & kq, const tdesc & md, int has_mask, const tdesc & d, float scale) {
#define SMM(NIT_) hipLaunchKernelGGL((k_soft_max_mul_mat_f16<G, NIT_>), grid, dim3(64 * SMM_NW), 0, s, a, kq, md, has_mask, d, scale)
    if (nit == 1) { SMM(1); return; }
    if constexpr (MAXC >= 2) if (nit == 2) { SMM(2); return; }
    if constexpr (MAXC >= 4) if (nit <= 4) { SMM(4); return; }
    SMM(0);
#undef SMM
}
// a = the f16 matrix (V^T view), kq = the logits SOFT_MAX reads, d = the product; false: shapes this kernel does not serve (the caller
// runs SOFT_MAX and MUL_MAT on their own)
bool launch_soft_max_mul_mat_f16(hipStream_t s, const tdesc & a, const tdesc & kq, const tdesc * mask, const tdesc & d, const float scale) {
    const int64_t K = a.ne[0];
    if (a.type != GGML_TYPE_F16 || !mm_vec_ok(a, kq, 2) || kq.ne[0] != K || kq.ne[1] != 1 || kq.ne[3] != 1 || a.ne[3] != 1 || kq.ne[2] % a.ne[2] != 0 || d.nb[0] != 4) return false;
    if (mask) {
        const int esz = mask->type == GGML_TYPE_F16 ? 2 : 4;
        if ((mask->type != GGML_TYPE_F16 && mask->type != GGML_TYPE_F32) || mask->nb[0] != esz || mask->ne[0] < K || mask->ne[3] != 1 || (((uintptr_t) mask->data) & 15) || (mask->nb[2] % 16)) return false;
    }
    const int G = (int) (kq.ne[2] / a.ne[2]);
    const int nit = (int) ((K + 512 * SMM_NW - 1) / (512 * SMM_NW));
    const tdesc md = mask ? *mask : kq;
    dim3 grid((unsigned) ((a.ne[1] + 3) / 4), (unsigned) a.ne[2]);
    switch (G) {  // cached logits / exponentials: at most 64 registers
        case 1: launch_smm_t<1, 4>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 2: launch_smm_t<2, 4>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 3: launch_smm_t<3, 2>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 4: launch_smm_t<4, 2>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 5: launch_smm_t<5, 1>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 6: launch_smm_t<6, 1>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 7: launch_smm_t<7, 1>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        case 8: launch_smm_t<8, 1>(s, grid, nit, a, kq, md, mask ? 1 : 0, d, scale); return true;
        default: break;
    }
    return false;
}

template <int G> static void launch_gqa_t(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d) {
    const int64_t K = a.ne[0];
    if (K <= 512) {
        const int lpr = mm_lanes_per_row(K, 8);
        const int rows_per_block = 16 * (64 / lpr);
        dim3 grid((unsigned) ((a.ne[1] + rows_per_block - 1) / rows_per_block), (unsigned) a.ne[2]);
        switch (lpr) {
            case 8: hipLaunchKernelGGL((k_mul_mat_f16_gqa_short<G, 8>), grid, dim3(256), 0, s, a, b, d); break;
            case 16: hipLaunchKernelGGL((k_mul_mat_f16_gqa_short<G, 16>), grid, dim3(256), 0, s, a, b, d); break;
            case 32: hipLaunchKernelGGL((k_mul_mat_f16_gqa_short<G, 32>), grid, dim3(256), 0, s, a, b, d); break;
            default: hipLaunchKernelGGL((k_mul_mat_f16_gqa_short<G, 64>), grid, dim3(256), 0, s, a, b, d); break;
        }
    } else {
        dim3 grid((unsigned) ((a.ne[1] + 3) / 4), (unsigned) a.ne[2]);
        hipLaunchKernelGGL(k_mul_mat_f16_gqa_long<G>, grid, dim3(256), 0, s, a, b, d);
    }
}

void launch_mul_mat_f(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, float * ws, size_t ws_bytes) {
    if (a.type == GGML_TYPE_BF16) {  // a weight matrix kept in bf16: its own kernels and routing (mmbf.hip)
        launch_mul_mat_bf16(s, a, b, d);
        return;
    }
    const int64_t K = a.ne[0];
    const bool w16 = a.type == GGML_TYPE_F16;
    const bool vec_ok = mm_vec_ok(a, b, w16 ? 2 : 4);
    if (w16 && vec_ok && ws && d.nb[0] == 4 && d.nb[1] == d.ne[0] * 4 && d.nb[2] == d.nb[1] * d.ne[1] && d.nb[3] == d.nb[2] * d.ne[2]) {
        int64_t Kc = 0;
        const int ks = mmf_ksplit_slices(a, b, &Kc);
        if (ks > 1 && mul_mat_f_workspace_bytes(a, b) <= ws_bytes) {
            const int64_t nbatch = b.ne[2] * b.ne[3];
            dim3 grid((unsigned) ks, (unsigned) nbatch);
            if (b.ne[1] <= 32) hipLaunchKernelGGL(k_mul_mat_f16_mma_ksplit<1>, grid, dim3(256), 0, s, a, b, ws, Kc);
            else hipLaunchKernelGGL(k_mul_mat_f16_mma_ksplit<2>, grid, dim3(256), 0, s, a, b, ws, Kc);
            launch_splitk_reduce(s, ws, ks, (int) (nbatch * b.ne[1]), (int) a.ne[1], (float *) d.data, a.ne[1], nullptr, 0);
            return;
        }
    }
    if (w16 && vec_ok && b.ne[1] >= 2) {
        const int64_t waves32 = ((a.ne[1] + 31) / 32) * ((b.ne[1] + 31) / 32) * b.ne[2] * b.ne[3];
        if (b.ne[1] < 16 || (K >= 1024 && waves32 < 2048)) {  // few tiles, long rows (or a handful of columns): split K inside the workgroup
            launch_mul_mat_mma16<elem_f16>(s, a, b, d);
            return;
        }
    }
    if (w16 && vec_ok && b.ne[1] >= 16 && K <= 128 && a.ne[1] >= 256 && b.ne[2] % a.ne[2] == 0) {  // short rows, many of them (K.Q): columns resident
        const int64_t gq = b.ne[2] / a.ne[2];
        if (gq % 2 == 0) launch_xres_t<2>(s, a, b, d);  // (4 heads' columns = 128 registers: with the row buffers past 256, one wave per SIMD, or spills)
        else launch_xres_t<1>(s, a, b, d);
        return;
    }
    if (w16 && vec_ok && b.ne[1] >= 16) {  // a batch of columns: the matrix cores
        dim3 grid((unsigned) ((a.ne[1] + 63) / 64), (unsigned) ((b.ne[1] + 63) / 64), (unsigned) (b.ne[2] * b.ne[3]));
        hipLaunchKernelGGL((k_mul_mat_mma<elem_f16, false>), grid, dim3(256), 0, s, a, b, d);
        return;
    }
    if (w16 && vec_ok && b.ne[1] == 1 && a.ne[3] == 1 && b.ne[3] == 1 && b.ne[2] % a.ne[2] == 0 && a.ne[1] >= 64) {  // a decode step's K.q / V^T.p
        switch (b.ne[2] / a.ne[2]) {
            case 1: launch_gqa_t<1>(s, a, b, d); return;
            case 2: launch_gqa_t<2>(s, a, b, d); return;
            case 3: launch_gqa_t<3>(s, a, b, d); return;
            case 4: launch_gqa_t<4>(s, a, b, d); return;
            case 5: launch_gqa_t<5>(s, a, b, d); return;
            case 6: launch_gqa_t<6>(s, a, b, d); return;
            case 7: launch_gqa_t<7>(s, a, b, d); return;
            case 8: launch_gqa_t<8>(s, a, b, d); return;
            default: break;
        }
    }
    if (w16) launch_mul_mat_dot<elem_f16>(s, a, b, d, vec_ok);
    else launch_mul_mat_dot<elem_f32>(s, a, b, d, vec_ok);
}


MI_TU_TOUCH(mmf)

}  // namespace mi355x
