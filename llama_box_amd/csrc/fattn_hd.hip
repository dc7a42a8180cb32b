// fattn_hd.hip — FLASH_ATTN_EXT over an f16 K / V at the head sizes that are a multiple of 8 but of neither 32 nor a power of two: 72, 80, 88 (SigLIP / Gemma-3,
// Qwen2-VL and 1408 / 16 vision towers; Phi-2, StableLM-3B) and 112.  Same contract as fattn.hip / fattn_mma.hip (Q rounded to f16, s = (K.Q) * scale (+ softcap)
// + slope * mask, -inf cells skipped, online softmax, f32 accumulation of P.V); what differs is how a row of D halves is laid over lanes and matrix-core steps:
//
//   k_fattn_split_hd<G>   1 .. 32 tokens (and every soft-capped / ALiBi / sink batch): k_fattn_split on SIXTEEN lanes a row, whatever D is — a trip is 64 cells as at
//                         128.  D / 8 = 9, 10, 11 or 14 of the 16 lanes are live; a dead lane (sl * 8 >= D) issues NO K, V or Q load and holds exact zeros, so
//                         the 16-lane DPP sum of the dot and the element-wise sums of the accumulators are those of the live lanes.  The bytes behind a head's
//                         row belong to the next head, the next cell or nobody: loading them and multiplying by a zero query is not the same thing (0 x NaN).
//   k_fattn_combine_hd    the merge of the split records, a thread per real dimension.
//   k_fattn_mma_hd<DP, NW> 33 tokens and more: k_fattn_mma computed at the padded size DP = 96 (72 / 80 / 88) or 128 (112).  The pad columns of the staged K tile
//                         and the pad entries of the query fragments are WRITTEN as zeros and never loaded, so every padded product adds an exact zero; V is
//                         staged for the real D / 8 chunks only (the pad rows of V^T are zeroed once: their output rows are never stored); output and record
//                         stores skip the runs at d0 >= D.  72 and 88 end in a half-live k-step (8 of its 16 dims).
//
// D is a RUN-TIME value in all three (one instantiation per G, one per (DP, NW)): records, the cross-wave merge and the stores use the real D, stride D + 2.
// DESIGN.md §4d has the resource table, the timings and what was not chosen.
#include <algorithm>
#include <cmath>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

struct fa_hd_geom {
    int D, n_q, n_head, n_kv_head, n_kv, n_splits, has_mask;
    float scale, softcap, max_bias, m0, m1;
    uint32_t n_head_log2;
};

// element-wise all-reduce over the four 16-lane DPP rows of a wave (fattn.hip: xrow_allsum)
static __device__ __forceinline__ float hd_xrow_allsum(const float x) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    float y = a + b;
    a = y;
    b = y;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}

#define FA_HD_SH 116  // floats per (wave, head) slot of the cross-wave merge: 112 values, max, sum, 2 pad (16-byte aligned rows)

template <int G>
__global__ void __launch_bounds__(256) k_fattn_split_hd(const tdesc q, const tdesc k, const tdesc v, const tdesc mask, const float * __restrict__ sinks, const tdesc dst,
                                                        const fa_hd_geom geo, float * __restrict__ ws) {
    constexpr int ROWL = 16;            // lanes per K / V row, live or not
    constexpr int ROWS = 64 / ROWL;     // rows per wave-instruction
    constexpr int NGRP = 4;             // row groups in flight per wave and trip
    constexpr int CELLS = NGRP * 4 * ROWS;  // cells per workgroup trip: 64
    __shared__ __attribute__((aligned(16))) float sh[4][G][FA_HD_SH];
    const int D = geo.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane / ROWL, sl = lane % ROWL;
    const bool live = sl * 8 < D;  // (D is a multiple of 8: a lane's eight dims are all real or all padding)
    const int split = blockIdx.x, kvh = blockIdx.y;
    const int tok = blockIdx.z % geo.n_q, bat = blockIdx.z / geo.n_q;
    const int per = (geo.n_kv + geo.n_splits - 1) / geo.n_splits;
    const int kv0 = split * per, kv1 = min(geo.n_kv, kv0 + per);
    const int64_t kb = bat / (q.ne[3] / k.ne[3]), vb = bat / (q.ne[3] / v.ne[3]);
    const uint16_t * mp = geo.has_mask ? (const uint16_t *) (mask.data + (int64_t) tok * mask.nb[1] + (int64_t) (bat % mask.ne[3]) * mask.nb[3]) : nullptr;
    const char * kbase = k.data + (int64_t) kvh * k.nb[2] + kb * k.nb[3] + sl * 16;
    const char * vbase = v.data + (int64_t) kvh * v.nb[2] + vb * v.nb[3] + sl * 16;

    uint4 kraw[NGRP], vraw[NGRP];
    float mv[NGRP];
    bool inr[NGRP];
    int p0 = kv0 + wave * ROWS;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
#define FA_HD_LOAD_TRIP()                                                                \
    _Pragma("unroll") for (int u = 0; u < NGRP; ++u) {                                  \
        const int p = p0 + u * 4 * ROWS + sub;                                           \
        inr[u] = p < kv1;                                                                \
        const int pc = min(p, kv1 - 1);                                                  \
        mv[u] = mp ? h2f(mp[pc]) : 0.0f;                                                 \
        kraw[u] = z4;                                                                    \
        vraw[u] = z4;                                                                    \
        if (live) { /* a dead lane's address lies behind the head's row: never formed into a load */ \
            kraw[u] = *(const uint4 *) (kbase + (int64_t) pc * k.nb[1]);                 \
            vraw[u] = *(const uint4 *) (vbase + (int64_t) pc * v.nb[1]);                 \
        }                                                                                \
    }
    if (kv0 < kv1) { FA_HD_LOAD_TRIP() }

    float qr[G][8], acc[G][8], m[G], l[G], slope[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int h = kvh * G + g;
        float4 qa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qb = qa;
        if (live) {
            const float4 * qp = (const float4 *) ((const float *) (q.data + (int64_t) tok * q.nb[1] + (int64_t) h * q.nb[2] + (int64_t) bat * q.nb[3]) + sl * 8);
            qa = qp[0];
            qb = qp[1];
        }
        const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            qr[g][i] = h2f(f2h(qv[i]));  // q_to_vec_dot: Q is converted to K's vec_dot_type (f16)
            acc[g][i] = 0.0f;
        }
        m[g] = -INFINITY;
        l[g] = 0.0f;
        slope[g] = geo.max_bias > 0.0f ? ((uint32_t) h < geo.n_head_log2 ? powf(geo.m0, (float) (h + 1)) : powf(geo.m1, (float) (2 * (h - geo.n_head_log2) + 1))) : 1.0f;
    }

    // one softmax state per wave, as k_fattn_split: all scores of a trip, the wave-wide maximum, one rescale, then the exponentials
    while (p0 < kv1) {
        float sc[NGRP][G];
        float vf[NGRP][8];
#pragma unroll
        for (int u = 0; u < NGRP; ++u) {
            const uint32_t ku[4] = {kraw[u].x, kraw[u].y, kraw[u].z, kraw[u].w}, vu[4] = {vraw[u].x, vraw[u].y, vraw[u].z, vraw[u].w};
            float kf[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                kf[2 * i] = h2f((uint16_t) (ku[i] & 0xFFFF));
                kf[2 * i + 1] = h2f((uint16_t) (ku[i] >> 16));
                vf[u][2 * i] = h2f((uint16_t) (vu[i] & 0xFFFF));
                vf[u][2 * i + 1] = h2f((uint16_t) (vu[i] >> 16));
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float t = 0.0f;
#pragma unroll
                for (int i = 0; i < 8; ++i) t = fmaf(kf[i], qr[g][i], t);
                t = row16_sum(t);  // (dead lanes add +0.0)
                float sv = t * geo.scale;
                if (geo.softcap != 0.0f) sv = geo.softcap * tanhf(sv);
                const float mvs = slope[g] * mv[u];
                sv += mvs;
                sc[u][g] = (inr[u] && !(mvs == -INFINITY)) ? sv : -INFINITY;
            }
        }
        if (p0 + CELLS < kv1) {  // the next trip's loads go out before the exponentials
            p0 += CELLS;
            FA_HD_LOAD_TRIP()
            p0 -= CELLS;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float mx = sc[0][g];
#pragma unroll
            for (int u = 1; u < NGRP; ++u) mx = fmaxf(mx, sc[u][g]);
            mx = wave_max(mx);
            const float mn = fmaxf(m[g], mx);
            if (mn == -INFINITY) continue;  // wave-uniform: nothing visible yet
            const float alpha = m[g] == -INFINITY ? 0.0f : expf(m[g] - mn);
            float ps = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[g][i] *= alpha;
#pragma unroll
            for (int u = 0; u < NGRP; ++u) {
                const float pe = sc[u][g] == -INFINITY ? 0.0f : expf(sc[u][g] - mn);
                ps += pe;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[g][i] = fmaf(pe, vf[u][i], acc[g][i]);
            }
            l[g] = l[g] * alpha + ps;
            m[g] = mn;
        }
        p0 += CELLS;
    }
#undef FA_HD_LOAD_TRIP
    // rows of the wave share (m); their partial sums add up element-wise across the four sub-rows
#pragma unroll
    for (int g = 0; g < G; ++g) {
        l[g] = hd_xrow_allsum(l[g]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = hd_xrow_allsum(acc[g][i]);
    }
    if (sub == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (live) {  // (a dead lane's slot would be the (max, sum) pair and the next head's values)
                *(float4 *) &sh[wave][g][sl * 8] = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
                *(float4 *) &sh[wave][g][sl * 8 + 4] = make_float4(acc[g][4], acc[g][5], acc[g][6], acc[g][7]);
            }
            if (sl == 0) {
                sh[wave][g][FA_HD_SH - 4] = m[g];
                sh[wave][g][FA_HD_SH - 3] = l[g];
            }
        }
    }
    __syncthreads();
    // merge the four waves; one thread per (g, d) of the REAL head size
    for (int e = tid; e < G * D; e += 256) {
        const int g = e / D, dd = e % D;
        const float m0 = sh[0][g][FA_HD_SH - 4], m1 = sh[1][g][FA_HD_SH - 4], m2 = sh[2][g][FA_HD_SH - 4], m3 = sh[3][g][FA_HD_SH - 4];
        const float mt = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        const float c0 = m0 == -INFINITY ? 0.0f : expf(m0 - mt), c1 = m1 == -INFINITY ? 0.0f : expf(m1 - mt);
        const float c2 = m2 == -INFINITY ? 0.0f : expf(m2 - mt), c3 = m3 == -INFINITY ? 0.0f : expf(m3 - mt);
        float a = ((sh[0][g][dd] * c0 + sh[1][g][dd] * c1) + sh[2][g][dd] * c2) + sh[3][g][dd] * c3;
        float lt = ((sh[0][g][FA_HD_SH - 3] * c0 + sh[1][g][FA_HD_SH - 3] * c1) + sh[2][g][FA_HD_SH - 3] * c2) + sh[3][g][FA_HD_SH - 3] * c3;
        const int h = kvh * G + g;
        if (geo.n_splits == 1) {
            if (sinks) {
                const float sk = sinks[h];
                const float mn = fmaxf(mt, sk);
                const float c = mt == -INFINITY ? 0.0f : expf(mt - mn);
                a *= c;
                lt = lt * c + expf(sk - mn);
            }
            float * out = (float *) (dst.data + (int64_t) h * dst.nb[1] + (int64_t) tok * dst.nb[2] + (int64_t) bat * dst.nb[3]);
            out[dd] = a * (1.0f / lt);
        } else {
            float * rec = ws + ((((int64_t) bat * geo.n_q + tok) * geo.n_head + h) * geo.n_splits + split) * (D + 2);
            rec[dd] = a;
            if (dd == 0) {
                rec[D] = mt;
                rec[D + 1] = lt;
            }
        }
    }
}

// k_fattn_combine with a run-time head size: a thread per output dimension (threads at or past D only take part in the wave reductions), lane s of every wave owns
// split s for the (max, sum) pairs; coefficient 0 selects, never multiplies (an empty record's values are anything).  Up to 64 splits.
__global__ void __launch_bounds__(128) k_fattn_combine_hd(const float * __restrict__ ws, const float * __restrict__ sinks, const tdesc dst, const int D, const int n_q, const int n_head,
                                                          const int n_splits) {
    const int h = blockIdx.x, tok = blockIdx.y, bat = blockIdx.z, dd = min((int) threadIdx.x, D - 1), lane = threadIdx.x & 63;
    const float * __restrict__ base = ws + (((int64_t) bat * n_q + tok) * n_head + h) * n_splits * (D + 2);
    const bool has = lane < n_splits;
    const float ms = has ? base[(int64_t) lane * (D + 2) + D] : -INFINITY;
    const float ls = has ? base[(int64_t) lane * (D + 2) + D + 1] : 0.0f;
    float mn = wave_max(ms);
    float sink_term = 0.0f;
    if (sinks) {
        mn = fmaxf(mn, sinks[h]);
        sink_term = expf(sinks[h] - mn);
    }
    const float cs = ms == -INFINITY ? 0.0f : expf(ms - mn);
    const float lt = wave_sum(ls * cs) + sink_term;
    float a = 0.0f;
    for (int u0 = 0; u0 < n_splits; u0 += 8) {  // eight records in flight per thread
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = base[(int64_t) min(u0 + j, n_splits - 1) * (D + 2) + dd];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = u0 + j < n_splits ? readlane_f32(cs, min(u0 + j, 63)) : 0.0f;
            a += c != 0.0f ? r[j] * c : 0.0f;
        }
    }
    if ((int) threadIdx.x < D) {
        float * out = (float *) (dst.data + (int64_t) h * dst.nb[1] + (int64_t) tok * dst.nb[2] + (int64_t) bat * dst.nb[3]);
        out[dd] = a * (1.0f / lt);
    }
}

// ------------------------------------------------------------------------------------------------ 33 tokens and more: the matrix cores at a padded head size
typedef _Float16 hd_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 hd_half4 __attribute__((ext_vector_type(4)));
typedef float hd_float16 __attribute__((ext_vector_type(16)));
typedef uint32_t hd_u32x4 __attribute__((ext_vector_type(4)));

struct fam_hd_geom {
    int D, n_q, n_head, n_kv_head, n_kv, has_mask, n_splits;
    float scale;
};

// k_fattn_mma's walk (fattn_mma.hip has the layout's reasons: S^T = K.Q^T with the query in the accumulator's column, V transposed while staged, tile states, the next
// tile's loads in flight during the two GEMMs) at DP columns of which the first geo.D are real.
// The 64-query workgroup at 128 columns holds 64 staging registers per thread and needs ~275: at two waves per SIMD (256 registers) it spills 17 of them, as
// k_fattn_mma<128, 2> does; this form is told one wave per SIMD instead (two such workgroups per CU, not four) and keeps everything in registers.
template <int DP, int NW>
__global__ void __launch_bounds__(NW * 64, (DP == 128 && NW == 2) ? 1 : 2) k_fattn_mma_hd(const tdesc q, const tdesc k, const tdesc v, const tdesc mask, const tdesc dst, const fam_hd_geom geo, float * __restrict__ ws,
                                                          const uint8_t * __restrict__ vis) {
    static_assert(DP == 96 || DP == 128, "padded head sizes");
    constexpr int TKV = 64;              // cells per tile
    constexpr int KS = (DP + 8) * 2;     // K tile row stride (bytes): an odd multiple of 16 at both padded sizes (13, 17)
    constexpr int VS = (TKV + 4) * 2;    // V^T tile row stride (bytes)
    constexpr int NS = DP / 16;          // k-steps over the padded head dimension
    constexpr int ND = DP / 32;          // output d-tiles
    static_assert((KS / 16) % 2 == 1, "conflict-free ds_read_b128");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char * Kt = smem;                    // [TKV][DP + 8] f16, columns D .. DP - 1 zero
    char * Vt = smem + TKV * KS;         // [DP][TKV + 4] f16 (transposed, swizzled), rows D .. DP - 1 zero

    const int D = geo.D, nch = D >> 3;   // real 16-byte chunks of a K / V row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, kg = lane >> 5;
    const int h = blockIdx.y, bat = blockIdx.z / geo.n_splits, split = blockIdx.z % geo.n_splits;
    const int tiles = (geo.n_kv + TKV - 1) / TKV, tps = (tiles + geo.n_splits - 1) / geo.n_splits;
    const int kv_begin = split * tps * TKV, kv_end = min(geo.n_kv, kv_begin + tps * TKV);
    const int kvh = h / (geo.n_head / geo.n_kv_head);
    const int qi = blockIdx.x * (NW * 32) + wave * 32 + fr;  // this lane's query token
    const int qrow = min(qi, geo.n_q - 1);
    const int64_t kb = bat / (q.ne[3] / k.ne[3]), vb = bat / (q.ne[3] / v.ne[3]);

    // Q^T fragments: step s holds head dims 16s + 8kg .. + 7 of this lane's query — zeros where those are padding (72 / 88: the kg = 1 half of the last real step)
    hd_half8 qf[NS];
    {
        const float * qp = (const float *) (q.data + (int64_t) qrow * q.nb[1] + (int64_t) h * q.nb[2] + (int64_t) bat * q.nb[3]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (2 * s + kg < nch) {
                a = *(const float4 *) (qp + 16 * s + 8 * kg);
                b = *(const float4 *) (qp + 16 * s + 8 * kg + 4);
            }
            qf[s] = (hd_half8){(_Float16) a.x, (_Float16) a.y, (_Float16) a.z, (_Float16) a.w, (_Float16) b.x, (_Float16) b.y, (_Float16) b.z, (_Float16) b.w};
        }
    }
    const uint16_t * mrow = geo.has_mask ? (const uint16_t *) (mask.data + (int64_t) qrow * mask.nb[1] + (int64_t) (bat % mask.ne[3]) * mask.nb[3]) : nullptr;
    const char * kbase = k.data + (int64_t) kvh * k.nb[2] + kb * k.nb[3];
    const char * vbase = v.data + (int64_t) kvh * v.nb[2] + vb * v.nb[3];

    constexpr float LOG2E = 1.4426950408889634f;
    const float sc2 = geo.scale * LOG2E;
    hd_float16 O[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.0f;
    const hd_float16 zero = O[0];
    float m = -INFINITY, l = 0.0f;

    // staging roles.  K: thread -> cell and its CH chunks of the PADDED row (a padding chunk is stored as zeros).  V: thread -> blocks of 4 cells x 8 dims over the
    // REAL chunks only; which block a thread takes does not change from tile to tile, so the division by the run-time chunk count is done once.
    constexpr int T = NW * 64;
    const int srow = tid / NW, spart = tid % NW;
    constexpr int CH = DP / (8 * NW);
    constexpr int VB = (16 * (DP / 8) + T - 1) / T;
    const int nblk = 16 * nch;
    int vblk[VB];  // (group of 4 cells) << 4 | chunk of the row, -1: this thread has no j-th block
#pragma unroll
    for (int j = 0; j < VB; ++j) {
        const int b = tid + j * T;
        vblk[j] = b < nblk ? ((b / nch) << 4) | (b % nch) : -1;
    }
    // the pad rows of V^T: nobody stages them and their output rows are never stored; zero, so that what the matrix cores read is defined
    for (int i = tid; i < (DP - D) * (VS / 8); i += T) *(uint2 *) (Vt + D * VS + i * 8) = make_uint2(0u, 0u);

    const int n_qt = (geo.n_q + 31) / 32;
    const int kt_begin = kv_begin / TKV, kt_end = (kv_end + TKV - 1) / TKV;
    uint8_t * const vt = (uint8_t *) (smem + TKV * KS + DP * VS);  // this split's tile states, the NW query tiles packed into a byte
    if (vis) {
        const uint8_t * visrow = vis + (int64_t) (blockIdx.x * NW) * tiles;
        for (int i = kt_begin + tid; i < kt_end; i += T) {
            uint32_t b = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if ((int) blockIdx.x * NW + w < n_qt) b |= (uint32_t) (visrow[(int64_t) w * tiles + i] & 3) << (2 * w);
            vt[i - kt_begin] = (uint8_t) b;
        }
        __syncthreads();
    }
    auto next_tile = [&](int kt) __attribute__((always_inline)) {
        if (vis)
            while (kt < kt_end && __builtin_amdgcn_readfirstlane((int) vt[kt - kt_begin]) == 0) ++kt;
        return kt;
    };
    hd_u32x4 kr[CH];
    uint4 vr[VB][4];
    auto load_tile = [&](const int kt) __attribute__((always_inline)) {
        const int c0 = kt * TKV;
        {
            const int pos = min(c0 + srow, geo.n_kv - 1);
            const hd_u32x4 * kp = (const hd_u32x4 *) (kbase + (int64_t) pos * k.nb[1]) + spart * CH;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                kr[i] = (hd_u32x4){0u, 0u, 0u, 0u};
                if (spart * CH + i < nch) kr[i] = kp[i];
            }
        }
#pragma unroll
        for (int j = 0; j < VB; ++j) {
            if (vblk[j] < 0) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pos = min(c0 + 4 * (vblk[j] >> 4) + r, geo.n_kv - 1);
                vr[j][r] = *((const uint4 *) (vbase + (int64_t) pos * v.nb[1]) + (vblk[j] & 15));
            }
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < CH; ++i) *(hd_u32x4 *) (Kt + srow * KS + (spart * CH + i) * 16) = kr[i];
#pragma unroll
        for (int j = 0; j < VB; ++j) {
            if (vblk[j] < 0) continue;
            const int kvq = vblk[j] >> 4, dch = vblk[j] & 15;
            const uint32_t r0[4] = {vr[j][0].x, vr[j][0].y, vr[j][0].z, vr[j][0].w}, r1[4] = {vr[j][1].x, vr[j][1].y, vr[j][1].z, vr[j][1].w};
            const uint32_t r2[4] = {vr[j][2].x, vr[j][2].y, vr[j][2].z, vr[j][2].w}, r3[4] = {vr[j][3].x, vr[j][3].y, vr[j][3].z, vr[j][3].w};
            const int kvs = 8 * (kvq ^ (2 * (dch >> 2)));  // (groups of 4 cells XOR-swizzled by the row's 32-dim tile, as k_fattn_mma)
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // dword e of a row holds head dims 2e, 2e + 1
                uint2 lo, hi;
                lo.x = __builtin_amdgcn_perm(r1[e], r0[e], 0x05040100u);
                lo.y = __builtin_amdgcn_perm(r3[e], r2[e], 0x05040100u);
                hi.x = __builtin_amdgcn_perm(r1[e], r0[e], 0x07060302u);
                hi.y = __builtin_amdgcn_perm(r3[e], r2[e], 0x07060302u);
                *(uint2 *) (Vt + (8 * dch + 2 * e) * VS + kvs) = lo;
                *(uint2 *) (Vt + (8 * dch + 2 * e + 1) * VS + kvs) = hi;
            }
        }
    };

    int kt = next_tile(kt_begin);
    if (kt < kt_end) load_tile(kt);
    while (kt < kt_end) {
        const int c0 = kt * TKV;
        const int mine = !vis ? 1 : (int) __builtin_amdgcn_readfirstlane((vt[kt - kt_begin] >> (2 * wave)) & 3);
        const bool tail = c0 + TKV > geo.n_kv;
        __syncthreads();  // nobody reads the previous tile any more (the first time: the pad rows of V^T are written)
        store_tile();
        // the mask words of this tile (only where it is neither hidden nor plainly visible), requested BEFORE the next tile's K / V: vmcnt retires in order
        uint2 mw[2][4] = {};
        const bool use_mask = geo.has_mask != 0 && mine == 1;  // (wave-uniform)
        if (use_mask) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) mw[t][g4] = *(const uint2 *) (mrow + min(c0 + 32 * t + 8 * g4 + 4 * kg, geo.n_kv - 4));
        }
        const int kt_next = next_tile(kt + 1);
        if (kt_next < kt_end) load_tile(kt_next);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        kt = kt_next;
        if (mine == 0) continue;  // none of this wave's queries sees the tile (the barriers are at the loop top)

        hd_float16 S[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            S[t] = zero;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const hd_half8 a = *(const hd_half8 *) (Kt + (32 * t + fr) * KS + (16 * s + 8 * kg) * 2);
                S[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[s], S[t], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
        if (use_mask || tail) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int p0 = c0 + 32 * t + 8 * g4 + 4 * kg;
                    float mv[4] = {0.f, 0.f, 0.f, 0.f};
                    if (use_mask) {
                        mv[0] = h2f((uint16_t) (mw[t][g4].x & 0xFFFF)); mv[1] = h2f((uint16_t) (mw[t][g4].x >> 16));
                        mv[2] = h2f((uint16_t) (mw[t][g4].y & 0xFFFF)); mv[3] = h2f((uint16_t) (mw[t][g4].y >> 16));
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float sv = fmaf(S[t][4 * g4 + e], sc2, mv[e] * LOG2E);
                        if (p0 + e >= geo.n_kv) sv = -INFINITY;
                        S[t][4 * g4 + e] = sv;
                        mx = fmaxf(mx, sv);
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = S[t][r] * sc2;
                    S[t][r] = sv;
                    mx = fmaxf(mx, sv);
                }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        if (__all(m_new == -INFINITY)) continue;
        const float mref = m_new == -INFINITY ? 0.0f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m - mref);
        float rs = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(S[t][r] - mref);
                S[t][r] = p;
                rs += p;
            }
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = m_new;
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                hd_half8 pb;
#pragma unroll
                for (int u = 0; u < 8; ++u) pb[u] = (_Float16) S[t][8 * s2 + u];
                const int kvg = 8 * t + 4 * s2 + kg;
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) {
                    const char * vrow = Vt + (32 * dt + fr) * VS;
                    const hd_half4 a0 = *(const hd_half4 *) (vrow + 8 * (kvg ^ (2 * dt))), a1 = *(const hd_half4 *) (vrow + 8 * ((kvg + 2) ^ (2 * dt)));
                    const hd_half8 a = (hd_half8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pb, O[dt], 0, 0, 0);
                }
            }
        }
    }
    if (qi >= geo.n_q) return;
    if (geo.n_splits == 1) {
        const float inv = 1.0f / l;
        float * out = (float *) (dst.data + (int64_t) h * dst.nb[1] + (int64_t) qi * dst.nb[2] + (int64_t) bat * dst.nb[3]);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * dt + 8 * g4 + 4 * kg;
                if (d0 < D) *(float4 *) (out + d0) = make_float4(O[dt][4 * g4] * inv, O[dt][4 * g4 + 1] * inv, O[dt][4 * g4 + 2] * inv, O[dt][4 * g4 + 3] * inv);
            }
    } else {  // partial record (O relative to m, m, l) at the real stride
        float * rec = ws + ((((int64_t) bat * geo.n_q + qi) * geo.n_head + h) * geo.n_splits + split) * (D + 2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * dt + 8 * g4 + 4 * kg;
                if (d0 < D) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) rec[d0 + e] = O[dt][4 * g4 + e];
                }
            }
        if (kg == 0) {
            rec[D] = m * (1.0f / LOG2E);  // the combine pass works in the natural-log domain
            rec[D + 1] = l;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_fattn_combine_hd(hipStream_t s, int D, const float * ws, const float * sinks, const tdesc & dst, int n_q, int n_head, int n_batch, int n_splits) {
    if (!fattn_hd_size(D) || n_splits < 1 || n_splits > 64) { MI_ERR("launch_fattn_combine_hd: head_dim %d with %d splits is not served", D, n_splits); abort(); }
    hipLaunchKernelGGL(k_fattn_combine_hd, dim3((unsigned) n_head, (unsigned) n_q, (unsigned) n_batch), dim3(128), 0, s, ws, sinks, dst, D, n_q, n_head, n_splits);
}

void launch_fattn_mma_hd(hipStream_t s, const dim3 grid, int nw, size_t vt_bytes, const tdesc & q, const tdesc & k, const tdesc & v, const tdesc & mk, const tdesc & dst, bool has_mask, float scale,
                         int n_splits, float * ws, const uint8_t * tile_vis) {
    fam_hd_geom geo;
    geo.D = (int) k.ne[0];
    geo.n_q = (int) q.ne[1];
    geo.n_head = (int) q.ne[2];
    geo.n_kv_head = (int) k.ne[2];
    geo.n_kv = (int) k.ne[1];
    geo.has_mask = has_mask ? 1 : 0;
    geo.n_splits = n_splits;
    geo.scale = scale;
    if (!fattn_hd_size(geo.D) || (nw != 2 && nw != 4)) { MI_ERR("launch_fattn_mma_hd: head_dim %d on %d waves is not served", geo.D, nw); abort(); }
    const int DP = geo.D <= 96 ? 96 : 128;
    const size_t lds = (size_t) 64 * (DP + 8) * 2 + (size_t) DP * (64 + 4) * 2 + vt_bytes;  // (at most 13 312 + 13 056 / 17 408 + 17 408 bytes of tiles + 16 384 states: below the 64 KB default)
    if (DP == 96) {
        if (nw == 4) hipLaunchKernelGGL((k_fattn_mma_hd<96, 4>), grid, dim3(256), lds, s, q, k, v, mk, dst, geo, ws, tile_vis);
        else hipLaunchKernelGGL((k_fattn_mma_hd<96, 2>), grid, dim3(128), lds, s, q, k, v, mk, dst, geo, ws, tile_vis);
    } else {
        if (nw == 4) hipLaunchKernelGGL((k_fattn_mma_hd<128, 4>), grid, dim3(256), lds, s, q, k, v, mk, dst, geo, ws, tile_vis);
        else hipLaunchKernelGGL((k_fattn_mma_hd<128, 2>), grid, dim3(128), lds, s, q, k, v, mk, dst, geo, ws, tile_vis);
    }
}

// 1 .. 32 tokens, and every batch the matrix cores do not take (soft-capping, ALiBi, sinks, n_kv % 4 != 0): the split kernel and, behind two splits or more, the combine pass
void launch_flash_attn_hd(hipStream_t s, const tdesc & q, const tdesc & k, const tdesc & v, const tdesc * mask, const float * sinks, const tdesc & dst, const fattn_params & p, void * workspace) {
    fa_hd_geom geo{};
    geo.D = (int) k.ne[0];
    geo.n_q = (int) q.ne[1];
    geo.n_head = (int) q.ne[2];
    geo.n_kv_head = (int) k.ne[2];
    geo.n_kv = (int) k.ne[1];
    geo.n_splits = p.n_splits;
    geo.has_mask = mask ? 1 : 0;
    geo.scale = p.logit_softcap != 0.0f ? p.scale / p.logit_softcap : p.scale;
    geo.softcap = p.logit_softcap;
    geo.max_bias = p.max_bias;
    geo.n_head_log2 = 1u << (uint32_t) floor(log2((double) geo.n_head));
    geo.m0 = powf(2.0f, -(p.max_bias) / (float) geo.n_head_log2);
    geo.m1 = powf(2.0f, -(p.max_bias / 2.0f) / (float) geo.n_head_log2);
    const int G = geo.n_kv_head > 0 ? geo.n_head / geo.n_kv_head : 0;
    if (!fattn_hd_size(geo.D) || v.ne[0] != k.ne[0] || p.kv_type != GGML_TYPE_F16 || k.type != GGML_TYPE_F16 || v.type != GGML_TYPE_F16 || p.dq || p.fat || p.lists || p.q8_out || G < 1 || G > 8 ||
        G * geo.n_kv_head != geo.n_head || geo.n_splits < 1 || geo.n_splits > 64) {
        MI_ERR("launch_flash_attn_hd: head_dim %d / group %d / %d splits reached the padded-row kernels in a form they do not serve", geo.D, G, geo.n_splits);
        abort();
    }
    const tdesc mk = mask ? *mask : q;
    float * ws = (float *) workspace;
    const dim3 grid((unsigned) geo.n_splits, (unsigned) geo.n_kv_head, (unsigned) (geo.n_q * q.ne[3]));
    g_fa_form = fa_form_code(FA_FORM_K_SPLIT, 0, 4, FA_FORM_KV_F16, 64, FA_FORM_TAIL_NONE) | fa_form_hd(geo.D);
    switch (G) {
#define FA_HD_CASE(GG) case GG: hipLaunchKernelGGL((k_fattn_split_hd<GG>), grid, dim3(256), 0, s, q, k, v, mk, sinks, dst, geo, ws); break;
        FA_HD_CASE(1) FA_HD_CASE(2) FA_HD_CASE(3) FA_HD_CASE(4) FA_HD_CASE(5) FA_HD_CASE(6) FA_HD_CASE(7) FA_HD_CASE(8)
#undef FA_HD_CASE
    }
    if (geo.n_splits > 1) launch_flash_attn_combine(s, geo.D, ws, sinks, dst, geo.n_q, geo.n_head, (int) q.ne[3], geo.n_splits, nullptr);
}

MI_TU_TOUCH(fattn_hd)

}  // namespace mi355x
