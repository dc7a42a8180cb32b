// fattn_hd.hip — FLASH_ATTN_EXT over an f16 K / V at the head sizes that are a multiple of 8 but of neither 32 nor a power of two: 72, 80, 88 (SigLIP / Gemma-3,
// Qwen2-VL and 1408 / 16 vision towers; Phi-2, StableLM-3B) and 112.  Same contract as fattn.hip / fattn_mma.hip (Q rounded to f16, s = (K.Q) * scale (+ softcap)
// + slope * mask, -inf cells skipped, online softmax, f32 accumulation of P.V); what differs is how a row of D halves is laid over lanes and matrix-core steps:
//
//   k_fattn_split_hd<G>   1 .. 32 tokens (and every soft-capped / ALiBi / sink batch): k_fattn_split on SIXTEEN lanes a row, whatever D is — a trip is 64 cells as at
//                         128.  D / 8 = 9, 10, 11 or 14 of the 16 lanes are live; a dead lane (sl * 8 >= D) issues NO K, V or Q load and holds exact zeros, so
//                         the 16-lane DPP sum of the dot and the element-wise sums of the accumulators are those of the live lanes.  The bytes behind a head's
//                         row belong to the next head, the next cell or nobody: loading them and multiplying by a zero query is not the same thing (0 x NaN).
//   k_fattn_combine_hd    the merge of the split records, a thread per real dimension.
//
// 33 tokens and more run on the matrix cores: k_fattn_mma<96 | 128, NW, false, PAD = true> (fattn_mma.hip), the walk of the other head sizes at a padded column count.
// D is a RUN-TIME value in all three (one instantiation per G, one per (padded size, NW)): records, the cross-wave merge and the stores use the real D, stride D + 2.
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
        l[g] = xrow_allsum(l[g]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = xrow_allsum(acc[g][i]);
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

// ------------------------------------------------------------------------------------------------ launchers
void launch_fattn_combine_hd(hipStream_t s, int D, const float * ws, const float * sinks, const tdesc & dst, int n_q, int n_head, int n_batch, int n_splits) {
    if (!fattn_hd_size(D) || n_splits < 1 || n_splits > 64) { MI_ERR("launch_fattn_combine_hd: head_dim %d with %d splits is not served", D, n_splits); abort(); }
    hipLaunchKernelGGL(k_fattn_combine_hd, dim3((unsigned) n_head, (unsigned) n_q, (unsigned) n_batch), dim3(128), 0, s, ws, sinks, dst, D, n_q, n_head, n_splits);
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
