// wkv_chunk.hip — RWKV_WKV6 and GATED_LINEAR_ATTN for prompt batches: the chunked restatement of k_rwkv_wkv6 (rwkv.hip) on the f32 matrix cores.  DESIGN.md §4k
// states the operand contract, the restatement and the rounding count; graph.cpp's rwkv_wkv_ok checks the contract, wkv_runs_chunked below routes.  Compiled with
// -ffp-contract=off: every product and sum outside an MFMA is one f32 rounding, in the order written.
//
// One chunk is Q = 16 tokens 0 .. Q-1 of one (sequence, head); S0 [i][j] the state it starts from, d_u[i] = td (WKV6) or g (GLA) of token u,
//     P0_t[i] = product over u < t of d_u[i],      P_(t,s)[i] = product over s < u < t of d_u[i]      (an empty product is 1)
//     WKV6: A[t][s] = sum_i r_t[i] k_s[i] P_(t,s)[i] (s < t),  A[t][t] = sum_i r_t[i] (tf[i] k_t[i]),   Y[t][j] = sum_i (r_t[i] P0_t[i]) S0[i][j] + sum_(s<=t) A[t][s] v_s[j]
//     GLA:  A[t][s] = sum_i qs_t[i] k_s[i] P_(t+1,s)[i] (s <= t),                                       Y[t][j] = sum_i (qs_t[i] P0_(t+1)[i]) S0[i][j] + sum_(s<=t) A[t][s] v_s[j]
//     both: S'[i][j] = P0_Q[i] S0[i][j] + sum_s (k_s[i] P_(Q,s)[i]) v_s[j]
// Every decay here is a RUNNING PRODUCT, reached from its predecessor by one multiplication: no quotient of cumulative decays, no logarithm, no exponential.  A decay
// of exactly 0 (or sixteen of 2^-11 in a row) makes a channel 0 and nothing inf or NaN.  The price: A is no matrix product; it is formed on the vector ALU.
//
// Work split.  A workgroup of NW = MI_WKV_CHUNK_WAVES = 4 waves owns one (sequence, head) and a tile of 16 NW value columns j; wave w owns 16 of them.  The wave's
// slab of the state, S[i][16 columns], lives in MFMA accumulators for the whole token loop (read once, written once): element [16 b + 4 (lane / 16) + v][lane % 16]
// in register 4 b + v.  That is the C / D layout of v_mfma_f32_16x16x4_f32 (tile b) and of v_mfma_f32_16x16x1_f32 (block b of four), and at the same time the B
// operand of the output product: step v of tile b takes k = lane / 16 as i = 16 b + 4 (lane / 16) + v, whose A operand is float v of the float4 a lane reads from
// R~'s LDS row at 16 b + 4 (lane / 16) (the pairing of ssm_chunk.hip).  The state never passes through LDS.
// A chunk, three barriers:
//   1. r (GLA: q * scale, that product's one rounding), k, d of the head [Q][S] and v of the tile [Q][16 NW] go to LDS; rows past the node's tokens are r = k = v = 0, d = 1.
//   2a. thread i < S walks t upward with p = P0: R~[t][i] = r_t[i] P0_t[i] (GLA: qs_t[i] P0_(t+1)[i]) and P0_Q[i] to LDS.
//   2b. A: lane = (s = lane / 4, run = lane % 4) of wave w owns the S / (4 NW) rows i of run (w, run) and keeps kp[i] = k_s[i] P_(t,s)[i] in registers while it walks t
//       upward: a = sum over its i of r_t[i] kp[i] (t == s, WKV6: of r_t[i] (tf[i] k_s[i])), then kp[i] *= d_t[i] (GLA: the multiplication first); the quad finishes
//       the sum with two DPP adds and writes its wave's partial A_w[t][s].  When the walk ends kp IS K~[s][i] = k_s[i] P_(Q,s)[i]: it goes to LDS.  With NW waves
//       the partials are summed ((A_0 + A_1) + A_2) + A_3 where A is read.
//   3. Y = R~ S0 (S / 4 MFMA steps, K = i) + A V (4 steps, K = s) in one accumulator, stored; then st[i][.] *= P0_Q[i] and, s ASCENDING, st += K~[s] (x) v_s as one
//      v_mfma_f32_16x16x1_f32 a token and 64 state rows: a K = 1 step adds ONE product to the accumulator, so the state sums in the serial kernel's order whatever
//      the order in which the hardware would add the four products of a K = 4 step.
// LDS (floats): sR, sK, sD, sRt [Q][S + 4], sKt [Q][S], sV [Q][16 NW + 4], sP [S], sA [NW][Q][20]: 50.7 KB at S 128, 30.5 KB at S 64.  Row strides S + 4, 20
// and 16 NW + 4 put the float4 reads of 16 consecutive rows and the reads of rows 4 apart on different banks.
// Deterministic: fixed orders everywhere, no scratch buffer, no atomics.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WQ = 16;   // tokens a chunk: the M and N of the MFMAs
constexpr int WAS = 20;  // row stride of a partial A, floats

struct wkv_chunk_args {
    const float * k, * v, * r, * tf, * td;  // GLA: r is q, td is g, tf unused
    const float * state;
    float * y, * st_out;
    int H, n_t;
    float scale;
    int vec;  // every operand starts on a 16-byte boundary
};

template <int S, int NW, bool GLA>
__global__ void __launch_bounds__(64 * NW) k_wkv_chunk(const wkv_chunk_args p) {
    constexpr int NT = 64 * NW, RS = S + 4, VS = 16 * NW + 4, S4 = S / 4, NB = S / 64, NI = S / (4 * NW);
    __shared__ __attribute__((aligned(16))) float sR[WQ * RS], sK[WQ * RS], sD[WQ * RS], sRt[WQ * RS], sKt[WQ * S], sV[WQ * VS], sP[S], sA[NW * WQ * WAS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, q = lane >> 4;
    const int h = blockIdx.x / (S / (16 * NW)), j0 = (blockIdx.x % (S / (16 * NW))) * 16 * NW + 16 * w;
    const int seq = blockIdx.y;
    const int64_t C = (int64_t) p.H * S;
    const int64_t hs = (int64_t) h * S;
    const int64_t st_at = ((int64_t) seq * p.H + h) * S * S + (int64_t) (4 * q) * S + j0 + j;  // row 4 q; register 4 b + v is 16 b + v rows further

    f32x16 st[NB];
#pragma unroll
    for (int b = 0; b < S / 16; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) st[b / 4][4 * (b % 4) + v] = p.state[st_at + (int64_t) (16 * b + v) * S];

    // 2b's lane: token s of the chunk, rows i0 .. i0 + NI - 1
    const int as = lane >> 2, i0 = (w * 4 + (lane & 3)) * NI;
    float tf[GLA ? 1 : NI];
    if constexpr (!GLA) {
#pragma unroll
        for (int n = 0; n < NI; ++n) tf[n] = p.tf[hs + i0 + n];
    }

    // A chunk's rows travel global memory -> registers -> LDS (RB float4s of k, r, d and 4 floats of v a thread); rows past the node's tokens are not loaded.  The
    // loads of chunk c + 1 are issued once chunk c stands in LDS and land behind its walks and products.
    constexpr int RB = WQ * S4 / NT;
    float4 fk[RB], fr[RB], fd[RB];
    float fv[4];
    auto fetch = [&](const int t0) {
        const int tc = min(WQ, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
#pragma unroll
        for (int x = 0; x < RB; ++x) {
            const int e = tid + NT * x, t = e / S4, c = 4 * (e % S4);
            fk[x] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            fr[x] = fk[x];
            fd[x] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (t < tc) {
                const int64_t at = (tok0 + t) * C + hs + c;
                if (p.vec) {
                    fk[x] = *(const float4 *) (p.k + at);
                    fr[x] = *(const float4 *) (p.r + at);
                    fd[x] = *(const float4 *) (p.td + at);
                } else {
                    fk[x] = make_float4(p.k[at], p.k[at + 1], p.k[at + 2], p.k[at + 3]);
                    fr[x] = make_float4(p.r[at], p.r[at + 1], p.r[at + 2], p.r[at + 3]);
                    fd[x] = make_float4(p.td[at], p.td[at + 1], p.td[at + 2], p.td[at + 3]);
                }
            }
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int e = tid + NT * x, t = e / (16 * NW), c = e % (16 * NW);
            fv[x] = t < tc ? p.v[(tok0 + t) * C + hs + (j0 - 16 * w) + c] : 0.0f;
        }
    };
    fetch(0);

    for (int t0 = 0; t0 < p.n_t; t0 += WQ) {
        const int tc = min(WQ, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
        __syncthreads();  // the chunk before this one has been read
        // ---- 1
#pragma unroll
        for (int x = 0; x < RB; ++x) {
            const int e = tid + NT * x, t = e / S4, c = 4 * (e % S4);
            *(float4 *) (sK + t * RS + c) = fk[x];
            if constexpr (GLA) *(float4 *) (sR + t * RS + c) = make_float4(fr[x].x * p.scale, fr[x].y * p.scale, fr[x].z * p.scale, fr[x].w * p.scale);
            else *(float4 *) (sR + t * RS + c) = fr[x];
            *(float4 *) (sD + t * RS + c) = fd[x];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int e = tid + NT * x;
            sV[(e / (16 * NW)) * VS + e % (16 * NW)] = fv[x];
        }
        if (t0 + WQ < p.n_t) fetch(t0 + WQ);
        __syncthreads();
        // ---- 2a
        for (int i = tid; i < S; i += NT) {
            float pr = 1.0f;
#pragma unroll
            for (int t = 0; t < WQ; ++t) {
                if constexpr (GLA) pr = pr * sD[t * RS + i];
                sRt[t * RS + i] = sR[t * RS + i] * pr;
                if constexpr (!GLA) pr = pr * sD[t * RS + i];
            }
            sP[i] = pr;
        }
        // ---- 2b
        {
            float kp[NI];
#pragma unroll
            for (int n4 = 0; n4 < NI / 4; ++n4) {
                const float4 k4 = *(const float4 *) (sK + as * RS + i0 + 4 * n4);
                kp[4 * n4] = k4.x; kp[4 * n4 + 1] = k4.y; kp[4 * n4 + 2] = k4.z; kp[4 * n4 + 3] = k4.w;
            }
#pragma unroll
            for (int t = 0; t < WQ; ++t) {
                float a = 0.0f;
#pragma unroll
                for (int n4 = 0; n4 < NI / 4; ++n4) {
                    const float4 r4 = *(const float4 *) (sR + t * RS + i0 + 4 * n4), d4 = *(const float4 *) (sD + t * RS + i0 + 4 * n4);
                    const float rr[4] = {r4.x, r4.y, r4.z, r4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int n = 4 * n4 + u;
                        if constexpr (GLA) {
                            if (t > as) kp[n] = kp[n] * dd[u];
                            if (t >= as) a += rr[u] * kp[n];
                        } else {
                            if (t >= as) a += rr[u] * (t == as ? tf[n] * kp[n] : kp[n]);
                            if (t > as) kp[n] = kp[n] * dd[u];
                        }
                    }
                }
                a += dpp_f32<MI_DPP_QUAD_XOR1>(a);
                a += dpp_f32<MI_DPP_QUAD_XOR2>(a);
                if ((lane & 3) == 0) sA[(w * WQ + t) * WAS + as] = a;
            }
#pragma unroll
            for (int n4 = 0; n4 < NI / 4; ++n4) *(float4 *) (sKt + as * S + i0 + 4 * n4) = make_float4(kp[4 * n4], kp[4 * n4 + 1], kp[4 * n4 + 2], kp[4 * n4 + 3]);
        }
        __syncthreads();
        // ---- 3: Y = R~ S0 + A V
        f32x4 Y = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int b = 0; b < S / 16; ++b) {
            const float4 a4 = *(const float4 *) (sRt + j * RS + 16 * b + 4 * q);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, st[b / 4][4 * (b % 4) + 0], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, st[b / 4][4 * (b % 4) + 1], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, st[b / 4][4 * (b % 4) + 2], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, st[b / 4][4 * (b % 4) + 3], Y, 0, 0, 0);
        }
        {
            float4 a4 = *(const float4 *) (sA + j * WAS + 4 * q);  // A[t = j][s = 4 q + v]
#pragma unroll
            for (int o = 1; o < NW; ++o) {
                const float4 b4 = *(const float4 *) (sA + (o * WQ + j) * WAS + 4 * q);
                a4 = make_float4(a4.x + b4.x, a4.y + b4.y, a4.z + b4.z, a4.w + b4.w);
            }
            const float * vp = sV + (4 * q) * VS + 16 * w + j;
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, vp[0], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, vp[VS], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, vp[2 * VS], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, vp[3 * VS], Y, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = 4 * q + v;
            if (t < tc) p.y[(tok0 + t) * C + hs + j0 + j] = Y[v];
        }
        // ---- 3: S' = diag(P0_Q) S0, then the tokens' outer products in ascending order, one product a K = 1 step
#pragma unroll
        for (int b = 0; b < S / 16; ++b) {
            const float4 p4 = *(const float4 *) (sP + 16 * b + 4 * q);
            st[b / 4][4 * (b % 4) + 0] = st[b / 4][4 * (b % 4) + 0] * p4.x;
            st[b / 4][4 * (b % 4) + 1] = st[b / 4][4 * (b % 4) + 1] * p4.y;
            st[b / 4][4 * (b % 4) + 2] = st[b / 4][4 * (b % 4) + 2] * p4.z;
            st[b / 4][4 * (b % 4) + 3] = st[b / 4][4 * (b % 4) + 3] * p4.w;
        }
#pragma unroll
        for (int s = 0; s < WQ; ++s) {
            const float vs = sV[s * VS + 16 * w + j];
#pragma unroll
            for (int g = 0; g < NB; ++g) st[g] = __builtin_amdgcn_mfma_f32_16x16x1f32(sKt[s * S + 64 * g + lane], vs, st[g], 0, 0, 0);  // block q of A: rows 64 g + 16 q + j
        }
    }
#pragma unroll
    for (int b = 0; b < S / 16; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) p.st_out[st_at + (int64_t) (16 * b + v) * S] = st[b / 4][4 * (b % 4) + v];
}

// which form serves the node: THE one place.  mode: the wkv_chunk switch — 0: the serial kernel everywhere; 2: the chunked form wherever the operands allow (tests,
// measurements); 1: routed — from MI_WKV_CHUNK_MIN_TOKENS tokens a sequence on (kernels.h says what was measured)
bool wkv_runs_chunked(const tdesc & k, const tdesc & state, int mode) {
    const int64_t S = k.ne[0], H = k.ne[1], T = k.ne[2];
    const int64_t n_state = state.ne[0] * state.ne[1] * state.ne[2] * state.ne[3];
    if (mode == 0 || (S != 64 && S != 128) || H < 1 || T < 1 || n_state < S * S * H || n_state % (S * S * H) != 0 || T % (n_state / (S * S * H)) != 0) return false;
    return mode == 2 || T / (n_state / (S * S * H)) >= MI_WKV_CHUNK_MIN_TOKENS;
}

template <int S, bool GLA>
static void launch_wkv_chunk_s(hipStream_t s, const wkv_chunk_args & p, const int n_seqs) {
    constexpr int NW = MI_WKV_CHUNK_WAVES;
    hipLaunchKernelGGL((k_wkv_chunk<S, NW, GLA>), dim3((unsigned) (p.H * (S / (16 * NW))), (unsigned) n_seqs), dim3(64 * NW), 0, s, p);
}
static bool launch_wkv_chunk_any(hipStream_t s, const char * who, const bool gla, const tdesc & k, const tdesc & v, const tdesc & r, const float * tf, const tdesc & td,
                                 const tdesc & state, const tdesc & dst, const float scale) {
    if (!wkv_runs_chunked(k, state, 2)) {
        MI_ERR("%s: head size %lld, %lld heads, %lld tokens are not served here", who, (long long) k.ne[0], (long long) k.ne[1], (long long) k.ne[2]);
        return false;
    }
    const int64_t S = k.ne[0], H = k.ne[1], T = k.ne[2], n_seqs = state.ne[0] * state.ne[1] * state.ne[2] * state.ne[3] / (S * S * H);
    wkv_chunk_args p;
    p.k = (const float *) k.data;
    p.v = (const float *) v.data;
    p.r = (const float *) r.data;
    p.tf = tf;
    p.td = (const float *) td.data;
    p.state = (const float *) state.data;
    p.y = (float *) dst.data;
    p.st_out = p.y + S * H * T;
    p.H = (int) H;
    p.n_t = (int) (T / n_seqs);
    p.scale = scale;
    p.vec = ((((uintptr_t) p.k) | ((uintptr_t) p.r) | ((uintptr_t) p.td)) & 15) == 0;
    if (S == 64) gla ? launch_wkv_chunk_s<64, true>(s, p, (int) n_seqs) : launch_wkv_chunk_s<64, false>(s, p, (int) n_seqs);
    else gla ? launch_wkv_chunk_s<128, true>(s, p, (int) n_seqs) : launch_wkv_chunk_s<128, false>(s, p, (int) n_seqs);
    return true;
}
bool launch_rwkv_wkv6_chunk(hipStream_t s, const tdesc & k, const tdesc & v, const tdesc & r, const tdesc & tf, const tdesc & td, const tdesc & state, const tdesc & dst) {
    return launch_wkv_chunk_any(s, "launch_rwkv_wkv6_chunk", false, k, v, r, (const float *) tf.data, td, state, dst, 1.0f);
}
bool launch_gated_linear_attn_chunk(hipStream_t s, const tdesc & k, const tdesc & v, const tdesc & q, const tdesc & g, const tdesc & state, const tdesc & dst, float scale) {
    return launch_wkv_chunk_any(s, "launch_gated_linear_attn_chunk", true, k, v, q, nullptr, g, state, dst, scale);
}

MI_TU_TOUCH(wkv_chunk)

}  // namespace mi355x
