// wkv7_chunk.hip — RWKV_WKV7 for prompt batches: the chunked restatement of k_rwkv_wkv7 (rwkv.hip) on the f32 matrix cores.  DESIGN.md §4k states the operand
// contract, the restatement and the rounding count; graph.cpp's rwkv_wkv_ok checks the contract, wkv7_runs_chunked below routes.  Compiled with -ffp-contract=off:
// every product and sum outside an MFMA is one f32 rounding, in the order written.
//
// One chunk is Q = 16 tokens 0 .. Q-1 of one (sequence, head); S0 [i][j] the state it starts from (i the value row, j reduced),
//     P0_t[j] = product over u < t of w_u[j],      P_(t,s)[j] = product over s < u < t of w_u[j]      (an empty product is 1)
//     state before token t: prev_t[i][j] = S0[i][j] P0_t[j] + sum_(s<t) (v_s[i] k_s[j] + sa_s[i] b_s[j]) P_(t,s)[j]
//     Aak[t][s] = sum_j a_t[j] k_s[j] P_(t,s)[j]      Aab[t][s] = sum_j a_t[j] b_s[j] P_(t,s)[j]      (s < t)
//     Ark[t][s] = sum_j r_t[j] k_s[j] P_(t+1,s)[j]    Arb[t][s] = sum_j r_t[j] b_s[j] P_(t+1,s)[j]    (s <= t)
//     sa_t[i] = sum_j (a_t[j] P0_t[j]) S0[i][j] + sum_(s<t) (Aak[t][s] v_s[i] + Aab[t][s] sa_s[i])     (t ascending: a forward substitution)
//     y_t[i]  = sum_j (r_t[j] P0_(t+1)[j]) S0[i][j] + sum_(s<=t) (Ark[t][s] v_s[i] + Arb[t][s] sa_s[i])
//     S'[i][j] = S0[i][j] P0_Q[j] + sum_s (v_s[i] K~[s][j] + sa_s[i] B~[s][j]),   K~[s] = k_s P_(Q,s),  B~[s] = b_s P_(Q,s)
// Every decay here is a RUNNING PRODUCT, reached from its predecessor by one multiplication: no quotient of cumulative decays, no logarithm, no exponential.  A decay
// of exactly 0 (or sixteen of 2^-11 in a row) makes a column 0 and nothing inf or NaN.  The price: the four A are no matrix products; they are formed on the vector ALU.
//
// Work split.  A workgroup of NW = MI_WKV7_CHUNK_WAVES waves owns one (sequence, head) and a tile of 16 NW value rows i; wave w owns 16 of them, all S columns.  The
// wave's slab lives TRANSPOSED in MFMA accumulators for the whole token loop (read once, written once): element [i = lane % 16][j = 16 b + 4 (lane / 16) + v] in
// register 4 b + v.  That is the C / D layout of v_mfma_f32_16x16x4_f32 (tile b, M = j, N = i) and of v_mfma_f32_16x16x1_f32 (block b of four), and at the same
// time the B operand of the products over j: step v of tile b takes k = lane / 16 as j = 16 b + 4 (lane / 16) + v, whose A operand is float v of the float4 a lane
// reads from a~'s (r~'s) LDS row at 16 b + 4 (lane / 16) — wkv_chunk.hip's pairing with the roles of the two indices exchanged.  The state never passes through LDS.
// A chunk, five barriers:
//   1. r, w, k, a, b of the head [Q][S] and v of the tile [Q][16 NW] go to LDS; rows past the node's tokens are r = k = v = a = b = 0, w = 1.
//   2. the walk.  4 NW lanes share token s = tid / (4 NW); a lane keeps kp = k_s P and bp = b_s P of its S / (4 NW) columns in registers and walks t upward: at t > s
//      it takes a_t . kp (Aak) and a_t . bp (Aab) and multiplies kp, bp by w_t; at t >= s it then takes r_t . kp (Ark) and r_t . bp (Arb).  The lanes of s finish each
//      sum with DPP adds (quad, half row, row: a fixed tree) and one of them writes A[t][s]; nothing is summed across waves.  When the walk ends kp IS K~[s] and bp
//      IS B~[s]: they go back over k_s and b_s, which no other lane reads.
//   3. in place: thread j walks t upward with p = P0: a~[t][j] = a_t[j] P0_t[j] over a, r~[t][j] = r_t[j] P0_(t+1)[j] over r (a second thread), P0_Q[j].
//   4. G = a~ S0^T (S / 4 MFMA steps, K = j) + Aak V (4 steps, K = s) in one accumulator, to the wave's own LDS tile [t][i].
//   5. lane i (all four lane groups alike) substitutes forward: sa_t = G[t][i] + sum_(s<t) Aab[t][s] sa_s, s ascending, the sixteen sa in registers.  Then
//      Y = r~ S0^T + Ark V + Arb SA (S / 4 + 8 steps), stored; then st[.][j] *= P0_Q[j] and, s ASCENDING, st += K~[s] (x) v_s and then st += B~[s] (x) sa_s, each one
//      v_mfma_f32_16x16x1_f32 a 64 columns: a K = 1 step adds ONE product to the accumulator, so the state sums in the serial kernel's order (prev w + v k) + sa b.
// LDS (floats): sR, sW, sK, sA, sB [Q][S + 4], sV [Q][16 NW + 4], sP [S], sM [4][Q][20], sG [NW][Q][20]: 57 344 bytes at S 128, 36 608 at S 64 with four waves.
// Deterministic: fixed orders everywhere, no scratch buffer, no atomics.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int W7Q = 16;   // tokens a chunk: the M and N of the MFMAs
constexpr int W7AS = 20;  // row stride of an A matrix and of a wave's G tile, floats

struct wkv7_chunk_args {
    const float * r, * w, * k, * v, * a, * b;
    const float * state;
    float * y, * st_out;
    int H, n_t;
    int vec;   // r, w, k, a, b start on 16-byte boundaries
    int svec;  // state and st_out too
};

// sum over the LS lanes that share a token of the walk, LS = 4 / 8 / 16 consecutive lanes: the same bits in each of them
template <int LS>
__device__ __forceinline__ float wkv7_group_sum(float x) {
    x += dpp_f32<MI_DPP_QUAD_XOR1>(x);
    x += dpp_f32<MI_DPP_QUAD_XOR2>(x);
    if constexpr (LS >= 8) x += dpp_f32<MI_DPP_HALF_MIRROR>(x);
    if constexpr (LS >= 16) x += dpp_f32<MI_DPP_ROW_MIRROR>(x);
    return x;
}

template <int S, int NW>
__global__ void __launch_bounds__(64 * NW) k_wkv7_chunk(const wkv7_chunk_args p) {
    static_assert(NW == 1 || NW == 2 || NW == 4, "the walk shares a token among 4 NW lanes of one DPP row");
    constexpr int NT = 64 * NW, RS = S + 4, VS = 16 * NW + 4, S4 = S / 4, NB = S / 64, LS = 4 * NW, NI = S / LS;
    __shared__ __attribute__((aligned(16))) float sR[W7Q * RS], sW[W7Q * RS], sK[W7Q * RS], sA[W7Q * RS], sB[W7Q * RS], sV[W7Q * VS], sP[S], sM[4 * W7Q * W7AS],
        sG[NW * W7Q * W7AS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, q = lane >> 4;
    const int h = blockIdx.x / (S / (16 * NW)), i0 = (blockIdx.x % (S / (16 * NW))) * 16 * NW + 16 * w;
    const int seq = blockIdx.y;
    const int64_t C = (int64_t) p.H * S;
    const int64_t hs = (int64_t) h * S;
    const int64_t st_at = (((int64_t) seq * p.H + h) * S + i0 + i) * S + 4 * q;  // row i0 + i, column 4 q; registers 4 b .. 4 b + 3 are 16 b columns further

    f32x16 st[NB];
#pragma unroll
    for (int b = 0; b < S / 16; ++b) {
        const float * s4 = p.state + st_at + 16 * b;
        const float4 x = p.svec ? *(const float4 *) s4 : make_float4(s4[0], s4[1], s4[2], s4[3]);
        st[b / 4][4 * (b % 4) + 0] = x.x; st[b / 4][4 * (b % 4) + 1] = x.y; st[b / 4][4 * (b % 4) + 2] = x.z; st[b / 4][4 * (b % 4) + 3] = x.w;
    }

    // the walk's lane: token as of the chunk, columns 4 (run + LS n4) .. + 3, n4 < NI / 4 (a float4 read of the LS lanes is one contiguous run)
    const int as = tid / LS, run = tid % LS;

    // A chunk's rows travel global memory -> registers -> LDS (RB float4s of r, w, k, a, b and 4 floats of v a thread); rows past the node's tokens are not loaded.
    // The loads of chunk c + 1 are issued once chunk c stands in LDS and land behind its walks and products.
    constexpr int RB = W7Q * S4 / NT;
    float4 fr[RB], fw[RB], fk[RB], fa[RB], fb[RB];
    float fv[4];
    auto ld4 = [&](const float * x) { return p.vec ? *(const float4 *) x : make_float4(x[0], x[1], x[2], x[3]); };
    auto fetch = [&](const int t0) {
        const int tc = min(W7Q, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
#pragma unroll
        for (int x = 0; x < RB; ++x) {
            const int e = tid + NT * x, t = e / S4, c = 4 * (e % S4);
            fr[x] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            fk[x] = fr[x]; fa[x] = fr[x]; fb[x] = fr[x];
            fw[x] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (t < tc) {
                const int64_t at = (tok0 + t) * C + hs + c;
                fr[x] = ld4(p.r + at); fw[x] = ld4(p.w + at); fk[x] = ld4(p.k + at); fa[x] = ld4(p.a + at); fb[x] = ld4(p.b + at);
            }
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int e = tid + NT * x, t = e / (16 * NW), c = e % (16 * NW);
            fv[x] = t < tc ? p.v[(tok0 + t) * C + hs + (i0 - 16 * w) + c] : 0.0f;
        }
    };
    fetch(0);

    for (int t0 = 0; t0 < p.n_t; t0 += W7Q) {
        const int tc = min(W7Q, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
        __syncthreads();  // the chunk before this one has been read
        // ---- 1
#pragma unroll
        for (int x = 0; x < RB; ++x) {
            const int e = tid + NT * x, at = (e / S4) * RS + 4 * (e % S4);
            *(float4 *) (sR + at) = fr[x];
            *(float4 *) (sW + at) = fw[x];
            *(float4 *) (sK + at) = fk[x];
            *(float4 *) (sA + at) = fa[x];
            *(float4 *) (sB + at) = fb[x];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int e = tid + NT * x;
            sV[(e / (16 * NW)) * VS + e % (16 * NW)] = fv[x];
        }
        if (t0 + W7Q < p.n_t) fetch(t0 + W7Q);
        __syncthreads();
        // ---- 2: the walk
        {
            float kp[NI], bp[NI];
#pragma unroll
            for (int n4 = 0; n4 < NI / 4; ++n4) {
                const int at = as * RS + 4 * (run + LS * n4);
                const float4 k4 = *(const float4 *) (sK + at), b4 = *(const float4 *) (sB + at);
                kp[4 * n4] = k4.x; kp[4 * n4 + 1] = k4.y; kp[4 * n4 + 2] = k4.z; kp[4 * n4 + 3] = k4.w;
                bp[4 * n4] = b4.x; bp[4 * n4 + 1] = b4.y; bp[4 * n4 + 2] = b4.z; bp[4 * n4 + 3] = b4.w;
            }
#pragma unroll
            for (int t = 0; t < W7Q; ++t) {
                float ak = 0.0f, ab = 0.0f, rk = 0.0f, rb = 0.0f;
#pragma unroll
                for (int n4 = 0; n4 < NI / 4; ++n4) {
                    const int at = t * RS + 4 * (run + LS * n4);
                    const float4 a4 = *(const float4 *) (sA + at), w4 = *(const float4 *) (sW + at), r4 = *(const float4 *) (sR + at);
                    const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, ww[4] = {w4.x, w4.y, w4.z, w4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int n = 4 * n4 + u;
                        if (t > as) {
                            ak += aa[u] * kp[n];
                            ab += aa[u] * bp[n];
                            kp[n] = kp[n] * ww[u];
                            bp[n] = bp[n] * ww[u];
                        }
                        if (t >= as) {
                            rk += rr[u] * kp[n];
                            rb += rr[u] * bp[n];
                        }
                    }
                }
                ak = wkv7_group_sum<LS>(ak);
                ab = wkv7_group_sum<LS>(ab);
                rk = wkv7_group_sum<LS>(rk);
                rb = wkv7_group_sum<LS>(rb);
                if (run == 0) {
                    sM[(0 * W7Q + t) * W7AS + as] = ak;
                    sM[(1 * W7Q + t) * W7AS + as] = ab;
                    sM[(2 * W7Q + t) * W7AS + as] = rk;
                    sM[(3 * W7Q + t) * W7AS + as] = rb;
                }
            }
#pragma unroll
            for (int n4 = 0; n4 < NI / 4; ++n4) {
                const int at = as * RS + 4 * (run + LS * n4);
                *(float4 *) (sK + at) = make_float4(kp[4 * n4], kp[4 * n4 + 1], kp[4 * n4 + 2], kp[4 * n4 + 3]);
                *(float4 *) (sB + at) = make_float4(bp[4 * n4], bp[4 * n4 + 1], bp[4 * n4 + 2], bp[4 * n4 + 3]);
            }
        }
        __syncthreads();  // the walk has read a, r and w as they came
        // ---- 3: a~ over a, r~ over r, P0_Q
        for (int e = tid; e < 2 * S; e += NT) {
            const int j = e % S;
            float pr = 1.0f;
            if (e < S) {
#pragma unroll
                for (int t = 0; t < W7Q; ++t) {
                    sA[t * RS + j] = sA[t * RS + j] * pr;
                    pr = pr * sW[t * RS + j];
                }
            } else {
#pragma unroll
                for (int t = 0; t < W7Q; ++t) {
                    pr = pr * sW[t * RS + j];
                    sR[t * RS + j] = sR[t * RS + j] * pr;
                }
                sP[j] = pr;
            }
        }
        __syncthreads();
        // ---- 4: G = a~ S0^T + Aak V
        const float * vp = sV + (4 * q) * VS + 16 * w + i;  // v_s[i] of s = 4 q (+ v: VS floats further)
        {
            f32x4 G = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int b = 0; b < S / 16; ++b) {
                const float4 a4 = *(const float4 *) (sA + i * RS + 16 * b + 4 * q);  // a~[t = lane % 16][j = 16 b + 4 q + v]
                G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, st[b / 4][4 * (b % 4) + 0], G, 0, 0, 0);
                G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, st[b / 4][4 * (b % 4) + 1], G, 0, 0, 0);
                G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, st[b / 4][4 * (b % 4) + 2], G, 0, 0, 0);
                G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, st[b / 4][4 * (b % 4) + 3], G, 0, 0, 0);
            }
            const float4 a4 = *(const float4 *) (sM + (0 * W7Q + i) * W7AS + 4 * q);  // Aak[t = lane % 16][s = 4 q + v]
            G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, vp[0], G, 0, 0, 0);
            G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, vp[VS], G, 0, 0, 0);
            G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, vp[2 * VS], G, 0, 0, 0);
            G = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, vp[3 * VS], G, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) sG[(w * W7Q + 4 * q + v) * W7AS + i] = G[v];
        }
        __syncthreads();  // (a wave reads only its own tile of sG)
        // ---- 5: the forward substitution, every lane for its row i
        float sa[W7Q];
#pragma unroll
        for (int t = 0; t < W7Q; ++t) {
            float acc = sG[(w * W7Q + t) * W7AS + i];
#pragma unroll
            for (int c = 0; 4 * c < t; ++c) {
                const float4 m4 = *(const float4 *) (sM + (1 * W7Q + t) * W7AS + 4 * c);  // Aab[t][4 c ..]: one address a wave
                const float mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (4 * c + u < t) acc += mm[u] * sa[4 * c + u];
            }
            sa[t] = acc;
        }
        // ---- 5: Y = r~ S0^T + Ark V + Arb SA
        f32x4 Y = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int b = 0; b < S / 16; ++b) {
            const float4 r4 = *(const float4 *) (sR + i * RS + 16 * b + 4 * q);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(r4.x, st[b / 4][4 * (b % 4) + 0], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(r4.y, st[b / 4][4 * (b % 4) + 1], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(r4.z, st[b / 4][4 * (b % 4) + 2], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(r4.w, st[b / 4][4 * (b % 4) + 3], Y, 0, 0, 0);
        }
        {
            const float4 k4 = *(const float4 *) (sM + (2 * W7Q + i) * W7AS + 4 * q), b4 = *(const float4 *) (sM + (3 * W7Q + i) * W7AS + 4 * q);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(k4.x, vp[0], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(k4.y, vp[VS], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(k4.z, vp[2 * VS], Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(k4.w, vp[3 * VS], Y, 0, 0, 0);
            // sa of s = 4 q + v: the lane holds all sixteen, its group picks four
            const float s0 = q == 0 ? sa[0] : q == 1 ? sa[4] : q == 2 ? sa[8] : sa[12], s1 = q == 0 ? sa[1] : q == 1 ? sa[5] : q == 2 ? sa[9] : sa[13];
            const float s2 = q == 0 ? sa[2] : q == 1 ? sa[6] : q == 2 ? sa[10] : sa[14], s3 = q == 0 ? sa[3] : q == 1 ? sa[7] : q == 2 ? sa[11] : sa[15];
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.x, s0, Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.y, s1, Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.z, s2, Y, 0, 0, 0);
            Y = __builtin_amdgcn_mfma_f32_16x16x4f32(b4.w, s3, Y, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = 4 * q + v;
            if (t < tc) p.y[(tok0 + t) * C + hs + i0 + i] = Y[v];
        }
        // ---- 5: S' = S0 diag(P0_Q), then the tokens' two outer products each in ascending order, one product a K = 1 step
#pragma unroll
        for (int b = 0; b < S / 16; ++b) {
            const float4 p4 = *(const float4 *) (sP + 16 * b + 4 * q);
            st[b / 4][4 * (b % 4) + 0] = st[b / 4][4 * (b % 4) + 0] * p4.x;
            st[b / 4][4 * (b % 4) + 1] = st[b / 4][4 * (b % 4) + 1] * p4.y;
            st[b / 4][4 * (b % 4) + 2] = st[b / 4][4 * (b % 4) + 2] * p4.z;
            st[b / 4][4 * (b % 4) + 3] = st[b / 4][4 * (b % 4) + 3] * p4.w;
        }
#pragma unroll
        for (int s = 0; s < W7Q; ++s) {
            const float vs = sV[s * VS + 16 * w + i];
#pragma unroll
            for (int g = 0; g < NB; ++g) {  // block q of A: columns 64 g + 16 q + i
                st[g] = __builtin_amdgcn_mfma_f32_16x16x1f32(sK[s * RS + 64 * g + lane], vs, st[g], 0, 0, 0);
                st[g] = __builtin_amdgcn_mfma_f32_16x16x1f32(sB[s * RS + 64 * g + lane], sa[s], st[g], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < S / 16; ++b) {
        float * o = p.st_out + st_at + 16 * b;
        const float4 x = make_float4(st[b / 4][4 * (b % 4) + 0], st[b / 4][4 * (b % 4) + 1], st[b / 4][4 * (b % 4) + 2], st[b / 4][4 * (b % 4) + 3]);
        if (p.svec) *(float4 *) o = x;
        else { o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w; }
    }
}

// which form serves a RWKV_WKV7 node: THE one place.  mode: the wkv_chunk switch — 0: the serial kernel everywhere; 2: the chunked form wherever the operands
// allow (tests, measurements); 1: routed — from MI_WKV7_CHUNK_MIN_TOKENS tokens a sequence on (kernels.h says what was measured)
bool wkv7_runs_chunked(const tdesc & r, const tdesc & state, int mode) {
    const int64_t S = r.ne[0], H = r.ne[1], T = r.ne[2];
    const int64_t n_state = state.ne[0] * state.ne[1] * state.ne[2] * state.ne[3];
    if (mode == 0 || (S != 64 && S != 128) || H < 1 || T < 1 || n_state < S * S * H || n_state % (S * S * H) != 0 || T % (n_state / (S * S * H)) != 0) return false;
    return mode == 2 || T / (n_state / (S * S * H)) >= MI_WKV7_CHUNK_MIN_TOKENS;
}

bool launch_rwkv_wkv7_chunk(hipStream_t s, const tdesc & r, const tdesc & w, const tdesc & k, const tdesc & v, const tdesc & a, const tdesc & b, const tdesc & state,
                            const tdesc & dst) {
    if (!wkv7_runs_chunked(r, state, 2)) {
        MI_ERR("launch_rwkv_wkv7_chunk: head size %lld, %lld heads, %lld tokens are not served here", (long long) r.ne[0], (long long) r.ne[1], (long long) r.ne[2]);
        return false;
    }
    constexpr int NW = MI_WKV7_CHUNK_WAVES;
    const int64_t S = r.ne[0], H = r.ne[1], T = r.ne[2], n_seqs = state.ne[0] * state.ne[1] * state.ne[2] * state.ne[3] / (S * S * H);
    wkv7_chunk_args p;
    p.r = (const float *) r.data;
    p.w = (const float *) w.data;
    p.k = (const float *) k.data;
    p.v = (const float *) v.data;
    p.a = (const float *) a.data;
    p.b = (const float *) b.data;
    p.state = (const float *) state.data;
    p.y = (float *) dst.data;
    p.st_out = p.y + S * H * T;
    p.H = (int) H;
    p.n_t = (int) (T / n_seqs);
    p.vec = ((((uintptr_t) p.r) | ((uintptr_t) p.w) | ((uintptr_t) p.k) | ((uintptr_t) p.a) | ((uintptr_t) p.b)) & 15) == 0;
    p.svec = ((((uintptr_t) p.state) | ((uintptr_t) p.st_out)) & 15) == 0;
    const dim3 grid((unsigned) (H * (S / (16 * NW))), (unsigned) n_seqs);
    if (S == 64) hipLaunchKernelGGL((k_wkv7_chunk<64, NW>), grid, dim3(64 * NW), 0, s, p);
    else hipLaunchKernelGGL((k_wkv7_chunk<128, NW>), grid, dim3(64 * NW), 0, s, p);
    return true;
}

MI_TU_TOUCH(wkv7_chunk)

}  // namespace mi355x
