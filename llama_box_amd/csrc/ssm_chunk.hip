// ssm_chunk.hip — SSM_SCAN in its Mamba-2 form (one A per head) for prompt batches: the chunked ("SSD") restatement of the recurrence of ssm.hip on the f32 matrix
// cores.  DESIGN.md §4i states the operand contract and the error account; graph.cpp's ssm_scan_ok checks the contract, ssm_scan_runs_chunked below routes.  Compiled
// with -ffp-contract=off.
//
// For CQ = 64 tokens of one (sequence, head), with dtp_t = softplus(dt_t), a_t = dtp_t A (<= 0) and cum_t = a_0 + .. + a_t (inclusive, from the chunk's first token),
// S0 [head_dim][d_state] the state the chunk starts from:
//     y_t = sum over s <= t of exp(cum_t - cum_s) (C_t . B_s) dtp_s x_s  +  exp(cum_t) (S0 C_t)
//     S'  = exp(cum_Q) S0 + sum over s of exp(cum_Q - cum_s) dtp_s x_s (x) B_s
// so the 64 dependent steps of k_ssm_scan become four small products and ONE dependent step a chunk.  Every decay is one expf of a difference of prefix sums (<= 0,
// clamped there), never a product or quotient of exponentials: dt = 100 (cum = -150) or dt = -30 (dtp = 1e-13) neither overflow nor meet 0 * inf.  The prefix sums
// are two-float (hi + lo, TwoSum) values summed in a fixed Hillis-Steele tree inside one wave: a difference cum_t - cum_s keeps the relative accuracy of its terms
// however large |cum| has grown behind a token that wipes the state.
//
// Work split.  A workgroup of four waves owns one (sequence, head, tile of CP = 64 head_dim rows).  v_mfma_f32_16x16x4_f32 throughout: A lane l = A[i = l % 16][k = l / 16],
// B lane l = B[k = l / 16][j = l % 16], C lane l = C[i = 4 (l / 16) + v][j = l % 16], v = 0 .. 3.  Wave w owns head_dim rows p = 16 w .. 16 w + 15 for ALL d_state
// elements and ALL tokens: the state lives TRANSPOSED in its accumulators, S^T[n][p] as d_state / 16 tiles (lane (j, q): p = j, n = 16 nt + 4 q + v), across the
// whole chunk loop — read once from the row ids[seq] selects (on the device), written once.  That layout is at the same time the B operand of Y = C S0^T: the MFMA
// step v of tile nt takes lane quarter q's n = 16 nt + 4 q + v, and the A operand of that step is one float of the float4 a lane reads from C's LDS row at
// n = 16 nt + 4 q: no cross-lane movement and no LDS round trip between the state update and the output product.  The same pairing (a float4 along K a lane, its four
// floats four MFMA steps) serves every product here:
//     1. G = C B^T          [t][s]  K = d_state   wave w: token tile t = 16 w .., the s tiles at or below the diagonal; A, B = float4 reads of sC / sB rows
//     2. G *= exp(cum_t - cum_s) where s <= t, 0 above, in the accumulators; written to sG
//     3. Y = C S0^T         [t][p]  K = d_state   A = sC float4, B = the state registers; then Y[t][.] *= exp(cum_t)
//        Y += G (x dtp)     [t][p]  K = s <= t    A = sG float4 (tiles above the diagonal skipped), B = x dtp in registers (16 a lane, read once a chunk)
//     4. S^T = exp(cum_Q) S^T + B^T (w x dtp)     [n][p]  K = s     A = sB read down a column (ds_read_b32, conflict-free), B = the registers of 3 times w_s
// LDS a chunk (floats): sB, sC [64][d_state + 4]; sX (raw x), sG [64][68]; dtp, cum hi / lo, exp(cum_t), w_s = exp(cum_Q - cum_s) [64] each: 103 680 bytes at d_state
// 128, 70 912 at 64.  Row strides 132 / 68 floats: a float4 read of 16 consecutive rows starts 4 banks apart (conflict-free in each 16-lane phase), the column reads
// of step 4 and the x reads land on 64 different banks.  d_state 256 would need 167 KB of the 160 KB: it stays on k_ssm_scan, as do d_state 16 and Mamba-1's per-element A.
// A last partial chunk is masked: rows past the node's tokens are zero in LDS (never loaded), their a_t is 0 (cum stays flat), their y is not stored.
// Deterministic: fixed orders everywhere, no atomics.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CQ = 64;   // tokens a chunk
constexpr int CP = 64;   // head_dim rows a workgroup: 16 a wave
constexpr int CXS = 68;  // row stride of sX and sG, floats

struct ssm_chunk_args {
    const char * s;       // [d_state, head_dim, n_head, n_rs] contiguous
    int64_t s_nb3;
    int n_rs;
    const char * x;       // [head_dim, n_head, n_t, n_s]: nb0 4, nb1 head_dim * 4
    int64_t x_nb2, x_nb3;
    const float * dt;     // [n_head, n_t, n_s] contiguous
    const float * A;      // [1, n_head]
    const char * B, * C;  // [d_state, n_group, n_t, n_s]: nb0 4, nb1 d_state * 4
    int64_t b_nb2, b_nb3, c_nb2, c_nb3;
    const int32_t * ids;  // [n_s]
    float * y;            // [head_dim, n_head, n_t, n_s] contiguous
    float * st_out;       // [d_state, head_dim, n_head, n_s] contiguous
    int head_dim, n_head, n_group, n_t;
    int p_tiles;          // workgroups a head: ceil(head_dim / CP)
    int vec_state;        // s rows and st_out rows are 16-byte aligned
    int vec_bc;           // B / C rows are
};
template <int D> constexpr size_t ssm_chunk_lds() { return sizeof(float) * (size_t) (2 * CQ * (D + 4) + 2 * CQ * CXS + 5 * CQ); }

__device__ __forceinline__ float4 ldg4(const float * p, const bool vec) { return vec ? *(const float4 *) p : make_float4(p[0], p[1], p[2], p[3]); }
__device__ __forceinline__ f32x4 mfma4(const float a, const float b, const f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// four MFMA steps along K: the floats of a lane's float4 pair up with the floats of the other operand's
__device__ __forceinline__ f32x4 mfma4x4(const float4 a, const float4 b, f32x4 c) {
    c = mfma4(a.x, b.x, c);
    c = mfma4(a.y, b.y, c);
    c = mfma4(a.z, b.z, c);
    return mfma4(a.w, b.w, c);
}
// (h, l) = (ah + al) + (bh + bl) to twice the working precision: TwoSum of the heads, the tails folded in, renormalised
__device__ __forceinline__ void two_add(const float ah, const float al, const float bh, const float bl, float & h, float & l) {
    const float s = ah + bh;
    const float bb = s - ah;
    float e = (ah - (s - bb)) + (bh - bb);
    e = e + (al + bl);
    h = s + e;
    l = e - (h - s);
}

template <int D>
__global__ void __launch_bounds__(256) k_ssm_scan_chunk(const ssm_chunk_args p) {
    constexpr int BS = D + 4, NT = D / 16, D4 = D / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float * sB = (float *) smem;
    float * sC = sB + CQ * BS;
    float * sX = sC + CQ * BS;
    float * sG = sX + CQ * CXS;
    float * sDtp = sG + CQ * CXS;
    float * sCh = sDtp + CQ;
    float * sCl = sCh + CQ;
    float * sEt = sCl + CQ;
    float * sW = sEt + CQ;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, q = lane >> 4;
    const int i3 = blockIdx.y;
    const int h = blockIdx.x / p.p_tiles, p0 = (blockIdx.x % p.p_tiles) * CP;
    const int g = p.n_group == 1 ? 0 : h;
    const int rows_total = p.head_dim * p.n_head;
    const int pw = p0 + 16 * w + j;                   // this lane's head_dim row
    const bool wave_live = p0 + 16 * w < p.head_dim;  // (head_dim 48: the fourth wave computes its share of G and nothing else)
    const bool lane_live = pw < p.head_dim;
    const float Ah = p.A[h];

    // (an id outside the cache is undefined upstream; it is clamped here so that no address leaves s)
    const int id = min(max(p.ids[i3], 0), p.n_rs - 1);
    f32x4 st[NT];
    {
        const float * sp = (const float *) (p.s + (int64_t) id * p.s_nb3) + ((int64_t) h * p.head_dim + pw) * D;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float4 v = lane_live ? ldg4(sp + 16 * nt + 4 * q, p.vec_state != 0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            st[nt] = f32x4{v.x, v.y, v.z, v.w};
        }
    }

    // A chunk's rows travel global memory -> registers -> LDS: B and C of the group (RB float4s a thread each), raw x of the tile's rows (thread = (token w + 4 i,
    // row lane)), dt of the head (first wave, lane = token).  Rows past the node's tokens and past head_dim are zero, not loaded.  The loads of chunk c + 1 are issued
    // once chunk c stands in LDS and land behind its products.
    constexpr int RB = CQ * D4 / 256, RX = CQ * CP / 256;
    float4 rb[RB], rc[RB];
    float rx[RX], rdt;
    auto fetch = [&](const int t0) {
        const int tc = min(CQ, p.n_t - t0);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int e = tid + 256 * i, t = e / D4, c4 = e % D4;
            rb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            rc[i] = rb[i];
            if (t < tc) {
                const int64_t at = (int64_t) g * D * 4 + (int64_t) c4 * 16;
                rb[i] = ldg4((const float *) (p.B + (int64_t) (t0 + t) * p.b_nb2 + (int64_t) i3 * p.b_nb3 + at), p.vec_bc != 0);
                rc[i] = ldg4((const float *) (p.C + (int64_t) (t0 + t) * p.c_nb2 + (int64_t) i3 * p.c_nb3 + at), p.vec_bc != 0);
            }
        }
#pragma unroll
        for (int i = 0; i < RX; ++i) {
            const int t = w + 4 * i;
            rx[i] = 0.0f;
            if (t < tc && p0 + lane < p.head_dim) rx[i] = *(const float *) (p.x + ((int64_t) h * p.head_dim + p0 + lane) * 4 + (int64_t) (t0 + t) * p.x_nb2 + (int64_t) i3 * p.x_nb3);
        }
        rdt = 0.0f;
        if (w == 0 && lane < tc) rdt = p.dt[(int64_t) h + (int64_t) p.n_head * ((int64_t) (t0 + lane) + (int64_t) p.n_t * i3)];
    };
    fetch(0);

    for (int t0 = 0; t0 < p.n_t; t0 += CQ) {
        const int tc = min(CQ, p.n_t - t0);
        __syncthreads();  // the chunk before this one has been read
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int e = tid + 256 * i, t = e / D4, c4 = e % D4;
            *(float4 *) (sB + t * BS + 4 * c4) = rb[i];
            *(float4 *) (sC + t * BS + 4 * c4) = rc[i];
        }
#pragma unroll
        for (int i = 0; i < RX; ++i) sX[(w + 4 * i) * CXS + lane] = rx[i];
        // ---- the first wave, lane = token: softplus, a = dtp A, the inclusive two-float prefix sum in a fixed tree, and the decays that depend on one token only
        if (w == 0) {
            float dtp = 0.0f;
            if (lane < tc) dtp = rdt <= 20.0f ? log1pf(expf(rdt)) : rdt;
            float hi = dtp * Ah, lo = 0.0f;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float ph = __shfl_up(hi, off), pl = __shfl_up(lo, off);
                float nh, nl;
                two_add(ph, pl, hi, lo, nh, nl);
                if (lane >= off) { hi = nh; lo = nl; }
            }
            const float th = __shfl(hi, 63), tl = __shfl(lo, 63);
            sDtp[lane] = dtp;
            sCh[lane] = hi;
            sCl[lane] = lo;
            sEt[lane] = expf(fminf(hi + lo, 0.0f));
            sW[lane] = expf(fminf((th - hi) + (tl - lo), 0.0f));
        }
        if (t0 + CQ < p.n_t) fetch(t0 + CQ);
        __syncthreads();

        // ---- 1, 2: G = C B^T for token tile w, masked and decayed, to sG
        {
            f32x4 acc[4];
#pragma unroll
            for (int si = 0; si < 4; ++si) acc[si] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int k0 = 0; k0 < D; k0 += 16) {
                const float4 a4 = *(const float4 *) (sC + (16 * w + j) * BS + k0 + 4 * q);
#pragma unroll
                for (int si = 0; si < 4; ++si) {
                    if (si <= w) acc[si] = mfma4x4(a4, *(const float4 *) (sB + (16 * si + j) * BS + k0 + 4 * q), acc[si]);
                }
            }
#pragma unroll
            for (int si = 0; si < 4; ++si) {
                if (si <= w) {
                    const int sc = 16 * si + j;
                    const float sh = sCh[sc], sl = sCl[sc];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int t = 16 * w + 4 * q + v;
                        const float arg = (sCh[t] - sh) + (sCl[t] - sl);
                        sG[t * CXS + sc] = sc <= t ? acc[si][v] * expf(fminf(arg, 0.0f)) : 0.0f;
                    }
                }
            }
        }
        // ---- 3a: Y = diag(exp(cum_t)) C S0^T, the state registers as the B operand
        f32x4 Y[4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) Y[ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (wave_live) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 b4 = make_float4(st[nt][0], st[nt][1], st[nt][2], st[nt][3]);
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) Y[ti] = mfma4x4(*(const float4 *) (sC + (16 * ti + j) * BS + 16 * nt + 4 * q), b4, Y[ti]);
            }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
                for (int v = 0; v < 4; ++v) Y[ti][v] = Y[ti][v] * sEt[16 * ti + 4 * q + v];
            }
        }
        __syncthreads();  // sG is whole
        if (wave_live) {
            // ---- 3b: Y += G (x dtp); x dtp rounded once, as the serial kernel's xdt
            float4 xr[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int s0 = 16 * ks + 4 * q;
                xr[ks] = make_float4(sX[(s0 + 0) * CXS + 16 * w + j] * sDtp[s0 + 0], sX[(s0 + 1) * CXS + 16 * w + j] * sDtp[s0 + 1],
                                     sX[(s0 + 2) * CXS + 16 * w + j] * sDtp[s0 + 2], sX[(s0 + 3) * CXS + 16 * w + j] * sDtp[s0 + 3]);
            }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
                for (int ks = 0; ks <= ti; ++ks) Y[ti] = mfma4x4(*(const float4 *) (sG + (16 * ti + j) * CXS + 16 * ks + 4 * q), xr[ks], Y[ti]);
            }
            if (lane_live) {
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int t = 16 * ti + 4 * q + v;
                        if (t < tc) p.y[(int64_t) h * p.head_dim + pw + (int64_t) rows_total * ((int64_t) (t0 + t) + (int64_t) p.n_t * i3)] = Y[ti][v];
                    }
                }
            }
            // ---- 4: S^T = exp(cum_Q) S^T + B^T (w x dtp)
            const float eq = sEt[CQ - 1];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int s0 = 16 * ks + 4 * q;
                xr[ks] = make_float4(xr[ks].x * sW[s0 + 0], xr[ks].y * sW[s0 + 1], xr[ks].z * sW[s0 + 2], xr[ks].w * sW[s0 + 3]);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f32x4 a = st[nt];
#pragma unroll
                for (int v = 0; v < 4; ++v) a[v] = a[v] * eq;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const float * bp = sB + (16 * ks + 4 * q) * BS + 16 * nt + j;
                    a = mfma4x4(make_float4(bp[0], bp[BS], bp[2 * BS], bp[3 * BS]), xr[ks], a);
                }
                st[nt] = a;
            }
        }
    }
    if (lane_live) {
        float * op = p.st_out + ((int64_t) i3 * rows_total + (int64_t) h * p.head_dim + pw) * D;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float * o = op + 16 * nt + 4 * q;
            if (p.vec_state) *(float4 *) o = make_float4(st[nt][0], st[nt][1], st[nt][2], st[nt][3]);
            else { o[0] = st[nt][0]; o[1] = st[nt][1]; o[2] = st[nt][2]; o[3] = st[nt][3]; }
        }
    }
}

// which form serves the node: THE one place.  mode: the ssm_chunk switch — 0: the serial kernel everywhere; 2: the chunked form wherever the operands allow (tests,
// measurements); 1: routed — from MI_SSM_CHUNK_MIN_TOKENS tokens on, at head_dim >= MI_SSM_CHUNK_MIN_HEAD_DIM (kernels.h says what was measured)
bool ssm_scan_runs_chunked(const tdesc & st, const tdesc & x, const tdesc & A, int mode) {
    const int64_t d_state = st.ne[0], head_dim = x.ne[0], n_t = x.ne[2];
    if (mode == 0 || A.ne[0] != 1 || (d_state != 64 && d_state != 128)) return false;
    if (x.ne[0] * x.ne[1] * x.ne[2] * x.ne[3] == 0) return false;
    if (mode == 2) return true;
    return n_t >= MI_SSM_CHUNK_MIN_TOKENS && head_dim >= MI_SSM_CHUNK_MIN_HEAD_DIM;
}

template <int D>
static bool launch_ssm_scan_chunk_d(hipStream_t s, const ssm_chunk_args & p, const int n_s) {
    static std::atomic<uint32_t> lds_raised{0};
    if (!ensure_dyn_lds((const void *) k_ssm_scan_chunk<D>, ssm_chunk_lds<D>(), lds_raised)) return false;  // (MI_ERR is ensure_dyn_lds's)
    hipLaunchKernelGGL((k_ssm_scan_chunk<D>), dim3((unsigned) (p.n_head * p.p_tiles), (unsigned) n_s), dim3(256), ssm_chunk_lds<D>(), s, p);
    return true;
}
bool launch_ssm_scan_chunk(hipStream_t s, const tdesc & st, const tdesc & x, const tdesc & dt, const tdesc & A, const tdesc & B, const tdesc & C, const tdesc & ids, const tdesc & dst) {
    const int64_t d_state = st.ne[0], head_dim = x.ne[0], n_head = x.ne[1], n_t = x.ne[2], n_s = x.ne[3], n_group = B.ne[1];
    if (head_dim * n_head * n_t * n_s == 0) return true;
    if (!ssm_scan_runs_chunked(st, x, A, 2) || (n_group != 1 && n_group != n_head)) {
        MI_ERR("launch_ssm_scan_chunk: d_state %lld, A [%lld, ..], %lld groups over %lld heads are not served here", (long long) d_state, (long long) A.ne[0], (long long) n_group, (long long) n_head);
        return false;
    }
    ssm_chunk_args p;
    p.s = st.data;
    p.s_nb3 = st.nb[3];
    p.n_rs = (int) st.ne[3];
    p.x = x.data;
    p.x_nb2 = x.nb[2];
    p.x_nb3 = x.nb[3];
    p.dt = (const float *) dt.data;
    p.A = (const float *) A.data;
    p.B = B.data;
    p.C = C.data;
    p.b_nb2 = B.nb[2];
    p.b_nb3 = B.nb[3];
    p.c_nb2 = C.nb[2];
    p.c_nb3 = C.nb[3];
    p.ids = (const int32_t *) ids.data;
    p.y = (float *) dst.data;
    p.st_out = p.y + head_dim * n_head * n_t * n_s;
    p.head_dim = (int) head_dim;
    p.n_head = (int) n_head;
    p.n_group = (int) n_group;
    p.n_t = (int) n_t;
    p.p_tiles = (int) ((head_dim + CP - 1) / CP);
    p.vec_state = ((((uintptr_t) st.data) | ((uintptr_t) st.nb[3]) | ((uintptr_t) p.st_out)) & 15) == 0;
    p.vec_bc = ((((uintptr_t) B.data) | ((uintptr_t) C.data) | ((uintptr_t) (B.nb[2] | B.nb[3] | C.nb[2] | C.nb[3]))) & 15) == 0;
    return d_state == 128 ? launch_ssm_scan_chunk_d<128>(s, p, (int) n_s) : launch_ssm_scan_chunk_d<64>(s, p, (int) n_s);
}

MI_TU_TOUCH(ssm_chunk)

}  // namespace mi355x
