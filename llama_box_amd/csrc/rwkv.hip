// rwkv.hip — what the linear-attention recurrent layers need beyond the attention and state-space families (llama.cpp archs rwkv6, rwkv6qwen2, rwkv7, arwkv7):
// the three state recurrences RWKV_WKV6, GATED_LINEAR_ATTN and RWKV_WKV7, and the helper ops L2_NORM, SQR and REPEAT.  DESIGN.md §4k states the operand contracts;
// graph.cpp's supports_op checks them (rwkv_wkv_ok, l2_norm_ok, repeat_ok), the launchers here trust them.  This file is compiled with -ffp-contract=off: every
// product and sum below is one f32 rounding, in the order written.
//
// Shared layout of the recurrences: S = head size (64 / 128), H heads, C = S * H, T tokens in n_seqs equal runs of n_t; per-token operands [S, H, T] contiguous,
// the state of sequence s at s * S * C with element (h, i, j) at h * S * S + i * S + j; dst = y [C, T], then the new states in the state layout.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

// ------------------------------------------------------------------------------------------------ RWKV_WKV6 / GATED_LINEAR_ATTN
// For token t, head h, column j, with y from 0 and i ascending:
//   WKV6: kv = v[j] * k[i];  y[j] += (kv * tf[i] + prev[i][j]) * r[i];  cur[i][j] = prev[i][j] * td[i] + kv
//   GLA:  kv = v[j] * k[i];  tmp = prev[i][j] * g[i] + kv;  y[j] += tmp * (q[i] * scale);  cur[i][j] = tmp
// A workgroup is ONE wave and owns 16 columns j of one (sequence, head): H * S / 16 workgroups a sequence (256 at 64 heads of 64, where one workgroup a head would
// leave three quarters of the CUs idle).  The lanes of a quad split the S rows i in four runs of NI = S / 4 (lane = 4 * column + run), so a lane keeps NI state
// elements in registers for the whole token loop — read once from `state`, written once behind y; a load instruction of the wave touches four rows of 16
// consecutive floats.  The lane sums its own rows in ascending order, the quad finishes y with two DPP adds ((y0 + y1) + (y2 + y3), the same bits in all four
// lanes): a fixed order, no LDS, no atomics.
// Tokens go in chunks of TC = 1024 / S.  Per chunk the wave stages k, r (GLA: q * scale, the product's one rounding) and td (g) of its head for all S rows and v of
// its 16 columns in LDS; a lane then reads its run as float4s (four addresses a wave: broadcasts).  tf sits in NI registers.
struct wkv6_args {
    const float * k, * v, * r, * tf, * td;  // GLA: r is q, td is g, tf unused
    const float * state;
    float * y, * st_out;
    int H, n_t;
    float scale;
};
template <int S> struct wkv6_geom {
    static constexpr int NI = S / 4;
    static constexpr int TC = 1024 / S;
};
template <int S, bool GLA>
__global__ void __launch_bounds__(64) k_rwkv_wkv6(const wkv6_args p) {
    constexpr int NI = wkv6_geom<S>::NI, TC = wkv6_geom<S>::TC, S4 = S / 4, SLABS = S / 16;
    __shared__ float4 sK[TC * S4], sR[TC * S4], sD[TC * S4];
    __shared__ float sV[TC][16];
    const int lane = threadIdx.x, run = lane & 3, jl = lane >> 2;
    const int h = blockIdx.x / SLABS, j0 = (blockIdx.x % SLABS) * 16;
    const int seq = blockIdx.y;
    const int i0 = run * NI;
    const int64_t C = (int64_t) p.H * S;
    const int64_t hs = (int64_t) h * S;
    const int64_t st_at = ((int64_t) seq * p.H + h) * S * S + (int64_t) i0 * S + j0 + jl;
    float st[NI], tf[GLA ? 1 : NI];
#pragma unroll
    for (int q = 0; q < NI; ++q) st[q] = p.state[st_at + (int64_t) q * S];
    if constexpr (!GLA) {
#pragma unroll
        for (int q = 0; q < NI; ++q) tf[q] = p.tf[hs + i0 + q];
    }
    for (int t0 = 0; t0 < p.n_t; t0 += TC) {
        const int tc = min(TC, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
        __syncthreads();  // the chunk before this one has been read
        for (int e = lane; e < tc * S; e += 64) {
            const int64_t at = (tok0 + e / S) * C + hs + e % S;
            ((float *) sK)[e] = p.k[at];
            if constexpr (GLA) ((float *) sR)[e] = p.r[at] * p.scale;
            else ((float *) sR)[e] = p.r[at];
            ((float *) sD)[e] = p.td[at];
        }
        for (int e = lane; e < tc * 16; e += 64) sV[e >> 4][e & 15] = p.v[(tok0 + (e >> 4)) * C + hs + j0 + (e & 15)];
        __syncthreads();
        for (int t = 0; t < tc; ++t) {
            const float v = sV[t][jl];
            float y = 0.0f;
#pragma unroll
            for (int q4 = 0; q4 < NI / 4; ++q4) {
                const float4 k4 = sK[t * S4 + i0 / 4 + q4], r4 = sR[t * S4 + i0 / 4 + q4], d4 = sD[t * S4 + i0 / 4 + q4];
                const float kk[4] = {k4.x, k4.y, k4.z, k4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q4 * 4 + u;
                    const float kv = v * kk[u];
                    if constexpr (GLA) {
                        const float tmp = st[q] * dd[u] + kv;
                        y += tmp * rr[u];
                        st[q] = tmp;
                    } else {
                        y += (kv * tf[q] + st[q]) * rr[u];
                        st[q] = st[q] * dd[u] + kv;
                    }
                }
            }
            y += dpp_f32<MI_DPP_QUAD_XOR1>(y);
            y += dpp_f32<MI_DPP_QUAD_XOR2>(y);
            if (run == 0) p.y[(tok0 + t) * C + hs + j0 + jl] = y;
        }
    }
#pragma unroll
    for (int q = 0; q < NI; ++q) p.st_out[st_at + (int64_t) q * S] = st[q];
}

template <int S, bool GLA>
static void launch_wkv6_s(hipStream_t s, const wkv6_args & p, const int n_seqs) {
    hipLaunchKernelGGL((k_rwkv_wkv6<S, GLA>), dim3((unsigned) (p.H * (S / 16)), (unsigned) n_seqs), dim3(64), 0, s, p);
}
// the operand extents shared by the three launchers: S, H, T from k-shaped operand x, n_seqs from the state's element count
static bool wkv_dims(const char * who, const tdesc & x, const tdesc & state, int64_t & S, int64_t & H, int64_t & T, int64_t & n_seqs) {
    S = x.ne[0];
    H = x.ne[1];
    T = x.ne[2];
    const int64_t n_state = state.ne[0] * state.ne[1] * state.ne[2] * state.ne[3];
    n_seqs = S > 0 && H > 0 ? n_state / (S * S * H) : 0;
    if ((S != 64 && S != 128) || H < 1 || T < 1 || n_seqs < 1 || T % n_seqs != 0 || n_state != S * S * H * n_seqs) {
        MI_ERR("%s: head size %lld, %lld heads, %lld tokens, %lld state elements are not served here", who, (long long) S, (long long) H, (long long) T, (long long) n_state);
        return false;
    }
    return true;
}
static bool launch_wkv6_any(hipStream_t s, const char * who, const bool gla, const tdesc & k, const tdesc & v, const tdesc & r, const float * tf, const tdesc & td,
                            const tdesc & state, const tdesc & dst, const float scale) {
    int64_t S, H, T, n_seqs;
    if (!wkv_dims(who, k, state, S, H, T, n_seqs)) return false;
    wkv6_args p;
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
    if (S == 64) gla ? launch_wkv6_s<64, true>(s, p, (int) n_seqs) : launch_wkv6_s<64, false>(s, p, (int) n_seqs);
    else gla ? launch_wkv6_s<128, true>(s, p, (int) n_seqs) : launch_wkv6_s<128, false>(s, p, (int) n_seqs);
    return true;
}
bool launch_rwkv_wkv6(hipStream_t s, const tdesc & k, const tdesc & v, const tdesc & r, const tdesc & tf, const tdesc & td, const tdesc & state, const tdesc & dst) {
    return launch_wkv6_any(s, "launch_rwkv_wkv6", false, k, v, r, (const float *) tf.data, td, state, dst, 1.0f);
}
bool launch_gated_linear_attn(hipStream_t s, const tdesc & k, const tdesc & v, const tdesc & q, const tdesc & g, const tdesc & state, const tdesc & dst, float scale) {
    return launch_wkv6_any(s, "launch_gated_linear_attn", true, k, v, q, nullptr, g, state, dst, scale);
}

// ------------------------------------------------------------------------------------------------ RWKV_WKV7
// For token t, head h and value row i (the reductions run over j, the contiguous dimension of a state row):
//   sa = sum over j of a[j] * prev[i][j];  cur[i][j] = prev[i][j] * w[j] + v[i] * k[j] + sa * b[j];  y[i] = sum over j of cur[i][j] * r[j]
// A workgroup is one wave and owns 16 rows i of one (sequence, head).  A DPP row of 16 lanes lies along j and holds a state row as NV = S / 64 float4s a lane
// (element group v * 16 + lane: a row's loads and stores are contiguous 16-byte accesses); a lane keeps four rows (i0 + 4 q + its DPP row), 16 NV state registers.
// Both sums are lane-local in ascending j, then the DPP row sum of dev_util.h (the same bits in all 16 lanes): sa is complete before any cur of the row is formed.
// Tokens go in chunks of TC = 512 / S; r, w, k, a, b of the head ([TC][S] each) and v of the 16 rows are staged in LDS once per chunk.
struct wkv7_args {
    const float * r, * w, * k, * v, * a, * b;
    const float * state;
    float * y, * st_out;
    int H, n_t;
    int vec;  // state rows and st_out rows are 16-byte aligned
};
template <int S> struct wkv7_geom {
    static constexpr int NV = S / 64;
    static constexpr int TC = 512 / S;
};
__device__ __forceinline__ float4 wkv_ld4(const float * p, const bool vec) { return vec ? *(const float4 *) p : make_float4(p[0], p[1], p[2], p[3]); }

template <int S>
__global__ void __launch_bounds__(64) k_rwkv_wkv7(const wkv7_args p) {
    constexpr int NV = wkv7_geom<S>::NV, TC = wkv7_geom<S>::TC, S4 = S / 4, SLABS = S / 16, RI = 4;
    __shared__ float4 sR[TC * S4], sW[TC * S4], sK[TC * S4], sA[TC * S4], sB[TC * S4];
    __shared__ float sV[TC][16];
    const int lane = threadIdx.x, li = lane & 15, rg = lane >> 4;
    const int h = blockIdx.x / SLABS, i0 = (blockIdx.x % SLABS) * 16;
    const int seq = blockIdx.y;
    const int64_t C = (int64_t) p.H * S;
    const int64_t hs = (int64_t) h * S;
    const int64_t st_at = (((int64_t) seq * p.H + h) * S + i0 + rg) * S + 4 * li;  // row i0 + rg; row q of the lane is 4 q rows further
    float4 st[RI][NV];
#pragma unroll
    for (int q = 0; q < RI; ++q)
#pragma unroll
        for (int v = 0; v < NV; ++v) st[q][v] = wkv_ld4(p.state + st_at + (int64_t) (4 * q) * S + 64 * v, p.vec != 0);
    for (int t0 = 0; t0 < p.n_t; t0 += TC) {
        const int tc = min(TC, p.n_t - t0);
        const int64_t tok0 = (int64_t) seq * p.n_t + t0;
        __syncthreads();  // the chunk before this one has been read
        for (int e = lane; e < tc * S; e += 64) {
            const int64_t at = (tok0 + e / S) * C + hs + e % S;
            ((float *) sR)[e] = p.r[at];
            ((float *) sW)[e] = p.w[at];
            ((float *) sK)[e] = p.k[at];
            ((float *) sA)[e] = p.a[at];
            ((float *) sB)[e] = p.b[at];
        }
        for (int e = lane; e < tc * 16; e += 64) sV[e >> 4][e & 15] = p.v[(tok0 + (e >> 4)) * C + hs + i0 + (e & 15)];
        __syncthreads();
        for (int t = 0; t < tc; ++t) {
            float4 r4[NV], w4[NV], k4[NV], a4[NV], b4[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int at = t * S4 + v * 16 + li;
                r4[v] = sR[at]; w4[v] = sW[at]; k4[v] = sK[at]; a4[v] = sA[at]; b4[v] = sB[at];
            }
#pragma unroll
            for (int q = 0; q < RI; ++q) {
                const float vv = sV[t][4 * q + rg];
                float sa = 0.0f;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    sa += a4[v].x * st[q][v].x;
                    sa += a4[v].y * st[q][v].y;
                    sa += a4[v].z * st[q][v].z;
                    sa += a4[v].w * st[q][v].w;
                }
                sa = row16_sum(sa);
                float y = 0.0f;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    st[q][v].x = (st[q][v].x * w4[v].x + vv * k4[v].x) + sa * b4[v].x;
                    st[q][v].y = (st[q][v].y * w4[v].y + vv * k4[v].y) + sa * b4[v].y;
                    st[q][v].z = (st[q][v].z * w4[v].z + vv * k4[v].z) + sa * b4[v].z;
                    st[q][v].w = (st[q][v].w * w4[v].w + vv * k4[v].w) + sa * b4[v].w;
                    y += st[q][v].x * r4[v].x;
                    y += st[q][v].y * r4[v].y;
                    y += st[q][v].z * r4[v].z;
                    y += st[q][v].w * r4[v].w;
                }
                y = row16_sum(y);
                if (li == 0) p.y[(tok0 + t) * C + hs + i0 + 4 * q + rg] = y;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RI; ++q)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float * o = p.st_out + st_at + (int64_t) (4 * q) * S + 64 * v;
            if (p.vec) *(float4 *) o = st[q][v];
            else { o[0] = st[q][v].x; o[1] = st[q][v].y; o[2] = st[q][v].z; o[3] = st[q][v].w; }
        }
}
bool launch_rwkv_wkv7(hipStream_t s, const tdesc & r, const tdesc & w, const tdesc & k, const tdesc & v, const tdesc & a, const tdesc & b, const tdesc & state, const tdesc & dst) {
    int64_t S, H, T, n_seqs;
    if (!wkv_dims("launch_rwkv_wkv7", r, state, S, H, T, n_seqs)) return false;
    wkv7_args p;
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
    p.vec = ((((uintptr_t) p.state) | ((uintptr_t) p.st_out)) & 15) == 0;
    const dim3 grid((unsigned) (H * (S / 16)), (unsigned) n_seqs);
    if (S == 64) hipLaunchKernelGGL((k_rwkv_wkv7<64>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((k_rwkv_wkv7<128>), grid, dim3(64), 0, s, p);
    return true;
}

// ------------------------------------------------------------------------------------------------ L2_NORM
// ggml_compute_forward_l2_norm_f32: sum = sum of (double) (x * x), the square an f32 product; scale = 1 / fmaxf(sqrtf((float) sum), eps); y = x * scale.
// One wave a row (RWKV-7's rows are one head long), four rows a workgroup; the row is read twice (the second time from the cache).  dst may BE src: a lane writes
// only elements it read itself, after the wave's sum.
__global__ void __launch_bounds__(256) k_l2_norm(const tdesc a, const tdesc d, const float eps, const int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // (whole waves leave; no barrier below)
    const int64_t i1 = row % a.ne[1], i2 = (row / a.ne[1]) % a.ne[2], i3 = row / (a.ne[1] * a.ne[2]);
    const float * x = (const float *) (a.data + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3]);
    float * y = (float *) (d.data + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]);
    const int64_t n = a.ne[0];
    double s = 0.0;
    for (int64_t i = lane; i < n; i += 64) s += (double) (x[i] * x[i]);
    const float scale = 1.0f / fmaxf(sqrtf((float) wave_sum_d(s)), eps);
    for (int64_t i = lane; i < n; i += 64) y[i] = x[i] * scale;
}
void launch_l2_norm(hipStream_t s, const tdesc & src, const tdesc & dst, float eps) {
    const int64_t rows = src.ne[1] * src.ne[2] * src.ne[3];
    if (rows == 0 || src.ne[0] == 0) return;
    hipLaunchKernelGGL(k_l2_norm, dim3((unsigned) ((rows + 3) / 4)), dim3(256), 0, s, src, dst, eps, rows);
}

// ------------------------------------------------------------------------------------------------ SQR
// (x / y carry no __restrict__: the _inplace form squares a tensor onto itself)
__global__ void __launch_bounds__(256) k_sqr(const float * x, float * y, const int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) y[i] = x[i] * x[i];
}
void launch_sqr(hipStream_t s, const tdesc & src, const tdesc & dst) {
    const int64_t n = src.ne[0] * src.ne[1] * src.ne[2] * src.ne[3];
    if (n == 0) return;
    hipLaunchKernelGGL(k_sqr, dim3((unsigned) std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, s, (const float *) src.data, (float *) dst.data, n);
}

// ------------------------------------------------------------------------------------------------ REPEAT
// dst[i3, i2, i1, i0] = src[i3 % ne3, i2 % ne2, i1 % ne1, i0 % ne0]: one thread a destination element (dst contiguous), the source with any strides
__global__ void __launch_bounds__(256) k_repeat(const tdesc a, const tdesc d, const int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) {
        const int64_t i0 = i % d.ne[0];
        int64_t r = i / d.ne[0];
        const int64_t i1 = r % d.ne[1];
        r /= d.ne[1];
        const int64_t i2 = r % d.ne[2], i3 = r / d.ne[2];
        ((uint32_t *) d.data)[i] = *(const uint32_t *) (a.data + (i0 % a.ne[0]) * a.nb[0] + (i1 % a.ne[1]) * a.nb[1] + (i2 % a.ne[2]) * a.nb[2] + (i3 % a.ne[3]) * a.nb[3]);
    }
}
void launch_repeat(hipStream_t s, const tdesc & src, const tdesc & dst) {
    const int64_t n = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (n == 0) return;
    hipLaunchKernelGGL(k_repeat, dim3((unsigned) std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, s, src, dst, n);
}

MI_TU_TOUCH(rwkv)

}  // namespace mi355x
