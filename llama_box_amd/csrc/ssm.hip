// ssm.hip — the three ops a state-space layer needs beyond the attention families (llama.cpp build_mamba_layer / build_mamba2_layer): CONCAT, SSM_CONV (with the
// bias ADD and the SILU that follow it folded in on request) and SSM_SCAN.  DESIGN.md §4i states the operand contracts; graph.cpp's supports_op checks them, the
// launchers here trust them.  This file is compiled with -ffp-contract=off: every product and sum below is one f32 rounding, in the order written.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

// ------------------------------------------------------------------------------------------------ CONCAT
// An exact element copy: one thread a destination element (dst contiguous), either source with any strides.  T is the element as an integer of its size.
template <typename T, int DIM>
__global__ void __launch_bounds__(256) k_concat(const tdesc a, const tdesc b, const tdesc d, const int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) {
        int64_t i0 = i % d.ne[0], r = i / d.ne[0];
        int64_t i1 = r % d.ne[1];
        r /= d.ne[1];
        int64_t i2 = r % d.ne[2], i3 = r / d.ne[2];
        const int64_t id = DIM == 0 ? i0 : DIM == 1 ? i1 : DIM == 2 ? i2 : i3;
        const bool hi = id >= a.ne[DIM];  // past a's extent: b's element
        const int64_t back = hi ? a.ne[DIM] : 0;
        if (DIM == 0) i0 -= back;
        if (DIM == 1) i1 -= back;
        if (DIM == 2) i2 -= back;
        if (DIM == 3) i3 -= back;
        const char * p = hi ? b.data + i0 * b.nb[0] + i1 * b.nb[1] + i2 * b.nb[2] + i3 * b.nb[3] : a.data + i0 * a.nb[0] + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3];
        ((T *) d.data)[i] = *(const T *) p;
    }
}
template <typename T>
static void launch_concat_t(hipStream_t s, const dim3 grid, const tdesc & a, const tdesc & b, const tdesc & d, int dim, int64_t n) {
    switch (dim) {
        case 0: hipLaunchKernelGGL((k_concat<T, 0>), grid, dim3(256), 0, s, a, b, d, n); break;
        case 1: hipLaunchKernelGGL((k_concat<T, 1>), grid, dim3(256), 0, s, a, b, d, n); break;
        case 2: hipLaunchKernelGGL((k_concat<T, 2>), grid, dim3(256), 0, s, a, b, d, n); break;
        default: hipLaunchKernelGGL((k_concat<T, 3>), grid, dim3(256), 0, s, a, b, d, n); break;
    }
}
bool launch_concat(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, int dim) {
    const int64_t n = d.ne[0] * d.ne[1] * d.ne[2] * d.ne[3];
    if (n == 0) return true;
    if (dim < 0 || dim > 3) { MI_ERR("launch_concat: dimension %d", dim); return false; }
    const dim3 grid((unsigned) std::min<int64_t>((n + 255) / 256, 8192));
    if (d.type == GGML_TYPE_F32 || d.type == GGML_TYPE_I32) launch_concat_t<uint32_t>(s, grid, a, b, d, dim, n);
    else if (d.type == GGML_TYPE_F16) launch_concat_t<uint16_t>(s, grid, a, b, d, dim, n);
    else { MI_ERR("launch_concat: type %d is not served here", d.type); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------ SSM_CONV (+ ADD bias, + SILU)
// out[i1, i2, i3] = sum over i0 < d_conv, ascending, of sx[i2 + i0, i1, i3] * c[i0, i1] (ggml_compute_forward_ssm_conv_f32: sumf = 0, sumf += s * c).  One thread
// an output element, i1 fastest across lanes (the store is coalesced; a lane's d_conv taps and its window are contiguous in sx / c).  FUSE: the `+ bias[i1]` of the
// ADD node and the silu_f of the UNARY node that follow, each its own f32 rounding — the bits of the unfused chain (ops.hip: k_binary, k_unary).
template <int DC, bool FUSE>
__global__ void __launch_bounds__(256) k_ssm_conv(const char * __restrict__ sx, const int64_t sx_nb1, const int64_t sx_nb2, const char * __restrict__ cw, const int64_t c_nb1,
                                                   float * __restrict__ y, const float * __restrict__ bias, const int64_t d_inner, const int64_t n_t, const int64_t total) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t i1 = i % d_inner, r = i / d_inner;
    const int64_t i2 = r % n_t, i3 = r / n_t;
    const float * x = (const float *) (sx + i3 * sx_nb2 + i1 * sx_nb1) + i2;
    const float * c = (const float *) (cw + i1 * c_nb1);
    float w[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) w[k] = c[k];
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < DC; ++k) sum += x[k] * w[k];
    if constexpr (FUSE) {
        sum = sum + bias[i1];
        sum = silu_f(sum);
    }
    y[i] = sum;
}
template <int DC>
static void launch_ssm_conv_dc(hipStream_t s, const dim3 grid, const tdesc & sx, const tdesc & c, float * y, const float * bias, int64_t d_inner, int64_t n_t, int64_t total) {
    if (bias) hipLaunchKernelGGL((k_ssm_conv<DC, true>), grid, dim3(256), 0, s, sx.data, sx.nb[1], sx.nb[2], c.data, c.nb[1], y, bias, d_inner, n_t, total);
    else hipLaunchKernelGGL((k_ssm_conv<DC, false>), grid, dim3(256), 0, s, sx.data, sx.nb[1], sx.nb[2], c.data, c.nb[1], y, bias, d_inner, n_t, total);
}
bool launch_ssm_conv(hipStream_t s, const tdesc & sx, const tdesc & c, const tdesc & dst, const float * bias) {
    const int64_t d_conv = c.ne[0], d_inner = c.ne[1], n_t = dst.ne[1], n_s = dst.ne[2];
    const int64_t total = d_inner * n_t * n_s;
    if (total == 0) return true;
    const dim3 grid((unsigned) ((total + 255) / 256));
    float * y = (float *) dst.data;
    switch (d_conv) {
        case 2: launch_ssm_conv_dc<2>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 3: launch_ssm_conv_dc<3>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 4: launch_ssm_conv_dc<4>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 5: launch_ssm_conv_dc<5>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 6: launch_ssm_conv_dc<6>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 7: launch_ssm_conv_dc<7>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        case 8: launch_ssm_conv_dc<8>(s, grid, sx, c, y, bias, d_inner, n_t, total); return true;
        default: MI_ERR("launch_ssm_conv: d_conv %lld is not served here", (long long) d_conv); return false;
    }
}

// ------------------------------------------------------------------------------------------------ SSM_SCAN
// For sequence i3, flat row r = i1 + h * head_dim, tokens in order (ggml_compute_forward_ssm_scan_f32):
//   dtp = dt <= 20 ? log1pf(expf(dt)) : dt;  xdt = x * dtp;  dA = expf(dtp * A);  state = state * dA + B * xdt;  y = sum over the state elements of state * C
// with one A per head (Mamba-2: A is [1, n_head]) or one per state element (Mamba-1: [d_state, n_head]).
//
// A workgroup is four waves and owns RPB consecutive rows of one sequence.  The LPR lanes of a row split its d_state elements as float4s (element group
// v * LPR + lane: a row's loads and stores are contiguous 16-byte accesses), so a row's state sits in NV float4 registers a lane for the whole token loop: read once
// from s at row ids[i3] (read on the device), written once behind y.  The sum for y is lane-local, then a DPP reduction inside the row's lanes (a quad for 4
// lanes, a DPP row for 16): no LDS, no atomics.
//                d_state 16: LPR 4, NV 1, 16 rows a wave     64: LPR 16, NV 1, 4 rows     128: LPR 16, NV 2, 4 rows     256: LPR 16, NV 4, 4 rows
// Tokens go in chunks of TC.  Per chunk the workgroup stages, once for all its rows: B and C of the group ([TC][d_state] each), x of its rows ([TC][RPB]), and per
// head it touches and token the softplus dtp and, for Mamba-2, dA — so log1pf / expf are evaluated once per head and token, not per lane.
// Rows tile the flat row index when n_group == 1 (B and C are the same for every head; the Mamba-1 case, head_dim 1) and each head on its own when n_group ==
// n_head (a workgroup then sits inside one head, whose group is its own).  Rows past the end of a tile's domain shadow its first row and store nothing.
template <int D> struct scan_geom {
    static constexpr int LPR = D >= 64 ? 16 : D / 4;
    static constexpr int NV = D / (4 * LPR);
    static constexpr int RPW = 64 / LPR;
    static constexpr int RPB = 4 * RPW;
    static constexpr int TC = D == 16 ? 32 : 2048 / D;
};
struct ssm_scan_args {
    const char * s;       // [d_state, head_dim, n_head, n_rs] contiguous
    int64_t s_nb3;
    int n_rs;
    const char * x;       // [head_dim, n_head, n_t, n_s]: nb0 4, nb1 head_dim * 4
    int64_t x_nb2, x_nb3;
    const float * dt;     // [n_head, n_t, n_s] contiguous
    const float * A;      // [d_state | 1, n_head] contiguous
    const char * B, * C;  // [d_state, n_group, n_t, n_s]: nb0 4, nb1 d_state * 4
    int64_t b_nb2, b_nb3, c_nb2, c_nb3;
    const int32_t * ids;  // [n_s]
    float * y;            // [head_dim, n_head, n_t, n_s] contiguous
    float * st_out;       // [d_state, head_dim, n_head, n_s] contiguous
    int head_dim, n_head, n_group, n_t;
    int dom_rows;         // rows of a tiling domain: head_dim * n_head (n_group == 1) or head_dim
    int tiles_per_dom;
    int vec_state;        // s rows and st_out rows are 16-byte aligned
    int vec_bc;           // B / C rows are
};
__device__ __forceinline__ float4 ld4(const float * p, const bool vec) { return vec ? *(const float4 *) p : make_float4(p[0], p[1], p[2], p[3]); }

template <int D, bool M2>
__global__ void __launch_bounds__(256) k_ssm_scan(const ssm_scan_args p) {
    using G = scan_geom<D>;
    constexpr int LPR = G::LPR, NV = G::NV, RPW = G::RPW, RPB = G::RPB, TC = G::TC, D4 = D / 4;
    __shared__ float4 sB[TC * D4], sC[TC * D4];
    __shared__ float sX[TC][RPB];
    __shared__ float sDt[RPB][TC];
    __shared__ float sDa[M2 ? RPB : 1][M2 ? TC : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i3 = blockIdx.y;
    const int dom = blockIdx.x / p.tiles_per_dom, tile = blockIdx.x % p.tiles_per_dom;
    const int rows_total = p.head_dim * p.n_head;
    const int row0 = tile * RPB;                     // the workgroup's first row inside its domain (always a row of it)
    const int rs = wave * RPW + lane / LPR, li = lane % LPR;
    const bool live = row0 + rs < p.dom_rows;
    const int r_first = dom * p.dom_rows + row0;
    const int r_last = dom * p.dom_rows + min(row0 + RPB, p.dom_rows) - 1;
    const int h_first = r_first / p.head_dim;
    const int n_hb = r_last / p.head_dim - h_first + 1;  // heads this workgroup touches: <= RPB
    const int r = live ? r_first + rs : r_first;
    const int h = r / p.head_dim, hs = h - h_first;
    const int g = p.n_group == 1 ? 0 : h_first;

    // (an id outside the cache is undefined upstream; it is clamped here so that no address leaves s)
    const int id = min(max(p.ids[i3], 0), p.n_rs - 1);
    const float * sp = (const float *) (p.s + (int64_t) id * p.s_nb3) + (int64_t) r * D;
    float4 st[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) st[v] = ld4(sp + 4 * (v * LPR + li), p.vec_state != 0);
    float4 Av[M2 ? 1 : NV];
    if constexpr (!M2) {
        const float * ap = p.A + (int64_t) h * D;
#pragma unroll
        for (int v = 0; v < NV; ++v) Av[v] = ld4(ap + 4 * (v * LPR + li), false);
    }

    for (int t0 = 0; t0 < p.n_t; t0 += TC) {
        const int tc = min(TC, p.n_t - t0);
        __syncthreads();  // the chunk before this one has been read
        for (int e = tid; e < tc * D4; e += 256) {
            const int t = e / D4, q = e % D4;
            const int64_t at = (int64_t) g * D * 4 + (int64_t) q * 16;
            sB[e] = ld4((const float *) (p.B + (int64_t) (t0 + t) * p.b_nb2 + (int64_t) i3 * p.b_nb3 + at), p.vec_bc != 0);
            sC[e] = ld4((const float *) (p.C + (int64_t) (t0 + t) * p.c_nb2 + (int64_t) i3 * p.c_nb3 + at), p.vec_bc != 0);
        }
        for (int e = tid; e < tc * RPB; e += 256) {
            const int t = e / RPB, j = e % RPB;
            sX[t][j] = row0 + j < p.dom_rows ? *(const float *) (p.x + (int64_t) (r_first + j) * 4 + (int64_t) (t0 + t) * p.x_nb2 + (int64_t) i3 * p.x_nb3) : 0.0f;
        }
        for (int e = tid; e < tc * n_hb; e += 256) {
            const int t = e / n_hb, j = e % n_hb;
            const float d = p.dt[(int64_t) (h_first + j) + (int64_t) p.n_head * ((int64_t) (t0 + t) + (int64_t) p.n_t * i3)];
            const float dtp = d <= 20.0f ? log1pf(expf(d)) : d;
            sDt[j][t] = dtp;
            if constexpr (M2) sDa[j][t] = expf(dtp * p.A[h_first + j]);
        }
        __syncthreads();
        for (int t = 0; t < tc; ++t) {
            const float dtp = sDt[hs][t];
            const float xdt = sX[t][rs] * dtp;
            float dA = 0.0f;
            if constexpr (M2) dA = sDa[hs][t];
            float sum = 0.0f;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const float4 b = sB[t * D4 + v * LPR + li], c = sC[t * D4 + v * LPR + li];
                float4 da;
                if constexpr (M2) da = make_float4(dA, dA, dA, dA);
                else da = make_float4(expf(dtp * Av[v].x), expf(dtp * Av[v].y), expf(dtp * Av[v].z), expf(dtp * Av[v].w));
                st[v].x = st[v].x * da.x + b.x * xdt;
                st[v].y = st[v].y * da.y + b.y * xdt;
                st[v].z = st[v].z * da.z + b.z * xdt;
                st[v].w = st[v].w * da.w + b.w * xdt;
                sum += st[v].x * c.x;
                sum += st[v].y * c.y;
                sum += st[v].z * c.z;
                sum += st[v].w * c.w;
            }
            if constexpr (LPR == 16) sum = row16_sum(sum);
            else {
                static_assert(LPR == 4, "a row is a quad or a DPP row");
                sum += dpp_f32<MI_DPP_QUAD_XOR1>(sum);
                sum += dpp_f32<MI_DPP_QUAD_XOR2>(sum);
            }
            if (live && li == 0) p.y[(int64_t) r + (int64_t) rows_total * ((int64_t) (t0 + t) + (int64_t) p.n_t * i3)] = sum;
        }
    }
    if (live) {
        float * op = p.st_out + ((int64_t) i3 * rows_total + r) * D;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float * o = op + 4 * (v * LPR + li);
            if (p.vec_state) *(float4 *) o = st[v];
            else { o[0] = st[v].x; o[1] = st[v].y; o[2] = st[v].z; o[3] = st[v].w; }
        }
    }
}
template <int D>
static void launch_ssm_scan_d(hipStream_t s, ssm_scan_args & p, const bool m2, const int n_dom, const int n_s) {
    p.tiles_per_dom = (p.dom_rows + scan_geom<D>::RPB - 1) / scan_geom<D>::RPB;
    const dim3 grid((unsigned) (n_dom * p.tiles_per_dom), (unsigned) n_s);
    if (m2) hipLaunchKernelGGL((k_ssm_scan<D, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_ssm_scan<D, false>), grid, dim3(256), 0, s, p);
}
bool launch_ssm_scan(hipStream_t s, const tdesc & st, const tdesc & x, const tdesc & dt, const tdesc & A, const tdesc & B, const tdesc & C, const tdesc & ids, const tdesc & dst) {
    const int64_t d_state = st.ne[0], head_dim = x.ne[0], n_head = x.ne[1], n_t = x.ne[2], n_s = x.ne[3], n_group = B.ne[1];
    if (head_dim * n_head * n_t * n_s == 0) return true;  // (a zero-element node; supports_op refuses n_t == 0 with sequences, whose state area would stay unwritten)
    if (n_group != 1 && n_group != n_head) { MI_ERR("launch_ssm_scan: %lld groups over %lld heads are not served here", (long long) n_group, (long long) n_head); return false; }
    ssm_scan_args p;
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
    p.dom_rows = (int) (n_group == 1 ? head_dim * n_head : head_dim);
    p.tiles_per_dom = 0;
    p.vec_state = ((((uintptr_t) st.data) | ((uintptr_t) st.nb[3]) | ((uintptr_t) p.st_out)) & 15) == 0;
    p.vec_bc = ((((uintptr_t) B.data) | ((uintptr_t) C.data) | ((uintptr_t) (B.nb[2] | B.nb[3] | C.nb[2] | C.nb[3]))) & 15) == 0;
    const bool m2 = A.ne[0] == 1;
    const int n_dom = (int) (n_group == 1 ? 1 : n_head);
    switch (d_state) {
        case 16: launch_ssm_scan_d<16>(s, p, m2, n_dom, (int) n_s); return true;
        case 64: launch_ssm_scan_d<64>(s, p, m2, n_dom, (int) n_s); return true;
        case 128: launch_ssm_scan_d<128>(s, p, m2, n_dom, (int) n_s); return true;
        case 256: launch_ssm_scan_d<256>(s, p, m2, n_dom, (int) n_s); return true;
        default: MI_ERR("launch_ssm_scan: d_state %lld is not served here", (long long) d_state); return false;
    }
}

MI_TU_TOUCH(ssm)

}  // namespace mi355x
