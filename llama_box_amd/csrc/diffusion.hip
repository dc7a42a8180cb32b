// diffusion.hip — what the image-generation graphs llama-box serves through --images (stable-diffusion.cpp: the UNet, the VAE, CLIP, the ESRGAN upscaler) need beyond
// the text and tower op set: GROUP_NORM (with the `* w`, `+ b` and SILU nodes that follow it), TIMESTEP_EMBEDDING, DIAG_MASK_INF and LEAKY_RELU.
// DESIGN.md §4n states the operand contracts; graph.cpp's supports_op checks them (one *_ok function an op), the launchers here trust them.  This file is compiled
// with -ffp-contract=off -fno-fast-math: every product, sum and quotient below is one f32 rounding, in the order written.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

// ------------------------------------------------------------------------------------------------ GROUP_NORM (+MUL, +ADD, +SILU)
// ggml_compute_forward_group_norm_f32, which is NORM's arithmetic (ops_act.hip: k_norm) with "row" read as "group": mean = (float) (sum of (double) x / n);
// v = x - mean; var = (float) (sum of (double) (v * v) / n), the square an f32 product; scale = 1 / sqrtf(var + eps); y = v * scale.  src and dst are contiguous
// [W, H, C, N]; with cpg = ceil(C / G) group g of a batch entry is channels [g cpg, min((g + 1) cpg, C)): ONE contiguous run of n = W H (channels) floats that
// starts (batch C + g cpg) W H floats into the tensor — at any 4-byte address (W H = 15: only every fourth group starts on 16 bytes).
// The writing pass of either form also stands for the nodes that follow in a UNet / VAE block, `* w[c]`, `+ b[c]` (w, b: C floats) and SILU, each with the
// rounding of the node it stands for — k_binary's product and sum, k_unary's silu_f —, so the fused bits are the unfused chain's.
// dst may BE src in both forms: nothing is written before the statistics are complete, and the writing pass reads an element in the thread that writes it.
// (x / y carry no __restrict__ for that reason.)
struct gn_args {
    const float * x;
    float * y;
    const float * w, * b;  // per channel, or null
    int silu;
    float eps;
    int64_t wh, C;   // W * H; channels
    int G, cpg;      // groups; channels of a full group
    double * part;   // split form: [2][G * N][nchunk] partial sums (sums of x, then sums of the centred squares)
    int nchunk;      // chunks of a full group
};
struct gn_group {
    int64_t base, n;  // first element in the tensor, length
    int64_t c0;       // first channel
};
__device__ __forceinline__ gn_group gn_locate(const gn_args & p, const int64_t gb) {
    const int64_t g = gb % p.G, batch = gb / p.G;
    gn_group r;
    r.c0 = g * p.cpg;
    r.n = std::min<int64_t>(p.cpg, p.C - r.c0) * p.wh;
    r.base = (batch * p.C + r.c0) * p.wh;
    return r;
}
// A thread works on vectors of four consecutive elements, fetched and stored as ONE 16-byte access that only promises dword alignment (a group starts at any 4-byte
// address); the last vector of a group may be cut short: `avail` (1 .. 4) of its elements exist, the others are neither read nor written.
typedef float __attribute__((ext_vector_type(4), aligned(4))) gn_f4;
__device__ __forceinline__ void gn_load(const float * x, const int64_t e0, const int64_t avail, const float fill, float (&v)[4]) {
    if (avail >= 4) {
        const gn_f4 t = *(const gn_f4 *) (x + e0);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < avail ? x[e0 + k] : fill;
    }
}
// four results r[] whose first is element e0 of its group: the nodes the launch stands for, applied in their order, then the store.  The channel comes from one
// 32-bit division a vector (a group is shorter than 2^31 elements: group_norm_ok) and a carry an element: a vector may cross a channel (W H % 4 != 0)
__device__ __forceinline__ void gn_finish(const gn_args & p, const gn_group & q, float * y, const int64_t e0, const int64_t avail, float (&r)[4]) {
    if (p.w) {
        uint32_t ch = (uint32_t) e0 / (uint32_t) p.wh, rem = (uint32_t) e0 - ch * (uint32_t) p.wh;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = std::min<int64_t>(q.c0 + ch, p.C - 1);  // (past a cut vector's end the channel may be one too far: clamped, the result is dropped)
            r[k] = r[k] * p.w[c];
            if (p.b) r[k] = r[k] + p.b[c];
            if (p.silu) r[k] = silu_f(r[k]);
            if (++rem == (uint32_t) p.wh) { rem = 0; ++ch; }
        }
    }
    if (avail >= 4) {
        gn_f4 o;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
        *(gn_f4 *) (y + e0) = o;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < avail) y[e0 + k] = r[k];
    }
}
// sum over the NW waves of a workgroup, the waves' sums added in wave order; every thread has finished what it did before the call when any thread returns
template <int NW> __device__ __forceinline__ double gn_block_sum(double v, double * sh) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) s += sh[i];
    return s;
}

// RESIDENT form: one workgroup of 1024 threads per (group, batch entry); the group sits in registers between the mean, the variance and the write, so memory is
// read once and written once.  A thread holds U vectors: elements 4 (threadIdx.x + 1024 u) ...  The bound is the register file's: 16 waves on a CU leave a lane
// 128 VGPRs (512 a SIMD lane / 4 waves a SIMD); 40 of them hold data — MI_GN_RESIDENT_MAX = 1024 x 40 = 40 960 values, 160 KB, the largest group of the SD 1.x
// UNet ([64, 64, 320] / 32) —, the rest addresses, the double sums and the affine operands.  LDS holds the 16 wave sums and nothing else.
template <int U>
__global__ void __launch_bounds__(1024) k_group_norm_resident(const gn_args p) {
    __shared__ double sh[16];
    const gn_group q = gn_locate(p, blockIdx.x);
    const float * x = p.x + q.base;
    float * y = p.y + q.base;
    float v[U][4];
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t e = (int64_t) (threadIdx.x + 1024 * u) * 4;
        if (e < q.n) gn_load(x, e, q.n - e, 0.0f, v[u]);
        else v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s += (double) v[u][0] + (double) v[u][1] + (double) v[u][2] + (double) v[u][3];
    const float mean = (float) (gn_block_sum<16>(s, sh) / (double) q.n);
    s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t e = (int64_t) (threadIdx.x + 1024 * u) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e + k < q.n) {
                v[u][k] = v[u][k] - mean;
                s += (double) (v[u][k] * v[u][k]);
            }
        }
    }
    const float var = (float) (gn_block_sum<16>(s, sh) / (double) q.n);
    const float scale = 1.0f / sqrtf(var + p.eps);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t e = (int64_t) (threadIdx.x + 1024 * u) * 4;
        if (e < q.n) {
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = v[u][k] * scale;
            gn_finish(p, q, y, e, q.n - e, r);
        }
    }
}

// SPLIT form: a group is cut into chunks of MI_GN_CHUNK values, one workgroup of 256 threads a chunk (four vectors a thread), three launches with the grid
// (chunks of a full group, G * N):
//   PASS 0  the chunk's double sum of x                        -> part[0][group][chunk]
//   PASS 1  the group's partial sums re-added in chunk order -> mean; the chunk's double sum of the f32 squares of x - mean -> part[1][group][chunk]
//   PASS 2  mean as in pass 1, the second partials re-added in chunk order -> var, scale; y = (x - mean) * scale [* w] [+ b] [silu]
// No atomics and no grid-wide wait: a launch boundary orders the passes, every sum has one fixed order, so a launch is deterministic and replays inside a hipGraph.
// Only pass 2 writes the tensor.  A workgroup whose chunk starts past its (shorter, last) group's end leaves at once; nobody reads its partial.
template <int PASS>
__global__ void __launch_bounds__(256) k_group_norm_split(const gn_args p) {
    __shared__ double sh[4];
    const int64_t gb = blockIdx.y;
    const gn_group q = gn_locate(p, gb);
    const int64_t e_lo = (int64_t) blockIdx.x * MI_GN_CHUNK;
    if (e_lo >= q.n) return;
    const int64_t e_hi = std::min<int64_t>(e_lo + MI_GN_CHUNK, q.n);
    const int nch = (int) ((q.n + MI_GN_CHUNK - 1) / MI_GN_CHUNK);
    double * p1 = p.part + gb * p.nchunk, * p2 = p.part + ((int64_t) gridDim.y + gb) * p.nchunk;
    float mean = 0.0f, scale = 0.0f;
    if constexpr (PASS >= 1) {
        double s = 0.0;
        for (int t = 0; t < nch; ++t) s += p1[t];
        mean = (float) (s / (double) q.n);
    }
    if constexpr (PASS == 2) {
        double s = 0.0;
        for (int t = 0; t < nch; ++t) s += p2[t];
        const float var = (float) (s / (double) q.n);
        scale = 1.0f / sqrtf(var + p.eps);
    }
    const float * x = p.x + q.base;
    constexpr int U = MI_GN_CHUNK / 1024;
    float v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t e = e_lo + (int64_t) (threadIdx.x + 256 * u) * 4;
        const float fill = PASS == 0 ? 0.0f : mean;  // (past the end: x - mean = 0)
        if (e < e_hi) gn_load(x, e, e_hi - e, fill, v[u]);
        else v[u][0] = v[u][1] = v[u][2] = v[u][3] = fill;
    }
    if constexpr (PASS == 2) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = e_lo + (int64_t) (threadIdx.x + 256 * u) * 4;
            if (e < e_hi) {
                float r[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = (v[u][k] - mean) * scale;
                gn_finish(p, q, p.y + q.base, e, e_hi - e, r);
            }
        }
    } else {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (PASS == 0) s += (double) v[u][k];
                else {
                    const float c = v[u][k] - mean;
                    s += (double) (c * c);
                }
            }
        }
        s = gn_block_sum<4>(s, sh);
        if (threadIdx.x == 0) (PASS == 0 ? p1 : p2)[blockIdx.x] = s;
    }
}

static int64_t gn_full_group(const tdesc & src, const int n_groups) { return src.ne[0] * src.ne[1] * ((src.ne[2] + n_groups - 1) / n_groups); }
// which form serves the node: THE one place.  form: the gn_form switch — 2: split everywhere; 1: resident wherever a full group fits the registers; 0: routed —
// resident up to MI_GN_ROUTED_MAX values a full group (kernels.h has the measurement), split above
bool group_norm_runs_resident(const tdesc & src, const int n_groups, const int form) {
    const int64_t n = gn_full_group(src, n_groups);
    if (form == 2 || n > MI_GN_RESIDENT_MAX) return false;
    return form == 1 || n <= MI_GN_ROUTED_MAX;
}
size_t group_norm_scratch_bytes(const tdesc & src, const int n_groups) {
    const int64_t nchunk = (gn_full_group(src, n_groups) + MI_GN_CHUNK - 1) / MI_GN_CHUNK;
    return (size_t) (2 * nchunk * n_groups * src.ne[3]) * sizeof(double);
}
bool launch_group_norm(hipStream_t s, const tdesc & src, const tdesc & dst, const int n_groups, const float eps, const float * mul_w, const float * add_b, const bool silu, const int form,
                       void * scratch, const size_t scratch_bytes) {
    gn_args p{};
    p.x = (const float *) src.data; p.y = (float *) dst.data;
    p.w = mul_w; p.b = mul_w ? add_b : nullptr; p.silu = (mul_w && add_b && silu) ? 1 : 0;
    p.eps = eps;
    p.wh = src.ne[0] * src.ne[1]; p.C = src.ne[2];
    p.G = n_groups; p.cpg = (int) ((src.ne[2] + n_groups - 1) / n_groups);
    const int64_t groups = (int64_t) n_groups * src.ne[3], n = gn_full_group(src, n_groups);
    if (groups == 0 || n == 0) return true;
    if (group_norm_runs_resident(src, n_groups, form)) {
        if (n <= 1024 * 4 * 3) hipLaunchKernelGGL(k_group_norm_resident<3>, dim3((unsigned) groups), dim3(1024), 0, s, p);  // (12 288 values: less unrolled code for the small groups)
        else hipLaunchKernelGGL(k_group_norm_resident<MI_GN_RESIDENT_MAX / 4096>, dim3((unsigned) groups), dim3(1024), 0, s, p);
        return true;
    }
    if (!scratch || scratch_bytes < group_norm_scratch_bytes(src, n_groups)) {
        MI_ERR("launch_group_norm: the split form needs %zu bytes of scratch, %zu were planned", group_norm_scratch_bytes(src, n_groups), scratch ? scratch_bytes : (size_t) 0);
        return false;
    }
    p.part = (double *) scratch;
    p.nchunk = (int) ((n + MI_GN_CHUNK - 1) / MI_GN_CHUNK);
    const dim3 grid((unsigned) p.nchunk, (unsigned) groups);
    hipLaunchKernelGGL(k_group_norm_split<0>, grid, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_group_norm_split<1>, grid, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_group_norm_split<2>, grid, dim3(256), 0, s, p);
    return true;
}

// ------------------------------------------------------------------------------------------------ TIMESTEP_EMBEDDING
// ggml_compute_forward_timestep_embedding_f32: half = dim / 2; for j < half: freq = expf(-logf(max_period) * j / half), arg = t * freq, y[j] = cosf(arg),
// y[j + half] = sinf(arg) — each product and quotient an f32 rounding, left to right; a row is dim rounded up to even wide and every column from 2 half on is 0.
// One thread a result element; the frequencies are evaluated here (DESIGN.md §4n says why no host table), with the device library's expf / logf / cosf / sinf.
__global__ void __launch_bounds__(256) k_timestep_embedding(const float * __restrict__ t, float * __restrict__ y, const int64_t ne0, const int64_t total, const int half, const int max_period) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t col = i % ne0, row = i / ne0;
    float r = 0.0f;
    if (col < 2 * (int64_t) half) {
        const int j = (int) (col < half ? col : col - half);
        const float freq = expf(-logf((float) max_period) * (float) j / (float) half);
        const float arg = t[row] * freq;
        r = col < half ? cosf(arg) : sinf(arg);
    }
    y[i] = r;
}
void launch_timestep_embedding(hipStream_t s, const tdesc & timesteps, const tdesc & dst, const int dim, const int max_period) {
    const int64_t total = dst.ne[0] * dst.ne[1];
    if (total == 0) return;
    hipLaunchKernelGGL(k_timestep_embedding, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, (const float *) timesteps.data, (float *) dst.data, dst.ne[0], total, dim / 2, max_period);
}

// ------------------------------------------------------------------------------------------------ DIAG_MASK_INF
// dst(i0, i1, ...) = -inf where i0 > n_past + i1, src's value elsewhere.  One thread a destination element; rows contiguous on both sides, the other strides free.
// In place (dst is a view of src: the same address and strides) only the masked cells are written.
__global__ void __launch_bounds__(256) k_diag_mask_inf(const tdesc a, const tdesc d, const int n_past, const int64_t total, const bool in_place) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t i0 = i % d.ne[0];
    int64_t r = i / d.ne[0];
    const int64_t i1 = r % d.ne[1];
    r /= d.ne[1];
    const int64_t i2 = r % d.ne[2], i3 = r / d.ne[2];
    const bool masked = i0 > (int64_t) n_past + i1;
    float * out = (float *) (d.data + i0 * 4 + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]);
    if (masked) *out = -INFINITY;
    else if (!in_place) *out = *(const float *) (a.data + i0 * 4 + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3]);
}
void launch_diag_mask_inf(hipStream_t s, const tdesc & src, const tdesc & dst, const int n_past) {
    const int64_t total = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (total == 0) return;
    hipLaunchKernelGGL(k_diag_mask_inf, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, src, dst, n_past, total, src.data == dst.data);
}

// ------------------------------------------------------------------------------------------------ LEAKY_RELU
// fmaxf(x, 0) + slope * fminf(x, 0), the product and the sum two f32 roundings.  The maximum and the minimum are written as selects so that the sign of a zero and a NaN
// do not hang on an instruction's reading of them: -0 ranks below +0 (IEEE 754-2019 maximumNumber / minimumNumber, what v_max_f32 / v_min_f32 give), a NaN gives way to
// the 0 — x = -0 is 0 + slope * -0, a NaN is 0 + slope * 0.  k_unary's launch shape; dst may be src.
__global__ void __launch_bounds__(256) k_leaky_relu(const float * x, float * y, const int64_t n, const float slope) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const float v = x[i];
        const float hi = v > 0.0f ? v : 0.0f, lo = v <= 0.0f ? v : 0.0f;
        const float q = slope * lo;
        y[i] = hi + q;
    }
}
void launch_leaky_relu(hipStream_t s, const tdesc & src, const tdesc & dst, const float slope) {
    const int64_t n = src.ne[0] * src.ne[1] * src.ne[2] * src.ne[3];
    if (n == 0) return;
    const unsigned grid = (unsigned) std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_leaky_relu, dim3(grid), dim3(256), 0, s, (const float *) src.data, (float *) dst.data, n, slope);
}

MI_TU_TOUCH(diffusion)

}  // namespace mi355x
