// ops_act.hip — LayerNorm, the GELU family and the gated units built on it (NORM; UNARY GELU / GELU_QUICK / GELU_ERF; GLU REGLU / GEGLU / GEGLU_QUICK /
// GEGLU_ERF): what the Gemma, BERT-style and LayerNorm-decoder graphs need beyond ops.hip.
//
// Arithmetic: ggml-cpu's, restated from memory ([UPSTREAM-MEMORY]).  GELU and GELU_QUICK are TABLES there — 65 536 f16 results indexed by the
// f16 rounding of the argument, filled at start-up with the process's own tanhf / expf.  The backend fills the same two tables with the same calls on the host
// (graph.cpp: act_tables_host) and uploads them; the kernels here round to f16 (f2h: round to nearest even), gather two bytes and apply the clamps.  Nothing of
// the table is evaluated on the device.  This file is compiled with -ffp-contract=off: every product and sum below is one f32 rounding.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

// sum over the 256 threads (4 waves) of a workgroup; every thread has finished what it did before the call when any thread returns
__device__ __forceinline__ double act_block_sum_d(double v, double * sh) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ------------------------------------------------------------------------------------------------ NORM (+MUL, +ADD)
// ggml_compute_forward_norm_f32: mean = (float) (sum of (double) x / n); v = x - mean; var = (float) (sum of (double) (v * v) / n), the square an f32 product;
// scale = 1 / sqrtf(var + eps); y = v * scale.  Optional fused `* w` and `+ b` (llama.cpp's build_norm with LLM_NORM: the MUL and ADD nodes that follow), each
// its own f32 rounding — the bits of the unfused chain.
// One workgroup per row.  VEC path (row starts of x / y and w / b 16-byte aligned, ne0 % 4 == 0): float4 loads, four independent ones per thread per trip; a row
// of up to 4096 values (ONE trip) stays in registers between the mean, the variance and the write, so memory is read once.  Wider rows and the scalar path read
// the row three times.  dst may BE src (the _inplace form): the block sums are barriers, so nothing is written before every read of both statistics passes has
// completed, and the write pass reads an element in the thread that writes it.  (x / y carry no __restrict__ for that reason.)
__global__ void __launch_bounds__(256) k_norm(const tdesc a, const tdesc d, const float eps, const float * __restrict__ w, const float * __restrict__ b) {
    __shared__ double sh[4];
    const int64_t row = blockIdx.x;
    const int64_t i1 = row % a.ne[1], i2 = (row / a.ne[1]) % a.ne[2], i3 = row / (a.ne[1] * a.ne[2]);
    const float * x = (const float *) (a.data + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3]);
    float * y = (float *) (d.data + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]);
    const int64_t n = a.ne[0];
    const bool vec = (n & 3) == 0 && ((((uintptr_t) x) | ((uintptr_t) y) | ((uintptr_t) w) | ((uintptr_t) b)) & 15) == 0;
    auto affine = [&](float4 r, const int64_t i) {
        if (w) { const float4 g = ((const float4 *) w)[i]; r.x = r.x * g.x; r.y = r.y * g.y; r.z = r.z * g.z; r.w = r.w * g.w; }
        if (b) { const float4 o = ((const float4 *) b)[i]; r.x = r.x + o.x; r.y = r.y + o.y; r.z = r.z + o.z; r.w = r.w + o.w; }
        return r;
    };
    if (vec) {
        const float4 * x4 = (const float4 *) x;
        float4 * y4 = (float4 *) y;
        const int64_t n4 = n >> 2;
        if (n4 <= 1024) {  // the row in registers: 4 float4 a thread
            float4 v[4];
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (threadIdx.x + 256 * u) < n4 ? x4[threadIdx.x + 256 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < 4; ++u) s += (double) v[u].x + (double) v[u].y + (double) v[u].z + (double) v[u].w;
            const float mean = (float) (act_block_sum_d(s, sh) / (double) n);
            s = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if ((threadIdx.x + 256 * u) < n4) {
                    v[u].x = v[u].x - mean; v[u].y = v[u].y - mean; v[u].z = v[u].z - mean; v[u].w = v[u].w - mean;
                    s += (double) (v[u].x * v[u].x) + (double) (v[u].y * v[u].y) + (double) (v[u].z * v[u].z) + (double) (v[u].w * v[u].w);
                }
            }
            const float var = (float) (act_block_sum_d(s, sh) / (double) n);
            const float scale = 1.0f / sqrtf(var + eps);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = threadIdx.x + 256 * u;
                if (i < n4) y4[i] = affine(make_float4(v[u].x * scale, v[u].y * scale, v[u].z * scale, v[u].w * scale), i);
            }
            return;
        }
        double s = 0.0;
        for (int64_t i0 = threadIdx.x; i0 < n4; i0 += 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (i0 + 256 * u) < n4 ? x4[i0 + 256 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < 4; ++u) s += (double) v[u].x + (double) v[u].y + (double) v[u].z + (double) v[u].w;
        }
        const float mean = (float) (act_block_sum_d(s, sh) / (double) n);
        s = 0.0;
        for (int64_t i0 = threadIdx.x; i0 < n4; i0 += 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (i0 + 256 * u) < n4 ? x4[i0 + 256 * u] : make_float4(mean, mean, mean, mean);  // (past the end: v - mean = 0)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 c = make_float4(v[u].x - mean, v[u].y - mean, v[u].z - mean, v[u].w - mean);
                s += (double) (c.x * c.x) + (double) (c.y * c.y) + (double) (c.z * c.z) + (double) (c.w * c.w);
            }
        }
        const float var = (float) (act_block_sum_d(s, sh) / (double) n);
        const float scale = 1.0f / sqrtf(var + eps);
        for (int64_t i0 = threadIdx.x; i0 < n4; i0 += 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) if ((i0 + 256 * u) < n4) v[u] = x4[i0 + 256 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = i0 + 256 * u;
                if (i < n4) y4[i] = affine(make_float4((v[u].x - mean) * scale, (v[u].y - mean) * scale, (v[u].z - mean) * scale, (v[u].w - mean) * scale), i);
            }
        }
        return;
    }
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += (double) x[i];
    const float mean = (float) (act_block_sum_d(s, sh) / (double) n);
    s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float c = x[i] - mean;
        s += (double) (c * c);
    }
    const float var = (float) (act_block_sum_d(s, sh) / (double) n);
    const float scale = 1.0f / sqrtf(var + eps);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        float r = (x[i] - mean) * scale;
        if (w) r = r * w[i];
        if (b) r = r + b[i];
        y[i] = r;
    }
}
void launch_norm(hipStream_t s, const tdesc & src, const tdesc & dst, float eps, const float * mul_w, const float * add_b) {
    const int64_t rows = src.ne[1] * src.ne[2] * src.ne[3];
    hipLaunchKernelGGL(k_norm, dim3((unsigned) rows), dim3(256), 0, s, src, dst, eps, mul_w, add_b);
}

// ------------------------------------------------------------------------------------------------ GELU / GELU_QUICK / GELU_ERF
// tab: T_gelu[65536] then T_quick[65536], f16 bits (backend_ctx::act_tab)
enum { ACT_GELU = 0, ACT_GELU_QUICK = 1, ACT_GELU_ERF = 2, ACT_RELU = 3 };
// ggml_gelu_f32: x <= -10 -> +0, x >= 10 -> x, else the table at the f16 rounding of x.  A NaN fails both comparisons and takes the table (whose NaN entries are NaN)
__device__ __forceinline__ float gelu_tab_f(const float x, const uint16_t * __restrict__ tab) {
    if (x <= -10.0f) return 0.0f;
    if (x >= 10.0f) return x;
    return h2f(tab[f2h(x)]);
}
// ggml_gelu_quick_f32: the table, no clamps — an |x| past the f16 range reads the entry of +-inf (+inf -> inf, -inf -> NaN: -inf * 0), as the reference does
__device__ __forceinline__ float gelu_quick_tab_f(const float x, const uint16_t * __restrict__ tab) { return h2f(tab[65536 + f2h(x)]); }
__device__ __forceinline__ float gelu_erf_f(const float x) {
    const float h = 0.5f * x;
    return h * (1.0f + erff(x * 0.70710678118654752440f));
}
template <int ACT> __device__ __forceinline__ float act_f(const float x, const uint16_t * __restrict__ tab) {
    if constexpr (ACT == ACT_GELU) return gelu_tab_f(x, tab);
    else if constexpr (ACT == ACT_GELU_QUICK) return gelu_quick_tab_f(x, tab);
    else if constexpr (ACT == ACT_GELU_ERF) return gelu_erf_f(x);
    else return x > 0.f ? x : 0.f;
}

template <int ACT>
__global__ void __launch_bounds__(256) k_gelu(const float * __restrict__ x, float * __restrict__ y, const int64_t n, const uint16_t * __restrict__ tab) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) y[i] = act_f<ACT>(x[i], tab);
}
bool launch_gelu(hipStream_t s, int uop, const tdesc & src, const tdesc & dst, const uint16_t * tab) {
    const int64_t n = src.ne[0] * src.ne[1] * src.ne[2] * src.ne[3];
    const unsigned grid = (unsigned) std::min<int64_t>((n + 255) / 256, 2048);
    const float * x = (const float *) src.data;
    float * y = (float *) dst.data;
    if (uop != GGML_UNARY_OP_GELU_ERF && !tab) { MI_ERR("launch_gelu: the GELU tables are not on the device"); return false; }
    switch (uop) {
        case GGML_UNARY_OP_GELU: hipLaunchKernelGGL(k_gelu<ACT_GELU>, dim3(grid), dim3(256), 0, s, x, y, n, tab); return true;
        case GGML_UNARY_OP_GELU_QUICK: hipLaunchKernelGGL(k_gelu<ACT_GELU_QUICK>, dim3(grid), dim3(256), 0, s, x, y, n, tab); return true;
        case GGML_UNARY_OP_GELU_ERF: hipLaunchKernelGGL(k_gelu<ACT_GELU_ERF>, dim3(grid), dim3(256), 0, s, x, y, n, tab); return true;
        default: MI_ERR("launch_gelu: unary op %d is not served here", uop); return false;
    }
}

// ------------------------------------------------------------------------------------------------ GLU: REGLU / GEGLU / GEGLU_QUICK / GEGLU_ERF
// y = act(a) * b (ggml_compute_forward_{reglu,geglu,geglu_quick,geglu_erf}_f32): split form (two tensors) or the two halves of one row; k_swiglu's mapping —
// grid.x = row (2-D, or dense 3-D / 4-D rows: a flat row index), grid.y = chunk of 1024 values, four values a thread; VEC: row starts and strides 16-byte
// aligned and nc % 4 == 0, one float4 per operand.  In GEGLU's x >= 10 branch act(a) is a itself, so the result is a * b.
template <int ACT, bool VEC>
__global__ void __launch_bounds__(256) k_glu(const char * __restrict__ pa, const char * __restrict__ pb, char * __restrict__ pd, const int64_t nc,
                                             const int64_t nba1, const int64_t nbb1, const int64_t nbd1, const uint16_t * __restrict__ tab) {
    const int64_t row = blockIdx.x;
    const float * a = (const float *) (pa + row * nba1);
    const float * b = (const float *) (pb + row * nbb1);
    float * y = (float *) (pd + row * nbd1);
    const int64_t i0 = ((int64_t) blockIdx.y * 256 + threadIdx.x) * 4;
    if constexpr (VEC) {
        if (i0 < nc) {  // (nc % 4 == 0)
            const float4 av = *(const float4 *) (a + i0), bv = *(const float4 *) (b + i0);
            *(float4 *) (y + i0) = make_float4(act_f<ACT>(av.x, tab) * bv.x, act_f<ACT>(av.y, tab) * bv.y, act_f<ACT>(av.z, tab) * bv.z, act_f<ACT>(av.w, tab) * bv.w);
        }
    } else {
        for (int64_t i = i0; i < i0 + 4 && i < nc; ++i) y[i] = act_f<ACT>(a[i], tab) * b[i];
    }
}
template <int ACT>
static void launch_glu_act(hipStream_t s, const dim3 grid, const bool vec, const char * pa, const char * pb, char * pd, int64_t nc, int64_t nba1, int64_t nbb1, int64_t nbd1, const uint16_t * tab) {
    if (vec) hipLaunchKernelGGL((k_glu<ACT, true>), grid, dim3(256), 0, s, pa, pb, pd, nc, nba1, nbb1, nbd1, tab);
    else hipLaunchKernelGGL((k_glu<ACT, false>), grid, dim3(256), 0, s, pa, pb, pd, nc, nba1, nbb1, nbd1, tab);
}
bool launch_glu(hipStream_t s, int glu_op, const tdesc & a, const tdesc * b, const tdesc & d, int swapped, const uint16_t * tab) {
    const int64_t rows = a.ne[1] * a.ne[2] * a.ne[3];
    const int64_t nc = d.ne[0];
    const char * pa = a.data;
    const char * pb = b ? b->data : a.data;
    if (!b) {
        pa += swapped ? nc * 4 : 0;
        pb += swapped ? 0 : nc * 4;
    }
    const int64_t nbb1 = b ? b->nb[1] : a.nb[1];
    const bool vec = (nc % 4) == 0 && (((uintptr_t) pa | (uintptr_t) pb | (uintptr_t) d.data | (uintptr_t) a.nb[1] | (uintptr_t) nbb1 | (uintptr_t) d.nb[1]) & 15) == 0;
    const dim3 grid((unsigned) rows, (unsigned) ((nc + 1023) / 1024));
    if ((glu_op == GGML_GLU_OP_GEGLU || glu_op == GGML_GLU_OP_GEGLU_QUICK) && !tab) { MI_ERR("launch_glu: the GELU tables are not on the device"); return false; }
    switch (glu_op) {
        case GGML_GLU_OP_REGLU: launch_glu_act<ACT_RELU>(s, grid, vec, pa, pb, d.data, nc, a.nb[1], nbb1, d.nb[1], tab); return true;
        case GGML_GLU_OP_GEGLU: launch_glu_act<ACT_GELU>(s, grid, vec, pa, pb, d.data, nc, a.nb[1], nbb1, d.nb[1], tab); return true;
        case GGML_GLU_OP_GEGLU_QUICK: launch_glu_act<ACT_GELU_QUICK>(s, grid, vec, pa, pb, d.data, nc, a.nb[1], nbb1, d.nb[1], tab); return true;
        case GGML_GLU_OP_GEGLU_ERF: launch_glu_act<ACT_GELU_ERF>(s, grid, vec, pa, pb, d.data, nc, a.nb[1], nbb1, d.nb[1], tab); return true;
        default: MI_ERR("launch_glu: GLU operator %d is not served here", glu_op); return false;
    }
}

MI_TU_TOUCH(ops_act)

}  // namespace mi355x
