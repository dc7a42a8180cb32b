// conv.hip — the front end and the projector tail of a vision / audio tower (llama-box --mmproj: ggml_conv_2d patch embeddings, Whisper-style ggml_conv_1d stems,
// Gemma-3's pooled projector, frame stacking, resized position embeddings): IM2COL, the f16 x f16 MUL_MAT that consumes it, POOL_1D / POOL_2D, PAD and UPSCALE.
// DESIGN.md §4m states the operand contracts; graph.cpp's supports_op checks them (one *_ok function an op), the launchers here trust them.  This file is compiled
// with -ffp-contract=off -fno-fast-math: every product, sum and quotient below is one f32 rounding, in the order written — the pools and the resize are the bits of
// their f32 twins (tests/conv_ref.py), the gathers are exact.
#include <algorithm>

#include "mm_dense.h"

namespace mi355x {

// ------------------------------------------------------------------------------------------------ IM2COL
// dst[n, oh, ow, ic * KH * KW + kh * KW + kw] = src[n, ic, oh * s1 + kh * d1 - p1, ow * s0 + kw * d0 - p0], zero outside the image; dst contiguous, so it is one flat
// array of rows of CK = IC * KH * KW elements.  A thread owns V consecutive elements of a row (V divides CK: a vector never crosses a row) and writes them with one
// store of V * sizeof(T) bytes — the launcher picks the widest V the row length and the base address allow (16 bytes at CK % 8 == 0 for f16; an odd CK leaves 2-byte
// stores).  (kw, kh, ic) of the first element come from three divisions, the others by carrying.  The 1-D form is the 2-D one with KH = OH = IH = 1.
struct im2col_args {
    const char * src;
    int64_t nb_row, nb_ic, nb_n;  // bytes between image rows, channels, batches
    int64_t IW, IH, KW, KH, OW, OH, CK;
    int s0, s1, p0, p1, d0, d1;
    int64_t n_vec;  // vectors of V elements in dst
};
template <typename T> __device__ __forceinline__ T im2col_cvt(const float v);
template <> __device__ __forceinline__ uint16_t im2col_cvt<uint16_t>(const float v) { return f2h(v); }  // round-to-nearest-even
template <> __device__ __forceinline__ float im2col_cvt<float>(const float v) { return v; }

template <typename T, int V>
__global__ void __launch_bounds__(256) k_im2col(const im2col_args p, T * __restrict__ dst) {
    const int64_t iv = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (iv >= p.n_vec) return;
    const int64_t e0 = iv * V;
    int64_t k = e0 % p.CK, r = e0 / p.CK;
    const int64_t ow = r % p.OW;
    r /= p.OW;
    const int64_t oh = r % p.OH, n = r / p.OH;
    int64_t kw = k % p.KW;
    k /= p.KW;
    int64_t kh = k % p.KH, ic = k / p.KH;
    const char * img = p.src + n * p.nb_n;
    const int64_t ih0 = oh * p.s1 - p.p1, iw0 = ow * p.s0 - p.p0;
    T out[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int64_t ih = ih0 + kh * p.d1, iw = iw0 + kw * p.d0;
        float v = 0.0f;
        if (ih >= 0 && ih < p.IH && iw >= 0 && iw < p.IW) v = *(const float *) (img + ic * p.nb_ic + ih * p.nb_row + iw * 4);
        out[i] = im2col_cvt<T>(v);
        if (++kw == p.KW) {
            kw = 0;
            if (++kh == p.KH) {
                kh = 0;
                ++ic;
            }
        }
    }
    typedef T vec_t __attribute__((ext_vector_type(V)));
    if constexpr (V == 1) dst[e0] = out[0];
    else {
        vec_t o;
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = out[i];
        *(vec_t *) (dst + e0) = o;
    }
}
template <typename T> static void launch_im2col_t(hipStream_t s, im2col_args p, char * dst, const int64_t n_elem) {
    constexpr int VMAX = 16 / (int) sizeof(T);
    int V = VMAX;
    while (V > 1 && ((p.CK % V) != 0 || (((uintptr_t) dst) % (V * sizeof(T))) != 0)) V >>= 1;
    p.n_vec = n_elem / V;
    const dim3 grid((unsigned) ((p.n_vec + 255) / 256));
    if (V == 8) { if constexpr (VMAX >= 8) hipLaunchKernelGGL((k_im2col<T, 8>), grid, dim3(256), 0, s, p, (T *) dst); }
    else if (V == 4) hipLaunchKernelGGL((k_im2col<T, 4>), grid, dim3(256), 0, s, p, (T *) dst);
    else if (V == 2) hipLaunchKernelGGL((k_im2col<T, 2>), grid, dim3(256), 0, s, p, (T *) dst);
    else hipLaunchKernelGGL((k_im2col<T, 1>), grid, dim3(256), 0, s, p, (T *) dst);
}
// kernel: only its extents are read ([KW, KH, IC, OC] / [KW, IC, OC]); src f32 [IW, IH, IC, N] / [IW, IC, N]; dst f16 / f32 [IC * KH * KW, OW, OH, N] / [IC * KW, OW, N]
bool launch_im2col(hipStream_t s, const tdesc & kernel, const tdesc & src, const tdesc & dst, const int32_t * op_params) {
    const bool is_2d = op_params[6] != 0;
    im2col_args p{};
    p.src = src.data;
    p.s0 = op_params[0]; p.p0 = op_params[2]; p.d0 = op_params[4];
    p.s1 = is_2d ? op_params[1] : 1; p.p1 = is_2d ? op_params[3] : 0; p.d1 = is_2d ? op_params[5] : 1;
    p.IW = src.ne[0]; p.IH = is_2d ? src.ne[1] : 1;
    p.KW = kernel.ne[0]; p.KH = is_2d ? kernel.ne[1] : 1;
    p.OW = dst.ne[1]; p.OH = is_2d ? dst.ne[2] : 1;
    p.CK = dst.ne[0];
    p.nb_row = is_2d ? src.nb[1] : 0; p.nb_ic = is_2d ? src.nb[2] : src.nb[1]; p.nb_n = is_2d ? src.nb[3] : src.nb[2];
    const int64_t n_elem = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (n_elem == 0) return true;
    if (dst.type == GGML_TYPE_F16) launch_im2col_t<uint16_t>(s, p, dst.data, n_elem);
    else if (dst.type == GGML_TYPE_F32) launch_im2col_t<float>(s, p, dst.data, n_elem);
    else { MI_ERR("launch_im2col: result type %d is not served here", dst.type); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------ MUL_MAT, f16 x f16
// ggml-cpu's arithmetic for vec_dot_type F16 when src1 already has that type: neither operand is rounded, products of two f16 values are exact in f32, f32 sums.
// Dot form: mm_dense.h's k_mul_mat_dot with the 2-byte src1 reader elem_f16_x16 — anything, odd K included.
// Matrix-core form: the 32 x 32 tile walk of k_mul_mat_mma (a wave owns 32 src0 rows x 32 src1 columns on v_mfma_f32_32x32x16_f16, K in steps of 16, four steps'
// loads in flight), with both operands 16-bit already and each lane's 16 bytes of a step fetched as 16 / W loads of W bytes: W = 16 needs 16-byte-aligned rows and
// K % 8 == 0, W = 8 serves 8-byte-aligned rows with K % 4 == 0 (K = 588, the 14 x 14 x 3 patch: rows of 1176 bytes), W = 4 any even K at 4-byte-aligned rows.  A load
// unit lies wholly inside the row or wholly past K (K is a multiple of its elements); past K the row's first unit is fetched instead — no branch between the loads — and
// masked to zero.  The order of the K steps is fixed: a launch is deterministic.
template <int W> __device__ __forceinline__ uint4 mmx_load8(const char * row, const int64_t e, const int64_t K) {
    uint32_t u[4];
    if constexpr (W == 16) {
        const bool in = e < K;
        const uint4 t = *(const uint4 *) (row + (in ? e : 0) * 2);
        const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
        return make_uint4(t.x & keep, t.y & keep, t.z & keep, t.w & keep);
    } else if constexpr (W == 8) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool in = e + 4 * j < K;
            const uint2 t = *(const uint2 *) (row + (in ? e + 4 * j : 0) * 2);
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            u[2 * j] = t.x & keep;
            u[2 * j + 1] = t.y & keep;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = e + 2 * j < K;
            const uint32_t t = *(const uint32_t *) (row + (in ? e + 2 * j : 0) * 2);
            u[j] = in ? t : 0u;
        }
    }
    return make_uint4(u[0], u[1], u[2], u[3]);
}
template <int W>
__global__ void __launch_bounds__(256) k_mul_mat_f16x_mma(const tdesc a, const tdesc b, const tdesc d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, g = lane >> 5;
    const int64_t row0 = ((int64_t) blockIdx.x * 2 + (wave & 1)) * 32, col0 = ((int64_t) blockIdx.y * 2 + (wave >> 1)) * 32;
    if (row0 >= a.ne[1] || col0 >= b.ne[1]) return;
    const int64_t i12 = blockIdx.z % b.ne[2], i13 = blockIdx.z / b.ne[2];
    const int64_t i02 = i12 / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t K = a.ne[0];
    const char * wrow = a.data + std::min<int64_t>(row0 + r32, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2] + i03 * a.nb[3];  // this lane's src0 row
    const char * xcol = b.data + std::min<int64_t>(col0 + r32, b.ne[1] - 1) * b.nb[1] + i12 * b.nb[2] + i13 * b.nb[3];  // this lane's src1 column
    mm_float16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = 0; k < K; k += 64) {
        uint4 w[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // k-group g of a step: elements k + 16 u + 8 g .. + 7
            const int64_t e = k + 16 * u + 8 * g;
            w[u] = mmx_load8<W>(wrow, e, K);
            x[u] = mmx_load8<W>(xcol, e, K);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = elem_f16::mfma32(__builtin_bit_cast(elem_f16::vec8, x[u]), w[u], acc);
    }
    // lane: src0 row row0 + r32; register i: src1 column col0 + (i & 3) + 8 (i >> 2) + 4 g
    const int64_t row = row0 + r32;
    if (row >= a.ne[1]) return;
    char * out = d.data + row * d.nb[0] + i12 * d.nb[2] + i13 * d.nb[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t col = col0 + (i & 3) + 8 * (i >> 2) + 4 * g;
        if (col < b.ne[1]) *(float *) (out + col * d.nb[1]) = acc[i];
    }
}
// the widest load unit (bytes) the matrix-core form may use on these operands; 0: none — an odd K, or rows that are only 2-byte aligned
static int mmx_load_width(const tdesc & a, const tdesc & b) {
    if (a.nb[0] != 2 || b.nb[0] != 2) return 0;
    const int64_t K = a.ne[0];
    for (int W = 16; W >= 4; W >>= 1) {
        bool ok = (K % (W / 2)) == 0 && ((((uintptr_t) a.data) | ((uintptr_t) b.data)) & (uintptr_t) (W - 1)) == 0;
        for (int i = 1; i < 4; ++i) ok = ok && (a.nb[i] % W) == 0 && (b.nb[i] % W) == 0;
        if (ok) return W;
    }
    return 0;
}
// which form serves the node.  mma: the conv_mma switch — 0: the dot form everywhere; 2: the matrix-core form wherever the operands allow (tests, measurements);
// 1: routed by the count of 32 x 32 result tiles.  A wave walks the whole K of its tile on its own, so a product of a few tiles is one dependent chain per wave
// (9.9 us at 2 tiles of K 588) while the dot form spreads the same work over hundreds of workgroups (6.8 us): below MI_CONV_MMA_MIN_TILES the dot form keeps
// the node (scripts/ubench/conv_bench.py)
bool mul_mat_f16x_runs_mma(const tdesc & a, const tdesc & b, const int mma) {
    if (mma == 0 || mmx_load_width(a, b) == 0) return false;
    return mma == 2 || ((a.ne[1] + 31) / 32) * ((b.ne[1] + 31) / 32) * b.ne[2] * b.ne[3] >= MI_CONV_MMA_MIN_TILES;
}
void launch_mul_mat_f16x(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, const int mma) {
    if (a.ne[1] == 0 || b.ne[1] == 0 || b.ne[2] * b.ne[3] == 0) return;
    if (mul_mat_f16x_runs_mma(a, b, mma)) {
        const dim3 grid((unsigned) ((a.ne[1] + 63) / 64), (unsigned) ((b.ne[1] + 63) / 64), (unsigned) (b.ne[2] * b.ne[3]));
        switch (mmx_load_width(a, b)) {
            case 16: hipLaunchKernelGGL(k_mul_mat_f16x_mma<16>, grid, dim3(256), 0, s, a, b, d); break;
            case 8: hipLaunchKernelGGL(k_mul_mat_f16x_mma<8>, grid, dim3(256), 0, s, a, b, d); break;
            default: hipLaunchKernelGGL(k_mul_mat_f16x_mma<4>, grid, dim3(256), 0, s, a, b, d); break;
        }
        return;
    }
    // 16-byte vector path of the dot kernel: K % 8 == 0 and every row start 16-byte aligned on both sides
    bool vec_ok = a.nb[0] == 2 && b.nb[0] == 2 && (a.ne[0] % 8) == 0 && ((((uintptr_t) a.data) | ((uintptr_t) b.data)) & 15) == 0;
    for (int i = 1; i < 4; ++i) vec_ok = vec_ok && (a.nb[i] % 16) == 0 && (b.nb[i] % 16) == 0;
    launch_mul_mat_dot<elem_f16_x16>(s, a, b, d, vec_ok);
}

// ------------------------------------------------------------------------------------------------ POOL_2D / POOL_1D
// One thread an output element (dst contiguous; src rows contiguous, the other strides free).  The accumulator starts at 0 (AVG) or -FLT_MAX (MAX), the window is
// walked ky outer, kx inner from (ox * s0 - p0, oy * s1 - p1), cells outside the plane are skipped, AVG then divides by (float) (k0 * k1): padding cells count in the
// divisor.  POOL_1D is the same walk with k1 = s1 = 1, p1 = 0 over rows of dim 1.
struct pool_args {
    const char * src;
    int64_t nb1, nb2, nb3;
    int64_t W, H, OW, OH, ne2;
    int k0, k1, s0, s1, p0, p1;
    int64_t total;
};
template <bool AVG>
__global__ void __launch_bounds__(256) k_pool(const pool_args p, float * __restrict__ dst) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    const int64_t ox = i % p.OW;
    int64_t r = i / p.OW;
    const int64_t oy = r % p.OH;
    r /= p.OH;
    const int64_t i2 = r % p.ne2, i3 = r / p.ne2;
    const char * plane = p.src + i2 * p.nb2 + i3 * p.nb3;
    const int64_t x0 = ox * p.s0 - p.p0, y0 = oy * p.s1 - p.p1;
    float acc = AVG ? 0.0f : -FLT_MAX;
    for (int ky = 0; ky < p.k1; ++ky) {
        const int64_t y = y0 + ky;
        if (y < 0 || y >= p.H) continue;
        const float * row = (const float *) (plane + y * p.nb1);
        for (int kx = 0; kx < p.k0; ++kx) {
            const int64_t x = x0 + kx;
            if (x < 0 || x >= p.W) continue;
            const float v = row[x];
            if (AVG) acc += v;
            else if (v > acc) acc = v;
        }
    }
    if (AVG) acc = acc / (float) (p.k0 * p.k1);
    dst[i] = acc;
}
bool launch_pool(hipStream_t s, const tdesc & src, const tdesc & dst, const int32_t * op_params, const bool is_2d) {
    pool_args p{};
    p.src = src.data;
    p.nb1 = src.nb[1]; p.nb2 = src.nb[2]; p.nb3 = src.nb[3];
    p.W = src.ne[0]; p.OW = dst.ne[0];
    if (is_2d) {
        p.k0 = op_params[1]; p.k1 = op_params[2]; p.s0 = op_params[3]; p.s1 = op_params[4]; p.p0 = op_params[5]; p.p1 = op_params[6];
        p.H = src.ne[1]; p.OH = dst.ne[1]; p.ne2 = dst.ne[2];
    } else {  // rows of dim 1 are planes of height 1: (i1, i2) -> (oy, i2) with the row stride as the "image row" stride and a window of one row
        p.k0 = op_params[1]; p.k1 = 1; p.s0 = op_params[2]; p.s1 = 1; p.p0 = op_params[3]; p.p1 = 0;
        p.H = src.ne[1]; p.OH = dst.ne[1]; p.ne2 = dst.ne[2];
    }
    p.total = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (p.total == 0) return true;
    const dim3 grid((unsigned) ((p.total + 255) / 256));
    if (op_params[0] == 1) hipLaunchKernelGGL(k_pool<true>, grid, dim3(256), 0, s, p, (float *) dst.data);
    else if (op_params[0] == 0) hipLaunchKernelGGL(k_pool<false>, grid, dim3(256), 0, s, p, (float *) dst.data);
    else { MI_ERR("launch_pool: pool op %d", op_params[0]); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------ PAD
// dst contiguous, every extent >= src's: src's values at the low indices, zero elsewhere.  One thread a destination element; src at any element-aligned strides.
__global__ void __launch_bounds__(256) k_pad(const tdesc a, const tdesc d, const int64_t total) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t i0 = i % d.ne[0];
    int64_t r = i / d.ne[0];
    const int64_t i1 = r % d.ne[1];
    r /= d.ne[1];
    const int64_t i2 = r % d.ne[2], i3 = r / d.ne[2];
    uint32_t v = 0;
    if (i0 < a.ne[0] && i1 < a.ne[1] && i2 < a.ne[2] && i3 < a.ne[3]) v = *(const uint32_t *) (a.data + i0 * a.nb[0] + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3]);
    ((uint32_t *) d.data)[i] = v;
}
void launch_pad(hipStream_t s, const tdesc & src, const tdesc & dst) {
    const int64_t total = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (total == 0) return;
    hipLaunchKernelGGL(k_pad, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, src, dst, total);
}

// ------------------------------------------------------------------------------------------------ UPSCALE
// sf_d = (float) dst.ne[d] / src.ne[d].  Nearest: src index (int64) ((float) i_d / sf_d) in every dimension.  Bilinear (no align-corners) over dims 0 and 1, nearest
// over dims 2 and 3: x = ((float) i0 + 0.5f) / sf0 - 0.5f, x0 = floorf(x), x1 = x0 + 1, both clamped to [0, W - 1], dx = x - (float) x0 with the CLAMPED x0, then clamped
// to [0, 1]; dim 1 alike; value = a (1 - dx) (1 - dy) + b dx (1 - dy) + c (1 - dx) dy + d dx dy, left to right.  One thread a destination element.
// (the nearest index is clamped to the source's extent for memory safety only: with extents below 2^24, which supports_op asks, the quotient never reaches it)
struct upscale_args {
    float sf0, sf1, sf2, sf3;
    int64_t total;
};
__device__ __forceinline__ int64_t upscale_nearest(const int64_t i, const float sf, const int64_t n) { return std::min<int64_t>((int64_t) ((float) i / sf), n - 1); }
template <bool BILINEAR>
__global__ void __launch_bounds__(256) k_upscale(const tdesc a, const tdesc d, const upscale_args p) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    const int64_t i0 = i % d.ne[0];
    int64_t r = i / d.ne[0];
    const int64_t i1 = r % d.ne[1];
    r /= d.ne[1];
    const int64_t i2 = r % d.ne[2], i3 = r / d.ne[2];
    const char * plane = a.data + upscale_nearest(i2, p.sf2, a.ne[2]) * a.nb[2] + upscale_nearest(i3, p.sf3, a.ne[3]) * a.nb[3];
    float v;
    if constexpr (BILINEAR) {
        const float x = ((float) i0 + 0.5f) / p.sf0 - 0.5f, y = ((float) i1 + 0.5f) / p.sf1 - 0.5f;
        int64_t x0 = (int64_t) floorf(x), y0 = (int64_t) floorf(y);
        int64_t x1 = x0 + 1, y1 = y0 + 1;
        x0 = std::max<int64_t>(0, std::min<int64_t>(x0, a.ne[0] - 1));
        x1 = std::max<int64_t>(0, std::min<int64_t>(x1, a.ne[0] - 1));
        y0 = std::max<int64_t>(0, std::min<int64_t>(y0, a.ne[1] - 1));
        y1 = std::max<int64_t>(0, std::min<int64_t>(y1, a.ne[1] - 1));
        float dx = x - (float) x0, dy = y - (float) y0;
        dx = fmaxf(0.0f, fminf(dx, 1.0f));
        dy = fmaxf(0.0f, fminf(dy, 1.0f));
        const float va = *(const float *) (plane + y0 * a.nb[1] + x0 * 4), vb = *(const float *) (plane + y0 * a.nb[1] + x1 * 4);
        const float vc = *(const float *) (plane + y1 * a.nb[1] + x0 * 4), vd = *(const float *) (plane + y1 * a.nb[1] + x1 * 4);
        const float t0 = va * (1.0f - dx) * (1.0f - dy);
        const float t1 = vb * dx * (1.0f - dy);
        const float t2 = vc * (1.0f - dx) * dy;
        const float t3 = vd * dx * dy;
        v = ((t0 + t1) + t2) + t3;
    } else {
        v = *(const float *) (plane + upscale_nearest(i1, p.sf1, a.ne[1]) * a.nb[1] + upscale_nearest(i0, p.sf0, a.ne[0]) * 4);
    }
    ((float *) d.data)[i] = v;
}
bool launch_upscale(hipStream_t s, const tdesc & src, const tdesc & dst, const int mode) {
    upscale_args p{};
    p.sf0 = (float) dst.ne[0] / src.ne[0]; p.sf1 = (float) dst.ne[1] / src.ne[1]; p.sf2 = (float) dst.ne[2] / src.ne[2]; p.sf3 = (float) dst.ne[3] / src.ne[3];
    p.total = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (p.total == 0) return true;
    const dim3 grid((unsigned) ((p.total + 255) / 256));
    if (mode == 0) hipLaunchKernelGGL(k_upscale<false>, grid, dim3(256), 0, s, src, dst, p);
    else if (mode == 1) hipLaunchKernelGGL(k_upscale<true>, grid, dim3(256), 0, s, src, dst, p);
    else { MI_ERR("launch_upscale: mode %d is not served here", mode); return false; }
    return true;
}

MI_TU_TOUCH(conv)

}  // namespace mi355x
