// mm_dense.h — what the dense mat-mul kernels of mmf.hip (f16 / f32 src0), mmbf.hip (bf16 src0) and mmid.hip (k_mmid_f) share: the element traits and the
// three kernels that exist once per 16-bit format.
//
// A kernel of this family restates ggml_compute_forward_mul_mat for vec_dot_type F16 / BF16 / F32: the f32 activations are FIRST rounded to src0's format (ggml-cpu's
// from_float), products of two 16-bit values are exact in f32 and the accumulation is f32.  The A / B lane maps and the C / D maps of the bf16 MFMA instructions
// are those of the f16 ones, so between the two formats only three things differ, and they are the traits' members: how eight f32 activations become an A operand,
// how a stored element becomes f32, and which instruction multiplies.  Everything else — addressing, masked tails, loop, reduction, epilogue — is written once
// below, and an f16 and a bf16 matrix holding the same values sum in the same order (tests/test_gpu_bf16_weights.py pins that bit for bit).
#pragma once
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"
#include "kv_quant.h"

namespace mi355x {

typedef float mm_float16 __attribute__((ext_vector_type(16)));
typedef float mm_float4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ element traits
// SIZE: bytes of a stored element, XSIZE: of a src1 element; x1: one src1 element at an address -> f32 as the product takes it; cvt1 / load1 / unpack8 / load8: stored elements (bits, or at an address) -> f32; round1: the from_float round trip of one
// activation, x8: of the eight at an address; vec8: the MFMA operand of eight, round8: eight f32 activations (as bits) -> the A operand; mfma32 / mfma16:
// v_mfma_f32_32x32x16 / v_mfma_f32_16x16x32 (B = 16 bytes as loaded).  Each member is the conversion its kernels have always used, in the form they used it: the
// kernels compile to the instruction streams they had before the formats shared a source (uint4 by reference for f16 and by value for bf16 is part of that).
struct elem_f32 {  // (the dot kernels only: no rounding, no matrix-core form)
    static constexpr int SIZE = 4, XSIZE = 4;
    static __device__ __forceinline__ void load8(const char * p, float (&w)[8]) {
        const float4 t0 = *(const float4 *) p, t1 = *(const float4 *) (p + 16);
        w[0] = t0.x; w[1] = t0.y; w[2] = t0.z; w[3] = t0.w; w[4] = t1.x; w[5] = t1.y; w[6] = t1.z; w[7] = t1.w;
    }
    static __device__ __forceinline__ float load1(const char * p) { return *(const float *) p; }
    static __device__ __forceinline__ float round1(const float v) { return v; }
    static __device__ __forceinline__ float x1(const char * p) { return *(const float *) p; }
    static __device__ __forceinline__ void x8(const char * p, float (&x)[8]) { load8(p, x); }
};

struct elem_f16 {
    static constexpr int SIZE = 2, XSIZE = 4;
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float cvt1(const uint16_t h) { return h2f(h); }
    static __device__ __forceinline__ void unpack8(const uint4 & t, float (&w)[8]) {
        const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[2 * i] = cvt1((uint16_t) (u[i] & 0xFFFF));
            w[2 * i + 1] = cvt1((uint16_t) (u[i] >> 16));
        }
    }
    static __device__ __forceinline__ void load8(const char * p, float (&w)[8]) { unpack8(*(const uint4 *) p, w); }
    static __device__ __forceinline__ float load1(const char * p) { return cvt1(*(const uint16_t *) p); }
    static __device__ __forceinline__ float round1(const float v) { return h2f(f2h(v)); }
    static __device__ __forceinline__ float x1(const char * p) { return round1(*(const float *) p); }
    static __device__ __forceinline__ void x8(const char * p, float (&x)[8]) {
        elem_f32::load8(p, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = round1(x[i]);
    }
    static __device__ __forceinline__ vec8 round8(const uint4 & p0, const uint4 & p1) {
        return (vec8){(_Float16) __builtin_bit_cast(float, p0.x), (_Float16) __builtin_bit_cast(float, p0.y), (_Float16) __builtin_bit_cast(float, p0.z),
                      (_Float16) __builtin_bit_cast(float, p0.w), (_Float16) __builtin_bit_cast(float, p1.x), (_Float16) __builtin_bit_cast(float, p1.y),
                      (_Float16) __builtin_bit_cast(float, p1.z), (_Float16) __builtin_bit_cast(float, p1.w)};
    }
    static __device__ __forceinline__ mm_float16 mfma32(const vec8 x, const uint4 & w, const mm_float16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(vec8, w), acc, 0, 0, 0);
    }
    static __device__ __forceinline__ mm_float4 mfma16(const vec8 x, const uint4 & w, const mm_float4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, __builtin_bit_cast(vec8, w), acc, 0, 0, 0);
    }
};

// (rounding: ggml_compute_fp32_to_bf16 — nearest even, subnormals kept, NaN kept quiet: f2bf of kv_quant.h, in integer arithmetic; a stored element is its 16
// bits shifted up.  round8 hands the eight bf16 on as the uint4 they are packed into: the operand type appears at the instruction only)
struct elem_bf16 {
    static constexpr int SIZE = 2, XSIZE = 4;
    typedef __bf16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float cvt1(const uint16_t h) { return __uint_as_float((uint32_t) h << 16); }
    static __device__ __forceinline__ void unpack8(const uint4 t, float (&w)[8]) {  // the low half of a dword shifted up, the high half masked in place
        const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[2 * i] = __uint_as_float(u[i] << 16);
            w[2 * i + 1] = __uint_as_float(u[i] & 0xFFFF0000u);
        }
    }
    static __device__ __forceinline__ void load8(const char * p, float (&w)[8]) { unpack8(*(const uint4 *) p, w); }
    static __device__ __forceinline__ float load1(const char * p) { return cvt1(*(const uint16_t *) p); }
    static __device__ __forceinline__ float round1(const float v) { return cvt1(f2bf(v)); }
    static __device__ __forceinline__ float x1(const char * p) { return round1(*(const float *) p); }
    static __device__ __forceinline__ uint32_t pack2(const float lo, const float hi) { return (uint32_t) f2bf(lo) | ((uint32_t) f2bf(hi) << 16); }
    static __device__ __forceinline__ uint4 round8(const uint4 p0, const uint4 p1) {
        uint4 o;
        o.x = pack2(__uint_as_float(p0.x), __uint_as_float(p0.y));
        o.y = pack2(__uint_as_float(p0.z), __uint_as_float(p0.w));
        o.z = pack2(__uint_as_float(p1.x), __uint_as_float(p1.y));
        o.w = pack2(__uint_as_float(p1.z), __uint_as_float(p1.w));
        return o;
    }
    static __device__ __forceinline__ void x8(const char * p, float (&x)[8]) { unpack8(round8(*(const uint4 *) p, *(const uint4 *) (p + 16)), x); }
    static __device__ __forceinline__ mm_float16 mfma32(const uint4 & x, const uint4 & w, const mm_float16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vec8, x), __builtin_bit_cast(vec8, w), acc, 0, 0, 0);
    }
    static __device__ __forceinline__ mm_float4 mfma16(const uint4 & x, const uint4 & w, const mm_float4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(vec8, x), __builtin_bit_cast(vec8, w), acc, 0, 0, 0);
    }
};

// f16 src0 against an f16 src1 (the convolution kernel behind an IM2COL; conv.hip): ggml-cpu's vec_dot_type F16 when src1 already has that type — nothing is
// rounded, an activation is read as the 2-byte element it is (the dot kernel only; the matrix-core form of this pair is conv.hip's own)
struct elem_f16_x16 : elem_f16 {
    static constexpr int XSIZE = 2;
    static __device__ __forceinline__ float x1(const char * p) { return load1(p); }
    static __device__ __forceinline__ void x8(const char * p, float (&x)[8]) { load8(p, x); }
};

// ------------------------------------------------------------------------------------------------ host helpers
// 16-byte vector path: contiguous dim 0 on both sides (src0 elements of esz bytes, f32 src1), K a multiple of 8, every row start 16-byte aligned
static inline bool mm_vec_ok(const tdesc & a, const tdesc & b, const size_t esz) {
    bool ok = a.nb[0] == esz && b.nb[0] == 4 && (a.ne[0] % 8) == 0 && (((uintptr_t) a.data) & 15) == 0 && (((uintptr_t) b.data) & 15) == 0;
    for (int i = 1; i < 4; ++i) ok = ok && (a.nb[i] % 16) == 0 && (b.nb[i] % 16) == 0;
    return ok;
}
// lanes that own a row of K elements, per_lane of them a lane and trip: the smallest of 8 .. 64 that covers the row in one trip
static inline int mm_lanes_per_row(const int64_t K, const int per_lane) {
    int lpr = 64;
    while (lpr > 8 && (int64_t) (lpr / 2) * per_lane >= K) lpr >>= 1;
    return lpr;
}

// ------------------------------------------------------------------------------------------------ the dot kernel
// Layout: a sub-wave group of LPR lanes owns one src0 row (LPR = 8..64 chosen so that 8-element vectors cover K), 64/LPR rows per wave, 4 waves per workgroup;
// rows are read with 16-byte loads when alignment allows (vec_ok), else element by element through the strides: unaligned operands, K % 8 != 0.  ggml
// broadcasting: src0 dims 2/3 repeat over src1's.
template <typename E>
__global__ void __launch_bounds__(256) k_mul_mat_dot(const tdesc a, const tdesc b, const tdesc d, const int lpr, const int vec_ok) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rpw = 64 / lpr;  // rows per wave
    const int sub = lane / lpr, sl = lane % lpr;
    const int64_t i01 = ((int64_t) blockIdx.x * 4 + wave) * rpw + sub;
    const int64_t i11 = blockIdx.y;
    const int64_t i12 = blockIdx.z % b.ne[2], i13 = blockIdx.z / b.ne[2];
    const int64_t i02 = i12 / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t K = a.ne[0];
    const bool live = i01 < a.ne[1];
    const int64_t r = live ? i01 : a.ne[1] - 1;
    const char * wrow = a.data + r * a.nb[1] + i02 * a.nb[2] + i03 * a.nb[3];
    const char * xcol = b.data + i11 * b.nb[1] + i12 * b.nb[2] + i13 * b.nb[3];
    float acc = 0.0f;
    if (vec_ok) {
        for (int64_t k = (int64_t) sl * 8; k < K; k += (int64_t) lpr * 8) {
            float w[8], x[8];
            E::load8(wrow + k * E::SIZE, w);
            E::x8(xcol + k * E::XSIZE, x);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fmaf(w[i], x[i], acc);
        }
    } else {
        for (int64_t k = sl; k < K; k += lpr) {
            const float wv = E::load1(wrow + k * a.nb[0]);
            const float xv = E::x1(xcol + k * b.nb[0]);
            acc = fmaf(wv, xv, acc);
        }
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (live && sl == 0) *(float *) (d.data + i01 * d.nb[0] + i11 * d.nb[1] + i12 * d.nb[2] + i13 * d.nb[3]) = acc;
}
template <typename E> static void launch_mul_mat_dot(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, const bool vec_ok) {
    const int lpr = mm_lanes_per_row(a.ne[0], vec_ok ? 8 : 1);
    const int rows_per_block = 4 * (64 / lpr);
    dim3 grid((unsigned) ((a.ne[1] + rows_per_block - 1) / rows_per_block), (unsigned) b.ne[1], (unsigned) (b.ne[2] * b.ne[3]));
    hipLaunchKernelGGL(k_mul_mat_dot<E>, grid, dim3(256), 0, s, a, b, d, lpr, vec_ok ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------ batches: 32 x 32 tiles
// (K.Q and V.softmax of a prompt chunk on the non-flash path — llama-box's default, engine_param.hpp:772-779 —, prompt batches over a bf16 weight.)  The dot
// kernel above reads a src0 row once per src1 column: 512 tokens against 512 cells took 0.64 ms per call, 41 of the 61 ms of a 512-token prefill.  Here a wave
// owns a 32 (src0 rows) x 32 (src1 columns) tile of one head on v_mfma_f32_32x32x16 and walks K in steps of 16: src0 is 16-bit already — 16 bytes per lane
// straight from memory into the B operand (n = row = lane & 31, k-group lane >> 5) —, src1 is rounded on the way into the A operand (m = column), exactly the
// rounding ggml-cpu's from_float applies; the accumulation is f32 (order differs from the CPU's, as between any two of its SIMD builds).  No LDS: the operand
// loads are row-strided (65 clocks per wave-instruction, scripts/ubench/ta_probe.hip) and that is the bound — 3 loads per MFMA —, which is still ~30x the dot
// kernel on these shapes.
// XPRE (bf16 only): src1 was rounded once by k_round_bf16 ([M][K] bf16 in scratch, described by `b`): one 16-byte load a step and no conversion in the loop
template <typename E, bool XPRE>
__global__ void __launch_bounds__(256) k_mul_mat_mma(const tdesc a, const tdesc b, const tdesc d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, g = lane >> 5;
    const int64_t row0 = ((int64_t) blockIdx.x * 2 + (wave & 1)) * 32, col0 = ((int64_t) blockIdx.y * 2 + (wave >> 1)) * 32;
    if (row0 >= a.ne[1] || col0 >= b.ne[1]) return;
    const int64_t i12 = blockIdx.z % b.ne[2], i13 = blockIdx.z / b.ne[2];
    const int64_t i02 = i12 / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t K = a.ne[0];
    const char * wrow = a.data + std::min<int64_t>(row0 + r32, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2] + i03 * a.nb[3] + g * 16;  // this lane's src0 row, its k-group
    const char * xcol = b.data + std::min<int64_t>(col0 + r32, b.ne[1] - 1) * b.nb[1] + i12 * b.nb[2] + i13 * b.nb[3] + g * (XPRE ? 16 : 32);  // this lane's src1 column
    mm_float16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = 0; k < K; k += 64) {  // 4 steps of 16 per trip, their loads in flight together
        // k-group g of a step: elements kk + 8g .. kk + 8g + 7; past the end (the last step of a K that is 8 mod 16 has no second group): the
        // row's first group is fetched instead — no branch between the loads — and masked to zeros
        uint4 w[4], x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t kk = k + 16 * u;
            const bool in = kk + 8 * g < K;
            const int64_t kc = in ? kk : -8 * g;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            w[u] = *(const uint4 *) (wrow + kc * 2);
            if constexpr (XPRE) {
                x0[u] = *(const uint4 *) (xcol + kc * 2);
                x1[u] = x0[u];
            } else {
                x0[u] = *(const uint4 *) (xcol + kc * 4);
                x1[u] = *(const uint4 *) (xcol + kc * 4 + 16);
            }
            w[u].x &= keep; w[u].y &= keep; w[u].z &= keep; w[u].w &= keep;
            x0[u].x &= keep; x0[u].y &= keep; x0[u].z &= keep; x0[u].w &= keep;
            x1[u].x &= keep; x1[u].y &= keep; x1[u].z &= keep; x1[u].w &= keep;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if constexpr (XPRE) acc = E::mfma32(x0[u], w[u], acc);
            else acc = E::mfma32(E::round8(x0[u], x1[u]), w[u], acc);
        }
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

// ------------------------------------------------------------------------------------------------ few tiles over long rows: 16 x 16 tiles
// The same contract for few output tiles and long rows (V^T.p of a -np decode batch on the non-flash path: 128 x 32 results per head over thousands of cells —
// 128 waves of the kernel above, each walking all of K, took 170 us), and for 2..15 columns: 16 x 16 tiles on v_mfma_f32_16x16x32 (A: src1 column
// m = lane & 15, B: src0 row n = lane & 15, k-group lane >> 4), the NWK waves of a workgroup take the K steps of ONE tile in turn and add up through LDS in
// wave order (deterministic).
template <typename E, int NWK>
__global__ void __launch_bounds__(64 * NWK) k_mul_mat_mma16(const tdesc a, const tdesc b, const tdesc d) {
    __shared__ mm_float4 red[NWK][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int64_t row0 = (int64_t) blockIdx.x * 16, col0 = (int64_t) blockIdx.y * 16;
    const int64_t i12 = blockIdx.z % b.ne[2], i13 = blockIdx.z / b.ne[2];
    const int64_t i02 = i12 / (b.ne[2] / a.ne[2]), i03 = i13 / (b.ne[3] / a.ne[3]);
    const int64_t K = a.ne[0];
    const char * wrow = a.data + std::min<int64_t>(row0 + r16, a.ne[1] - 1) * a.nb[1] + i02 * a.nb[2] + i03 * a.nb[3] + kg * 16;
    const char * xcol = b.data + std::min<int64_t>(col0 + r16, b.ne[1] - 1) * b.nb[1] + i12 * b.nb[2] + i13 * b.nb[3] + kg * 32;
    mm_float4 acc = {0, 0, 0, 0};
    for (int64_t k = (int64_t) wave * 32; k < K; k += 32 * NWK * 4) {  // 4 steps' loads in flight
        uint4 w[4], x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t kk = k + (int64_t) u * 32 * NWK;
            const bool in = kk + 8 * kg < K;  // past the end: fetch the row's first group instead (no branch between the loads) and mask it to zeros
            const int64_t kc = in ? kk : -8 * kg;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            w[u] = *(const uint4 *) (wrow + kc * 2);
            x0[u] = *(const uint4 *) (xcol + kc * 4);
            x1[u] = *(const uint4 *) (xcol + kc * 4 + 16);
            w[u].x &= keep; w[u].y &= keep; w[u].z &= keep; w[u].w &= keep;
            x0[u].x &= keep; x0[u].y &= keep; x0[u].z &= keep; x0[u].w &= keep;
            x1[u].x &= keep; x1[u].y &= keep; x1[u].z &= keep; x1[u].w &= keep;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = E::mfma16(E::round8(x0[u], x1[u]), w[u], acc);
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < NWK; ++w) acc += red[w][lane];
    // lane: src0 row row0 + r16; register i: src1 column col0 + 4 kg + i
    const int64_t row = row0 + r16;
    if (row >= a.ne[1]) return;
    char * out = d.data + row * d.nb[0] + i12 * d.nb[2] + i13 * d.nb[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t col = col0 + 4 * kg + i;
        if (col < b.ne[1]) *(float *) (out + col * d.nb[1]) = acc[i];
    }
}
template <typename E> static void launch_mul_mat_mma16(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d) {
    dim3 grid((unsigned) ((a.ne[1] + 15) / 16), (unsigned) ((b.ne[1] + 15) / 16), (unsigned) (b.ne[2] * b.ne[3]));
    if (a.ne[0] >= 4096) hipLaunchKernelGGL((k_mul_mat_mma16<E, 16>), grid, dim3(1024), 0, s, a, b, d);
    else hipLaunchKernelGGL((k_mul_mat_mma16<E, 8>), grid, dim3(512), 0, s, a, b, d);
}

}  // namespace mi355x
