// mmbf.hip — mat-mul with a bf16 src0: the weight matrices of a model stored in bf16.
//
// Restates ggml_compute_forward_mul_mat for vec_dot_type BF16: the f32 activations are FIRST rounded to bf16 (ggml-cpu's from_float:
// ggml_compute_fp32_to_bf16 — nearest even, subnormals kept, NaN kept quiet: f2bf of kv_quant.h, in integer arithmetic), a weight is its 16
// bits shifted up, the products of two bf16 values are exact in f32 and the accumulation is f32 (the CPU sums in double; only the order and
// the width of the sum differ — the gate is tests/test_gpu_ops.py::test_mul_mat_f's NMSE 1e-11).
//
// Forms (launch_mul_mat_bf16 / mul_mat_bf16_form decide in one place):
//   k_mmv_bf16<NC, R, NT>   1 .. 8 columns: the weight stream.  The columns are staged ONCE per workgroup into LDS as bf16, a wave owns R rows
//                           and keeps 8 16-byte loads (8 KiB) in flight ahead of the FMAs.
//   k_mul_mat_mma16         few columns / few tiles over long rows: 16 x 16 tiles on v_mfma_f32_16x16x32_bf16
//   k_mul_mat_mma           batches: 32 x 32 tiles on v_mfma_f32_32x32x16_bf16, src1 rounded in the loop or once ahead of it (k_round_bf16)
//   k_mul_mat_dot           the dot kernel: unaligned operands, K % 8 != 0, broadcast batches
// The last three are mm_dense.h's templates — the kernels mmf.hip runs over f16 operands — instantiated for elem_bf16; the streaming kernel, the rounding
// launch, the form decision, the timing classes and the launchers are this file's own.
#include <cstdlib>

#include "mm_dense.h"

namespace mi355x {

// src1 [K, M] f32 (rows 16-byte aligned, K % 8 == 0) -> [M][K] bf16: one thread per 8 values
__global__ void __launch_bounds__(256) k_round_bf16(const char * __restrict__ X, const int64_t x_nb1, uint4 * __restrict__ out, const int ng, const int64_t total) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t c = i / ng, g = i - c * ng;
    const char * xp = X + c * x_nb1 + g * 32;
    out[i] = elem_bf16::round8(*(const uint4 *) xp, *(const uint4 *) (xp + 16));
}

// ---- 1 .. 8 columns: the weight stream.  A decode step of a bf16 model reads every weight once (16 GB a token at 8 B parameters) and does two flops a byte: the
// kernel is its loads.  The dot kernel gives a wave one or two dependent 1-KiB loads at a time; here
//   * the grid is a fixed number of workgroups (two a CU, fewer when the rows do not fill them) that stay for the whole matrix: a workgroup (4 waves) rounds the
//     M <= NC activation columns to bf16 ONCE into LDS ([NC][K] bf16 — no quantise launch, no prologue: the rounding IS the staging) and its waves then walk
//     groups of R consecutive rows, wave w of W taking groups w, w + W, ... (neighbouring waves read neighbouring rows at any one time),
//   * a lane's unit is one 16-byte load of eight weights at k = 8 (lane + 64 t): one wave-instruction covers 1 KiB, eight whole 128-byte lines of ONE row,
//   * 8 / R trips x R rows = 8 loads a lane are requested before the first FMA of a round; with 1 or 2 columns the next round's — of the same rows or of the
//     wave's next group — before the current one is multiplied (the first round's go out ahead of the staging),
//   * f32 FMAs into R x NC accumulators, wave_sum at the end of a group, lane 0 stores.
// NT: the weight loads carry the non-temporal hint (read once; rows are whole lines wherever K * 2 % 128 == 0).  Past a row's end a lane fetches the row's first
// group instead and multiplies zeros; past the last row a wave re-reads row N - 1 and stores nothing.
typedef uint32_t mmbf_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ uint4 mmbf_ld16(const char * p) {
    if (NT) return __builtin_bit_cast(uint4, __builtin_nontemporal_load((const mmbf_u32x4 *) p));
    return *(const uint4 *) p;
}
template <int NC, int R, bool NT>
__global__ void __launch_bounds__(256) k_mmv_bf16(const char * __restrict__ W, const int64_t w_nb1, const char * __restrict__ X, const int64_t x_nb1, float * __restrict__ D,
                                                   const int64_t d_nb1, const int K, const int N, const int M) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NC][K / 8] groups of 8 bf16
    constexpr int TR = 8 / R;                                     // trips a round
    constexpr bool DB = NC <= 2;                                  // the next round's loads go out ahead of this round's FMAs (4 and 8 columns: the accumulators take those registers; other waves cover)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = (int) gridDim.x * 4, n_grp = (N + R - 1) / R;
    const int ng = K >> 3;
    auto fetch = [&](const int grp, const int g0, uint4 (&w)[TR][R]) {
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const int g = g0 + 64 * t + lane;
            const size_t off = (size_t) (g < ng ? g : 0) * 16;
#pragma unroll
            for (int r = 0; r < R; ++r) w[t][r] = mmbf_ld16<NT>(W + (size_t) min(grp * R + r, N - 1) * w_nb1 + off);
        }
    };
    uint4 w[TR][R];
    int grp = (int) blockIdx.x * 4 + wave, g0 = 0;
    if (grp < n_grp) fetch(grp, 0, w);
    for (int i = tid; i < NC * ng; i += 256) {
        const int c = i / ng, g = i - c * ng;
        uint4 o = make_uint4(0, 0, 0, 0);
        if (c < M) {
            const char * xp = X + (size_t) c * x_nb1 + (size_t) g * 32;
            o = elem_bf16::round8(*(const uint4 *) xp, *(const uint4 *) (xp + 16));
        }
        *(uint4 *) (smem + (size_t) i * 16) = o;
    }
    __syncthreads();
    float acc[R][NC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[r][c] = 0.0f;
    while (grp < n_grp) {  // (grp, g0: uniform over the wave)
        int grp_n = grp, g0_n = g0 + 64 * TR;
        if (g0_n >= ng) {
            grp_n = grp + n_waves;
            g0_n = 0;
        }
        const bool more = grp_n < n_grp;
        uint4 wn[DB ? TR : 1][DB ? R : 1];
        if constexpr (DB) {
            if (more) fetch(grp_n, g0_n, wn);
        }
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const int g = g0 + 64 * t + lane;
            const bool in = g < ng;
            const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
            const int gc = in ? g : 0;
            float wf[R][8];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint4 q = w[t][r];
                q.x &= keep; q.y &= keep; q.z &= keep; q.w &= keep;
                elem_bf16::unpack8(q, wf[r]);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float xf[8];
                elem_bf16::unpack8(*(const uint4 *) (smem + ((size_t) c * ng + gc) * 16), xf);
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[r][c] = fmaf(wf[r][i], xf[i], acc[r][c]);
            }
        }
        if (grp_n != grp) {  // the group's last round: its R x NC sums
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float v = wave_sum(acc[r][c]);
                    if (lane == 0 && grp * R + r < N && c < M) D[(size_t) c * d_nb1 + grp * R + r] = v;
                    acc[r][c] = 0.0f;
                }
        }
        if (more) {
            if constexpr (DB) {
#pragma unroll
                for (int t = 0; t < TR; ++t)
#pragma unroll
                    for (int r = 0; r < R; ++r) w[t][r] = wn[t][r];
            } else fetch(grp_n, g0_n, w);
        }
        grp = grp_n;
        g0 = g0_n;
    }
}

// ------------------------------------------------------------------------------------------------ routing
#define MMV_LDS_MAX (64 * 1024)

// widest column chunk of the streaming kernel whose staged columns ([cap][K] bf16) fit one launch's LDS
static int mmv_col_cap(const int64_t K) {
    int cap = 8;
    while (cap > 1 && (int64_t) cap * K * 2 > MMV_LDS_MAX) cap >>= 1;
    return cap;
}
// force: MI_BF16_* to measure or test a form where it can serve the operands (else the form decided here), -1 = decide; max_cols: the widest batch the streaming
// kernel takes (0 .. 8, the hand-over to the 16 x 16 tiles; 0: never — the dot kernel serves one column)
int mul_mat_bf16_form(const tdesc & a, const tdesc & b, const tdesc & d, const int force, const int max_cols) {
    const int64_t K = a.ne[0], N = a.ne[1], M = b.ne[1];
    if (!mm_vec_ok(a, b, 2) || force == MI_BF16_DOT) return MI_BF16_DOT;
    const bool flat = a.ne[2] == 1 && a.ne[3] == 1 && b.ne[2] == 1 && b.ne[3] == 1 && d.nb[0] == 4 && (d.nb[1] % 4) == 0;
    const bool mmv_ok = flat && K * 2 <= MMV_LDS_MAX && K <= INT32_MAX / 16 && N <= INT32_MAX / 8 && M <= 65535;
    if (force == MI_BF16_MMA16 || force == MI_BF16_MMA) return force;
    if ((force == MI_BF16_MMV || force == MI_BF16_MMV_COLS) && mmv_ok) return M == 1 ? MI_BF16_MMV : MI_BF16_MMV_COLS;
    // measured hand-overs (profiles/r09_bf16_bench.txt): the streaming kernel up to 4 columns, up to 8 where the matrix has 8192 rows or more (at 8
    // columns it loses to the 16 x 16 tiles at 4096 x 4096 and 4096 x 1024, and wins at 4096 x 14336 and 4096 x 128256), and only while ALL columns fit one
    // launch's LDS (K = 14336: 2 columns — in two launches 4 columns took 58.7 us against 33.3 us on the tiles)
    const int64_t nc = M <= 2 ? M : (M <= 4 ? 4 : 8);  // columns the kernel stages
    if (mmv_ok && M <= std::min(8, max_cols) && (M <= 4 || N >= 8192) && nc * K * 2 <= MMV_LDS_MAX) return M == 1 ? MI_BF16_MMV : MI_BF16_MMV_COLS;
    if (M < 2) return MI_BF16_DOT;
    const int64_t waves32 = ((N + 31) / 32) * ((M + 31) / 32) * b.ne[2] * b.ne[3];
    // (mmf.hip hands its f16 attention operands over at 2048 waves; weight matrices measured: 16 x 16 tiles win at 64 columns x 4096 rows [256 waves] and lose at
    // 64 x 14336 [896], 512 x 1024 [512] and 16 x 128256 [4008])
    if (M < 16 || (K >= 1024 && waves32 < 512)) return MI_BF16_MMA16;
    return MI_BF16_MMA;
}
const char * mul_mat_bf16_class(const int form, const int64_t M) {
    switch (form) {
        case MI_BF16_MMV: return "mmv_bf16_nc1";
        case MI_BF16_MMV_COLS: return M <= 2 ? "mmv_bf16_nc2" : (M <= 4 ? "mmv_bf16_nc4" : "mmv_bf16_nc8");
        case MI_BF16_MMA16: return "mul_mat_bf16_mma16";
        case MI_BF16_MMA: return "mul_mat_bf16_mma";
        default: return "mul_mat_bf16_dot";
    }
}

// workgroups of the streaming launch: two a CU (8 waves x 8 KiB requested ahead of the FMAs), fewer when the row groups do not fill them
static int mmv_grid(const int64_t n_grp) {
    static const int n_cu = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            (void) hipGetLastError();
            v = 256;
        }
        return v;
    }();
    return (int) std::max<int64_t>(1, std::min<int64_t>((n_grp + 3) / 4, 2 * (int64_t) n_cu));
}
template <int NC, int R> static void launch_mmv_t(hipStream_t s, const tdesc & a, const char * x, int64_t x_nb1, float * dst, int64_t d_nb1, int m, bool nt) {
    const int K = (int) a.ne[0], N = (int) a.ne[1];
    const dim3 grid((unsigned) mmv_grid((N + R - 1) / R));
    const size_t lds = (size_t) NC * K * 2;
    if (nt) hipLaunchKernelGGL((k_mmv_bf16<NC, R, true>), grid, dim3(256), lds, s, a.data, (int64_t) a.nb[1], x, x_nb1, dst, d_nb1, K, N, m);
    else hipLaunchKernelGGL((k_mmv_bf16<NC, R, false>), grid, dim3(256), lds, s, a.data, (int64_t) a.nb[1], x, x_nb1, dst, d_nb1, K, N, m);
}
template <int NC> static void launch_mmv_nc(hipStream_t s, const tdesc & a, const char * x, int64_t x_nb1, float * dst, int64_t d_nb1, int m, bool nt) {
    // rows a group: more rows share one read of the staged columns, but every wave of the grid (8 a CU) should still get several groups
    const int64_t N = a.ne[1];
    if (N >= 65536) launch_mmv_t<NC, 4>(s, a, x, x_nb1, dst, d_nb1, m, nt);
    else if (N >= 16384 || NC >= 4) launch_mmv_t<NC, 2>(s, a, x, x_nb1, dst, d_nb1, m, nt);  // (4 / 8 columns on one row a group: 8 trips x NC staged groups held at once — 256 VGPRs and AGPR copies)
    else if constexpr (NC < 4) launch_mmv_t<NC, 1>(s, a, x, x_nb1, dst, d_nb1, m, nt);
}
// columns in chunks of the widest NC whose staged columns fit LDS; the weights are streamed once a chunk
static void launch_mmv(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, const bool nt) {
    const int64_t M = b.ne[1];
    const int cap = mmv_col_cap(a.ne[0]);
    for (int64_t c0 = 0; c0 < M; c0 += cap) {
        const int m = (int) std::min<int64_t>(cap, M - c0);
        const char * x = b.data + c0 * b.nb[1];
        float * dst = (float *) (d.data + c0 * d.nb[1]);
        const int64_t d_nb1 = (int64_t) (d.nb[1] / 4);
        if (m == 1) launch_mmv_nc<1>(s, a, x, b.nb[1], dst, d_nb1, m, nt);
        else if (m == 2) launch_mmv_nc<2>(s, a, x, b.nb[1], dst, d_nb1, m, nt);
        else if (m <= 4) launch_mmv_nc<4>(s, a, x, b.nb[1], dst, d_nb1, m, nt);
        else launch_mmv_nc<8>(s, a, x, b.nb[1], dst, d_nb1, m, nt);
    }
}
int mul_mat_bf16_launches(const int form, const tdesc & a, const tdesc & b) {
    if (form != MI_BF16_MMV && form != MI_BF16_MMV_COLS) return 1;
    const int cap = mmv_col_cap(a.ne[0]);
    return (int) ((b.ne[1] + cap - 1) / cap);
}

// scratch of the 32 x 32 tile form with src1 rounded to bf16 once ahead of the launch (0: the operands do not take that form)
size_t mul_mat_bf16_workspace_bytes(const tdesc & a, const tdesc & b) {
    if (!mm_vec_ok(a, b, 2) || a.ne[2] != 1 || a.ne[3] != 1 || b.ne[2] != 1 || b.ne[3] != 1 || b.ne[1] < 64) return 0;
    return (size_t) (b.ne[1] * a.ne[0] * 2);
}
// form: what mul_mat_bf16_form answered for these operands (< 0: asked here, with the defaults); nt: the weight loads of the streaming kernel carry the
// non-temporal hint; ws / ws_bytes: scratch — when it holds mul_mat_bf16_workspace_bytes, the 32 x 32 tile form reads src1 from a bf16 copy made once
void launch_mul_mat_bf16(hipStream_t s, const tdesc & a, const tdesc & b, const tdesc & d, int form, const bool nt, void * ws, const size_t ws_bytes) {
    const int64_t K = a.ne[0];
    if (form < 0) form = mul_mat_bf16_form(a, b, d, -1, MI_BF16_MMV_MAX_COLS);
    switch (form) {
        case MI_BF16_MMV: case MI_BF16_MMV_COLS:
            launch_mmv(s, a, b, d, nt);
            return;
        case MI_BF16_MMA16:
            launch_mul_mat_mma16<elem_bf16>(s, a, b, d);
            return;
        case MI_BF16_MMA: {
            dim3 grid((unsigned) ((a.ne[1] + 63) / 64), (unsigned) ((b.ne[1] + 63) / 64), (unsigned) (b.ne[2] * b.ne[3]));
            const size_t need = ws ? mul_mat_bf16_workspace_bytes(a, b) : 0;
            if (need > 0 && need <= ws_bytes && (((uintptr_t) ws) & 15) == 0) {
                const int ng = (int) (K / 8);
                const int64_t total = (int64_t) ng * b.ne[1];
                hipLaunchKernelGGL(k_round_bf16, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, b.data, (int64_t) b.nb[1], (uint4 *) ws, ng, total);
                tdesc xb = b;
                xb.data = (char *) ws;
                xb.nb[0] = 2;
                xb.nb[1] = (size_t) K * 2;
                xb.nb[2] = xb.nb[1] * (size_t) b.ne[1];
                xb.nb[3] = xb.nb[2];
                hipLaunchKernelGGL((k_mul_mat_mma<elem_bf16, true>), grid, dim3(256), 0, s, a, xb, d);
                return;
            }
            hipLaunchKernelGGL((k_mul_mat_mma<elem_bf16, false>), grid, dim3(256), 0, s, a, b, d);
            return;
        }
        default: break;
    }
    launch_mul_mat_dot<elem_bf16>(s, a, b, d, mm_vec_ok(a, b, 2));
}

MI_TU_TOUCH(mmbf)

}  // namespace mi355x
