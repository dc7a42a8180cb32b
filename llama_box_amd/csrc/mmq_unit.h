// mmq_unit.h — the integer matrix-core work unit that mmq_skinny.hip (dense weights x 2..32 columns, and its wide form) and mmid_group.hip (expert weights x the
// pairs routed to one expert) share: 32 weight rows x one 256-value super-block x 32 activation columns, staged in LDS as sk_fmt lays it out.  mmq_skinny.hip's
// header says why the unit looks the way it does (weights = B operand, digit planes, the f16 bsum MFMA); nothing here knows where the operands came from.
#pragma once

#include "dev_util.h"
#include "kernels.h"
#include "mmvq_types.h"

namespace mi355x {

typedef _Float16 half8s __attribute__((ext_vector_type(8)));
typedef float float16s __attribute__((ext_vector_type(16)));
typedef int int4s __attribute__((ext_vector_type(4)));
typedef int int2s __attribute__((ext_vector_type(2)));
typedef int int16s __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));

constexpr int SK_NW = 8;            // waves per workgroup
constexpr int SK_BTOK = 304;        // LDS bytes per token of the activation unit: 256 qs + 32 bsums (f16) + 16 pad (76 dwords = 4 * 19)
constexpr int SK_B_BYTES = 32 * SK_BTOK;
template <int QT> struct sk_fmt;
template <> struct sk_fmt<4> { static constexpr int BYTES = 144, PIECES = 9, ROW = 144; };   // 36 dwords = 4 * 9
template <> struct sk_fmt<5> { static constexpr int BYTES = 176, PIECES = 11, ROW = 176; };  // 44 dwords = 4 * 11
template <> struct sk_fmt<6> { static constexpr int BYTES = 210, PIECES = 14, ROW = 240; };  // 14 pieces + 16 pad: 60 dwords = 4 * 15
template <int QT> constexpr int sk_wave_lds() { return 32 * sk_fmt<QT>::ROW + SK_B_BYTES + 128; }

__device__ __forceinline__ uint32_t sk_pack_h2(const float a, const float b) {
    typedef _Float16 half2s __attribute__((ext_vector_type(2)));
    const half2s h = {(_Float16) a, (_Float16) b};
    return __builtin_bit_cast(uint32_t, h);
}

// four bytes of a dword times a small digit with ONE v_pk_mul_lo_u16 (every byte product stays below 256: no carry crosses a byte)
__device__ __forceinline__ uint32_t sk_pk_mul(const uint32_t a, const uint32_t b) {
    typedef unsigned short ushort2s __attribute__((ext_vector_type(2)));
    const ushort2s r = __builtin_bit_cast(ushort2s, a) * __builtin_bit_cast(ushort2s, b);
    return __builtin_bit_cast(uint32_t, r);
}
// byte K of w replicated into both 16-bit lanes: 0x00bb00bb
template <int K> __device__ __forceinline__ uint32_t sk_rep_byte(const uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c000c00u | (uint32_t) K | ((uint32_t) K << 16)); }

// One unit (32 weight rows x one super-block x 32 tokens) of Q4_K / Q5_K: arow = this lane's row in the staged weight unit ([row][block
// bytes]), btok = this lane's token in the staged activation unit ([token][256 qs | 32 bsums f16 | ..]), dAs = the 32 activation block
// scales; g = lane >> 5 (the k-group of the MFMA operands).  Adds the unit's contribution to acc (register i: token (i & 3) + 8 (i >> 2) + 4 g).
// The 6-bit sub-block scale cannot ride in an int8 operand (sc * q reaches 945), and folding each MFMA's int32 result with the
// lane's scale costs 16 v_mul_i32_i24 per MFMA — measured at ~6.8 clocks each where an fp32 fma issues in 2
// (scripts/ubench/valu_probe.hip): 128 of them were half of a unit's time.  So the scale is split into digits, sc = 8 s1 + s0 (Q4_K:
// q <= 15, digits <= 7, products <= 105) or 16 s2 + 4 s1 + s0 (Q5_K: q <= 31, digits <= 3, products <= 93), one int8 weight operand per
// digit (four nibbles x digit = ONE v_pk_mul_lo_u16), and the digit planes accumulate over all eight sub-blocks INSIDE the matrix
// cores (C operand): sum_j sc_j (q . y)_j = 8 P1 + P0, the same integers ggml-cpu computes, with no per-sub-block fold at all.
template <int QT> __device__ __forceinline__ void sk_unit_k45(const char * __restrict__ arow, const char * __restrict__ btok, const float * __restrict__ dAs, const int g, float (&acc)[16]) {
    constexpr int NP = QT == 4 ? 2 : 3;              // digit planes
    constexpr uint32_t DM = QT == 4 ? 0x07070707u : 0x03030303u;
    constexpr int DS = QT == 4 ? 3 : 2;              // bits per digit
    const int16s zeroi = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float16s zerof = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint4 hdr = *(const uint4 *) arow;
    const float d = h2f((uint16_t) (hdr.x & 0xFFFF)), dmin = h2f((uint16_t) (hdr.x >> 16));
    // the 12 packed bytes: scales 0..3 / 4..7 and mins 0..3 / 4..7 as one byte each
    const uint32_t slo = hdr.y & 0x3F3F3F3Fu, shi = (hdr.w & 0x0F0F0F0Fu) | ((hdr.y >> 2) & 0x30303030u);
    const uint32_t mlo = hdr.z & 0x3F3F3F3Fu, mhi = ((hdr.w >> 4) & 0x0F0F0F0Fu) | ((hdr.z >> 2) & 0x30303030u);
    // mins: sum_j m_j * (sum of the 32 activations of sub-block j) = sum over the sixteen 16-value bsums with m_{k/2}; this lane's k-group
    // covers bsums 8g .. 8g+7, i.e. mins 4g .. 4g+3, each twice: 0x6400 | n == 1024 + n in f16, minus 1024
    float16s ms;
    {
        typedef _Float16 half2s __attribute__((ext_vector_type(2)));
        const uint32_t msrc = g ? mhi : mlo;
        const half2s k1024 = {(_Float16) 1024.0f, (_Float16) 1024.0f};
        uint4 mfu;
        mfu.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2s, sk_rep_byte<0>(msrc) | 0x64006400u) - k1024);
        mfu.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2s, sk_rep_byte<1>(msrc) | 0x64006400u) - k1024);
        mfu.z = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2s, sk_rep_byte<2>(msrc) | 0x64006400u) - k1024);
        mfu.w = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2s, sk_rep_byte<3>(msrc) | 0x64006400u) - k1024);
        const half8s bsf = *(const half8s *) (btok + 256 + 16 * g);
        ms = __builtin_amdgcn_mfma_f32_32x32x16_f16(bsf, __builtin_bit_cast(half8s, mfu), zerof, 0, 0, 0);
    }
    // digit dwords: plane n of scales 0..3 / 4..7
    uint32_t dlo[NP], dhi[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        dlo[n] = (slo >> (DS * n)) & DM;
        dhi[n] = (shi >> (DS * n)) & DM;
    }
    uint4 qh = make_uint4(0, 0, 0, 0);
    if constexpr (QT == 5) qh = *(const uint4 *) (arow + 16 + 16 * g);
    int16s pl[NP];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint4 raw = *(const uint4 *) (arow + (QT == 5 ? 48 : 16) + 32 * p + 16 * g);
        uint32_t wlo[4] = {raw.x & 0x0F0F0F0Fu, raw.y & 0x0F0F0F0Fu, raw.z & 0x0F0F0F0Fu, raw.w & 0x0F0F0F0Fu};
        uint32_t whi[4] = {(raw.x >> 4) & 0x0F0F0F0Fu, (raw.y >> 4) & 0x0F0F0F0Fu, (raw.z >> 4) & 0x0F0F0F0Fu, (raw.w >> 4) & 0x0F0F0F0Fu};
        if constexpr (QT == 5) {
            const uint32_t h4[4] = {qh.x, qh.y, qh.z, qh.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wlo[k] |= ((h4[k] >> (2 * p)) & 0x01010101u) << 4;
                whi[k] |= ((h4[k] >> (2 * p + 1)) & 0x01010101u) << 4;
            }
        }
        const int4s y0 = *(const int4s *) (btok + 64 * p + 16 * g);
        const int4s y1 = *(const int4s *) (btok + 64 * p + 32 + 16 * g);
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            // sub-blocks 2p (low nibbles) and 2p + 1 (high nibbles): their digit n, replicated into both 16-bit lanes
            const uint32_t src = p < 2 ? dlo[n] : dhi[n];
            const uint32_t e0 = (p & 1) ? sk_rep_byte<2>(src) : sk_rep_byte<0>(src), e1 = (p & 1) ? sk_rep_byte<3>(src) : sk_rep_byte<1>(src);
            int4s a0, a1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[k] = (int) sk_pk_mul(wlo[k], e0);
                a1[k] = (int) sk_pk_mul(whi[k], e1);
            }
            pl[n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(y0, a0, p == 0 ? zeroi : pl[n], 0, 0, 0);
            pl[n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(y1, a1, pl[n], 0, 0, 0);
        }
    }
    // ---- fold the unit
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 dy = *(const float4 *) (dAs + 8 * q + 4 * g);
        const float dyv[4] = {dy.x, dy.y, dy.z, dy.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * q + r;
            int isum;
            if constexpr (QT == 4) isum = (pl[1][i] << 3) + pl[0][i];
            else isum = (pl[2][i] << 4) + (pl[1][i] << 2) + pl[0][i];
            const float v = __builtin_fmaf(-dmin, ms[i], d * (float) isum);
            acc[i] = __builtin_fmaf(dyv[r], v, acc[i]);
        }
    }
}

// The same unit of Q6_K: arow = this lane's row of the staged unit, the block's 210 bytes from its first (the fetch has undone the 0 / 2-byte shift); zeroi /
// zerof = the caller's sixteen zeros as int16s / float16s.  A straight-line MACRO, not a function: as a __forceinline__ function taking acc by
// reference, the very same text made the compiler give k_mmq_skinny's Q6_K instantiations a scratch frame (408 - 488 bytes per lane; none this way).
// (the fold stays on v_mad_i32_i24 here although it issues at ~6.8 clocks (scripts/ubench/valu_probe.hip): the fp32 form of it —
// cvt + fma, 2 clocks each — was built and made the compiler park the prefetched unit in scratch (156 bytes per lane))
#define SK_UNIT_Q6(arow, btok, dAs, g, acc, zeroi, zerof)                                                                                                                        \
    {                                                                                                                                                                \
        int16s isum = zeroi;                                                                                                                                         \
        float16s ms;                                                                                                                                                 \
        float d;                                                                                                                                                     \
        const uint4 scb = *(const uint4 *) (arow + 192);                                                                                                             \
        d = h2f(*(const uint16_t *) (arow + 208));                                                                                                                   \
        const uint32_t scw[4] = {scb.x, scb.y, scb.z, scb.w};                                                                                                        \
        int sc[16];                                                                                                                                                  \
        _Pragma("unroll") for (int s = 0; s < 16; ++s) sc[s] = (int) (int8_t) (scw[s >> 2] >> (8 * (s & 3)));                                                        \
        _Pragma("unroll") for (int h = 0; h < 2; ++h)                                                                                                                \
            _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                                                          \
                /* l = 16 t + 8 g .. + 7 of half h: ql[64h + l], ql[64h + 32 + l], qh[32h + l] carry the four sub-blocks 8h + 2k + t */                              \
                const uint2 qa = *(const uint2 *) (arow + 64 * h + 16 * t + 8 * g);                                                                                  \
                const uint2 qb = *(const uint2 *) (arow + 64 * h + 32 + 16 * t + 8 * g);                                                                             \
                const uint2 qc = *(const uint2 *) (arow + 128 + 32 * h + 16 * t + 8 * g);                                                                            \
                int2s v[4];                                                                                                                                          \
                v[0][0] = (int) ((qa.x & 0x0F0F0F0Fu) | ((qc.x << 4) & 0x30303030u));                                                                                \
                v[0][1] = (int) ((qa.y & 0x0F0F0F0Fu) | ((qc.y << 4) & 0x30303030u));                                                                                \
                v[1][0] = (int) ((qb.x & 0x0F0F0F0Fu) | ((qc.x << 2) & 0x30303030u));                                                                                \
                v[1][1] = (int) ((qb.y & 0x0F0F0F0Fu) | ((qc.y << 2) & 0x30303030u));                                                                                \
                v[2][0] = (int) (((qa.x >> 4) & 0x0F0F0F0Fu) | (qc.x & 0x30303030u));                                                                                \
                v[2][1] = (int) (((qa.y >> 4) & 0x0F0F0F0Fu) | (qc.y & 0x30303030u));                                                                                \
                v[3][0] = (int) (((qb.x >> 4) & 0x0F0F0F0Fu) | ((qc.x >> 2) & 0x30303030u));                                                                         \
                v[3][1] = (int) (((qb.y >> 4) & 0x0F0F0F0Fu) | ((qc.y >> 2) & 0x30303030u));                                                                         \
                _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                                                      \
                    const int s = 8 * h + 2 * k + t;                                                                                                                 \
                    const int2s y = *(const int2s *) (btok + 16 * s + 8 * g);                                                                                        \
                    const int16s tk = __builtin_amdgcn_mfma_i32_32x32x16_i8(__builtin_bit_cast(long, y), __builtin_bit_cast(long, v[k]), zeroi, 0, 0, 0);            \
                    _Pragma("unroll") for (int i = 0; i < 16; ++i) isum[i] += __mul24(tk[i], sc[s]);                                                                 \
                }                                                                                                                                                    \
            }                                                                                                                                                        \
        /* the codes are q + 32: subtract 32 * sum_s sc_s * bsum_s (one f16 MFMA, exact integers) */                                                                 \
        const half8s bsf = *(const half8s *) (btok + 256 + 16 * g);                                                                                                  \
        uint4 sfu;                                                                                                                                                   \
        sfu.x = g ? sk_pack_h2((float) sc[8], (float) sc[9]) : sk_pack_h2((float) sc[0], (float) sc[1]);                                                             \
        sfu.y = g ? sk_pack_h2((float) sc[10], (float) sc[11]) : sk_pack_h2((float) sc[2], (float) sc[3]);                                                           \
        sfu.z = g ? sk_pack_h2((float) sc[12], (float) sc[13]) : sk_pack_h2((float) sc[4], (float) sc[5]);                                                           \
        sfu.w = g ? sk_pack_h2((float) sc[14], (float) sc[15]) : sk_pack_h2((float) sc[6], (float) sc[7]);                                                           \
        ms = __builtin_amdgcn_mfma_f32_32x32x16_f16(bsf, __builtin_bit_cast(half8s, sfu), zerof, 0, 0, 0);                                                           \
        /* fold the unit: tokens of register i are (i & 3) + 8 (i >> 2) + 4 g */                                                                                     \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                                                              \
            const float4 dy = *(const float4 *) (dAs + 8 * q + 4 * g);                                                                                               \
            const float dyv[4] = {dy.x, dy.y, dy.z, dy.w};                                                                                                           \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                                          \
                const int i = 4 * q + r;                                                                                                                             \
                const float v = d * (float) (isum[i] - 32 * (int) ms[i]);                                                                                            \
                acc[i] = __builtin_fmaf(dyv[r], v, acc[i]);                                                                                                          \
            }                                                                                                                                                        \
        }                                                                                                                                                            \
    }

// CUs of the current device: the persistent grids of both files are one workgroup per CU
int skinny_n_cu();

}  // namespace mi355x
