// fattn_mla.hip — FLASH_ATTN_EXT at K 576 / V 512 over ONE shared KV head: the node llama.cpp's deepseek2 graph builds per layer with -fa (multi-head latent
// attention with the absorbed wk_b / wv_b: every query head reads the same compressed cache row, whose first or last 512 columns are also the value row).
//
// Same arithmetic as fattn_mma.hip (Q rounded to f16, s = (K·Q)*scale + mask, online softmax in the base-2 domain, P rounded to f16 for the second product, f32
// accumulation) and the same transposed layout on v_mfma_f32_32x32x16_f16: S^T = K·Q^T has the query in the accumulator COLUMN, so the running max, the running sum
// and the rescale factor are per-lane scalars, and the score registers of a lane are, as they stand, the B operand of O^T = V^T·P^T (V is transposed while staged).
//
// What is this file's own:
//   * a query ROW is a (token, head) pair, r = t * n_head + h: with one KV head every head multiplies the same K tile, so one decode token of a 128-head model
//     is already 128 rows — two workgroups of 64 rows (two 32-column blocks).  A lane takes its mask row from t = r / n_head; rows past n_q * n_head are dead
//     (loads clamped, nothing stored).  dst [512, n_head, n_q] is contiguous, so row r's output is simply the r-th run of 512 floats.
//   * the 576-wide contraction and the 512-wide output are split over the FOUR WAVES.  A lane cannot hold a query's 576 dims (144 registers per column block) and
//     its 512 outputs (256 registers per column block); wave w holds the fragments of head dims [144w, 144w + 144) — 9 k-steps, 36 registers per column block — and
//     computes a PARTIAL S^T over them; the four partial tiles meet in LDS (four slots, summed in wave order 0, 1, 2, 3: deterministic) and every wave runs the same
//     softmax step on the sum.  Wave w then accumulates O^T for its own output dims [128w, 128w + 128): 4 d-tiles x 2 column blocks x 16 = 128 accumulator
//     registers, kept in the AGPR half of the file.
//   * V may ALIAS K (a view into K's rows at element offset 0 or 64): the tile is fetched from HBM once, and the registers that fill the K tile also build V^T.
//     The separate-tensor form fetches v's own rows; both forms write the same V^T bytes and run the same instruction sequence on them, so they agree bit for bit.
//
// Decisions (profiles/fa_mla_resources.txt):
//   tile: 32 cells a trip.  LDS per workgroup: K [32][584] f16 = 37 376 B, V^T [512][36] f16 = 36 864 B, four score slots [2][16][64] f32 = 32 768 B: 107 008 B.
//     At 64 cells the three areas are 74 752 + 69 632 + 65 536 = 209 920 B, more than a CU has (160 KiB).
//   exchange: four slots, not LDS float adds — atomic adds land in arrival order and the sum would change from run to run.
//   one workgroup per CU (__launch_bounds__(256, 1)): 128 accumulators + 72 query registers + 32 scores + 48 .. 80 staging registers per lane need the whole
//     512-entry file of a SIMD, and two workgroups' LDS (214 016 B) would not fit either.
// Three barriers a tile (tile in LDS | partial scores in their slots | top of the next trip); the next tile's global loads are issued right behind the LDS stores of
// the current one and fly during both products.  Rows past n_kv are WRITTEN as zeros and never loaded, their scores are forced to -inf: any n_kv is served.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"

namespace mi355x {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

struct fmla_geom {
    int n_q, n_head, n_kv;
    int n_rows;    // n_q * n_head: the (token, head) rows of one batch entry
    int has_mask;
    int mask_al;   // every mask row starts 8-byte aligned: a full tile reads four mask values per load
    int n_splits;
    int voff;      // aliased form: v's first column inside the K row, in 16-byte chunks (0 or 8)
    float scale;
};

constexpr int MLA_DK = 576, MLA_DV = 512;
constexpr int MLA_BKV = 32;                  // cells per trip
constexpr int MLA_ROWS = 64;                 // query rows per workgroup
constexpr int MLA_KS = (MLA_DK + 8) * 2;     // K tile row stride (bytes): 73 x 16, an odd multiple -> conflict-free ds_read_b128
constexpr int MLA_VS = (MLA_BKV + 4) * 2;    // V^T tile row stride (bytes): 18 dwords -> 32 rows x ds_read_b64 cover the 64 banks once
constexpr int MLA_KCH = MLA_DK / 8;          // 16-byte chunks of a K row (72)
constexpr int MLA_SLOT = 2 * 16 * 64;        // floats of one wave's partial score tile
constexpr int MLA_REC = MLA_DV + 4;          // floats of a partial record: O[512], m (base-2 domain), l, two of padding (16-byte rows)
constexpr size_t MLA_LDS = (size_t) MLA_BKV * MLA_KS + (size_t) MLA_DV * MLA_VS + 4 * MLA_SLOT * sizeof(float);
static_assert((MLA_KS / 16) % 2 == 1, "conflict-free ds_read_b128");
static_assert(MLA_LDS == 107008, "the LDS map of the header comment");

template <bool ALIAS>
__global__ void __launch_bounds__(256, 1) k_fattn_mla(const tdesc q, const tdesc k, const tdesc v, const tdesc mask, const tdesc dst, const fmla_geom geo, float * __restrict__ ws) {
    constexpr int BKV = MLA_BKV, KS = MLA_KS, VS = MLA_VS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char * Kt = smem;                                            // [BKV][576 + 8] f16
    char * Vt = smem + BKV * KS;                                 // [512][BKV + 4] f16, transposed, groups of 4 cells XOR-swizzled by the row's 32-dim tile
    float * Sx = (float *) (smem + BKV * KS + MLA_DV * VS);      // [wave][column block][4 registers][lane][4] f32

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, kg = lane >> 5;
    const int split = blockIdx.y, bat = blockIdx.z;
    const int tiles = (geo.n_kv + BKV - 1) / BKV, tps = (tiles + geo.n_splits - 1) / geo.n_splits;
    const int kt_begin = min(tiles, split * tps), kt_end = min(tiles, kt_begin + tps);  // (a split past the end of the cache: an empty range)

    // this lane's two query rows (column fr of the two 32-column blocks), their fragments of this wave's 144 head dims, their mask rows
    int row[2];
    const uint16_t * mrow[2];
    half8 qf[2][9];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        row[c] = (int) blockIdx.x * MLA_ROWS + 32 * c + fr;
        const int rc = min(row[c], geo.n_rows - 1);
        const int t = rc / geo.n_head, h = rc - t * geo.n_head;
        const float * qp = (const float *) (q.data + (int64_t) t * q.nb[1] + (int64_t) h * q.nb[2] + (int64_t) bat * q.nb[3]) + 144 * wave + 8 * kg;
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const float4 a = *(const float4 *) (qp + 16 * s), b = *(const float4 *) (qp + 16 * s + 4);
            qf[c][s] = (half8){(_Float16) a.x, (_Float16) a.y, (_Float16) a.z, (_Float16) a.w, (_Float16) b.x, (_Float16) b.y, (_Float16) b.z, (_Float16) b.w};
        }
        mrow[c] = geo.has_mask ? (const uint16_t *) (mask.data + (int64_t) t * mask.nb[1] + (int64_t) (bat % mask.ne[3]) * mask.nb[3]) : nullptr;
    }
    const char * kbase = k.data + (int64_t) (bat / (q.ne[3] / k.ne[3])) * k.nb[3];
    [[maybe_unused]] const char * vbase = v.data + (int64_t) (bat / (q.ne[3] / v.ne[3])) * v.nb[3];

    constexpr float LOG2E = 1.4426950408889634f;
    const float sc2 = geo.scale * LOG2E;
    float16v O[2][4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[c][dt][r] = 0.0f;
    const float16v zero = O[0][0];
    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.0f, 0.0f};

    // staging.  A thread moves BLOCKS of 4 cells x 8 head dims (one 16-byte chunk of four consecutive rows): the unit that is transposed in registers (16 v_perm) and
    // written as 8 ds_write_b64 of V^T.  K: 8 groups of cells x 72 chunks = 576 blocks, two a thread and a third on wave 0; the separate V: 8 x 64 = 512, two a thread.
    const int nkb = wave == 0 ? 3 : 2;  // (wave-uniform)
    int kq[3], kc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int b = tid + 256 * j;
        kq[j] = b / MLA_KCH;
        kc[j] = b - MLA_KCH * kq[j];
    }
    u32x4v kr[3][4];
    [[maybe_unused]] u32x4v vr[ALIAS ? 1 : 2][4];
    auto load_tile = [&](const int kt) __attribute__((always_inline)) {
        const int kv0 = kt * BKV;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pos = kv0 + 4 * kq[j] + r;
                    kr[j][r] = (u32x4v){0u, 0u, 0u, 0u};  // a row past n_kv is zeros in LDS: never loaded (0 x NaN is NaN)
                    if (pos < geo.n_kv) kr[j][r] = *(const u32x4v *) (kbase + (int64_t) pos * k.nb[1] + kc[j] * 16);
                }
            }
        }
        if constexpr (!ALIAS) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int b = tid + 256 * j, vq = b >> 6, vc = b & 63;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pos = kv0 + 4 * vq + r;
                    vr[j][r] = (u32x4v){0u, 0u, 0u, 0u};
                    if (pos < geo.n_kv) vr[j][r] = *(const u32x4v *) (vbase + (int64_t) pos * v.nb[1] + vc * 16);
                }
            }
        }
    };
    // cells 4vq .. 4vq + 3 of value dims 8vc .. 8vc + 7 -> V^T.  (the group of 4 cells is XOR-swizzled by the row's 32-dim tile: the lanes that write one group —
    // rows 8 dims apart, 16 banks apart mod 64 — would meet in 4 bank pairs; the readers' tile index is wave-uniform)
    auto put_vt = [&](const u32x4v x0, const u32x4v x1, const u32x4v x2, const u32x4v x3, const int vq, const int vc) __attribute__((always_inline)) {
        const int kvs = 8 * (vq ^ ((vc >> 2) & 7));
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // dword e of a row holds dims 2e, 2e + 1
            uint2 lo, hi;
            lo.x = __builtin_amdgcn_perm(x1[e], x0[e], 0x05040100u);  // {row0.lo16, row1.lo16}
            lo.y = __builtin_amdgcn_perm(x3[e], x2[e], 0x05040100u);
            hi.x = __builtin_amdgcn_perm(x1[e], x0[e], 0x07060302u);  // {row0.hi16, row1.hi16}
            hi.y = __builtin_amdgcn_perm(x3[e], x2[e], 0x07060302u);
            *(uint2 *) (Vt + (8 * vc + 2 * e) * VS + kvs) = lo;
            *(uint2 *) (Vt + (8 * vc + 2 * e + 1) * VS + kvs) = hi;
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) *(u32x4v *) (Kt + (4 * kq[j] + r) * KS + kc[j] * 16) = kr[j][r];
                if constexpr (ALIAS) {  // the same registers are the value rows where the chunk lies inside v's 512 columns
                    const int vc = kc[j] - geo.voff;
                    if (vc >= 0 && vc < MLA_DV / 8) put_vt(kr[j][0], kr[j][1], kr[j][2], kr[j][3], kq[j], vc);
                }
            }
        }
        if constexpr (!ALIAS) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int b = tid + 256 * j;
                put_vt(vr[j][0], vr[j][1], vr[j][2], vr[j][3], b >> 6, b & 63);
            }
        }
    };

    if (kt_begin < kt_end) load_tile(kt_begin);
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int kv0 = kt * BKV;
        const bool tail = kv0 + BKV > geo.n_kv;
        // the accumulators live in the AGPR half of the register file (fattn_mma.hip, head size 256: said once per tile, or the allocator carries them through VGPRs)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) asm volatile("" : "+a"(O[c][dt]));
        __syncthreads();  // nobody reads the previous tile or its score slots any more
        store_tile();
        // the mask values of this tile, requested BEFORE the next tile's K / V: vmcnt retires in order, so waiting for them leaves the younger requests in flight.
        // word [c][g4]: cells kv0 + 8 g4 + 4 kg .. + 3 of column block c's query (registers 4 g4 .. 4 g4 + 3 of the score tile)
        uint2 mw[2][4] = {};
        if (geo.has_mask) {
            if (geo.mask_al && !tail) {  // (block-uniform)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) mw[c][g4] = *(const uint2 *) (mrow[c] + kv0 + 8 * g4 + 4 * kg);
            } else {  // any row alignment, any n_kv: one value a load, none past the row's end
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const int p0 = kv0 + 8 * g4 + 4 * kg;
                        uint32_t w[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = p0 + e < geo.n_kv ? (uint32_t) mrow[c][p0 + e] : 0u;
                        mw[c][g4] = make_uint2(w[0] | (w[1] << 16), w[2] | (w[3] << 16));
                    }
            }
        }
        if (kt + 1 < kt_end) load_tile(kt + 1);
        // (a bare barrier behind the LDS writes: __syncthreads() would also wait vmcnt(0), i.e. for the loads just issued)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

        // ---- this wave's partial S^T = K[:, 144w .. 144w + 143] · Q^T[144w .. 144w + 143, :], both column blocks from one read of K
        float16v S[2] = {zero, zero};
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const half8 a = *(const half8 *) (Kt + fr * KS + (144 * wave + 16 * s + 8 * kg) * 2);
            S[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[0][s], S[0], 0, 0, 0);
            S[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[1][s], S[1], 0, 0, 0);
        }
        // ---- the four partial tiles meet in LDS: every lane writes and reads the same places (16 bytes a lane: no conflicts), summed in wave order
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(float4 *) (Sx + wave * MLA_SLOT + ((c * 4 + g4) * 64 + lane) * 4) = make_float4(S[c][4 * g4], S[c][4 * g4 + 1], S[c][4 * g4 + 2], S[c][4 * g4 + 3]);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float * sp = Sx + ((c * 4 + g4) * 64 + lane) * 4;
                const float4 a0 = *(const float4 *) sp, a1 = *(const float4 *) (sp + MLA_SLOT), a2 = *(const float4 *) (sp + 2 * MLA_SLOT), a3 = *(const float4 *) (sp + 3 * MLA_SLOT);
                S[c][4 * g4] = ((a0.x + a1.x) + a2.x) + a3.x;
                S[c][4 * g4 + 1] = ((a0.y + a1.y) + a2.y) + a3.y;
                S[c][4 * g4 + 2] = ((a0.z + a1.z) + a2.z) + a3.z;
                S[c][4 * g4 + 3] = ((a0.w + a1.w) + a2.w) + a3.w;
            }
        // ---- scale, mask, online softmax: a lane is two queries (one per column block), its registers 16 of the tile's 32 cells
        float mx[2] = {-INFINITY, -INFINITY};
        if (geo.has_mask || tail) {  // (block-uniform)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int p0 = kv0 + 8 * g4 + 4 * kg;
                    const float mv[4] = {h2f((uint16_t) (mw[c][g4].x & 0xFFFF)), h2f((uint16_t) (mw[c][g4].x >> 16)), h2f((uint16_t) (mw[c][g4].y & 0xFFFF)), h2f((uint16_t) (mw[c][g4].y >> 16))};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float sv = fmaf(S[c][4 * g4 + e], sc2, mv[e] * LOG2E);  // base-2 domain: p = 2^(s - m) is one v_exp_f32
                        if (p0 + e >= geo.n_kv) sv = -INFINITY;
                        S[c][4 * g4 + e] = sv;
                        mx[c] = fmaxf(mx[c], sv);
                    }
                }
        } else {  // no mask, every cell inside the cache: one multiply per score (= fmaf(s, sc2, +0.0))
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = S[c][r] * sc2;
                    S[c][r] = sv;
                    mx[c] = fmaxf(mx[c], sv);
                }
        }
        float alpha[2];
        bool any = false;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], 32, 64));
            const float m_new = fmaxf(m[c], mx[c]);
            any = any || m_new != -INFINITY;
            const float mref = m_new == -INFINITY ? 0.0f : m_new;  // this query sees nothing yet: every exponent below is -inf -> 0
            alpha[c] = __builtin_amdgcn_exp2f(m[c] - mref);
            float rs = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(S[c][r] - mref);
                S[c][r] = p;
                rs += p;
            }
            rs += __shfl_xor(rs, 32, 64);
            l[c] = l[c] * alpha[c] + rs;
            m[c] = m_new;
        }
        if (!__any(any)) continue;  // nothing visible to any of the 64 rows so far (every wave decides alike; the barriers are at the loop top)
        if (!__all(alpha[0] == 1.0f && alpha[1] == 1.0f)) {  // (wave-uniform) one d-tile at a time through VGPRs and back
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    asm volatile("" : "+a"(O[c][dt]));
                    float16v o = O[c][dt];
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[r] *= alpha[c];
                    asm volatile("" : "+a"(o));
                    O[c][dt] = o;
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        // ---- O^T[128w .. 128w + 127, :] += V^T·P^T: a lane's registers 8 s2 .. 8 s2 + 7 are cells {16 s2 + 4 kg .. + 3, 16 s2 + 8 + 4 kg .. + 3}; the contraction index is
        // only a label, so the A operand reads V^T in that order (two 8-byte runs of the row of its output dim); one read of V^T serves both column blocks
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            half8 pb[2];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int u = 0; u < 8; ++u) pb[c][u] = (_Float16) S[c][8 * s2 + u];
            const int kvg = 4 * s2 + kg;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const char * vrow = Vt + (128 * wave + 32 * dt + fr) * VS;
                const int x = (4 * wave + dt) & 7;
                const half4v a0 = *(const half4v *) (vrow + 8 * (kvg ^ x)), a1 = *(const half4v *) (vrow + 8 * ((kvg + 2) ^ x));
                const half8 a = (half8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                O[0][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pb[0], O[0][dt], 0, 0, 0);
                O[1][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pb[1], O[1][dt], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (row[c] >= geo.n_rows) continue;  // a dead row: it multiplied a clamped duplicate
        if (geo.n_splits == 1) {
            const float inv = 1.0f / l[c];
            float * out = (float *) (dst.data + (int64_t) bat * dst.nb[3]) + (int64_t) row[c] * MLA_DV + 128 * wave;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(float4 *) (out + 32 * dt + 8 * g4 + 4 * kg) = make_float4(O[c][dt][4 * g4] * inv, O[c][dt][4 * g4 + 1] * inv, O[c][dt][4 * g4 + 2] * inv, O[c][dt][4 * g4 + 3] * inv);
        } else {  // partial record (O relative to m; m; l) for k_fattn_mla_combine.  An empty or wholly masked range leaves m = -inf, l = 0, O = 0
            float * rec = ws + (((int64_t) bat * geo.n_rows + row[c]) * geo.n_splits + split) * MLA_REC;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(float4 *) (rec + 128 * wave + 32 * dt + 8 * g4 + 4 * kg) = make_float4(O[c][dt][4 * g4], O[c][dt][4 * g4 + 1], O[c][dt][4 * g4 + 2], O[c][dt][4 * g4 + 3]);
            if (wave == 0 && kg == 0) {
                rec[MLA_DV] = m[c];
                rec[MLA_DV + 1] = l[c];
            }
        }
    }
}

// merges the n_splits partial records of a (token, head) row: a workgroup per row, a thread per four output dims.  A record with m = -inf (an empty or wholly
// masked range, whose O is zeros) gets the weight 0; a row nobody saw anything of divides 0 by 0, as the one-split kernel does.  The weights are worked out once, by
// one lane per split, and left in LDS: the walk over the records then has no load that waits for another (a first form read m, branched and only then asked for O —
// 64 round trips in a row).
__global__ void __launch_bounds__(128) k_fattn_mla_combine(const float * __restrict__ ws, const tdesc dst, const int n_rows, const int n_splits) {
    __shared__ float wgt[64], Ls;
    const int row = blockIdx.x, bat = blockIdx.y, tid = threadIdx.x, d0 = 4 * tid;
    const float * rec = ws + ((int64_t) bat * n_rows + row) * n_splits * MLA_REC;
    if (tid < 64) {  // (n_splits <= 64: the launcher)
        const bool live = tid < n_splits;
        const float ms = live ? rec[(int64_t) tid * MLA_REC + MLA_DV] : -INFINITY, ls = live ? rec[(int64_t) tid * MLA_REC + MLA_DV + 1] : 0.0f;
        const float M = wave_max(ms);
        const float w = ms == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(ms - M);
        wgt[tid] = w;
        const float L = wave_sum(w * ls);  // (a fixed order of additions)
        if (tid == 0) Ls = L;
    }
    __syncthreads();
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
    for (int s = 0; s < n_splits; ++s) {
        const float w = wgt[s];
        const float4 o = *(const float4 *) (rec + (int64_t) s * MLA_REC + d0);
        acc.x += w * o.x;
        acc.y += w * o.y;
        acc.z += w * o.z;
        acc.w += w * o.w;
    }
    const float inv = 1.0f / Ls;
    *(float4 *) ((float *) (dst.data + (int64_t) bat * dst.nb[3]) + (int64_t) row * MLA_DV + d0) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
}

// ------------------------------------------------------------------------------------------------ host side
// KV splits: row blocks x batch entries rarely fill the chip on their own (one decode token of 128 heads is two workgroups), so the cell range is split until 256
// workgroups exist — at least two trips (64 cells) a split, so that a split's query fragments and its record are paid for by some cells; 64 at the most.
int fattn_mla_pick_splits(const tdesc & q, const tdesc & k) {
    const int64_t wgs = ((q.ne[1] * q.ne[2] + MLA_ROWS - 1) / MLA_ROWS) * q.ne[3];
    const int64_t tiles = (k.ne[1] + MLA_BKV - 1) / MLA_BKV;
    const int64_t want = (256 + wgs - 1) / wgs;
    return (int) std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(64, tiles / 2)));
}
size_t fattn_mla_ws_bytes(const tdesc & q, int n_splits) {
    return n_splits > 1 ? (size_t) q.ne[1] * (size_t) q.ne[2] * (size_t) q.ne[3] * (size_t) n_splits * MLA_REC * sizeof(float) : 0;
}
// v is a view into k's rows (graph.cpp: fa_mla_ok has checked shapes, types and strides): the same row stride, the same batch stride, 0 or 64 elements into the row
static bool fattn_mla_aliased(const tdesc & k, const tdesc & v, int * off_chunks) {
    const int64_t d = v.data - k.data;
    if (v.nb[1] != k.nb[1] || v.nb[3] != k.nb[3] || v.ne[3] != k.ne[3] || (d != 0 && d != 128)) return false;
    *off_chunks = (int) (d / 16);
    return true;
}
// -> the number of launches (1, or 2 with the combine pass)
int launch_flash_attn_mla(hipStream_t s, const tdesc & q, const tdesc & k, const tdesc & v, const tdesc * mask, const tdesc & dst, float scale, int n_splits, void * workspace) {
    if (k.ne[0] != MLA_DK || v.ne[0] != MLA_DV || k.ne[2] != 1 || v.ne[2] != 1 || ((uintptr_t) q.data & 15) || ((uintptr_t) k.data & 15) || ((uintptr_t) v.data & 15) || ((uintptr_t) dst.data & 15) ||
        n_splits < 1 || n_splits > 64 || (n_splits > 1 && (workspace == nullptr || ((uintptr_t) workspace & 15)))) {
        MI_ERR("launch_flash_attn_mla: a node fa_mla_ok does not describe (K %lld / V %lld, %lld KV heads, %d splits) or operands off their 16-byte alignment", (long long) k.ne[0],
               (long long) v.ne[0], (long long) k.ne[2], n_splits);
        abort();
    }
    fmla_geom geo{};
    geo.n_q = (int) q.ne[1];
    geo.n_head = (int) q.ne[2];
    geo.n_kv = (int) k.ne[1];
    geo.n_rows = geo.n_q * geo.n_head;
    geo.has_mask = mask ? 1 : 0;
    geo.mask_al = mask && !(mask->nb[1] % 8) && !(mask->nb[3] % 8) && !((uintptr_t) mask->data & 7) ? 1 : 0;
    geo.n_splits = n_splits;
    geo.scale = scale;
    const bool aliased = fattn_mla_aliased(k, v, &geo.voff);
    const tdesc mk = mask ? *mask : q;
    const dim3 grid((unsigned) ((geo.n_rows + MLA_ROWS - 1) / MLA_ROWS), (unsigned) n_splits, (unsigned) q.ne[3]);
    // 107 008 bytes of dynamic LDS: above the 64 KB default, raised once per (form, device)
    static std::atomic<uint32_t> raised[2] = {{0}, {0}};
    if (aliased) {
        (void) ensure_dyn_lds((const void *) k_fattn_mla<true>, MLA_LDS, raised[0]);  // (on failure the launch fails and graph_compute reports it)
        hipLaunchKernelGGL(k_fattn_mla<true>, grid, dim3(256), MLA_LDS, s, q, k, v, mk, dst, geo, (float *) workspace);
    } else {
        (void) ensure_dyn_lds((const void *) k_fattn_mla<false>, MLA_LDS, raised[1]);
        hipLaunchKernelGGL(k_fattn_mla<false>, grid, dim3(256), MLA_LDS, s, q, k, v, mk, dst, geo, (float *) workspace);
    }
    g_fa_form = fa_form_code(FA_FORM_K_MLA, aliased ? 1 : 0, 4, FA_FORM_KV_F16, 64, n_splits > 1 ? FA_FORM_TAIL_COMBINE : FA_FORM_TAIL_NONE);
    if (n_splits == 1) return 1;
    hipLaunchKernelGGL(k_fattn_mla_combine, dim3((unsigned) geo.n_rows, (unsigned) q.ne[3]), dim3(128), 0, s, (const float *) workspace, dst, geo.n_rows, n_splits);
    return 2;
}

MI_TU_TOUCH(fattn_mla)

}  // namespace mi355x
