// mmid_group_mxfp4.hip — the grouped form of MUL_MAT_ID for MXFP4 experts (gpt-oss prompt batches): k_mmid_group (mmid_group.hip) orders the pairs by expert and
// writes the tile table; k_mmid_grouped_mxfp4, here, multiplies every 32-column tile with its expert's rows on the integer matrix cores.
//
// Arithmetic: ggml-cpu's ggml_vec_dot_mxfp4_q8_0.  Per 32-value block an int32 sum of table value x int8 activation (exact), then one f32 term
// (d_x * scale) * sumi with scale = mxfp4_scale_bits(e).  A block IS the K extent of v_mfma_i32_32x32x32_i8: one MFMA onto a zero accumulator gives the
// 32 x 32 block sums of (32 columns) x (32 rows), and the f32 term is one multiply, one convert and one fma per output on the VALU.
//
// Data movement — nothing of the weights goes through LDS:
//   weights      lane (row = lane & 31, g = lane >> 5) of the B operand needs values 16 g .. 16 g + 15 of its row's block: the LOW (g = 0) or HIGH (g = 1) nibbles
//                of the block's 16 code bytes.  Both halves issue the same 1-byte-aligned 16-byte load (a 17-byte block starts at any address; one
//                global_load_dwordx4) and the e byte; a shift by 4 g, a mask and mxfp4_bytes (two byte permutes a dword) leave the register operand.  The
//                two halves of a wave read the same bytes in the same instruction: no second line is fetched, and what the duplicate costs is address
//                cycles of a kernel that waits on its VALU (below), so neither a cross-lane hand-over nor alternating blocks would buy time.
//   activations  lane (column = lane & 31, g) of the A operand loads bytes 16 g .. 16 g + 15 of q80_dev::qs of ITS pair's row — perm[first + column], row
//                tok * b_rows + (b_rows == 1 ? 0 : slot) — straight into the operand (a 36-byte block: dword-aligned), and the block's d.  The tile's rows
//                are shared by the workgroups of the moment and hit in L2.  Columns at or beyond the live count read the last live column's row
//                and are never stored.
//   column scales  a lane's sixteen outputs are columns (i & 3) + 8 (i >> 2) + 4 g, its own d is column lane & 31: the 32 d's cross the wave through 128 bytes
//                of wave-private LDS (one ds_write_b32, four ds_read_b128 a block; no barrier: one wave, in order).
//   K split      wave w of eight takes blocks w, w + 8, ..; K = 2880 is 90 blocks (two waves take twelve, six eleven), K = 32 one block (seven waves add
//                +0.0f).  The unit after the one being multiplied — the next block of the item, or the first block of the workgroup's NEXT item, whose tile
//                record and perm entry were requested at the top of this item — is in flight in ten registers while this one is multiplied.  The eight
//                partial 32 x 32 results meet in LDS ([column][row]) and are summed in wave order by 512 threads, two outputs each.
//   store        dst + tok * dst_nb2 + slot * dst_nb1 + row, 32 consecutive lanes 32 consecutive rows; ADD_ID's bias[expert][row] is one f32 add there.  Tiles
//                of the pseudo-group (ids outside the experts) store zeros and read nothing of `as`.
// The grid is one workgroup a CU walking the items (tile, 32-row panel) with its stride; items at or beyond n_tiles * N / 32 end the walk: neither grid nor
// control flow of the host depends on the ids, and the node replays inside a captured hipGraph.
//
// A pair's result depends on its expert's weights and its own activation row alone: a column of the MFMA is a function of its own A row, a wave's blocks are
// w, w + 8, .. whatever the tile holds, the waves are summed in wave order — not on the column it landed in, on its neighbours, or on the tile count.
//
// LDS 8 x (4096 + 128) = 33 792 bytes, static.  Registers, what bounds the kernel and the timings: DESIGN.md 4l, profiles/mmid_grouped_mxfp4_ubench.txt.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"
#include "mmq_unit.h"
#include "mmvq_types.h"

namespace mi355x {

constexpr int MX_NW = 8;                        // waves per workgroup: the K split
constexpr int MX_WAVE_LDS = 32 * 32 * 4 + 128;  // a wave's partial 32 x 32 result [column][row] and the 32 column scales of its block
struct __attribute__((packed, aligned(4))) u128_a4 { uint32_t x, y, z, w; };  // (half of q80_dev::qs: 36-byte blocks)

__global__ void __launch_bounds__(MX_NW * 64, 1) k_mmid_grouped_mxfp4(const mmid_args a, const int * __restrict__ hdr, const int4 * __restrict__ tiles, const int * __restrict__ perm,
                                                                      const int max_tiles) {
    __shared__ __attribute__((aligned(16))) char smem[MX_NW * MX_WAVE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, g = lane >> 5;  // (row: the weight row of the B operand and of the outputs; the column of the A operand)
    const int nblk = a.K / 32, npan = a.N / 32;
    const int n_items = min(hdr[0], max_tiles) * npan;  // item = tile * npan + panel: the workgroups of one moment share a tile's activations in L2
    const uint32_t tok_bytes = (uint32_t) nblk * (uint32_t) sizeof(q80_dev);  // (rows x tok_bytes < 2^31: mmid_grouped_supported — 32-bit lane offsets)
    const uint32_t sh = 4u * (uint32_t) g;
    float * const own = (float *) (smem + wave * MX_WAVE_LDS);
    float * const dxs = own + 32 * 32;
    const int16s zeroi = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    // the next item of this workgroup: its tile record, this lane's column of perm, and — once MX_ROWS ran — this lane's weight row and activation row
    int4 nrec = make_int4(-1, 0, 1, 0);
    int npr = 0;
    const uint8_t * nwrow = a.W;
    const char * nacol = (const char *) a.act;
    // the unit in flight: 16 code bytes and the e byte of (row, block), 16 activation bytes and d of (column, block)
    u128_a1 pw = {0, 0, 0, 0};
    u128_a4 pa = {0, 0, 0, 0};
    uint32_t pe = 0;
    float pd = 0.0f;
    // (straight-line macros, as in mmid_group.hip)
#define MX_META(item_)                                                                                                  \
    {                                                                                                                   \
        nrec = tiles[(item_) / npan];                                                                                   \
        npr = perm[nrec.y + min(row, nrec.z - 1)]; /* column `row` of the tile; beyond the live count: the last live one */ \
    }
#define MX_ROWS(item_)                                                                                                  \
    {                                                                                                                   \
        const int pn_ = (item_) - ((item_) / npan) * npan;                                                              \
        nwrow = a.W + (size_t) nrec.x * (size_t) a.w_nb2 + (size_t) (pn_ * 32 + row) * (size_t) a.w_nb1;                \
        const int br_ = a.b_rows == 1 ? npr / a.n_used : npr; /* tok * b_rows + slot is the pair index itself when b has a row per slot */ \
        nacol = (const char *) a.act + (uint32_t) br_ * tok_bytes;                                                      \
    }
#define MX_ISSUE(wrow_, acol_, b_)                                                                                      \
    {                                                                                                                   \
        const uint8_t * wb_ = (wrow_) + (size_t) (b_) * 17;                                                             \
        pe = wb_[0];                                                                                                    \
        pw = *(const u128_a1 *) (wb_ + 1);                                                                              \
        const char * ab_ = (acol_) + (uint32_t) (b_) * (uint32_t) sizeof(q80_dev);                                      \
        pa = *(const u128_a4 *) (ab_ + 16 * g);                                                                         \
        pd = *(const float *) (ab_ + 32); /* q80_dev::d */                                                              \
    }
    // the first unit of the workgroup's next item (waves without a block and items of the pseudo-group have none)
#define MX_FIRST_OF(item_)                                                                                              \
    if ((item_) < n_items && nrec.x >= 0 && wave < nblk) {                                                              \
        MX_ROWS(item_)                                                                                                  \
        MX_ISSUE(nwrow, nacol, wave)                                                                                    \
    }
    if ((int) blockIdx.x < n_items) MX_META((int) blockIdx.x)
    MX_FIRST_OF((int) blockIdx.x)

    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int4 rec = nrec;
        const int pr = npr;
        const uint8_t * const wrow = nwrow;
        const char * const acol = nacol;
        const int nitem = item + (int) gridDim.x;
        if (nitem < n_items) MX_META(nitem)  // (consumed by MX_FIRST_OF at the end of this item's blocks: a whole item ahead)
        // ---- the store roles: thread o = tid + 512 q sums column o >> 5 = 2 wave + g + 16 q, row o & 31
        const int n = (item - (item / npan) * npan) * 32 + row;
        float * dp[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = __shfl(pr, 2 * wave + g + 16 * q);
            const int tok = p / a.n_used, slot = p - tok * a.n_used;
            dp[q] = a.dst + (int64_t) tok * a.dst_nb2 + (int64_t) slot * a.dst_nb1 + n;
        }
        if (rec.x < 0) {  // (uniform over the workgroup) no expert: nothing of `as` is read, zeros
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (2 * wave + g + 16 * q < rec.z) *dp[q] = 0.0f;
            MX_FIRST_OF(nitem)
            continue;
        }
        const float bv = a.bias ? ((const float *) (a.bias + (size_t) rec.x * a.bias_nb1))[n] : 0.0f;  // (ADD_ID in the store)

        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int b = wave; b < nblk; b += MX_NW) {
            const uint32_t cq[4] = {pw.x, pw.y, pw.z, pw.w};
            const int4s av = {(int) pa.x, (int) pa.y, (int) pa.z, (int) pa.w};
            const float sc = __uint_as_float(mxfp4_scale_bits(pe));
            dxs[row] = pd;  // (both halves hold their column's d: the same value to the same word)
            if (b + MX_NW < nblk) MX_ISSUE(wrow, acol, b + MX_NW)
            else MX_FIRST_OF(nitem)
            int4s wv;
#pragma unroll
            for (int k = 0; k < 4; ++k) wv[k] = (int) mxfp4_bytes((cq[k] >> sh) & 0x0F0F0F0Fu);
            const int16s si = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, wv, zeroi, 0, 0, 0);  // register i: column (i & 3) + 8 (i >> 2) + 4 g, row `row`
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 dy = *(const float4 *) (dxs + 8 * q + 4 * g);
                const float dyv[4] = {dy.x, dy.y, dy.z, dy.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[4 * q + r] = __builtin_fmaf(dyv[r] * sc, (float) si[4 * q + r], acc[4 * q + r]);
            }
        }

        // ---- the K slices meet in LDS: each wave leaves its 32 x 32 partial [column][row], then every thread sums two outputs over the waves in wave order
#pragma unroll
        for (int i = 0; i < 16; ++i) own[((i & 3) + 8 * (i >> 2) + 4 * g) * 32 + row] = acc[i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o = tid + q * MX_NW * 64;
            float v = *(const float *) (smem + o * 4);
#pragma unroll
            for (int w = 1; w < MX_NW; ++w) v += *(const float *) (smem + w * MX_WAVE_LDS + o * 4);
            if ((o >> 5) < rec.z) *dp[q] = a.bias ? v + bv : v;
        }
        __syncthreads();  // the areas are free for the next item's partials
    }
#undef MX_META
#undef MX_ROWS
#undef MX_ISSUE
#undef MX_FIRST_OF
}

// (the operands were checked and the tile table written by launch_mmid_grouped, mmid_group.hip)
void launch_mmid_grouped_mxfp4(hipStream_t s, const mmid_args & a, const mmid_group_scratch & g) {
    // one workgroup per CU; the worst-case item count only caps the grid of a small node
    const int64_t items = (int64_t) g.max_tiles * (a.N / 32);
    hipLaunchKernelGGL(k_mmid_grouped_mxfp4, dim3((unsigned) std::min<int64_t>(items, skinny_n_cu())), dim3(MX_NW * 64), 0, s, a, g.hdr, g.tiles, g.perm, g.max_tiles);
}

MI_TU_TOUCH(mmid_group_mxfp4)

}  // namespace mi355x
