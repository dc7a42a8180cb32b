// mmid_group.hip — MUL_MAT_ID for batches: the (slot, token) pairs grouped by expert ON THE DEVICE, and each group's pairs multiplied as the columns of
// the integer matrix-core unit of mmq_unit.h (K-quant experts: Q4_K / Q5_K / Q6_K).  MXFP4 experts share the grouping kernel and the scratch layout; their
// product kernel is mmid_group_mxfp4.hip's.
//
// mmid.hip serves a batch as n_used * n_tokens independent mat-vecs: every pair streams its whole expert matrix and does one column of v_dot4 arithmetic per
// weight byte.  Here a weight byte read from memory meets up to 32 columns:
//
//   k_mmid_group   (one workgroup, geometry from shapes only) reads the ids through their token stride, counts the pairs of every expert in an LDS histogram,
//                  scans it, and writes into the node's scratch
//                    perm[P]      the pair indices tok * n_used + slot ordered by expert (the order inside a group is whatever the LDS atomics gave: no
//                                 result depends on it),
//                    tiles[]      one record per 32-column tile: {expert, first index in perm, live columns 1..32}; an expert with c pairs gets
//                                 ceil(c / 32) tiles, so there are at most floor(P / 32) + min(n_expert + 1, P) of them,
//                    n_tiles.
//                  Pairs whose id is outside [0, n_expert) form one pseudo-group (expert -1): its tiles store zeros and read nothing of `as`.
//   k_mmid_grouped<QT>  a persistent grid, one workgroup of eight waves per CU, walks the items (tile, 32-row panel) with a stride of the grid; items at or
//                  beyond n_tiles * N / 32 end the walk, so the grid never depends on the ids.  An item is k_mmq_skinny's item with two changes: the weight
//                  rows start at W + expert * w_nb2, and the activation fetch is a GATHER — column j of the tile is the Q8_K row of pair perm[first + j],
//                  row tok * b_rows + (b_rows == 1 ? 0 : slot) of the activation area.  The rows of an item are read from perm once (lanes 0..31 one
//                  column each, handed to the fetch roles by ds_bpermute), ahead of the item's first loads.  Columns at or beyond the live count fetch the
//                  last live column's row and are never stored.  Wave w takes super-blocks w, w + 8, ..; the eight partial 32 x 32 results meet in LDS
//                  and are summed in wave order; the next item's first weight loads fly meanwhile.  Store: column j goes to dst + tok * dst_nb2 + slot * dst_nb1,
//                  32 consecutive lanes writing 32 consecutive rows; ADD_ID's bias (mmid_args::bias) is one f32 add there.
//
// A pair's result depends on its expert's weights and its own activation row alone: a column of the MFMA is a function of its own A row, the K split is by
// wave index whatever the tile holds, and waves without a super-block add +0.0f — not on the column it landed in, on its neighbours, or on the tile count.
#include <algorithm>

#include "dev_util.h"
#include "kernels.h"
#include "mmq_unit.h"
#include "mmvq_types.h"

namespace mi355x {

// scratch of one node: [16 ints: n_tiles, ..][tile records, 16 bytes each][perm] (kernels.h: mmid_group_scratch)
constexpr size_t GR_HDR_BYTES = MI_MMID_GROUP_HDR_BYTES;
int64_t mmid_group_max_tiles(int64_t n_pairs, int64_t n_expert) { return n_pairs / 32 + std::min(n_expert + 1, n_pairs); }
size_t mmid_group_scratch_bytes(int64_t n_pairs, int64_t n_expert) {
    return GR_HDR_BYTES + (size_t) mmid_group_max_tiles(n_pairs, n_expert) * sizeof(int4) + (((size_t) n_pairs + 3) & ~(size_t) 3) * sizeof(int32_t);
}

// ------------------------------------------------------------------------------------------------ grouping
constexpr int GR_NT = 1024;         // threads; thread t owns groups 2t and 2t + 1 in the scan
constexpr int GR_MAXG = 2 * GR_NT;  // >= n_expert + 1 (launcher: n_expert <= MI_MMID_GROUP_MAX_EXPERT)

__global__ void __launch_bounds__(GR_NT) k_mmid_group(const char * __restrict__ ids, const int64_t ids_nb1, const int n_used, const int n_pairs, const int n_expert,
                                                      int * __restrict__ hdr, int4 * __restrict__ tiles, int * __restrict__ perm) {
    __shared__ int cnt[GR_MAXG];  // pairs per group, then each group's cursor into perm
    __shared__ uint32_t wsum[GR_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cnt[tid] = 0;
    cnt[tid + GR_NT] = 0;
    __syncthreads();
    auto group_of = [&](const int p) {
        const int tok = p / n_used, slot = p - tok * n_used;
        const int id = *(const int32_t *) (ids + (size_t) tok * ids_nb1 + (size_t) slot * 4);
        return (unsigned) id < (unsigned) n_expert ? id : n_expert;  // outside the experts: the pseudo-group
    };
    for (int p = tid; p < n_pairs; p += GR_NT) atomicAdd(&cnt[group_of(p)], 1);
    __syncthreads();
    // exclusive scan over the groups of (tiles << 16 | pairs): pairs add up to n_pairs <= 65535, so no carry reaches the tile field
    const int c0 = cnt[2 * tid], c1 = cnt[2 * tid + 1];
    const uint32_t k0 = (uint32_t) c0 | ((uint32_t) ((c0 + 31) >> 5) << 16), k1 = (uint32_t) c1 | ((uint32_t) ((c1 + 31) >> 5) << 16);
    uint32_t incl = k0 + k1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t) __shfl_up((int) incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < GR_NT / 64; ++w) {
        const uint32_t v = wsum[w];
        if (w < wave) base += v;
        total += v;
    }
    const uint32_t ex0 = base + incl - k0 - k1, ex1 = ex0 + k0;
    cnt[2 * tid] = (int) (ex0 & 0xFFFFu);  // (this thread's own two entries: nobody else reads them before the barrier below)
    cnt[2 * tid + 1] = (int) (ex1 & 0xFFFFu);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ge = 2 * tid + h, c = h ? c1 : c0;
        const uint32_t ex = h ? ex1 : ex0;
        const int t0 = (int) (ex >> 16), p0 = (int) (ex & 0xFFFFu);
        for (int k = 0; 32 * k < c; ++k) tiles[t0 + k] = make_int4(ge < n_expert ? ge : -1, p0 + 32 * k, min(32, c - 32 * k), 0);
    }
    if (tid == 0) hdr[0] = (int) (total >> 16);
    __syncthreads();
    for (int p = tid; p < n_pairs; p += GR_NT) perm[atomicAdd(&cnt[group_of(p)], 1)] = p;
}

// ------------------------------------------------------------------------------------------------ product
template <int QT>
__global__ void __launch_bounds__(SK_NW * 64, 1) k_mmid_grouped(const mmid_args a, const int * __restrict__ hdr, const int4 * __restrict__ tiles, const int * __restrict__ perm,
                                                                const int max_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef sk_fmt<QT> F;
    // PF: the next unit's weight pieces are requested a whole unit ahead and wait in registers across the multiply (Q4_K).  Q5_K (a third digit plane) and Q6_K
    // (sixteen scales and the v_mad fold) have no room for that: with it the compiler parked the prefetched unit in a scratch frame (124 / 356 bytes per lane).
    // Their weights are requested at the top of their own unit, with the activations; the second wave of the SIMD covers part of the wait
    constexpr bool PF = QT == 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, g = lane >> 5;
    const int nblk = a.K / 256, npan = a.N / 32;
    const int n_items = min(hdr[0], max_tiles) * npan;  // item = tile * npan + panel: the workgroups of one moment share a tile's activations in L2
    const int w_nb1 = (int) a.w_nb1;

    char * const As = smem + wave * sk_wave_lds<QT>();
    char * const Bs = As + 32 * F::ROW;
    float * const dAs = (float *) (Bs + SK_B_BYTES);

    // ---- fetch roles of the weight unit: k_mmq_skinny's (mmq_skinny.hip says how the pieces are dealt)
    constexpr int HEAD = QT == 6 ? 0 : F::PIECES - 8;
    constexpr int NLT = QT == 6 ? 8 : 4;
    constexpr int NLH = (32 * HEAD + 63) / 64;
    constexpr int NLA = NLT + NLH;
    const int at_off = QT == 6 ? (lane >> 4) * w_nb1 + (lane & 15) * 16 : (lane >> 3) * w_nb1 + (HEAD + (lane & 7)) * 16;
    const int at_lds = QT == 6 ? (lane >> 4) * F::ROW + (lane & 15) * 16 : (lane >> 3) * F::ROW + (HEAD + (lane & 7)) * 16;
    const int at_step = (QT == 6 ? 4 : 8) * w_nb1;
    constexpr int at_lstep = (QT == 6 ? 4 : 8) * F::ROW;
    int ah_off[NLH > 0 ? NLH : 1], ah_lds[NLH > 0 ? NLH : 1];
#pragma unroll
    for (int u = 0; u < NLH; ++u) {
        const int pi = min(lane + 64 * u, 32 * HEAD - 1);
        const int r = pi / (HEAD > 0 ? HEAD : 1), pc = pi - r * HEAD;
        ah_off[u] = r * w_nb1 + pc * 16;
        ah_lds[u] = r * F::ROW + pc * 16;
    }
    const bool ah_last_live = ((32 * HEAD) % 64) == 0 || lane < ((32 * HEAD) % 64);
    // ---- fetch roles of the activation unit: qs u = 0..7, column (lane >> 4) + 4 u, piece lane & 15; bsums: column lane >> 1, piece 16 + (lane & 1); scale: column
    // `row`.  The column's row in the activation area is the item's business (br_*, below)
    const char * const act_base = (const char *) a.act;
    const uint32_t tok_bytes = (uint32_t) nblk * (uint32_t) sizeof(q8k_dev);  // (rows x tok_bytes < 2^31: mmid_grouped_supported — a uniform base + 32-bit lane offsets)
    const uint32_t bq_pc = (lane & 15) * 16; const int bq_lds = (lane >> 4) * SK_BTOK + (lane & 15) * 16;
    const uint32_t bs_pc = 256 + (lane & 1) * 16; const int bs_lds = (lane >> 1) * SK_BTOK + 256 + (lane & 1) * 16;

    u32x4s ga[NLA], gb[9] = {};
    float gd = 0.0f;
    // the item whose loads are in flight: its weight rows, live columns and the activation rows of this lane's fetch roles
    int nx_item = blockIdx.x, nx_sb = wave, nx_expert = -1, nx_cnt = 0;
    const uint8_t * nx_rows = a.W;
    int br = 0;  // lane l: the activation row of column l & 31 of that item (the fetch roles take theirs by ds_bpermute when they issue: ten registers fewer)
    const int16s zeroi = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float16s zerof = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // (straight-line macros, not lambdas: register arrays captured by reference end up in scratch memory)
    // GR_ISSUE: the weight pieces of the unit (nx_item, sb), requested a whole unit ahead where PF (HBM / MALL); GR_ISSUE_B: its activation pieces, requested at the top of the
    // unit itself (L2 hits: the tile's rows are shared by every workgroup of the moment) while the weights are staged — a unit ahead as well, the compiler parked the
    // prefetched registers in a scratch frame (Q4_K: 24 bytes per lane; none this way)
#define GR_META(item)                                                                                                   \
    {                                                                                                                   \
        const int t_ = (item) / npan, pn_ = (item) - t_ * npan;                                                         \
        const int4 rec_ = tiles[t_];                                                                                    \
        nx_expert = rec_.x;                                                                                             \
        nx_cnt = rec_.z;                                                                                                \
        nx_rows = a.W + (size_t) max(rec_.x, 0) * (size_t) a.w_nb2 + (size_t) pn_ * 32 * (size_t) w_nb1;                \
        const int pr_ = perm[rec_.y + min(row, rec_.z - 1)]; /* column `row` of the tile; beyond the live count: the last live one */ \
        br = a.b_rows == 1 ? pr_ / a.n_used : pr_; /* tok * b_rows + slot is the pair index itself when b has a row per slot */ \
    }
#define GR_ISSUE(sb)                                                                                                    \
    {                                                                                                                   \
        const uint8_t * wb = nx_rows + (QT == 6 ? (size_t) (sb) * 210 - 2 * ((sb) & 1) : (size_t) (sb) * F::BYTES);     \
        _Pragma("unroll") for (int u = 0; u < NLT; ++u) ga[u] = *(const u32x4s *) (wb + at_off + u * at_step);          \
        _Pragma("unroll") for (int u = 0; u < NLH; ++u) ga[NLT + u] = *(const u32x4s *) (wb + ah_off[u]);               \
    }
#define GR_ISSUE_B(sb)                                                                                                  \
    {                                                                                                                   \
        const char * ab = act_base + (size_t) (sb) * sizeof(q8k_dev);                                                   \
        _Pragma("unroll") for (int u = 0; u < 8; ++u)                                                                   \
            if (4 * u < nx_cnt) gb[u] = *(const u32x4s *) (ab + ((uint32_t) __shfl(br, (lane >> 4) + 4 * u) * tok_bytes + bq_pc)); /* columns 4u .. 4u+3: skipped beyond the live count */ \
        gb[8] = *(const u32x4s *) (ab + ((uint32_t) __shfl(br, lane >> 1) * tok_bytes + bs_pc));                       \
        gd = *(const float *) (ab + ((uint32_t) br * tok_bytes + 304u)); /* q8k_dev::d */                               \
    }
    // to this wave's next unit: items of the pseudo-group have none
#define GR_NORMALISE()                                                                 \
    while (nx_item < n_items && (nx_sb >= nblk || nx_expert < 0)) {                    \
        nx_item += gridDim.x;                                                          \
        nx_sb = wave;                                                                  \
        if (nx_item < n_items) GR_META(nx_item)                                        \
    }
    if (wave >= nblk) nx_item = n_items;  // fewer super-blocks than waves: this wave has no unit in any item (it adds zeros in the reductions)
    if (nx_item < n_items) GR_META(nx_item)
    GR_NORMALISE()
    if constexpr (PF) { if (nx_item < n_items) GR_ISSUE(nx_sb) }

    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        // ---- the store roles of this item, requested ahead of its units: thread o = tid + 512 q sums column o >> 5, row o & 31
        const int tile = item / npan, pn = item - tile * npan;
        const int4 rec = tiles[tile];
        const int n = pn * 32 + (tid & 31);
        int pr[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) pr[q] = perm[rec.y + min((tid >> 5) + 16 * q, rec.z - 1)];
        auto dst_of = [&](const int p) {
            const int tok = p / a.n_used, slot = p - tok * a.n_used;
            return a.dst + (int64_t) tok * a.dst_nb2 + (int64_t) slot * a.dst_nb1 + n;
        };
        if (rec.x < 0) {  // (uniform over the workgroup) no expert: nothing of `as` was read, zeros
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if ((tid >> 5) + 16 * q < rec.z) *dst_of(pr[q]) = 0.0f;
            continue;
        }
        const float bv = a.bias ? ((const float *) (a.bias + (size_t) rec.x * a.bias_nb1))[n] : 0.0f;  // (ADD_ID in the store)

        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        while (nx_item == item) {
            if constexpr (!PF) GR_ISSUE(nx_sb)
            GR_ISSUE_B(nx_sb)
            // ---- registers -> the wave's LDS area
            if constexpr (QT == 6) {
                const int sh = 2 * (nx_sb & 1);  // the block starts `sh` bytes into the fetched window
#pragma unroll
                for (int u = 0; u < NLT; ++u) {
                    const uint32_t nx = (uint32_t) __shfl_down((int) ga[u].x, 1);  // first dword of the row's next piece
                    u32x4s o;
                    o.x = __builtin_amdgcn_alignbyte(ga[u].y, ga[u].x, sh);
                    o.y = __builtin_amdgcn_alignbyte(ga[u].z, ga[u].y, sh);
                    o.z = __builtin_amdgcn_alignbyte(ga[u].w, ga[u].z, sh);
                    o.w = __builtin_amdgcn_alignbyte(nx, ga[u].w, sh);
                    if ((lane & 15) < 14) *(u32x4s *) (As + at_lds + u * at_lstep) = o;  // 14 pieces cover the 210 bytes
                }
            } else {
#pragma unroll
                for (int u = 0; u < NLT; ++u) *(u32x4s *) (As + at_lds + u * at_lstep) = ga[u];
#pragma unroll
                for (int u = 0; u < NLH; ++u)
                    if (u + 1 < NLH || ah_last_live) *(u32x4s *) (As + ah_lds[u]) = ga[NLT + u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (4 * u < rec.z) *(u32x4s *) (Bs + bq_lds + u * 4 * SK_BTOK) = gb[u];
            *(u32x4s *) (Bs + bs_lds) = gb[8];
            if (g == 0) dAs[row] = gd;
            // ---- the next unit's loads (of this item or of the workgroup's next one) fly while this one is multiplied
            nx_sb += SK_NW;
            GR_NORMALISE()
            if constexpr (PF) { if (nx_item < n_items) GR_ISSUE(nx_sb) }

            const char * const arow = As + row * F::ROW;   // this lane's weight row (B operand: n = row)
            const char * const btok = Bs + row * SK_BTOK;  // this lane's column (A operand: m = column)
            if constexpr (QT == 6) SK_UNIT_Q6(arow, btok, dAs, g, acc, zeroi, zerof)
            else sk_unit_k45<QT>(arow, btok, dAs, g, acc);
        }

        // ---- the K slices meet in LDS: each wave leaves its 32 x 32 partial [column][row] at the start of its own area, then every thread sums two
        // outputs over the waves in wave order
        float * const own = (float *) As;
#pragma unroll
        for (int i = 0; i < 16; ++i) own[((i & 3) + 8 * (i >> 2) + 4 * g) * 32 + row] = acc[i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o = tid + q * SK_NW * 64;
            float v = *(const float *) (smem + o * 4);
#pragma unroll
            for (int w = 1; w < SK_NW; ++w) v += *(const float *) (smem + w * sk_wave_lds<QT>() + o * 4);
            if ((o >> 5) < rec.z) *dst_of(pr[q]) = a.bias ? v + bv : v;
        }
        __syncthreads();  // the areas are free for the next item's units
    }
#undef GR_META
#undef GR_ISSUE
#undef GR_ISSUE_B
#undef GR_NORMALISE
}

template <int QT> static bool launch_grouped_t(hipStream_t s, const mmid_args & a, const int * hdr, const int4 * tiles, const int * perm, int max_tiles) {
    static std::atomic<uint32_t> lds_raised{0};
    const size_t lds = (size_t) SK_NW * sk_wave_lds<QT>();
    if (!ensure_dyn_lds((const void *) k_mmid_grouped<QT>, lds, lds_raised)) return false;  // (MI_ERR is ensure_dyn_lds's)
    // one workgroup per CU (its LDS areas fill the CU); the worst-case item count only caps the grid of a small node
    const int64_t items = (int64_t) max_tiles * (a.N / 32);
    hipLaunchKernelGGL((k_mmid_grouped<QT>), dim3((unsigned) std::min<int64_t>(items, skinny_n_cu())), dim3(SK_NW * 64), lds, s, a, hdr, tiles, perm, max_tiles);
    return true;
}

// the operands the grouped form serves (graph.cpp's mmid_runs_grouped adds the pair threshold and the switch): K-quant experts of whole super-blocks and whole
// 32-row panels, rows packed back to back; Q6_K: every row of every expert dword-aligned, so that the 0 / 2-byte shift of a super-block is the same in all of them;
// MXFP4 experts (mmid_group_mxfp4.hip) of whole 32-value blocks and whole 32-row panels, rows packed back to back at any byte alignment
bool mmid_grouped_supported(const mmid_args & a) {
    const bool mx = a.type == GGML_TYPE_MXFP4;
    const int blk = mx ? 32 : 256;
    if (a.K < blk || (a.K % blk) != 0 || a.N < 32 || (a.N % 32) != 0 || a.n_expert < 1 || a.n_expert > MI_MMID_GROUP_MAX_EXPERT) return false;
    if (a.n_used < 1 || a.n_tokens < 1 || (int64_t) a.n_used * a.n_tokens >= 65536 || (a.b_rows != 1 && a.b_rows != a.n_used)) return false;
    const int64_t nblk = a.K / blk;
    if ((int64_t) a.n_tokens * a.b_rows * nblk * (int64_t) (mx ? sizeof(q80_dev) : sizeof(q8k_dev)) >= INT32_MAX) return false;  // (the gather's 32-bit lane offsets into the activation area)
    if (mmid_group_max_tiles((int64_t) a.n_used * a.n_tokens, a.n_expert) * (a.N / 32) >= INT32_MAX) return false;  // (the kernels count their items in an int)
    if (mx) return a.w_nb1 == nblk * 17;
    if (a.type == GGML_TYPE_Q4_K) return a.w_nb1 == nblk * 144;
    if (a.type == GGML_TYPE_Q5_K) return a.w_nb1 == nblk * 176;
    if (a.type == GGML_TYPE_Q6_K) return a.w_nb1 == nblk * 210 && (a.w_nb1 % 4) == 0 && (a.w_nb2 % 4) == 0 && ((uintptr_t) a.W % 4) == 0;
    return false;
}

bool launch_mmid_grouped(hipStream_t s, const mmid_args & a, void * scratch, size_t scratch_bytes) {
    const int64_t n_pairs = (int64_t) a.n_used * a.n_tokens;
    if (!mmid_grouped_supported(a) || a.act == nullptr) {
        MI_ERR("launch_mmid_grouped: operands the grouped form does not serve (type %d, K %d, N %d, %d experts, %d x %d pairs)", a.type, a.K, a.N, a.n_expert, a.n_used, a.n_tokens);
        return false;
    }
    if (scratch == nullptr || ((uintptr_t) scratch % 16) != 0 || scratch_bytes < mmid_group_scratch_bytes(n_pairs, a.n_expert)) {
        MI_ERR("launch_mmid_grouped: %zu bytes of scratch, %zu needed", scratch_bytes, mmid_group_scratch_bytes(n_pairs, a.n_expert));
        return false;
    }
    const mmid_group_scratch g = mmid_group_layout(scratch, n_pairs, a.n_expert);
    int * const hdr = g.hdr;
    int4 * const tiles = g.tiles;
    int * const perm = g.perm;
    const int max_tiles = g.max_tiles;
    hipLaunchKernelGGL(k_mmid_group, dim3(1), dim3(GR_NT), 0, s, a.ids, a.ids_nb1, a.n_used, (int) n_pairs, a.n_expert, hdr, tiles, perm);
    if (a.type == GGML_TYPE_MXFP4) {
        launch_mmid_grouped_mxfp4(s, a, g);
        return true;
    }
    if (a.type == GGML_TYPE_Q4_K) return launch_grouped_t<4>(s, a, hdr, tiles, perm, max_tiles);
    if (a.type == GGML_TYPE_Q5_K) return launch_grouped_t<5>(s, a, hdr, tiles, perm, max_tiles);
    return launch_grouped_t<6>(s, a, hdr, tiles, perm, max_tiles);
}

MI_TU_TOUCH(mmid_group)

}  // namespace mi355x
