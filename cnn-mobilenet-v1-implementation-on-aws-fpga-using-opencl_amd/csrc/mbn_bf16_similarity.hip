// mbn_bf16_similarity.hip — nearest neighbours on a bf16 gallery for gfx950 (include/mbn.h, "Nearest neighbours"): the k best gallery rows per
// query under score = (queries . gallery^T) * q_scale * g_scale, the gallery stored in 16 bits and the fp32 queries split EXACTLY into three bf16
// planes h + m + l (mbn_x6.h), so the product runs on v_mfma_f32_32x32x16_bf16 and loses nothing of the queries. The epilogue is the running
// top-k of mbn_f32_similarity.hip: the [Q][G] product is never in memory. DESIGN.md 7f.
//
//   simb_split    the prologue: queries [Q][D] fp32 -> their split image [Q][3][D] bf16 (plane-major per row) behind the candidates in the workspace
//   simb_topk     the fused GEMM + top-k over work units (query tile, gallery chunk); writes k candidates per (chunk, query) to the workspace
//   sim_merge     one wave per query: the chunks' candidates -> topk_idx / topk_score (mbn_similarity_list.h, with the ranking and the lists)
//   rows_pack     mbn_embed_rows_bf16: one wave per row, fp32 or bf16 rows -> bf16 rows (RNE) and 1 / sqrt(sum of squares) of the ROUNDED row
//
// MFMA sides. v_mfma_f32_32x32x16_bf16 takes A [32 i][16 k] and B [16 k][32 j], lane l feeding A[i = l & 31][k = 8 (l >> 5) .. + 7] and
// B[k = 8 (l >> 5) .. + 7][j = l & 31] as eight bf16 of one 16-byte register group, and leaves D[i][j] with j = l & 31 and
// i = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15, in lane l. The GALLERY is the A side and the QUERIES the B side, as in the fp32 kernel: a lane
// owns ONE query and keeps its top-k as a sorted list in registers, one comparison per new score on the common path.
//
// The d order. A k-tile is 64 bf16: a 128-byte row, eight 16-byte chunks, chunk c = d / 8 % 8, in the byte geometry and swizzle (mbn_swz) of the
// fp32 kernel's tiles. One ds_read_b128 is one operand: at k step j = 0..3 of k-tile t lane half h reads chunk 2 j + h, which is
// d = 64 t + 16 j + 8 h .. + 7. Per k step, in ascending d, THREE instructions add to the one accumulator of a pair, the query planes in the order
// l, m, h (smallest terms first); an instruction adds its 16 exact products. Elements past D are zeros on the gallery side. The order is a
// function of D alone, the two scales multiply in a fixed order and the ranking is a total order: the output bytes are the same at every planning
// CU count and on every graph replay.
//
// Work split inside a workgroup (4 waves, a q_tile x 128 tile per stage). With the fp32 kernel's split (a wave owns 32 gallery rows and every
// query block) a k step costs 1 + 3 NQ ds_read_b128 for 3 NQ MFMAs of 8 passes: 7 reads of 8 LDS clocks in each of four waves, 224 clocks of
// the CU's one LDS pipe against 192 clocks of MFMA per SIMD: the LDS reads bind, and the B side is read four times. Here the waves split BOTH
// sides: q_tile = 64 is 2 x 2 waves, a wave owning ONE 32-query block and TWO 32-row gallery blocks (2 A + 3 B reads for 6 MFMAs: 160 LDS clocks
// against 192 of MFMA, two accumulator blocks); q_tile = 32 is 4 x 1 waves of one row block each (1 + 3 reads for 3 MFMAs), where the gallery's
// HBM bytes bind and not the loop. So a wave keeps one list per lane, the loop is bound by MFMA issue at q_tile = 64, and what feeds it is
// (128 + 3 q_tile) x 128 B per k-tile from L2: 40 KB per 96 MFMAs, about 53 B / clock / CU at full MFMA rate, which is near what an XCD's L2 gives
// a CU. A larger query tile would lower it and does not fit two workgroups' rings.
//
// Data movement. D % 64 == 0: the gallery k-tile and the three query-plane k-tiles (rows p * q_tile + query of the slot's second part) arrive
// by direct-to-LDS loads (buffer_load_dwordx4 ... lds, the swizzle applied to the per-lane SOURCE chunk) into a two-slot ring, the loads of
// stage s + 1 in flight under the MFMAs of stage s, one barrier per stage. Other D (D % 8 == 0): both are staged through registers, chunks at
// or past D as zeros, one slot, two barriers per stage. The split image comes from the prologue kernel and not from the loop: splitting in the
// loop would repeat 3 converts and 2 subtractions per element in every stage of every unit.
//
// LDS: a ring slot is (128 + 3 q_tile) rows of 128 B: 28 KB (q_tile 32) or 40 KB (q_tile 64); the ring 56 / 80 KB, the unit-end lists overlaid.
// Two workgroups per CU are planned (mbn_persistent_grid below): 2 x 80 KB is the CU's 160 KB, and one workgroup's barrier and unit-end merge
// run under the other's MFMAs. Scratch 0.
#include "mbn_internal.h"
#include "mbn_device.h"
#include "mbn_x6.h"
#include "mbn_similarity_list.h"

namespace {

constexpr int SB_GP = 128;              // gallery rows per panel
constexpr int SB_NT = 256;              // threads per workgroup

struct SimBArgs {
    const uint16_t *gallery, *qimg;     // [G][D] bf16; the split image [Q][3][D] bf16
    const float *q_scale, *g_scale;
    int2 *ws;                           // [chunks][Q][k] (index, score bits)
    int Q, G, D, k;
    int qtiles, chunks, g_tile;
};

// One thread per 8 query elements: 32 bytes in, 16 bytes out to each plane's row. Q * D / 8 threads (below 2^26: mbn_similarity_envelope_bf16)
__global__ __launch_bounds__(256) void simb_split(uint16_t *img, const float *queries, int Q, int D)
{
    const int per_row = D >> 3;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Q * per_row) return;
    const int row = t / per_row, d = (t - row * per_row) * 8;
    const float *x = queries + (size_t)row * D + d;
    u4 h, m, l;
    mbn_x6_split8(*reinterpret_cast<const f4 *>(x), *reinterpret_cast<const f4 *>(x + 4), h, m, l);
    uint16_t *o = img + (size_t)row * 3 * D + d;
    *reinterpret_cast<u4 *>(o) = h;
    *reinterpret_cast<u4 *>(o + D) = m;
    *reinterpret_cast<u4 *>(o + 2 * D) = l;
}

// LD pieces of 8 rows x 128 B of this wave: buffer_load_dwordx4 ... lds writes 1 KiB linearly at the wave-uniform LDS address; piece p lands 32 tile
// rows behind piece p - 1 (sim_dma_rows of mbn_f32_similarity.hip on 2-byte elements: the offsets are bytes)
__device__ __forceinline__ void simb_dma_rows(const __amdgpu_buffer_rsrc_t rsrc, float *lds_rows, const unsigned *voff, int soff, const int LD)
{
#pragma unroll
    for (int p = 0; p < LD; p++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(lds_rows + 32 * p * 32), 16, voff[p], soff, 0, 0);
}

// NQ 32-query blocks per tile (q_tile = 32 NQ), NQ x 4 / NQ waves; KCAP list slots; DMA: D % 64 == 0, direct-to-LDS staging
template <int NQ, int KCAP, bool DMA>
__global__ __launch_bounds__(SB_NT) void simb_topk(SimBArgs a)
{
    constexpr int QT = 32 * NQ;
    constexpr int WGAL = 4 / NQ;                               // waves along the gallery
    constexpr int RB = SB_GP / 32 / WGAL;                      // 32-row gallery blocks per wave: 1 or 2
    constexpr int LPQ = 2 * WGAL;                              // lists per query at the unit's end: gallery waves x lane halves
    constexpr int QROWS = 3 * QT;                              // query rows of a slot: plane p of tile query j at row p * QT + j
    constexpr int TILE = (SB_GP + QROWS) * 32;                 // 4-byte words per ring slot: gallery k-tile, then the planes' k-tiles
    constexpr int NBUF = DMA ? 2 : 1;
    constexpr int LISTS = SB_NT * KCAP;                        // the unit-end merge: [query][gallery wave * 2 + half][slot], scores then indices
    constexpr int LDSW = NBUF * TILE > 2 * LISTS ? NBUF * TILE : 2 * LISTS;
    constexpr int GLD = SB_GP * 8 / SB_NT, QLD = QROWS * 8 / SB_NT;      // 16-byte pieces per thread per k-tile: 4 and 3 NQ
    static_assert(QT * LPQ == SB_NT, "one thread per list at the unit's end");
    __shared__ __attribute__((aligned(16))) float lds[LDSW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wq = wave & (NQ - 1), wg = wave / NQ;            // this wave's query block and its first gallery block (RB * wg)
    const int li = lane & 31, lh = lane >> 5;
    const int nk = (a.D + 63) >> 6;
    const int nunits = a.qtiles * a.chunks;                    // below 2^31: mbn_similarity_envelope_bf16
    const int st_ch = tid & 7, st_r = tid >> 3;                // staging: tile row st_r + 32 p, 16-byte LDS slot st_ch
    const __amdgpu_buffer_rsrc_t qrsrc = mbn_make_rsrc(a.qimg, (unsigned)a.Q * 3u * (unsigned)a.D * 2u);      // below 3 * 2^30 bytes

    for (int vb = blockIdx.x; vb < nunits; vb += gridDim.x) {
        const int unit = mbn_xcd_remap(vb, nunits);
        const int chunk = unit / a.qtiles, q0 = (unit - chunk * a.qtiles) * QT;
        const int g0 = chunk * a.g_tile;
        const int gend = g0 + a.g_tile < a.G ? g0 + a.g_tile : a.G;
        const int panels = (gend - g0 + SB_GP - 1) / SB_GP;
        const int stages = panels * nk;

        // byte offsets of this thread's pieces at k-tile 0. Rows past Q / past G are clamped: computed, never ranked
        unsigned q_vo[QLD], g_vo[GLD];
#pragma unroll
        for (int p = 0; p < QLD; p++) {
            const int row = st_r + 32 * p, plane = row / QT;
            int q = q0 + row - plane * QT;
            if (q >= a.Q) q = a.Q - 1;
            const int c = DMA ? (st_ch ^ (row >> 1)) & 7 : st_ch;
            q_vo[p] = (((unsigned)q * 3u + plane) * (unsigned)a.D + c * 8) * 2u;
        }
        auto set_panel = [&](int gp0) {
            const int last = a.G - 1 - gp0;                     // >= 0: a panel starts inside the gallery
#pragma unroll
            for (int p = 0; p < GLD; p++) {
                const int row = st_r + 32 * p;
                const int r = row < last ? row : last;
                const int c = DMA ? (st_ch ^ (row >> 1)) & 7 : st_ch;
                g_vo[p] = ((unsigned)r * (unsigned)a.D + c * 8) * 2u;
            }
        };
        // one k-tile of the gallery and of the three planes into ring slot `buf`
        auto stage_dma = [&](const uint16_t *gbase, unsigned gbytes, int k0, int buf) __attribute__((always_inline)) {
            float *base = lds + buf * TILE;
            simb_dma_rows(mbn_make_rsrc(gbase, gbytes), base + 8 * wave_u * 32, g_vo, k0 * 2, GLD);
            simb_dma_rows(qrsrc, base + (SB_GP + 8 * wave_u) * 32, q_vo, k0 * 2, QLD);
        };

        SimList<KCAP> best;
        best.clear();
        int qmine = q0 + 32 * wq + li;
        if (qmine >= a.Q) qmine = a.Q - 1;
        const float qs = a.q_scale ? a.q_scale[qmine] : 1.f;
        f16v acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rb][r] = 0.f;

        // the panel whose k-tiles are being LOADED (one stage ahead of the one being multiplied under DMA)
        int ld_panel = 0, ld_kt = 0;
        const uint16_t *ld_base = a.gallery + (size_t)g0 * a.D;
        auto ld_bytes = [&](int panel) {
            const int rows = gend - (g0 + panel * SB_GP);
            return (unsigned)(rows < SB_GP ? rows : SB_GP) * (unsigned)a.D * 2u;
        };
        set_panel(g0);
        if (DMA) stage_dma(ld_base, ld_bytes(0), 0, 0);

        int kt = 0, panel = 0;
        for (int s = 0; s < stages; s++) {
            const float *As, *Bs;
            if constexpr (DMA) {
                // stage s has landed (each wave waits for its own loads, vmcnt(0), ahead of the barrier) and every wave is done with the other slot
                mbn_waitcnt<0>();
                if (s + 1 < stages) {
                    if (++ld_kt == nk) {
                        ld_kt = 0;
                        ld_panel++;
                        ld_base += (size_t)SB_GP * a.D;
                        set_panel(g0 + ld_panel * SB_GP);
                    }
                    stage_dma(ld_base, ld_bytes(ld_panel), ld_kt * 64, (s + 1) & 1);
                }
                As = lds + (s & 1) * TILE;
            } else {
                if (s > 0 && kt == 0) {
                    ld_base += (size_t)SB_GP * a.D;
                    set_panel(g0 + panel * SB_GP);
                }
                const bool ok = kt * 64 + st_ch * 8 < a.D;       // D % 8 == 0: a chunk is whole or past the row
                const u4 zero4 = u4{ 0u, 0u, 0u, 0u };
                u4 gr[GLD], qr[QLD];
#pragma unroll
                for (int p = 0; p < GLD; p++)
                    gr[p] = ok ? *reinterpret_cast<const u4 *>(reinterpret_cast<const char *>(ld_base) + g_vo[p] + kt * 128) : zero4;
#pragma unroll
                for (int p = 0; p < QLD; p++)
                    qr[p] = ok ? *reinterpret_cast<const u4 *>(reinterpret_cast<const char *>(a.qimg) + q_vo[p] + kt * 128) : zero4;
                __syncthreads();                                  // the slot's previous k-tile is read by every wave
#pragma unroll
                for (int p = 0; p < GLD; p++) *reinterpret_cast<u4 *>(lds + mbn_swz(st_r + 32 * p, st_ch)) = gr[p];
#pragma unroll
                for (int p = 0; p < QLD; p++) *reinterpret_cast<u4 *>(lds + SB_GP * 32 + mbn_swz(st_r + 32 * p, st_ch)) = qr[p];
                __syncthreads();
                As = lds;
            }
            Bs = As + SB_GP * 32;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = 2 * j + lh;
                u4 av[RB], bv[3];
#pragma unroll
                for (int rb = 0; rb < RB; rb++) av[rb] = *reinterpret_cast<const u4 *>(As + mbn_swz(32 * (RB * wg + rb) + li, c));
#pragma unroll
                for (int p = 0; p < 3; p++) bv[p] = *reinterpret_cast<const u4 *>(Bs + mbn_swz(p * QT + 32 * wq + li, c));
#pragma unroll
                for (int p = 2; p >= 0; p--)                      // l, m, h
#pragma unroll
                    for (int rb = 0; rb < RB; rb++)
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, av[rb]), __builtin_bit_cast(bf8, bv[p]), acc[rb], 0, 0, 0);
            }
            if (++kt < nk) continue;
            // ---- a panel's sums are complete: scale and rank this lane's 16 gallery rows per row block, in ascending index order
            kt = 0;
            const int grow0 = g0 + panel * SB_GP + 32 * RB * wg + 4 * lh;
            panel++;
#pragma unroll
            for (int rb = 0; rb < RB; rb++) {
                float gs[16];                                     // the 16 loads go out together, ahead of the first compare
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int gi = grow0 + 32 * rb + (r & 3) + 8 * (r >> 2);
                    gs[r] = a.g_scale ? a.g_scale[gi < gend ? gi : gend - 1] : 1.f;
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int gi = grow0 + 32 * rb + (r & 3) + 8 * (r >> 2);
                    float sc = acc[rb][r];
                    if (a.q_scale) sc = sc * qs;
                    if (a.g_scale) sc = sc * gs[r];
                    if (gi < gend) best.push(sc, gi);
                    acc[rb][r] = 0.f;
                }
            }
        }

        // ---- unit end: the LPQ lists of a query meet in LDS (the ring is free behind the barrier), LPQ neighbouring lanes per query merge them
        __syncthreads();
        float *ls = lds;
        int *lx = reinterpret_cast<int *>(lds + LISTS);
        {
            const int o = ((32 * wq + li) * LPQ + 2 * wg + lh) * KCAP;
#pragma unroll
            for (int j = 0; j < KCAP; j++) { ls[o + j] = best.s[j]; lx[o + j] = best.i[j]; }
        }
        __syncthreads();
        {
            SimList<KCAP> m, o;                                   // thread t takes list t: query t / LPQ, list t % LPQ (consecutive LDS words)
#pragma unroll
            for (int j = 0; j < KCAP; j++) { m.s[j] = ls[tid * KCAP + j]; m.i[j] = lx[tid * KCAP + j]; }
#pragma unroll
            for (int d = 1; d < LPQ; d <<= 1) {
#pragma unroll
                for (int j = 0; j < KCAP; j++) { o.s[j] = __shfl_xor(m.s[j], d, 64); o.i[j] = __shfl_xor(m.i[j], d, 64); }
                m.merge(o);
            }
            const int q = q0 + tid / LPQ;
            if (tid % LPQ == 0 && q < a.Q) {
                int2 *w = a.ws + ((size_t)chunk * a.Q + q) * a.k;
#pragma unroll
                for (int j = 0; j < KCAP; j++)
                    if (j < a.k) w[j] = int2{ m.i[j], __float_as_int(m.s[j]) };
            }
        }
        __syncthreads();                                          // the lists are read before the next unit's first k-tile lands on them
    }
}

// One wave per row, four rows per workgroup. Lane l owns the 8-element groups l, l + 64, ... of the row: two 16-byte loads (fp32, rounded to
// nearest even by the hardware convert, a NaN stays a NaN) or one (bf16), one 16-byte store, then an fmaf chain over the ROUNDED elements in
// order and the fold of the wave's 64 partial sums, as rows_norm (mbn_f32_similarity.hip). The order depends on D alone
template <typename T>
__global__ __launch_bounds__(256) void rows_pack(uint16_t *out, float *inv_norm, const T *in, int N, int D)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const T *x = in + (size_t)row * D;
    float acc = 0.f;
    for (int d = 8 * lane; d < D; d += 512) {
        u4 p;
        if constexpr (sizeof(T) == 4) p = __builtin_bit_cast(u4, __builtin_convertvector(mbn_ld8(x + d), bf8));
        else p = *reinterpret_cast<const u4 *>(x + d);
        if (out) *reinterpret_cast<u4 *>(out + (size_t)row * D + d) = p;
        const f8 v = mbn_widen8(p);
#pragma unroll
        for (int e = 0; e < 8; e++) acc = fmaf(v[e], v[e], acc);
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (inv_norm && lane == 0) inv_norm[row] = acc == 0.f ? 0.f : 1.0f / sqrtf(acc);      // both correctly rounded (hipcc's default)
}

template <int NQ, int KCAP>
void simb_launch(const SimBArgs &a, hipStream_t s, unsigned grid)
{
    if (a.D % 64 == 0) hipLaunchKernelGGL((simb_topk<NQ, KCAP, true>), dim3(grid), dim3(SB_NT), 0, s, a);
    else hipLaunchKernelGGL((simb_topk<NQ, KCAP, false>), dim3(grid), dim3(SB_NT), 0, s, a);
}

}   // namespace

// The arguments are inside mbn_similarity_envelope_bf16 and the pointers checked (mbn_similarity_topk_bf16). Three launches on s
int mbn_launch_bf16_similarity_topk(mbn_context *ctx, hipStream_t s, int32_t *idx, float *score, const float *queries, const void *gallery,
                                    const float *q_scale, const float *g_scale, int Q, int G, int D, int k, void *workspace)
{
    int q_tile = 0, g_tile = 0;
    if (mbn_similarity_tile_bf16(&q_tile, &g_tile, Q, D) != MBN_OK) return MBN_EINVAL;
    SimBArgs a;
    a.gallery = (const uint16_t *)gallery; a.q_scale = q_scale; a.g_scale = g_scale; a.ws = (int2 *)workspace;
    a.Q = Q; a.G = G; a.D = D; a.k = k;
    a.qtiles = (Q + q_tile - 1) / q_tile; a.chunks = (G + g_tile - 1) / g_tile; a.g_tile = g_tile;
    uint16_t *img = (uint16_t *)((char *)workspace + mbn_similarity_split_offset_bf16(Q, G, D, k));
    a.qimg = img;
    hipLaunchKernelGGL(simb_split, dim3((unsigned)((Q * (D / 8) + 255) / 256)), dim3(256), 0, s, img, queries, Q, D);
    // resident workgroups per CU: TWO. The ring is 56 KB (q_tile 32) or 80 KB (q_tile 64) of the CU's 160 KB, so a third does not fit beside
    // two of the wide form; two keep a second wave on every SIMD, whose MFMAs cover the first's barrier, epilogue and unit-end merge
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, 2, (long long)a.qtiles * a.chunks);
    const int cap = k <= 4 ? 4 : 8;
    if (q_tile == 32) { if (cap == 4) simb_launch<1, 4>(a, s, grid); else simb_launch<1, 8>(a, s, grid); }
    else { if (cap == 4) simb_launch<2, 4>(a, s, grid); else simb_launch<2, 8>(a, s, grid); }
    if (cap == 4) hipLaunchKernelGGL(sim_merge<4>, dim3((unsigned)Q), dim3(64), 0, s, idx, score, (const int2 *)workspace, Q, a.chunks, k);
    else hipLaunchKernelGGL(sim_merge<8>, dim3((unsigned)Q), dim3(64), 0, s, idx, score, (const int2 *)workspace, Q, a.chunks, k);
    return MBN_OK;
}

// out (may be null) [N][D] bf16 = the rows rounded, inv_norm (may be null) [N] of the rounded rows; in fp32 or bf16 by dtype. D % 8 == 0 and the
// pointers are checked
int mbn_launch_rows_pack_bf16(mbn_context *, hipStream_t s, void *out, float *inv_norm, const void *in, int dtype, int N, int D)
{
    const dim3 grid((unsigned)((N + 3) / 4));
    if (dtype == MBN_DT_BF16) hipLaunchKernelGGL(rows_pack<uint16_t>, grid, dim3(256), 0, s, (uint16_t *)out, inv_norm, (const uint16_t *)in, N, D);
    else hipLaunchKernelGGL(rows_pack<float>, grid, dim3(256), 0, s, (uint16_t *)out, inv_norm, (const float *)in, N, D);
    return MBN_OK;
}
