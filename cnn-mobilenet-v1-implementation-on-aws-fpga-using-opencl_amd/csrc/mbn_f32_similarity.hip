// mbn_f32_similarity.hip — nearest neighbours on embeddings for gfx950 (include/mbn.h, "Nearest neighbours"): the k best gallery rows per
// query under score = (queries . gallery^T) * q_scale * g_scale, as an fp32 MFMA GEMM whose epilogue is a running top-k. The [Q][G] product is
// never in memory: a score lives in one accumulator register between the last v_mfma of its sum and one compare. DESIGN.md 7f.
//
//   sim_topk      the fused GEMM + top-k over work units (query tile, gallery chunk); writes k candidates per (chunk, query) to the workspace
//   sim_merge     one wave per query: the chunks' candidates -> topk_idx / topk_score (mbn_similarity_list.h, with the ranking and the lists)
//   rows_norm     mbn_row_inv_norm_f32 and mbn_embed_rows: one wave per row, optional widening copy, 1 / sqrt(sum of squares)
//
// MFMA sides. v_mfma_f32_32x32x2_f32 takes A [32 i][2 k] and B [2 k][32 j] with lane l feeding A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31],
// and leaves D[i][j] with j = l & 31 and i = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15, in lane l. The GALLERY is the A side and the QUERIES are
// the B side: a lane then owns ONE query (column l & 31 of each of the NQ 32-query blocks of the tile) and 16 gallery rows per 32-row block, which
// it meets in ascending index order (r ascending inside a panel, panels ascending). So the top-k of a query is a list in that lane's registers
// (KCAP = 4 or 8 slots of score + index, sorted best first), a new score costs ONE comparison with the list's last slot on the common path, and
// nothing crosses lanes inside the gallery loop. The two lane halves and the four waves of a workgroup hold eight lists per query; they meet once
// per work unit, through LDS.
//
// The d order. Operands pass LDS as in mbn_f32_pw.hip: k-tiles of 32 floats (128-byte rows, 16-byte chunks XOR-swizzled by row / 2: mbn_swz), one
// ds_read_b128 per lane feeding four MFMAs, lane half h owning k = 32 t + 8 g + 4 h .. + 3 of group g of k-tile t. A sum therefore runs over
// t = 0 .. ceil(D / 32) - 1, g = 0..3, s = 0..3, each instruction adding the products at d = 32 t + 8 g + s and d + 4; elements past D are zeros
// on both sides. That order is a function of D alone: not of Q, G, the tile or chunk a pair falls in, or the number of workgroups. With the
// fmul order of the two scales fixed too, a pair's score bits are fixed, and the ranking is a strict total order over (score, index), so the k
// best of a query are ONE set in ONE order however the gallery is chunked and merged: the output bytes are the same at every planning CU count
// and on every graph replay.
//
// Data movement. A workgroup (4 waves) works on a q_tile x 128 tile per stage: wave w owns gallery rows 32 w .. 32 w + 31 of the panel and all
// q_tile queries. D % 32 == 0: both operands' k-tiles arrive by direct-to-LDS loads (buffer_load_dwordx4 ... lds, the swizzle applied to the
// per-lane SOURCE chunk) into a two-slot ring, the loads of stage s + 1 in flight under the MFMAs of stage s, one barrier per stage; the stages
// of a unit's panels run through without a break. The gallery's descriptor is rebuilt per panel on a 64-bit base (offsets inside a panel stay
// below 2 MB). The query k-tile comes along with the gallery's instead of staying resident for the unit: q_tile x D floats (128 KB at D = 1024)
// beside the ring would leave one workgroup per CU, and the re-read is L2 traffic (q_tile / 128 of the gallery's LDS fill), not HBM traffic.
// D % 32 != 0 (short or ragged rows): both k-tiles are staged through registers with zeros past D, one slot, two barriers per stage.
//
// Work split. Unit u = (chunk u / qtiles, query tile u % qtiles) in mbn_xcd_remap order: the query tiles of one gallery chunk run next to each
// other on one XCD, so a chunk is fetched from HBM once and re-read from that L2. Persistent workgroups walk the units with stride gridDim; a unit
// writes its own [chunk][query][k] slots of the workspace, so no workgroup waits for another and none of them needs to know the grid.
#include "mbn_internal.h"
#include "mbn_device.h"
#include "mbn_similarity_list.h"

namespace {

constexpr int SIM_GP = 128;             // gallery rows per panel (32 per wave)
constexpr int SIM_NT = 256;             // threads per workgroup

struct SimArgs {
    const float *queries, *gallery, *q_scale, *g_scale;
    int2 *ws;                // [chunks][Q][k] (index, score bits)
    int Q, G, D, k;
    int qtiles, chunks, g_tile;
};

// LD pieces of 8 rows x 128 B of this wave: buffer_load_dwordx4 ... lds writes 1 KiB linearly at the wave-uniform LDS address; piece p lands 32 tile
// rows behind piece p - 1. (A __device__ function, not a lambda of the kernel: see lds_dma_rows in mbn_f32_pw.hip.)
__device__ __forceinline__ void sim_dma_rows(const __amdgpu_buffer_rsrc_t rsrc, float *lds_rows, const unsigned *voff, int soff, const int LD)
{
#pragma unroll
    for (int p = 0; p < LD; p++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(lds_rows + 32 * p * 32), 16, voff[p], soff, 0, 0);
}

// NQ 32-query blocks per tile (q_tile = 32 NQ); KCAP list slots; DMA: D % 32 == 0, direct-to-LDS staging
template <int NQ, int KCAP, bool DMA>
__global__ __launch_bounds__(SIM_NT) void sim_topk(SimArgs a)
{
    constexpr int QT = 32 * NQ;
    constexpr int TILE = (SIM_GP + QT) * 32;                   // floats per ring slot: gallery k-tile, then query k-tile
    constexpr int NBUF = DMA ? 2 : 1;
    constexpr int LISTS = 8 * QT * KCAP;                       // the unit-end merge: [query][wave * 2 + half][slot], scores then indices
    constexpr int LDSF = NBUF * TILE > 2 * LISTS ? NBUF * TILE : 2 * LISTS;
    constexpr int GLD = SIM_GP * 8 / SIM_NT, QLD = QT * 8 / SIM_NT;      // 16-byte pieces per thread per k-tile: 4 and NQ
    __shared__ __attribute__((aligned(16))) float lds[LDSF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int li = lane & 31, lh = lane >> 5;
    const int nk = (a.D + 31) >> 5;
    const int nunits = a.qtiles * a.chunks;                    // below 2^31: mbn_similarity_envelope
    const int st_ch = tid & 7, st_r = tid >> 3;                // staging: tile row st_r + 32 p, 16-byte LDS slot st_ch
    const unsigned q_bytes = (unsigned)a.Q * (unsigned)a.D * 4u;
    const __amdgpu_buffer_rsrc_t qrsrc = mbn_make_rsrc(a.queries, q_bytes);

    for (int vb = blockIdx.x; vb < nunits; vb += gridDim.x) {
        const int unit = mbn_xcd_remap(vb, nunits);
        const int chunk = unit / a.qtiles, q0 = (unit - chunk * a.qtiles) * QT;
        const int g0 = chunk * a.g_tile;
        const int gend = g0 + a.g_tile < a.G ? g0 + a.g_tile : a.G;
        const int panels = (gend - g0 + SIM_GP - 1) / SIM_GP;
        const int stages = panels * nk;

        // source offsets of this thread's pieces. Rows past Q / past G are clamped: computed, never ranked
        unsigned q_vo[QLD], g_vo[GLD];
#pragma unroll
        for (int p = 0; p < QLD; p++) {
            const int row = st_r + 32 * p;
            int q = q0 + row;
            if (q >= a.Q) q = a.Q - 1;
            const int c = DMA ? (st_ch ^ (row >> 1)) & 7 : st_ch;
            q_vo[p] = ((unsigned)q * (unsigned)a.D + c * 4) * 4u;
        }
        auto set_panel = [&](int gp0) {
            const int last = a.G - 1 - gp0;                     // >= 0: a panel starts inside the gallery
#pragma unroll
            for (int p = 0; p < GLD; p++) {
                const int row = st_r + 32 * p;
                const int r = row < last ? row : last;
                const int c = DMA ? (st_ch ^ (row >> 1)) & 7 : st_ch;
                g_vo[p] = ((unsigned)r * (unsigned)a.D + c * 4) * 4u;
            }
        };
        // one k-tile of both operands into ring slot `buf`: a wave-instruction writes 8 rows x 128 B linearly at a wave-uniform LDS address
        auto stage_dma = [&](const float *gbase, unsigned gbytes, int k0, int buf) __attribute__((always_inline)) {
            float *base = lds + buf * TILE;
            sim_dma_rows(mbn_make_rsrc(gbase, gbytes), base + 8 * wave_u * 32, g_vo, k0 * 4, GLD);
            sim_dma_rows(qrsrc, base + (SIM_GP + 8 * wave_u) * 32, q_vo, k0 * 4, QLD);
        };

        SimList<KCAP> best[NQ];
        float qs[NQ];
#pragma unroll
        for (int nq = 0; nq < NQ; nq++) {
            best[nq].clear();
            int q = q0 + 32 * nq + li;
            if (q >= a.Q) q = a.Q - 1;
            qs[nq] = a.q_scale ? a.q_scale[q] : 1.f;
        }
        f16v acc[NQ];
#pragma unroll
        for (int nq = 0; nq < NQ; nq++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[nq][r] = 0.f;

        // the panel whose k-tiles are being LOADED (one stage ahead of the one being multiplied under DMA)
        int ld_panel = 0, ld_kt = 0;
        const float *ld_base = a.gallery + (size_t)g0 * a.D;
        auto ld_bytes = [&](int panel) {
            const int rows = gend - (g0 + panel * SIM_GP);
            return (unsigned)(rows < SIM_GP ? rows : SIM_GP) * (unsigned)a.D * 4u;
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
                        ld_base += (size_t)SIM_GP * a.D;
                        set_panel(g0 + ld_panel * SIM_GP);
                    }
                    stage_dma(ld_base, ld_bytes(ld_panel), ld_kt * 32, (s + 1) & 1);
                }
                As = lds + (s & 1) * TILE;
            } else {
                if (s > 0 && kt == 0) {
                    ld_base += (size_t)SIM_GP * a.D;
                    set_panel(g0 + panel * SIM_GP);
                }
                const bool ok = kt * 32 + st_ch * 4 < a.D;
                const f4 zero4 = f4{ 0.f, 0.f, 0.f, 0.f };
                f4 gr[GLD], qr[QLD];
#pragma unroll
                for (int p = 0; p < GLD; p++)
                    gr[p] = ok ? *reinterpret_cast<const f4 *>(reinterpret_cast<const char *>(ld_base) + g_vo[p] + kt * 128) : zero4;
#pragma unroll
                for (int p = 0; p < QLD; p++)
                    qr[p] = ok ? *reinterpret_cast<const f4 *>(reinterpret_cast<const char *>(a.queries) + q_vo[p] + kt * 128) : zero4;
                __syncthreads();                                  // the slot's previous k-tile is read by every wave
#pragma unroll
                for (int p = 0; p < GLD; p++) *reinterpret_cast<f4 *>(lds + mbn_swz(st_r + 32 * p, st_ch)) = gr[p];
#pragma unroll
                for (int p = 0; p < QLD; p++) *reinterpret_cast<f4 *>(lds + SIM_GP * 32 + mbn_swz(st_r + 32 * p, st_ch)) = qr[p];
                __syncthreads();
                As = lds;
            }
            Bs = As + SIM_GP * 32;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = 2 * g + lh;
                const f4 av = *reinterpret_cast<const f4 *>(As + mbn_swz(32 * wave + li, c));
                f4 bv[NQ];
#pragma unroll
                for (int nq = 0; nq < NQ; nq++) bv[nq] = *reinterpret_cast<const f4 *>(Bs + mbn_swz(32 * nq + li, c));
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int nq = 0; nq < NQ; nq++) acc[nq] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[nq][e], acc[nq], 0, 0, 0);
            }
            if (++kt < nk) continue;
            // ---- a panel's sums are complete: scale and rank this lane's 16 gallery rows per query block, in ascending index order
            kt = 0;
            const int grow0 = g0 + panel * SIM_GP + 32 * wave + 4 * lh;
            panel++;
            float gs[16];                                         // the 16 loads go out together, ahead of the first compare
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gi = grow0 + (r & 3) + 8 * (r >> 2);
                gs[r] = a.g_scale ? a.g_scale[gi < gend ? gi : gend - 1] : 1.f;
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gi = grow0 + (r & 3) + 8 * (r >> 2);
                const bool in = gi < gend;
#pragma unroll
                for (int nq = 0; nq < NQ; nq++) {
                    float sc = acc[nq][r];
                    if (a.q_scale) sc = sc * qs[nq];
                    if (a.g_scale) sc = sc * gs[r];
                    if (in) best[nq].push(sc, gi);
                    acc[nq][r] = 0.f;
                }
            }
        }

        // ---- unit end: the eight lists of a query meet in LDS (the ring is free behind the barrier), eight lanes per query merge them
        __syncthreads();
        float *ls = lds;
        int *lx = reinterpret_cast<int *>(lds + LISTS);
#pragma unroll
        for (int nq = 0; nq < NQ; nq++)
#pragma unroll
            for (int j = 0; j < KCAP; j++) {
                const int o = ((32 * nq + li) * 8 + 2 * wave + lh) * KCAP + j;
                ls[o] = best[nq].s[j];
                lx[o] = best[nq].i[j];
            }
        __syncthreads();
        // thread t takes list t (query t >> 3, list t & 7: consecutive LDS words) and the eight neighbours fold by halves across lanes
#pragma unroll 1
        for (int t = tid; t < 8 * QT; t += SIM_NT) {
            SimList<KCAP> m, o;
#pragma unroll
            for (int j = 0; j < KCAP; j++) { m.s[j] = ls[t * KCAP + j]; m.i[j] = lx[t * KCAP + j]; }
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) {
#pragma unroll
                for (int j = 0; j < KCAP; j++) { o.s[j] = __shfl_xor(m.s[j], d, 64); o.i[j] = __shfl_xor(m.i[j], d, 64); }
                m.merge(o);
            }
            const int q = q0 + (t >> 3);
            if ((t & 7) == 0 && q < a.Q) {
                int2 *w = a.ws + ((size_t)chunk * a.Q + q) * a.k;
#pragma unroll
                for (int j = 0; j < KCAP; j++)
                    if (j < a.k) w[j] = int2{ m.i[j], __float_as_int(m.s[j]) };
            }
        }
        __syncthreads();                                          // the lists are read before the next unit's first k-tile lands on them
    }
}

// One wave per row, four rows per workgroup. Lane l owns the 4-element groups l, l + 64, ... of the row: 16-byte loads (fp32) or 8-byte loads
// (bf16, widened exactly), an fmaf chain over its elements in order, then the wave's 64 partial sums fold by halves. The order depends on D alone
template <typename T>
__global__ __launch_bounds__(256) void rows_norm(float *out, float *inv_norm, const T *in, int N, int D)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const T *x = in + (size_t)row * D;
    float acc = 0.f;
    for (int d = 4 * lane; d < D; d += 256) {
        f4 v;
        if constexpr (sizeof(T) == 4) v = *reinterpret_cast<const f4 *>(x + d);
        else {
            const u2 p = *reinterpret_cast<const u2 *>(x + d);
            v = f4{ __builtin_bit_cast(float, p.x << 16), __builtin_bit_cast(float, p.x & 0xffff0000u), __builtin_bit_cast(float, p.y << 16),
                    __builtin_bit_cast(float, p.y & 0xffff0000u) };
        }
        if (out) *reinterpret_cast<f4 *>(out + (size_t)row * D + d) = v;
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (inv_norm && lane == 0) inv_norm[row] = acc == 0.f ? 0.f : 1.0f / sqrtf(acc);      // both correctly rounded (hipcc's default)
}

template <int NQ, int KCAP>
void sim_launch(const SimArgs &a, hipStream_t s, unsigned grid)
{
    if (a.D % 32 == 0) hipLaunchKernelGGL((sim_topk<NQ, KCAP, true>), dim3(grid), dim3(SIM_NT), 0, s, a);
    else hipLaunchKernelGGL((sim_topk<NQ, KCAP, false>), dim3(grid), dim3(SIM_NT), 0, s, a);
}

}   // namespace

// The arguments are inside mbn_similarity_envelope and the pointers checked (mbn_similarity_topk_f32)
int mbn_launch_f32_similarity_topk(mbn_context *ctx, hipStream_t s, int32_t *idx, float *score, const float *queries, const float *gallery,
                                   const float *q_scale, const float *g_scale, int Q, int G, int D, int k, void *workspace)
{
    int q_tile = 0, g_tile = 0;
    if (mbn_similarity_tile(&q_tile, &g_tile, Q, D) != MBN_OK) return MBN_EINVAL;
    SimArgs a;
    a.queries = queries; a.gallery = gallery; a.q_scale = q_scale; a.g_scale = g_scale; a.ws = (int2 *)workspace;
    a.Q = Q; a.G = G; a.D = D; a.k = k;
    a.qtiles = (Q + q_tile - 1) / q_tile; a.chunks = (G + g_tile - 1) / g_tile; a.g_tile = g_tile;
    // resident workgroups per CU: the ring (40 / 48 KB, 20 / 24 KB staged through registers) and 4 waves of at most 128 VGPRs leave room for 3
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, 3, (long long)a.qtiles * a.chunks);
    const int cap = k <= 4 ? 4 : 8;
    if (q_tile == 32) { if (cap == 4) sim_launch<1, 4>(a, s, grid); else sim_launch<1, 8>(a, s, grid); }
    else { if (cap == 4) sim_launch<2, 4>(a, s, grid); else sim_launch<2, 8>(a, s, grid); }
    if (cap == 4) hipLaunchKernelGGL(sim_merge<4>, dim3((unsigned)Q), dim3(64), 0, s, idx, score, (const int2 *)workspace, Q, a.chunks, k);
    else hipLaunchKernelGGL(sim_merge<8>, dim3((unsigned)Q), dim3(64), 0, s, idx, score, (const int2 *)workspace, Q, a.chunks, k);
    return MBN_OK;
}

// out (may be null) [N][D] fp32 = the rows widened, inv_norm (may be null) [N]; in fp32 or bf16 by dtype. D % 4 == 0 and the pointers are checked
int mbn_launch_rows_norm(mbn_context *, hipStream_t s, float *out, float *inv_norm, const void *in, int dtype, int N, int D)
{
    const dim3 grid((unsigned)((N + 3) / 4));
    if (dtype == MBN_DT_BF16) hipLaunchKernelGGL(rows_norm<uint16_t>, grid, dim3(256), 0, s, out, inv_norm, (const uint16_t *)in, N, D);
    else hipLaunchKernelGGL(rows_norm<float>, grid, dim3(256), 0, s, out, inv_norm, (const float *)in, N, D);
    return MBN_OK;
}
