// mbn_similarity_list.h — what the nearest-neighbour kernels (mbn_f32_similarity.hip, mbn_bf16_similarity.hip) must agree on: the ranking, the
// sorted top-k list a lane keeps in registers, and the one-wave-per-query merge of the workspace [chunks][Q][k] both of them fill.
#pragma once

#include "mbn_device.h"

namespace {

constexpr int SIM_EMPTY = 0x7fffffff;   // index of an empty slot: with score -inf it loses against every ranked entry, -inf scores included

// the ranking: a beats b when its score is higher, or equal with the lower index. A NaN beats nothing and is beaten by nothing: it never enters a list
__device__ __forceinline__ bool sim_beats(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

template <int KCAP>
struct SimList {
    float s[KCAP];
    int i[KCAP];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < KCAP; j++) { s[j] = -INFINITY; i[j] = SIM_EMPTY; }
    }
    // one candidate: a single comparison unless it enters; then it takes the last slot and rises by compare-exchange (static indices only)
    __device__ __forceinline__ void push(float cs, int ci)
    {
        if (!sim_beats(cs, ci, s[KCAP - 1], i[KCAP - 1])) return;
        s[KCAP - 1] = cs; i[KCAP - 1] = ci;
#pragma unroll
        for (int j = KCAP - 1; j > 0; j--) {
            const bool up = sim_beats(s[j], i[j], s[j - 1], i[j - 1]);
            const float ts = s[j]; const int ti = i[j];
            s[j] = up ? s[j - 1] : ts; i[j] = up ? i[j - 1] : ti;
            s[j - 1] = up ? ts : s[j - 1]; i[j - 1] = up ? ti : i[j - 1];
        }
    }
    // the KCAP best of this list and another sorted one: slot j against the other's slot KCAP - 1 - j keeps the KCAP best as a bitonic sequence,
    // log2 KCAP half-cleaners sort it. Entries are distinct under the order except empty slots, which are interchangeable
    __device__ __forceinline__ void merge(const SimList &o)
    {
#pragma unroll
        for (int j = 0; j < KCAP; j++) {
            const bool take = sim_beats(o.s[KCAP - 1 - j], o.i[KCAP - 1 - j], s[j], i[j]);
            s[j] = take ? o.s[KCAP - 1 - j] : s[j]; i[j] = take ? o.i[KCAP - 1 - j] : i[j];
        }
#pragma unroll
        for (int st = KCAP / 2; st > 0; st >>= 1)
#pragma unroll
            for (int j = 0; j < KCAP; j++)
                if ((j & st) == 0) {
                    const bool sw = sim_beats(s[j + st], i[j + st], s[j], i[j]);
                    const float ts = s[j]; const int ti = i[j];
                    s[j] = sw ? s[j + st] : ts; i[j] = sw ? i[j + st] : ti;
                    s[j + st] = sw ? ts : s[j + st]; i[j + st] = sw ? ti : i[j + st];
                }
    }
};

// One wave per query: lane l merges chunks l, l + 64, ..., then the 64 lists fold by halves across the wave. Lane 0 writes the k slots:
// an empty one as index -1, score 0
template <int KCAP>
__global__ __launch_bounds__(64) void sim_merge(int32_t *idx, float *score, const int2 *ws, int Q, int chunks, int k)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    SimList<KCAP> m, o;
    m.clear();
    for (int c = lane; c < chunks; c += 64) {
        const int2 *w = ws + ((size_t)c * Q + q) * k;
        o.clear();
#pragma unroll
        for (int j = 0; j < KCAP; j++)
            if (j < k) { const int2 v = w[j]; o.i[j] = v.x; o.s[j] = __int_as_float(v.y); }
        m.merge(o);
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < KCAP; j++) { o.s[j] = __shfl_xor(m.s[j], d, 64); o.i[j] = __shfl_xor(m.i[j], d, 64); }
        m.merge(o);
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < KCAP; j++)
            if (j < k) {
                const bool none = m.i[j] == SIM_EMPTY;
                idx[(size_t)q * k + j] = none ? -1 : m.i[j];
                score[(size_t)q * k + j] = none ? 0.f : m.s[j];
            }
}

}   // namespace
