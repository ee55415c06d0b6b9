// adj_true of ONE image from its 2 N detector label ids and the class x attribute cosine table (contract:
// xggm_label_adjacency_f32 in xggm.h).  One workgroup per image; shared by the split builder (label_adjacency.hip) and by
// role 1 of the batch gather (batch_gather.hip), so both write the same bits.
// The finishing steps are those of cosine_adj_kernel (preprocess.hip) and cosine_adj_long_kernel (graph_long.hip), word
// for word: c[i][j] = table[obj_i][attr_j] for j >= i, c + c on the diagonal and c + 0.f off it, the maximum by fmaxf,
// every value divided by it, written to [i][j] and [j][i].  The values are looked up twice (maximum, then output) rather
// than kept: 16 KB of LDS or 64 registers per thread at N = 128 would be the gather kernel's, feature roles included,
// while the 2.56 MB table of the published vocabularies stays in L2.
#pragma once
#include "common.h"

namespace label_adj {

constexpr int N_MAX = 128;

struct Smem {
    int32_t lab[2 * N_MAX];  // class ids, then (at N) attribute ids
    float red[16];
    int bad;
};

__device__ __forceinline__ float pair_value(const float* __restrict__ table, int Va, const Smem& sm, int N, int i, int j) {
    const float c = table[(int64_t)sm.lab[i] * Va + sm.lab[N + j]];  // j >= i
    return i == j ? c + c : c + 0.f;
}

// Call from every thread of a workgroup of NT threads (barriers inside); 1 <= N <= N_MAX.  An id outside [0, Vc) /
// [0, Va) is never used as an index: the whole image becomes NaN.
template <int NT>
__device__ __forceinline__ void image(const float* __restrict__ table, int Vc, int Va, const int32_t* __restrict__ obj,
                                      const int32_t* __restrict__ att, float* __restrict__ out, int N, Smem& sm) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) sm.bad = 0;
    __syncthreads();
    for (int t = tid; t < 2 * N; t += NT) {
        const int v = t < N ? obj[t] : att[t - N];
        sm.lab[t] = v;
        if (v < 0 || v >= (t < N ? Vc : Va)) sm.bad = 1;  // every writer stores the same value
    }
    __syncthreads();
    const int nn = N * N;
    if (sm.bad) {  // uniform
        for (int e = tid; e < nn; e += NT) out[e] = __builtin_nanf("");
        return;
    }
    float mx = -INFINITY;
    for (int e = tid; e < nn; e += NT) {
        const int i = e / N, j = e - i * N;
        if (j >= i) mx = fmaxf(mx, pair_value(table, Va, sm, N, i, j));
    }
    mx = wave_max(mx);
    if (lane == 0) sm.red[wid] = mx;
    __syncthreads();
    mx = sm.red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) mx = fmaxf(mx, sm.red[w]);
    // element e = (i, j) takes the pair (min, max): [i][j] and [j][i] hold the same quotient, stores stay coalesced
    for (int e = tid; e < nn; e += NT) {
        const int i = e / N, j = e - i * N;
        out[e] = pair_value(table, Va, sm, N, min(i, j), max(i, j)) / mx;
    }
}

}  // namespace label_adj
