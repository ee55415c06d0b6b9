// adj_true from detector labels (contract: xggm_label_cosine_table_f32 / xggm_label_adjacency_f32 in xggm.h).
//
// An image's adjacency (data/preprocess/vqa/compute_adjacency.py:38-45, :75-90) depends only on its 2 N label ids, and
// there are only Vc x Va distinct class / attribute cosines.  xggm_label_cosine_table_f32 computes them ONCE, with the
// arithmetic of the per-image kernels (preprocess.hip, graph_long.hip): each dot product and each squared norm is one
// fmaf chain over k ascending from 0.f, the quotient is dot / (max(sqrt(n2c), eps) * max(sqrt(n2a), eps)) -- so the table
// holds the bits those kernels recompute for every image.  xggm_label_adjacency_f32 then builds an image from
// N (N + 1) / 2 look-ups (label_adjacency.h).
#include "common.h"
#include "label_adjacency.h"
#include "xggm.h"

namespace {

constexpr int NT = 256, TP = 64, DC = 32, LDC = TP + 1;

// Workgroup (bx, by) owns the 64 x 64 pairs of class rows 64 bx .. and attribute rows 64 by ..; thread (ti = tid / 16,
// tj = tid % 16) the pairs (ti + 16 u, tj + 16 v), u, v < 4.  D streams through LDS in chunks of 32, transposed.
__global__ __launch_bounds__(NT) void label_cosine_table_kernel(const float* __restrict__ C, const float* __restrict__ A,
                                                                float* __restrict__ table, int Vc, int Va, int D, float eps) {
    __shared__ float cs[DC * LDC];  // cs[k][i]
    __shared__ float as[DC * LDC];  // as[k][j]
    __shared__ float nrm[2 * TP];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.x * TP, j0 = blockIdx.y * TP;
    float dot[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) dot[u][v] = 0.f;
    float n2 = 0.f;  // squared norm of class row tid (tid < 64) or attribute row tid - 64 (tid < 128) of the tile
    const float* myrow = (tid < TP ? cs : as) + (tid & (TP - 1));
    for (int k0 = 0; k0 < D; k0 += DC) {
        for (int e = tid; e < TP * (DC / 4); e += NT) {
            const int r = e / (DC / 4), c = (e % (DC / 4)) * 4;
            float4 vc = make_float4(0.f, 0.f, 0.f, 0.f), va = vc;
            if (k0 + c < D) {  // D % 4 == 0; rows past the vocabulary and columns past D are zeros: fmaf(0, 0, s) == s
                if (i0 + r < Vc) vc = *reinterpret_cast<const float4*>(C + (int64_t)(i0 + r) * D + k0 + c);
                if (j0 + r < Va) va = *reinterpret_cast<const float4*>(A + (int64_t)(j0 + r) * D + k0 + c);
            }
            cs[(c + 0) * LDC + r] = vc.x; cs[(c + 1) * LDC + r] = vc.y; cs[(c + 2) * LDC + r] = vc.z; cs[(c + 3) * LDC + r] = vc.w;
            as[(c + 0) * LDC + r] = va.x; as[(c + 1) * LDC + r] = va.y; as[(c + 2) * LDC + r] = va.z; as[(c + 3) * LDC + r] = va.w;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < DC; ++k) {  // k ascending: every pair's dot product is one fmaf chain over the embedding
            float cv[4], av[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                cv[u] = cs[k * LDC + ti + 16 * u];
                av[u] = as[k * LDC + tj + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) dot[u][v] = fmaf(cv[u], av[v], dot[u][v]);
            const float w = myrow[k * LDC];
            n2 = fmaf(w, w, n2);
        }
        __syncthreads();
    }
    if (tid < 2 * TP) nrm[tid] = fmaxf(sqrtf(n2), eps);  // torch.cosine_similarity: each norm clamped from below
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = ti + 16 * u, j = tj + 16 * v;
            if (i0 + i < Vc && j0 + j < Va) table[(int64_t)(i0 + i) * Va + j0 + j] = dot[u][v] / (nrm[i] * nrm[TP + j]);
        }
}

__global__ __launch_bounds__(NT) void label_adjacency_kernel(const float* __restrict__ table, int Vc, int Va,
                                                             const int32_t* __restrict__ obj, const int32_t* __restrict__ att,
                                                             float* __restrict__ adj, int N) {
    __shared__ label_adj::Smem sm;
    const int64_t b = blockIdx.x;
    label_adj::image<NT>(table, Vc, Va, obj + b * N, att + b * N, adj + b * N * N, N, sm);
}

bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p % n) != 0; }
}  // namespace

extern "C" int xggm_label_cosine_table_f32(const float* cls, const float* attr, float* table, int Vc, int Va, int D, float eps,
                                           hipStream_t st) {
    const char* who = "xggm_label_cosine_table_f32";
    XGGM_REQUIRE(cls && attr && table, "%s: null pointer (cls, attr, table)", who);
    XGGM_REQUIRE(Vc > 0 && Va > 0, "%s: Vc=%d Va=%d labels, at least one of each expected", who, Vc, Va);
    XGGM_REQUIRE(Va <= 65535 * TP, "%s: Va=%d exceeds the grid's %d attribute rows", who, Va, 65535 * TP);
    XGGM_REQUIRE(D > 0 && D % 4 == 0, "%s: embedding width %d must be a multiple of 4", who, D);
    XGGM_REQUIRE(!misaligned(cls, 16) && !misaligned(attr, 16), "%s: embeddings must be 16-byte aligned", who);
    XGGM_REQUIRE(!misaligned(table, 4), "%s: the table must be 4-byte aligned", who);
    hipLaunchKernelGGL(label_cosine_table_kernel, dim3(ceil_div(Vc, TP), ceil_div(Va, TP)), dim3(NT), 0, st, cls, attr, table, Vc,
                       Va, D, eps);
    return xggm_check_launch(who);
}

extern "C" int xggm_label_adjacency_f32(const float* table, int Vc, int Va, const int32_t* obj_labels, const int32_t* attr_labels,
                                        float* adj, int n, int N, hipStream_t st) {
    const char* who = "xggm_label_adjacency_f32";
    XGGM_REQUIRE(table && obj_labels && attr_labels && adj, "%s: null pointer (table, obj_labels, attr_labels, adj)", who);
    XGGM_REQUIRE(Vc > 0 && Va > 0, "%s: Vc=%d Va=%d labels, at least one of each expected", who, Vc, Va);
    XGGM_REQUIRE(n > 0, "%s: n=%d images", who, n);
    XGGM_REQUIRE(N >= 1 && N <= label_adj::N_MAX, "%s: N = %d objects (1..%d)", who, N, label_adj::N_MAX);
    XGGM_REQUIRE(!misaligned(table, 4) && !misaligned(obj_labels, 4) && !misaligned(attr_labels, 4) && !misaligned(adj, 4),
                 "%s: a 4-byte field is misaligned", who);
    hipLaunchKernelGGL(label_adjacency_kernel, dim3(n), dim3(NT), 0, st, table, Vc, Va, obj_labels, attr_labels, adj, N);
    return xggm_check_launch(who);
}
