// The graph kernels of graph.hip, gat.hip and preprocess.hip for 64 < N <= 128 objects (100-box features, the 128-object
// limit of the encoder).  The 64-object files are untouched: at N <= 64 every launch and every bit stays as it was, and
// these entry points refuse N <= 64 as those refuse N > 64.  Adjacency-shaped tensors are fp32, node features are T.
//
// What changes at 128 is the layout, not the arithmetic: a row or column of the adjacency no longer fits one lane per
// neighbour, and an N x N fp32 tile (66 KB padded) no longer fits in static LDS beside anything else.
//
//   xggm_aggregate_long   out = [out +] self*x + scale * M' @ x     M' = M | M^T | M + M^T
//                         GCNConv aggregate (src/module/gcn.py:28), GIN aggregate (src/module/gin.py:32) and every
//                         backward-through-x of them and of S = x x^T.
//                         CHOSEN: the neighbour dimension runs in two 64-wide halves and the accumulators stay in
//                         registers (acc[NI] of four floats per lane, NI = ceil(N / 16) <= 8: rows are padded to the next
//                         multiple of 16 only, N = 100 runs 7 row tiles).  Per half the LDS holds M'[:, 64 h .. 64 h + 63]
//                         and the x slab [64, 64]; x is read from HBM once, out written once (16-byte stores for fp32, 8-byte
//                         for bf16).  fp32: v_mfma_f32_16x16x4_f32, exact in fp32 storage.  bf16: M' = hi + lo, two bf16 terms
//                         (16 mantissa bits), the adjacency is never rounded to bf16; v_mfma_f32_16x16x32_bf16.
//                         -Rpass-analysis=kernel-resource-usage (gfx950, NI = 8):
//                           aggregate_long_kernel<float, 8>   VGPRs 76, AGPRs 36, scratch 0, LDS 54272 B, occupancy 3 waves/SIMD
//                           aggregate_long_kernel<float, 7>   VGPRs 70, AGPRs 32, scratch 0, LDS 50048 B, occupancy 3   (N = 100)
//                           aggregate_long_bf16_kernel<8>     VGPRs 82, AGPRs 32, scratch 0, LDS 46080 B, occupancy 3
//                           aggregate_long_bf16_kernel<7>     VGPRs 80, AGPRs 28, scratch 0, LDS 41472 B, occupancy 3   (N = 100)
//                         (the occupancy is the LDS's: two to three workgroups of four waves per CU, as the 64-object kernels;
//                         every other kernel of this file: scratch 0 as well, at most 82 VGPRs.)
//   xggm_agg_dot_long     d eps of GIN: sum dh * (M @ x), the output rows in two halves of 64 (the [N][64] slice of M^T in LDS,
//                         64 accumulators per thread), then the same ordered grid sum as the short kernel.
//   xggm_adj_regen_long_fwd/bwd  column-max normalisation + sigmoid + zero diagonal of S = x x^T
//                         (src/module/graph_generative_modeling.py:225-228).  Column i is scanned by two threads, rows
//                         0..63 and 64..N-1, each in ascending order with a strict '>' (first index wins inside a half); the
//                         halves meet through LDS and the upper one wins only if strictly larger (first index wins across
//                         rows 63 / 64 as well): torch.max(dim=1).  Reads are coalesced along the column index; nothing
//                         N x N lives in LDS.
//   xggm_adj_init_long_fwd/bwd  encoder_adj scatter into the strict upper triangle, symmetrise, symmetric Gaussian noise,
//                         grad_log_noise (src/vqa/vqacpv2.py:195-202 + src/module/graph_utils.py:162-168); the same triu
//                         enumeration (xggm_triu_index).
//   xggm_gat_att_long_fwd/bwd  GATConv attention (src/module/gat.py:25-49): one wave per softmax row, two entries per lane
//                         (j = lane, lane + 64); backward column sums by two threads per column, rows ascending in each
//                         half, lower half + upper half.
//   xggm_cosine_adjacency_long_f32  data/preprocess/vqa/compute_adjacency.py:38-45 + :90.  One workgroup per image, every
//                         thread owns an 8 x 8 register tile of the 128 x 128 pairs (rows ti + 16 u, columns tj + 16 v); the
//                         embeddings stream through LDS transposed in 32-wide chunks (33 KB instead of the 200 KB the short
//                         layout would need).  The thread that holds c[i][j], j >= i, writes both a[i][j] and a[j][i]: no
//                         N x N exchange.
// Every sum runs in an order fixed by the code (k ascending inside an MFMA chain or an fmaf chain, wave_sum's fixed
// tree, waves in index order); no floating-point atomics; every load and store is bounded element-wise.
#include "common.h"
#include "xggm.h"

namespace {

constexpr int NT = 256;
constexpr int NL_MIN = 65, NL_MAX = 128;  // objects these entry points take
constexpr int KH = 64;                        // neighbours per half

#define XGGM_LONG_N(name, N)                                                                                      \
    XGGM_REQUIRE((N) >= NL_MIN && (N) <= NL_MAX, "%s: N=%d is outside 65..128 (N <= 64 is the short entry point's)", \
                 name, (N))

inline int grid1d(int64_t n) { return (int)std::min<int64_t>(ceil_div64(n, NT), 2048); }

// ------------------------------------------------------------------------------- aggregate, fp32 matrix cores
// One workgroup = one sample x 64 feature columns, wave w owns columns 16 w .. 16 w + 15 and all NI row tiles.  As in
// aggregate_kernel the operands are swapped (D^T = x^T M'^T): a lane ends with FOUR CONSECUTIVE columns of one row.
typedef __attribute__((ext_vector_type(4))) float float4_t;
constexpr int AGG_COLS = 64, AGG_LDX = 80;
template <typename T, int NI>
__global__ __launch_bounds__(NT) void aggregate_long_kernel(const float* __restrict__ Mx, const T* __restrict__ x, T* out, int N,
                                                            int H, int mode, float scale, const float* scale_ptr, float self_w,
                                                            int accumulate) {
    constexpr int NR = NI * 16, LDM = KH + 2;
    __shared__ float Mp[NR * LDM];      // Mp[i][jj] = M'[i][64 h + jj]
    __shared__ __attribute__((aligned(16))) float xs[KH * AGG_LDX];  // xs[jj][c] = x[64 h + jj][cb + c]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cb = blockIdx.x * AGG_COLS;
    const float* Mb = Mx + (int64_t)b * N * N;
    const T* xb = x + (int64_t)b * N * H + cb;
    const int fr = lane & 15, fq = lane >> 4, c0 = wid * 16;
    float4_t acc[NI], sx[NI];
#pragma unroll
    for (int t = 0; t < NI; ++t) acc[t] = sx[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k0 = h * KH;
        if (h) __syncthreads();  // the first half's fragment reads are done
        if (mode == XGGM_AGG_TRANSPOSE) {  // i fastest: the reads of M[j][i] are coalesced
            for (int e = tid; e < NR * KH; e += NT) {
                const int i = e % NR, jj = e / NR, j = k0 + jj;
                Mp[i * LDM + jj] = (i < N && j < N) ? Mb[j * N + i] : 0.f;
            }
        } else {
            for (int e = tid; e < NR * KH; e += NT) {
                const int i = e / KH, jj = e % KH, j = k0 + jj;
                float v = 0.f;
                if (i < N && j < N) {
                    v = Mb[i * N + j];
                    if (mode == XGGM_AGG_SYMMETRIZE) v += Mb[j * N + i];
                }
                Mp[i * LDM + jj] = v;
            }
        }
        for (int e = tid; e < KH * (AGG_COLS / 4); e += NT) {  // 4 columns per thread
            const int jj = e / (AGG_COLS / 4), c = (e % (AGG_COLS / 4)) * 4, j = k0 + jj;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (j < N && cb + c < H) load4(xb + (int64_t)j * H + c, v);  // H % 4 == 0
            *reinterpret_cast<float4*>(xs + jj * AGG_LDX + c) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        const int kend = min(KH, (N - k0 + 3) & ~3);  // (neighbours beyond N are zero in LDS; whole steps of them are skipped)
        for (int j0 = 0; j0 < kend; j0 += 4) {
            const float xa = xs[(j0 + fq) * AGG_LDX + c0 + fr];  // A operand: x^T, row = column c0 + fr, k = j0 + fq
#pragma unroll
            for (int t = 0; t < NI; ++t)                          // B operand: M'^T, k = j0 + fq, column = row t*16 + fr
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, Mp[(t * 16 + fr) * LDM + j0 + fq], acc[t], 0, 0, 0);
        }
        if (self_w != 0.f) {  // the self term's x rows are those of the half they sit in
#pragma unroll
            for (int t = 0; t < NI; ++t)
                if (t / 4 == h) sx[t] = *reinterpret_cast<const float4_t*>(xs + (t * 16 + fr - k0) * AGG_LDX + c0 + 4 * fq);
        }
    }
    if (scale_ptr) scale *= (1.0f + *scale_ptr);  // GIN: (1 + eps)
    // lane holds out[i = t*16 + fr][c = c0 + 4 fq .. + 3]
    const int c = cb + c0 + 4 * fq;
    if (c >= H) return;
    T* ob = out + (int64_t)b * N * H + c;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
        const int i = t * 16 + fr;
        if (i < N) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = scale * acc[t][r];
            if (self_w != 0.f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += self_w * sx[t][r];
            }
            if (accumulate) {
                float o[4];
                load4(ob + (int64_t)i * H, o);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += o[r];
            }
            store4(ob + (int64_t)i * H, v);
        }
    }
}

// ---- bf16 storage: the same product on the bf16 matrix cores, M' = hi + lo as in aggregate_bf16_kernel ---------------
//   x half-slab [64, 64] bf16 by 16-byte loads -> LDS [k = jj][n = c] (row stride 72), read transposed
//   (ds_read_b64_tr_b16) as the A operand x^T; M' goes from global (L2: the column blocks of a sample run on one XCD)
//   straight to hi / lo [i][k = jj] (row stride 72), read by rows (ds_read_b128) as the B operand M'^T.
typedef __attribute__((ext_vector_type(8))) short agg_short8;
typedef __attribute__((ext_vector_type(4))) short agg_short4;
typedef __attribute__((ext_vector_type(8))) __bf16 agg_bf16x8;
template <int NI>
__global__ __launch_bounds__(NT) void aggregate_long_bf16_kernel(const float* __restrict__ Mx, const bf16* __restrict__ x,
                                                                 bf16* out, int B, int N, int H, int mode, float scale,
                                                                 const float* scale_ptr, float self_w, int accumulate) {
    constexpr int NR = NI * 16, LDX = 72, LDM = 72;
    __shared__ __attribute__((aligned(16))) bf16 xs[KH * LDX];
    __shared__ __attribute__((aligned(16))) bf16 Mh[NR * LDM];
    __shared__ __attribute__((aligned(16))) bf16 Ml[NR * LDM];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ncb = (H + AGG_COLS - 1) / AGG_COLS;
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int b = (q / ncb) * 8 + xcd, cb = (q % ncb) * AGG_COLS;
    if (b >= B) return;  // (whole workgroup: the padding blocks of a batch that is not a multiple of 8)
    const float* Mb = Mx + (int64_t)b * N * N;
    const bf16* xb = x + (int64_t)b * N * H + cb;
    const int fr = lane & 15, fq = lane >> 4, c0 = wid * 16;
    float4_t acc[NI], sx[NI];
#pragma unroll
    for (int t = 0; t < NI; ++t) acc[t] = sx[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k0 = h * KH;
        if (h) __syncthreads();  // the first half's fragment reads are done
        for (int e = tid; e < KH * 8; e += NT) {  // 8 chunks of 8 columns per k-row
            const int jj = e >> 3, c = (e & 7) * 8, j = k0 + jj;
            agg_short8 v = {};
            if (j < N && cb + c + 8 <= H) v = *reinterpret_cast<const agg_short8*>(xb + (int64_t)j * H + c);  // H % 8 == 0 here
            *reinterpret_cast<agg_short8*>(xs + jj * LDX + c) = v;
        }
        for (int e = tid; e < NR * KH / 4; e += NT) {  // four consecutive k per thread: 8-byte LDS stores
            int i, jj0;
            if (mode == XGGM_AGG_TRANSPOSE) {  // i fastest: the reads of M[j][i] are coalesced
                i = e % NR;
                jj0 = 4 * (e / NR);
            } else {
                i = (4 * e) / KH;
                jj0 = (4 * e) % KH;
            }
            agg_short4 h4, l4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = k0 + jj0 + u;
                float v = 0.f;
                if (i < N && j < N) {
                    if (mode == XGGM_AGG_PLAIN) v = Mb[i * N + j];
                    else if (mode == XGGM_AGG_TRANSPOSE) v = Mb[j * N + i];
                    else v = Mb[i * N + j] + Mb[j * N + i];
                }
                const bf16 hi = __float2bfloat16(v);
                h4[u] = __builtin_bit_cast(short, hi);
                l4[u] = __builtin_bit_cast(short, __float2bfloat16(v - __bfloat162float(hi)));
            }
            *reinterpret_cast<agg_short4*>(Mh + i * LDM + jj0) = h4;
            *reinterpret_cast<agg_short4*>(Ml + i * LDM + jj0) = l4;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KH; ks += 32) {
            if (k0 + ks >= N) continue;  // (uniform: a whole step of neighbours beyond N)
            // A operand x^T: lane (fr, fq) gets column c0 + fr, k = ks + 8 fq .. + 7 through two transposing reads
            const int qq = fr >> 2, pp = fr & 3;
            const bf16* a0 = xs + (ks + 8 * fq + qq) * LDX + c0 + 4 * pp;
            const agg_short4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) agg_short4*)(a0));
            const agg_short4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) agg_short4*)(a0 + 4 * LDX));
            agg_short8 av;
            av[0] = lo4[0]; av[1] = lo4[1]; av[2] = lo4[2]; av[3] = lo4[3];
            av[4] = hi4[0]; av[5] = hi4[1]; av[6] = hi4[2]; av[7] = hi4[3];
            const agg_bf16x8 a = __builtin_bit_cast(agg_bf16x8, av);
#pragma unroll
            for (int t = 0; t < NI; ++t) {
                const agg_bf16x8 bh = __builtin_bit_cast(agg_bf16x8, *reinterpret_cast<const agg_short8*>(Mh + (t * 16 + fr) * LDM + ks + fq * 8));
                const agg_bf16x8 bl = __builtin_bit_cast(agg_bf16x8, *reinterpret_cast<const agg_short8*>(Ml + (t * 16 + fr) * LDM + ks + fq * 8));
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bl, acc[t], 0, 0, 0);
            }
        }
        if (self_w != 0.f) {  // the self term's x rows are those of the half they sit in
#pragma unroll
            for (int t = 0; t < NI; ++t)
                if (t / 4 == h) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sx[t][r] = __bfloat162float(xs[(t * 16 + fr - k0) * LDX + c0 + 4 * fq + r]);
                }
        }
    }
    if (scale_ptr) scale *= (1.0f + *scale_ptr);  // GIN: (1 + eps)
    // lane holds out[i = t*16 + fr][c = c0 + 4 fq .. + 3]
    const int c = cb + c0 + 4 * fq;
    if (c >= H) return;
    bf16* ob = out + (int64_t)b * N * H + c;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
        const int i = t * 16 + fr;
        if (i < N) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = scale * acc[t][r];
            if (self_w != 0.f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += self_w * sx[t][r];
            }
            if (accumulate) {
                float o[4];
                load4(ob + (int64_t)i * H, o);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += o[r];
            }
            store4(ob + (int64_t)i * H, v);
        }
    }
}

// d eps of GIN: sum_{b,i,c} dh[b,i,c] * (A @ x)[b,i,c]  -> one scalar.  Each thread owns one feature column; the output
// rows run in two halves of 64 (64 accumulators per thread, Mt[j][il] = A[64 ih + il][j] in LDS, row stride 65).
template <typename T>
__global__ __launch_bounds__(NT) void agg_dot_long_kernel(const float* __restrict__ Mx, const T* __restrict__ x,
                                                          const T* __restrict__ dh, float* out, int N, int H, float* ws) {
    constexpr int LDT = KH + 1;
    __shared__ float Mt[NL_MAX * LDT];
    __shared__ float red[NT / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* Mb = Mx + (int64_t)b * N * N;
    const int c = blockIdx.x * NT + tid;
    const T* xb = x + (int64_t)b * N * H + c;
    const T* db = dh + (int64_t)b * N * H + c;
    float total = 0.f;
#pragma unroll 1
    for (int ih = 0; ih < 2; ++ih) {
        const int i0 = ih * KH;
        if (ih) __syncthreads();
        for (int e = tid; e < KH * NL_MAX; e += NT) {
            const int il = e / NL_MAX, j = e % NL_MAX;
            Mt[j * LDT + il] = (i0 + il < N && j < N) ? Mb[(i0 + il) * N + j] : 0.f;
        }
        __syncthreads();
        if (c < H) {
            float acc[KH];
#pragma unroll
            for (int il = 0; il < KH; ++il) acc[il] = 0.f;
            for (int j = 0; j < N; ++j) {
                const float xj = to_f32(xb[(int64_t)j * H]);
#pragma unroll
                for (int il = 0; il < KH; ++il) acc[il] += Mt[j * LDT + il] * xj;
            }
#pragma unroll
            for (int il = 0; il < KH; ++il)
                if (i0 + il < N) total += acc[il] * to_f32(db[(int64_t)(i0 + il) * H]);
        }
    }
    total = wave_sum(total);
    if ((tid & 63) == 0) red[tid >> 6] = total;
    __syncthreads();
    // the workgroups' sums are added in index order by the one that finishes last (ordered_grid_sum): no float atomics
    float sum;
    if (ordered_grid_sum((red[0] + red[1]) + (red[2] + red[3]), ws, gridDim.x * gridDim.y, blockIdx.y * gridDim.x + blockIdx.x, sum))
        *out += sum;
}

// ------------------------------------------------------------------------------- adjacency regeneration
// one workgroup per sample.  Thread (i = tid & 127, hh = tid >> 7) scans rows 64 hh .. of column i.
__global__ __launch_bounds__(NT) void adj_regen_long_fwd_kernel(const float* __restrict__ S, float* adj, float* colmax,
                                                                int32_t* argmax, int N) {
    __shared__ float hm[2 * NL_MAX];
    __shared__ int ha[2 * NL_MAX];
    __shared__ float mx[NL_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int i = tid & (NL_MAX - 1), hh = tid >> 7;
    const float* Sb = S + (int64_t)b * N * N;
    if (i < N) {
        // max over rows r of S[r][i]; torch.max(dim=1) returns the FIRST arg-max on ties: ascending rows, strict '>'
        const int r0 = hh * KH, r1 = hh ? N : KH;
        float m = Sb[r0 * N + i];
        int a = r0;
        for (int r = r0 + 1; r < r1; ++r) {
            const float v = Sb[r * N + i];
            if (v > m) {
                m = v;
                a = r;
            }
        }
        hm[hh * NL_MAX + i] = m;
        ha[hh * NL_MAX + i] = a;
    }
    __syncthreads();
    if (tid < N) {
        float m = hm[tid];
        int a = ha[tid];
        if (hm[NL_MAX + tid] > m) {  // the upper half only if strictly larger
            m = hm[NL_MAX + tid];
            a = ha[NL_MAX + tid];
        }
        mx[tid] = m;
        colmax[(int64_t)b * N + tid] = m;
        argmax[(int64_t)b * N + tid] = a;
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += NT) {
        const int r = e / N, j = e % N;
        adj[(int64_t)b * N * N + e] = (r == j) ? 0.f : sigmoid_f(Sb[e] / mx[r]);
    }
}

// dS from d_adj:  R = S[i][j]/m_i, A = sigmoid(R) off-diagonal;  dR = dA * A (1 - A);
// dS[i][j] = dR/m_i;  dm_i = -sum_j dR[i][j] S[i][j] / m_i^2;  dS[argmax_i][i] += dm_i
// Pass 1: one wave per row i, two entries per lane, dm_i to LDS.  Pass 2: every element once, with dm_j added where
// argmax_j == i (a single store per element, no read-modify-write).
__global__ __launch_bounds__(NT) void adj_regen_long_bwd_kernel(const float* __restrict__ d_adj, const float* __restrict__ S,
                                                                const float* __restrict__ adj, const float* __restrict__ colmax,
                                                                const int32_t* __restrict__ argmax, float* dS, int N) {
    __shared__ float dm[NL_MAX], ms[NL_MAX];
    __shared__ int am[NL_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t ob = (int64_t)b * N * N;
    if (tid < N) {
        ms[tid] = colmax[(int64_t)b * N + tid];
        am[tid] = argmax[(int64_t)b * N + tid];
    }
    for (int i = wid; i < N; i += NT / 64) {
        const float m = colmax[(int64_t)b * N + i];
        float part = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            if (j < N && j != i) {
                const int e = i * N + j;
                const float a = adj[ob + e];
                part += d_adj[ob + e] * a * (1.f - a) * S[ob + e];
            }
        }
        part = wave_sum(part);  // (lane's lower entry + upper entry), then the fixed tree over the lanes
        if (lane == 0) dm[i] = -part / (m * m);
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += NT) {
        const int i = e / N, j = e % N;
        const float a = adj[ob + e];
        const float dr = (i == j) ? 0.f : d_adj[ob + e] * a * (1.f - a);
        float v = dr / ms[i];
        if (am[j] == i) v += dm[j];
        dS[ob + e] = v;
    }
}

// ------------------------------------------------------------------------------- adjacency init + edge noise
// k-th strict-upper-triangle entry in row-major order: (0,1),(0,2)...(0,N-1),(1,2)...  (the enumeration of graph.hip)
__host__ __device__ inline int triu_k(int i, int j, int N) { return i * N - (i * (i + 1)) / 2 + (j - i - 1); }

__global__ __launch_bounds__(NT) void adj_init_long_fwd_kernel(const float* __restrict__ e, const float* __restrict__ randn,
                                                               float* adj, float* gradlog, int B, int N, int NE, float sigma,
                                                               const uint64_t* rng, uint32_t sid) {
    const int64_t total = (int64_t)B * N * N;
    uint64_t seed = 0, off = 0;
    if (!randn && rng) {
        seed = rng[0];
        off = rng[1];
    }
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
        const int b = (int)(t / (N * N)), r = (int)(t % (N * N)), i = r / N, j = r % N;
        float a = 0.f, n = 0.f;
        if (i != j) {
            const int lo = min(i, j), hi = max(i, j);
            if (e) a = e[(int64_t)b * NE + triu_k(lo, hi, N)];
            const int64_t uidx = ((int64_t)b * N + lo) * N + hi;  // the upper-triangle draw is mirrored
            const float z = randn ? randn[uidx] : (rng ? philox_normal(seed, off, sid, (uint64_t)uidx) : 0.f);
            n = z * sigma;
        }
        adj[t] = a + n;
        if (gradlog) gradlog[t] = -n / (sigma * sigma);
    }
}

// one thread per (sample, row i, column j > i): k = triu_k(i, j), no inversion of the enumeration
__global__ __launch_bounds__(NT) void adj_init_long_bwd_kernel(const float* __restrict__ d_adj, float* d_e, int B, int N, int NE) {
    const int64_t total = (int64_t)B * N * N;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < total; t += (int64_t)gridDim.x * NT) {
        const int b = (int)(t / (N * N)), r = (int)(t % (N * N)), i = r / N, j = r % N;
        if (j <= i) continue;
        const float* g = d_adj + (int64_t)b * N * N;
        d_e[(int64_t)b * NE + triu_k(i, j, N)] = g[i * N + j] + g[j * N + i];
    }
}

// ------------------------------------------------------------------------------- graph attention
// s: [B*N, 2] fp32 (s1 = col 0, s2 = col 1); adj fp32 [B,N,N]; att out fp32 [B,N,N].  One wave per row, j = lane, lane + 64.
__global__ __launch_bounds__(NT) void gat_att_long_fwd_kernel(const float* __restrict__ s, const float* __restrict__ adj,
                                                              float* att, int B, int N, float alpha) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int rows = B * N;
    for (int r = blockIdx.x * 4 + wid; r < rows; r += gridDim.x * 4) {
        const int b = r / N;
        const float s1 = s[2 * r];
        float v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            v[u] = -INFINITY;
            if (j < N) {
                const float raw = s1 + s[2 * (b * N + j) + 1];
                v[u] = raw > 0.f ? raw : alpha * raw;
                if (adj[(int64_t)r * N + j] == 0.f) v[u] = -9e15f;  // a fully masked row comes out uniform, as in the reference
            }
        }
        const float m = wave_max(fmaxf(v[0], v[1]));
        const float e0 = __expf(v[0] - m);                       // lane < 64 < N
        const float e1 = lane + 64 < N ? __expf(v[1] - m) : 0.f;
        const float sum = wave_sum(e0 + e1);
        att[(int64_t)r * N + lane] = e0 / sum;
        if (lane + 64 < N) att[(int64_t)r * N + lane + 64] = e1 / sum;
    }
}

// d_att -> ds [B*N, 2] (T).  One workgroup per sample.  Pass 1: one wave per row -- dot_i = sum_j att da (to LDS) and
// the row sum ds1_i.  Pass 2: thread (j = tid & 127, hh = tid >> 7) adds column j's entries over rows 64 hh .., ascending;
// ds2_j = lower half + upper half.
template <typename T>
__global__ __launch_bounds__(NT) void gat_att_long_bwd_kernel(const float* __restrict__ d_att, const float* __restrict__ att,
                                                              const float* __restrict__ s, const float* __restrict__ adj, T* ds,
                                                              int N, float alpha) {
    __shared__ float dots[NL_MAX], s1s[NL_MAX], half[2 * NL_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int i = wid; i < N; i += NT / 64) {
        const int r = b * N + i;
        const float s1 = s[2 * r];
        float a[2] = {0.f, 0.f}, da[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            if (j < N) {
                a[u] = att[(int64_t)r * N + j];
                da[u] = d_att[(int64_t)r * N + j];
            }
        }
        const float dot = wave_sum(a[0] * da[0] + a[1] * da[1]);
        float de = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = lane + 64 * u;
            if (j < N && adj[(int64_t)r * N + j] != 0.f) {
                const float raw = s1 + s[2 * (b * N + j) + 1];
                de += a[u] * (da[u] - dot) * (raw > 0.f ? 1.f : alpha);
            }
        }
        const float rs = wave_sum(de);
        if (lane == 0) {
            ds[2 * (int64_t)r] = from_f32<T>(rs);
            dots[i] = dot;
            s1s[i] = s1;
        }
    }
    __syncthreads();
    const int j = tid & (NL_MAX - 1), hh = tid >> 7;
    float cs = 0.f;
    if (j < N) {
        const float s2 = s[2 * (b * N + j) + 1];
        const int i1 = hh ? N : KH;
        for (int i = hh * KH; i < i1; ++i) {
            const int64_t e = (int64_t)(b * N + i) * N + j;
            if (adj[e] != 0.f) {
                const float raw = s1s[i] + s2;
                cs += att[e] * (d_att[e] - dots[i]) * (raw > 0.f ? 1.f : alpha);
            }
        }
    }
    half[tid] = cs;
    __syncthreads();
    if (tid < N) ds[2 * ((int64_t)b * N + tid) + 1] = from_f32<T>(half[tid] + half[NL_MAX + tid]);
}

// ------------------------------------------------------------------------------- cosine adjacency
// One workgroup per image.  Thread (ti = tid / 16, tj = tid % 16) owns pairs (i = ti + 16 u, j = tj + 16 v), u, v < 8.
constexpr int DC = 32, LDC = NL_MAX + 1;
__global__ __launch_bounds__(NT) void cosine_adj_long_kernel(const float* __restrict__ C, const float* __restrict__ A, float* out,
                                                             int N, int D, float eps) {
    __shared__ float cs[DC * LDC];  // cs[k][i]: class embeddings of the chunk, transposed
    __shared__ float as[DC * LDC];  // as[k][j]: attribute embeddings
    __shared__ float nrm[2 * NL_MAX];
    __shared__ float red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ti = tid >> 4, tj = tid & 15;
    const float* Cb = C + (int64_t)blockIdx.x * N * D;
    const float* Ab = A + (int64_t)blockIdx.x * N * D;
    float dot[8][8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) dot[u][v] = 0.f;
    float n2 = 0.f;  // squared norm of row tid & 127 of the class (tid < 128) or attribute (tid >= 128) embeddings
    const float* myrow = (tid < NL_MAX ? cs : as) + (tid & (NL_MAX - 1));
    for (int k0 = 0; k0 < D; k0 += DC) {
        for (int e = tid; e < NL_MAX * (DC / 4); e += NT) {
            const int r = e / (DC / 4), c = (e % (DC / 4)) * 4;
            float4 vc = make_float4(0.f, 0.f, 0.f, 0.f), va = vc;
            if (r < N && k0 + c < D) {  // D % 4 == 0
                vc = *reinterpret_cast<const float4*>(Cb + (int64_t)r * D + k0 + c);
                va = *reinterpret_cast<const float4*>(Ab + (int64_t)r * D + k0 + c);
            }
            cs[(c + 0) * LDC + r] = vc.x; cs[(c + 1) * LDC + r] = vc.y; cs[(c + 2) * LDC + r] = vc.z; cs[(c + 3) * LDC + r] = vc.w;
            as[(c + 0) * LDC + r] = va.x; as[(c + 1) * LDC + r] = va.y; as[(c + 2) * LDC + r] = va.z; as[(c + 3) * LDC + r] = va.w;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < DC; ++k) {  // k ascending: every pair's dot product is one fmaf chain over the embedding
            float cv[8], av[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                cv[u] = cs[k * LDC + ti + 16 * u];
                av[u] = as[k * LDC + tj + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int v = 0; v < 8; ++v) dot[u][v] = fmaf(cv[u], av[v], dot[u][v]);
            const float w = myrow[k * LDC];
            n2 = fmaf(w, w, n2);
        }
        __syncthreads();
    }
    nrm[tid] = fmaxf(sqrtf(n2), eps);  // torch.cosine_similarity: each norm clamped from below (rows >= N: eps, unused)
    __syncthreads();
    // c[i][j] = cos for j >= i, 0 below; a = c + c^T: a[i][j] = a[j][i] = c[i][j] (i < j), a[i][i] = 2 c[i][i]
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int i = ti + 16 * u, j = tj + 16 * v;
            if (i < N && j < N && j >= i) {
                const float cv = dot[u][v] / (nrm[i] * nrm[NL_MAX + j]);
                dot[u][v] = i == j ? cv + cv : cv + 0.f;
                mx = fmaxf(mx, dot[u][v]);
            }
        }
    mx = wave_max(mx);
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float* ob = out + (int64_t)blockIdx.x * N * N;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int i = ti + 16 * u, j = tj + 16 * v;
            if (i < N && j < N && j >= i) {
                const float o = dot[u][v] / mx;
                ob[i * N + j] = o;
                if (j != i) ob[j * N + i] = o;
            }
        }
}

// ------------------------------------------------------------------------------- host side
template <typename T>
int aggregate_long(const char* name, const float* M, const void* x, void* out, int B, int N, int H, int mode, float scale,
                   const float* scale_ptr, float self_w, int accumulate, hipStream_t st) {
    XGGM_REQUIRE(M && x && out && B > 0 && H > 0, "%s: bad arguments", name);
    XGGM_LONG_N(name, N);
    XGGM_REQUIRE(mode >= 0 && mode <= XGGM_AGG_SYMMETRIZE, "%s: bad mode %d", name, mode);
    XGGM_REQUIRE(B <= 65535, "%s: batch too large", name);
    XGGM_REQUIRE(H % 4 == 0, "%s: H=%d must be a multiple of 4", name, H);
    const int ni = ceil_div(N, 16);  // 5 .. 8
#define AGG_LONG_CASE(K, NI, ...)                                                       \
    case NI:                                                                            \
        hipLaunchKernelGGL((K), __VA_ARGS__);                                           \
        break;
    if constexpr (sizeof(T) == 2) {
        // bf16 storage, 8-aligned rows: bf16 matrix cores with the adjacency split into hi + lo
        if (H % 8 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0) {
            const dim3 g8(ceil_div(B, 8) * 8 * ceil_div(H, AGG_COLS));
            switch (ni) {
                AGG_LONG_CASE(aggregate_long_bf16_kernel<5>, 5, g8, dim3(NT), 0, st, M, (const bf16*)x, (bf16*)out, B, N, H, mode, scale, scale_ptr, self_w, accumulate)
                AGG_LONG_CASE(aggregate_long_bf16_kernel<6>, 6, g8, dim3(NT), 0, st, M, (const bf16*)x, (bf16*)out, B, N, H, mode, scale, scale_ptr, self_w, accumulate)
                AGG_LONG_CASE(aggregate_long_bf16_kernel<7>, 7, g8, dim3(NT), 0, st, M, (const bf16*)x, (bf16*)out, B, N, H, mode, scale, scale_ptr, self_w, accumulate)
                AGG_LONG_CASE(aggregate_long_bf16_kernel<8>, 8, g8, dim3(NT), 0, st, M, (const bf16*)x, (bf16*)out, B, N, H, mode, scale, scale_ptr, self_w, accumulate)
            }
            return xggm_check_launch(name);
        }
    }
    const dim3 grid(ceil_div(H, AGG_COLS), B);
    switch (ni) {
        AGG_LONG_CASE((aggregate_long_kernel<T, 5>), 5, grid, dim3(NT), 0, st, M, (const T*)x, (T*)out, N, H, mode, scale, scale_ptr, self_w, accumulate)
        AGG_LONG_CASE((aggregate_long_kernel<T, 6>), 6, grid, dim3(NT), 0, st, M, (const T*)x, (T*)out, N, H, mode, scale, scale_ptr, self_w, accumulate)
        AGG_LONG_CASE((aggregate_long_kernel<T, 7>), 7, grid, dim3(NT), 0, st, M, (const T*)x, (T*)out, N, H, mode, scale, scale_ptr, self_w, accumulate)
        AGG_LONG_CASE((aggregate_long_kernel<T, 8>), 8, grid, dim3(NT), 0, st, M, (const T*)x, (T*)out, N, H, mode, scale, scale_ptr, self_w, accumulate)
    }
#undef AGG_LONG_CASE
    return xggm_check_launch(name);
}

template <typename T>
int agg_dot_long(const char* name, const float* M, const void* x, const void* dh, float* out, int B, int N, int H, float* ws,
                 hipStream_t st) {
    XGGM_REQUIRE(M && x && dh && out && ws && B > 0 && H > 0 && B <= 65535, "%s: bad arguments", name);
    XGGM_LONG_N(name, N);
    dim3 grid(ceil_div(H, NT), B);
    XGGM_REQUIRE((int64_t)grid.x * grid.y <= XGGM_SUM_WS_FLOATS - 8, "%s: %lld workgroups exceed the sum workspace", name,
                 (long long)grid.x * grid.y);
    hipLaunchKernelGGL((agg_dot_long_kernel<T>), grid, dim3(NT), 0, st, M, (const T*)x, (const T*)dh, out, N, H, ws);
    return xggm_check_launch(name);
}

}  // namespace

extern "C" int xggm_adj_regen_long_fwd(const float* S, float* adj, float* colmax, int32_t* argmax, int B, int N, hipStream_t st) {
    XGGM_REQUIRE(S && adj && colmax && argmax && B > 0, "xggm_adj_regen_long_fwd: bad arguments");
    XGGM_LONG_N("xggm_adj_regen_long_fwd", N);
    hipLaunchKernelGGL(adj_regen_long_fwd_kernel, dim3(B), dim3(NT), 0, st, S, adj, colmax, argmax, N);
    return xggm_check_launch("xggm_adj_regen_long_fwd");
}

extern "C" int xggm_adj_regen_long_bwd(const float* d_adj, const float* S, const float* adj, const float* colmax,
                                       const int32_t* argmax, float* dS, int B, int N, hipStream_t st) {
    XGGM_REQUIRE(d_adj && S && adj && colmax && argmax && dS && B > 0, "xggm_adj_regen_long_bwd: bad arguments");
    XGGM_LONG_N("xggm_adj_regen_long_bwd", N);
    hipLaunchKernelGGL(adj_regen_long_bwd_kernel, dim3(B), dim3(NT), 0, st, d_adj, S, adj, colmax, argmax, dS, N);
    return xggm_check_launch("xggm_adj_regen_long_bwd");
}

extern "C" int xggm_adj_init_long_fwd(const float* e, const float* randn, float* adj, float* gradlog, int B, int N, float sigma,
                                      const uint64_t* rng, uint32_t sid, hipStream_t st) {
    XGGM_REQUIRE(adj && B > 0, "xggm_adj_init_long_fwd: bad arguments B=%d", B);
    XGGM_LONG_N("xggm_adj_init_long_fwd", N);
    XGGM_REQUIRE(sigma > 0.f, "xggm_adj_init_long_fwd: sigma must be > 0");
    hipLaunchKernelGGL(adj_init_long_fwd_kernel, dim3(grid1d((int64_t)B * N * N)), dim3(NT), 0, st, e, randn, adj, gradlog, B, N,
                       N * (N - 1) / 2, sigma, rng, sid);
    return xggm_check_launch("xggm_adj_init_long_fwd");
}

extern "C" int xggm_adj_init_long_bwd(const float* d_adj, float* d_e, int B, int N, hipStream_t st) {
    XGGM_REQUIRE(d_adj && d_e && B > 0, "xggm_adj_init_long_bwd: bad arguments");
    XGGM_LONG_N("xggm_adj_init_long_bwd", N);
    hipLaunchKernelGGL(adj_init_long_bwd_kernel, dim3(grid1d((int64_t)B * N * N)), dim3(NT), 0, st, d_adj, d_e, B, N,
                       N * (N - 1) / 2);
    return xggm_check_launch("xggm_adj_init_long_bwd");
}

extern "C" int xggm_gat_att_long_fwd(const float* s, const float* adj, float* att, int B, int N, float alpha, hipStream_t st) {
    XGGM_REQUIRE(s && adj && att && B > 0, "xggm_gat_att_long_fwd: bad arguments B=%d", B);
    XGGM_LONG_N("xggm_gat_att_long_fwd", N);
    XGGM_REQUIRE((int64_t)B * N <= INT32_MAX / 2, "xggm_gat_att_long_fwd: B=%d too large", B);
    hipLaunchKernelGGL(gat_att_long_fwd_kernel, dim3(std::min(ceil_div(B * N, 4), 2048)), dim3(NT), 0, st, s, adj, att, B, N,
                       alpha);
    return xggm_check_launch("xggm_gat_att_long_fwd");
}

extern "C" int xggm_cosine_adjacency_long_f32(const float* cls, const float* attr, float* adj, int n_img, int N, int D, float eps,
                                              hipStream_t st) {
    XGGM_REQUIRE(cls && attr && adj && n_img > 0, "xggm_cosine_adjacency_long_f32: bad arguments");
    XGGM_LONG_N("xggm_cosine_adjacency_long_f32", N);
    XGGM_REQUIRE(D > 0 && D % 4 == 0, "xggm_cosine_adjacency_long_f32: embedding width %d must be a multiple of 4", D);
    XGGM_REQUIRE(reinterpret_cast<uintptr_t>(cls) % 16 == 0 && reinterpret_cast<uintptr_t>(attr) % 16 == 0,
                 "xggm_cosine_adjacency_long_f32: embeddings must be 16-byte aligned");
    hipLaunchKernelGGL(cosine_adj_long_kernel, dim3(n_img), dim3(NT), 0, st, cls, attr, adj, N, D, eps);
    return xggm_check_launch("xggm_cosine_adjacency_long_f32");
}

#define GRAPH_LONG_API(SUF, T)                                                                                              \
    extern "C" int xggm_aggregate_long_##SUF(const float* M, const void* x, void* out, int B, int N, int H, int mode,      \
                                             float scale, const float* scale_ptr, float self_w, int accumulate,           \
                                             hipStream_t st) {                                                             \
        return aggregate_long<T>("xggm_aggregate_long_" #SUF, M, x, out, B, N, H, mode, scale, scale_ptr, self_w,         \
                                 accumulate, st);                                                                          \
    }                                                                                                                       \
    extern "C" int xggm_agg_dot_long_##SUF(const float* M, const void* x, const void* dh, float* out, int B, int N, int H, \
                                           float* ws, hipStream_t st) {                                                    \
        return agg_dot_long<T>("xggm_agg_dot_long_" #SUF, M, x, dh, out, B, N, H, ws, st);                                \
    }                                                                                                                       \
    extern "C" int xggm_gat_att_long_bwd_##SUF(const float* d_att, const float* att, const float* s, const float* adj,    \
                                               void* ds, int B, int N, float alpha, hipStream_t st) {                      \
        XGGM_REQUIRE(d_att && att && s && adj && ds && B > 0, "xggm_gat_att_long_bwd_" #SUF ": bad arguments");           \
        XGGM_LONG_N("xggm_gat_att_long_bwd_" #SUF, N);                                                                     \
        hipLaunchKernelGGL((gat_att_long_bwd_kernel<T>), dim3(B), dim3(NT), 0, st, d_att, att, s, adj, (T*)ds, N, alpha);  \
        return xggm_check_launch("xggm_gat_att_long_bwd_" #SUF);                                                           \
    }

GRAPH_LONG_API(f32, float)
GRAPH_LONG_API(bf16, bf16)
