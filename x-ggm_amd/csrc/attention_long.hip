// Attention core for long sentences and 100-box features: problems whose longer side has 65 .. 128 rows (each side
// 1 .. 128), head width 64.  softmax(Q K^T / sqrt(d) + mask) -> dropout -> P V and the backward, with the contracts of
// attention.hip / attention_mfma.hip (which keep serving everything up to 64 x 64):
//   * one workgroup owns a (sample, head), forward and backward: dK, dV and the bias partials are summed over the query
//     rows in index order, no floating-point atomics, two launches give the same bits,
//   * the dropout keep-scale of probability (i, j) is dropout_scale / dropout_scale4 of element
//     ((b * heads + h) * Sq + i) * Sk + j; P and the mask are recomputed in the backward, nothing but the inputs is saved,
//   * the softmax runs over the whole row in two passes (maximum, then sum): a row is at most 128 scores and stays in
//     registers (matrix-core kernels) or LDS (fp32 kernels) -- no online rescaling,
//   * rows and columns past the problem enter no product and no store.
// bf16 storage with 16-byte aligned operands runs on the matrix cores: the wave that owns query rows 16 w .. 16 w + 15
// computes the TRANSPOSED score tiles S^T = K Q^T (and dP^T = V dO^T) of those rows against every key, so a lane holds
// four consecutive keys of ONE query row per tile -- 8 tiles x 4 = 32 scores of a row per lane, the row spread over the
// four lanes fr, fr + 16, fr + 32, fr + 48.  Maximum, sum and the row sum of dP P are finished with two cross-lane
// exchanges, one Philox call serves the four keys of a tile (Sk % 4 == 0), and P D / dS leave as 8-byte bf16 stores
// into the operand images of the second products.  No fp32 score tile passes through LDS: the backward's images
// (Q, K, V, dO: 4 x 128 x 80 bf16; dS and P D: 2 x 128 x 136 bf16) take 148 KiB of the CU's 160.
// fp32 storage, and bf16 storage that fails the alignment rule, run fp32 arithmetic throughout: K and V stay resident
// in LDS as fp32 and the query rows are walked in blocks of 32; the dK / dV tiles of a thread stay in its registers
// across the blocks.
// attention_common.h holds what this file shares with attention.hip and attention_mfma.hip: the argument structs, Drop,
// the MFMA fragments, store_grad_tile, load_tile / dot64 / axpy4 / fold_bias of the fp32 kernels, the LDS sizes
// (mfma_fwd_lds, mfma_bwd_lds) and the launch helper.
#include "attention_common.h"

namespace {
using namespace attn;

constexpr int SMAX = 128;  // rows of either side

// ================================================================================================ matrix cores (bf16)
namespace mc {

constexpr int NT = 512;      // 8 waves: wave w owns query rows 16 w .. 16 w + 15 in the row phase
constexpr int TJ = SMAX / 16;  // key tiles of a row

// rows (<= 128) x 64 bf16 tile: two 16-byte chunks per thread.  fetch only issues the loads of the rows inside the
// problem (the loads of all tiles of a workgroup are in flight together); the padding rows are zeros from the fetch on.
// (attention_mfma.hip has its own pair on purpose: a 64-row tile with clamped, branch-free loads, zeroed at the commit.)
struct TileRegs { short8_t v[2]; };
__device__ __forceinline__ TileRegs tile_fetch(const bf16* base, int64_t rs, int valid, int tid) {
    TileRegs t;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int c = tid + it * NT, r = c >> 3, cc = (c & 7) * 8;
        const short8_t zero = {};
        t.v[it] = r < valid ? *reinterpret_cast<const short8_t*>(base + (int64_t)r * rs + cc) : zero;
    }
    return t;
}
__device__ __forceinline__ void tile_commit(bf16* lds, const TileRegs& t, int rows, int tid) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int c = tid + it * NT, r = c >> 3, cc = (c & 7) * 8;
        if (r < rows) *reinterpret_cast<short8_t*>(lds + r * LDT + cc) = t.v[it];
    }
}

// a query row's 128 scores live in the lanes fr, fr + 16, fr + 32, fr + 48: two exchanges finish a row reduction
__device__ __forceinline__ float row4_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float row4_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// transposed score tiles of query rows row0 .. row0 + 15 against the key tiles [0, ntk): s[tj][r] = score of query
// row0 + fr and key 16 tj + 4 fq + r, -inf outside the problem.  Returns the lane's maximum.
__device__ __forceinline__ float score_tiles(const AttnArgs& a, const bf16* Qs, const bf16* Ks, int row0, int ntk, int b, int lane,
                                             float4_t (&s)[TJ]) {
    const int fr = lane & 15, fq = lane >> 4;
    const bf16x8_t q0 = frag_rows(Qs, LDT, row0, 0, lane), q1 = frag_rows(Qs, LDT, row0, 32, lane);
    const bool row_in = row0 + fr < a.Sq;
    float m = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
        if (tj < ntk) {
            float4_t acc = {0.f, 0.f, 0.f, 0.f};
            acc = ATTN_MFMA(frag_rows(Ks, LDT, tj * 16, 0, lane), q0, acc);
            acc = ATTN_MFMA(frag_rows(Ks, LDT, tj * 16, 32, lane), q1, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = tj * 16 + fq * 4 + r;
                const bool in = row_in && j < a.Sk;
                const float mk = (a.mask && in) ? a.mask[(int64_t)b * a.Sk + j] : 0.f;
                s[tj][r] = in ? acc[r] * a.scale + mk : -INFINITY;
                m = fmaxf(m, s[tj][r]);
            }
        }
    }
    return m;
}

__global__ __launch_bounds__(NT) void attn_long_fwd_mc(AttnArgs a, bf16* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk;
    const int RQ = rup(Sq, 16), RK = rup(Sk, 32), LDP = RK + 8;  // mfma_fwd_lds has the same counts
    bf16* Qs = reinterpret_cast<bf16*>(smem_raw);
    bf16* Ks = Qs + RQ * LDT;
    bf16* Vs = Ks + RK * LDT;
    bf16* Pb = Vs + RK * LDT;  // [RQ][LDP] bf16 probabilities (dropout folded in)
    {
        const TileRegs tq_ = tile_fetch((const bf16*)a.q + (int64_t)b * Sq * a.q_rs + h * D, a.q_rs, Sq, tid);
        const TileRegs tk_ = tile_fetch((const bf16*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
        const TileRegs tv_ = tile_fetch((const bf16*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
        tile_commit(Qs, tq_, RQ, tid);
        tile_commit(Ks, tk_, RK, tid);
        tile_commit(Vs, tv_, RK, tid);
    }
    __syncthreads();
    const int row0 = wid * 16, ntk = RK / 16;
    const bool mine = row0 < RQ;  // wave-uniform
    if (mine) {
        float4_t s[TJ];
        const float m = row4_max(score_tiles(a, Qs, Ks, row0, ntk, b, lane, s));
        float sum = 0.f;
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
            if (tj < ntk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[tj][r] = s[tj][r] > -INFINITY ? __expf(s[tj][r] - m) : 0.f;
                    sum += s[tj][r];
                }
        sum = row4_sum(sum);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
        const Drop dr(a, b, h);
        const int i = row0 + fr;
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
            if (tj < ntk) {
                const int j0 = tj * 16 + fq * 4;
                float ds[4] = {1.f, 1.f, 1.f, 1.f};
                if (i < Sq && j0 < Sk) dr.scale4<true>(i, j0, Sk, ds);
                short4_t pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = __builtin_bit_cast(short, __float2bfloat16(s[tj][e] * inv * ds[e]));
                *reinterpret_cast<short4_t*>(Pb + i * LDP + j0) = pk;  // zeros outside the problem
            }
    }
    __syncthreads();
    // O = P V of the wave's own rows.  The tiles go back through LDS (the wave's rows of the Q image are dead) so that
    // the context leaves as whole 16-byte row pieces.
    bf16* Os = Qs;
    if (mine) {
#pragma unroll
        for (int tc = 0; tc < 4; ++tc) {
            float4_t acc = {0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < RK; ks += 32)
                acc = ATTN_MFMA(frag_rows(Pb, LDP, row0, ks, lane), frag_tr(Vs, LDT, ks, tc * 16, lane), acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) Os[(row0 + fq * 4 + r) * LDT + tc * 16 + fr] = __float2bfloat16(acc[r]);
        }
    }
    __syncthreads();
    for (int c = tid; c < Sq * 8; c += NT) {
        const int i = c >> 3, cc = (c & 7) * 8;
        *reinterpret_cast<short8_t*>(out + ((int64_t)b * Sq + i) * a.o_rs + h * D + cc) =
            *reinterpret_cast<const short8_t*>(Os + i * LDT + cc);
    }
}

__global__ __launch_bounds__(NT) void attn_long_bwd_mc(AttnArgs a, AttnGrad g) {
    // bias gradients: column sums of dQ / dK / dV, one slot per 16-row tile (<= 8), written by the wave that owns the
    // tile and added in tile order at the end -- the same bits whatever the scheduling
    __shared__ float csum[3][TJ][D];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk;
    const int RQ = rup(Sq, 32), RK = rup(Sk, 32), LDP = RK + 8;  // both also serve as reduction lengths; mfma_bwd_lds has the same counts
    bf16* Qs = reinterpret_cast<bf16*>(smem_raw);
    bf16* Ks = Qs + RQ * LDT;
    bf16* Vs = Ks + RK * LDT;
    bf16* dOs = Vs + RK * LDT;
    bf16* dSb = dOs + RQ * LDT;  // [RQ][LDP] bf16: dS (scaled)
    bf16* Pdb = dSb + RQ * LDP;  // [RQ][LDP] bf16: P with dropout folded in
    {
        const TileRegs tq_ = tile_fetch((const bf16*)a.q + (int64_t)b * Sq * a.q_rs + h * D, a.q_rs, Sq, tid);
        const TileRegs tk_ = tile_fetch((const bf16*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
        const TileRegs tv_ = tile_fetch((const bf16*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
        const TileRegs to_ = tile_fetch((const bf16*)g.d_out + (int64_t)b * Sq * a.o_rs + h * D, a.o_rs, Sq, tid);
        tile_commit(Qs, tq_, RQ, tid);
        tile_commit(Ks, tk_, RK, tid);
        tile_commit(Vs, tv_, RK, tid);
        tile_commit(dOs, to_, RQ, tid);
    }
    __syncthreads();
    // row phase: S^T and dP^T tiles of the wave's 16 query rows in registers, softmax recomputed, then
    // dS = P (dP D - rowsum(dP D P)) scale and Pd = P D as bf16 operands.  Rows / columns outside the problem are zero.
    const int row0 = wid * 16, ntk = RK / 16;
    if (row0 < RQ) {  // wave-uniform
        float4_t s[TJ], dp[TJ];
        const float m = row4_max(score_tiles(a, Qs, Ks, row0, ntk, b, lane, s));
        {
            const bf16x8_t o0 = frag_rows(dOs, LDT, row0, 0, lane), o1 = frag_rows(dOs, LDT, row0, 32, lane);
#pragma unroll
            for (int tj = 0; tj < TJ; ++tj)
                if (tj < ntk) {
                    float4_t acc = {0.f, 0.f, 0.f, 0.f};
                    acc = ATTN_MFMA(frag_rows(Vs, LDT, tj * 16, 0, lane), o0, acc);
                    dp[tj] = ATTN_MFMA(frag_rows(Vs, LDT, tj * 16, 32, lane), o1, acc);
                }
        }
        float sum = 0.f;
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
            if (tj < ntk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[tj][r] = s[tj][r] > -INFINITY ? __expf(s[tj][r] - m) : 0.f;
                    sum += s[tj][r];
                }
        sum = row4_sum(sum);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
        const Drop dr(a, b, h);
        const int i = row0 + fr;
        float rs = 0.f;
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
            if (tj < ntk) {
                const int j0 = tj * 16 + fq * 4;
                float dm[4] = {1.f, 1.f, 1.f, 1.f};
                if (i < Sq && j0 < Sk) dr.scale4<true>(i, j0, Sk, dm);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pr = s[tj][e] * inv;   // P (zero outside the problem)
                    const float dd = dp[tj][e] * dm[e];  // dP D
                    rs += pr * dd;
                    s[tj][e] = pr;
                    dp[tj][e] = dd;
                }
                // P D leaves now: the keep-scales need not stay in registers
                short4_t kp;
#pragma unroll
                for (int e = 0; e < 4; ++e) kp[e] = __builtin_bit_cast(short, __float2bfloat16(s[tj][e] * dm[e]));
                *reinterpret_cast<short4_t*>(Pdb + i * LDP + j0) = kp;
            }
        rs = row4_sum(rs);
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
            if (tj < ntk) {
                const int j0 = tj * 16 + fq * 4;
                short4_t ks;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    ks[e] = __builtin_bit_cast(short, __float2bfloat16(s[tj][e] * (dp[tj][e] - rs) * a.scale));
                *reinterpret_cast<short4_t*>(dSb + i * LDP + j0) = ks;
            }
    }
    __syncthreads();
    // third phase and bias tail: the same text as in attn_bwd_mfma_kernel (attention_mfma.hip) but for the 64-bit row
    // base.  Moved into one shared device function it compiles to other code in both kernels -- here from 101 VGPRs to
    // all 128 plus spills (584 bytes of scratch) -- so the two copies stay, next to the kernels whose registers they share.
    bf16 *dq = (bf16*)g.dq, *dk = (bf16*)g.dk, *dv = (bf16*)g.dv;
    const int tq = rup(Sq, 16) / 16, tk = rup(Sk, 16) / 16;
    // 4 column tiles each for dQ (tq row tiles), dK and dV (tk row tiles): one list shared by the waves
    const int n_dq = tq * 4, n_dk = tk * 4;
    for (int t = wid; t < n_dq + 2 * n_dk; t += NT / 64) {
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        if (t < n_dq) {
            const int ti = t >> 2, tc = t & 3;  // dQ = dS K: k = j
            for (int ks = 0; ks < RK; ks += 32)
                acc = ATTN_MFMA(frag_tr(Ks, LDT, ks, tc * 16, lane), frag_rows(dSb, LDP, ti * 16, ks, lane), acc);
            store_grad_tile(acc, dq + h * D, g.dq_rs, (int64_t)b * Sq, Sq, ti * 16, tc * 16, g.dbq ? csum[0][ti] : nullptr, lane);
        } else if (t < n_dq + n_dk) {
            const int u = t - n_dq, tj = u >> 2, tc = u & 3;  // dK = dS^T Q: k = i
            for (int ks = 0; ks < RQ; ks += 32)
                acc = ATTN_MFMA(frag_tr(Qs, LDT, ks, tc * 16, lane), frag_tr(dSb, LDP, ks, tj * 16, lane), acc);
            store_grad_tile(acc, dk + h * D, g.dk_rs, (int64_t)b * Sk, Sk, tj * 16, tc * 16, g.dbk ? csum[1][tj] : nullptr, lane);
        } else {
            const int u = t - n_dq - n_dk, tj = u >> 2, tc = u & 3;  // dV = (P D)^T dO: k = i
            for (int ks = 0; ks < RQ; ks += 32)
                acc = ATTN_MFMA(frag_tr(dOs, LDT, ks, tc * 16, lane), frag_tr(Pdb, LDP, ks, tj * 16, lane), acc);
            store_grad_tile(acc, dv + h * D, g.dv_rs, (int64_t)b * Sk, Sk, tj * 16, tc * 16, g.dbv ? csum[2][tj] : nullptr, lane);
        }
    }
    if (g.dbq || g.dbk) {
        __syncthreads();
        const int kind = tid / D, c = tid - kind * D;
        float* dst = kind == 0 ? g.dbq : kind == 1 ? g.dbk : kind == 2 ? g.dbv : nullptr;
        if (dst) {
            const int nt = kind == 0 ? tq : tk;
            float s = csum[kind][0][c];
            for (int u = 1; u < nt; ++u) s += csum[kind][u][c];
            dst[(int64_t)b * g.db_bs + h * D + c] = s;  // partial row of this sample: summed over the batch by the reduce launch
        }
    }
}

constexpr size_t BWD_STATIC_LDS = sizeof(float) * 3 * TJ * D;  // csum of attn_long_bwd_mc

}  // namespace mc

// ================================================================================================ fp32 arithmetic
namespace sc {

constexpr int NT = 512;
constexpr int QB = 32;     // query rows per block: K and V stay resident, Q (dO) and the score rows are per block
constexpr int KI = SMAX * 16 / NT;  // (key row, column group) items of dK / dV per thread

// scores + softmax (+ dropout scale matrix) of the nq query rows from q0 into LDS.  P: probabilities, Dm: dropout
// scale (only written when p > 0).  Wave w owns rows w, w + 8, ...; a lane holds keys lane and lane + 64.
__device__ __forceinline__ void scores_softmax(const AttnArgs& a, const float* Qs, const float* Ks, float* P, float* Dm, int b, int h,
                                               int q0, int nq, int tid) {
    const int Sk = a.Sk, ldp = Sk + 1;
    for (int s = tid; s < nq * Sk; s += NT) {
        const int i = s / Sk, j = s % Sk;
        float v = dot64(Qs + i * LD, Ks + j * LD) * a.scale;
        if (a.mask) v += a.mask[(int64_t)b * Sk + j];
        P[i * ldp + j] = v;
    }
    __syncthreads();
    const int lane = tid & 63, wid = tid >> 6;
    const Drop dr(a, b, h);
    for (int i = wid; i < nq; i += NT / 64) {
        const int j1 = lane + 64;
        const float v0 = lane < Sk ? P[i * ldp + lane] : -INFINITY;
        const float v1 = j1 < Sk ? P[i * ldp + j1] : -INFINITY;
        const float m = wave_max(fmaxf(v0, v1));
        const float e0 = lane < Sk ? __expf(v0 - m) : 0.f;
        const float e1 = j1 < Sk ? __expf(v1 - m) : 0.f;
        const float sum = wave_sum(e0 + e1);
        if (lane < Sk) {
            P[i * ldp + lane] = e0 / sum;
            if (a.p > 0.f) Dm[i * ldp + lane] = dr.scale(q0 + i, lane, Sk);
        }
        if (j1 < Sk) {
            P[i * ldp + j1] = e1 / sum;
            if (a.p > 0.f) Dm[i * ldp + j1] = dr.scale(q0 + i, j1, Sk);
        }
    }
    __syncthreads();
}

template <typename T> __global__ __launch_bounds__(NT) void attn_long_fwd_sc(AttnArgs a, T* out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk, ldp = Sk + 1;
    float* Ks = smem;
    float* Vs = Ks + Sk * LD;
    float* Qs = Vs + Sk * LD;
    float* P = Qs + QB * LD;
    float* Dm = P + QB * ldp;
    load_tile<NT>(Ks, (const T*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
    load_tile<NT>(Vs, (const T*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
    for (int q0 = 0; q0 < Sq; q0 += QB) {
        const int nq = min(QB, Sq - q0);
        __syncthreads();  // the block before is read to the end
        load_tile<NT>(Qs, (const T*)a.q + ((int64_t)b * Sq + q0) * a.q_rs + h * D, a.q_rs, nq, tid);
        __syncthreads();
        scores_softmax(a, Qs, Ks, P, Dm, b, h, q0, nq, tid);
        // O[i][c..c+3] = sum_j P[i][j] * D[i][j] * V[j][c..c+3]
        for (int w = tid; w < nq * 16; w += NT) {
            const int i = w >> 4, c = (w & 15) * 4;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < Sk; ++j) {
                float pj = P[i * ldp + j];
                if (a.p > 0.f) pj *= Dm[i * ldp + j];
                axpy4(o, pj, Vs + j * LD + c);
            }
            store4(out + ((int64_t)b * Sq + q0 + i) * a.o_rs + h * D + c, o);
        }
    }
}

template <typename T> __global__ __launch_bounds__(NT) void attn_long_bwd_sc(AttnArgs a, AttnGrad g) {
    __shared__ float red[NT / 16][D];  // bias gradients, see fold_bias
    float cq[4] = {0.f, 0.f, 0.f, 0.f};
    float ok[KI][4], ov[KI][4];  // dK / dV of items tid, tid + NT, ...: summed over the query blocks in row order
#pragma unroll
    for (int n = 0; n < KI; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) ok[n][e] = ov[n][e] = 0.f;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk, ldp = Sk + 1;
    const T* d_out = (const T*)g.d_out;
    T *dq = (T*)g.dq, *dk = (T*)g.dk, *dv = (T*)g.dv;
    float* Ks = smem;
    float* Vs = Ks + Sk * LD;
    float* Qs = Vs + Sk * LD;
    float* dOs = Qs + QB * LD;
    float* P = dOs + QB * LD;
    float* Dm = P + QB * ldp;
    float* dS = Dm + QB * ldp;
    load_tile<NT>(Ks, (const T*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
    load_tile<NT>(Vs, (const T*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
    for (int q0 = 0; q0 < Sq; q0 += QB) {
        const int nq = min(QB, Sq - q0);
        __syncthreads();  // the block before is read to the end
        load_tile<NT>(Qs, (const T*)a.q + ((int64_t)b * Sq + q0) * a.q_rs + h * D, a.q_rs, nq, tid);
        load_tile<NT>(dOs, d_out + ((int64_t)b * Sq + q0) * a.o_rs + h * D, a.o_rs, nq, tid);
        __syncthreads();
        scores_softmax(a, Qs, Ks, P, Dm, b, h, q0, nq, tid);
        // dP[i][j] = D[i][j] * sum_c dO[i][c] V[j][c]
        for (int s = tid; s < nq * Sk; s += NT) {
            const int i = s / Sk, j = s % Sk;
            float v = dot64(dOs + i * LD, Vs + j * LD);
            if (a.p > 0.f) v *= Dm[i * ldp + j];
            dS[i * ldp + j] = v;
        }
        __syncthreads();
        // dS = P * (dP - rowsum(dP * P)) * scale
        {
            const int lane = tid & 63, wid = tid >> 6;
            for (int i = wid; i < nq; i += NT / 64) {
                const int j1 = lane + 64;
                const float p0 = lane < Sk ? P[i * ldp + lane] : 0.f, p1 = j1 < Sk ? P[i * ldp + j1] : 0.f;
                const float d0 = lane < Sk ? dS[i * ldp + lane] : 0.f, d1 = j1 < Sk ? dS[i * ldp + j1] : 0.f;
                const float rs = wave_sum(p0 * d0 + p1 * d1);
                if (lane < Sk) dS[i * ldp + lane] = p0 * (d0 - rs) * a.scale;
                if (j1 < Sk) dS[i * ldp + j1] = p1 * (d1 - rs) * a.scale;
            }
        }
        __syncthreads();
        // dQ[i][c] = sum_j dS[i][j] K[j][c]: nq * 16 <= NT items, one per thread
        if (tid < nq * 16) {
            const int i = tid >> 4, c = (tid & 15) * 4;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < Sk; ++j) {
                const float s = dS[i * ldp + j];
                axpy4(o, s, Ks + j * LD + c);
            }
            store4(dq + ((int64_t)b * Sq + q0 + i) * g.dq_rs + h * D + c, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) cq[e] += o[e];
        }
        // dK[j][c] += sum_i dS[i][j] Q[i][c];  dV[j][c] += sum_i P[i][j] D[i][j] dO[i][c]
#pragma unroll
        for (int n = 0; n < KI; ++n) {
            const int w = tid + n * NT, j = w >> 4, c = (w & 15) * 4;
            if (j < Sk) {
                for (int i = 0; i < nq; ++i) {
                    const float s = dS[i * ldp + j];
                    float pj = P[i * ldp + j];
                    if (a.p > 0.f) pj *= Dm[i * ldp + j];
                    axpy4(ok[n], s, Qs + i * LD + c);
                    axpy4(ov[n], pj, dOs + i * LD + c);
                }
            }
        }
    }
    float ck[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < KI; ++n) {
        const int w = tid + n * NT, j = w >> 4, c = (w & 15) * 4;
        if (j < Sk) {
            store4(dk + ((int64_t)b * Sk + j) * g.dk_rs + h * D + c, ok[n]);
            store4(dv + ((int64_t)b * Sk + j) * g.dv_rs + h * D + c, ov[n]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ck[e] += ok[n][e];
                cv[e] += ov[n][e];
            }
        }
    }
    const int64_t po = (int64_t)b * g.db_bs + h * D;  // this (sample, head)'s partial row
    if (g.dbq) fold_bias<NT>(red, cq, g.dbq + po, tid);
    if (g.dbk) fold_bias<NT>(red, ck, g.dbk + po, tid);
    if (g.dbv) fold_bias<NT>(red, cv, g.dbv + po, tid);
}

constexpr size_t BWD_STATIC_LDS = sizeof(float) * (NT / 16) * D;  // red of attn_long_bwd_sc
inline size_t fwd_lds(int Sk) { return sizeof(float) * ((size_t)(2 * Sk + QB) * LD + 2 * (size_t)QB * (Sk + 1)); }
inline size_t bwd_lds(int Sk) { return sizeof(float) * ((size_t)(2 * Sk + 2 * QB) * LD + 3 * (size_t)QB * (Sk + 1)); }

}  // namespace sc

}  // namespace

// called by attention.hip with validated problems, 1 <= Sq, Sk <= 128.  matrix_core: bf16 storage whose pointers and
// strides pass the alignment rule of the matrix-core kernels (16-byte operands, 8-byte gradients)
int xggm_attn_fwd_long(const xggm_attn_problem& q, bool is_bf16, bool matrix_core, const uint64_t* rng, hipStream_t st) {
    const AttnArgs a = args_of(q, rng);
    const int grid = q.B * q.heads;
    if (is_bf16 && matrix_core)
        return launch(mc::attn_long_fwd_mc, "xggm_attn_fwd(long, mfma)", grid, mc::NT, mfma_fwd_lds(q.Sq, q.Sk, false), 0, st, a, (bf16*)q.out);
    if (is_bf16)
        return launch(sc::attn_long_fwd_sc<bf16>, "xggm_attn_fwd(long)", grid, sc::NT, sc::fwd_lds(q.Sk), 0, st, a, (bf16*)q.out);
    return launch(sc::attn_long_fwd_sc<float>, "xggm_attn_fwd(long)", grid, sc::NT, sc::fwd_lds(q.Sk), 0, st, a, (float*)q.out);
}

int xggm_attn_bwd_long(const xggm_attn_problem& q, bool is_bf16, bool matrix_core, const uint64_t* rng, hipStream_t st) {
    const AttnArgs a = args_of(q, rng);
    const AttnGrad g = grad_of(q);
    const int grid = q.B * q.heads;
    if (is_bf16 && matrix_core)
        return launch(mc::attn_long_bwd_mc, "xggm_attn_bwd(long, mfma)", grid, mc::NT, mfma_bwd_lds(q.Sq, q.Sk, false), mc::BWD_STATIC_LDS, st, a, g);
    if (is_bf16) return launch(sc::attn_long_bwd_sc<bf16>, "xggm_attn_bwd(long)", grid, sc::NT, sc::bwd_lds(q.Sk), sc::BWD_STATIC_LDS, st, a, g);
    return launch(sc::attn_long_bwd_sc<float>, "xggm_attn_bwd(long)", grid, sc::NT, sc::bwd_lds(q.Sk), sc::BWD_STATIC_LDS, st, a, g);
}
