// What the three translation units of the attention core share (attention.hip: fp32 arithmetic up to 64 x 64 and the
// dispatcher; attention_mfma.hip: matrix cores up to 64 x 64; attention_long.hip: 65 .. 128 rows, both arithmetics):
// the kernel arguments, the dropout keep-scale, the MFMA fragments and the gradient-tile store of the matrix-core
// backward, the fp32 tile helpers of the scalar kernels, the LDS sizes and the one launch helper.  The row phases
// (scores, softmax, dropout) and the tile_fetch / tile_commit pairs differ by design and stay in their files.
#pragma once
#include "common.h"
#include "xggm.h"

// bf16 matrix-core versions (attention_mfma.hip): one or two validated problems per launch
int xggm_attn_fwd_mfma_group(const xggm_attn_problem* probs, int n, const uint64_t* rng, const PrefetchArgs& pf, hipStream_t st);
int xggm_attn_bwd_mfma_group(const xggm_attn_problem* probs, int n, const uint64_t* rng, const PrefetchArgs& pf, hipStream_t st);
// problems with 65 .. 128 rows on a side (attention_long.hip): one validated problem per launch.  matrix_core: bf16
// storage whose pointers and strides pass the alignment rule of the matrix-core kernels
int xggm_attn_fwd_long(const xggm_attn_problem& q, bool is_bf16, bool matrix_core, const uint64_t* rng, hipStream_t st);
int xggm_attn_bwd_long(const xggm_attn_problem& q, bool is_bf16, bool matrix_core, const uint64_t* rng, hipStream_t st);

namespace attn {

constexpr int D = 64;        // head width
constexpr int LD = D + 4;    // fp32 tile row stride: float4-aligned rows, conflict-free 16-byte reads
constexpr int LDT = D + 16;  // bf16 tile row stride in elements (160 B): b128 rows 16-B aligned; tr-reads of k-rows 8 apart share banks (2-way; the GEMM swaps half-blocks against this, see gemm.hip fast_frag -- here the phases are barrier-latency-bound)

__host__ __device__ constexpr int rup(int x, int m) { return (x + m - 1) / m * m; }

// ---- kernel arguments ------------------------------------------------------------------------------------------------
// operands are untyped: the kernels cast them to their storage type where they use them
struct AttnArgs {
    const void *q, *k, *v;
    const float* mask;  // additive [B, Sk] or null
    int64_t q_rs, k_rs, v_rs, o_rs;  // row strides in elements
    int B, heads, Sq, Sk;
    float scale, p;
    const uint64_t* rng;
    uint32_t sid;
};
struct AttnGrad {
    const void* d_out;
    void *dq, *dk, *dv;
    int64_t dq_rs, dk_rs, dv_rs;
    float *dbq, *dbk, *dbv;  // or null: bias-gradient partial rows of this (sample, head)
    int64_t db_bs;
};
inline AttnArgs args_of(const xggm_attn_problem& q, const uint64_t* rng) {
    return AttnArgs{q.q, q.k, q.v, q.mask, q.q_rs, q.k_rs, q.v_rs, q.o_rs, q.B, q.heads, q.Sq, q.Sk, q.scale, q.p, rng, q.sid};
}
inline AttnGrad grad_of(const xggm_attn_problem& q) {
    return AttnGrad{q.d_out, q.dq, q.dk, q.dv, q.dq_rs, q.dk_rs, q.dv_rs, q.dbq, q.dbk, q.dbv, q.db_bs};
}

// ---- launching -------------------------------------------------------------------------------------------------------
// `lds` bytes of dynamic LDS on top of the kernel's `fixed` bytes of static LDS.  xggm_reserve_lds opts in by the dynamic
// size alone and does nothing up to 48 KiB: where only the sum passes 48 KiB the opt-in is asked for all the same.
constexpr size_t LDS_NO_OPT_IN = 48 * 1024;
template <typename K, typename... A>
int launch(K kernel, const char* who, int grid, int nt, size_t lds, size_t fixed, hipStream_t st, A... args) {
    const size_t reserve = (lds <= LDS_NO_OPT_IN && lds + fixed > LDS_NO_OPT_IN) ? LDS_NO_OPT_IN + 1024 : lds;
    if (int e = xggm_reserve_lds(reinterpret_cast<const void*>(kernel), reserve, who)) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(nt), lds, st, args...);
    return xggm_check_launch(who);
}

// ---- dropout ---------------------------------------------------------------------------------------------------------
// keep-scale of probability (i, j) of this (sample, head): a pure function of the Philox state, recomputed wherever it
// is needed instead of being parked in LDS
struct Drop {
    float p, ik;
    uint64_t seed, off, base;
    uint32_t sid;
    __device__ __forceinline__ Drop(const AttnArgs& a, int b, int h) : p(a.p), ik(a.p > 0.f ? 1.f / (1.f - a.p) : 1.f), seed(0), off(0),
                                                                     base(((uint64_t)b * a.heads + h) * a.Sq * a.Sk), sid(a.sid) {
        if (a.p > 0.f) {
            seed = a.rng[0];
            off = a.rng[1];
        }
    }
    __device__ __forceinline__ float scale(int i, int j, int Sk) const {
        return p > 0.f ? dropout_scale(p, ik, seed, off, sid, base + (uint64_t)i * Sk + j) : 1.f;
    }
    // keep-scales of (i, j0 .. j0 + 3), j0 % 4 == 0: one Philox call when the four element indices share it
    // (Sk % 4 == 0), one per key otherwise.  PAST_SK: the group may reach past Sk; those keys get 1 and no call.  The
    // kernels up to 64 x 64 pass false: their padding keys meet a zero probability, and their instruction stream stays
    template <bool PAST_SK>
    __device__ __forceinline__ void scale4(int i, int j0, int Sk, float (&s)[4]) const {
        if (PAST_SK) s[0] = s[1] = s[2] = s[3] = 1.f;
        if (p <= 0.f) {
            if (!PAST_SK) s[0] = s[1] = s[2] = s[3] = 1.f;
            return;
        }
        if ((Sk & 3) == 0) {
            dropout_scale4(p, ik, seed, off, sid, base + (uint64_t)i * Sk + j0, s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (!PAST_SK || j0 + e < Sk) s[e] = dropout_scale(p, ik, seed, off, sid, base + (uint64_t)i * Sk + j0 + e);
        }
    }
};

// ---- matrix cores: 16x16x32 bf16 MFMA on LDS images ------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float float4_t;

#define ATTN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

// dynamic LDS of the matrix-core kernels, with the row counts of their carve-ups.  Q (and dO) have RQ rows -- M of every
// product, in the backward also a reduction length, hence 32 --, K and V have RK; the probability images P D (and dS)
// are [RQ][LDP] bf16.  score_tiles: the kernels up to 64 x 64 also pass the scores (and dP) through LDS as fp32
// [R16][lds_s]; the long ones keep them in registers.
__host__ __device__ constexpr size_t mfma_fwd_lds(int Sq, int Sk, bool score_tiles) {
    const int RQ = rup(Sq, 16), RK = rup(Sk, 32), LDP = RK + 8, lds_s = rup(Sk, 16) + 1;
    return sizeof(bf16) * ((size_t)(RQ + 2 * RK) * LDT + (size_t)RQ * LDP) + (score_tiles ? sizeof(float) * RQ * lds_s : 0);
}
__host__ __device__ constexpr size_t mfma_bwd_lds(int Sq, int Sk, bool score_tiles) {
    const int RQ = rup(Sq, 32), RK = rup(Sk, 32), LDP = RK + 8, R16 = rup(Sq, 16), lds_s = rup(Sk, 16) + 1;
    return sizeof(bf16) * ((size_t)(2 * RQ + 2 * RK) * LDT + 2 * (size_t)RQ * LDP) + (score_tiles ? sizeof(float) * 2 * R16 * lds_s : 0);
}

// operand whose reduction index k is contiguous: lane (fr, fq) gets row row0+fr, k = k0+8fq .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const bf16* lds, int ld, int row0, int k0, int lane) {
    const int fr = lane & 15, fq = lane >> 4;
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const short8_t*>(lds + (row0 + fr) * ld + k0 + fq * 8));
}
// operand stored [k][n] (n contiguous): lane gets n = n0+fr, k = k0+8fq .. +7 through two transposing reads
__device__ __forceinline__ bf16x8_t frag_tr(const bf16* lds, int ld, int k0, int n0, int lane) {
    const int fr = lane & 15, fq = lane >> 4, q = fr >> 2, p = fr & 3;
    const bf16* a0 = lds + (k0 + 8 * fq + q) * ld + n0 + 4 * p;
    const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(a0));
    const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)(a0 + 4 * ld));
    short8_t v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
    v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_bit_cast(bf16x8_t, v);
}

// store a 16x16 gradient tile (rows row0.., 16 columns at col0) and fold its column sums into csum.  The tile comes out
// of an MFMA with SWAPPED operands: lane (fr, fq) holds row fr, columns 4 fq .. 4 fq + 3 -- one 8-byte store per lane
// (was four 2-byte ones) and column sums by DPP moves inside the 16-lane rows (was two ds_bpermute round trips).
// Row: the type of the row index, int where B * S rows fit it (the kernels up to 64 x 64), int64_t in the long ones.
template <typename Row>
__device__ __forceinline__ void store_grad_tile(const float4_t& acc, bf16* dst, int64_t rs, Row row_base, int rows_valid, int row0,
                                                int col0, float* csum, int lane) {
    const int fr = lane & 15, fq = lane >> 4;
    const int i = row0 + fr;
    const bool ok = i < rows_valid;
    if (ok) {
        short4_t pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = __builtin_bit_cast(short, __float2bfloat16(acc[r]));
        *reinterpret_cast<short4_t*>(dst + (int64_t)(row_base + i) * rs + col0 + 4 * fq) = pk;
    }
    if (csum) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = ok ? acc[r] : 0.f;
            s += dpp_move<0xB1>(s);
            s += dpp_move<0x4E>(s);
            s += dpp_move<0x141>(s);
            s += dpp_move<0x140>(s);  // every lane of the 16-lane row holds the column's sum over the tile's rows
            if (fr == 0) csum[col0 + 4 * fq + r] = s;  // this row tile's own slot: no atomics, see the kernel's tail
        }
    }
}

// ---- fp32 arithmetic: tiles of the scalar kernels (NT threads) -------------------------------------------------------
template <int NT, typename T>
__device__ __forceinline__ void load_tile(float* lds, const T* base, int64_t rs, int rows, int tid) {
    // rows x 64 elements, 16 chunks of 4 per row
    for (int c = tid; c < rows * 16; c += NT) {
        const int r = c >> 4, cc = (c & 15) * 4;
        float t[4];
        load4(base + (int64_t)r * rs + cc, t);
        *reinterpret_cast<float4*>(lds + r * LD + cc) = make_float4(t[0], t[1], t[2], t[3]);
    }
}

__device__ __forceinline__ float dot64(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + c);
        const float4 y = *reinterpret_cast<const float4*>(b + c);
        s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    return s;
}

// o[0 .. 3] += s * row[0 .. 3]
__device__ __forceinline__ void axpy4(float (&o)[4], float s, const float* row) {
    const float4 x = *reinterpret_cast<const float4*>(row);
    o[0] += s * x.x;
    o[1] += s * x.y;
    o[2] += s * x.z;
    o[3] += s * x.w;
}

// column sums of dQ / dK / dV over a sample's rows (bias gradients) in the scalar backward kernels: every thread keeps
// the sums of ITS column group over its rows in c4 (NT % 16 == 0: a thread's columns never change), the threads of a
// column group are added in index order through `red`, and dst -- 64 columns -- is a partial row of this (sample, head)
// nobody else writes.  Uniform: every thread of the workgroup calls it.
template <int NT>
__device__ __forceinline__ void fold_bias(float (&red)[NT / 16][D], const float (&c4)[4], float* dst, int tid) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid >> 4][(tid & 15) * 4 + e] = c4[e];
    __syncthreads();
    if (tid < D) {
        float s = 0.f;
        for (int g = 0; g < NT / 16; ++g) s += red[g][tid];  // fixed order
        dst[tid] = s;
    }
}

}  // namespace attn
