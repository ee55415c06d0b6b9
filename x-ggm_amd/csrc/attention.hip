// xggm_attn_fwd / xggm_attn_bwd: the small-sequence attention core of BertAttention
// (src/lxrt/modeling.py:355-373): softmax(Q K^T / sqrt(d) + mask) -> dropout -> P V, and its
// backward.  Sequences on this path are 20 tokens / 36 objects (<= 64), d = 64, so a whole
// (batch, head) problem -- Q, K, V tiles, the score matrix and, in backward, dO and dS --
// lives in the LDS of one 256-thread workgroup: HBM traffic is exactly one read of
// Q/K/V(/dO) and one write of O (dQ/dK/dV).  Nothing but the inputs is saved for backward:
// P and the Philox dropout mask are recomputed.  Per-row softmax uses wave64 shuffle
// reductions; fp32 math throughout.  These scalar kernels serve fp32 storage (exact parity
// mode); bf16 storage runs the matrix-core versions of attention_mfma.hip.
// attention_common.h holds what this file shares with attention_mfma.hip and attention_long.hip: the argument structs,
// load_tile / dot64 / fold_bias and the launch helper.  The grouped dispatcher at the end of this file decides which of
// the three files serves a problem (route).
#include "attention_common.h"

namespace {
using namespace attn;

constexpr int NT = 256;
constexpr int SHORT_ROWS = 64;  // the kernels of this file and of attention_mfma.hip: a whole problem in one LDS tile
constexpr int LONG_ROWS = 128;  // attention_long.hip, reached through the grouped entry points only
bool g_attn_scalar = false;  // test hook (xggm_attn_set_scalar): bf16 on the scalar kernels

// scores + softmax (+ dropout scale matrix) into LDS.  P: probabilities, Dm: dropout scale
// (only written when p > 0).  Wave w owns rows w, w+4, ...
__device__ __forceinline__ void scores_softmax(const AttnArgs& a, const float* Qs, const float* Ks, float* P, float* Dm, int b,
                                               int h, int tid) {
    const int Sq = a.Sq, Sk = a.Sk, ldp = Sk + 1;
    for (int s = tid; s < Sq * Sk; s += NT) {
        const int i = s / Sk, j = s % Sk;
        float v = dot64(Qs + i * LD, Ks + j * LD) * a.scale;
        if (a.mask) v += a.mask[(int64_t)b * Sk + j];
        P[i * ldp + j] = v;
    }
    __syncthreads();
    const int lane = tid & 63, wid = tid >> 6;
    uint64_t seed = 0, off = 0;
    if (a.p > 0.f) {
        seed = a.rng[0];
        off = a.rng[1];
    }
    const float ik = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
    for (int i = wid; i < Sq; i += NT / 64) {
        const float v = lane < Sk ? P[i * ldp + lane] : -INFINITY;
        const float m = wave_max(v);
        const float e = lane < Sk ? __expf(v - m) : 0.f;
        const float sum = wave_sum(e);
        if (lane < Sk) {
            P[i * ldp + lane] = e / sum;
            if (a.p > 0.f) {
                const uint64_t idx = (((uint64_t)b * a.heads + h) * Sq + i) * Sk + lane;
                Dm[i * ldp + lane] = dropout_scale(a.p, ik, seed, off, a.sid, idx);
            }
        }
    }
    __syncthreads();
}

template <typename T> __global__ __launch_bounds__(NT) void attn_fwd_kernel(AttnArgs a, T* out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk, ldp = Sk + 1;
    float* Qs = smem;
    float* Ks = Qs + Sq * LD;
    float* Vs = Ks + Sk * LD;
    float* P = Vs + Sk * LD;
    float* Dm = P + Sq * ldp;
    load_tile<NT>(Qs, (const T*)a.q + (int64_t)b * Sq * a.q_rs + h * D, a.q_rs, Sq, tid);
    load_tile<NT>(Ks, (const T*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
    load_tile<NT>(Vs, (const T*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
    __syncthreads();
    scores_softmax(a, Qs, Ks, P, Dm, b, h, tid);
    // O[i][c..c+3] = sum_j P[i][j] * D[i][j] * V[j][c..c+3]
    for (int w = tid; w < Sq * 16; w += NT) {
        const int i = w >> 4, c = (w & 15) * 4;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < Sk; ++j) {
            float pj = P[i * ldp + j];
            if (a.p > 0.f) pj *= Dm[i * ldp + j];
            axpy4(o, pj, Vs + j * LD + c);
        }
        store4(out + ((int64_t)b * Sq + i) * a.o_rs + h * D + c, o);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void attn_bwd_kernel(AttnArgs a, const T* d_out, T* dq, T* dk, T* dv, int64_t dq_rs,
                                                      int64_t dk_rs, int64_t dv_rs, float* dbq, float* dbk, float* dbv,
                                                      int64_t db_bs) {
    __shared__ float red[NT / 16][D];  // bias gradients, see fold_bias
    float cq[4] = {0.f, 0.f, 0.f, 0.f}, ck[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
    const int Sq = a.Sq, Sk = a.Sk, ldp = Sk + 1;
    float* Qs = smem;
    float* Ks = Qs + Sq * LD;
    float* Vs = Ks + Sk * LD;
    float* dOs = Vs + Sk * LD;
    float* P = dOs + Sq * LD;
    float* Dm = P + Sq * ldp;
    float* dS = Dm + Sq * ldp;
    load_tile<NT>(Qs, (const T*)a.q + (int64_t)b * Sq * a.q_rs + h * D, a.q_rs, Sq, tid);
    load_tile<NT>(Ks, (const T*)a.k + (int64_t)b * Sk * a.k_rs + h * D, a.k_rs, Sk, tid);
    load_tile<NT>(Vs, (const T*)a.v + (int64_t)b * Sk * a.v_rs + h * D, a.v_rs, Sk, tid);
    load_tile<NT>(dOs, d_out + (int64_t)b * Sq * a.o_rs + h * D, a.o_rs, Sq, tid);
    __syncthreads();
    scores_softmax(a, Qs, Ks, P, Dm, b, h, tid);
    // dP[i][j] = D[i][j] * sum_c dO[i][c] V[j][c]
    for (int s = tid; s < Sq * Sk; s += NT) {
        const int i = s / Sk, j = s % Sk;
        float v = dot64(dOs + i * LD, Vs + j * LD);
        if (a.p > 0.f) v *= Dm[i * ldp + j];
        dS[i * ldp + j] = v;
    }
    __syncthreads();
    // dS = P * (dP - rowsum(dP * P)) * scale
    {
        const int lane = tid & 63, wid = tid >> 6;
        for (int i = wid; i < Sq; i += NT / 64) {
            const float pv = lane < Sk ? P[i * ldp + lane] : 0.f;
            const float dp = lane < Sk ? dS[i * ldp + lane] : 0.f;
            const float rs = wave_sum(pv * dp);
            if (lane < Sk) dS[i * ldp + lane] = pv * (dp - rs) * a.scale;
        }
    }
    __syncthreads();
    // dQ[i][c] = sum_j dS[i][j] K[j][c]
    // whole waves iterate (the shuffles below need every lane); lanes past the end are predicated
    for (int w = tid; w < ((Sq * 16 + 63) & ~63); w += NT) {
        const bool valid = w < Sq * 16;
        const int i = valid ? (w >> 4) : 0, c = (w & 15) * 4;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < (valid ? Sk : 0); ++j) {
            const float s = dS[i * ldp + j];
            axpy4(o, s, Ks + j * LD + c);
        }
        if (valid) store4(dq + ((int64_t)b * Sq + i) * dq_rs + h * D + c, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) cq[e] += o[e];  // rows past the end contributed zeros
    }
    // dK[j][c] = sum_i dS[i][j] Q[i][c];  dV[j][c] = sum_i P[i][j] D[i][j] dO[i][c]
    for (int w = tid; w < ((Sk * 16 + 63) & ~63); w += NT) {
        const bool valid = w < Sk * 16;
        const int j = valid ? (w >> 4) : 0, c = (w & 15) * 4;
        float ok[4] = {0.f, 0.f, 0.f, 0.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < (valid ? Sq : 0); ++i) {
            const float s = dS[i * ldp + j];
            float pj = P[i * ldp + j];
            if (a.p > 0.f) pj *= Dm[i * ldp + j];
            axpy4(ok, s, Qs + i * LD + c);
            axpy4(ov, pj, dOs + i * LD + c);
        }
        if (valid) {
            store4(dk + ((int64_t)b * Sk + j) * dk_rs + h * D + c, ok);
            store4(dv + ((int64_t)b * Sk + j) * dv_rs + h * D + c, ov);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ck[e] += ok[e];
            cv[e] += ov[e];
        }
    }
    const int64_t po = (int64_t)b * db_bs + h * D;  // this (sample, head)'s partial row
    if (dbq) fold_bias<NT>(red, cq, dbq + po, tid);
    if (dbk) fold_bias<NT>(red, ck, dbk + po, tid);
    if (dbv) fold_bias<NT>(red, cv, dbv + po, tid);
}

// ---- which kernels serve a problem -------------------------------------------------------------------------------
// bit 0: matrix cores (attention_mfma.hip, or the matrix-core kernels of attention_long.hip), bit 1: attention_long.hip
enum Path { SHORT_SCALAR = 0, SHORT_MFMA = 1, LONG_SCALAR = 2, LONG_MFMA = 3 };
constexpr int PATH_MFMA = 1, PATH_LONG = 2;

// The only place that decides it.  Matrix cores: bf16 storage whose operands (q, k, v and out, in the backward dO) are
// 16-byte aligned with row strides that are multiples of 8 -- the tiles are fetched in 16-byte chunks -- and, in the
// backward, 8-byte aligned gradients (8-byte gradient stores); never under the xggm_attn_set_scalar hook.
Path route(const xggm_attn_problem& q, bool is_bf16, bool backward) {
    const auto bits = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    const bool operands16 = (bits(q.q) | bits(q.k) | bits(q.v) | bits(backward ? q.d_out : q.out)) % 16 == 0 && q.q_rs % 8 == 0 &&
                            q.k_rs % 8 == 0 && q.v_rs % 8 == 0 && q.o_rs % 8 == 0;
    const bool grads8 = !backward || (bits(q.dq) | bits(q.dk) | bits(q.dv)) % 8 == 0;
    const bool mfma = is_bf16 && !g_attn_scalar && operands16 && grads8;
    const bool is_long = q.Sq > SHORT_ROWS || q.Sk > SHORT_ROWS;
    return Path((mfma ? PATH_MFMA : 0) | (is_long ? PATH_LONG : 0));
}

// ---- argument checks ---------------------------------------------------------------------------------------------
// max_rows: SHORT_ROWS for the plain entry points (their contract), LONG_ROWS for the grouped ones
int check(const char* who, const xggm_attn_problem& q, const uint64_t* rng, int head_dim, int max_rows) {
    XGGM_REQUIRE(head_dim == D, "%s: head_dim %d != 64", who, head_dim);
    XGGM_REQUIRE(q.B > 0 && q.heads > 0 && q.Sq > 0 && q.Sk > 0, "%s: empty problem", who);
    if (max_rows <= SHORT_ROWS)
        XGGM_REQUIRE(q.Sq <= 64 && q.Sk <= 64, "%s: Sq=%d Sk=%d exceed the 64-row LDS tile", who, q.Sq, q.Sk);
    XGGM_REQUIRE(q.Sq <= LONG_ROWS && q.Sk <= LONG_ROWS, "%s: Sq=%d Sk=%d exceed the 128 rows the attention core serves", who,
                 q.Sq, q.Sk);
    XGGM_REQUIRE(q.q && q.k && q.v, "%s: null pointer", who);
    XGGM_REQUIRE(q.q_rs % 4 == 0 && q.k_rs % 4 == 0 && q.v_rs % 4 == 0 && q.o_rs % 4 == 0, "%s: row strides must be multiples of 4",
                 who);
    XGGM_REQUIRE(q.p >= 0.f && q.p < 1.f && (q.p == 0.f || rng), "%s: bad dropout arguments", who);
    XGGM_REQUIRE((int64_t)q.B * q.heads < (1 << 30), "%s: grid too large", who);
    return XGGM_OK;
}

int check_fwd(const xggm_attn_problem& q, const uint64_t* rng, int head_dim, int max_rows, bool is_bf16) {
    if (int e = check("xggm_attn_fwd", q, rng, head_dim, max_rows)) return e;
    const Path r = route(q, is_bf16, false);
    XGGM_REQUIRE(q.out, "xggm_attn_fwd: null output");
    XGGM_REQUIRE(!q.out8 || (is_bf16 && reinterpret_cast<uintptr_t>(q.out8) % 8 == 0),
                 "xggm_attn_fwd: the e4m3 output copy needs bf16 storage and an 8-byte aligned buffer");
    XGGM_REQUIRE(!q.out8 || (r & PATH_MFMA),
                 "xggm_attn_fwd: the e4m3 output copy is written by the matrix-core kernel only (16-byte aligned operands, "
                 "strides multiples of 8)");
    XGGM_REQUIRE(!q.out8 || !(r & PATH_LONG), "xggm_attn_fwd: the e4m3 output copy is written for problems of at most 64 rows "
                                              "(Sq=%d Sk=%d)", q.Sq, q.Sk);
    return XGGM_OK;
}

int check_bwd(const xggm_attn_problem& q, const uint64_t* rng, int head_dim, int max_rows) {
    if (int e = check("xggm_attn_bwd", q, rng, head_dim, max_rows)) return e;
    XGGM_REQUIRE(q.d_out && q.dq && q.dk && q.dv, "xggm_attn_bwd: null pointer");
    XGGM_REQUIRE(q.dq_rs % 4 == 0 && q.dk_rs % 4 == 0 && q.dv_rs % 4 == 0, "xggm_attn_bwd: row strides must be multiples of 4");
    XGGM_REQUIRE((q.dbk == nullptr) == (q.dbv == nullptr), "xggm_attn_bwd: dbk and dbv go together");
    XGGM_REQUIRE(!(q.dbq || q.dbk) || q.B == 1 || q.db_bs >= (int64_t)q.heads * D,
                 "xggm_attn_bwd: the bias-gradient partial rows need a batch stride db_bs >= heads * 64 (got %lld)",
                 (long long)q.db_bs);
    return XGGM_OK;
}

// ---- the grouped dispatcher, forward and backward ----------------------------------------------------------------
// A whole (sample, head) of a short scalar problem in the LDS of one workgroup.  These two launches do not go through
// attn::launch: they have never asked for the large-LDS opt-in, although their fp32 images pass 48 KiB well inside the
// 64 x 64 they serve (the 64 x 64 backward takes 117 KiB), and these launches have been accepted all along.  Whether
// they should reserve as well is a separate question; this keeps them launching as they always have.
template <typename T>
int launch_short_scalar(bool backward, const xggm_attn_problem& q, const uint64_t* rng, hipStream_t st) {
    const AttnArgs a = args_of(q, rng);
    const size_t score = sizeof(float) * (size_t)q.Sq * (q.Sk + 1);  // P, Dm (and dS)
    if (backward) {
        const size_t lds = sizeof(float) * (size_t)(2 * q.Sq + 2 * q.Sk) * LD + 3 * score;
        hipLaunchKernelGGL((attn_bwd_kernel<T>), dim3(q.B * q.heads), dim3(NT), lds, st, a, (const T*)q.d_out, (T*)q.dq, (T*)q.dk,
                           (T*)q.dv, q.dq_rs, q.dk_rs, q.dv_rs, q.dbq, q.dbk, q.dbv, q.db_bs);
    } else {
        const size_t lds = sizeof(float) * (size_t)(q.Sq + 2 * q.Sk) * LD + 2 * score;
        hipLaunchKernelGGL((attn_fwd_kernel<T>), dim3(q.B * q.heads), dim3(NT), lds, st, a, (T*)q.out);
    }
    return xggm_check_launch(backward ? "xggm_attn_bwd" : "xggm_attn_fwd");
}

// every problem is checked before the first launch.  Problems that can run on the short matrix-core kernels are launched
// in pairs (the first pair carries `prefetch`), the rest one by one; the short problems around a long or a scalar one
// are paired as if it were not there.
template <typename T>
int run_grouped(bool backward, const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,
                const xggm_prefetch* prefetch, hipStream_t st, int max_rows) {
    constexpr bool is_bf16 = sizeof(T) == 2;
    const char* who = backward ? "xggm_attn_bwd" : "xggm_attn_fwd";
    XGGM_REQUIRE(probs && n > 0, "%s: no problems", who);
    PrefetchArgs pf;
    if (int e = xggm_prefetch_args(prefetch, &pf, who)) return e;
    for (int i = 0; i < n; ++i)
        if (int e = backward ? check_bwd(probs[i], rng, head_dim, max_rows) : check_fwd(probs[i], rng, head_dim, max_rows, is_bf16))
            return e;
    xggm_attn_problem pend[2];
    int np = 0;
    const auto flush = [&]() {
        const int e = (backward ? xggm_attn_bwd_mfma_group : xggm_attn_fwd_mfma_group)(pend, np, rng, pf, st);
        np = 0;
        pf = PrefetchArgs{};
        return e;
    };
    for (int i = 0; i < n; ++i) {
        const xggm_attn_problem& q = probs[i];
        const Path r = route(q, is_bf16, backward);
        int e = XGGM_OK;
        if (r == SHORT_MFMA) {
            pend[np++] = q;
            if (np == 2 || i == n - 1) e = flush();
        } else if (r == SHORT_SCALAR) {
            e = launch_short_scalar<T>(backward, q, rng, st);
        } else {
            e = (backward ? xggm_attn_bwd_long : xggm_attn_fwd_long)(q, is_bf16, r == LONG_MFMA, rng, st);
        }
        if (e) return e;
    }
    return np ? flush() : XGGM_OK;
}

// the plain entry points: one problem of at most 64 x 64
xggm_attn_problem plain_problem(const void* q, const void* k, const void* v, const float* mask, int B, int heads, int Sq, int Sk,
                                int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, float scale, float p, uint32_t sid) {
    xggm_attn_problem pr{};
    pr.q = q; pr.k = k; pr.v = v; pr.mask = mask;
    pr.B = B; pr.heads = heads; pr.Sq = Sq; pr.Sk = Sk;
    pr.q_rs = q_rs; pr.k_rs = k_rs; pr.v_rs = v_rs; pr.o_rs = o_rs;
    pr.scale = scale; pr.p = p; pr.sid = sid;
    return pr;
}

template <typename T>
int attn_fwd(const void* q, const void* k, const void* v, const float* mask, void* out, int B, int heads, int Sq, int Sk,
             int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, float scale, float p, const uint64_t* rng,
             uint32_t sid, hipStream_t st) {
    xggm_attn_problem pr = plain_problem(q, k, v, mask, B, heads, Sq, Sk, q_rs, k_rs, v_rs, o_rs, scale, p, sid);
    pr.out = out;
    return run_grouped<T>(false, &pr, 1, head_dim, rng, nullptr, st, SHORT_ROWS);
}

template <typename T>
int attn_bwd(const void* q, const void* k, const void* v, const float* mask, const void* d_out, void* dq, void* dk, void* dv,
             int B, int heads, int Sq, int Sk, int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs,
             int64_t dq_rs, int64_t dk_rs, int64_t dv_rs, float scale, float p, const uint64_t* rng, uint32_t sid,
             float* dbq, float* dbk, float* dbv, int64_t db_bs, hipStream_t st) {
    xggm_attn_problem pr = plain_problem(q, k, v, mask, B, heads, Sq, Sk, q_rs, k_rs, v_rs, o_rs, scale, p, sid);
    pr.d_out = d_out; pr.dq = dq; pr.dk = dk; pr.dv = dv;
    pr.dq_rs = dq_rs; pr.dk_rs = dk_rs; pr.dv_rs = dv_rs;
    pr.dbq = dbq; pr.dbk = dbk; pr.dbv = dbv; pr.db_bs = db_bs;
    return run_grouped<T>(true, &pr, 1, head_dim, rng, nullptr, st, SHORT_ROWS);
}

}  // namespace

#define ATTN_API(SUF, T)                                                                                                   \
    extern "C" int xggm_attn_fwd_##SUF(const void* q, const void* k, const void* v, const float* mask, void* out, int B,  \
                                       int heads, int Sq, int Sk, int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs, \
                                       int64_t o_rs, float scale, float p, const uint64_t* rng, uint32_t sid,            \
                                       hipStream_t st) {                                                                  \
        return attn_fwd<T>(q, k, v, mask, out, B, heads, Sq, Sk, head_dim, q_rs, k_rs, v_rs, o_rs, scale, p, rng, sid, st);\
    }                                                                                                                      \
    extern "C" int xggm_attn_bwd_##SUF(const void* q, const void* k, const void* v, const float* mask, const void* d_out,  \
                                       void* dq, void* dk, void* dv, int B, int heads, int Sq, int Sk, int head_dim,      \
                                       int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, int64_t dq_rs,             \
                                       int64_t dk_rs, int64_t dv_rs, float scale, float p, const uint64_t* rng,           \
                                       uint32_t sid, float* dbq, float* dbk, float* dbv, int64_t db_bs,                  \
                                       hipStream_t st) {                                                                  \
        return attn_bwd<T>(q, k, v, mask, d_out, dq, dk, dv, B, heads, Sq, Sk, head_dim, q_rs, k_rs, v_rs, o_rs, dq_rs,    \
                           dk_rs, dv_rs, scale, p, rng, sid, dbq, dbk, dbv, db_bs, st);                                    \
    }                                                                                                                      \
    extern "C" int xggm_attn_fwd_grouped_##SUF(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,   \
                                               const xggm_prefetch* prefetch, hipStream_t st) {                           \
        return run_grouped<T>(false, probs, n, head_dim, rng, prefetch, st, LONG_ROWS);                                   \
    }                                                                                                                      \
    extern "C" int xggm_attn_bwd_grouped_##SUF(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,   \
                                               const xggm_prefetch* prefetch, hipStream_t st) {                           \
        return run_grouped<T>(true, probs, n, head_dim, rng, prefetch, st, LONG_ROWS);                                    \
    }

ATTN_API(f32, float)
ATTN_API(bf16, bf16)

// test / A-B hook: 1 = bf16 attention on the scalar fp32-math kernels, 0 = matrix-core kernels
extern "C" int xggm_attn_set_scalar(int on) {
    g_attn_scalar = on != 0;
    return XGGM_OK;
}
