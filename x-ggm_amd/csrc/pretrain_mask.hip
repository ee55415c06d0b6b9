// Pre-training batch masking on the device: random_word / random_feat / the QA answer draw of
// src/pretrain/lxmert_pretrain.py:76-215 in ONE launch (contract: xggm_pretrain_corrupt_* in xggm.h).
// The role of a workgroup comes from blockIdx alone -- object rows first, then the token blocks, then the answer blocks --
// so every branch below is uniform within a workgroup.  Every decision is taken in double from the fp32 draw, the IEEE
// operations the reference performs on Python floats; the element count of those decisions is B T + B O + B.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;
typedef int i4 __attribute__((ext_vector_type(4)));

struct CorruptK {
    xggm_pretrain_corrupt_args a;  // pool / P resolved
    int vec;                       // rows move as 16-byte vectors
    int row_blocks, tok_blocks;
};

// draw `k` (0..4 in the order of xggm.h) of element idx: the supplied buffer, else Philox stream sid_base + k
__device__ __forceinline__ float draw_of(const float* buf, const xggm_pretrain_corrupt_args& a, uint32_t k, uint64_t idx) {
    if (buf) return buf[idx];
    return philox_uniform(a.rng[0], a.rng[1], a.sid_base + k, idx);
}
// floor(u2 * n) in double, held inside [0, n): a supplied draw outside [0, 1) must not become an address
__device__ __forceinline__ int64_t pick_of(float u2, int64_t n) {
    const double v = (double)u2 * (double)n;
    int64_t i = v >= 0.0 ? (int64_t)v : 0;
    return i > n - 1 ? n - 1 : i;
}

template <typename E>  // E: the raw storage word of a feature (uint32_t for fp32, uint16_t for bf16); rows are only moved
__device__ __forceinline__ void row_role(const CorruptK& k) {
    const xggm_pretrain_corrupt_args& a = k.a;
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)a.B * a.O, F = a.F;
    const E* feats = reinterpret_cast<const E*>(a.feats);
    const E* pool = reinterpret_cast<const E*>(a.pool);
    E* out = reinterpret_cast<E*>(a.masked_feat);
    for (int64_t r = blockIdx.x; r < R; r += k.row_blocks) {
        // one draw per row, the same in every lane: through an SGPR, so the branches below are scalar branches
        const float u = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(draw_of(a.u_obj, a, 2, (uint64_t)r))));
        const E* src = feats + r * F;
        bool zero = false;
        float fm = 0.f;
        if ((double)u < a.obj_mask_rate) {  // random_feat, :119-134
            fm = 1.f;
            const double p = (double)u / a.obj_mask_rate;
            if (p < 0.8) {
                zero = true;
            } else if (p < 0.9) {
                const float u2 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(draw_of(a.u_obj_pick, a, 3, (uint64_t)r))));
                src = pool + pick_of(u2, a.P) * F;
            }
        }
        if (tid == 0) a.feat_mask[r] = fm;
        E* dst = out + r * F;
        if (k.vec) {
            const int nvec = (int)(F * (int64_t)sizeof(E) / 16);
            const i4* s = reinterpret_cast<const i4*>(src);
            i4* d = reinterpret_cast<i4*>(dst);
            for (int i = tid; i < nvec; i += 4 * NT) {  // up to four 16-byte loads in flight per thread before the first store
                i4 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (!zero && i + j * NT < nvec) ? s[i + j * NT] : (i4){0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j * NT < nvec) d[i + j * NT] = v[j];
            }
        } else {
            for (int i = tid; i < (int)F; i += NT) dst[i] = zero ? (E)0 : src[i];
        }
    }
}

__device__ __forceinline__ void token_role(const CorruptK& k) {
    const xggm_pretrain_corrupt_args& a = k.a;
    const int64_t idx = (int64_t)(blockIdx.x - k.row_blocks) * NT + threadIdx.x;
    if (idx >= (int64_t)a.B * a.T) return;
    const int t = (int)(idx % a.T);
    const int64_t id = a.input_ids[idx];
    int64_t out = id, label = -1;
    // [CLS], the last real token ([SEP]) and padding are never drawn for (:156-172)
    const bool eligible = t >= 1 && t < a.T - 1 && a.input_mask[idx] == 1 && a.input_mask[idx + 1] == 1;
    if (eligible) {
        const float u = draw_of(a.u_word, a, 0, (uint64_t)idx);
        if ((double)u < a.word_mask_rate) {  // random_word, :86-107
            label = id;
            const double p = (double)u / a.word_mask_rate;
            if (p < 0.8)
                out = a.mask_id;
            else if (p < 0.9)
                out = pick_of(draw_of(a.u_word_pick, a, 1, (uint64_t)idx), a.vocab_size);
        }
    }
    a.input_ids_out[idx] = out;
    a.masked_lm_labels[idx] = label;
}

__device__ __forceinline__ void answer_role(const CorruptK& k) {
    const xggm_pretrain_corrupt_args& a = k.a;
    const int64_t b = (int64_t)(blockIdx.x - k.row_blocks - k.tok_blocks) * NT + threadIdx.x;
    if (b >= a.B) return;
    const int64_t* ids = a.label_ids + b * a.K;
    const float* sc = a.label_scores + b * a.K;
    int n = 0;
    int64_t last = -1;
    double sum = 0.0;
    for (int j = 0; j < a.K; ++j)
        if (ids[j] >= 0) {
            ++n;
            last = ids[j];
            sum += (double)sc[j];
        }
    int64_t ans = -1;
    if (n > 0 && a.is_matched[b] == 1) {  // :187-199
        ans = last;  // one key, or the fallback of the inverse CDF
        if (n > 1) {
            const double target = (double)draw_of(a.u_ans, a, 4, (uint64_t)b) * sum;
            double c = 0.0;
            for (int j = 0; j < a.K; ++j)
                if (ids[j] >= 0) {
                    c += (double)sc[j];
                    if (target < c) {
                        ans = ids[j];
                        break;
                    }
                }
        }
    }
    a.ans[b] = ans;
}

template <typename E>
__global__ __launch_bounds__(NT) void pretrain_corrupt_kernel(const CorruptK k) {
    const int blk = blockIdx.x;
    if (blk < k.row_blocks)
        row_role<E>(k);
    else if (blk < k.row_blocks + k.tok_blocks)
        token_role(k);
    else
        answer_role(k);
}

__global__ __launch_bounds__(NT) void uniform_kernel(float* out, int64_t n, const uint64_t* rng, uint32_t sid) {
    const uint64_t seed = rng[0], off = rng[1];
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        out[i] = philox_uniform(seed, off, sid, (uint64_t)i);
}

bool overlaps(const void* p, int64_t np, const void* q, int64_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

template <typename E>
int corrupt(const xggm_pretrain_corrupt_args* args, hipStream_t st, const char* who) {
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    CorruptK k;
    k.a = *args;
    xggm_pretrain_corrupt_args& a = k.a;
    XGGM_REQUIRE(a.B > 0 && a.T > 0 && a.O > 0 && a.F > 0 && a.K > 0, "%s: B=%d T=%d O=%d F=%d K=%d must all be positive", who, a.B,
                 a.T, a.O, a.F, a.K);
    XGGM_REQUIRE((int64_t)a.B * a.T < (1ll << 31) && (int64_t)a.B * a.O < (1ll << 31), "%s: B T and B O must stay below 2^31", who);
    XGGM_REQUIRE(a.feats && a.masked_feat && a.feat_mask, "%s: null feats / masked_feat / feat_mask", who);
    XGGM_REQUIRE(a.input_ids && a.input_mask && a.input_ids_out && a.masked_lm_labels, "%s: null token pointer", who);
    XGGM_REQUIRE(a.label_ids && a.label_scores && a.is_matched && a.ans, "%s: null answer pointer", who);
    XGGM_REQUIRE(a.word_mask_rate >= 0.0 && a.word_mask_rate <= 1.0 && a.obj_mask_rate >= 0.0 && a.obj_mask_rate <= 1.0,
                 "%s: mask rates %g / %g outside [0, 1]", who, a.word_mask_rate, a.obj_mask_rate);
    XGGM_REQUIRE(a.vocab_size > 0, "%s: vocab_size %lld must be positive", who, (long long)a.vocab_size);
    XGGM_REQUIRE(a.rng || (a.u_word && a.u_word_pick && a.u_obj && a.u_obj_pick && a.u_ans),
                 "%s: a null draw buffer needs rng", who);
    if (!a.pool) {
        a.pool = a.feats;
        a.P = (int64_t)a.B * a.O;
    }
    XGGM_REQUIRE(a.P > 0, "%s: pool of %lld rows", who, (long long)a.P);
    const int64_t row = (int64_t)a.F * (int64_t)sizeof(E), out_bytes = (int64_t)a.B * a.O * row;
    XGGM_REQUIRE(!overlaps(a.masked_feat, out_bytes, a.feats, out_bytes), "%s: masked_feat aliases feats (rows are written out of place)", who);
    XGGM_REQUIRE(!overlaps(a.masked_feat, out_bytes, a.pool, a.P * row), "%s: masked_feat aliases pool", who);
    k.vec = row % 16 == 0 && ((uintptr_t)a.feats | (uintptr_t)a.pool | (uintptr_t)a.masked_feat) % 16 == 0;
    const int64_t R = (int64_t)a.B * a.O;
    k.row_blocks = (int)std::min<int64_t>(R, XGGM_PRETRAIN_CORRUPT_ROW_GRID);
    k.tok_blocks = (int)ceil_div64((int64_t)a.B * a.T, NT);
    const int ans_blocks = ceil_div(a.B, NT);
    hipLaunchKernelGGL(pretrain_corrupt_kernel<E>, dim3(k.row_blocks + k.tok_blocks + ans_blocks), dim3(NT), 0, st, k);
    return xggm_check_launch(who);
}
}  // namespace

extern "C" int xggm_pretrain_corrupt_f32(const xggm_pretrain_corrupt_args* args, hipStream_t st) {
    return corrupt<uint32_t>(args, st, "xggm_pretrain_corrupt_f32");
}
extern "C" int xggm_pretrain_corrupt_bf16(const xggm_pretrain_corrupt_args* args, hipStream_t st) {
    return corrupt<uint16_t>(args, st, "xggm_pretrain_corrupt_bf16");
}

extern "C" int xggm_uniform(float* out, int64_t n, const uint64_t* rng, uint32_t sid, hipStream_t st) {
    XGGM_REQUIRE(out && n > 0 && rng, "xggm_uniform: bad arguments");
    hipLaunchKernelGGL(uniform_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n, NT), 4096)), dim3(NT), 0, st, out, n, rng, sid);
    return xggm_check_launch("xggm_uniform");
}
