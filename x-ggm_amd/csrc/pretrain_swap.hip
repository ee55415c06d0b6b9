// Matched-sentence swap of LXMERT pre-training on the device: what LXMERTTorchDataset.__getitem__ does per example with
// Python's random (src/pretrain/lxmert_data.py:173-183), for a whole clean batch in ONE launch (contract:
// xggm_pretrain_swap in xggm.h).  One wave per row: the decision of a row is the same in every lane (it goes through SGPRs),
// so every branch below is uniform within a wave.  Every decision is taken in double from the fp32 draw, the IEEE
// operations the reference performs on Python floats; rows are only moved, nothing is rounded.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256, WAVE = 64, ROWS = NT / WAVE;  // rows per workgroup
typedef int i4 __attribute__((ext_vector_type(4)));

struct SwapK {
    xggm_pretrain_swap_args a;  // pool / P resolved
    int vec;                    // rows move as 16-byte vectors
};

__device__ __forceinline__ float uniform_lane(float v) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
// draw `k` (5: u_swap, 6: u_pick) of element idx: the supplied buffer, else Philox stream sid_base + k
__device__ __forceinline__ float draw_of(const float* buf, const xggm_pretrain_swap_args& a, uint32_t k, uint64_t idx) {
    if (buf) return uniform_lane(buf[idx]);
    return uniform_lane(philox_uniform(a.rng[0], a.rng[1], a.sid_base + k, idx));
}
// floor(u * n) in double, held inside [0, n): a supplied draw outside [0, 1) must not become an address
__device__ __forceinline__ int64_t pick_of(float u, int64_t n) {
    const double v = (double)u * (double)n;
    int64_t i = v >= 0.0 ? (int64_t)v : 0;
    return i > n - 1 ? n - 1 : i;
}

__device__ __forceinline__ void move_row(const int64_t* src, int64_t* dst, int T, int vec, int lane) {
    if (vec) {
        const int nvec = T / 2;
        const i4* s = reinterpret_cast<const i4*>(src);
        i4* d = reinterpret_cast<i4*>(dst);
        for (int i = lane; i < nvec; i += WAVE) d[i] = s[i];
    } else {
        for (int i = lane; i < T; i += WAVE) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(NT) void pretrain_swap_kernel(const SwapK k) {
    const xggm_pretrain_swap_args& a = k.a;
    const int lane = threadIdx.x % WAVE;
    const int64_t b = (int64_t)blockIdx.x * ROWS + threadIdx.x / WAVE;
    if (b >= a.B) return;
    const int64_t m_in = a.matched_in ? a.matched_in[b] : 1;
    int64_t matched = m_in;
    const int64_t* src_ids = a.ids + b * a.T;
    const int64_t* src_mask = a.mask + b * a.T;
    if (m_in == 1 && (double)draw_of(a.u_swap, a, 5, (uint64_t)b) < a.rate) {  // :178
        const int64_t own = a.img[b];
        bool found = false;
        for (int r = 0; r < XGGM_PRETRAIN_SWAP_TRIES && !found; ++r) {  // :180-182, bounded
            const int64_t j = pick_of(draw_of(a.u_pick, a, 6, (uint64_t)b * XGGM_PRETRAIN_SWAP_TRIES + r), a.P);
            if (a.pool_img[j] != own) {
                found = true;
                matched = 0;
                src_ids = a.pool_ids + j * a.T;
                src_mask = a.pool_mask + j * a.T;
            }
        }
        if (!found && lane == 0) atomicAdd(a.exhausted, 1);
    }
    move_row(src_ids, a.out_ids + b * a.T, a.T, k.vec, lane);
    move_row(src_mask, a.out_mask + b * a.T, a.T, k.vec, lane);
    if (lane == 0) a.is_matched[b] = matched;
}

bool overlaps(const void* p, int64_t np, const void* q, int64_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
}  // namespace

extern "C" int xggm_pretrain_swap(const xggm_pretrain_swap_args* args, hipStream_t st) {
    const char* who = "xggm_pretrain_swap";
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    SwapK k;
    k.a = *args;
    xggm_pretrain_swap_args& a = k.a;
    XGGM_REQUIRE(a.B > 0 && a.T > 0, "%s: B=%d T=%d must both be positive", who, a.B, a.T);
    XGGM_REQUIRE((int64_t)a.B * a.T < (1ll << 31), "%s: B T must stay below 2^31", who);
    XGGM_REQUIRE(a.ids && a.mask && a.img, "%s: null ids / mask / img", who);
    XGGM_REQUIRE(a.out_ids && a.out_mask && a.is_matched && a.exhausted, "%s: null output pointer", who);
    const int n_pool = (a.pool_ids != nullptr) + (a.pool_mask != nullptr) + (a.pool_img != nullptr);
    XGGM_REQUIRE(n_pool == 0 || n_pool == 3, "%s: a pool needs pool_ids, pool_mask and pool_img (%d of 3 given)", who, n_pool);
    XGGM_REQUIRE(a.rate >= 0.0 && a.rate <= 1.0, "%s: rate %g outside [0, 1]", who, a.rate);
    XGGM_REQUIRE(a.rng || (a.u_swap && a.u_pick), "%s: a null draw buffer needs rng", who);
    if (!n_pool) {
        a.pool_ids = a.ids;
        a.pool_mask = a.mask;
        a.pool_img = a.img;
        a.P = a.B;
    }
    XGGM_REQUIRE(a.P > 0, "%s: pool of %lld rows", who, (long long)a.P);
    const int64_t row = (int64_t)a.T * 8, out_bytes = (int64_t)a.B * row, vec_bytes = (int64_t)a.B * 8;
    // every output against every other buffer the launch reads or writes: rows are written out of place while other waves
    // still read theirs (a NULL pool IS the batch), and two outputs that share bytes would overwrite each other
    const void* outs[4] = {a.out_ids, a.out_mask, a.is_matched, a.exhausted};
    const int64_t out_n[4] = {out_bytes, out_bytes, vec_bytes, 4};
    const void* ins[7] = {a.ids, a.mask, a.pool_ids, a.pool_mask, a.img, a.pool_img, a.matched_in};
    const int64_t in_n[7] = {out_bytes, out_bytes, a.P * row, a.P * row, vec_bytes, a.P * 8, vec_bytes};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 7; ++i)
            XGGM_REQUIRE(!ins[i] || !overlaps(outs[o], out_n[o], ins[i], in_n[i]),
                         "%s: an output aliases ids / mask / img / matched_in / pool (everything is written out of place)", who);
        for (int q = o + 1; q < 4; ++q)
            XGGM_REQUIRE(!overlaps(outs[o], out_n[o], outs[q], out_n[q]), "%s: two outputs alias each other", who);
    }
    k.vec = row % 16 == 0 && ((uintptr_t)a.ids | (uintptr_t)a.mask | (uintptr_t)a.pool_ids | (uintptr_t)a.pool_mask |
                              (uintptr_t)a.out_ids | (uintptr_t)a.out_mask) % 16 == 0;
    hipLaunchKernelGGL(pretrain_swap_kernel, dim3(ceil_div(a.B, ROWS)), dim3(NT), 0, st, k);
    return xggm_check_launch(who);
}
