// 64-bit fingerprints of byte ranges of device memory (xggm_fingerprint_spans, include/xggm.h): the replica drift guard
// of the data-parallel path (dist.ReplicaGuard) compares one word per (buffer, arena group) across the ranks instead of
// the buffers themselves.  Integer arithmetic only: the fingerprint is a sum mod 2^64 of per-word contributions, so how
// a range is cut among lanes, waves and workgroups cannot change a bit of it.
//
// A read-only stream: one 16-byte load per lane and step, four in flight, a 64-bit accumulator per lane, DPP wave
// reduction, one partial per workgroup in the caller's workspace; a second, tiny launch adds the partials of every
// range and writes EVERY output word (empty ranges: 0).  Per 32-bit word the loop spends one v_mul_lo_u32, one
// v_mad_u64_u32 and a handful of full-rate integer instructions (DESIGN.md section 6 has the count against the HBM rate).
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;
constexpr int MAX_FP_SPANS = 64;      // ranges per grid (the table travels as a kernel argument)
constexpr int DEFAULT_FP_WGS = 2048;  // 256 CUs x 8 resident workgroups of 256 threads
constexpr uint32_t GOLD = 0x9E3779B9u, MIXMUL = 0x7FEB352Du;

struct FpSpans {
    const uint32_t* ptr[MAX_FP_SPANS];
    int64_t words[MAX_FP_SPANS];
    uint32_t salt[MAX_FP_SPANS];
    int blk0[MAX_FP_SPANS + 1];
    int n;
};

// contribution of word `w` at index idx: `ks` = idx * GOLD + salt, `odd` = 2 * (idx mod 2^31) + 1
__device__ __forceinline__ uint64_t fp_word(uint32_t w, uint32_t ks, uint32_t odd) {
    uint32_t x = (w ^ ks) * MIXMUL;
    x ^= x >> 15;
    return (uint64_t)x * (uint64_t)odd;
}

// wrapping sum over the wave, every lane active (the pattern of wave_sum in common.h)
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    v += dpp_move64<0xB1>(v);
    v += dpp_move64<0x4E>(v);
    v += dpp_move64<0x141>(v);
    v += dpp_move64<0x140>(v);
    return (lane64(v, 0) + lane64(v, 16)) + (lane64(v, 32) + lane64(v, 48));
}

typedef uint32_t __attribute__((ext_vector_type(4))) u4;

__device__ __forceinline__ uint64_t fp_vec(const u4 v, uint32_t ks, uint32_t odd) {
    return (fp_word(v.x, ks, odd) + fp_word(v.y, ks + GOLD, odd + 2u)) +
           (fp_word(v.z, ks + 2u * GOLD, odd + 4u) + fp_word(v.w, ks + 3u * GOLD, odd + 6u));
}

__global__ __launch_bounds__(NT) void fingerprint_kernel(FpSpans sp, uint64_t* __restrict__ ws) {
    int k = 0;
    for (int j = 1; j < sp.n; ++j)
        if ((int)blockIdx.x >= sp.blk0[j]) k = j;
    const uint32_t* __restrict__ p = sp.ptr[k];
    const int64_t W = sp.words[k];
    const uint32_t salt = sp.salt[k];
    const int b = blockIdx.x - sp.blk0[k], nb = sp.blk0[k + 1] - sp.blk0[k];
    // words in front of the first 16-byte boundary (the pointer is 4-byte aligned), 16-byte body, up to three words behind
    int64_t head = (int64_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
    if (head > W) head = W;
    const int64_t n4 = (W - head) >> 2, tail0 = head + (n4 << 2);
    const u4* __restrict__ q = reinterpret_cast<const u4*>(p + head);
    const int64_t stride = (int64_t)nb * NT;
    uint64_t acc = 0;
    int64_t i = (int64_t)b * NT + threadIdx.x;
    // index of the vector's first word, times GOLD plus salt, and its odd factor 2 * (idx mod 2^31) + 1: all of them
    // advance by constants, in wrapping 32-bit arithmetic (the contract takes the index mod 2^32 / mod 2^31)
    const uint32_t idx = (uint32_t)(head + (i << 2));
    uint32_t ks = idx * GOLD + salt, odd = (idx << 1) | 1u;
    const uint32_t d_idx = (uint32_t)(stride << 2), d_ks = d_idx * GOLD, d_odd = d_idx << 1;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const u4 a = __builtin_nontemporal_load(q + i), bb = __builtin_nontemporal_load(q + i + stride),
                 c = __builtin_nontemporal_load(q + i + 2 * stride), d = __builtin_nontemporal_load(q + i + 3 * stride);
        acc += (fp_vec(a, ks, odd) + fp_vec(bb, ks + d_ks, odd + d_odd)) +
               (fp_vec(c, ks + 2u * d_ks, odd + 2u * d_odd) + fp_vec(d, ks + 3u * d_ks, odd + 3u * d_odd));
        ks += 4u * d_ks;
        odd += 4u * d_odd;
    }
    for (; i < n4; i += stride) {
        acc += fp_vec(q[i], ks, odd);
        ks += d_ks;
        odd += d_odd;
    }
    if (b == 0) {
        const int64_t t = threadIdx.x;
        if (t < head) {
            const uint32_t j = (uint32_t)t;
            acc += fp_word(p[t], j * GOLD + salt, (j << 1) | 1u);
        }
        if (t < W - tail0) {
            const uint32_t j = (uint32_t)(tail0 + t);
            acc += fp_word(p[tail0 + t], j * GOLD + salt, (j << 1) | 1u);
        }
    }
    acc = wave_sum_u64(acc);
    __shared__ uint64_t s_red[NT / 64];
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// one wave per range: its partials added (any order gives the same word), the output word written even when the
// range is empty
__global__ __launch_bounds__(64) void fingerprint_finish_kernel(FpSpans sp, const uint64_t* __restrict__ ws,
                                                                 uint64_t* __restrict__ out) {
    const int k = blockIdx.x;
    uint64_t acc = 0;
    for (int b = sp.blk0[k] + threadIdx.x; b < sp.blk0[k + 1]; b += 64) acc += ws[b];
    acc = wave_sum_u64(acc);
    if (threadIdx.x == 0) out[k] = acc;
}
}  // namespace

extern "C" size_t xggm_fingerprint_workspace_bytes(int n_spans, int max_workgroups) {
    (void)n_spans;  // the ranges of a call go through the workspace MAX_FP_SPANS at a time
    const int cap = max_workgroups > 0 ? max_workgroups : DEFAULT_FP_WGS;
    return sizeof(uint64_t) * ((size_t)cap + MAX_FP_SPANS);
}

extern "C" int xggm_fingerprint_spans(const xggm_fp_span* spans, int n_spans, uint64_t* out, void* ws, size_t ws_bytes,
                                      int max_workgroups, hipStream_t st) {
    XGGM_REQUIRE(n_spans >= 0 && max_workgroups >= 0, "xggm_fingerprint_spans: bad arguments (n_spans = %d, max_workgroups = %d)",
                 n_spans, max_workgroups);
    if (n_spans == 0) return XGGM_OK;
    XGGM_REQUIRE(spans && out && ws, "xggm_fingerprint_spans: null spans / out / workspace");
    XGGM_REQUIRE(reinterpret_cast<uintptr_t>(out) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 8 == 0,
                 "xggm_fingerprint_spans: out and workspace must be 8-byte aligned");
    XGGM_REQUIRE(ws_bytes >= xggm_fingerprint_workspace_bytes(n_spans, max_workgroups),
                 "xggm_fingerprint_spans: workspace of %zu bytes, xggm_fingerprint_workspace_bytes asks for %zu", ws_bytes,
                 xggm_fingerprint_workspace_bytes(n_spans, max_workgroups));
    for (int i = 0; i < n_spans; ++i) {
        XGGM_REQUIRE(spans[i].bytes >= 0 && spans[i].bytes % 4 == 0, "xggm_fingerprint_spans: span %d: %lld bytes (a non-negative "
                     "multiple of 4 is required)", i, (long long)spans[i].bytes);
        XGGM_REQUIRE(spans[i].bytes == 0 || spans[i].ptr, "xggm_fingerprint_spans: span %d: null pointer", i);
        XGGM_REQUIRE(reinterpret_cast<uintptr_t>(spans[i].ptr) % 4 == 0, "xggm_fingerprint_spans: span %d: pointer must be "
                     "4-byte aligned", i);
    }
    const int cap = max_workgroups > 0 ? max_workgroups : DEFAULT_FP_WGS;
    for (int c0 = 0; c0 < n_spans; c0 += MAX_FP_SPANS) {
        const int n = std::min(MAX_FP_SPANS, n_spans - c0);
        FpSpans sp;
        sp.n = n;
        int64_t total = 0;
        for (int i = 0; i < n; ++i) total += spans[c0 + i].bytes >> 2;
        // `cap` workgroups shared out by length, at least 8 loads per thread where a range is long enough, at least one
        // workgroup per non-empty range: never more than cap + n partials
        int nblk = 0;
        for (int i = 0; i < MAX_FP_SPANS; ++i) {
            const int64_t W = i < n ? spans[c0 + i].bytes >> 2 : 0;
            sp.ptr[i] = i < n ? static_cast<const uint32_t*>(spans[c0 + i].ptr) : nullptr;
            sp.words[i] = W;
            sp.salt[i] = i < n ? spans[c0 + i].salt : 0u;
            sp.blk0[i] = nblk;
            if (W > 0)
                nblk += (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(W, (int64_t)NT * 32),
                                                                   (int64_t)((double)cap * (double)W / (double)total)));
        }
        sp.blk0[MAX_FP_SPANS] = nblk;
        XGGM_REQUIRE(nblk <= cap + n, "xggm_fingerprint_spans: internal: %d partials for %d workgroups", nblk, cap);
        if (nblk > 0)
            hipLaunchKernelGGL(fingerprint_kernel, dim3(nblk), dim3(NT), 0, st, sp, static_cast<uint64_t*>(ws));
        hipLaunchKernelGGL(fingerprint_finish_kernel, dim3(n), dim3(64), 0, st, sp, static_cast<const uint64_t*>(ws), out + c0);
    }
    return xggm_check_launch("xggm_fingerprint_spans");
}
