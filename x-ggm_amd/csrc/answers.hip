// The answer log (xggm_answer_pick_f32, include/xggm.h): arg-max of every logit row of a batch, appended -- with the
// row's soft score and a running score sum when a target is given -- to buffers that stay on the device.  It replaces
// the reference's `logit.max(1)[1].cpu()` per training iteration (src/vqa/vqacpv2.py:180-181) and per validation
// batch (:333-334): the host reads the log once per sweep or epoch instead of once per batch.
//
// One workgroup per row (several rows per workgroup past PICK_GRID rows): a row is 7 ... 12.5 KB, so 256 threads hold
// it in at most four 16-byte loads each, all issued before the first is used.  (value, index) pairs travel as ONE
// 64-bit integer whose unsigned order IS the rule of torch.max -- greater wins, equal keeps the smaller index, NaN
// beats everything, the earlier NaN beats the later one -- so the reduction is a plain u64 maximum: DPP inside a wave,
// LDS across the four waves.  The labels are stored by wave 0, one lane per row of the workgroup, the scores with
// write-through stores; the workgroup that draws the last ticket of common.h::ordered_grid_sum then adds the scores
// in row order and advances the cursor.  Every workgroup has read the cursor before it stored and before it took its
// ticket, and the cursor moves only after the last ticket.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;
constexpr int PICK_GRID = 128;    // workgroups: each one pays a ticket (the capped loss grids of loss_optim.hip)
constexpr int PICK_ROWS = 64;     // rows per workgroup at most: wave 0 stores them, one lane each
constexpr int PICK_MAX_B = 4096 * PICK_ROWS;  // the ticket workspace holds 4096 partials
constexpr int SUM_CHUNK = 1024;   // scores the finishing workgroup stages in LDS per round

// key of (value, index): the order of torch.max as an unsigned comparison.  High word: the float's bits made monotone
// (sign flipped for positives, all bits for negatives; -0 counts as +0), 0xFFFFFFFF for every NaN -- above +inf.  Low
// word: ~index, so that among equal values the smaller index is the larger key.  0 is below every real key.
__device__ __forceinline__ uint64_t pick_key(float v, uint32_t idx) {
    uint32_t b = __float_as_uint(v), k;
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) {
        k = 0xFFFFFFFFu;
    } else {
        if (b == 0x80000000u) b = 0u;
        k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((uint64_t)k << 32) | (uint32_t)~idx;
}
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// every lane active (the pattern of wave_max in common.h)
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = umax64(v, dpp_move64<0xB1>(v));
    v = umax64(v, dpp_move64<0x4E>(v));
    v = umax64(v, dpp_move64<0x141>(v));
    v = umax64(v, dpp_move64<0x140>(v));
    return umax64(umax64(lane64(v, 0), lane64(v, 16)), umax64(lane64(v, 32), lane64(v, 48)));
}

__global__ __launch_bounds__(NT) void answer_pick_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                         const float* __restrict__ target, int64_t target_stride, int B, int A,
                                                         const int* __restrict__ rows, xggm_answer_log lg, float* ws) {
    __shared__ uint64_t s_best[2][NT / 64];
    __shared__ int s_label[PICK_ROWS];
    __shared__ int s_fin;
    __shared__ float s_sc[SUM_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = rows ? min(max(*rows, 0), B) : B;
    const int64_t c = *lg.cursor;
    const bool fits = c >= 0 && c + n <= lg.capacity;

    if (fits) {
        int it = 0;
        for (int row = blockIdx.x; row < n; row += gridDim.x, ++it) {
            const float* __restrict__ p = logits + (int64_t)row * row_stride;
            // floats in front of the first 16-byte boundary (rows are only 4-byte aligned: A is odd or 2 mod 4 more
            // often than not), the 16-byte body, up to three floats behind it
            int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
            if (head > A) head = A;
            const int n4 = (A - head) >> 2, tail0 = head + (n4 << 2);
            const float4* __restrict__ q = reinterpret_cast<const float4*>(p + head);
            const bool has_h = tid < head, has_t = tid < A - tail0;
            float hv = 0.f, tv = 0.f;
            if (has_h) hv = p[tid];
            if (has_t) tv = p[tail0 + tid];
            uint64_t best = 0;
            for (int j0 = 0; j0 < n4; j0 += 4 * NT) {  // one round for A <= 4096
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * NT + tid;
                    v[u] = j < n4 ? q[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * NT + tid;
                    if (j < n4) {
                        const uint32_t i0 = (uint32_t)(head + (j << 2));
                        best = umax64(umax64(best, pick_key(v[u].x, i0)), pick_key(v[u].y, i0 + 1u));
                        best = umax64(umax64(best, pick_key(v[u].z, i0 + 2u)), pick_key(v[u].w, i0 + 3u));
                    }
                }
            }
            if (has_h) best = umax64(best, pick_key(hv, (uint32_t)tid));
            if (has_t) best = umax64(best, pick_key(tv, (uint32_t)(tail0 + tid)));
            best = wave_max_u64(best);
            // two buffers by parity: the barrier of the NEXT row stands between thread 0's reads and the overwriting
            if (lane == 0) s_best[it & 1][wid] = best;
            __syncthreads();
            if (tid == 0) {
                const uint64_t m = umax64(umax64(s_best[it & 1][0], s_best[it & 1][1]), umax64(s_best[it & 1][2], s_best[it & 1][3]));
                s_label[it] = (int)~(uint32_t)m;
            }
        }
        __syncthreads();
        // wave 0 stores the workgroup's rows, lane k its k-th: the look-ups in the target run side by side, and thread
        // 0's wait in front of its ticket (ordered_grid_sum) covers every store of its wave
        const int row = blockIdx.x + lane * gridDim.x;
        if (wid == 0 && row < n) {
            const int label = s_label[lane];
            lg.labels[c + row] = label;
            if (target)
                __hip_atomic_store(lg.scores + c + row, target[(int64_t)row * target_stride + label], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    float unused;
    const bool fin = ordered_grid_sum(0.f, ws, gridDim.x, blockIdx.x, unused);
    if (tid == 0) s_fin = fin ? 1 : 0;
    __syncthreads();
    if (!s_fin) return;
    // the finishing workgroup: every other one has read the cursor, stored and drawn its ticket
    if (!fits) {
        if (tid == 0) {
            const int f = *lg.flags;
            *lg.flags = (f | 1) + (f < 0x7FFFFFFC ? 2 : 0);
        }
        return;
    }
    if (target && lg.score_sum) {
        // the scores come back with device-scope loads (they were written through, past the other XCDs' L2), a chunk at
        // a time into LDS; ONE thread adds them in row order
        double s = tid == 0 ? *lg.score_sum : 0.0;
        for (int r0 = 0; r0 < n; r0 += SUM_CHUNK) {
            const int m = min(SUM_CHUNK, n - r0);
            for (int i = tid; i < m; i += NT)
                s_sc[i] = __hip_atomic_load(lg.scores + c + r0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (tid == 0)
                for (int i = 0; i < m; ++i) s += (double)s_sc[i];
            __syncthreads();
        }
        if (tid == 0) *lg.score_sum = s;
    }
    if (tid == 0) *lg.cursor = c + n;
}
}  // namespace

extern "C" int xggm_answer_pick_f32(const float* logits, int64_t row_stride, const float* target, int64_t target_stride, int B,
                                    int A, const int* rows, xggm_answer_log* log, float* ws, hipStream_t st) {
    XGGM_REQUIRE(logits && log && ws, "xggm_answer_pick_f32: null logits / log / workspace");
    XGGM_REQUIRE(log->labels && log->cursor && log->flags, "xggm_answer_pick_f32: the log needs labels, cursor and flags");
    XGGM_REQUIRE(A > 0 && B > 0 && B <= PICK_MAX_B, "xggm_answer_pick_f32: bad shape (B = %d, A = %d; 0 < B <= %d, A > 0)", B, A,
                 PICK_MAX_B);
    XGGM_REQUIRE(row_stride >= A, "xggm_answer_pick_f32: row_stride %lld below A = %d", (long long)row_stride, A);
    XGGM_REQUIRE(!target || log->scores, "xggm_answer_pick_f32: a target needs log->scores");
    XGGM_REQUIRE(!target || target_stride >= A, "xggm_answer_pick_f32: target_stride %lld below A = %d", (long long)target_stride,
                 A);
    XGGM_REQUIRE(log->capacity >= 0, "xggm_answer_pick_f32: negative capacity");
    XGGM_REQUIRE(reinterpret_cast<uintptr_t>(logits) % 4 == 0 && reinterpret_cast<uintptr_t>(target) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(log->scores) % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(log->flags) % 4 == 0,
                 "xggm_answer_pick_f32: logits, target, scores, rows and flags must be 4-byte aligned");
    XGGM_REQUIRE(reinterpret_cast<uintptr_t>(log->labels) % 8 == 0 && reinterpret_cast<uintptr_t>(log->cursor) % 8 == 0 &&
                     reinterpret_cast<uintptr_t>(log->score_sum) % 8 == 0,
                 "xggm_answer_pick_f32: labels, cursor and score_sum must be 8-byte aligned");
    const int grid = std::max(std::min(B, PICK_GRID), ceil_div(B, PICK_ROWS));
    hipLaunchKernelGGL(answer_pick_kernel, dim3(grid), dim3(NT), 0, st, logits, row_stride, target, target_stride, B, A, rows, *log,
                       ws);
    return xggm_check_launch("xggm_answer_pick_f32");
}
