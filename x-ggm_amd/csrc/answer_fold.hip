// The answer-log fold (xggm_answer_log_fold, include/xggm.h): under data parallelism every rank appends the answers of
// ITS share of a sweep to a log of its own; after the sweep the ranks' packed logs are all-gathered -- one collective per
// sweep or epoch, never per step -- and ONE launch merges them into a destination log in sweep order.  It replaces what the
// reference does on the host for its --multiGPU runs: the per-batch `logit.max(1)[1].cpu()` of every replica's rows
// (src/vqa/vqacpv2.py:180-181, :333-334, gathered by nn.DataParallel, src/lxrt/entry.py:183-184) and the dict the train
// score is computed from (:285).
//
// Nothing is computed: 8-byte labels and 4-byte scores move from position p of rank r to destination d, where (r, p) is
// worked out from d and HOST values alone (the expected counts travel in the kernel arguments).  One thread per
// destination index, grid-stride, so every d in [0, total) is written exactly once and nothing else is; what the device
// cursors hold decides no address.  Thread 0 of workgroup 0 alone reads the ranks' header words, in rank order, and writes
// the destination's header and the flag: one writer, one order, no atomics -- the same bits on every rank.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;
constexpr int MAX_GRID = 2048;
constexpr int MAX_RANKS = XGGM_FOLD_MAX_RANKS;

struct AnswerFoldArgs {
    const int64_t* logs;  // rank r's packed log: logs + r * log_stride
    int64_t log_stride, src_capacity;
    int64_t expect[MAX_RANKS];
    int64_t first[MAX_RANKS];  // CONCAT: destination of rank r's position 0
    int64_t total, block;
    int world, layout, with_scores;
    xggm_answer_log dst;
    int64_t* flag;
};

__global__ __launch_bounds__(NT) void answer_log_fold_kernel(AnswerFoldArgs a) {
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t d = (int64_t)blockIdx.x * NT + threadIdx.x; d < a.total; d += stride) {
        int r = 0;
        int64_t p = d;
        if (a.layout == XGGM_FOLD_CONCAT) {
            // the last rank whose first destination is <= d: uniform loop, the table is read with a uniform index.  An
            // empty rank shares its first destination with its successor and is passed over; d < total ends the walk on
            // a rank that holds position p
            int64_t base = 0;
            for (int q = 1; q < a.world; ++q) {
                const int64_t f = a.first[q];
                if (d >= f) {
                    r = q;
                    base = f;
                }
            }
            p = d - base;
        } else {
            const int64_t blk = d / a.block;
            r = (int)(blk % a.world);
            p = (blk / a.world) * a.block + d % a.block;
        }
        const int64_t* src = a.logs + (int64_t)r * a.log_stride + 3;
        a.dst.labels[d] = src[p];
        if (a.with_scores) a.dst.scores[d] = reinterpret_cast<const float*>(src + a.src_capacity)[p];
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sum = 0.0;
    int64_t bits = 0, bad_rank = -1;
    for (int r = 0; r < a.world; ++r) {
        const int64_t* h = a.logs + (int64_t)r * a.log_stride;
        const bool cursor_off = h[0] != a.expect[r], refused = h[2] != 0;
        sum = sum + __longlong_as_double(h[1]);
        bits |= (cursor_off ? 1 : 0) | (refused ? 2 : 0);
        if ((cursor_off || refused) && bad_rank < 0) bad_rank = r;
    }
    *a.dst.cursor = a.total;
    if (a.dst.score_sum) *a.dst.score_sum = sum;
    *a.dst.flags = 0;
    *a.flag = bits ? (bits | (bad_rank << 8)) : 0;
}

inline bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }
// [p, p + bytes) meets [q, q + qbytes)
inline bool meets(const void* p, size_t bytes, const void* q, size_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && bytes && a < b + qbytes && b < a + bytes;
}
}  // namespace

extern "C" int xggm_answer_log_fold(const int64_t* logs, int64_t log_stride, int64_t src_capacity, int with_scores, int world,
                                    int layout, int64_t block, const int64_t* expect, xggm_answer_log* dst, int64_t* flag,
                                    hipStream_t st) {
    XGGM_REQUIRE(logs && expect && dst && flag, "xggm_answer_log_fold: null logs / expect / dst / flag");
    XGGM_REQUIRE(dst->labels && dst->cursor && dst->flags, "xggm_answer_log_fold: the destination needs labels, cursor and flags");
    XGGM_REQUIRE(world >= 1 && world <= MAX_RANKS, "xggm_answer_log_fold: world = %d (1 <= world <= %d)", world, MAX_RANKS);
    XGGM_REQUIRE(layout == XGGM_FOLD_CONCAT || layout == XGGM_FOLD_INTERLEAVE, "xggm_answer_log_fold: unknown layout %d", layout);
    XGGM_REQUIRE(src_capacity >= 1 && src_capacity < ((int64_t)1 << 40), "xggm_answer_log_fold: src_capacity = %lld",
                 (long long)src_capacity);
    XGGM_REQUIRE(dst->capacity >= 1 && dst->capacity < ((int64_t)1 << 40), "xggm_answer_log_fold: destination capacity = %lld",
                 (long long)dst->capacity);
    AnswerFoldArgs a;
    int64_t total = 0;
    for (int r = 0; r < MAX_RANKS; ++r) {
        a.expect[r] = r < world ? expect[r] : 0;
        a.first[r] = total;
        if (r >= world) continue;
        XGGM_REQUIRE(expect[r] >= 0 && expect[r] <= src_capacity, "xggm_answer_log_fold: expect[%d] = %lld outside [0, src_capacity %lld]",
                     r, (long long)expect[r], (long long)src_capacity);
        total += expect[r];
    }
    XGGM_REQUIRE(total >= 1 && total <= dst->capacity, "xggm_answer_log_fold: %lld answers in all (1 <= total <= capacity %lld)",
                 (long long)total, (long long)dst->capacity);
    if (layout == XGGM_FOLD_INTERLEAVE) {
        XGGM_REQUIRE(block >= 1, "xggm_answer_log_fold: block = %lld (interleave needs block >= 1)", (long long)block);
        for (int r = 0; r < world; ++r)
            XGGM_REQUIRE(expect[r] == expect[0] && expect[r] % block == 0,
                         "xggm_answer_log_fold: interleave needs equal counts that are multiples of block %lld (expect[%d] = %lld, "
                         "expect[0] = %lld)", (long long)block, r, (long long)expect[r], (long long)expect[0]);
    }
    XGGM_REQUIRE(!with_scores || dst->scores, "xggm_answer_log_fold: with_scores needs dst->scores");
    const int64_t words = 3 + src_capacity + (with_scores ? (src_capacity + 1) / 2 : 0);
    XGGM_REQUIRE(log_stride >= words, "xggm_answer_log_fold: log_stride %lld shorter than one packed log of %lld words",
                 (long long)log_stride, (long long)words);
    XGGM_REQUIRE(aligned(logs, 8) && aligned(dst->labels, 8) && aligned(dst->cursor, 8) && aligned(dst->score_sum, 8) &&
                     aligned(flag, 8),
                 "xggm_answer_log_fold: logs, labels, cursor, score_sum and flag must be 8-byte aligned");
    XGGM_REQUIRE(aligned(dst->scores, 4) && aligned(dst->flags, 4), "xggm_answer_log_fold: scores and flags must be 4-byte aligned");
    const size_t span = (size_t)((world - 1) * log_stride + words) * 8, cap = (size_t)dst->capacity;
    XGGM_REQUIRE(!meets(dst->labels, cap * 8, logs, span) && !meets(dst->scores, cap * 4, logs, span) &&
                     !meets(dst->cursor, 8, logs, span) && !meets(dst->score_sum, 8, logs, span) &&
                     !meets(dst->flags, 4, logs, span) && !meets(flag, 8, logs, span),
                 "xggm_answer_log_fold: the destination's buffers and the flag must not overlap the gathered logs");
    a.logs = logs, a.log_stride = log_stride, a.src_capacity = src_capacity;
    a.total = total, a.block = layout == XGGM_FOLD_INTERLEAVE ? block : 1;
    a.world = world, a.layout = layout, a.with_scores = with_scores ? 1 : 0;
    a.dst = *dst;
    a.flag = flag;
    const int grid = (int)std::min<int64_t>((total + NT - 1) / NT, MAX_GRID);
    hipLaunchKernelGGL(answer_log_fold_kernel, dim3(grid), dim3(NT), 0, st, a);
    return xggm_check_launch("xggm_answer_log_fold");
}
