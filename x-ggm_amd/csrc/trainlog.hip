// The training log (xggm_train_log_append, include/xggm.h): one record per optimiser pass -- the loss and its terms,
// the pre-clip gradient norm, the schedule value -- appended to a ring that stays on the device, with running fp64 sums
// per pass kind and the index of the first record that holds a non-finite value.  It replaces the per-iteration reads
// of the reference's loop, `total_loss += loss.detach() / logit.size(0)` (src/vqa/vqacpv2.py:179) and the scalars it
// hands to tensorboard (:256-270): the host reads the log once per N iterations or per epoch.
//
// Nothing is computed: the values already sit in device scalars that earlier launches of the stream wrote (the loss
// kernels' slots, the norm's finishing launch, the schedule table).  One workgroup of one wave; lanes 0 .. COLS - 1 fetch
// one column each so that the loads are in flight together, then lane 0 alone stores the row, adds to the sums in column
// order and moves the cursor -- one writer, one order, hence the same bits eagerly, replayed from a graph or beside other
// work.  Launches that share a log are ordered by their stream; nothing is exchanged inside a launch.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int COLS = XGGM_TRAINLOG_COLS;
constexpr int KINDS = XGGM_TRAINLOG_KINDS;

struct TrainLogArgs {
    const float* src[COLS];  // NULL = column absent
    float mul[COLS];
    int kind;
    const int64_t* step;  // or NULL
    xggm_train_log log;
};

__global__ __launch_bounds__(64) void train_log_append_kernel(TrainLogArgs a) {
    __shared__ float s_v[COLS];
    __shared__ int s_present[COLS];
    const int lane = threadIdx.x;
    if (blockIdx.x != 0) return;
    if (lane < COLS) {
        const float* p = nullptr;
        float m = 1.f;
#pragma unroll
        for (int i = 0; i < COLS; ++i)  // constant indices: the argument block stays in registers
            if (lane == i) {
                p = a.src[i];
                m = a.mul[i];
            }
        s_present[lane] = p != nullptr;
        s_v[lane] = p ? *p * m : 0.f;
    }
    __syncthreads();
    if (lane != 0) return;
    const xggm_train_log& lg = a.log;
    const int64_t r = *lg.cursor;
    // unsigned: whatever the cursor word holds, the row index stays inside [0, capacity)
    const int64_t row = (int64_t)((uint64_t)r % (uint64_t)lg.capacity);
    double* sums = lg.sums + a.kind * COLS;
    int mask = 0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        const float v = s_v[i];
        lg.values[row * COLS + i] = v;
        if (s_present[i]) {
            mask |= 1 << i;
            sums[i] = sums[i] + (double)v;
            bad |= (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;  // inf or NaN
        }
    }
    if (lg.steps && a.step) lg.steps[row] = *a.step;
    lg.kinds[row] = a.kind | (mask << 8);
    lg.counts[a.kind] += 1;
    if (bad && *lg.first_bad < 0) *lg.first_bad = r;
    *lg.cursor = r + 1;
}

inline bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }
}  // namespace

extern "C" int xggm_train_log_append(const float* const* src, const float* mul, int n, int kind, const int64_t* step,
                                     xggm_train_log* log, hipStream_t st) {
    XGGM_REQUIRE(src && log, "xggm_train_log_append: null column array / log");
    XGGM_REQUIRE(n > 0 && n <= COLS, "xggm_train_log_append: n = %d columns (0 < n <= %d)", n, COLS);
    XGGM_REQUIRE(kind >= 0 && kind < KINDS, "xggm_train_log_append: kind = %d (0 <= kind < %d)", kind, KINDS);
    XGGM_REQUIRE(log->capacity > 0, "xggm_train_log_append: capacity = %lld must be positive", (long long)log->capacity);
    XGGM_REQUIRE(log->values && log->kinds && log->cursor && log->sums && log->counts && log->first_bad,
                 "xggm_train_log_append: the log needs values, kinds, cursor, sums, counts and first_bad");
    XGGM_REQUIRE(aligned(log->steps, 8) && aligned(log->cursor, 8) && aligned(log->sums, 8) && aligned(log->counts, 8) &&
                     aligned(log->first_bad, 8) && aligned(step, 8),
                 "xggm_train_log_append: steps, cursor, sums, counts, first_bad and step must be 8-byte aligned");
    XGGM_REQUIRE(aligned(log->values, 4) && aligned(log->kinds, 4), "xggm_train_log_append: values and kinds must be 4-byte aligned");
    TrainLogArgs a;
    for (int i = 0; i < COLS; ++i) {
        a.src[i] = i < n ? src[i] : nullptr;
        a.mul[i] = (i < n && mul) ? mul[i] : 1.f;
        XGGM_REQUIRE(aligned(a.src[i], 4), "xggm_train_log_append: column %d is not 4-byte aligned", i);
    }
    a.kind = kind;
    a.step = step;
    a.log = *log;
    hipLaunchKernelGGL(train_log_append_kernel, dim3(1), dim3(64), 0, st, a);
    return xggm_check_launch("xggm_train_log_append");
}
