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

// The fold (xggm_train_log_fold, include/xggm.h): data-parallel pre-training keeps one log per rank; at read-back time the
// ranks' rings are all-gathered and ONE launch replaces this rank's n records by their mean over the ranks -- the
// reference's `loss.mean()` / `losses.mean(0)` over its replicas (src/pretrain/lxmert_pretrain.py:311-313, :323-325) --
// so that every rank reads the same numbers.  One workgroup: thread i (strided) owns record i, adds its `world` values
// per column in rank order and scales once; after the barrier threads 0 .. KINDS * COLS - 1 own one running sum each and
// add the folded records in record order, as the appends would have.  Fixed orders, no floating-point atomics: the
// same bits on every rank.  The two integer minima (first disagreeing record, first non-finite record) go through LDS.
struct TrainLogFoldArgs {
    const float* vals;       // rank r, record i, column c: vals[r * val_stride + i * COLS + c]
    const int32_t* kinds;    // kinds[r * kind_stride + i]: kind | (present mask << 8)
    const int64_t* steps;    // steps[r * step_stride + i], or NULL
    const int64_t* cursors;  // cursors[r * cursor_stride], or NULL
    int64_t val_stride, kind_stride, step_stride, cursor_stride;
    int world, n;
    float inv;  // 1 / world
    xggm_train_log log;
    int64_t* flag;
};

constexpr int FOLD_THREADS = 256;
constexpr int NONE = 0x7FFFFFFF;

__global__ __launch_bounds__(FOLD_THREADS) void train_log_fold_kernel(TrainLogFoldArgs a) {
    __shared__ int s_differ, s_bad;
    const int tid = threadIdx.x;
    if (blockIdx.x != 0) return;
    if (tid == 0) {
        s_differ = NONE;
        s_bad = NONE;
    }
    __syncthreads();
    const xggm_train_log& lg = a.log;
    int differ = NONE, bad = NONE;
    for (int i = tid; i < a.n; i += FOLD_THREADS) {
        const int32_t k0 = a.kinds[i];
        const int64_t st0 = a.steps ? a.steps[i] : 0;
        int mask = (k0 >> 8) & 0xFF;
        bool d = false;
        for (int r = 1; r < a.world; ++r) {
            const int32_t k = a.kinds[r * a.kind_stride + i];
            d |= k != k0;  // the kind or the present columns
            mask &= k >> 8;
            if (a.steps) d |= a.steps[r * a.step_stride + i] != st0;
        }
        bool nonfinite = false;
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            float acc = a.vals[(int64_t)i * COLS + c];
            for (int r = 1; r < a.world; ++r) acc += a.vals[r * a.val_stride + (int64_t)i * COLS + c];
            // one rank: the record as it is.  An absent column holds 0, as an append leaves it
            const float v = a.world == 1 ? acc : (((mask >> c) & 1) ? acc * a.inv : 0.f);
            lg.values[(int64_t)i * COLS + c] = v;
            nonfinite |= ((mask >> c) & 1) && (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;
        }
        lg.kinds[i] = (k0 & 0xFF) | (mask << 8);
        if (d && differ == NONE) differ = i;  // i only grows: the first of this thread
        if (nonfinite && bad == NONE) bad = i;
    }
    if (differ != NONE) atomicMin(&s_differ, differ);
    if (bad != NONE) atomicMin(&s_bad, bad);
    __syncthreads();  // the folded rows are visible to the whole workgroup
    if (tid < KINDS * COLS) {
        const int kind = tid / COLS, c = tid % COLS;
        double s = 0.0;
        int64_t cnt = 0;
        for (int i = 0; i < a.n; ++i) {
            const int32_t k = lg.kinds[i];
            if ((k & 0xFF) != kind) continue;
            ++cnt;
            if ((k >> (8 + c)) & 1) s = s + (double)lg.values[(int64_t)i * COLS + c];
        }
        lg.sums[tid] = s;
        if (c == 0) lg.counts[kind] = cnt;
    }
    if (tid != 0) return;
    bool cursor_off = false;
    if (a.cursors)
        for (int r = 0; r < a.world; ++r) cursor_off |= a.cursors[r * a.cursor_stride] != (int64_t)a.n;
    *a.flag = s_differ != NONE ? (int64_t)s_differ : (cursor_off ? (int64_t)a.n : -1);
    *lg.first_bad = s_bad != NONE ? *lg.cursor - a.n + s_bad : -1;
}

inline bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }
}  // namespace

extern "C" int xggm_train_log_fold(const float* vals, const int32_t* kinds, const int64_t* steps, const int64_t* cursors,
                                   int64_t val_stride, int64_t kind_stride, int64_t step_stride, int64_t cursor_stride,
                                   int world, int64_t n, xggm_train_log* log, int64_t* flag, hipStream_t st) {
    XGGM_REQUIRE(world >= 1 && world <= 65536, "xggm_train_log_fold: world = %d (1 <= world <= 65536)", world);
    XGGM_REQUIRE(log, "xggm_train_log_fold: null log");
    XGGM_REQUIRE(log->values && log->kinds && log->cursor && log->sums && log->counts && log->first_bad,
                 "xggm_train_log_fold: the log (ring) needs values, kinds, cursor, sums, counts and first_bad");
    XGGM_REQUIRE(vals && kinds && flag, "xggm_train_log_fold: null gathered values / kinds / flag");
    XGGM_REQUIRE(log->capacity > 0 && log->capacity < NONE, "xggm_train_log_fold: capacity = %lld (0 < capacity < 2^31 - 1)",
                 (long long)log->capacity);
    XGGM_REQUIRE(n >= 1 && n <= log->capacity, "xggm_train_log_fold: n = %lld records (1 <= n <= capacity %lld)", (long long)n,
                 (long long)log->capacity);
    XGGM_REQUIRE(world == 1 || (val_stride >= n * COLS && kind_stride >= n && (!steps || step_stride >= n) &&
                                (!cursors || cursor_stride >= 1)),
                 "xggm_train_log_fold: rank strides (%lld, %lld, %lld, %lld) shorter than one rank's %lld records",
                 (long long)val_stride, (long long)kind_stride, (long long)step_stride, (long long)cursor_stride, (long long)n);
    XGGM_REQUIRE(aligned(steps, 8) && aligned(cursors, 8) && aligned(flag, 8) && aligned(log->cursor, 8) && aligned(log->sums, 8) &&
                     aligned(log->counts, 8) && aligned(log->first_bad, 8),
                 "xggm_train_log_fold: steps, cursors, flag, cursor, sums, counts and first_bad must be 8-byte aligned");
    XGGM_REQUIRE(aligned(vals, 4) && aligned(kinds, 4) && aligned(log->values, 4) && aligned(log->kinds, 4),
                 "xggm_train_log_fold: values and kinds (gathered and the log's) must be 4-byte aligned");
    TrainLogFoldArgs a;
    a.vals = vals, a.kinds = kinds, a.steps = steps, a.cursors = cursors;
    a.val_stride = val_stride, a.kind_stride = kind_stride, a.step_stride = step_stride, a.cursor_stride = cursor_stride;
    a.world = world, a.n = (int)n;
    a.inv = 1.f / (float)world;
    a.log = *log;
    a.flag = flag;
    hipLaunchKernelGGL(train_log_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, st, a);
    return xggm_check_launch("xggm_train_log_fold");
}

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
