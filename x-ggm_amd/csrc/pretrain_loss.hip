// Losses of LXMERT pre-training (LXRTPretraining.forward, src/lxrt/modeling.py:1009-1046):
//   xggm_mlm_select      the rows of the language stream whose masked_lm_label counts, compacted in ascending row order
//   xggm_vocab_ce_*      nn.CrossEntropyLoss(ignore_index=-1) over the vocabulary (:1011-1014) on those compacted rows
//   xggm_visual_loss_*   the per-row object losses weighted by a confidence and averaged over ALL rows (:1024-1046)
// The masked-LM logits are [rows, 30522]: about 15 % of the rows carry a label, so the list of those rows is built on the
// device (no host read) and decoder, loss and gradients run over `cap` compacted rows instead of B T.
//
// mlm_select: workgroup c owns rows [256 c, 256 c + 256).  It counts the labelled rows in front of its chunk and in the
// whole input itself (thread-strided int sums: integers, so any order gives the same number; a few KB of labels from L2
// per workgroup at pre-training shapes), ranks its own rows with a ballot prefix inside each wave and the waves in wave
// order, and copies its rows to their slots.  No atomics: the list is a function of the labels alone.  The rows [n, cap)
// of the gathered activations are zero-filled by the workgroups in turn, so a product over all `cap` rows is harmless.
//
// vocab_ce: one 1024-thread workgroup owns a row at a time.  Thread t owns the 16-byte chunks t, t + 1024, ... of the row
// (4 floats or 8 bf16): a row of up to 32768 elements (30522 word pieces) is read ONCE and stays in 32 registers per thread
// through the max and the sum; a longer row is folded online (running max, rescaled sum), also in one read.  Rows start
// 16-byte aligned (ld is padded by the caller); columns [V, ld) read as -inf and get exact zeros in the backward.
//
// visual_loss: one 256-thread workgroup owns a row of every job at a time (min(R, 128) workgroups walking rows).
//
// Every sum has a fixed order: a thread's elements in index order, the fixed cross-lane tree of wave_sum, the waves in wave
// order through LDS, a workgroup's rows in row order, the workgroups in index order by the one that draws the last ticket.
// No floating-point atomics: the same bits whatever the scheduling.
#include <math.h>
#include "common.h"
#include "xggm.h"

namespace {

// ------------------------------------------------------------------------------------------------ 16-byte chunks of a row
template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int N = 4; typedef float4 raw; };
struct __attribute__((aligned(16))) bf16x8 { bf16 v[8]; };
template <> struct Chunk<bf16> { static constexpr int N = 8; typedef bf16x8 raw; };

__device__ __forceinline__ void unpack(const float4& t, float (&o)[4]) { o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w; }
__device__ __forceinline__ void unpack(const bf16x8& t, float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = __bfloat162float(t.v[i]);
}
__device__ __forceinline__ void pack(const float (&o)[4], float4& t) { t = make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ void pack(const float (&o)[8], bf16x8& t) {
#pragma unroll
    for (int i = 0; i < 8; ++i) t.v[i] = __float2bfloat16(o[i]);
}

// sum / max of one value per thread over a workgroup of NW waves, waves in wave order; every thread gets the result
template <int NW>
__device__ __forceinline__ float block_sum(float a) {
    __shared__ float red[NW];
    a = wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += red[w];
    return r;
}
template <int NW>
__device__ __forceinline__ float block_max(float a) {
    __shared__ float red[NW];
    a = wave_max(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = fmaxf(r, red[w]);
    return r;
}
template <int NW>
__device__ __forceinline__ int block_sum_int(int a) {
    __shared__ int red[NW];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    int r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += red[w];
    return r;
}

// ================================================================================================ mlm_select
constexpr int SEL_NT = 256;  // threads of a workgroup = rows of a scan chunk

struct SelArgs {
    const int64_t* labels;
    const void* x;
    int M, H, cap, V;
    int64_t ignore_index;
    int *row_index, *label, *n, *overflow;
    void* out;
};

__device__ __forceinline__ bool sel_counts(const SelArgs& a, int r) {
    const int64_t l = a.labels[r];
    return l != a.ignore_index && l >= 0 && l < (int64_t)a.V;
}

__global__ __launch_bounds__(SEL_NT) void mlm_select_kernel(SelArgs a, int row_bytes) {
    __shared__ int s_wave[SEL_NT / 64];
    __shared__ int s_rows[SEL_NT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = blockIdx.x * SEL_NT;
    // labelled rows in front of this chunk, and in the whole input
    int before = 0, all = 0;
    for (int r = tid; r < a.M; r += SEL_NT) {
        const int f = sel_counts(a, r) ? 1 : 0;
        all += f;
        before += r < c0 ? f : 0;
    }
    before = block_sum_int<SEL_NT / 64>(before);
    all = block_sum_int<SEL_NT / 64>(all);
    // rank of this thread's row among the chunk's labelled rows
    const int r = c0 + tid;
    const bool mine = r < a.M && sel_counts(a, r);
    const unsigned long long bal = __ballot(mine);
    const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int wave_off = 0, chunk_cnt = 0;
#pragma unroll
    for (int w = 0; w < SEL_NT / 64; ++w) {
        wave_off += w < wv ? s_wave[w] : 0;
        chunk_cnt += s_wave[w];
    }
    const int local = wave_off + in_wave;
    if (mine) {
        s_rows[local] = r;
        const int pos = before + local;
        if (pos < a.cap) {
            a.row_index[pos] = r;
            a.label[pos] = (int)a.labels[r];
        }
    }
    __syncthreads();
    const int n = all < a.cap ? all : a.cap;
    if (blockIdx.x == 0 && tid == 0) {
        *a.n = n;
        *a.overflow = all > a.cap ? 1 : 0;
    }
    // the list's tail: no row, no label
    for (int j = n + blockIdx.x * SEL_NT + tid; j < a.cap; j += gridDim.x * SEL_NT) {
        a.row_index[j] = -1;
        a.label[j] = -1;
    }
    // gather this chunk's rows, 16 bytes per thread and step
    typedef int i4 __attribute__((ext_vector_type(4)));
    const int nvec = row_bytes >> 4;
    const i4* src = reinterpret_cast<const i4*>(a.x);
    i4* dst = reinterpret_cast<i4*>(a.out);
    int keep = a.cap - before;  // slots left for this chunk
    keep = keep < 0 ? 0 : (keep < chunk_cnt ? keep : chunk_cnt);
    for (int i = tid; i < keep * nvec; i += SEL_NT) {
        const int j = i / nvec, v = i - j * nvec;
        dst[(int64_t)(before + j) * nvec + v] = src[(int64_t)s_rows[j] * nvec + v];
    }
    // zero rows [n, cap), the workgroups in turn
    const int64_t tail0 = (int64_t)n * nvec, tail1 = (int64_t)a.cap * nvec;
    for (int64_t i = tail0 + (int64_t)blockIdx.x * SEL_NT + tid; i < tail1; i += (int64_t)gridDim.x * SEL_NT)
        dst[i] = (i4){0, 0, 0, 0};
}

template <typename T>
int mlm_select(const xggm_mlm_select_args* p, hipStream_t st, const char* who) {
    XGGM_REQUIRE(p, "%s: null arguments", who);
    XGGM_REQUIRE(p->M > 0 && p->M <= XGGM_MLM_SELECT_MAX_ROWS && p->H > 0 && p->H <= (1 << 16) && p->V > 0, "%s: bad shape M=%d H=%d V=%d", who,
                 p->M, p->H, p->V);
    XGGM_REQUIRE(p->cap > 0 && p->cap <= (1 << 22), "%s: capacity %d must be positive", who, p->cap);
    XGGM_REQUIRE(p->labels && p->x && p->out, "%s: labels, x and out are required", who);
    XGGM_REQUIRE(p->row_index && p->label && p->n && p->overflow, "%s: row_index, label, n and overflow are required", who);
    const int row_bytes = p->H * (int)sizeof(T);
    XGGM_REQUIRE(row_bytes % 16 == 0 && (uintptr_t)p->x % 16 == 0 && (uintptr_t)p->out % 16 == 0,
                 "%s: rows of %d bytes: x and out must be 16-byte aligned with rows a multiple of 16 bytes", who, row_bytes);
    SelArgs a{p->labels, p->x, p->M, p->H, p->cap, p->V, p->ignore_index, p->row_index, p->label, p->n, p->overflow, p->out};
    hipLaunchKernelGGL(mlm_select_kernel, dim3(ceil_div(p->M, SEL_NT)), dim3(SEL_NT), 0, st, a, row_bytes);
    return xggm_check_launch(who);
}

// backward of the gather: d_x [M, H] holds row j of `src` at row row_index[j] (j < n) and exact zeros elsewhere.  The list
// ascends, so workgroup j also owns the rows between the previous entry and its own (the last one: up to M) and no row is
// written twice: one launch, no memset in front.
__global__ __launch_bounds__(SEL_NT) void mlm_scatter_kernel(const void* src_, const int* row_index, const int* n_, void* out_,
                                                              int M, int cap, int row_bytes) {
    typedef int i4 __attribute__((ext_vector_type(4)));
    const int nvec = row_bytes >> 4, tid = threadIdx.x, j = blockIdx.x;
    int n = *n_;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const i4* src = reinterpret_cast<const i4*>(src_);
    i4* out = reinterpret_cast<i4*>(out_);
    if (n == 0) {  // nothing selected: the workgroups share the zero fill
        for (int64_t i = (int64_t)j * SEL_NT + tid; i < (int64_t)M * nvec; i += (int64_t)gridDim.x * SEL_NT) out[i] = (i4){0, 0, 0, 0};
        return;
    }
    if (j >= n) return;
    int z0, z1, own = -1;  // zero rows [z0, z1), then copy row `own`
    {
        own = row_index[j];
        z0 = j == 0 ? 0 : row_index[j - 1] + 1;
        z1 = own;
        if (own < 0 || own >= M || z0 < 0 || z0 > own) return;  // not a list mlm_select wrote: touch nothing
    }
    for (int64_t i = (int64_t)z0 * nvec + tid; i < (int64_t)z1 * nvec; i += SEL_NT) out[i] = (i4){0, 0, 0, 0};
    if (own >= 0) {
        for (int v = tid; v < nvec; v += SEL_NT) out[(int64_t)own * nvec + v] = src[(int64_t)j * nvec + v];
        if (j == n - 1)
            for (int64_t i = (int64_t)(own + 1) * nvec + tid; i < (int64_t)M * nvec; i += SEL_NT) out[i] = (i4){0, 0, 0, 0};
    }
}

template <typename T>
int mlm_scatter(const void* src, const int* row_index, const int* n, void* out, int M, int H, int cap, hipStream_t st,
                const char* who) {
    XGGM_REQUIRE(M > 0 && M <= XGGM_MLM_SELECT_MAX_ROWS && H > 0 && H <= (1 << 16), "%s: bad shape M=%d H=%d", who, M, H);
    XGGM_REQUIRE(cap > 0 && cap <= (1 << 22), "%s: capacity %d must be positive", who, cap);
    XGGM_REQUIRE(src && row_index && n && out, "%s: src, row_index, n and out are required", who);
    const int row_bytes = H * (int)sizeof(T);
    XGGM_REQUIRE(row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0,
                 "%s: rows of %d bytes: src and out must be 16-byte aligned with rows a multiple of 16 bytes", who, row_bytes);
    hipLaunchKernelGGL(mlm_scatter_kernel, dim3(cap), dim3(SEL_NT), 0, st, src, row_index, n, out, M, cap, row_bytes);
    return xggm_check_launch(who);
}

// ================================================================================================ vocab_ce
constexpr int CE_NT = 1024;
constexpr int CE_NW = CE_NT / 64;
constexpr int CE_EPT = 32;                 // elements of a row a thread keeps in registers
constexpr int CE_REG_MAX = CE_NT * CE_EPT;  // longest register-resident row (XGGM_VOCAB_CE_REG_MAX)
constexpr int CE_FWD_GRID = XGGM_VOCAB_CE_FWD_GRID;          // workgroups (tickets) of the forward: ordered_grid_sum takes up to 4096
constexpr int CE_BWD_GRID = XGGM_VOCAB_CE_BWD_GRID;
static_assert(CE_REG_MAX == XGGM_VOCAB_CE_REG_MAX, "xggm.h names the register-resident limit");

struct CeArgs {
    void* logits;
    const int *label, *n, *overflow;
    int cap, V;
    int64_t ld;
    float *loss, *ws, *save;
    const float* gout;
};

// chunk at element i0 of a row (i0 < ld, whole inside ld); columns >= V read as `fill`
template <typename T>
__device__ __forceinline__ void ce_load(const T* row, int i0, int V, float fill, float (&o)[Chunk<T>::N]) {
    const typename Chunk<T>::raw t = *reinterpret_cast<const typename Chunk<T>::raw*>(row + i0);
    unpack(t, o);
    if (i0 + Chunk<T>::N > V) {
#pragma unroll
        for (int j = 0; j < Chunk<T>::N; ++j) o[j] = i0 + j < V ? o[j] : fill;
    }
}

template <typename T, bool REG>
__global__ __launch_bounds__(CE_NT) void vocab_ce_fwd_kernel(CeArgs a) {
    constexpr int CH = Chunk<T>::N, NCH = CE_EPT / CH;
    const int tid = threadIdx.x;
    int n = *a.n;
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    const T* base = reinterpret_cast<const T*>(a.logits);
    float acc = 0.f;  // this workgroup's rows, in row order (uniform over the threads)
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const T* row = base + (int64_t)r * a.ld;
        float mz, sz;
        if (REG) {
            float v[CE_EPT];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int i0 = CH * (k * CE_NT + tid);
                float o[CH];
                if (i0 < a.V) {
                    ce_load<T>(row, i0, a.V, -INFINITY, o);
                } else {
#pragma unroll
                    for (int j = 0; j < CH; ++j) o[j] = -INFINITY;
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) v[CH * k + j] = o[j];
            }
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < CE_EPT; ++i) m = fmaxf(m, v[i]);
            mz = block_max<CE_NW>(m);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < CE_EPT; ++i)
                if (v[i] != -INFINITY) s += expf(v[i] - mz);  // (a NaN logit stays: the loss is NaN, as the reference's)
            sz = block_sum<CE_NW>(s);
        } else {
            float m0 = -INFINITY, s0 = 0.f;
            const int nk = (a.V + CH * CE_NT - 1) / (CH * CE_NT);
            for (int k = 0; k < nk; ++k) {
                const int i0 = CH * (k * CE_NT + tid);
                if (i0 >= a.V) break;
                float o[CH];
                ce_load<T>(row, i0, a.V, -INFINITY, o);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (!(o[j] <= m0)) {  // (a NaN takes this branch and stays)
                        s0 *= expf(m0 - o[j]);
                        m0 = o[j];
                    }
                    if (o[j] != -INFINITY) s0 += expf(o[j] - m0);
                }
            }
            mz = block_max<CE_NW>(m0);
            sz = block_sum<CE_NW>(m0 != -INFINITY ? s0 * expf(m0 - mz) : 0.f);  // a thread without elements adds nothing
        }
        const float lz = logf(sz);
        const int label = a.label[r];
        if (label >= 0 && label < a.V) acc += (lz + mz) - to_f32(row[label]);  // a label outside the vocabulary adds nothing
        if (tid == 0) {
            a.save[2 * (int64_t)r] = mz;
            a.save[2 * (int64_t)r + 1] = lz;
        }
    }
    float total;
    if (ordered_grid_sum(acc, a.ws, gridDim.x, blockIdx.x, total)) {
        const bool over = a.overflow && *a.overflow != 0;
        *a.loss += over ? NAN : total / (float)n;  // n == 0: 0 / 0, the NaN of torch's mean over nothing
    }
}

template <typename T>
__global__ __launch_bounds__(CE_NT) void vocab_ce_bwd_kernel(CeArgs a) {
    constexpr int CH = Chunk<T>::N;
    const int tid = threadIdx.x;
    int n = *a.n;
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    const bool over = a.overflow && *a.overflow != 0;
    const float coef = over ? NAN : *a.gout / (float)n;  // a truncated list never yields a usable gradient
    T* base = reinterpret_cast<T*>(a.logits);
    const int nk = (int)((a.ld + CH * CE_NT - 1) / (CH * CE_NT));
    for (int r = blockIdx.x; r < a.cap; r += gridDim.x) {
        T* row = base + (int64_t)r * a.ld;
        const int label = r < n ? a.label[r] : -1;
        const bool live = r < n && label >= 0 && label < a.V;  // (wave-uniform)
        const float mz = live ? a.save[2 * (int64_t)r] : 0.f, lz = live ? a.save[2 * (int64_t)r + 1] : 0.f;
#pragma unroll 4
        for (int k = 0; k < nk; ++k) {
            const int i0 = CH * (k * CE_NT + tid);
            if (i0 >= a.ld) break;
            float o[CH];
            if (live && i0 < a.V) {
                ce_load<T>(row, i0, a.V, -INFINITY, o);
#pragma unroll
                for (int j = 0; j < CH; ++j)
                    o[j] = i0 + j < a.V ? coef * (expf(o[j] - mz - lz) - (i0 + j == label ? 1.f : 0.f)) : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) o[j] = 0.f;
            }
            typename Chunk<T>::raw t;
            pack(o, t);
            *reinterpret_cast<typename Chunk<T>::raw*>(row + i0) = t;
        }
    }
}

template <typename T>
int ce_check(const xggm_vocab_ce_args* p, const char* who, CeArgs* a) {
    XGGM_REQUIRE(p, "%s: null arguments", who);
    XGGM_REQUIRE(p->cap > 0 && p->cap <= (1 << 22), "%s: capacity %d must be positive", who, p->cap);
    XGGM_REQUIRE(p->V > 0 && p->V <= (1 << 24), "%s: bad vocabulary size V=%d", who, p->V);
    XGGM_REQUIRE(p->ld >= p->V, "%s: row stride ld=%lld is shorter than V=%d", who, (long long)p->ld, p->V);
    XGGM_REQUIRE(p->ld % Chunk<T>::N == 0 && p->ld <= (1 << 25), "%s: row stride ld=%lld must be a multiple of %d elements (16 bytes)",
                 who, (long long)p->ld, Chunk<T>::N);
    XGGM_REQUIRE(p->logits && p->label && p->n, "%s: logits, label and n are required", who);
    XGGM_REQUIRE((uintptr_t)p->logits % 16 == 0, "%s: logits must be 16-byte aligned", who);
    XGGM_REQUIRE(p->save, "%s: the save buffer (2 cap floats) is required", who);
    *a = CeArgs{p->logits, p->label, p->n, p->overflow, p->cap, p->V, p->ld, p->loss, p->ws, p->save, p->gout};
    return XGGM_OK;
}

template <typename T>
int vocab_ce_fwd(const xggm_vocab_ce_args* p, hipStream_t st, const char* who) {
    CeArgs a;
    if (int rc = ce_check<T>(p, who, &a)) return rc;
    XGGM_REQUIRE(p->loss, "%s: the loss slot is required", who);
    XGGM_REQUIRE(p->ws, "%s: the workspace ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0) is required", who);
    const dim3 grid(std::min(a.cap, CE_FWD_GRID));
    if (a.V <= CE_REG_MAX)
        hipLaunchKernelGGL((vocab_ce_fwd_kernel<T, true>), grid, dim3(CE_NT), 0, st, a);
    else
        hipLaunchKernelGGL((vocab_ce_fwd_kernel<T, false>), grid, dim3(CE_NT), 0, st, a);
    return xggm_check_launch(who);
}

template <typename T>
int vocab_ce_bwd(const xggm_vocab_ce_args* p, hipStream_t st, const char* who) {
    CeArgs a;
    if (int rc = ce_check<T>(p, who, &a)) return rc;
    XGGM_REQUIRE(p->gout, "%s: gout (the upstream gradient, a device scalar) is required", who);
    hipLaunchKernelGGL(vocab_ce_bwd_kernel<T>, dim3(std::min(a.cap, CE_BWD_GRID)), dim3(CE_NT), 0, st, a);
    return xggm_check_launch(who);
}

// ================================================================================================ visual_loss
constexpr int VL_NT = 256;
constexpr int VL_NW = VL_NT / 64;
constexpr int VL_GRID = XGGM_VISUAL_LOSS_GRID;
static_assert(VL_GRID <= SUM2_MAX_BLOCKS && CE_FWD_GRID <= 4096, "ticket grids of common.h");
constexpr int VL_JOBS = XGGM_VISUAL_MAX_JOBS;

struct VlJob {
    int kind, W, vec;  // vec: rows of scores (and target) can be read four elements at a time
    const void* scores;
    const int64_t* label_index;
    const float *target, *mask_conf;
    float weight;
    float* loss;
    void* d_score;
};
struct VlArgs {
    VlJob job[VL_JOBS];
    int n_jobs, R;
    int64_t ignore_index;
    float *ws, *save;
    const float* gout;
};

// elements [i0, i0 + 4) of a row of W
template <typename T>
__device__ __forceinline__ void vl_load(const T* p, int W, int i0, bool vec, float fill, float (&o)[4]) {
    if (vec) {
        load4(p + i0, o);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = i0 + j < W ? to_f32(p[i0 + j]) : fill;
    }
}
template <typename T>
__device__ __forceinline__ void vl_store(T* p, int W, int i0, bool vec, const float (&o)[4]) {
    if (vec) {
        store4(p + i0, o);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < W) p[i0 + j] = from_f32<T>(o[j]);
    }
}

__device__ __forceinline__ int vl_label(const VlJob& jb, int r, int64_t ignore_index) {
    const int64_t li = jb.label_index[r];
    return (li == ignore_index || li < 0 || li >= jb.W) ? -1 : (int)li;
}

// three sums over the grid in one go: partials in ws[HEAD + 3 blk + j], added in index order by the workgroup that draws
// the last ticket (ordered_grid_sum2 of common.h with one more value).  nblk <= VL_GRID, VL_NT >= nblk threads.
__device__ __forceinline__ bool ordered_grid_sum3(const float (&v)[VL_JOBS], float* ws, int nblk, int blk, float (&tot)[VL_JOBS]) {
    __shared__ int s_last;
    __shared__ float s_part[VL_JOBS * VL_GRID];
    unsigned* counter = reinterpret_cast<unsigned*>(ws);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < VL_JOBS; ++j)
            __hip_atomic_store(ws + SUM_WS_HEAD + VL_JOBS * blk + j, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores acknowledged before the ticket (common.h)
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = (t == (unsigned)nblk - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return false;
    for (int i = threadIdx.x; i < VL_JOBS * nblk; i += blockDim.x)
        s_part[i] = __hip_atomic_load(ws + SUM_WS_HEAD + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int j = 0; j < VL_JOBS; ++j) tot[j] = 0.f;
    for (int i = 0; i < nblk; ++i)  // index order, one thread
#pragma unroll
        for (int j = 0; j < VL_JOBS; ++j) tot[j] += s_part[VL_JOBS * i + j];
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    return true;
}

template <typename T>
__global__ __launch_bounds__(VL_NT) void visual_loss_fwd_kernel(VlArgs a) {
    const int tid = threadIdx.x;
    float acc[VL_JOBS] = {0.f, 0.f, 0.f};  // this workgroup's rows per job, in row order (uniform over the threads)
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
#pragma unroll
        for (int q = 0; q < VL_JOBS; ++q) {
            if (q >= a.n_jobs) break;
            const VlJob& jb = a.job[q];
            const T* s = reinterpret_cast<const T*>(jb.scores) + (int64_t)r * jb.W;
            const bool vec = jb.vec != 0;
            const float conf = jb.mask_conf[r];
            if (jb.kind == XGGM_VISUAL_CE) {
                float m0 = -INFINITY, s0 = 0.f;
                for (int i0 = 4 * tid; i0 < jb.W; i0 += 4 * VL_NT) {
                    float o[4];
                    vl_load<T>(s, jb.W, i0, vec, -INFINITY, o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!(o[j] <= m0)) {  // (a NaN takes this branch and stays)
                            s0 *= expf(m0 - o[j]);
                            m0 = o[j];
                        }
                        if (o[j] != -INFINITY) s0 += expf(o[j] - m0);
                    }
                }
                const float mz = block_max<VL_NW>(m0);
                const float sz = block_sum<VL_NW>(m0 != -INFINITY ? s0 * expf(m0 - mz) : 0.f);
                const float lz = logf(sz);
                const int label = vl_label(jb, r, a.ignore_index);
                if (label >= 0) acc[q] += ((lz + mz) - to_f32(s[label])) * conf;
                if (tid == 0) {
                    a.save[2 * ((int64_t)q * a.R + r)] = mz;
                    a.save[2 * ((int64_t)q * a.R + r) + 1] = lz;
                }
            } else {
                const float* y = jb.target + (int64_t)r * jb.W;
                float v = 0.f;
                for (int i0 = 4 * tid; i0 < jb.W; i0 += 4 * VL_NT) {
                    float o[4], t[4];
                    vl_load<T>(s, jb.W, i0, vec, 0.f, o);
                    vl_load<float>(y, jb.W, i0, vec, 0.f, t);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = fabsf(o[j] - t[j]);
                        v += d < 1.f ? 0.5f * d * d : d - 0.5f;  // SmoothL1, beta = 1
                    }
                }
                v = block_sum<VL_NW>(v);
                acc[q] += v / (float)jb.W * conf;
            }
        }
    }
    float tot[VL_JOBS];
    if (ordered_grid_sum3(acc, a.ws, gridDim.x, blockIdx.x, tot)) {
#pragma unroll
        for (int q = 0; q < VL_JOBS; ++q)
            if (q < a.n_jobs) *a.job[q].loss += tot[q] / (float)a.R * a.job[q].weight;
    }
}

template <typename T>
__global__ __launch_bounds__(VL_NT) void visual_loss_bwd_kernel(VlArgs a) {
    const int tid = threadIdx.x;
    const float g = *a.gout;
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
#pragma unroll
        for (int q = 0; q < VL_JOBS; ++q) {
            if (q >= a.n_jobs) break;
            const VlJob& jb = a.job[q];
            const T* s = reinterpret_cast<const T*>(jb.scores) + (int64_t)r * jb.W;
            T* d = reinterpret_cast<T*>(jb.d_score) + (int64_t)r * jb.W;
            const bool vec = jb.vec != 0;
            const float conf = jb.mask_conf[r];
            if (jb.kind == XGGM_VISUAL_CE) {
                const int label = vl_label(jb, r, a.ignore_index);
                const bool live = label >= 0 && conf != 0.f;  // else exact zeros
                const float coef = g * jb.weight * conf / (float)a.R;
                const float mz = a.save[2 * ((int64_t)q * a.R + r)], lz = a.save[2 * ((int64_t)q * a.R + r) + 1];
                for (int i0 = 4 * tid; i0 < jb.W; i0 += 4 * VL_NT) {
                    float o[4] = {0.f, 0.f, 0.f, 0.f};
                    if (live) {
                        vl_load<T>(s, jb.W, i0, vec, -INFINITY, o);
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = coef * (expf(o[j] - mz - lz) - (i0 + j == label ? 1.f : 0.f));
                    }
                    vl_store<T>(d, jb.W, i0, vec, o);
                }
            } else {
                const float* y = jb.target + (int64_t)r * jb.W;
                const float coef = g * jb.weight * conf / ((float)a.R * (float)jb.W);
                for (int i0 = 4 * tid; i0 < jb.W; i0 += 4 * VL_NT) {
                    float o[4] = {0.f, 0.f, 0.f, 0.f}, t[4];
                    if (conf != 0.f) {
                        vl_load<T>(s, jb.W, i0, vec, 0.f, o);
                        vl_load<float>(y, jb.W, i0, vec, 0.f, t);
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = coef * fminf(fmaxf(o[j] - t[j], -1.f), 1.f);
                    }
                    vl_store<T>(d, jb.W, i0, vec, o);
                }
            }
        }
    }
}

template <typename T>
int vl_check(const xggm_visual_loss_args* p, const char* who, bool bwd, VlArgs* a) {
    XGGM_REQUIRE(p, "%s: null arguments", who);
    XGGM_REQUIRE(p->n_jobs >= 1 && p->n_jobs <= VL_JOBS, "%s: %d jobs (1 to %d per launch)", who, p->n_jobs, VL_JOBS);
    XGGM_REQUIRE(p->R > 0 && p->R <= (1 << 22), "%s: bad row count R=%d", who, p->R);
    XGGM_REQUIRE(p->save, "%s: the save buffer (2 * %d * R floats) is required", who, VL_JOBS);
    for (int q = 0; q < p->n_jobs; ++q) {
        const xggm_visual_job& j = p->job[q];
        XGGM_REQUIRE(j.kind == XGGM_VISUAL_CE || j.kind == XGGM_VISUAL_L2, "%s: job %d: unknown kind %d", who, q, j.kind);
        XGGM_REQUIRE(j.W > 0 && j.W <= (1 << 20), "%s: job %d: bad width W=%d", who, q, j.W);
        XGGM_REQUIRE(j.scores && j.mask_conf, "%s: job %d: scores and mask_conf are required", who, q);
        if (j.kind == XGGM_VISUAL_CE)
            XGGM_REQUIRE(j.label_index, "%s: job %d: cross-entropy needs label_index", who, q);
        else
            XGGM_REQUIRE(j.target, "%s: job %d: the regression needs target", who, q);
        if (bwd)
            XGGM_REQUIRE(j.d_score, "%s: job %d: d_score is required", who, q);
        else
            XGGM_REQUIRE(j.loss, "%s: job %d: the loss slot is required", who, q);
        VlJob& o = a->job[q];
        // four elements at a time where every row of scores, d_score and target starts on such a boundary
        const uintptr_t al = 4 * sizeof(T);
        o.vec = j.W % 4 == 0 && (uintptr_t)j.scores % al == 0 && (uintptr_t)j.d_score % al == 0 && (uintptr_t)j.target % 16 == 0;
        o.kind = j.kind; o.W = j.W; o.scores = j.scores; o.label_index = j.label_index; o.target = j.target;
        o.mask_conf = j.mask_conf; o.weight = j.weight; o.loss = j.loss; o.d_score = j.d_score;
    }
    for (int q = p->n_jobs; q < VL_JOBS; ++q) a->job[q] = VlJob{};
    a->n_jobs = p->n_jobs; a->R = p->R; a->ignore_index = p->ignore_index; a->ws = p->ws; a->save = p->save; a->gout = p->gout;
    return XGGM_OK;
}

template <typename T>
int visual_loss_fwd(const xggm_visual_loss_args* p, hipStream_t st, const char* who) {
    VlArgs a;
    if (int rc = vl_check<T>(p, who, false, &a)) return rc;
    XGGM_REQUIRE(p->ws, "%s: the workspace ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0) is required", who);
    hipLaunchKernelGGL(visual_loss_fwd_kernel<T>, dim3(std::min(a.R, VL_GRID)), dim3(VL_NT), 0, st, a);
    return xggm_check_launch(who);
}

template <typename T>
int visual_loss_bwd(const xggm_visual_loss_args* p, hipStream_t st, const char* who) {
    VlArgs a;
    if (int rc = vl_check<T>(p, who, true, &a)) return rc;
    XGGM_REQUIRE(p->gout, "%s: gout (the upstream gradient, a device scalar) is required", who);
    hipLaunchKernelGGL(visual_loss_bwd_kernel<T>, dim3(std::min(a.R, VL_GRID)), dim3(VL_NT), 0, st, a);
    return xggm_check_launch(who);
}

}  // namespace

extern "C" int xggm_mlm_select_f32(const xggm_mlm_select_args* args, hipStream_t st) {
    return mlm_select<float>(args, st, "xggm_mlm_select_f32");
}
extern "C" int xggm_mlm_select_bf16(const xggm_mlm_select_args* args, hipStream_t st) {
    return mlm_select<bf16>(args, st, "xggm_mlm_select_bf16");
}
extern "C" int xggm_mlm_scatter_f32(const void* src, const int* row_index, const int* n, void* out, int M, int H, int cap,
                                    hipStream_t st) {
    return mlm_scatter<float>(src, row_index, n, out, M, H, cap, st, "xggm_mlm_scatter_f32");
}
extern "C" int xggm_mlm_scatter_bf16(const void* src, const int* row_index, const int* n, void* out, int M, int H, int cap,
                                     hipStream_t st) {
    return mlm_scatter<bf16>(src, row_index, n, out, M, H, cap, st, "xggm_mlm_scatter_bf16");
}
extern "C" int xggm_vocab_ce_fwd_f32(const xggm_vocab_ce_args* args, hipStream_t st) {
    return vocab_ce_fwd<float>(args, st, "xggm_vocab_ce_fwd_f32");
}
extern "C" int xggm_vocab_ce_fwd_bf16(const xggm_vocab_ce_args* args, hipStream_t st) {
    return vocab_ce_fwd<bf16>(args, st, "xggm_vocab_ce_fwd_bf16");
}
extern "C" int xggm_vocab_ce_bwd_f32(const xggm_vocab_ce_args* args, hipStream_t st) {
    return vocab_ce_bwd<float>(args, st, "xggm_vocab_ce_bwd_f32");
}
extern "C" int xggm_vocab_ce_bwd_bf16(const xggm_vocab_ce_args* args, hipStream_t st) {
    return vocab_ce_bwd<bf16>(args, st, "xggm_vocab_ce_bwd_bf16");
}
extern "C" int xggm_visual_loss_fwd_f32(const xggm_visual_loss_args* args, hipStream_t st) {
    return visual_loss_fwd<float>(args, st, "xggm_visual_loss_fwd_f32");
}
extern "C" int xggm_visual_loss_fwd_bf16(const xggm_visual_loss_args* args, hipStream_t st) {
    return visual_loss_fwd<bf16>(args, st, "xggm_visual_loss_fwd_bf16");
}
extern "C" int xggm_visual_loss_bwd_f32(const xggm_visual_loss_args* args, hipStream_t st) {
    return visual_loss_bwd<float>(args, st, "xggm_visual_loss_bwd_f32");
}
extern "C" int xggm_visual_loss_bwd_bf16(const xggm_visual_loss_args* args, hipStream_t st) {
    return visual_loss_bwd<bf16>(args, st, "xggm_visual_loss_bwd_bf16");
}
