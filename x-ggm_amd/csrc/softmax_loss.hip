// Answer losses with a softmax over the answer axis:
//   XGGM_SOFTMAX_FOCAL   Focal of src/module/vqa_debias_loss_functions.py:74-81
//   XGGM_SOFTMAX_CE      nn.CrossEntropyLoss(ignore_index) of src/gqa/gqa_ood.py:116 (--mceLoss), mean over the valid rows
// With p = softmax(z) over a row, c = (1 - softmax(b))^2 of the sample's bias row and f = log(p + 1e-5) c:
//   FOCAL  loss = (1 / B) sum_{r,a} [max(f, 0) - f y + log1p(exp(-|f|))]      (= BCEWithLogits(f, y), mean, times A)
//          w = g (sigmoid(f) - y) / B,  u = w c p / (p + 1e-5),  d z_j = u_j - p_j sum_a u_a
//   CE     loss = scale sum_valid (logsumexp(z_r) - z_r[label_r]) / n_valid,  d z = g scale / n_valid (p - onehot), 0 on ignored rows
// One 256-thread workgroup owns a row at a time (min(B, ROW_GRID) workgroups walking rows blk, blk + grid, ...).  Thread t
// owns the 4-element chunks t, t + 256, ... of the row: a row of up to 256 * 16 elements (1842, 2274, 3129 answers) is read
// ONCE and stays in registers through the max, the sum and the element pass; a longer row is re-read chunk by chunk.
// Chunks are loaded as one 16-byte access declared 4-byte aligned (rows of odd length start on 4-byte boundaries only;
// global memory takes such accesses), the last partial chunk element by element.
// Every sum has a fixed order: a thread's elements in index order, the fixed cross-lane tree of wave_sum, the four waves in
// wave order through LDS, a workgroup's rows in row order, the workgroups in index order by the one that draws the last
// ticket (ordered_grid_sum2).  No floating-point atomics: the same bits whatever the scheduling.
// The forward leaves per row {max z, log sum exp(z - max), max b, sum exp(b - max b)} and the label in `save`, so the
// backward is ONE launch that recomputes p from them.
#include <math.h>
#include "common.h"
#include "xggm.h"

namespace {

constexpr int NT = 256;
constexpr int EPT = 16;                // elements of a row a thread keeps in registers
constexpr int REG_MAX = NT * EPT;      // longest register-resident row
constexpr int ROW_GRID = SUM2_MAX_BLOCKS;  // workgroups (tickets) per launch: the cap of DESIGN section 2(e)
constexpr float FOCAL_EPS = 1e-5f;

struct __attribute__((packed, aligned(4))) f4u { float v[4]; };  // 16 bytes at a 4-byte boundary

struct Args {  // xggm_softmax_loss_args by value, pointers typed
    const float *logits, *labels, *bias;
    const int64_t *label_index, *bias_index;
    int64_t bias_row_stride, bias_rows, ignore_index;
    float scale;
    int kind, B, A;
    float *loss, *ws, *save;
    const float* gout;
    float* d_logit;
    int accumulate;
};

// the two values of every thread, summed / maximised over the workgroup (all threads get both results)
__device__ __forceinline__ void block_sum2(float& a, float& b) {
    __shared__ float red[2][NT / 64];
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}
__device__ __forceinline__ void block_max2(float& a, float& b) {
    __shared__ float red[2][NT / 64];
    a = wave_max(a);
    b = wave_max(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    b = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
}

__device__ __forceinline__ float sigmoid_stable(float x) {
    const float t = expf(-fabsf(x)), r = 1.f / (1.f + t);
    return x >= 0.f ? r : t * r;
}

// elements [i0, i0 + 4) of a row of A: one 16-byte access when the chunk is whole, else element by element; `fill` past A
__device__ __forceinline__ void load_chunk(const float* p, int A, int i0, float fill, float (&o)[4]) {
    if (i0 + 4 <= A) {
        const f4u t = *reinterpret_cast<const f4u*>(p + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = t.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = i0 + j < A ? p[i0 + j] : fill;
    }
}
__device__ __forceinline__ void store_chunk(float* p, int A, int i0, const float (&o)[4], int accumulate) {
    if (i0 + 4 <= A) {
        f4u t;
        if (accumulate) {
            t = *reinterpret_cast<const f4u*>(p + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) t.v[j] = __fadd_rn(t.v[j], o[j]);  // (never contracted into the product in front)
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) t.v[j] = o[j];
        }
        *reinterpret_cast<f4u*>(p + i0) = t;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < A) p[i0 + j] = accumulate ? __fadd_rn(p[i0 + j], o[j]) : o[j];
    }
}

// A row as its owner threads see it: REG keeps the thread's EPT elements in registers (one read of the row), else every
// pass re-reads its chunks.  Chunk k of thread t covers elements 4 (k NT + t) ... + 3.
template <bool REG>
struct Row {
    const float* p;
    int A;
    float fill;
    float r[REG ? EPT : 4];
    __device__ __forceinline__ void open(const float* p_, int A_, float fill_) {
        p = p_;
        A = A_;
        fill = fill_;
        if (REG) {
#pragma unroll
            for (int k = 0; k < EPT / 4; ++k) {
                float o[4];
                load_chunk(p, A, 4 * (k * NT + (int)threadIdx.x), fill, o);
#pragma unroll
                for (int j = 0; j < 4; ++j) r[4 * k + j] = o[j];
            }
        }
    }
    __device__ __forceinline__ void chunk(int k, float (&o)[4]) const {
        if (REG) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = r[4 * k + j];
        } else {
            load_chunk(p, A, 4 * (k * NT + (int)threadIdx.x), fill, o);
        }
    }
};
// full unrolling keeps a register-resident row in registers; the chunk loop of a re-read row stays a loop
template <bool REG>
constexpr int UNROLL = REG ? EPT / 4 : 1;
template <bool REG>
__device__ __forceinline__ int chunks_of(int A) {
    return REG ? EPT / 4 : (A + 4 * NT - 1) / (4 * NT);
}

// max and sum exp(. - max) of two rows at once (the second may be absent): one barrier pair for the maxima, one for the sums.
// A thread folds its elements online (running max, rescaled sum) in index order, so a re-read row is read once here too.
template <bool REG>
__device__ __forceinline__ void row_stats(const Row<REG>& z, const Row<REG>* b, int nk, float& mz, float& sz, float& mb,
                                          float& sb) {
    float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f;
#pragma unroll UNROLL<REG>
    for (int k = 0; k < nk; ++k) {
        float v[4];
        z.chunk(k, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(v[j] <= m0)) {  // (a NaN takes this branch and stays: the loss is NaN, as the reference's)
                s0 *= expf(m0 - v[j]);
                m0 = v[j];
            }
            if (v[j] != -INFINITY) s0 += expf(v[j] - m0);
        }
        if (b) {
            b->chunk(k, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(v[j] <= m1)) {  // (a NaN takes this branch and stays: the loss is NaN, as the reference's)
                    s1 *= expf(m1 - v[j]);
                    m1 = v[j];
                }
                if (v[j] != -INFINITY) s1 += expf(v[j] - m1);
            }
        }
    }
    mz = m0;
    mb = m1;
    block_max2(mz, mb);
    sz = m0 != -INFINITY ? s0 * expf(m0 - mz) : 0.f;  // a thread without elements adds nothing
    sb = m1 != -INFINITY ? s1 * expf(m1 - mb) : 0.f;
    block_sum2(sz, sb);
}

__device__ __forceinline__ const float* bias_row(const Args& a, int r) {
    int64_t i = a.bias_index ? a.bias_index[r] : (int64_t)r;
    i = i < 0 ? 0 : (i >= a.bias_rows ? a.bias_rows - 1 : i);  // an index outside the table never leaves it
    return a.bias + i * a.bias_row_stride;
}

// f = log(p + eps) c of one element, with p and c
__device__ __forceinline__ float focal_logit(float z, float b, float mz, float lz, float mb, float inv_sb, float& p, float& c) {
    p = expf(z - mz - lz);
    const float q = 1.f - expf(b - mb) * inv_sb;
    c = q * q;
    return logf(p + FOCAL_EPS) * c;
}

// label of row r for CE: label_index[r], else the first arg-max of the soft scores; -1: the row is ignored
template <bool REG>
__device__ __forceinline__ int ce_label(const Args& a, int r, int nk) {
    if (a.label_index) {
        const int64_t li = a.label_index[r];
        return (li == a.ignore_index || li < 0 || li >= a.A) ? -1 : (int)li;
    }
    Row<REG> y;
    y.open(a.labels + (int64_t)r * a.A, a.A, -INFINITY);
    float mx = -INFINITY, unused = 0.f;
#pragma unroll UNROLL<REG>
    for (int k = 0; k < nk; ++k) {
        float v[4];
        y.chunk(k, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, v[j]);
    }
    block_max2(mx, unused);
    // the first index that holds the maximum: indices below 2^24 are exact as floats, the smallest one is -max(-i)
    float first = -INFINITY;
    unused = 0.f;
#pragma unroll UNROLL<REG>
    for (int k = 0; k < nk; ++k) {
        float v[4];
        y.chunk(k, v);
        const int i0 = 4 * (k * NT + (int)threadIdx.x);
#pragma unroll
        for (int j = 3; j >= 0; --j)
            if (i0 + j < a.A && v[j] == mx) first = fmaxf(first, -(float)(i0 + j));
    }
    block_max2(first, unused);
    if (!(mx > 0.f) || first == -INFINITY) return -1;  // no positive score: an answer outside the vocabulary
    const int64_t li = (int64_t)(-first);
    return li == a.ignore_index ? -1 : (int)li;
}

template <bool REG>
__global__ __launch_bounds__(NT) void softmax_loss_fwd_kernel(Args a) {
    const int tid = threadIdx.x, nk = chunks_of<REG>(a.A);
    const bool focal = a.kind == XGGM_SOFTMAX_FOCAL;
    int* save_label = reinterpret_cast<int*>(a.save + 4 * (int64_t)a.B);
    float acc0 = 0.f, acc1 = 0.f;  // this workgroup's rows, in row order (uniform over the threads)
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        Row<REG> z;
        z.open(a.logits + (int64_t)r * a.A, a.A, -INFINITY);
        float mz, sz, mb = 0.f, sb = 1.f;
        if (focal) {
            Row<REG> b, y;
            b.open(bias_row(a, r), a.A, -INFINITY);
            row_stats<REG>(z, &b, nk, mz, sz, mb, sb);
            const float lz = logf(sz), inv_sb = 1.f / sb;
            y.open(a.labels + (int64_t)r * a.A, a.A, 0.f);
            float v0 = 0.f, v1 = 0.f;
#pragma unroll UNROLL<REG>
            for (int k = 0; k < nk; ++k) {
                float zv[4], bv[4], yv[4];
                z.chunk(k, zv);
                b.chunk(k, bv);
                y.chunk(k, yv);
                const int i0 = 4 * (k * NT + tid);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i0 + j >= a.A) continue;
                    float p, c;
                    const float f = focal_logit(zv[j], bv[j], mz, lz, mb, inv_sb, p, c);
                    v0 += fmaxf(f, 0.f) - f * yv[j] + log1pf(expf(-fabsf(f)));
                }
            }
            block_sum2(v0, v1);
            acc0 += v0;
            if (tid == 0) {
                a.save[4 * (int64_t)r] = mz;
                a.save[4 * (int64_t)r + 1] = lz;
                a.save[4 * (int64_t)r + 2] = mb;
                a.save[4 * (int64_t)r + 3] = sb;
                save_label[r] = -1;
            }
        } else {
            const int label = ce_label<REG>(a, r, nk);
            row_stats<REG>(z, nullptr, nk, mz, sz, mb, sb);
            const float lz = logf(sz);
            if (label >= 0) {
                acc0 += (lz + mz) - a.logits[(int64_t)r * a.A + label];
                acc1 += 1.f;
            }
            if (tid == 0) {
                a.save[4 * (int64_t)r] = mz;
                a.save[4 * (int64_t)r + 1] = lz;
                a.save[4 * (int64_t)r + 2] = 0.f;
                a.save[4 * (int64_t)r + 3] = 1.f;
                save_label[r] = label;
            }
        }
    }
    float t0, t1;
    if (ordered_grid_sum2(acc0, acc1, a.ws, gridDim.x, blockIdx.x, t0, t1)) {
        if (focal) {
            *a.loss += t0 / (float)a.B;
            a.save[5 * (int64_t)a.B] = (float)a.B;
        } else {
            *a.loss += a.scale * t0 / t1;  // no valid row: 0 / 0, the NaN of torch's mean over nothing
            a.save[5 * (int64_t)a.B] = t1;
        }
    }
}

template <bool REG>
__global__ __launch_bounds__(NT) void softmax_loss_bwd_kernel(Args a) {
    const int tid = threadIdx.x, nk = chunks_of<REG>(a.A);
    const bool focal = a.kind == XGGM_SOFTMAX_FOCAL;
    const int* save_label = reinterpret_cast<const int*>(a.save + 4 * (int64_t)a.B);
    const float g = a.gout ? *a.gout : 1.f;
    const float n_valid = a.save[5 * (int64_t)a.B];
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        const float mz = a.save[4 * (int64_t)r], lz = a.save[4 * (int64_t)r + 1];
        float* d = a.d_logit + (int64_t)r * a.A;
        if (!focal) {
            const int label = save_label[r];
            if (label < 0 && a.accumulate) continue;  // an ignored row adds exactly nothing
            const float coef = label < 0 ? 0.f : g * a.scale / n_valid;
            Row<REG> z;
            if (label >= 0) z.open(a.logits + (int64_t)r * a.A, a.A, -INFINITY);
#pragma unroll UNROLL<REG>
            for (int k = 0; k < nk; ++k) {
                const int i0 = 4 * (k * NT + tid);
                if (i0 >= a.A) continue;
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (label >= 0) {
                    float zv[4];
                    z.chunk(k, zv);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = coef * (expf(zv[j] - mz - lz) - (i0 + j == label ? 1.f : 0.f));
                }
                store_chunk(d, a.A, i0, o, a.accumulate);
            }
            continue;
        }
        const float mb = a.save[4 * (int64_t)r + 2], inv_sb = 1.f / a.save[4 * (int64_t)r + 3];
        const float cw = g / (float)a.B;
        Row<REG> z, b, y;
        z.open(a.logits + (int64_t)r * a.A, a.A, -INFINITY);
        b.open(bias_row(a, r), a.A, -INFINITY);
        y.open(a.labels + (int64_t)r * a.A, a.A, 0.f);
        // u of the thread's elements: kept in registers beside the row, recomputed in the second pass of a re-read row
        float u[REG ? EPT : 4];
        float su = 0.f, unused = 0.f;
#pragma unroll UNROLL<REG>
        for (int k = 0; k < nk; ++k) {
            float zv[4], bv[4], yv[4];
            z.chunk(k, zv);
            b.chunk(k, bv);
            y.chunk(k, yv);
            const int i0 = 4 * (k * NT + tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float uj = 0.f;
                if (i0 + j < a.A) {
                    float p, c;
                    const float f = focal_logit(zv[j], bv[j], mz, lz, mb, inv_sb, p, c);
                    uj = cw * (sigmoid_stable(f) - yv[j]) * c * p / (p + FOCAL_EPS);
                }
                if (REG) u[4 * k + j] = uj;
                su += uj;
            }
        }
        block_sum2(su, unused);
#pragma unroll UNROLL<REG>
        for (int k = 0; k < nk; ++k) {
            const int i0 = 4 * (k * NT + tid);
            if (i0 >= a.A) continue;
            float zv[4], o[4];
            z.chunk(k, zv);
            if (REG) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = u[4 * k + j] - expf(zv[j] - mz - lz) * su;
            } else {
                float bv[4], yv[4];
                b.chunk(k, bv);
                y.chunk(k, yv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float p, c;
                    const float f = focal_logit(zv[j], bv[j], mz, lz, mb, inv_sb, p, c);
                    o[j] = cw * (sigmoid_stable(f) - yv[j]) * c * p / (p + FOCAL_EPS) - p * su;
                }
            }
            store_chunk(d, a.A, i0, o, a.accumulate);
        }
    }
}

int check_common(const xggm_softmax_loss_args* p, const char* who, Args* a) {
    XGGM_REQUIRE(p, "%s: null arguments", who);
    XGGM_REQUIRE(p->kind == XGGM_SOFTMAX_FOCAL || p->kind == XGGM_SOFTMAX_CE, "%s: unknown kind %d", who, p->kind);
    XGGM_REQUIRE(p->B > 0 && p->A > 0 && p->B <= (1 << 20) && p->A <= (1 << 24), "%s: bad shape B=%d A=%d", who, p->B, p->A);
    XGGM_REQUIRE(p->logits, "%s: logits is required", who);
    if (p->kind == XGGM_SOFTMAX_CE) {
        XGGM_REQUIRE(p->labels || p->label_index, "%s: cross-entropy needs labels or label_index", who);
    } else {
        XGGM_REQUIRE(p->labels, "%s: Focal needs labels", who);
        XGGM_REQUIRE(p->bias, "%s: Focal needs bias", who);
        XGGM_REQUIRE(p->bias_row_stride >= p->A && p->bias_rows >= 1, "%s: bias table of %lld rows with row stride %lld (A=%d)",
                     who, (long long)p->bias_rows, (long long)p->bias_row_stride, p->A);
        XGGM_REQUIRE(p->bias_index || p->bias_rows >= p->B, "%s: a bias of %lld rows for %d samples needs bias_index", who,
                     (long long)p->bias_rows, p->B);
    }
    XGGM_REQUIRE(p->save, "%s: the save buffer (5 B + 1 floats) is required", who);
    const bool focal = p->kind == XGGM_SOFTMAX_FOCAL;
    a->logits = p->logits; a->labels = p->labels; a->bias = focal ? p->bias : nullptr;
    a->label_index = focal ? nullptr : p->label_index; a->bias_index = focal ? p->bias_index : nullptr;
    a->bias_row_stride = p->bias_row_stride; a->bias_rows = p->bias_rows; a->ignore_index = p->ignore_index;
    a->scale = p->scale; a->kind = p->kind; a->B = p->B; a->A = p->A;
    a->loss = p->loss; a->ws = p->ws; a->save = p->save; a->gout = p->gout; a->d_logit = p->d_logit;
    a->accumulate = p->accumulate;
    return XGGM_OK;
}

int softmax_loss_fwd(const xggm_softmax_loss_args* p, hipStream_t st) {
    Args a;
    if (int rc = check_common(p, "xggm_softmax_loss_fwd", &a)) return rc;
    XGGM_REQUIRE(p->loss, "xggm_softmax_loss_fwd: the loss slot is required");
    XGGM_REQUIRE(p->ws, "xggm_softmax_loss_fwd: the workspace ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0) is required");
    const dim3 grid(std::min(a.B, ROW_GRID));
    if (a.A <= REG_MAX)
        hipLaunchKernelGGL(softmax_loss_fwd_kernel<true>, grid, dim3(NT), 0, st, a);
    else
        hipLaunchKernelGGL(softmax_loss_fwd_kernel<false>, grid, dim3(NT), 0, st, a);
    return xggm_check_launch("xggm_softmax_loss_fwd");
}

int softmax_loss_bwd(const xggm_softmax_loss_args* p, hipStream_t st) {
    Args a;
    if (int rc = check_common(p, "xggm_softmax_loss_bwd", &a)) return rc;
    XGGM_REQUIRE(p->d_logit, "xggm_softmax_loss_bwd: d_logit is required");
    XGGM_REQUIRE(p->gout, "xggm_softmax_loss_bwd: gout (the upstream gradient, a device scalar) is required");
    const dim3 grid(std::min(a.B, ROW_GRID));
    if (a.A <= REG_MAX)
        hipLaunchKernelGGL(softmax_loss_bwd_kernel<true>, grid, dim3(NT), 0, st, a);
    else
        hipLaunchKernelGGL(softmax_loss_bwd_kernel<false>, grid, dim3(NT), 0, st, a);
    return xggm_check_launch("xggm_softmax_loss_bwd");
}

}  // namespace

extern "C" int xggm_softmax_loss_fwd_f32(const xggm_softmax_loss_args* args, hipStream_t st) { return softmax_loss_fwd(args, st); }
extern "C" int xggm_softmax_loss_bwd_f32(const xggm_softmax_loss_args* args, hipStream_t st) { return softmax_loss_bwd(args, st); }
