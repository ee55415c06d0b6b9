// Debias answer losses for language-prior benchmarks (VQA-CP v2, GQA-OOD): src/module/vqa_debias_loss_functions.py:84-207.
//   xggm_debias_fwd_*   ReweightByInvBias / BiasProduct / LearnedMixin, ONE launch (the Hd-long dot of LearnedMixin's
//                       bias_lin included)
//   xggm_debias_bwd_*   d_logit, d_hidden and the gradients of bias_lin.weight, bias_lin.bias and smooth_param: a row
//                       kernel and (only where a parameter gradient is wanted) a one-pass column kernel
// With p = log(b + s), q = log(1 - b + s), e = g (p - q) and d = z + e the three kinds share
//     loss_elem = softplus(-d) y + softplus(d) (1 - y) = max(d, 0) - d y + log1p(exp(-|d|)),   d loss_elem / d d = sigmoid(d) - y
// (BiasProduct: g = 1; ReweightByInvBias: e = 0 and a weight 1 - b), and LearnedMixin's entropy penalty of the
// renormalised pair (g p, g q) is that of the two-way distribution (sigmoid(e), sigmoid(-e)):
//     H(e) = log1p(t) + |e| t / (1 + t),  t = exp(-|e|);   dH/de = -e sigmoid(e) sigmoid(-e) = -e t / (1 + t)^2.
// One workgroup works on a row at a time (at most ROW_GRID workgroups, each walking rows blk, blk + grid, ...): every sum
// over a row is a block sum, every sum over rows is taken in row order by one thread -- no floating-point atomics, the
// same bits whatever the scheduling.  Rows of odd length (A = 3129) start on 4-byte boundaries only: all loads are
// scalar.  The work is ~1e5 elements with ~10 transcendentals each: latency, not bandwidth, so the libm-accurate
// expf / logf / log1pf are affordable and keep the fp32 parity bound.
#include "common.h"
#include "xggm.h"

namespace {

constexpr int NT = 256;
constexpr int ROW_GRID = 32;  // workgroups (tickets) per launch; more rows than that are walked in rounds

__device__ __forceinline__ float block_sum(float v) {
    __shared__ float red[NT / 64];
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// 1 / (1 + exp(-x)) without overflow on either side
__device__ __forceinline__ float sigmoid_stable(float x) {
    const float t = expf(-fabsf(x)), r = 1.f / (1.f + t);
    return x >= 0.f ? r : t * r;
}

struct Args {  // xggm_debias_args by value, pointers typed
    const float *logits, *labels, *bias;
    const int64_t* bias_index;
    int64_t bias_row_stride, bias_rows;
    const void* hidden;
    const float *lin_w, *lin_b, *smooth_param;
    float constant_smooth, w;
    int kind, B, A, Hd;
    float *loss, *save, *ws;
    const float* gout;
    void *d_logit, *d_hidden;
    float *d_lin_w, *d_lin_b, *d_smooth, *part;
    int dlogit_f32, accumulate;
};

__device__ __forceinline__ const float* bias_row(const Args& a, int r) {
    int64_t i = a.bias_index ? a.bias_index[r] : (int64_t)r;
    i = i < 0 ? 0 : (i >= a.bias_rows ? a.bias_rows - 1 : i);  // an index outside the table never leaves it
    return a.bias + i * a.bias_row_stride;
}
__device__ __forceinline__ float smooth_of(const Args& a) {
    return a.constant_smooth + (a.smooth_param ? sigmoid_stable(*a.smooth_param) : 0.f);
}

template <typename T>
__global__ __launch_bounds__(NT) void debias_fwd_kernel(Args a) {
    const int tid = threadIdx.x;
    const bool mixin = a.kind == XGGM_DEBIAS_LEARNED_MIXIN, rew = a.kind == XGGM_DEBIAS_REWEIGHT;
    const float s = smooth_of(a);
    const float c_loss = rew ? 1.f : 1.f / (float)a.B;
    const float c_ent = mixin ? a.w / ((float)a.B * (float)a.A) : 0.f;
    float acc0 = 0.f, acc1 = 0.f;  // this workgroup's rows, in row order (uniform over the threads)
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        float g = 1.f;
        if (mixin) {
            const T* h = static_cast<const T*>(a.hidden) + (int64_t)r * a.Hd;
            float dot = 0.f;
            for (int j = tid; j < a.Hd; j += NT) dot = fmaf(to_f32(h[j]), a.lin_w[j], dot);
            const float pre = block_sum(dot) + a.lin_b[0];
            g = softplus_f(pre);
            if (tid == 0) {
                a.save[r] = pre;
                a.save[a.B + r] = g;
            }
        }
        const float *z = a.logits + (int64_t)r * a.A, *y = a.labels + (int64_t)r * a.A, *b = bias_row(a, r);
        float v0 = 0.f, v1 = 0.f;
        for (int i = tid; i < a.A; i += NT) {
            const float bi = b[i], yi = y[i];
            if (rew) {
                const float d = z[i], wt = 1.f - bi;
                v0 += wt * (fmaxf(d, 0.f) - d * yi + log1pf(expf(-fabsf(d))));
                v1 += wt;
            } else {
                const float e = g * (logf(bi + s) - logf(1.f - bi + s));
                const float d = z[i] + e;
                float v = (fmaxf(d, 0.f) - d * yi + log1pf(expf(-fabsf(d)))) * c_loss;
                if (mixin) {
                    const float ae = fabsf(e), t = expf(-ae);
                    v += c_ent * (log1pf(t) + ae * t / (1.f + t));
                }
                v0 += v;
            }
        }
        acc0 += block_sum(v0);
        if (rew) acc1 += block_sum(v1);
    }
    float t0, t1;
    if (ordered_grid_sum2(acc0, acc1, a.ws, gridDim.x, blockIdx.x, t0, t1)) {
        if (rew) {
            *a.loss += t0 / t1;
            a.save[0] = t1;  // the backward divides by the same sum of weights
        } else {
            *a.loss += t0;
        }
    }
}

template <typename T>
__device__ __forceinline__ void store_dlogit(const Args& a, int64_t i, float v) {
    if (a.dlogit_f32)
        static_cast<float*>(a.d_logit)[i] = v;
    else
        static_cast<T*>(a.d_logit)[i] = from_f32<T>(v);
}

// row kernel of the backward: d_logit, d_hidden, and per row {d loss / d pre, d loss / d s} into part[2 r], part[2 r + 1]
template <typename T>
__global__ __launch_bounds__(NT) void debias_bwd_rows_kernel(Args a) {
    const int tid = threadIdx.x;
    const bool mixin = a.kind == XGGM_DEBIAS_LEARNED_MIXIN, rew = a.kind == XGGM_DEBIAS_REWEIGHT;
    const float gk = a.gout ? *a.gout : 1.f;
    const float s = smooth_of(a);
    const float c_loss = gk / (rew ? a.save[0] : (float)a.B);
    const float c_ent = mixin ? gk * a.w / ((float)a.B * (float)a.A) : 0.f;
    const bool want_s = a.smooth_param != nullptr && a.part != nullptr && !rew;
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        const float g = mixin ? a.save[a.B + r] : 1.f;
        const float *z = a.logits + (int64_t)r * a.A, *y = a.labels + (int64_t)r * a.A, *b = bias_row(a, r);
        const int64_t o = (int64_t)r * a.A;
        float dg = 0.f, ds = 0.f;
        for (int i = tid; i < a.A; i += NT) {
            const float bi = b[i];
            if (rew) {
                store_dlogit<T>(a, o + i, (1.f - bi) * (sigmoid_stable(z[i]) - y[i]) * c_loss);
                continue;
            }
            const float lo = bi + s, hi = 1.f - bi + s;
            const float pq = logf(lo) - logf(hi), e = g * pq;
            const float dz = (sigmoid_stable(z[i] + e) - y[i]) * c_loss;
            store_dlogit<T>(a, o + i, dz);
            float te = dz;  // d loss / d e
            if (mixin) {
                const float t = expf(-fabsf(e)), u = 1.f + t;
                te -= c_ent * e * t / (u * u);
            }
            dg += te * pq;
            ds += te * g * (1.f / lo - 1.f / hi);
        }
        if (rew) continue;
        float dpre = 0.f;
        if (mixin) {
            dpre = block_sum(dg) * sigmoid_stable(a.save[r]);  // g = softplus(pre)
            if (a.d_hidden) {
                T* dh = static_cast<T*>(a.d_hidden) + (int64_t)r * a.Hd;
                for (int j = tid; j < a.Hd; j += NT) dh[j] = from_f32<T>(dpre * a.lin_w[j]);
            }
        }
        if (a.part) {
            const float dsr = want_s ? block_sum(ds) : 0.f;
            if (tid == 0) {
                a.part[2 * r] = dpre;
                a.part[2 * r + 1] = dsr;
            }
        }
    }
}

// column kernel: d bias_lin.weight[j] = sum_r dpre_r hidden[r][j], d bias_lin.bias = sum_r dpre_r, d smooth_param = (sum_r
// ds_r) sigmoid'(smooth_param) -- every sum in row order by one thread
template <typename T>
__global__ __launch_bounds__(NT) void debias_bwd_params_kernel(Args a) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (a.d_lin_w && j < a.Hd) {
        const T* h = static_cast<const T*>(a.hidden) + j;
        float acc = 0.f;
        for (int r = 0; r < a.B; ++r) acc = fmaf(a.part[2 * r], to_f32(h[(int64_t)r * a.Hd]), acc);
        a.d_lin_w[j] = a.accumulate ? a.d_lin_w[j] + acc : acc;
    }
    if (j == 0 && a.d_lin_b) {
        float acc = 0.f;
        for (int r = 0; r < a.B; ++r) acc += a.part[2 * r];
        a.d_lin_b[0] = a.accumulate ? a.d_lin_b[0] + acc : acc;
    }
    if (j == 1 && a.d_smooth) {
        float acc = 0.f;
        for (int r = 0; r < a.B; ++r) acc += a.part[2 * r + 1];
        const float sg = sigmoid_stable(*a.smooth_param);
        acc *= sg * (1.f - sg);
        a.d_smooth[0] = a.accumulate ? a.d_smooth[0] + acc : acc;
    }
}

int check_common(const xggm_debias_args* p, const char* who, Args* a) {
    XGGM_REQUIRE(p, "%s: null arguments", who);
    XGGM_REQUIRE(p->kind == XGGM_DEBIAS_REWEIGHT || p->kind == XGGM_DEBIAS_BIAS_PRODUCT || p->kind == XGGM_DEBIAS_LEARNED_MIXIN,
                 "%s: unknown kind %d", who, p->kind);
    XGGM_REQUIRE(p->B > 0 && p->A > 0 && p->B <= (1 << 20) && p->A <= (1 << 24), "%s: bad shape B=%d A=%d", who, p->B, p->A);
    XGGM_REQUIRE(p->logits && p->labels && p->bias, "%s: logits, labels and bias are required", who);
    XGGM_REQUIRE(p->bias_row_stride >= p->A && p->bias_rows >= 1, "%s: bias table of %lld rows with row stride %lld (A=%d)", who,
                 (long long)p->bias_rows, (long long)p->bias_row_stride, p->A);
    XGGM_REQUIRE(p->bias_index || p->bias_rows >= p->B, "%s: a bias of %lld rows for %d samples needs bias_index", who,
                 (long long)p->bias_rows, p->B);
    if (p->kind == XGGM_DEBIAS_LEARNED_MIXIN) {
        XGGM_REQUIRE(p->hidden && p->lin_w && p->lin_b && p->Hd > 0 && p->Hd <= (1 << 16),
                     "%s: LearnedMixin needs hidden, bias_lin.weight, bias_lin.bias and 0 < Hd <= 65536 (Hd=%d)", who, p->Hd);
        XGGM_REQUIRE(p->save, "%s: LearnedMixin needs the save buffer (2 B floats)", who);
    }
    if (p->kind == XGGM_DEBIAS_REWEIGHT) {
        XGGM_REQUIRE(p->save, "%s: ReweightByInvBias needs the save buffer (the sum of weights)", who);
        XGGM_REQUIRE(!p->smooth_param, "%s: ReweightByInvBias has no smooth_param", who);
    }
    a->logits = p->logits; a->labels = p->labels; a->bias = p->bias; a->bias_index = p->bias_index;
    a->bias_row_stride = p->bias_row_stride; a->bias_rows = p->bias_rows;
    a->hidden = p->hidden; a->lin_w = p->lin_w; a->lin_b = p->lin_b; a->smooth_param = p->smooth_param;
    a->constant_smooth = p->constant_smooth; a->w = p->w;
    a->kind = p->kind; a->B = p->B; a->A = p->A; a->Hd = p->kind == XGGM_DEBIAS_LEARNED_MIXIN ? p->Hd : 0;
    a->loss = p->loss; a->save = p->save; a->ws = p->ws; a->gout = p->gout;
    a->d_logit = p->d_logit; a->d_hidden = p->d_hidden;
    a->d_lin_w = p->d_lin_w; a->d_lin_b = p->d_lin_b; a->d_smooth = p->d_smooth; a->part = p->part;
    a->dlogit_f32 = p->dlogit_f32; a->accumulate = p->accumulate;
    return XGGM_OK;
}

template <typename T>
int debias_fwd(const xggm_debias_args* p, hipStream_t st) {
    Args a;
    if (int rc = check_common(p, "xggm_debias_fwd", &a)) return rc;
    XGGM_REQUIRE(p->loss && p->ws, "xggm_debias_fwd: the loss slot and its workspace (XGGM_SUM_WS_FLOATS floats, ws[0] == 0)");
    hipLaunchKernelGGL((debias_fwd_kernel<T>), dim3(std::min(a.B, ROW_GRID)), dim3(NT), 0, st, a);
    return xggm_check_launch("xggm_debias_fwd");
}

template <typename T>
int debias_bwd(const xggm_debias_args* p, hipStream_t st) {
    Args a;
    if (int rc = check_common(p, "xggm_debias_bwd", &a)) return rc;
    XGGM_REQUIRE(p->d_logit, "xggm_debias_bwd: d_logit is required");
    const bool mixin = a.kind == XGGM_DEBIAS_LEARNED_MIXIN, rew = a.kind == XGGM_DEBIAS_REWEIGHT;
    XGGM_REQUIRE(mixin || !(p->d_lin_w || p->d_lin_b || p->d_hidden), "xggm_debias_bwd: only LearnedMixin has bias_lin and hidden");
    XGGM_REQUIRE((p->d_lin_w != nullptr) == (p->d_lin_b != nullptr), "xggm_debias_bwd: d_lin_w and d_lin_b come together");
    XGGM_REQUIRE(!p->d_smooth || (p->smooth_param && !rew), "xggm_debias_bwd: d_smooth without smooth_param");
    const bool params = p->d_lin_w || p->d_smooth;
    XGGM_REQUIRE(!params || p->part, "xggm_debias_bwd: parameter gradients need the scratch `part` (2 B floats)");
    if (!params) a.part = nullptr;
    hipLaunchKernelGGL((debias_bwd_rows_kernel<T>), dim3(std::min(a.B, ROW_GRID)), dim3(NT), 0, st, a);
    if (int rc = xggm_check_launch("xggm_debias_bwd")) return rc;
    if (params) {
        const int cols = p->d_lin_w ? a.Hd : 0;
        hipLaunchKernelGGL((debias_bwd_params_kernel<T>), dim3(std::max(1, ceil_div(cols, NT))), dim3(NT), 0, st, a);
        return xggm_check_launch("xggm_debias_bwd (parameters)");
    }
    return XGGM_OK;
}

}  // namespace

extern "C" int xggm_debias_fwd_f32(const xggm_debias_args* args, hipStream_t st) { return debias_fwd<float>(args, st); }
extern "C" int xggm_debias_fwd_bf16(const xggm_debias_args* args, hipStream_t st) { return debias_fwd<bf16>(args, st); }
extern "C" int xggm_debias_bwd_f32(const xggm_debias_args* args, hipStream_t st) { return debias_bwd<float>(args, st); }
extern "C" int xggm_debias_bwd_bf16(const xggm_debias_args* args, hipStream_t st) { return debias_bwd<bf16>(args, st); }
