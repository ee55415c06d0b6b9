// Loss kernels and the fused optimiser.
//   xggm_dsm_loss_fwd/bwd   denoising score matching  (src/vqa/vqacpv2.py:48-51)
//   xggm_symkl_fwd/bwd      symmetric KL of row softmaxes (src/vqa/vqacpv2.py:54-61)
//   xggm_bce_fwd/bwd        BCEWithLogits(mean) * A   (src/vqa/vqacpv2.py:131,173)
//   xggm_sqnorm_* / xggm_clip_norm_*  sum of squares of gradient ranges in a fixed order (clip_grad_norm_, vqacpv2.py:175)
//   xggm_optim_multi        clip-scale + BertAdam update + bf16 shadow weight, ONE pass over
//                           p/g/m/v (src/lxrt/optimization.py:159-193): 16 B read + 12(+2) B
//                           written per parameter, the HBM floor of the update; the same pass for
//                           torch.optim's Adam / AdamW / Adamax / SGD / RMSprop rules (src/param.py:9-31)
//   xggm_sched_step         warmup_linear(step/t_total) on the device-resident step counter
//   xggm_sched_step_ex      schedule kinds per entry + bias corrections in double from the device counter
//                           (optimization.py:42-48,177-181) so a captured graph replays correctly
// Scalars (losses, norms, schedule values, upstream gradients) live in device memory: nothing
// here synchronises with the host.
#include "common.h"
#include "xggm.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float block_sum(float v) {
    __shared__ float red[NT / 64];
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

inline int grid1d(int64_t n, int cap = 1024) { return (int)std::min<int64_t>(ceil_div64(n, NT), cap); }
// workgroups of a kernel that ends in ordered_grid_sum: every one pays a ticket, and the last one adds them all.  While
// the ticket sat behind a device-scope release fence (a write-back of the XCD's L2), 1024 workgroups made the DSM loss
// 36 us instead of 15 and the grid was held at 128 -- which left the symmetric KL's forward with nine rows per workgroup
// (29 us against its backward's 12).  The fence is gone (common.h): one workgroup per four rows again, up to 512.
constexpr int LOSS_GRID = 512;

// ------------------------------------------------------------------------------- DSM
template <typename T>
__global__ __launch_bounds__(NT) void dsm_fwd_kernel(const T* __restrict__ s, const float* __restrict__ g, float* loss,
                                                     int64_t n, float coef, float* ws) {
    float acc = 0.f;
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(g)) & 15) == 0 ? n >> 2 : 0;
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < n4; t += (int64_t)gridDim.x * NT) {  // four elements per load
        float sv[4], gv[4];
        load4(s + 4 * t, sv);
        load4(g + 4 * t, gv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = sv[i] - gv[i];
            acc += d * d;
        }
    }
    for (int64_t t = 4 * n4 + (int64_t)blockIdx.x * NT + threadIdx.x; t < n; t += (int64_t)gridDim.x * NT) {
        const float d = to_f32(s[t]) - g[t];
        acc += d * d;
    }
    acc = block_sum(acc);
    float total;
    if (ordered_grid_sum(acc, ws, gridDim.x, blockIdx.x, total)) *loss += total * coef;
}
template <typename T>
__global__ __launch_bounds__(NT) void dsm_bwd_kernel(const T* __restrict__ s, const float* __restrict__ g,
                                                     const float* __restrict__ gout, T* ds, int64_t n, float coef) {
    const float k = 2.f * coef * (gout ? *gout : 1.f);
    for (int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x; t < n; t += (int64_t)gridDim.x * NT)
        ds[t] = from_f32<T>(k * (to_f32(s[t]) - g[t]));
}

// ------------------------------------------------------------------------------- symmetric KL
// per row: f = sum_c (px - py)(lpx - lpy);  df/dx_k = px_k (u_k - <u>_px) + w_k,
// df/dy_k = -py_k (u_k - <u>_py) - w_k  with u = lpx - lpy, w = px - py.
template <typename T, int NV>
__global__ __launch_bounds__(NT) void symkl_kernel(const T* __restrict__ x, const T* __restrict__ y, float* loss,
                                                   const float* __restrict__ gout, T* dx, T* dy, int rows, int W, float coef,
                                                   int accumulate, float* ws) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float gk = coef * ((dx || dy) && gout ? *gout : 1.f);
    float total = 0.f;
    for (int row = blockIdx.x * 4 + wid; row < rows; row += gridDim.x * 4) {
        const int64_t rb = (int64_t)row * W;
        float xv[NV], yv[NV];
        float mx = -INFINITY, my = -INFINITY;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 64 + lane;
            xv[v] = c < W ? to_f32(x[rb + c]) : -INFINITY;
            yv[v] = c < W ? to_f32(y[rb + c]) : -INFINITY;
            mx = fmaxf(mx, xv[v]);
            my = fmaxf(my, yv[v]);
        }
        mx = wave_max(mx);
        my = wave_max(my);
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 64 + lane;
            if (c < W) {
                sx += __expf(xv[v] - mx);
                sy += __expf(yv[v] - my);
            }
        }
        const float lx = mx + __logf(wave_sum(sx)), ly = my + __logf(wave_sum(sy));
        float f = 0.f, upx = 0.f, upy = 0.f;
        float u[NV], px[NV], py[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 64 + lane;
            u[v] = px[v] = py[v] = 0.f;
            if (c < W) {
                const float lpx = xv[v] - lx, lpy = yv[v] - ly;
                px[v] = __expf(lpx);
                py[v] = __expf(lpy);
                u[v] = lpx - lpy;
                f += (px[v] - py[v]) * u[v];
                upx += px[v] * u[v];
                upy += py[v] * u[v];
            }
        }
        total += f;  // lane partial; reduced once per block below
        if (dx || dy) {
            upx = wave_sum(upx);
            upy = wave_sum(upy);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = v * 64 + lane;
                if (c < W) {
                    const float w = px[v] - py[v];
                    if (dx) {
                        float gx = gk * (px[v] * (u[v] - upx) + w);
                        if (accumulate) gx += to_f32(dx[rb + c]);
                        dx[rb + c] = from_f32<T>(gx);
                    }
                    if (dy) {
                        float gy = gk * (-py[v] * (u[v] - upy) - w);
                        if (accumulate) gy += to_f32(dy[rb + c]);
                        dy[rb + c] = from_f32<T>(gy);
                    }
                }
            }
        }
    }
    if (loss) {
        total = block_sum(total);
        float sum;
        if (ordered_grid_sum(total, ws, gridDim.x, blockIdx.x, sum)) *loss += sum * coef;
    }
}

// ------------------------------------------------------------------------------- BCE with logits
__global__ __launch_bounds__(NT) void bce_fwd_kernel(const float* __restrict__ l, const float* __restrict__ t, float* loss,
                                                     int64_t n, float coef, float* ws) {
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float z = l[i];
        acc += fmaxf(z, 0.f) - z * t[i] + log1pf(__expf(-fabsf(z)));
    }
    acc = block_sum(acc);
    float total;
    if (ordered_grid_sum(acc, ws, gridDim.x, blockIdx.x, total)) *loss += total * coef;
}
template <typename T>
__global__ __launch_bounds__(NT) void bce_bwd_kernel(const float* __restrict__ l, const float* __restrict__ t,
                                                     const float* __restrict__ gout, T* dl, int64_t n, float coef) {
    const float k = coef * (gout ? *gout : 1.f);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        dl[i] = from_f32<T>(k * (sigmoid_f(l[i]) - t[i]));
}

// ------------------------------------------------------------------------------- optimiser
// The gradient norm (clip_grad_norm_, vqacpv2.py:175): "sum (the squares of) some ranges in a fixed order, then finish a
// scalar", in two launches.  norm_partials_kernel: every workgroup owns one slice of one range and writes its partial to
// ws in (range, slice) order.  norm_finish_kernel: one workgroup adds the partials in that order -- no floating-point
// atomics, the same bits whatever the scheduling, so replicas that hold the same gradients keep the same norm.  A
// separate launch instead of a last-arriver finish in the first kernel: the device-scope fence that needs costs an L2
// write-back per workgroup (3.5 -> 1.6 TB/s measured).  norm_of_ranges (below) shares out the workgroups.
//
// one workgroup's share of one range: slice b of nb, four 16-byte loads in flight per thread
template <bool SQ>
__device__ __forceinline__ float span_partial(const float* __restrict__ g, int64_t n, int b, int nb) {
    const int64_t n4 = n >> 2;
    typedef float __attribute__((ext_vector_type(4))) f4;
    const f4* g4 = reinterpret_cast<const f4*>(g);
    const int64_t stride = (int64_t)nb * NT;
    float acc = 0.f;
    int64_t i = (int64_t)b * NT + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f4 a = __builtin_nontemporal_load(g4 + i), bb = __builtin_nontemporal_load(g4 + i + stride),
                 c = __builtin_nontemporal_load(g4 + i + 2 * stride), d = __builtin_nontemporal_load(g4 + i + 3 * stride);
        if (SQ)
            acc += (a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w) + (bb.x * bb.x + bb.y * bb.y + bb.z * bb.z + bb.w * bb.w) +
                   (c.x * c.x + c.y * c.y + c.z * c.z + c.w * c.w) + (d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w);
        else
            acc += ((a.x + a.y) + (a.z + a.w)) + ((bb.x + bb.y) + (bb.z + bb.w)) + ((c.x + c.y) + (c.z + c.w)) +
                   ((d.x + d.y) + (d.z + d.w));
    }
    for (; i < n4; i += stride) {
        const f4 v = g4[i];
        acc += SQ ? v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w : (v.x + v.y) + (v.z + v.w);
    }
    if (b == 0 && threadIdx.x < (n & 3)) {
        const float v = g[(n4 << 2) + threadIdx.x];
        acc += SQ ? v * v : v;
    }
    return block_sum(acc);
}

// the same slice of a range of a bf16 buffer (the data-parallel wire arena): 8 elements per 16-byte load, four in flight
__device__ __forceinline__ float span_partial_bf16(const bf16* __restrict__ g, int64_t n, int b, int nb) {
    typedef short __attribute__((ext_vector_type(8))) s8;
    const s8* g8 = reinterpret_cast<const s8*>(g);
    const int64_t n8 = n >> 3, stride = (int64_t)nb * NT;
    float acc = 0.f;
    auto sq8 = [](const s8 v) {
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = __bfloat162float(__builtin_bit_cast(bf16, (short)v[e]));
            t += f * f;
        }
        return t;
    };
    int64_t i = (int64_t)b * NT + threadIdx.x;
    for (; i + 3 * stride < n8; i += 4 * stride) {
        const s8 a = __builtin_nontemporal_load(g8 + i), bb = __builtin_nontemporal_load(g8 + i + stride),
                 c = __builtin_nontemporal_load(g8 + i + 2 * stride), d = __builtin_nontemporal_load(g8 + i + 3 * stride);
        acc += (sq8(a) + sq8(bb)) + (sq8(c) + sq8(d));
    }
    for (; i < n8; i += stride) acc += sq8(g8[i]);
    if (b == 0 && threadIdx.x < (n & 7)) {
        const float f = __bfloat162float(g[(n8 << 3) + threadIdx.x]);
        acc += f * f;
    }
    return block_sum(acc);
}

// ranges [0, n_sq) are squared, [n_sq, n) summed as they are (fp32 only: a bf16 launch has n_sq == n)
constexpr int MAX_NORM_SPANS = 24;
template <typename T>
struct NormSpans {
    const T* ptr[MAX_NORM_SPANS];
    int64_t len[MAX_NORM_SPANS];
    int blk0[MAX_NORM_SPANS + 1];  // first workgroup of each range
    int n, n_sq;
};
// first stage: workgroup blockIdx.x finds its range k and its slice of it, and leaves that slice's sum in ws[blockIdx.x]
template <typename T>
__global__ __launch_bounds__(NT) void norm_partials_kernel(NormSpans<T> sp, float* ws) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < MAX_NORM_SPANS; ++j)
        if (j < sp.n && (int)blockIdx.x >= sp.blk0[j]) k = j;
    const int b = blockIdx.x - sp.blk0[k], nb = sp.blk0[k + 1] - sp.blk0[k];
    float acc;
    if constexpr (std::is_same<T, float>::value)
        acc = k < sp.n_sq ? span_partial<true>(sp.ptr[k], sp.len[k], b, nb) : span_partial<false>(sp.ptr[k], sp.len[k], b, nb);
    else
        acc = span_partial_bf16(sp.ptr[k], sp.len[k], b, nb);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

struct AdamArgs {
    float* p;
    const void* g;          // fp32, or bf16 when GB16
    float* m;
    float* v;
    bf16* shadow;
    int64_t n;
    const float* sqnorm;    // device scalar: sum of squares over ALL grads of the step (or null)
    float max_norm;
    float lr;
    const float* lr_dev;    // device scalar replacing lr (or null)
    const float* lr_scale;  // device scalar from xggm_sched_step (or null = 1)
    float b1, b2, eps, wd;
    unsigned char* shadow8;     // e4m3 copy of the updated weights (or null)
    const uint16_t* w8_id;      // per 256-element arena chunk: entry of the scale table, 0 = no e4m3 copy
    const float* w8_qscale;
    float* w8_amax;
    int64_t elem0;              // arena offset of p[0] (multiple of 256 with shadow8)
    float g_scale;              // gradients are SUMS over data-parallel ranks: 1 / world (1 otherwise)
    int w8_slots;               // floats every w8_amax entry is spread over (>= 1)
};

// One element of src/lxrt/optimization.py:159-193 (no bias correction, decoupled weight decay) with the shape of every
// multiply-add PINNED: which products fuse into an fma is otherwise the compiler's choice per instantiation under
// -ffp-contract=fast (the backend fuses whatever the source says), and the fp32- and the bf16-gradient instantiation of
// this template then differed in the last bit of v and p.  __fmul_rn / __fadd_rn are rounded on their own and never
// fused; the three fmaf are the fusions wanted.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float gk, float b1, float b2, float eps, float wd, float lr) {
    m = __fmaf_rn(m, b1, __fmul_rn(1.f - b1, gk));
    v = __fmaf_rn(v, b2, __fmul_rn(__fmul_rn(1.f - b2, gk), gk));
    const float upd = __fadd_rn(m / __fadd_rn(sqrtf(v), eps), __fmul_rn(wd, p));
    p = __fmaf_rn(-lr, upd, p);
}

// The reference's other optimisers (src/param.py:9-31, src/vqa/vqacpv2.py:141: torch.optim classes) on the same pass.
// A rule is a compile-time instantiation of the body; SGD and RMSprop come with and without a momentum buffer so that a
// buffer the rule does not have is neither read nor written.
enum { R_BERT = 0, R_ADAM, R_ADAMAX, R_SGD0, R_SGDM, R_RMS0, R_RMSM };
template <int RULE> struct RuleTraits {
    static constexpr bool use_m = RULE == R_BERT || RULE == R_ADAM || RULE == R_ADAMAX || RULE == R_SGDM || RULE == R_RMSM;
    static constexpr bool use_v = RULE == R_BERT || RULE == R_ADAM || RULE == R_ADAMAX || RULE == R_RMS0 || RULE == R_RMSM;
};
struct RuleArgs {
    const float* hs = nullptr;  // device: {1 / bc1, 1 / sqrt(bc2), first step} (xggm_sched_step_ex)
    float omb1 = 0.f, omb2 = 0.f;  // 1 - b1, 1 - b2 (RMSprop: 1 - alpha), rounded from DOUBLE differences
    float mom = 0.f, omd = 0.f;    // momentum, 1 - dampening
    int nesterov = 0;
    int decoupled = 0;             // AdamW: p *= 1 - lr * wd first, no wd in g'
};
// what a rule needs once per launch and span (uniform over the grid)
struct RuleStep {
    float lr;         // scheduled lr; Adam / Adamax: lr / bc1
    float isb2 = 1.f;  // 1 / sqrt(bc2)
    float dec = 1.f;   // AdamW: 1 - lr * wd
    float wd = 0.f;    // coupled weight decay of g'
    bool first = false;
};
template <int RULE>
__device__ __forceinline__ RuleStep rule_step(const AdamArgs& a, const RuleArgs& r, float lr) {
    RuleStep s;
    s.lr = lr;
    s.wd = a.wd;
    if (RULE == R_BERT) return s;
    if (r.decoupled) {
        s.dec = __fmaf_rn(-lr, a.wd, 1.f);
        s.wd = 0.f;
    }
    if (RULE == R_ADAM || RULE == R_ADAMAX) {
        s.lr = __fmul_rn(lr, r.hs[0]);
        s.isb2 = r.hs[1];
    }
    if (RULE == R_SGDM) s.first = r.hs[2] != 0.f;
    return s;
}
// the same under a hyper map (bertadam_body, MAP): lr and wd are the element's param_group's, per lane; `u` is
// rule_step's result for the span, whose device scalars (isb2, first and -- kept in u.lr by the caller, who passes lr 1 --
// 1 / bc1) are taken over, so they are read once per thread.  The derived values have rule_step's pinned shapes.
template <int RULE>
__device__ __forceinline__ RuleStep rule_step_lane(const RuleArgs& r, const RuleStep& u, float lr, float wd) {
    RuleStep s;
    s.lr = lr;
    s.wd = wd;
    if (RULE == R_BERT) return s;
    if (r.decoupled) {
        s.dec = __fmaf_rn(-lr, wd, 1.f);
        s.wd = 0.f;
    }
    if (RULE == R_ADAM || RULE == R_ADAMAX) {
        s.lr = __fmul_rn(lr, u.lr);
        s.isb2 = u.isb2;
    }
    s.first = u.first;
    return s;
}
// One element; the multiply-adds are pinned as in adam_update, so the fp32- and the bf16-gradient instantiation of a
// rule give the same bits on the same values.  Operation order after torch/optim/{adam,adamax,sgd,rmsprop}.py
// (_single_tensor_*); with a zero gradient and zero state a zero p stays exactly zero under every rule, and so do its
// shadow and m; v does too except under Adamax, whose exp_inf = max(b2 u, |g| + eps) becomes eps by torch's definition.
template <int RULE, bool MAP = false>
__device__ __forceinline__ void rule_update(float& p, float& m, float& v, float gk, const AdamArgs& a, const RuleArgs& r,
                                            const RuleStep& s) {
    if (RULE == R_BERT) {
        adam_update(p, m, v, gk, a.b1, a.b2, a.eps, MAP ? s.wd : a.wd, s.lr);
        return;
    }
    if (r.decoupled) p = __fmul_rn(p, s.dec);
    const float g = __fmaf_rn(s.wd, p, gk);
    if (RULE == R_ADAM) {
        m = __fmaf_rn(__fadd_rn(g, -m), r.omb1, m);
        v = __fmaf_rn(v, a.b2, __fmul_rn(__fmul_rn(r.omb2, g), g));
        p = __fmaf_rn(-s.lr, m / __fmaf_rn(sqrtf(v), s.isb2, a.eps), p);
    } else if (RULE == R_ADAMAX) {
        m = __fmaf_rn(__fadd_rn(g, -m), r.omb1, m);
        v = fmaxf(__fmul_rn(a.b2, v), __fadd_rn(fabsf(g), a.eps));
        p = __fmaf_rn(-s.lr, m / v, p);
    } else if (RULE == R_SGD0) {
        p = __fmaf_rn(-s.lr, g, p);
    } else if (RULE == R_SGDM) {
        m = s.first ? g : __fmaf_rn(r.mom, m, __fmul_rn(r.omd, g));
        p = __fmaf_rn(-s.lr, r.nesterov ? __fmaf_rn(r.mom, m, g) : m, p);
    } else {  // R_RMS0, R_RMSM
        v = __fmaf_rn(v, a.b2, __fmul_rn(__fmul_rn(r.omb2, g), g));
        const float d = g / __fadd_rn(sqrtf(v), a.eps);
        if (RULE == R_RMSM) {
            m = __fmaf_rn(r.mom, m, d);
            p = __fmaf_rn(-s.lr, m, p);
        } else {
            p = __fmaf_rn(-s.lr, d, p);
        }
    }
}

// One float4 of each of p, g, m, v per step; UNR = 2 independent float4 quadruples per thread and
// iteration (loads issued before any use).  g is read once and m, v, shadow are not re-read before the
// next step: non-temporal accesses keep them from displacing the weights' bf16 shadow in L2/MALL.
// Measured on MI355X (tools/bench_adam.py, 110 M parameters): 4.7 TB/s with plain accesses and a 4096-block
// grid-stride loop, 6.3 TB/s with non-temporal g/m/v and one or two float4 quadruples per thread.
//
// MAP (split param_groups): lr and weight decay are the element's own -- hm.ids holds one id per 8 elements of the arena
// (tensors start on multiples of 8, so a float4 never mixes two tensors; a wave does, in the vector region: the values are
// per lane), hm.table {lr, weight_decay} per id.  Id 0 = not in this optimiser: nothing of the element is written (p, m,
// v, shadow, e4m3 copy).  The span's a.lr / a.lr_dev / a.wd are not read; lr_scale, the clip scale and everything else
// are the span's.  The map is a compile-time switch: without it the body is the code it was.
struct HyperMap {
    const unsigned char* ids = nullptr;
    const float2* table = nullptr;
    unsigned n_table = 0;
};
template <bool GB16, int RULE, bool MAP>
__device__ __forceinline__ void bertadam_body(const AdamArgs& a, const int blk, const int nblk, const RuleArgs& ra,
                                              const HyperMap& hm) {
    constexpr int UNR = 2;
    constexpr bool USE_M = RuleTraits<RULE>::use_m, USE_V = RuleTraits<RULE>::use_v;
    float coef = 1.f;
    if (a.sqnorm) {
        const float total = sqrtf(*a.sqnorm);
        coef = fminf(a.max_norm / (total + 1e-6f), 1.f);  // torch.nn.utils.clip_grad_norm_
    }
    coef *= a.g_scale;
    // MAP: the span's schedule value alone; rule_step with lr 1 then leaves 1 / bc1 in rs.lr (1 * x is x)
    const float lr = (MAP ? 1.f : (a.lr_dev ? *a.lr_dev : a.lr)) * (a.lr_scale ? *a.lr_scale : 1.f);
    const float lr_scale = lr;
    const RuleStep rs = rule_step<RULE>(a, ra, MAP ? 1.f : lr);
    const int64_t n4 = a.n >> 2;
    typedef float __attribute__((ext_vector_type(4))) f4;
    typedef short __attribute__((ext_vector_type(4))) s4;
    const int64_t stride = (int64_t)nblk * NT;
    const int lane = threadIdx.x & 63;
    // every wave handles 64 consecutive float4 = one 256-element chunk of the arena per unrolled step, so the
    // chunk's scale-table entry is wave-uniform.  The trip count is made block-uniform (i0 of thread 0) so that
    // the wave reduction below runs with all lanes present; lanes beyond n4 only idle.
    for (int64_t b0 = (int64_t)blk * NT; b0 < n4; b0 += stride * UNR) {
        const int64_t i0 = b0 + threadIdx.x;
        f4 p[UNR], g[UNR], m[UNR], v[UNR];
        // e4m3 copy: the chunk's scale-table entry and its scale are fetched FIRST -- the oldest loads of the iteration,
        // so waiting for them (to issue the dependent scale load) leaves the streams below in flight, and both are long
        // back when the packed bytes are stored (they sat behind the update's arithmetic before: a dependent L2 round
        // trip or two at the end of every step)
        unsigned w8id[UNR];
        unsigned hid[UNR];  // MAP: the float4's param_group, 0 (also past the end, and for an id the table does not hold) = skip
        if (MAP) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t i = i0 + u * stride;
                const unsigned id = i < n4 ? hm.ids[(a.elem0 + 4 * i) >> 3] : 0u;
                hid[u] = id < hm.n_table ? id : 0u;
            }
        }
        if (a.shadow8) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t iw = (b0 + (threadIdx.x & ~63)) + u * stride;
                w8id[u] = iw < n4 ? a.w8_id[(a.elem0 + 4 * iw) >> 8] : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n4 && (!MAP || hid[u])) {
                p[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.p) + i);
                if (GB16) {
                    const s4 gb = __builtin_nontemporal_load(reinterpret_cast<const s4*>(a.g) + i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) g[u][k] = __bfloat162float(__builtin_bit_cast(bf16, (short)gb[k]));
                } else {
                    g[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.g) + i);
                }
                if (USE_M) m[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.m) + i);
                if (USE_V) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.v) + i);
                if (!USE_M) m[u] = f4{0.f, 0.f, 0.f, 0.f};
                if (!USE_V) v[u] = f4{0.f, 0.f, 0.f, 0.f};
            }
        }
        float w8q[UNR];
        if (a.shadow8) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) w8q[u] = w8id[u] ? a.w8_qscale[w8id[u]] : 0.f;
        }
        float2 hyp[UNR];
        if (MAP) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) hyp[u] = hid[u] ? hm.table[hid[u]] : float2{0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t i = i0 + u * stride;
            const bool on = i < n4 && (!MAP || hid[u]);
            if (on) {
                const RuleStep rl = MAP ? rule_step_lane<RULE>(ra, rs, __fmul_rn(hyp[u].x, lr_scale), hyp[u].y) : rs;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pk = p[u][k], mk = m[u][k], vk = v[u][k];
                    rule_update<RULE, MAP>(pk, mk, vk, __fmul_rn(g[u][k], coef), a, ra, rl);
                    p[u][k] = pk;
                    m[u][k] = mk;
                    v[u][k] = vk;
                }
                __builtin_nontemporal_store(p[u], reinterpret_cast<f4*>(a.p) + i);
                if (USE_M) __builtin_nontemporal_store(m[u], reinterpret_cast<f4*>(a.m) + i);
                if (USE_V) __builtin_nontemporal_store(v[u], reinterpret_cast<f4*>(a.v) + i);
                if (a.shadow) {
                    s4 sh;
#pragma unroll
                    for (int k = 0; k < 4; ++k) sh[k] = __builtin_bit_cast(short, __float2bfloat16(p[u][k]));
                    reinterpret_cast<s4*>(a.shadow)[i] = sh;
                }
            }
            if (a.shadow8) {
                // chunk of lane 0 == chunk of every lane of the wave; lanes past the end contribute nothing
                const unsigned id = w8id[u];
                if (id) {
                    const float q = w8q[u];
                    float mx = 0.f;
                    if (on) {
                        mx = fmaxf(fmaxf(fabsf(p[u][0]), fabsf(p[u][1])), fmaxf(fabsf(p[u][2]), fabsf(p[u][3])));
                        reinterpret_cast<int*>(a.shadow8)[i] = pack4_e4m3(p[u][0], p[u][1], p[u][2], p[u][3], q);
                    }
                    // Only maxima near or beyond the representable range matter to the next scale (e4m3 is a
                    // floating-point format: a stale smaller range costs nothing until values shrink by orders of
                    // magnitude, see xggm_fp8_scale_update): a few per cent of the waves issue the atomic.
                    mx = wave_max(mx);
                    if (lane == 0 && mx > 0.75f * 448.f / q) amax_record(a.w8_amax + (int64_t)id * a.w8_slots, a.w8_slots, blk, mx);
                }
            }
        }
    }
    if (blk == 0 && threadIdx.x < (a.n & 3)) {  // (ranges with an e4m3 copy are multiples of 256: no tail there)
        const int64_t i = (n4 << 2) + threadIdx.x;
        RuleStep rl = rs;
        if (MAP) {
            unsigned id = hm.ids[(a.elem0 + i) >> 3];
            if (id >= hm.n_table) id = 0u;
            if (!id) return;
            const float2 h = hm.table[id];
            rl = rule_step_lane<RULE>(ra, rs, __fmul_rn(h.x, lr_scale), h.y);
        }
        const float gi = GB16 ? __bfloat162float(reinterpret_cast<const bf16*>(a.g)[i]) : reinterpret_cast<const float*>(a.g)[i];
        float p = a.p[i], m = USE_M ? a.m[i] : 0.f, v = USE_V ? a.v[i] : 0.f;
        rule_update<RULE, MAP>(p, m, v, __fmul_rn(gi, coef), a, ra, rl);
        if (USE_M) a.m[i] = m;
        if (USE_V) a.v[i] = v;
        a.p[i] = p;
        if (a.shadow) a.shadow[i] = __float2bfloat16(p);
    }
}

// several spans (the arena groups a pass updates, or a rank's slices of them) in ONE launch: a workgroup finds its span
// in the prefix table and runs the same body on its share of that span's grid.  Four launches per pass before; every
// launch boundary leaves the chip draining one update's tail while the next one's first loads have not been issued.
// r[] stands behind blk0 and n: BertAdam reads no rule arguments, and what it does read keeps the kernel-argument
// offsets of a table without them.
constexpr int ADAM_MULTI = 8;
struct OptimSpans {
    AdamArgs a[ADAM_MULTI];
    int blk0[ADAM_MULTI + 1];
    int n;
    RuleArgs r[ADAM_MULTI];
};
// the kernel of every rule (the trace tools find the end of a pass by this name); hm is read under MAP only
template <bool GB16, int RULE, bool MAP>
__global__ __launch_bounds__(NT) void bertadam_multi_kernel(OptimSpans sp, HyperMap hm) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MULTI; ++k)
        if (k < sp.n && (int)blockIdx.x >= sp.blk0[k]) j = k;
    bertadam_body<GB16, RULE, MAP>(sp.a[j], (int)blockIdx.x - sp.blk0[j], sp.blk0[j + 1] - sp.blk0[j], sp.r[j], hm);
}

// Delayed scaling of the e4m3 operands (weights and activation sites share one table).  Producers record the
// maximum of a step only when it comes near the representable range 448 / q (> 1/2 of it; the weight update
// > 3/4), so per entry: a recorded maximum m within the history -> range = margin * m; nothing recorded for a whole
// history -> the range halves when `shrink` (values have shrunk a lot; still no overflow, finer subnormals) or stays
// (weights).  qscale <= 0 marks an entry that has not been calibrated: its producers quantise with 1 and record
// every maximum, and it stays uncalibrated until something was recorded.
// One workgroup of 16 waves; a wave takes FOUR entries per round with all eight loads in flight together (lane s reads
// slot s of an entry's maximum, lane j element j of its history: coalesced, reduced with wave_max).  The first form --
// one thread per entry walking its 64 slots -- took 12.8 us per launch, five launches per iteration of the fp8 step.
__global__ __launch_bounds__(1024) void fp8_scale_update_kernel(float* amax, float* hist, float* qscale, float* dscale, int64_t* pos,
                                                                int n, int hist_len, float margin, int shrink, int bump, int slots) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int slot = (int)(*pos % hist_len);
    constexpr int E = 4;
    for (int i0 = wid * E; i0 < n; i0 += 16 * E) {
        float am[E], h[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = i0 + e;
            am[e] = (i < n && lane < slots) ? amax[(int64_t)i * slots + lane] : 0.f;
            h[e] = (i < n && lane < hist_len) ? hist[(int64_t)i * hist_len + lane] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = i0 + e;
            if (i < n && lane < slots) amax[(int64_t)i * slots + lane] = 0.f;
            const float a = wave_max(am[e]);
            const float m = wave_max(lane == slot ? a : h[e]);  // the history with this step's maximum in its slot
            if (i < n && lane == 0) {
                hist[(int64_t)i * hist_len + slot] = a;
                const float q0 = qscale[i];
                float q = q0;
                if (m > 0.f) q = 448.f / (m * margin);
                else if (q0 > 0.f && shrink && slot == hist_len - 1) q = fminf(q0 * 2.f, 1.0995e12f);
                if (q > 0.f) {
                    qscale[i] = q;
                    dscale[i] = 1.f / q;
                }
            }
        }
    }
    __syncthreads();  // every wave has read *pos
    if (bump && threadIdx.x == 0) *pos += 1;
}

// the float schedule step of one counter: *lr_scale = warmup_linear(*step / t_total, warmup); *step += 1
// (optimization.py:42-48; t_total <= 0: scale = 1)
__device__ __forceinline__ void sched_step_f32(int64_t* step, float* lr_scale, int64_t t_total, float warmup) {
    const int64_t s = *step;
    float sc = 1.f;
    if (t_total > 0) {
        const float x = (float)((double)s / (double)t_total);
        sc = x < warmup ? x / warmup : fmaxf((x - 1.f) / (warmup - 1.f), 0.f);
    }
    *lr_scale = sc;
    *step = s + 1;
}

// that step for several counters of one table in ONE launch (all parameter groups of an optimiser step)
constexpr int MAX_SCHED = 16;
struct SchedArgs {
    int index[MAX_SCHED];
    int64_t t_total[MAX_SCHED];
    float warmup[MAX_SCHED];
    int n;
};
__global__ void sched_multi_kernel(int64_t* steps, float* lr_scale, SchedArgs a) {
    const int i = threadIdx.x;
    if (blockIdx.x != 0 || i >= a.n) return;
    sched_step_f32(steps + a.index[i], lr_scale + a.index[i], a.t_total[i], a.warmup[i]);
}

// second stage of the norm: one workgroup adds the partials in index order, seeds / extends the running sum, scales it,
// writes the norm, and takes the tail of the pass along (schedule step of sa.n counters, RNG advance): the host issues
// no fill, add, sqrt, schedule or RNG kernels around it.
__global__ __launch_bounds__(NT) void norm_finish_kernel(const float* __restrict__ ws, int nblk, float* out, float* norm, float mul,
                                                         int64_t* steps, float* lr_scale, SchedArgs sa, uint64_t* rng,
                                                         uint64_t rng_by, int accumulate) {
    float t = 0.f;
    for (int b = threadIdx.x; b < nblk; b += NT) t += ws[b];
    t = block_sum(t);
    if (threadIdx.x == 0) {
        const float s = ((accumulate ? *out : 0.f) + t) * mul;
        *out = s;
        if (norm) *norm = sqrtf(s);
        if (rng) rng[1] += rng_by;
    }
    const int i = threadIdx.x;
    if (i < sa.n) sched_step_f32(steps + sa.index[i], lr_scale + sa.index[i], sa.t_total[i], sa.warmup[i]);
}

// sched_multi_kernel with a schedule kind per entry (src/lxrt/optimization.py:27-48), evaluated in double, and the
// per-step scalars of the torch.optim rules: bias corrections 1 - b^t from the DEVICE counter, in double, once per step
// (fp32 1 - b2^t at t = 1, b2 = 0.999 is wrong by 1.3e-5 relative; torch takes them from Python floats)
struct SchedExArgs {
    int index[MAX_SCHED];
    int kind[MAX_SCHED];
    int64_t t_total[MAX_SCHED];
    double warmup[MAX_SCHED];
    double b1[MAX_SCHED], b2[MAX_SCHED];
    int n;
};
__global__ void sched_ex_kernel(int64_t* steps, float* lr_scale, float* hs, SchedExArgs a) {
    const int i = threadIdx.x;
    if (blockIdx.x != 0 || i >= a.n) return;
    const int k = a.index[i];
    const int64_t s = steps[k];
    double sc = 1.0;
    if (a.t_total[i] > 0) {
        const double x = (double)s / (double)a.t_total[i], w = a.warmup[i];
        if (x < w) sc = x / w;
        else if (a.kind[i] == XGGM_SCHED_COSINE) sc = 0.5 * (1.0 + cos(3.141592653589793 * x));
        else if (a.kind[i] == XGGM_SCHED_CONSTANT) sc = 1.0;
        else sc = fmax((x - 1.0) / (w - 1.0), 0.0);
    }
    lr_scale[k] = (float)sc;
    steps[k] = s + 1;
    if (hs) {
        const double t = (double)(s + 1);
        hs[4 * k + 0] = (float)(1.0 / (1.0 - pow(a.b1[i], t)));
        hs[4 * k + 1] = (float)(1.0 / sqrt(1.0 - pow(a.b2[i], t)));
        hs[4 * k + 2] = s == 0 ? 1.f : 0.f;
        hs[4 * k + 3] = 0.f;
    }
}

__global__ void rng_advance_kernel(uint64_t* rng, uint64_t by) {
    if (threadIdx.x == 0 && blockIdx.x == 0) rng[1] += by;
}

__global__ __launch_bounds__(NT) void cast_bf16_kernel(const float* __restrict__ x, bf16* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        out[i] = __float2bfloat16(x[i]);
}

__global__ __launch_bounds__(NT) void dropout_mask_kernel(float* out, int64_t n, float p, const uint64_t* rng, uint32_t sid) {
    const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        out[i] = p > 0.f ? dropout_scale(p, ik, rng[0], rng[1], sid, (uint64_t)i) : 1.f;
}

__global__ __launch_bounds__(NT) void normal_kernel(float* out, int64_t n, const uint64_t* rng, uint32_t sid) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        out[i] = philox_normal(rng[0], rng[1], sid, (uint64_t)i);
}

template <typename T>
int symkl(const void* x, const void* y, float* loss, const float* gout, void* dx, void* dy, int rows, int W, float coef,
          int accumulate, float* ws, hipStream_t st) {
    XGGM_REQUIRE(x && y && rows > 0 && W > 0, "xggm_symkl: bad arguments");
    XGGM_REQUIRE(!loss || ws, "xggm_symkl: the loss sum needs its workspace (XGGM_SUM_WS_FLOATS floats, ws[0] == 0)");
    XGGM_REQUIRE(W <= 64 * 16, "xggm_symkl: row width %d > 1024", W);
    XGGM_REQUIRE(loss || dx || dy, "xggm_symkl: nothing to compute");
    // the loss sum ends in ordered_grid_sum (a release fence and a ticket per workgroup): few, fat workgroups there
    const int grid = std::min(ceil_div(rows, 4), loss ? LOSS_GRID : 1024);
    const int nv = ceil_div(W, 64);
#define SYMKL_LAUNCH(NV)                                                                                               \
    hipLaunchKernelGGL((symkl_kernel<T, NV>), dim3(grid), dim3(NT), 0, st, (const T*)x, (const T*)y, loss, gout, (T*)dx, \
                       (T*)dy, rows, W, coef, accumulate, ws)
    if (nv <= 1) SYMKL_LAUNCH(1);
    else if (nv <= 2) SYMKL_LAUNCH(2);
    else if (nv <= 4) SYMKL_LAUNCH(4);
    else if (nv <= 8) SYMKL_LAUNCH(8);
    else if (nv <= 12) SYMKL_LAUNCH(12);
    else SYMKL_LAUNCH(16);
#undef SYMKL_LAUNCH
    return xggm_check_launch("xggm_symkl");
}

// ------------------------------------------------------------------------------- norm of ranges: host side
struct TailArgs {
    SchedArgs sa;
    int64_t* steps = nullptr;
    float* lr_scale = nullptr;
    uint64_t* rng = nullptr;
    uint64_t rng_by = 0;
};
int tail_args_of(const xggm_pass_tail* tail, TailArgs& ta) {
    ta.sa.n = 0;
    if (!tail) return XGGM_OK;
    XGGM_REQUIRE(tail->n >= 0 && tail->n <= MAX_SCHED && (tail->n == 0 || (tail->steps && tail->lr_scale && tail->index &&
                                                                         tail->t_total && tail->warmup)),
                 "xggm_clip_norm: bad schedule entries (n = %d, at most %d)", tail->n, MAX_SCHED);
    ta.sa.n = tail->n;
    for (int i = 0; i < tail->n; ++i) {
        XGGM_REQUIRE(tail->index[i] >= 0, "xggm_clip_norm: negative schedule index");
        for (int j = 0; j < i; ++j)
            XGGM_REQUIRE(tail->index[j] != tail->index[i], "xggm_clip_norm: counter %d listed twice", tail->index[i]);
        ta.sa.index[i] = tail->index[i];
        ta.sa.t_total[i] = tail->t_total[i];
        ta.sa.warmup[i] = tail->warmup[i];
    }
    ta.steps = tail->steps;
    ta.lr_scale = tail->lr_scale;
    ta.rng = tail->rng;
    ta.rng_by = tail->rng_by;
    return XGGM_OK;
}

// The one planner behind the five xggm_sqnorm_* / xggm_clip_norm_* entries: validates the n <= MAX_NORM_SPANS ranges
// (squared ones first), hands every range workgroups in proportion to its length -- 4096 in all plus at most one per
// range (the partials fit XGGM_SQNORM_WS_FLOATS), no more than leave a thread eight 16-byte loads, at least one --
// and issues the first stage (if there is any range) and the finish.  `who`: the entry's name, for the error texts.
template <typename T>
struct NormRange {
    const T* base;
    int64_t off, len;
    bool sq;
};
template <typename T>
int norm_of_ranges(const char* who, const NormRange<T>* r, int n, float* out, float* norm, float* ws, int accumulate, float mul,
                   const xggm_pass_tail* tail, hipStream_t st) {
    constexpr int VEC = 16 / sizeof(T), PER = 8 * VEC;  // elements per 16-byte load; per thread of a full workgroup
    XGGM_REQUIRE(out && ws && n >= 0 && n <= MAX_NORM_SPANS, "%s: bad arguments (null out or ws, or %d ranges)", who, n);
    NormSpans<T> sp;
    sp.n = n;
    sp.n_sq = 0;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        XGGM_REQUIRE(reinterpret_cast<uintptr_t>(r[i].base) % 16 == 0, "%s: buffers must be 16-byte aligned", who);
        XGGM_REQUIRE(r[i].off >= 0 && r[i].len > 0 && r[i].off % VEC == 0, "%s: range %d (offset %lld, length %lld) must be "
                     "non-empty and start on a multiple of %d", who, i, (long long)r[i].off, (long long)r[i].len, VEC);
        XGGM_REQUIRE(r[i].sq ? sp.n_sq == i : sizeof(T) == 4, "%s: internal: range %d out of place", who, i);
        sp.n_sq += r[i].sq;
        sp.ptr[i] = r[i].base + r[i].off;
        sp.len[i] = r[i].len;
        total += r[i].len;
    }
    int nblk = 0;
    for (int i = 0; i < n; ++i) {
        sp.blk0[i] = nblk;
        nblk += (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(sp.len[i], (int64_t)NT * PER), (4096 - n) * sp.len[i] / total + 1));
    }
    sp.blk0[n] = nblk;
    XGGM_REQUIRE(nblk <= 4100, "%s: internal: %d partials", who, nblk);
    TailArgs ta;
    if (int e = tail_args_of(tail, ta)) return e;
    if (nblk > 0) hipLaunchKernelGGL(norm_partials_kernel<T>, dim3(nblk), dim3(NT), 0, st, sp, ws);
    hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(NT), 0, st, ws, nblk, out, norm, mul, ta.steps, ta.lr_scale, ta.sa, ta.rng,
                       ta.rng_by, accumulate);
    return xggm_check_launch(who);
}

}  // namespace

#define LOSS_API(SUF, T)                                                                                                   \
    extern "C" int xggm_dsm_loss_fwd_##SUF(const void* s, const float* g, float* loss, int64_t n, float coef, float* ws,  \
                                           hipStream_t st) {                                                              \
        XGGM_REQUIRE(s && g && loss && ws && n > 0, "xggm_dsm_loss_fwd: bad arguments");                                   \
        hipLaunchKernelGGL((dsm_fwd_kernel<T>), dim3(grid1d(n / 4 + 1, LOSS_GRID)), dim3(NT), 0, st, (const T*)s, g, loss, n, coef, ws); \
        return xggm_check_launch("xggm_dsm_loss_fwd");                                                                    \
    }                                                                                                                      \
    extern "C" int xggm_dsm_loss_bwd_##SUF(const void* s, const float* g, const float* gout, void* ds, int64_t n,         \
                                           float coef, hipStream_t st) {                                                  \
        XGGM_REQUIRE(s && g && ds && n > 0, "xggm_dsm_loss_bwd: bad arguments");                                           \
        hipLaunchKernelGGL((dsm_bwd_kernel<T>), dim3(grid1d(n)), dim3(NT), 0, st, (const T*)s, g, gout, (T*)ds, n, coef); \
        return xggm_check_launch("xggm_dsm_loss_bwd");                                                                    \
    }                                                                                                                      \
    extern "C" int xggm_symkl_##SUF(const void* x, const void* y, float* loss, const float* gout, void* dx, void* dy,     \
                                    int rows, int W, float coef, int accumulate, float* ws, hipStream_t st) {             \
        return symkl<T>(x, y, loss, gout, dx, dy, rows, W, coef, accumulate, ws, st);                                     \
    }                                                                                                                      \
    extern "C" int xggm_bce_bwd_##SUF(const float* l, const float* t, const float* gout, void* dl, int64_t n, float coef, \
                                      hipStream_t st) {                                                                   \
        XGGM_REQUIRE(l && t && dl && n > 0, "xggm_bce_bwd: bad arguments");                                                \
        hipLaunchKernelGGL((bce_bwd_kernel<T>), dim3(grid1d(n)), dim3(NT), 0, st, l, t, gout, (T*)dl, n, coef);           \
        return xggm_check_launch("xggm_bce_bwd");                                                                         \
    }

LOSS_API(f32, float)
LOSS_API(bf16, bf16)

extern "C" int xggm_bce_fwd(const float* l, const float* t, float* loss, int64_t n, float coef, float* ws, hipStream_t st) {
    XGGM_REQUIRE(l && t && loss && ws && n > 0, "xggm_bce_fwd: bad arguments");
    hipLaunchKernelGGL(bce_fwd_kernel, dim3(grid1d(n, LOSS_GRID)), dim3(NT), 0, st, l, t, loss, n, coef, ws);
    return xggm_check_launch("xggm_bce_fwd");
}

extern "C" int xggm_sqnorm_f32(const float* g, int64_t n, float* out, float* ws, hipStream_t st) {
    XGGM_REQUIRE(g && n > 0, "xggm_sqnorm_f32: bad arguments");
    const NormRange<float> r{g, 0, n, true};
    return norm_of_ranges("xggm_sqnorm_f32", &r, 1, out, nullptr, ws, 1, 1.f, nullptr, st);
}

extern "C" int xggm_sqnorm_multi_f32(const float* base, const int64_t* offsets, const int64_t* lengths, int n, float* out,
                                     float* norm, float* ws, int overwrite, int square, float mul, hipStream_t st) {
    // 16 and not MAX_NORM_SPANS: how callers chunk their ranges decides the workgroups each gets, and so the bits
    XGGM_REQUIRE(base && offsets && lengths && n >= 0 && n <= 16,
                 "xggm_sqnorm_multi_f32: bad arguments (n = %d, at most 16 ranges)", n);
    NormRange<float> r[16];
    for (int i = 0; i < n; ++i) r[i] = {base, offsets[i], lengths[i], square != 0};
    return norm_of_ranges("xggm_sqnorm_multi_f32", r, n, out, norm, ws, !overwrite, mul, nullptr, st);
}

namespace {
int adam_args_of(const xggm_adam_args* x, AdamArgs& a) {
    XGGM_REQUIRE(x && x->p && x->g && x->m && x->v && x->n > 0, "xggm_optim_multi: bad arguments");
    XGGM_REQUIRE((reinterpret_cast<uintptr_t>(x->p) | reinterpret_cast<uintptr_t>(x->m) | reinterpret_cast<uintptr_t>(x->v)) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(x->g) % (x->g_bf16 ? 8 : 16) == 0,
                 "xggm_optim_multi: pointers must be 16-byte aligned (bf16 gradients: 8)");
    XGGM_REQUIRE(!x->shadow_bf16 || reinterpret_cast<uintptr_t>(x->shadow_bf16) % 8 == 0, "xggm_optim_multi: shadow misaligned");
    XGGM_REQUIRE(!x->shadow8 || (x->w8_id && x->w8_qscale && x->w8_amax && x->elem0 % 256 == 0 && x->n % 4 == 0 &&
                                 reinterpret_cast<uintptr_t>(x->shadow8) % 4 == 0),
                 "xggm_optim_multi: the e4m3 copy needs the chunk table, the scale table and a range that starts on a "
                 "256-element chunk of the arena");
    a = AdamArgs{x->p, x->g, x->m, x->v, (bf16*)x->shadow_bf16, x->n, x->sqnorm, x->max_norm, x->lr, x->lr_dev, x->lr_scale,
                 x->b1, x->b2, x->eps, x->weight_decay, (unsigned char*)x->shadow8, x->w8_id, x->w8_qscale, x->w8_amax, x->elem0,
                 x->g_scale > 0.f ? x->g_scale : 1.f, x->w8_amax_slots > 1 ? x->w8_amax_slots : 1};
    return XGGM_OK;
}

// the checks of a call with a hyper map, all before any launch: the map covers every span, and a span starts on a whole
// id (then no float4 of it straddles two)
int hyper_map_of(const xggm_hyper_map* map, const char* who, HyperMap& hm) {
    XGGM_REQUIRE(map && map->ids && map->table, "%s: the hyper map needs its id map and its {lr, weight_decay} table", who);
    XGGM_REQUIRE(map->n_table >= 1 && map->n_table <= 256, "%s: hyper table of %d entries (1 .. 256: entry 0 + one per param_group)",
                 who, map->n_table);
    XGGM_REQUIRE(map->n_ids > 0 && reinterpret_cast<uintptr_t>(map->table) % 8 == 0, "%s: empty id map or misaligned hyper table", who);
    hm.ids = map->ids;
    hm.table = reinterpret_cast<const float2*>(map->table);
    hm.n_table = (unsigned)map->n_table;
    return XGGM_OK;
}
int span_in_map(const xggm_adam_args& x, const xggm_hyper_map* map, const char* who, int i) {
    XGGM_REQUIRE(x.elem0 >= 0 && x.elem0 % 8 == 0, "%s: span %d: elem0 %lld must be a multiple of 8 (one id per 8 elements)", who, i,
                 (long long)x.elem0);
    XGGM_REQUIRE(x.n > 0 && (x.elem0 + x.n + 7) / 8 <= map->n_ids, "%s: span %d [%lld, %lld) lies outside the id map (%lld ids)", who, i,
                 (long long)x.elem0, (long long)(x.elem0 + x.n), (long long)map->n_ids);
    return XGGM_OK;
}

// a span's rule arguments (the complements in double) and the values a rule keeps in the span itself
int rule_args_of(const xggm_optim_args& x, int inst, const char* who, AdamArgs& a, RuleArgs& r) {
    r = RuleArgs();
    if (inst == R_BERT) return XGGM_OK;
    XGGM_REQUIRE(!x.a.shadow8, "%s: the e4m3 weight copy is written by the BertAdam rule only", who);
    XGGM_REQUIRE(x.step_scalars || !(inst == R_ADAM || inst == R_ADAMAX || inst == R_SGDM),
                 "%s: rule %d needs step_scalars (xggm_sched_step_ex)", who, x.rule);
    r.hs = x.step_scalars;
    r.decoupled = x.rule == XGGM_RULE_ADAMW;
    r.mom = (float)x.momentum;
    r.nesterov = x.nesterov != 0;
    r.omd = (float)(1.0 - x.dampening);
    if (inst == R_ADAM || inst == R_ADAMAX) {
        XGGM_REQUIRE(x.b1 >= 0.0 && x.b1 < 1.0 && x.b2 >= 0.0 && x.b2 < 1.0, "%s: betas outside [0, 1)", who);
        a.b1 = (float)x.b1;
        a.b2 = (float)x.b2;
        r.omb1 = (float)(1.0 - x.b1);
        r.omb2 = (float)(1.0 - x.b2);
    } else if (inst == R_RMS0 || inst == R_RMSM) {
        a.b2 = (float)x.alpha;
        r.omb2 = (float)(1.0 - x.alpha);
    }
    return XGGM_OK;
}

template <int RULE>
void launch_spans(const OptimSpans& sp, const HyperMap* hm, bool gb, int nblk, hipStream_t st) {
    const HyperMap none;
    if (hm) {
        if (gb) hipLaunchKernelGGL((bertadam_multi_kernel<true, RULE, true>), dim3(nblk), dim3(NT), 0, st, sp, *hm);
        else hipLaunchKernelGGL((bertadam_multi_kernel<false, RULE, true>), dim3(nblk), dim3(NT), 0, st, sp, *hm);
    } else if (gb) {
        hipLaunchKernelGGL((bertadam_multi_kernel<true, RULE, false>), dim3(nblk), dim3(NT), 0, st, sp, none);
    } else {
        hipLaunchKernelGGL((bertadam_multi_kernel<false, RULE, false>), dim3(nblk), dim3(NT), 0, st, sp, none);
    }
}
}  // namespace

// the planner of the update: the map and every span are checked first, then one launch per ADAM_MULTI spans
extern "C" int xggm_optim_multi(const xggm_optim_args* args, int n, const xggm_hyper_map* map, hipStream_t st) {
    const char* who = "xggm_optim_multi";
    XGGM_REQUIRE(args && n > 0, "%s: no spans", who);
    HyperMap hm;
    if (map) {
        if (int e = hyper_map_of(map, who, hm)) return e;
        for (int i = 0; i < n; ++i)
            if (int e = span_in_map(args[i].a, map, who, i)) return e;
    }
    const int rule = args[0].rule;
    XGGM_REQUIRE(rule >= XGGM_RULE_BERTADAM && rule <= XGGM_RULE_RMSPROP, "%s: unknown rule %d", who, rule);
    const bool mom0 = args[0].momentum == 0.0, gb = args[0].a.g_bf16 != 0;
    int inst = R_BERT;
    if (rule == XGGM_RULE_ADAM || rule == XGGM_RULE_ADAMW) inst = R_ADAM;
    else if (rule == XGGM_RULE_ADAMAX) inst = R_ADAMAX;
    else if (rule == XGGM_RULE_SGD) inst = mom0 ? R_SGD0 : R_SGDM;
    else if (rule == XGGM_RULE_RMSPROP) inst = mom0 ? R_RMS0 : R_RMSM;
    AdamArgs a;
    RuleArgs r;
    for (int i = 0; i < n; ++i) {
        if (int e = adam_args_of(&args[i].a, a)) return e;
        XGGM_REQUIRE(args[i].rule == rule && (args[i].momentum == 0.0) == mom0 && (args[i].a.g_bf16 != 0) == gb,
                     "%s: the spans of one call share the rule, the gradient type and whether momentum is zero", who);
        if (int e = rule_args_of(args[i], inst, who, a, r)) return e;
    }
    for (int i0 = 0; i0 < n; i0 += ADAM_MULTI) {
        OptimSpans sp;
        sp.n = std::min(ADAM_MULTI, n - i0);
        int nblk = 0;
        for (int i = 0; i < sp.n; ++i) {
            adam_args_of(&args[i0 + i].a, sp.a[i]);
            rule_args_of(args[i0 + i], inst, who, sp.a[i], sp.r[i]);
            sp.blk0[i] = nblk;
            nblk += grid1d(sp.a[i].n / 8 + 1, 65536);
        }
        sp.blk0[sp.n] = nblk;
        const HyperMap* h = map ? &hm : nullptr;
        switch (inst) {
            case R_BERT: launch_spans<R_BERT>(sp, h, gb, nblk, st); break;
            case R_ADAM: launch_spans<R_ADAM>(sp, h, gb, nblk, st); break;
            case R_ADAMAX: launch_spans<R_ADAMAX>(sp, h, gb, nblk, st); break;
            case R_SGD0: launch_spans<R_SGD0>(sp, h, gb, nblk, st); break;
            case R_SGDM: launch_spans<R_SGDM>(sp, h, gb, nblk, st); break;
            case R_RMS0: launch_spans<R_RMS0>(sp, h, gb, nblk, st); break;
            default: launch_spans<R_RMSM>(sp, h, gb, nblk, st);
        }
        if (int e = xggm_check_launch(who)) return e;
    }
    return XGGM_OK;
}

extern "C" int xggm_sqnorm_bf16(const void* g, int64_t n, float* out, float* ws, hipStream_t st) {
    XGGM_REQUIRE(g && n > 0, "xggm_sqnorm_bf16: bad arguments");
    const NormRange<bf16> r{(const bf16*)g, 0, n, true};
    return norm_of_ranges("xggm_sqnorm_bf16", &r, 1, out, nullptr, ws, 1, 1.f, nullptr, st);
}

extern "C" int xggm_fp8_scale_update(float* amax, float* hist, float* qscale, float* dscale, int64_t* pos, int n,
                                     int hist_len, float margin, int shrink, int bump, int amax_slots, hipStream_t st) {
    const int slots = amax_slots > 1 ? amax_slots : 1;
    XGGM_REQUIRE(slots <= 64 && (slots & (slots - 1)) == 0, "xggm_fp8_scale_update: amax_slots %d must be a power of two <= 64", slots);
    XGGM_REQUIRE(amax && hist && qscale && dscale && pos && n > 0 && n <= 1024 && hist_len > 0 && hist_len <= 64 && margin >= 1.f,
                 "xggm_fp8_scale_update: bad arguments (n = %d <= 1024 entries, history %d <= 64, margin %g >= 1)", n,
                 hist_len, (double)margin);
    hipLaunchKernelGGL(fp8_scale_update_kernel, dim3(1), dim3(1024), 0, st, amax, hist, qscale, dscale, pos, n, hist_len,
                       margin, shrink, bump, slots);
    return xggm_check_launch("xggm_fp8_scale_update");
}

extern "C" int xggm_sched_step(int64_t* step, float* lr_scale, int64_t t_total, float warmup, hipStream_t st) {
    XGGM_REQUIRE(step && lr_scale, "xggm_sched_step: null pointer");
    SchedArgs a;
    a.n = 1;
    a.index[0] = 0;
    a.t_total[0] = t_total;
    a.warmup[0] = warmup;
    hipLaunchKernelGGL(sched_multi_kernel, dim3(1), dim3(64), 0, st, step, lr_scale, a);
    return xggm_check_launch("xggm_sched_step");
}

extern "C" int xggm_sched_step_multi(int64_t* steps, float* lr_scale, const int* index, const int64_t* t_total,
                                     const float* warmup, int n, hipStream_t st) {
    XGGM_REQUIRE(steps && lr_scale && index && t_total && warmup && n > 0 && n <= MAX_SCHED,
                 "xggm_sched_step_multi: bad arguments (n = %d, at most %d counters per call)", n, MAX_SCHED);
    SchedArgs a;
    a.n = n;
    for (int i = 0; i < n; ++i) {
        XGGM_REQUIRE(index[i] >= 0, "xggm_sched_step_multi: negative index");
        for (int j = 0; j < i; ++j) XGGM_REQUIRE(index[j] != index[i], "xggm_sched_step_multi: counter %d listed twice", index[i]);
        a.index[i] = index[i];
        a.t_total[i] = t_total[i];
        a.warmup[i] = warmup[i];
    }
    hipLaunchKernelGGL(sched_multi_kernel, dim3(1), dim3(64), 0, st, steps, lr_scale, a);
    return xggm_check_launch("xggm_sched_step_multi");
}

extern "C" int xggm_sched_step_ex(int64_t* steps, float* lr_scale, float* step_scalars, const xggm_sched_entry* entries, int n,
                                  hipStream_t st) {
    XGGM_REQUIRE(steps && lr_scale && entries && n > 0 && n <= MAX_SCHED,
                 "xggm_sched_step_ex: bad arguments (n = %d, at most %d counters per call)", n, MAX_SCHED);
    SchedExArgs a;
    a.n = n;
    for (int i = 0; i < n; ++i) {
        const xggm_sched_entry& e = entries[i];
        XGGM_REQUIRE(e.index >= 0, "xggm_sched_step_ex: negative index");
        XGGM_REQUIRE(e.kind >= XGGM_SCHED_LINEAR && e.kind <= XGGM_SCHED_CONSTANT, "xggm_sched_step_ex: unknown schedule kind %d", e.kind);
        XGGM_REQUIRE(e.b1 >= 0.0 && e.b1 < 1.0 && e.b2 >= 0.0 && e.b2 < 1.0, "xggm_sched_step_ex: betas outside [0, 1)");
        for (int j = 0; j < i; ++j) XGGM_REQUIRE(entries[j].index != e.index, "xggm_sched_step_ex: counter %d listed twice", e.index);
        a.index[i] = e.index;
        a.kind[i] = e.kind;
        a.t_total[i] = e.t_total;
        a.warmup[i] = e.warmup;
        a.b1[i] = e.b1;
        a.b2[i] = e.b2;
    }
    hipLaunchKernelGGL(sched_ex_kernel, dim3(1), dim3(64), 0, st, steps, lr_scale, step_scalars, a);
    return xggm_check_launch("xggm_sched_step_ex");
}

extern "C" int xggm_clip_norm_f32(const float* g, const int64_t* offsets, const int64_t* lengths, int n, const float* slots,
                                  const int64_t* slot_offsets, const int64_t* slot_lengths, int n_slots, float* out, float* norm,
                                  float* ws, float mul, const xggm_pass_tail* tail, hipStream_t st) {
    XGGM_REQUIRE(n >= 0 && n_slots >= 0 && n + n_slots <= MAX_NORM_SPANS && (n == 0 || (g && offsets && lengths)) &&
                     (n_slots == 0 || (slots && slot_offsets && slot_lengths)),
                 "xggm_clip_norm_f32: bad arguments (%d + %d ranges, at most %d in all)", n, n_slots, MAX_NORM_SPANS);
    NormRange<float> r[MAX_NORM_SPANS];
    for (int i = 0; i < n; ++i) r[i] = {g, offsets[i], lengths[i], true};
    for (int i = 0; i < n_slots; ++i) r[n + i] = {slots, slot_offsets[i], slot_lengths[i], false};
    return norm_of_ranges("xggm_clip_norm_f32", r, n + n_slots, out, norm, ws, 0, mul, tail, st);
}

extern "C" int xggm_clip_norm_bf16(const void* g, const int64_t* offsets, const int64_t* lengths, int n, float* out, float* norm,
                                   float* ws, int accumulate, float mul, const xggm_pass_tail* tail, hipStream_t st) {
    XGGM_REQUIRE(n >= 0 && n <= MAX_NORM_SPANS && (n == 0 || (g && offsets && lengths)),
                 "xggm_clip_norm_bf16: bad arguments (%d ranges, at most %d)", n, MAX_NORM_SPANS);
    NormRange<bf16> r[MAX_NORM_SPANS];
    for (int i = 0; i < n; ++i) r[i] = {(const bf16*)g, offsets[i], lengths[i], true};
    return norm_of_ranges("xggm_clip_norm_bf16", r, n, out, norm, ws, accumulate, mul, tail, st);
}

extern "C" int xggm_rng_advance(uint64_t* rng, uint64_t by, hipStream_t st) {
    XGGM_REQUIRE(rng, "xggm_rng_advance: null pointer");
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(64), 0, st, rng, by);
    return xggm_check_launch("xggm_rng_advance");
}

extern "C" int xggm_cast_f32_to_bf16(const float* x, void* out, int64_t n, hipStream_t st) {
    XGGM_REQUIRE(x && out && n > 0, "xggm_cast_f32_to_bf16: bad arguments");
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid1d(n, 4096)), dim3(NT), 0, st, x, (bf16*)out, n);
    return xggm_check_launch("xggm_cast_f32_to_bf16");
}

extern "C" int xggm_dropout_mask(float* out, int64_t n, float p, const uint64_t* rng, uint32_t sid, hipStream_t st) {
    XGGM_REQUIRE(out && n > 0 && p >= 0.f && p < 1.f && (p == 0.f || rng), "xggm_dropout_mask: bad arguments");
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid1d(n)), dim3(NT), 0, st, out, n, p, rng, sid);
    return xggm_check_launch("xggm_dropout_mask");
}

extern "C" int xggm_normal(float* out, int64_t n, const uint64_t* rng, uint32_t sid, hipStream_t st) {
    XGGM_REQUIRE(out && n > 0 && rng, "xggm_normal: bad arguments");
    hipLaunchKernelGGL(normal_kernel, dim3(grid1d(n)), dim3(NT), 0, st, out, n, rng, sid);
    return xggm_check_launch("xggm_normal");
}
