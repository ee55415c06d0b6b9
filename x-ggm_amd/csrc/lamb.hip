// BertLamb: BertAdam's step (src/lxrt/optimization.py:159-193) with a layer-wise trust ratio ||p_T|| / ||u_T|| per parameter
// tensor T between its lines 171 and 192; the clip scale in front of it is clip_grad_norm_'s (src/vqa/vqacpv2.py:125-128 builds
// the optimiser this stands in for).
//   xggm_lamb_workspace_bytes   the scratch of a call
//   xggm_lamb_multi             phase A (moments + per-chunk sums of p^2 and u^2), finish (per-tensor ratios), phase B (apply)
//
// A rule that reads a statistic of the tensor it updates cannot be one pass: u is known only after m and v, the ratio only
// after every u of the tensor.  Phase A reads g, m, v, p (16 B, bf16 gradients 14), writes m, v (8 B); phase B reads m, v, p
// (12 B) and writes p and the shadow (4 + 2 B): 24 + 18 B per parameter against the one-pass update's 30.
//
// WHO SUMS WHAT.  A tensor is cut into chunks of XGGM_LAMB_CHUNK = 2048 elements counted from ITS first element, so the
// order of a tensor's sums depends on its length alone (xggm.h writes the order down).  The arena is cut into ranges of the
// same 2048 elements counted from element 0; workgroup b of a span takes range floor(elem0 / 2048) + b, clipped to the span,
// and owns every chunk whose FIRST element lies in it -- chunks of one tensor start 2048 apart, so at most one per tensor,
// and the chunk is summed by that workgroup alone even where it runs on into the next range.  A big tensor gives every
// workgroup exactly one full chunk (256 threads x two float4 of each stream: the shape of the one-pass update); in the
// vector region a workgroup walks the few tensors that start in its range.  The chunk's sums go to slot range + T of the
// workspace: consecutive for a tensor's chunks, disjoint between tensors (tensor T + 1 starts at or behind T's last chunk).
//
// HOW AN ELEMENT FINDS ITS TENSOR.  It does not: a workgroup finds the first tensor that reaches into its range by a binary
// search over the sorted DEVICE table {elem0, n, adapted} (24 B per tensor, ~12 KB for the full model: it lives in L2; the
// search is uniform over the workgroup, log2(n_tensors) dependent loads once per workgroup) and walks on from there.  No
// per-element map is read: 0 B per parameter.  Alignment gaps belong to no tensor and are neither read nor written.
#include "common.h"
#include "xggm.h"

namespace {

constexpr int NT = 256;
constexpr int CH = XGGM_LAMB_CHUNK;
constexpr int LAMB_MULTI = 8;
static_assert(CH == 2 * 4 * NT, "a chunk is two float4 per thread of a workgroup");

struct LambSpan {
    float* p;
    const void* g;  // fp32, or bf16 when GB16
    float* m;
    float* v;
    bf16* shadow;
    int64_t n, elem0;
    const float* sqnorm;
    const float* lr_dev;
    const float* lr_scale;
    float max_norm, lr, b1, b2, eps, wd, g_scale;
};
struct LambSpans {
    LambSpan a[LAMB_MULTI];
    int blk0[LAMB_MULTI + 1];
    int n;
};
struct LambTable {
    const xggm_lamb_tensor* t;
    int n;
    const unsigned char* ids;  // hyper map (MAP), as xggm_optim_multi reads it
    const float2* table;
    unsigned n_table;
    double2* ws;       // {sum p^2, sum u^2} per chunk, slot = range + tensor index
    int64_t n_slots;
    float* ratios;     // per tensor: written by the finish, read by phase B
};

// the two halves of BertAdam's element (loss_optim.hip::adam_update), multiply-adds pinned the same way: with a ratio of 1
// the bits are that function's.  Phase A and phase B both call lamb_u, so the norm describes what is applied.
__device__ __forceinline__ void lamb_moments(float& m, float& v, float gk, float b1, float b2) {
    m = __fmaf_rn(m, b1, __fmul_rn(1.f - b1, gk));
    v = __fmaf_rn(v, b2, __fmul_rn(__fmul_rn(1.f - b2, gk), gk));
}
__device__ __forceinline__ float lamb_u(float m, float v, float p, float eps, float wd) {
    return __fadd_rn(m / __fadd_rn(sqrtf(v), eps), __fmul_rn(wd, p));
}

// a[t] over the 256 threads -> the chunk's (or the tensor's) sum on every thread, in the order xggm.h gives: inside each
// wave a[l] += a[l + h] for h = 32 .. 1, then (w0 + w1) + (w2 + w3).  Call from every thread of the workgroup.
__device__ __forceinline__ void block_sum2(double& x, double& y) {
    __shared__ double red[2][NT / 64];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        x += __shfl_down(x, h, 64);
        y += __shfl_down(y, h, 64);
    }
    __syncthreads();  // (the previous call's reads of red)
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = x;
        red[1][threadIdx.x >> 6] = y;
    }
    __syncthreads();
    x = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    y = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// first tensor that ends behind position `a` (the table is sorted and its tensors are disjoint); uniform over the workgroup
__device__ __forceinline__ int first_tensor_behind(const xggm_lamb_tensor* __restrict__ t, int n, int64_t a) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid].elem0 + t[mid].n > a) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ int span_of_block(const LambSpans& sp) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < LAMB_MULTI; ++k)
        if (k < sp.n && (int)blockIdx.x >= sp.blk0[k]) j = k;
    return j;
}

typedef float __attribute__((ext_vector_type(4))) f4;
typedef short __attribute__((ext_vector_type(4))) s4;

// APPLY = false: phase A.  APPLY = true: phase B.  One body, so both walk the same chunks.
template <bool GB16, bool MAP, bool APPLY>
__global__ __launch_bounds__(NT) void lamb_kernel(LambSpans sp, LambTable tb) {
    const LambSpan& a = sp.a[span_of_block(sp)];
    const int64_t s0 = a.elem0, s1 = a.elem0 + a.n;
    const int64_t R = s0 / CH + ((int)blockIdx.x - sp.blk0[span_of_block(sp)]);
    const int64_t a0 = max(R * CH, s0), a1 = min((R + 1) * CH, s1);
    float coef = 1.f;
    if (!APPLY) {
        if (a.sqnorm) {
            const float total = sqrtf(*a.sqnorm);
            coef = fminf(a.max_norm / (total + 1e-6f), 1.f);  // torch.nn.utils.clip_grad_norm_
        }
        coef *= a.g_scale;
    }
    // (the shapes of the one-pass update: MAP multiplies the tensor's lr by the span's schedule value alone)
    const float lr_span = (MAP ? 1.f : (a.lr_dev ? *a.lr_dev : a.lr)) * (a.lr_scale ? *a.lr_scale : 1.f);
    const int tid = threadIdx.x;
    for (int T = first_tensor_behind(tb.t, tb.n, a0); T < tb.n; ++T) {
        const int64_t e0 = tb.t[T].elem0, nT = tb.t[T].n;
        if (e0 >= a1) break;
        if (e0 < s0 || nT <= 0 || (e0 & 7)) continue;  // not a tensor of this span
        const int64_t cs = e0 >= a0 ? e0 : e0 + (a0 - e0 + CH - 1) / CH * CH;  // T's chunk that starts in this range
        const int64_t te = min(e0 + nT, s1);
        if (cs >= a1 || cs >= te) continue;
        const int64_t slot = R + T;
        if (slot >= tb.n_slots) continue;
        float wd = a.wd, lr = lr_span;
        if (MAP) {
            unsigned id = tb.ids[e0 >> 3];
            if (id >= tb.n_table) id = 0u;
            if (!id) continue;  // not in this optimiser: no byte of the tensor is written
            const float2 h = tb.table[id];
            lr = __fmul_rn(h.x, lr_span);
            wd = h.y;
        }
        if (APPLY) lr = __fmul_rn(lr, tb.ratios[T]);  // (a ratio of 1 leaves lr's bits)
        const int len = (int)(min(cs + CH, te) - cs), q = len >> 2;
        const int64_t off = cs - s0;
        float* P = a.p + off;
        float* M = a.m + off;
        float* V = a.v + off;
        f4 p[2], g[2], m[2], v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = tid + u * NT;
            if (j < q) {
                p[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(P) + j);
                m[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(M) + j);
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(V) + j);
                if (!APPLY) {
                    if (GB16) {
                        const s4 gb = __builtin_nontemporal_load(reinterpret_cast<const s4*>(reinterpret_cast<const bf16*>(a.g) + off) + j);
#pragma unroll
                        for (int k = 0; k < 4; ++k) g[u][k] = __bfloat162float(__builtin_bit_cast(bf16, (short)gb[k]));
                    } else {
                        g[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(reinterpret_cast<const float*>(a.g) + off) + j);
                    }
                }
            }
        }
        double sp2 = 0.0, su2 = 0.0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = tid + u * NT;
            if (j < q) {
                if (APPLY) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) p[u][k] = __fmaf_rn(-lr, lamb_u(m[u][k], v[u][k], p[u][k], a.eps, wd), p[u][k]);
                    __builtin_nontemporal_store(p[u], reinterpret_cast<f4*>(P) + j);
                    if (a.shadow) {
                        s4 sh;
#pragma unroll
                        for (int k = 0; k < 4; ++k) sh[k] = __builtin_bit_cast(short, __float2bfloat16(p[u][k]));
                        reinterpret_cast<s4*>(a.shadow + off)[j] = sh;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float mk = m[u][k], vk = v[u][k];
                        lamb_moments(mk, vk, __fmul_rn(g[u][k], coef), a.b1, a.b2);
                        const double pd = (double)p[u][k], ud = (double)lamb_u(mk, vk, p[u][k], a.eps, wd);
                        sp2 += pd * pd;
                        su2 += ud * ud;
                        m[u][k] = mk;
                        v[u][k] = vk;
                    }
                    __builtin_nontemporal_store(m[u], reinterpret_cast<f4*>(M) + j);
                    __builtin_nontemporal_store(v[u], reinterpret_cast<f4*>(V) + j);
                }
            }
        }
        if ((len & 3) && tid == (q & (NT - 1))) {  // the n & 3 tail: the thread whose float4 it would have been, behind that
            for (int k = 0; k < (len & 3); ++k) {  // thread's own full float4 (if any): the order of a full chunk
                const int i = 4 * q + k;
                float pk = P[i], mk = M[i], vk = V[i];
                if (APPLY) {
                    pk = __fmaf_rn(-lr, lamb_u(mk, vk, pk, a.eps, wd), pk);
                    P[i] = pk;
                    if (a.shadow) a.shadow[off + i] = __float2bfloat16(pk);
                } else {
                    const float gi = GB16 ? __bfloat162float(reinterpret_cast<const bf16*>(a.g)[off + i])
                                          : reinterpret_cast<const float*>(a.g)[off + i];
                    lamb_moments(mk, vk, __fmul_rn(gi, coef), a.b1, a.b2);
                    const double pd = (double)pk, ud = (double)lamb_u(mk, vk, pk, a.eps, wd);
                    sp2 += pd * pd;
                    su2 += ud * ud;
                    M[i] = mk;
                    V[i] = vk;
                }
            }
        }
        if (!APPLY) {
            block_sum2(sp2, su2);
            if (tid == 0) tb.ws[slot] = double2{sp2, su2};
        }
    }
}

// one workgroup per tensor of the table: a tensor that starts in one of the launch's spans gets its chunks' sums added in
// chunk order (thread t takes chunks t, t + 256, ... in turn, then block_sum2) and its ratio written; any other is left alone
template <bool MAP>
__global__ __launch_bounds__(NT) void lamb_finish_kernel(LambSpans sp, LambTable tb) {
    const int T = blockIdx.x;
    const int64_t e0 = tb.t[T].elem0, nT = tb.t[T].n;
    int64_t s1 = -1;
#pragma unroll
    for (int k = 0; k < LAMB_MULTI; ++k)
        if (k < sp.n && e0 >= sp.a[k].elem0 && e0 < sp.a[k].elem0 + sp.a[k].n) s1 = sp.a[k].elem0 + sp.a[k].n;
    if (s1 < 0 || nT <= 0 || (e0 & 7)) return;
    bool adapted = tb.t[T].adapted != 0;
    if (MAP) {
        const unsigned id = tb.ids[e0 >> 3];
        if (id == 0u || id >= tb.n_table) adapted = false;  // not in this optimiser: phase A left no sums
    }
    const int64_t base = e0 / CH + T, nch = (min(e0 + nT, s1) - e0 + CH - 1) / CH;
    double x = 0.0, y = 0.0;
    if (adapted && base + nch <= tb.n_slots) {
        for (int64_t c = threadIdx.x; c < nch; c += NT) {
            const double2 s = tb.ws[base + c];
            x += s.x;
            y += s.y;
        }
    }
    block_sum2(x, y);
    if (threadIdx.x == 0) tb.ratios[T] = (adapted && x > 0.0 && y > 0.0) ? (float)(sqrt(x) / sqrt(y)) : 1.f;
}

template <bool GB16, bool MAP>
void launch_lamb(const LambSpans& sp, const LambTable& tb, int nblk, hipStream_t st) {
    hipLaunchKernelGGL((lamb_kernel<GB16, MAP, false>), dim3(nblk), dim3(NT), 0, st, sp, tb);
    hipLaunchKernelGGL((lamb_finish_kernel<MAP>), dim3(tb.n), dim3(NT), 0, st, sp, tb);
    hipLaunchKernelGGL((lamb_kernel<GB16, MAP, true>), dim3(nblk), dim3(NT), 0, st, sp, tb);
}

}  // namespace

extern "C" size_t xggm_lamb_workspace_bytes(int64_t arena_elems, int n_tensors) {
    if (arena_elems < 0 || n_tensors < 0) return 0;
    return sizeof(double2) * (size_t)(arena_elems / CH + n_tensors + 1);
}

extern "C" int xggm_lamb_multi(const xggm_adam_args* spans, int n, const xggm_lamb_tensor* tensors, int n_tensors,
                               const xggm_hyper_map* map, float* ratios_out, void* ws, size_t ws_bytes, hipStream_t st) {
    const char* who = "xggm_lamb_multi";
    XGGM_REQUIRE(spans && n > 0, "%s: no spans", who);
    XGGM_REQUIRE(tensors && n_tensors > 0 && reinterpret_cast<uintptr_t>(tensors) % 8 == 0,
                 "%s: the tensor table is missing, empty or not 8-byte aligned", who);
    XGGM_REQUIRE(ratios_out && reinterpret_cast<uintptr_t>(ratios_out) % 4 == 0, "%s: ratios_out is missing or misaligned", who);
    XGGM_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0, "%s: the workspace is missing or not 16-byte aligned", who);
    if (map) {
        XGGM_REQUIRE(map->ids && map->table, "%s: the hyper map needs its id map and its {lr, weight_decay} table", who);
        XGGM_REQUIRE(map->n_table >= 1 && map->n_table <= 256, "%s: hyper table of %d entries (1 .. 256: entry 0 + one per param_group)",
                     who, map->n_table);
        XGGM_REQUIRE(map->n_ids > 0 && reinterpret_cast<uintptr_t>(map->table) % 8 == 0, "%s: empty id map or misaligned hyper table", who);
    }
    const bool gb = spans[0].g_bf16 != 0;
    int64_t end = 0, blocks = 0;
    for (int i = 0; i < n; ++i) {
        const xggm_adam_args& x = spans[i];
        XGGM_REQUIRE(x.p && x.g && x.m && x.v && x.n > 0, "%s: span %d: null pointer or no elements", who, i);
        XGGM_REQUIRE((reinterpret_cast<uintptr_t>(x.p) | reinterpret_cast<uintptr_t>(x.m) | reinterpret_cast<uintptr_t>(x.v)) % 16 == 0 &&
                         reinterpret_cast<uintptr_t>(x.g) % (x.g_bf16 ? 8 : 16) == 0,
                     "%s: span %d: pointers must be 16-byte aligned (bf16 gradients: 8)", who, i);
        XGGM_REQUIRE(!x.shadow_bf16 || reinterpret_cast<uintptr_t>(x.shadow_bf16) % 8 == 0, "%s: span %d: shadow misaligned", who, i);
        XGGM_REQUIRE(!x.shadow8, "%s: span %d: the e4m3 weight copy is written by xggm_optim_multi only", who, i);
        XGGM_REQUIRE((x.g_bf16 != 0) == gb, "%s: the spans of one call share the gradient type", who);
        XGGM_REQUIRE(x.elem0 >= end && x.elem0 % 8 == 0, "%s: span %d: elem0 %lld must be a multiple of 8 and not lie in front of the "
                     "end of the span before it (%lld): spans come in arena order and do not overlap", who, i, (long long)x.elem0,
                     (long long)end);
        XGGM_REQUIRE(!map || (x.elem0 + x.n + 7) / 8 <= map->n_ids, "%s: span %d [%lld, %lld) lies outside the id map (%lld ids)", who, i,
                     (long long)x.elem0, (long long)(x.elem0 + x.n), (long long)(map ? map->n_ids : 0));
        end = x.elem0 + x.n;
        blocks += (end - 1) / CH - x.elem0 / CH + 1;
    }
    XGGM_REQUIRE(blocks < (int64_t)1 << 31, "%s: %lld workgroups", who, (long long)blocks);
    XGGM_REQUIRE(ws_bytes >= xggm_lamb_workspace_bytes(end, n_tensors), "%s: workspace of %zu bytes, xggm_lamb_workspace_bytes(%lld, %d) "
                 "= %zu", who, ws_bytes, (long long)end, n_tensors, xggm_lamb_workspace_bytes(end, n_tensors));
    LambTable tb{tensors, n_tensors, map ? map->ids : nullptr, map ? reinterpret_cast<const float2*>(map->table) : nullptr,
                 map ? (unsigned)map->n_table : 0u, reinterpret_cast<double2*>(ws), (int64_t)(ws_bytes / sizeof(double2)), ratios_out};
    for (int i0 = 0; i0 < n; i0 += LAMB_MULTI) {
        LambSpans sp;
        sp.n = std::min(LAMB_MULTI, n - i0);
        int nblk = 0;
        for (int i = 0; i < sp.n; ++i) {
            const xggm_adam_args& x = spans[i0 + i];
            sp.a[i] = LambSpan{x.p, x.g, x.m, x.v, (bf16*)x.shadow_bf16, x.n, x.elem0, x.sqnorm, x.lr_dev, x.lr_scale, x.max_norm, x.lr,
                               x.b1, x.b2, x.eps, x.weight_decay, x.g_scale > 0.f ? x.g_scale : 1.f};
            sp.blk0[i] = nblk;
            nblk += (int)((x.elem0 + x.n - 1) / CH - x.elem0 / CH + 1);
        }
        sp.blk0[sp.n] = nblk;
        if (map) {
            if (gb) launch_lamb<true, true>(sp, tb, nblk, st);
            else launch_lamb<false, true>(sp, tb, nblk, st);
        } else if (gb) {
            launch_lamb<true, false>(sp, tb, nblk, st);
        } else {
            launch_lamb<false, false>(sp, tb, nblk, st);
        }
        if (int e = xggm_check_launch(who)) return e;
    }
    return XGGM_OK;
}
