/* xggm.h -- C ABI of the MI355X-native X-GGM training-step hot path (libxggm_hip.so).
 *
 * The reference (jingjing12110/X-GGM) is pure PyTorch and has no native interface; this
 * header is the boundary SURVEY.md section 8(b) specifies: one extern "C" entry point per
 * fused op and direction.  Each declaration cites the reference call site it replaces
 * (paths relative to /root/reference).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless said otherwise; tensors are row-major and
 *    contiguous except where a stride argument exists.  The caller owns all memory,
 *    including workspaces; nothing here allocates, frees or synchronises -- work is only
 *    enqueued on `stream` (graph-capture safe).
 *  - `_f32` / `_bf16` in a symbol name is the STORAGE type "T" of activations and of the
 *    GEMM operands.  Arithmetic is fp32 (bf16 MFMA accumulates in fp32).  Parameters that
 *    are vectors (biases, LayerNorm gains), parameter gradients, adjacency-shaped tensors
 *    [B,N,N], losses and optimiser state are always fp32.
 *  - Return value: 0 = ok; non-zero = error, message via xggm_last_error() (thread-local).
 *    Reentrant and thread-safe: called from the host thread in forward and from the
 *    autograd thread in backward.  All launch state travels in the arguments, the tile of a
 *    grouped GEMM launch included (argument `tile`).  The only process-wide state are the A/B
 *    hooks xggm_gemm_set_tile, xggm_gemm_set_group_tile, xggm_gemm_set_generic,
 *    xggm_attn_set_scalar and the instrumented build's stamp / ablation hooks: tests, tools and
 *    the bench's A/B variables write them, the product never does.  A GEMM entry point reads
 *    its hooks once per call, so one launch sees one consistent set of values.
 *  - Randomness: `rng` points to two device uint64 {seed, offset}; dropout masks and
 *    Gaussian draws are pure functions of (seed, offset, stream id `sid`, element index), so
 *    backward regenerates the forward mask.  xggm_rng_advance() bumps the offset once per
 *    pass.  p == 0 (or a supplied `randn`) ignores `rng`.
 */
#ifndef XGGM_H
#define XGGM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* xggm_stream_t; /* == hipStream_t */

#define XGGM_VERSION 100

/* activation codes of xggm_gemm_* */
#define XGGM_ACT_NONE 0
#define XGGM_ACT_GELU 1      /* erf-GELU, src/lxrt/modeling.py:116-124 */
#define XGGM_ACT_SIGMOID 2   /* encoder_adj, src/vqa/vqacpv2_model.py:91-94 */
#define XGGM_ACT_TANH 3      /* BertPooler, src/lxrt/modeling.py:614-620 */
#define XGGM_ACT_GELU_GRAD 4 /* C = acc * gelu'(aux): backward of BertIntermediate fused into dgrad */

/* matrix modes of xggm_aggregate_* */
#define XGGM_AGG_PLAIN 0
#define XGGM_AGG_TRANSPOSE 1
#define XGGM_AGG_SYMMETRIZE 2

int xggm_version(void);
const char* xggm_last_error(void);
/* Weight prefetch: up to four byte ranges (each non-null, 16-byte aligned, >= 16 bytes) that the FIRST carrier kernel
 * launched by an xggm_ln_fwd_grouped_* / xggm_ln_bwd_grouped_* / xggm_attn_*_grouped_* call (argument `prefetch`, NULL =
 * none) reads beside its own work and discards: the weights of the Linear products that follow
 * (src/lxrt/modeling.py:344-347, 384-388, 428-445) are then in the Infinity Cache.  Speed only -- no result depends on
 * it.  The scalar attention kernels (fp32 storage, unaligned bf16 operands) read none. */
typedef struct xggm_prefetch { const void* ptr[4]; size_t bytes[4]; int n; } xggm_prefetch;

/* ---- dense products --------------------------------------------------------------------
 * C[z][m][n] = epilogue( alpha * sum_k A(z,m,k) * B(z,k,n) ),
 *   A(z,m,k) = A[z*a_bs + m*a_rs + k*a_ks],  B(z,k,n) = B[z*b_bs + n*b_ns + k*b_ks],
 *   C at C[z*c_bs + m*ldc + n].
 * epilogue: v = alpha*acc + bias[n]; preact (if given) <- v; v = act(v) (GELU_GRAD: v *
 * gelu'(aux)); v += residual; C = accumulate ? C + v : v; C is T, or float when c_f32.
 * colsum (or NULL; bias gradients): fp32 [batch][ceil(M/32)][N] PARTIAL column sums of v -- row r of batch z holds
 * sum over output rows 32r .. 32r+31 of v[z][m][n]; every element is written exactly once by exactly one workgroup,
 * in a fixed summation order (no floating-point atomics anywhere on the path: a pass gives the same bits whatever the
 * scheduling).  The caller adds the partial rows into the gradient with xggm_partial_reduce_batch (K = 1, H = N,
 * nblk = batch * ceil(M/32)).
 * Replaces nn.Linear forward/backward (src/lxrt/modeling.py:345-347, 385, 429, 442, 617;
 * src/module/gcn.py:28; src/vqa/vqacpv2_model.py:63-105) and torch.bmm(x, x^T)
 * (src/module/graph_generative_modeling.py:225). */
int xggm_gemm_f32(const void* A, const void* B, void* C, int M, int N, int K, int64_t a_rs, int64_t a_ks, int64_t b_ns,
                  int64_t b_ks, int64_t ldc, int batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, const float* bias,
                  const void* residual, void* preact, const void* aux, float* colsum, int act, int c_f32, int accumulate,
                  float alpha, xggm_stream_t stream);
int xggm_gemm_bf16(const void* A, const void* B, void* C, int M, int N, int K, int64_t a_rs, int64_t a_ks, int64_t b_ns,
                   int64_t b_ks, int64_t ldc, int batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, const float* bias,
                   const void* residual, void* preact, const void* aux, float* colsum, int act, int c_f32, int accumulate,
                   float alpha, xggm_stream_t stream);
/* Up to 4 independent products in ONE launch (forward of both modalities, dgrad + wgrad of a layer):
 * skinny problems that cannot fill 256 CUs alone share a grid.  `probs` is a HOST array; fields as
 * the arguments of xggm_gemm_*.  Falls back to one launch per problem for shapes the tuned kernel
 * does not take (unaligned strides, fp32).  A dimension that is not a multiple of 8 (2274 answers, 630 edges)
 * stays on the tuned path when the operand's leading stride is padded to a multiple of 8 (whatever the
 * padding holds). */
typedef struct xggm_gemm_problem {
    const void* A;
    const void* B;
    void* C;
    int M, N, K;
    int64_t a_rs, a_ks, b_ns, b_ks, ldc;
    int batch;
    int64_t a_bs, b_bs, c_bs;
    const float* bias;
    const void* residual;
    void* preact;
    const void* aux;
    float* colsum;
    int act, c_f32, accumulate;
    float alpha;
    /* or NULL.  fp32 outputs on the tuned bf16 kernels only: slot [batch][ceil(M/64)][ceil(N/64)] receives the sum of
     * squares of the values this launch STORED in that 64 x 64 block of C (after `accumulate`); every slot is written
     * by one workgroup, so a fixed-order sum of the slots is the squared norm of the weight gradient without another
     * pass over it (nn.utils.clip_grad_norm_, src/vqa/vqacpv2.py:175). */
    float* sqsum;
    /* e4m3 side of the mixed-precision forward (xggm_gemm_grouped_fp8e4m3 reads scale_a / scale_b; every bf16-output
     * kernel honours c8): scale_a, scale_b: device scalars, the reciprocals of the per-tensor quantisation scales of
     * A and B (NULL = 1).  c8 (or NULL): a second copy of the stored result as OCP e4m3 bytes, layout of C, each
     * value multiplied by *c8_qscale (NULL = 1) and saturated to +-448 -- the operand of the NEXT forward product,
     * written by its producer instead of by a quantisation pass; *c8_amax (or NULL) is raised to max |value| (one
     * atomic per workgroup; feeds the delayed scale update, xggm_fp8_scale_update). */
    const float* scale_a;
    const float* scale_b;
    void* c8;
    const float* c8_qscale;
    float* c8_amax;
    /* amax entries may be spread over `amax_slots` floats (a power of two <= 64; 0 reads as 1): workgroup w raises
     * c8_amax[w % amax_slots] and xggm_fp8_scale_update takes the maximum over the slots.  Hundreds of workgroups
     * raising ONE address are same-address device-scope atomics the kernel end waits for (measured: +2 us per LayerNorm
     * launch, +3.9 us per attention launch, 0.25 ms per iteration of the fp8 step). */
    int amax_slots;
} xggm_gemm_problem;
/* `tile` of the three grouped entry points: 0 = the library chooses (cost model, the 8-wave rule, the four-wave
 * 128 x 128 rule); 1: 64 x 64, 2: 128 x 64, 3: 128 x 128, 4: 128 x 128 on 8 waves; 7 / 8 / 9: 128 x 128 / 128 x 64 /
 * 64 x 64 on the role k-loop (four loader + four compute waves; a group with a ragged k-tile takes the four-wave
 * tile of the same shape).  Any other value is an error and nothing is enqueued.  Precedence: a non-zero `tile` wins;
 * otherwise the process-wide hook xggm_gemm_set_group_tile; otherwise the library's choice.  The tile changes speed,
 * never products or column sums; the `sqsum` slots add their squares in a tile-dependent, fixed order. */
int xggm_gemm_grouped_f32(const xggm_gemm_problem* probs, int n, int tile, xggm_stream_t stream);
int xggm_gemm_grouped_bf16(const xggm_gemm_problem* probs, int n, int tile, xggm_stream_t stream);
/* fp8 forward product of the mixed-precision configuration (BASELINE.json configs[4]: "fp8 MFMA path for LXMERT
 * QKV/FFN GEMMs"; the Linear layers of src/lxrt/modeling.py:345-347 (query/key/value), :429 (intermediate),
 * :442 (output) -- the reference itself is fp32 only, `--fp16` is unused):
 *   C[m,n] = act(scale_a * scale_b * sum_k A(m,k) B(n,k) + bias[n]) (+ residual[m,n])
 * A [M, K] and B [N, K] hold OCP e4m3fn bytes (k contiguous; row strides a_rs / b_ns in elements, multiples of
 * 16, like K; 16-byte aligned bases); scale_a / scale_b: device scalars (null = 1), the reciprocals of the
 * per-tensor quantisation scales; fp32 accumulation; bias fp32 or null; C / residual / preact bf16 with row
 * stride ldc (c_f32 != 0: C fp32); act: XGGM_ACT_NONE .. XGGM_ACT_TANH as in xggm_gemm_bf16. */
int xggm_gemm_fp8e4m3(const void* A, const void* B, void* C, int M, int N, int K, int64_t a_rs, int64_t b_ns, int64_t ldc,
                      const float* scale_a, const float* scale_b, const float* bias, const void* residual, void* preact,
                      int act, int c_f32, xggm_stream_t stream);
/* The same product for up to 6 problems in one launch (the language and the vision stream of a layer, the two
 * directions of a cross-attention layer): every problem has e4m3 operands A [M, K] / B [N, K], k contiguous (a_ks =
 * b_ks = 1, strides in elements = bytes, multiples of 16 like K), its own scale_a / scale_b, and the bf16 epilogue of
 * xggm_gemm_grouped_bf16 (bias, GELU + pre-activation, residual, fp32 split-K slabs through batch / c_f32, c8).  Not
 * for the backward: dgrad / wgrad stay bf16.  `tile` as above, except that there is no role k-loop for e4m3 operands:
 * 7 / 8 / 9 are accepted and all run the 64 x 64 tile. */
int xggm_gemm_grouped_fp8e4m3(const xggm_gemm_problem* probs, int n, int tile, xggm_stream_t stream);
/* Delayed per-tensor scaling of the e4m3 operands: one table (amax, history, qscale, dscale = 1 / qscale) whose
 * entries are weight operands and activation sites.  Protocol of the producers (LayerNorm / GELU epilogue /
 * attention output / BertAdam): an entry with qscale <= 0 is uncalibrated -- they quantise with 1 and record every
 * maximum; otherwise they quantise with qscale and record the maximum of the step in amax only when it exceeds half
 * (BertAdam: three quarters) of the representable range 448 / qscale: e4m3 is a floating-point format, so a stale
 * SMALLER maximum costs no precision and only a larger one saturates, and the same-address atomics stay rare.
 * This call, for the n entries the pointers address (amax, qscale, dscale: n floats; hist: n x hist_len):
 *   hist[i][*pos % hist_len] = amax[i]; amax[i] = 0; m = max_j hist[i][j];
 *   m > 0: qscale[i] = 448 / (margin * m)          (range = margin x the largest recent maximum)
 *   m == 0, shrink != 0, history just wrapped: qscale[i] *= 2   (nothing near the range for hist_len calls)
 *   dscale[i] = 1 / qscale[i];   bump != 0: *pos += 1.
 * Activation sites: once per pass, margin 1.25, shrink, bump.  Weight operands: for the parameter groups a pass
 * updates, BEFORE xggm_optim_multi writes their e4m3 copies with the new scale (margin 4/3, no shrink, no bump).
 * Everything is device-resident (graph replay); n <= 1024.  `amax_slots` (power of two <= 64, 0 = 1): entry i's maximum
 * is the largest of amax[i * amax_slots .. + amax_slots - 1] (all cleared). */
int xggm_fp8_scale_update(float* amax, float* hist, float* qscale, float* dscale, int64_t* pos, int n, int hist_len,
                          float margin, int shrink, int bump, int amax_slots, xggm_stream_t stream);
/* y[i] = e4m3fn(clamp(x[i] * *qscale, -448, 448)), round-to-nearest-even; x fp32 / bf16, n % 8 == 0; qscale: device
 * scalar or null (1); amax: device scalar or null, raised to max |x| (atomic; the caller zeroes it): the next
 * step's scale without another pass over x. */
int xggm_quantize_fp8e4m3_f32(const void* x, void* y, int64_t n, const float* qscale, float* amax, xggm_stream_t stream);
int xggm_quantize_fp8e4m3_bf16(const void* x, void* y, int64_t n, const float* qscale, float* amax, xggm_stream_t stream);
/* HOST, A/B hook: tile of the grouped launches whose `tile` argument is 0 (values as that argument; 0: the library
 * chooses).  Process-wide and unordered against launches on other threads: for tests, tools and the bench's
 * XGGM_GROUP_TILE only. */
int xggm_gemm_set_group_tile(int v);
/* HOST: 1 = run bf16 GEMMs on the generic 64x64 kernel, 0 = tuned kernels (default); A/B tests */
int xggm_gemm_set_generic(int on);
/* HOST: pin the tuned bf16 kernel variant of single launches (1: 64x64 depth 2, 2: 64x64 depth 4,
 * 3: 128x64 depth 2, 5: 128x128 depth 2, 6/7/8: 64x64 / 128x64 / 128x128 depth 1; 0: heuristic;
 * | 0x100 turns the XCD-aware tile order off) */
int xggm_gemm_set_tile(int variant);
/* out[n] += sum_m x[m*ld + n]  (bias gradients; `out` must hold the running value) */
int xggm_colsum_f32(const void* x, float* out, int M, int N, int64_t ld, float* ws, size_t ws_bytes,
                    xggm_stream_t stream);
int xggm_colsum_bf16(const void* x, float* out, int M, int N, int64_t ld, float* ws, size_t ws_bytes,
                     xggm_stream_t stream);
size_t xggm_colsum_workspace_bytes(int M, int N);

/* ---- attention core: src/lxrt/modeling.py:355-373 (BertAttention.forward after the
 * projections).  q/k/v/out rows of sample b start at row b*S of a matrix with the given row
 * stride (so fused-QKV buffers are addressed in place); head h occupies columns
 * [64h, 64h+64).  mask: additive [B,Sk] fp32 or NULL.  Sq, Sk <= 64 through these four entry points (the grouped ones
 * below take up to 128), head_dim == 64.
 * backward: dbq/dbk/dbv (NULL ok; dbk and dbv go together): fp32 [B][heads*64] PARTIAL rows with batch stride db_bs
 * elements -- row b receives the column sums of dq/dk/dv over sample b's rows, each element written once by the
 * (sample, head) workgroup that owns it, in a fixed order.  Summed over b into the query/key/value bias gradients by
 * xggm_partial_reduce_batch (ws = dbq laid out [B][3][H]: K = 3, nblk = B) -- no floating-point atomics. */
int xggm_attn_fwd_f32(const void* q, const void* k, const void* v, const float* mask, void* out, int B, int heads, int Sq,
                      int Sk, int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, float scale, float p,
                      const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_attn_fwd_bf16(const void* q, const void* k, const void* v, const float* mask, void* out, int B, int heads, int Sq,
                       int Sk, int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t o_rs, float scale, float p,
                       const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_attn_bwd_f32(const void* q, const void* k, const void* v, const float* mask, const void* d_out, void* dq, void* dk,
                      void* dv, int B, int heads, int Sq, int Sk, int head_dim, int64_t q_rs, int64_t k_rs, int64_t v_rs,
                      int64_t o_rs, int64_t dq_rs, int64_t dk_rs, int64_t dv_rs, float scale, float p, const uint64_t* rng,
                      uint32_t sid, float* dbq, float* dbk, float* dbv, int64_t db_bs, xggm_stream_t stream);
int xggm_attn_bwd_bf16(const void* q, const void* k, const void* v, const float* mask, const void* d_out, void* dq,
                       void* dk, void* dv, int B, int heads, int Sq, int Sk, int head_dim, int64_t q_rs, int64_t k_rs,
                       int64_t v_rs, int64_t o_rs, int64_t dq_rs, int64_t dk_rs, int64_t dv_rs, float scale, float p,
                       const uint64_t* rng, uint32_t sid, float* dbq, float* dbk, float* dbv, int64_t db_bs,
                       xggm_stream_t stream);

/* Grouped form: independent attention problems (the language and the vision stream of a layer, or
 * the two directions of a cross-attention layer, src/lxrt/modeling.py:485-516) in one launch; two
 * problems share a grid, more are launched in consecutive pairs.  Fields as the arguments above;
 * the backward fields are ignored by the forward entry points.
 * Limits: 1 <= Sq, Sk <= 128.  A problem with Sq > 64 or Sk > 64 ("long": attention_long.hip) is a launch of its own and
 * ignores the prefetch ranges; the problems of at most 64 x 64 around it are paired, and the first pair carries the ranges,
 * as if it were not there, so a group may mix both.  out8 (the e4m3 copy) is refused for a long problem.  Every problem of
 * the group is checked before the first launch: a call that returns XGGM_ERR_ARG has launched nothing.  Same arithmetic
 * contracts on both sides of 64: fixed summation order (no floating-point atomics), the dropout decision of probability
 * (i, j) a function of element ((b * heads + h) * Sq + i) * Sk + j, a two-pass softmax over the whole row, fp32 arithmetic
 * for fp32 storage and for bf16 storage whose pointers are not 16-byte aligned or whose strides are not multiples of 8. */
typedef struct xggm_attn_problem {
    const void* q;
    const void* k;
    const void* v;
    const float* mask;
    void* out;
    int B, heads, Sq, Sk;
    int64_t q_rs, k_rs, v_rs, o_rs;
    float scale, p;
    uint32_t sid;
    const void* d_out;
    void* dq;
    void* dk;
    void* dv;
    int64_t dq_rs, dk_rs, dv_rs;
    float* dbq;
    float* dbk;
    float* dbv;
    int64_t db_bs; /* batch stride (floats) of the dbq / dbk / dbv partial rows, see above */
    /* forward, bf16 storage only: out8 (or NULL) = e4m3 copy of `out` scaled by *qscale (NULL = 1), rows of o_rs
     * bytes -- the A operand of the fp8 output projection; *amax (or NULL) raised to max |out| */
    void* out8;
    const float* qscale;
    float* amax;
    int amax_slots; /* see xggm_gemm_problem.amax_slots */
} xggm_attn_problem;
int xggm_attn_fwd_grouped_f32(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,
                              const xggm_prefetch* prefetch, xggm_stream_t stream);
int xggm_attn_fwd_grouped_bf16(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,
                               const xggm_prefetch* prefetch, xggm_stream_t stream);
int xggm_attn_bwd_grouped_f32(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,
                              const xggm_prefetch* prefetch, xggm_stream_t stream);
int xggm_attn_bwd_grouped_bf16(const xggm_attn_problem* probs, int n, int head_dim, const uint64_t* rng,
                               const xggm_prefetch* prefetch, xggm_stream_t stream);

/* HOST: 1 = run bf16 attention on the scalar kernels (A/B tests), 0 = matrix-core kernels */
int xggm_attn_set_scalar(int on);

/* ---- row kernels -----------------------------------------------------------------------
 * out = [out +] out_scale * drop_post( LN( drop_pre(in + bias) + residual ; gamma, beta, eps) )
 * in/residual/out/z_out: T [M,H]; z_out (may alias `in`) receives the LN input, stats [M,2]
 * = {mean, rstd}.  BertAttOutput/BertOutput: src/lxrt/modeling.py:384-388, 441-445; GCNConv
 * LN: src/module/gcn.py:29; GNN read-outs with dropout(.5) and sum: src/module/gcn.py:70-77;
 * head tails: src/vqa/vqacpv2_model.py:63-105.  H % 4 == 0, H <= 2048. */
int xggm_ln_fwd_f32(const void* in, const float* bias, const void* residual, const float* gamma, const float* beta,
                    void* out, void* z_out, float* stats, int M, int H, float eps, float p_pre, float p_post,
                    const uint64_t* rng, uint32_t sid_pre, uint32_t sid_post, int accumulate, float out_scale,
                    xggm_stream_t stream);
int xggm_ln_fwd_bf16(const void* in, const float* bias, const void* residual, const float* gamma, const float* beta,
                     void* out, void* z_out, float* stats, int M, int H, float eps, float p_pre, float p_post,
                     const uint64_t* rng, uint32_t sid_pre, uint32_t sid_post, int accumulate, float out_scale,
                     xggm_stream_t stream);
/* dy = grad of `out`.  d_in: grad of `in` (NULL ok); d_res: grad of `residual` (NULL ok,
 * accumulate_dres adds to it); dgamma/dbeta/dbias (NULL ok) are ACCUMULATED (+=).
 * gelu_aux (T [M,H], NULL ok): `in` was gelu(u) of a Linear -> d_in (and dbias) are further
 * multiplied by gelu'(u), i.e. they become the gradients of u and of that Linear's bias. */
int xggm_ln_bwd_f32(const void* dy, const void* z, const float* stats, const float* gamma, void* d_in, void* d_res,
                    float* dgamma, float* dbeta, float* dbias, int M, int H, float p_pre, float p_post, const uint64_t* rng,
                    uint32_t sid_pre, uint32_t sid_post, float out_scale, int accumulate_dres, const void* gelu_aux,
                    float* ws, size_t ws_bytes, xggm_stream_t stream);
int xggm_ln_bwd_bf16(const void* dy, const void* z, const float* stats, const float* gamma, void* d_in, void* d_res,
                     float* dgamma, float* dbeta, float* dbias, int M, int H, float p_pre, float p_post,
                     const uint64_t* rng, uint32_t sid_pre, uint32_t sid_post, float out_scale, int accumulate_dres,
                     const void* gelu_aux, float* ws, size_t ws_bytes, xggm_stream_t stream);
/* Grouped forms: up to 4 independent row sets with the same H, eps, dropout rates and scaling (the
 * language and the vision stream of one LXMERT layer, src/lxrt/modeling.py:494-516) in ONE launch;
 * more than 4 problems are launched in consecutive groups.  Fields as the arguments above. */
typedef struct xggm_ln_fwd_problem {
    const void* in;
    const float* bias;
    const void* residual;
    const float* gamma;
    const float* beta;
    void* out;
    void* z_out;
    float* stats;
    int M;
    uint32_t sid_pre, sid_post;
    /* in_slabs > 0: `in` is fp32 and holds in_slabs partial sums [in_slabs][M][H] (split-K products of a long-K
     * GEMM, xggm_gemm_* with batch = in_slabs, c_f32 = 1): the row kernel adds them in order on the way in, so
     * the GEMM gets in_slabs times the workgroups and no reduction pass exists.  0: `in` is T [M][H]. */
    int in_slabs;
    /* out8 (or NULL; bf16 storage only): e4m3 copy of `out` scaled by *qscale (NULL = 1), [M][H] bytes -- the A operand
     * of the following fp8 product (QKV / FFN input); *amax (or NULL) is raised to max |out| (one atomic per workgroup). */
    void* out8;
    const float* qscale;
    float* amax;
    int amax_slots; /* see xggm_gemm_problem.amax_slots */
} xggm_ln_fwd_problem;
typedef struct xggm_ln_bwd_problem {
    const void* dy;
    const void* z;
    const float* stats;
    const float* gamma;
    void* d_in;
    void* d_res;
    float* dgamma; /* all three NULL: sums stay in ws for xggm_partial_reduce_batch */
    float* dbeta;
    float* dbias;
    const void* gelu_aux;
    float* ws;
    size_t ws_bytes;
    int M;
    uint32_t sid_pre, sid_post;
    int accumulate_dres;
} xggm_ln_bwd_problem;
int xggm_ln_fwd_grouped_f32(const xggm_ln_fwd_problem* probs, int n, int H, float eps, float p_pre, float p_post,
                            const uint64_t* rng, int accumulate, float out_scale, const xggm_prefetch* prefetch,
                            xggm_stream_t stream);
int xggm_ln_fwd_grouped_bf16(const xggm_ln_fwd_problem* probs, int n, int H, float eps, float p_pre, float p_post,
                             const uint64_t* rng, int accumulate, float out_scale, const xggm_prefetch* prefetch,
                             xggm_stream_t stream);
int xggm_ln_bwd_grouped_f32(const xggm_ln_bwd_problem* probs, int n, int H, float p_pre, float p_post,
                            const uint64_t* rng, float out_scale, const xggm_prefetch* prefetch, xggm_stream_t stream);
int xggm_ln_bwd_grouped_bf16(const xggm_ln_bwd_problem* probs, int n, int H, float p_pre, float p_post,
                             const uint64_t* rng, float out_scale, const xggm_prefetch* prefetch, xggm_stream_t stream);
/* out = sum over n <= 4 terms of dropout_p_post(LayerNorm(in[k]; gamma[k], beta[k], eps)) in ONE launch: the
 * jump-knowledge read-out of the graph blocks (src/module/gcn.py:70-77, src/module/gin.py:80-87).  The sum is held in
 * fp32 and rounded once.  stats[k] (or NULL): [M][2] (mean, rstd) of term k for xggm_ln_bwd_* (whose `z` is in[k] itself:
 * the terms have no bias, residual or input dropout).  `out` may not alias a term. */
typedef struct xggm_ln_sum_args {
    const void* in[4];
    const float* gamma[4];
    const float* beta[4];
    float* stats[4];
    uint32_t sid_post[4];
    void* out;
    int n, M, H;
    float eps, p_post;
    const uint64_t* rng;
} xggm_ln_sum_args;
int xggm_ln_sum_fwd_f32(const xggm_ln_sum_args* args, xggm_stream_t stream);
int xggm_ln_sum_fwd_bf16(const xggm_ln_sum_args* args, xggm_stream_t stream);
/* workspaces (bytes) of the backward row kernels: they hold one partial row per workgroup and
 * reduced vector, summed by a second kernel instead of contended atomics */
size_t xggm_ln_bwd_workspace_bytes(int M, int H);
size_t xggm_visn_embed_bwd_workspace_bytes(int M, int H);
/* Deferred second stage.  xggm_ln_bwd called with dgamma = dbeta = dbias = NULL only fills its
 * workspace ws[nblk][3][H] (nblk = workspace_bytes / (12 H)); the sums of many such workspaces
 * are then added to their gradients by ONE launch at the end of the backward pass instead of one
 * tiny launch per LayerNorm (58 per pass in LXMERT 9/5/5).  target[k] += sum_b ws[b][k][:]. */
typedef struct xggm_reduce_job {
    const float* ws;
    int nblk, K, H; /* K <= 3 partial vectors of H floats per workgroup */
    float* target[3]; /* NULL = vector not wanted */
} xggm_reduce_job;
int xggm_partial_reduce_batch(const xggm_reduce_job* jobs, int n, xggm_stream_t stream);
/* BertEmbeddings: src/lxrt/modeling.py:298-313.  ids/seg: int64 [M] (M = B*Tlen), tables T.
 * forward: out8 (or NULL; bf16 storage only) = e4m3 copy of `out` scaled by *qscale, *amax raised to max |out|
 * (amax_slots as in xggm_gemm_problem): the operand of the first fp8 product, written by its producer.
 * backward: the table gradients are GATHERED by an owner per table row (the first batch row that looked it up adds
 * the dz rows of every look-up in row order): no atomics, a fixed summation order; row 0 (padding_idx) gets none. */
int xggm_embed_fwd_f32(const int64_t* ids, const int64_t* seg, const void* word, const void* pos, const void* type,
                       const float* gamma, const float* beta, void* out, void* z_out, float* stats, int M, int Tlen, int H,
                       float eps, float p, const uint64_t* rng, uint32_t sid, void* out8, const float* qscale, float* amax,
                       int amax_slots, xggm_stream_t stream);
int xggm_embed_fwd_bf16(const int64_t* ids, const int64_t* seg, const void* word, const void* pos, const void* type,
                        const float* gamma, const float* beta, void* out, void* z_out, float* stats, int M, int Tlen, int H,
                        float eps, float p, const uint64_t* rng, uint32_t sid, void* out8, const float* qscale, float* amax,
                        int amax_slots, xggm_stream_t stream);
/* xggm_embed_fwd_* with up to XGGM_SIDE_MAX pieces of a pass's input glue done by workgroups appended to its grid instead
 * of launches of their own: XGGM_SIDE_ADDITIVE_MASK dst[i] (fp32) = (1 - src[i] (int64)) * -10000 (xggm_additive_mask,
 * src/lxrt/modeling.py:919-928); XGGM_SIDE_CAST_BF16 dst[i] (bf16) = src[i] (fp32) (xggm_cast_f32_to_bf16: the visual
 * features / boxes, src/lxrt/modeling.py:546-550).  The embedding kernel itself reads none of the outputs. */
#define XGGM_SIDE_MAX 3
#define XGGM_SIDE_ADDITIVE_MASK 1
#define XGGM_SIDE_CAST_BF16 2
typedef struct xggm_side_jobs {
    int n;
    struct {
        int kind;
        const void* src;
        void* dst;
        int64_t count;
    } job[XGGM_SIDE_MAX];
} xggm_side_jobs;
int xggm_embed_fwd_side_f32(const int64_t* ids, const int64_t* seg, const void* word, const void* pos, const void* type,
                            const float* gamma, const float* beta, void* out, void* z_out, float* stats, int M, int Tlen, int H,
                            float eps, float p, const uint64_t* rng, uint32_t sid, void* out8, const float* qscale, float* amax,
                            int amax_slots, const xggm_side_jobs* side, xggm_stream_t stream);
int xggm_embed_fwd_side_bf16(const int64_t* ids, const int64_t* seg, const void* word, const void* pos, const void* type,
                             const float* gamma, const float* beta, void* out, void* z_out, float* stats, int M, int Tlen, int H,
                             float eps, float p, const uint64_t* rng, uint32_t sid, void* out8, const float* qscale, float* amax,
                             int amax_slots, const xggm_side_jobs* side, xggm_stream_t stream);
int xggm_embed_bwd_f32(const int64_t* ids, const int64_t* seg, const void* dy, const void* z, const float* stats,
                       const float* gamma, void* dz_ws, float* dword, float* dpos, float* dtype, float* dgamma,
                       float* dbeta, int M, int Tlen, int H, float p, const uint64_t* rng, uint32_t sid, float* ws,
                       size_t ws_bytes, xggm_stream_t stream);
int xggm_embed_bwd_bf16(const int64_t* ids, const int64_t* seg, const void* dy, const void* z, const float* stats,
                        const float* gamma, void* dz_ws, float* dword, float* dpos, float* dtype, float* dgamma,
                        float* dbeta, int M, int Tlen, int H, float p, const uint64_t* rng, uint32_t sid, float* ws,
                        size_t ws_bytes, xggm_stream_t stream);
/* xggm_embed_bwd_* that also LISTS what it did to the word table's gradient (M <= the capacity of the three buffers):
 * row_ids[r] = ids[r]; row_sq[r] = |dword[ids[r]]|^2 after the add where batch row r is the owner of that table row, 0
 * elsewhere (so sum(row_sq[0 .. M)) is the table's contribution to clip_grad_norm_ when the table was zero before);
 * *row_n = M.  A caller that keeps the invariant "every non-zero row of dword is listed" clears the table with
 * xggm_zero_ranges_rows_f32 and never reads its 94 MB for the norm. */
int xggm_embed_bwd_listed_f32(const int64_t* ids, const int64_t* seg, const void* dy, const void* z, const float* stats,
                              const float* gamma, void* dz_ws, float* dword, float* dpos, float* dtype, float* dgamma,
                              float* dbeta, int M, int Tlen, int H, float p, const uint64_t* rng, uint32_t sid, float* ws,
                              size_t ws_bytes, int64_t* row_ids, float* row_sq, int* row_n, xggm_stream_t stream);
int xggm_embed_bwd_listed_bf16(const int64_t* ids, const int64_t* seg, const void* dy, const void* z, const float* stats,
                               const float* gamma, void* dz_ws, float* dword, float* dpos, float* dtype, float* dgamma,
                               float* dbeta, int M, int Tlen, int H, float p, const uint64_t* rng, uint32_t sid, float* ws,
                               size_t ws_bytes, int64_t* row_ids, float* row_sq, int* row_n, xggm_stream_t stream);
/* VisualFeatEncoder tail: src/lxrt/modeling.py:546-556.  u = feat @ W_f^T (T, from
 * xggm_gemm); boxes T [M,4]; W_b fp32 [H,4].  z1 may alias u.  stats [M,4]. */
int xggm_visn_embed_fwd_f32(const void* u, const float* bf, const void* boxes, const float* Wb, const float* bb,
                            const float* g1, const float* b1, const float* g2, const float* b2, void* out, void* z1,
                            void* z2, float* stats, int M, int H, float eps, float p, const uint64_t* rng, uint32_t sid,
                            void* out8, const float* qscale, float* amax, int amax_slots, xggm_stream_t stream);
int xggm_visn_embed_fwd_bf16(const void* u, const float* bf, const void* boxes, const float* Wb, const float* bb,
                             const float* g1, const float* b1, const float* g2, const float* b2, void* out, void* z1,
                             void* z2, float* stats, int M, int H, float eps, float p, const uint64_t* rng, uint32_t sid,
                             void* out8, const float* qscale, float* amax, int amax_slots, xggm_stream_t stream);
int xggm_visn_embed_bwd_f32(const void* dy, const void* z1, const void* z2, const float* stats, const void* boxes,
                            const float* g1, const float* g2, void* du, float* dbf, float* dg1, float* db1, float* dWb,
                            float* dbb, float* dg2, float* db2, int M, int H, float p, const uint64_t* rng, uint32_t sid,
                            float* ws, size_t ws_bytes, xggm_stream_t stream);
int xggm_visn_embed_bwd_bf16(const void* dy, const void* z1, const void* z2, const float* stats, const void* boxes,
                             const float* g1, const float* g2, void* du, float* dbf, float* dg1, float* db1, float* dWb,
                             float* dbb, float* dg2, float* db2, int M, int H, float p, const uint64_t* rng, uint32_t sid,
                             float* ws, size_t ws_bytes, xggm_stream_t stream);

/* ---- graph-generative kernels (adjacency tensors fp32 [B,N,N], N <= 64) -----------------
 * out = [out +] self_w * x + scale * (1 + *scale_ptr) * M' @ x; x/out T [B,N,H].
 * GCNConv aggregate src/module/gcn.py:28; GIN src/module/gin.py:32. */
int xggm_aggregate_f32(const float* M, const void* x, void* out, int B, int N, int H, int mode, float scale,
                       const float* scale_ptr, float self_w, int accumulate, xggm_stream_t stream);
int xggm_aggregate_bf16(const float* M, const void* x, void* out, int B, int N, int H, int mode, float scale,
                        const float* scale_ptr, float self_w, int accumulate, xggm_stream_t stream);
/* GCNConv's tail in one launch (bf16 storage): out = LayerNorm(res + M @ y; gamma, beta, eps) per sample, y = x W^T
 * taken first by a plain product -- LN(x + W (A x)) = LN(x + A (x W^T)), src/module/gcn.py:22-29.  y, res, out, z_out:
 * bf16 [B, N, H], H in {64, 128, 256, 768}; z_out (or NULL) = the rounded pre-normalisation rows and stats (or NULL) =
 * [B*N][2] (mean, rstd), both as xggm_ln_fwd_* leaves them for xggm_ln_bwd_*.  res may be y's own input x; out / z_out
 * may not alias y. */
int xggm_agg_residual_ln_bf16(const float* M, const void* y, const void* res, const float* gamma, const float* beta, void* out,
                              void* z_out, float* stats, int B, int N, int H, float eps, xggm_stream_t stream);
/* *out += sum_{b,i,c} dh[b,i,c] * (M @ x)[b,i,c]   (gradient of GIN's eps); ws: see XGGM_SUM_WS_FLOATS */
int xggm_agg_dot_f32(const float* M, const void* x, const void* dh, float* out, int B, int N, int H, float* ws,
                     xggm_stream_t stream);
int xggm_agg_dot_bf16(const float* M, const void* x, const void* dh, float* out, int B, int N, int H, float* ws,
                      xggm_stream_t stream);
/* adjacency regeneration from S = x x^T: src/module/graph_generative_modeling.py:225-228.
 * adj[i][j] = sigmoid(S[i][j] / max_r S[r][i]), zero diagonal; colmax/argmax [B,N] saved
 * (argmax = first index of the column maximum, as torch.max). */
int xggm_adj_regen_fwd(const float* S, float* adj, float* colmax, int32_t* argmax, int B, int N, xggm_stream_t stream);
int xggm_adj_regen_bwd(const float* d_adj, const float* S, const float* adj, const float* colmax, const int32_t* argmax,
                       float* dS, int B, int N, xggm_stream_t stream);
/* adjacency initialisation: src/vqa/vqacpv2.py:195-202 + src/module/graph_utils.py:162-168.
 * e fp32 [B, N(N-1)/2] (NULL = zeros); entry k goes to (i,j), the k-th element of the strict
 * upper triangle in row-major order, and to (j,i).  Noise: sigma * randn[b,min,max] mirrored
 * (randn fp32 [B,N,N] or NULL = Philox draw); gradlog = -noise / sigma^2 (NULL ok). */
int xggm_adj_init_fwd(const float* e, const float* randn, float* adj, float* gradlog, int B, int N, float sigma,
                      const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_adj_init_bwd(const float* d_adj, float* d_e, int B, int N, xggm_stream_t stream);
/* HOST helper: the (i,j) of entry k (bit-exactness tests of the index map) */
int xggm_triu_index(int k, int N, int* i_out, int* j_out);
/* add_feature_noise_v2: src/module/graph_utils.py:144-149; gradlog fp32 */
int xggm_feature_noise_f32(const void* x, const float* randn, void* out, float* gradlog, int64_t n, float sigma,
                           const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_feature_noise_bf16(const void* x, const float* randn, void* out, float* gradlog, int64_t n, float sigma,
                            const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
/* out[B,2H] = [x, tanh(mean_n nodes)]: src/vqa/vqacpv2.py:216-218 */
int xggm_pool_concat_fwd_f32(const void* x, const void* nodes, void* out, int B, int N, int H, xggm_stream_t stream);
int xggm_pool_concat_fwd_bf16(const void* x, const void* nodes, void* out, int B, int N, int H, xggm_stream_t stream);
int xggm_pool_concat_bwd_f32(const void* d_out, const void* out, void* dx, void* dnodes, int B, int N, int H,
                             int accumulate_dx, xggm_stream_t stream);
int xggm_pool_concat_bwd_bf16(const void* d_out, const void* out, void* dx, void* dnodes, int B, int N, int H,
                              int accumulate_dx, xggm_stream_t stream);
/* x.unsqueeze(1).repeat(1,N,1) and its backward: src/vqa/vqacpv2.py:228 */
int xggm_bcast_rows_f32(const void* x, void* out, int B, int N, int H, xggm_stream_t stream);
int xggm_bcast_rows_bf16(const void* x, void* out, int B, int N, int H, xggm_stream_t stream);
int xggm_sum_rows_f32(const void* g, void* out, int B, int N, int H, xggm_stream_t stream);
int xggm_sum_rows_bf16(const void* g, void* out, int B, int N, int H, xggm_stream_t stream);

/* ---- graph attention (GATConv, src/module/gat.py:25-49) ---------------------------------------
 * s fp32 [B*N,2] = h [a1 a2] (from xggm_gemm, c_f32); att[i][j] = softmax_j(adj_ij == 0 ? -9e15 :
 * LeakyReLU_alpha(s1_i + s2_j)).  backward: ds (T [B*N,2]) from d_att. */
int xggm_gat_att_fwd(const float* s, const float* adj, float* att, int B, int N, float alpha, xggm_stream_t stream);
int xggm_gat_att_bwd_f32(const float* d_att, const float* att, const float* s, const float* adj, void* ds, int B, int N,
                         float alpha, xggm_stream_t stream);
int xggm_gat_att_bwd_bf16(const float* d_att, const float* att, const float* s, const float* adj, void* ds, int B, int N,
                          float alpha, xggm_stream_t stream);
/* out[m*ld_out + c] = elu(x[m*D + c]) (head concat = column slice), and its backward from y */
int xggm_elu_fwd_f32(const void* x, void* out, int M, int D, int64_t ld_out, xggm_stream_t stream);
int xggm_elu_fwd_bf16(const void* x, void* out, int M, int D, int64_t ld_out, xggm_stream_t stream);
int xggm_elu_bwd_f32(const void* dy, const void* y, void* dx, int M, int D, int64_t ld, xggm_stream_t stream);
int xggm_elu_bwd_bf16(const void* dy, const void* y, void* dx, int M, int D, int64_t ld, xggm_stream_t stream);
/* F.dropout(x, p) with the Philox mask of (rng, sid); applying it to a gradient is its backward */
int xggm_dropout_f32(const void* x, void* out, int64_t n, float p, const uint64_t* rng, uint32_t sid,
                     xggm_stream_t stream);
int xggm_dropout_bf16(const void* x, void* out, int64_t n, float p, const uint64_t* rng, uint32_t sid,
                      xggm_stream_t stream);

/* ---- the graph kernels for 64 < N <= 128 objects (graph_long.hip) -------------------------------
 * Each takes the arguments of its twin above and computes the same thing; N <= 64 and N > 128 are refused on the host
 * before any launch (the twins keep refusing N > 64).  fp32 needs H % 4 == 0, the bf16 matrix-core path H % 8 == 0.
 * GCNConv aggregate src/module/gcn.py:28; GIN src/module/gin.py:32. */
int xggm_aggregate_long_f32(const float* M, const void* x, void* out, int B, int N, int H, int mode, float scale,
                            const float* scale_ptr, float self_w, int accumulate, xggm_stream_t stream);
int xggm_aggregate_long_bf16(const float* M, const void* x, void* out, int B, int N, int H, int mode, float scale,
                             const float* scale_ptr, float self_w, int accumulate, xggm_stream_t stream);
/* *out += sum_{b,i,c} dh[b,i,c] * (M @ x)[b,i,c]   (gradient of GIN's eps); ws: see XGGM_SUM_WS_FLOATS */
int xggm_agg_dot_long_f32(const float* M, const void* x, const void* dh, float* out, int B, int N, int H, float* ws,
                          xggm_stream_t stream);
int xggm_agg_dot_long_bf16(const float* M, const void* x, const void* dh, float* out, int B, int N, int H, float* ws,
                           xggm_stream_t stream);
/* adjacency regeneration from S = x x^T: src/module/graph_generative_modeling.py:225-228 (argmax = first index of the
 * column maximum, as torch.max) */
int xggm_adj_regen_long_fwd(const float* S, float* adj, float* colmax, int32_t* argmax, int B, int N, xggm_stream_t stream);
int xggm_adj_regen_long_bwd(const float* d_adj, const float* S, const float* adj, const float* colmax, const int32_t* argmax,
                            float* dS, int B, int N, xggm_stream_t stream);
/* adjacency initialisation: src/vqa/vqacpv2.py:195-202 + src/module/graph_utils.py:162-168; the enumeration of
 * xggm_triu_index */
int xggm_adj_init_long_fwd(const float* e, const float* randn, float* adj, float* gradlog, int B, int N, float sigma,
                           const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_adj_init_long_bwd(const float* d_adj, float* d_e, int B, int N, xggm_stream_t stream);
/* graph attention (GATConv, src/module/gat.py:25-49) */
int xggm_gat_att_long_fwd(const float* s, const float* adj, float* att, int B, int N, float alpha, xggm_stream_t stream);
int xggm_gat_att_long_bwd_f32(const float* d_att, const float* att, const float* s, const float* adj, void* ds, int B, int N,
                              float alpha, xggm_stream_t stream);
int xggm_gat_att_long_bwd_bf16(const float* d_att, const float* att, const float* s, const float* adj, void* ds, int B, int N,
                               float alpha, xggm_stream_t stream);
/* adj_true of 65..128 objects: data/preprocess/vqa/compute_adjacency.py:38-45 + :90 (see xggm_cosine_adjacency_f32) */
int xggm_cosine_adjacency_long_f32(const float* cls, const float* attr, float* adj, int n_img, int N, int D, float eps,
                                   xggm_stream_t stream);

/* ---- losses (scalars are device fp32; *loss must hold the running value, usually 0) ------
 * Sums over the whole grid are taken WITHOUT floating-point atomics: every workgroup leaves its partial in `ws`, the
 * workgroup that finishes last adds the partials in index order and updates *loss (same bits whatever the
 * scheduling).  `ws`: XGGM_SUM_WS_FLOATS floats of device memory owned by the caller, ws[0] == 0 at launch (the
 * kernels leave it 0, so one zeroed buffer serves every launch of a stream).
 * loss_func: src/vqa/vqacpv2.py:48-51.  *loss += coef * sum (s-g)^2; ds = gout*2*coef*(s-g) */
#define XGGM_SUM_WS_FLOATS 4104
int xggm_dsm_loss_fwd_f32(const void* s, const float* g, float* loss, int64_t n, float coef, float* ws,
                          xggm_stream_t stream);
int xggm_dsm_loss_fwd_bf16(const void* s, const float* g, float* loss, int64_t n, float coef, float* ws,
                           xggm_stream_t stream);
int xggm_dsm_loss_bwd_f32(const void* s, const float* g, const float* gout, void* ds, int64_t n, float coef,
                          xggm_stream_t stream);
int xggm_dsm_loss_bwd_bf16(const void* s, const float* g, const float* gout, void* ds, int64_t n, float coef,
                           xggm_stream_t stream);
/* compute_kl_loss: src/vqa/vqacpv2.py:54-61.  rows x W; *loss += coef * sum_rows f (NULL
 * skips); dx/dy (NULL ok) = [+] *gout * coef * df. */
int xggm_symkl_f32(const void* x, const void* y, float* loss, const float* gout, void* dx, void* dy, int rows, int W,
                   float coef, int accumulate, float* ws, xggm_stream_t stream);
int xggm_symkl_bf16(const void* x, const void* y, float* loss, const float* gout, void* dx, void* dy, int rows, int W,
                    float coef, int accumulate, float* ws, xggm_stream_t stream);
/* nn.BCEWithLogitsLoss()(logit, target) * A: src/vqa/vqacpv2.py:131,173; logits fp32 */
int xggm_bce_fwd(const float* logit, const float* target, float* loss, int64_t n, float coef, float* ws,
                 xggm_stream_t stream);
int xggm_bce_bwd_f32(const float* logit, const float* target, const float* gout, void* dlogit, int64_t n, float coef,
                     xggm_stream_t stream);
int xggm_bce_bwd_bf16(const float* logit, const float* target, const float* gout, void* dlogit, int64_t n, float coef,
                      xggm_stream_t stream);
/* Debias answer losses of the language-prior benchmarks (VQA-CP v2, GQA-OOD): ReweightByInvBias, BiasProduct and
 * LearnedMixin of src/module/vqa_debias_loss_functions.py:84-207 (Plain, :67-71, is xggm_bce_* with coef = 1 / B).
 * z = logits, y = labels, b = bias in [0, 1] (all fp32 [B, A], rows 4-byte aligned are enough), s = constant_smooth
 * (+ sigmoid(*smooth_param) when given), p = log(b + s), q = log(1 - b + s):
 *   LEARNED_MIXIN   g_r = softplus(hidden[r] . lin_w + *lin_b);  d = z + g_r (p - q)
 *                   *loss += mean_r sum_a [softplus(-d) y + softplus(d) (1 - y)] + w * mean_{r,a} H(g_r (p - q)),
 *                   H(e) the entropy of (sigmoid(e), sigmoid(-e)): the penalty of :201-207
 *   BIAS_PRODUCT    the same with g = 1 and no penalty (:113-138)
 *   REWEIGHT        *loss += sum (1 - b) bce_elem(z, y) / sum (1 - b)          (:85-93)
 * (all at the scale of BCEWithLogits(mean) * A).  The results are finite wherever the reference's are: s > 0, or no
 * bias entry at exactly 0 or 1.
 * Row r reads bias + i * bias_row_stride with i = bias_index ? bias_index[r] : r, clamped into [0, bias_rows): with an
 * index the bias is a small [groups, A] prior table and never exists as [B, A].
 * The _f32 / _bf16 suffix names the type of hidden, d_hidden and d_logit (dlogit_f32 != 0: d_logit is fp32 under either
 * suffix -- the answer head keeps fp32 logits); logits, labels, bias and the three parameters (fp32 masters) are fp32.
 * forward: ONE launch; needs loss, ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0 at launch, left 0) and `save`.
 * backward: reads what the forward left in `save`; d_logit = *gout (NULL: 1) * d loss / d z always; LEARNED_MIXIN also
 * d_hidden[r] = dpre_r * lin_w (NULL: not wanted).  Parameter gradients (all NULL: not wanted; d_lin_w and d_lin_b come
 * together) cost a second launch that adds the per-row terms the first left in `part` in row order; accumulate != 0
 * adds them to d_lin_w [Hd], d_lin_b [1], d_smooth [1] instead of overwriting.
 * No floating-point atomics, every sum in a fixed order; no allocation, no host synchronisation: legal inside a stream
 * capture.  Refused before any launch: unknown kind, B or A <= 0, a null logits / labels / bias, LEARNED_MIXIN without
 * hidden / lin_w / lin_b / Hd / save, REWEIGHT without save or with a smooth_param, a bias of fewer than B rows without
 * an index, parameter gradients without `part`. */
#define XGGM_DEBIAS_REWEIGHT 1
#define XGGM_DEBIAS_BIAS_PRODUCT 2
#define XGGM_DEBIAS_LEARNED_MIXIN 3
typedef struct xggm_debias_args {
    const float* logits;       /* [B, A] */
    const float* labels;       /* [B, A] soft scores */
    const float* bias;         /* [bias_rows, >= A] */
    int64_t bias_row_stride;   /* floats between two rows of bias, >= A */
    int64_t bias_rows;         /* rows of bias: B, or the groups of a prior table */
    const int64_t* bias_index; /* [B] row of bias per sample, or NULL */
    const void* hidden;        /* [B, Hd], LEARNED_MIXIN only */
    int Hd;
    const float* lin_w;        /* bias_lin.weight [Hd] */
    const float* lin_b;        /* bias_lin.bias [1] */
    const float* smooth_param; /* [1] or NULL */
    float constant_smooth;
    float w;                   /* weight of the entropy penalty */
    int kind, B, A;
    float* loss;               /* forward: the slot the loss is added to */
    float* save;               /* LEARNED_MIXIN: 2 B floats (pre-activation, g per row); REWEIGHT: 1 float (sum of weights) */
    float* ws;                 /* forward: XGGM_SUM_WS_FLOATS floats */
    const float* gout;         /* backward: upstream gradient, DEVICE scalar, or NULL */
    void* d_logit;             /* backward: [B, A] */
    int dlogit_f32;
    void* d_hidden;            /* backward: [B, Hd] or NULL */
    float* d_lin_w;            /* backward: [Hd] or NULL */
    float* d_lin_b;            /* backward: [1] or NULL */
    float* d_smooth;           /* backward: [1] or NULL */
    float* part;               /* backward: scratch of 2 B floats, needed for parameter gradients */
    int accumulate;
} xggm_debias_args;
int xggm_debias_fwd_f32(const xggm_debias_args* args, xggm_stream_t stream);
int xggm_debias_fwd_bf16(const xggm_debias_args* args, xggm_stream_t stream);
int xggm_debias_bwd_f32(const xggm_debias_args* args, xggm_stream_t stream);
int xggm_debias_bwd_bf16(const xggm_debias_args* args, xggm_stream_t stream);
/* Answer losses with a softmax over the answer axis: Focal of src/module/vqa_debias_loss_functions.py:74-81 and the
 * nn.CrossEntropyLoss(ignore_index=-1) of --mceLoss (src/param.py:78, src/gqa/gqa_ood.py:116).  z = logits, y = labels
 * (fp32 [B, A], rows 4-byte aligned are enough), p = softmax(z) over a row:
 *   FOCAL   c = (1 - softmax(b))^2, b the sample's bias row (bias, bias_row_stride, bias_rows, bias_index as in
 *           xggm_debias_args: row bias_index[r], clamped into [0, bias_rows), of a small prior table);  f = log(p + 1e-5) c
 *           *loss += (1 / B) sum_{r,a} [max(f, 0) - f y + log1p(exp(-|f|))]     (BCEWithLogits(f, y), mean, times A: :79-80)
 *           d_logit[r][j] = u_j - p_j sum_a u_a,  u = *gout (sigmoid(f) - y) / B * c p / (p + 1e-5); bias and labels get none.
 *           `scale`, `ignore_index` and `label_index` are not read.
 *   CE      label_r = label_index[r] when label_index is given, else the FIRST index of the maximum of labels[r]
 *           (torch.max(1)), or ignore_index when that maximum is <= 0 (an answer outside the vocabulary).  Rows whose label
 *           equals ignore_index are ignored; a label_index entry outside [0, A) that is not ignore_index cannot be refused
 *           from the host: the kernel treats that row as ignored too.
 *           *loss += scale * sum_valid (logsumexp(z_r) - z_r[label_r]) / n_valid
 *           d_logit = *gout * scale / n_valid * (p - onehot(label)) on valid rows, exactly 0 on ignored rows.
 *           No valid row: the loss is NaN (0 / 0, torch's mean over nothing) and d_logit all zero.
 * forward: ONE launch of min(B, 128) workgroups; needs loss, ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0 at launch, left 0)
 * and save (5 B + 1 floats: per row max z, log sum exp(z - max), max b, sum exp(b - max b); B int32 labels, -1 = ignored;
 * n_valid).  backward: ONE launch that reads `save`; accumulate != 0 adds to d_logit instead of overwriting.
 * No floating-point atomics, every sum in a fixed order; no allocation, no host synchronisation: legal inside a stream
 * capture.  Refused before any launch: a null struct, unknown kind, B or A <= 0, null logits, CE with neither labels nor
 * label_index, FOCAL without labels or bias, a bias_row_stride < A, a bias of fewer than B rows without bias_index, a
 * missing save; forward without loss or ws; backward without d_logit or gout. */
#define XGGM_SOFTMAX_FOCAL 1
#define XGGM_SOFTMAX_CE 2
typedef struct xggm_softmax_loss_args {
    const float* logits;        /* [B, A] */
    const float* labels;        /* [B, A] soft scores; CE: may be NULL when label_index is given */
    const int64_t* label_index; /* CE: [B] class per sample (takes precedence over labels), or NULL */
    const float* bias;          /* FOCAL: [bias_rows, >= A] */
    int64_t bias_row_stride;    /* floats between two rows of bias, >= A */
    int64_t bias_rows;          /* rows of bias: B, or the groups of a prior table */
    const int64_t* bias_index;  /* [B] row of bias per sample, or NULL */
    int64_t ignore_index;       /* CE: the label of rows that do not count */
    float scale;                /* CE: factor on the mean */
    int kind, B, A;
    float* loss;                /* forward: the slot the loss is added to */
    float* ws;                  /* forward: XGGM_SUM_WS_FLOATS floats */
    float* save;                /* 5 B + 1 floats: written by the forward, read by the backward */
    const float* gout;          /* backward: upstream gradient, DEVICE scalar */
    float* d_logit;             /* backward: [B, A] fp32 */
    int accumulate;
} xggm_softmax_loss_args;
int xggm_softmax_loss_fwd_f32(const xggm_softmax_loss_args* args, xggm_stream_t stream);
int xggm_softmax_loss_bwd_f32(const xggm_softmax_loss_args* args, xggm_stream_t stream);

/* Losses of LXMERT pre-training: LXRTPretraining.forward, src/lxrt/modeling.py:955-1061 (trained by
 * src/pretrain/lxmert_pretrain.py:221-306).  The matched loss (:1017-1023) and the QA loss (:1047-1059) are
 * xggm_softmax_loss_*_f32 with XGGM_SOFTMAX_CE; the masked-LM loss (:1009-1016) and the object losses (:1024-1046) are here.
 *
 * xggm_mlm_select: the rows of x [M, H] (M = B T, the language stream) whose masked_lm_label counts, in ascending row
 * order: row_index[j], label[j] (int32 [cap]) for j < *n, -1 behind; out [cap, H] holds those rows of x and exact zeros in
 * rows [*n, cap), so a product over all cap rows is harmless.  A row counts when its label is not ignore_index AND lies in
 * [0, V): as in XGGM_SOFTMAX_CE, a label outside the vocabulary cannot be refused from the host and the row is ignored.
 * The order comes from a prefix count (integers, no atomics): the same labels give the same list.  The host reads nothing.
 * More than cap rows: *n = cap, the list holds the FIRST cap rows and *overflow = 1 (else 0); xggm_vocab_ce_fwd_* turns
 * that flag into a NaN loss, so a capacity that is too small is never a silent truncation.
 * One launch of ceil(M / 256) workgroups; each counts the labels in front of its chunk itself, so the cost grows with
 * M^2 / 256 label reads: M = B T is a few thousand in pre-training, and M above XGGM_MLM_SELECT_MAX_ROWS is refused.  x and out 16-byte aligned, H * sizeof(element) a multiple of 16.
 * xggm_mlm_scatter_*: the gather's backward -- out [M, H] = row j of src [cap, H] at row row_index[j] (j < *n), exact zeros
 * elsewhere; one launch, every row written once. */
#define XGGM_MLM_SELECT_MAX_ROWS 65536
typedef struct xggm_mlm_select_args {
    const int64_t* labels;  /* [M] masked_lm_labels */
    const void* x;          /* [M, H] */
    int M, H, cap, V;
    int64_t ignore_index;
    int* row_index;         /* [cap] */
    int* label;             /* [cap] */
    int* n;                 /* [1] min(rows that count, cap) */
    int* overflow;          /* [1] 1 when more than cap rows count */
    void* out;              /* [cap, H] */
} xggm_mlm_select_args;
int xggm_mlm_select_f32(const xggm_mlm_select_args* args, xggm_stream_t stream);
int xggm_mlm_select_bf16(const xggm_mlm_select_args* args, xggm_stream_t stream);
int xggm_mlm_scatter_f32(const void* src, const int* row_index, const int* n, void* out, int M, int H, int cap,
                         xggm_stream_t stream);
int xggm_mlm_scatter_bf16(const void* src, const int* row_index, const int* n, void* out, int M, int H, int cap,
                          xggm_stream_t stream);
/* xggm_vocab_ce_*: nn.CrossEntropyLoss(ignore_index=-1) over the vocabulary (src/lxrt/modeling.py:1009-1016) on the
 * compacted rows: logits [cap, ld] in the suffix's type with ld >= V a multiple of 16 bytes (30522 -> 30528) and a 16-byte
 * aligned base; label int32 [cap] and *n as xggm_mlm_select left them (n is clamped into [0, cap]).
 *   forward   *loss += sum_{r < n} (logsumexp(z_r[0:V]) - z_r[label_r]) / n;  save[2 r] = max, save[2 r + 1] = log sum
 *             exp(z - max) of row r < n.  Every row is read once: up to XGGM_VOCAB_CE_REG_MAX columns it stays in the
 *             registers of a 1024-thread workgroup, a longer row is folded online.  *overflow != 0 (NULL: not looked at):
 *             the loss is NaN.  n == 0: the loss is NaN (0 / 0, torch's mean over nothing, the convention of
 *             XGGM_SOFTMAX_CE) and the gradient all zero.
 *   backward  ONE launch that OVERWRITES the logits with *gout (p - onehot(label)) / n in their own type, exact zeros on
 *             rows >= n and in the columns [V, ld).  *overflow != 0: the rows < n get NaN instead -- a truncated list yields
 *             neither a usable loss nor a usable gradient.
 * A label entry outside [0, V) (xggm_mlm_select writes none) adds nothing to the loss and gets a zero row.
 * No floating-point atomics, every sum in a fixed order; no allocation, no host synchronisation.  Refused before any
 * launch: a null struct, cap <= 0, V <= 0, ld < V or not a multiple of 16 bytes, null or misaligned logits, null label / n /
 * save; forward without loss or ws; backward without gout. */
#define XGGM_VOCAB_CE_REG_MAX 32768
#define XGGM_VOCAB_CE_FWD_GRID 1024 /* workgroups of the forward: more rows are walked */
#define XGGM_VOCAB_CE_BWD_GRID 2048 /* workgroups of the backward */
typedef struct xggm_vocab_ce_args {
    void* logits;         /* [cap, ld]; the backward overwrites it with the gradient */
    const int* label;     /* [cap] */
    const int* n;         /* [1] device */
    const int* overflow;  /* [1] device, or NULL */
    int cap, V;
    int64_t ld;           /* elements between two rows */
    float* loss;          /* forward: the slot the loss is added to */
    float* ws;            /* forward: XGGM_SUM_WS_FLOATS floats */
    float* save;          /* 2 cap floats: written by the forward, read by the backward */
    const float* gout;    /* backward: upstream gradient, DEVICE scalar */
} xggm_vocab_ce_args;
int xggm_vocab_ce_fwd_f32(const xggm_vocab_ce_args* args, xggm_stream_t stream);
int xggm_vocab_ce_fwd_bf16(const xggm_vocab_ce_args* args, xggm_stream_t stream);
int xggm_vocab_ce_bwd_f32(const xggm_vocab_ce_args* args, xggm_stream_t stream);
int xggm_vocab_ce_bwd_bf16(const xggm_vocab_ce_args* args, xggm_stream_t stream);
/* xggm_visual_loss_*: the object losses of src/lxrt/modeling.py:1024-1046, up to XGGM_VISUAL_MAX_JOBS of them in one
 * launch over the same R = B * objects rows (--visualLosses may name any subset of obj, attr, feat).  Per job, with
 * c_r = mask_conf[r] (fp32 [R]) and scores [R, W] in the suffix's type:
 *   XGGM_VISUAL_CE  l_r = logsumexp(s_r) - s_r[label_index[r]], 0 where the label is ignore_index (or outside [0, W))
 *   XGGM_VISUAL_L2  l_r = mean_i SmoothL1(s_r[i] - target[r][i]), beta = 1, target fp32 [R, W]
 *   *loss += weight * (1 / R) sum_r l_r c_r          (the mean runs over ALL rows, ignored ones included)
 *   d_score = *gout * weight * c_r / R * (softmax(s_r) - onehot)   or   ... / (R W) * clamp(s - target, -1, 1);
 *   exact zeros on ignored rows and on rows of confidence 0.
 * forward: ONE launch of min(R, 128) workgroups; needs ws (XGGM_SUM_WS_FLOATS floats, ws[0] == 0 at launch, left 0), a loss
 * slot per job and save (2 * XGGM_VISUAL_MAX_JOBS * R floats).  backward: ONE launch, d_score per job in the scores' type.
 * No floating-point atomics, every sum in a fixed order.  Refused before any launch: a null struct, n_jobs outside
 * [1, XGGM_VISUAL_MAX_JOBS], R <= 0, an unknown kind, W <= 0, null scores / mask_conf, CE without label_index, L2 without
 * target, a missing save; forward without ws or a loss slot; backward without gout or d_score. */
#define XGGM_VISUAL_CE 1
#define XGGM_VISUAL_L2 2
#define XGGM_VISUAL_MAX_JOBS 3
#define XGGM_VISUAL_LOSS_GRID 128 /* workgroups of either launch: more rows are walked */
typedef struct xggm_visual_job {
    int kind, W;
    const void* scores;          /* [R, W] */
    const int64_t* label_index;  /* CE: [R] */
    const float* target;         /* L2: [R, W] */
    const float* mask_conf;      /* [R] */
    float weight;
    float* loss;                 /* forward: the slot this job's loss is added to */
    void* d_score;               /* backward: [R, W] */
} xggm_visual_job;
typedef struct xggm_visual_loss_args {
    xggm_visual_job job[XGGM_VISUAL_MAX_JOBS];
    int n_jobs, R;
    int64_t ignore_index;
    float* ws;          /* forward: XGGM_SUM_WS_FLOATS floats */
    float* save;        /* 2 * XGGM_VISUAL_MAX_JOBS * R floats: written by the forward, read by the backward */
    const float* gout;  /* backward: upstream gradient, DEVICE scalar */
} xggm_visual_loss_args;
int xggm_visual_loss_fwd_f32(const xggm_visual_loss_args* args, xggm_stream_t stream);
int xggm_visual_loss_fwd_bf16(const xggm_visual_loss_args* args, xggm_stream_t stream);
int xggm_visual_loss_bwd_f32(const xggm_visual_loss_args* args, xggm_stream_t stream);
int xggm_visual_loss_bwd_bf16(const xggm_visual_loss_args* args, xggm_stream_t stream);

/* xggm_pretrain_corrupt_*: the corruption src/pretrain/lxmert_pretrain.py:76-215 applies to every example on the host --
 * random_word (:76-112), random_feat (:115-136) and the QA answer draw (:186-199) -- for a whole batch that is already on the
 * device, in ONE launch.  The suffix is the type of the features.  The outputs are the arguments of LXRTPretraining.forward
 * (:302-305) that the corruption produces; nothing is changed in place.
 *   object rows  r = (b, o) of feats [B, O, F], draw u = u_obj[r]:
 *                u < obj_mask_rate: feat_mask[r] = 1 and, with p = u / obj_mask_rate,  p < 0.8: masked_feat[r] = 0 (feats
 *                is not read);  p < 0.9: masked_feat[r] = pool[floor(u_obj_pick[r] * P)];  else a copy.
 *                u >= obj_mask_rate: a copy, feat_mask[r] = 0.
 *                pool [P, F] (NULL: the batch's own clean feats as [B O, F]) stands in for the reference's
 *                torchdset.random_feat(), a random object of a random datum of the whole data set (two integer draws there,
 *                one row index here): the one deviation.  Rows move as 16-byte vectors when F * sizeof(element) is a
 *                multiple of 16 and feats / pool / masked_feat are 16-byte aligned, element by element otherwise.
 *   tokens       position (b, t) is eligible iff t >= 1, input_mask[b, t] == 1, t < T - 1 and input_mask[b, t + 1] == 1 (not
 *                [CLS], not the last real token [SEP], not padding: :156-172).  Eligible, draw u = u_word[b, t]:
 *                u < word_mask_rate: masked_lm_labels = the original id and, with p = u / word_mask_rate,  p < 0.8: mask_id;
 *                p < 0.9: floor(u_word_pick[b, t] * vocab_size);  else the id stays.  Every other position keeps its id and
 *                gets the label -1.
 *   answer       label_ids [B, K] (int64, -1 = no key, the keys of example.label in insertion order), label_scores [B, K]:
 *                no key or is_matched[b] != 1: ans[b] = -1; one key: that key; otherwise the first key k with
 *                u_ans[b] * sum < s_0 + ... + s_k (sums left to right over the valid keys), the last valid key as the
 *                fallback.  The reference draws this case with np.random.multinomial(1, s / sum) (:196-199), whose stream
 *                cannot be fed from outside: same distribution, not the same bits.
 * Every comparison, u / rate, u2 * n and the running sums are evaluated in double from the fp32 draw -- the IEEE operations the
 * reference performs on Python floats -- so a decision is the reference's for every fp32 u, the thresholds included.  A
 * supplied pick draw outside [0, 1) is held inside the table.
 * Draws: five buffers, u_word [B, T], u_word_pick [B, T], u_obj [B, O], u_obj_pick [B, O], u_ans [B] (fp32 in [0, 1)).  A NULL
 * buffer number k (0..4 in that order) means philox_uniform(seed, offset, sid_base + k, row-major index) with {seed, offset} =
 * rng[0..1] -- exactly what xggm_uniform(out, n, rng, sid_base + k) exports.  rng is only read: the caller advances it
 * (xggm_rng_advance) once per batch.
 * One launch: min(B O, XGGM_PRETRAIN_CORRUPT_ROW_GRID) workgroups of 256 threads walk the rows, ceil(B T / 256) trailing
 * workgroups take one token per thread, ceil(B / 256) one sample per thread; no result depends on the geometry.  No atomics,
 * no allocation, no host synchronisation.  Refused before any launch: a null struct, B, T, O, F or K <= 0, a null required
 * pointer, rates outside [0, 1], vocab_size <= 0, a NULL draw buffer without rng, masked_feat overlapping feats or pool. */
#define XGGM_PRETRAIN_CORRUPT_ROW_GRID 65536 /* workgroups of the object rows: more rows are walked */
typedef struct xggm_pretrain_corrupt_args {
    const void* feats;             /* [B, O, F] clean features */
    const void* pool;              /* [P, F] or NULL */
    void* masked_feat;             /* [B, O, F] out */
    float* feat_mask;              /* [B, O] out */
    const int64_t* input_ids;      /* [B, T] */
    const int64_t* input_mask;     /* [B, T] */
    int64_t* input_ids_out;        /* [B, T] out */
    int64_t* masked_lm_labels;     /* [B, T] out */
    const int64_t* label_ids;      /* [B, K] */
    const float* label_scores;     /* [B, K] */
    const int64_t* is_matched;     /* [B] */
    int64_t* ans;                  /* [B] out */
    int B, T, O, F, K;
    int64_t P;                     /* rows of pool (ignored when pool is NULL) */
    int64_t vocab_size, mask_id;
    double word_mask_rate, obj_mask_rate;
    const float* u_word;           /* the five draw buffers, each may be NULL */
    const float* u_word_pick;
    const float* u_obj;
    const float* u_obj_pick;
    const float* u_ans;
    const uint64_t* rng;           /* {seed, offset}; needed when a draw buffer is NULL */
    uint32_t sid_base;
} xggm_pretrain_corrupt_args;
int xggm_pretrain_corrupt_f32(const xggm_pretrain_corrupt_args* args, xggm_stream_t stream);
int xggm_pretrain_corrupt_bf16(const xggm_pretrain_corrupt_args* args, xggm_stream_t stream);

/* xggm_pretrain_swap: the matched-sentence swap LXMERTTorchDataset.__getitem__ applies to every example on the host with
 * Python's random (src/pretrain/lxmert_data.py:173-183) -- with probability 0.5 the sentence is replaced by the sentence of
 * a random datum of ANOTHER image and is_matched becomes 0 -- for a whole clean batch that is already on the device, in ONE
 * launch, ahead of xggm_pretrain_corrupt_* (the reference swaps in the data set, then masks: the same order).
 *   ids, mask [B, T] int64: the clean sentences; img [B] int64: an integer key per image; matched_in [B] int64 or NULL (all 1).
 *   pool_ids, pool_mask [P, T], pool_img [P]: the sentences a swap draws from (the reference: every datum of the data set);
 *   all three NULL: the batch's own rows, P = B.
 *   row b:  matched_in[b] != 1:            a copy, is_matched[b] = matched_in[b] (no draw is looked at);
 *           else u_swap[b] < rate false:   a copy, is_matched[b] = 1;
 *           else for r = 0 .. TRIES - 1:   j = min(floor(u_pick[b, r] * P), P - 1); the FIRST j with pool_img[j] != img[b]
 *                                          wins: out row = pool row j (ids and mask), is_matched[b] = 0;
 *           all TRIES candidates show img[b]: a copy, is_matched[b] = 1 and *exhausted += 1.
 * Two deviations from the reference: its `while other_datum['img_id'] == img_id` loop (:181-182) has no bound -- here
 * XGGM_PRETRAIN_SWAP_TRIES candidates are looked at and a row that finds none stays matched and is COUNTED (a pool of one
 * image would hang the reference); and its random.randint(0, n - 1) is taken as floor(u * n) of one uniform draw: the same
 * distribution, not the stream of Python's generator.
 * u_swap < rate and u_pick * P are evaluated in double from the fp32 draw, as in xggm_pretrain_corrupt_*; a supplied pick
 * draw outside [0, 1) is held inside the pool.  Rows move as 16-byte vectors when T * 8 is a multiple of 16 and ids, mask,
 * the pool and the outputs are 16-byte aligned, element by element otherwise.  No floating-point arithmetic touches the
 * data: every output is exact.
 * Draws: u_swap [B] and u_pick [B, TRIES] (fp32 in [0, 1)).  A NULL buffer means philox_uniform(seed, offset, sid_base + 5,
 * b) resp. philox_uniform(seed, offset, sid_base + 6, b * TRIES + r) with {seed, offset} = rng[0..1]: streams 5 and 6 behind
 * the five of xggm_pretrain_corrupt_* at the same sid_base, exactly what xggm_uniform(out, n, rng, sid_base + 5 / 6) exports.
 * rng is only read.
 * exhausted: int32 [1], only ever grows (one integer atomic add per exhausted row: no result depends on an order).
 * One launch, one wave per row; no allocation, no host synchronisation.  Refused before any launch: a null struct, a null
 * ids / mask / img or output pointer (out_ids, out_mask, is_matched, exhausted), B, T or P <= 0, a pool with one of its
 * three pointers missing, rate outside [0, 1], a NULL draw buffer without rng, an output (out_ids, out_mask, is_matched,
 * exhausted) overlapping ids, mask, img, matched_in, the pool or another output. */
#define XGGM_PRETRAIN_SWAP_TRIES 8
typedef struct xggm_pretrain_swap_args {
    const int64_t* ids;        /* [B, T] */
    const int64_t* mask;       /* [B, T] */
    const int64_t* img;        /* [B] */
    const int64_t* matched_in; /* [B] or NULL */
    const int64_t* pool_ids;   /* [P, T] or NULL */
    const int64_t* pool_mask;  /* [P, T] or NULL */
    const int64_t* pool_img;   /* [P] or NULL */
    int64_t* out_ids;          /* [B, T] out */
    int64_t* out_mask;         /* [B, T] out */
    int64_t* is_matched;       /* [B] out */
    int32_t* exhausted;        /* [1] in/out */
    int B, T;
    int64_t P;                 /* rows of the pool (ignored when the pool is NULL) */
    double rate;
    const float* u_swap;       /* [B] or NULL */
    const float* u_pick;       /* [B, TRIES] or NULL */
    const uint64_t* rng;       /* {seed, offset}; needed when a draw buffer is NULL */
    uint32_t sid_base;
} xggm_pretrain_swap_args;
int xggm_pretrain_swap(const xggm_pretrain_swap_args* args, xggm_stream_t stream);

/* xggm_batch_gather: a batch assembled from a split that is RESIDENT on the device, in ONE launch.  It replaces what the
 * reference does on the host every step: collate B items (src/vqa/vqacpv2_data.py:98-127: features, normalised boxes, the
 * soft-score target row, the adjacency), tokenise B questions and copy four tensors to the device
 * (src/vqa/vqacpv2.py:164-171).  Output row b (0 <= b < B) is built from sample s = order[start + b]; r = q_row[s] is its
 * image, stored once however many samples refer to it.
 * Tables (device, only read):
 *   feats [n_img, N, F] bf16 bit patterns, or fp32 when feats_f32;  boxes [n_img, N, 4] f32;  adj [n_img, N, N] f32 or NULL;
 *   q_row [n_q] int32;  q_ids [n_q, T] int32 (zero behind the sentence);  q_len [n_q] int32 (tokens, [CLS] / [SEP] included);
 *   q_label [n_q, K] int32 (-1: unused slot) and q_score [n_q, K] f32;  q_bias_index [n_q] int64 or NULL.
 * Selection: order [n] int64 on the device; start and B are host values.
 * Outputs (device):
 *   out_feats   row b at out_feats + b * out_feats_stride ELEMENTS, bf16 or fp32 (out_f32) <- feats[r].  Same type: the bits.
 *               fp32 -> bf16: the bits of torch.Tensor.to(torch.bfloat16) (round to nearest even, the largest finite values
 *               round up to inf, NaN -> 0x7FC0; nothing is flushed).  bf16 -> fp32: bits << 16.
 *   out_boxes   [B, N, 4] f32 <- boxes[r];  out_adj [B, N, N] f32 or NULL (not written) <- adj[r];
 *   input_ids, input_mask, segment_ids  int64 [B, T]: q_ids[s], (t < q_len[s]), 0;
 *   target      f32 row b at target + b * target_stride elements, or NULL (not written): A zeros, then
 *               target[q_label[s, k]] = q_score[s, k] for every k with q_label[s, k] >= 0.  The labels of a sample are
 *               distinct; the zero-fill and the scatter of a row run in one workgroup with a barrier between them;
 *   bias_index  int64 [B] or NULL <- q_bias_index[s];  sample int64 [B] or NULL <- s.
 * Feature rows move as 16-byte vectors (F % 8 == 0; table base, output base 16-byte aligned and the output row stride a
 * multiple of 8 elements), a box is one 16-byte vector.  Rows that are no 16-byte multiples -- target (A = 2274, 29), adj
 * with odd N -- move element by element inside their own bounds: no vector straddles a row end.  Nothing is written outside
 * rows 0 .. B - 1 of an output, nor between two rows where a stride exceeds the row.  No atomics: every output element
 * has one writer.  One launch; nothing is allocated, copied or synchronised, so the call can be captured in a graph (order
 * is read at run time: a replay follows what order holds then).
 * The kernel TRUSTS order[i] in [0, n_q), q_row in [0, n_img), q_label in [-1, A) and q_len in [0, T]: the caller validates
 * them once, when the tables are uploaded.
 * Refused before any launch: a null struct; a null or misaligned pointer (feats, boxes tables and outputs: 16 bytes; the
 * other fields: their element size; an optional field may be NULL, but an output whose table is NULL is refused);
 * B < 1 (or > 65535); start < 0 or start + B > n; T, K, A, N or F < 1; F % 8 != 0; a row stride below its row. */
typedef struct xggm_batch_gather_args {
    const void* feats;             /* [n_img, N, F] bf16 bits or fp32 */
    const float* boxes;            /* [n_img, N, 4] */
    const float* adj;              /* [n_img, N, N] or NULL */
    const int32_t* q_row;          /* [n_q] */
    const int32_t* q_ids;          /* [n_q, T] */
    const int32_t* q_len;          /* [n_q] */
    const int32_t* q_label;        /* [n_q, K] or NULL (no target) */
    const float* q_score;          /* [n_q, K] or NULL (no target) */
    const int64_t* q_bias_index;   /* [n_q] or NULL */
    const int64_t* order;          /* [n] */
    int64_t n, start;
    void* out_feats;
    int64_t out_feats_stride;      /* elements between two rows */
    float* out_boxes;              /* [B, N, 4] */
    float* out_adj;                /* [B, N, N] or NULL */
    int64_t* input_ids;            /* [B, T] */
    int64_t* input_mask;           /* [B, T] */
    int64_t* segment_ids;          /* [B, T] */
    float* target;                 /* rows of A or NULL */
    int64_t target_stride;         /* elements between two rows */
    int64_t* bias_index;           /* [B] or NULL */
    int64_t* sample;               /* [B] or NULL */
    int B, T, K, A, N, F;
    int feats_f32, out_f32;
} xggm_batch_gather_args;
int xggm_batch_gather(const xggm_batch_gather_args* args, xggm_stream_t stream);

/* xggm_batch_gather_labels: xggm_batch_gather for a store that keeps NO [n_img, N, N] adjacency.  out_adj[b] is made in
 * the launch from image r's label ids and the class x attribute cosine table, by the per-image code of
 * xggm_label_adjacency_f32 (below: data/preprocess/vqa/compute_adjacency.py:38-45, :75-90) -- the same bits that entry
 * writes for the row.  Every other role, output, rule and refusal is xggm_batch_gather's; args->adj must be NULL (a
 * stored table beside the label tables is refused), N <= 128, the label tables non-null and 4-byte aligned, Vc, Va > 0.
 * An image with an id outside [0, Vc) / [0, Va) gets an all-NaN out_adj row; nothing is read outside the table. */
typedef struct xggm_label_adj_args {
    const float* table;            /* [Vc, Va] of xggm_label_cosine_table_f32 */
    const int32_t* obj_labels;     /* [n_img, N] */
    const int32_t* attr_labels;    /* [n_img, N] */
    int Vc, Va;
} xggm_label_adj_args;
int xggm_batch_gather_labels(const xggm_batch_gather_args* args, const xggm_label_adj_args* labels, xggm_stream_t stream);

/* xggm_pretrain_gather: a CLEAN pre-training batch assembled from a corpus that is RESIDENT on the device, with the
 * matched-sentence swap fused in, in ONE launch.  It replaces what LXMERTTorchDataset.__getitem__ does per example on the
 * host (src/pretrain/lxmert_data.py:148-199: look the image up, copy its features, boxes, object / attribute labels and
 * confidences, swap the sentence with probability 0.5, build the answer dict) plus the collation and the copies of the
 * batch.  Output row b (0 <= b < B) is built from sample s = order[start + b]; r = q_row[s] is its image, stored once
 * however many sentences refer to it.
 * Tables (device, only read):
 *   per image   feats [n_img, O, F] bf16 bit patterns, or fp32 when feats_f32;  boxes [n_img, O, 4] f32 (already
 *               normalised);  obj_labels, attr_labels [n_img, O] int32;  obj_confs, attr_confs [n_img, O] f32;
 *   per sample  q_row [n_q] int32;  q_ids [n_q, T] int32 ([CLS] tokens [SEP], zero behind the sentence);  q_len [n_q] int32
 *               (tokens, [CLS] / [SEP] included);  q_label [n_q, K] int32 (the keys of example.label in insertion order, -1
 *               padded: the order matters to the answer draw of xggm_pretrain_corrupt_*);  q_score [n_q, K] f32.
 * Selection: order [n] int64 on the device, read at run time; start and B are host values.
 * Outputs (device) -- the clean batch xggm_pretrain_corrupt_* takes, plus img_ids:
 *   out_feats   row b at out_feats + b * out_feats_stride ELEMENTS, bf16 or fp32 (out_f32) <- feats[r], the four type pairs
 *               exactly as in xggm_batch_gather (same type: the bits; fp32 -> bf16: torch's rounding; bf16 -> fp32: << 16);
 *   out_boxes [B, O, 4] f32 <- boxes[r];  out_obj_labels, out_attr_labels int64 [B, O] (widened);  out_obj_confs,
 *   out_attr_confs f32 [B, O];
 *   input_ids, input_mask, segment_ids  int64 [B, T]: q_ids[j], (t < q_len[j]), 0 with j = s unless the row swapped (below);
 *   label_ids int64 [B, K] <- q_label[s] (widened, -1 kept);  label_scores f32 [B, K] <- q_score[s];
 *   is_matched int64 [B];  img_ids int64 [B] <- r;  sample int64 [B] or NULL <- s;
 *   swapped_from int64 [B] or NULL: the sample whose sentence row b carries, -1 when it is its own.
 *   Labels, features and img_ids always belong to s: only the sentence can come from elsewhere (:178-183).
 * The fused swap is the rule and the draw streams of xggm_pretrain_swap, unchanged; its pool is EVERY sample of the store
 * (the reference: "a random datum of the data set", :180) and its image key is q_row:
 *   swap == 0: no draw is read, is_matched[b] = 1, rng may be NULL;
 *   else (double)u_swap[b] < rate false: the row keeps its sentence, is_matched[b] = 1;
 *   else for r = 0 .. XGGM_PRETRAIN_SWAP_TRIES - 1: j = min(floor((double)u_pick[b, r] * n_q), n_q - 1) (a pick below 0 is
 *        held at 0); the FIRST j with q_row[j] != q_row[s] supplies q_ids[j] and q_len[j], is_matched[b] = 0;
 *   no candidate qualifies: the row stays matched and *exhausted += 1 (one vector integer atomic add per such row).
 *   A NULL draw buffer means philox_uniform(seed, offset, sid_base + 5, b) resp. (..., sid_base + 6, b * TRIES + r) with
 *   {seed, offset} = rng[0..1]; rng is only read.  The decision of a row is taken by one workgroup from wave-uniform values.
 * Grid (roles, B) as xggm_batch_gather: role 0 of a row takes the decision and writes every small field, roles 1 .. move
 * the feature row as 16-byte vectors (F % 8 == 0, 16-byte aligned bases, a row stride that is a multiple of 8 elements); a
 * box is one 16-byte vector.  Rows of T, O or K elements need not be multiples of 16 bytes: they move element by element
 * inside their own bounds, no vector straddles a row end.  Every output element has one writer; nothing is written outside
 * rows 0 .. B - 1 of an output, nor between two rows where the stride exceeds the row.  One launch; nothing is allocated,
 * copied or synchronised, so the call can be captured in a graph (order, rng and the draws are read at run time).
 * The kernel TRUSTS order[i] in [0, n_q), q_row in [0, n_img) and q_len in [0, T]: the caller validates them once, when
 * the tables are uploaded.
 * Refused before any launch: a null struct; a null or misaligned required pointer (feats, boxes tables and outputs: 16
 * bytes; the other fields: their element size; only sample and swapped_from may be NULL -- an output whose table is NULL is
 * refused); B < 1 (or > 65535); start < 0 or start + B > n; T, K, O, F, n_img or n_q < 1; F % 8 != 0; a feature row stride
 * below the row or no multiple of 8; swap with rate outside [0, 1], with NULL exhausted, or with a NULL draw buffer and
 * NULL rng; an output overlapping a table, order, rng, a draw buffer or another output. */
typedef struct xggm_pretrain_gather_args {
    const void* feats;             /* [n_img, O, F] bf16 bits or fp32 */
    const float* boxes;            /* [n_img, O, 4] */
    const int32_t* obj_labels;     /* [n_img, O] */
    const int32_t* attr_labels;    /* [n_img, O] */
    const float* obj_confs;        /* [n_img, O] */
    const float* attr_confs;       /* [n_img, O] */
    const int32_t* q_row;          /* [n_q] */
    const int32_t* q_ids;          /* [n_q, T] */
    const int32_t* q_len;          /* [n_q] */
    const int32_t* q_label;        /* [n_q, K] */
    const float* q_score;          /* [n_q, K] */
    const int64_t* order;          /* [n] */
    int64_t n_img, n_q, n, start;
    void* out_feats;
    int64_t out_feats_stride;      /* elements between two rows */
    float* out_boxes;              /* [B, O, 4] */
    int64_t* out_obj_labels;       /* [B, O] */
    int64_t* out_attr_labels;      /* [B, O] */
    float* out_obj_confs;          /* [B, O] */
    float* out_attr_confs;         /* [B, O] */
    int64_t* input_ids;            /* [B, T] */
    int64_t* input_mask;           /* [B, T] */
    int64_t* segment_ids;          /* [B, T] */
    int64_t* label_ids;            /* [B, K] */
    float* label_scores;           /* [B, K] */
    int64_t* is_matched;           /* [B] */
    int64_t* img_ids;              /* [B] */
    int64_t* sample;               /* [B] or NULL */
    int64_t* swapped_from;         /* [B] or NULL */
    int B, T, K, O, F;
    int feats_f32, out_f32;
    int swap;                      /* 0: no swap, no draw is read */
    double rate;
    const float* u_swap;           /* [B] or NULL */
    const float* u_pick;           /* [B, TRIES] or NULL */
    const uint64_t* rng;           /* {seed, offset}; needed when swap and a draw buffer is NULL */
    uint32_t sid_base;
    int32_t* exhausted;            /* [1] in/out; needed when swap */
} xggm_pretrain_gather_args;
int xggm_pretrain_gather(const xggm_pretrain_gather_args* args, xggm_stream_t stream);

/* ---- preprocessing that feeds the path ----------------------------------------------------
 * adj_true of every sample: data/preprocess/vqa/compute_adjacency.py:38-45 (compute_cosin_sim_v2) + :90.
 *   c[i][j] = cos(cls[i], attr[j]) for j >= i, 0 below the diagonal  (torch.cosine_similarity, eps 1e-6: each
 *   norm clamped from below by eps);  a = c + c^T (the diagonal counts twice);  adj = a / max(a).
 * cls, attr: fp32 [n_img][N][D] (BERT pooled embeddings of the objects' class and attribute names), adj: fp32
 * [n_img][N][N]; N <= 64, D % 4 == 0. */
int xggm_cosine_adjacency_f32(const float* cls, const float* attr, float* adj, int n_img, int N, int D, float eps,
                              xggm_stream_t stream);

/* adj_true from the detector's label ids.  The reference embeds the 2 N label strings of every image with BERT and calls
 * torch.cosine_similarity 666 times per image (data/preprocess/vqa/compute_adjacency.py:38-45, :75-90:
 * compute_cosin_sim_v2 and its caller); but an image's adjacency depends only on its ids, and there are only Vc x Va distinct cosines.
 * xggm_label_cosine_table_f32: cls fp32 [Vc][D], attr fp32 [Va][D] (pooled embeddings of objects_vocab.txt /
 *   attributes_vocab.txt) -> table fp32 [Vc][Va],
 *     table[o][a] = dot(cls_o, attr_a) / (max(sqrt(|cls_o|^2), eps) * max(sqrt(|attr_a|^2), eps)),
 *   each of the three sums ONE fmaf chain over k ascending from 0.f -- the arithmetic of xggm_cosine_adjacency_f32 and
 *   xggm_cosine_adjacency_long_f32, so the table holds the bits those compute per image.  No matrix cores, no split sum.
 *   D % 4 == 0, cls / attr 16-byte aligned, Vc, Va > 0.
 * xggm_label_adjacency_f32: obj_labels, attr_labels int32 [n][N], 1 <= N <= 128 -> adj fp32 [n][N][N]; per image
 *   c[i][j] = table[obj_i][attr_j] for j >= i, c + c on the diagonal and c + 0.f off it, the maximum by fmaxf, every
 *   value divided by it, written to [i][j] and [j][i]: bit-equal to the two cosine entries on the gathered embeddings.
 *   An image with an id outside [0, Vc) / [0, Va) is all NaN (its neighbours are untouched); nothing is read outside the
 *   table.  One workgroup per image; no atomics.
 * Refused before any launch: a null pointer, Vc or Va <= 0, n <= 0, N outside 1..128, D % 4 != 0, misaligned tables. */
int xggm_label_cosine_table_f32(const float* cls, const float* attr, float* table, int Vc, int Va, int D, float eps,
                                xggm_stream_t stream);
int xggm_label_adjacency_f32(const float* table, int Vc, int Va, const int32_t* obj_labels, const int32_t* attr_labels,
                             float* adj, int n, int N, xggm_stream_t stream);

/* ---- optimiser ---------------------------------------------------------------------------
 * The gradient norm (nn.utils.clip_grad_norm_, src/vqa/vqacpv2.py:175).  Five entries, ONE mechanism -- "sum (the
 * squares of) some ranges in a fixed order, then finish a scalar" -- in two launches (one when there is no range):
 *  - ranges: [offsets[i], offsets[i] + lengths[i]) of a 16-byte aligned buffer, non-empty, starting on a multiple of 4
 *    (fp32) or 8 (bf16) elements; offsets / lengths are HOST arrays.  Squared ranges come first, then (fp32 only) ranges
 *    summed as they are: the gradient-norm slots of the weight-gradient GEMMs (xggm_gemm_problem.sqsum) already hold
 *    sums of squares.
 *  - fixed (range, slice) order: every range gets workgroups in proportion to its length (about 4096 in all), every
 *    workgroup sums one slice of one range and writes its partial to `ws` at its (range, slice) position; a second
 *    one-workgroup launch adds the partials in that order.  No floating-point atomics: the bits depend on the ranges
 *    of the call alone, so data-parallel replicas that hold identical gradients compute identical norms and stay
 *    bit-identical.  How ranges are grouped into calls decides the slices, and so the bits.
 *  - `ws`: caller-owned scratch of XGGM_SQNORM_WS_FLOATS floats (contents irrelevant before, undefined after).
 *  - finish: *out = ((accumulate ? *out : 0) + sum) * mul; *norm (or NULL) = sqrt(*out), the total norm clip_grad_norm_
 *    returns.  accumulate extends a sum that another call (or an all-reduce over the ranks) has left in *out; mul = 1 /
 *    world^2 turns the norm of SUMMED data-parallel gradients into the norm of their average.  With no range at all the
 *    call only seeds / finishes.
 *  - `tail` (xggm_clip_norm_*, or NULL): work of the pass that the finishing workgroup takes along, see xggm_pass_tail.
 *
 * xggm_sqnorm_f32: one squared range, the whole of g[0, n); accumulate = 1, mul = 1, no norm. */
#define XGGM_SQNORM_WS_FLOATS 4100
int xggm_sqnorm_f32(const float* g, int64_t n, float* out, float* ws, xggm_stream_t stream);
/* up to 16 ranges of ONE fp32 buffer, all squared (square != 0) or all summed as they are (square == 0);
 * accumulate = !overwrite. */
int xggm_sqnorm_multi_f32(const float* base, const int64_t* offsets, const int64_t* lengths, int n, float* out, float* norm,
                          float* ws, int overwrite, int square, float mul, xggm_stream_t stream);
/* xggm_sqnorm_f32 over a bf16 buffer (the data-parallel wire arena) */
int xggm_sqnorm_bf16(const void* g, int64_t n, float* out, float* ws, xggm_stream_t stream);
/* *lr_scale = warmup_linear(*step / t_total, warmup); *step += 1 (optimization.py:42-48) */
int xggm_sched_step(int64_t* step, float* lr_scale, int64_t t_total, float warmup, xggm_stream_t stream);
/* the same for n <= 16 distinct counters steps[index[i]] / lr_scale[index[i]] of one table in one launch (all
 * parameter groups of one optimiser step); index, t_total, warmup: HOST arrays of n entries */
int xggm_sched_step_multi(int64_t* steps, float* lr_scale, const int* index, const int64_t* t_total, const float* warmup,
                          int n, xggm_stream_t stream);

/* The fused optimiser update: ONE entry for every rule.  A span is BertAdam.step (src/lxrt/optimization.py:159-193) or a
 * torch.optim rule on a contiguous range, fused with the clip scale min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) and the
 * bf16 shadow-weight write, with everything a deployment variant needs in one argument block (HOST struct, copied):
 *  - g_bf16 != 0: `g` holds bf16 gradients (the data-parallel wire arena the weight-gradient GEMMs write and
 *    RCCL reduces in place: no fp32 copy of the matrix gradients exists);
 *  - lr_dev (or NULL): device scalar that replaces `lr` (edits of param_groups[i]['lr'] reach replayed graphs);
 *  - shadow8 (or NULL): e4m3 copy of the updated weights for the fp8 forward products, written in the same pass.
 *    Per-tensor scales: w8_id[(elem0 + i) >> 8] (uint16 per 256-element chunk of the arena, 0 = this chunk has no
 *    e4m3 copy) selects the entry of w8_qscale the value is multiplied by, and w8_amax[id] is raised to max |p_new|
 *    for the next scale update (xggm_fp8_scale_update).  `elem0`: arena offset of p[0], a multiple of 256 when
 *    shadow8 is given.
 * p, m, v are 16-byte aligned, g too (bf16: 8), the shadow 8. */
typedef struct xggm_adam_args {
    float* p;
    const void* g;
    float* m;
    float* v;
    void* shadow_bf16;
    int64_t n;
    const float* sqnorm;
    float max_norm;
    float lr;
    const float* lr_dev;
    const float* lr_scale;
    float b1, b2, eps, weight_decay;
    int g_bf16;
    void* shadow8;
    const uint16_t* w8_id;
    const float* w8_qscale;
    float* w8_amax;
    int64_t elem0;
    float g_scale; /* > 0: every gradient is multiplied by it (1 / world: the exchange SUMS over the data-parallel ranks
                      and the average is taken here); <= 0 reads as 1 */
    int w8_amax_slots; /* entry id of w8_amax starts at w8_amax[id * max(1, w8_amax_slots)]; see xggm_gemm_problem.amax_slots */
} xggm_adam_args;
/* The reference's other optimisers (src/param.py:9-31 binds --optim rms|adam|adamw|adamax|sgd to torch.optim classes,
 * src/vqa/vqacpv2.py:141 builds args.optimizer(self.model.parameters(), args.lr)) on the same fused pass as BertAdam:
 * clip scale, update, bf16 shadow, n & 3 tail, spans through a prefix table.  torch's single-tensor semantics with
 * g' = g * coef + weight_decay * p (coef: clip scale times g_scale):
 *   ADAM     m += (g' - m)(1 - b1); v = b2 v + (1 - b2) g'^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
 *   ADAMW    p *= 1 - lr * weight_decay first, then ADAM with g' = g * coef
 *   ADAMAX   m as ADAM; v = max(b2 v, |g'| + eps); p -= lr / bc1 * m / v
 *   SGD      momentum == 0: p -= lr g' (m, v neither read nor written); else m = g' at the group's first step,
 *            momentum * m + (1 - dampening) g' after it; p -= lr * (nesterov ? g' + momentum * m : m)
 *   RMSPROP  v = alpha v + (1 - alpha) g'^2; d = g' / (sqrt(v) + eps); momentum == 0: p -= lr d (m untouched), else
 *            m = momentum * m + d; p -= lr m
 * `a` holds the span (for the torch rules a.b1 / a.b2 are ignored, a.shadow8 must be NULL; a.eps and a.weight_decay are
 * used).  The complements 1 - b1, 1 - b2, 1 - dampening, 1 - alpha are taken in DOUBLE on the host
 * (fp32 1 - 0.999f is off by 1.3e-5 relative).  bc = 1 - b^t comes from `step_scalars`: three device floats {1 / bc1,
 * 1 / sqrt(bc2), first-step flag} that xggm_sched_step_ex computed in double from the device-resident step counter
 * (required for ADAM / ADAMW / ADAMAX and for SGD with momentum; NULL elsewhere).
 * XGGM_RULE_BERTADAM is BertAdam on `a` alone: the rule fields are zero and not read. */
#define XGGM_RULE_BERTADAM 0
#define XGGM_RULE_ADAM 1
#define XGGM_RULE_ADAMW 2
#define XGGM_RULE_ADAMAX 3
#define XGGM_RULE_SGD 4
#define XGGM_RULE_RMSPROP 5
typedef struct xggm_optim_args {
    xggm_adam_args a;
    int rule;                  /* XGGM_RULE_*: the same for every span of a call */
    const float* step_scalars; /* device: {1 / bc1, 1 / sqrt(bc2), first step ? 1 : 0} of this span's group */
    double b1, b2;             /* ADAM / ADAMW / ADAMAX */
    double momentum;           /* SGD, RMSPROP (zero or not: the same for every span of a call) */
    double dampening;          /* SGD */
    double alpha;              /* RMSPROP */
    int nesterov;              /* SGD */
} xggm_optim_args;

/* Split param_groups (`map`, or NULL): lr and weight decay PER TENSOR, for an optimiser whose param_groups cut
 * through a contiguous range (the BERT "no decay for bias / LayerNorm" grouping, layer-wise lr decay, parameters left out).
 *   ids    DEVICE, one uint8 per 8 elements of the arena: element i of a span reads ids[(elem0 + i) >> 3].  Tensors start on
 *          multiples of 8 elements, so 8 elements never mix two tensors: 1/8 byte of map per parameter.
 *   table  DEVICE, n_table pairs {lr, weight_decay}, 8-byte aligned; entry 0 is not read.
 * Per element: lr = table[id].lr * *lr_scale and weight_decay = table[id].weight_decay take the place of the span's lr /
 * lr_dev / weight_decay (which are not read); the schedule value, the clip scale, g_scale, the rule's arguments, the bf16
 * shadow and the e4m3 copy are the span's, and the arithmetic is the unmapped update's bit for bit.
 * Id 0 (and any id >= n_table) means "not in this optimiser": p, m, v, the shadow and the e4m3 copy of such an element are
 * not written.  Alignment gaps hold zeros and may carry any id.  Checked with a map: ids and table non-NULL,
 * 1 <= n_table <= 256, every span's elem0 a multiple of 8 and [elem0, elem0 + n) inside the n_ids * 8 elements the map covers. */
typedef struct xggm_hyper_map {
    const uint8_t* ids;
    int64_t n_ids;
    const float* table;
    int n_table;
} xggm_hyper_map;
/* n spans (HOST array: every arena group a pass updates, or a rank's slices of them under the sharded update), one launch
 * per 8 spans; all spans share rule, gradient type and whether momentum is zero (src/param.py:9-31,
 * src/vqa/vqacpv2.py:141).  The map and every span are checked before any launch.  No atomics beyond the e4m3 maxima, no
 * allocation, no synchronisation. */
int xggm_optim_multi(const xggm_optim_args* args, int n, const xggm_hyper_map* map /* or NULL */, xggm_stream_t stream);

/* BertLamb: BertAdam.step (src/lxrt/optimization.py:159-193) with a layer-wise trust ratio between its lines 171 and 192 --
 * LAMB, the large-batch remedy of the BERT code base, for the optimiser that src/vqa/vqacpv2.py:125-128 builds.  Per
 * parameter tensor T, with g' = g * coef and coef the clip scale times g_scale as in xggm_adam_args:
 *     m = b1 m + (1 - b1) g'        v = b2 v + (1 - b2) g'^2
 *     u = m / (sqrt(v) + eps) + weight_decay * p
 *     r_T = (float)(sqrt(Sp) / sqrt(Su))  if T is adapted and Sp > 0 and Su > 0,  else 1
 *           Sp = sum over T of (double)p^2 (the values BEFORE the step), Su = sum over T of (double)u^2
 *     p  -= (lr * lr_scale * r_T) * u, then the bf16 shadow
 * with every fp32 operation shaped as in xggm_optim_multi's BertAdam rule, so that r_T = 1 gives that rule's bits in p, m,
 * v and the shadow.
 *   spans    HOST array of n xggm_adam_args (shadow8 NULL), in arena order, not overlapping, elem0 a multiple of 8; all share
 *            the gradient type.  elem0 is always read here: it places the span against the tensor table.
 *   tensors  DEVICE table of n_tensors entries {elem0, n, adapted}, sorted by elem0, disjoint, every elem0 a multiple of 8
 *            (tensors start on multiples of 8 elements, as the hyper map assumes).  A tensor takes part when its first element
 *            lies in a span; it must then end inside that span.  Elements of a span that belong to no tensor (alignment gaps)
 *            are neither read nor written: they hold zeros and keep them.  The table may list tensors outside every span.
 *   map      the xggm_hyper_map of xggm_optim_multi, or NULL: lr and weight_decay of a tensor are those of the id of its first
 *            element.  Id 0 (or >= n_table): no byte of the tensor is written, its ratio reads 1.
 *   ratios_out  DEVICE float [n_tensors]: r_T of every tensor that took part; the others keep what they held.
 *   ws       DEVICE scratch of xggm_lamb_workspace_bytes(arena_elems, n_tensors) bytes, 16-byte aligned, arena_elems >= the end
 *            of the last span; needs no initialisation, undefined after.
 * ORDER OF THE SUMS (of Sp over x = p^2 and of Su over x = u^2; it depends on the tensor's length alone: not on the grid, the
 * timing, where the tensor lies or which other tensors the call updates).  All squares and additions are fp64 (the square of
 * an fp32 value is exact there); there is no floating-point atomic.  The tensor is cut into chunks of XGGM_LAMB_CHUNK = 2048
 * elements from its first element on, the last one padded with +0.0.  Within a chunk, element e belongs to thread
 * t = (e / 4) % 256:
 *     a[t] = (((((((+0.0 + x[4t]) + x[4t+1]) + x[4t+2]) + x[4t+3]) + x[1024+4t]) + x[1025+4t]) + x[1026+4t]) + x[1027+4t]
 *     then inside each run of 64 threads (l = t % 64), for h = 32, 16, 8, 4, 2, 1:   a[l] = a[l] + a[l + h]   for l in [0, h)
 *     partial = (a[0] + a[64]) + (a[128] + a[192])
 * and over the chunks c = 0 .. C - 1 of the tensor:  b[t] = ((+0.0 + partial[t]) + partial[t + 256]) + ... for t in [0, 256)
 * (+0.0 where t >= C), reduced by the same two lines.  numpy: xggm_amd.lxrt.optimization.lamb_sum_host.
 * Three launches per 8 spans, behind each other on the stream: phase A reads g, m, v, p, writes m and v and leaves the chunks'
 * sums in ws; a finish with one workgroup per table entry writes ratios_out; phase B recomputes u from m, v, p with the same
 * device function (the norm describes what is applied) and writes p and the shadow.  Every argument is checked before the
 * first launch: null spans / tensors / ratios_out / ws, n or n_tensors < 1, a span with a null pointer, no elements, a
 * misaligned pointer, an e4m3 copy, another gradient type, an elem0 that is no multiple of 8 or lies in front of the previous
 * span's end, or (with a map) beyond the id map; a bad map; ws_bytes below the declared size.  No allocation, no
 * synchronisation: legal inside a stream capture. */
#define XGGM_LAMB_CHUNK 2048
typedef struct xggm_lamb_tensor {
    int64_t elem0;   /* arena offset of the tensor's first element */
    int64_t n;       /* its elements */
    int64_t adapted; /* 0: r_T = 1 */
} xggm_lamb_tensor;
size_t xggm_lamb_workspace_bytes(int64_t arena_elems, int n_tensors);
int xggm_lamb_multi(const xggm_adam_args* spans, int n, const xggm_lamb_tensor* tensors, int n_tensors,
                    const xggm_hyper_map* map /* or NULL */, float* ratios_out, void* ws, size_t ws_bytes, xggm_stream_t stream);

/* xggm_sched_step_multi with a schedule kind per entry (src/lxrt/optimization.py:27-48: warmup_cosine, warmup_constant,
 * warmup_linear; the xggm_sched_step* calls keep meaning warmup_linear) and the per-step scalars of xggm_optim_multi:
 * for entry i with k = index, s = steps[k]: lr_scale[k] = kind(s / t_total, warmup) in double (1 when t_total <= 0),
 * steps[k] = t = s + 1 and, with step_scalars (or NULL), step_scalars[4 k ..] = {1 / (1 - b1^t), 1 / sqrt(1 - b2^t),
 * s == 0 ? 1 : 0, 0} -- computed ONCE per step in double from the device counter (graphs replay it), as torch computes
 * them from Python floats (src/param.py:9-31, src/vqa/vqacpv2.py:141).  entries: HOST array, n <= 16 distinct counters. */
#define XGGM_SCHED_LINEAR 0
#define XGGM_SCHED_COSINE 1
#define XGGM_SCHED_CONSTANT 2
typedef struct xggm_sched_entry {
    int index;
    int kind; /* XGGM_SCHED_* */
    int64_t t_total;
    double warmup;
    double b1, b2;
} xggm_sched_entry;
int xggm_sched_step_ex(int64_t* steps, float* lr_scale, float* step_scalars, const xggm_sched_entry* entries, int n,
                       xggm_stream_t stream);

/* The tail of a pass in two launches instead of seven: the norm (see "optimiser" above) over up to 24 ranges in all --
 * `n` ranges of the gradient buffer `g` (squared) and `n_slots` ranges of the slot table the weight-gradient products
 * filled (summed as they are); accumulate = 0.  With `tail` the finishing workgroup also performs
 * xggm_sched_step_multi's schedule step for tail->n counters (BertAdam.step's bookkeeping,
 * src/lxrt/optimization.py:170-180; index, t_total, warmup: HOST arrays) and, with tail->rng, xggm_rng_advance(rng,
 * rng_by). */
typedef struct {
    int64_t* steps;
    float* lr_scale;
    const int* index;
    const int64_t* t_total;
    const float* warmup;
    int n;
    uint64_t* rng; /* or NULL */
    uint64_t rng_by;
} xggm_pass_tail;
int xggm_clip_norm_f32(const float* g, const int64_t* offsets, const int64_t* lengths, int n, const float* slots,
                       const int64_t* slot_offsets, const int64_t* slot_lengths, int n_slots, float* out, float* norm, float* ws,
                       float mul, const xggm_pass_tail* tail, xggm_stream_t stream);
/* the same over up to 24 squared ranges of a BF16 buffer (the data-parallel wire arena); accumulate = 1 is the sharded
 * update's second half */
int xggm_clip_norm_bf16(const void* g, const int64_t* offsets, const int64_t* lengths, int n, float* out, float* norm, float* ws,
                        int accumulate, float mul, const xggm_pass_tail* tail, xggm_stream_t stream);

/* out = in with the diagonal of every [N, N] matrix zeroed: adj_true.triu(1) + adj_true.tril(-1), src/vqa/vqacpv2.py:188 */
int xggm_zero_diag_f32(const float* in, float* out, int B, int N, xggm_stream_t stream);
/* out[i] = (1 - mask[i]) * -10000: additive attention mask from the int64 token mask, src/lxrt/modeling.py:919-928 */
int xggm_additive_mask(const int64_t* mask, float* out, int64_t n, xggm_stream_t stream);
/* *out = *a + *b + *c + *d (NULL terms skipped): the sum of the loss terms of a pass, src/vqa/vqacpv2.py:220-221 */
int xggm_add_scalars_f32(const float* a, const float* b, const float* c, const float* d, float* out, xggm_stream_t stream);
/* out = a + b (+ c (+ d)), n elements, summed in fp32 and rounded once; out may alias an input.  Replaces the sums
 * torch's autograd engine forms (at::add) where a tensor of the training loop feeds several consumers
 * (reference: x, feat_seq[1], node_feats, adj_noise in src/vqa/vqacpv2.py:195-251). */
int xggm_add_n_f32(const float* a, const float* b, const float* c, const float* d, float* out, int64_t n, xggm_stream_t stream);
int xggm_add_n_bf16(const void* a, const void* b, const void* c, const void* d, void* out, int64_t n, xggm_stream_t stream);
/* Rows of a [V, H] table by index (H % 4 == 0; indices outside [0, V) are skipped): dst[i, :] = bf16(src[idx[i], :]) and
 * dst[idx[i], :] = src[i, :] (duplicate indices must carry identical rows).  Data parallelism exchanges only the rows of
 * the word-embedding gradient (nn.Embedding(30522, 768), src/lxrt/modeling.py:283) that some rank touched.
 * Four elements per access: gather needs src 16-byte and dst 8-byte aligned, scatter src and dst 8-byte aligned; a
 * misaligned pointer is refused on the host. */
int xggm_gather_rows_bf16(const float* src, const int64_t* idx, void* dst, int n, int H, int64_t V, xggm_stream_t stream);
int xggm_scatter_rows_bf16(const void* src, const int64_t* idx, void* dst, int n, int H, int64_t V, xggm_stream_t stream);
/* dst [rows, ld] bf16 = cast(src [rows, n], fp32 if src_f32 else bf16), columns n .. ld - 1 zero: the padded row stride
 * the backward products of an odd-width output run on (answer logits of src/vqa/vqacpv2_model.py:63-70). */
int xggm_pad_rows_bf16(const void* src, int src_f32, void* dst, int rows, int n, int ld, xggm_stream_t stream);
/* zero up to 16 element ranges [offset[i], offset[i] + length[i]) of one fp32 buffer in ONE launch: the
 * atomically accumulated gradient ranges of all parameter groups at the start of a backward pass.
 * offsets / lengths are HOST arrays (copied into the kernel arguments); both multiples of 4. */
int xggm_zero_ranges_f32(float* base, const int64_t* offsets, const int64_t* lengths, int n, xggm_stream_t stream);
/* the same fill (n may be 0) and, in the same launch, rows row_ids[0 .. min(*row_n, row_cap)) of the fp32 table
 * [R, H] zeroed (row_ids / row_n: DEVICE buffers, as xggm_embed_bwd_listed_* left them; H a multiple of 4) */
int xggm_zero_ranges_rows_f32(float* base, const int64_t* offsets, const int64_t* lengths, int n, float* table,
                              const int64_t* row_ids, const int* row_n, int row_cap, int64_t R, int H, xggm_stream_t stream);

/* ---- small element-wise kernels ---------------------------------------------------------
 * out = scale * (1 + *scale_ptr) * x   (GIN's (1+eps), src/module/gin.py:32) */
int xggm_scale_f32(const void* x, void* out, int64_t n, float scale, const float* scale_ptr, xggm_stream_t stream);
int xggm_scale_bf16(const void* x, void* out, int64_t n, float scale, const float* scale_ptr, xggm_stream_t stream);
/* out(T) = dy(fp32) * y(fp32) * (1 - y): backward of encoder_adj's Sigmoid (vqacpv2_model.py:93) */
int xggm_sigmoid_bwd_f32(const float* dy, const float* y, void* out, int64_t n, xggm_stream_t stream);
int xggm_sigmoid_bwd_bf16(const float* dy, const float* y, void* out, int64_t n, xggm_stream_t stream);
/* out(T) = dy(T) * (1 - y(T)^2): backward of BertPooler's tanh (src/lxrt/modeling.py:619) */
int xggm_tanh_bwd_f32(const void* dy, const void* y, void* out, int64_t n, xggm_stream_t stream);
int xggm_tanh_bwd_bf16(const void* dy, const void* y, void* out, int64_t n, xggm_stream_t stream);
/* out(T) = x(fp32): loader tensors (feats, boxes) and fp32 logit gradients entering the T path.  Four elements per
 * access: x 16-byte aligned, out 16-byte (fp32) / 8-byte (bf16) aligned, else refused on the host. */
int xggm_cast_from_f32_f32(const float* x, void* out, int64_t n, xggm_stream_t stream);
int xggm_cast_from_f32_bf16(const float* x, void* out, int64_t n, xggm_stream_t stream);

/* ---- replica drift guard -----------------------------------------------------------------
 * 64-bit fingerprints of byte ranges of device memory.  The reference keeps ONE set of weights under nn.DataParallel
 * (src/lxrt/entry.py:183-184), so its replicas are identical for free; here every rank owns a copy that a collective
 * could let drift, and dist.ReplicaGuard compares one word per (buffer, arena group) across the ranks.
 *
 * THE CONTRACT (restated in numpy by xggm_amd.fingerprint.fingerprint_host; the tests compare the two bit for bit).
 * For the little-endian 32-bit words w[0 .. W) of a range, W = bytes / 4, and a 32-bit salt, all arithmetic wrapping:
 *     k(i) = (i * 0x9E3779B9 + salt)        mod 2^32
 *     x(i) = (w[i] ^ k(i)) * 0x7FEB352D     mod 2^32;      x(i) ^= x(i) >> 15
 *     fp   = sum over i of   x(i) * (2 * (i mod 2^31) + 1)      mod 2^64;      fp of no words = 0
 *  - a pure function of (bytes, salt): a sum mod 2^64 has no order, so grid shape, workgroup count, device and
 *    address do not enter;
 *  - w -> x(i) is a bijection of the 32-bit words for every i (xor with a constant, multiplication by an odd number,
 *    xor-shift), and the factor of x(i) is odd and below 2^32: changing ONE word moves fp by a non-zero product below
 *    2^64, i.e. with certainty; exchanging two unequal words changes it except by accident, because both k(i) and the
 *    factor depend on the index;
 *  - the salt separates buffers whose bits could coincide (params / m / v / shadow).
 * One multiply in the mix, not the two of a full avalanche hash: 32-bit integer multiplies are quarter rate on gfx950
 * and the kernel has to stay bound by HBM.
 *
 * out[i] (DEVICE, n_spans words, 8-byte aligned) = fp of spans[i] (HOST array, copied); every word is written, empty
 * ranges give 0.  ptr 4-byte aligned (non-null when bytes > 0), bytes a non-negative multiple of 4.  All ranges of a
 * call share one grid (64 ranges per grid beyond that) of about max_workgroups workgroups (0: the library chooses; at
 * least one per non-empty range) plus one small finishing launch; `ws`: caller-owned DEVICE scratch of
 * xggm_fingerprint_workspace_bytes(n_spans, max_workgroups) bytes, 8-byte aligned, contents irrelevant before and
 * undefined after.  No host synchronisation, no allocation: legal inside a stream capture. */
typedef struct xggm_fp_span {
    const void* ptr;
    int64_t bytes;
    uint32_t salt;
    uint32_t pad;
} xggm_fp_span;
size_t xggm_fingerprint_workspace_bytes(int n_spans, int max_workgroups);
int xggm_fingerprint_spans(const xggm_fp_span* spans, int n_spans, uint64_t* out, void* ws, size_t ws_bytes,
                           int max_workgroups, xggm_stream_t stream);

/* ---- answer log ---------------------------------------------------------------------------
 * The reference turns logits into answers on the host: `logit.max(1)[1].cpu()` in every training iteration
 * (src/vqa/vqacpv2.py:180-181, scored per epoch by the evaluator, src/vqa/vqacpv2_data.py:134-142) and per batch of
 * the validation sweep (src/vqa/vqacpv2.py:333-334; GQA twin src/gqa/gqa_ood.py:379-403).  Here one launch APPENDS the
 * chosen answers of a batch to buffers that stay on the device, and the host reads the log once per sweep / epoch.
 *
 * For row b < n, n = rows ? clamp(*rows, 0, B) : B (`rows`: DEVICE int, the kept rows of a padded short batch; rows
 * >= n are neither read nor logged), and c = *cursor on entry:
 *     label        = what torch.max(logits, 1) returns on the CPU: the first maximal index; a row holding NaN gives
 *                    the index of its FIRST NaN; +-inf are ordinary values; -0 == +0
 *     labels[c+b]  = label
 *     scores[c+b]  = target[b * target_stride + label]                       (with a target)
 *     *score_sum   = (..((*score_sum + scores[c]) + scores[c+1]) + ..)       (with a target and score_sum; fp64, row
 *                    order, one thread: the same bits eagerly, replayed from a graph or beside other work)
 *     *cursor      = c + n
 * If c + n > capacity NOTHING is stored, *cursor stays and *flags = (*flags | 1) + 2: bit 0 says an append did not
 * fit, the bits above it count the refused appends.  No store leaves [0, capacity) under any input.
 * logits: fp32 [B, A] with row_stride >= A floats (4-byte aligned rows are enough; 16-byte loads are used where the
 * row allows them); target: fp32 [B, A] with target_stride >= A, or NULL.  A target needs `scores`.  B <= 262144.
 * `ws`: XGGM_SUM_WS_FLOATS floats as for the losses (ws[0] == 0 at launch, left 0).  One launch of min(B, 128)
 * workgroups (more only past 8192 rows), no allocation, no host synchronisation: legal inside a stream capture.
 * Launches that share a log must be ordered against each other (one stream, or graphs replayed on it). */
typedef struct xggm_answer_log {
    int64_t* labels;   /* [capacity] chosen answer indices */
    float* scores;     /* [capacity] soft score per sample, or NULL */
    int64_t* cursor;   /* samples logged so far */
    double* score_sum; /* running sum of the scores, or NULL */
    int* flags;        /* bit 0: an append did not fit; bits 1..: how many did not */
    int64_t capacity;  /* size of labels / scores */
} xggm_answer_log;
int xggm_answer_pick_f32(const float* logits, int64_t row_stride, const float* target, int64_t target_stride, int B, int A,
                         const int* rows, xggm_answer_log* log, float* ws, xggm_stream_t stream);

/* xggm_answer_log_fold: the data-parallel ranks' answer logs merged into ONE log in sweep order.  The reference's
 * --multiGPU runs hand every replica a slice of the batch and collect the answers on the host: `logit.max(1)[1].cpu()` in
 * the training loop (src/vqa/vqacpv2.py:180-181, the train score of :285) and in the validation sweep (:333-334), over
 * the replicas of nn.DataParallel (src/lxrt/entry.py:183-184).  Here every rank appends to a log of its own; after a sweep
 * or an epoch the packed logs are all-gathered -- one collective per sweep, never per step -- and ONE launch merges them.
 *
 * logs: DEVICE int64; rank r's packed log starts at logs + r * log_stride (int64 words) and is laid out as
 *     [cursor, score_sum (fp64 bits), flags, labels[src_capacity], scores (fp32, two per word; with_scores only)]
 * with the same src_capacity on every rank.  expect: HOST array of `world` counts (copied into the kernel arguments): how
 * many answers rank r must hold; total = sum(expect).  Position p in [0, expect[r]) of rank r goes to destination d:
 *     XGGM_FOLD_CONCAT      d = expect[0] + .. + expect[r-1] + p               (a validation sweep cut into contiguous
 *                                                                              slices; counts may differ, 0 is allowed)
 *     XGGM_FOLD_INTERLEAVE  d = ((p / block) * world + r) * block + p % block  (a training epoch whose global step holds
 *                           `world` blocks of `block` samples, rank r's the r-th; every expect[r] equal, a multiple of block)
 * Written: dst->labels[d]; dst->scores[d] (with_scores); *dst->cursor = total; *dst->score_sum = ((+0.0 + s_0) + s_1) + ..
 * over the ranks' fp64 sums in rank order (when dst->score_sum is given); *dst->flags = 0; and *flag: 0 when every rank's
 * cursor equals its expect[r] and every rank's flags word (all 64 bits) is 0, else
 *     bit 0: a cursor differs;  bit 1: a rank carries refused appends;  bits 8..: the lowest offending rank.
 * The copy is carried out either way.  Every address is decided by HOST values: the kernel copies expect[r] positions
 * whatever the device cursors say, and no store leaves labels[0, total), scores[0, total), the three header words and
 * *flag under any device contents.  No atomics: the header words are written by one lane; labels move as 8-byte and scores
 * as 4-byte elements (with an odd capacity in front of it a scores region is only 4-byte aligned).  The gathered logs are
 * only read.  One launch, no allocation, no host synchronisation: legal inside a stream capture.
 * Refused before any launch: a null logs / expect / dst / flag / dst->labels / cursor / flags; world outside [1,
 * XGGM_FOLD_MAX_RANKS]; expect[r] < 0 or > src_capacity; total < 1 or > dst->capacity; an unknown layout; INTERLEAVE with
 * unequal counts, block < 1 or a count that is no multiple of block; with_scores without dst->scores; log_stride shorter
 * than one packed log; dst buffers or the flag overlapping the gathered logs; logs, labels, cursor, score_sum, flag not
 * 8-byte or scores, flags not 4-byte aligned. */
#define XGGM_FOLD_MAX_RANKS 64
#define XGGM_FOLD_CONCAT 0
#define XGGM_FOLD_INTERLEAVE 1
int xggm_answer_log_fold(const int64_t* logs, int64_t log_stride, int64_t src_capacity, int with_scores, int world, int layout,
                         int64_t block, const int64_t* expect, xggm_answer_log* dst, int64_t* flag, xggm_stream_t stream);

/* ---- sweep score --------------------------------------------------------------------------
 * The reference scores a sweep on the host: `evaluator.evaluate(quesid2ans)` walks a {question_id: answer string} dict
 * through id2datum / ans2label (src/vqa/vqacpv2_data.py:134-142, src/gqa/gqa_ood_data.py:160-167), four times per epoch
 * for the validation split (src/vqa/vqacpv2.py:271-272, :293-294) and once for the training answers (:285).  The ground
 * truth of every sample already lies on the device, in the q_label / q_score tables of xggm_batch_gather; ONE launch scores
 * the `labels` of an answer log against them.  Position i in [0, n):
 *     s        = order ? order[i] : i                       (order: int64 [n]; the sample the i-th logged answer belongs to)
 *     a        = labels[i]                                  (int64 [n])
 *     w        = keep ? (keep[i] != 0) : 1                  (keep: uint8 [n]; 0 drops the position -- a question id that
 *                                                            occurs again later in the sweep, as a dict assignment would)
 *     g        = q_group ? q_group[s] : none                (q_group: int32 [n_q], values in [0, G))
 *     score    = q_score[s][k] for the FIRST k < K with q_label[s][k] == a and q_label[s][k] >= 0, else 0
 *                                                           (q_label int32 [n_q, K], -1 = unused slot; q_score fp32 [n_q, K])
 *     v[i]     = w ? (double)score : +0.0;   v_g[i] = (w and g == group) ? (double)score : +0.0
 * A position with s outside [0, n_q) or g outside [0, G) contributes nothing to any word, none of its table rows is read
 * (q_group[s] is, when only g offends) and flag bit 1 is raised -- whatever its w.
 * out (DEVICE int64, 3 + 2 G words, every one written):
 *     [flags, count_all, count_g[0 .. G), sum_all, sum_g[0 .. G)]      counts: the positions with w = 1; sums: fp64 bit patterns
 *     flags bit 0: `cursor` (DEVICE int64, may be NULL) was given and *cursor != n;  bit 1: an index was out of range.
 * ORDER OF THE SUMS (of sum_all over v, of sum_g over v_g; it depends on n alone, not on the grid, the timing or the device):
 * v is cut into chunks of XGGM_SCORE_CHUNK = 1024 positions, the last one padded with +0.0.  Within a chunk, with x = its
 * 1024 values:
 *     a[t]  = (((+0.0 + x[t]) + x[t + 256]) + x[t + 512]) + x[t + 768]          for t in [0, 256)
 *     then for h = 128, 64, 32, 16, 8, 4, 2, 1:   a[t] = a[t] + a[t + h]          for t in [0, h)
 *     partial = a[0]
 * and the sum is (((+0.0 + partial[0]) + partial[1]) + ...) in chunk order.  All additions are fp64; there is no
 * floating-point atomic.  numpy: x.reshape(4, 256), three row additions, eight times a = a[:h] + a[h:], then a running sum
 * (xggm_amd.answers.score_host).
 * One workgroup per chunk leaves its 3 + 2 G words in `ws` with write-through stores and takes a ticket (the publication
 * pattern of common.h::ordered_grid_sum); the workgroup that draws the last ticket combines the chunks in index order.
 * `ws`: caller-owned DEVICE scratch of xggm_answer_score_workspace_bytes(n, G) bytes, 8-byte aligned; its first 8 bytes are
 * 0 at the first launch and the kernel leaves them 0; the rest needs no initialisation.  labels, order, keep and the tables
 * are only read; nothing outside out[0 .. 3 + 2 G) and the declared workspace is written.  Rows of q_label / q_score are read
 * with 4-byte loads: K is free.  One launch, no allocation, no host synchronisation: legal inside a stream capture.
 * Refused before any launch: null labels / q_label / q_score / out / ws; n < 1 (or > 2^31 - 1); n_q < 1; K < 1; G outside
 * [0, XGGM_SCORE_MAX_GROUPS]; q_group without G or G without q_group; labels, order, cursor, out, ws not 8-byte or a table
 * not 4-byte aligned; ws_bytes below the declared size. */
#define XGGM_SCORE_MAX_GROUPS 16
#define XGGM_SCORE_CHUNK 1024
size_t xggm_answer_score_workspace_bytes(int64_t n, int G);
int xggm_answer_score(const int64_t* labels, const int64_t* order, const uint8_t* keep, const int32_t* q_label,
                      const float* q_score, const int32_t* q_group, int64_t n, int64_t n_q, int K, int G, const int64_t* cursor,
                      int64_t* out, void* ws, size_t ws_bytes, xggm_stream_t stream);

/* ---- training log -------------------------------------------------------------------------
 * The reference loop reads its scalars from the GPU in every iteration: the running loss, `total_loss += loss.detach()
 * / logit.size(0)` (src/vqa/vqacpv2.py:179), and the tensorboard scalars Train/batch_loss, Train/average_loss and lr
 * (src/vqa/vqacpv2.py:256-270; GQA twin src/gqa/gqa_ood.py:165-292).  Here one short launch at the end of an optimiser
 * pass APPENDS one record of up to XGGM_TRAINLOG_COLS device scalars to a ring that stays on the device, and the host
 * reads the ring once per N iterations or per epoch.  Nothing is computed: the values are the ones earlier launches of
 * the stream left in device memory.
 *
 * src: HOST array of n <= COLS DEVICE pointers to single floats (copied into the kernel arguments, like the ranges of
 * xggm_zero_ranges_f32); a NULL entry = the column is absent.  mul: HOST array of n floats, or NULL = all ones.
 * step: DEVICE int64 (an optimiser step counter) or NULL.  With r = *cursor on entry and row = r % capacity:
 *     v_i                   = *src[i] * mul[i]                 (present columns; ONE fp32 multiply)
 *     values[row*COLS + i]  = v_i; absent columns and columns >= n hold 0.0f and their mask bit is clear
 *     steps[row]            = *step                            (when both `steps` and `step` are given)
 *     kinds[row]            = kind | mask << 8                 (bit i of mask: column i is present)
 *     sums[kind][i]         = sums[kind][i] + (double)v_i      (present columns only; non-finite values included: the
 *                             sum then turns NaN or inf, as the reference's total_loss would)
 *     counts[kind]         += 1
 *     *first_bad            = r   when *first_bad < 0 and some present v_i is inf or NaN
 *     *cursor               = r + 1
 * One thread does the stores and the sums, in column order: the same bits eagerly, replayed from a graph or beside other
 * work on the device.  No store leaves the described buffers under any input.  One launch of one wave, no allocation,
 * no host synchronisation: legal inside a stream capture.  Launches that share a log must be ordered against each
 * other (one stream, or graphs replayed on it).  Refused before any launch: n outside (0, COLS], kind outside [0,
 * KINDS), capacity <= 0, a null values / kinds / cursor / sums / counts / first_bad, 64-bit buffers that are not 8-byte
 * aligned, values / kinds / columns that are not 4-byte aligned. */
#define XGGM_TRAINLOG_COLS 8
#define XGGM_TRAINLOG_KINDS 4
typedef struct xggm_train_log {
    float* values;      /* [capacity, COLS]  record r lives in row r % capacity */
    int64_t* steps;     /* [capacity] optimiser step counter at the append, or NULL */
    int32_t* kinds;     /* [capacity] kind | (present-column mask << 8) */
    int64_t* cursor;    /* records appended so far (never wraps) */
    double* sums;       /* [KINDS, COLS] running sums per kind and column */
    int64_t* counts;    /* [KINDS] records per kind */
    int64_t* first_bad; /* -1, or the index of the first record with a non-finite present column */
    int64_t capacity;
} xggm_train_log;
int xggm_train_log_append(const float* const* src, const float* mul, int n, int kind, const int64_t* step,
                          xggm_train_log* log, xggm_stream_t stream);

/* xggm_train_log_fold: the mean of the data-parallel ranks' logs, folded into this rank's ring.  The reference averages
 * the per-replica losses of every step, `loss.mean()` and `losses.mean(0)` (src/pretrain/lxmert_pretrain.py:311-313,
 * :323-325); here every rank appends to a log of its own and, at read-back time, the rings are all-gathered into device
 * buffers -- one collective per read-back, never per step -- and ONE launch folds them.
 *
 * The n records are ALL records of the log since its reset, not wrapped: record i lives in row i (n <= capacity).  Rank
 * r's copy of record i: values vals[r * val_stride + i * COLS + c], kind word kinds[r * kind_stride + i] (kind | present
 * mask << 8, as the append stores it), step steps[r * step_stride + i] (steps NULL: not compared), cursor
 * cursors[r * cursor_stride] (cursors NULL: not compared); strides in elements of the respective type.  Per record and
 * column the `world` fp32 values are added in rank order (((v0 + v1) + v2) ...) and multiplied once by the fp32 value
 * 1 / world; a column is present in the result only if it is present on EVERY rank, an absent one holds 0.  world == 1
 * is the identity on values and kind words.  A NaN on any rank is a NaN in the mean.  Written: log->values and
 * log->kinds rows [0, n), log->sums and log->counts (all KINDS: recomputed in fp64 over the folded records in record
 * order, as the appends would have accumulated them), log->first_bad (-1, or *cursor - n + the first folded record with
 * a non-finite present column) and *flag: -1 when for every record the kind word and the step are the same on every rank
 * and every cursor equals n; else the index of the first record that disagrees, or n when only a cursor does.  The fold
 * is carried out either way; log->steps and log->cursor are left alone.
 *
 * One workgroup, fixed orders, no floating-point atomics: the same bits on every rank.  No store leaves the described
 * buffers under any input; no allocation, no host synchronisation.  Refused before any launch: world < 1, a null log /
 * ring buffer / vals / kinds / flag, capacity <= 0 or >= 2^31 - 1, n outside [1, capacity], (world > 1) a rank stride
 * shorter than n records, 64-bit buffers that are not 8-byte aligned, values / kinds that are not 4-byte aligned. */
int xggm_train_log_fold(const float* vals, const int32_t* kinds, const int64_t* steps, const int64_t* cursors,
                        int64_t val_stride, int64_t kind_stride, int64_t step_stride, int64_t cursor_stride, int world,
                        int64_t n, xggm_train_log* log, int64_t* flag, xggm_stream_t stream);

/* xggm_tokenize_wordpiece: sentences -> token ids for a whole corpus in ONE launch: what the host does per sentence with
 * BertTokenizer.tokenize(sent.strip()) (src/lxrt/tokenization.py:72-348) followed by convert_sents_to_features
 * (src/lxrt/entry.py:37-72; src/pretrain/lxmert_pretrain.py:149 for the pre-training set) -- clean the text, put spaces
 * around CJK characters, split on whitespace and pass never_split tokens through untouched (:188-207), lower-case, NFD and
 * drop Mn (:209-218), split on punctuation (:220-240), greedy longest-match-first WordPiece with "##" continuations where a
 * word of more than XGGM_TOKENIZE_MAX_WORD code points or with an unmatched remainder is [UNK] (:299-348), keep T - 2
 * tokens, add [CLS] and [SEP], pad with zeros.  Integer work only: every output is exact.
 *   bytes [n_bytes] uint8: the sentences' UTF-8 one behind the other; offsets [n + 1] int64 (device): sentence i is
 *   bytes[offsets[i] : offsets[i + 1]].  host_offsets: the same n + 1 values in HOST memory, read here before the launch
 *   (they are what is refused below); the kernel holds every read inside [offsets[i], offsets[i + 1]) and inside the buffer.
 * Tables, built on the host (xggm_amd.lxrt.tokenization.device_tables):
 *   cp_table [0x110000] uint32, one entry per code point: bits 0-2 the action (0 keep, 1 drop: U+0000, U+FFFD, Cc / Cf but
 *     \t \n \r; 2 whitespace: " \t\n\r", Zs, U+2028, U+2029; 3 CJK: a token of its own; 4 HOST, see below), bits 3-4 the
 *     length nf of the folded sequence [c for c in NFD(lower(cp)) if category(c) != "Mn"] (0 .. 3), bits 5-7 "folded
 *     character f is punctuation", bits 8-28 the folded code point (nf == 1) or the index of nf entries of cp_ext (nf > 1).
 *   cp_ext [n_ext] uint32: the folded sequences longer than one.
 *   init_slots [init_cap, 4], cont_slots [cont_cap, 4] uint32: open-addressing (linear probing) hash tables over the
 *     vocabulary -- every token under its own spelling, and every "##x" token under x -- a slot is {hash >> 32, id, offset
 *     into blob, length}, id -1 = empty; the capacities are powers of two and at least one slot is empty.  The hash of code
 *     points c_0 .. c_k is h = (.. ((c_0 + 1) M + (c_1 + 1)) M ..) + (c_k + 1) modulo 2^64 with M = XGGM_TOKENIZE_HASH_MUL, the
 *     first slot (h ^ (h >> 32)) & (cap - 1).  Dropping the last code point is (h - (c_k + 1)) * XGGM_TOKENIZE_HASH_MUL_INV,
 *     so the longest-match loop walks the candidates of a word without a prefix array.  A hit counts only after the code
 *     points in blob [n_blob] uint32 compare equal: a collision can cost a probe, never a wrong id.
 *   never_cps, never_off [n_never + 1] int32: the code points of the never_split tokens (n_never <= XGGM_TOKENIZE_MAX_NEVER).
 *   cls_id, sep_id, unk_id: the ids of [CLS], [SEP], [UNK].
 * Outputs, each may be NULL (not all), every element is written:
 *   ids [n, T] int32, len [n] int32 (tokens with [CLS] and [SEP]): the q_ids / q_len layout of the resident stores;
 *   block [3, n, T] int64: input_ids, input_mask, segment_ids, what SentenceBatcher returns;
 *   flags [n] uint8: bit 0 = the row needs the host: up to where the sentence stopped it holds a HOST code point or a
 *     malformed or cut-off UTF-8 sequence (such a byte is dropped); the row is written all the same, with ids of the tables;
 *   flagged int32 [1]: += the number of flagged rows (one integer atomic add per flagged row; the caller zeroes it).
 * HOST code points: the two effects of the host's fold that are not a function of one code point -- U+03A3, whose
 * lower-case form depends on its neighbours (final sigma), and the code points whose fold keeps a character of non-zero
 * canonical combining class, which NFD may reorder against a neighbour of the same kind.
 * A sentence stops once T - 2 tokens exist (the word that reaches the limit is finished first: it may still become ONE
 * [UNK]); what lies behind that point is not read.
 * One launch, one thread per sentence, workgroups of one wave; the only runtime-indexed scratch, the folded code points of
 * the word in flight (XGGM_TOKENIZE_MAX_WORD x 64 dwords), lives in LDS, so xggm_tokenize_workspace_bytes(n, T) is 0 and
 * nothing is allocated.  No host synchronisation.
 * Refused before any launch: a null struct, a null bytes (with n_bytes > 0) / offsets / host_offsets / cp_table / blob /
 * init_slots / cont_slots, every output null, n < 1, T < 2, offsets that are negative or fall ("not monotonic") or lie past
 * n_bytes, a capacity that is not a power of two, n_never outside [0, MAX_NEVER], offsets / block not 8-byte aligned, ids /
 * len / flagged or a table not 4-byte aligned, slots not 16-byte aligned. */
#define XGGM_TOKENIZE_MAX_WORD 100
#define XGGM_TOKENIZE_MAX_NEVER 8
#define XGGM_TOKENIZE_HASH_MUL 0x9E3779B97F4A7C15ull
#define XGGM_TOKENIZE_HASH_MUL_INV 0xF1DE83E19937733Dull
typedef struct xggm_tokenize_args {
    const uint8_t* bytes;         /* [n_bytes] */
    int64_t n_bytes;
    const int64_t* offsets;       /* [n + 1] device */
    const int64_t* host_offsets;  /* [n + 1] host */
    int64_t n;
    int T;
    const uint32_t* cp_table;     /* [0x110000] */
    const uint32_t* cp_ext;       /* [n_ext] */
    int64_t n_ext;
    const uint32_t* init_slots;   /* [init_cap, 4] */
    int64_t init_cap;
    const uint32_t* cont_slots;   /* [cont_cap, 4] */
    int64_t cont_cap;
    const uint32_t* blob;         /* [n_blob] */
    int64_t n_blob;
    const uint32_t* never_cps;
    const int32_t* never_off;     /* [n_never + 1] */
    int n_never;
    int32_t cls_id, sep_id, unk_id;
    int32_t* ids;                 /* [n, T] out or NULL */
    int32_t* len;                 /* [n] out or NULL */
    int64_t* block;               /* [3, n, T] out or NULL */
    uint8_t* flags;               /* [n] out or NULL */
    int32_t* flagged;             /* [1] in/out or NULL */
} xggm_tokenize_args;
int xggm_tokenize_wordpiece(const xggm_tokenize_args* args, xggm_stream_t stream);
size_t xggm_tokenize_workspace_bytes(int64_t n, int T);

/* xggm_tsv_decode: the six base64 fields of n lines of a bottom-up feature TSV (train2014_obj36.tsv, vg_gqa_obj36.tsv ...)
 * -> rows [row0, row0 + n) of the stores' image tables in ONE launch: what the host does per line with base64.b64decode +
 * np.frombuffer + reshape (src/utils.py:41-52) and, with normalize != 0, per item with the box normalisation and its range
 * check (src/pretrain/lxmert_data.py:165-171, src/vqa/vqacpv2_data.py:108-117).  Integer and bit work, one correctly rounded
 * division: every output is exact.  O objects and F features per object are fixed per table.
 *   text [alloc_bytes] uint8 (device): a chunk of the file as it is, of which [0, n_bytes) is text.  Field starts have no
 *   alignment and the kernel fetches whole aligned 16-byte words around a field, so text must be 16-byte aligned and
 *   alloc_bytes, the size of its allocation, a multiple of 16 (>= n_bytes): every read stays inside [0, alloc_bytes).
 *   desc [n, XGGM_TSV_DESC] int64 (device): per line XGGM_TSV_FIELDS (offset, length) pairs into text -- objects_id,
 *   objects_conf, attrs_id, attrs_conf, boxes, features, the file's order -- then img_w, img_h.  The host finds them
 *   (xggm_amd.tools.tsv.scan_chunk).  host_desc: the same values in HOST memory, read here before the launch (they are
 *   what is refused below); the kernel holds every read inside the buffer whatever the device copy says.
 * Outputs, each may be NULL (not all; flags and counts are the same whichever tables are asked for: every field is
 * decoded); of rows [row0, row0 + n) every element is written, no store ever leaves them:
 *   feats [capacity, O, F] fp32 (bit copies of the O F little-endian fp32) or, feats_bf16 != 0, bf16 rounded to nearest
 *     even: bit for bit torch.Tensor.to(torch.bfloat16) on every non-NaN input (0x7F7FFFFF becomes inf); a NaN becomes 0x7FC0;
 *   boxes [capacity, O, 4] fp32; normalize != 0: columns 0, 2 divided by (float)img_w, columns 1, 3 by (float)img_h,
 *     correctly rounded (numpy's b[:, (0, 2)] /= img_w on float32), then checked in double: b < 1 + 1e-5 and -b < 1e-5
 *     (a NaN fails);
 *   obj_labels, attr_labels [capacity, O] int32 from the O little-endian int64 of objects_id / attrs_id; a value outside
 *     int32 is flagged and stored as 0;  obj_confs, attr_confs [capacity, O] fp32 bit copies;
 *   flags [n] uint32, one per LINE (not per table row): bit 0 a character outside the base64 alphabet, or '=' anywhere but
 *     the last one or two places that bytes % 3 calls for (or something else there); bit 1 a field whose length is not
 *     4 ceil(bytes / 3) for this O, F; bit 2 an id outside int32; bit 3 a box outside the range check; bit 4 a non-finite
 *     feature (informational); bits 8 .. 13 which of the six fields raised bits 0-1;
 *   counts [2] int32 (the caller zeroes them): += the lines with any of bits 0-2, += the lines with bit 3 (one integer
 *     atomic add per such line; there are no other atomics).
 * A line with bit 0 or 1 still writes its whole rows: a field of the wrong length decodes to zeros, a wrong character to
 * six zero bits.  Lines with bits 0-2 are for the host path to redo (utils.load_obj_tsv): base64.b64decode skips what
 * this kernel flags.
 * One launch, one workgroup of 256 threads per line; text is staged through LDS (37 KB), nothing is allocated, there is
 * no workspace and no host synchronisation.
 * Refused before any launch: a null struct / text / desc / host_desc, every output null, n < 1, O outside [1,
 * XGGM_TSV_MAX_OBJECTS], F < 1, F % 8 != 0 (feature rows move 16 bytes per lane), O F >= 2^28, row0 < 0 or row0 + n beyond
 * capacity, an offset or length that is negative or ends past n_bytes, (normalize) img_w or img_h outside [1, 2^24), text
 * not 16-byte aligned or alloc_bytes no multiple of 16 or below n_bytes, feats not 16-byte aligned, another table not 4-byte
 * aligned. */
#define XGGM_TSV_FIELDS 6
#define XGGM_TSV_DESC 14
#define XGGM_TSV_MAX_OBJECTS 128
typedef struct xggm_tsv_decode_args {
    const uint8_t* text;          /* [alloc_bytes] */
    int64_t n_bytes, alloc_bytes;
    const int64_t* desc;          /* [n, XGGM_TSV_DESC] device */
    const int64_t* host_desc;     /* [n, XGGM_TSV_DESC] host */
    int64_t n;
    int O, F;
    int feats_bf16, normalize;
    int64_t row0, capacity;
    void* feats;                  /* [capacity, O, F] out or NULL */
    float* boxes;                 /* [capacity, O, 4] out or NULL */
    int32_t* obj_labels;          /* [capacity, O] out or NULL */
    int32_t* attr_labels;
    float* obj_confs;
    float* attr_confs;
    uint32_t* flags;              /* [n] out or NULL */
    int32_t* counts;              /* [2] in/out or NULL */
} xggm_tsv_decode_args;
int xggm_tsv_decode(const xggm_tsv_decode_args* args, xggm_stream_t stream);

/* ---- utilities ---------------------------------------------------------------------------*/
int xggm_rng_advance(uint64_t* rng, uint64_t by, xggm_stream_t stream);
int xggm_cast_f32_to_bf16(const float* x, void* out, int64_t n, xggm_stream_t stream);
/* test hooks: the dropout keep-scale (0 or 1/(1-p)) and N(0,1) draw of elements 0..n-1 */
int xggm_dropout_mask(float* out, int64_t n, float p, const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
int xggm_normal(float* out, int64_t n, const uint64_t* rng, uint32_t sid, xggm_stream_t stream);
/* the uniform [0, 1) draw of elements 0..n-1 of stream sid: what a NULL draw buffer of xggm_pretrain_corrupt_* stands for */
int xggm_uniform(float* out, int64_t n, const uint64_t* rng, uint32_t sid, xggm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* XGGM_H */
