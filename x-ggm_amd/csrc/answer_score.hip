// The sweep score (xggm_answer_score, include/xggm.h): the labels of an answer log scored against the q_label / q_score
// tables of a device-resident split, in ONE launch -- what `evaluator.evaluate(quesid2ans)` computes on the host from a
// {question_id: answer string} dict (src/vqa/vqacpv2_data.py:134-142; GQA twin src/gqa/gqa_ood_data.py:160-167), with the
// counts and sums per group (answer type, head / tail) beside the total.
//
// One workgroup per chunk of 1024 positions, a lane per position and four positions per lane (coalesced: t, t + 256, ...).
// A position is ~100 bytes of dependent reads -- label, order, keep, then the sample's group and its K label slots, rows of
// 4 K bytes at a 4-byte alignment, read element by element -- so the launch is bound by latency, not by bytes: the four
// positions of a lane have their first-level loads issued together.  The sums are fp64 and their order is the one the
// header writes down: per lane in position order, a halving tree over the 256 lanes in LDS, then the chunks in index
// order by the workgroup that draws the last ticket.  The chunk partials travel as in common.h::ordered_grid_sum: 8-byte
// device-scope (write-through) stores by lanes of wave 0, that wave's s_waitcnt vmcnt(0), ONE ticket add by its lane 0; the
// finishing workgroup reads them back with device-scope loads behind the barrier its ticket lane joined.  Counts and the
// flag are integers: LDS atomics, exact in any order.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;
constexpr int PER = XGGM_SCORE_CHUNK / NT;             // positions per lane
constexpr int MAX_R = 1 + XGGM_SCORE_MAX_GROUPS;       // sums (counts) of a chunk: all, then one per group
constexpr int MAX_W = 3 + 2 * XGGM_SCORE_MAX_GROUPS;   // words of a chunk's partial == words of the output
constexpr int TILE = 64;                               // chunk partials the finishing workgroup stages in LDS per round
constexpr int WS_HEAD = 2;                             // words in front of the partials: the ticket counter, padding
static_assert(PER * NT == XGGM_SCORE_CHUNK, "a chunk is a whole number of positions per lane");
static_assert(TILE * MAX_W <= MAX_R * NT, "the staged partials reuse the LDS of the lane sums");

struct ScoreArgs {
    const int64_t* labels;
    const int64_t* order;
    const uint8_t* keep;
    const int32_t* q_label;
    const float* q_score;
    const int32_t* q_group;
    const int64_t* cursor;
    int64_t* out;
    int64_t* ws;
    int64_t n, n_q;
    int K, G;
};

__global__ __launch_bounds__(NT) void answer_score_kernel(ScoreArgs a) {
    __shared__ double s_val[MAX_R][NT];
    __shared__ int s_cnt[MAX_R];
    __shared__ int s_flag, s_last;
    const int tid = threadIdx.x;
    const int R = 1 + a.G, W = 3 + 2 * a.G;
    for (int r = 0; r < R; ++r) s_val[r][tid] = 0.0;
    if (tid < MAX_R) s_cnt[tid] = 0;
    if (tid == 0) s_flag = 0;
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * XGGM_SCORE_CHUNK;
    int64_t lab[PER], smp[PER];
    bool in[PER], w[PER], ok[PER];
    int g[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t i = base + tid + j * NT;
        in[j] = i < a.n;
        lab[j] = in[j] ? a.labels[i] : -1;
        smp[j] = in[j] ? (a.order ? a.order[i] : i) : -1;
        w[j] = in[j] && (a.keep ? a.keep[i] != 0 : true);
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        ok[j] = in[j] && smp[j] >= 0 && smp[j] < a.n_q;
        g[j] = (ok[j] && a.q_group) ? a.q_group[smp[j]] : 0;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (ok[j] && a.q_group && (g[j] < 0 || g[j] >= a.G)) ok[j] = false;
        bad = bad || (in[j] && !ok[j]);
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {  // position order: the lane's four values are added as the header says
        if (!(ok[j] && w[j])) continue;
        const int32_t* __restrict__ ql = a.q_label + smp[j] * a.K;
        float sc = 0.f;
        for (int k = 0; k < a.K; ++k) {
            const int32_t l = ql[k];
            if (l >= 0 && (int64_t)l == lab[j]) {
                sc = a.q_score[smp[j] * a.K + k];
                break;
            }
        }
        s_val[0][tid] += (double)sc;
        atomicAdd(&s_cnt[0], 1);
        if (a.q_group) {
            s_val[1 + g[j]][tid] += (double)sc;
            atomicAdd(&s_cnt[1 + g[j]], 1);
        }
    }
    if (bad) atomicOr(&s_flag, 2);

    // halving tree over the lanes, every sum of the chunk side by side: step h writes [r][t < h] and reads [r][t + h]
    for (int h = NT / 2; h >= 1; h >>= 1) {
        __syncthreads();
        for (int idx = tid; idx < R * h; idx += NT) {
            const int r = idx / h, t = idx - r * h;
            s_val[r][t] += s_val[r][t + h];
        }
    }
    __syncthreads();

    // the chunk's partial, laid out like the output; W <= 35 lanes of wave 0 store it, lane 0 waits for the wave's stores
    // and takes the ticket
    int64_t* part = a.ws + WS_HEAD + (int64_t)blockIdx.x * W;
    if (tid < W) {
        int64_t word;
        if (tid == 0) word = s_flag;
        else if (tid <= R) word = s_cnt[tid - 1];
        else word = (int64_t)__double_as_longlong(s_val[tid - 1 - R][0]);
        __hip_atomic_store(part + tid, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) {
        unsigned* counter = reinterpret_cast<unsigned*>(a.ws);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = (t == gridDim.x - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;

    // the finishing workgroup: every chunk's partial is out.  A tile of partials at a time into LDS (coalesced device-scope
    // loads: they were written through, past the other XCDs' L2), then lane j < W adds word j of the chunks in index order.
    int64_t* tile = reinterpret_cast<int64_t*>(&s_val[0][0]);
    const int64_t C = gridDim.x;
    int64_t acc_i = 0;
    double acc_d = 0.0;
    for (int64_t c0 = 0; c0 < C; c0 += TILE) {
        const int m = C - c0 < TILE ? (int)(C - c0) : TILE;
        __syncthreads();  // the previous tile (the first round: the lane sums) has been consumed
        for (int idx = tid; idx < m * W; idx += NT)
            tile[idx] = __hip_atomic_load(a.ws + WS_HEAD + c0 * W + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tid < W) {
            for (int c = 0; c < m; ++c) {
                const int64_t x = tile[c * W + tid];
                if (tid == 0) acc_i |= x;
                else if (tid <= R) acc_i += x;
                else acc_d += __longlong_as_double((long long)x);
            }
        }
    }
    if (tid < W) {
        if (tid == 0 && a.cursor && *a.cursor != a.n) acc_i |= 1;
        a.out[tid] = tid <= R ? acc_i : (int64_t)__double_as_longlong(acc_d);
    }
    if (tid == 0)  // ready for the next launch
        __hip_atomic_store(reinterpret_cast<unsigned*>(a.ws), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline int64_t score_chunks(int64_t n) { return ceil_div64(n, XGGM_SCORE_CHUNK); }
inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
}  // namespace

extern "C" size_t xggm_answer_score_workspace_bytes(int64_t n, int G) {
    if (n < 1 || n > INT32_MAX || G < 0 || G > XGGM_SCORE_MAX_GROUPS) return 0;
    return sizeof(int64_t) * (size_t)(WS_HEAD + score_chunks(n) * (3 + 2 * G));
}

extern "C" int xggm_answer_score(const int64_t* labels, const int64_t* order, const uint8_t* keep, const int32_t* q_label,
                                 const float* q_score, const int32_t* q_group, int64_t n, int64_t n_q, int K, int G,
                                 const int64_t* cursor, int64_t* out, void* ws, size_t ws_bytes, hipStream_t st) {
    XGGM_REQUIRE(labels && q_label && q_score && out && ws, "xggm_answer_score: null labels / q_label / q_score / out / workspace");
    XGGM_REQUIRE(n >= 1 && n <= INT32_MAX, "xggm_answer_score: n = %lld outside [1, 2^31 - 1]", (long long)n);
    XGGM_REQUIRE(n_q >= 1, "xggm_answer_score: n_q = %lld, at least one sample expected", (long long)n_q);
    XGGM_REQUIRE(K >= 1, "xggm_answer_score: K = %d, at least one label slot expected", K);
    XGGM_REQUIRE(G >= 0 && G <= XGGM_SCORE_MAX_GROUPS, "xggm_answer_score: G = %d outside [0, %d]", G, XGGM_SCORE_MAX_GROUPS);
    XGGM_REQUIRE(!q_group || G > 0, "xggm_answer_score: q_group without G (the number of groups)");
    XGGM_REQUIRE(q_group || G == 0, "xggm_answer_score: G = %d without q_group", G);
    XGGM_REQUIRE(aligned(labels, 8) && aligned(order, 8) && aligned(cursor, 8) && aligned(out, 8) && aligned(ws, 8),
                 "xggm_answer_score: labels, order, cursor, out and the workspace must be 8-byte aligned");
    XGGM_REQUIRE(aligned(q_label, 4) && aligned(q_score, 4) && aligned(q_group, 4),
                 "xggm_answer_score: q_label, q_score and q_group must be 4-byte aligned");
    const size_t need = xggm_answer_score_workspace_bytes(n, G);
    XGGM_REQUIRE(ws_bytes >= need, "xggm_answer_score: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    ScoreArgs a;
    a.labels = labels, a.order = order, a.keep = keep, a.q_label = q_label, a.q_score = q_score, a.q_group = q_group;
    a.cursor = cursor, a.out = out, a.ws = static_cast<int64_t*>(ws);
    a.n = n, a.n_q = n_q, a.K = K, a.G = G;
    hipLaunchKernelGGL(answer_score_kernel, dim3((unsigned)score_chunks(n)), dim3(NT), 0, st, a);
    return xggm_check_launch("xggm_answer_score");
}
