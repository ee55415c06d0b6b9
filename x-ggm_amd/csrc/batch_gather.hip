// A training / validation batch assembled from a split that is RESIDENT on the device, in ONE launch (contract:
// xggm_batch_gather in xggm.h).  The host loop it replaces collates B items out of per-image records, converts the
// questions to ids and ships four tensors over PCIe every step (src/vqa/vqacpv2_data.py:98-127, src/vqa/vqacpv2.py:164-171).
// Output row b is built from sample s = order[start + b]; its image row is q_row[s].
// Grid (x, y) = (roles, B).  Role 0: the target row (zero-fill, barrier, scatter), the three sentence tensors and the two
// per-sample scalars.  Role 1: boxes and adjacency.  Roles 2 ..: the feature row in runs of 8 elements per lane, a 16-byte
// load or store on the bf16 side and two on the fp32 side.  Every output element has one writer (the target row: one
// workgroup, ordered by its barrier); nothing is accumulated, so there are no atomics.
#include "common.h"
#include "feat_move.h"
#include "label_adjacency.h"
#include "xggm.h"

namespace {
using feat_move::NT;
using feat_move::RUNS;
using feat_move::u4;

// LABELS: role 1 makes out_adj[b] from the image's label ids and the pair table (label_adjacency.h) instead of copying a
// stored row; every other role and output is the same code.
template <bool LABELS>
__global__ __launch_bounds__(NT) void batch_gather_kernel(const xggm_batch_gather_args a, const int adj_vec, const xggm_label_adj_args l) {
    const int64_t b = blockIdx.y;
    const int64_t s = a.order[a.start + b];
    const int role = blockIdx.x, tid = threadIdx.x;
    if (role >= 2) {
        const int64_t row = a.q_row[s];
        const int64_t runs = (int64_t)a.N * a.F / 8;  // F % 8 == 0: a row is a whole number of runs
        feat_move::move_row_any(a.feats_f32, a.out_f32,
                                reinterpret_cast<const char*>(a.feats) + row * runs * (a.feats_f32 ? 32 : 16),
                                reinterpret_cast<char*>(a.out_feats) + b * a.out_feats_stride * (a.out_f32 ? 4 : 2), runs, role - 2);
        return;
    }
    if (role == 1) {
        const int64_t row = a.q_row[s];
        // a box is one 16-byte vector
        const u4* bs = reinterpret_cast<const u4*>(a.boxes) + row * a.N;
        u4* bd = reinterpret_cast<u4*>(a.out_boxes) + b * a.N;
        for (int i = tid; i < a.N; i += NT) bd[i] = bs[i];
        if constexpr (LABELS) {
            if (a.out_adj) {  // uniform: no lane skips the helper's barriers
                __shared__ label_adj::Smem sm;
                label_adj::image<NT>(l.table, l.Vc, l.Va, l.obj_labels + row * a.N, l.attr_labels + row * a.N,
                                     a.out_adj + b * a.N * a.N, a.N, sm);
            }
        } else if (a.out_adj) {
            const int nn = a.N * a.N;
            const float* as = a.adj + row * nn;
            float* ad = a.out_adj + b * nn;
            if (adj_vec) {  // N * N % 4 == 0: rows start and end on 16-byte boundaries
                const u4* s4 = reinterpret_cast<const u4*>(as);
                u4* d4 = reinterpret_cast<u4*>(ad);
                for (int i = tid; i < nn / 4; i += NT) d4[i] = s4[i];
            } else {        // a row of N * N * 4 bytes that no vector may straddle: element by element
                for (int i = tid; i < nn; i += NT) ad[i] = as[i];
            }
        }
        return;
    }
    // role 0
    const int len = a.q_len[s];
    const int32_t* qi = a.q_ids + s * a.T;
    for (int t = tid; t < a.T; t += NT) {
        a.input_ids[b * a.T + t] = qi[t];
        a.input_mask[b * a.T + t] = t < len ? 1 : 0;
        a.segment_ids[b * a.T + t] = 0;
    }
    if (tid == 0) {
        if (a.bias_index) a.bias_index[b] = a.q_bias_index[s];
        if (a.sample) a.sample[b] = s;
    }
    if (a.target) {  // uniform: no lane skips the barrier
        // the row stride is only 4-byte aligned for the answer counts in use (2274, 29): element by element, inside [0, A)
        float* t = a.target + b * a.target_stride;
        for (int i = tid; i < a.A; i += NT) t[i] = 0.f;
        __syncthreads();  // the zeros of this row are written (and waited for) before any score lands on them
        for (int k = tid; k < a.K; k += NT) {
            const int l = a.q_label[s * a.K + k];
            if (l >= 0) t[l] = a.q_score[s * a.K + k];  // labels of a sample are distinct: one lane per element
        }
    }
}

bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p % n) != 0; }

int launch(const char* who, const xggm_batch_gather_args* args, const xggm_label_adj_args* lab, bool labels, hipStream_t st) {
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    XGGM_REQUIRE(!labels || lab, "%s: null label struct", who);
    const xggm_batch_gather_args& a = *args;
    XGGM_REQUIRE(a.B >= 1, "%s: B=%d, at least one row expected", who, a.B);
    XGGM_REQUIRE(a.T >= 1 && a.K >= 1 && a.A >= 1 && a.N >= 1 && a.F >= 1,
                 "%s: T=%d K=%d A=%d N=%d F=%d must all be positive", who, a.T, a.K, a.A, a.N, a.F);
    XGGM_REQUIRE(a.F % 8 == 0, "%s: F=%d is no multiple of 8 (feature rows move 16 bytes per lane)", who, a.F);
    XGGM_REQUIRE(a.B <= 65535, "%s: B=%d exceeds the grid's 65535 rows", who, a.B);
    XGGM_REQUIRE((int64_t)a.N * a.N < (1ll << 31) && (int64_t)a.N * a.F < (1ll << 31), "%s: N * N and N * F must stay below 2^31", who);
    XGGM_REQUIRE(a.order, "%s: null order", who);
    XGGM_REQUIRE(a.start >= 0 && a.n >= 0 && a.start + a.B <= a.n,
                 "%s: rows start=%lld .. start + B=%lld leave order[%lld]", who, (long long)a.start,
                 (long long)(a.start + a.B), (long long)a.n);
    XGGM_REQUIRE(a.feats && a.boxes && a.q_row && a.q_ids && a.q_len, "%s: null table (feats, boxes, q_row, q_ids, q_len)", who);
    XGGM_REQUIRE(a.out_feats && a.out_boxes && a.input_ids && a.input_mask && a.segment_ids,
                 "%s: null output (feats, boxes, input_ids, input_mask, segment_ids)", who);
    if (labels) {
        XGGM_REQUIRE(!a.adj, "%s: a stored adjacency table beside the label tables (one source of adj_true only)", who);
        XGGM_REQUIRE(lab->table && lab->obj_labels && lab->attr_labels, "%s: null label table (table, obj_labels, attr_labels)", who);
        XGGM_REQUIRE(lab->Vc > 0 && lab->Va > 0, "%s: Vc=%d Va=%d labels, at least one of each expected", who, lab->Vc, lab->Va);
        XGGM_REQUIRE(a.N <= label_adj::N_MAX, "%s: N = %d objects (1..%d with label tables)", who, a.N, label_adj::N_MAX);
        XGGM_REQUIRE(!misaligned(lab->table, 4) && !misaligned(lab->obj_labels, 4) && !misaligned(lab->attr_labels, 4),
                     "%s: a 4-byte label field is misaligned", who);
    } else {
        XGGM_REQUIRE(!a.out_adj || a.adj, "%s: an adjacency output needs the adjacency table", who);
    }
    XGGM_REQUIRE(!a.target || (a.q_label && a.q_score), "%s: a target output needs q_label and q_score", who);
    XGGM_REQUIRE(!a.bias_index || a.q_bias_index, "%s: a bias_index output needs q_bias_index", who);
    XGGM_REQUIRE(!misaligned(a.feats, 16) && !misaligned(a.boxes, 16) && !misaligned(a.out_feats, 16) && !misaligned(a.out_boxes, 16),
                 "%s: feats and boxes (tables and outputs) must be 16-byte aligned", who);
    XGGM_REQUIRE(a.out_feats_stride >= (int64_t)a.N * a.F && a.out_feats_stride % 8 == 0,
                 "%s: feature row stride %lld (elements) must be a multiple of 8 and at least N * F = %lld", who,
                 (long long)a.out_feats_stride, (long long)a.N * a.F);
    XGGM_REQUIRE(!a.target || a.target_stride >= a.A, "%s: target row stride %lld below A=%d", who, (long long)a.target_stride, a.A);
    XGGM_REQUIRE(!misaligned(a.adj, 4) && !misaligned(a.out_adj, 4) && !misaligned(a.target, 4) && !misaligned(a.q_score, 4) &&
                     !misaligned(a.q_row, 4) && !misaligned(a.q_ids, 4) && !misaligned(a.q_len, 4) && !misaligned(a.q_label, 4),
                 "%s: a 4-byte field is misaligned", who);
    XGGM_REQUIRE(!misaligned(a.order, 8) && !misaligned(a.q_bias_index, 8) && !misaligned(a.input_ids, 8) && !misaligned(a.input_mask, 8) &&
                     !misaligned(a.segment_ids, 8) && !misaligned(a.bias_index, 8) && !misaligned(a.sample, 8),
                 "%s: an 8-byte field is misaligned", who);
    const int64_t runs = (int64_t)a.N * a.F / 8;
    const int adj_vec = a.out_adj && ((int64_t)a.N * a.N) % 4 == 0 && !misaligned(a.adj, 16) && !misaligned(a.out_adj, 16);
    const dim3 grid((unsigned)(2 + ceil_div64(runs, NT * RUNS)), (unsigned)a.B);
    if (labels) hipLaunchKernelGGL(batch_gather_kernel<true>, grid, dim3(NT), 0, st, a, adj_vec, *lab);
    else hipLaunchKernelGGL(batch_gather_kernel<false>, grid, dim3(NT), 0, st, a, adj_vec, xggm_label_adj_args{});
    return xggm_check_launch(who);
}
}  // namespace

extern "C" int xggm_batch_gather(const xggm_batch_gather_args* args, hipStream_t st) {
    return launch("xggm_batch_gather", args, nullptr, false, st);
}

extern "C" int xggm_batch_gather_labels(const xggm_batch_gather_args* args, const xggm_label_adj_args* labels, hipStream_t st) {
    return launch("xggm_batch_gather_labels", args, labels, true, st);
}
