// A clean LXMERT pre-training batch assembled from a corpus that is RESIDENT on the device, with the matched-sentence swap
// fused in, in ONE launch (contract: xggm_pretrain_gather in xggm.h).  It replaces LXMERTTorchDataset.__getitem__
// (src/pretrain/lxmert_data.py:148-199) per example, the collation of B examples and the copies of the batch.
// Output row b is built from sample s = order[start + b]; its image row is q_row[s].
// Grid (x, y) = (roles, B).  Role 0: the swap decision of the row (wave-uniform: every draw and every looked-up image row
// goes through readfirstlane, as in pretrain_swap.hip) and every small field.  Roles 1 ..: the feature row in runs of 8
// elements per lane (feat_move.h, shared with batch_gather.hip).  Every output element has one writer; the only atomic is
// the integer add of a row whose candidates were all of its own image.
#include "common.h"
#include "feat_move.h"
#include "xggm.h"

namespace {
using feat_move::NT;
using feat_move::RUNS;
using feat_move::u4;

__device__ __forceinline__ float uniform_lane(float v) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
// draw `k` (5: u_swap, 6: u_pick) of element idx: the supplied buffer, else Philox stream sid_base + k
__device__ __forceinline__ float draw_of(const float* buf, const xggm_pretrain_gather_args& a, uint32_t k, uint64_t idx) {
    if (buf) return uniform_lane(buf[idx]);
    return uniform_lane(philox_uniform(a.rng[0], a.rng[1], a.sid_base + k, idx));
}
// floor(u * n) in double, held inside [0, n): a supplied draw outside [0, 1) must not become an address
__device__ __forceinline__ int64_t pick_of(float u, int64_t n) {
    const double v = (double)u * (double)n;
    int64_t i = v >= 0.0 ? (int64_t)v : 0;
    return i > n - 1 ? n - 1 : i;
}

__global__ __launch_bounds__(NT) void pretrain_gather_kernel(const xggm_pretrain_gather_args a) {
    const int64_t b = blockIdx.y;
    const int64_t s = a.order[a.start + b];
    const int role = blockIdx.x, tid = threadIdx.x;
    const int own = __builtin_amdgcn_readfirstlane(a.q_row[s]);
    if (role >= 1) {
        const int64_t runs = (int64_t)a.O * a.F / 8;  // F % 8 == 0: a row is a whole number of runs
        feat_move::move_row_any(a.feats_f32, a.out_f32,
                                reinterpret_cast<const char*>(a.feats) + own * runs * (a.feats_f32 ? 32 : 16),
                                reinterpret_cast<char*>(a.out_feats) + b * a.out_feats_stride * (a.out_f32 ? 4 : 2), runs, role - 1);
        return;
    }
    // role 0: the decision (src/pretrain/lxmert_data.py:178-183), the same in every lane of every wave
    int64_t sent = s, matched = 1, from = -1;
    if (a.swap && (double)draw_of(a.u_swap, a, 5, (uint64_t)b) < a.rate) {
        bool found = false;
        for (int r = 0; r < XGGM_PRETRAIN_SWAP_TRIES && !found; ++r) {
            const int64_t j = pick_of(draw_of(a.u_pick, a, 6, (uint64_t)b * XGGM_PRETRAIN_SWAP_TRIES + r), a.n_q);
            if (__builtin_amdgcn_readfirstlane(a.q_row[j]) != own) {
                found = true;
                matched = 0;
                sent = from = j;
            }
        }
        if (!found && tid == 0) atomicAdd(a.exhausted, 1);
    }
    // the sentence: rows of T elements, element by element inside [0, T)
    const int len = a.q_len[sent];
    const int32_t* qi = a.q_ids + sent * a.T;
    for (int t = tid; t < a.T; t += NT) {
        a.input_ids[b * a.T + t] = qi[t];
        a.input_mask[b * a.T + t] = t < len ? 1 : 0;
        a.segment_ids[b * a.T + t] = 0;
    }
    // the answer keys of the sample itself
    for (int k = tid; k < a.K; k += NT) {
        a.label_ids[b * a.K + k] = a.q_label[s * a.K + k];
        a.label_scores[b * a.K + k] = a.q_score[s * a.K + k];
    }
    // the per-object fields of the image; a box is one 16-byte vector
    const int64_t io = (int64_t)own * a.O, bo = b * a.O;
    const u4* bs = reinterpret_cast<const u4*>(a.boxes) + io;
    u4* bd = reinterpret_cast<u4*>(a.out_boxes) + bo;
    for (int o = tid; o < a.O; o += NT) {
        bd[o] = bs[o];
        a.out_obj_labels[bo + o] = a.obj_labels[io + o];
        a.out_attr_labels[bo + o] = a.attr_labels[io + o];
        a.out_obj_confs[bo + o] = a.obj_confs[io + o];
        a.out_attr_confs[bo + o] = a.attr_confs[io + o];
    }
    if (tid == 0) {
        a.is_matched[b] = matched;
        a.img_ids[b] = own;
        if (a.sample) a.sample[b] = s;
        if (a.swapped_from) a.swapped_from[b] = from;
    }
}

bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p % n) != 0; }
bool overlaps(const void* p, int64_t np, const void* q, int64_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}
struct Span {
    const void* p;
    int64_t bytes;
};
}  // namespace

extern "C" int xggm_pretrain_gather(const xggm_pretrain_gather_args* args, hipStream_t st) {
    const char* who = "xggm_pretrain_gather";
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    const xggm_pretrain_gather_args& a = *args;
    XGGM_REQUIRE(a.B >= 1, "%s: B=%d, at least one row expected", who, a.B);
    XGGM_REQUIRE(a.B <= 65535, "%s: B=%d exceeds the grid's 65535 rows", who, a.B);
    XGGM_REQUIRE(a.T >= 1 && a.K >= 1 && a.O >= 1 && a.F >= 1 && a.n_img >= 1 && a.n_q >= 1,
                 "%s: T=%d K=%d O=%d F=%d n_img=%lld n_q=%lld must all be positive", who, a.T, a.K, a.O, a.F,
                 (long long)a.n_img, (long long)a.n_q);
    XGGM_REQUIRE(a.F % 8 == 0, "%s: F=%d is no multiple of 8 (feature rows move 16 bytes per lane)", who, a.F);
    XGGM_REQUIRE((int64_t)a.O * a.F < (1ll << 31) && a.n_img < (1ll << 31), "%s: O * F and n_img must stay below 2^31", who);
    XGGM_REQUIRE(a.order, "%s: null order", who);
    XGGM_REQUIRE(a.start >= 0 && a.n >= 0 && a.start + a.B <= a.n, "%s: rows start=%lld .. start + B=%lld leave order[%lld]",
                 who, (long long)a.start, (long long)(a.start + a.B), (long long)a.n);
    XGGM_REQUIRE(a.feats && a.boxes && a.obj_labels && a.attr_labels && a.obj_confs && a.attr_confs,
                 "%s: null image table (feats, boxes, obj_labels, attr_labels, obj_confs, attr_confs)", who);
    XGGM_REQUIRE(a.q_row && a.q_ids && a.q_len && a.q_label && a.q_score,
                 "%s: null sample table (q_row, q_ids, q_len, q_label, q_score)", who);
    XGGM_REQUIRE(a.out_feats && a.out_boxes && a.out_obj_labels && a.out_attr_labels && a.out_obj_confs && a.out_attr_confs &&
                     a.input_ids && a.input_mask && a.segment_ids && a.label_ids && a.label_scores && a.is_matched && a.img_ids,
                 "%s: null output (only sample and swapped_from may be left out)", who);
    XGGM_REQUIRE(!misaligned(a.feats, 16) && !misaligned(a.boxes, 16) && !misaligned(a.out_feats, 16) && !misaligned(a.out_boxes, 16),
                 "%s: feats and boxes (tables and outputs) must be 16-byte aligned", who);
    XGGM_REQUIRE(a.out_feats_stride >= (int64_t)a.O * a.F && a.out_feats_stride % 8 == 0,
                 "%s: feature row stride %lld (elements) must be a multiple of 8 and at least O * F = %lld", who,
                 (long long)a.out_feats_stride, (long long)a.O * a.F);
    XGGM_REQUIRE(!misaligned(a.obj_labels, 4) && !misaligned(a.attr_labels, 4) && !misaligned(a.obj_confs, 4) && !misaligned(a.attr_confs, 4) &&
                     !misaligned(a.q_row, 4) && !misaligned(a.q_ids, 4) && !misaligned(a.q_len, 4) && !misaligned(a.q_label, 4) &&
                     !misaligned(a.q_score, 4) && !misaligned(a.out_obj_confs, 4) && !misaligned(a.out_attr_confs, 4) &&
                     !misaligned(a.label_scores, 4) && !misaligned(a.u_swap, 4) && !misaligned(a.u_pick, 4) && !misaligned(a.exhausted, 4),
                 "%s: a 4-byte field is misaligned", who);
    XGGM_REQUIRE(!misaligned(a.order, 8) && !misaligned(a.out_obj_labels, 8) && !misaligned(a.out_attr_labels, 8) &&
                     !misaligned(a.input_ids, 8) && !misaligned(a.input_mask, 8) && !misaligned(a.segment_ids, 8) &&
                     !misaligned(a.label_ids, 8) && !misaligned(a.is_matched, 8) && !misaligned(a.img_ids, 8) &&
                     !misaligned(a.sample, 8) && !misaligned(a.swapped_from, 8) && !misaligned(a.rng, 8),
                 "%s: an 8-byte field is misaligned", who);
    if (a.swap) {
        XGGM_REQUIRE(a.rate >= 0.0 && a.rate <= 1.0, "%s: rate %g outside [0, 1]", who, a.rate);
        XGGM_REQUIRE(a.exhausted, "%s: a swap needs the exhausted counter", who);
        XGGM_REQUIRE(a.rng || (a.u_swap && a.u_pick), "%s: a null draw buffer needs rng", who);
    }
    // every output against everything the launch reads and against every other output: rows are written while other
    // workgroups still read the tables, and two outputs that share bytes would overwrite each other
    const int64_t B = a.B, esz_in = a.feats_f32 ? 4 : 2, esz_out = a.out_f32 ? 4 : 2, OF = (int64_t)a.O * a.F;
    const int64_t bo = B * a.O, bt = B * a.T, bk = B * a.K;
    const Span outs[] = {{a.out_feats, ((B - 1) * a.out_feats_stride + OF) * esz_out}, {a.out_boxes, bo * 16},
                         {a.out_obj_labels, bo * 8}, {a.out_attr_labels, bo * 8}, {a.out_obj_confs, bo * 4}, {a.out_attr_confs, bo * 4},
                         {a.input_ids, bt * 8}, {a.input_mask, bt * 8}, {a.segment_ids, bt * 8}, {a.label_ids, bk * 8},
                         {a.label_scores, bk * 4}, {a.is_matched, B * 8}, {a.img_ids, B * 8}, {a.sample, B * 8},
                         {a.swapped_from, B * 8}, {a.swap ? a.exhausted : nullptr, 4}};
    const int64_t io = a.n_img * a.O;
    const Span ins[] = {{a.feats, a.n_img * OF * esz_in}, {a.boxes, io * 16}, {a.obj_labels, io * 4}, {a.attr_labels, io * 4},
                        {a.obj_confs, io * 4}, {a.attr_confs, io * 4}, {a.q_row, a.n_q * 4}, {a.q_ids, a.n_q * a.T * 4},
                        {a.q_len, a.n_q * 4}, {a.q_label, a.n_q * a.K * 4}, {a.q_score, a.n_q * a.K * 4}, {a.order, a.n * 8},
                        {a.swap ? (const void*)a.rng : nullptr, 16}, {a.swap ? a.u_swap : nullptr, B * 4},
                        {a.swap ? a.u_pick : nullptr, B * XGGM_PRETRAIN_SWAP_TRIES * 4}};
    const int n_out = sizeof(outs) / sizeof(outs[0]), n_in = sizeof(ins) / sizeof(ins[0]);
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o].p) continue;
        for (int i = 0; i < n_in; ++i)
            XGGM_REQUIRE(!ins[i].p || !overlaps(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes),
                         "%s: an output aliases a table, order, rng or a draw buffer", who);
        for (int q = o + 1; q < n_out; ++q)
            XGGM_REQUIRE(!outs[q].p || !overlaps(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes),
                         "%s: two outputs alias each other", who);
    }
    const int64_t runs = OF / 8;
    const dim3 grid((unsigned)(1 + ceil_div64(runs, NT * RUNS)), (unsigned)a.B);
    hipLaunchKernelGGL(pretrain_gather_kernel, grid, dim3(NT), 0, st, a);
    return xggm_check_launch(who);
}
