// The STAGED SGD step (gfx950 / MI355X).
//
// Reference semantics: the same batch-synchronous step as bpr_train.hip
//   loader    daisy/utils/dataset.py:5-27          forward   daisy/model/MFRecommender.py:63-68
//   loss      MFRecommender.py:70-97, loss.py:5-33 backward  AbstractRecommender.py:125
//   SGD       AbstractRecommender.py:56,126
//
// Why a second organisation of the step.  The phase kernels of bpr_train.hip move 8.3 table rows per
// interaction (k_fwd 3, item pass 2 + a random 8-byte coefficient gather per entry that costs a full
// 128-byte fabric request, user pass 3.3) and the PMC counters say every one of them already runs at the
// fabric rate for the bytes it moves (profiles/r01_*): the lever left is FEWER BYTES.  Here:
//
//   k_unorm          sum over the batch of |P[u]|^2 from a per-row cache (4 B / sample): the one batch-wide
//                    quantity the user update needs BEFORE it runs (reg_2 * p / |P[u]|_F, MFRecommender.py:94)
//   k_staged_user    forward + user update in ONE pass over the user-grouped samples: gathers p_u, q_i, q_j
//                    once, forms both scores, the loss term and c = dL/dx, accumulates the seven batch sums,
//                    updates P[u] in place (single owner per row, run/slot/edge reduction like bpr_train.hip)
//                    and writes m_s = c_s * p_u(pre-step) to stage[slot(s)]: one 256-B row per sample
//   k_staged_item    segmented reduction over the item-sorted entries: gQ[i] = sum_e (+/-) m_{s(e)} - the
//                    coefficient rides inside the staged row, so an entry costs ONE row gather and no
//                    coefficient gather; the segment's owner then applies regulariser + SGD to Q[i] IN PLACE
//                    (no gQ round trip, no run lists, no separate apply pass).  Multi-GPU: writes the data
//                    term + (n_pos, n_neg) per item instead, for a reduce-scatter.
//
// Row traffic per interaction at d=64:  user pass 2 Q rows + 0.43 P rows read, 0.43 P rows + 1 stage row
// written; item pass 2 stage rows read (+ the touched Q rows once) = ~1.5 KB instead of ~2.1 KB.
// (BPR / HL have dL/dneg = -dL/dpos, so one premultiplied row serves both entries of a sample; TOP1 keeps
// the plain row in the stage and gathers its two coefficients.)
//
// Either layout of the epoch plan (epoch_plan.hip) feeds the step through a StreamView.
//
// This file: staged_path - what a call runs, decided once -, the SGD and Adam step drivers, the Adam catch-up and the
// C ABI.  The kernels of the two passes and their launchers: bpr_staged_user.hip, bpr_staged_item.hip; what the three
// share: bpr_staged.h.
#include <math.h>
#include <stdlib.h>

#include "bpr_staged.h"

namespace daisy {

constexpr size_t kStreamTableBytes = (size_t)512 << 20;   // user tables beyond this are read past the caches (k_staged_user)

// the staged step covers every loss of the reference (loss.py:5-33, MFRecommender.py:70-97): the point-wise ones
// need a point-wise batch (rows (user, item, label)) and vice versa; FM biases ride on the plain / point flavours
bool staged_supported(const daisy_bpr_ctx *ctx, int loss_type) {
    if (loss_type < DAISY_LOSS_BPR || loss_type > DAISY_LOSS_SL) return false;
    return (loss_type >= DAISY_LOSS_CL) == (ctx->sv.pointwise != 0);
}

static inline bool premul_loss(int loss_type) { return loss_type == DAISY_LOSS_BPR || loss_type == DAISY_LOSS_HL; }

// flavour of the two passes (k_staged_user): FM's pairwise runs take the plain one (its item biases need the bare
// coefficients)
static int staged_mode(const daisy_bpr_ctx *ctx, int loss_type) {
    if (loss_type >= DAISY_LOSS_CL) return kModePoint;
    return (premul_loss(loss_type) && !ctx->bu) ? kModePremul : kModePlain;
}

static StagedAdam adam_consts(float lr, float beta1, float beta2, float eps, int64_t step) {
    StagedAdam a{};
    // step `step`'s constants: the host arithmetic of daisy_adam_dense / daisy_adam_lazy_table (same bits as table[step])
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    a.step_size = (float)((double)lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.t = (int32_t)step;
    return a;
}

// The pre-norm pass over a batch of B samples: its workgroups, and whether its consumers add the partial sums themselves.
// Batches up to kPreBlocks / 2 workgroups of pre-norm work: they do (one launch less; what bounds a step of that size).
// Larger ones: a full grid and a reduction - every workgroup of the user pass re-adding thousands of partial sums
// measured slower than the launch it saves.
static inline int prenorm_grid(int64_t B) { return grid_for(B, kBlock * 4); }
static inline bool prenorm_folds(int gn) { return gn <= kPreBlocks / 2; }

// What a call runs - the one place that decides, and the only one in the staged translation units that reads the
// environment.  Once per process: DAISY_STAGED_UGRID / _IGRID (grid caps of the two passes; IGRID 0: 16 384 x 256
// threads), DAISY_STAGED_RIDE (0: the next batch's pre-norm never rides).  Per call, because the tests switch them:
// DAISY_STAGED_SPARSE (0 / 1 force the dense / sparse flavour of the SGD item pass), DAISY_EDGE_BLOCKS (edge chains in
// two levels: 0 never, 1 always), DAISY_STAGED_MERGE (three-launch form: 0 never, 1 whenever the buffers allow it).
// parts: kStagedUser / kStagedItem - one phase of a multi-GPU step - or kStagedStep.  P: the user table of a whole step.
static int staged_path(const daisy_bpr_ctx *ctx, const char *who, const StagedStep &st, int parts, const float *P, bool apply,
                       int slice, StagedPath *out) {
    auto knob = [](const char *name, int unset) { const char *env = getenv(name); return env ? atoi(env) : unset; };
    static const int tune_ug = knob("DAISY_STAGED_UGRID", kMaxGrid), tune_ig = knob("DAISY_STAGED_IGRID", 0),
                     tune_ride = knob("DAISY_STAGED_RIDE", 1);
    if (!ctx->batch_set) { set_error("%s: no batch set", who); return DAISY_ERR_STATE; }
    if (st.loss_type < DAISY_LOSS_BPR || st.loss_type > DAISY_LOSS_SL) {
        set_error("Invalid loss type: %d", st.loss_type);
        return DAISY_ERR_ARG;
    }
    if (!staged_supported(ctx, st.loss_type)) {
        set_error("%s: loss type %d does not match the batch layout (point-wise=%d)", who, st.loss_type, ctx->sv.pointwise);
        return DAISY_ERR_ARG;
    }
    if (st.adam && !apply) { set_error("staged item pass: the Adam owner update needs the in-place form"); return DAISY_ERR_ARG; }
    const StreamView &v = ctx->sv;
    const daisy_epoch_plan *pl = ctx->cur_plan;
    StagedPath q{};
    q.mode = staged_mode(ctx, st.loss_type);
    q.has_pos = v.s_rec != nullptr;
    q.p_stream = (ctx->p_stream_mode >= 0) ? (ctx->p_stream_mode != 0) : ((size_t)ctx->U * (size_t)ctx->d * 4 > kStreamTableBytes);
    q.adam = st.adam != nullptr; q.apply = apply; q.fused = parts == kStagedStep; q.slice = slice;
    // Four launches inside an SGD epoch: user pass, its edges (+ the reduction of its sums), item pass (+ the NEXT batch's
    // pre-norm partial sums, when it comes from the same partitioned plan), its edges (+ their reduction).  A step for
    // which nothing rode - the first of an epoch, every Adam step (its catch-up changes the rows first) - computes its
    // own pre-norm first
    if (q.fused) {
        q.ride = !q.adam && tune_ride && pl && pl->kind == 1 && ctx->cur_gen == pl->build_gen && ctx->cur_k + 1 < pl->num_batches &&
                 daisy_epoch_plan_batch_rows(pl, ctx->cur_k + 1) > 0;
        if (q.ride) { q.gn = prenorm_grid(plan_stream_view(pl, ctx->cur_k + 1).B); q.ride_fold = prenorm_folds(q.gn); }
        const bool have_pre = !q.adam && ctx->pre_ready && pl && ctx->pre_plan == pl && ctx->pre_k == ctx->cur_k &&
                              ctx->pre_gen == ctx->cur_gen && ctx->cur_gen == pl->build_gen && ctx->pre_P == P &&
                              ctx->p_sqnorm_of == P && (ctx->pre_n > 0 || ctx->pre_stats == st.stats);
        q.pre_own = !have_pre;
        q.gp = prenorm_grid(v.B);
        q.n_pre = have_pre ? ctx->pre_n : (prenorm_folds(q.gp) ? q.gp : 0);
    }
    bool overflow = false;
    int rc = dispatch_d(ctx->d, [&](auto cfg) {
        using C = decltype(cfg);
        if (parts & kStagedUser) {
            q.u_blk = StagedUserBlk<C>::value;
            constexpr int E = StagedUserCfg<C, StagedUserBlk<C>::value>::E;
            q.u_chunks = (v.B + E - 1) / E;
            overflow = q.u_chunks > ctx->edge_chunks;
            q.gu = grid_for(q.u_chunks, 1, tune_ug < kMaxGrid ? tune_ug : kMaxGrid);
            q.n_ue = grid_for(q.u_chunks, C::GROUPS_PER_BLOCK);
        }
        // THREE launches (MergedJob) for SGD batches whose user pass leaves at most kMergeMaxPartials rows of partial sums
        // (every item workgroup adds them itself): B <= 32768 at d = 64.  (Round 5, same box, four vs three launches: B =
        // 32 768 - 1024 rows of partial sums - 36.9 -> 33.4 us per step; B = 65 536 - 2048 rows - 51.6 -> 58.6, and with the
        // user pass capped at 1024 workgroups a tie: profiles/r05_mid_matrix.txt)
        constexpr int kMergeMaxPartials = 1024;
        if (q.fused && !q.adam) {
            const int tune_merge = knob("DAISY_STAGED_MERGE", -1);
            q.merge = tune_merge != 0 && ctx->edge2_vec != nullptr && v.B <= kMergeMaxBatch && (!q.ride || q.ride_fold) &&
                      (tune_merge > 0 || q.gu <= kMergeMaxPartials);
        }
        if (!(parts & kStagedItem)) return DAISY_OK;
        // (the three-launch form is written for 256-thread workgroups)
        q.i_blk = q.merge ? kBlock : kStagedItemBlock;
        const int E_dense = q.merge ? StagedItemCfg<C, kBlock>::E : StagedItemCfg<C, kStagedItemBlock>::E;
        const int E_sparse = q.merge ? StagedItemCfg<C, kBlock, true>::E : StagedItemCfg<C, kStagedItemBlock, true>::E;
        // the sparse flavour (StagedItemCfg) when a dense chunk's item range would not fit the LDS window: expected
        // items under a chunk = chunk entries x items / entries  >  rows of the window
        const int win_rows = (kItemWinFloats * q.i_blk / kBlock) / (C::NE * C::LPR);
        const int tune_sparse = knob("DAISY_STAGED_SPARSE", -1);
        q.sparse = apply && !q.adam && (tune_sparse >= 0 ? tune_sparse != 0 : (double)v.E * win_rows < (double)E_dense * (double)ctx->I);
        q.i_chunk = q.sparse ? E_sparse : E_dense;
        q.i_chunks = (v.E + q.i_chunk - 1) / q.i_chunk;
        overflow = overflow || q.i_chunks > (q.merge ? ctx->edge2_chunks : ctx->edge_chunks);
        q.gi = grid_for(v.E, q.i_chunk, tune_ig > 0 ? tune_ig : 16384 * kBlock / q.i_blk);
        q.n_ie = grid_for(q.i_chunks, C::GROUPS_PER_BLOCK);
        // Edge chains in two levels when the batch can hold a segment of 16 chunks or more: the hottest item's share of
        // the set (the index counted it) x the batch's entries, with room for its fluctuation; unknown - a batch that did
        // not come from a partitioned plan - means a large batch
        const double hot = (ctx->batch_kind == 1 && pl) ? pl->hot_item_share * (double)v.E : -1.0;
        const char *env_eb = getenv("DAISY_EDGE_BLOCKS");       // (set: any value but 0 is "always")
        q.two_level = !q.merge && q.i_chunks / kEdgeBlock + 2 <= ctx->eb_blocks &&
                      (env_eb ? atoi(env_eb) != 0
                                : (hot >= 0.0 ? (hot + 4.0 * sqrt(hot) >= 16.0 * q.i_chunk) : q.i_chunks >= 64 * kEdgeBlock));
        return DAISY_OK;
    });
    if (rc) return rc;
    if (overflow) { set_error("staged step: the batch needs more edge records than the context holds"); return DAISY_ERR_STATE; }
    *out = q;
    return DAISY_OK;
}

int staged_sgd_step(daisy_bpr_ctx *ctx, float *P, float *Q, int loss_type, float gamma, float lr, float reg_1,
                    float reg_2, double *stats, double *epoch_acc, double *step_loss, hipStream_t s) {
    const StagedStep st{loss_type, gamma, lr, reg_1, reg_2, stats, epoch_acc, step_loss, nullptr, false, s};
    StagedPath path;
    int rc = staged_path(ctx, "sgd_step", st, kStagedStep, P, true, -1, &path);
    if (rc) return rc;
    ctx->pre_ready = false;                  // consumed, or stale
    if (path.pre_own && (rc = staged_prenorm(ctx, P, stats, path.gp, path.n_pre > 0, s))) return rc;
    if ((rc = staged_user(ctx, path, st, P, Q))) return rc;
    if (path.ride) {                         // what the next step of the same plan will find waiting
        ctx->pre_plan = ctx->cur_plan; ctx->pre_k = ctx->cur_k + 1; ctx->pre_gen = ctx->cur_gen;
        ctx->pre_P = P; ctx->pre_stats = stats; ctx->pre_n = path.ride_fold ? path.gn : 0;
    }
    if ((rc = staged_item(ctx, path, st, P, Q, nullptr))) return rc;
    ctx->pre_ready = path.ride;
    ctx->fwd_done = false;
    return DAISY_OK;
}

// ---- lazy Adam on the staged step ------------------------------------------------------------------------
// Rows a batch references are brought to step t-1 before its forward pass (the zero-gradient replay of
// adam_claim_row, adam_lazy.hip).  Samples are grouped by user and entries sorted by item, so the first record of a
// run of equal ids is the row's single owner: no atomics.  The user side also refreshes the row-norm cache.
template <class C>
__global__ __launch_bounds__(kBlock) void k_staged_adam_catchup(StreamView v, int d, float *__restrict__ P,
                                                                float *__restrict__ Q, StagedAdam a,
                                                                const float2 *__restrict__ table,
                                                                float *__restrict__ p_sqnorm, int users_only) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR, group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const int64_t total = users_only ? v.B : v.B + v.E;
    for (int64_t x = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; x < total; x += gstride) {
        const bool user_side = x < v.B;
        int64_t row;
        if (user_side) {
            row = (int64_t)sv_user(v, x);
            if (x > 0 && (int64_t)sv_user(v, x - 1) == row) continue;
        } else {
            const int64_t e = x - v.B;
            row = (int64_t)(sv_key(v, e) >> 1);
            if (e > 0 && (int64_t)(sv_key(v, e - 1) >> 1) == row) continue;
        }
        float *W = user_side ? P : Q, *M = user_side ? a.mP : a.mQ, *V = user_side ? a.vP : a.vQ;
        int32_t *last = user_side ? a.lastP : a.lastQ;
        const int32_t old = last[row];
        if (old >= a.t - 1) continue;
        Row<C> w, m, vv, g;
        w.load(W + row * d, lane, d); m.load(M + row * d, lane, d); vv.load(V + row * d, lane, d);
        g.zero();
        for (int32_t st = old + 1; st < a.t; ++st) {                  // zero-gradient steps old+1 .. t-1
            const float2 c = table[st];
            adam_row<C>(w, m, vv, g, c.x, c.y, a.beta1, a.beta2, a.eps);
        }
        // (Round 4, measured and rejected - profiles/r04_bench_adam_fused_catchup_rejected.txt, r04_adam_prefetch_ab.txt:
        // NOT writing the users back and replaying the same steps in the user pass, which then gathers each sample's
        // moments - three row transfers per stale user less, but the replay is ~60 VALU cycles per element and step
        // (sqrt, two divides) and doing it twice cost more than the traffic: 2.80 -> 3.62 ms per step at 10 M x 1 M.
        // Gathering the moments with the rows WITHOUT the replay, so that a run's owner commits from registers: no
        // change either way (1.293 / 1.291 and 3.032 / 3.039 ms, same box) at 180 instead of 161 VGPRs.)
        w.store(W + row * d, lane, d); m.store(M + row * d, lane, d); vv.store(V + row * d, lane, d);
        if (lane == 0) last[row] = a.t - 1;
        if (user_side) {
            const float sq = row_dot<C>(w, w);
            if (lane == 0) p_sqnorm[row] = sq;
        }
    }
}

int staged_adam_step(daisy_bpr_ctx *ctx, float *P, float *Q, int loss_type, float gamma, float reg_1, float reg_2,
                     const StagedAdam &a, const float *table, bool bias_grad_out, double *stats, double *epoch_acc,
                     double *step_loss, hipStream_t s) {
    const StagedStep st{loss_type, gamma, 0.f, reg_1, reg_2, stats, epoch_acc, step_loss, &a, bias_grad_out, s};
    StagedPath path;
    int rc = staged_path(ctx, "staged_adam_step", st, kStagedStep, P, true, -1, &path);
    if (rc) return rc;
    const StreamView &v = ctx->sv;
    const int d = ctx->d;
    // the row-norm cache has to exist before the catch-up refreshes the rows it changes
    if ((rc = staged_norm_cache(ctx, P, s))) return rc;
    rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((k_staged_adam_catchup<C>), dim3(grid_for(v.B + v.E, C::GROUPS_PER_BLOCK, kMaxGridSparse)),
                           dim3(kBlock), 0, s, v, d, P, Q, a, reinterpret_cast<const float2 *>(table), ctx->p_sqnorm, 0);
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    if ((rc = staged_prenorm(ctx, P, stats, path.gp, path.n_pre > 0, s))) return rc;
    if ((rc = staged_user(ctx, path, st, P, Q))) return rc;
    if ((rc = staged_item(ctx, path, st, P, Q, nullptr))) return rc;
    ctx->fwd_done = false;
    return DAISY_OK;
}

}  // namespace daisy

using namespace daisy;

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

int daisy_bpr_ctx_invalidate_cache(daisy_bpr_ctx *ctx) {
    DAISY_CHECK_ARG(ctx != nullptr, "ctx_invalidate_cache: NULL context");
    ctx->p_sqnorm_of = nullptr;
    ctx->pre_ready = false;       // the next batch's pre-norm that rode on the last item pass was summed from the old cache
    return DAISY_OK;
}

int daisy_bpr_ctx_set_p_stream(daisy_bpr_ctx *ctx, int32_t mode) {
    DAISY_CHECK_ARG(ctx != nullptr, "ctx_set_p_stream: NULL context");
    DAISY_CHECK_ARG(mode >= -1 && mode <= 1, "ctx_set_p_stream: mode %d not in -1 (automatic), 0, 1", mode);
    ctx->p_stream_mode = mode;
    return DAISY_OK;
}

int daisy_bpr_staged_prenorm(daisy_bpr_ctx *ctx, const float *P, double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && stats, "staged_prenorm: NULL argument");
    if (!ctx->batch_set) { set_error("staged_prenorm: no batch set"); return DAISY_ERR_STATE; }
    return staged_prenorm(ctx, P, stats, prenorm_grid(ctx->sv.B), false, as_stream(stream));     // (the ranks all-reduce the sum)
}

// the user pass of a multi-GPU step, SGD (adam == nullptr) or Adam; the caller all-reduces the reduced sums
static int staged_user_phase(daisy_bpr_ctx *ctx, const char *who, float *P, const float *Q, const StagedStep &st) {
    StagedPath path;
    int rc = staged_path(ctx, who, st, kStagedUser, nullptr, true, -1, &path);
    if (rc) return rc;
    if (ctx->p_sqnorm_of != P) {
        set_error("%s: daisy_bpr_staged_prenorm has not run on this table", who);
        return DAISY_ERR_STATE;
    }
    if (st.adam && ctx->bu) { set_error("%s: contexts with FM biases are not supported by the phase form", who); return DAISY_ERR_ARG; }
    if ((rc = staged_user(ctx, path, st, P, Q))) return rc;
    return launch_reduce_partials(ctx->partials, path.gu, st.stats, false, 0.f, 0.f, nullptr, nullptr, st.s);
}

int daisy_bpr_staged_user(daisy_bpr_ctx *ctx, float *P, const float *Q, int32_t loss_type, float gamma, float lr,
                          float reg_1, float reg_2, double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats, "staged_user: NULL argument");
    return staged_user_phase(ctx, "staged_user", P, Q,
                             StagedStep{loss_type, gamma, lr, reg_1, reg_2, stats, nullptr, nullptr, nullptr, false, as_stream(stream)});
}

// the item pass of a multi-GPU step (slice < 0: the whole batch): in place on Q, or the data term + counts to gQ / cnt
static int staged_item_phase(daisy_bpr_ctx *ctx, const char *who, int loss_type, float *Qo, float *cnt, bool apply, int slice,
                             float lr, float reg_1, float reg_2, const double *stats, daisy_stream_t stream) {
    // (the item pass only reads the stats)
    const StagedStep st{loss_type, 0.f, lr, reg_1, reg_2, const_cast<double *>(stats), nullptr, nullptr, nullptr, false, as_stream(stream)};
    StagedPath path;
    int rc = staged_path(ctx, who, st, kStagedItem, nullptr, apply, slice, &path);
    if (rc) return rc;
    return staged_item(ctx, path, st, nullptr, Qo, cnt);
}

int daisy_bpr_staged_item(daisy_bpr_ctx *ctx, int32_t loss_type, float *Q, float *gQ, float *cnt, float lr,
                          float reg_1, float reg_2, const double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && stats && ((Q && !gQ) || (!Q && gQ && cnt)),
                    "staged_item: give either Q (apply in place) or gQ + cnt (gradient output)");
    return staged_item_phase(ctx, "staged_item", loss_type, Q ? Q : gQ, cnt, Q != nullptr, -1, lr, reg_1, reg_2, stats, stream);
}

int daisy_bpr_staged_item_slices(daisy_bpr_ctx *ctx, const int32_t *item_bounds, int32_t n_slices, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && item_bounds && n_slices >= 1 && n_slices <= kMaxItemSlices,
                    "staged_item_slices: 1..%d slices", kMaxItemSlices);
    if (!ctx->batch_set) { set_error("staged_item_slices: no batch set"); return DAISY_ERR_STATE; }
    for (int k = 0; k <= n_slices; ++k)
        DAISY_CHECK_ARG(item_bounds[k] >= 0 && (k == 0 || item_bounds[k] >= item_bounds[k - 1]),
                        "staged_item_slices: the item bounds must not decrease");
    DAISY_CHECK_ARG(item_bounds[0] == 0 && item_bounds[n_slices] >= ctx->I,
                    "staged_item_slices: the slices must cover the items 0..%lld", (long long)ctx->I);
    if (int rc = staged_slice_ranges(ctx, item_bounds, n_slices, as_stream(stream))) return rc;
    ctx->n_slices = n_slices;
    return DAISY_OK;
}

int daisy_bpr_staged_item_slice(daisy_bpr_ctx *ctx, int32_t loss_type, float *gQ, float *cnt, int32_t slice, float lr,
                                float reg_1, float reg_2, const double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && gQ && cnt && stats, "staged_item_slice: NULL argument");
    DAISY_CHECK_ARG(slice >= 0 && slice < ctx->n_slices, "staged_item_slice: slice %d of %d (daisy_bpr_staged_item_slices first)",
                    slice, ctx->n_slices);
    return staged_item_phase(ctx, "staged_item_slice", loss_type, gQ, cnt, false, slice, lr, reg_1, reg_2, stats, stream);
}

int daisy_bpr_staged_adam_step(daisy_bpr_ctx *ctx, float *P, float *Q, int32_t loss_type, float gamma, float lr,
                               float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP, float *mQ, float *vQ,
                               int32_t *lastQ, const float *table, float beta1, float beta2, float eps, int64_t step,
                               double *stats, double *epoch_acc, double *step_loss, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && mP && vP && lastP && mQ && vQ && lastQ && table && stats && step >= 1,
                    "staged_adam_step: bad argument");
    StagedAdam a = adam_consts(lr, beta1, beta2, eps, step);
    a.mP = mP; a.vP = vP; a.lastP = lastP; a.mQ = mQ; a.vQ = vQ; a.lastQ = lastQ;
    struct HaltScope {
        daisy_bpr_ctx *c;
        HaltScope(daisy_bpr_ctx *c_, const double *h) : c(c_) { c->v.halt = h; c->sv.halt = h; }
        ~HaltScope() { c->v.halt = nullptr; c->sv.halt = nullptr; }
    } halt_scope(ctx, epoch_acc ? epoch_acc + 1 : nullptr);
    const bool bias_grad_out = ctx->bu != nullptr;         // FM: the caller's dense optimiser steps the biases
    if (bias_grad_out && !(ctx->g_bu && ctx->g_bi)) {
        set_error("staged_adam_step: the context has biases but no g_u_bias / g_i_bias outputs");
        return DAISY_ERR_ARG;
    }
    return staged_adam_step(ctx, P, Q, loss_type, gamma, reg_1, reg_2, a, table, bias_grad_out, stats, epoch_acc,
                            step_loss, as_stream(stream));
}

// The epoch loop of GeneralRecommender.fit (AbstractRecommender.py:118-128) with torch.optim.Adam
// (AbstractRecommender.py:54): every batch of a built plan through the staged Adam step, enqueued natively - steps
// first_step, first_step + 1, ... - and, flush != 0, the rows no batch referenced brought up to the epoch's last step
// (daisy_adam_lazy_flush on both tables), so the tables are current when the call's work has drained.
int daisy_bpr_fit_epoch_adam(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, float *P, float *Q, int32_t loss_type,
                             float gamma, float lr, float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP,
                             float *mQ, float *vQ, int32_t *lastQ, const float *table, int64_t table_steps, float beta1,
                             float beta2, float eps, int64_t first_step, int32_t flush, double *stats, double *epoch_acc,
                             double *step_losses, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && plan && P && Q && mP && vP && lastP && mQ && vQ && lastQ && table && stats && first_step >= 1,
                    "fit_epoch_adam: bad argument");
    if (!plan->built) { set_error("fit_epoch_adam: plan has not been built"); return DAISY_ERR_STATE; }
    DAISY_CHECK_ARG(loss_type >= DAISY_LOSS_BPR && loss_type <= DAISY_LOSS_SL, "Invalid loss type: %d", loss_type);
    DAISY_CHECK_ARG(first_step + plan->num_batches - 1 <= table_steps,
                    "fit_epoch_adam: the constants table holds %lld steps, the epoch ends at step %lld",
                    (long long)table_steps, (long long)(first_step + plan->num_batches - 1));
    if (ctx->bu) {          // FM: the biases step through the caller's dense optimiser between two steps
        set_error("fit_epoch_adam: contexts with FM biases are driven step by step (daisy_bpr_staged_adam_step)");
        return DAISY_ERR_ARG;
    }
    if (small_epoch_supported(ctx, plan, loss_type)) {
        // batches of a few hundred samples over the sorted plan (the reference's default batch): every step of the epoch
        // inside one persistent workgroup, like the SGD epoch (csrc/bpr_small.hip) - 48 -> ~12 us per step at B = 256
        DAISY_CHECK_ARG(plan->U == ctx->U && plan->I == ctx->I, "fit_epoch_adam: plan does not fit the context");
        SmallAdamArgs ad{mP, vP, lastP, mQ, vQ, lastQ, table, beta1, beta2, eps, first_step};
        int rc = small_fit_epoch(ctx, plan, P, Q, loss_type, gamma, lr, reg_1, reg_2, stats, epoch_acc, step_losses, as_stream(stream), &ad);
        if (rc) return rc;
    } else {
        if (plan->kind == 0) {
            set_error("fit_epoch_adam: a plan in the sorted layout is only run by the small-batch epoch kernel "
                      "(daisy_bpr_small_epoch_supported); build the partitioned layout (daisy_epoch_plan_build_indexed)");
            return DAISY_ERR_ARG;
        }
    for (int64_t k = 0; k < plan->num_batches; ++k) {
        int rc = daisy_bpr_set_batch_from_plan(ctx, plan, k, stream);
        if (rc) return rc;
        rc = daisy_bpr_staged_adam_step(ctx, P, Q, loss_type, gamma, lr, reg_1, reg_2, mP, vP, lastP, mQ, vQ, lastQ, table,
                                        beta1, beta2, eps, first_step + k, stats, epoch_acc,
                                        step_losses ? step_losses + k : nullptr, stream);
        if (rc) return rc;
    }
    }
    if (flush && plan->num_batches > 0) {
        const int64_t t = first_step + plan->num_batches - 1;
        int rc = daisy_adam_lazy_flush(P, mP, vP, lastP, ctx->U, ctx->d, table, beta1, beta2, eps, t, stream);
        if (rc) return rc;
        if ((rc = daisy_adam_lazy_flush(Q, mQ, vQ, lastQ, ctx->I, ctx->d, table, beta1, beta2, eps, t, stream))) return rc;
        ctx->p_sqnorm_of = nullptr;          // the flush rewrote rows of P behind the row-norm cache
        ctx->pre_ready = false;
    }
    return DAISY_OK;
}

int daisy_bpr_small_epoch_supported(const daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, int32_t loss_type) {
    if (!ctx || !plan || !plan->built) return 0;
    if (!small_epoch_supported(ctx, plan, loss_type)) return 0;
    return small_epoch_adam_pays(ctx, plan) ? 3 : 1;
}

int daisy_bpr_staged_adam_catchup_users(daisy_bpr_ctx *ctx, float *P, float *mP, float *vP, int32_t *lastP,
                                        const float *table, float beta1, float beta2, float eps, int64_t step,
                                        daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && mP && vP && lastP && table && step >= 1, "staged_adam_catchup_users: bad argument");
    if (!ctx->batch_set) { set_error("staged_adam_catchup_users: no batch set"); return DAISY_ERR_STATE; }
    StagedAdam a = adam_consts(0.f, beta1, beta2, eps, step);
    a.mP = mP; a.vP = vP; a.lastP = lastP;
    hipStream_t s = as_stream(stream);
    const StreamView &v = ctx->sv;
    const int d = ctx->d;
    int rc = staged_norm_cache(ctx, P, s);
    if (rc) return rc;
    rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((k_staged_adam_catchup<C>), dim3(grid_for(v.B, C::GROUPS_PER_BLOCK, kMaxGridSparse)), dim3(kBlock),
                           0, s, v, d, P, (float *)nullptr, a, reinterpret_cast<const float2 *>(table), ctx->p_sqnorm, 1);
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_bpr_staged_user_adam(daisy_bpr_ctx *ctx, float *P, const float *Q, int32_t loss_type, float gamma, float lr,
                               float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP, float beta1, float beta2,
                               float eps, int64_t step, double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats && mP && vP && lastP && step >= 1, "staged_user_adam: NULL argument");
    StagedAdam a = adam_consts(lr, beta1, beta2, eps, step);
    a.mP = mP; a.vP = vP; a.lastP = lastP;
    return staged_user_phase(ctx, "staged_user_adam", P, Q,
                             StagedStep{loss_type, gamma, 0.f, reg_1, reg_2, stats, nullptr, nullptr, &a, false, as_stream(stream)});
}

int daisy_item_apply_counts_adam(float *Q, float *g, float *cnt, float *m, float *v, int64_t rows, int32_t d, float lr,
                                 float reg_1, float reg_2, float beta1, float beta2, float eps, int64_t step,
                                 const double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(Q && g && cnt && m && v && stats && rows > 0 && step >= 1, "item_apply_counts_adam: bad argument");
    const StagedAdam a = adam_consts(lr, beta1, beta2, eps, step);
    return item_apply_counts(Q, g, cnt, m, v, rows, (int)d, reg_1, reg_2, row_opt(lr, &a, false), stats, as_stream(stream));
}

int daisy_item_apply_counts(float *Q, float *g, float *cnt, int64_t rows, int32_t d, float lr, float reg_1,
                            float reg_2, const double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(Q && g && cnt && stats && rows > 0, "item_apply_counts: bad argument");
    return item_apply_counts(Q, g, cnt, nullptr, nullptr, rows, (int)d, reg_1, reg_2, row_opt(lr, nullptr, false), stats,
                             as_stream(stream));
}

}  // extern "C"
