// Shared between the translation units of the STAGED step (see the header comment of bpr_staged.hip):
//   bpr_staged.hip        staged_path - what a step runs, decided once -, the SGD and Adam step drivers, the C ABI
//   bpr_staged_user.hip   the pre-norm kernels, k_staged_user, k_staged_user_edges and their launchers
//   bpr_staged_item.hip   k_staged_item, its edge kernels, k_item_apply_counts*, k_slice_ranges and their launchers
// Here: the chunk shapes of the two passes, the argument blocks of their kernels, the device code both passes run (the
// three-launch form carries the user pass's edge chains inside the item launch), and StagedPath / StagedStep, which are
// all a launcher is told.  bpr_train.hip reads the chunk shapes to size the context's edge records.
#pragma once
#include <type_traits>

#include "bpr_internal.h"

namespace daisy {

constexpr int kItemWinFloats = 6144;      // 24 KB of Q rows per workgroup of the item pass (96 rows at d = 64); rows of two
                                          // float4 per lane get 16 KB, wider ones none (their partial-sum slots already
                                          // take the LDS that four workgroups per CU leave)

// threads per workgroup of the item pass outside the three-launch form.  Its four barriers per chunk make a workgroup as
// slow as its slowest wave's gathers; two waves per workgroup instead of four (round 5, same box): 222 -> 216 us at
// BASELINE configs[1], 296 -> 285 us at 10 M x 1 M shapes; one wave (64 threads: four times the chunks, edge records and
// finishers) loses again (227 / 307 us).  Rounds 2 / 3 had measured 128 "the same" - with the commit stalls still in.
constexpr int kStagedUserBlock = 128, kStagedItemBlock = 128;    // threads per workgroup of the two passes (measured:
                                                                 // user pass 387 -> 360 us at 128, item pass indifferent)

// samples per lane group per chunk in the user pass (3 row gathers each).  Measured at d=64: 4 (128 VGPRs,
// 4 waves/SIMD) beats 8 (178 VGPRs, 2 waves/SIMD) by 10 % at C2 shapes and ties at C3 shapes.
// BLK: threads per workgroup.  A workgroup's waves load together and compute together (the barriers of the
// run/slot reduction keep them in step), so smaller workgroups interleave memory and VALU phases better
// across the CU; the price is more chunk boundaries (edge records).
template <class C, int BLK = kBlock>
struct StagedUserCfg {
    static constexpr int RUN_BY_REGS = (C::NE <= 8) ? 4 : 2;
    static constexpr int RUN = RUN_BY_REGS < C::LPR ? RUN_BY_REGS : C::LPR;
    static constexpr int G = BLK / C::LPR;
    static constexpr int E = G * RUN;
};
// workgroup size of the user pass: 128 threads; ONE wave (its barriers are free) for rows of two float4 per
// lane (64 < d <= 128: 1.40 -> 1.27 ms per 2M-sample step at d=128; slower at d <= 64 (0.60 -> 0.71), and
// rows of four float4 per lane would need more edge records than the context holds)
template <class C>
struct StagedUserBlk {
    static constexpr int value = (C::NE == 8 && C::LPR == 16) ? 64 : ((C::LPR <= 32) ? kStagedUserBlock : kBlock);
};
// SPARSE: few entries per item (small batches, or huge item tables): nearly every entry ends a segment, and each end is a
// commit that needs the item's row of Q - a DEPENDENT read inside the reduction loop wherever the row is not in the LDS
// window (which holds a contiguous item range and therefore only helps dense batches).  At B = 4096 over 100 K items the
// 16 commits of a 16-entry run were 16 trips to memory one after the other: 14 us for a pass that moves 2 MB.  The sparse
// flavour takes runs of 4 entries (four times the workgroups: these batches do not fill the chip anyway) and gathers
// the Q row of EVERY entry together with its staged row, so a commit waits for nothing.
template <class C, int BLK = kBlock, bool SPARSE = false>
struct StagedItemCfg {
    // staged rows in flight per lane group: 64 row registers in every shape (16 x 4 floats, 8 x 8, 4 x 16)
    static constexpr int RUN4 = 16, RUN8 = 8, RUN16 = 4;
    static constexpr int RUN_BY_REGS = SPARSE ? ((C::NE <= 8) ? 4 : 2) : ((C::NE <= 4) ? RUN4 : ((C::NE <= 8) ? RUN8 : RUN16));
    static constexpr int RUN = RUN_BY_REGS < C::LPR ? RUN_BY_REGS : C::LPR;
    static constexpr int G = BLK / C::LPR;
    static constexpr int E = G * RUN;
};

// The NEXT batch's pre-norm riding on this step's item pass (single-GPU epoch loops): once the user pass and its edge
// kernel are done, P and the row-norm cache are final for this step, so the extra workgroups [first_block, gridDim.x)
// of the item-pass launch do k_unorm's work for batch k+1 and an extra workgroup of the item-edge launch adds the
// partial sums (RideReduce) - two launches less per step (k_unorm, k_unorm_reduce: ~12 us of kernels and two
// kernel boundaries of a 0.57 ms step, one of five launches below ~130 k samples).
struct RideUnorm {
    const float *p_sqnorm; const uint4 *s_rec; int64_t B;        // the sample records of the NEXT batch (partitioned plan)
    double *partials; int first_block, nblocks;      // nblocks == 0: nothing rides
};
struct RideReduce { const double *partials; int n; double *stats; };    // n == 0: nothing rides

__device__ __forceinline__ void unorm_block(const RideUnorm &r, int b) {
    double acc = 0.0;
    for (int64_t s = (int64_t)b * blockDim.x + threadIdx.x; s < r.B; s += (int64_t)r.nblocks * blockDim.x)
        acc += (double)r.p_sqnorm[r.s_rec[s].x];
    __shared__ double sm_ride[kBlock / kWave];
    const double w = wave_sum_f64(acc);
    if ((threadIdx.x % kWave) == 0) sm_ride[threadIdx.x / kWave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < (int)blockDim.x / kWave; ++k) t += sm_ride[k];
        r.partials[b] = t;
    }
}

// Sum |P[u_s]|^2 over the batch as the user pass needs it before its first update.  n_pre == 0: stats holds it (the
// phase API: the host has all-reduced it over the ranks).  Otherwise the single-GPU step skips k_unorm_reduce and
// every wave adds k_unorm's n_pre (<= kPreBlocks) partial sums itself - the same loads in the same order in every
// wave of every workgroup, so all of them see the same bits.
struct PreNorm { const double *partials; int n; };
__device__ __forceinline__ double prenorm_sum(const double *__restrict__ stats, PreNorm pre) {
    if (pre.n == 0) return stats[DAISY_ST_SQ_U_PRE];
    double t = 0.0;
    for (int b = threadIdx.x % kWave; b < pre.n; b += kWave) t += pre.partials[b];
    return wave_sum_f64(t);
}

// what the owner of a finished user run does with g = sum_s dL/dx_s (q_i - q_j) over the run's n samples:
// regulariser (MFRecommender.py:94-95), the optimiser's step on P[u] in place, the row-norm cache
template <class C, bool ADAM>
__device__ __forceinline__ void user_commit(float *__restrict__ P, float *__restrict__ p_sqnorm, int64_t user, Row<C> &p,
                                            const Row<C> &acc, float n, float reg_1, float rU, const RowOpt &opt, int lane,
                                            int d, bool stream_row = false, const Row<C> *m_pre = nullptr,
                                            const Row<C> *v_pre = nullptr) {
    const float w1 = reg_1 * n, w2 = rU * n;
    Row<C> g;
#pragma unroll
    for (int k = 0; k < C::NE; ++k) g.v[k] = acc.v[k] + fmaf(w2, p.v[k], w1 * sgn(p.v[k]));
    row_apply<C, ADAM>(p, g, opt, user, lane, d, m_pre, v_pre);
    if (stream_row) p.store_nt(P + user * d, lane, d);      // (a table far beyond the caches: see StreamView::p_stream)
    else p.store(P + user * d, lane, d);
    const float sq = row_dot<C>(p, p);
    if (lane == 0) p_sqnorm[user] = sq;
}

// FM: the user bias follows its user's run (u_bias[u] -= lr * sum of the run's dL/dpos + dL/dneg, or the sum itself
// for a dense optimiser)
__device__ __forceinline__ void user_bias_commit(const StagedBias &fm, int64_t user, float sb, float lr, int lane) {
    if (fm.bu && lane == 0) {
        if (fm.grad_out) fm.g_bu[user] = sb;
        else fm.bu[user] = fmaf(-lr, sb, fm.bu[user]);
    }
}

struct UserEdges {
    float *vec;        // [2*nchunks][d] partial user gradients of runs that cross a chunk boundary
    int32_t *user;     // [2*nchunks]    their user (-1: none); [2c] head edge, [2c+1] tail edge
    float *n;          // [2*nchunks][2] their sample counts and (FM) coefficient sums
    int32_t *whole;    // [nchunks]      the head edge's run also fills the whole chunk
};

// how a sample reaches the item pass:
//   kModePremul  pairwise loss with dL/dneg = -dL/dpos (BPR, HL): stage[slot] = dL/dpos * p_u serves both entries
//   kModePlain   any pairwise loss: stage[slot] = p_u, coef[slot] = (dL/dpos, dL/dneg) (TOP1; FM's pairwise runs,
//                whose item biases need the bare coefficients)
//   kModePoint   point-wise loss (CL / SL, MFRecommender.py:75-81): rows are (user, item, label), ONE entry per
//                sample, stage[slot] = dL/dpred * p_u (+ coef[slot].x = dL/dpred when there are FM biases)
enum { kModePremul = 0, kModePlain = 1, kModePoint = 2 };

// chains of edge records: the chunk whose TAIL edge starts a run owns it.  A user whose run crosses a
// chunk boundary is touched by nobody else in this step, so P[u] is still the pre-step row here.
// The single-GPU step gives this launch one more workgroup (red.nblocks > 0), which does what k_reduce_partials
// would do in a launch of its own: the user pass's per-workgroup sums -> stats, norms, loss.
struct ReduceJob {
    const double *partials;
    int nblocks;                 // 0: no reduction rides on this launch
    double *stats, *epoch_acc, *step_loss;
};
template <class C, bool ADAM>
__device__ __forceinline__ void user_edges_block(unsigned bid, unsigned nb, float *__restrict__ P, int64_t nchunks, int d,
                                                 const double *__restrict__ stats, const RowOpt &opt, float reg_1,
                                                 float reg_2, const UserEdges &ed, float *__restrict__ p_sqnorm,
                                                 const PreNorm &pre, const ReduceJob &red, const StagedBias &fm) {
    const double sq_pre = prenorm_sum(stats, pre);
    if (red.nblocks > 0) {            // workgroup 0 (dispatched first: its chain of dependent loads is the longest)
        if (bid == 0) {
            reduce_partials_block(red.partials, red.nblocks, red.stats, true, reg_1, reg_2, red.epoch_acc, red.step_loss);
            if (threadIdx.x == 0 && pre.n) red.stats[DAISY_ST_SQ_U_PRE] = sq_pre;
            // FM, SGD: bias_ -= lr * sum_b (dL/dpos + dL/dneg)  (a dense optimiser reads the sum from stats instead)
            if (threadIdx.x == 0 && fm.bu && !fm.grad_out)
                fm.b0[0] = fmaf(-opt.lr, (float)red.stats[DAISY_ST_SUM_COEF], fm.b0[0]);
            return;
        }
        nb -= 1; bid -= 1;
    }
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)nb * C::GROUPS_PER_BLOCK;
    const float rU = inv_or_zero(sqrt(sq_pre), reg_2);
    for (int64_t c = (int64_t)bid * C::GROUPS_PER_BLOCK + group; c < nchunks; c += gstride) {
        const int uu = ed.user[2 * c + 1];
        if (uu < 0) continue;
        Row<C> acc, t;
        acc.load(ed.vec + (2 * c + 1) * d, lane, d);
        float ns = ed.n[2 * (2 * c + 1)], sb = ed.n[2 * (2 * c + 1) + 1];
        for (int64_t k = c + 1; k < nchunks && ed.user[2 * k] == uu; ++k) {
            t.load(ed.vec + (2 * k) * d, lane, d);
#pragma unroll
            for (int q = 0; q < C::NE; ++q) acc.v[q] += t.v[q];
            ns += ed.n[2 * (2 * k)];
            sb += ed.n[2 * (2 * k) + 1];
            if (!ed.whole[k]) break;
        }
        Row<C> p;
        p.load(P + (int64_t)uu * d, lane, d);
        user_commit<C, ADAM>(P, p_sqnorm, uu, p, acc, ns, reg_1, rU, opt, lane, d);
        user_bias_commit(fm, uu, sb, opt.lr, lane);
    }
}

// The THREE-LAUNCH form of the step (batches up to kMergeMaxBatch samples, where a step is a chain of launches of ~4.5 us
// each and not bytes): the user pass's edge chains + the reduction of its sums, and the item pass, touch disjoint data
// - the chains write rows of P and the norm cache, the item pass reads the stage and Q - once the item workgroups stop
// waiting for the reduced norms: every one of them adds the user pass's per-workgroup sums itself (partials_sums: the
// same loads in the same order as the reduction, so the same bits).  The item launch then carries the chains and the
// reduction as extra workgroups behind its own; the next batch's pre-norm, which needs the chains' rows, moves on to the
// item-edge launch.
struct MergedJob {
    float *P; int64_t u_nchunks; UserEdges ued; float *p_sqnorm; PreNorm pre; ReduceJob red;
    int n_ue;                    // workgroups for the user pass's edge chains (the reduction's workgroup not counted)
};

struct ItemEdges2 {
    float *vec;          // [2*nchunks][d]  partial gradient rows; [2c] head edge (inherited), [2c+1] tail edge
    int32_t *item;       // [2*nchunks]     their item (-1: none)
    float *cnt;          // [2*nchunks][4]  their (n_pos, n_neg, sum of the coefficients (FM), -)
    int32_t *whole;      // [nchunks]       the head edge's segment also runs on into the next chunk
};

// Long edge chains in two levels (round 5).  A segment that runs through N chunks is a chain of N head edges which
// its owner adds one after the other: ~42 entries per item at BASELINE configs[1] make chains of one or two links, but with
// a Zipf(1.0) popularity the hottest item holds 7 % of a batch's entries - a chain of 2300 links walked by ONE lane group,
// 198 us of a 0.83 ms step (profiles/r05_notes.txt).  Level 1 (this kernel, one lane group per block of kEdgeBlock
// chunks): the sum of the head edges of the chain that ENTERS the block at its first chunk, as far as it runs inside the
// block, and whether it leaves the block at the other end.  Level 2 (k_staged_item_edges): an owner walks to the next
// block boundary link by link and from there block by block.  Fixed order, single writer: reproducible like the chains.
struct EdgeBlocks { float *vec; int32_t *item; float *cnt; int32_t *through; };      // vec == NULL: chains link by link

// ---------------------------------------------------------------------------------------------------------
// host side: what a call runs (decided by staged_path, bpr_staged.hip) and the launchers of the two passes
// ---------------------------------------------------------------------------------------------------------
struct StagedAdam {           // the lazy Adam state of both tables for step t (daisy_bpr_staged_adam_step)
    float *mP, *vP; int32_t *lastP;
    float *mQ, *vQ; int32_t *lastQ;
    float step_size, bc2_sqrt, beta1, beta2, eps;
    int32_t t;
};
// optimiser of one table's row owners; a == nullptr: SGD
inline RowOpt row_opt(float lr, const StagedAdam *a, bool user_side) {
    RowOpt o{};
    o.lr = lr;
    if (a) {
        o.m = user_side ? a->mP : a->mQ;
        o.v = user_side ? a->vP : a->vQ;
        o.last = user_side ? a->lastP : a->lastQ;
        o.step_size = a->step_size; o.bc2_sqrt = a->bc2_sqrt;
        o.beta1 = a->beta1; o.beta2 = a->beta2; o.eps = a->eps;
        o.t = a->t;
    }
    return o;
}

// hyper-parameters and outputs of one step (or of one phase of it)
struct StagedStep {
    int loss_type;
    float gamma, lr, reg_1, reg_2;
    double *stats, *epoch_acc, *step_loss;     // epoch_acc / step_loss: the whole step in one call only, and optional
    const StagedAdam *adam;                    // nullptr: SGD
    bool bias_grad_out;                        // FM: the bias gradients go to g_bu / g_bi for a dense optimiser
    hipStream_t s;
};

// What a call runs: filled once by staged_path before anything is launched and handed on; the launchers decide nothing.
enum { kStagedUser = 1, kStagedItem = 2, kStagedStep = 3 };      // the passes of a call; both: the whole step
struct StagedPath {
    int mode;                    // kModePremul / kModePlain / kModePoint
    bool has_pos, p_stream;      // partitioned plan (the slot comes with the record); P read and written past the caches
    bool adam, apply;            // the owners' optimiser; item pass in place (else: data term + entry counts out)
    bool fused;                  // the whole step: the reduction of the user pass's sums rides on its edge work
    // this batch's pre-norm.  pre_own: the step launches it first (k_unorm over gp workgroups) - nothing rode for it
    bool pre_own;
    int gp, n_pre;               // n_pre > 0: that many partial sums wait behind the user pass's own; 0: stats[SQ_U_PRE]
    // user pass: threads per workgroup, chunks, grid, workgroups of its edge chains
    int u_blk, gu, n_ue;
    int64_t u_chunks;
    // item pass (slice >= 0: that item slice of the batch only): threads per workgroup, entries per chunk, chunks, grid,
    // workgroups of its edge chains; sparse flavour; edge chains in two levels
    int slice, i_blk, i_chunk, gi, n_ie;
    int64_t i_chunks;
    bool sparse, two_level;
    bool merge;                  // the three-launch form (MergedJob): final
    // the NEXT batch's pre-norm rides on this step (RideUnorm) over gn workgroups; ride_fold: its consumers add the
    // partial sums themselves, else they are reduced on the item-edge launch (RideReduce)
    bool ride, ride_fold;
    int gn;
};

// a runtime value of the path as a compile-time tag, f(std::integral_constant<...>{}): a kernel's template arguments are
// chosen in one place, its launcher
template <class F>
inline void with_flag(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
inline void with_mode(int mode, F &&f) {
    if (mode == kModePremul) f(std::integral_constant<int, kModePremul>{});
    else if (mode == kModePlain) f(std::integral_constant<int, kModePlain>{});
    else f(std::integral_constant<int, kModePoint>{});
}

// argument blocks that the user pass's edge work takes wherever it runs (its own launch, or the item launch when merged)
inline StagedBias staged_bias(const daisy_bpr_ctx *ctx, bool grad_out) {
    return StagedBias{ctx->bu, ctx->bi, ctx->b0, ctx->g_bu, ctx->g_bi, grad_out ? 1 : 0};
}
inline UserEdges staged_user_edges(const daisy_bpr_ctx *ctx) {
    return UserEdges{ctx->edge_vec, ctx->edge_user, ctx->edge_n, ctx->edge_whole};
}
inline PreNorm staged_pre(const daisy_bpr_ctx *ctx, const StagedPath &path) {
    return PreNorm{ctx->partials + (size_t)kMaxGrid * 8, path.n_pre};
}
inline ReduceJob staged_reduce(const daisy_bpr_ctx *ctx, const StagedPath &path, const StagedStep &st) {
    return ReduceJob{ctx->partials, path.fused ? path.gu : 0, st.stats, st.epoch_acc, st.step_loss};    // phases: the caller reduces
}

// bpr_staged_user.hip.  staged_norm_cache: (re)builds the cache of |P[u]|^2 when it does not describe P; staged_prenorm:
// that, k_unorm over gn workgroups and - unless the consumers fold the partial sums - k_unorm_reduce -> stats[SQ_U_PRE]
int staged_norm_cache(daisy_bpr_ctx *ctx, const float *P, hipStream_t s);
int staged_prenorm(daisy_bpr_ctx *ctx, const float *P, double *stats, int gn, bool fold, hipStream_t s);
int staged_user(daisy_bpr_ctx *ctx, const StagedPath &path, const StagedStep &st, float *P, const float *Q);
// bpr_staged_item.hip.  Qo = Q (path.apply) or gQ with cnt_out f32[I][2]; P: the three-launch form's edge chains write it
int staged_item(daisy_bpr_ctx *ctx, const StagedPath &path, const StagedStep &st, float *P, float *Qo, float *cnt_out);
int staged_slice_ranges(daisy_bpr_ctx *ctx, const int32_t *item_bounds, int n_slices, hipStream_t s);
int item_apply_counts(float *Q, float *g, float *cnt, float *m, float *v, int64_t rows, int d, float reg_1, float reg_2,
                      const RowOpt &opt, const double *stats, hipStream_t s);      // m == nullptr: SGD with opt.lr

}  // namespace daisy
