/*
 * daisyrec_amd.h — C ABI of the MI355X-native MF + BPR training hot path.
 *
 * This is the drop-in boundary: every entry point takes plain device pointers,
 * sizes and a HIP stream (void* == hipStream_t).  No torch / C++ types cross
 * it.  The reference (AmazingDD/daisyRec v2.3.0) is pure Python; each function
 * below names the reference interface it replaces (file:line relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding a daisyRec
 * maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`
 *   - tables are row-major fp32  P[user_num][d], Q[item_num][d]
 *     (nn.Embedding.weight, MFRecommender.py:53-54); they are updated IN PLACE
 *   - indices are int32 (`.astype(np.int32)`, sampler.py:101) unless stated
 *   - every call only ENQUEUES work on `stream`; nothing synchronises the host
 *   - return value: 0 = ok, otherwise an error code; daisy_last_error() gives
 *     the message (thread local)
 */
#ifndef DAISYREC_AMD_H
#define DAISYREC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAISY_ABI_VERSION 8

typedef void *daisy_stream_t; /* hipStream_t */

enum daisy_status {
    DAISY_OK = 0,
    DAISY_ERR_ARG = 1,  /* bad argument (null pointer, size out of range, unsupported d) */
    DAISY_ERR_HIP = 2,  /* a HIP runtime call failed */
    DAISY_ERR_STATE = 3 /* call order violated (e.g. step before set_batch) */
};

/* daisy/utils/loss.py:5-33.  (AbstractRecommender.py:79-93 builds them.) */
enum daisy_loss {
    DAISY_LOSS_BPR = 0, /* -(gamma + sigmoid(pos-neg)).log().sum()          loss.py:10-13 */
    DAISY_LOSS_HL = 1,  /* clamp(1-(pos-neg), min=0).sum()                  loss.py:20-23 */
    DAISY_LOSS_TL = 2,  /* sigmoid(neg-pos).sum()+sigmoid(neg**2).sum()     loss.py:30-33 */
    /* point-wise (AbstractRecommender.py:80-83, MFRecommender.py:75-81): rows are (user, item, label) */
    DAISY_LOSS_CL = 3,  /* nn.BCEWithLogitsLoss(reduction='sum')(pred, label)               */
    DAISY_LOSS_SL = 4   /* nn.MSELoss(reduction='sum')(pred, label)                         */
};

/* how the item-side gradient is accumulated (entries of a batch are always sorted by item) */
enum daisy_item_mode {
    DAISY_ITEM_ATOMIC = 0,  /* one fp32 atomic row per entry (kept for A/B measurements only) */
    DAISY_ITEM_SORTED = 1,  /* one owner per row, entries summed in plan order: bitwise reproducible */
    DAISY_ITEM_CHUNKED = 2, /* segmented reduction through LDS accumulators (throughput mode) */
    DAISY_ITEM_FUSED = 3    /* daisy_bpr_sgd_step / daisy_bpr_fit_epoch_sgd only: the STAGED step (forward fused
                               into the user pass, coefficient-scaled user rows staged for the item pass,
                               item rows committed by the owner of their segment); every loss of loss.py:5-33
                               (point-wise ones on point-wise batches), with or without FM biases (ABI 4).
                               Bitwise reproducible.  After a step inside an epoch loop stats[DAISY_ST_SQ_U_PRE]
                               already holds the NEXT batch's value (it rides on this step's item pass). */
};

/* order of an epoch (what DataLoader(shuffle=...) decides, dataset.py:5-7) */
enum daisy_order_mode {
    DAISY_ORDER_IDENTITY = 0, /* shuffle=False: triples in array order                          */
    DAISY_ORDER_PERM = 1,     /* explicit permutation: perm[p] = triple served at position p     */
    DAISY_ORDER_FEISTEL = 2   /* shuffle=True on the device: keyed bijection of (seed, epoch)    */
};

/* layout of the caller-owned `stats` vector (device, double[DAISY_STATS_LEN]) */
enum daisy_stats_slot {
    DAISY_ST_LOSS_DATA = 0, /* sum of per-sample loss terms                    */
    DAISY_ST_L1_U = 1,      /* |P[u]|_1  over the gathered batch               */
    DAISY_ST_L1_I = 2,      /* |Q[i]|_1                                        */
    DAISY_ST_L1_J = 3,      /* |Q[j]|_1                                        */
    DAISY_ST_SQ_U = 4,      /* sum P[u]^2  (slots 0..6 are SUMS: all-reducible)*/
    DAISY_ST_SQ_I = 5,
    DAISY_ST_SQ_J = 6,
    DAISY_ST_LOSS = 7,      /* total loss of the step (written by finalize)    */
    DAISY_ST_NORM_U = 8,    /* |P[u]|_F (written by finalize)                  */
    DAISY_ST_NORM_I = 9,
    DAISY_ST_NORM_J = 10,
    DAISY_ST_NORM_U_PRE = 11, /* (unused since ABI 3; see DAISY_ST_SQ_U_PRE)                 */
    DAISY_ST_SUM_COEF = 12,   /* sum_b (dL/dpos + dL/dneg) = dL/d bias_ (FM); a batch sum like 0..6:
                                 multi-GPU callers all-reduce it with them before finalize       */
    DAISY_ST_SQ_U_PRE = 13,   /* staged step: sum P[u]^2 over the batch from the row-norm cache, known
                                 BEFORE the user pass (a sum: multi-GPU callers all-reduce it)    */
    DAISY_STATS_LEN = 16
};

const char *daisy_last_error(void);
int daisy_abi_version(void);

/* ------------------------------------------------------------------------
 * Training context: owns the per-step scratch (grouped batch, coefficients,
 * sort buffers, partial sums).  One per (process, GPU).
 * ---------------------------------------------------------------------- */
typedef struct daisy_bpr_ctx daisy_bpr_ctx;

int daisy_bpr_ctx_create(daisy_bpr_ctx **out, int64_t max_batch, int32_t d, int64_t user_num,
                         int64_t item_num);
int daisy_bpr_ctx_destroy(daisy_bpr_ctx *ctx);
/* bytes of device scratch the context holds (for reporting) */
size_t daisy_bpr_ctx_scratch_bytes(const daisy_bpr_ctx *ctx);

/* ------------------------------------------------------------------------
 * Epoch plan: replaces one pass of `for batch in DataLoader(BasicDataset(triples),
 * batch_size, shuffle)` (dataset.py:5-27) + `.to(device)` (MFRecommender.py:71-72,83).
 * One build per epoch lays the epoch out batch by batch in HBM — batch k holds exactly
 * the triples DataLoader's k-th batch would (last batch partial, drop_last=False) —
 * each batch grouped by user, plus its item entries sorted by item, so the step
 * kernels update every table row from a single owner instead of through atomics.
 * ---------------------------------------------------------------------- */
typedef struct daisy_epoch_plan daisy_epoch_plan;

int daisy_epoch_plan_create(daisy_epoch_plan **out, int64_t max_triples, int64_t user_num,
                            int64_t item_num);
int daisy_epoch_plan_destroy(daisy_epoch_plan *plan);
size_t daisy_epoch_plan_bytes(const daisy_epoch_plan *plan);
/* triples: int32 [n_triples][3]; perm: int64 [n_triples], only for DAISY_ORDER_PERM;
 * (seed, epoch) only for DAISY_ORDER_FEISTEL; user_base is subtracted from the user
 * ids (user-sharded tables).  flags: DAISY_PLAN_TRIPLES_USER_SORTED promises that the
 * triple array is sorted by user (CSR order), so grouping a batch by user only needs a
 * stable partition by batch (one radix pass); a wrong promise gives wrong updates. */
#define DAISY_PLAN_TRIPLES_USER_SORTED 1
#define DAISY_PLAN_POINTWISE 2 /* rows are (user, item, label): CL / SL losses */
int daisy_epoch_plan_build(daisy_epoch_plan *plan, const int32_t *triples, int64_t n_triples,
                           const int64_t *perm, int32_t order_mode, uint64_t seed, uint64_t epoch,
                           int64_t batch_size, int32_t user_base, int32_t flags,
                           daisy_stream_t stream);
int64_t daisy_epoch_plan_num_batches(const daisy_epoch_plan *plan);
/* daisy_epoch_plan_build only enqueues; ids outside [0,user_num) x [0,item_num) (after user_base) are
 * replaced by 0 there - never an out-of-bounds access - and remembered.  This call synchronises the stream
 * and returns DAISY_ERR_ARG if the last build saw one (the reference raises IndexError in nn.Embedding,
 * MFRecommender.py:64-65).  daisy_bpr_ctx_validate_batch: the same for the batch last set with
 * daisy_bpr_set_batch / daisy_bpr_set_batch_from_triples. */
int daisy_epoch_plan_validate(const daisy_epoch_plan *plan, daisy_stream_t stream);
int daisy_bpr_ctx_validate_batch(const daisy_bpr_ctx *ctx, daisy_stream_t stream);
/* copy batch k of a built plan into caller buffers (inspection / tests): u,i,j int32 [B]
 * grouped by user; optional item entries [2B] sorted by item: ent_item, ent_s (sample
 * position | 0x80000000 for the negative slot), ent_u (user of that sample).
 * *B_out_host (host pointer, may be NULL) receives the batch size. */
int daisy_epoch_plan_read_batch(const daisy_epoch_plan *plan, int64_t k, int32_t *u, int32_t *i,
                                int32_t *j, int32_t *ent_item, uint32_t *ent_s, int32_t *ent_u,
                                int64_t *B_out_host, daisy_stream_t stream);
/* out[t] = position of triple t in the DAISY_ORDER_FEISTEL order of (seed, epoch) */
int daisy_feistel_positions(int64_t n, uint64_t seed, uint64_t epoch, int64_t *out,
                            daisy_stream_t stream);
/* the same for a subset of the triples: out[k] = position of triple ids[k] among all n (-1 for an id outside 0..n-1):
 * what a rank of a multi-GPU fit needs for its rows (daisy_epoch_plan_build_positions) */
int daisy_feistel_positions_at(const int64_t *ids, int64_t n_ids, int64_t n, uint64_t seed, uint64_t epoch,
                               int64_t *out, daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Static index of a training set + the PARTITIONED epoch plan (ABI 3).
 * BasicDataset holds one immutable triple array for the whole fit (dataset.py:21); only the batch
 * membership changes per epoch (DataLoader(shuffle=True), dataset.py:5-7).  So the set is indexed once -
 * triples in CSR (user-sorted) order, their 2n item entries sorted by item - and an epoch plan is two
 * stable one-digit partitions of those arrays by batch id (a stable partition of a sorted list leaves
 * every batch sorted): 32 B of plan per interaction instead of 112, one counting + one scatter pass
 * instead of two payload-carrying radix sorts.  The resulting plan feeds the staged step
 * (DAISY_ITEM_FUSED) only.
 * daisy_train_index_create validates 0 <= user - user_base < user_num, 0 <= item < item_num for every
 * triple (one host sync) and returns DAISY_ERR_ARG where the reference raises IndexError in
 * nn.Embedding (MFRecommender.py:64-65).  flags: DAISY_PLAN_TRIPLES_USER_SORTED - the array is already
 * in CSR order and is used in place (the caller keeps it alive); otherwise the index owns a sorted copy;
 * DAISY_PLAN_POINTWISE (ABI 4) - rows are (user, item, label) (CL / SL, sampler.py:93-98): ONE item entry per
 * row, the third column is carried as the label and not validated as an id.
 * ---------------------------------------------------------------------- */
typedef struct daisy_train_index daisy_train_index;
int daisy_train_index_create(daisy_train_index **out, const int32_t *triples, int64_t n_triples,
                             int64_t user_num, int64_t item_num, int32_t user_base, int32_t flags,
                             daisy_stream_t stream);
int daisy_train_index_destroy(daisy_train_index *index);
size_t daisy_train_index_bytes(const daisy_train_index *index);
/* same batches as daisy_epoch_plan_build on the same (order_mode, perm | seed, epoch, batch_size): batch k
 * holds the triples at epoch positions [k*B, (k+1)*B), grouped by user (CSR order inside a batch); its
 * entries are sorted by item, ties in CSR order */
int daisy_epoch_plan_build_indexed(daisy_epoch_plan *plan, const daisy_train_index *index,
                                   const int64_t *perm, int32_t order_mode, uint64_t seed, uint64_t epoch,
                                   int64_t batch_size, daisy_stream_t stream);
/* ONE RANK'S SHARE of an epoch (multi-GPU fit; the reference iterates one DataLoader on one device,
 * dataset.py:5-7 + AbstractRecommender.py:117-129).  `index` holds the rows this rank owns (its user range),
 * positions[r] in [0, n_total) is the place of the caller's row r in the epoch order of ALL n_total rows (distinct
 * values; int64).  Batch k = the held rows with position in [k*B, (k+1)*B): the union of the ranks' batches k is
 * exactly batch k of the single-device epoch.  Batches differ in size (possibly 0 rows:
 * daisy_epoch_plan_batch_rows); num_batches = ceil(n_total / B); one host sync per build.  Contexts that read the
 * plan need max_batch >= batch_size (stage slots are epoch positions minus k*B). */
int daisy_epoch_plan_build_positions(daisy_epoch_plan *plan, const daisy_train_index *index,
                                     const int64_t *positions, int64_t n_total, int64_t batch_size,
                                     daisy_stream_t stream);
/* The item pass of a multi-GPU step in item slices, so that the exchange of a finished slice (reduce-scatter, owner
 * update, all-gather) runs while the next slice is reduced.  item_bounds[0..n_slices] (host; item_bounds[0] = 0,
 * non-decreasing, item_bounds[n_slices] >= item_num; at most 16 slices) cut the items; _slices locates the cuts in
 * the current batch's item-sorted entries (one tiny kernel), _slice(s) writes gQ / cnt of the items of slice s like
 * daisy_bpr_staged_item(gQ, cnt).  Same counts; same gQ up to the order in which the partial sums of a long segment
 * meet (the cuts move workgroup boundaries); the same cuts give the same bits on every rank and in every run. */
int daisy_bpr_staged_item_slices(daisy_bpr_ctx *ctx, const int32_t *item_bounds, int32_t n_slices,
                                 daisy_stream_t stream);
int daisy_bpr_staged_item_slice(daisy_bpr_ctx *ctx, int32_t loss_type, float *gQ, float *cnt, int32_t slice,
                                float lr, float reg_1, float reg_2, const double *stats, daisy_stream_t stream);
/* The staged step with torch.optim.Adam on both tables (AbstractRecommender.py:54; ABI 4), lazy form: the rows the
 * current batch references are first brought to step `step`-1 (zero-gradient replays, see daisy_adam_lazy_catchup),
 * then the user pass and the item pass apply step `step` to the rows they own (moments m*, v*, stamps last*: the
 * state of daisy_adam_lazy_* / ops.LazyAdam; `table` = daisy_adam_lazy_table(lr, ...) copied to the device).  Rows no batch has
 * referenced stay behind until daisy_adam_lazy_flush.  Same arithmetic as daisy_adam_dense on every element.
 * FM biases (daisy_bpr_ctx_set_bias): their gradients go to g_u_bias / g_i_bias / stats[DAISY_ST_SUM_COEF] for the
 * caller's dense optimiser.  Every loss of loss.py:5-33; point-wise ones on point-wise batches. */
int daisy_bpr_staged_adam_step(daisy_bpr_ctx *ctx, float *P, float *Q, int32_t loss_type, float gamma, float lr,
                               float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP, float *mQ, float *vQ, int32_t *lastQ,
                               const float *table, float beta1, float beta2, float eps, int64_t step, double *stats,
                               double *epoch_acc, double *step_loss, daisy_stream_t stream);
/* The same in phases, for a multi-GPU step (user-sharded): the users' rows of P are rank-local
 * and keep the lazy form - catchup_users brings the rows the local batch references to step-1, staged_user_adam is
 * daisy_bpr_staged_user with the Adam owner update; the item side goes through the gradient form of
 * daisy_bpr_staged_item and, after the reduce-scatter, daisy_item_apply_counts_adam: torch's DENSE Adam over the owner's
 * block of Q (every row steps in every step; moments m, v [rows][d] of the block). */
int daisy_bpr_staged_adam_catchup_users(daisy_bpr_ctx *ctx, float *P, float *mP, float *vP, int32_t *lastP,
                                        const float *table, float beta1, float beta2, float eps, int64_t step,
                                        daisy_stream_t stream);
int daisy_bpr_staged_user_adam(daisy_bpr_ctx *ctx, float *P, const float *Q, int32_t loss_type, float gamma, float lr,
                               float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP, float beta1, float beta2,
                               float eps, int64_t step, double *stats, daisy_stream_t stream);
int daisy_item_apply_counts_adam(float *Q, float *g, float *cnt, float *m, float *v, int64_t rows, int32_t d, float lr,
                                 float reg_1, float reg_2, float beta1, float beta2, float eps, int64_t step,
                                 const double *stats, daisy_stream_t stream);
/* rows of batch k held by this plan (host value; -1: no such batch) */
int64_t daisy_epoch_plan_batch_rows(const daisy_epoch_plan *plan, int64_t k);

/* The staged step keeps |P[u]|^2 of every row in the context; every entry point that writes P through the
 * context keeps it current or drops it.  A caller that changes P by other means calls this first. */
int daisy_bpr_ctx_invalidate_cache(daisy_bpr_ctx *ctx);

/* Staged step, user pass: rows of P read and written PAST the caches (nontemporal loads + owner stores) - for user
 * tables so far beyond the 256 MB Infinity Cache that a row returns only once every few steps (then the cache is left to
 * Q and the stage).  mode -1 (default): automatic, on for tables > 512 MB (measured: -3.4 ... -5.1 % per step at
 * 10 M x 64, +0.7 ... +3 % at 1 M x 64); 0: off; 1: on.  Same arithmetic either way (MFRecommender.py:63-97): only the
 * cache policy of the accesses changes. */
int daisy_bpr_ctx_set_p_stream(daisy_bpr_ctx *ctx, int32_t mode);

/* The staged step in phases (what daisy_bpr_sgd_step(DAISY_ITEM_FUSED) runs back to back), so that a
 * multi-GPU step can put its collectives between them:
 *   prenorm : stats[DAISY_ST_SQ_U_PRE] = sum_b |P[u_b]|^2                      -> all-reduce (8 B)
 *   user    : forward + criterion + user-side backward + SGD on the touched rows of P
 *             (MFRecommender.py:63-97, AbstractRecommender.py:125-126); stats[0..6] = the batch sums
 *                                                                              -> all-reduce, daisy_bpr_finalize
 *   item    : item-side backward.  Q != NULL: + SGD on the touched rows of Q in place (needs the finalized
 *             norms in stats); gQ/cnt != NULL instead: gQ[r] = data term of dL/dQ[r] and cnt[r] = (number
 *             of positive, negative entries) f32[I][2] for the touched rows (others untouched: keep both
 *             zero between steps)                                             -> reduce-scatter both
 *   daisy_item_apply_counts : the row owner's SGD step from reduced (g, cnt): adds the regulariser
 *             share from the GLOBAL counts, clears g and cnt. */
int daisy_bpr_staged_prenorm(daisy_bpr_ctx *ctx, const float *P, double *stats, daisy_stream_t stream);
int daisy_bpr_staged_user(daisy_bpr_ctx *ctx, float *P, const float *Q, int32_t loss_type, float gamma,
                          float lr, float reg_1, float reg_2, double *stats, daisy_stream_t stream);
int daisy_bpr_staged_item(daisy_bpr_ctx *ctx, int32_t loss_type, float *Q, float *gQ, float *cnt, float lr,
                          float reg_1, float reg_2, const double *stats, daisy_stream_t stream);
int daisy_item_apply_counts(float *Q, float *g, float *cnt, int64_t rows, int32_t d, float lr, float reg_1,
                            float reg_2, const double *stats, daisy_stream_t stream);

/* batches set with daisy_bpr_set_batch / _from_triples are (user, item, label) rows (CL / SL) */
int daisy_bpr_ctx_set_pointwise(daisy_bpr_ctx *ctx, int32_t pointwise);
/* FM (FMRecommender.py:46-68): score(u,item) = <P[u],Q[item]> + u_bias[u] + i_bias[item] + bias_.
 * Attaches the bias parameters (device, caller-owned: u_bias f32[U], i_bias f32[I], bias f32[1]) to
 * the context; u_bias == NULL detaches them (plain MF).  From then on
 *   daisy_bpr_forward        adds them to both scores and reduces stats[DAISY_ST_SUM_COEF];
 *   daisy_bpr_item_grad*     accumulates g_i_bias[item] = sum of the item's coefficients (f32[I],
 *                            zero between steps like gQ; mandatory);
 *   daisy_bpr_item_sgd_apply does i_bias -= lr*g_i_bias and clears g_i_bias;
 *   daisy_bpr_user_sgd       does u_bias[u] -= lr*sum(cp+cn) and bias -= lr*stats[SUM_COEF];
 *   daisy_bpr_user_grad      writes g_u_bias[u] (f32[U]) and g_bias[0] instead (needed only for this
 *                            call; may be NULL otherwise) - dense Adam then runs daisy_adam_dense on them.
 * The regularisers of FM.calc_loss (FMRecommender.py:77-93) are those of MF: embeddings only.
 * DAISY_ITEM_FUSED (ABI 4): the staged step carries the biases itself - the user pass adds them to the scores and
 * updates u_bias[u] along each user run, the item pass i_bias[item] along each segment, bias from
 * stats[DAISY_ST_SUM_COEF] (SGD in place; daisy_bpr_staged_adam_step writes g_u_bias / g_i_bias instead). */
int daisy_bpr_ctx_set_bias(daisy_bpr_ctx *ctx, float *u_bias, float *i_bias, float *bias,
                           float *g_u_bias, float *g_i_bias, float *g_bias);
/* make batch k of a built plan current (no copy) */
int daisy_bpr_set_batch_from_plan(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, int64_t k,
                                  daisy_stream_t stream);
/* One collated batch outside a plan: rows idx[0..B) of the int32 [N,3] triple array
 * (idx == NULL: rows start..start+B); builds a one-batch plan inside the context. */
int daisy_bpr_set_batch_from_triples(daisy_bpr_ctx *ctx, const int32_t *triples, int64_t n_triples,
                                     const int64_t *idx, int64_t start, int64_t B,
                                     int32_t user_base, daisy_stream_t stream);
/* Same from three separate int32 arrays (what default_collate yields). */
int daisy_bpr_set_batch(daisy_bpr_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j,
                        int64_t B, daisy_stream_t stream);

/* MF.forward x2 + criterion (MFRecommender.py:63-68,73,83-85; loss.py): per-sample
 * d(loss)/d(pos), d(loss)/d(neg) kept in the context; the seven batch SUMS go
 * to stats[0..6]. */
int daisy_bpr_forward(daisy_bpr_ctx *ctx, const float *P, const float *Q, int32_t loss_type,
                      float gamma, double *stats, daisy_stream_t stream);

/* Regulariser + total loss of MF.calc_loss (MFRecommender.py:88-89,94-95) from the
 * (possibly all-reduced) sums: stats[7..10].  epoch_acc (device double[2], may
 * be NULL): [0] += loss  (`current_loss += loss.item()`, AbstractRecommender.py:128),
 * [1] += isnan(loss)     (AbstractRecommender.py:122-123).
 * step_loss (may be NULL) receives the step's loss. */
int daisy_bpr_finalize(daisy_bpr_ctx *ctx, double *stats, float reg_1, float reg_2,
                       double *epoch_acc, double *step_loss, daisy_stream_t stream);

/* autograd backward w.r.t. embed_item.weight, restricted to the touched rows
 * (AbstractRecommender.py:125): gQ[r] = dL/dQ[r] for every item r of the batch.
 * gQ must be all zero on entry (daisy_bpr_item_sgd_apply / daisy_adam_dense leave
 * it so). */
int daisy_bpr_item_grad(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                        float reg_1, float reg_2, float *gQ, int32_t item_mode,
                        daisy_stream_t stream);

/* The same gradient in two parts (chunked mode only), so that a multi-GPU step can form the
 * data term  sum_e c_e * p_u(e)  while the all-reduce of the batch sums is still in flight, and
 * add the regulariser share (which needs the global norms in stats[8..10]) afterwards. */
int daisy_bpr_item_grad_data(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                             float *gQ, int32_t item_mode, daisy_stream_t stream);
int daisy_bpr_item_grad_reg(daisy_bpr_ctx *ctx, const float *Q, const double *stats, float reg_1,
                            float reg_2, float *gQ, daisy_stream_t stream);

/* backward w.r.t. embed_user.weight + optim.SGD.step on the touched user rows
 * (AbstractRecommender.py:125-126).  Reads Q, so it must run BEFORE the item
 * rows are committed. */
int daisy_bpr_user_sgd(daisy_bpr_ctx *ctx, float *P, const float *Q, const double *stats, float lr,
                       float reg_1, float reg_2, daisy_stream_t stream);
/* same gradient written to gP[U][d] instead (dense optimisers) */
int daisy_bpr_user_grad(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                        float reg_1, float reg_2, float *gP, daisy_stream_t stream);

/* optim.SGD.step on the item table: Q[r] -= lr*gQ[r]; gQ[r] = 0 for the distinct
 * items of the current batch (dense != 0: every row, used after an all-reduce
 * of gQ). */
int daisy_bpr_item_sgd_apply(daisy_bpr_ctx *ctx, float *Q, float *gQ, float lr, int32_t dense,
                             daisy_stream_t stream);

/* torch.optim.Adam.step (defaults, AbstractRecommender.py:54), DENSE like the
 * reference: every element moves every step.  g is zeroed.  step is 1-based.
 * (The four dense optimisers - this one, Adagrad, RMSprop, SGD - are csrc/dense_opt.hip.) */
int daisy_adam_dense(float *W, float *g, float *m, float *v, int64_t n, float lr, float beta1,
                     float beta2, float eps, int64_t step, daisy_stream_t stream);

/* The same optimiser without moving every row in every step (MF tables; same result bit for bit).  A row's Adam
 * sequence depends only on its own gradients, so rows without a gradient are left behind and replayed in registers
 * when they are next needed: last[r] (int32, zero-initialised) = the step row r has been updated to.
 *   daisy_adam_lazy_table    host: table[2*s], table[2*s+1] = lr/(1-beta1^s), sqrt(1-beta2^s) for s = 1..n_steps
 *                            (float[2*(n_steps+1)], the host arithmetic of daisy_adam_dense); upload it once.
 *   daisy_adam_lazy_catchup  before the forward pass of step `step`: every row the current batch references is
 *                            brought to step-1 (zero-gradient steps replayed).
 *   daisy_adam_lazy_step     after the gradients: the referenced rows take step `step` with gP / gQ (cleared).
 *   daisy_adam_lazy_flush    all rows of one table to `step` (end of an epoch / of fit, before anything else reads
 *                            the table).
 * The batch is the context's current one (sorted plan layout or daisy_bpr_set_batch*). */
int daisy_adam_lazy_table(float lr, float beta1, float beta2, int64_t n_steps, float *table_host);
int daisy_adam_lazy_catchup(daisy_bpr_ctx *ctx, float *P, float *mP, float *vP, int32_t *lastP, float *Q, float *mQ,
                            float *vQ, int32_t *lastQ, const float *table, float beta1, float beta2, float eps,
                            int64_t step, daisy_stream_t stream);
int daisy_adam_lazy_step(daisy_bpr_ctx *ctx, float *P, float *gP, float *mP, float *vP, int32_t *lastP, float *Q,
                         float *gQ, float *mQ, float *vQ, int32_t *lastQ, const float *table, float beta1, float beta2,
                         float eps, int64_t step, daisy_stream_t stream);
int daisy_adam_lazy_flush(float *W, float *m, float *v, int32_t *last, int64_t rows, int32_t d, const float *table,
                          float beta1, float beta2, float eps, int64_t step, daisy_stream_t stream);

/* torch.optim.Adagrad.step / torch.optim.RMSprop.step with torch's defaults (AbstractRecommender.py:58,60;
 * Adagrad: lr_decay 0, eps 1e-10; RMSprop: alpha 0.99, eps 1e-8, no momentum), dense like the reference;
 * g is zeroed.  (optim.SparseAdam, :62, refuses the reference's dense embedding gradients at its first step:
 * the host mirror raises the same RuntimeError.) */
int daisy_adagrad_dense(float *W, float *g, float *state_sum, int64_t n, float lr, float eps,
                        daisy_stream_t stream);
int daisy_rmsprop_dense(float *W, float *g, float *square_avg, int64_t n, float lr, float alpha, float eps,
                        daisy_stream_t stream);

/* One whole `zero_grad / calc_loss / backward / SGD.step` on one GPU
 * (AbstractRecommender.py:119-128) for the batch set by daisy_bpr_set_batch*. */
int daisy_bpr_sgd_step(daisy_bpr_ctx *ctx, float *P, float *Q, int32_t loss_type, float gamma,
                       float lr, float reg_1, float reg_2, float *gQ, double *stats,
                       double *epoch_acc, double *step_loss, int32_t item_mode,
                       daisy_stream_t stream);

/* The inner `for batch in pbar` loop of GeneralRecommender.fit
 * (AbstractRecommender.py:118-128) for one epoch: every batch of a built plan,
 * enqueued natively with no host synchronisation.  step_losses (may be NULL)
 * gets one loss per step. */
int daisy_bpr_fit_epoch_sgd(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, float *P, float *Q,
                            int32_t loss_type, float gamma, float lr, float reg_1, float reg_2,
                            float *gQ, double *stats, double *epoch_acc, double *step_losses,
                            int32_t item_mode, daisy_stream_t stream);

/* The same loop with torch.optim.Adam (AbstractRecommender.py:54,118-128; ABI 6): every batch of a built plan through
 * daisy_bpr_staged_adam_step - steps first_step, first_step + 1, ... (the constants table must hold table_steps >=
 * first_step + num_batches - 1 steps) - enqueued natively: a reference run at its default batch (256 ... a few thousand
 * rows) is not bound by one host round trip per batch.  flush != 0: the rows no batch referenced are brought up to the
 * epoch's last step (daisy_adam_lazy_flush on both tables), i.e. both tables equal the dense optimiser's after the
 * epoch.  MF only: contexts with FM biases are driven step by step (their biases step through the caller's dense
 * optimiser between two steps) and are refused. */
int daisy_bpr_fit_epoch_adam(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, float *P, float *Q, int32_t loss_type,
                             float gamma, float lr, float reg_1, float reg_2, float *mP, float *vP, int32_t *lastP,
                             float *mQ, float *vQ, int32_t *lastQ, const float *table, int64_t table_steps, float beta1,
                             float beta2, float eps, int64_t first_step, int32_t flush, double *stats,
                             double *epoch_acc, double *step_losses, daisy_stream_t stream);

/* ABI 7.  1 when the epochs of `plan` (built, sorted layout: daisy_epoch_plan_build) run inside ONE persistent workgroup
 * (csrc/bpr_small.hip: batches of at most 256 samples - the reference's default, basic.yaml:23 -, pairwise losses, no FM
 * biases, rows that fit the LDS); daisy_bpr_fit_epoch_sgd takes that path by itself, and daisy_bpr_fit_epoch_adam accepts
 * a sorted-layout plan exactly when this returns 1 (AbstractRecommender.py:54,103-137: the loop body at B = 256 is bound
 * by kernel boundaries, not by bytes: SGD 8.7 us, Adam 48 -> 35 us per step at ml-100k shapes).  Bit 0: supported; bit 1
 * (value 3): the Adam form is also expected to beat the chain of launches - tables of at most 32 rows per sample of a batch,
 * so that the rows a step references sat out a few steps, not thousands (its zero-gradient replay is the cost). */
int daisy_bpr_small_epoch_supported(const daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, int32_t loss_type);

/* One SGD epoch of MANY independent models in one call (a grid over lr / reg / factors, the folds of a cross-validation,
 * the trials of a search: tune.py's `hyperopt_trail` x `fold_num` fits): the small-batch epoch keeps one workgroup - one CU -
 * busy, so `count` models are `count` workgroups of one launch per kernel shape instead of `count` epochs one after another.
 * Every trial is what one daisy_bpr_fit_epoch_sgd call takes (without gQ and the item mode) and ends with the same bits in
 * P, Q, stats, epoch_acc and step_losses (may be NULL) as that call.  Every trial must be a small-batch epoch
 * (daisy_bpr_small_epoch_supported & 1) whose plan fits its context; two trials may share a plan, which is only read, but
 * not P, Q, stats or epoch_acc; all on one device.  A violation is DAISY_ERR_ARG naming the trial, before anything is
 * launched.  workspace: device memory of at least count * DAISY_SMALL_TRIAL_WS_BYTES bytes, not reused before the
 * stream has passed the call.  count == 0 is DAISY_OK. */
#define DAISY_SMALL_TRIAL_WS_BYTES 192
typedef struct daisy_small_trial {
    daisy_bpr_ctx *ctx;
    const daisy_epoch_plan *plan;
    float *P, *Q;
    int32_t loss_type;
    float gamma, lr, reg_1, reg_2;
    double *stats, *epoch_acc, *step_losses;
} daisy_small_trial;
int daisy_bpr_fit_epoch_sgd_many(const daisy_small_trial *trials, int32_t count, void *workspace, size_t workspace_bytes,
                                 daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Scoring / ranking  (MFRecommender.py:99-133)
 * ---------------------------------------------------------------------- */
/* MF.forward (MFRecommender.py:63-68): out[b] = <P[u_b], Q[i_b]> */
int daisy_mf_predict(const float *P, const float *Q, int32_t d, const int64_t *u, const int64_t *i,
                     int64_t B, float *out, daisy_stream_t stream);
size_t daisy_mf_rank_workspace_bytes(int64_t B, int64_t C);
/* MF.rank inner loop (MFRecommender.py:109-121): scores = bmm, argsort descending
 * (stable), gather candidate ids, first topk -> out_ids int64 [B][topk].
 * scores_out (may be NULL) receives the fp32 [B][C] score matrix. */
int daisy_mf_rank_topk(const float *P, const float *Q, int32_t d, const int64_t *us,
                       const int64_t *cands, int64_t B, int64_t C, int32_t topk, int64_t *out_ids,
                       float *scores_out, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream);
size_t daisy_mf_full_rank_workspace_bytes(int64_t item_num);
/* FM.predict / rank / full_rank (FMRecommender.py:95-133): the MF entry points plus
 * `+ (u_bias[u] + i_bias[item]) + bias[0]` on every score, in the reference's order of additions;
 * same workspaces; u_bias == NULL gives the MF result. */
int daisy_fm_predict(const float *P, const float *Q, const float *u_bias, const float *i_bias,
                     const float *bias, int32_t d, const int64_t *u, const int64_t *i, int64_t B,
                     float *out, daisy_stream_t stream);
int daisy_fm_rank_topk(const float *P, const float *Q, const float *u_bias, const float *i_bias,
                       const float *bias, int32_t d, const int64_t *us, const int64_t *cands,
                       int64_t B, int64_t C, int32_t topk, int64_t *out_ids, float *scores_out,
                       void *workspace, size_t workspace_bytes, daisy_stream_t stream);
int daisy_fm_full_rank(const float *P, const float *Q, const float *u_bias, const float *i_bias,
                       const float *bias, int32_t d, int64_t item_num, int64_t u, int32_t topk,
                       int64_t *out_ids, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream);
/* MF.full_rank (MFRecommender.py:126-133): argsort(P[u] @ Q^T, descending)[:topk] */
int daisy_mf_full_rank(const float *P, const float *Q, int32_t d, int64_t item_num, int64_t u,
                       int32_t topk, int64_t *out_ids, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream);
/* Full ranking of n users in two launches (csrc/rank_full.hip, additive to ABI 8): for every users[b] (int64 [n], any
 * order, duplicates allowed) the topk items of all item_num by score <P[u], Q[i]> (+ (u_bias[u] + i_bias[i]) + bias[0]
 * when the three are given: all NULL or none), best first, equal scores by ascending item id (-0.0 equals +0.0, a NaN
 * score ranks first), without the items of the user's exclusion row.  P and Q are fp32 rows of d columns (the padded
 * tables are fine: zero columns add zero).  The exclusion is a device CSR over all users - excl_indptr int64
 * [user_num + 1], excl_items int32, ascending inside a row, duplicates allowed, exactly what daisy_build_user_csr
 * returns (both NULL: nothing excluded).  Row contents are only compared, never used as an index: a row that breaks
 * the contract may cost missed exclusions, never an out-of-bounds access; user ids and excl_indptr are the caller's
 * to validate.  out_ids int64 [n, topk], out_scores fp32 [n, topk] or NULL; positions beyond a user's eligible items
 * hold id -1 and score -inf.  1 <= topk <= min(item_num, 128): the candidate buffers live in LDS, and a larger topk is
 * DAISY_ERR_ARG with the cap in the message, never a truncation.  item_slices: 0 picks the number of item slices per
 * user tile from the tile counts, another value is clamped to the number of 128-item tiles; the result does not
 * depend on it, bit for bit.  Nothing of size n * item_num is allocated: the workspace holds item_slices partial top-k
 * lists per user.  Every argument is checked before the first HIP call. */
size_t daisy_full_rank_users_workspace_bytes(int64_t n, int64_t item_num, int32_t topk, int32_t item_slices);
int daisy_full_rank_users(const float *P, const float *Q, const float *u_bias, const float *i_bias, const float *bias,
                          int32_t d, int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                          const int32_t *excl_items, int32_t topk, int32_t item_slices, int64_t *out_ids,
                          float *out_scores, void *workspace, size_t workspace_bytes, daisy_stream_t stream);
/* Exact ranks of held-out items over all items (csrc/rank_positions.hip; additive to ABI 8).  P, Q, the
 * bias triple, d, item_num, users [n], the exclusion CSR and item_slices are daisy_full_rank_users'.  t_indptr int64
 * [user_num + 1] / t_items int32: the TARGET CSR over all users, ascending inside a row (daisy_build_user_csr's).
 * out_indptr int64 [n + 1]: the prefix sum of the target-row lengths of users[0 .. n), built by the caller; n_targets =
 * out_indptr[n].  With word(u, j) = (key of the fp32 score << 32) | (0xFFFFFFFF - j) of daisy_full_rank_users and E_u the
 * items of [0, item_num) outside u's exclusion row, request b's target number r (row order) gets
 *   out_pos[out_indptr[b] + r]   int32: #{ j in E_u : word(u, j) > word(u, t) } - its 0-based rank, score descending, a
 *                                NaN first, equal scores by ascending id; -1 for a target outside [0, item_num) (it is
 *                                range-checked before it indexes anything) or inside the exclusion row
 *   out_scores[...]              fp32 or NULL: the target's score, bit for bit daisy_full_rank_users'; -inf where pos = -1
 *   out_eligible[b]              int32 or NULL: |E_u|
 * so that with the same arguments daisy_full_rank_users' ids[b][pos] == t for every target with 0 <= pos < topk.  There
 * is no cap on the row length (a row is split into blocks of 32 targets on the device).  The counts are integer atomics:
 * the result does not depend on item_slices, the schedule or the run, bit for bit.  Row contents of the exclusion are
 * only compared; user ids, the indptr arrays and out_indptr are the caller's to validate.  Every argument is checked
 * before the first HIP call. */
size_t daisy_full_rank_positions_workspace_bytes(int64_t n, int64_t n_targets);
int daisy_full_rank_positions(const float *P, const float *Q, const float *u_bias, const float *i_bias, const float *bias,
                              int32_t d, int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                              const int32_t *excl_items, const int64_t *t_indptr, const int32_t *t_items,
                              const int64_t *out_indptr, int64_t n_targets, int32_t item_slices, int32_t *out_pos,
                              float *out_scores, int32_t *out_eligible, void *workspace, size_t workspace_bytes,
                              daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Uniform negative sampler (sampler.py:55-103, uniform branch :82-89)
 * ---------------------------------------------------------------------- */
size_t daisy_csr_workspace_bytes(int64_t n);
/* get_ur (utils.py:19-34) as a CSR: for n (user,item) pairs build indptr int64[U+1]
 * and the per-user SORTED item lists int32[n] (pairs must be duplicate free,
 * as loader.py:201 guarantees). */
int daisy_build_user_csr(const int32_t *users, const int32_t *items, int64_t n, int64_t user_num,
                         int64_t *indptr, int32_t *csr_items, void *workspace,
                         size_t workspace_bytes, daisy_stream_t stream);
/* js[u][k], k<num_ng, for EVERY user id (sampler.py:63,84-89): uniform with
 * replacement over {0..item_num-1} minus the user's CSR row; -1 if that set is
 * empty.  Counter-based Philox4x32-10: stream = epoch, index = u*num_ng+k. */
int daisy_sample_neg_per_user(const int64_t *indptr, const int32_t *csr_items, int64_t user_num,
                              int64_t item_num, int32_t num_ng, uint64_t seed, uint64_t epoch,
                              int32_t *js, daisy_stream_t stream);
/* SkipGramNegativeSampler.sampling (sampler.py:133-155, Item2Vec's sampler): the user sequences (items in train-set
 * order, seq_items[n] with seq_ptr[U+1] and the owner seq_user[n] of every element), the window half-width, the
 * users' train rows as a CSR with sorted distinct items.  Element e writes rows [row_offsets[e], row_offsets[e+1]) of
 * out (int32 [rows][3]): its (target, context, 1) rows in window order, then as many (target, negative, 0) rows with
 * negatives uniform from the complement of its user's row (Philox(seed, stream_id, row/2 + k)); row_offsets = the
 * exclusive scan of 2 * (window size of e).  bad_flag |= 1 when a user has no negative to draw. */
int daisy_skipgram_samples(const int32_t *seq_items, const int32_t *seq_user, const int64_t *seq_ptr,
                           const int64_t *row_offsets, int64_t n, int32_t context_window, const int64_t *ur_indptr,
                           const int32_t *ur_items, int64_t item_num, uint64_t seed, uint64_t stream_id, int32_t *out,
                           int32_t *bad_flag, daisy_stream_t stream);
/* sampler.py:76-80, the 'high-pop' / 'low-pop' share of a user's negatives: k draws per row from the categorical
 * distribution whose inclusive cumulative sums are cdf[0..item_num) (float64, any positive total), by inverse CDF on
 * Philox(seed, stream_id, row*k + c); written to out[row*ld + col0 + c].  Like np.random.choice(p=...) in the
 * reference, the draws do not exclude the user's positives. */
int daisy_sample_categorical(const double *cdf, int64_t item_num, int64_t rows, int32_t k, uint64_t seed,
                             uint64_t stream_id, int32_t *out, int32_t ld, int32_t col0, daisy_stream_t stream);
/* df.explode('neg_set') (sampler.py:91,100-101): triples int32 [n*num_ng][3] in
 * train-set row order, each interaction repeated num_ng times. */
int daisy_expand_triples(const int32_t *users, const int32_t *items, int64_t n, const int32_t *js,
                         int32_t num_ng, int32_t *triples, daisy_stream_t stream);
/* per-interaction variant (fresh negatives for every triple, re-drawable per
 * epoch): rewrites column 2 of triples [n][3] in place. */
int daisy_resample_neg_per_interaction(const int64_t *indptr, const int32_t *csr_items,
                                       int64_t item_num, int32_t *triples, int64_t n,
                                       uint64_t seed, uint64_t epoch, daisy_stream_t stream);

/* build_candidates_set (utils.py:53-85): for each of n_users test users (ids in `users`)
 * cand_num candidates int64 [n_users][cand_num]: uniform negatives (with replacement) from
 * the items in neither the user's test CSR row nor train CSR row, then the test items in
 * ascending order; a user with more than cand_num test items gets cand_num draws from them.
 * The two rows of a user must be disjoint (they are, by construction of the split). */
int daisy_build_candidates(const int64_t *indptr_test, const int32_t *items_test,
                           const int64_t *indptr_train, const int32_t *items_train,
                           const int64_t *users, int64_t n_users, int64_t item_num,
                           int32_t cand_num, uint64_t seed, int64_t *out, daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side epoch order (replaces RandomSampler's torch.randperm for the
 * throughput loader; dataset.py:5-7 shuffle=True): perm = a uniformly random
 * permutation of 0..n-1 derived from (seed, epoch) by sorting Philox keys.
 * ---------------------------------------------------------------------- */
size_t daisy_randperm_workspace_bytes(int64_t n);
int daisy_randperm(int64_t n, uint64_t seed, uint64_t epoch, int64_t *perm, void *workspace,
                   size_t workspace_bytes, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * NeuMF (daisy/model/NeuMFRecommender.py:15-233)
 *   GMF branch  g = uG[u] * iG[item]                                  (:119-122)
 *   MLP branch  x0 = [uM[u] | iM[item]];  x_l = ReLU(Linear_l(Dropout(x_{l-1}))), l = 1..L   (:60-66,123-127)
 *   pred = predict_layer(concat(g, x_L))            (model GMF / MLP: one branch only)  (:129-137)
 * The MLP tower runs on the matrix cores (fp32 MFMA tiles, bias+ReLU+dropout fused into the
 * epilogue; backward data/weight GEMMs with the ReLU gate fused); gathers, the loss epilogue
 * (shared with MF: daisy_loss ids) and the embedding-gradient scatter are HBM-bound kernels.
 * Parameters stay caller-owned (the nn.Module's tensors), passed as a table of device pointers.
 * ---------------------------------------------------------------------- */
#define DAISY_NEUMF_MAX_LAYERS 8
typedef enum { DAISY_NEUMF_FULL = 0, DAISY_NEUMF_GMF = 1, DAISY_NEUMF_MLP = 2 } daisy_neumf_model;
typedef struct {
    float *uG, *iG;                       /* embed_user_GMF [U,d], embed_item_GMF [I,d]            */
    float *uM, *iM;                       /* embed_user_MLP [U,dm], embed_item_MLP [I,dm], dm = d*2^(L-1) */
    float *W[DAISY_NEUMF_MAX_LAYERS];     /* Linear l weight [n_l/2, n_l] row-major, n_1 = 2*dm (:61-65) */
    float *b[DAISY_NEUMF_MAX_LAYERS];     /* Linear l bias   [n_l/2]                                */
    float *Wp, *bp;                       /* predict_layer weight [1, d or 2d], bias [1]   (:68-73) */
} daisy_neumf_params;
/* stats vector of a training step (device, double[DAISY_NEUMF_STATS_LEN]) */
enum {
    DAISY_NST_LOSS_DATA = 0,                         /* sum of the criterion terms                  */
    DAISY_NST_L1 = 1,  /* +0 uG[u], +1 uM[u], +2 iG[i], +3 iM[i], +4 iG[j]: sum |x| over the batch */
    DAISY_NST_SQ = 6,  /* same five, sum x^2                                                        */
    DAISY_NST_LOSS = 11,                             /* NeuMF.calc_loss value (:139-169)             */
    DAISY_NST_NORM = 12,                             /* same five, Frobenius norms                   */
    DAISY_NST_LOSS_SUM = 17,  /* running sum of DAISY_NST_LOSS over the steps since the caller zeroed it: a step   */
                              /* clears slots 0..16 only (an epoch's loss without a launch per step to add it up) */
    DAISY_NEUMF_STATS_LEN = 24
};
typedef struct daisy_neumf_ctx daisy_neumf_ctx;
/* activation workspace for up to max_rows (user,item) pairs per call (a training batch of B
 * pairwise samples forwards 2B rows).  factors % 4 == 0, 1 <= num_layers <= DAISY_NEUMF_MAX_LAYERS. */
int daisy_neumf_ctx_create(daisy_neumf_ctx **out, int64_t max_rows, int32_t factors, int32_t num_layers,
                           int32_t model, int64_t user_num, int64_t item_num);
int daisy_neumf_ctx_destroy(daisy_neumf_ctx *ctx);
size_t daisy_neumf_ctx_bytes(const daisy_neumf_ctx *ctx);
/* bf16_gemm = 1: the MLP tower's GEMMs round their fp32 operands to bf16 on the way into LDS and run
 * v_mfma_f32_32x32x16_bf16 (fp32 accumulate) wherever the tile shape allows (128-row / 64|128-column
 * multiples, K multiple of 32, 16-byte aligned operands; other shapes stay fp32).
 * bf16_gemm = 2 (BASELINE configs[3] "MLP via MFMA bf16"): the activations X_l, the back-propagated dZ_l and a
 * per-call copy of the MLP weights are STORED as bf16 in HBM as well (half the operand traffic, which is what
 * bounds level 1); embeddings, GMF branch, weight gradients and the optimiser stay fp32.  Applies to calls
 * whose row count is a multiple of 128 and whose layer widths are multiples of 64, level 1 otherwise.
 * Throughput modes: results differ from the fp32 parity mode by bf16 rounding (~3 significant digits).
 * Default: 0. */
int daisy_neumf_ctx_set_precision(daisy_neumf_ctx *ctx, int32_t bf16_gemm);
/* NeuMF.forward in eval mode (:118-137) on n pairs -> out f32[n]; processed in chunks of max_rows.
 * Pairs are given in one of three layouts (the three callers of the reference):
 *   users/items i64[n]                                   predict (:171-176), forward
 *   users i64[B], items = cands i64[B*C], C > 0          rank  (:178-209): user of pair e = users[e / C]
 *   users i64[1], items == NULL, C == 0                  full_rank (:211-233): item of pair e = e   */
int daisy_neumf_scores(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const int64_t *users,
                       const int64_t *items, int64_t n, int64_t C, float *out, daisy_stream_t stream);
/* "These users x all items" (additive to ABI 8): out f32[m][item_num], out[b][i] = the eval-mode score of
 * (users[b], i), users i64[m] in any order, duplicates allowed.  The m * item_num pairs run through the forward code of
 * daisy_neumf_scores in pieces of max_rows - pair e = (users[e / item_num], e % item_num), formed in the gather: no
 * candidate array of m * item_num ids exists.  A pair's score is computed by the same instructions as there; in the
 * bf16 levels its bits depend on the piece's row count exactly as they do there (level 2 needs whole 128-row tiles). */
int daisy_neumf_scores_users(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const int64_t *users, int64_t m,
                             float *out, daisy_stream_t stream);
/* One training batch of NeuMF.calc_loss + backward (:139-169): rows (u, i, j) int32[B] (point-wise
 * losses: j = label).  ACCUMULATES the dense gradients into `grads` (same table layout; zero before
 * the first step, the optimiser kernels below clear what they consume) and writes stats.
 * dropout_p in [0,1): keep masks come from a counter hash of (seed, layer, row, column) - a fresh
 * `seed` per step gives fresh masks; p == 0 is the deterministic path the golden vectors pin. */
int daisy_neumf_step_grads(daisy_neumf_ctx *ctx, const daisy_neumf_params *params,
                           const daisy_neumf_params *grads, const int32_t *u, const int32_t *i,
                           const int32_t *j, int64_t B, int32_t loss_type, float gamma, float reg_1,
                           float reg_2, float dropout_p, uint64_t seed, double *stats,
                           daisy_stream_t stream);
/* One epoch of the reference's training loop (AbstractRecommender.py:112-128: zero_grad / calc_loss / backward /
 * optimizer.step per batch) over the batches [s, s+batch) of the n samples (u, i, j), issued from the library: step k
 * (1-based, counted on from step0) = daisy_neumf_step_grads with seed = seed_hi | (step0 + k), then the dense optimiser
 * (0 SGD, 1 Adam, 2 Adagrad, 3 RMSprop: torch defaults, the daisy_*_dense kernels) on the flat parameter vector W and
 * its gradient g (n_flat floats: every tensor of `params` / `grads` is a view into them; state0 / state1: exp_avg /
 * exp_avg_sq, state_sum, square_avg; Adam's step count is step0 + k).  stats[DAISY_NST_LOSS_SUM] grows by the
 * steps' losses.  Same kernels as the per-step calls - what it removes is the host's per-step work. */
int daisy_neumf_fit_epoch(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const daisy_neumf_params *grads,
                          const int32_t *u, const int32_t *i, const int32_t *j, int64_t n, int64_t batch, int32_t loss_type,
                          float gamma, float reg_1, float reg_2, float dropout_p, uint64_t seed_hi, int64_t step0,
                          int32_t optimizer, float lr, float *W, float *g, float *state0, float *state1, int64_t n_flat,
                          double *stats, daisy_stream_t stream);
/* optim.SGD step on one dense tensor: W -= lr*g; g = 0   (AbstractRecommender.py:56; csrc/dense_opt.hip) */
int daisy_sgd_dense(float *W, float *g, int64_t n, float lr, daisy_stream_t stream);
/* the argsort / top-k tail of every rank(): scores f32[B,C] (+ candidate ids i64[B,C]) -> ids of the
 * topk best per row, stable descending like torch.argsort(descending=True); workspace as
 * daisy_mf_rank_workspace_bytes(B, C).  full-rank variant: scores f32[I] -> item ids i64[topk],
 * workspace as daisy_mf_full_rank_workspace_bytes(I). */
int daisy_topk_from_scores(const float *scores, const int64_t *cands, int64_t B, int64_t C, int32_t topk,
                           int64_t *out_ids, void *workspace, size_t workspace_bytes,
                           daisy_stream_t stream);
int daisy_full_topk_from_scores(const float *scores, int64_t item_num, int32_t topk, int64_t *out_ids,
                                void *workspace, size_t workspace_bytes, daisy_stream_t stream);
/* The MFMA products of csrc/gemm.hip (NeuMF's tower and Multi-VAE's layers run on them) as entry points of their own:
 * C[M,N] = A[M,K] * B[N,K]^T on the fp32 MFMA tile kernel the MLP tower uses (test / bench hook) */
int daisy_gemm_nt_f32(const float *A, const float *B, float *C, int64_t M, int32_t N, int32_t K,
                      daisy_stream_t stream);
/* C[M,N] = A[M,K] * B[N,K]^T with all three matrices stored as bf16 (fp32 accumulate, round to nearest even): the
 * GEMM of precision level 2 (test / bench hook); M % 128 == 0, N % 64 == 0 (% 128 when N > 64), K % 32 == 0 */
int daisy_gemm_nt_bf16(const uint16_t *A, const uint16_t *B, uint16_t *C, int64_t M, int32_t N, int32_t K,
                       daisy_stream_t stream);
/* C[M,N] (fp32, accumulated into: zero it first) += At[K,M]^T * Bt[K,N] with both operands stored as bf16 and
 * contiguous along their rows, the reduction over K cut into k_chunk slices that add with fp32 atomics: the
 * weight-gradient GEMM of precision level 2, gW = dZ^T X (NeuMFRecommender.py:139-169 through autograd; test / bench
 * hook); M % 128 == 0, N % 64 == 0 (% 128 when N > 64), K % 32 == 0, k_chunk % 32 == 0 */
int daisy_gemm_tn_bf16(const uint16_t *At, const uint16_t *Bt, float *C, int64_t M, int32_t N, int64_t K,
                       int64_t k_chunk, daisy_stream_t stream);
/* same with the precision switch of daisy_neumf_ctx_set_precision */
int daisy_gemm_nt(const float *A, const float *B, float *C, int64_t M, int32_t N, int32_t K, int32_t bf16,
                  daisy_stream_t stream);
/* One product through any launcher of csrc/gemm.hip (test hook): C(m,n) = epilogue(sum_k A(m,k) B(n,k)) with
 * A(m,k) = A[m*sam + k*sak], B(n,k) = B[n*sbn + k*sbk], C(m,n) = C[m*ldc + n*scn] (scn 0 means 1), strides in elements.
 * k_chunk < K cuts the k range into slices (DAISY_GEMM_EPI_ATOMIC only): slice z is STORED at C + z*slice_stride, or,
 * with slice_stride 0, all slices are added into C with fp32 atomics (so is a single slice).
 * Before anything is launched every index the product can touch is checked against the element counts n_*, and the
 * shape against what the launcher takes: a descriptor that fails is DAISY_ERR_ARG with the field's name in the message.
 * `path` receives what the launcher resolved: family (0 k_gemm, 1 k_gemm_bf16, 2 k_gemm_h, 3 k_gemm_pair) | WN << 2 |
 * FAST << 4 | DROP << 5 | AK << 6 | BK << 7 | k slices << 8 | (pair: k slices of the second product) << 20.
 * dry_run != 0: check, resolve, write `path` and return - no HIP call is made and no pointer but the descriptors' own is
 * read (the alignment of A, B, C and gate still decides the path). */
#define DAISY_GEMM_LAUNCH 0       /* launch_gemm: fp32 storage (bf16 != 0: bf16 MFMA inputs where the shape allows) */
#define DAISY_GEMM_LAUNCH_H 1     /* launch_gemm_h: A and B stored as bf16; C and gate bf16 (c_bf16) or fp32 */
#define DAISY_GEMM_LAUNCH_PAIR 2  /* launch_gemm_pair: two fp32 products of the same N in one launch */
#define DAISY_GEMM_EPI_STORE 0
#define DAISY_GEMM_EPI_BIAS_RELU 1 /* max(acc + bias[n], 0) */
#define DAISY_GEMM_EPI_GATE 2      /* acc * (gate[m*ldg + n] > 0 ? gate_scale : 0); gate NULL: acc */
#define DAISY_GEMM_EPI_ATOMIC 3
typedef struct daisy_gemm_desc {
    int32_t launcher, epilogue;
    int32_t bf16;                 /* DAISY_GEMM_LAUNCH: the throughput-mode flag of GemmOp */
    int32_t c_bf16;               /* DAISY_GEMM_LAUNCH_H, BIAS_RELU / GATE: C (and gate) are bf16; 0: fp32 */
    const void *A, *B;
    void *C;
    const float *bias;            /* f32[N] */
    const void *gate;
    int64_t sam, sak, sbn, sbk, ldc, scn, ldg;
    int64_t M, N, K, k_chunk, slice_stride;
    int64_t n_A, n_B, n_C, n_bias, n_gate;      /* elements of each buffer */
    float gate_scale;
    float drop_p;                 /* BIAS_RELU / GATE: dropout of output element m*N + n at probability drop_p (0: off) */
    uint64_t drop_seed;
    uint32_t drop_stream;
    int32_t dry_run;
    uint32_t path;                /* out */
    uint32_t reserved;
} daisy_gemm_desc;
/* b != NULL: the pair a, b through launch_gemm_pair (both descriptors name DAISY_GEMM_LAUNCH_PAIR, the same epilogue -
 * STORE or ATOMIC - and the same N); a's dry_run decides, both receive `path`. */
int daisy_gemm_case(daisy_gemm_desc *a, daisy_gemm_desc *b, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * LightGCN (daisy/model/LightGCNRecommender.py:17-210)
 *   A_hat = D^-1/2 A D^-1/2 over the N = U + I nodes of the bipartite interaction graph  (:74-107)
 *   out   = mean(E_0, A_hat E_0, ..., A_hat^L E_0),  E_0 = [embed_user; embed_item]        (:117-129)
 * and the BPR (or HL/TL/CL/SL) loss of MF on the rows of `out`, regularisers on the rows of E_0
 * (:131-169).  The propagation is a sparse x dense product: HBM-bound row gathers + a segmented
 * reduction, run on the same kernel as MF's item pass.  The loss / gradient-wrt-out part IS the MF
 * path (daisy_bpr_forward / _item_grad_data / _user_grad on the two halves of `out`); these entry
 * points add the graph, the propagation and its transpose (A_hat is symmetric).
 * ---------------------------------------------------------------------- */
typedef struct daisy_lgcn_graph daisy_lgcn_graph;
/* build A_hat from the training interactions (device int32[n] each; duplicate pairs collapse like the
 * reference's dict, :88-90).  Values are formed in float64 and stored as float32 like scipy -> torch
 * (:93-105).  Synchronises the stream once (number of distinct pairs). */
int daisy_lgcn_graph_create(daisy_lgcn_graph **out, const int32_t *users, const int32_t *items, int64_t n,
                            int64_t user_num, int64_t item_num, daisy_stream_t stream);
int daisy_lgcn_graph_destroy(daisy_lgcn_graph *g);
int64_t daisy_lgcn_graph_nnz(const daisy_lgcn_graph *g);          /* stored entries = 2 x distinct pairs */
/* flag != 0: the products use a row-owner kernel that sums every row's entries in stored order (bitwise
 * reproducible, slower on long rows) instead of the chunked segmented reduction (whose rows that span
 * three or more chunks are combined with fp32 atomics in arrival order).  Default 0. */
int daisy_lgcn_graph_set_reproducible(daisy_lgcn_graph *g, int32_t flag);
size_t daisy_lgcn_graph_bytes(const daisy_lgcn_graph *g);
/* COO copy of A_hat, rows then columns ascending (inspection / tests): int32[nnz], int32[nnz], f32[nnz] */
int daisy_lgcn_graph_read(const daisy_lgcn_graph *g, int32_t *row, int32_t *col, float *val,
                          daisy_stream_t stream);
/* Y = A_hat X, X and Y f32[N, d] (Y != X) */
int daisy_lgcn_spmm(const daisy_lgcn_graph *g, const float *X, float *Y, int32_t d, daisy_stream_t stream);
/* Rows [row_lo, row_hi) of the same product: Yrows[r - row_lo] = (A_hat X)[r] - the per-rank share of a
 * row-sharded multi-GPU propagation (BASELINE configs[4]; the ranks all-gather their row blocks per layer).
 * Yrows must be preceded and followed by one spare row of d floats (they may be overwritten).  The first call
 * on a graph synchronises the stream once (row offsets). */
int daisy_lgcn_spmm_rows(const daisy_lgcn_graph *g, const float *X, float *Yrows, int32_t d, int64_t row_lo,
                         int64_t row_hi, daisy_stream_t stream);
/* LightGCN.forward (:117-129): out = mean_k A_hat^k E0;  work: f32[2*N*d] scratch */
int daisy_lgcn_propagate(const daisy_lgcn_graph *g, const float *E0, int32_t d, int32_t num_layers,
                         float *work, float *out, daisy_stream_t stream);
/* its transpose applied to the gradient G = dL/d out:  dE0 += 1/(L+1) sum_k A_hat^k G */
int daisy_lgcn_backprop(const daisy_lgcn_graph *g, const float *G, int32_t d, int32_t num_layers, float *work,
                        float *dE0, daisy_stream_t stream);
/* regulariser gradient on the ego rows of one batch (:150-163): for every sample
 * dE0[row] += reg_1*sign(e) + reg_2*e/|rows|_F for row in (u, U+i, U+j [pairwise only]); the three
 * Frobenius norms are stats[DAISY_ST_NORM_U/I/J] of a finalized MF context whose sums were taken on E0.
 * Deterministic: occurrences are counted with integer atomics into count_ws (int32[2*(U+I)], all zero on
 * entry, left all zero), then every touched row is updated once. */
int daisy_lgcn_reg_grad(const float *E0, const int32_t *u, const int32_t *i, const int32_t *j, int64_t B,
                        int64_t user_num, int64_t item_num, int32_t d, int32_t pointwise, float reg_1,
                        float reg_2, const double *stats, int32_t *count_ws, float *dE0,
                        daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * NGCF (daisy/model/NGCFRecommender.py:62-252): the LightGCN adjacency A_hat plus one dense bi-interaction
 * layer per hidden width.  Layer k maps E = E^{k-1} [N, d_in] to E^k [N, d_out]:
 *   X   = A_hat_drop E                                        daisy_lgcn_spmm_ex (node dropout: A_hat_drop)
 *   Z   = (E + X) W1^T + b1 + (X * E) W2^T + b2               one GEMM, K = 2 d_in: [S | T] [W1 | W2]^T
 *   Y   = normalize(dropout_p(LeakyReLU_0.2(Z)))              row L2 norm, clamp 1e-12 (F.normalize)
 * E and Y are column slices of the concat buffer out = [E^0 | E^1 | ... | E^L] (row pitches lde / ldy).  Widths
 * d_in, d_out are 1..DAISY_NGCF_MAX_WIDTH.  W1, W2 are nn.Linear weights [d_out][d_in], b1, b2 [d_out].
 * Dropout keep bits are a counter hash of (seed, stream, index): message dropout of layer k uses stream
 * DAISY_NGCF_MESS_STREAM + k and index r * d_out + c; node dropout uses DAISY_NGCF_NODE_STREAM and the index
 * of the stored entry of A_hat (daisy_lgcn_graph_read order).  Kept values are scaled by 1 / (1 - p).
 * ---------------------------------------------------------------------- */
#define DAISY_NGCF_MAX_WIDTH 256
#define DAISY_NGCF_NODE_STREAM 0x100u
#define DAISY_NGCF_MESS_STREAM 0x200u
/* Y = A_hat_drop X (or its transpose), X and Y f32 row slices of pitch ldx / ldy (>= d), d in 1..512, X and Y
 * distinct.  accumulate != 0: Y += instead of Y =.  node_p in [0, 1): node dropout of the stored entries
 * (seed as above; 0: A_hat itself).  transpose != 0: A_hat_drop^T - the same entries with the keep bit of
 * each entry's mirror (A_hat is symmetric, the masked matrix is not).  Row-owner kernel: every row is summed
 * in a fixed order (rows longer than 256 entries in segments whose partial sums are added in segment order), so the
 * result is bitwise reproducible.  The first call builds the row segments (one host synchronisation), the first
 * masked transpose the mirror permutation; both are kept with the graph. */
int daisy_lgcn_spmm_ex(const daisy_lgcn_graph *g, const float *X, int64_t ldx, float *Y, int64_t ldy, int32_t d,
                       int32_t accumulate, float node_p, uint64_t seed, int32_t transpose, daisy_stream_t stream);
/* out[e] = keep bit (1 / 0) of index e < n of dropout stream `stream_id` at probability p in [0, 1) (test hook) */
int daisy_dropout_mask(uint64_t seed, uint32_t stream_id, int64_t n, float p, uint8_t *out, daisy_stream_t stream);
/* bytes of the workspace of daisy_ngcf_layer_backward (dZ and the per-workgroup weight-gradient partials) */
size_t daisy_ngcf_ws_bytes(int64_t n, int32_t d_in, int32_t d_out);
/* forward of layer `layer` (0-based) over n rows: Y (pitch ldy) and norm[n] = |dropout(LeakyReLU(Z))| per row.
 * X: f32[n, d_in] contiguous (saved for the backward pass). */
int daisy_ngcf_layer_forward(const float *E, int64_t lde, const float *X, const float *W1, const float *b1,
                             const float *W2, const float *b2, float *Y, int64_t ldy, float *norm, int64_t n,
                             int32_t d_in, int32_t d_out, float mess_p, uint64_t seed, int32_t layer,
                             daisy_stream_t stream);
/* backward of the same layer, given dY = dL/dY (pitch ldd) and the forward's Y, norm, E, X:
 *   dZ           = LeakyReLU' * dropout' * normalize'(dY)
 *   [dS | dT]    = dZ [W1 | W2]
 *   dE[n, d_in]  = gprev + dS + dT * X        (gprev: pitch ldg, NULL for 0; dE contiguous)
 *   dX[n, d_in]  = dS + dT * E                (the caller adds A_hat_drop^T dX to dE: daisy_lgcn_spmm_ex)
 * and the per-workgroup partials of dW = dZ^T [S | T], db = sum dZ into ws (daisy_ngcf_ws_bytes). */
int daisy_ngcf_layer_backward(const float *dY, int64_t ldd, const float *Y, int64_t ldy, const float *norm,
                              const float *E, int64_t lde, const float *X, const float *W1, const float *W2,
                              const float *gprev, int64_t ldg, float *dE, float *dX, float *ws, int64_t n,
                              int32_t d_in, int32_t d_out, float mess_p, uint64_t seed, int32_t layer,
                              daisy_stream_t stream);
/* dW1, dW2 [d_out][d_in] and db1, db2 [d_out] += the partials of ws summed in a fixed order (no float atomics:
 * bitwise repeatable).  db1 and db2 receive the same sum (Z = ... + b1 + b2). */
int daisy_ngcf_wgrad_reduce(const float *ws, int64_t n, int32_t d_in, int32_t d_out, float *dW1, float *db1,
                            float *dW2, float *db2, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * Item2Vec (rest of SURVEY.md §8f rank 4; daisy/model/Item2VecRecommender.py:15-112).
 * Training IS the point-wise MF path on ONE shared table S (rows (target, context, label), loss CL, no
 * regulariser): daisy_bpr_forward(P = Q = S) -> daisy_bpr_user_grad (targets) + daisy_bpr_item_grad_data
 * (contexts) into two gradient buffers -> daisy_axpby_f32 -> daisy_adam_dense.  After training the user
 * table is user_embedding[u] = sum of S over the user's training items (:56-59): daisy_csr_row_sum on the
 * CSR of daisy_build_user_csr.  predict / rank / full_rank are the MF entry points.
 * ---------------------------------------------------------------------- */
/* y = a*x + b*y over n floats; zero_x != 0 also clears x (a consumed gradient buffer) */
int daisy_axpby_f32(float *x, float a, float b, float *y, int64_t n, int32_t zero_x, daisy_stream_t stream);
/* out[r] = sum_{e in [indptr[r], indptr[r+1])} X[cols[e]]  (rows with no entries are left untouched) */
int daisy_csr_row_sum(const int64_t *indptr, const int32_t *cols, const float *X, int64_t rows, int32_t d,
                      float *out, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * NFM (daisy/model/NFMRecommender.py:15-209).  Stage 0 is the bi-interaction x0 = P[u] * Q[i] followed by
 * FM_layers (BatchNorm1d when batch_norm, Dropout); stage l = 1..L is Linear(d, d), BatchNorm1d, activation,
 * Dropout (deep_layers); pred = (h_L + ub[u] + ib[i] + bias) . wp.  factors 1..DAISY_NFM_MAX_FACTORS,
 * num_layers 0..DAISY_NFM_MAX_LAYERS, fp32.  A pairwise training step forwards two calls of B rows each (positives,
 * then negatives): each call takes its own batch statistics and updates the running statistics once
 * (momentum 0.1, eps 1e-5, unbiased running variance), as the reference's two forward() calls do.
 * Dropout keep bits: drop_keep(seed, DAISY_NFM_DROP_STREAM + stage, row * d + column), rows of the negatives'
 * call numbered B..2B-1 (daisy_dropout_mask reproduces a stream).  Every reduction runs in a fixed order, no
 * float atomics: a step is bitwise repeatable.
 * ---------------------------------------------------------------------- */
#define DAISY_NFM_MAX_LAYERS 8
#define DAISY_NFM_MAX_FACTORS 256
#define DAISY_NFM_DROP_STREAM 0x300u
#define DAISY_NFM_SMALL_MAX_B 256
/* the two implementations of a training step (same arithmetic, same bits): the small step runs the whole step in ONE
 * workgroup (one launch; B <= DAISY_NFM_SMALL_MAX_B), the layered step one launch per phase over all workgroups */
enum { DAISY_NFM_PATH_AUTO = 0, DAISY_NFM_PATH_SMALL = 1, DAISY_NFM_PATH_LAYERED = 2 };
typedef enum { DAISY_NFM_ACT_NONE = 0, DAISY_NFM_ACT_RELU = 1, DAISY_NFM_ACT_SIGMOID = 2, DAISY_NFM_ACT_TANH = 3 } daisy_nfm_act;
typedef struct {
    float *P, *Q;                                  /* embed_user / embed_item weight [U][d], [I][d] */
    float *ub, *ib, *bias;                         /* u_bias [U], i_bias [I], bias_ [1] */
    float *bn_w[DAISY_NFM_MAX_LAYERS + 1];         /* BatchNorm weight / bias of stage s [d] (batch_norm only) */
    float *bn_b[DAISY_NFM_MAX_LAYERS + 1];
    float *W[DAISY_NFM_MAX_LAYERS];                /* Linear l+1 weight [d][d], bias [d] */
    float *b[DAISY_NFM_MAX_LAYERS];
    float *wp;                                     /* prediction.weight [d] */
} daisy_nfm_params;
typedef struct {                                   /* BatchNorm buffers of stage s (batch_norm only) */
    float *mean[DAISY_NFM_MAX_LAYERS + 1];         /* running_mean [d] */
    float *var[DAISY_NFM_MAX_LAYERS + 1];          /* running_var [d] */
    int64_t *nbt[DAISY_NFM_MAX_LAYERS + 1];        /* num_batches_tracked [1] */
} daisy_nfm_bn_state;
/* stats vector of a training step (device, double[DAISY_NFM_STATS_LEN]) */
enum {
    DAISY_NFM_ST_LOSS = 0,        /* the step's loss (criterion + regulariser) */
    DAISY_NFM_ST_LOSS_SUM = 1,    /* += loss every step (the epoch's loss) */
    DAISY_NFM_ST_LOSS_DATA = 2,   /* the criterion */
    DAISY_NFM_ST_NORM_U = 3,      /* Frobenius norms of the gathered user, positive item, negative item rows */
    DAISY_NFM_ST_NORM_I = 4,
    DAISY_NFM_ST_NORM_J = 5,
    DAISY_NFM_ST_NONFINITE = 6,   /* += 1 for every step whose loss is not finite */
    DAISY_NFM_STATS_LEN = 8
};
typedef struct daisy_nfm_ctx daisy_nfm_ctx;
/* max_rows: rows of one forward call (the batch size B; daisy_nfm_scores in training mode: the pairs scored).
 * act: daisy_nfm_act; batch_norm: 0 / 1; user_num, item_num < 2^31. */
int daisy_nfm_ctx_create(daisy_nfm_ctx **out, int64_t max_rows, int32_t factors, int32_t num_layers, int32_t act,
                         int32_t batch_norm, int64_t user_num, int64_t item_num);
int daisy_nfm_ctx_destroy(daisy_nfm_ctx *ctx);
size_t daisy_nfm_ctx_bytes(const daisy_nfm_ctx *ctx);
/* which path daisy_nfm_step_grads takes: DAISY_NFM_PATH_AUTO (default: the layered path, the faster of the two at every
 * measured batch), or forced (a forced small path refuses batches above DAISY_NFM_SMALL_MAX_B) */
int daisy_nfm_ctx_set_path(daisy_nfm_ctx *ctx, int32_t path);
/* NFM.calc_loss + backward (:125-151) for one batch (u, i, j)[B] (point-wise losses: j holds the labels): the
 * gradients accumulate (+=) into `grads` (same layout as params), the running statistics of `bn` are updated, the
 * loss goes to stats.  reg_1 / reg_2: L1 / Frobenius norms of the gathered embedding rows.  dropout_p in [0, 1).
 * B must be > 1 when batch_norm (torch's "Expected more than 1 value per channel when training"). */
int daisy_nfm_step_grads(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_params *grads,
                         const daisy_nfm_bn_state *bn, const int32_t *u, const int32_t *i, const int32_t *j, int64_t B,
                         int32_t loss_type, float gamma, float reg_1, float reg_2, float dropout_p, uint64_t seed,
                         double *stats, daisy_stream_t stream);
/* one epoch of AbstractRecommender.fit's loop over the batches of (u, i, j)[n]: step k (1-based, counted on from
 * step0) = daisy_nfm_step_grads with seed = seed_hi | (step0 + k), then the dense optimiser (0 SGD, 1 Adam,
 * 2 Adagrad, 3 RMSprop; torch defaults) over the flat parameter vector W / gradient g [n_flat] (g cleared).  Adam's
 * bias correction counts its own steps from opt_step0 (the steps the optimiser has taken: a fresh torch optimiser per
 * fit starts at 0). */
int daisy_nfm_fit_epoch(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_params *grads,
                        const daisy_nfm_bn_state *bn, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n,
                        int64_t batch, int32_t loss_type, float gamma, float reg_1, float reg_2, float dropout_p,
                        uint64_t seed_hi, int64_t step0, int64_t opt_step0, int32_t optimizer, float lr, float *W, float *g,
                        float *state0, float *state1, int64_t n_flat, double *stats, daisy_stream_t stream);
/* NFM.forward's score of n pairs into out[n]: C > 0: pair e = (users[e / C], items[e]) (rank); items == NULL:
 * (users[0], e) (full_rank); C == 0 with items: (users[e], items[e]).  train == 0: eval mode (running statistics,
 * no dropout, one fused kernel).  train != 0: training mode - batch statistics over all n pairs, one update of
 * the running statistics, dropout_p with `seed` (n <= max_rows). */
int daisy_nfm_scores(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_bn_state *bn, const int64_t *users,
                     const int64_t *items, int64_t n, int64_t C, int32_t train, float dropout_p, uint64_t seed, float *out,
                     daisy_stream_t stream);
/* "These users x all items" in eval mode only (additive to ABI 8): out f32[m][item_num], out[b][i] = the
 * score daisy_nfm_scores (train == 0) gives the pair (users[b], i), from the same fused kernel - a pair's score depends on
 * the pair alone, so the bits do not depend on m.  users i64[m], any order, duplicates allowed; pair e = (users[e /
 * item_num], e % item_num) is formed in the kernel: no candidate array of m * item_num ids exists.  Running statistics
 * are read, never written. */
int daisy_nfm_scores_users(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_bn_state *bn,
                           const int64_t *users, int64_t m, float *out, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * Multi-VAE (daisy/model/VAECFRecommender.py, VAECF).  Encoder [I] + hidden + [lat], decoder [lat/2] +
 * reversed(hidden) + [I], Linear layers with Tanh between them, fp32.  The parameters live in ONE flat buffer W in the
 * module's order (encoder.0.weight, encoder.0.bias, encoder.2.weight, ..., decoder.*): every tensor as torch lays it
 * out except encoder.0.weight, which is stored item-major ([I][hidden0], the transpose of torch's [hidden0][I]) so
 * that the sparse first layer reads whole rows.  The gradient buffer g has the same layout and must be zero on entry
 * (the dense optimisers leave it so).
 * The user histories are a CSR over users (row_ptr [user_num + 1], col int32, val float32; entries with value 0
 * dropped, items ascending within a row).  A batch of B users holds the concatenation of its rows' entries (n_entries
 * of them, the caller's count).  Noise: keep[n_entries] (one byte per batch entry, 0 = dropped) and eps[B][lat/2]
 * (the reparameterisation's normal draws) when given; otherwise keep = drop_keep(seed, DAISY_VAE_KEEP_STREAM, entry)
 * and eps = Box-Muller over the counter hash of (seed, DAISY_VAE_EPS_STREAM, b * (lat/2) + j).  Every reduction runs
 * in a fixed order, no float atomics: a step is bitwise repeatable.
 * ---------------------------------------------------------------------- */
#define DAISY_VAE_MAX_HIDDEN 8
#define DAISY_VAE_KEEP_STREAM 0x400u
#define DAISY_VAE_EPS_STREAM 0x401u
enum {
    DAISY_VAE_ST_LOSS = 0,        /* the step's loss (CE + anneal * KL) */
    DAISY_VAE_ST_LOSS_SUM = 1,    /* += loss every step (the epoch's loss) */
    DAISY_VAE_ST_CE = 2,          /* -(log_softmax(z) * R).sum(1).mean() */
    DAISY_VAE_ST_KL = 3,          /* -0.5 * mean(sum(1 + logvar - mu^2 - exp(logvar))) (before anneal) */
    DAISY_VAE_ST_NONFINITE = 4,   /* += 1 for every step whose loss is not finite */
    DAISY_VAE_ST_BAD_ROWS = 5,    /* += 1 per batch row whose user id is out of range or whose entries overflow n_entries */
    DAISY_VAE_STATS_LEN = 8
};
typedef struct daisy_vae_ctx daisy_vae_ctx;
/* max_batch: users per step or scoring call; max_entries: history entries of such a batch (at most); hidden[n_hidden]:
 * mlp_hidden_size (0 .. DAISY_VAE_MAX_HIDDEN layers, widths >= 1); latent_dim >= 2; item_num < 2^24. */
int daisy_vae_ctx_create(daisy_vae_ctx **out, int64_t max_batch, int64_t max_entries, int64_t item_num, int32_t n_hidden,
                         const int32_t *hidden, int32_t latent_dim);
int daisy_vae_ctx_destroy(daisy_vae_ctx *ctx);
size_t daisy_vae_ctx_bytes(const daisy_vae_ctx *ctx);
/* floats of the flat parameter buffer (0 for NULL) */
int64_t daisy_vae_param_count(const daisy_vae_ctx *ctx);
/* VAECF.calc_loss + backward for the users[B] (int64): gradients into g, loss into stats.  train != 0: dropout_p on
 * the input and z = mu + eps * exp(logvar / 2); train == 0: eval mode (no dropout, z = mu).  anneal: the KL weight of
 * this step (min(anneal_cap, update / total_anneal_steps), rounded to fp32). */
int daisy_vae_step_grads(daisy_vae_ctx *ctx, const float *W, float *g, const int64_t *row_ptr, const int32_t *col,
                         const float *val, int64_t user_num, const int64_t *users, int64_t B, int64_t n_entries,
                         const uint8_t *keep, const float *eps, int32_t train, float dropout_p, float anneal, uint64_t seed,
                         double *stats, daisy_stream_t stream);
/* one epoch of AbstractRecommender.fit's loop over users[n] in epoch order, batches of `batch`: step k (1-based,
 * counted on from step0) = daisy_vae_step_grads in training mode with the device noise of seed = seed_hi | (step0 + k)
 * and anneal = min(anneal_cap, (update0 + k) / total_anneal_steps) (anneal_cap when total_anneal_steps <= 0), then
 * the dense optimiser (0 SGD, 1 Adam, 2 Adagrad, 3 RMSprop; torch defaults) over W / g (g cleared).  entries[k - 1]
 * (host memory): n_entries of batch k.  Adam's bias correction counts from opt_step0. */
int daisy_vae_fit_epoch(daisy_vae_ctx *ctx, float *W, float *g, const int64_t *row_ptr, const int32_t *col, const float *val,
                        int64_t user_num, const int64_t *users, int64_t n, int64_t batch, const int64_t *entries,
                        float dropout_p, double anneal_cap, int64_t total_anneal_steps, int64_t update0, uint64_t seed_hi,
                        int64_t step0, int64_t opt_step0, int32_t optimizer, float lr, float *state0, float *state1,
                        double *stats, daisy_stream_t stream);
/* VAECF.forward's scores of the users[B]: items == NULL: out[B][item_num] (every item); otherwise out[B][C] for the
 * candidates items[B][C] (int64, ids checked by the caller), through the candidates' rows of the last layer only.
 * train / keep / eps / dropout_p / seed as in daisy_vae_step_grads. */
int daisy_vae_scores(daisy_vae_ctx *ctx, const float *W, const int64_t *row_ptr, const int32_t *col, const float *val,
                     int64_t user_num, const int64_t *users, int64_t B, int64_t n_entries, const int64_t *items, int64_t C,
                     const uint8_t *keep, const float *eps, int32_t train, float dropout_p, uint64_t seed, float *out,
                     daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * SLiM (daisy/model/SLiMRecommender.py, SLiM): one non-negative elastic net per item column over the Gram matrix,
 * truncated to the topk largest coefficients, scored by a sparse product (csrc/slim.hip).
 * X is the [user_num, item_num] rating matrix as a CSR (row_ptr int64 [user_num + 1], col int32 ascending within a
 * row, val float32, duplicate (user, item) pairs already summed).
 * ---------------------------------------------------------------------- */
#define DAISY_SLIM_LDS_ITEMS 9984   /* item_num up to which the descent state (w, H: 16 bytes per item) lives in LDS */
#define DAISY_SLIM_MAX_TOPK 1024
enum { DAISY_SLIM_PATH_AUTO = 0, DAISY_SLIM_PATH_LDS = 1, DAISY_SLIM_PATH_GLOBAL = 2 };
/* bytes of daisy_slim_gram's workspace: one [item_num, item_num] fp32 partial product and the [tile_rows, item_num]
 * fp32 tile the user blocks are densified into (tile_rows <= 0: the default, at most 1024 rows; otherwise rounded up to a
 * multiple of 16).  0 for item_num < 1. */
size_t daisy_slim_gram_workspace_bytes(int64_t user_num, int64_t item_num, int64_t tile_rows);
/* DAISY_ERR_ARG, with the three figures in the message, when G (item_num^2 * 4 bytes) plus that workspace does not fit
 * the offered_bytes the caller can give them; no HIP call. */
int daisy_slim_gram_fits(int64_t user_num, int64_t item_num, int64_t tile_rows, size_t offered_bytes);
/* G = X^T X, fp32 [item_num, item_num] (SLiMRecommender.py:84: ElasticNet(precompute=True) forms it in every fit):
 * blocks of users are densified into the tile, tile^T tile runs on the fp32 MFMA product and the blocks' products are
 * added in block order: no atomics, reproducible run to run, exact while every partial sum is an integer below 2^24.
 * The tile's rows follow from workspace_bytes (as daisy_slim_gram_workspace_bytes lays it out; at least 16 rows). */
int daisy_slim_gram(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                    float *G, void *workspace, size_t workspace_bytes, daisy_stream_t stream);
/* bytes of daisy_slim_cd's workspace (column counter, diagonal of G and, on the global path, w and H of every
 * workgroup) for ncols columns; path: DAISY_SLIM_PATH_* (AUTO: LDS up to DAISY_SLIM_LDS_ITEMS items).  0 on bad arguments. */
size_t daisy_slim_cd_workspace_bytes(int64_t item_num, int64_t ncols, int32_t path);
/* SLiMRecommender.py:73-107 for the columns [col0, col0 + ncols): per column j the cyclic coordinate descent of
 *   min 1/2 w'Qw - q'w + a |w|_1 + 1/2 b |w|^2 over w >= 0,  Q = G without row / column j, q = G[:, j] (q[j] = 0),
 *   a = alpha * l1_ratio * n_users, b = alpha * (1 - l1_ratio) * n_users
 * (sklearn's enet_coordinate_descent_gram with positive=True, selection='cyclic'): w, H = Qw and the duality gap in
 * fp64, G widened on load and never written; stops when gap < tol * G[j, j], after max_iter sweeps at the latest.  Then
 * the truncation of :86-107: the min(nz - 1, topk) largest coefficients (ties: lower row), rounded to fp32.
 * Outputs: kept_count int32 [ncols]; kept_row int32 / kept_val float32 [ncols, topk], descending value then ascending
 * row, unused slots (-1, 0); sweeps int32 [ncols] (0 for a column with G[j, j] == 0); gap float64 [ncols]; moves int64
 * [ncols] or NULL: the coordinate updates that changed a value, each of which read one row of G (a measurement hook).
 * One workgroup per column, fed from an atomic column counter; the result does not depend on which workgroup ran a
 * column.  alpha > 0, 0 <= l1_ratio <= 1, tol >= 0, max_iter >= 1, 1 <= topk <= DAISY_SLIM_MAX_TOPK. */
int daisy_slim_cd(const float *G, int64_t item_num, int64_t n_users, double alpha, double l1_ratio, double tol,
                  int32_t max_iter, int32_t topk, int64_t col0, int64_t ncols, int32_t *kept_count, int32_t *kept_row,
                  float *kept_val, int32_t *sweeps, double *gap, int64_t *moves, int32_t path, void *workspace,
                  size_t workspace_bytes, daisy_stream_t stream);
/* rows of A_tilde = X W (SLiMRecommender.py:123-127, 135, 144) for the users[B] (int64): out[B][C] at the candidates
 * items[B][C] (int64), or out[B][item_num] when items == NULL.  W is the truncated matrix by column (w_ptr int64
 * [item_num + 1], w_row int32 ascending within a column, w_val float32).  A score is the fp64 sum over its column's
 * entries in ascending row of X[u, row] * val, rounded once to fp32.  One workgroup per user: the user's row of X is
 * scattered into LDS (path LDS; AUTO up to 32768 items) or looked up by binary search in the CSR row (path GLOBAL).
 * A user or item id out of range scores 0. */
int daisy_slim_scores(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                      const int64_t *w_ptr, const int32_t *w_row, const float *w_val, const int64_t *users, int64_t B,
                      const int64_t *items, int64_t C, float *out, int32_t path, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * PureSVD (daisy/model/PureSVDRecommender.py, PureSVD): scikit-learn's randomized_svd of the rating matrix, restated
 * as sparse x tall-skinny products, Cholesky-QR2 orthonormalisation and one small one-sided Jacobi SVD, all in fp64
 * (csrc/puresvd.hip).  Dense matrices are fp64, row-major, on the device; c (columns of a tall-skinny
 * matrix, sides of the small square ones) is at most DAISY_PSVD_MAX_C.  Every result is reproducible run to run: no
 * floating-point atomics, every sum in a fixed order.
 * ---------------------------------------------------------------------- */
#define DAISY_PSVD_MAX_C 256
enum { DAISY_PSVD_CONVERGED = 0, DAISY_PSVD_NOT_CONVERGED = 1 };
/* Y[n_rows, c] = A X, A the CSR of daisy_slim_gram's layout ([n_rows, n_cols], val widened to fp64 on load), X fp64
 * [n_cols, c]: one workgroup per row, a row's non-zeros accumulated in stored order; an empty row writes zeros. */
int daisy_psvd_spmm(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t n_rows, int64_t n_cols,
                    const double *X, int32_t c, double *Y, daisy_stream_t stream);
/* rows per block of daisy_psvd_gram for block_rows <= 0 (the default: 256, or more so that there are at most 256
 * blocks), else block_rows rounded up to a multiple of 4; and the bytes of its workspace (one [c, c] partial product
 * per block).  0 on bad arguments. */
int64_t daisy_psvd_gram_block_rows(int64_t n, int64_t block_rows);
size_t daisy_psvd_gram_workspace_bytes(int64_t n, int32_t c, int64_t block_rows);
/* G[c, c] = Y^T Y of Y [n, c] on the fp64 MFMA (v_mfma_f64_16x16x4_f64): every block of rows writes its partial
 * product, a second pass adds the partial products in block order.  G is bitwise symmetric. */
int daisy_psvd_gram(const double *Y, int64_t n, int32_t c, double *G, int64_t block_rows, void *workspace,
                    size_t workspace_bytes, daisy_stream_t stream);
/* The upper-triangular R [c, c] with R^T R = G (one workgroup), for G = Y^T Y of a Y with n rows.  Column j is DROPPED
 * when its pivot d_j = G_jj - sum_{i<j} R_ij^2 is not > 64 n eps G_jj (eps = 2^-52): R_jj = 0 and the rest of row j is
 * zero; the entries above the diagonal in column j are kept.  Rinv [c, c] gets the inverse of R restricted to the kept
 * columns (zero rows and columns for the dropped ones), *dropped (a device int32) the number of dropped columns. */
int daisy_psvd_chol(const double *G, int32_t c, int64_t n, double *R, double *Rinv, int32_t *dropped,
                    daisy_stream_t stream);
/* C[n, c2] = Y[n, c] T[c, c2] on the fp64 MFMA; k ascending in every element's sum. */
int daisy_psvd_gemm(const double *Y, const double *T, double *C, int64_t n, int32_t c, int32_t c2,
                    daisy_stream_t stream);
/* One-sided (Hestenes) Jacobi SVD of A [c, c] = U diag(s) V^T in one workgroup: round-robin pairs of ROWS are rotated
 * until a whole sweep rotates nothing (|a_p . a_q| <= sqrt(c) eps |a_p| |a_q| for every pair) or max_sweeps sweeps are
 * done.  U [c, c] (orthogonal: the product of the rotations), s [c] sorted non-increasing (ties in row order),
 * V [c, c] (column i the right vector of s[i]; a zero column where s[i] == 0).  info int32 [2] on the device:
 * {DAISY_PSVD_CONVERGED or DAISY_PSVD_NOT_CONVERGED, sweeps done}.  workspace: daisy_psvd_jacobi_workspace_bytes(c). */
size_t daisy_psvd_jacobi_workspace_bytes(int32_t c);
int daisy_psvd_jacobi(const double *A, int32_t c, int32_t max_sweeps, double *U, double *s, double *V, int32_t *info,
                      void *workspace, size_t workspace_bytes, daisy_stream_t stream);
/* scores[B, C] (fp64) = user_vec[users[b]] . item_vec[items[b][c]] (items == NULL: every item, C = item_num), the sum
 * over the k factors in ascending order; then, unless out_ids == NULL (scores only), out_ids [B, min(topk, C)] = the
 * candidates' ids (positions when items == NULL) of the largest scores, compared as fp64, ties to the lower position.
 * One workgroup per user row.  An id out of range scores 0; a row with fewer than topk comparable scores (NaN) is
 * filled with -1. */
int daisy_psvd_rank(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                    const int64_t *users, int64_t B, const int64_t *items, int64_t C, int32_t topk, double *scores,
                    int64_t *out_ids, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * EASE (daisy/model/EASERecommender.py, EASE): B = -P / diag(P) with a zero diagonal, P = (X^T X + reg I)^-1, by a
 * blocked fp64 Cholesky factorisation, the blocked inverse of the factor and one product, all on the fp64 MFMA
 * (csrc/ease.hip).  Matrices are fp64, row-major [n, n], on the device; every element index is 64-bit.
 * Every result is reproducible run to run: no atomics, every element's sum over k ascending in a fixed workgroup.
 * The stages share one small workspace of daisy_ease_workspace_bytes(n) bytes: potrf writes the inverses of the diagonal
 * blocks into it, potri reads them, weights keeps diag(P) in it.
 * ---------------------------------------------------------------------- */
#define DAISY_EASE_BLOCK 64
/* bytes of the shared workspace (ceil(n / 64) blocks of 64 x 64 doubles, plus n doubles); 0 on bad arguments */
size_t daisy_ease_workspace_bytes(int64_t item_num);
/* bytes a fit holds at its peak (during potri): TWO fp64 [item_num, item_num] buffers - one that holds the system, then
 * L, then P, then B in place, and one for L^-1 - plus the workspace.  (Before that, the fp32 Gram matrix of
 * daisy_slim_gram and the system: 1.5 such buffers.)  0 on bad arguments. */
size_t daisy_ease_fit_bytes(int64_t item_num);
/* DAISY_OK when daisy_ease_fit_bytes(item_num) <= offered_bytes, else DAISY_ERR_ARG with the sizes in
 * daisy_last_error(); makes no HIP call: callers refuse a fit before anything is allocated. */
int daisy_ease_fits(int64_t item_num, size_t offered_bytes);
/* EASERecommender.py:37-39: A = (double) G + reg I, G the fp32 [item_num, item_num] output of daisy_slim_gram. */
int daisy_ease_system(const float *G, int64_t item_num, double reg, double *A, daisy_stream_t stream);
/* First half of EASERecommender.py:41 (np.linalg.inv): the lower Cholesky factor A = L L^T in place, right-looking
 * with blocks of DAISY_EASE_BLOCK: (a) one workgroup factors the diagonal block in LDS and writes its triangular inverse
 * to the workspace, (b) the panel below it is solved against the block (products between 16-column groups on the fp64
 * MFMA, the 16 x 16 diagonal tiles by substitution: exact when the factor is an integer matrix), (c) the trailing
 * matrix loses L21 L21^T on the fp64 MFMA, lower tiles only.  Only A's lower triangle is read; the strict upper
 * triangle is left as it was.  *info (a device int32): 0, or 1 + the first column whose pivot is not > 0 or not a
 * number (what follows that column in L is then meaningless). */
int daisy_ease_potrf(double *A, int64_t n, int32_t *info, void *workspace, size_t workspace_bytes, daisy_stream_t stream);
/* Second half of EASERecommender.py:41: from L (daisy_ease_potrf, with the workspace it filled) T = L^-1 block row by
 * block row (T[i, j] = -Dinv_i sum_k L[i, k] T[k, j] on the fp64 MFMA; T is scratch [n, n], its blocks above the
 * diagonal are not written), then P = T^T T: the tiles on and above the diagonal are computed and mirrored, so P is
 * bitwise symmetric.  P may be L's buffer; T must be one of its own. */
int daisy_ease_potri(const double *L, int64_t n, double *T, double *P, const void *workspace, size_t workspace_bytes,
                     daisy_stream_t stream);
/* EASERecommender.py:42-43: B[i, j] = -P[i, j] / P[j, j], B[j, j] = 0.  B may be P's buffer. */
int daisy_ease_weights(const double *P, int64_t n, double *B, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream);
/* EASERecommender.py:49-71 (predict, rank, full_rank), arguments as daisy_psvd_rank: scores[B, C] (fp64) =
 * sum over the CSR entries (r, v) of row users[b] of X, in stored (ascending item) order, of (double) v * W[r, item], at
 * the candidates items[B][C] (items == NULL: every item, C = item_num); then, unless out_ids == NULL (scores only),
 * out_ids [B, min(topk, C)] = the candidates' ids (positions when items == NULL) of the largest scores, compared as
 * fp64, ties to the lower position.  One workgroup per user row.  A user or item id out of range scores 0; a row with
 * fewer than topk comparable scores (NaN) is filled with -1.  X: the CSR of daisy_slim_gram's layout; W fp64
 * [item_num, item_num]. */
int daisy_ease_rank(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W, int64_t user_num,
                    int64_t item_num, const int64_t *users, int64_t B, const int64_t *items, int64_t C, int32_t topk,
                    double *scores, int64_t *out_ids, daisy_stream_t stream);

/* -------------------------------------------------------------------------
 * ItemKNN / UserKNN (daisy/model/KNNCFRecommender.py, Similarity / ItemKNNCF / UserKNNCF): the similarity of the columns
 * of a data matrix D [n_rows, n] (X for ItemKNN, X^T for UserKNN) from G = D^T D (daisy_slim_gram), the K largest
 * weights of every column, and the fp64 scores (csrc/knn.hip).  D is a CSR of daisy_slim_gram's layout.
 * Reproducible run to run: no floating-point atomics, every floating-point sum in a fixed order.
 * ---------------------------------------------------------------------- */
#define DAISY_KNN_MAX_K 1024
/* what daisy_knn_center does to the stored values of D */
enum { DAISY_KNN_CENTER_NONE = 0, DAISY_KNN_CENTER_ROW = 1, DAISY_KNN_CENTER_COL = 2, DAISY_KNN_CENTER_BINARY = 3 };
/* the weight of daisy_knn_select (KNNCFRecommender.py:313-337); PLAIN: w / shrink when shrink != 0, else w */
enum { DAISY_KNN_COSINE = 0, DAISY_KNN_ASYMMETRIC = 1, DAISY_KNN_TANIMOTO = 2, DAISY_KNN_DICE = 3, DAISY_KNN_TVERSKY = 4,
       DAISY_KNN_PLAIN = 5 };
/* KNNCFRecommender.py:172-178: mean[r] = the fp32 sum of row r's stored values (a wave per row: lane l adds the entries
 * l, l + 64, ... in stored order, the lanes meet in a fixed tree) divided by their count; 0 for an empty row. */
int daisy_knn_row_means(const int64_t *row_ptr, const float *val, int64_t n_rows, float *mean, daisy_stream_t stream);
/* KNNCFRecommender.py:165-233: out[e] = val[e] - mean[row of e] (CENTER_ROW, mean [n_rows]: 'adjusted'), val[e] -
 * mean[col[e]] (CENTER_COL, mean [n_cols]: 'pearson'; the column means are the row means of the other orientation's CSR),
 * 1 (CENTER_BINARY: jaccard, tanimoto, dice, tversky) or val[e] (CENTER_NONE).  A value that becomes exactly 0 stays
 * stored.  out may be val. */
int daisy_knn_center(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t n_rows, int64_t n_cols,
                     int32_t mode, const float *mean, float *out, daisy_stream_t stream);
/* KNNCFRecommender.py:257-261: ss[i] = G[i, i], its correctly rounded square root when take_sqrt != 0. */
int daisy_knn_diag(const float *G, int64_t n, int32_t take_sqrt, float *ss, daisy_stream_t stream);
/* KNNCFRecommender.py:302-356 for every column j of the symmetric G fp32 [n, n]: w[i] = G[j, i], w[j] = 0, then in fp32,
 * every operation rounded on its own (no fused multiply-add):
 *   COSINE      w * (1 / (ss[j] * ss[i] + shrink + 1e-6))
 *   ASYMMETRIC  w * (1 / (ss[j]^(2 alpha) * ss[i]^(2 (1 - alpha)) + shrink + 1e-6)); alpha == 0.5 takes COSINE's path
 *   TANIMOTO    w * (1 / (ss[j] + ss[i] - w + shrink + 1e-6))
 *   DICE        w * (1 / (ss[j] + ss[i] + shrink + 1e-6))
 *   TVERSKY     w * (1 / (w + (ss[j] - w) + (ss[i] - w) + shrink + 1e-6))
 *   PLAIN       w / shrink when shrink != 0, else w
 * Of the min(K, n) largest weights of the column, as signed values with -0.0 == +0.0, the non-zero ones are kept: ties at
 * the boundary go to the LOWER row (the reference leaves them to argpartition).  Outputs in daisy_slim_cd's fixed-pitch
 * form: count int32 [n]; rows int32 / vals float32 [n, K], ascending row within a column, unused slots (-1, 0).
 * One workgroup per column at a time: the K-th largest weight by a radix select over an order-preserving 32-bit key
 * (four histogram passes of 8 bits, integer atomics in LDS), one ordered pass that assigns the slots by a workgroup
 * prefix scan; the weights are recomputed on every pass, so n is not bounded by the LDS.  1 <= K <= DAISY_KNN_MAX_K (K >=
 * n is allowed), shrink finite and >= 0, 0 <= alpha <= 1. */
int daisy_knn_select(const float *G, const float *ss, int64_t n, int32_t mode, float shrink, float alpha, int32_t K,
                     int32_t *count, int32_t *rows, float *vals, daisy_stream_t stream);
/* KNNCFRecommender.py:432 / :510 and predict, rank, full_rank: scores[B, C] (fp64) = sum over k ascending of
 * L[users[b], k] * R[k, item], L a CSR [n_rows, inner] with fp32 values, R [inner, n_cols] by column (r_ptr int64
 * [n_cols + 1], r_row int32 ascending within a column, r_val fp32), at the candidates items[B][C] (items == NULL: every
 * column, C = n_cols); then, unless out_ids == NULL, out_ids [B, topk] = the candidates' ids (positions when items ==
 * NULL) of the largest scores, compared as fp64, ties to the lower position.  ItemKNN: L = X, R = W by column; UserKNN:
 * L = W by row, R = X by column.  One workgroup per row: L's row is scattered into LDS (path LDS; AUTO up to inner =
 * 32768) or looked up by binary search (path GLOBAL; DAISY_SLIM_PATH_*).  An id out of range scores 0. */
int daisy_knn_rank(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                   const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols, const int64_t *users,
                   int64_t B, const int64_t *items, int64_t C, int32_t topk, double *scores, int64_t *out_ids, int32_t path,
                   daisy_stream_t stream);
/* bytes a fit of D [n_rows, n] holds at its peak: G (n^2 fp32), the workspace of daisy_slim_gram, and the outputs of
 * daisy_knn_select with the norms.  The dense G bounds n (UserKNN: n = user_num).  0 on bad arguments. */
size_t daisy_knn_fit_bytes(int64_t n_rows, int64_t n, int32_t K);
/* DAISY_OK when daisy_knn_fit_bytes <= offered_bytes, else DAISY_ERR_ARG with the sizes in daisy_last_error(); makes no
 * HIP call: callers refuse a fit before anything is allocated. */
int daisy_knn_fits(int64_t n_rows, int64_t n, int32_t K, size_t offered_bytes);

/* ------------------------------------------------------------------------
 * Full ranking of many users on fp64 scores: EASE, SLiM, ItemKNN / UserKNN, PureSVD (csrc/rank_full_f64.hip,
 * csrc/rank_f64_users.h, csrc/score_f64.h; additive to ABI 8)
 * ---------------------------------------------------------------------- */
/* For every users[b] (int64 [n], any order, duplicates allowed) the topk items of ALL item_num (n_cols), best first, without
 * the items of the user's exclusion row, in one launch of one workgroup per user.  The score of (user, item) is the
 * model's own: the expression of daisy_ease_rank, daisy_slim_scores, daisy_knn_rank and daisy_psvd_rank, from the same
 * device function, so the bits agree; the model arguments are those entries' without items / C / scores.  Order: score
 * descending compared as fp64 (SLiM: after its rounding to fp32), -0.0 equal to +0.0, equal scores by ascending item id,
 * a score that is not a number is never selected.  The exclusion is daisy_full_rank_users': excl_indptr int64
 * [user_num + 1] (n_rows for knn), excl_items int32 ascending inside a row, duplicates allowed, both NULL or both given;
 * row contents are only compared, never used as an index: an entry >= item_num or an unsorted row may cost missed
 * exclusions, never an out-of-bounds access; user ids and excl_indptr are the caller's to validate (a user id out of range
 * scores 0 everywhere and excludes nothing).  out_ids int64 [n, topk]; out_scores [n, topk] (fp64; fp32 for SLiM) or
 * NULL; positions beyond a user's eligible, comparable items hold id -1 and score -inf.  1 <= topk <= 128 (topk above
 * item_num is allowed): a larger topk is DAISY_ERR_ARG with the cap in the message.  Every argument is checked before the
 * first HIP call; n == 0 returns DAISY_OK without a launch.  No workspace: daisy_rank_f64_users_workspace_bytes is 0 for
 * every shape - the candidates of a user live in LDS and nothing of size n * item_num is written or allocated. */
size_t daisy_rank_f64_users_workspace_bytes(int64_t n, int64_t item_num, int32_t topk);
int daisy_ease_full_rank_users(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W, int64_t user_num,
                               int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                               const int32_t *excl_items, int32_t topk, int64_t *out_ids, double *out_scores,
                               daisy_stream_t stream);
int daisy_slim_full_rank_users(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                               const int64_t *w_ptr, const int32_t *w_row, const float *w_val, const int64_t *users, int64_t n,
                               const int64_t *excl_indptr, const int32_t *excl_items, int32_t topk, int64_t *out_ids,
                               float *out_scores, int32_t path, daisy_stream_t stream);
int daisy_knn_full_rank_users(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                              const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                              const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                              int32_t topk, int64_t *out_ids, double *out_scores, int32_t path, daisy_stream_t stream);
int daisy_psvd_full_rank_users(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                               const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                               int32_t topk, int64_t *out_ids, double *out_scores, daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Exact ranks of held-out items over all items on fp64 scores: EASE, SLiM, ItemKNN / UserKNN, PureSVD
 * (csrc/rank_positions_f64.hip, csrc/rank_f64_positions.h, csrc/rank_count.h; additive to ABI 8)
 * ---------------------------------------------------------------------- */
/* The model arguments, users [n], the exclusion CSR and SLiM's / KNN's path are the *_full_rank_users sibling's; the scores
 * come from the same scorer and device function, so they are that entry's bits.  tgt_indptr int64 [user_num + 1] /
 * tgt_items int32: the TARGET CSR over all users (daisy_build_user_csr's).  out_indptr int64 [n + 1]: the prefix sum of the
 * target-row lengths of users[0 .. n), built by the caller; n_targets = out_indptr[n].  Order: the key of score + 0.0
 * descending (SLiM: after its rounding to fp32), equal keys by ascending item id, a NaN is never ranked.  With E_u the
 * items of [0, item_num) outside u's exclusion row whose score is a number, request b's target number r (row order) gets
 *   out_pos[out_indptr[b] + r]   int32: #{ j in E_u : j comes before t } - its 0-based rank; -1 for a target outside
 *                                [0, item_num) (it is range-checked before it indexes anything), inside the exclusion row
 *                                or with a NaN score
 *   out_scores[...]              fp64 (fp32 for SLiM) or NULL: the target's score; -inf for the first two cases of pos = -1,
 *                                the computed NaN for the third
 *   out_eligible[b]              int32 or NULL: |E_u|
 * so that with the same arguments the sibling's ids[b][pos] == t for every target with 0 <= pos < topk, and no other
 * target appears in row b.  One launch of one 256-thread workgroup per request, which takes the target row in blocks of
 * 512 (sorted in LDS; every item looks up its bucket by binary search) and scores the items once per block: no cap on the
 * row length, no workspace, nothing of size n * item_num.  A request without targets streams only when out_eligible is
 * given.  The counts are integer LDS atomics: two runs give the same bits.  Row contents of the exclusion are only
 * compared, writes to out_pos / out_scores are bounded by n_targets; user ids, the indptr arrays and out_indptr are the
 * caller's to validate.  Every argument is checked before the first HIP call; n == 0 returns DAISY_OK without a launch. */
int daisy_ease_full_rank_positions(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W,
                                   int64_t user_num, int64_t item_num, const int64_t *users, int64_t n,
                                   const int64_t *excl_indptr, const int32_t *excl_items, const int64_t *tgt_indptr,
                                   const int32_t *tgt_items, const int64_t *out_indptr, int64_t n_targets, int32_t *out_pos,
                                   double *out_scores, int32_t *out_eligible, daisy_stream_t stream);
int daisy_slim_full_rank_positions(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num,
                                   int64_t item_num, const int64_t *w_ptr, const int32_t *w_row, const float *w_val,
                                   const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                   const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                   int64_t n_targets, int32_t *out_pos, float *out_scores, int32_t *out_eligible, int32_t path,
                                   daisy_stream_t stream);
int daisy_knn_full_rank_positions(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                                  const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                                  const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                  const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                  int64_t n_targets, int32_t *out_pos, double *out_scores, int32_t *out_eligible, int32_t path,
                                  daisy_stream_t stream);
int daisy_psvd_full_rank_positions(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                                   const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                   const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                   int64_t n_targets, int32_t *out_pos, double *out_scores, int32_t *out_eligible,
                                   daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Masked top-k over rows of fp32 scores (csrc/rank_rows.hip; additive to ABI 8): the selector of
 * full_rank_users for NeuMF, NFM and Multi-VAE, whose scores come out of kernels of their own
 * ---------------------------------------------------------------------- */
/* For every row r < m of scores (row r = scores[r * pitch .. + item_num), pitch >= item_num) the topk items, best first:
 * score descending, a NaN first, -0.0 equal to +0.0, equal scores by ascending item id - daisy_full_rank_users' order.
 * One launch of one 256-thread workgroup per row; float4 loads when scores is 16-byte aligned and pitch % 4 == 0, element
 * loads otherwise (chosen once per launch; the result is the same).  excl_indptr int64 [user_num + 1] / excl_items int32
 * (ascending inside a row, duplicates allowed: what daisy_build_user_csr returns; both or none) drop the items of CSR row
 * row_users[r] from row r; row_users int64 [m] (any order, duplicates allowed) may be NULL only without an exclusion.  Row
 * contents are only compared, never used as an index: an unsorted row or an entry >= item_num may cost missed exclusions,
 * never an out-of-bounds access; row_users and excl_indptr are the caller's to validate.  out_ids int64 [m, topk];
 * out_scores fp32 [m, topk] or NULL holds the row's own stored value at the selected id (re-read, not decoded: a NaN keeps
 * its payload, a zero its sign); positions beyond a row's eligible items hold id -1 and score -inf.  1 <= topk <=
 * min(item_num, 128): a larger topk is DAISY_ERR_ARG with the cap in the message.  Every argument is checked before the
 * first HIP call; m == 0 returns DAISY_OK without a launch.  No workspace, no global or floating-point atomics: the
 * candidates of a row live in LDS, their order is total, and two runs give the same bits. */
int daisy_rank_rows_f32(const float *scores, int64_t m, int64_t item_num, int64_t pitch, const int64_t *row_users,
                        const int64_t *excl_indptr, const int32_t *excl_items, int32_t topk, int64_t *out_ids,
                        float *out_scores, daisy_stream_t stream);
/* Exact ranks of held-out items over rows of fp32 scores (csrc/rank_rows_positions.hip; additive to ABI 8).
 * scores, m, item_num, pitch and the exclusion CSR are daisy_rank_rows_f32's; row_users int64 [m] is required: row_users[r]
 * names the CSR row of both the exclusion and the targets of score row r.  tgt_indptr / tgt_items, out_indptr int64
 * [m + 1] (the prefix sum of the rows' target-row lengths) and n_targets are as in daisy_ease_full_rank_positions.  With
 * word(j) = (key of scores[r][j] << 32) | (0xFFFFFFFF - j) - score descending, a NaN first, -0.0 equal to +0.0, equal
 * scores by ascending id - target t of row r gets
 *   out_pos      int32: #{ j < item_num not excluded : word(j) > word(t) }; -1 for a target outside [0, item_num) (range-
 *                checked before it indexes anything) or excluded
 *   out_scores   fp32 or NULL: the row's own stored value with its bits; -inf where pos = -1
 *   out_eligible int32 [m] or NULL: item_num - (distinct excluded ids in [0, item_num))
 * so that with the same arguments daisy_rank_rows_f32's ids[r][pos] == t wherever pos < topk.  One launch of one
 * 256-thread workgroup per row; float4 loads when scores is 16-byte aligned and pitch % 4 == 0, element loads otherwise; no
 * load reaches past item_num values of a row.  Target rows longer than 512 re-read the score row once per block of 512.
 * No workspace, integer LDS atomics only: two runs give the same bits.  Writes are bounded by n_targets.  Every argument
 * is checked before the first HIP call; m == 0 returns DAISY_OK without a launch. */
int daisy_rank_rows_positions_f32(const float *scores, int64_t m, int64_t item_num, int64_t pitch, const int64_t *row_users,
                                  const int64_t *excl_indptr, const int32_t *excl_items, const int64_t *tgt_indptr,
                                  const int32_t *tgt_items, const int64_t *out_indptr, int64_t n_targets, int32_t *out_pos,
                                  float *out_scores, int32_t *out_eligible, daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * MostPop(daisy/model/PopRecommender.py) and the ranking KPIs (daisy/utils/metrics.py): csrc/pop.hip, csrc/metrics.hip;
 * DESIGN.md §20.
 * ---------------------------------------------------------------------- */
/* PopRecommender.py:30-33 (fit): cnt int64 [item_num] = the occurrences of every id in items [nnz] (int32, or int64 when
 * items_is_i64 != 0; an id outside [0, item_num) is skipped), by integer atomics; score fp64 [item_num] = cnt / (1 + cnt),
 * the reference's one division on float64 counts, hence its bits. */
int daisy_pop_fit(const void *items, int32_t items_is_i64, int64_t nnz, int64_t item_num, int64_t *cnt, double *score,
                  daisy_stream_t stream);
/* PopRecommender.py:35-54 (predict, rank, full_rank): gathered [B, C] (fp64) = score[items[b][c]] (0 for an id out of
 * range), out_ids [B, topk] = the candidates' ids of the largest scores, compared as fp64, ties to the lower candidate
 * position (the reference's argsort leaves them open).  items == NULL: the full rank - one row (B <= 1), C = item_num,
 * gathered unused (may be NULL), out_ids = positions.  1 <= topk <= C. */
int daisy_pop_rank(const double *score, int64_t item_num, const int64_t *items, int64_t B, int64_t C, int32_t topk,
                   double *gathered, int64_t *out_ids, daisy_stream_t stream);

/* The KPIs of daisy_ranking_kpis: bit (1 << id) of its `metrics` mask.  The first DAISY_KPI_PER_USER have a value per
 * list; the requested ones take the slots 0, 1, ... of the outputs in this order.  Coverage has only its counts. */
enum {
    DAISY_KPI_PRECISION = 0,  /* metrics.py:148-158 */
    DAISY_KPI_RECALL = 1,     /* metrics.py:160-170 */
    DAISY_KPI_HIT = 2,        /* metrics.py:229-239 */
    DAISY_KPI_MRR = 3,        /* metrics.py:172-186 */
    DAISY_KPI_MAP = 4,        /* metrics.py:188-202 */
    DAISY_KPI_NDCG = 5,       /* metrics.py:204-227 */
    DAISY_KPI_F1 = 6,         /* metrics.py:263-278 */
    DAISY_KPI_AUC = 7,        /* metrics.py:241-261 */
    DAISY_KPI_POPULARITY = 8, /* metrics.py:104-122 */
    DAISY_KPI_DIVERSITY = 9,  /* metrics.py:124-146 */
    DAISY_KPI_PER_USER = 10,
    DAISY_KPI_COVERAGE = 10,  /* metrics.py:98-102 */
    DAISY_KPI_COUNT = 11
};
#define DAISY_METRICS_MAX_K 256
#define DAISY_METRICS_MAX_CUTOFFS 12
#define DAISY_METRICS_MAX_CATS 256
#define DAISY_METRICS_MAX_CAT_WORDS 4
/* bytes of daisy_ranking_kpis' workspace (the workgroups' partial sums; the coverage bitmaps); 0 on bad arguments */
size_t daisy_ranking_kpis_workspace_bytes(int64_t n, int32_t nc, int64_t item_num, uint32_t metrics);
/* calc_ranking_results / Metric.run (metrics.py:18-96) for ALL cutoffs and ALL requested KPIs in one pass over pred.
 *   pred [n, K] item ids, row-major, best first (int32, or int64 when pred_is_i64 != 0); an id outside [0, item_num) is
 *   never a hit.  indptr / gt_items: the truths as daisy_build_user_csr's CSR over user_num users.  users int64 [n]: the
 *   owner of every list (test_u; any order, repeats allowed; a user outside [0, user_num) has no truths).
 *   cutoffs_host int32 [nc]: HOST memory (they travel as kernel arguments), >= 1, strictly ascending, <= K <=
 *   DAISY_METRICS_MAX_K, nc <= DAISY_METRICS_MAX_CUTOFFS.  disc fp64 [K] = 1 / log2(p + 2), built on the host (needed for
 *   ndcg).  item_pop fp64 [item_num] (needed for popularity).  cat_bits uint64 [item_num, cat_words]: bit c of an item's
 *   row = it has category c, n_cats <= DAISY_METRICS_MAX_CATS, cat_words = ceil(n_cats / 64); sqrt_tab fp64 [n_cats + 1] =
 *   sqrt(0 .. n_cats) (both needed for diversity).
 * With r the hit mask of the first k positions (binary search in the user's row; duplicates count per position, as
 * np.in1d counts them), hits = popcount(r), gt = the row's length:
 *   precision hits / k; recall hits / gt; hit 1 or 0; mrr 1 / (first hit + 1) or 0; map the mean over the hit positions p
 *   of popcount(r[:p + 1]) / (p + 1) or 0; ndcg sum_{p hit} disc[p] / sum_{p < hits} disc[p] or 0; f1 2 pre rec / (pre +
 *   rec); auc (the pairs hit-before-miss) / (hits (k - hits)) - 0 / 0 is NaN for f1 and auc, as in the reference;
 *   popularity sum of item_pop over the DISTINCT hit items / gt or 0; diversity the mean over the pairs i < j < k of
 *   sqrt_tab[popcount(cat[pred_i] xor cat[pred_j])], NaN for k = 1.
 * Outputs: per_user fp64 [slots, nc, n] (may be NULL), means fp64 [slots, nc] (the sum of a workgroup's 256 lists, then
 * of the workgroups, both in a fixed order, divided by n: a NaN value makes its mean NaN), cover_counts int64 [nc] = the
 * distinct in-range ids of pred[:, :k] (integer atomic OR on a bitmap per cutoff, then popcounts).  No floating-point
 * atomics: two calls give the same bits.  One wave per list; lists longer than 64 run in chunks of 64. */
int daisy_ranking_kpis(const void *pred, int32_t pred_is_i64, int64_t n, int32_t K, const int64_t *indptr,
                       const int32_t *gt_items, int64_t user_num, const int64_t *users, const int32_t *cutoffs_host,
                       int32_t nc, const double *disc, const double *item_pop, int64_t item_num, const uint64_t *cat_bits,
                       int32_t cat_words, int32_t n_cats, const double *sqrt_tab, uint32_t metrics, double *per_user,
                       double *means, int64_t *cover_counts, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream);

/* The per-list KPIs of daisy_ranking_kpis from rank positions (csrc/metrics_positions.hip): the
 * reference's list definitions applied to the implied list of length K, at ANY K >= 1.  out_indptr int64 [n + 1] /
 * positions int32: daisy_full_rank_positions' outputs (-1: not ranked); gt_len int64 [n] or NULL: the truths of a request
 * (NULL: its row length); eligible int32 [n].  cutoffs_host as in daisy_ranking_kpis without the upper bound.  metrics:
 * bits DAISY_KPI_PRECISION .. DAISY_KPI_AUC and DAISY_KPI_FULL_AUC; any other bit is DAISY_ERR_ARG (popularity, diversity
 * and coverage need the lists).  disc fp64 [disc_len] = 1 / log2(p + 2) and disc_cum = its running sum, built on the host
 * (needed for ndcg; disc_len > every position below the largest cutoff).  With h the positions < K, r the rank of a hit
 * among the hits, Ke = min(K, eligible): precision h / Ke; recall h / gt_len; hit; mrr 1 / (min pos + 1) if < K; map the
 * mean over the hits of (r + 1) / (pos + 1); ndcg sum disc[pos] / disc_cum[h - 1]; f1 2 pre rec / (pre + rec); auc sum
 * over the hits of ((Ke - 1 - pos) - (h - 1 - r)) / (h (Ke - h)); full_auc, the same at every cutoff, sum over the T'
 * ranked targets of ((E - T') - (pos - r)) / (T' (E - T')).  0 / 0 is NaN, as in daisy_ranking_kpis.  Outputs as there:
 * per_user fp64 [slots, nc, n] or NULL, means fp64 [slots, nc]; slots in bit order.  Sums run in a fixed order. */
#define DAISY_KPI_FULL_AUC 11
size_t daisy_position_kpis_workspace_bytes(int64_t n, int32_t nc, uint32_t metrics);
int daisy_position_kpis(const int64_t *out_indptr, const int32_t *positions, const int64_t *gt_len, const int32_t *eligible,
                        int64_t n, const int32_t *cutoffs_host, int32_t nc, const double *disc, const double *disc_cum,
                        int64_t disc_len, uint32_t metrics, double *per_user, double *means, void *workspace,
                        size_t workspace_bytes, daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Preprocessor.process (daisy/utils/loader.py:176-189) and split_test / split_validation (daisy/utils/splitter.py):
 * csrc/prep.hip, csrc/split.hip; DESIGN.md §21.  Integer work throughout: no floating-point atomics, two calls give the
 * same bytes.  The entries allocate their own scratch, read a few totals back and return with the stream drained.
 * ---------------------------------------------------------------------- */
/* codes int32 [n] = the rank of ids[e] (any int64) among the column's distinct values; tokens int64 [n]: the distinct
 * values ascending in its first *n_distinct_host (HOST) places.  Sort, run heads, scan, scatter.  1 <= n < 2^31. */
int daisy_prep_encode(const int64_t *ids, int64_t n, int32_t *codes, int64_t *tokens, int64_t *n_distinct_host,
                      daisy_stream_t stream);
enum { DAISY_PREP_ORIGIN = 0, DAISY_PREP_FILTER = 1, DAISY_PREP_CORE = 2 };      /* prepro 'origin', 'Nfilter', 'Ncore' */
/* The whole of process() on the raw columns users / items / timestamp (int64 [n]) and rating (fp64 [n]; may be NULL
 * without a threshold):
 *   drop_duplicates([user, item], keep='last') - the largest row number of every pair stays;
 *   rating >= threshold when use_threshold != 0 (a NaN is dropped);
 *   mode FILTER, or CORE at level 1 (u) / 2 (i): one pass against the counts of that frame; CORE at level 3 (ui):
 *   round-synchronous peeling - every live row whose user or item has < N live rows leaves, the counts follow, until a
 *   round removes nothing (one word read by the host per round);
 *   the category codes of the survivors and their tokens; the stable sort by timestamp (ties stay in row order);
 *   item_pop fp64 [item_num] = count / user_num when want_pop != 0.
 * Outputs (device, room for n each): rows int64 = positions in the input in final order, user_code / item_code int32,
 * uid_token / iid_token int64 ascending, item_pop.  stats_host int64 [4] (HOST) = rows kept, user_num, item_num, peel
 * rounds that removed rows.  1 <= n < 2^31, N >= 1. */
int daisy_prep_process(const int64_t *users, const int64_t *items, const double *rating, const int64_t *timestamp, int64_t n,
                       int32_t use_threshold, double threshold, int32_t mode, int32_t level, int32_t N, int32_t want_pop,
                       int64_t *rows, int32_t *user_code, int32_t *item_code, int64_t *uid_token, int64_t *iid_token,
                       double *item_pop, int64_t *stats_host, daisy_stream_t stream);
enum { DAISY_SPLIT_TLOO = 0, DAISY_SPLIT_UTFO = 1, DAISY_SPLIT_UFO = 2, DAISY_SPLIT_RLOO = 3, DAISY_SPLIT_RSBR = 4 };
/* splitter.py:50-86 over dense user codes (int32 [n], < user_num; unused by RSBR):
 *   TLOO  per user the row of the largest timestamp (int64 [n]), ties to the earliest row; test in ascending row order;
 *   UTFO  per user the rows after its first ceil(len * one_minus_size) in row order (one_minus_size = 1 - size from the
 *         caller, as the reference forms it);
 *   UFO / RLOO / RSBR  every row gets the Philox key of (seed, fold, row); the first rint(len * size) rows of every user
 *         in key order (UFO), the first one (RLOO), the first (int64)(n * size) of all rows (RSBR).
 * test int64 [n]: users ascending, within a user by row (UTFO) or key (random methods); train int64 [n]: the complement,
 * ascending.  counts_host int64 [2] (HOST) = the lengths of train and test.  1 <= n < 2^31, 0 < size < 1. */
int daisy_split_ids(int32_t method, const int32_t *user_code, const int64_t *timestamp, int64_t n, int64_t user_num, double size,
                    double one_minus_size, uint64_t seed, uint64_t fold, int64_t *train, int64_t *test, int64_t *counts_host,
                    daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * get_history_matrix (daisy/utils/utils.py:87-123), the CSR that AERecommender.get_user_rating_matrix implies
 * (AbstractRecommender.py:147-158) built without the padded pair, and pandas.unique's first-seen order (AEDataset,
 * dataset.py:52): csrc/history.hip; DESIGN.md §23.  row / col: dense int32 codes in frame order, row < row_num,
 * col < col_num (the caller checks the ranges); val fp64 [n] or NULL for all ones, cast to fp32 once.  Integer work
 * apart from that cast, no floating-point atomic, two calls give the same bytes.  The entries allocate their own
 * scratch and return with the stream drained.  1 <= n < 2^31, 1 <= row_num, col_num < 2^31.
 * ---------------------------------------------------------------------- */
/* history_len int64 [row_num] = the entries of every row; *longest_host (HOST) = the longest.  Also what the fill reads:
 * order int32 [n] = the frame positions in a stable sort by row code, start int64 [row_num + 1] = where every row's
 * entries begin in it. */
int daisy_history_counts(const int32_t *row, int64_t n, int64_t row_num, int32_t *order, int64_t *start,
                         int64_t *history_len, int64_t *longest_host, daisy_stream_t stream);
/* history_matrix int64 [row_num, L], history_value fp32 [row_num, L]: row r = its entries in frame order from column 0,
 * then zeros.  Every cell is written exactly once (no memset); cell indices are 64-bit.  order / start from
 * daisy_history_counts, L >= the longest row. */
int daisy_history_fill(const int32_t *order, const int64_t *start, const int32_t *col, const double *val, int64_t n,
                       int64_t row_num, int64_t L, int64_t *history_matrix, float *history_value, daisy_stream_t stream);
/* The rows of the rating matrix the padded pair stands for, as a CSR: row_ptr int64 [row_num + 1], out_col int32 and
 * out_val fp32 (room for n each), columns ascending within a row.  Of a duplicated (row, col) the last in frame order
 * stays; a row shorter than the longest loses its column 0 (the padding overwrites it); a row as long as the longest
 * keeps it; entries whose fp32 value is 0 are dropped.  totals_host int64 [2] (HOST) = nnz, the longest row. */
int daisy_history_csr(const int32_t *row, const int32_t *col, const double *val, int64_t n, int64_t row_num, int64_t col_num,
                      int64_t *row_ptr, int32_t *out_col, float *out_val, int64_t *totals_host, daisy_stream_t stream);
/* out int64 (room for min(n, id_num)): the distinct values of ids (int32 [n], < id_num) in order of first appearance;
 * *count_host (HOST) = their number.  Integer atomicMin of the frame position per id, then a compaction in frame order. */
int daisy_history_first_seen(const int32_t *ids, int64_t n, int64_t id_num, int64_t *out, int64_t *count_host,
                             daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * iALS / WRMF (Hu, Koren, Volinsky 2008; no counterpart in the reference): weighted matrix factorisation of implicit
 * feedback by alternating least squares (csrc/ials.hip).  The tables are fp32 [n, d] with an explicit row
 * pitch (ld >= d, in elements), 1 <= d <= DAISY_IALS_MAX_D; the sparse operand is daisy_slim_gram's CSR (row_ptr int64
 * [rows + 1], col int32, val fp32 - nnz entries each).  All arithmetic between the fp32 operands and the fp32 result is
 * fp64 in a fixed order: no floating-point atomics, two calls give the same bits.
 * ---------------------------------------------------------------------- */
#define DAISY_IALS_MAX_D 128
/* G fp64 [d, d] = Y^T Y on the fp64 MFMA: blocks of rows write partial products, a second pass adds them in block order.
 * G is bitwise symmetric.  n >= 1. */
size_t daisy_ials_gram_workspace_bytes(int64_t n, int32_t d);
int daisy_ials_gram(const float *Y, int64_t n, int64_t ld, int32_t d, double *G, void *workspace, size_t workspace_bytes,
                    daisy_stream_t stream);
/* One half-sweep: for every CSR row u, X[u] = fp32(A_u^-1 b_u) with A_u = G + reg I + sum_i alpha r_ui y_i y_i^T and
 * b_u = sum_i (1 + alpha r_ui) y_i over the row's entries in stored order, G = Y^T Y of the other side's table Y
 * [n_other, d] (daisy_ials_gram).  One workgroup per row: the rank-one updates on the fp64 MFMA, a Cholesky factorisation
 * and both triangular solves in LDS.  An empty row gives exact zeros.  A column id outside [0, n_other) contributes
 * nothing (callers validate).  A pivot that is not positive and finite makes the row's output NaN and records
 * 1 + the row index in *info (int32, device) by an integer atomicMin: the smallest such row, 0 when there is none.
 * dump_A fp64 [rows, d, d] (full symmetric) and dump_b fp64 [rows, d], each or both NULL, receive the systems before
 * they are factored.  reg = 0 is allowed. */
int daisy_ials_half_sweep(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t rows, int64_t nnz,
                          int64_t n_other, const float *Y, int64_t ldy, int32_t d, const double *G, double alpha, double reg,
                          float *X, int64_t ldx, int32_t *info, double *dump_A, double *dump_b, daisy_stream_t stream);
/* *out (fp64, device) = sum_u [ x_u^T G x_u + sum_{i in row u} ((1 + alpha r_ui)(1 - s_ui)^2 - s_ui^2) ]
 *                       + reg (|X|^2 + trace G), s_ui = <x_u, y_i>: the weighted squared error over ALL cells plus the
 * regulariser, without a pass over the cells.  One partial per row (the workspace), added in a fixed order. */
size_t daisy_ials_objective_workspace_bytes(int64_t rows);
int daisy_ials_objective(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t rows, int64_t nnz,
                         int64_t n_other, const float *X, int64_t ldx, const float *Y, int64_t ldy, int32_t d, const double *G,
                         double alpha, double reg, double *out, void *workspace, size_t workspace_bytes,
                         daisy_stream_t stream);

/* ------------------------------------------------------------------------
 * Two-hop walk with a per-row top-K (csrc/walk2.hip; additive to ABI 8): the primitive of RP3beta and
 * P3alpha (Cooper et al. 2014, Paudel et al. 2016; no counterpart in the reference).  A is a CSR [n_rows, inner], B a CSR
 * [inner, n_cols], both of daisy_slim_gram's layout (row_ptr int64, col int32, val fp32); the columns of every row of B
 * are ascending and distinct (callers validate).  For every row i of A:
 *   acc[j] = sum over the stored entries u of row i, in stored order, of A[i, u] * B[u, j]: every product rounded to fp32,
 *            then added in fp32 (no fused multiply-add);
 *   w[j]   = acc[j] * col_scale[j], one rounded fp32 multiply (col_scale == NULL: w = acc); zero_diagonal: w[i] = 0;
 *   the K largest strictly positive w are kept, ties at the boundary to the LOWER j; zero, negative and NaN never;
 *   normalize: the kept values are divided by their fp32 sum, taken in ascending j.
 * Outputs in daisy_knn_select's fixed-pitch form: count int32 [n_rows]; cols int32 / vals fp32 [n_rows, K], ascending j,
 * unused slots (-1, 0).  1 <= K <= DAISY_KNN_MAX_K (K >= n_cols is allowed).  A column id of A outside [0, inner) or of B
 * outside [0, n_cols) contributes nothing.
 * One workgroup per source row at a time, rows handed out by an integer counter; the dense accumulator over n_cols lives in
 * LDS (path LDS; AUTO up to DAISY_WALK2_LDS_COLS columns) or in a slab of the workspace per workgroup (path GLOBAL;
 * DAISY_SLIM_PATH_*).  n_groups: the workgroups of the launch (0: chosen from the shape).  No floating-point atomics:
 * every acc[j] receives its terms in ascending u whatever the path and n_groups - two runs, the two paths and any two
 * n_groups give the same bits.  The work is the number of two-hop paths, the memory n_rows * K. */
#define DAISY_WALK2_LDS_COLS 32768
/* bytes of workspace daisy_walk2_topk needs (the row counter, and the slabs of path GLOBAL); 0 on bad arguments */
size_t daisy_walk2_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t path, int32_t n_groups);
int daisy_walk2_topk(const int64_t *a_ptr, const int32_t *a_col, const float *a_val, int64_t n_rows, int64_t inner,
                     const int64_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t n_cols, const float *col_scale,
                     int32_t zero_diagonal, int32_t normalize, int32_t K, int32_t *count, int32_t *cols, float *vals,
                     int32_t path, int32_t n_groups, void *workspace, size_t workspace_bytes, daisy_stream_t stream);

/* micro-benchmarks of the memory system used to place the kernels on the
 * roofline (tools/membench.py); not part of the reference surface. */
int daisy_membench(int32_t what, float *table, int64_t rows, int32_t d, const int32_t *idx,
                   int64_t n, float *out, daisy_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DAISYREC_AMD_H */
