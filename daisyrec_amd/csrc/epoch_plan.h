// The epoch plan (epoch_plan.hip), the static train index it is partitioned from, and the two views of one batch that
// the step kernels read.
#pragma once

#include "common.h"

namespace daisy {

constexpr uint32_t kNegBit = 0x80000000u;

// What the step kernels see of the current batch (pointers into an epoch plan).
//   sample s in [0,B):  user = ukey[s] & umask,  (pos item, neg item) = ij[s]
//                       samples of one user are contiguous (stable order)
//   entry  q in [0,2B): item = (ekey[q] & imask) >> 1, negative slot = ekey[q] & 1 (ascending, stable),
//                       esu[q] = (sample position s | kNegBit for the negative slot, user of s)
struct BatchView {
    const uint32_t *ukey;
    const int2 *ij;
    const uint32_t *ekey;
    const uint2 *esu;
    // run-length encoding of the batch's entry keys: run m in [run_off[0], run_off[1]) has
    // run_key[m] = item << 1 | neg and run_cnt[m] entries (an item owns 1 or 2 adjacent runs)
    const uint32_t *run_key, *run_cnt;
    const int32_t *run_off;
    uint32_t umask, imask;
    // point-wise losses (CL / SL, MFRecommender.py:75-81): ij[s] = (item, label); the "negative"
    // slot of a sample is an inert copy of its item (coefficient 0, not counted by the regulariser)
    int32_t pointwise;
    int64_t B;
    // FM (FMRecommender.py:61-68): score += u_bias[u] + i_bias[item] + bias_; bu == nullptr -> plain MF.
    // g_bi accumulates like gQ (zero between steps, consumed by k_item_apply); g_bu / g_b0 are only
    // written by the gradient-output user pass (Adam); the SGD user pass updates bu and b0 in place.
    float *bu, *bi, *b0;
    float *g_bu, *g_bi, *g_b0;
    // set for the duration of daisy_bpr_sgd_step / daisy_bpr_fit_epoch_sgd: the epoch's count of non-finite step
    // losses (epoch_acc[1]).  Once it is > 0 every kernel that changes a table returns at once: the epoch stops at its
    // first non-finite loss like the reference's loop (AbstractRecommender.py:122-123), with one host sync per epoch
    const double *halt;
};

// What the STAGED step (bpr_staged.hip and its two passes, bpr_staged_user.hip / bpr_staged_item.hip) sees of the current batch.  Either layout of the epoch plan
// can feed it:
//   sample s in [0,B):  partitioned layout: s_rec[s] = {user, pos item, neg item, epoch position}, stage slot of the sample
//                       = position - pos_base;   sorted layout (s_rec == NULL): user = s_user[s] & umask, (pos item, neg
//                       item) = s_ij[s], stage slot = s.  Samples of one user are contiguous; the slots are a bijection
//                       onto [0,B)
//   entry  q in [0,E):  item = (e_key[q*e_kstride] & imask) >> 1, negative slot = e_key[..] & 1 (ascending, stable);
//                       stage slot of the sample it belongs to = (e_pos[q*e_stride] & ~kNegBit) - pos_base
//                       (partitioned layout: 8-byte records {key, position}, both strides 2)
struct StreamView {
    const uint4 *s_rec;
    const uint32_t *s_user;
    const int2 *s_ij;
    const uint32_t *e_key;
    const uint32_t *e_pos;
    uint32_t umask, imask;
    int32_t e_kstride, e_stride;
    uint32_t pos_base;
    int64_t B, E;
    const double *halt;      // see BatchView::halt
    int32_t pointwise;       // rows are (user, item, label): E = B entries in the partitioned layout; the sorted
                             // layout keeps an inert negative slot per sample (E = 2B)
    int32_t p_stream;        // the user pass reads and writes P past the caches (tables far beyond them: set by the host)
};
// the sample as {user, pos item, neg item, stage slot} / the user alone / an entry's key  (any layout; the hot kernels
// read the layout they were compiled for directly)
__device__ __forceinline__ uint4 sv_sample(const StreamView &v, int64_t s) {
    if (v.s_rec) { uint4 r = v.s_rec[s]; r.w -= v.pos_base; return r; }
    const int2 ij = v.s_ij[s];
    return make_uint4(v.s_user[s] & v.umask, (uint32_t)ij.x, (uint32_t)ij.y, (uint32_t)s);
}
__device__ __forceinline__ uint32_t sv_user(const StreamView &v, int64_t s) {
    return v.s_rec ? v.s_rec[s].x : (v.s_user[s] & v.umask);
}
__device__ __forceinline__ uint32_t sv_key(const StreamView &v, int64_t e) { return v.e_key[e * v.e_kstride] & v.imask; }
}  // namespace daisy

// Static index of a training set (built once per fit): the triples in CSR (user-sorted) order and
// their item entries sorted by item.  The partitioned epoch plan is two stable one-digit partitions
// of these arrays by batch id.
struct daisy_train_index {
    int64_t n, U, I;
    int32_t user_base;
    const int32_t *triples;   // [n][3] CSR order: the caller's array, or `sorted_copy`
    daisy::DeviceArena keep;  // ent_t, ent_key and - the caller's array was not user-sorted - sorted_copy, orig
    int32_t *sorted_copy;     // owned copy when the caller's array was not user-sorted
    uint32_t *orig;           // [n] row of the caller's array behind CSR row t (NULL: identity); epoch positions
                              //     (perm / Feistel / identity) always refer to the caller's rows
    uint32_t *ent_t;          // [2n] triple index | slot << 31, sorted by ent_key (stable: t ascending)
    uint32_t *ent_key;        // [2n] item << 1 | slot
    int32_t pointwise;        // rows are (user, item, label): ONE entry per row (n_ent = n), else two (n_ent = 2n)
    int64_t n_ent;
    int64_t max_item_entries; // entries of the most frequent item (the longest segment an item pass can meet, scaled by
                              // the batch's share of the set: decides whether its edge chains are reduced in two levels)
};

// Epoch plan: the whole epoch laid out batch by batch (see the header comment of epoch_plan.hip).
// Two layouts:
//   kind 0 (sorted, daisy_epoch_plan_build):          packed sort keys + run lists; every phase kernel reads it
//   kind 1 (partitioned, daisy_epoch_plan_build_indexed): plain SoA records, 32 B per interaction; staged step only
struct daisy_epoch_plan {
    int64_t max_triples, U, I;
    daisy::DeviceArena arena;    // kind 0 buffers (allocated by the first daisy_epoch_plan_build)
    size_t temp_bytes;
    // double buffers of the two radix sorts
    uint32_t *k32[2];     // [2n] 32-bit keys
    uint64_t *k64[2];     // [2n] 64-bit keys (only when batch bits + id bits > 32)
    uint64_t *v64[2];     // [2n] payloads
    uint32_t *ukey;       // [n]  sorted sample keys (batch << ubits | user)
    uint64_t *uval;       // [n]  (i, j)
    uint32_t *ekey;       // [2n] sorted entry keys (batch << ibits | item)
    uint64_t *eval;       // [2n] (s | neg, u)
    uint32_t *run_key;    // [2n]  item << 1 | neg of every run of equal entry keys
    uint32_t *run_cnt;    // [2n]  its length
    int32_t *run_off;     // [max_triples+2] first run of every batch; [num_batches] = total
    uint32_t *run_total;  // [1]   number of runs (device)
    int *bad;             // [1]   bit 0: an id of the last build lay outside the tables, bit 1: a bad permutation entry
    uint32_t umask, imask;
    void *temp;
    int64_t n, batch_size, num_batches;
    int32_t pointwise;
    bool built;
    int32_t kind;
    // kind 1 buffers: record set [x] of the LSD passes.  part[0] (allocated by the first daisy_epoch_plan_build_indexed) also
    // holds the counts, the scan scratch, p_inv and p_park; part[1] is allocated by the first build of more than 256 batches,
    // whose LSD passes ping-pong between the sets
    daisy::DeviceArena part[2];
    uint4 *p_srec[2];                   // [n]   sample records {user, pos item, neg item / label, epoch position}
    uint2 *p_erec[2];                   // [2n]  entry records {item << 1 | slot, epoch position of the sample}
    uint32_t *p_counts, *p_offsets;     // [ndig * ntiles] per-tile digit counts / their exclusive scan
    uint32_t *p_inv;                    // [n]   inverse of an explicit permutation (DAISY_ORDER_PERM)
    uint32_t *p_park;                   // [2n]  device shuffle: the epoch positions the entry records' counting kernel walked
                                        //       to, parked for their scatter kernel
    void *p_scan;                       // rocPRIM scan scratch
    size_t p_scan_bytes;
    int32_t p_cur;                      // record set holding the finished plan
    double hot_item_share;              // max_item_entries / n_ent of the index the plan was built from
    uint64_t build_gen;                 // id of the build the plan currently holds, unique in the process (what a
                                        // batch index refers to: a context that computed something ahead for "batch k+1"
                                        // must not mistake a rebuilt - or another plan at the same address - for it)
    // daisy_epoch_plan_build_positions: this plan holds a SUBSET of the epoch's rows (one rank's share), batch k =
    // the held rows whose epoch position lies in [k*B, (k+1)*B): record ranges differ per batch
    int64_t *h_off;                     // host, [num_batches+1] first record of every batch (NULL: k*batch_size)
    int64_t *d_off;                     // device scratch of the same
    int64_t h_off_cap;
};

namespace daisy {
// what the step files call.  A plan owns no device memory until its first build; plan_bytes: both layouts' arenas now
int plan_alloc(daisy_epoch_plan **out, int64_t max_triples, int64_t U, int64_t I);
int plan_free(daisy_epoch_plan *p);
size_t plan_bytes(const daisy_epoch_plan *p);
int plan_build(daisy_epoch_plan *p, const int32_t *triples, int64_t n, int64_t start, const int64_t *perm, int order_mode,
               uint64_t seed, uint64_t epoch, int64_t batch_size, int32_t user_base, int32_t flags, hipStream_t s,
               int64_t perm_limit = -1);
int plan_report_bad(const daisy_epoch_plan *p, const char *who, hipStream_t s);
BatchView plan_view(const daisy_epoch_plan *p, int64_t k);                 // batch k of the sorted layout
StreamView stream_view_of(const BatchView &v);
StreamView plan_stream_view(const daisy_epoch_plan *p, int64_t k);         // batch k of the partitioned layout
}  // namespace daisy
