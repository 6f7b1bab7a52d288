// Segmented sum over entries sorted by row (segsum.hip): the library's sparse x dense product.
//   out[row] = sum over the row's entries e of  w_e * X[col_e]
// Callers: the MF item gradient of the phase kernels (bpr_train.hip: rows = items, X = P, w = the loss coefficients),
// LightGCN's propagation (lightgcn.hip) and the NeuMF table scatter (neumf_scatter.hip).
#pragma once

#include "epoch_plan.h"

namespace daisy {

// Segments shared by neighbouring chunks leave their chunk as edge records, which k_item_edges chains in chunk order.
// Scratch for segsum_chunks(n_entries, d) chunks.
struct ItemEdges {
    float *vec;          // [2*nchunks][d]  partial gradient rows; [2c] head edge (inherited), [2c+1] tail edge
    int32_t *item;       // [2*nchunks]     their item (-1: none)
    float *b;            // [2*nchunks]     FM: partial coefficient sums
    int32_t *whole;      // [nchunks]       the head edge's segment also runs on into the next chunk
    const double *halt = nullptr;   // BatchView::halt of the step the records belong to
};

// Chunks of a sum over n_entries entries of width d: an upper bound for every caller.  It is computed from the default
// run length of the row shape (RunCfg<C>); segsum_rows' longer runs on wide rows only make larger, hence fewer, chunks.
int64_t segsum_chunks(int64_t n_entries, int d);

// out[row] = sum over the row's entries of coef[e].x * X[col_e] on a synthetic view: ekey[e] = row << 1,
// esu[e] = (e, col), coef[e] = (value, 0).  Rows without entries are not written; n_entries must be even.
// edge_* are scratch for segsum_chunks(n_entries, d) chunks: vec f32[2*chunks*d], item i32[2*chunks],
// b f32[2*chunks], whole i32[chunks].  x_bf16: X holds bf16 rows (uint16_t [rows][d]) instead of fp32.
int segsum_rows(const float *X, const float2 *coef, const uint32_t *ekey, const uint2 *esu, int64_t n_entries,
                int d, float *out, float *edge_vec, int32_t *edge_item, float *edge_b, int32_t *edge_whole,
                hipStream_t s, bool x_bf16 = false);

// The MF item gradient's data term over the 2*v.B item-sorted entries of a batch:
//   gQ[item] = sum_e c_e * P[u(e)],  g_bi[item] = sum_e c_e  (g_bi may be NULL)
// `edges` holds records for segsum_chunks(2 * v.B, d) chunks; its halt is taken from the view.
int segsum_item_grad(const BatchView &v, const float *P, const float2 *coef, int d, float *gQ, ItemEdges edges,
                     float *g_bi, hipStream_t s);

}  // namespace daisy
