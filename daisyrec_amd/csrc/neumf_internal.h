// Shared between csrc/neumf.hip (the NeuMF step and its layer-by-layer kernels), csrc/neumf_scatter.hip (the embedding
// gradients), csrc/neumf_tower.hip (the fused tower kernel) and csrc/neumf_mid.hip (the small-step kernel): what a call
// runs, the scatter's state and the argument blocks and entry points of the two fused kernels.
#pragma once
#include "common.h"
#include "pairs.h"

namespace daisy {

// ---- what one call runs: resolved once per call (neumf_path, csrc/neumf.hip) and handed on; nobody decides again
struct NeumfPath {
    bool H;                           // bf16 storage (precision level 2) with every GEMM of the call made of whole tiles
    bool mid;                         // everything between the gather and the scatter in one launch (csrc/neumf_mid.hip)
    bool fact;                        // the first layer through the embedding tables
    bool tower;                       // layers 2..3, predict layer, criterion and their backward pass fused (csrc/neumf_tower.hip)
    bool params_aligned;              // every parameter and table of the call is 16-byte aligned (k_nmf_mid reads float4)
    bool w23_aligned;                 // W2 / W3 are 16-byte aligned (the tower reads them as float4)
};

// ---- the embedding gradients (csrc/neumf_scatter.hip)
constexpr int kScanMaxRows = 8192;    // most rows of a step the scanning kernel takes (its keys, masks and round numbers: 116 KB of LDS)

// The scatter's state: the context's shape (filled in by daisy_neumf_ctx_create) and the scratch of the owner-based chain,
// allocated at its first use and freed by neumf_scatter_release.
struct NeumfScatter {
    int64_t max_rows, U, I;
    int d, dm, model;
    DeviceArena arena;
    int32_t *ku, *ki, *val, *ks, *vs, *cu, *ci, *cj;
    uint32_t *ekey; uint2 *esu; float2 *w;
    // row sums by table row: MLP users, MLP items, GMF users, GMF items (adjacent slots, all-zero between calls).  With
    // path.fact the first two are left holding S_u / S_i, the segment sums of dZ_1: the first layer's backward pass through
    // the tables (csrc/neumf.hip) reads them and zeroes them again
    float *sum, *sum2, *sumg, *sumg2, *edge_vec, *edge_b;
    int32_t *edge_item, *edge_whole;
    void *tmp; size_t tmp_bytes;
    DeviceArena cs_arena;             // the counting pass's two buffers: both or neither
    int32_t *cs_hist;                 // [2 sides][kCsNW waves][key stride] counts -> prefixes, then [2][stride] totals
    void *cs_ent;                     // the two sides' entry lists (CsEntries)
};
// g.{uG,iG,uM,iM} += the embedding gradients of the step and the regulariser's.  DX0: the MLP tower's input gradient,
// [R, 2*dm] (bf16 under path.H); with path.fact it is dZ_1 (bf16 [R, n1]) and the MLP tables' share is left in sum / sum2
int neumf_scatter(NeumfScatter &sc, const NeumfPath &path, const daisy_neumf_params &p, const daisy_neumf_params &g,
                  const PairSrc &src, int64_t R, int pointwise, const float *dpred, const float *DX0, const double *stats,
                  float reg_1, float reg_2, hipStream_t s);
void neumf_scatter_release(NeumfScatter &sc);

// ---- the fused tower kernel (csrc/neumf_tower.hip): layers 2..3 + predict layer + criterion + their backward pass
struct TowerArgs {
    const uint16_t *tu, *ti;          // bf16 [U][4d], [I][4d]: the first layer's table products (FACT)
    const float2 *nu, *ni;            // per table row (sum |x|, sum x^2) of uM / iM
    const float *b1;                  // [4d]
    const float *W2, *W3;             // fp32 [2d][4d], [d][2d] (16-byte aligned): rounded to bf16 as the kernel loads them
    const float *b2, *b3, *Wp, *bp;   // fp32 [2d], [d], [2d], [1]
    const float *uG, *iG;             // fp32 [U][d], [I][d]
    const int32_t *u, *i, *j;         // the batch (j: negatives, or the labels of a point-wise loss)
    int64_t B;
    int pointwise, loss_type;
    float gamma;
    uint16_t *dZ1;                    // out: bf16 [R][4d], gradient wrt the first layer's pre-activation
    float *dpred;                     // out: [R]
    float *ws;                        // per-workgroup partial sums (neumf_tower_ws_bytes)
    double *wsd;                      // (set by neumf_tower_step: the doubles behind the floats of `ws`)
};
int neumf_tower_blocks(int64_t tiles);
size_t neumf_tower_ws_bytes(int d, int nblocks);
// one launch of the tower over R rows + the fixed-order reduction of the workgroups' sums into the gradients (+=) and stats
int neumf_tower_step(const TowerArgs &args, int d, int64_t R, float *gW2, float *gW3, float *gb2, float *gb3, float *gWp,
                     float *gbp, double *stats, float reg_1, float reg_2, hipStream_t s);

// ---- the small-step kernel (csrc/neumf_mid.hip): a step of at most kScanMaxRows rows whose MLP weights fit the LDS - the gather,
// every layer, the predict layer, the criterion and their backward pass, everything before the scatter, in ONE launch (fp32)
struct MidArgs {
    const float *uG, *iG, *uM, *iM;   // the embedding tables ([U][d], [I][d], [U][dm], [I][dm]); u, i, j: the batch
    const int32_t *u, *i;
    int dm;
    float *DX0;                       // out: [R][w0] gradient wrt x0 = [uM[u] | iM[item]] (dropout mask of the input applied)
    float *pred, *dpred;              // out: [R]
    const float *W[DAISY_NEUMF_MAX_LAYERS], *b[DAISY_NEUMF_MAX_LAYERS];
    const float *Wp, *bp;
    int width[DAISY_NEUMF_MAX_LAYERS + 1];
    int L, d;
    const int32_t *j;                 // the negatives, or the labels of a point-wise loss
    int B, R, pointwise, loss_type;
    float gamma;
    uint32_t thresh;                  // dropout: keep threshold (0: off), scale, seed
    float scale;
    uint64_t seed;
    float *ws;                        // per-workgroup partial sums (neumf_mid_ws_bytes)
};
bool neumf_mid_fits(int L, const int *width, int d);
size_t neumf_mid_ws_bytes(int L, const int *width, int d, int max_rows);
// the launch + the fixed-order reduction of the workgroups' sums into the gradients (+=), the loss and the norms
int neumf_mid_step(const MidArgs &args, float *const *gW, float *const *gb, float *gWp, float *gbp, double *stats, float reg_1,
                   float reg_2, hipStream_t s);

}  // namespace daisy
