// Shared between csrc/neumf.hip (the layer-by-layer NeuMF step), csrc/neumf_tower.hip (the fused tower kernel) and
// csrc/neumf_mid.hip (the small-step kernel): the argument blocks of the two fused kernels and their entry points.
#pragma once
#include "common.h"

namespace daisy {

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

// ---- the small-step kernel (csrc/neumf_mid.hip): a step of at most 1024 rows whose MLP weights fit the LDS - the gather, every
// layer, the predict layer, the criterion and their backward pass, everything before the scatter, in ONE launch (fp32)
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
