// MF + BPR training step for gfx950 (MI355X): hand-written gather / dot /
// loss-coefficient / scatter-update kernels.
//
// Reference semantics being reproduced (file:line in AmazingDD/daisyRec):
//   loader       daisy/utils/dataset.py:5-27 (DataLoader(shuffle=True) over BasicDataset)
//   forward      daisy/model/MFRecommender.py:63-68
//   loss         daisy/model/MFRecommender.py:70-97 + daisy/utils/loss.py:5-33
//   backward     autograd through 7 embedding lookups (AbstractRecommender.py:125)
//   SGD / Adam   daisy/model/AbstractRecommender.py:48-67,126
//
// The step is BATCH SYNCHRONOUS like autograd + optimizer.step: every gradient
// is formed from the tables as they were when the step began.  The kernel order
// guarantees it without a copy of the tables:
//   k_fwd          reads P,Q            writes coef, partial sums
//   k_item_grad_*  reads P,Q            writes gQ  (side buffer; also what the
//                                       multi-GPU path all-reduces; throughput
//                                       mode: segsum.hip, data term only)
//   k_user         reads P[u] (owner),Q writes P[u]   (one owner per user row:
//                                       every batch is grouped by user)
//   k_item_apply   reads gQ,Q           writes Q, zeroes gQ
//
// Measured on MI355X (profiles/r01_probe_*): random 256-B row gathers / plain
// stores run at 5-8 TB/s, fp32 global atomics at 0.3 TB/s.  So every scatter is
// organised around OWNERSHIP instead of atomics: the epoch plan (epoch_plan.hip)
// hands over every batch grouped by user, plus a list of its item entries sorted
// by item; the item gradient is then a segmented reduction over that list
// (segsum.hip).  Lazy Adam for the tables: adam_lazy.hip.
//
// HBM/L2 view: a d=64 row is 256 B = 16 lanes x float4, one coalesced request
// per quarter wave; four rows are in flight per wave instruction.
#include <string.h>

#include "bpr_staged.h"
#include "segsum.h"

namespace daisy {

// daisy_bpr_set_batch: three id columns -> the rows a one-batch plan is built from
__global__ void k_pack_triples(const int32_t *__restrict__ u, const int32_t *__restrict__ i,
                               const int32_t *__restrict__ j, int64_t B, int32_t *__restrict__ out) {
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < B;
         s += (int64_t)gridDim.x * blockDim.x) {
        out[3 * s] = u[s]; out[3 * s + 1] = i[s]; out[3 * s + 2] = j[s];
    }
}

// ---------------------------------------------------------------------------
// forward: scores, coefficients, the seven batch sums
// ---------------------------------------------------------------------------
// A lane group takes a run of LPR consecutive samples: lane x loads the ids of sample x (one
// coalesced read), the rows of FWD_SUB samples are in flight together, their two scores land in
// lane x, and the loss epilogue (exp/log) is evaluated once per run with one sample per lane
// instead of once per sample on a single lane.
constexpr int kFwdSub = 4;      // samples whose rows are in flight together, at up to 4 floats per lane
template <class C>
struct FwdCfg {
    static constexpr int RUN = C::LPR;
    static constexpr int SUB = (C::NE <= 4) ? kFwdSub : ((C::NE <= 8) ? 2 : 1);
};

template <class C, bool POINTWISE>
__global__ __launch_bounds__(kBlock) void k_fwd(const float *__restrict__ P,
                                                const float *__restrict__ Q, BatchView v, int d,
                                                int loss_type, float gamma,
                                                float2 *__restrict__ coef,
                                                double *__restrict__ partials) {
    constexpr int RUN = FwdCfg<C>::RUN, SUB = FwdCfg<C>::SUB;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const int64_t nruns = (v.B + RUN - 1) / RUN;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t r = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; r < nruns; r += gstride) {
        const int64_t t0 = r * RUN;
        const int cnt = (v.B - t0 < RUN) ? (int)(v.B - t0) : RUN;
        // the ids of a tail run are clamped to its last sample, so no load sits behind a branch
        // (a guarded load makes the compiler drain vmcnt first); the duplicates are masked below
        const int64_t il = t0 + ((lane < cnt) ? lane : cnt - 1);
        const int32_t my_u = (int32_t)(v.ukey[il] & v.umask);
        const int2 my_ij = v.ij[il];
        float my_pos = 0.f, my_neg = 0.f;
#pragma unroll
        for (int x0 = 0; x0 < RUN; x0 += SUB) {
            Row<C> p[SUB], qi[SUB], qj[SUB];
#pragma unroll
            for (int y = 0; y < SUB; ++y) {
                const int x = x0 + y;
                p[y].load_clamped(P + (int64_t)group_bcast<C>(my_u, x) * d, lane, d);
                qi[y].load_clamped(Q + (int64_t)group_bcast<C>(my_ij.x, x) * d, lane, d);
                if constexpr (!POINTWISE) qj[y].load_clamped(Q + (int64_t)group_bcast<C>(my_ij.y, x) * d, lane, d);
                else qj[y].zero();                       // point-wise: j is the label, no second row
            }
#pragma unroll
            for (int y = 0; y < SUB; ++y) {
                const float pos = row_dot<C>(p[y], qi[y]);
                const float neg = row_dot<C>(p[y], qj[y]);
                if (lane == x0 + y) { my_pos = pos; my_neg = neg; }
                const float w = (x0 + y < cnt) ? 1.f : 0.f;     // 0 for the clamped duplicates
#pragma unroll
                for (int k = 0; k < C::NE; ++k) {
                    acc[1] = fmaf(w, fabsf(p[y].v[k]), acc[1]);
                    acc[2] = fmaf(w, fabsf(qi[y].v[k]), acc[2]);
                    acc[4] = fmaf(w * p[y].v[k], p[y].v[k], acc[4]);
                    acc[5] = fmaf(w * qi[y].v[k], qi[y].v[k], acc[5]);
                    if constexpr (!POINTWISE) {
                        acc[3] = fmaf(w, fabsf(qj[y].v[k]), acc[3]);
                        acc[6] = fmaf(w * qj[y].v[k], qj[y].v[k], acc[6]);
                    }
                }
            }
        }
        if (lane < cnt) {
            if (v.bu) {                                   // FMRecommender.py:65-66
                const float b0 = v.b0[0], ub = v.bu[my_u];
                my_pos += (ub + v.bi[my_ij.x]) + b0;
                if constexpr (!POINTWISE) my_neg += (ub + v.bi[my_ij.y]) + b0;
            }
            float term, cp, cn;
            pair_coef(loss_type, my_pos, POINTWISE ? (float)my_ij.y : my_neg, gamma, term, cp, cn);
            coef[t0 + lane] = make_float2(cp, cn);
            acc[0] += term;
            acc[7] += cp + cn;                            // d loss / d bias_
        }
    }
    __shared__ double sm[kBlock / kWave][8];
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double w = wave_sum_f64((double)acc[k]);
        if ((threadIdx.x % kWave) == 0) sm[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) t += sm[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * 8 + threadIdx.x] = t;
    }
}

// fixed-order reduction of the per-workgroup sums -> stats[0..6]; FINALIZE: also the norms and
// the loss (single-GPU step: no all-reduce between the two); reduce_partials_block: bpr_internal.h
template <bool FINALIZE>
__global__ __launch_bounds__(kBlock) void k_reduce_partials(const double *__restrict__ partials,
                                                            int nblocks, double *__restrict__ stats,
                                                            float reg_1, float reg_2,
                                                            double *__restrict__ epoch_acc,
                                                            double *__restrict__ step_loss) {
    reduce_partials_block(partials, nblocks, stats, FINALIZE, reg_1, reg_2, epoch_acc, step_loss);
}

__global__ void k_finalize(double *__restrict__ stats, float reg_1, float reg_2,
                           double *__restrict__ epoch_acc, double *__restrict__ step_loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) finalize_stats(stats, reg_1, reg_2, epoch_acc, step_loss);
}

// ---------------------------------------------------------------------------
// item gradient, legacy mode: one fp32 atomic row per entry (kept for A/B
// measurements; 0.3 TB/s on MI355X)
// ---------------------------------------------------------------------------
template <class C, bool REG>
__global__ __launch_bounds__(kBlock) void k_item_grad_atomic(
    const float *__restrict__ P, const float *__restrict__ Q, BatchView v,
    const float2 *__restrict__ coef, int d, const double *__restrict__ stats, float reg_1,
    float reg_2, float *__restrict__ gQ) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const float rI = REG ? inv_or_zero(stats[DAISY_ST_NORM_I], reg_2) : 0.f;
    const float rJ = REG ? inv_or_zero(stats[DAISY_ST_NORM_J], reg_2) : 0.f;
    for (int64_t s = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; s < v.B; s += gstride) {
        const int64_t uu = v.ukey[s] & v.umask;
        const int2 ij = v.ij[s];
        const float2 c = coef[s];
        Row<C> p, gi, gj;
        p.load(P + uu * d, lane, d);
        if constexpr (REG) {
            Row<C> qi, qj;
            qi.load(Q + (int64_t)ij.x * d, lane, d);
            qj.load(Q + (int64_t)(v.pointwise ? ij.x : ij.y) * d, lane, d);
#pragma unroll
            for (int k = 0; k < C::NE; ++k) {
                gi.v[k] = fmaf(c.x, p.v[k], fmaf(rI, qi.v[k], reg_1 * sgn(qi.v[k])));
                gj.v[k] = fmaf(c.y, p.v[k], fmaf(rJ, qj.v[k], reg_1 * sgn(qj.v[k])));
            }
        } else {
#pragma unroll
            for (int k = 0; k < C::NE; ++k) {
                gi.v[k] = c.x * p.v[k];
                gj.v[k] = c.y * p.v[k];
            }
        }
        gi.atomic_add_to(gQ + (int64_t)ij.x * d, lane, d);
        if (!v.pointwise) gj.atomic_add_to(gQ + (int64_t)ij.y * d, lane, d);
        if (v.g_bi && lane == 0) {
            unsafeAtomicAdd(v.g_bi + ij.x, c.x);
            if (!v.pointwise) unsafeAtomicAdd(v.g_bi + ij.y, c.y);
        }
    }
}

// ---------------------------------------------------------------------------
// item gradient, reproducible mode: the group that sees the head of an item's
// run owns the row and sums its entries in plan order (fixed, so bitwise
// reproducible).   gQ[r] = sum_e c_e*p_u(e) + reg terms
// ---------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(kBlock) void k_item_grad_sorted(
    const float *__restrict__ P, const float *__restrict__ Q, const float2 *__restrict__ coef,
    BatchView v, int d, const double *__restrict__ stats, float reg_1, float reg_2,
    float *__restrict__ gQ) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const int64_t n = 2 * v.B;
    const float rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
    const float rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    for (int64_t pos = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; pos < n; pos += gstride) {
        const uint32_t r = (v.ekey[pos] & v.imask) >> 1;
        if (pos > 0 && ((v.ekey[pos - 1] & v.imask) >> 1) == r) continue;  // not a segment head
        Row<C> acc;
        acc.zero();
        float n_pos = 0.f, n_neg = 0.f, csum = 0.f;
        for (int64_t q = pos; q < n && ((v.ekey[q] & v.imask) >> 1) == r; ++q) {
            const uint2 su = v.esu[q];
            const bool is_neg = (su.x & kNegBit) != 0;
            const float2 c2 = coef[su.x & ~kNegBit];
            const float c = is_neg ? c2.y : c2.x;
            csum += c;
            n_pos += is_neg ? 0.f : 1.f;
            n_neg += (is_neg && !v.pointwise) ? 1.f : 0.f;
            Row<C> p;
            p.load(P + (int64_t)su.y * d, lane, d);
#pragma unroll
            for (int k = 0; k < C::NE; ++k) acc.v[k] = fmaf(c, p.v[k], acc.v[k]);
        }
        Row<C> qr;
        qr.load(Q + (int64_t)r * d, lane, d);
        const float w1 = reg_1 * (n_pos + n_neg);
        const float w2 = n_pos * rI + n_neg * rJ;
#pragma unroll
        for (int k = 0; k < C::NE; ++k) acc.v[k] += fmaf(w2, qr.v[k], w1 * sgn(qr.v[k]));
        acc.store(gQ + (int64_t)r * d, lane, d);
        if (v.g_bi && lane == 0) v.g_bi[r] = csum;
    }
}

// regulariser share of the item gradient (MFRecommender.py:88-89), one lane group per
// distinct item of the batch (head run of the plan's run list):
//   gQ[item] += reg_1*(np+nn)*sign(q) + reg_2*(np/|Q[i]|_F + nn/|Q[j]|_F)*q
__device__ __forceinline__ bool run_head(const BatchView &v, int64_t m, int64_t m0, int64_t m1,
                                         int64_t &item, float &fp, float &fn) {
    const uint32_t key = v.run_key[m];
    if (m > m0 && (v.run_key[m - 1] >> 1) == (key >> 1)) return false;   // the item's second run
    item = key >> 1;
    const float c = (float)v.run_cnt[m];
    fp = (key & 1u) ? 0.f : c;
    fn = (key & 1u) ? c : 0.f;
    if (!(key & 1u) && m + 1 < m1 && (v.run_key[m + 1] >> 1) == (key >> 1)) fn = (float)v.run_cnt[m + 1];
    if (v.pointwise) fn = 0.f;      // the negative slots are inert copies
    return true;
}

template <class C>
__global__ __launch_bounds__(kBlock) void k_item_reg(const float *__restrict__ Q, BatchView v, int d,
                                                     const double *__restrict__ stats, float reg_1,
                                                     float reg_2, float *__restrict__ gQ) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const int64_t m0 = v.run_off[0], m1 = v.run_off[1];
    const float rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
    const float rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    for (int64_t m = m0 + (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; m < m1; m += gstride) {
        int64_t r;
        float fp, fn;
        if (!run_head(v, m, m0, m1, r, fp, fn)) continue;
        Row<C> g, q;
        g.load(gQ + r * d, lane, d);
        q.load(Q + r * d, lane, d);
        const float w1 = reg_1 * (fp + fn), w2 = fp * rI + fn * rJ;
#pragma unroll
        for (int k = 0; k < C::NE; ++k) g.v[k] += fmaf(w2, q.v[k], w1 * sgn(q.v[k]));
        g.store(gQ + r * d, lane, d);
    }
}

// ---------------------------------------------------------------------------
// user rows: the batch is grouped by user, the group that sees the head of a
// user's run owns P[u]:  g = sum_b (cp*q_i + cn*q_j) + n*(reg_1*sign(p) + reg_2*p/|P[u]|_F)
//   SGD : P[u] -= lr*g  (in place, single writer)      GRAD: gP[u] = g
// ---------------------------------------------------------------------------
template <class C, bool SGD>
__global__ __launch_bounds__(kBlock) void k_user(float *__restrict__ P, const float *__restrict__ Q,
                                                 BatchView v, const float2 *__restrict__ coef, int d,
                                                 const double *__restrict__ stats, float lr,
                                                 float reg_1, float reg_2, float *__restrict__ gP) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const float rU = inv_or_zero(stats[DAISY_ST_NORM_U], reg_2);
    for (int64_t pos = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; pos < v.B; pos += gstride) {
        const uint32_t uu = v.ukey[pos] & v.umask;
        if (pos > 0 && (v.ukey[pos - 1] & v.umask) == uu) continue;  // not the head of this user's run
        Row<C> p, acc;
        p.load(P + (int64_t)uu * d, lane, d);
        acc.zero();
        float n = 0.f, csum = 0.f;
        for (int64_t q = pos; q < v.B && (v.ukey[q] & v.umask) == uu; ++q) {
            const float2 c = coef[q];
            csum += c.x + c.y;
            const int2 ij = v.ij[q];
            Row<C> qi, qj;
            qi.load(Q + (int64_t)ij.x * d, lane, d);
            qj.load(Q + (int64_t)(v.pointwise ? ij.x : ij.y) * d, lane, d);
#pragma unroll
            for (int k = 0; k < C::NE; ++k)
                acc.v[k] = fmaf(c.x, qi.v[k], fmaf(c.y, qj.v[k], acc.v[k]));
            n += 1.f;
        }
        const float w1 = reg_1 * n, w2 = rU * n;
#pragma unroll
        for (int k = 0; k < C::NE; ++k) {
            const float g = acc.v[k] + fmaf(w2, p.v[k], w1 * sgn(p.v[k]));
            if constexpr (SGD) p.v[k] = fmaf(-lr, g, p.v[k]);
            else p.v[k] = g;
        }
        if constexpr (SGD) p.store(P + (int64_t)uu * d, lane, d);
        else p.store(gP + (int64_t)uu * d, lane, d);
        if (v.bu && lane == 0) {                           // d loss / d u_bias[u] = sum (cp + cn)
            if constexpr (SGD) v.bu[uu] = fmaf(-lr, csum, v.bu[uu]);
            else v.g_bu[uu] = csum;
        }
    }
    if (v.bu && blockIdx.x == 0 && threadIdx.x == 0) {     // the global bias (FMRecommender.py:59)
        const float g0 = (float)stats[DAISY_ST_SUM_COEF];
        if constexpr (SGD) v.b0[0] = fmaf(-lr, g0, v.b0[0]);
        else v.g_b0[0] = g0;
    }
}

// ---------------------------------------------------------------------------
// commit the item rows: Q[r] -= lr*gQ[r]; gQ[r] = 0, one lane group per distinct
// item of the batch (head run of the plan's run list; dense != 0: every row, after an
// all-reduce of gQ).  WITH_REG: gQ holds the data term only and the regulariser
// share is added here (single-GPU SGD step: saves one pass over the touched rows).
// ---------------------------------------------------------------------------
template <class C, bool WITH_REG>
__global__ __launch_bounds__(kBlock) void k_item_apply(float *__restrict__ Q, float *__restrict__ gQ,
                                                       BatchView v, int64_t n_dense, int d, float lr,
                                                       int dense, const double *__restrict__ stats,
                                                       float reg_1, float reg_2) {
    if (halted(v.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    float rI = 0.f, rJ = 0.f;
    if constexpr (WITH_REG) {
        rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
        rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    }
    const int64_t m0 = dense ? 0 : (int64_t)v.run_off[0];
    const int64_t m1 = dense ? n_dense : (int64_t)v.run_off[1];
    for (int64_t m = m0 + (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; m < m1; m += gstride) {
        int64_t r = m;
        float fp = 0.f, fn = 0.f;
        if (!dense && !run_head(v, m, m0, m1, r, fp, fn)) continue;
        Row<C> g, q, z;
        g.load(gQ + r * d, lane, d);
        q.load(Q + r * d, lane, d);
        z.zero();
        if constexpr (WITH_REG) {
            const float w1 = reg_1 * (fp + fn), w2 = fp * rI + fn * rJ;
#pragma unroll
            for (int k = 0; k < C::NE; ++k) g.v[k] += fmaf(w2, q.v[k], w1 * sgn(q.v[k]));
        }
#pragma unroll
        for (int k = 0; k < C::NE; ++k) q.v[k] = fmaf(-lr, g.v[k], q.v[k]);
        q.store(Q + r * d, lane, d);
        z.store(gQ + r * d, lane, d);
        if (v.bi && lane == 0) {
            v.bi[r] = fmaf(-lr, v.g_bi[r], v.bi[r]);
            v.g_bi[r] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// user rows, throughput mode: the same run/slot scheme as k_item_grad_chunked over the
// user-grouped samples, so every lane group streams RUN samples (2 item rows + the user
// row each, all gathers in flight together) whatever the run lengths are.
//   in-run user:            its group owns P[u]: P[u] -= lr*(sum + n*reg(p))     in place
//   run crossing groups:    LDS slot, finished by one group after the barrier
//   run crossing chunks:    partial (sum, n) to the chunk's head/tail EDGE record; k_user_edges
//                           walks each chain from the chunk where the run starts and updates P[u]
//                           (no global atomics, and P[u] is read before anybody writes it)
// ---------------------------------------------------------------------------
template <class C>
struct UserRunCfg {
#ifndef DAISY_USER_RUN
#define DAISY_USER_RUN 8      // samples per lane group per chunk (3 rows each in flight): 4 -> 8 was +6 % on the step
#endif
    static constexpr int RUN = (C::NE <= 4 && C::LPR >= DAISY_USER_RUN) ? DAISY_USER_RUN : ((C::LPR >= 4) ? 4 : C::LPR);
    static constexpr int G = C::GROUPS_PER_BLOCK;
    static constexpr int E = G * RUN;
};

template <class C>
__device__ __forceinline__ void user_finish_row(Row<C> &p, const Row<C> &acc, float n, float lr,
                                                float reg_1, float rU) {
    const float w1 = reg_1 * n, w2 = rU * n;
#pragma unroll
    for (int k = 0; k < C::NE; ++k) {
        const float g = acc.v[k] + fmaf(w2, p.v[k], w1 * sgn(p.v[k]));
        p.v[k] = fmaf(-lr, g, p.v[k]);
    }
}

template <class C>
__global__ __launch_bounds__(kBlock) void k_user_chunked(
    float *__restrict__ P, const float *__restrict__ Q, BatchView v, const float2 *__restrict__ coef,
    int d, const double *__restrict__ stats, float lr, float reg_1, float reg_2,
    float *__restrict__ edge_vec, int32_t *__restrict__ edge_user, float *__restrict__ edge_n,
    int32_t *__restrict__ edge_whole) {
    if (halted(v.halt)) return;
    constexpr int G = UserRunCfg<C>::G, RUN = UserRunCfg<C>::RUN, E = UserRunCfg<C>::E;
    constexpr int ROWF = C::NE * C::LPR;
    // run-crossing partial sums are parked per group (<= 2: the run it continues, the run it hands on)
    // and added by the slot's finisher in group order: fixed summation order, no LDS atomics
    __shared__ float part_acc[2 * G * ROWF];
    __shared__ float part_n[2 * G], part_b[2 * G];   // part_b: FM, sum of (cp + cn) = d loss / d u_bias
    __shared__ int part_slot[2 * G];
    __shared__ int slot_user[G + 1], slot_next[G + 1];
    __shared__ int run_first[G], run_last[G];

    const int tid = threadIdx.x;
    const int lane = tid % C::LPR;
    const int group = tid / C::LPR;
    const int64_t n = v.B;
    const int64_t nchunks = (n + E - 1) / E;
    const float rU = inv_or_zero(stats[DAISY_ST_NORM_U], reg_2);

    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t c0 = chunk * E;
        const int64_t t0 = c0 + (int64_t)group * RUN;
        const int64_t t1 = (t0 + RUN < n) ? (t0 + RUN) : n;
        const int cnt = (t0 < n) ? (int)(t1 - t0) : 0;

        // ---- hop 1: metadata of the run (lane x <- sample x) and its two neighbours
        // (unconditional loads on clamped addresses: see k_item_grad_chunked)
        const int64_t last = n - 1;
        const int64_t il = (t0 + lane < n) ? (t0 + lane) : last;
        const uint32_t k_me = v.ukey[il];
        const int2 ij_me = v.ij[il];
        const float2 c_me = coef[il];
        const float2 my_c = (lane < cnt) ? c_me : make_float2(0.f, 0.f);
        const uint32_t k_prev = v.ukey[(t0 > 0) ? ((t0 - 1 < n) ? t0 - 1 : last) : 0];
        const uint32_t k_next = v.ukey[(t1 < n) ? t1 : last];
        const uint32_t k_cprev = v.ukey[(c0 > 0) ? c0 - 1 : 0];
        const int32_t my_user = (lane < cnt) ? (int32_t)(k_me & v.umask) : -1;
        const int2 my_ij = (lane < cnt) ? ij_me : make_int2(0, 0);
        const int32_t user_prev = (cnt > 0 && t0 > 0) ? (int32_t)(k_prev & v.umask) : -1;
        const int32_t user_next = (cnt > 0 && t1 < n) ? (int32_t)(k_next & v.umask) : -1;
        const int32_t chunk_prev_user = (c0 > 0) ? (int32_t)(k_cprev & v.umask) : -1;
        if (tid < 2 * G) part_slot[tid] = -1;
        if (tid <= G) { slot_user[tid] = -1; slot_next[tid] = 0; }
        const int32_t user_first = group_bcast<C>(my_user, 0);
        const int32_t user_last = __shfl(my_user, cnt > 0 ? cnt - 1 : 0, C::LPR);
        if (lane == 0) {
            run_first[group] = cnt > 0 ? user_first : -2;
            run_last[group] = cnt > 0 ? user_last : -2;
        }

        // ---- hop 2: the three rows of every sample of the run
        Row<C> qi[RUN], qj[RUN], pr[RUN];
        if (__all(cnt == RUN)) {        // wave-uniform: no branch between the 3*RUN gathers
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const int32_t ux = group_bcast<C>(my_user, x);
                const int ix = group_bcast<C>(my_ij.x, x);
                const int jx = v.pointwise ? ix : group_bcast<C>(my_ij.y, x);
                qi[x].load(Q + (int64_t)ix * d, lane, d);
                qj[x].load(Q + (int64_t)jx * d, lane, d);
                pr[x].load(P + (int64_t)ux * d, lane, d);
            }
        } else {
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const int32_t ux = group_bcast<C>(my_user, x);
                const int ix = group_bcast<C>(my_ij.x, x);
                const int jx = v.pointwise ? ix : group_bcast<C>(my_ij.y, x);
                if (x < cnt) {
                    qi[x].load(Q + (int64_t)ix * d, lane, d);
                    qj[x].load(Q + (int64_t)jx * d, lane, d);
                    pr[x].load(P + (int64_t)ux * d, lane, d);
                } else {
                    qi[x].zero(); qj[x].zero(); pr[x].zero();
                }
            }
        }
        __syncthreads();

        if (cnt > 0) {
            const bool cont = (t0 > 0) && (user_prev == user_first);
            int cur_slot = -1;
            if (cont) {
                if (group == 0) cur_slot = 0;
                else {
                    int gs = group - 1;
                    while (gs > 0 && run_first[gs] == user_first && run_last[gs - 1] == user_first) --gs;
                    const bool inherited = (gs == 0) && (run_first[0] == user_first) && (c0 > 0) &&
                                           (chunk_prev_user == user_first);
                    cur_slot = inherited ? 0 : gs + 1;
                }
            }
            int32_t cur_user = user_first;
            Row<C> pcur = pr[0];                     // P row of the current run's user
            Row<C> acc;
            acc.zero();
            float cn_ = 0.f, cb_ = 0.f;
            auto finish = [&](bool ends_here, bool to_next_chunk, const Row<C> &prow) {
                if (cur_slot < 0 && ends_here) {     // this group owns P[cur_user]
                    Row<C> pn = prow;
                    user_finish_row<C>(pn, acc, cn_, lr, reg_1, rU);
                    pn.store(P + (int64_t)cur_user * d, lane, d);
                    if (v.bu && lane == 0) v.bu[cur_user] = fmaf(-lr, cb_, v.bu[cur_user]);
                } else {
                    const int s = (cur_slot >= 0) ? cur_slot : group + 1;
                    const int q = group * 2 + ((cur_slot >= 0) ? 0 : 1);
                    float *dst = part_acc + q * ROWF;
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) dst[k * C::LPR + lane] = acc.v[k];
                    if (lane == 0) {
                        part_slot[q] = s;
                        part_n[q] = cn_;
                        part_b[q] = cb_;
                        slot_user[s] = cur_user;
                        if (to_next_chunk) slot_next[s] = 1;
                    }
                }
            };
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                if (x < cnt) {
                    const int32_t ux = group_bcast<C>(my_user, x);
                    const float cp = group_bcast<C>(my_c.x, x);
                    const float cn = group_bcast<C>(my_c.y, x);
                    if (ux != cur_user) {
                        finish(true, false, pcur);
                        cur_user = ux;
                        cur_slot = -1;
                        pcur = pr[x];
                        acc.zero();
                        cn_ = 0.f;
                        cb_ = 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < C::NE; ++k)
                        acc.v[k] = fmaf(cp, qi[x].v[k], fmaf(cn, qj[x].v[k], acc.v[k]));
                    cn_ += 1.f;
                    cb_ += cp + cn;
                }
            }
            const bool continues = (t1 < n) && (user_next == cur_user);
            finish(!continues, continues && (group == G - 1), pcur);
        }
        __syncthreads();

        // ---- one finisher per used slot; runs shared with a neighbouring chunk go to the edges
        if (tid == 0) { edge_user[2 * chunk] = -1; edge_user[2 * chunk + 1] = -1; edge_whole[chunk] = 0; }
        __syncthreads();
        for (int s = group; s <= G; s += G) {
            const int uu = slot_user[s];
            if (uu < 0) continue;
            Row<C> g;
            g.zero();
            float ns = 0.f, sb = 0.f;
            for (int q = 0; q < 2 * G; ++q) {
                if (part_slot[q] != s) continue;
                const float *src = part_acc + q * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) g.v[k] += src[k * C::LPR + lane];
                ns += part_n[q];
                sb += part_b[q];
            }
            const bool from_prev = (s == 0), to_next = slot_next[s] != 0;
            if (!from_prev && !to_next) {
                Row<C> p;
                p.load(P + (int64_t)uu * d, lane, d);
                user_finish_row<C>(p, g, ns, lr, reg_1, rU);
                p.store(P + (int64_t)uu * d, lane, d);
                if (v.bu && lane == 0) v.bu[uu] = fmaf(-lr, sb, v.bu[uu]);
            } else {
                const int64_t e = 2 * chunk + (from_prev ? 0 : 1);
                g.store(edge_vec + e * d, lane, d);
                if (lane == 0) {
                    edge_user[e] = uu;
                    edge_n[2 * e] = ns;
                    edge_n[2 * e + 1] = sb;
                    if (from_prev && to_next) edge_whole[chunk] = 1;
                }
            }
        }
        __syncthreads();
    }
    if (v.bu && blockIdx.x == 0 && tid == 0)               // the global bias (FMRecommender.py:59)
        v.b0[0] = fmaf(-lr, (float)stats[DAISY_ST_SUM_COEF], v.b0[0]);
}

// chains of edge records: the chunk whose TAIL edge starts a run owns it
template <class C>
__global__ __launch_bounds__(kBlock) void k_user_edges(float *__restrict__ P, int64_t nchunks, int d,
                                                       const double *__restrict__ stats, float lr,
                                                       float reg_1, float reg_2,
                                                       const float *__restrict__ edge_vec,
                                                       const int32_t *__restrict__ edge_user,
                                                       const float *__restrict__ edge_n,
                                                       const int32_t *__restrict__ edge_whole,
                                                       float *__restrict__ u_bias, const double *__restrict__ halt) {
    if (halted(halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const float rU = inv_or_zero(stats[DAISY_ST_NORM_U], reg_2);
    for (int64_t c = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; c < nchunks; c += gstride) {
        const int uu = edge_user[2 * c + 1];
        if (uu < 0) continue;
        Row<C> acc, t;
        acc.load(edge_vec + (2 * c + 1) * d, lane, d);
        float ns = edge_n[2 * (2 * c + 1)], sb = edge_n[2 * (2 * c + 1) + 1];
        for (int64_t k = c + 1; k < nchunks && edge_user[2 * k] == uu; ++k) {
            t.load(edge_vec + (2 * k) * d, lane, d);
#pragma unroll
            for (int q = 0; q < C::NE; ++q) acc.v[q] += t.v[q];
            ns += edge_n[2 * (2 * k)];
            sb += edge_n[2 * (2 * k) + 1];
            if (!edge_whole[k]) break;
        }
        Row<C> p;
        p.load(P + (int64_t)uu * d, lane, d);
        user_finish_row<C>(p, acc, ns, lr, reg_1, rU);
        p.store(P + (int64_t)uu * d, lane, d);
        if (u_bias && lane == 0) u_bias[uu] = fmaf(-lr, sb, u_bias[uu]);
    }
}

int launch_reduce_partials(const double *partials, int nblocks, double *stats, bool finalize, float reg_1,
                           float reg_2, double *epoch_acc, double *step_loss, hipStream_t s) {
    if (finalize)
        hipLaunchKernelGGL((k_reduce_partials<true>), dim3(1), dim3(kBlock), 0, s, partials, nblocks, stats, reg_1,
                           reg_2, epoch_acc, step_loss);
    else
        hipLaunchKernelGGL((k_reduce_partials<false>), dim3(1), dim3(kBlock), 0, s, partials, nblocks, stats, 0.f,
                           0.f, (double *)nullptr, (double *)nullptr);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace daisy

using namespace daisy;

static void view_bias(daisy_bpr_ctx *ctx) {
    BatchView &v = ctx->v;
    v.bu = ctx->bu; v.bi = ctx->bi; v.b0 = ctx->b0;
    v.g_bu = ctx->g_bu; v.g_bi = ctx->g_bi; v.g_b0 = ctx->g_b0;
}

// the context's current batch: a batch of the sorted plan layout, which every phase reads
static void adopt_sorted_batch(daisy_bpr_ctx *ctx, const BatchView &v) {
    ctx->v = v;
    ctx->sv = stream_view_of(ctx->v);
    ctx->batch_kind = 0;
    view_bias(ctx);
    ctx->cur_plan = nullptr;
    ctx->batch_set = true; ctx->fwd_done = false; ctx->n_slices = 0;
}

// a phase that reads the sorted layout, called on a batch of a partitioned plan
static int partitioned_batch_error(const char *who) {
    set_error("%s: the current batch comes from a partitioned plan (daisy_epoch_plan_build_indexed), which only "
              "daisy_bpr_sgd_step / daisy_bpr_fit_epoch_sgd with DAISY_ITEM_FUSED and the daisy_bpr_staged_* phases read", who);
    return DAISY_ERR_STATE;
}

static int launch_item_reg(daisy_bpr_ctx *ctx, const float *Q, const double *stats, float reg_1, float reg_2,
                           float *gQ, hipStream_t s) {
    const BatchView &v = ctx->v;
    return dispatch_d(ctx->d, [&](auto cfg) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((k_item_reg<C>),
                           dim3(grid_for(2 * v.B < ctx->I ? 2 * v.B : ctx->I, C::GROUPS_PER_BLOCK * 2)),
                           dim3(kBlock), 0, s, Q, v, ctx->d, stats, reg_1, reg_2, gQ);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    });
}

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

int daisy_bpr_ctx_validate_batch(const daisy_bpr_ctx *ctx, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx != nullptr, "ctx_validate_batch: NULL context");
    if (!ctx->batch_set) { set_error("ctx_validate_batch: no batch set"); return DAISY_ERR_STATE; }
    if (!ctx->own_plan || !ctx->own_plan->built || ctx->v.ukey != ctx->own_plan->ukey) return DAISY_OK;   // from an epoch plan
    return plan_report_bad(ctx->own_plan, "set_batch", as_stream(stream));
}

int daisy_bpr_ctx_create(daisy_bpr_ctx **out, int64_t max_batch, int32_t d, int64_t user_num,
                         int64_t item_num) {
    DAISY_CHECK_ARG(out != nullptr, "ctx_create: out is NULL");
    DAISY_CHECK_ARG(max_batch > 0 && max_batch < ((int64_t)1 << 30), "ctx_create: max_batch=%lld out of range",
                    (long long)max_batch);
    DAISY_CHECK_ARG(d > 0 && d <= kMaxD, "ctx_create: unsupported d=%d", d);
    DAISY_CHECK_ARG(user_num > 0 && user_num <= INT32_MAX && item_num > 0 && item_num <= INT32_MAX,
                    "ctx_create: user_num/item_num out of int32 range");
    daisy_bpr_ctx *c = new daisy_bpr_ctx();
    c->max_batch = max_batch; c->d = d; c->U = user_num; c->I = item_num;
    c->batch_set = false; c->fwd_done = false; c->own_plan = nullptr;
    c->last_item_mode = DAISY_ITEM_SORTED;
    c->pointwise = 0;
    c->bu = c->bi = c->b0 = c->g_bu = c->g_bi = c->g_b0 = nullptr;
    c->cur_plan = c->pre_plan = nullptr; c->cur_k = c->pre_k = -1; c->cur_gen = c->pre_gen = 0;
    c->pre_P = nullptr; c->pre_stats = nullptr; c->pre_n = 0; c->pre_ready = false;
    c->p_stream_mode = -1;
    DeviceArena &a = c->arena;
    a.add(&c->coef, (size_t)max_batch * 8);
    a.add(&c->partials, ((size_t)kMaxGrid * 8 + kPreBlocks) * 8);
    a.add(&c->tmp_triples, (size_t)max_batch * 12);
    // edge records: two per chunk of the user pass (B samples) or of the item pass (2B entries)
    size_t max_chunks = 0, chunks2 = 0;
    const size_t ci = (size_t)segsum_chunks(2 * max_batch, d);
    (void)dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        const size_t cu = ((size_t)max_batch + UserRunCfg<C>::E - 1) / UserRunCfg<C>::E;
        // staged passes (bpr_staged.h): the sparse flavour of the item pass has its smallest chunks, over 2 B entries, and
        // the user pass's B samples never make more chunks than that
        using Sparse = StagedItemCfg<C, kStagedItemBlock, true>;
        static_assert(Sparse::E <= StagedItemCfg<C, kStagedItemBlock>::E && Sparse::E <= 2 * StagedUserCfg<C, StagedUserBlk<C>::value>::E,
                      "the edge records are sized by the sparse item pass");
        const size_t cs = (2 * (size_t)max_batch + Sparse::E - 1) / Sparse::E;
        // the item pass's own edge records in the three-launch form (256-thread workgroups, batches up to kMergeMaxBatch)
        using Merged = StagedItemCfg<C, kBlock, true>;
        static_assert(Merged::E <= StagedItemCfg<C, kBlock>::E, "the second set is sized by the sparse flavour too");
        const size_t merge_b = (size_t)(max_batch < kMergeMaxBatch ? max_batch : kMergeMaxBatch);
        chunks2 = 2 * merge_b / Merged::E + 2;
        max_chunks = (cu > ci ? cu : ci);
        if (cs > max_chunks) max_chunks = cs;
        max_chunks += 2;
        return DAISY_OK;
    });
    const size_t n_edge = 2 * max_chunks;
    c->edge_chunks = (int64_t)max_chunks;
    a.add(&c->edge_vec, n_edge * (size_t)d * 4); a.add(&c->edge_user, n_edge * 4); a.add(&c->edge_n, n_edge * 8);
    a.add(&c->edge_whole, n_edge * 4);
    a.add(&c->edge_cnt, n_edge * 16);             // staged item pass: (n_pos, n_neg, coefficient sum, -) per edge record
    const size_t n_eb = max_chunks / kEdgeBlock + 2;      // block sums of long edge chains (k_staged_item_edge_blocks)
    a.add(&c->eb_vec, n_eb * (size_t)d * 4); a.add(&c->eb_item, n_eb * 4); a.add(&c->eb_cnt, n_eb * 16); a.add(&c->eb_through, n_eb * 4);
    const size_t n_edge2 = 2 * chunks2;
    a.add(&c->edge2_vec, n_edge2 * (size_t)d * 4); a.add(&c->edge2_item, n_edge2 * 4); a.add(&c->edge2_cnt, n_edge2 * 16);
    a.add(&c->edge2_whole, n_edge2 * 4);
    a.add(&c->slice_rng, (kMaxItemSlices + 1) * 8);
    a.add(&c->p_stage, (size_t)max_batch * (size_t)d * 4);
    a.add(&c->p_sqnorm, (size_t)user_num * 4);
    if (int rc = a.alloc("ctx_create")) {
        delete c;
        return rc;
    }
    c->eb_blocks = (int64_t)n_eb;
    c->edge2_chunks = (int64_t)chunks2;
    c->n_slices = 0;
    c->batch_kind = 0;
    c->p_sqnorm_of = nullptr;
    *out = c;
    return DAISY_OK;
}

int daisy_bpr_ctx_destroy(daisy_bpr_ctx *ctx) {
    if (!ctx) return DAISY_OK;
    int rc = DAISY_OK;
    if (ctx->own_plan) rc = plan_free(ctx->own_plan);
    const hipError_t e = ctx->arena.release() ? hipSuccess : hipGetLastError();
    delete ctx;
    if (e != hipSuccess) {
        set_error("ctx_destroy: hipFree failed: %s", hipGetErrorString(e));
        return DAISY_ERR_HIP;
    }
    return rc;
}

size_t daisy_bpr_ctx_scratch_bytes(const daisy_bpr_ctx *ctx) {
    if (!ctx) return 0;
    return ctx->arena.bytes() + (ctx->own_plan ? plan_bytes(ctx->own_plan) : 0);
}

static int ensure_own_plan(daisy_bpr_ctx *ctx) {
    if (ctx->own_plan) return DAISY_OK;
    return plan_alloc(&ctx->own_plan, ctx->max_batch, ctx->U, ctx->I);
}

int daisy_bpr_ctx_set_pointwise(daisy_bpr_ctx *ctx, int32_t pointwise) {
    DAISY_CHECK_ARG(ctx != nullptr, "ctx_set_pointwise: NULL argument");
    ctx->pointwise = pointwise ? 1 : 0;
    return DAISY_OK;
}

int daisy_bpr_ctx_set_bias(daisy_bpr_ctx *ctx, float *u_bias, float *i_bias, float *bias,
                           float *g_u_bias, float *g_i_bias, float *g_bias) {
    DAISY_CHECK_ARG(ctx != nullptr, "ctx_set_bias: NULL context");
    if (u_bias == nullptr) {                  // detach: plain MF again
        ctx->bu = ctx->bi = ctx->b0 = ctx->g_bu = ctx->g_bi = ctx->g_b0 = nullptr;
    } else {
        DAISY_CHECK_ARG(i_bias && bias && g_i_bias,
                        "ctx_set_bias: u_bias, i_bias, bias and g_i_bias must all be given");
        ctx->bu = u_bias; ctx->bi = i_bias; ctx->b0 = bias;
        ctx->g_bu = g_u_bias; ctx->g_bi = g_i_bias; ctx->g_b0 = g_bias;
    }
    if (ctx->batch_set) view_bias(ctx);
    return DAISY_OK;
}

int daisy_bpr_set_batch_from_plan(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, int64_t k,
                                  daisy_stream_t stream) {
    (void)stream;
    DAISY_CHECK_ARG(ctx && plan, "set_batch_from_plan: NULL argument");
    if (!plan->built) { set_error("set_batch_from_plan: plan has not been built"); return DAISY_ERR_STATE; }
    DAISY_CHECK_ARG(k >= 0 && k < plan->num_batches, "set_batch_from_plan: batch %lld not in 0..%lld",
                    (long long)k, (long long)plan->num_batches);
    DAISY_CHECK_ARG(plan->batch_size <= ctx->max_batch && plan->U == ctx->U && plan->I == ctx->I,
                    "set_batch_from_plan: plan (batch %lld, U %lld, I %lld) does not fit the context",
                    (long long)plan->batch_size, (long long)plan->U, (long long)plan->I);
    if (plan->kind == 1) {            // partitioned layout: only the staged step can read it
        if (daisy_epoch_plan_batch_rows(plan, k) == 0) {
            set_error("set_batch_from_plan: batch %lld holds no rows of this plan (a rank's share of the epoch: "
                      "check daisy_epoch_plan_batch_rows first)", (long long)k);
            return DAISY_ERR_STATE;
        }
        ctx->sv = plan_stream_view(plan, k);
        memset(&ctx->v, 0, sizeof(ctx->v));
        ctx->v.B = ctx->sv.B;
        ctx->batch_kind = 1;
        ctx->cur_plan = plan; ctx->cur_k = k; ctx->cur_gen = plan->build_gen;
        ctx->batch_set = true; ctx->fwd_done = false; ctx->n_slices = 0;
    } else {
        adopt_sorted_batch(ctx, plan_view(plan, k));
    }
    return DAISY_OK;
}

int daisy_bpr_set_batch_from_triples(daisy_bpr_ctx *ctx, const int32_t *triples, int64_t n_triples,
                                     const int64_t *idx, int64_t start, int64_t B, int32_t user_base,
                                     daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && triples, "set_batch_from_triples: NULL argument");
    DAISY_CHECK_ARG(B > 0 && B <= ctx->max_batch, "set_batch_from_triples: B=%lld not in 1..%lld",
                    (long long)B, (long long)ctx->max_batch);
    DAISY_CHECK_ARG(idx || (start >= 0 && start + B <= n_triples),
                    "set_batch_from_triples: rows %lld..%lld outside 0..%lld", (long long)start,
                    (long long)(start + B), (long long)n_triples);
    int rc = ensure_own_plan(ctx);
    if (rc) return rc;
    // a one-batch plan over the selected rows
    rc = plan_build(ctx->own_plan, triples, B, idx ? 0 : start, idx, idx ? DAISY_ORDER_PERM : DAISY_ORDER_IDENTITY,
                    0, 0, B, user_base, ctx->pointwise ? DAISY_PLAN_POINTWISE : 0, as_stream(stream), idx ? n_triples : -1);
    if (rc) return rc;
    adopt_sorted_batch(ctx, plan_view(ctx->own_plan, 0));
    return DAISY_OK;
}

int daisy_bpr_set_batch(daisy_bpr_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j,
                        int64_t B, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && u && i && j, "set_batch: NULL argument");
    DAISY_CHECK_ARG(B > 0 && B <= ctx->max_batch, "set_batch: B=%lld not in 1..%lld", (long long)B,
                    (long long)ctx->max_batch);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_pack_triples, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, s, u, i, j, B,
                       ctx->tmp_triples);
    DAISY_LAUNCH_CHECK();
    return daisy_bpr_set_batch_from_triples(ctx, ctx->tmp_triples, B, nullptr, 0, B, 0, stream);
}

static int forward_impl(daisy_bpr_ctx *ctx, const float *P, const float *Q, int32_t loss_type,
                        float gamma, double *stats, bool finalize, float reg_1, float reg_2,
                        double *epoch_acc, double *step_loss, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats, "forward: NULL argument");
    DAISY_CHECK_ARG(loss_type >= DAISY_LOSS_BPR && loss_type <= DAISY_LOSS_SL,
                    "Invalid loss type: %d", loss_type);
    if (!ctx->batch_set) { set_error("forward: no batch set"); return DAISY_ERR_STATE; }
    if (ctx->batch_kind != 0) return partitioned_batch_error("forward");
    DAISY_CHECK_ARG((loss_type >= DAISY_LOSS_CL) == (ctx->v.pointwise != 0),
                    "forward: loss type %d does not match the batch layout (point-wise=%d)", loss_type,
                    ctx->v.pointwise);
    hipStream_t s = as_stream(stream);
    const BatchView &v = ctx->v;
    const int d = ctx->d;
    int grid = 0;
    int rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        grid = grid_for(v.B, C::GROUPS_PER_BLOCK * FwdCfg<C>::RUN);
        if (v.pointwise)
            hipLaunchKernelGGL((k_fwd<C, true>), dim3(grid), dim3(kBlock), 0, s, P, Q, v, d, (int)loss_type,
                               gamma, ctx->coef, ctx->partials);
        else
            hipLaunchKernelGGL((k_fwd<C, false>), dim3(grid), dim3(kBlock), 0, s, P, Q, v, d, (int)loss_type,
                               gamma, ctx->coef, ctx->partials);
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    if ((rc = launch_reduce_partials(ctx->partials, grid, stats, finalize, reg_1, reg_2, epoch_acc, step_loss, s)))
        return rc;
    ctx->fwd_done = true;
    return DAISY_OK;
}

int daisy_bpr_forward(daisy_bpr_ctx *ctx, const float *P, const float *Q, int32_t loss_type,
                      float gamma, double *stats, daisy_stream_t stream) {
    return forward_impl(ctx, P, Q, loss_type, gamma, stats, false, 0.f, 0.f, nullptr, nullptr, stream);
}

int daisy_bpr_finalize(daisy_bpr_ctx *ctx, double *stats, float reg_1, float reg_2,
                       double *epoch_acc, double *step_loss, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && stats, "finalize: NULL argument");
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1), 0, as_stream(stream), stats, reg_1, reg_2, epoch_acc,
                       step_loss);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

static int item_grad_impl(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                          float reg_1, float reg_2, float *gQ, int32_t item_mode, bool data_only,
                          daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats && gQ, "item_grad: NULL argument");
    if (item_mode == DAISY_ITEM_FUSED) item_mode = DAISY_ITEM_CHUNKED;   // phase API: same item kernel
    DAISY_CHECK_ARG(item_mode >= DAISY_ITEM_ATOMIC && item_mode <= DAISY_ITEM_CHUNKED,
                    "item_grad: bad item_mode %d", item_mode);
    ctx->last_item_mode = item_mode;
    if (!ctx->fwd_done) { set_error("item_grad: forward has not run for this batch"); return DAISY_ERR_STATE; }
    hipStream_t s = as_stream(stream);
    const BatchView &v = ctx->v;
    const int d = ctx->d;
    const bool reg = (reg_1 != 0.f) || (reg_2 != 0.f);
    if (item_mode == DAISY_ITEM_CHUNKED) {
        // the user pass has not run yet: its edge records serve the item entries first
        const ItemEdges ed{ctx->edge_vec, ctx->edge_user, ctx->edge_n, ctx->edge_whole};
        if (int rc = segsum_item_grad(v, P, ctx->coef, d, gQ, ed, v.g_bi, s)) return rc;
        return (reg && !data_only) ? launch_item_reg(ctx, Q, stats, reg_1, reg_2, gQ, s) : DAISY_OK;
    }
    return dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        if (item_mode == DAISY_ITEM_SORTED)
            hipLaunchKernelGGL((k_item_grad_sorted<C>),
                               dim3(grid_for(2 * v.B, C::GROUPS_PER_BLOCK, kMaxGridSparse)), dim3(kBlock), 0,
                               s, P, Q, ctx->coef, v, d, stats, reg_1, reg_2, gQ);
        else if (reg)
            hipLaunchKernelGGL((k_item_grad_atomic<C, true>), dim3(grid_for(v.B, C::GROUPS_PER_BLOCK * 4)),
                               dim3(kBlock), 0, s, P, Q, v, ctx->coef, d, stats, reg_1, reg_2, gQ);
        else
            hipLaunchKernelGGL((k_item_grad_atomic<C, false>), dim3(grid_for(v.B, C::GROUPS_PER_BLOCK * 4)),
                               dim3(kBlock), 0, s, P, Q, v, ctx->coef, d, stats, reg_1, reg_2, gQ);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    });
}

int daisy_bpr_item_grad(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                        float reg_1, float reg_2, float *gQ, int32_t item_mode,
                        daisy_stream_t stream) {
    return item_grad_impl(ctx, P, Q, stats, reg_1, reg_2, gQ, item_mode, false, stream);
}

int daisy_bpr_item_grad_data(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                             float *gQ, int32_t item_mode, daisy_stream_t stream) {
    if (item_mode == DAISY_ITEM_FUSED) item_mode = DAISY_ITEM_CHUNKED;
    DAISY_CHECK_ARG(item_mode == DAISY_ITEM_CHUNKED,
                    "item_grad_data: only the chunked mode splits data term and regulariser (mode %d)", item_mode);
    return item_grad_impl(ctx, P, Q, stats, 0.f, 0.f, gQ, item_mode, true, stream);
}

int daisy_bpr_item_grad_reg(daisy_bpr_ctx *ctx, const float *Q, const double *stats, float reg_1,
                            float reg_2, float *gQ, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && Q && stats && gQ, "item_grad_reg: NULL argument");
    if (!ctx->batch_set) { set_error("item_grad_reg: no batch set"); return DAISY_ERR_STATE; }
    if (ctx->batch_kind != 0) return partitioned_batch_error("item_grad_reg");
    if (reg_1 == 0.f && reg_2 == 0.f) return DAISY_OK;
    return launch_item_reg(ctx, Q, stats, reg_1, reg_2, gQ, as_stream(stream));
}

static int user_pass(daisy_bpr_ctx *ctx, float *P, const float *Q, const double *stats, float lr,
                     float reg_1, float reg_2, float *gP, bool sgd, daisy_stream_t stream,
                     bool chunked = false) {
    ctx->p_sqnorm_of = nullptr;   // P rows change behind the row-norm cache of the staged step
    ctx->pre_ready = false;       // (and behind a pre-norm the staged step computed ahead)
    if (!ctx->fwd_done) { set_error("user update: forward has not run for this batch"); return DAISY_ERR_STATE; }
    hipStream_t s = as_stream(stream);
    const BatchView &v = ctx->v;
    const int d = ctx->d;
    return dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        const int grid = grid_for(v.B, C::GROUPS_PER_BLOCK * 2);
        if (sgd && chunked && C::NE <= 4) {
            const int64_t nchunks = (v.B + UserRunCfg<C>::E - 1) / UserRunCfg<C>::E;
            hipLaunchKernelGGL((k_user_chunked<C>), dim3(grid_for(nchunks, 1, 16384)), dim3(kBlock), 0,
                               s, P, Q, v, ctx->coef, d, stats, lr, reg_1, reg_2, ctx->edge_vec,
                               ctx->edge_user, ctx->edge_n, ctx->edge_whole);
            hipLaunchKernelGGL((k_user_edges<C>), dim3(grid_for(nchunks, C::GROUPS_PER_BLOCK)),
                               dim3(kBlock), 0, s, P, nchunks, d, stats, lr, reg_1, reg_2, ctx->edge_vec,
                               ctx->edge_user, ctx->edge_n, ctx->edge_whole, v.bu, v.halt);
        } else if (sgd)
            hipLaunchKernelGGL((k_user<C, true>), dim3(grid), dim3(kBlock), 0, s, P, Q, v, ctx->coef, d,
                               stats, lr, reg_1, reg_2, gP);
        else {
            if (v.bu && !(v.g_bu && v.g_b0)) {
                set_error("user_grad: the context has biases but no g_u_bias / g_bias outputs");
                return DAISY_ERR_ARG;
            }
            hipLaunchKernelGGL((k_user<C, false>), dim3(grid), dim3(kBlock), 0, s, P, Q, v, ctx->coef, d,
                               stats, lr, reg_1, reg_2, gP);
        }
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    });
}

int daisy_bpr_user_sgd(daisy_bpr_ctx *ctx, float *P, const float *Q, const double *stats, float lr,
                       float reg_1, float reg_2, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats, "user_sgd: NULL argument");
    // throughput kernel when the step's item gradient was formed in throughput mode,
    // the reproducible run-owner kernel otherwise
    return user_pass(ctx, P, Q, stats, lr, reg_1, reg_2, nullptr, true, stream,
                     ctx->last_item_mode == DAISY_ITEM_CHUNKED);
}

int daisy_bpr_user_grad(daisy_bpr_ctx *ctx, const float *P, const float *Q, const double *stats,
                        float reg_1, float reg_2, float *gP, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats && gP, "user_grad: NULL argument");
    return user_pass(ctx, const_cast<float *>(P), Q, stats, 0.f, reg_1, reg_2, gP, false, stream);
}

static int item_apply_impl(daisy_bpr_ctx *ctx, float *Q, float *gQ, float lr, int32_t dense,
                           const double *stats, float reg_1, float reg_2, bool with_reg,
                           daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && Q && gQ, "item_sgd_apply: NULL argument");
    if (!dense && !ctx->batch_set) { set_error("item_sgd_apply: no batch set"); return DAISY_ERR_STATE; }
    if (!dense && ctx->batch_kind != 0) return partitioned_batch_error("item_sgd_apply with dense == 0");
    hipStream_t s = as_stream(stream);
    const int d = ctx->d;
    const BatchView &v = ctx->v;
    const int64_t n = dense ? ctx->I : (2 * v.B < ctx->I ? 2 * v.B : ctx->I);   // upper bound of rows
    return dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        const int grid = grid_for(n, C::GROUPS_PER_BLOCK * 2);
        if (with_reg)
            hipLaunchKernelGGL((k_item_apply<C, true>), dim3(grid), dim3(kBlock), 0, s, Q, gQ, v, ctx->I, d,
                               lr, (int)dense, stats, reg_1, reg_2);
        else
            hipLaunchKernelGGL((k_item_apply<C, false>), dim3(grid), dim3(kBlock), 0, s, Q, gQ, v, ctx->I, d,
                               lr, (int)dense, stats, reg_1, reg_2);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    });
}

int daisy_bpr_item_sgd_apply(daisy_bpr_ctx *ctx, float *Q, float *gQ, float lr, int32_t dense,
                             daisy_stream_t stream) {
    return item_apply_impl(ctx, Q, gQ, lr, dense, nullptr, 0.f, 0.f, false, stream);
}

int daisy_bpr_sgd_step(daisy_bpr_ctx *ctx, float *P, float *Q, int32_t loss_type, float gamma,
                       float lr, float reg_1, float reg_2, float *gQ, double *stats,
                       double *epoch_acc, double *step_loss, int32_t item_mode,
                       daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && P && Q && stats, "sgd_step: NULL argument");
    if (!ctx->batch_set) { set_error("sgd_step: no batch set"); return DAISY_ERR_STATE; }
    // with an epoch accumulator the step belongs to an epoch loop: it does nothing once a step of the epoch has had a
    // non-finite loss (AbstractRecommender.py:122-123 raises before that step's backward; here the phase kernels stop
    // exactly there, the staged step has already moved the user rows of the offending step when its loss is known)
    struct HaltScope {
        daisy_bpr_ctx *c;
        HaltScope(daisy_bpr_ctx *c_, const double *h) : c(c_) { c->v.halt = h; c->sv.halt = h; }
        ~HaltScope() { c->v.halt = nullptr; c->sv.halt = nullptr; }
    } halt_scope(ctx, epoch_acc ? epoch_acc + 1 : nullptr);
    if (item_mode == DAISY_ITEM_FUSED) {
        // the staged step (bpr_staged.hip): pairwise losses without FM biases; anything else runs the phase kernels
        if (staged_supported(ctx, loss_type))
            return staged_sgd_step(ctx, P, Q, loss_type, gamma, lr, reg_1, reg_2, stats, epoch_acc, step_loss,
                                   as_stream(stream));
        item_mode = DAISY_ITEM_CHUNKED;
    }
    DAISY_CHECK_ARG(gQ != nullptr, "sgd_step: gQ is NULL");
    int rc;
    if ((rc = forward_impl(ctx, P, Q, loss_type, gamma, stats, true, reg_1, reg_2, epoch_acc, step_loss,
                           stream))) return rc;
    // throughput mode: gQ carries the data term only, the commit kernel adds the regulariser
    const bool fold_reg = (item_mode == DAISY_ITEM_CHUNKED) && (reg_1 != 0.f || reg_2 != 0.f);
    if ((rc = item_grad_impl(ctx, P, Q, stats, reg_1, reg_2, gQ, item_mode, fold_reg, stream))) return rc;
    if ((rc = user_pass(ctx, P, Q, stats, lr, reg_1, reg_2, nullptr, true, stream,
                        item_mode == DAISY_ITEM_CHUNKED))) return rc;
    if ((rc = item_apply_impl(ctx, Q, gQ, lr, 0, stats, reg_1, reg_2, fold_reg, stream))) return rc;
    return DAISY_OK;
}

int daisy_bpr_fit_epoch_sgd(daisy_bpr_ctx *ctx, const daisy_epoch_plan *plan, float *P, float *Q,
                            int32_t loss_type, float gamma, float lr, float reg_1, float reg_2,
                            float *gQ, double *stats, double *epoch_acc, double *step_losses,
                            int32_t item_mode, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && plan && P && Q && stats, "fit_epoch: NULL argument");
    if (!plan->built) { set_error("fit_epoch: plan has not been built"); return DAISY_ERR_STATE; }
    DAISY_CHECK_ARG(loss_type >= DAISY_LOSS_BPR && loss_type <= DAISY_LOSS_SL, "Invalid loss type: %d", loss_type);
    // batches of a few hundred samples (the reference's default 256): all steps of the epoch inside one
    // persistent workgroup - the step is bound by kernel-boundary latency there, not by bandwidth
    if ((item_mode == DAISY_ITEM_CHUNKED || item_mode == DAISY_ITEM_FUSED) && small_epoch_supported(ctx, plan, loss_type)) {
        DAISY_CHECK_ARG(plan->U == ctx->U && plan->I == ctx->I, "fit_epoch: plan does not fit the context");
        return small_fit_epoch(ctx, plan, P, Q, loss_type, gamma, lr, reg_1, reg_2, stats, epoch_acc, step_losses,
                               as_stream(stream));
    }
    for (int64_t k = 0; k < plan->num_batches; ++k) {
        int rc = daisy_bpr_set_batch_from_plan(ctx, plan, k, stream);
        if (rc) return rc;
        rc = daisy_bpr_sgd_step(ctx, P, Q, loss_type, gamma, lr, reg_1, reg_2, gQ, stats, epoch_acc,
                                step_losses ? step_losses + k : nullptr, item_mode, stream);
        if (rc) return rc;
    }
    return DAISY_OK;
}

int daisy_bpr_fit_epoch_sgd_many(const daisy_small_trial *trials, int32_t count, void *workspace, size_t workspace_bytes,
                                 daisy_stream_t stream) {
    DAISY_CHECK_ARG(count >= 0, "fit_epoch_sgd_many: count=%d", count);
    if (count == 0) return DAISY_OK;
    DAISY_CHECK_ARG(trials != nullptr, "fit_epoch_sgd_many: trials is NULL");
    return small_fit_epoch_many(trials, count, workspace, workspace_bytes, as_stream(stream));
}

}  // extern "C"
