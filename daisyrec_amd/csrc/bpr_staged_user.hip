// The staged step's user side (see bpr_staged.hip for the step and bpr_staged.h for what is shared with the item pass):
// the row-norm cache and the pre-norm kernels, k_staged_user, the user pass's edge chains, and their launchers.
#include "bpr_staged.h"

namespace daisy {

template <class C>
__global__ __launch_bounds__(kBlock) void k_row_sqnorm(const float *__restrict__ W, int64_t rows, int d,
                                                       float *__restrict__ out) {
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    for (int64_t r = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; r < rows; r += gstride) {
        Row<C> w;
        w.load(W + r * d, lane, d);
        const float s = row_dot<C>(w, w);
        if (lane == 0) out[r] = s;
    }
}

// partials[block] = sum over the block's samples of |P[u_s]|^2 (from the cache)
__global__ __launch_bounds__(kBlock) void k_unorm(const float *__restrict__ p_sqnorm, StreamView v,
                                                  double *__restrict__ partials) {
    double acc = 0.0;
    for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < v.B;
         s += (int64_t)gridDim.x * blockDim.x)
        acc += (double)p_sqnorm[sv_user(v, s)];
    __shared__ double sm[kBlock / kWave];
    const double w = wave_sum_f64(acc);
    if ((threadIdx.x % kWave) == 0) sm[threadIdx.x / kWave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < kBlock / kWave; ++k) t += sm[k];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void k_unorm_reduce(const double *__restrict__ partials, int nblocks,
                                                         double *__restrict__ stats) {
    __shared__ double sm[kBlock];
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) t += partials[b];
    sm[threadIdx.x] = t;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) stats[DAISY_ST_SQ_U_PRE] = sm[0];
}

// Forward + user update in one pass over the user-grouped samples (see the header comment).
//   in-run user:          its group owns P[u]: regulariser + optimiser step in place
//   run crossing groups:  partial sums parked in LDS, added by the slot's finisher in group order
//   run crossing chunks:  edge records, chained by k_staged_user_edges in chunk order
// (no atomics, fixed summation order: bitwise reproducible).
// HAS_POS: the stage slot of a sample comes from the plan (partitioned layout) instead of its position.
template <class C, int BLK, int MODE, bool HAS_POS, bool ADAM>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu((C::NE <= 4 && !ADAM) ? 4 : 2, 8))) void k_staged_user(
    float *__restrict__ P, const float *__restrict__ Q, StreamView v, int d, const double *__restrict__ stats,
    RowOpt opt, float reg_1, float reg_2, int loss_type, float gamma, float *__restrict__ stage,
    float2 *__restrict__ coef, float *__restrict__ p_sqnorm, double *__restrict__ partials, UserEdges ed,
    PreNorm pre, StagedBias fm) {
    // an earlier step of this epoch had a non-finite loss: the epoch has stopped.  The word is requested here and looked
    // at behind the first chunk's gathers (before anything is stored): a launch-bound step - a few thousand samples -
    // is a chain of dependent trips to memory, and this one now travels with the metadata instead of in front of it
    const double halt_word = v.halt ? *v.halt : 0.0;
    constexpr int G = StagedUserCfg<C, BLK>::G, RUN = StagedUserCfg<C, BLK>::RUN, E = StagedUserCfg<C, BLK>::E;
    constexpr int ROWF = C::NE * C::LPR;
    constexpr bool PAIR = MODE != kModePoint;
    constexpr bool BIAS = MODE != kModePremul;          // FM biases ride on the plain / point flavours only
    __shared__ float part_acc[2 * G * ROWF];
    __shared__ float part_n[2 * G], part_b[2 * G];
    __shared__ int part_slot[2 * G];
    // the pre-step row of P of a run that leaves its group through the TAIL: the slot's finisher commits from it.  (Until
    // round 5 the finisher loaded the row again - a dependent trip to memory behind this chunk's row and stage STORES, which
    // the vector-memory counter also counts: s_waitcnt vmcnt(0) in front of the commit waited for all of them.)
    __shared__ float part_p[G * ROWF];
    __shared__ float part_m[ADAM ? G * ROWF : 4], part_v[ADAM ? G * ROWF : 4];      // ... and (Adam) its moments
    __shared__ int slot_user[G + 1], slot_next[G + 1];
    __shared__ int run_first[G], run_last[G];

    const int tid = threadIdx.x;
    const int lane = tid % C::LPR;
    const int group = tid / C::LPR;
    const int64_t n = v.B;
    const int64_t nchunks = (n + E - 1) / E;
    const float rU = inv_or_zero(sqrt(prenorm_sum(stats, pre)), reg_2);
    const bool has_bias = BIAS && fm.bu != nullptr;
    const float b0 = has_bias ? fm.b0[0] : 0.f;
    float acc7[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t c0 = chunk * E;
        const int64_t t0 = c0 + (int64_t)group * RUN;
        const int64_t t1 = (t0 + RUN < n) ? (t0 + RUN) : n;
        const int cnt = (t0 < n) ? (int)(t1 - t0) : 0;

        // ---- hop 1: metadata of the run (lane x <- sample x) and its neighbours; every load is
        // unconditional on a clamped address (a branch around a load drains vmcnt first)
        const int64_t last = n - 1;
        const int64_t il = (t0 + lane < n) ? (t0 + lane) : last;
        const int64_t i_prev = (t0 > 0) ? ((t0 - 1 < n) ? t0 - 1 : last) : 0, i_next = (t1 < n) ? t1 : last;
        const int64_t i_cprev = (c0 > 0) ? c0 - 1 : 0;
        uint32_t k_me, slot_me, k_prev, k_next, k_cprev;
        int2 ij_me;
        if constexpr (HAS_POS) {            // partitioned plan: one 16-byte record per sample
            const uint4 rec = v.s_rec[il];
            k_me = rec.x; ij_me = make_int2((int)rec.y, (int)rec.z); slot_me = rec.w - v.pos_base;
            k_prev = v.s_rec[i_prev].x; k_next = v.s_rec[i_next].x; k_cprev = v.s_rec[i_cprev].x;
        } else {
            k_me = v.s_user[il] & v.umask; ij_me = v.s_ij[il]; slot_me = (uint32_t)il;
            k_prev = v.s_user[i_prev] & v.umask; k_next = v.s_user[i_next] & v.umask; k_cprev = v.s_user[i_cprev] & v.umask;
        }
        const int32_t my_user = (lane < cnt) ? (int32_t)k_me : -1;
        const int2 my_ij = (lane < cnt) ? ij_me : make_int2(0, 0);
        const int32_t user_prev = (cnt > 0 && t0 > 0) ? (int32_t)k_prev : -1;
        const int32_t user_next = (cnt > 0 && t1 < n) ? (int32_t)k_next : -1;
        const int32_t chunk_prev_user = (c0 > 0) ? (int32_t)k_cprev : -1;
        if (tid < 2 * G) part_slot[tid] = -1;
        if (tid <= G) { slot_user[tid] = -1; slot_next[tid] = 0; }
        const int32_t user_first = group_bcast<C>(my_user, 0);
        const int32_t user_last = __shfl(my_user, cnt > 0 ? cnt - 1 : 0, C::LPR);
        if (lane == 0) {
            run_first[group] = cnt > 0 ? user_first : -2;
            run_last[group] = cnt > 0 ? user_last : -2;
        }
        // FM: the biases of lane x's own sample (scalar gathers: the tables are small next to the factor rows)
        float my_bsp = 0.f, my_bsn = 0.f;
        if constexpr (BIAS) {
            if (has_bias && lane < cnt) {
                const float bu = fm.bu[k_me];
                my_bsp = (bu + fm.bi[ij_me.x]) + b0;                 // FMRecommender.py:66
                if constexpr (PAIR) my_bsn = (bu + fm.bi[ij_me.y]) + b0;
            }
        }

        // ---- hop 2: the rows of every sample of the run
        Row<C> qi[RUN], qj[PAIR ? RUN : 1], pr[RUN];
        // Adam: the moments of every sample's user row travel with the row (round 5): the run's owner then commits from
        // registers.  (Round 4 had measured exactly this as "no change" - with its first use still behind a vmcnt(0) wait
        // for the run's stage stores; see the touch below.)
        Row<C> pm[ADAM ? RUN : 1], pv[ADAM ? RUN : 1];
        auto moments = [&](int x, int64_t urow) {
            if constexpr (ADAM) {
                pm[x].load(opt.m + urow * d, lane, d);
                pv[x].load(opt.v + urow * d, lane, d);
            }
        };
        if (__all(cnt == RUN) && v.p_stream) {     // (wave-uniform: no branch between the gathers)
            // a user table far beyond the Infinity Cache: its rows come back once every few steps, so they are read and
            // written past the caches and leave them to Q (10 M x 1 M shapes: 449 -> 420 us per pass with BOTH the loads
            // and the owner's store nontemporal - either alone measured no gain; at 1 M users, where most rows return in
            // the next step, 3 % slower: the host decides)
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                qi[x].load(Q + (int64_t)group_bcast<C>(my_ij.x, x) * d, lane, d);
                if constexpr (PAIR) qj[x].load(Q + (int64_t)group_bcast<C>(my_ij.y, x) * d, lane, d);
                pr[x].load_nt(P + (int64_t)group_bcast<C>(my_user, x) * d, lane, d);
                moments(x, (int64_t)group_bcast<C>(my_user, x));
            }
        } else if (__all(cnt == RUN)) {
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                qi[x].load(Q + (int64_t)group_bcast<C>(my_ij.x, x) * d, lane, d);
                if constexpr (PAIR) qj[x].load(Q + (int64_t)group_bcast<C>(my_ij.y, x) * d, lane, d);
                pr[x].load(P + (int64_t)group_bcast<C>(my_user, x) * d, lane, d);
                moments(x, (int64_t)group_bcast<C>(my_user, x));
            }
        } else {
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const int32_t ux = group_bcast<C>(my_user, x);
                const int ix = group_bcast<C>(my_ij.x, x);
                const int jx = group_bcast<C>(my_ij.y, x);
                if (x < cnt) {
                    qi[x].load(Q + (int64_t)ix * d, lane, d);
                    if constexpr (PAIR) qj[x].load(Q + (int64_t)jx * d, lane, d);
                    pr[x].load(P + (int64_t)ux * d, lane, d);
                    moments(x, (int64_t)ux);
                } else {
                    qi[x].zero(); pr[x].zero();
                    if constexpr (PAIR) qj[x].zero();
                    if constexpr (ADAM) { pm[x].zero(); pv[x].zero(); }
                }
            }
        }
        if (halt_word > 0.0) return;           // (uniform over the grid; nothing has been written yet)
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
            // ---- forward: scores of the run's samples -> lane x; one loss epilogue per run, a sample per lane
            float my_sp = 0.f, my_sn = 0.f;
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                if (x < cnt) {
                    const float sp = row_dot<C>(pr[x], qi[x]);
                    float sn = 0.f;
                    if constexpr (PAIR) sn = row_dot<C>(pr[x], qj[x]);
                    if (lane == x) { my_sp = sp; my_sn = sn; }
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) {
                        acc7[1] += fabsf(pr[x].v[k]);
                        acc7[2] += fabsf(qi[x].v[k]);
                        acc7[4] = fmaf(pr[x].v[k], pr[x].v[k], acc7[4]);
                        acc7[5] = fmaf(qi[x].v[k], qi[x].v[k], acc7[5]);
                        if constexpr (PAIR) {
                            acc7[3] += fabsf(qj[x].v[k]);
                            acc7[6] = fmaf(qj[x].v[k], qj[x].v[k], acc7[6]);
                        }
                    }
                }
            }
            float2 my_c = make_float2(0.f, 0.f);
            if (lane < cnt) {
                float term;
                if constexpr (BIAS) { my_sp += my_bsp; my_sn += my_bsn; }
                if constexpr (!PAIR) my_sn = (float)my_ij.y;               // the label (sampler.py:93-98)
                pair_coef(loss_type, my_sp, my_sn, gamma, term, my_c.x, my_c.y);
                acc7[0] += term;
                if constexpr (BIAS) acc7[7] += my_c.x + my_c.y;            // dL/d bias_ (FM)
                if (MODE == kModePlain || (MODE == kModePoint && has_bias)) coef[slot_me] = my_c;
            }

            // ---- user gradient over the runs of equal users; the staged rows leave on the way
            int32_t cur_user = user_first;
            Row<C> pcur = pr[0];                     // pre-step P row of the current run's user
            Row<C> mcur, vcur;                       // (Adam) and its moments
            if constexpr (ADAM) {
                mcur = pm[0]; vcur = pv[0];
                // the moment registers are "used" here, in front of the first store of this chunk: the compiler's wait
                // for their gathers happens now, and the commits below wait for nothing
#pragma unroll
                for (int x = 0; x < RUN; ++x)
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) { asm volatile("" : "+v"(pm[x].v[k])); asm volatile("" : "+v"(pv[x].v[k])); }
            }
            Row<C> acc;
            acc.zero();
            float cn_ = 0.f, sb_ = 0.f;
            auto finish = [&](bool ends_here, bool to_next_chunk, const Row<C> &prow) {
                if (cur_slot < 0 && ends_here) {     // this group owns P[cur_user]
                    Row<C> pn = prow;
                    user_commit<C, ADAM>(P, p_sqnorm, cur_user, pn, acc, cn_, reg_1, rU, opt, lane, d, v.p_stream != 0,
                                         ADAM ? &mcur : nullptr, ADAM ? &vcur : nullptr);
                    if constexpr (BIAS) user_bias_commit(fm, cur_user, sb_, opt.lr, lane);
                } else {
                    const int s = (cur_slot >= 0) ? cur_slot : group + 1;
                    const int q = group * 2 + ((cur_slot >= 0) ? 0 : 1);
                    float *dst = part_acc + q * ROWF;
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) dst[k * C::LPR + lane] = acc.v[k];
                    if (cur_slot < 0) {              // the run began here: its pre-step row for slot group + 1's finisher
                        float *pd = part_p + group * ROWF;
#pragma unroll
                        for (int k = 0; k < C::NE; ++k) pd[k * C::LPR + lane] = prow.v[k];
                        if constexpr (ADAM) {
                            float *md = part_m + group * ROWF, *vd = part_v + group * ROWF;
#pragma unroll
                            for (int k = 0; k < C::NE; ++k) { md[k * C::LPR + lane] = mcur.v[k]; vd[k * C::LPR + lane] = vcur.v[k]; }
                        }
                    }
                    if (lane == 0) {
                        part_slot[q] = s;
                        part_n[q] = cn_;
                        part_b[q] = sb_;
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
                    const uint32_t sl = group_bcast<C>(slot_me, x);
                    if (ux != cur_user) {
                        finish(true, false, pcur);
                        cur_user = ux;
                        cur_slot = -1;
                        pcur = pr[x];
                        if constexpr (ADAM) { mcur = pm[x]; vcur = pv[x]; }
                        acc.zero();
                        cn_ = 0.f; sb_ = 0.f;
                    }
                    // stage rows: written once here, read by the item pass of the same step and never again - the
                    // stores are nontemporal so that they do not evict the factor tables from L2 / the Infinity Cache
                    // (-2.5 % per step at both BASELINE shapes; nontemporal LOADS of the stage measured neutral to
                    // slightly worse: the item pass loads them plainly)
                    if constexpr (MODE != kModePlain) {
                        Row<C> m;
#pragma unroll
                        for (int k = 0; k < C::NE; ++k) m.v[k] = cp * pr[x].v[k];
                        m.store_nt(stage + (int64_t)sl * d, lane, d);
                    } else {
                        pr[x].store_nt(stage + (int64_t)sl * d, lane, d);
                    }
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) {
                        if constexpr (PAIR) acc.v[k] = fmaf(cp, qi[x].v[k], fmaf(cn, qj[x].v[k], acc.v[k]));
                        else acc.v[k] = fmaf(cp, qi[x].v[k], acc.v[k]);
                    }
                    cn_ += 1.f;
                    if constexpr (BIAS) sb_ += cp + cn;
                }
            }
            const bool continues = (t1 < n) && (user_next == cur_user);
            finish(!continues, continues && (group == G - 1), pcur);
        }
        __syncthreads();

        // ---- one finisher per used slot; runs shared with a neighbouring chunk go to the edges
        if (tid == 0) { ed.user[2 * chunk] = -1; ed.user[2 * chunk + 1] = -1; ed.whole[chunk] = 0; }
        __syncthreads();
        for (int s = group; s <= G; s += G) {
            const int uu = slot_user[s];
            if (uu < 0) continue;
            Row<C> g;
            g.zero();
            float ns = 0.f, sb = 0.f;
            auto add_part = [&](int q) {
                const float *src = part_acc + q * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) g.v[k] += src[k * C::LPR + lane];
                ns += part_n[q];
                sb += part_b[q];
            };
            // slot s in group order: the tail of group s - 1 (where the run began), then the heads of the groups s, s + 1,
            // ... it runs through (see k_staged_item: the same chain instead of a scan over all 2 G parked sums)
            if (s > 0 && part_slot[2 * s - 1] == s) add_part(2 * s - 1);
            for (int q = 2 * s; q < 2 * G && part_slot[q] == s; q += 2) add_part(q);
            const bool from_prev = (s == 0), to_next = slot_next[s] != 0;
            if (!from_prev && !to_next) {
                Row<C> p;                            // (s >= 1: the tail of group s - 1 parked the row)
                const float *ps = part_p + (s - 1) * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) p.v[k] = ps[k * C::LPR + lane];
                Row<C> mrow, vrow;
                if constexpr (ADAM) {
                    const float *ms = part_m + (s - 1) * ROWF, *vs = part_v + (s - 1) * ROWF;
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) { mrow.v[k] = ms[k * C::LPR + lane]; vrow.v[k] = vs[k * C::LPR + lane]; }
                }
                user_commit<C, ADAM>(P, p_sqnorm, uu, p, g, ns, reg_1, rU, opt, lane, d, false, ADAM ? &mrow : nullptr,
                                     ADAM ? &vrow : nullptr);
                if constexpr (BIAS) user_bias_commit(fm, uu, sb, opt.lr, lane);
            } else {
                const int64_t e = 2 * chunk + (from_prev ? 0 : 1);
                g.store(ed.vec + e * d, lane, d);
                if (lane == 0) {
                    ed.user[e] = uu;
                    ed.n[2 * e] = ns;
                    ed.n[2 * e + 1] = sb;
                    if (from_prev && to_next) ed.whole[chunk] = 1;
                }
            }
        }
        __syncthreads();
    }
    __shared__ double sm7[BLK / kWave][8];
    const int wave = tid / kWave;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double w = (double)wave_sum_f32_dpp(acc7[k]);     // fp32 inside the wave, fp64 across waves and workgroups
        if ((tid % kWave) == 0) sm7[wave][k] = w;
    }
    __syncthreads();
    if (tid < 8) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < BLK / kWave; ++w) t += sm7[w][tid];
        partials[(int64_t)blockIdx.x * 8 + tid] = t;           // [7]: sum of dL/dpos + dL/dneg (FM's bias_; 0 without biases)
    }
}

template <class C, bool ADAM>
__global__ __launch_bounds__(kBlock) void k_staged_user_edges(float *__restrict__ P, int64_t nchunks, int d,
                                                              const double *__restrict__ stats, RowOpt opt,
                                                              float reg_1, float reg_2, UserEdges ed,
                                                              float *__restrict__ p_sqnorm, PreNorm pre,
                                                              ReduceJob red, const double *__restrict__ halt,
                                                              StagedBias fm) {
    if (halted(halt)) return;              // (the riding reduction too: the epoch's sums stay at the offending step)
    user_edges_block<C, ADAM>(blockIdx.x, gridDim.x, P, nchunks, d, stats, opt, reg_1, reg_2, ed, p_sqnorm, pre, red, fm);
}

// ---- launchers: what the path says, nothing else
int staged_norm_cache(daisy_bpr_ctx *ctx, const float *P, hipStream_t s) {
    if (ctx->p_sqnorm_of == P) return DAISY_OK;
    return dispatch_d(ctx->d, [&](auto cfg) {          // one dense pass over P
        using C = decltype(cfg);
        hipLaunchKernelGGL((k_row_sqnorm<C>), dim3(grid_for(ctx->U, C::GROUPS_PER_BLOCK * 4)), dim3(kBlock), 0, s,
                           P, ctx->U, ctx->d, ctx->p_sqnorm);
        ctx->p_sqnorm_of = P;
        return DAISY_OK;
    });
}

int staged_prenorm(daisy_bpr_ctx *ctx, const float *P, double *stats, int gn, bool fold, hipStream_t s) {
    if (int rc = staged_norm_cache(ctx, P, s)) return rc;
    double *pre = fold ? ctx->partials + (size_t)kMaxGrid * 8 : ctx->partials;   // fold: behind the user pass's own sums
    hipLaunchKernelGGL(k_unorm, dim3(gn), dim3(kBlock), 0, s, ctx->p_sqnorm, ctx->sv, pre);
    if (!fold) hipLaunchKernelGGL(k_unorm_reduce, dim3(1), dim3(kBlock), 0, s, pre, gn, stats);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// the user pass and - unless the item launch carries them (path.merge) - its edge chains, with the reduction of the
// pass's sums as one more workgroup when the whole step runs in one call (path.fused)
int staged_user(daisy_bpr_ctx *ctx, const StagedPath &path, const StagedStep &st, float *P, const float *Q) {
    ctx->pre_ready = false;                // (P is about to change: a pre-norm computed ahead of this pass is stale)
    StreamView v = ctx->sv;
    v.p_stream = path.p_stream;
    const int d = ctx->d;
    const UserEdges ed = staged_user_edges(ctx);
    const PreNorm pre = staged_pre(ctx, path);
    const ReduceJob red = staged_reduce(ctx, path, st);
    const RowOpt opt = row_opt(st.lr, st.adam, true);
    const StagedBias fm = staged_bias(ctx, st.bias_grad_out);
    int rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        constexpr int BLK = StagedUserBlk<C>::value;
        with_mode(path.mode, [&](auto mode_tag) { with_flag(path.has_pos, [&](auto hp_tag) { with_flag(path.adam, [&](auto adam_tag) {
            hipLaunchKernelGGL((k_staged_user<C, BLK, decltype(mode_tag)::value, decltype(hp_tag)::value, decltype(adam_tag)::value>),
                               dim3(path.gu), dim3(BLK), 0, st.s, P, Q, v, d, st.stats, opt, st.reg_1, st.reg_2, st.loss_type,
                               st.gamma, ctx->p_stage, ctx->coef, ctx->p_sqnorm, ctx->partials, ed, pre, fm);
        }); }); });
        if (!path.merge) with_flag(path.adam, [&](auto adam_tag) {
            hipLaunchKernelGGL((k_staged_user_edges<C, decltype(adam_tag)::value>), dim3(path.n_ue + (path.fused ? 1 : 0)),
                               dim3(kBlock), 0, st.s, P, path.u_chunks, d, st.stats, opt, st.reg_1, st.reg_2, ed, ctx->p_sqnorm,
                               pre, red, v.halt, fm);
        });
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace daisy
