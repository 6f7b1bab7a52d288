// The staged step's item side (see bpr_staged.hip for the step and bpr_staged.h for what is shared with the user pass):
// k_staged_item, its edge chains in one or two levels, the owner's share of a multi-GPU step (k_item_apply_counts*), the
// item slices, and their launchers.
#include "bpr_staged.h"

namespace daisy {

constexpr int kItemWaves = 4;      // occupancy floor of the plain SGD item pass, waves per SIMD (see k_staged_item)

// pre-step rows of Q staged in LDS for the commits of one chunk (k_staged_item): rows [first, first + rows)
// (the pointer is an LDS-address-space pointer on purpose: as a generic pointer the commit's row read - window or memory,
// chosen per row - was if-converted into ONE flat_load of a selected address, and a pending FLAT access makes the compiler
// wait for vmcnt(0) AND lgkmcnt(0): every commit then waited for the previous commit's row STORE to land in L2, a full
// trip to memory inside the reduction loop - round 5, profiles/r05_item_pass_counters.txt)
typedef __attribute__((address_space(3))) const float lds_cfloat;
struct QWindow { lds_cfloat *lds; int32_t first, rows; };

// what the owner of a finished segment does with  g = sum_e w_e * stage[slot(e)]  and the entry counts:
//   APPLY:  regulariser reg_1*(np+nn)*sign(q) + reg_2*(np/|Q[i]|_F + nn/|Q[j]|_F)*q  (MFRecommender.py:88-89), then the
//           optimiser's step on Q[item] in place; FM: i_bias[item] follows with the sum of the coefficients
//   else:   gQ[item] = g (data term), cnt[item] = (np, nn): what a multi-GPU step reduce-scatters (FM: g_i_bias[item] =
//           the sum of the coefficients, which the ranks all-reduce)
template <class C, bool APPLY, bool ADAM>
__device__ __forceinline__ void item_commit(float *__restrict__ Qo, float *__restrict__ cnt_out, int64_t item,
                                            const Row<C> &g, float np, float nn, float sb, int lane, int d,
                                            const RowOpt &opt, float reg_1, float rI, float rJ, const StagedBias &fm,
                                            const QWindow win = QWindow{(lds_cfloat *)nullptr, 0, 0},
                                            const Row<C> *qpre = nullptr) {
    if constexpr (APPLY) {
        Row<C> q;
        bool in_lds = false;
        if (qpre) {                                    // (compile-time at every call site) gathered with the stage rows
            q = *qpre;
            in_lds = true;
        } else if constexpr (C::VEC == 4) {
            const uint32_t off = (uint32_t)((int32_t)item - win.first);
            if (off < (uint32_t)win.rows) {            // the row waits in LDS: no dependent trip to memory
                in_lds = true;
                lds_cfloat *src = win.lds + off * (uint32_t)d;
                typedef float v4f __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int c = 0; c < C::NV; ++c) {
                    const int e = (c * C::LPR + lane) * 4;
                    v4f t = {0.f, 0.f, 0.f, 0.f};
                    if (C::EXACT || e < d) t = *reinterpret_cast<__attribute__((address_space(3))) const v4f *>(src + e);
                    q.v[c * 4 + 0] = t.x; q.v[c * 4 + 1] = t.y; q.v[c * 4 + 2] = t.z; q.v[c * 4 + 3] = t.w;
                }
            }
        }
        if (!in_lds) {
            q.load(Qo + item * d, lane, d);
            // the wait for THIS load stays inside this branch (a "use" of its registers): behind the join the compiler
            // would wait for vmcnt(0) on every path, i.e. also where the row came from LDS and only STORES are in flight
#pragma unroll
            for (int k = 0; k < C::NE; ++k) asm volatile("" : "+v"(q.v[k]));
        }
        const float w1 = reg_1 * (np + nn), w2 = np * rI + nn * rJ;
        Row<C> gg;
#pragma unroll
        for (int k = 0; k < C::NE; ++k) gg.v[k] = g.v[k] + fmaf(w2, q.v[k], w1 * sgn(q.v[k]));
        row_apply<C, ADAM>(q, gg, opt, item, lane, d);
        q.store(Qo + item * d, lane, d);
        if (fm.bi && lane == 0) {
            if (fm.grad_out) fm.g_bi[item] = sb;
            else fm.bi[item] = fmaf(-opt.lr, sb, fm.bi[item]);
        }
    } else {
        g.store(Qo + item * d, lane, d);
        if (lane == 0) {
            cnt_out[2 * item] = np; cnt_out[2 * item + 1] = nn;
            if (fm.bi) fm.g_bi[item] = sb;       // FM under a multi-GPU step: dL/d i_bias[item] travels like gQ's rows
        }
    }
}

// Item pass over the staged rows (see the header comment): the run/slot/edge segmented reduction of
// k_item_grad_chunked (segsum.hip) with the coefficient inside the gathered row and the commit in
// the owner.  A workgroup takes a chunk of G*RUN consecutive entries, every lane group a run of RUN.
// MODE (see k_staged_user): premul - entry weight +/-1; plain - the sample's (dL/dpos, dL/dneg) gathered from coef;
// point - weight 1 (a negative slot, which only the sorted layout's point-wise batches have, is inert: weight 0, not
// counted).
// (Occupancy floor: four waves per SIMD; two for the Adam and three-launch forms; three for the sparse flavour of rows of
// 16 floats per lane - d > 128 -, whose two Q rows per run do not fit 128 registers.)
// MERGED (three-launch form, see MergedJob; SGD in place only): the launch also carries the user pass's edge chains and
// the reduction of its sums, as workgroups behind the item pass's own, and every item workgroup derives the norms (and
// whether this step's loss is finite) from the user pass's per-workgroup sums itself.
template <class C, int BLK, int MODE, bool APPLY, bool ADAM, bool SPARSE, bool MERGED = false>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu((ADAM || MERGED) ? 2 : ((SPARSE && C::NE > 8) ? 3 : kItemWaves), 8))) void k_staged_item(const float *__restrict__ stage,
                                                        const float2 *__restrict__ coef, StreamView v, int d,
                                                        float *__restrict__ Qo, float *__restrict__ cnt_out,
                                                        const double *__restrict__ stats, RowOpt opt,
                                                        float reg_1, float reg_2, ItemEdges2 ed,
                                                        const int64_t *__restrict__ erange, StagedBias fm,
                                                        RideUnorm ride, MergedJob mj) {
    static_assert(!MERGED || (APPLY && !ADAM && BLK == kBlock), "the three-launch form: SGD in place, 256-thread workgroups");
    // this step's loss (reduced behind the user pass) or an earlier one was not finite: nothing may be written.  Requested
    // here, looked at behind the first chunk's gathers (see k_staged_user)
    double halt_word = v.halt ? *v.halt : 0.0;
    if (ride.nblocks && (int)blockIdx.x >= ride.first_block) {      // the next batch's pre-norm rides on this launch
        if (halt_word > 0.0) return;
        unorm_block(ride, (int)blockIdx.x - ride.first_block);
        return;
    }
    int item_grid = ride.nblocks ? ride.first_block : (int)gridDim.x;
    float rI = 0.f, rJ = 0.f;
    if constexpr (MERGED) {
        item_grid = (int)gridDim.x - mj.n_ue - 1;
        if ((int)blockIdx.x >= item_grid) {                         // the user pass's edge chains and its reduction
            if (halt_word > 0.0) return;
            user_edges_block<C, false>(blockIdx.x - item_grid, mj.n_ue + 1, mj.P, mj.u_nchunks, d, stats, opt, reg_1, reg_2,
                                       mj.ued, mj.p_sqnorm, mj.pre, mj.red, fm);
            return;
        }
        // what the reduction workgroup will write to stats, formed here from the same sums in the same order
        const double (*sums)[8] = partials_sums(mj.red.partials, mj.red.nblocks);
        double nU, nI, nJ;
        const double loss = loss_from_sums(&(*sums)[0], reg_1, reg_2, nU, nI, nJ);
        // this step's loss is not finite: the epoch stops here - when the caller gave a halt word at all; a bare step
        // (no epoch accumulator) applies the whole step in the four-launch form, and so must this one: its edge launch
        // and the user pass's edge chains have no word to look at
        if (v.halt && (!(loss == loss) || isinf(loss))) halt_word = 1.0;
        rI = inv_or_zero(nI, reg_2);
        rJ = inv_or_zero(nJ, reg_2);
    }
    using Cfg = StagedItemCfg<C, BLK, SPARSE>;
    constexpr int G = Cfg::G, RUN = Cfg::RUN, E = Cfg::E;
    // erange: only the entries [erange[0], erange[1]) - an item range of the batch (the entries are sorted by item, so
    // no segment crosses the cut and the piece is reduced exactly like a whole batch).  Multi-GPU steps cut the item
    // pass into such slices so that a finished slice can be exchanged while the next one is reduced.
    if (erange) {
        const int64_t lo = erange[0];
        v.e_key += lo * v.e_kstride;
        v.e_pos += lo * v.e_stride;
        v.E = erange[1] - lo;
    }
    constexpr int ROWF = C::NE * C::LPR;
    constexpr bool BIAS = MODE != kModePremul;
    __shared__ int slot_item[G + 1], slot_shared[G + 1];
    __shared__ int run_first[G], run_last[G];
    __shared__ float part_acc[2 * G * ROWF];               // [group][head|tail] parked partial sums
    __shared__ float part_np[2 * G], part_nn[2 * G], part_b[2 * G];
    __shared__ int part_slot[2 * G];                       //      the slot each belongs to (-1: unused)
    // Q rows of the chunk's item range [first item, last item], copied by LDS-DMA while the stage rows are in flight:
    // a commit inside the reduction then costs no dependent trip to memory (at a few entries per item - 10 M x 1 M
    // shapes - 355 -> 320 us per pass).  Only for d % 4 == 0 (16-byte units); rows past the window (sparse batches: few
    // entries spread over many items) are loaded directly.
    constexpr bool WIN = APPLY && C::VEC == 4 && C::NE <= 8 && !SPARSE;
    constexpr bool QPRE = APPLY && SPARSE;                 // the Q row of every entry rides with its staged row
    // (24 KB per 256 threads: the CU's LDS is shared by 256 / BLK times as many workgroups, a chunk covers BLK / 256 of the items)
    constexpr int WINF = ((C::NE <= 4) ? kItemWinFloats : (kItemWinFloats * 2 / 3)) * BLK / kBlock;
    __shared__ __attribute__((aligned(16))) float qwin[WIN ? WINF : 4];
    // sparse flavour: the pre-step row of Q of a segment that leaves its run through the TAIL, for the slot's finisher (a
    // load there would sit behind this chunk's row stores: k_staged_user's part_p has the story)
    __shared__ float part_q[QPRE ? G * ROWF : 4];

    const int tid = threadIdx.x;
    const int lane = tid % C::LPR;
    const int group = tid / C::LPR;
    const int64_t n = v.E;
    const int64_t nchunks = (n + E - 1) / E;
    const bool has_bias = BIAS && fm.bi != nullptr;
    if constexpr (APPLY && !MERGED) {
        rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
        rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    }

    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += item_grid) {
        const int64_t c0 = chunk * E;
        const int64_t t0 = c0 + (int64_t)group * RUN;
        const int64_t t1 = (t0 + RUN < n) ? (t0 + RUN) : n;
        const int cnt = (t0 < n) ? (int)(t1 - t0) : 0;       // entries of this run

        // ---- hop 1: the run's metadata, lane x <- entry x, plus the entries around the run
        const int64_t last = n - 1;
        const int64_t il = (t0 + lane < n) ? (t0 + lane) : last;
        const uint32_t k_me = sv_key(v, il);
        const uint32_t slot_me = (v.e_pos[il * v.e_stride] & ~kNegBit) - v.pos_base;
        const uint32_t k_prev = sv_key(v, (t0 > 0) ? ((t0 - 1 < n) ? t0 - 1 : last) : 0);
        const uint32_t k_next = sv_key(v, (t1 < n) ? t1 : last);
        const uint32_t k_cprev = sv_key(v, (c0 > 0) ? c0 - 1 : 0);
        const int32_t my_item = (lane < cnt) ? (int32_t)(k_me >> 1) : -1;
        const int32_t my_neg = (int32_t)(k_me & 1u);
        const int32_t item_prev = (cnt > 0 && t0 > 0) ? (int32_t)(k_prev >> 1) : -1;
        const int32_t item_next = (cnt > 0 && t1 < n) ? (int32_t)(k_next >> 1) : -1;
        // (workgroup-uniform values that come out of a vector load: as scalars they cost no vector register)
        const int32_t chunk_prev_item = (c0 > 0) ? __builtin_amdgcn_readfirstlane((int32_t)(k_cprev >> 1)) : -1;
        QWindow win{(lds_cfloat *)qwin, 0, 0};
        if constexpr (WIN) {
            const int64_t c1 = (c0 + E < n) ? (c0 + E) : n;
            win.first = __builtin_amdgcn_readfirstlane((int32_t)(sv_key(v, c0) >> 1));
            const int32_t item_hi = __builtin_amdgcn_readfirstlane((int32_t)(sv_key(v, c1 - 1) >> 1));
            const int32_t cap = WINF / d;
            win.rows = (item_hi - win.first + 1 < cap) ? (item_hi - win.first + 1) : cap;
            const int units = win.rows * (d >> 2);                      // 16-byte units, contiguous in Q
            const float *src = Qo + (int64_t)win.first * d;
            const int wave_base = __builtin_amdgcn_readfirstlane((tid / kWave) * kWave);
            for (int u0 = 0; u0 < units; u0 += BLK) {                   // (workgroup-uniform trip count)
                const int u = u0 + tid;
                if (u < units)
                    __builtin_amdgcn_global_load_lds(src + 4 * (int64_t)u,
                                                     (__attribute__((address_space(3))) void *)(qwin + 4 * (u0 + wave_base)),
                                                     16, 0, 0);
            }
        }
        if (tid < 2 * G) part_slot[tid] = -1;
        if (tid <= G) { slot_item[tid] = -1; slot_shared[tid] = 0; }
        const int32_t item_first = group_bcast<C>(my_item, 0);
        const int32_t item_last = __shfl(my_item, cnt > 0 ? cnt - 1 : 0, C::LPR);
        if (lane == 0) {
            run_first[group] = cnt > 0 ? item_first : -2;
            run_last[group] = cnt > 0 ? item_last : -2;
        }

        // ---- hop 2: all staged rows of the run (and, for the flavours whose coefficients are not in the row, theirs)
        float my_w, my_c = 0.f;             // weight of the entry's staged row; its bare coefficient (FM's item bias)
        if constexpr (MODE == kModePremul) {
            my_w = (lane < cnt) ? (my_neg ? -1.f : 1.f) : 0.f;
        } else if constexpr (MODE == kModePlain) {
            const float2 c2 = coef[slot_me];
            my_w = (lane < cnt) ? (my_neg ? c2.y : c2.x) : 0.f;
            my_c = my_w;
        } else {
            my_w = (lane < cnt && !my_neg) ? 1.f : 0.f;
            if (has_bias) my_c = (lane < cnt && !my_neg) ? coef[slot_me].x : 0.f;
        }
        Row<C> p[RUN], qe[QPRE ? RUN : 1];
        if (__all(cnt == RUN)) {        // wave-uniform: every run of this wave is full
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                p[x].load(stage + (int64_t)group_bcast<C>(slot_me, x) * d, lane, d);
                if constexpr (QPRE) qe[x].load(Qo + (int64_t)group_bcast<C>(my_item, x) * d, lane, d);
            }
        } else {
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const uint32_t sx = group_bcast<C>(slot_me, x);
                const int32_t ix = group_bcast<C>(my_item, x);
                if (x < cnt) {
                    p[x].load(stage + (int64_t)sx * d, lane, d);
                    if constexpr (QPRE) qe[x].load(Qo + (int64_t)ix * d, lane, d);
                } else {
                    p[x].zero();
                    if constexpr (QPRE) qe[x].zero();
                }
            }
        }
        // the window has landed before anyone reads it.  (Round 4 tried the counted form - the LDS-DMA issued from an asm
        // statement so that the compiler keeps no LDS write pending on the VM counter, s_waitcnt vmcnt(RUN * NV) here,
        // the window read as a proper ds_read_b128 instead of the flat load a generic pointer yields - so that the
        // reduction starts on the first stage rows while the last are in flight: 24 B of scratch at the 128-register
        // cap, and within +-1.5 % of this form at both BASELINE shapes, same box: profiles/r04_item_plan_variants.txt.
        // The pass is not bound by this wait.)
        if constexpr (WIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (the same for the window: one LDS read that may alias the LDS-DMA's destination makes the compiler's own wait for
        // the DMA happen HERE, once, instead of in front of every commit's window read)
        if constexpr (WIN) {
            float w0 = ((lds_cfloat *)qwin)[tid & 3];
            asm volatile("" : "+v"(w0));
        }
        // every gathered row register is "used" here, so the COMPILER waits for the gathers here and knows they are done:
        // with the wait hidden in the asm statement above it kept all of them pending in its scoreboard, and since the
        // vector-memory counter also counts stores, the first use of a row behind a commit's store (data-dependent
        // control flow, merged states) became s_waitcnt vmcnt(0) - the reduction waited for every row store it issued
#pragma unroll
        for (int x = 0; x < RUN; ++x) {
#pragma unroll
            for (int k = 0; k < C::NE; ++k) asm volatile("" : "+v"(p[x].v[k]));
            if constexpr (QPRE) {
#pragma unroll
                for (int k = 0; k < C::NE; ++k) asm volatile("" : "+v"(qe[x].v[k]));
            }
        }
        if (halt_word > 0.0) return;           // (uniform over the grid; nothing has been written yet)
        __syncthreads();

        if (cnt > 0) {
            const bool cont = (t0 > 0) && (item_prev == item_first);
            int cur_slot = -1;                      // >= 0: the current segment began before this run
            if (cont) {
                if (group == 0) cur_slot = 0;       // inherited from the previous chunk
                else {
                    int gs = group - 1;
                    while (gs > 0 && run_first[gs] == item_first && run_last[gs - 1] == item_first) --gs;
                    const bool inherited = (gs == 0) && (run_first[0] == item_first) && (c0 > 0) &&
                                           (chunk_prev_item == item_first);
                    cur_slot = inherited ? 0 : gs + 1;
                }
            }
            int32_t cur_item = item_first;
            Row<C> acc;
            acc.zero();
            float np = 0.f, nn = 0.f, sb = 0.f;
            Row<C> qcur;                            // QPRE: the pre-step row of the current segment's item
            if constexpr (QPRE) qcur = qe[0];
            auto finish = [&](bool ends_here, bool to_next_chunk) {
                if (cur_slot < 0 && ends_here) {    // interior: this group owns the item's row
                    item_commit<C, APPLY, ADAM>(Qo, cnt_out, cur_item, acc, np, nn, sb, lane, d, opt, reg_1, rI, rJ, fm, win,
                                                QPRE ? &qcur : nullptr);
                } else {                            // crosses a run boundary: park it for the slot's finisher
                    const int s = (cur_slot >= 0) ? cur_slot : group + 1;
                    const int q = group * 2 + ((cur_slot >= 0) ? 0 : 1);
                    float *dst = part_acc + q * ROWF;
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) dst[k * C::LPR + lane] = acc.v[k];
                    if constexpr (QPRE) {
                        if (cur_slot < 0) {
                            float *qd = part_q + group * ROWF;
#pragma unroll
                            for (int k = 0; k < C::NE; ++k) qd[k * C::LPR + lane] = qcur.v[k];
                        }
                    }
                    if (lane == 0) {
                        part_slot[q] = s;
                        part_np[q] = np;
                        part_nn[q] = nn;
                        part_b[q] = sb;
                        slot_item[s] = cur_item;
                        if (to_next_chunk) slot_shared[s] = 1;
                    }
                }
            };
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                if (x < cnt) {
                    const int32_t it = group_bcast<C>(my_item, x);
                    const float wx = group_bcast<C>(my_w, x);
                    const float ng = (float)group_bcast<C>(my_neg, x);
                    if (it != cur_item) {           // previous segment ended inside this run
                        finish(true, false);
                        cur_item = it;
                        cur_slot = -1;
                        acc.zero();
                        np = 0.f; nn = 0.f; sb = 0.f;
                        if constexpr (QPRE) qcur = qe[x];
                    }
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) acc.v[k] = fmaf(wx, p[x].v[k], acc.v[k]);
                    if constexpr (MODE == kModePoint) {
                        np += 1.f - ng;             // (an inert negative slot is not counted)
                    } else {
                        np += 1.f - ng;
                        nn += ng;
                    }
                    if constexpr (BIAS) sb += group_bcast<C>(my_c, x);
                }
            }
            const bool continues = (t1 < n) && (item_next == cur_item);
            finish(!continues, continues && (group == G - 1));
        }
        __syncthreads();

        if (tid == 0) { ed.item[2 * chunk] = -1; ed.item[2 * chunk + 1] = -1; ed.whole[chunk] = 0; }
        __syncthreads();
        // one finisher per used slot (G+1 slots over G groups): the parked partials in group order
        for (int s = group; s <= G; s += G) {
            const int r = slot_item[s];
            if (r < 0) continue;
            Row<C> g;
            g.zero();
            float sp = 0.f, sn = 0.f, sc = 0.f;
            auto add_part = [&](int q) {
                const float *src = part_acc + q * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) g.v[k] += src[k * C::LPR + lane];
                sp += part_np[q];
                sn += part_nn[q];
                sc += part_b[q];
            };
            // the partial sums of slot s, in group order: the TAIL of group s - 1 (the run the segment began in; slot 0
            // came from the previous chunk and has none), then the HEADS of the groups s, s + 1, ... it runs through -
            // consecutive by construction.  (Until round 5 a scan over all 2 G parked slots: 32 dependent LDS reads per
            // finisher where two or three are needed - 1.3 of the ~1.8 us a chunk spends behind its gathers.)
            if (s > 0 && part_slot[2 * s - 1] == s) add_part(2 * s - 1);
            for (int q = 2 * s; q < 2 * G && part_slot[q] == s; q += 2) add_part(q);
            const bool from_prev = (s == 0), to_next = slot_shared[s] != 0;
            if (from_prev || to_next) {
                const int64_t e = 2 * chunk + (from_prev ? 0 : 1);
                g.store(ed.vec + e * d, lane, d);
                if (lane == 0) {
                    ed.item[e] = r;
                    ed.cnt[4 * e] = sp;
                    ed.cnt[4 * e + 1] = sn;
                    ed.cnt[4 * e + 2] = sc;
                    if (from_prev && to_next) ed.whole[chunk] = 1;
                }
            } else if constexpr (QPRE) {             // (s >= 1 here: the tail of group s - 1 parked the pre-step row)
                Row<C> qrow;
                const float *qs = part_q + (s - 1) * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) qrow.v[k] = qs[k * C::LPR + lane];
                item_commit<C, APPLY, ADAM>(Qo, cnt_out, r, g, sp, sn, sc, lane, d, opt, reg_1, rI, rJ, fm, win, &qrow);
            } else {
                item_commit<C, APPLY, ADAM>(Qo, cnt_out, r, g, sp, sn, sc, lane, d, opt, reg_1, rI, rJ, fm, win);
            }
        }
        __syncthreads();   // the slots are reused by the next chunk
    }
}

// How many of flag[first], flag[first + 1], ... (at most maxn) are non-zero before the first zero.  One lane group: its
// lanes load C::LPR flags at a time, the wave ballot hands every group its own bits (a group that has left the loop
// contributes none).  A chain's links used to be found one dependent load after the other - ~1 us per link.
template <class C>
__device__ __forceinline__ int64_t group_leading_ones(const int32_t *__restrict__ flag, int64_t first, int64_t maxn, int lane) {
    constexpr int GPW = kWave / C::LPR;
    const int gw = (threadIdx.x % kWave) / C::LPR;
    int64_t total = 0;
    for (int64_t base = 0; base < maxn; base += C::LPR) {
        const int64_t idx = base + lane;
        const bool f = idx < maxn && flag[first + idx] != 0;
        const uint64_t m = __ballot(f);
        int ones;
        if constexpr (GPW == 1) ones = (m == ~0ull) ? 64 : __builtin_ctzll(~m);
        else ones = __builtin_ctzll(~((m >> (C::LPR * gw)) & ((1ull << C::LPR) - 1)));
        total += ones;
        if (ones < C::LPR) break;
    }
    return total < maxn ? total : maxn;
}

// acc += the `count` records first, first + step, ... of (vec, cnt), in that order, four loads in flight
template <class C>
__device__ __forceinline__ void add_edge_records(Row<C> &acc, float &sp, float &sn, float &sc, const float *__restrict__ vec,
                                                 const float *__restrict__ cnt, int64_t first, int64_t step, int64_t count,
                                                 int lane, int d) {
    if (count == 1) {                       // (the common chain at uniform ids: one link - one load, not four clamped ones)
        Row<C> t;
        t.load(vec + first * d, lane, d);
#pragma unroll
        for (int e = 0; e < C::NE; ++e) acc.v[e] += t.v[e];
        sp += cnt[4 * first]; sn += cnt[4 * first + 1]; sc += cnt[4 * first + 2];
        return;
    }
    for (int64_t j = 0; j < count; j += 4) {
        Row<C> t[4];
        float c0[4], c1[4], c2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = first + ((j + q < count) ? (j + q) : (count - 1)) * step;      // (clamped: no load behind a branch)
            t[q].load(vec + r * d, lane, d);
            c0[q] = cnt[4 * r]; c1[q] = cnt[4 * r + 1]; c2[q] = cnt[4 * r + 2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (j + q < count) {
#pragma unroll
                for (int e = 0; e < C::NE; ++e) acc.v[e] += t[q].v[e];
                sp += c0[q]; sn += c1[q]; sc += c2[q];
            }
        }
    }
}

template <class C>
__global__ __launch_bounds__(kBlock) void k_staged_item_edge_blocks(ItemEdges2 ed, int64_t nchunks, int d,
                                                                    const int64_t *__restrict__ erange, int chunk_entries,
                                                                    const double *__restrict__ halt, EdgeBlocks eb) {
    if (halted(halt)) return;
    if (erange) nchunks = (erange[1] - erange[0] + chunk_entries - 1) / chunk_entries;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t nblocks = (nchunks + kEdgeBlock - 1) / kEdgeBlock;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    for (int64_t b = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; b < nblocks; b += gstride) {
        const int64_t k0 = b * kEdgeBlock;
        const int64_t k1 = (k0 + kEdgeBlock < nchunks) ? k0 + kEdgeBlock : nchunks;
        const int it = ed.item[2 * k0];
        int through = 0;
        if (it >= 0) {
            // chunk k0's head edge is the chain's; chunk k + 1's is too iff the chain also fills chunk k and runs on
            const int64_t ones = group_leading_ones<C>(ed.whole, k0, k1 - k0, lane);
            const int64_t links = (ones + 1 < k1 - k0) ? ones + 1 : k1 - k0;
            through = (ones == k1 - k0) ? 1 : 0;           // every chunk of the block belongs to the chain, and it runs on
            Row<C> acc;
            acc.zero();
            float sp = 0.f, sn = 0.f, sc = 0.f;
            add_edge_records<C>(acc, sp, sn, sc, ed.vec, ed.cnt, 2 * k0, 2, links, lane, d);
            acc.store(eb.vec + b * d, lane, d);
            if (lane == 0) { eb.cnt[4 * b] = sp; eb.cnt[4 * b + 1] = sn; eb.cnt[4 * b + 2] = sc; }
        }
        if (lane == 0) { eb.item[b] = it; eb.through[b] = through; }
    }
}

// chains of edge records - the chunk whose TAIL edge starts a segment owns it and adds the head edges of
// the chunks it runs through, in chunk order (single writer per row, fixed order)
template <class C, bool APPLY, bool ADAM>
__global__ __launch_bounds__(kBlock) void k_staged_item_edges(ItemEdges2 ed, int64_t nchunks, int d,
                                                              float *__restrict__ Qo, float *__restrict__ cnt_out,
                                                              const double *__restrict__ stats, RowOpt opt,
                                                              float reg_1, float reg_2,
                                                              const int64_t *__restrict__ erange, int chunk_entries,
                                                              const double *__restrict__ halt, StagedBias fm,
                                                              RideReduce rr, RideUnorm ride, EdgeBlocks eb) {
    if (halted(halt)) return;
    if (ride.nblocks && (int)blockIdx.x >= ride.first_block) {     // three-launch form: the next batch's pre-norm rides HERE
        unorm_block(ride, (int)blockIdx.x - ride.first_block);     // (the user pass's edge chains ran in the item launch)
        return;
    }
    unsigned nb = ride.nblocks ? (unsigned)ride.first_block : gridDim.x;
    if (rr.n) {                            // the last workgroup adds the next batch's pre-norm partial sums (k_unorm_reduce)
        nb -= 1;
        if (blockIdx.x == nb) {
            __shared__ double sm[kBlock];
            double t = 0.0;
            for (int b = threadIdx.x; b < rr.n; b += kBlock) t += rr.partials[b];
            sm[threadIdx.x] = t;
            __syncthreads();
            for (int off = kBlock / 2; off > 0; off >>= 1) {
                if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
                __syncthreads();
            }
            if (threadIdx.x == 0) rr.stats[DAISY_ST_SQ_U_PRE] = sm[0];
            return;
        }
    }
    if (erange) nchunks = (erange[1] - erange[0] + chunk_entries - 1) / chunk_entries;      // chunks of the slice
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)nb * C::GROUPS_PER_BLOCK;
    float rI = 0.f, rJ = 0.f;
    if constexpr (APPLY) {
        rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
        rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    }
    for (int64_t c = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; c < nchunks; c += gstride) {
        const int it = ed.item[2 * c + 1];
        if (it < 0) continue;
        Row<C> acc;
        acc.load(ed.vec + (2 * c + 1) * d, lane, d);
        float sp = ed.cnt[4 * (2 * c + 1)], sn = ed.cnt[4 * (2 * c + 1) + 1], sc = ed.cnt[4 * (2 * c + 1) + 2];
        // link by link - to the end of the chain, or (two levels) to the next block boundary: chunk c + 1's head edge is
        // the chain's (this tail edge runs on into it); chunk k + 1's is iff the chain also fills chunk k
        const int64_t k = c + 1;
        int64_t reach = nchunks;
        if (eb.vec != nullptr) {
            const int64_t bnd = (k + kEdgeBlock - 1) / kEdgeBlock * kEdgeBlock;
            reach = bnd < nchunks ? bnd : nchunks;
        }
        bool open = k < nchunks && ed.item[2 * k] == it;
        if (open && reach > k) {
            const int64_t ones = group_leading_ones<C>(ed.whole, k, reach - k, lane);
            const int64_t links = (ones + 1 < reach - k) ? ones + 1 : reach - k;
            add_edge_records<C>(acc, sp, sn, sc, ed.vec, ed.cnt, 2 * k, 2, links, lane, d);
            open = ones == reach - k;
        }
        // block by block: the block sum of the chain that enters block b is this chain's; it runs on while `through`
        if (eb.vec != nullptr && open && reach < nchunks) {
            const int64_t b0 = reach / kEdgeBlock, nb = (nchunks + kEdgeBlock - 1) / kEdgeBlock;
            if (eb.item[b0] == it) {
                const int64_t ones = group_leading_ones<C>(eb.through, b0, nb - b0, lane);
                const int64_t blocks = (ones + 1 < nb - b0) ? ones + 1 : nb - b0;
                add_edge_records<C>(acc, sp, sn, sc, eb.vec, eb.cnt, b0, 1, blocks, lane, d);
            }
        }
        item_commit<C, APPLY, ADAM>(Qo, cnt_out, it, acc, sp, sn, sc, lane, d, opt, reg_1, rI, rJ, fm);
    }
}

// Q[r] -= lr*(g[r] + regulariser from the GLOBAL entry counts); g[r] = 0, cnt[r] = 0: the owner's share of a
// multi-GPU step after the reduce-scatter of (gQ, cnt)
template <class C>
__global__ __launch_bounds__(kBlock) void k_item_apply_counts(float *__restrict__ Q, float *__restrict__ g,
                                                              float *__restrict__ cnt, int64_t rows, int d,
                                                              float lr, float reg_1, float reg_2,
                                                              const double *__restrict__ stats) {
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const float rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
    const float rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    for (int64_t r = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; r < rows; r += gstride) {
        const float np = cnt[2 * r], nn = cnt[2 * r + 1];
        if (np + nn == 0.f) continue;              // untouched by every rank: the row does not move
        Row<C> gr, z;
        gr.load(g + r * d, lane, d);
        RowOpt opt{};
        opt.lr = lr;
        item_commit<C, true, false>(Q, nullptr, r, gr, np, nn, 0.f, lane, d, opt, reg_1, rI, rJ, StagedBias{});
        z.zero();
        z.store(g + r * d, lane, d);
        if (lane == 0) { cnt[2 * r] = 0.f; cnt[2 * r + 1] = 0.f; }
    }
}

// The same owner step with torch.optim.Adam (multi-GPU staged step): DENSE over the owner's block - every row steps in
// every step like torch's optimiser (rows without an entry: zero gradient, the moments decay), at I/N rows per rank.
template <class C>
__global__ __launch_bounds__(kBlock) void k_item_apply_counts_adam(float *__restrict__ Q, float *__restrict__ g,
                                                                   float *__restrict__ cnt, float *__restrict__ m,
                                                                   float *__restrict__ vv, int64_t rows, int d,
                                                                   float reg_1, float reg_2, RowOpt opt,
                                                                   const double *__restrict__ stats) {
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    const float rI = inv_or_zero(stats[DAISY_ST_NORM_I], reg_2);
    const float rJ = inv_or_zero(stats[DAISY_ST_NORM_J], reg_2);
    for (int64_t r = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; r < rows; r += gstride) {
        const float np = cnt[2 * r], nn = cnt[2 * r + 1];
        Row<C> q, gr, mr, vr;
        q.load(Q + r * d, lane, d);
        mr.load(m + r * d, lane, d);
        vr.load(vv + r * d, lane, d);
        gr.zero();
        if (np + nn != 0.f) {
            gr.load(g + r * d, lane, d);
            const float w1 = reg_1 * (np + nn), w2 = np * rI + nn * rJ;
#pragma unroll
            for (int k = 0; k < C::NE; ++k) gr.v[k] += fmaf(w2, q.v[k], w1 * sgn(q.v[k]));
        }
        adam_row<C>(q, mr, vr, gr, opt.step_size, opt.bc2_sqrt, opt.beta1, opt.beta2, opt.eps);
        q.store(Q + r * d, lane, d);
        mr.store(m + r * d, lane, d);
        vr.store(vv + r * d, lane, d);
        if (np + nn != 0.f) {
            Row<C> z;
            z.zero();
            z.store(g + r * d, lane, d);
            if (lane == 0) { cnt[2 * r] = 0.f; cnt[2 * r + 1] = 0.f; }
        }
    }
}

// rng[s] = first entry of the batch whose item is >= bounds.b[s]  (s = 0..S; the entries are sorted by item)
struct SliceBounds { int32_t b[kMaxItemSlices + 1]; };
__global__ void k_slice_ranges(StreamView v, SliceBounds bounds, int S, int64_t *__restrict__ rng) {
    const int s = threadIdx.x;
    if (s > S) return;
    int64_t lo = 0, hi = v.E;
    const uint32_t want = (uint32_t)bounds.b[s];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((sv_key(v, mid) >> 1) < want) lo = mid + 1; else hi = mid;
    }
    rng[s] = lo;
}

// ---- launchers: what the path says, nothing else
// the item pass, (path.two_level) the block sums of its edge chains, its edge chains.  path.merge (three-launch form;
// apply, SGD): the item launch carries the user pass's edge work, the item pass keeps its edge records in the context's
// second set, and the next batch's pre-norm rides on the item-EDGE launch instead of the item launch
int staged_item(daisy_bpr_ctx *ctx, const StagedPath &path, const StagedStep &st, float *P, float *Qo, float *cnt_out) {
    const int64_t *erange = (path.slice >= 0) ? ctx->slice_rng + path.slice : nullptr;
    const StreamView &v = ctx->sv;
    const int d = ctx->d;
    const ItemEdges2 ed = path.merge ? ItemEdges2{ctx->edge2_vec, ctx->edge2_item, ctx->edge2_cnt, ctx->edge2_whole}
                                     : ItemEdges2{ctx->edge_vec, ctx->edge_user, ctx->edge_cnt, ctx->edge_whole};
    const EdgeBlocks eb = path.two_level ? EdgeBlocks{ctx->eb_vec, ctx->eb_item, ctx->eb_cnt, ctx->eb_through}
                                         : EdgeBlocks{nullptr, nullptr, nullptr, nullptr};
    const RowOpt opt = row_opt(st.lr, st.adam, false);
    const StagedBias fm = staged_bias(ctx, st.bias_grad_out);
    const double *stats = st.stats;
    RideUnorm ride{nullptr, nullptr, 0, nullptr, 0, 0}, ru_edge = ride;
    RideReduce rr{nullptr, 0, nullptr};
    if (path.ride) {
        const StreamView nv = plan_stream_view(ctx->cur_plan, ctx->cur_k + 1);
        ride = RideUnorm{ctx->p_sqnorm, nv.s_rec, nv.B, path.ride_fold ? ctx->partials + (size_t)kMaxGrid * 8 : ctx->partials,
                         0, path.gn};
        if (!path.ride_fold) rr = RideReduce{ride.partials, path.gn, st.stats};
    }
    const int ge_own = path.n_ie + (rr.n ? 1 : 0);
    RideUnorm ru = ride;
    MergedJob mj{};
    if (path.merge) {                    // the ride moves to the edge launch; the user pass's edge work joins this one
        ru_edge = ride;
        ru_edge.first_block = ge_own;
        ru.nblocks = 0;
        mj = MergedJob{P, path.u_chunks, staged_user_edges(ctx), ctx->p_sqnorm, staged_pre(ctx, path),
                       staged_reduce(ctx, path, st), path.n_ue};
    }
    ru.first_block = path.gi;            // the riding workgroups follow the item pass's own
    const dim3 g(path.gi + ru.nblocks + (path.merge ? mj.n_ue + 1 : 0)), ge(ge_own + ru_edge.nblocks);
    int rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        auto item = [&](auto blk_tag, auto mode_tag, auto ap_tag, auto adam_tag, auto sp_tag, auto mg_tag) {
            constexpr int BLK = decltype(blk_tag)::value;
            constexpr bool AP = decltype(ap_tag)::value, AD = decltype(adam_tag)::value, SP = decltype(sp_tag)::value,
                           MG = decltype(mg_tag)::value;
            // the kernel exists for (AP, AD, SP, MG) =    in place, SGD: (1,0,0,0) (1,0,1,0), and at 256 threads
            //   gradient out: (0,0,0,0)   Adam: (1,1,0,0)          three-launch form: (1,0,0,1) (1,0,1,1)
            // - six per mode at BLK = 256, four at 128; staged_path yields nothing else
            if constexpr ((AP || !AD) && (!SP || (AP && !AD)) && (!MG || (AP && !AD && BLK == kBlock)))
                hipLaunchKernelGGL((k_staged_item<C, BLK, decltype(mode_tag)::value, AP, AD, SP, MG>), g, dim3(BLK), 0, st.s,
                                   ctx->p_stage, ctx->coef, v, d, Qo, cnt_out, stats, opt, st.reg_1, st.reg_2, ed, erange, fm,
                                   ru, mj);
        };
        with_flag(path.i_blk == kBlock, [&](auto big) { with_mode(path.mode, [&](auto m) { with_flag(path.apply, [&](auto ap) {
            with_flag(path.adam, [&](auto ad) { with_flag(path.sparse, [&](auto sp) { with_flag(path.merge, [&](auto mg) {
                item(std::integral_constant<int, decltype(big)::value ? kBlock : kStagedItemBlock>{}, m, ap, ad, sp, mg);
            }); }); });
        }); }); });
        if (path.two_level)
            hipLaunchKernelGGL((k_staged_item_edge_blocks<C>),
                               dim3(grid_for((path.i_chunks + kEdgeBlock - 1) / kEdgeBlock, C::GROUPS_PER_BLOCK)), dim3(kBlock), 0,
                               st.s, ed, path.i_chunks, d, erange, path.i_chunk, v.halt, eb);
        with_flag(path.apply, [&](auto ap) { with_flag(path.adam, [&](auto ad) {
            constexpr bool AP = decltype(ap)::value, AD = decltype(ad)::value;
            if constexpr (AP || !AD)
                hipLaunchKernelGGL((k_staged_item_edges<C, AP, AD>), ge, dim3(kBlock), 0, st.s, ed, path.i_chunks, d, Qo, cnt_out,
                                   stats, opt, st.reg_1, st.reg_2, erange, path.i_chunk, v.halt, fm, rr, ru_edge, eb);
        }); });
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int staged_slice_ranges(daisy_bpr_ctx *ctx, const int32_t *item_bounds, int n_slices, hipStream_t s) {
    SliceBounds sb;
    for (int k = 0; k <= n_slices; ++k) sb.b[k] = item_bounds[k];
    hipLaunchKernelGGL(k_slice_ranges, dim3(1), dim3(64), 0, s, ctx->sv, sb, n_slices, ctx->slice_rng);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int item_apply_counts(float *Q, float *g, float *cnt, float *m, float *v, int64_t rows, int d, float reg_1, float reg_2,
                      const RowOpt &opt, const double *stats, hipStream_t s) {
    int rc = dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        const dim3 grid(grid_for(rows, C::GROUPS_PER_BLOCK * 2));
        if (m) hipLaunchKernelGGL((k_item_apply_counts_adam<C>), grid, dim3(kBlock), 0, s, Q, g, cnt, m, v, rows, d, reg_1, reg_2,
                                  opt, stats);
        else hipLaunchKernelGGL((k_item_apply_counts<C>), grid, dim3(kBlock), 0, s, Q, g, cnt, rows, d, opt.lr, reg_1, reg_2, stats);
        return DAISY_OK;
    });
    if (rc) return rc;
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace daisy
