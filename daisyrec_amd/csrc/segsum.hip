// Segmented sum over entries sorted by row, for gfx950 (MI355X): the library's shared sparse x dense product
//   out[row] = sum over the row's entries e of  w_e * X[col_e]
// The entries arrive as a BatchView: ekey[e] holds the row (sorted), esu[e] = (index of the weight in coef, column).
// The MF item gradient is one caller (rows = items, the entries are the batch's positives and negatives sorted by
// item, X = P, w = the loss coefficients: the data term  sum_e c_e * p_u(e)  only; the regulariser share is added by
// k_item_reg or folded into the commit kernel, bpr_train.hip); LightGCN's propagation and the NeuMF table scatter
// are the others (segsum_rows).
//
// Measured on MI355X (profiles/r01_probe_*): random 256-B row gathers / plain stores run at 5-8 TB/s, fp32 global
// atomics at 0.3 TB/s.  So the sum is organised around OWNERSHIP instead of atomics, and its summation order is
// fixed: the result is bitwise reproducible.
//
// A workgroup takes a chunk of G*RUN consecutive entries, every lane group a run of RUN of them: one load fetches
// the run's metadata (lane x <- entry x), then all RUN row gathers are in flight together.  A segment (= all entries
// of one row) that lies inside one run is summed in registers and stored straight to the output by its group (single
// owner, no atomics, no LDS).  Only segments that cross a run boundary - at most one per boundary - go through an LDS
// slot (slot s>0: the segment that starts in run s-1; slot 0: the segment inherited from the previous chunk): a group
// does not add its run-crossing partial sums into the slot but parks them (<= 2 per group: the segment it continues,
// the segment it hands on), and after a barrier the slot's finisher adds them in group order and writes the slot
// once: a plain store if the segment lies inside the chunk; segments shared with a neighbouring chunk (<= 2 per
// chunk) leave the chunk as edge records that k_item_edges chains in chunk order.
#include "bpr_internal.h"
#include "segsum.h"

namespace daisy {

template <class C, int RUN_OVERRIDE = 0>
struct RunCfg {
    // needs RUN <= LPR (lane x holds the metadata of entry x); RUN*NE row registers are live at once
    static constexpr int RUN_BY_REGS = (C::NE <= 4) ? 16 : ((C::NE <= 8) ? 4 : 2);
    static constexpr int RUN_AUTO = RUN_BY_REGS < C::LPR ? RUN_BY_REGS : C::LPR;
    static constexpr int RUN = (RUN_OVERRIDE > 0 && RUN_OVERRIDE <= C::LPR) ? RUN_OVERRIDE : RUN_AUTO;
    static constexpr int G = C::GROUPS_PER_BLOCK;
    static constexpr int E = G * RUN;
};

// The run length segsum_rows uses for a row shape.  Wide rows (d > 128: 16 floats per lane) default to 2 rows in
// flight per lane group; 4 measured faster for the NeuMF tables (fewer, longer chunks: 3 barriers per chunk).  The
// MF item gradient (segsum_item_grad) keeps the default for every shape.
template <class C>
constexpr int kSegsumRowsRun = (C::NE == 16) ? 4 : 0;

template <class C, int RUN_OVERRIDE = 0, bool XH = false>      // XH: the gathered rows are bf16
__global__ __launch_bounds__(kBlock) void k_item_grad_chunked(const float *__restrict__ P,
                                                              const float2 *__restrict__ coef,
                                                              BatchView v, int d,
                                                              float *__restrict__ gQ, ItemEdges edges) {
    if (halted(v.halt)) return;
    constexpr int G = RunCfg<C, RUN_OVERRIDE>::G, RUN = RunCfg<C, RUN_OVERRIDE>::RUN,
                  E = RunCfg<C, RUN_OVERRIDE>::E;
    constexpr int ROWF = C::NE * C::LPR;
    __shared__ int slot_item[G + 1], slot_shared[G + 1];
    __shared__ int run_first[G], run_last[G];
    __shared__ float part_acc[2 * G * ROWF];     // [group][head|tail] parked partial sums
    __shared__ float part_b[2 * G];              // FM: sum of the coefficients (d loss / d i_bias)
    __shared__ int part_slot[2 * G];             // the slot each belongs to (-1: unused)

    const int tid = threadIdx.x;
    const int lane = tid % C::LPR;
    const int group = tid / C::LPR;
    const int64_t n = 2 * v.B;
    const int64_t nchunks = (n + E - 1) / E;

    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t c0 = chunk * E;
        const int64_t t0 = c0 + (int64_t)group * RUN;
        const int64_t t1 = (t0 + RUN < n) ? (t0 + RUN) : n;
        const int cnt = (t0 < n) ? (int)(t1 - t0) : 0;       // entries of this run

        // ---- hop 1: the run's metadata, lane x <- entry x; plus the entries just before and
        // after the run (same address on every lane: one request)
        // Every load is unconditional on a clamped address (n >= 1 here): a branch around a
        // load makes the compiler drain vmcnt before it, which would serialise these requests
        // into one memory round trip each.
        const int64_t last = n - 1;
        const int64_t il = (t0 + lane < n) ? (t0 + lane) : last;
        const uint32_t k_me = v.ekey[il];
        const uint2 su_me = v.esu[il];
        const uint32_t k_prev = v.ekey[(t0 > 0) ? ((t0 - 1 < n) ? t0 - 1 : last) : 0];
        const uint32_t k_next = v.ekey[(t1 < n) ? t1 : last];
        const uint32_t k_cprev = v.ekey[(c0 > 0) ? c0 - 1 : 0];
        const int32_t my_item = (lane < cnt) ? (int32_t)((k_me & v.imask) >> 1) : -1;
        const uint2 my_su = (lane < cnt) ? su_me : make_uint2(0u, 0u);
        const int32_t item_prev = (cnt > 0 && t0 > 0) ? (int32_t)((k_prev & v.imask) >> 1) : -1;
        const int32_t item_next = (cnt > 0 && t1 < n) ? (int32_t)((k_next & v.imask) >> 1) : -1;
        const int32_t chunk_prev_item = (c0 > 0) ? (int32_t)((k_cprev & v.imask) >> 1) : -1;
        if (tid < 2 * G) part_slot[tid] = -1;
        if (tid <= G) { slot_item[tid] = -1; slot_shared[tid] = 0; }
        const int32_t item_first = group_bcast<C>(my_item, 0);
        const int32_t item_last = __shfl(my_item, cnt > 0 ? cnt - 1 : 0, C::LPR);
        if (lane == 0) {
            run_first[group] = cnt > 0 ? item_first : -2;
            run_last[group] = cnt > 0 ? item_last : -2;
        }

        // ---- hop 2: coefficient of entry `lane`, and all row gathers of the run
        const float2 c2 = coef[su_me.x & ~kNegBit];
        const float my_c = (lane < cnt) ? ((su_me.x & kNegBit) ? c2.y : c2.x) : 0.f;
        Row<C> p[RUN];
        if (__all(cnt == RUN)) {        // wave-uniform: every run of this wave is full
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const uint32_t ux = group_bcast<C>(my_su.y, x);
                if constexpr (XH) p[x].load_bf16(reinterpret_cast<const uint16_t *>(P) + (int64_t)ux * d, lane, d);
                else p[x].load(P + (int64_t)ux * d, lane, d);
            }
        } else {
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                const uint32_t ux = group_bcast<C>(my_su.y, x);
                if (x >= cnt) p[x].zero();
                else if constexpr (XH) p[x].load_bf16(reinterpret_cast<const uint16_t *>(P) + (int64_t)ux * d, lane, d);
                else p[x].load(P + (int64_t)ux * d, lane, d);
            }
        }
        __syncthreads();

        if (cnt > 0) {
            const bool cont = (t0 > 0) && (item_prev == item_first);
            int cur_slot = -1;                      // >= 0: the current segment began before this run
            if (cont) {
                if (group == 0) cur_slot = 0;       // inherited from the previous chunk
                else {
                    int gs = group - 1;
                    while (gs > 0 && run_first[gs] == item_first && run_last[gs - 1] == item_first) --gs;
                    // the segment holds the last entry of run gs; it began there unless run 0 is
                    // all this item and the chunk itself continues the previous chunk
                    const bool inherited = (gs == 0) && (run_first[0] == item_first) && (c0 > 0) &&
                                           (chunk_prev_item == item_first);
                    cur_slot = inherited ? 0 : gs + 1;
                }
            }
            int32_t cur_item = item_first;
            Row<C> acc;
            acc.zero();
            float accb = 0.f;
            auto finish = [&](bool ends_here, bool to_next_chunk) {
                if (cur_slot < 0 && ends_here) {    // interior: this group owns gQ[cur_item]
                    acc.store(gQ + (int64_t)cur_item * d, lane, d);
                    if (v.g_bi && lane == 0) v.g_bi[cur_item] = accb;
                } else {                            // crosses a run boundary: LDS slot
                    const int s = (cur_slot >= 0) ? cur_slot : group + 1;
                    // park it: head partial (continued segment) or tail partial
                    const int q = group * 2 + ((cur_slot >= 0) ? 0 : 1);
                    float *dst = part_acc + q * ROWF;
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) dst[k * C::LPR + lane] = acc.v[k];
                    if (lane == 0) {
                        part_slot[q] = s;
                        part_b[q] = accb;
                        slot_item[s] = cur_item;
                        if (to_next_chunk) slot_shared[s] = 1;
                    }
                }
            };
#pragma unroll
            for (int x = 0; x < RUN; ++x) {
                if (x < cnt) {
                    const int32_t it = group_bcast<C>(my_item, x);
                    const float cx = group_bcast<C>(my_c, x);
                    if (it != cur_item) {           // previous segment ended inside this run
                        finish(true, false);
                        cur_item = it;
                        cur_slot = -1;
                        acc.zero();
                        accb = 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < C::NE; ++k) acc.v[k] = fmaf(cx, p[x].v[k], acc.v[k]);
                    accb += cx;
                }
            }
            const bool continues = (t1 < n) && (item_next == cur_item);
            finish(!continues, continues && (group == G - 1));
        }
        __syncthreads();

        if (tid == 0) { edges.item[2 * chunk] = -1; edges.item[2 * chunk + 1] = -1; edges.whole[chunk] = 0; }
        __syncthreads();
        // one write per used slot (G+1 slots over G groups)
        for (int s = group; s <= G; s += G) {
            const int r = slot_item[s];
            if (r < 0) continue;
            Row<C> g;
            g.zero();                               // the parked partials of this slot, in group order
            float gb = 0.f;
            for (int q = 0; q < 2 * G; ++q) {
                if (part_slot[q] != s) continue;
                const float *src = part_acc + q * ROWF;
#pragma unroll
                for (int k = 0; k < C::NE; ++k) g.v[k] += src[k * C::LPR + lane];
                gb += part_b[q];
            }
            const bool from_prev = (s == 0), to_next = slot_shared[s] != 0;
            if (from_prev || to_next) {
                const int64_t e = 2 * chunk + (from_prev ? 0 : 1);
                g.store(edges.vec + e * d, lane, d);
                if (lane == 0) {
                    edges.item[e] = r;
                    edges.b[e] = gb;
                    if (from_prev && to_next) edges.whole[chunk] = 1;
                }
            } else {
                g.store(gQ + (int64_t)r * d, lane, d);
                if (v.g_bi && lane == 0) v.g_bi[r] = gb;
            }
        }
        __syncthreads();   // the slots are reused by the next chunk
    }
}

// chains of edge records - the chunk whose TAIL edge starts a segment owns it and adds the head edges
// of the chunks it runs through, in chunk order (single writer per row, fixed order)
template <class C>
__global__ __launch_bounds__(kBlock) void k_item_edges(ItemEdges edges, int64_t nchunks, int d,
                                                       float *__restrict__ gQ, float *__restrict__ g_bi) {
    if (halted(edges.halt)) return;
    const int lane = threadIdx.x % C::LPR;
    const int group = threadIdx.x / C::LPR;
    const int64_t gstride = (int64_t)gridDim.x * C::GROUPS_PER_BLOCK;
    for (int64_t c = (int64_t)blockIdx.x * C::GROUPS_PER_BLOCK + group; c < nchunks; c += gstride) {
        const int it = edges.item[2 * c + 1];
        if (it < 0) continue;
        Row<C> acc, t;
        acc.load(edges.vec + (2 * c + 1) * d, lane, d);
        float sb = edges.b[2 * c + 1];
        for (int64_t k = c + 1; k < nchunks && edges.item[2 * k] == it; ++k) {
            t.load(edges.vec + (2 * k) * d, lane, d);
#pragma unroll
            for (int q = 0; q < C::NE; ++q) acc.v[q] += t.v[q];
            sb += edges.b[2 * k];
            if (!edges.whole[k]) break;
        }
        acc.store(gQ + (int64_t)it * d, lane, d);
        if (g_bi && lane == 0) g_bi[it] = sb;
    }
}

// both launches of a sum over the 2*v.B entries of `v`, at the row shape's run length RO (0: the default)
template <class C, int RO, bool XH>
static int launch_segsum(const BatchView &v, const float *X, const float2 *coef, int d, float *out,
                          const ItemEdges &ed, float *out_b, hipStream_t s) {
    const int64_t n = 2 * v.B;
    const int64_t nchunks = (n + RunCfg<C, RO>::E - 1) / RunCfg<C, RO>::E;
    hipLaunchKernelGGL((k_item_grad_chunked<C, RO, XH>), dim3(grid_for(n, RunCfg<C, RO>::E, 16384)), dim3(kBlock), 0, s,
                       X, coef, v, d, out, ed);
    hipLaunchKernelGGL((k_item_edges<C>), dim3(grid_for(nchunks, C::GROUPS_PER_BLOCK)), dim3(kBlock), 0, s, ed,
                       nchunks, d, out, out_b);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int64_t segsum_chunks(int64_t n_entries, int d) {
    int64_t nchunks = 0;
    (void)dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        static_assert(RunCfg<C>::E <= RunCfg<C, kSegsumRowsRun<C>>::E, "the default run makes the smaller chunks");
        nchunks = (n_entries + RunCfg<C>::E - 1) / RunCfg<C>::E;
        return DAISY_OK;
    });
    return nchunks;
}

int segsum_rows(const float *X, const float2 *coef, const uint32_t *ekey, const uint2 *esu, int64_t n_entries,
                int d, float *out, float *edge_vec, int32_t *edge_item, float *edge_b, int32_t *edge_whole,
                hipStream_t s, bool x_bf16) {
    if (n_entries <= 0) return DAISY_OK;
    if (n_entries & 1) { set_error("segsum_rows: odd entry count %lld", (long long)n_entries); return DAISY_ERR_ARG; }
    BatchView v{};
    v.ekey = ekey;
    v.esu = esu;
    v.imask = 0xFFFFFFFFu;
    v.B = n_entries / 2;
    const ItemEdges ed{edge_vec, edge_item, edge_b, edge_whole};
    return dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        if (x_bf16) return launch_segsum<C, kSegsumRowsRun<C>, true>(v, X, coef, d, out, ed, nullptr, s);
        return launch_segsum<C, kSegsumRowsRun<C>, false>(v, X, coef, d, out, ed, nullptr, s);
    });
}

int segsum_item_grad(const BatchView &v, const float *P, const float2 *coef, int d, float *gQ, ItemEdges edges,
                     float *g_bi, hipStream_t s) {
    BatchView vv = v;
    vv.g_bi = g_bi;
    edges.halt = v.halt;
    return dispatch_d(d, [&](auto cfg) {
        using C = decltype(cfg);
        return launch_segsum<C, 0, false>(vv, P, coef, d, gQ, edges, g_bi, s);
    });
}

}  // namespace daisy
