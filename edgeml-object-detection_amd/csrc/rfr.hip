// regression.py's RandomForestRegressor(n_estimators, max_depth, min_samples_split), bootstrap on and every
// feature tried at every node (sklearn's defaults), behind fit_model's StandardScaler (edgeml_amd/rfr.py,
// DESIGN.md 6f): every tree of every cross-validation fold in flight, plain launches only, no host round trip
// between the levels.
//
// The bootstrap of a tree reaches it as integer row weights w (drawn on the host from numpy's frozen stream); a
// row with w = 0 does not exist for that tree.  The targets are carried as integers yq = rint((y - F0) 2^q), so
// every weighted sum is an exact int64 and the gain of a candidate split depends on the candidate alone; among
// bit-equal gains the lowest feature wins, then the lowest threshold.  A tree is built level by level and its
// nodes are numbered breadth first: the children of the split nodes of a level get consecutive ids in parent
// order, left then right, by a prefix sum, so the numbering needs no atomics.  The live nodes of a level (those
// no leaf rule has closed yet) are numbered 0 .. live - 1 in id order: a row carries its node's live slot.
//
//   rfr_root_kernel     a workgroup per (fold, tree): the root's count, weighted count, sum and sum of squares,
//                       its record, slot 0 for the in-bag rows.
//   rfr_scan_kernel     one launch per level, a workgroup of four waves per (fold, tree, group of features).  One
//                       wave walks one (fold, feature) list of the training rows in value order (order and values
//                       are streamed and shared by all trees; the row's slot and weight of this tree and the
//                       shared yq are gathered) in chunks of 64 rows.  Per distinct live node of a chunk (the
//                       first remaining lane's node, a ballot of the equal lanes) a 64-lane inclusive scan of w
//                       and w yq gives the exact left sums; the node's running (w_l, c_l, S_l, previous value)
//                       and its best candidate live in LDS, per wave.  A candidate lies between consecutive
//                       in-bag rows a < b of a node with b > a + 1e-7f (float32); gain = diff * diff / (wl * wr),
//                       diff = wr * Sl - wl * Sr, every operation rounded by itself (the file is built with
//                       -ffp-contract=off, the division is IEEE).  The waves' bests are merged under the tie
//                       rule, compared by (gain, feature), so the result does not depend on which wave or group
//                       met which feature.  A level with more live nodes than the LDS holds is scanned in
//                       slices of RFR_SLICE nodes.  A tree with no live node returns at once.
//   rfr_select_kernel   a workgroup per (fold, tree): the groups' bests merged (same rule), the node's record,
//                       the children's ids by a prefix sum over the level's nodes, their count, weighted count
//                       and sum from the split record, the rows moved to their children, the children's sum of
//                       squares (integer atomics: exact in any order), sklearn's leaf rules on the children
//                       (depth, min_samples_split, fewer than 2 rows, impurity <= eps evaluated exactly as
//                       W sum w yq^2 - S^2 <= W^2 2^(2q-52) in 128-bit integers), the next level's live slots.
//   rfr_predict_kernel  a workgroup per feature row: standardise, round to float32, one thread per tree walks it,
//                       one thread adds the leaf values in tree order and divides by the number of trees.
#include <cstdint>

#include "fold_math.hpp"
#include "kernels.hpp"
#include "tree_math.hpp"

namespace edgedet {

constexpr int RFR_NT = 256;
constexpr int RFR_WAVES = RFR_NT / 64;  // one list per wave
constexpr int RFR_SLICE = 128;          // live nodes one scan pass holds in LDS: 56 bytes per wave and node
constexpr int RFR_MAXDEPTH = 64;
constexpr int RFR_MAXGROUPS = 16;
constexpr int RFR_PRED_TREES = 1024;
constexpr int RFR_TIED = 1 << 16;       // a candidate's feature word: feature | RFR_TIED, -1 for none

// --------------------------------------------------------------------------------------- sizes
static int64_t rfr_cap(int64_t n, int max_depth) {
    const int64_t by_rows = 2 * n - 1;
    if (max_depth + 1 >= 40) return by_rows;
    const int64_t by_depth = ((int64_t)1 << (max_depth + 1)) - 1;
    return by_depth < by_rows ? by_depth : by_rows;
}

// the most nodes of one level that are still open: each holds max(2, min_samples_split) in-bag rows or more
static int64_t rfr_maxlive(int64_t n, int max_depth, int mss) {
    int64_t by_rows = n / (mss < 2 ? 2 : mss);
    if (by_rows < 1) by_rows = 1;
    if (max_depth - 1 >= 40) return by_rows;
    const int64_t by_depth = (int64_t)1 << (max_depth - 1);
    return by_depth < by_rows ? by_depth : by_rows;
}

struct RfrWs {
    int32_t *slot, *nW, *nslot, *slot_node, *live, *cwl, *ccl, *cf;
    int64_t *nS, *cS;
    gu64* nQ;
    double *cg, *ct;
    int64_t bytes;
};

// rows: slots (rows of all folds times trees); nodes: node records (trees times cap); lives: trees times maxlive
static RfrWs rfr_ws(void* base, int64_t rows, int64_t trees, int64_t nodes, int64_t lives, int64_t groups,
                    bool node_stats) {
    RfrWs w;
    char* p = (char*)base;
    auto take = [&](int64_t bytes) {
        char* r = p;
        p += (bytes + 7) / 8 * 8;
        return r;
    };
    const int64_t cand = lives * groups;
    w.nQ = (gu64*)take(nodes * 4 * 8);
    w.nS = (int64_t*)take(node_stats ? nodes * 8 : 0);
    w.cS = (int64_t*)take(cand * 8);
    w.cg = (double*)take(cand * 8);
    w.ct = (double*)take(cand * 8);
    w.slot = (int32_t*)take(rows * 4);
    w.nW = (int32_t*)take(node_stats ? nodes * 4 : 0);
    w.nslot = (int32_t*)take(nodes * 4);
    w.slot_node = (int32_t*)take(lives * 4);
    w.live = (int32_t*)take(trees * 4);
    w.cwl = (int32_t*)take(cand * 4);
    w.ccl = (int32_t*)take(cand * 4);
    w.cf = (int32_t*)take(cand * 4);
    w.bytes = (int64_t)(p - (char*)base);
    return w;
}

struct RfrCand {  // the best candidates of a level: [tree][group][live slot]
    double *gain, *thr;
    int64_t* Sl;
    int32_t *wl, *cl, *feat;
};

struct RfrTree {  // one fit's tree arrays [F][T][cap], node_count [F][T], tied [F], status [F]
    int16_t* feature;
    double* threshold;
    int32_t* left;
    double* value;
    int32_t* nsamp;
    int32_t* node_count;
    int32_t* tied;
    int32_t* status;
};

struct RfrBest {
    double gain, thr;
    int64_t Sl;
    int wl, cl, feat;  // feat: feature | RFR_TIED, -1 for none
};

// b joins a under the tie rule: the greater gain; among equal gains the lower feature, and the node counts as tied
__device__ __forceinline__ void rfr_join(RfrBest& a, const RfrBest& b) {
    if (b.feat < 0) return;
    if (b.gain > a.gain) {
        a = b;
    } else if (b.gain == a.gain) {
        if ((b.feat & 0xffff) < (a.feat & 0xffff)) a = b;
        a.feat |= RFR_TIED;
    }
}

__device__ __forceinline__ RfrBest rfr_merge_groups(const RfrCand& c, int64_t tree, int G, int64_t maxlive, int s) {
    RfrBest a = {-1.0, 0.0, 0, 0, 0, -1};
    for (int g = 0; g < G; ++g) {
        const int64_t i = (tree * G + g) * maxlive + s;
        const RfrBest b = {c.gain[i], c.thr[i], c.Sl[i], c.wl[i], c.cl[i], c.feat[i]};
        rfr_join(a, b);
    }
    return a;
}

// w r^2 into the four limb accumulators of one node, in global memory: integer sums, exact in any order
__device__ __forceinline__ void rfr_acc_sq(gu64* Q4, int wt, int64_t r) {
    gu64 limb[4];
    tree_sq_limbs(r, limb);
    for (int i = 0; i < 4; ++i) atomicAdd(&Q4[i], (gu64)wt * limb[i]);
}

__device__ __forceinline__ bool rfr_pure(int W, int64_t S, gu64* Q4, int q) {
    gu64 Q[4];  // written by other waves' atomics: read past the vector cache
    for (int i = 0; i < 4; ++i) Q[i] = __hip_atomic_load(&Q4[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return tree_pure(W, S, Q, q);
}

// exclusive prefix count of flag over the workgroup's threads, and the total; every thread calls it
__device__ __forceinline__ int rfr_block_rank(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gu64 m = __ballot(flag);
    const int within = __popcll(m & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
    __syncthreads();
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < RFR_WAVES; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    return before + within;
}

// ------------------------------------------------------------------------------------------ root
__global__ void __launch_bounds__(RFR_NT) rfr_root_kernel(int T, int mss, int64_t cap, int64_t maxlive,
                                                          const int64_t* __restrict__ tr_off,
                                                          const int32_t* __restrict__ qv,
                                                          const double* __restrict__ init,
                                                          const uint8_t* __restrict__ w,
                                                          const int64_t* __restrict__ yq, int32_t* slot, int32_t* live,
                                                          int32_t* slot_node, int32_t* nW, int64_t* nS, gu64* nQ,
                                                          RfrTree tr) {
    __shared__ gu64 sS, sQ[4];
    __shared__ int sc, sW, open;
    const int tid = threadIdx.x;
    const int64_t ft = blockIdx.x;
    const int f = (int)(ft / T), t = (int)(ft % T);
    const int64_t off = tr_off[f], n = tr_off[f + 1] - off, rb = off * T + (int64_t)t * n, nb = ft * cap;
    if (tid == 0) {
        sS = 0;
        sc = 0;
        sW = 0;
    }
    if (tid < 4) sQ[tid] = 0;
    __syncthreads();
    for (int64_t p = tid; p < n; p += RFR_NT) {
        const int wt = w[rb + p];
        slot[rb + p] = wt > 0 ? 0 : -1;
        if (wt == 0) continue;
        const int64_t r = yq[off + p];
        gu64 limb[4];
        tree_sq_limbs(r, limb);
        atomicAdd(&sc, 1);
        atomicAdd(&sW, wt);
        atomicAdd(&sS, (gu64)((int64_t)wt * r));
        for (int i = 0; i < 4; ++i) atomicAdd(&sQ[i], (gu64)wt * limb[i]);
    }
    __syncthreads();
    if (tid == 0) {
        const int W = sW, cnt = sc, q = qv[f];
        const int64_t S = (int64_t)sS;
        gu64 Q[4] = {sQ[0], sQ[1], sQ[2], sQ[3]};
        nW[nb] = W;
        nS[nb] = S;
        for (int i = 0; i < 4; ++i) nQ[nb * 4 + i] = Q[i];
        tr.nsamp[nb] = cnt;
        tr.value[nb] = W > 0 ? init[f] + ((double)S / (double)W) * ldexp(1.0, -q) : 0.0;
        tr.node_count[ft] = 1;
        open = cnt >= mss && cnt >= 2 && !tree_pure(W, S, Q, q) ? 1 : 0;
        live[ft] = open;
        slot_node[ft * maxlive] = 0;
    }
    __syncthreads();
    if (open) return;
    for (int64_t p = tid; p < n; p += RFR_NT) slot[rb + p] = -1;
}

// ------------------------------------------------------------------------------------------ scan
__global__ void __launch_bounds__(RFR_NT) rfr_scan_kernel(int D, int T, int G, int64_t maxlive, int64_t cap,
                                                          const int32_t* __restrict__ ord,
                                                          const float* __restrict__ sv,
                                                          const int64_t* __restrict__ tr_off, int64_t n1,
                                                          const uint8_t* __restrict__ w,
                                                          const int64_t* __restrict__ yq,
                                                          const int32_t* __restrict__ slot,
                                                          const int32_t* __restrict__ live,
                                                          const int32_t* __restrict__ slot_node,
                                                          const int32_t* __restrict__ nW,
                                                          const int64_t* __restrict__ nS, RfrCand out) {
    __shared__ int tW[RFR_SLICE];
    __shared__ int64_t tS[RFR_SLICE];
    // per wave: a node's running left sums along the list being walked, and its best candidate so far.  Lanes
    // of one wave hand these to each other between iterations, in program order: volatile keeps every access.
    __shared__ volatile int rwl[RFR_WAVES][RFR_SLICE], rcl[RFR_WAVES][RFR_SLICE];
    __shared__ volatile int64_t rSl[RFR_WAVES][RFR_SLICE];
    __shared__ volatile float rpv[RFR_WAVES][RFR_SLICE];
    __shared__ volatile double bg[RFR_WAVES][RFR_SLICE], bt[RFR_WAVES][RFR_SLICE];
    __shared__ volatile int64_t bS[RFR_WAVES][RFR_SLICE];
    __shared__ volatile int bwl[RFR_WAVES][RFR_SLICE], bcl[RFR_WAVES][RFR_SLICE], bf[RFR_WAVES][RFR_SLICE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ft = blockIdx.x;
    const int g = blockIdx.y;
    int nl = live[ft];
    if (nl <= 0) return;  // uniform: the tree is finished
    if (nl > maxlive) nl = (int)maxlive;
    const int f = (int)(ft / T), t = (int)(ft % T);
    const int64_t off = tr_off ? tr_off[f] : 0;
    const int n = (int)(tr_off ? tr_off[f + 1] - off : n1);
    const int64_t rb = off * T + (int64_t)t * n, nb = ft * cap;
    const int Dg = (D + G - 1) / G, j0 = g * Dg, j1 = j0 + Dg < D ? j0 + Dg : D;
    const int chunks = (n + 63) / 64;
    const gu64 below_me = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int s0 = 0; s0 < nl; s0 += RFR_SLICE) {
        const int ns = nl - s0 < RFR_SLICE ? nl - s0 : RFR_SLICE;
        __syncthreads();  // the merge of the slice before has read the bests
        for (int i = tid; i < ns; i += RFR_NT) {
            const int id = slot_node[ft * maxlive + s0 + i];
            tW[i] = nW[nb + id];
            tS[i] = nS[nb + id];
        }
        for (int i = lane; i < ns; i += 64) {
            bg[wave][i] = -1.0;
            bt[wave][i] = 0.0;
            bS[wave][i] = 0;
            bwl[wave][i] = 0;
            bcl[wave][i] = 0;
            bf[wave][i] = -1;
        }
        __syncthreads();
        for (int j = j0 + wave; j < j1; j += RFR_WAVES) {
            for (int i = lane; i < ns; i += 64) {
                rwl[wave][i] = 0;
                rcl[wave][i] = 0;
                rSl[wave][i] = 0;
                rpv[wave][i] = 0.f;
            }
            const int32_t* o = ord + off * D + (int64_t)j * n;
            const float* s = sv + off * D + (int64_t)j * n;
            for (int c = 0; c < chunks; ++c) {
                const int i = c * 64 + lane;
                const bool act = i < n;
                const int p = act ? o[i] : 0;
                const float v = act ? s[i] : 0.f;
                const int sl = act ? slot[rb + p] - s0 : -1;
                const int wt = sl >= 0 && sl < ns ? (int)w[rb + p] : 0;
                const bool in = wt > 0;
                gu64 remaining = __ballot(in);
                if (remaining == 0) continue;  // uniform
                const int64_t x = in ? (int64_t)wt * yq[off + p] : 0;
                while (remaining) {  // uniform: one round per distinct node of the chunk
                    const int m = __shfl(sl, __ffsll((long long)remaining) - 1);
                    const bool flag = in && sl == m;
                    const gu64 mask = __ballot(flag);
                    remaining &= ~mask;
                    const int mw = flag ? wt : 0;
                    const int64_t mx = flag ? x : 0;
                    int cw = mw;
                    int64_t cx = mx;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int uw = __shfl_up(cw, d);
                        const int64_t ux = __shfl_up(cx, d);
                        if (lane >= d) {
                            cw += uw;
                            cx += ux;
                        }
                    }
                    const gu64 below = mask & below_me;
                    const int prev = below ? 63 - __clzll((long long)below) : 0;
                    float a = __shfl(v, prev);
                    const int r_wl = rwl[wave][m], r_cl = rcl[wave][m];
                    const int64_t r_Sl = rSl[wave][m];
                    if (!below) a = rpv[wave][m];
                    const int cl = r_cl + __popcll(below), wl = r_wl + (cw - mw);
                    const int64_t Sl = r_Sl + (cx - mx);
                    double gain = -1.0;
                    if (flag && cl > 0 && v > a + 1e-7f) {
                        const int wr = tW[m] - wl;
                        const int64_t Sr = tS[m] - Sl;
                        const double diff = (double)wr * (double)Sl - (double)wl * (double)Sr;
                        gain = diff * diff / ((double)wl * (double)wr);
                    }
                    double gm = gain;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) gm = fmax(gm, __shfl_xor(gm, d));
                    if (gm >= 0.0) {  // uniform; the lowest lane at the maximum holds the lowest threshold
                        const gu64 win = __ballot(gain == gm);
                        if (lane == __ffsll((long long)win) - 1) {
                            const double have = bg[wave][m];
                            if (gm > have) {
                                bg[wave][m] = gm;
                                bt[wave][m] = (double)a / 2.0 + (double)v / 2.0;
                                bS[wave][m] = Sl;
                                bwl[wave][m] = wl;
                                bcl[wave][m] = cl;
                                bf[wave][m] = j;
                            } else if (gm == have && (bf[wave][m] & 0xffff) != j) {
                                bf[wave][m] = bf[wave][m] | RFR_TIED;
                            }
                        }
                    }
                    if (lane == 63 - __clzll((long long)mask)) {  // the node's last row of the chunk
                        rwl[wave][m] = r_wl + cw;
                        rcl[wave][m] = cl + 1;
                        rSl[wave][m] = r_Sl + cx;
                        rpv[wave][m] = v;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < ns; i += RFR_NT) {
            RfrBest a = {-1.0, 0.0, 0, 0, 0, -1};
            for (int k = 0; k < RFR_WAVES; ++k) {
                const RfrBest b = {bg[k][i], bt[k][i], bS[k][i], bwl[k][i], bcl[k][i], bf[k][i]};
                rfr_join(a, b);
            }
            const int64_t c = (ft * G + g) * maxlive + s0 + i;
            out.gain[c] = a.gain;
            out.thr[c] = a.thr;
            out.Sl[c] = a.Sl;
            out.wl[c] = a.wl;
            out.cl[c] = a.cl;
            out.feat[c] = a.feat;
        }
    }
}

// ---------------------------------------------------------------------------------------- select
__global__ void __launch_bounds__(RFR_NT) rfr_select_kernel(int level, int max_depth, int mss, int D, int64_t N, int T,
                                                            int G, int64_t maxlive, int64_t cap,
                                                            const float* __restrict__ z32,
                                                            const int32_t* __restrict__ tr_idx,
                                                            const int64_t* __restrict__ tr_off,
                                                            const int32_t* __restrict__ qv,
                                                            const double* __restrict__ init,
                                                            const uint8_t* __restrict__ w,
                                                            const int64_t* __restrict__ yq, int32_t* slot,
                                                            int32_t* live, int32_t* slot_node, int32_t* nW, int64_t* nS,
                                                            gu64* nQ, int32_t* nslot, RfrCand cand, RfrTree tr) {
    __shared__ int wsum[RFR_WAVES];
    const int tid = threadIdx.x;
    const int64_t ft = blockIdx.x;
    int nl = live[ft];
    if (nl <= 0) return;  // uniform: the tree is finished
    if (nl > maxlive) nl = (int)maxlive;
    const int f = (int)(ft / T), t = (int)(ft % T);
    const int64_t off = tr_off[f], n = tr_off[f + 1] - off, rb = off * T + (int64_t)t * n, nb = ft * cap;
    const int q = qv[f];
    const double unq = ldexp(1.0, -q), F0 = init[f];
    const int first = tr.node_count[ft];  // the first child's id
    __syncthreads();                      // everyone has read what thread 0 rewrites at the end
    // the records of the level's live nodes, and their children's
    int splits = 0, tied = 0;
    for (int b = 0; b < nl; b += RFR_NT) {
        const int s = b + tid;
        RfrBest best = {-1.0, 0.0, 0, 0, 0, -1};
        if (s < nl) best = rfr_merge_groups(cand, ft, G, maxlive, s);
        int total;
        const int rank = rfr_block_rank(best.feat >= 0, wsum, total);
        if (best.feat >= 0) {
            const int id = slot_node[ft * maxlive + s];
            const int64_t l = (int64_t)first + 2 * (int64_t)(splits + rank);
            if (l + 1 >= cap) {  // cannot happen: a tree on n rows has at most 2 n - 1 nodes
                atomicMax(&tr.status[f], 1);
            } else {
                tr.feature[nb + id] = (int16_t)(best.feat & 0xffff);
                tr.threshold[nb + id] = best.thr;
                tr.left[nb + id] = (int32_t)l;
                if (best.feat & RFR_TIED) ++tied;
                const int cc[2] = {best.cl, tr.nsamp[nb + id] - best.cl};
                const int cW[2] = {best.wl, nW[nb + id] - best.wl};
                const int64_t cS[2] = {best.Sl, nS[nb + id] - best.Sl};
                for (int k = 0; k < 2; ++k) {
                    tr.nsamp[nb + l + k] = cc[k];
                    nW[nb + l + k] = cW[k];
                    nS[nb + l + k] = cS[k];
                    for (int i = 0; i < 4; ++i) nQ[(nb + l + k) * 4 + i] = 0;
                    tr.value[nb + l + k] = F0 + ((double)cS[k] / (double)cW[k]) * unq;
                }
            }
        }
        splits += total;
    }
    if (tied > 0) atomicAdd(&tr.tied[f], tied);
    const int children = 2 * splits;
    __syncthreads();
    if (children == 0 || (int64_t)first + children > cap) {  // uniform
        if (tid == 0) live[ft] = 0;
        return;
    }
    // the rows move to their children (slot holds the child's id for a moment) and add to its sum of squares
    for (int64_t p = tid; p < n; p += RFR_NT) {
        const int s = slot[rb + p];
        if (s < 0) continue;
        const int id = slot_node[ft * maxlive + s];
        const int fe = tr.feature[nb + id];
        if (fe < 0) {
            slot[rb + p] = -1;
            continue;
        }
        const float z = z32[((int64_t)f * N + tr_idx[off + p]) * D + fe];
        const int child = tr.left[nb + id] + ((double)z > tr.threshold[nb + id] ? 1 : 0);
        slot[rb + p] = child;
        rfr_acc_sq(&nQ[(nb + child) * 4], (int)w[rb + p], yq[off + p]);
    }
    __syncthreads();
    // the leaf rules on the children; the open ones get the next level's live slots, in id order
    int open = 0;
    for (int b = 0; b < children; b += RFR_NT) {
        const int c = b + tid;
        const int64_t id = (int64_t)first + c;
        bool alive = false;
        if (c < children) {
            const int cnt = tr.nsamp[nb + id];
            alive = level + 1 < max_depth && cnt >= mss && cnt >= 2 && !rfr_pure(nW[nb + id], nS[nb + id], &nQ[(nb + id) * 4], q);
        }
        int total;
        const int rank = rfr_block_rank(alive, wsum, total);
        if (c < children) {
            int s = alive ? open + rank : -1;
            if (s >= maxlive) {  // cannot happen: every open node holds max(2, min_samples_split) rows
                atomicMax(&tr.status[f], 2);
                s = -1;
            }
            nslot[nb + id] = s;
            if (s >= 0) slot_node[ft * maxlive + s] = (int32_t)id;
        }
        open += total;
    }
    __syncthreads();
    for (int64_t p = tid; p < n; p += RFR_NT) {
        const int child = slot[rb + p];
        if (child >= 0) slot[rb + p] = nslot[nb + child];
    }
    if (tid == 0) {
        tr.node_count[ft] = first + children;
        live[ft] = open < maxlive ? open : (int)maxlive;
    }
}

// ------------------------------------------------------------------------------- the unit export
// the nodes' count, weighted count, sum and sum of squares for a given map of rows to nodes: node id = slot
__global__ void __launch_bounds__(RFR_NT) rfr_unit_stats_kernel(int64_t n, int nn, const uint8_t* __restrict__ w,
                                                                const int64_t* __restrict__ yq,
                                                                const int32_t* __restrict__ slot, int32_t* cnt,
                                                                int32_t* nW, int64_t* nS, gu64* nQ, int32_t* live,
                                                                int32_t* slot_node) {
    const int64_t p = (int64_t)blockIdx.x * RFR_NT + threadIdx.x;
    if (blockIdx.x == 0) {
        for (int s = threadIdx.x; s < nn; s += RFR_NT) slot_node[s] = s;
        if (threadIdx.x == 0) live[0] = nn;
    }
    if (p >= n) return;
    const int s = slot[p], wt = w[p];
    if (s < 0 || s >= nn || wt == 0) return;
    atomicAdd(&cnt[s], 1);
    atomicAdd(&nW[s], wt);
    atomicAdd((gu64*)&nS[s], (gu64)((int64_t)wt * yq[p]));
    rfr_acc_sq(&nQ[(int64_t)s * 4], wt, yq[p]);
}

struct RfrRec {  // the unit export's records [nn]
    int32_t* feature;
    double *threshold, *gain;
    int32_t *wl, *cl;
    int64_t* Sl;
    int32_t *leaf, *tied;
};

__global__ void __launch_bounds__(RFR_NT) rfr_record_kernel(int nn, int G, int mss, int q,
                                                            const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ nW,
                                                            const int64_t* __restrict__ nS, gu64* nQ, RfrCand cand,
                                                            RfrRec rec) {
    const int s = blockIdx.x * RFR_NT + threadIdx.x;
    if (s >= nn) return;
    const RfrBest b = rfr_merge_groups(cand, 0, G, nn, s);
    const bool found = b.feat >= 0;
    const bool closed = cnt[s] < 2 || cnt[s] < mss || rfr_pure(nW[s], nS[s], &nQ[(int64_t)s * 4], q);
    rec.feature[s] = found ? (b.feat & 0xffff) : -1;
    rec.threshold[s] = found ? b.thr : 0.0;
    rec.gain[s] = found ? b.gain : -1.0;
    rec.wl[s] = found ? b.wl : 0;
    rec.cl[s] = found ? b.cl : 0;
    rec.Sl[s] = found ? b.Sl : 0;
    rec.leaf[s] = !found || closed ? 1 : 0;
    rec.tied[s] = found && (b.feat & RFR_TIED) ? 1 : 0;
}

// --------------------------------------------------------------------------------------- predict
__global__ void __launch_bounds__(RFR_NT) rfr_predict_kernel(const double* __restrict__ feat, int D,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ scale,
                                                             const int16_t* __restrict__ feature,
                                                             const double* __restrict__ threshold,
                                                             const int32_t* __restrict__ left,
                                                             const double* __restrict__ value, int T, int64_t cap,
                                                             double* __restrict__ est) {
    __shared__ float z[FOLD_MAXD];
    __shared__ double leafv[RFR_PRED_TREES];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < D) z[tid] = (float)((feat[b * D + tid] - mean[tid]) / scale[tid]);
    __syncthreads();
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += RFR_PRED_TREES) {
        const int cnt = T - t0 < RFR_PRED_TREES ? T - t0 : RFR_PRED_TREES;
        for (int i = tid; i < cnt; i += RFR_NT) {
            const int64_t tb = (int64_t)(t0 + i) * cap;
            int64_t idx = 0;
            for (int64_t step = 0; step < cap; ++step) {  // a child's id exceeds its parent's: at most cap steps
                const int fe = feature[tb + idx];
                if (fe < 0 || fe >= D) break;
                const int64_t nx = (int64_t)left[tb + idx] + ((double)z[fe] > threshold[tb + idx] ? 1 : 0);
                if (nx <= idx || nx >= cap) break;
                idx = nx;
            }
            leafv[i] = value[tb + idx];
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < cnt; ++i) acc = acc + leafv[i];  // tree order
        __syncthreads();
    }
    if (tid == 0) est[b] = acc / (double)T;
}

static bool rfr_opts_ok(int32_t T, int32_t max_depth, int32_t mss, int32_t groups) {
    return T >= 1 && max_depth >= 1 && max_depth <= RFR_MAXDEPTH && mss >= 2 && groups >= 1 && groups <= RFR_MAXGROUPS;
}

static int64_t rfr_max_rows(const int64_t* tr_off_host, int32_t folds) {
    int64_t m = 0;
    for (int f = 0; f < folds; ++f) m = tr_off_host[f + 1] - tr_off_host[f] > m ? tr_off_host[f + 1] - tr_off_host[f] : m;
    return m;
}

}  // namespace edgedet

using namespace edgedet;

// ------------------------------------------------------------------------------------- the C-ABI
extern "C" int64_t edgedet_rfr_node_cap(int64_t n, int32_t max_depth) {
    if (n < 1 || n >= ((int64_t)1 << 30) || max_depth < 1 || max_depth > RFR_MAXDEPTH) return -1;
    return rfr_cap(n, max_depth);
}

extern "C" int64_t edgedet_rfr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D, int32_t T,
                                              int32_t max_depth, int32_t min_samples_split, int32_t groups) {
    if (!folds_ok(tr_off_host, folds, 0, true, (1 << 30) - 1) || !fold_dims_ok(D) ||
        !rfr_opts_ok(T, max_depth, min_samples_split, groups))
        return -1;
    const int64_t nmax = rfr_max_rows(tr_off_host, folds), trees = (int64_t)folds * T;
    return rfr_ws(nullptr, tr_off_host[folds] * T, trees, trees * rfr_cap(nmax, max_depth),
                  trees * rfr_maxlive(nmax, max_depth, min_samples_split), groups, true)
        .bytes;
}

extern "C" int64_t edgedet_rfr_best_split_workspace_size(int64_t n, int64_t D, int32_t nn, int32_t groups) {
    if (n < 1 || n >= ((int64_t)1 << 30) || !fold_dims_ok(D) || nn < 1 || nn > (1 << 20) || groups < 1 ||
        groups > RFR_MAXGROUPS)
        return -1;
    return rfr_ws(nullptr, 0, 1, nn, nn, groups, false).bytes;
}

extern "C" int edgedet_rfr_fit(const float* z32, int64_t N, int64_t D, const double* x, const double* mean,
                               const double* scale, const int32_t* tr_idx, const int32_t* ord, const float* sorted,
                               const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* init,
                               const int32_t* q_host, const int32_t* q, const uint8_t* w, const int64_t* yq, int32_t T,
                               int32_t max_depth, int32_t min_samples_split, int32_t groups, void* ws,
                               int64_t ws_bytes, int16_t* feature, double* threshold, int32_t* left, double* value,
                               int32_t* n_node_samples, int32_t* node_count, int32_t* tied, int32_t* status,
                               double* est, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && N < ((int64_t)1 << 30),
                    "rfr_fit: 1 <= features <= 255, 1 <= rows < 2^30");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, 0, true, (1 << 30) - 1),
                    "rfr_fit: every fold needs 1 to 2^30 - 1 training rows");
    EDGEDET_REQUIRE(rfr_opts_ok(T, max_depth, min_samples_split, groups),
                    "rfr_fit: n_estimators >= 1, 1 <= max_depth <= 64, min_samples_split >= 2, 1 <= groups <= 16");
    EDGEDET_REQUIRE(z32 && x && mean && scale && tr_idx && ord && sorted && tr_off && init && q_host && q && w && yq &&
                        ws && feature && threshold && left && value && n_node_samples && node_count && tied &&
                        status && est,
                    "rfr_fit: null pointer");
    for (int f = 0; f < folds; ++f)
        EDGEDET_REQUIRE(q_host[f] >= TREE_QMIN && q_host[f] <= TREE_QMAX, "rfr_fit: 26 <= q <= 1000");
    const int64_t nmax = rfr_max_rows(tr_off_host, folds), trees = (int64_t)folds * T;
    const int64_t cap = rfr_cap(nmax, max_depth), maxlive = rfr_maxlive(nmax, max_depth, min_samples_split);
    EDGEDET_REQUIRE(trees < ((int64_t)1 << 31) && trees * cap < ((int64_t)1 << 40), "rfr_fit: too many trees");
    const RfrWs s = rfr_ws(ws, tr_off_host[folds] * T, trees, trees * cap, trees * maxlive, groups, true);
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= s.bytes,
                    "rfr_fit: workspace smaller than edgedet_rfr_workspace_size, or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t nodes = (size_t)(trees * cap);
    EDGEDET_CHECK_HIP(hipMemsetAsync(feature, 0xff, nodes * 2, st));  // -1: a leaf
    EDGEDET_CHECK_HIP(hipMemsetAsync(left, 0xff, nodes * 4, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(threshold, 0, nodes * 8, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(value, 0, nodes * 8, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(n_node_samples, 0, nodes * 4, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(tied, 0, (size_t)folds * 4, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)folds * 4, st));
    const RfrTree tr = {feature, threshold, left, value, n_node_samples, node_count, tied, status};
    const RfrCand cand = {s.cg, s.ct, s.cS, s.cwl, s.ccl, s.cf};
    const dim3 block(RFR_NT), per_tree((unsigned)trees), scan((unsigned)trees, (unsigned)groups);
    hipLaunchKernelGGL(rfr_root_kernel, per_tree, block, 0, st, (int)T, (int)min_samples_split, cap, maxlive, tr_off, q,
                       init, w, yq, s.slot, s.live, s.slot_node, s.nW, s.nS, s.nQ, tr);
    EDGEDET_LAUNCH_CHECK();
    for (int level = 0; level < max_depth; ++level) {
        hipLaunchKernelGGL(rfr_scan_kernel, scan, block, 0, st, (int)D, (int)T, (int)groups, maxlive, cap, ord, sorted,
                           tr_off, (int64_t)0, w, yq, s.slot, s.live, s.slot_node, s.nW, s.nS, cand);
        EDGEDET_LAUNCH_CHECK();
        hipLaunchKernelGGL(rfr_select_kernel, per_tree, block, 0, st, level, (int)max_depth, (int)min_samples_split,
                           (int)D, N, (int)T, (int)groups, maxlive, cap, z32, tr_idx, tr_off, q, init, w, yq, s.slot,
                           s.live, s.slot_node, s.nW, s.nS, s.nQ, s.nslot, cand, tr);
        EDGEDET_LAUNCH_CHECK();
    }
    for (int f = 0; f < folds; ++f) {
        const int64_t tb = (int64_t)f * T * cap;
        hipLaunchKernelGGL(rfr_predict_kernel, dim3((unsigned)N), block, 0, st, x, (int)D, mean + (int64_t)f * D,
                           scale + (int64_t)f * D, feature + tb, threshold + tb, left + tb, value + tb, (int)T, cap,
                           est + (int64_t)f * N);
        EDGEDET_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int edgedet_rfr_best_split(const int32_t* ord, const float* sorted, int64_t n, int64_t D,
                                      const int32_t* slot, const uint8_t* w, const int64_t* yq, int32_t nn, int32_t q,
                                      int32_t min_samples_split, int32_t groups, void* ws, int64_t ws_bytes,
                                      int32_t* cnt, int32_t* W, int64_t* S, int32_t* feature, double* threshold,
                                      double* gain, int32_t* wl, int32_t* cl, int64_t* Sl, int32_t* leaf,
                                      int32_t* tied, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && n >= 1 && n < ((int64_t)1 << 30),
                    "rfr_best_split: 1 <= features <= 255, 1 <= rows < 2^30");
    EDGEDET_REQUIRE(nn >= 1 && nn <= (1 << 20) && min_samples_split >= 2 && groups >= 1 && groups <= RFR_MAXGROUPS,
                    "rfr_best_split: 1 <= nodes <= 2^20, min_samples_split >= 2, 1 <= groups <= 16");
    EDGEDET_REQUIRE(q >= TREE_QMIN && q <= TREE_QMAX, "rfr_best_split: 26 <= q <= 1000");
    EDGEDET_REQUIRE(ord && sorted && slot && w && yq && ws && cnt && W && S && feature && threshold && gain && wl &&
                        cl && Sl && leaf && tied,
                    "rfr_best_split: null pointer");
    const RfrWs s = rfr_ws(ws, 0, 1, nn, nn, groups, false);
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= s.bytes,
                    "rfr_best_split: workspace smaller than edgedet_rfr_best_split_workspace_size, or not 8-byte "
                    "aligned");
    hipStream_t st = (hipStream_t)stream;
    EDGEDET_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)nn * 4, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(W, 0, (size_t)nn * 4, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(S, 0, (size_t)nn * 8, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(s.nQ, 0, (size_t)nn * 32, st));
    const dim3 block(RFR_NT);
    hipLaunchKernelGGL(rfr_unit_stats_kernel, dim3((unsigned)cdiv(n, RFR_NT)), block, 0, st, n, (int)nn, w, yq, slot,
                       cnt, W, S, s.nQ, s.live, s.slot_node);
    EDGEDET_LAUNCH_CHECK();
    const RfrCand cand = {s.cg, s.ct, s.cS, s.cwl, s.ccl, s.cf};
    hipLaunchKernelGGL(rfr_scan_kernel, dim3(1, (unsigned)groups), block, 0, st, (int)D, 1, (int)groups, (int64_t)nn,
                       (int64_t)nn, ord, sorted, (const int64_t*)nullptr, n, w, yq, slot, s.live, s.slot_node, W, S,
                       cand);
    EDGEDET_LAUNCH_CHECK();
    const RfrRec rec = {feature, threshold, gain, wl, cl, Sl, leaf, tied};
    hipLaunchKernelGGL(rfr_record_kernel, dim3((unsigned)cdiv(nn, RFR_NT)), block, 0, st, (int)nn, (int)groups,
                       (int)min_samples_split, (int)q, cnt, W, S, s.nQ, cand, rec);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_rfr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean,
                                         const double* scale, const int16_t* feature, const double* threshold,
                                         const int32_t* left, const double* value, int32_t T, int64_t cap,
                                         double* est, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && B >= 1 && B < ((int64_t)1 << 31),
                    "rfr_model_predict: 1 <= features <= 255, 1 <= rows < 2^31");
    EDGEDET_REQUIRE(T >= 1 && cap >= 1 && cap < ((int64_t)1 << 31), "rfr_model_predict: n_estimators >= 1, 1 <= cap < 2^31");
    EDGEDET_REQUIRE(feat && mean && scale && feature && threshold && left && value && est,
                    "rfr_model_predict: null pointer");
    hipLaunchKernelGGL(rfr_predict_kernel, dim3((unsigned)B), dim3(RFR_NT), 0, (hipStream_t)stream, feat, (int)D, mean,
                       scale, feature, threshold, left, value, (int)T, cap, est);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
