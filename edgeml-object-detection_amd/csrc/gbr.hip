// regression.py's GradientBoostingRegressor(learning_rate, n_estimators, subsample=1.0), max_depth <= 4,
// criterion friedman_mse, behind fit_model's StandardScaler (edgeml_amd/gbr.py): every
// cross-validation fold in flight, plain launches only, no host round trip between stages.
//
// What makes the fit reproducible bit for bit, on any grid and in any order of summation: the residuals of a
// stage are carried as integers rq = rint(r 2^q), so every residual sum is an exact int64 and the gain of a
// candidate split depends on the candidate alone; among bit-equal gains the lowest feature wins, then the
// lowest threshold.
//
//   gbr_prepare_kernel  z32 [F][N][D] = float((x - mean) / scale), a true float64 division: sklearn's trees
//                       see float32.
//   gbr_scan_kernel     one launch per tree level; a workgroup of eight waves per (fold, feature) list of the
//                       training rows in value order (order and values are streamed, the row's node and rq
//                       gathered), each wave on its own run of the list, started from the exact totals of the
//                       runs before it.  Per chunk of 64 rows and live node: a ballot picks the node's
//                       lanes, a 64-lane inclusive scan gives the exact left sum, the ballot's lower bits the
//                       left count and the lane of the previous row of the node.  A candidate lies
//                       between two consecutive rows a < b of a node with b > a + 1e-7f (float32); gain =
//                       diff * diff / (wl * wr), diff = wr * Sl - wl * Sr, every operation rounded by itself
//                       (the file is built with -ffp-contract=off, the division is IEEE).  Per (fold, node,
//                       feature) the greatest gain, the lowest threshold among equals.
//   gbr_select_kernel   a workgroup per fold: per live node the arg-best over the features (lowest feature
//                       among bit-equal gains), sklearn's leaf rules (fewer than 2 rows, no valid candidate,
//                       impurity <= eps evaluated exactly as n sum rq^2 - S^2 <= n^2 2^(2q-52) in 128-bit
//                       integers), the node's record in heap layout, the rows moved to their children, the
//                       children's count, sum and sum of squares; after the last level the children's values.
//   gbr_update_kernel   after the last level: every row of the dataset walks the new tree, F += lr * value
//                       (product and sum rounded separately); the training rows' next rq, the root's sums.
//   gbr_predict_kernel  a workgroup per feature row: standardise, round to float32, the leaf values of the
//                       stages gathered in parallel, lr * value added to init in stage order by one thread.
#include <cstdint>

#include "fold_math.hpp"
#include "kernels.hpp"
#include "tree_math.hpp"

namespace edgedet {

constexpr int GBR_NT = 256;
constexpr int GBR_SCAN_W = 8;     // waves that share one (fold, feature) list
constexpr int GBR_SCAN_NT = 64 * GBR_SCAN_W;
constexpr int GBR_NODES = 8;      // live nodes of one scanned level: depth <= 4
constexpr int GBR_MAXDEPTH = 4;
constexpr int GBR_PRED_STAGES = 1024;
constexpr int GBR_QMIN = TREE_QMIN, GBR_QMAX = TREE_QMAX;
constexpr uint8_t GBR_DEAD = 255;  // a training row that sits in a finished leaf

// ------------------------------------------------------------------------------------ standardise
__global__ void __launch_bounds__(GBR_NT) gbr_prepare_kernel(const double* __restrict__ x, int64_t N, int D,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ scale,
                                                             float* __restrict__ z32) {
    const int64_t e = (int64_t)blockIdx.x * GBR_NT + threadIdx.x;
    if (e >= N * D) return;
    const int f = blockIdx.y, j = (int)(e % D);
    z32[(int64_t)f * N * D + e] = (float)((x[e] - mean[f * D + j]) / scale[f * D + j]);
}

// ------------------------------------------------------------------------------------ exact sums
// count, sum and sum of squares of rq per node, accumulated with integer atomics in LDS: exact in any order.
// The 128-bit square goes in as four 32-bit limbs, each into a 64-bit accumulator (fewer than 2^31 rows).
__device__ __forceinline__ void gbr_acc(gu64* sS, gu64* sQ, int* sc, int m, int64_t r) {
    if (sS) atomicAdd(&sS[m], (gu64)r);
    gu64 limb[4];
    tree_sq_limbs(r, limb);
    for (int i = 0; i < 4; ++i) atomicAdd(&sQ[m * 4 + i], limb[i]);
    if (sc) atomicAdd(&sc[m], 1);
}

__global__ void __launch_bounds__(GBR_NT) gbr_stats_kernel(int nn, const int64_t* __restrict__ tr_off, int64_t n1,
                                                           const uint8_t* __restrict__ node,
                                                           const int64_t* __restrict__ rq, int64_t* stS, gu64* stQ,
                                                           int32_t* stc) {
    __shared__ gu64 sS[GBR_NODES], sQ[GBR_NODES * 4];
    __shared__ int sc[GBR_NODES];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int64_t off = tr_off ? tr_off[f] : 0, n = tr_off ? tr_off[f + 1] - off : n1;
    if (tid < GBR_NODES) {
        sS[tid] = 0;
        sc[tid] = 0;
    }
    if (tid < GBR_NODES * 4) sQ[tid] = 0;
    __syncthreads();
    for (int64_t p = tid; p < n; p += GBR_NT) {
        const int nd = node[off + p];
        if (nd < nn) gbr_acc(sS, sQ, sc, nd, rq[off + p]);
    }
    __syncthreads();
    if (tid < GBR_NODES) {
        stS[f * GBR_NODES + tid] = (int64_t)sS[tid];
        stc[f * GBR_NODES + tid] = sc[tid];
    }
    if (tid < GBR_NODES * 4) stQ[f * GBR_NODES * 4 + tid] = sQ[tid];
}

// ------------------------------------------------------------------------------------------ scan
// A workgroup of eight waves per (fold, feature) list; wave w takes the w-th run of 64-row chunks.  Pass 1: every
// wave's count, sum and last value per node over its run (integer sums: exact in any order).  Pass 2: the scan
// proper, each wave starting from the totals of the runs before its own.
template <int NN>
__global__ void __launch_bounds__(GBR_SCAN_NT) gbr_scan_kernel(int D, int folds, const int32_t* __restrict__ ord,
                                                               const float* __restrict__ sv,
                                                               const int64_t* __restrict__ tr_off, int64_t n1,
                                                               const uint8_t* __restrict__ node,
                                                               const int64_t* __restrict__ rq,
                                                               const int64_t* __restrict__ stS,
                                                               const int32_t* __restrict__ stc,
                                                               double* __restrict__ cgain, double* __restrict__ cthr,
                                                               int32_t* __restrict__ cwl, int64_t* __restrict__ cSl) {
    __shared__ int64_t pS[GBR_SCAN_W][NN], qS[GBR_SCAN_W][NN];
    __shared__ double qg[GBR_SCAN_W][NN], qt[GBR_SCAN_W][NN];
    __shared__ int pc[GBR_SCAN_W][NN], qw[GBR_SCAN_W][NN];
    __shared__ float pv[GBR_SCAN_W][NN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t list = blockIdx.x;  // < folds * D
    const int f = (int)(list / D), j = (int)(list % D);
    const int64_t off = tr_off ? tr_off[f] : 0;
    const int n = (int)(tr_off ? tr_off[f + 1] - off : n1);
    const int32_t* o = ord + off * D + (int64_t)j * n;
    const float* s = sv + off * D + (int64_t)j * n;
    const int chunks = (n + 63) / 64, per = (chunks + GBR_SCAN_W - 1) / GBR_SCAN_W;
    const int c0 = wave * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    int tc[NN], cc[NN], bw[NN];
    int64_t tS[NN], cS[NN], bS[NN];
    float cv[NN];
    double bg[NN], bt[NN];
#pragma unroll
    for (int m = 0; m < NN; ++m) {
        tc[m] = stc[f * GBR_NODES + m];
        tS[m] = stS[f * GBR_NODES + m];
        cc[m] = 0;
        cS[m] = 0;
        cv[m] = -INFINITY;
        bg[m] = -1.0;
        bt[m] = 0.0;
        bw[m] = 0;
        bS[m] = 0;
    }
    for (int c = c0; c < c1; ++c) {  // pass 1: per lane, reduced once at the end
        const int i = c * 64 + lane;
        if (i < n) {
            const int p = o[i];
            const float v = s[i];
            const int nd = node[off + p];
            const int64_t r = rq[off + p];
#pragma unroll
            for (int m = 0; m < NN; ++m)
                if (nd == m) {
                    cS[m] += r;
                    cc[m] += 1;
                    cv[m] = fmaxf(cv[m], v);
                }
        }
    }
#pragma unroll
    for (int m = 0; m < NN; ++m) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cS[m] += __shfl_xor(cS[m], d);
            cc[m] += __shfl_xor(cc[m], d);
            cv[m] = fmaxf(cv[m], __shfl_xor(cv[m], d));
        }
        if (lane == 0) {
            pS[wave][m] = cS[m];
            pc[wave][m] = cc[m];
            pv[wave][m] = cv[m];
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NN; ++m) {  // the runs before this wave's: the values ascend along the list
        cc[m] = 0;
        cS[m] = 0;
        cv[m] = 0.f;
        for (int w = 0; w < wave; ++w)
            if (pc[w][m] > 0) {
                cc[m] += pc[w][m];
                cS[m] += pS[w][m];
                cv[m] = pv[w][m];
            }
    }
    const gu64 below_me = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int c = c0; c < c1; ++c) {
        const int i = c * 64 + lane;
        const bool act = i < n;
        const int p = act ? o[i] : 0;
        const float v = act ? s[i] : 0.f;
        const int nd = act ? (int)node[off + p] : (int)GBR_DEAD;
        const int64_t r = act ? rq[off + p] : 0;
#pragma unroll
        for (int m = 0; m < NN; ++m) {
            const bool flag = nd == m;
            const gu64 mask = __ballot(flag);
            if (mask == 0) continue;  // uniform
            int64_t x = flag ? r : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t up = __shfl_up(x, d);
                if (lane >= d) x += up;
            }
            const gu64 below = mask & below_me;
            const int prev = below ? 63 - __clzll(below) : 0;
            float a = __shfl(v, prev);
            if (!below) a = cv[m];
            const int wl = cc[m] + __popcll(below);
            const int64_t Sl = cS[m] + (x - (flag ? r : 0));
            if (flag && wl > 0 && v > a + 1e-7f) {
                const int wr = tc[m] - wl;
                const int64_t Sr = tS[m] - Sl;
                const double diff = (double)wr * (double)Sl - (double)wl * (double)Sr;
                const double gain = diff * diff / ((double)wl * (double)wr);
                if (gain > bg[m]) {  // a lane meets its candidates in ascending threshold order
                    bg[m] = gain;
                    bt[m] = (double)a / 2.0 + (double)v / 2.0;
                    bw[m] = wl;
                    bS[m] = Sl;
                }
            }
            cS[m] += __shfl(x, 63);
            cc[m] += __popcll(mask);
            cv[m] = __shfl(v, 63 - __clzll(mask));
        }
    }
#pragma unroll
    for (int m = 0; m < NN; ++m) {
        double g = bg[m], t = bt[m];
        int w = bw[m];
        int64_t S = bS[m];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double og = __shfl_xor(g, d), ot = __shfl_xor(t, d);
            const int ow = __shfl_xor(w, d);
            const int64_t oS = __shfl_xor(S, d);
            if (og > g || (og == g && ot < t)) {
                g = og;
                t = ot;
                w = ow;
                S = oS;
            }
        }
        if (lane == 0) {
            qg[wave][m] = g;
            qt[wave][m] = t;
            qw[wave][m] = w;
            qS[wave][m] = S;
        }
    }
    __syncthreads();
    if (threadIdx.x < NN) {
        const int m = threadIdx.x;
        int best = 0;
        for (int w = 1; w < GBR_SCAN_W; ++w)
            if (qg[w][m] > qg[best][m] || (qg[w][m] == qg[best][m] && qt[w][m] < qt[best][m])) best = w;
        const int64_t c = ((int64_t)f * GBR_NODES + m) * D + j;
        cgain[c] = qg[best][m];
        cthr[c] = qt[best][m];
        cwl[c] = qw[best][m];
        cSl[c] = qS[best][m];
    }
}

// ---------------------------------------------------------------------------------------- select
struct GbrTree {  // one fit's tree arrays, heap layout: [F][T][ni] / [F][T][nv]
    int16_t* feature;
    double* threshold;
    double* value;
    int32_t* nodes;  // [F][T]
    int32_t* tied;   // [F]
    int T, stage, depth;
};

struct GbrRec {  // the unit export's records [nn]; null in a fit
    int32_t* feature;
    double* threshold;
    double* gain;
    int32_t* wl;
    int64_t* Sl;
    int32_t* leaf;
    int32_t* tied;
};

__global__ void __launch_bounds__(GBR_NT) gbr_select_kernel(int level, int D, int64_t N, const float* __restrict__ z32,
                                                            const int32_t* __restrict__ tr_idx,
                                                            const int64_t* __restrict__ tr_off, int64_t n1,
                                                            const int32_t* __restrict__ qv, int q1,
                                                            const double* __restrict__ cgain,
                                                            const double* __restrict__ cthr,
                                                            const int32_t* __restrict__ cwl,
                                                            const int64_t* __restrict__ cSl, int64_t* stS, gu64* stQ,
                                                            int32_t* stc, uint8_t* node,
                                                            const int64_t* __restrict__ rq, GbrTree tr, GbrRec rec) {
    __shared__ int dfeat[GBR_NODES];
    __shared__ double dthr[GBR_NODES];
    __shared__ gu64 kS[2 * GBR_NODES], kQ[2 * GBR_NODES * 4];
    __shared__ int kc[2 * GBR_NODES];
    __shared__ double rg[GBR_NT / 64];
    __shared__ int rj[GBR_NT / 64], rc[GBR_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int nn = 1 << level, hb = nn - 1;
    const int64_t off = tr_off ? tr_off[f] : 0, n = tr_off ? tr_off[f + 1] - off : n1;
    const int q = qv ? qv[f] : q1;
    const double unq = ldexp(1.0, -q);
    const bool apply = rec.feature == nullptr;
    const int ni = (1 << tr.depth) - 1, nv = (2 << tr.depth) - 1;
    const int64_t ti = ((int64_t)f * tr.T + tr.stage) * ni, tv = ((int64_t)f * tr.T + tr.stage) * nv;
    if (tid < 2 * GBR_NODES) {
        kS[tid] = 0;
        kc[tid] = 0;
    }
    if (tid < 2 * GBR_NODES * 4) kQ[tid] = 0;
    if (apply && level == 0 && tid == 0) tr.nodes[(int64_t)f * tr.T + tr.stage] = 0;
    __syncthreads();
    for (int m = 0; m < nn; ++m) {
        const int cnt = stc[f * GBR_NODES + m];
        const int64_t S = stS[f * GBR_NODES + m];
        const int64_t c = ((int64_t)f * GBR_NODES + m) * D;
        const double mine = tid < D ? cgain[c + tid] : -1.0;
        double g = mine;
        int j = tid;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double og = __shfl_xor(g, d);
            const int oj = __shfl_xor(j, d);
            if (og > g || (og == g && oj < j)) {
                g = og;
                j = oj;
            }
        }
        if (lane == 0) {
            rg[wave] = g;
            rj[wave] = j;
        }
        __syncthreads();
        g = rg[0];
        j = rj[0];
#pragma unroll
        for (int w = 1; w < GBR_NT / 64; ++w)
            if (rg[w] > g || (rg[w] == g && rj[w] < j)) {
                g = rg[w];
                j = rj[w];
            }
        const gu64 same = __ballot(tid < D && mine == g);
        if (lane == 0) rc[wave] = __popcll(same);
        __syncthreads();
        const int ties = rc[0] + rc[1] + rc[2] + rc[3];
        if (tid == 0) {
            const bool found = cnt >= 2 && g >= 0.0;
            const bool leaf = !found || tree_pure(cnt, S, stQ + (f * GBR_NODES + m) * 4, q);
            const bool split = !leaf;
            const double thr = found ? cthr[c + j] : 0.0;
            const int wl = found ? cwl[c + j] : 0;
            const int64_t Sl = found ? cSl[c + j] : 0;
            if (apply) {
                tr.feature[ti + hb + m] = split ? (int16_t)j : (int16_t)-1;
                tr.threshold[ti + hb + m] = split ? thr : 0.0;
                tr.value[tv + hb + m] = cnt > 0 ? ((double)S / (double)cnt) * unq : 0.0;
                if (split) {
                    tr.nodes[(int64_t)f * tr.T + tr.stage] += 1;
                    if (ties >= 2) tr.tied[f] += 1;
                }
            } else {
                rec.feature[m] = found ? j : -1;
                rec.threshold[m] = thr;
                rec.gain[m] = found ? g : -1.0;
                rec.wl[m] = wl;
                rec.Sl[m] = Sl;
                rec.leaf[m] = leaf ? 1 : 0;
                rec.tied[m] = found && ties >= 2 ? 1 : 0;
            }
            dfeat[m] = split ? j : -1;
            dthr[m] = thr;
            if (split) {
                kc[2 * m] = wl;
                kS[2 * m] = (gu64)Sl;
                kc[2 * m + 1] = cnt - wl;
                kS[2 * m + 1] = (gu64)(S - Sl);
            }
        }
        __syncthreads();
    }
    if (!apply) return;
    const bool last = level + 1 == tr.depth;
    for (int64_t p = tid; p < n; p += GBR_NT) {
        const int nd = node[off + p];
        if (nd >= nn) continue;
        const int fe = dfeat[nd];
        if (fe < 0) {
            node[off + p] = GBR_DEAD;
            continue;
        }
        const float z = z32[((int64_t)f * N + tr_idx[off + p]) * D + fe];
        const int child = 2 * nd + ((double)z > dthr[nd] ? 1 : 0);
        node[off + p] = (uint8_t)child;
        if (!last) gbr_acc(nullptr, kQ, nullptr, child, rq[off + p]);  // count and sum come from the split record
    }
    __syncthreads();
    if (tid < 2 * nn) {
        if (last) {  // the children are leaves by the depth limit: their values
            tr.value[tv + (2 * nn - 1) + tid] = kc[tid] > 0 ? ((double)(int64_t)kS[tid] / (double)kc[tid]) * unq : 0.0;
        } else {     // 2 nn <= GBR_NODES here
            stc[f * GBR_NODES + tid] = kc[tid];
            stS[f * GBR_NODES + tid] = (int64_t)kS[tid];
            for (int i = 0; i < 4; ++i) stQ[(f * GBR_NODES + tid) * 4 + i] = kQ[tid * 4 + i];
        }
    }
    if (last && tid == 0) {  // the root's sums of the next stage are accumulated by gbr_update_kernel
        stS[f * GBR_NODES] = 0;
        for (int i = 0; i < 4; ++i) stQ[f * GBR_NODES * 4 + i] = 0;
    }
}

// ---------------------------------------------------------------------------------------- update
__device__ __forceinline__ int gbr_walk(const int16_t* __restrict__ feature, const double* __restrict__ threshold,
                                        const float* z, int depth) {
    int idx = 0;
    for (int l = 0; l < depth; ++l) {
        const int fe = feature[idx];
        if (fe < 0) break;
        idx = 2 * idx + 1 + ((double)z[fe] > threshold[idx] ? 1 : 0);
    }
    return idx;
}

// stage < 0: F = init, the first residuals.  status [F]: 0, or the 1-based stage whose residuals overflowed.
__global__ void __launch_bounds__(GBR_NT) gbr_update_kernel(int stage, int depth, int T, int D, int64_t N,
                                                            const float* __restrict__ z32,
                                                            const int32_t* __restrict__ pos,
                                                            const double* __restrict__ y,
                                                            const int64_t* __restrict__ tr_off,
                                                            const int32_t* __restrict__ qv,
                                                            const double* __restrict__ init, double lr,
                                                            const int16_t* __restrict__ feature,
                                                            const double* __restrict__ threshold,
                                                            const double* __restrict__ value, double* F, int64_t* rq,
                                                            uint8_t* node, int64_t* stS, gu64* stQ, int32_t* stc,
                                                            int32_t* status, int32_t* tied) {
    __shared__ gu64 sS[1], sQ[4];
    const int tid = threadIdx.x, f = blockIdx.y;
    const int64_t row = (int64_t)blockIdx.x * GBR_NT + tid;
    if (tid == 0) sS[0] = 0;
    if (tid < 4) sQ[tid] = 0;
    __syncthreads();
    const int64_t off = tr_off[f], n = tr_off[f + 1] - off;
    if (row < N) {
        double Fn;
        if (stage < 0) {
            Fn = init[f];
        } else {
            const int ni = (1 << depth) - 1, nv = (2 << depth) - 1;
            const int64_t t = (int64_t)f * T + stage;
            const int leaf = gbr_walk(feature + t * ni, threshold + t * ni, z32 + ((int64_t)f * N + row) * D, depth);
            const double step = lr * value[t * nv + leaf];
            Fn = F[(int64_t)f * N + row] + step;
        }
        F[(int64_t)f * N + row] = Fn;
        const int p = pos[(int64_t)f * N + row];
        if (p >= 0 && p < n) {
            const double r = y[(int64_t)f * N + row] - Fn;
            const double t = r * ldexp(1.0, qv[f]);
            const int64_t lim = (int64_t)1 << (62 - tree_ceil_log2(n));
            bool bad = !(fabs(t) < 9.0e18);
            int64_t v = bad ? 0 : __double2ll_rn(t);
            bad = bad || v >= lim || v <= -lim;
            if (bad) {
                atomicCAS(&status[f], 0, stage + 2);
                v = 0;
            }
            rq[off + p] = v;
            node[off + p] = 0;
            gbr_acc(sS, sQ, nullptr, 0, v);
        }
    }
    __syncthreads();
    if (tid == 0) {
        atomicAdd((gu64*)&stS[f * GBR_NODES], sS[0]);
        for (int i = 0; i < 4; ++i) atomicAdd(&stQ[f * GBR_NODES * 4 + i], sQ[i]);
        if (blockIdx.x == 0) {
            stc[f * GBR_NODES] = (int32_t)n;
            if (stage < 0) tied[f] = 0;
        }
    }
}

// --------------------------------------------------------------------------------------- predict
__global__ void __launch_bounds__(GBR_NT) gbr_predict_kernel(const double* __restrict__ feat, int D,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ scale,
                                                             const int16_t* __restrict__ feature,
                                                             const double* __restrict__ threshold,
                                                             const double* __restrict__ value, double init, double lr,
                                                             int T, int depth, double* __restrict__ est) {
    __shared__ float z[FOLD_MAXD];
    __shared__ double step[GBR_PRED_STAGES];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < D) z[tid] = (float)((feat[b * D + tid] - mean[tid]) / scale[tid]);
    __syncthreads();
    const int ni = (1 << depth) - 1, nv = (2 << depth) - 1;
    double F = init;
    for (int s0 = 0; s0 < T; s0 += GBR_PRED_STAGES) {
        const int cnt = T - s0 < GBR_PRED_STAGES ? T - s0 : GBR_PRED_STAGES;
        for (int i = tid; i < cnt; i += GBR_NT) {
            const int64_t s = s0 + i;
            step[i] = lr * value[s * nv + gbr_walk(feature + s * ni, threshold + s * ni, z, depth)];
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < cnt; ++i) F = F + step[i];  // stage order
        __syncthreads();
    }
    if (tid == 0) est[b] = F;
}

// ------------------------------------------------------------------------------------- the C-ABI
struct GbrWs {
    int64_t* rq;
    double *cgain, *cthr;
    int64_t *cSl, *stS;
    gu64* stQ;
    int32_t *cwl, *stc;
    uint8_t* node;
    int64_t bytes;
};

static GbrWs gbr_ws(void* base, int64_t rows, int64_t folds, int64_t D) {
    GbrWs w;
    char* p = (char*)base;
    auto take = [&](int64_t bytes) {
        char* r = p;
        p += (bytes + 7) / 8 * 8;
        return r;
    };
    const int64_t cand = folds * GBR_NODES * D;
    w.rq = (int64_t*)take(rows * 8);
    w.cgain = (double*)take(cand * 8);
    w.cthr = (double*)take(cand * 8);
    w.cSl = (int64_t*)take(cand * 8);
    w.stS = (int64_t*)take(folds * GBR_NODES * 8);
    w.stQ = (gu64*)take(folds * GBR_NODES * 4 * 8);
    w.cwl = (int32_t*)take(cand * 4);
    w.stc = (int32_t*)take(folds * GBR_NODES * 4);
    w.node = (uint8_t*)take(rows);
    w.bytes = (int64_t)(p - (char*)base);
    return w;
}

static int gbr_launch_scan(int nn, int D, int folds, const int32_t* ord, const float* sv, const int64_t* tr_off,
                           int64_t n1, const uint8_t* node, const int64_t* rq, const GbrWs& w, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)folds * D)), block(GBR_SCAN_NT);
#define GBR_SCAN(NN)                                                                                              \
    hipLaunchKernelGGL(gbr_scan_kernel<NN>, grid, block, 0, st, D, folds, ord, sv, tr_off, n1, node, rq, w.stS,   \
                       w.stc, w.cgain, w.cthr, w.cwl, w.cSl)
    switch (nn) {
        case 1: GBR_SCAN(1); break;
        case 2: GBR_SCAN(2); break;
        case 4: GBR_SCAN(4); break;
        default: GBR_SCAN(8); break;
    }
#undef GBR_SCAN
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

}  // namespace edgedet

using namespace edgedet;

extern "C" int64_t edgedet_gbr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D) {
    if (!folds_ok(tr_off_host, folds, 0, true, INT32_MAX) || !fold_dims_ok(D)) return -1;
    return gbr_ws(nullptr, tr_off_host[folds], folds, D).bytes;
}

extern "C" int edgedet_gbr_prepare(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                                   int32_t folds, float* z32, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && N < ((int64_t)1 << 31) && folds >= 1 && folds <= 65535,
                    "gbr_prepare: 1 <= features <= 255, 1 <= rows < 2^31, 1 <= folds <= 65535");
    EDGEDET_REQUIRE(x && mean && scale && z32, "gbr_prepare: null pointer");
    hipLaunchKernelGGL(gbr_prepare_kernel, dim3((unsigned)cdiv(N * D, GBR_NT), (unsigned)folds), dim3(GBR_NT), 0,
                       (hipStream_t)stream, x, N, (int)D, mean, scale, z32);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_gbr_fit(const float* z32, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                               const int32_t* pos, const int32_t* ord, const float* sorted,
                               const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* init,
                               const int32_t* q_host, const int32_t* q, double learning_rate, int32_t T, int32_t depth,
                               void* ws, int64_t ws_bytes, int16_t* feature, double* threshold, double* value,
                               double* est, int32_t* nodes, int32_t* tied, int32_t* status, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && N < ((int64_t)1 << 31),
                    "gbr_fit: 1 <= features <= 255, 1 <= rows < 2^31");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, 0, true, INT32_MAX),
                    "gbr_fit: every fold needs 1 to 2^31 - 1 training rows");
    EDGEDET_REQUIRE(depth >= 1 && depth <= GBR_MAXDEPTH && T >= 1, "gbr_fit: 1 <= max_depth <= 4, n_estimators >= 1");
    EDGEDET_REQUIRE(z32 && y && tr_idx && pos && ord && sorted && tr_off && init && q_host && q && ws && feature &&
                        threshold && value && est && nodes && tied && status,
                    "gbr_fit: null pointer");
    for (int f = 0; f < folds; ++f)
        EDGEDET_REQUIRE(q_host[f] >= GBR_QMIN && q_host[f] <= GBR_QMAX, "gbr_fit: 26 <= q <= 1000");
    GbrWs w = gbr_ws(ws, tr_off_host[folds], folds, D);
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= w.bytes,
                    "gbr_fit: workspace smaller than edgedet_gbr_workspace_size, or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    EDGEDET_CHECK_HIP(hipMemsetAsync(w.stS, 0, (size_t)folds * GBR_NODES * 8, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(w.stQ, 0, (size_t)folds * GBR_NODES * 4 * 8, st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)folds * 4, st));
    const dim3 ugrid((unsigned)cdiv(N, GBR_NT), (unsigned)folds), block(GBR_NT);
    const GbrRec none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int s = -1; s < T; ++s) {
        if (s >= 0) {
            for (int level = 0; level < depth; ++level) {
                const int rc = gbr_launch_scan(1 << level, (int)D, folds, ord, sorted, tr_off, 0, w.node, w.rq, w, st);
                if (rc != 0) return rc;
                const GbrTree tr = {feature, threshold, value, nodes, tied, T, s, depth};
                hipLaunchKernelGGL(gbr_select_kernel, dim3((unsigned)folds), block, 0, st, level, (int)D, N, z32, tr_idx,
                                   tr_off, (int64_t)0, q, 0, w.cgain, w.cthr, w.cwl, w.cSl, w.stS, w.stQ, w.stc, w.node,
                                   w.rq, tr, none);
                EDGEDET_LAUNCH_CHECK();
            }
        }
        hipLaunchKernelGGL(gbr_update_kernel, ugrid, block, 0, st, s, depth, T, (int)D, N, z32, pos, y, tr_off, q, init,
                           learning_rate, feature, threshold, value, est, w.rq, w.node, w.stS, w.stQ, w.stc, status,
                           tied);
        EDGEDET_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int edgedet_gbr_best_split(const int32_t* ord, const float* sorted, int64_t n, int64_t D,
                                      const uint8_t* node, const int64_t* rq, int32_t nn, int32_t q, void* ws,
                                      int64_t ws_bytes, int32_t* feature, double* threshold, double* gain, int32_t* wl,
                                      int64_t* Sl, int32_t* leaf, int32_t* tied, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && n >= 1 && n < ((int64_t)1 << 31),
                    "gbr_best_split: 1 <= features <= 255, 1 <= rows < 2^31");
    EDGEDET_REQUIRE(nn == 1 || nn == 2 || nn == 4 || nn == 8, "gbr_best_split: 1, 2, 4 or 8 nodes");
    EDGEDET_REQUIRE(q >= GBR_QMIN && q <= GBR_QMAX, "gbr_best_split: 26 <= q <= 1000");
    EDGEDET_REQUIRE(ord && sorted && node && rq && ws && feature && threshold && gain && wl && Sl && leaf && tied,
                    "gbr_best_split: null pointer");
    GbrWs w = gbr_ws(ws, n, 1, D);
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= w.bytes,
                    "gbr_best_split: workspace smaller than edgedet_gbr_workspace_size, or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gbr_stats_kernel, dim3(1), dim3(GBR_NT), 0, st, (int)nn, (const int64_t*)nullptr, n, node, rq,
                       w.stS, w.stQ, w.stc);
    EDGEDET_LAUNCH_CHECK();
    const int rc = gbr_launch_scan(nn, (int)D, 1, ord, sorted, nullptr, n, node, rq, w, st);
    if (rc != 0) return rc;
    int level = 0;
    while ((1 << level) < nn) ++level;
    const GbrTree tr = {nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, GBR_MAXDEPTH};
    const GbrRec rec = {feature, threshold, gain, wl, Sl, leaf, tied};
    hipLaunchKernelGGL(gbr_select_kernel, dim3(1), dim3(GBR_NT), 0, st, level, (int)D, n, (const float*)nullptr,
                       (const int32_t*)nullptr, (const int64_t*)nullptr, n, (const int32_t*)nullptr, (int)q, w.cgain,
                       w.cthr, w.cwl, w.cSl, w.stS, w.stQ, w.stc, (uint8_t*)nullptr, rq, tr, rec);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_gbr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean,
                                         const double* scale, const int16_t* feature, const double* threshold,
                                         const double* value, double init, double learning_rate, int32_t T,
                                         int32_t depth, double* est, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && B >= 1 && B < ((int64_t)1 << 31),
                    "gbr_model_predict: 1 <= features <= 255, 1 <= rows < 2^31");
    EDGEDET_REQUIRE(depth >= 1 && depth <= GBR_MAXDEPTH && T >= 1,
                    "gbr_model_predict: 1 <= max_depth <= 4, n_estimators >= 1");
    EDGEDET_REQUIRE(feat && mean && scale && feature && threshold && value && est, "gbr_model_predict: null pointer");
    hipLaunchKernelGGL(gbr_predict_kernel, dim3((unsigned)B), dim3(GBR_NT), 0, (hipStream_t)stream, feat, (int)D, mean,
                       scale, feature, threshold, value, init, learning_rate, (int)T, (int)depth, est);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
