// regression.py's SVR (rbf) and LinearSVR on the device, every cross-validation fold in flight, each solved
// to a certified optimum of its strongly convex objective.  Float64 throughout, fixed-order
// sums, no float atomics.  The standardisation is edgedet_reg_scaler's (csrc/regress.hip); the shared steps
// (zscore, sqdist, lane16_sum, block_sum, the scaler's staging in LDS) are fold_math.hpp's.
//
//   svr_std_kernel      Z = (x - mean) * (1 / scale) of every fold's training rows into the workspace, and
//                       |z|^2 of every row: sixteen lanes per row.
//   svr_gamma_kernel    sklearn's gamma='scale' per fold: 1 / (D var), var the population variance of all
//                       entries of Z (two passes, one workgroup per fold).
//   svr_kmat_kernel     K[i][j] = exp(-gamma max(|a|^2 + |b|^2 - 2 a.b, 0)) by v_mfma_f64_16x16x4_f64: a wave
//                       per 16 x 16 tile, four tiles per workgroup (the tiling of regress.hip's knn_dist_kernel).
//   svr_smo_kernel      one workgroup per fold: SMO on beta = alpha - alpha*, libsvm's second-order working-set
//                       selection, gradient and beta in LDS, kernel rows read from the HBM matrix.
//   svr_predict_kernel  sum_j beta_j exp(-gamma |z - z_j|^2) + b for every row and fold: distance tiles by
//                       the matrix instruction, exponential and weighted row sum in the same kernel.
//   lsvr_fit_kernel     one workgroup per fold: blocked exact dual coordinate descent in natural cyclic order
//                       (liblinear's L2-regularised L1-loss SVR dual, bias as a feature of value 1), stopped on
//                       the duality gap.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "fold_math.hpp"
#include "kernels.hpp"

namespace edgedet {

constexpr int SVR_NT = 1024;
constexpr int SVR_EPT = 4;       // training rows per thread of the SMO workgroup
constexpr int SVR_MAXN = 4000;   // training rows per fold: gradient and beta, 2 x 32,000 bytes of LDS
constexpr double SVR_TAU = 1e-12;  // libsvm's floor on a non-positive curvature
constexpr int LSVR_NT = 256;
constexpr int LSVR_CHECK = 10;   // sweeps between two evaluations of the duality gap

// the fold's kernel matrix starts at sum_{g < f} n_g^2
__device__ __forceinline__ int64_t svr_koff(const int64_t* tr_off, int fold) {
    int64_t o = 0;
    for (int g = 0; g < fold; ++g) {
        const int64_t n = tr_off[g + 1] - tr_off[g];
        o += n * n;
    }
    return o;
}

// ------------------------------------------------------------------------------------ standardise
__global__ void __launch_bounds__(SVR_NT) svr_std_kernel(const double* __restrict__ x, int D,
                                                         const int32_t* __restrict__ tr_idx,
                                                         const int64_t* __restrict__ tr_off,
                                                         const double* __restrict__ mean,
                                                         const double* __restrict__ scale, double* z, double* nrm) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    const int fold = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = tr_off[fold], n = tr_off[fold + 1] - t0;
    if ((int64_t)blockIdx.x * 64 >= n) return;  // uniform: the grid covers the largest fold
    stage_scaler(sm, si, mean, scale, fold, D);
    __syncthreads();
    const int sub = tid & 15;
    const int64_t r = (int64_t)blockIdx.x * 64 + (tid >> 4);
    const bool ok = r < n;
    double acc = 0.0;
    if (ok) {
        const double* src = x + fold_row(tr_idx, t0, r) * D;
        double* dst = z + (t0 + r) * D;
        for (int k = sub; k < D; k += 16) {
            const double v = zscore(src[k], sm[k], si[k]);
            dst[k] = v;
            acc += v * v;
        }
    }
    acc = lane16_sum(acc);
    if (ok && sub == 0) nrm[t0 + r] = acc;
}

// |z|^2 of the rows of one matrix (the unit operator's norms): svr_std_kernel's k order, then lane16_sum
__global__ void __launch_bounds__(SVR_NT) svr_norm_kernel(const double* __restrict__ z, int64_t n, int D,
                                                          double* nrm) {
    const int tid = threadIdx.x, sub = tid & 15;
    const int64_t r = (int64_t)blockIdx.x * 64 + (tid >> 4);
    const bool ok = r < n;
    double acc = 0.0;
    if (ok)
        for (int k = sub; k < D; k += 16) {
            const double v = z[r * D + k];
            acc += v * v;
        }
    acc = lane16_sum(acc);
    if (ok && sub == 0) nrm[r] = acc;
}

// ------------------------------------------------------------------------------------------ gamma
// tr_off null: one matrix of n_one rows at z.  gamma_in > 0 is passed through.
__global__ void __launch_bounds__(SVR_NT) svr_gamma_kernel(const double* __restrict__ z, int D,
                                                           const int64_t* __restrict__ tr_off, int64_t n_one,
                                                           double gamma_in, double* gamma) {
    __shared__ double red[SVR_NT];
    const int fold = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = tr_off ? tr_off[fold] : 0, n = tr_off ? tr_off[fold + 1] - t0 : n_one;
    const double* zf = z + t0 * D;
    const int64_t cnt = n * D;
    double acc = 0.0;
    for (int64_t e = tid; e < cnt; e += SVR_NT) acc += zf[e];
    const double mu = block_sum<SVR_NT>(acc, red) / (double)cnt;
    acc = 0.0;
    for (int64_t e = tid; e < cnt; e += SVR_NT) {
        const double d = zf[e] - mu;
        acc += d * d;
    }
    const double var = block_sum<SVR_NT>(acc, red) / (double)cnt;
    if (tid == 0) gamma[fold] = gamma_in > 0.0 ? gamma_in : (var != 0.0 ? 1.0 / ((double)D * var) : 1.0);
}

// ---------------------------------------------------------------------------------- kernel matrix
// Lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15] of a k-step of four; element i of the result is
// D[(l >> 4) + 4 i][l & 15].  z is standardised already.
__global__ void __launch_bounds__(256) svr_kmat_kernel(const double* __restrict__ z, int D,
                                                       const int64_t* __restrict__ tr_off, int64_t n_one,
                                                       const double* __restrict__ nrm,
                                                       const double* __restrict__ gamma, double* K) {
    const int fold = blockIdx.z, tid = threadIdx.x;
    const int64_t t0 = tr_off ? tr_off[fold] : 0, n = tr_off ? tr_off[fold + 1] - t0 : n_one;
    if ((int64_t)blockIdx.x * 64 >= n || (int64_t)blockIdx.y * 16 >= n) return;  // uniform
    const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.y * 16, b0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    const int64_t qa = q0 + m, bb = b0 + m;
    const bool oka = qa < n, okb = bb < n;
    const double* rowa = z + (t0 + (oka ? qa : 0)) * D;
    const double* rowb = z + (t0 + (okb ? bb : 0)) * D;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + kk;
        const bool okk = k < D;
        const double a = oka && okk ? rowa[k] : 0.0;
        const double b = okb && okk ? rowb[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    if (!okb) return;
    const double nb = nrm[t0 + bb], g = gamma[fold];
    double* Kf = K + (tr_off ? svr_koff(tr_off, fold) : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t q = q0 + kk + 4 * i;
        if (q < n) {
            Kf[q * n + bb] = exp(-g * sqdist(nrm[t0 + q], nb, acc[i]));
        }
    }
}

// -------------------------------------------------------------------------------------------- SMO
// minimise 1/2 beta^T K beta - y^T beta + eps |beta|_1, -C <= beta <= C, sum beta = 0.  With g = K beta - y,
// beta_t can rise while beta_t < C, at the rate u_t = g_t + eps (beta_t >= 0) or g_t - eps (beta_t < 0), and
// fall while beta_t > -C, at d_t = g_t + eps (beta_t > 0) or g_t - eps (beta_t <= 0): libsvm's I_up / I_low
// of the 2n-variable problem with alpha alpha* = 0.  m = max_up -u_t, M = min_low -d_t, stop on m - M <= tol.
struct SvrParams {
    const double* K;
    const double* y;         // [F][N]
    const int32_t* tr_idx;
    const int64_t* tr_off;
    double* beta;            // [T]
    double* intercept;       // [F]
    double* viol;            // [F]
    int32_t* iters;          // [F]
    int32_t* status;         // [F]: 0 ok, 1 not converged in max_iter
    int64_t N;
    double C, eps, tol;
    int max_iter;
};

struct SvrPick {
    double v;
    int i;
};

__device__ __forceinline__ bool svr_better(double v, int i, const SvrPick& o) {
    return v > o.v || (v == o.v && i < o.i);
}

// the largest value, ties to the lowest index; every thread returns the same pick.  One barrier: the caller
// alternates between two slot arrays.
__device__ __forceinline__ SvrPick svr_block_argmax(SvrPick x, double* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(x.v, o);
        const int oi = __shfl_xor(x.i, o);
        if (svr_better(ov, oi, x)) {
            x.v = ov;
            x.i = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = x.v;
        si[threadIdx.x >> 6] = x.i;
    }
    __syncthreads();
    SvrPick r{sv[0], si[0]};
    for (int w = 1; w < SVR_NT / 64; ++w)
        if (svr_better(sv[w], si[w], r)) {
            r.v = sv[w];
            r.i = si[w];
        }
    return r;
}

__global__ void __launch_bounds__(SVR_NT) svr_smo_kernel(SvrParams p) {
    __shared__ double sG[SVR_MAXN], sB[SVR_MAXN];
    __shared__ double sv[2][SVR_NT / 64], smin[SVR_NT / 64], ssum[2][SVR_NT / 64];
    __shared__ int si[2][SVR_NT / 64];
    const int fold = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = p.tr_off[fold];
    const int n = (int)(p.tr_off[fold + 1] - t0);
    const double* K = p.K + svr_koff(p.tr_off, fold);
    const double C = p.C, eps = p.eps;
    double yt[SVR_EPT], kd[SVR_EPT];
#pragma unroll
    for (int e = 0; e < SVR_EPT; ++e) {
        const int t = tid + e * SVR_NT;
        yt[e] = 0.0;
        kd[e] = 1.0;
        if (t < n) {
            yt[e] = p.y[(int64_t)fold * p.N + fold_row(p.tr_idx, t0, t)];
            kd[e] = K[(int64_t)t * n + t];
            sB[t] = 0.0;
            sG[t] = -yt[e];
        }
    }
    int iter = 0;
    bool conv = false, verified = false;
    double gmax = 0.0, gmin = 0.0;
    for (;;) {
        SvrPick a{-INFINITY, INT_MAX};
#pragma unroll
        for (int e = 0; e < SVR_EPT; ++e) {
            const int t = tid + e * SVR_NT;
            if (t < n) {
                const double b = sB[t];
                if (b < C) {
                    const double val = -(sG[t] + (b >= 0.0 ? eps : -eps));
                    if (svr_better(val, t, a)) {
                        a.v = val;
                        a.i = t;
                    }
                }
            }
        }
        a = svr_block_argmax(a, sv[0], si[0]);
        const int i = a.i;  // C > 0 and sum beta = 0: some beta_t < C
        gmax = a.v;
        if (i == INT_MAX) break;  // uniform: only a non-finite gradient leaves no candidate; status 1
        const double kii = K[(int64_t)i * n + i];
        double ki[SVR_EPT];
        SvrPick best{-INFINITY, INT_MAX};
        double lmin = INFINITY;
#pragma unroll
        for (int e = 0; e < SVR_EPT; ++e) {
            const int t = tid + e * SVR_NT;
            ki[e] = 0.0;
            if (t < n) {
                ki[e] = K[(int64_t)i * n + t];
                const double b = sB[t];
                if (b > -C) {
                    const double d = sG[t] + (b > 0.0 ? eps : -eps);
                    lmin = fmin(lmin, -d);
                    const double gain = gmax + d;
                    if (gain > 0.0) {
                        double curv = (kii + kd[e]) - 2.0 * ki[e];
                        if (curv <= 0.0) curv = SVR_TAU;
                        const double obj = gain * gain / curv;
                        if (svr_better(obj, t, best)) {
                            best.v = obj;
                            best.i = t;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lmin = fmin(lmin, __shfl_xor(lmin, o));
        if ((tid & 63) == 0) smin[tid >> 6] = lmin;
        best = svr_block_argmax(best, sv[1], si[1]);  // its barrier also orders the smin stores
        gmin = smin[0];
        for (int w = 1; w < SVR_NT / 64; ++w) gmin = fmin(gmin, smin[w]);
        const int j = best.i;
        if (gmax - gmin <= p.tol || j == INT_MAX) {  // uniform
            if (verified) {
                conv = true;
                break;
            }
            // the running gradient passes: once more on g = K beta - y recomputed from beta (K is symmetric)
            __syncthreads();
#pragma unroll
            for (int e = 0; e < SVR_EPT; ++e) {
                const int t = tid + e * SVR_NT;
                if (t < n) {
                    double acc = 0.0;
                    for (int s = 0; s < n; ++s) acc += K[(int64_t)s * n + t] * sB[s];
                    sG[t] = acc - yt[e];
                }
            }
            verified = true;
            continue;
        }
        verified = false;
        if (iter >= p.max_iter) break;  // uniform
        const double bi = sB[i], bj = sB[j];
        const double dj = sG[j] + (bj > 0.0 ? eps : -eps);
        double curv = (kii + K[(int64_t)j * n + j]) - 2.0 * K[(int64_t)i * n + j];
        if (curv <= 0.0) curv = SVR_TAU;
        // the rates hold until a coordinate reaches zero or the box: libsvm clips there too (alpha* = 0)
        const double room_i = bi < 0.0 ? -bi : C - bi, room_j = bj > 0.0 ? bj : bj + C;
        const double room = fmin(room_i, room_j);
        double delta = (gmax + dj) / curv;
        delta = delta < room ? delta : room;
        const double nbi = delta == room_i ? (bi < 0.0 ? 0.0 : C) : bi + delta;
        const double nbj = delta == room_j ? (bj > 0.0 ? 0.0 : -C) : bj - delta;
        __syncthreads();  // every thread has read beta_i, beta_j and g_j
#pragma unroll
        for (int e = 0; e < SVR_EPT; ++e) {
            const int t = tid + e * SVR_NT;
            if (t < n) {
                sG[t] += delta * (ki[e] - K[(int64_t)j * n + t]);
                if (t == i) sB[t] = nbi;
                if (t == j) sB[t] = nbj;
            }
        }
        ++iter;
    }
    // libsvm's intercept: the mean of -(g_t + eps sign beta_t) over the free support vectors, or the midpoint
    // of [M, m] without any
    double fs = 0.0, fc = 0.0;
#pragma unroll
    for (int e = 0; e < SVR_EPT; ++e) {
        const int t = tid + e * SVR_NT;
        if (t < n) {
            const double b = sB[t];
            p.beta[t0 + t] = b;
            if (b != 0.0 && fabs(b) < C) {
                fs += -(sG[t] + (b > 0.0 ? eps : -eps));
                fc += 1.0;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fs += __shfl_xor(fs, o);
        fc += __shfl_xor(fc, o);
    }
    if ((tid & 63) == 0) {
        ssum[0][tid >> 6] = fs;
        ssum[1][tid >> 6] = fc;
    }
    __syncthreads();
    if (tid == 0) {
        fs = 0.0;
        fc = 0.0;
        for (int w = 0; w < SVR_NT / 64; ++w) {
            fs += ssum[0][w];
            fc += ssum[1][w];
        }
        p.intercept[fold] = fc > 0.0 ? fs / fc : 0.5 * (gmax + gmin);
        p.viol[fold] = gmax - gmin;
        p.iters[fold] = iter;
        p.status[fold] = conv ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------- predict
// out[f][q] = sum_j beta_j exp(-gamma max(|z_q|^2 + |z_j|^2 - 2 z_q.z_j, 0)) + b: a wave per sixteen rows of
// the dataset, walking the fold's training rows sixteen at a time; each lane sums its training column over the
// tiles in order, then the sixteen columns are added by a butterfly.
__global__ void __launch_bounds__(256) svr_predict_kernel(const double* __restrict__ x, int64_t N, int D,
                                                          const double* __restrict__ mean,
                                                          const double* __restrict__ scale,
                                                          const int64_t* __restrict__ tr_off,
                                                          const double* __restrict__ z,
                                                          const double* __restrict__ nrm,
                                                          const double* __restrict__ beta,
                                                          const double* __restrict__ intercept,
                                                          const double* __restrict__ gamma, double* out) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    const int fold = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = tr_off[fold], n = tr_off[fold + 1] - t0;
    stage_scaler_padded<256>(sm, si, mean, scale, fold, D);
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int64_t q0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (q0 >= N) return;  // uniform per wave, after the only barrier
    const int64_t qa = q0 + m;
    const bool oka = qa < N;
    const double* rowa = x + (oka ? qa : 0) * D;
    double qn = 0.0;
    for (int k = kk; k < D; k += 4) {
        const double a = oka ? zscore(rowa[k], sm[k], si[k]) : 0.0;
        qn += a * a;
    }
    qn += __shfl_xor(qn, 16);
    qn += __shfl_xor(qn, 32);
    double qi[4], sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) qi[i] = __shfl(qn, kk + 4 * i);  // lane kk + 4 i holds row kk + 4 i
    const double g = gamma[fold];
    for (int64_t b0 = 0; b0 < n; b0 += 16) {
        const int64_t bb = b0 + m;
        const bool okb = bb < n;
        const double* rowb = z + (t0 + (okb ? bb : 0)) * D;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < D; k0 += 4) {
            const int k = k0 + kk;
            const bool okk = k < D;
            const double a = oka && okk ? zscore(rowa[k], sm[k], si[k]) : 0.0;
            const double b = okb && okk ? rowb[k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        const double nb = okb ? nrm[t0 + bb] : 0.0, wb = okb ? beta[t0 + bb] : 0.0;
        if (wb != 0.0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] += wb * exp(-g * sqdist(qi[i], nb, acc[i]));
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double s = lane16_sum(sum[i]);
        const int64_t q = q0 + kk + 4 * i;
        if (m == 0 && q < N) out[(int64_t)fold * N + q] = s + intercept[fold];
    }
}

// ------------------------------------------------------------------------------------------- LSVR
// P(v) = 1/2 |v|^2 + C sum_i max(0, |y_i - v.x~_i| - eps), x~ = (z, 1); D(beta) = -1/2 |X~^T beta|^2 + y^T beta
// - eps |beta|_1 on |beta_i| <= C.  Coordinate i: with g = v.x~_i - y_i and h = |x~_i|^2 (>= 1), the exact
// minimiser is beta_i <- clip(soft(beta_i - g / h, eps / h), -C, C).  Sixteen coordinates at a time: their
// gradients and 16 x 16 Gram matrix M by the matrix instruction, then the sixteen sequential updates on M
// (g_a += d_s M[a][s] for a > s), then v += sum_a d_a x~_a.
struct LsvrParams {
    const double* z;         // [T][D] standardised training rows
    const double* y;         // [F][N]
    const int32_t* tr_idx;
    const int64_t* tr_off;
    double* beta;            // [T]
    double* v;               // [F][D + 1]
    double* res;             // [F][2]: gap, tol
    int32_t* sweeps;         // [F]
    int32_t* status;         // [F]: 0 ok, 1 not converged in max_sweeps
    int64_t N;
    double C, eps, tol_abs, tol_rel;
    int D, max_sweeps;
};

// v = X~^T beta from scratch into sv, then the duality gap P(v) - D(beta)
__device__ double lsvr_gap(const LsvrParams& p, const double* zf, const double* yf, const double* bf, int64_t t0,
                           int n, double* sv, double* red) {
    const int tid = threadIdx.x, D = p.D, Dt = D + 1;
    __syncthreads();  // beta's stores are done
    if (tid < Dt) {
        double acc = 0.0;
        if (tid < D)
            for (int i = 0; i < n; ++i) acc += bf[i] * zf[(int64_t)i * D + tid];
        else
            for (int i = 0; i < n; ++i) acc += bf[i];
        sv[tid] = acc;
    }
    __syncthreads();
    const double vv = block_sum<LSVR_NT>(tid < Dt ? sv[tid] * sv[tid] : 0.0, red);
    const int sub = tid & 15, grp = tid >> 4;
    double hinge = 0.0, yb = 0.0, l1 = 0.0;
    for (int i0 = 0; i0 < n; i0 += LSVR_NT / 16) {
        const int i = i0 + grp;
        const bool ok = i < n;
        double dot = 0.0;
        if (ok)
            for (int k = sub; k < Dt; k += 16) dot += (k < D ? zf[(int64_t)i * D + k] : 1.0) * sv[k];
        dot = lane16_sum(dot);
        if (ok && sub == 0) {
            const double yi = yf[fold_row(p.tr_idx, t0, i)], b = bf[i];
            hinge += fmax(fabs(yi - dot) - p.eps, 0.0);
            yb += yi * b;
            l1 += fabs(b);
        }
    }
    hinge = block_sum<LSVR_NT>(hinge, red);
    yb = block_sum<LSVR_NT>(yb, red);
    l1 = block_sum<LSVR_NT>(l1, red);
    return ((vv + p.C * hinge) - yb) + p.eps * l1;
}

__global__ void __launch_bounds__(LSVR_NT) lsvr_fit_kernel(LsvrParams p) {
    __shared__ double sv[FOLD_MAXD], red[LSVR_NT], part[4][256], sM[256], dpart[4][4][16], sg[16], sd[16];
    const int fold = blockIdx.x, tid = threadIdx.x, D = p.D, Dt = D + 1;
    const int64_t t0 = p.tr_off[fold];
    const int n = (int)(p.tr_off[fold + 1] - t0);
    const double* zf = p.z + t0 * D;
    const double* yf = p.y + (int64_t)fold * p.N;
    double* bf = p.beta + t0;
    const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    double p0 = 0.0;
    for (int i = tid; i < n; i += LSVR_NT) {
        bf[i] = 0.0;
        p0 += fmax(fabs(yf[fold_row(p.tr_idx, t0, i)]) - p.eps, 0.0);
    }
    p0 = p.C * block_sum<LSVR_NT>(p0, red);
    const double tol = p.tol_abs > 0.0 ? p.tol_abs : p.tol_rel * p0;
    int sweep = 0;
    bool conv = false;
    double gap = 0.0;
    for (;;) {
        if (sweep % LSVR_CHECK == 0 || sweep >= p.max_sweeps) {  // uniform
            gap = lsvr_gap(p, zf, yf, bf, t0, n, sv, red);     // also refreshes the running v
            conv = gap <= tol;
            if (conv || sweep >= p.max_sweeps) break;
        }
        for (int i0 = 0; i0 < n; i0 += 16) {
            const int r = i0 + m;
            const bool ok = r < n;
            const double* zr = zf + (int64_t)(ok ? r : 0) * D;
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
            double dot = 0.0;
            double xs[FOLD_MAXD / 16];  // every load in flight before the first matrix instruction
#pragma unroll
            for (int u = 0; u < FOLD_MAXD / 16; ++u) {
                const int k = 4 * wave + 16 * u + kk;
                xs[u] = ok ? (k < D ? zr[k] : (k == D ? 1.0 : 0.0)) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < FOLD_MAXD / 16; ++u) {
                const int k0 = 4 * wave + 16 * u, k = k0 + kk;
                if (k0 < Dt) {  // uniform per wave
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[u], xs[u], acc, 0, 0, 0);
                    dot += k < Dt ? xs[u] * sv[k] : 0.0;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) part[wave][(kk + 4 * i) * 16 + m] = acc[i];
            dpart[wave][kk][m] = dot;
            __syncthreads();
            sM[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
            if (tid < 16) {
                double g = 0.0;
                for (int w = 0; w < 4; ++w)
                    for (int q = 0; q < 4; ++q) g += dpart[w][q][tid];
                sg[tid] = i0 + tid < n ? g - yf[fold_row(p.tr_idx, t0, i0 + tid)] : 0.0;
            }
            __syncthreads();
            if (wave == 0) {  // every group of sixteen lanes runs the same sixteen updates; the first stores
                double Ma[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) Ma[s] = sM[m * 16 + s];
                double g = sg[m], bn_mine = 0.0, d_mine = 0.0;
                const double bo = ok ? bf[r] : 0.0;
                double h = 1.0;
#pragma unroll
                for (int s = 0; s < 16; ++s) h = (s == m && ok) ? Ma[s] : h;
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const double u = bo - g / h, mag = fabs(u) - p.eps / h;
                    double bn = mag > 0.0 ? (u > 0.0 ? mag : -mag) : 0.0;
                    bn = bn > p.C ? p.C : (bn < -p.C ? -p.C : bn);
                    const double d = ok ? bn - bo : 0.0;
                    const double ds = __shfl(d, s, 16);
                    if (m == s) {
                        bn_mine = bn;
                        d_mine = ds;
                    }
                    if (m > s) g += ds * Ma[s];
                }
                if (lane < 16) {
                    sd[m] = d_mine;
                    if (ok) bf[r] = bn_mine;
                }
            }
            __syncthreads();
            if (tid < Dt) {
                double xs[16];  // every load in flight before the first use; d is zero past the fold's last row
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int rr = i0 + s < n ? i0 + s : n - 1;
                    xs[s] = tid < D ? zf[(int64_t)rr * D + tid] : 1.0;
                }
                double a = sv[tid];
#pragma unroll
                for (int s = 0; s < 16; ++s) a += sd[s] * xs[s];
                sv[tid] = a;
            }
            __syncthreads();
        }
        ++sweep;
    }
    // sv holds X~^T beta recomputed from the final beta
    if (tid < Dt) p.v[(int64_t)fold * Dt + tid] = sv[tid];
    if (tid == 0) {
        p.res[2 * fold] = gap;
        p.res[2 * fold + 1] = tol;
        p.sweeps[fold] = sweep;
        p.status[fold] = conv ? 0 : 1;
    }
}

// ------------------------------------------------------------------------------------- the C-ABI
static int64_t svr_ws_doubles(const int64_t* tr_off_host, int32_t folds, int64_t D, bool with_kernel) {
    const int64_t T = tr_off_host[folds];
    int64_t k = 0;
    for (int f = 0; f < folds && with_kernel; ++f) {
        const int64_t n = tr_off_host[f + 1] - tr_off_host[f];
        k += n * n;
    }
    return T * D + T + k;  // Z, |z|^2, K
}

extern "C" int64_t edgedet_svr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D,
                                              int32_t with_kernel) {
    if (!fold_dims_ok(D) || !folds_ok(tr_off_host, folds, 0, true)) return -1;
    return svr_ws_doubles(tr_off_host, folds, D, with_kernel != 0) * (int64_t)sizeof(double);
}

extern "C" int edgedet_svr_kernel_matrix(const double* z, int64_t n, int64_t D, double gamma_in, double* norm,
                                         double* gamma, double* K, void* stream) {
    EDGEDET_REQUIRE(z && norm && gamma && K, "svr_kernel_matrix: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && n >= 1 && n <= 65535 * 16, "svr_kernel_matrix: 1 <= features <= 255, 1 <= rows");
    EDGEDET_REQUIRE(gamma_in >= 0.0, "svr_kernel_matrix: gamma > 0, or 0 for gamma='scale'");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(svr_norm_kernel, dim3((unsigned)cdiv(n, 64)), dim3(SVR_NT), 0, st, z, n, (int)D, norm);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(svr_gamma_kernel, dim3(1), dim3(SVR_NT), 0, st, z, (int)D, (const int64_t*)nullptr, n,
                       gamma_in, gamma);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(svr_kmat_kernel, dim3((unsigned)cdiv(n, 64), (unsigned)cdiv(n, 16), 1), dim3(256), 0, st, z,
                       (int)D, (const int64_t*)nullptr, n, norm, gamma, K);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

// Z and |z|^2 of every fold's training rows into the head of the workspace
static int svr_standardise(const double* x, int64_t D, const int32_t* tr_idx, const int64_t* tr_off_host,
                           const int64_t* tr_off, int32_t folds, const double* mean, const double* scale, double* ws,
                           hipStream_t st) {
    int64_t nmax = 0;
    for (int f = 0; f < folds; ++f) nmax = std::max(nmax, tr_off_host[f + 1] - tr_off_host[f]);
    const int64_t T = tr_off_host[folds];
    hipLaunchKernelGGL(svr_std_kernel, dim3((unsigned)cdiv(nmax, 64), (unsigned)folds), dim3(SVR_NT), 0, st, x, (int)D,
                       tr_idx, tr_off, mean, scale, ws, ws + T * D);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_svr_fit(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                               const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                               const double* scale, double C, double epsilon, double tol, int32_t max_iter, void* ws,
                               int64_t ws_bytes, double* beta, double* intercept, double* gamma, double* viol,
                               int32_t* iters, int32_t* status, void* stream) {
    EDGEDET_REQUIRE(x && y && tr_idx && tr_off_host && tr_off && mean && scale && ws && beta && intercept && gamma &&
                        viol && iters && status,
                    "svr_fit: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1, "svr_fit: 1 <= features <= 255");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, N, true), "svr_fit: fold offsets (every fold non-empty)");
    EDGEDET_REQUIRE(C > 0.0 && epsilon >= 0.0 && tol > 0.0 && max_iter >= 1,
                    "svr_fit: C > 0, epsilon >= 0, tol > 0, max_iter >= 1");
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0, "svr_fit: the workspace is not 8-byte aligned");
    int64_t nmax = 0;
    for (int f = 0; f < folds; ++f) nmax = std::max(nmax, tr_off_host[f + 1] - tr_off_host[f]);
    EDGEDET_REQUIRE(nmax <= SVR_MAXN, "svr_fit: at most 4,000 training rows per fold (the gradient lives in LDS)");
    EDGEDET_REQUIRE(ws_bytes >= svr_ws_doubles(tr_off_host, folds, D, true) * (int64_t)sizeof(double),
                    "svr_fit: workspace smaller than edgedet_svr_workspace_size");
    hipStream_t st = (hipStream_t)stream;
    const int64_t T = tr_off_host[folds];
    double* z = (double*)ws;
    double* nrm = z + T * D;
    double* K = nrm + T;
    if (svr_standardise(x, D, tr_idx, tr_off_host, tr_off, folds, mean, scale, z, st) != 0) return -3;
    hipLaunchKernelGGL(svr_gamma_kernel, dim3((unsigned)folds), dim3(SVR_NT), 0, st, z, (int)D, tr_off, (int64_t)0, 0.0,
                       gamma);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(svr_kmat_kernel, dim3((unsigned)cdiv(nmax, 64), (unsigned)cdiv(nmax, 16), (unsigned)folds),
                       dim3(256), 0, st, z, (int)D, tr_off, (int64_t)0, nrm, gamma, K);
    EDGEDET_LAUNCH_CHECK();
    SvrParams p{};
    p.K = K;
    p.y = y;
    p.tr_idx = tr_idx;
    p.tr_off = tr_off;
    p.beta = beta;
    p.intercept = intercept;
    p.viol = viol;
    p.iters = iters;
    p.status = status;
    p.N = N;
    p.C = C;
    p.eps = epsilon;
    p.tol = tol;
    p.max_iter = max_iter;
    hipLaunchKernelGGL(svr_smo_kernel, dim3((unsigned)folds), dim3(SVR_NT), 0, st, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_svr_predict(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                                   const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const void* ws,
                                   int64_t ws_bytes, const double* beta, const double* intercept, const double* gamma,
                                   double* out, void* stream) {
    EDGEDET_REQUIRE(x && mean && scale && tr_off_host && tr_off && ws && beta && intercept && gamma && out,
                    "svr_predict: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && N <= (int64_t)INT_MAX * 64, "svr_predict: 1 <= features <= 255");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, 0, true), "svr_predict: fold offsets (every fold non-empty)");
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0, "svr_predict: the workspace is not 8-byte aligned");
    EDGEDET_REQUIRE(ws_bytes >= svr_ws_doubles(tr_off_host, folds, D, false) * (int64_t)sizeof(double),
                    "svr_predict: workspace smaller than edgedet_svr_workspace_size");
    const int64_t T = tr_off_host[folds];
    const double* z = (const double*)ws;
    hipLaunchKernelGGL(svr_predict_kernel, dim3((unsigned)cdiv(N, 64), (unsigned)folds), dim3(256), 0,
                       (hipStream_t)stream, x, N, (int)D, mean, scale, tr_off, z, z + T * D, beta, intercept, gamma, out);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_lsvr_fit(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                                const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                                const double* scale, double C, double epsilon, double tol_abs, double tol_rel,
                                int32_t max_sweeps, void* ws, int64_t ws_bytes, double* beta, double* v, double* res,
                                int32_t* sweeps, int32_t* status, void* stream) {
    EDGEDET_REQUIRE(x && y && tr_idx && tr_off_host && tr_off && mean && scale && ws && beta && v && res && sweeps &&
                        status,
                    "lsvr_fit: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1, "lsvr_fit: 1 <= features <= 255");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, N, true), "lsvr_fit: fold offsets (every fold non-empty)");
    EDGEDET_REQUIRE(tr_off_host[folds] <= INT_MAX, "lsvr_fit: too many training rows");
    EDGEDET_REQUIRE(C > 0.0 && epsilon >= 0.0 && (tol_abs > 0.0 || tol_rel > 0.0) && max_sweeps >= 1,
                    "lsvr_fit: C > 0, epsilon >= 0, a positive tolerance, max_sweeps >= 1");
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0, "lsvr_fit: the workspace is not 8-byte aligned");
    EDGEDET_REQUIRE(ws_bytes >= svr_ws_doubles(tr_off_host, folds, D, false) * (int64_t)sizeof(double),
                    "lsvr_fit: workspace smaller than edgedet_svr_workspace_size");
    hipStream_t st = (hipStream_t)stream;
    double* z = (double*)ws;
    if (svr_standardise(x, D, tr_idx, tr_off_host, tr_off, folds, mean, scale, z, st) != 0) return -3;
    LsvrParams p{};
    p.z = z;
    p.y = y;
    p.tr_idx = tr_idx;
    p.tr_off = tr_off;
    p.beta = beta;
    p.v = v;
    p.res = res;
    p.sweeps = sweeps;
    p.status = status;
    p.N = N;
    p.C = C;
    p.eps = epsilon;
    p.tol_abs = tol_abs;
    p.tol_rel = tol_rel;
    p.D = (int)D;
    p.max_sweeps = max_sweeps;
    hipLaunchKernelGGL(lsvr_fit_kernel, dim3((unsigned)folds), dim3(LSVR_NT), 0, st, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

}  // namespace edgedet
