// regression.py's deterministic sklearn estimators on the device, every cross-validation fold in flight:
// LinearRegression (LR), ElasticNet (EN), BayesianRidge (BR) and KNeighborsRegressor (KNR), each behind
// fit_model's StandardScaler (regression.py:38-77).  Float64 throughout; the steps shared with the other
// estimator files (zscore, sqdist, lane16_sum, block_sum / block_max, fold_row) are fold_math.hpp's.
//
//   reg_scaler_kernel  one workgroup per fold: mean, population variance and scale = sqrt(var) of every
//                      column over the fold's training rows (constant columns take scale 1 by sklearn's
//                      _is_constant_feature rule), and the mean of the fold's target.
//   reg_gram_kernel    G = Z~^T Z~ with v_mfma_f64_16x16x4_f64, Z~ = (Z, y - ymean, 0 ...) of width Dp =
//                      D + 1 padded to a multiple of 16: every operand element is standardised in the load,
//                      (x - mean) * (1 / scale).  G[:D,:D] = Z^T Z, G[:D,D] = Z^T yc, G[D,D] = yc^T yc.  One
//                      workgroup per 16x16 tile of the lower triangle and fold, four waves splitting the rows
//                      and summed in a fixed order (the tile pattern of baseline.hip's svm_hessian_tile).
//   reg_eigh_kernel    one workgroup per fold: cyclic parallel Jacobi on G[:D,:D] (round-robin ordering, D/2
//                      disjoint rotations per round), matrix in an HBM workspace and eigenvectors (as rows)
//                      in the output, until the off-diagonal norm is <= D eps |G|_F.  Serves LR and BR.
//   reg_lr_kernel      the minimum-norm least-squares solution over the eigenvalues > tau lambda_max.
//   reg_br_kernel      sklearn's BayesianRidge fixed-point loop in the eigenbasis (n > D branch).
//   reg_en_kernel      covariance-form cyclic coordinate descent on Q = G / n, stopped on the norm of the
//                      optimality residual z (a subgradient of the objective) recomputed from scratch.
//   reg_predict_kernel standardised row . coef + ymean for every row of the dataset and fold.
//   knn_norm / knn_dist / knn_select   squared distances |a|^2 + |b|^2 - 2 a.b by the fp64 matrix
//                      instruction into an HBM workspace, then per query an exact k-smallest selection on the
//                      float64 keys (a bitwise bisection on the key, ties at the k-th distance to the lowest
//                      training position) and the mean of the k targets summed in position order.
#include <vector>

#include "fold_math.hpp"
#include "kernels.hpp"

namespace edgedet {

constexpr int REG_NT = 1024;
constexpr double REG_EPS = 2.220446049250313e-16;

static int64_t reg_dp(int64_t D) { return (D + 1 + 15) / 16 * 16; }
static int64_t reg_de(int64_t D) { return (D + 1) / 2 * 2; }  // Jacobi order: D rounded up to even

// --------------------------------------------------------------------------------------- scaler
// A column per thread (tid & 255), four row groups (tid >> 8) summed in a fixed order.
__global__ void __launch_bounds__(REG_NT) reg_scaler_kernel(const double* __restrict__ x, int D,
                                                            const double* __restrict__ y, int64_t N,
                                                            const int32_t* __restrict__ tr_idx,
                                                            const int64_t* __restrict__ tr_off, double* mean,
                                                            double* scale, double* ymean) {
    __shared__ double red[REG_NT];
    const int fold = blockIdx.x, tid = threadIdx.x, col = tid & 255, rg = tid >> 8;
    const int64_t t0 = tr_off[fold], n = tr_off[fold + 1] - t0;
    double acc = 0.0;
    if (col < D)
        for (int64_t r = rg; r < n; r += 4) acc += x[fold_row(tr_idx, t0, r) * D + col];
    else if (col == D && y)
        for (int64_t r = rg; r < n; r += 4) acc += y[(int64_t)fold * N + fold_row(tr_idx, t0, r)];
    red[tid] = acc;
    __syncthreads();
    const double mu = (((red[col] + red[256 + col]) + red[512 + col]) + red[768 + col]) / (double)n;
    __syncthreads();
    acc = 0.0;
    if (col < D)
        for (int64_t r = rg; r < n; r += 4) {
            const double d = x[fold_row(tr_idx, t0, r) * D + col] - mu;
            acc += d * d;
        }
    red[tid] = acc;
    __syncthreads();
    if (rg == 0 && col < D) {
        const double var = (((red[col] + red[256 + col]) + red[512 + col]) + red[768 + col]) / (double)n;
        // sklearn _is_constant_feature: var <= n eps var + (n mean eps)^2
        const double nm = (double)n * mu * REG_EPS;
        const bool constant = var <= (double)n * REG_EPS * var + nm * nm;
        mean[(int64_t)fold * D + col] = mu;
        scale[(int64_t)fold * D + col] = constant ? 1.0 : sqrt(var);
    }
    if (rg == 0 && col == D) ymean[fold] = y ? mu : 0.0;
}

// ----------------------------------------------------------------------------------------- Gram
// One 16x16 tile (ta >= tb) of the lower triangle, mirrored into the upper one.  Lane l holds
// A[l & 15][l >> 4] and B[l >> 4][l & 15] (k = four rows r), results D[(l >> 4) + 4 i][l & 15] in element i.
__global__ void __launch_bounds__(256) reg_gram_kernel(const double* __restrict__ x, int D, int Dp,
                                                       const double* __restrict__ y, int64_t N,
                                                       const int32_t* __restrict__ tr_idx,
                                                       const int64_t* __restrict__ tr_off,
                                                       const double* __restrict__ mean,
                                                       const double* __restrict__ scale,
                                                       const double* __restrict__ ymean, double* G) {
    __shared__ double part[4][256];
    const int fold = blockIdx.y, tile = blockIdx.x;
    const int64_t t0 = tr_off[fold], n = tr_off[fold + 1] - t0;
    int ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= tile) ++ta;
    const int tb = tile - ta * (ta + 1) / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kk = lane >> 4;
    const int ca = 16 * ta + m, cb = 16 * tb + m;
    // column c of Z~: c < D a standardised feature, c == D the centred target, c > D zero
    const double ma = ca < D ? mean[(int64_t)fold * D + ca] : (ca == D ? ymean[fold] : 0.0);
    const double mb = cb < D ? mean[(int64_t)fold * D + cb] : (cb == D ? ymean[fold] : 0.0);
    const double ia = ca < D ? 1.0 / scale[(int64_t)fold * D + ca] : 1.0;
    const double ib = cb < D ? 1.0 / scale[(int64_t)fold * D + cb] : 1.0;
    const bool ya = ca == D && y, yb = cb == D && y;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    constexpr int U = 4;  // k-steps whose loads are in flight together
    for (int64_t r0 = 4 * (int64_t)wave; r0 < n; r0 += 16 * U) {
        double a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = r0 + 16 * u + kk;
            a[u] = 0.0;
            b[u] = 0.0;
            if (r < n) {
                const int64_t row = fold_row(tr_idx, t0, r);
                if (ca < D)
                    a[u] = zscore(x[row * D + ca], ma, ia);
                else if (ya)
                    a[u] = y[(int64_t)fold * N + row] - ma;
                if (cb < D)
                    b[u] = zscore(x[row * D + cb], mb, ib);
                else if (yb)
                    b[u] = y[(int64_t)fold * N + row] - mb;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][(kk + 4 * i) * 16 + m] = acc[i];
    __syncthreads();
    const int e = threadIdx.x, row = 16 * ta + (e >> 4), col = 16 * tb + (e & 15);
    const double g = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
    double* Gf = G + (int64_t)fold * Dp * Dp;
    Gf[(int64_t)row * Dp + col] = g;
    if (ta != tb) Gf[(int64_t)col * Dp + row] = g;
}

// ------------------------------------------------------------------------ symmetric eigensolver
struct EighParams {
    const double* G;   // [F][Dp][Dp]
    double* A;         // workspace [F][De][De]
    double* lam;       // [F][D] eigenvalues clamped at 0, in the solver's order
    double* vt;        // [F][D][D] row i = eigenvector i
    int32_t* sweeps;   // [F]
    int32_t* status;   // [F]: 0 ok, 1 not converged in max_sweeps
    double* offnorm;   // [F][2]: final off-diagonal norm, the threshold D eps |G|_F
    int D, Dp, De, max_sweeps;
};

__global__ void __launch_bounds__(REG_NT) reg_eigh_kernel(EighParams p) {
    __shared__ double red[REG_NT];
    __shared__ double sc[FOLD_MAXD / 2], ss[FOLD_MAXD / 2];
    __shared__ int sp[FOLD_MAXD / 2], sq[FOLD_MAXD / 2];
    const int fold = blockIdx.x, tid = threadIdx.x, D = p.D, De = p.De, np = De / 2, n1 = De - 1;
    const double* G = p.G + (int64_t)fold * p.Dp * p.Dp;
    double* A = p.A + (int64_t)fold * De * De;
    double* Vt = p.vt + (int64_t)fold * D * D;
    double fro = 0.0;
    for (int e = tid; e < De * De; e += REG_NT) {
        const int i = e / De, j = e - i * De;
        const double g = i < D && j < D ? G[(int64_t)i * p.Dp + j] : 0.0;
        A[e] = g;
        fro += g * g;
    }
    for (int e = tid; e < D * D; e += REG_NT) Vt[e] = (e / D == e % D) ? 1.0 : 0.0;
    fro = sqrt(block_sum<REG_NT>(fro, red));
    const double thresh = (double)D * REG_EPS * fro;
    int sweep = 0;
    double off = 0.0;
    bool conv = false;
    for (;;) {
        double o = 0.0;
        for (int e = tid; e < De * De; e += REG_NT) {
            const int i = e / De, j = e - i * De;
            const double a = A[e];
            o += i != j ? a * a : 0.0;
        }
        off = sqrt(block_sum<REG_NT>(o, red));
        conv = off <= thresh;
        if (conv || sweep >= p.max_sweeps) break;  // uniform
        for (int r = 0; r < n1; ++r) {
            if (tid < np) {
                int a, b;
                if (tid == 0) {
                    a = n1;
                    b = r;
                } else {
                    a = (r + tid) % n1;
                    b = (r - tid + n1) % n1;
                }
                const int pp = a < b ? a : b, qq = a < b ? b : a;
                const double apq = A[(int64_t)pp * De + qq];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double app = A[(int64_t)pp * De + pp], aqq = A[(int64_t)qq * De + qq];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                }
                sp[tid] = pp;
                sq[tid] = qq;
                sc[tid] = c;
                ss[tid] = s;
            }
            __syncthreads();
            // rows: A <- J^T A, Vt <- J^T Vt
            for (int e = tid; e < np * De; e += REG_NT) {
                const int pr = e / De, k = e - pr * De;
                const double s = ss[pr];
                if (s != 0.0) {
                    const double c = sc[pr];
                    const int pp = sp[pr], qq = sq[pr];
                    const double ap = A[(int64_t)pp * De + k], aq = A[(int64_t)qq * De + k];
                    A[(int64_t)pp * De + k] = c * ap - s * aq;
                    A[(int64_t)qq * De + k] = s * ap + c * aq;
                    if (k < D) {  // s != 0 implies pp, qq < D: the padding row and column stay zero
                        const double vp = Vt[(int64_t)pp * D + k], vq = Vt[(int64_t)qq * D + k];
                        Vt[(int64_t)pp * D + k] = c * vp - s * vq;
                        Vt[(int64_t)qq * D + k] = s * vp + c * vq;
                    }
                }
            }
            __syncthreads();
            // columns: A <- A J
            for (int e = tid; e < np * De; e += REG_NT) {
                const int k = e / np, pr = e - k * np;
                const double s = ss[pr];
                if (s != 0.0) {
                    const double c = sc[pr];
                    const int pp = sp[pr], qq = sq[pr];
                    const double ap = A[(int64_t)k * De + pp], aq = A[(int64_t)k * De + qq];
                    A[(int64_t)k * De + pp] = c * ap - s * aq;
                    A[(int64_t)k * De + qq] = s * ap + c * aq;
                }
            }
            __syncthreads();
            if (tid < np && ss[tid] != 0.0) {  // the rotated pair is annihilated exactly
                A[(int64_t)sp[tid] * De + sq[tid]] = 0.0;
                A[(int64_t)sq[tid] * De + sp[tid]] = 0.0;
            }
            __syncthreads();
        }
        ++sweep;
    }
    for (int i = tid; i < D; i += REG_NT) {
        const double l = A[(int64_t)i * De + i];
        p.lam[(int64_t)fold * D + i] = l > 0.0 ? l : 0.0;
    }
    if (tid == 0) {
        p.sweeps[fold] = sweep;
        p.status[fold] = conv ? 0 : 1;
        p.offnorm[2 * fold] = off;
        p.offnorm[2 * fold + 1] = thresh;
    }
}

// ------------------------------------------------------------------------------------------- LR
// coef = V+ diag(1 / lam+) V+^T Z^T y over lam > tau lam_max: the minimum-norm least-squares solution.
__global__ void __launch_bounds__(256) reg_lr_kernel(const double* __restrict__ G, int D, int Dp,
                                                     const double* __restrict__ lam,
                                                     const double* __restrict__ vt, double tau, double* coef,
                                                     int32_t* rank, double* min_ratio) {
    __shared__ double red[256], sq[FOLD_MAXD], st[FOLD_MAXD];
    const int fold = blockIdx.x, tid = threadIdx.x;
    const double* Gf = G + (int64_t)fold * Dp * Dp;
    const double* Vt = vt + (int64_t)fold * D * D;
    const double l = tid < D ? lam[(int64_t)fold * D + tid] : 0.0;
    if (tid < D) sq[tid] = Gf[(int64_t)tid * Dp + D];
    const double lmax = block_max<256>(l, red);  // its barriers order the sq stores
    const bool keep = tid < D && lmax > 0.0 && l > tau * lmax;
    double t = 0.0;
    if (keep) {
        double pi = 0.0;
        for (int j = 0; j < D; ++j) pi += Vt[(int64_t)tid * D + j] * sq[j];
        t = pi / l;
    }
    st[tid] = t;
    const double nkeep = block_sum<256>(keep ? 1.0 : 0.0, red);  // also orders the st stores
    const double rmin = -block_max<256>(keep ? -(l / lmax) : -1.0, red);
    if (tid < D) {
        double c = 0.0;
        for (int i = 0; i < D; ++i) c += Vt[(int64_t)i * D + tid] * st[i];
        coef[(int64_t)fold * D + tid] = c;
    }
    if (tid == 0) {
        rank[fold] = (int32_t)nkeep;
        min_ratio[fold] = nkeep > 0.0 ? rmin : 0.0;
    }
}

// ------------------------------------------------------------------------------------------- BR
// sklearn BayesianRidge.fit (n_samples > n_features), in the eigenbasis of Z^T Z: with p = V^T Z^T y,
// coef = V (p / (lam + lambda / alpha)) and sse = |y - Z coef|^2 = y^T y - 2 c.p + sum lam c^2.
struct BrParams {
    const double* G;
    const double* lam;
    const double* vt;
    const int64_t* tr_off;
    double* coef;       // [F][D]
    double* hyper;      // [F][2]: alpha, lambda
    int32_t* n_iter;    // [F]
    double alpha_1, alpha_2, lambda_1, lambda_2, tol;
    int D, Dp, max_iter;
};

__global__ void __launch_bounds__(256) reg_br_kernel(BrParams p) {
    __shared__ double red[256], sq[FOLD_MAXD], sc[FOLD_MAXD];
    const int fold = blockIdx.x, tid = threadIdx.x, D = p.D;
    const double* Gf = p.G + (int64_t)fold * p.Dp * p.Dp;
    const double* Vt = p.vt + (int64_t)fold * D * D;
    const double n = (double)(p.tr_off[fold + 1] - p.tr_off[fold]);
    const double l = tid < D ? p.lam[(int64_t)fold * D + tid] : 0.0;
    if (tid < D) sq[tid] = Gf[(int64_t)tid * p.Dp + D];
    __syncthreads();
    double pi = 0.0;  // (V^T Z^T y)_tid
    if (tid < D)
        for (int j = 0; j < D; ++j) pi += Vt[(int64_t)tid * D + j] * sq[j];
    const double yy = Gf[(int64_t)D * p.Dp + D];
    double alpha = 1.0 / (yy / n + REG_EPS), lambda = 1.0;
    double coef = 0.0, coef_old = 0.0;
    int iter = 0;
    for (; iter < p.max_iter; ++iter) {
        const double ci = tid < D ? pi / (l + lambda / alpha) : 0.0;
        __syncthreads();
        sc[tid] = ci;
        __syncthreads();
        coef = 0.0;
        if (tid < D)
            for (int i = 0; i < D; ++i) coef += Vt[(int64_t)i * D + tid] * sc[i];
        const double cp = block_sum<256>(ci * pi, red);
        const double lcc = block_sum<256>(l * ci * ci, red);
        const double sse = (yy - 2.0 * cp) + lcc;
        const double gamma = block_sum<256>(tid < D ? (alpha * l) / (lambda + alpha * l) : 0.0, red);
        const double c2 = block_sum<256>(coef * coef, red);
        lambda = (gamma + 2.0 * p.lambda_1) / (c2 + 2.0 * p.lambda_2);
        alpha = (n - gamma + 2.0 * p.alpha_1) / (sse + 2.0 * p.alpha_2);
        const double dc = block_sum<256>(fabs(coef_old - coef), red);
        if (iter != 0 && dc < p.tol) break;  // uniform
        coef_old = coef;
    }
    const int n_iter = iter < p.max_iter ? iter + 1 : p.max_iter;
    const double ci = tid < D ? pi / (l + lambda / alpha) : 0.0;
    __syncthreads();
    sc[tid] = ci;
    __syncthreads();
    if (tid < D) {
        coef = 0.0;
        for (int i = 0; i < D; ++i) coef += Vt[(int64_t)i * D + tid] * sc[i];
        p.coef[(int64_t)fold * D + tid] = coef;
    }
    if (tid == 0) {
        p.hyper[2 * fold] = alpha;
        p.hyper[2 * fold + 1] = lambda;
        p.n_iter[fold] = n_iter;
    }
}

// ------------------------------------------------------------------------------------------- EN
// minimise 1/2 w^T Q w - q.w + a r |w|_1 + 1/2 a (1 - r) |w|^2, Q = Z^T Z / n, q = Z^T yc / n (sklearn's
// ElasticNet objective).  The smooth gradient h = Q w - q is kept and updated by delta Q[:, j] after each
// coordinate.  z_j = g_j + a r sign(w_j) where w_j != 0 and max(|g_j| - a r, 0) where w_j == 0, with
// g = h + a (1 - r) w, is a subgradient: the fit stops at |z|_2 <= tol, checked on an h recomputed from w.
struct EnParams {
    const double* G;
    const int64_t* tr_off;
    double* coef;      // [F][D]
    double* res;       // [F][2]: |z|, tol
    int32_t* sweeps;   // [F]
    int32_t* status;   // [F]: 0 ok, 1 not converged in max_sweeps
    double alpha, l1_ratio, tol_rel, tol_abs;
    int D, Dp, max_sweeps;
};

__global__ void __launch_bounds__(256) reg_en_kernel(EnParams p) {
    __shared__ double red[256], sw[FOLD_MAXD], sh[FOLD_MAXD];
    const int fold = blockIdx.x, tid = threadIdx.x, D = p.D, Dp = p.Dp;
    const double* Gf = p.G + (int64_t)fold * Dp * Dp;
    const double inv_n = 1.0 / (double)(p.tr_off[fold + 1] - p.tr_off[fold]);
    const double l1 = p.alpha * p.l1_ratio, l2 = p.alpha * (1.0 - p.l1_ratio);
    const double qj = tid < D ? Gf[(int64_t)tid * Dp + D] * inv_n : 0.0;
    const double tol = p.tol_abs > 0.0 ? p.tol_abs : p.tol_rel * block_max<256>(fabs(qj), red);
    sw[tid] = 0.0;
    sh[tid] = -qj;
    __syncthreads();
    int sweep = 0;
    double zn = 0.0;
    bool conv = false;
    for (;;) {
        // |z| on the running h; when it passes, once more on h = Q w - q recomputed from w
        for (int pass = 0; pass < 2; ++pass) {
            double z = 0.0;
            if (tid < D) {
                const double w = sw[tid], g = sh[tid] + l2 * w;
                z = w != 0.0 ? g + (w > 0.0 ? l1 : -l1) : fmax(fabs(g) - l1, 0.0);
            }
            zn = sqrt(block_sum<256>(z * z, red));
            conv = zn <= tol;
            if (!conv || pass == 1) break;  // uniform
            double h = 0.0;
            if (tid < D) {
                for (int k = 0; k < D; ++k) h += Gf[(int64_t)k * Dp + tid] * sw[k];
                h = h * inv_n - qj;
            }
            __syncthreads();
            sh[tid] = h;
            __syncthreads();
        }
        if (conv || sweep >= p.max_sweeps) break;  // uniform
        for (int j = 0; j < D; ++j) {
            const double wj = sw[j];
            const double qjj = Gf[(int64_t)j * Dp + j] * inv_n;
            const double tmp = qjj * wj - sh[j];
            const double mag = fabs(tmp) - l1;
            const double wn = mag > 0.0 ? (tmp > 0.0 ? mag : -mag) / (qjj + l2) : 0.0;
            const double delta = wn - wj;
            __syncthreads();  // every thread has read sw[j] and sh[j]
            if (delta != 0.0) {  // uniform
                if (tid < D) sh[tid] += delta * (Gf[(int64_t)j * Dp + tid] * inv_n);
                if (tid == j) sw[j] = wn;
                __syncthreads();
            }
        }
        ++sweep;
    }
    if (tid < D) p.coef[(int64_t)fold * D + tid] = sw[tid];
    if (tid == 0) {
        p.res[2 * fold] = zn;
        p.res[2 * fold + 1] = tol;
        p.sweeps[fold] = sweep;
        p.status[fold] = conv ? 0 : 1;
    }
}

// -------------------------------------------------------------------------------------- predict
// out[f][i] = sum_k (x[i][k] - mean[f][k]) (1 / scale[f][k]) coef[f][k] + ymean[f]: sixteen lanes per row,
// butterfly sum.
__global__ void __launch_bounds__(REG_NT) reg_predict_kernel(const double* __restrict__ x, int64_t N, int D,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ scale,
                                                             const double* __restrict__ coef,
                                                             const double* __restrict__ ymean, double* out) {
    __shared__ double sm[FOLD_MAXD], sv[FOLD_MAXD];
    const int fold = blockIdx.y, tid = threadIdx.x;
    if (tid < D) {
        sm[tid] = mean[(int64_t)fold * D + tid];
        sv[tid] = (1.0 / scale[(int64_t)fold * D + tid]) * coef[(int64_t)fold * D + tid];
    }
    __syncthreads();
    const int sub = tid & 15, grp = tid >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * REG_NT;
    for (int64_t rr = 0; rr < REG_NT; rr += REG_NT / 16) {
        const int64_t r = r0 + rr + grp;
        const bool ok = r < N;
        double acc = 0.0;
        if (ok)
            for (int k = sub; k < D; k += 16) acc += zscore(x[r * D + k], sm[k], sv[k]);
        acc = lane16_sum(acc);
        if (ok && sub == 0) out[(int64_t)fold * N + r] = acc + ymean[fold];
    }
}

// ------------------------------------------------------------------------------------------ KNR
// |z_i|^2 of every standardised row, per fold: sixteen lanes per row.
__global__ void __launch_bounds__(REG_NT) knn_norm_kernel(const double* __restrict__ x, int64_t N, int D,
                                                          const double* __restrict__ mean,
                                                          const double* __restrict__ scale, double* norm) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    const int fold = blockIdx.y, tid = threadIdx.x;
    stage_scaler(sm, si, mean, scale, fold, D);
    __syncthreads();
    const int sub = tid & 15, grp = tid >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * REG_NT;
    for (int64_t rr = 0; rr < REG_NT; rr += REG_NT / 16) {
        const int64_t r = r0 + rr + grp;
        const bool ok = r < N;
        double acc = 0.0;
        if (ok)
            for (int k = sub; k < D; k += 16) {
                const double z = zscore(x[r * D + k], sm[k], si[k]);
                acc += z * z;
            }
        acc = lane16_sum(acc);
        if (ok && sub == 0) norm[(int64_t)fold * N + r] = acc;
    }
}

// dist[f][i][b] = max(|z_i|^2 + |z_t|^2 - 2 z_i.z_t, 0), t = the fold's b-th training row: a wave per
// 16 (queries) x 16 (training rows) tile, four tiles along the training rows per workgroup.  The fold's
// slab starts at N * tr_off[f] and has row stride n_f.
__global__ void __launch_bounds__(256) knn_dist_kernel(const double* __restrict__ x, int64_t N, int D,
                                                       const int32_t* __restrict__ tr_idx,
                                                       const int64_t* __restrict__ tr_off,
                                                       const double* __restrict__ mean,
                                                       const double* __restrict__ scale,
                                                       const double* __restrict__ norm, double* dist) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    const int fold = blockIdx.z, tid = threadIdx.x;
    const int64_t t0 = tr_off[fold], n = tr_off[fold + 1] - t0;
    if ((int64_t)blockIdx.x * 64 >= n) return;  // uniform: the grid covers the largest fold
    stage_scaler_padded<256>(sm, si, mean, scale, fold, D);
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.y * 16, b0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    const int64_t qa = q0 + m, bb = b0 + m;
    const bool oka = qa < N, okb = bb < n;
    const double* rowa = x + (oka ? qa : 0) * D;
    const double* rowb = x + (okb ? fold_row(tr_idx, t0, bb) : 0) * D;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + kk;
        const bool okk = k < D;
        const double a = oka && okk ? zscore(rowa[k], sm[k], si[k]) : 0.0;
        const double b = okb && okk ? zscore(rowb[k], sm[k], si[k]) : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    if (!okb) return;
    const double nb = norm[(int64_t)fold * N + fold_row(tr_idx, t0, bb)];
    double* slab = dist + N * t0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t q = q0 + kk + 4 * i;
        if (q < N) slab[q * n + bb] = sqdist(norm[(int64_t)fold * N + q], nb, acc[i]);
    }
}

constexpr int KNN_NT = 256;

__device__ __forceinline__ int knn_block_count(int v, int* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = KNN_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per query and fold.  The k-th smallest key T is built bit by bit (keys are non-negative
// doubles, so their bit patterns order as unsigned integers): the largest T with count(key < T) <= k - 1.
// Selected: every key < T and the first k - count(key < T) positions with key == T; written in position
// order, and the estimate is the mean of their targets summed in that order.
__global__ void __launch_bounds__(KNN_NT) knn_select_kernel(const double* __restrict__ dist, int64_t N,
                                                            const double* __restrict__ y,
                                                            const int32_t* __restrict__ tr_idx,
                                                            const int64_t* __restrict__ tr_off, int k, double* est,
                                                            int32_t* nbr) {
    __shared__ int red[KNN_NT];
    __shared__ int base_lt[KNN_NT], base_eq[KNN_NT];
    __shared__ double sy[KNN_NT];
    const int fold = blockIdx.y, tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t t0 = tr_off[fold];
    const int n = (int)(tr_off[fold + 1] - t0);
    const unsigned long long* key = (const unsigned long long*)(dist + N * t0 + q * n);
    unsigned long long T = 0;
    for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long cand = T | (1ull << bit);
        int c = 0;
        for (int j = tid; j < n; j += KNN_NT) c += key[j] < cand ? 1 : 0;
        if (knn_block_count(c, red) <= k - 1) T = cand;  // uniform
    }
    const int chunk = (n + KNN_NT - 1) / KNN_NT;
    const int j0 = tid * chunk < n ? tid * chunk : n, j1 = j0 + chunk < n ? j0 + chunk : n;
    int lt = 0, eq = 0;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long v = key[j];
        lt += v < T ? 1 : 0;
        eq += v == T ? 1 : 0;
    }
    __syncthreads();
    base_lt[tid] = lt;
    base_eq[tid] = eq;
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0;
        for (int t = 0; t < KNN_NT; ++t) {
            const int x0 = base_lt[t], x1 = base_eq[t];
            base_lt[t] = a;
            base_eq[t] = b;
            a += x0;
            b += x1;
        }
        red[0] = a;
    }
    __syncthreads();
    const int need = k - red[0];  // ties taken at the k-th distance, >= 1
    int32_t* out = nbr + ((int64_t)fold * N + q) * k;
    int bl = base_lt[tid], be = base_eq[tid];
    for (int j = j0; j < j1; ++j) {
        const unsigned long long v = key[j];
        if (v < T) {
            out[bl + (be < need ? be : need)] = j;
            ++bl;
        } else if (v == T) {
            if (be < need) out[bl + be] = j;
            ++be;
        }
    }
    __syncthreads();  // the positions are visible to the whole workgroup
    double acc = 0.0;
    for (int c0 = 0; c0 < k; c0 += KNN_NT) {
        const int c = c0 + tid;
        if (c < k) sy[tid] = y[(int64_t)fold * N + fold_row(tr_idx, t0, out[c])];
        __syncthreads();
        if (tid == 0) {
            const int m = k - c0 < KNN_NT ? k - c0 : KNN_NT;
            for (int i = 0; i < m; ++i) acc += sy[i];
        }
        __syncthreads();
    }
    if (tid == 0) est[(int64_t)fold * N + q] = acc / (double)k;
}

// ------------------------------------------------------------------------------------- the C-ABI
static size_t reg_ws_doubles(int64_t folds, int64_t D, int64_t N, int64_t T) {
    const size_t eigh = (size_t)folds * reg_de(D) * reg_de(D);
    const size_t knn = (size_t)N * (size_t)T + (size_t)folds * (size_t)N;
    return eigh > knn ? eigh : knn;
}

extern "C" int64_t edgedet_reg_workspace_size(int32_t folds, int64_t D, int64_t N, int64_t total_rows) {
    if (folds < 1 || !fold_dims_ok(D) || N < 0 || total_rows < 0) return -1;
    return (int64_t)(reg_ws_doubles(folds, D, N, total_rows) * sizeof(double));
}

extern "C" int edgedet_reg_scaler(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                                  const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, double* mean,
                                  double* scale, double* ymean, void* stream) {
    EDGEDET_REQUIRE(x && tr_off_host && tr_off && mean && scale && ymean, "reg_scaler: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1, "reg_scaler: 1 <= features <= 255");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, N, tr_idx != nullptr), "reg_scaler: fold offsets");
    hipLaunchKernelGGL(reg_scaler_kernel, dim3((unsigned)folds), dim3(REG_NT), 0, (hipStream_t)stream, x, (int)D, y, N,
                       tr_idx, tr_off, mean, scale, ymean);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_gram(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                                const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                                const double* scale, const double* ymean, double* G, void* stream) {
    EDGEDET_REQUIRE(x && tr_off_host && tr_off && mean && scale && ymean && G, "reg_gram: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1, "reg_gram: 1 <= features <= 255");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, N, tr_idx != nullptr), "reg_gram: fold offsets");
    const int Dp = (int)reg_dp(D), nt = Dp / 16;
    hipLaunchKernelGGL(reg_gram_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)folds), dim3(256), 0,
                       (hipStream_t)stream, x, (int)D, Dp, y, N, tr_idx, tr_off, mean, scale, ymean, G);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_eigh(const double* G, int64_t D, int32_t folds, void* ws, int64_t ws_bytes,
                                int32_t max_sweeps, double* lam, double* vt, int32_t* sweeps, int32_t* status,
                                double* offnorm, void* stream) {
    EDGEDET_REQUIRE(G && ws && lam && vt && sweeps && status && offnorm, "reg_eigh: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && folds >= 1 && folds <= 65535 && max_sweeps >= 1, "reg_eigh: 1 <= order <= 255");
    EDGEDET_REQUIRE(ws_bytes >= (int64_t)(reg_ws_doubles(folds, D, 0, 0) * sizeof(double)),
                    "reg_eigh: workspace smaller than edgedet_reg_workspace_size");
    EighParams p{};
    p.G = G;
    p.A = (double*)ws;
    p.lam = lam;
    p.vt = vt;
    p.sweeps = sweeps;
    p.status = status;
    p.offnorm = offnorm;
    p.D = (int)D;
    p.Dp = (int)reg_dp(D);
    p.De = (int)reg_de(D);
    p.max_sweeps = max_sweeps;
    hipLaunchKernelGGL(reg_eigh_kernel, dim3((unsigned)folds), dim3(REG_NT), 0, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_fit_lr(const double* G, int64_t D, int32_t folds, const double* lam, const double* vt,
                                  double tau, double* coef, int32_t* rank, double* min_ratio, void* stream) {
    EDGEDET_REQUIRE(G && lam && vt && coef && rank && min_ratio, "reg_fit_lr: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && folds >= 1 && folds <= 65535 && tau >= 0.0, "reg_fit_lr: 1 <= features <= 255");
    hipLaunchKernelGGL(reg_lr_kernel, dim3((unsigned)folds), dim3(256), 0, (hipStream_t)stream, G, (int)D,
                       (int)reg_dp(D), lam, vt, tau, coef, rank, min_ratio);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_fit_br(const double* G, int64_t D, const int64_t* tr_off_host, const int64_t* tr_off,
                                  int32_t folds, const double* lam, const double* vt, double alpha_1, double alpha_2,
                                  double lambda_1, double lambda_2, double tol, int32_t max_iter, double* coef,
                                  double* hyper, int32_t* n_iter, void* stream) {
    EDGEDET_REQUIRE(G && tr_off_host && tr_off && lam && vt && coef && hyper && n_iter, "reg_fit_br: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && folds >= 1 && folds <= 65535 && max_iter >= 1, "reg_fit_br: 1 <= features <= 255");
    for (int f = 0; f < folds; ++f)
        EDGEDET_REQUIRE(tr_off_host[f + 1] - tr_off_host[f] > D, "reg_fit_br: needs more training rows than features");
    BrParams p{};
    p.G = G;
    p.lam = lam;
    p.vt = vt;
    p.tr_off = tr_off;
    p.coef = coef;
    p.hyper = hyper;
    p.n_iter = n_iter;
    p.alpha_1 = alpha_1;
    p.alpha_2 = alpha_2;
    p.lambda_1 = lambda_1;
    p.lambda_2 = lambda_2;
    p.tol = tol;
    p.D = (int)D;
    p.Dp = (int)reg_dp(D);
    p.max_iter = max_iter;
    hipLaunchKernelGGL(reg_br_kernel, dim3((unsigned)folds), dim3(256), 0, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_fit_en(const double* G, int64_t D, const int64_t* tr_off_host, const int64_t* tr_off,
                                  int32_t folds, double alpha, double l1_ratio, double tol_rel, double tol_abs,
                                  int32_t max_sweeps, double* coef, double* res, int32_t* sweeps, int32_t* status,
                                  void* stream) {
    EDGEDET_REQUIRE(G && tr_off_host && tr_off && coef && res && sweeps && status, "reg_fit_en: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && folds >= 1 && folds <= 65535 && max_sweeps >= 1, "reg_fit_en: 1 <= features <= 255");
    EDGEDET_REQUIRE(alpha > 0.0 && l1_ratio >= 0.0 && l1_ratio < 1.0 && (tol_abs > 0.0 || tol_rel > 0.0),
                    "reg_fit_en: alpha > 0, 0 <= l1_ratio < 1 (a strongly convex objective), a positive tolerance");
    for (int f = 0; f < folds; ++f)
        EDGEDET_REQUIRE(tr_off_host[f + 1] - tr_off_host[f] >= 1, "reg_fit_en: an empty training set");
    EnParams p{};
    p.G = G;
    p.tr_off = tr_off;
    p.coef = coef;
    p.res = res;
    p.sweeps = sweeps;
    p.status = status;
    p.alpha = alpha;
    p.l1_ratio = l1_ratio;
    p.tol_rel = tol_rel;
    p.tol_abs = tol_abs;
    p.D = (int)D;
    p.Dp = (int)reg_dp(D);
    p.max_sweeps = max_sweeps;
    hipLaunchKernelGGL(reg_en_kernel, dim3((unsigned)folds), dim3(256), 0, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_reg_predict(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                                   const double* coef, const double* ymean, int32_t folds, double* out,
                                   void* stream) {
    EDGEDET_REQUIRE(x && mean && scale && coef && ymean && out, "reg_predict: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && folds >= 1 && folds <= 65535, "reg_predict: 1 <= features <= 255");
    hipLaunchKernelGGL(reg_predict_kernel, dim3((unsigned)cdiv(N, REG_NT), (unsigned)folds), dim3(REG_NT), 0,
                       (hipStream_t)stream, x, N, (int)D, mean, scale, coef, ymean, out);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_knn_fit_predict(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                                       const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds,
                                       const double* mean, const double* scale, int32_t k, void* ws, int64_t ws_bytes,
                                       double* est, int32_t* nbr, void* stream) {
    EDGEDET_REQUIRE(x && y && tr_idx && tr_off_host && tr_off && mean && scale && ws && est && nbr,
                    "knn_fit_predict: null pointer");
    EDGEDET_REQUIRE(fold_dims_ok(D) && N >= 1 && N <= 65535 * 16, "knn_fit_predict: 1 <= features <= 255, rows <= 1,048,560");
    EDGEDET_REQUIRE(folds_ok(tr_off_host, folds, N, true), "knn_fit_predict: fold offsets");
    int64_t nmax = 0;
    for (int f = 0; f < folds; ++f) {
        const int64_t n = tr_off_host[f + 1] - tr_off_host[f];
        EDGEDET_REQUIRE(k >= 1 && k <= n, "knn_fit_predict: 1 <= n_neighbors <= training rows of every fold");
        nmax = n > nmax ? n : nmax;
    }
    const int64_t T = tr_off_host[folds];
    EDGEDET_REQUIRE(ws_bytes >= (int64_t)(reg_ws_doubles(folds, D, N, T) * sizeof(double)),
                    "knn_fit_predict: workspace smaller than edgedet_reg_workspace_size");
    hipStream_t st = (hipStream_t)stream;
    double* dist = (double*)ws;
    double* norm = dist + N * T;
    hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)cdiv(N, REG_NT), (unsigned)folds), dim3(REG_NT), 0, st, x, N,
                       (int)D, mean, scale, norm);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_dist_kernel, dim3((unsigned)cdiv(nmax, 64), (unsigned)cdiv(N, 16), (unsigned)folds),
                       dim3(256), 0, st, x, N, (int)D, tr_idx, tr_off, mean, scale, norm, dist);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)N, (unsigned)folds), dim3(KNN_NT), 0, st, dist, N, y, tr_idx,
                       tr_off, (int)k, est, nbr);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

}  // namespace edgedet
