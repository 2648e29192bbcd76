// The two comparison baselines of baseline.py on the device, every cross-validation fold in flight.
//
// DCSB (baseline.py:67-152 fit_dcsb), bit-exact, float64 and integer arithmetic only.
//   dcsb_fit_kernel: one workgroup per fold.  (1) the bisection for the confidence threshold
//   (:96-107, bounded at DCSB_MAX_STEPS halvings: the reference loops forever when the count of
//   detections cannot meet the label count), (2) filter_box (:80-88) at that threshold and at 0.5 for
//   every image, (3) the grid search over n_thresh 1..10 x the area grid (:111-126) with accuracies as
//   integer counts, one cell per thread, and the reference's tie-breaks (first maximum along the area
//   axis, a strictly greater accuracy to replace an earlier n_thresh), (4) the estimate of every image
//   (:129-141; the host splits it by the fold's mask).
//
// Adaptive Feeding (baseline.py:29-64 fit_af): LinearSVC(dual=False, class_weight={0: 1, 1: w}), i.e.
//   f(v) = 1/2 |v|^2 + sum_i C_i max(0, 1 - s_i v.x~_i)^2,  x~ = (x, 1), s = +-1,
//   solved per fold by a damped Newton method in float64:
//   svm_eval_kernel    one workgroup per fold: d = X~ v, the active set (margin < 1), f, the gradient
//                      and its norm; a fold whose norm is <= tol is done;
//   svm_hessian_kernel H = I + X~^T diag(2 C [margin < 1]) X~ with v_mfma_f64_16x16x4_f64, one
//                      workgroup per 16x16 tile of the lower triangle and fold, its four waves splitting
//                      the rows and summed in a fixed order (deterministic);
//   svm_step_kernel    one workgroup per fold: Cholesky of H in its HBM workspace (a 206 x 206 float64
//                      matrix does not fit LDS), the two triangular solves, an Armijo backtracking line
//                      search and the update of v.
//   X~ is [N][Dp] with Dp = D + 1 padded to a multiple of 16 by zero columns: a zero column has
//   H[j][.] = e_j and gradient v_j, so its weight stays exactly 0 from a zero start.
#include <vector>

#include "fold_math.hpp"
#include "kernels.hpp"

namespace edgedet {

// ------------------------------------------------------------------------------------------ DCSB
constexpr int DCSB_NT = 256;
constexpr int DCSB_MAX_STEPS = 64;
constexpr int DCSB_MAX_N = 10;     // n_thresh 1..10
constexpr int DCSB_MAX_GRID = 128;  // area thresholds

struct DcsbParams {
    const double* conf;      // [n_det] flattened per image
    const double* area;      // [n_det]
    const int64_t* det_off;  // [N + 1]
    const int64_t* label_num;  // [N]
    const int32_t* reward;   // [N] 0 / 1
    const int32_t* tr_idx;   // training images of every fold
    const int64_t* tr_off;   // [F + 1]
    const double* grid;      // [n_grid]
    int32_t* ws_num;         // [F][2][N]: count of conf > conf_thresh, count of conf > 0.5
    double* ws_area;         // [F][N]: minimum area among conf > conf_thresh (0 when none)
    double* thresh;          // [F][2]: conf_thresh, area_thresh
    int32_t* num_thresh;     // [F]
    int32_t* est;            // [F][N]
    int32_t* status;         // [F]: 0 ok, 1 bisection did not converge, 2 no cell with a positive accuracy
    int32_t* steps;          // [F] bisection steps taken
    int64_t N;
    int n_grid;
};

__global__ void __launch_bounds__(DCSB_NT) dcsb_fit_kernel(DcsbParams p) {
    const int fold = blockIdx.x, tid = threadIdx.x;
    __shared__ long long red[DCSB_NT];
    __shared__ int cell[DCSB_MAX_N * DCSB_MAX_GRID];
    __shared__ int sh_n, sh_a;
    const int32_t* tr = p.tr_idx + p.tr_off[fold];
    const int64_t ntr = p.tr_off[fold + 1] - p.tr_off[fold];
    int32_t* est_num = p.ws_num + (int64_t)fold * 2 * p.N;
    int32_t* det_num = est_num + p.N;
    double* est_area = p.ws_area + (int64_t)fold * p.N;

    long long lab = 0;
    for (int64_t r = tid; r < ntr; r += DCSB_NT) lab += p.label_num[tr[r]];
    const long long sum_label = block_sum<DCSB_NT>(lab, red);

    // (1) bisection: low = mid when count(conf > mid) - sum(label) >= 0, otherwise high = mid
    double low = 0.0, high = 1.0, mid = 0.0;
    bool found = false;
    int steps = 0;
    while (!found && steps < DCSB_MAX_STEPS) {
        mid = (low + high) / 2;
        long long c = 0;
        for (int64_t r = tid; r < ntr; r += DCSB_NT) {
            const int64_t i = tr[r];
            for (int64_t j = p.det_off[i]; j < p.det_off[i + 1]; ++j) c += p.conf[j] > mid ? 1 : 0;
        }
        const long long diff = block_sum<DCSB_NT>(c, red) - sum_label;
        if (diff >= 0)
            low = mid;
        else
            high = mid;
        found = (double)(diff < 0 ? -diff : diff) / (double)sum_label < 1e-4;  // inf / nan never pass
        ++steps;
    }
    if (tid == 0) {
        p.steps[fold] = steps;
        p.status[fold] = found ? 0 : 1;
        p.thresh[2 * fold] = mid;
        p.thresh[2 * fold + 1] = 0.0;
        p.num_thresh[fold] = 0;
    }
    if (!found) return;  // uniform
    const double conf_thresh = mid;

    // (2) filter_box at conf_thresh and at 0.5, every image of the dataset
    for (int64_t i = tid; i < p.N; i += DCSB_NT) {
        int ne = 0, nd = 0;
        double amin = 0.0;
        for (int64_t j = p.det_off[i]; j < p.det_off[i + 1]; ++j) {
            const double c = p.conf[j];
            if (c > conf_thresh) {
                const double a = p.area[j];
                amin = ne == 0 ? a : (a < amin ? a : amin);
                ++ne;
            }
            nd += c > 0.5 ? 1 : 0;
        }
        est_num[i] = ne;
        det_num[i] = nd;
        est_area[i] = amin;
    }
    __syncthreads();

    // (3) grid search: the number of training images with estimate == reward, one cell per thread
    const int n_cell = DCSB_MAX_N * p.n_grid;
    for (int c = tid; c < n_cell; c += DCSB_NT) {
        const int n_thresh = c / p.n_grid + 1;
        const double a_thresh = p.grid[c % p.n_grid];
        int hit = 0;
        for (int64_t r = 0; r < ntr; ++r) {
            const int64_t i = tr[r];
            const int ne = est_num[i];
            const int e = ne != det_num[i] && (ne > n_thresh || est_area[i] < a_thresh) ? 1 : 0;
            hit += e == p.reward[i] ? 1 : 0;
        }
        cell[c] = hit;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0, bn = 0, ba = 0;
        for (int n = 0; n < DCSB_MAX_N; ++n) {
            int a_best = 0;
            for (int a = 1; a < p.n_grid; ++a)
                if (cell[n * p.n_grid + a] > cell[n * p.n_grid + a_best]) a_best = a;  // np.argmax: first maximum
            if (cell[n * p.n_grid + a_best] > best) {
                best = cell[n * p.n_grid + a_best];
                bn = n + 1;
                ba = a_best;
            }
        }
        sh_n = bn;
        sh_a = ba;
        if (bn == 0) p.status[fold] = 2;
        p.num_thresh[fold] = bn;
        p.thresh[2 * fold + 1] = p.grid[ba];
    }
    __syncthreads();
    const int num_thresh = sh_n;
    const double area_thresh = p.grid[sh_a];

    // (4) the estimate of every image
    for (int64_t i = tid; i < p.N; i += DCSB_NT) {
        const int ne = est_num[i];
        p.est[(int64_t)fold * p.N + i] = ne != det_num[i] && (ne > num_thresh || est_area[i] < area_thresh) ? 1 : 0;
    }
}

extern "C" int edgedet_dcsb_fit(const double* conf, const double* area, const int64_t* det_off, int64_t N,
                                const int64_t* label_num, const int32_t* reward, const int32_t* tr_idx,
                                const int64_t* tr_off, int32_t folds, const double* grid, int32_t n_grid,
                                int32_t* ws_num, double* ws_area, double* thresh, int32_t* num_thresh, int32_t* est,
                                int32_t* status, int32_t* steps, void* stream) {
    EDGEDET_REQUIRE(conf && area && det_off && label_num && reward && tr_idx && tr_off && grid && ws_num && ws_area &&
                        thresh && num_thresh && est && status && steps,
                    "dcsb_fit: null pointer");
    EDGEDET_REQUIRE(N >= 1 && folds >= 1 && n_grid >= 1 && n_grid <= DCSB_MAX_GRID, "dcsb_fit: sizes (area grid <= 128)");
    DcsbParams p{};
    p.conf = conf;
    p.area = area;
    p.det_off = det_off;
    p.label_num = label_num;
    p.reward = reward;
    p.tr_idx = tr_idx;
    p.tr_off = tr_off;
    p.grid = grid;
    p.ws_num = ws_num;
    p.ws_area = ws_area;
    p.thresh = thresh;
    p.num_thresh = num_thresh;
    p.est = est;
    p.status = status;
    p.steps = steps;
    p.N = N;
    p.n_grid = n_grid;
    hipLaunchKernelGGL(dcsb_fit_kernel, dim3((unsigned)folds), dim3(DCSB_NT), 0, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------ Adaptive Feeding
constexpr int SVM_NT = 1024;
constexpr int SVM_MAXD = 256;  // padded width (features + bias)
constexpr int SVM_LS_MAX = 40;  // halvings of the line search

struct SvmWs {  // the per-call workspace, carved out of one buffer
    double* H;     // [F][Dp][Dp]
    double* d;     // [T] decision value of every training row (T = tr_off[F])
    double* w;     // [T] 2 C [margin < 1]
    double* q;     // [T] gradient coefficient, then X~ p of the line search
    double* g;     // [F][Dp]
    double* f;     // [F]
    int32_t* done;  // [F]
};

static size_t svm_ws_doubles(int64_t folds, int64_t Dp, int64_t T) {
    return (size_t)folds * Dp * Dp + 3 * (size_t)T + (size_t)folds * Dp + 2 * (size_t)folds;
}

static SvmWs svm_carve(void* ws, int64_t folds, int64_t Dp, int64_t T) {
    SvmWs s;
    s.H = (double*)ws;
    s.d = s.H + folds * Dp * Dp;
    s.w = s.d + T;
    s.q = s.w + T;
    s.g = s.q + T;
    s.f = s.g + folds * Dp;
    s.done = (int32_t*)(s.f + folds);  // [F] int32 within F doubles
    return s;
}

struct SvmParams {
    const double* x;  // [N][Dp]
    const int32_t* y;  // [N] 0 / 1
    const int32_t* tr_idx;
    const int64_t* tr_off;
    double* v;  // [F][Dp]
    SvmWs ws;
    int32_t* iters;   // [F]
    double* gnorm;    // [F]
    int32_t* status;  // [F]: 0 ok, 2 line search failed, 3 Hessian not positive definite
    double pos_weight, tol;
    int Dp;
};

// out[r] = x[idx[r]] . vec for r < n: sixteen lanes per row (128-byte loads), butterfly sum.
__device__ __forceinline__ void svm_rows_dot(const double* __restrict__ x, int Dp, const int32_t* __restrict__ idx,
                                             int64_t n, const double* vec, double* __restrict__ out) {
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    for (int64_t r0 = 0; r0 < n; r0 += SVM_NT / 16) {
        const int64_t r = r0 + grp;
        const bool ok = r < n;
        const double* row = x + (int64_t)(ok ? (idx ? idx[r] : r) : 0) * Dp;
        double acc = 0.0;
        if (ok)
            for (int k = sub; k < Dp; k += 16) acc += row[k] * vec[k];
        acc = lane16_sum(acc);
        if (ok && sub == 0) out[r] = acc;
    }
}

__global__ void __launch_bounds__(SVM_NT) svm_eval_kernel(SvmParams p) {
    const int fold = blockIdx.x, tid = threadIdx.x, Dp = p.Dp;
    __shared__ double sv[SVM_MAXD];
    __shared__ double red[SVM_NT];
    if (p.ws.done[fold]) return;
    const int64_t t0 = p.tr_off[fold], n = p.tr_off[fold + 1] - t0;
    const int32_t* idx = p.tr_idx + t0;
    double* d = p.ws.d + t0;
    double* w = p.ws.w + t0;
    double* q = p.ws.q + t0;
    double* v = p.v + (int64_t)fold * Dp;
    if (tid < Dp) sv[tid] = v[tid];
    __syncthreads();
    svm_rows_dot(p.x, Dp, idx, n, sv, d);
    __syncthreads();
    double loss = 0.0;
    for (int64_t r = tid; r < n; r += SVM_NT) {
        const bool pos = p.y[idx[r]] != 0;
        const double s = pos ? 1.0 : -1.0, C = pos ? p.pos_weight : 1.0;
        const double h = 1.0 - s * d[r];
        const bool act = h > 0.0;
        w[r] = act ? 2.0 * C : 0.0;
        q[r] = act ? 2.0 * C * s * h : 0.0;
        loss += act ? C * h * h : 0.0;
    }
    loss = block_sum<SVM_NT>(loss, red);  // also orders the q stores before the loads below
    // gradient g = v - X~^T q: a column per thread, four row groups summed in a fixed order
    const int col = tid & (SVM_MAXD - 1), rg = tid >> 8;
    double acc = 0.0;
    if (col < Dp)
        for (int64_t r = rg; r < n; r += SVM_NT / SVM_MAXD) acc += q[r] * p.x[(int64_t)idx[r] * Dp + col];
    __syncthreads();
    red[tid] = acc;
    __syncthreads();
    if (tid < Dp) {
        const double gj = sv[tid] - (((red[tid] + red[SVM_MAXD + tid]) + red[2 * SVM_MAXD + tid]) + red[3 * SVM_MAXD + tid]);
        p.ws.g[(int64_t)fold * Dp + tid] = gj;
        red[tid] = gj;
    }
    __syncthreads();
    if (tid == 0) {
        double gg = 0.0, vv = 0.0;
        for (int k = 0; k < Dp; ++k) {
            gg += red[k] * red[k];
            vv += sv[k] * sv[k];
        }
        const double gn = sqrt(gg);
        p.ws.f[fold] = 0.5 * vv + loss;
        p.gnorm[fold] = gn;
        if (gn <= p.tol) p.ws.done[fold] = 1;
    }
}

// H[a][b] = [a == b] + sum_r w[r] x[idx[r]][a] x[idx[r]][b] for one 16x16 tile (ta >= tb) of the lower
// triangle, mirrored into the upper one.  v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15] (k = four rows r), and results D[(l >> 4) + 4 i][l & 15] in element i.
__device__ __forceinline__ void svm_hessian_tile(const double* __restrict__ x, int Dp, const int32_t* __restrict__ idx,
                                                 int64_t n, const double* __restrict__ w, double* __restrict__ H,
                                                 int tile, double (*part)[256]) {
    int ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= tile) ++ta;
    const int tb = tile - ta * (ta + 1) / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, kk = lane >> 4;
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
                const double* row = x + (int64_t)(idx ? idx[r] : r) * Dp;
                a[u] = w[r] * row[16 * ta + m];
                b[u] = row[16 * tb + m];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][(kk + 4 * i) * 16 + m] = acc[i];
    __syncthreads();
    const int e = threadIdx.x, row = 16 * ta + (e >> 4), col = 16 * tb + (e & 15);
    const double h = (((part[0][e] + part[1][e]) + part[2][e]) + part[3][e]) + (row == col ? 1.0 : 0.0);
    H[(int64_t)row * Dp + col] = h;
    if (ta != tb) H[(int64_t)col * Dp + row] = h;
}

__global__ void __launch_bounds__(256) svm_hessian_kernel(SvmParams p) {
    __shared__ double part[4][256];
    const int fold = blockIdx.y;
    if (p.ws.done[fold]) return;
    const int64_t t0 = p.tr_off[fold];
    svm_hessian_tile(p.x, p.Dp, p.tr_idx + t0, p.tr_off[fold + 1] - t0, p.ws.w + t0,
                     p.ws.H + (int64_t)fold * p.Dp * p.Dp, blockIdx.x, part);
}

// the unit operator: one matrix, rows idx[0..n) (or 0..n when idx is null) with weights w
__global__ void __launch_bounds__(256) svm_hessian_unit_kernel(const double* x, int Dp, const int32_t* idx, int64_t n,
                                                               const double* w, double* H) {
    __shared__ double part[4][256];
    svm_hessian_tile(x, Dp, idx, n, w, H, blockIdx.x, part);
}

__global__ void __launch_bounds__(SVM_NT) svm_step_kernel(SvmParams p) {
    const int fold = blockIdx.x, tid = threadIdx.x, Dp = p.Dp;
    __shared__ double sv[SVM_MAXD], sy[SVM_MAXD], colj[SVM_MAXD];
    __shared__ double red[SVM_NT];
    __shared__ int bad;
    if (p.ws.done[fold]) return;
    const int64_t t0 = p.tr_off[fold], n = p.tr_off[fold + 1] - t0;
    const int32_t* idx = p.tr_idx + t0;
    double* H = p.ws.H + (int64_t)fold * Dp * Dp;
    double* v = p.v + (int64_t)fold * Dp;
    const double* g = p.ws.g + (int64_t)fold * Dp;
    if (tid == 0) bad = 0;
    if (tid < Dp) {
        sv[tid] = v[tid];
        sy[tid] = -g[tid];
    }
    __syncthreads();
    // right-looking Cholesky of the lower triangle, in place: H = L L^T
    const int tx = tid & 63, ty = tid >> 6;
    for (int j = 0; j < Dp; ++j) {
        const double piv = H[(int64_t)j * Dp + j];
        if (!(piv > 0.0)) {  // uniform: every thread reads the same element
            if (tid == 0) bad = 1;
            break;
        }
        const double ljj = sqrt(piv);
        __syncthreads();  // every thread has read the pivot
        if (tid == 0) H[(int64_t)j * Dp + j] = ljj;
        for (int i = j + 1 + tid; i < Dp; i += SVM_NT) {
            const double l = H[(int64_t)i * Dp + j] / ljj;
            H[(int64_t)i * Dp + j] = l;
            colj[i] = l;
        }
        __syncthreads();
        for (int i = j + 1 + ty; i < Dp; i += SVM_NT / 64) {
            const double li = colj[i];
            for (int k = j + 1 + tx; k <= i; k += 64) H[(int64_t)i * Dp + k] -= li * colj[k];
        }
        __syncthreads();
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) {
            p.status[fold] = 3;
            p.ws.done[fold] = 1;
        }
        return;
    }
    // L y = -g (column sweep), then L^T p = y (row sweep); p ends in sy
    for (int j = 0; j < Dp; ++j) {
        const double yj = sy[j] / H[(int64_t)j * Dp + j];
        __syncthreads();
        if (tid == 0) sy[j] = yj;
        for (int i = j + 1 + tid; i < Dp; i += SVM_NT) sy[i] -= H[(int64_t)i * Dp + j] * yj;
        __syncthreads();
    }
    for (int j = Dp - 1; j >= 0; --j) {
        const double pj = sy[j] / H[(int64_t)j * Dp + j];
        __syncthreads();
        if (tid == 0) sy[j] = pj;
        for (int i = tid; i < j; i += SVM_NT) sy[i] -= H[(int64_t)j * Dp + i] * pj;
        __syncthreads();
    }
    // line search along p: f(v + t p) <= f(v) + 1e-4 t g.p (+ a few ulps of f: near the optimum the
    // decrease is below the rounding of the sum)
    double* q = p.ws.q + t0;
    const double* d = p.ws.d + t0;
    svm_rows_dot(p.x, Dp, idx, n, sy, q);
    const double gp = block_sum<SVM_NT>(tid < Dp ? g[tid] * sy[tid] : 0.0, red);  // also orders the q stores
    const double f0 = p.ws.f[fold];
    const double slack = 16.0 * 2.220446049250313e-16 * fabs(f0);
    double t = 1.0;
    bool ok = false;
    for (int it = 0; it < SVM_LS_MAX && !ok; ++it) {
        double part = 0.0;
        if (tid < Dp) {
            const double vk = sv[tid] + t * sy[tid];
            part = 0.5 * vk * vk;
        }
        for (int64_t r = tid; r < n; r += SVM_NT) {
            const bool pos = p.y[idx[r]] != 0;
            const double s = pos ? 1.0 : -1.0, C = pos ? p.pos_weight : 1.0;
            const double h = 1.0 - s * (d[r] + t * q[r]);
            part += h > 0.0 ? C * h * h : 0.0;
        }
        const double fn = block_sum<SVM_NT>(part, red);
        ok = fn <= f0 + 1e-4 * t * gp + slack;
        if (!ok) t *= 0.5;
    }
    if (!ok) {
        if (tid == 0) {
            p.status[fold] = 2;
            p.ws.done[fold] = 1;
        }
        return;
    }
    if (tid < Dp) v[tid] = sv[tid] + t * sy[tid];
    if (tid == 0) p.iters[fold] += 1;
}

// out[f][i] = x[i] . v[f] for every row
__global__ void __launch_bounds__(SVM_NT) svm_decision_kernel(const double* x, int64_t N, int Dp, const double* v,
                                                              double* out) {
    __shared__ double sv[SVM_MAXD];
    const int fold = blockIdx.y;
    if ((int)threadIdx.x < Dp) sv[threadIdx.x] = v[(int64_t)fold * Dp + threadIdx.x];
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * SVM_NT;  // SVM_NT / 16 rows per pass, 16 passes per workgroup
    const int64_t n = N - r0 < SVM_NT ? N - r0 : SVM_NT;
    svm_rows_dot(x + r0 * Dp, Dp, nullptr, n, sv, out + (int64_t)fold * N + r0);
}

static bool svm_dims_ok(int64_t Dp) { return Dp >= 16 && Dp <= SVM_MAXD && Dp % 16 == 0; }

extern "C" int64_t edgedet_svm_workspace_size(int32_t folds, int64_t Dp, int64_t total_rows) {
    if (folds < 1 || !svm_dims_ok(Dp) || total_rows < 0) return -1;
    return (int64_t)(svm_ws_doubles(folds, Dp, total_rows) * sizeof(double));
}

extern "C" int edgedet_svm_hessian(const double* x, int64_t Dp, const int32_t* idx, int64_t n, const double* w,
                                   double* H, void* stream) {
    EDGEDET_REQUIRE(x && w && H, "svm_hessian: null pointer");
    EDGEDET_REQUIRE(svm_dims_ok(Dp) && n >= 0, "svm_hessian: width a multiple of 16, <= 256");
    const int nt = (int)Dp / 16;
    hipLaunchKernelGGL(svm_hessian_unit_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, (hipStream_t)stream,
                       x, (int)Dp, idx, n, w, H);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_svm_fit(const double* x, int64_t N, int64_t Dp, const int32_t* y, double pos_weight,
                               const int32_t* tr_idx, const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds,
                               double* v, void* ws, int64_t ws_bytes, int32_t max_iter, double tol, int32_t* iters,
                               double* gnorm, int32_t* status, void* stream) {
    EDGEDET_REQUIRE(x && y && tr_idx && tr_off_host && tr_off && v && ws && iters && gnorm && status,
                    "svm_fit: null pointer");
    EDGEDET_REQUIRE(svm_dims_ok(Dp) && N >= 1 && folds >= 1 && folds <= 65535 && max_iter >= 1,
                    "svm_fit: width a multiple of 16, <= 256");
    const int64_t T = tr_off_host[folds];
    EDGEDET_REQUIRE(T >= 0 && ws_bytes >= (int64_t)(svm_ws_doubles(folds, Dp, T) * sizeof(double)),
                    "svm_fit: workspace smaller than edgedet_svm_workspace_size");
    hipStream_t st = (hipStream_t)stream;
    SvmParams p{};
    p.x = x;
    p.y = y;
    p.tr_idx = tr_idx;
    p.tr_off = tr_off;
    p.v = v;
    p.ws = svm_carve(ws, folds, Dp, T);
    p.iters = iters;
    p.gnorm = gnorm;
    p.status = status;
    p.pos_weight = pos_weight;
    p.tol = tol;
    p.Dp = (int)Dp;
    EDGEDET_CHECK_HIP(hipMemsetAsync(p.ws.done, 0, folds * sizeof(int32_t), st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(iters, 0, folds * sizeof(int32_t), st));
    EDGEDET_CHECK_HIP(hipMemsetAsync(status, 0, folds * sizeof(int32_t), st));
    const int nt = (int)Dp / 16;
    std::vector<int32_t> done_host((size_t)folds, 0);
    int32_t* done = done_host.data();
    bool all = false;
    for (int it = 0; it <= max_iter && !all; ++it) {
        hipLaunchKernelGGL(svm_eval_kernel, dim3((unsigned)folds), dim3(SVM_NT), 0, st, p);
        EDGEDET_LAUNCH_CHECK();
        EDGEDET_CHECK_HIP(hipMemcpyAsync(done, p.ws.done, folds * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        EDGEDET_CHECK_HIP(hipStreamSynchronize(st));
        all = true;
        for (int f = 0; f < folds; ++f) all = all && done[f] != 0;
        if (all || it == max_iter) break;
        hipLaunchKernelGGL(svm_hessian_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)folds), dim3(256), 0, st, p);
        EDGEDET_LAUNCH_CHECK();
        hipLaunchKernelGGL(svm_step_kernel, dim3((unsigned)folds), dim3(SVM_NT), 0, st, p);
        EDGEDET_LAUNCH_CHECK();
    }
    if (!all) {  // folds still above tol after max_iter steps: status 1
        std::vector<int32_t> s_host((size_t)folds, 0);
        int32_t* s = s_host.data();
        EDGEDET_CHECK_HIP(hipMemcpyAsync(s, status, folds * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        EDGEDET_CHECK_HIP(hipStreamSynchronize(st));
        for (int f = 0; f < folds; ++f)
            if (!done[f] && s[f] == 0) s[f] = 1;
        EDGEDET_CHECK_HIP(hipMemcpyAsync(status, s, folds * sizeof(int32_t), hipMemcpyHostToDevice, st));
        EDGEDET_CHECK_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int edgedet_svm_decision(const double* x, int64_t N, int64_t Dp, const double* v, int32_t folds,
                                    double* out, void* stream) {
    EDGEDET_REQUIRE(x && v && out, "svm_decision: null pointer");
    EDGEDET_REQUIRE(svm_dims_ok(Dp) && N >= 1 && folds >= 1 && folds <= 65535, "svm_decision: width a multiple of 16, <= 256");
    hipLaunchKernelGGL(svm_decision_kernel, dim3((unsigned)cdiv(N, SVM_NT), (unsigned)folds), dim3(SVM_NT), 0,
                       (hipStream_t)stream, x, N, (int)Dp, v, out);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

}  // namespace edgedet
