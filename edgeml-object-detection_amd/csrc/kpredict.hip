// Prediction from the stored rows of a saved SVR (rbf) or KNeighborsRegressor model (edgeml_amd/kpredict.py):
// what the offloading cascade needs to be driven by a wts<k>.pickle of either kind.  Float64 throughout,
// fixed-order sums, no float atomics.  An estimate is a function of (feature row, model) only: it does not
// depend on the batch the row arrives in or on its place in that batch.
//
//   kp_prepare_kernel   once per loaded model: Z = zscore(x, mean, 1 / scale) of the stored rows and |z|^2 of
//                       each: sixteen lanes per row, k = sub, sub + 16, ..., then lane16_sum (fold_math.hpp),
//                       as svr_std_kernel and knn_norm_kernel take them.
//   kp_tile_kernel      a workgroup per (64 stored rows x 16 queries), a wave per 16 x 16 tile.  The sixteen
//                       queries are standardised into LDS by zscore and their norms taken in that same
//                       sixteen-lane order; the dot products come from v_mfma_f64_16x16x4_f64 with k ascending
//                       in steps of four, operands past D, n or B zero; d = sqdist(nq, nb, acc).  The fits
//                       (knn_dist_kernel, svr_kmat_kernel) call the same three functions on the same k order,
//                       so a pair's distance is the fit's bit for bit wherever the pair sits in a tile.
//                         KNR: d goes to the workspace [B][n].
//                         SVR: beta_j exp(-gamma d), the tile's sixteen stored columns added by a butterfly
//                              into one partial per (query, tile) in the workspace [B][tiles].
//   kp_svr_sum_kernel   a wave per query: lane l adds the partials of tiles l, l + 64, ... in order, a butterfly
//                       of 32 .. 1 adds the lanes, then the intercept.  The order depends on n alone.
//   kp_select_kernel    knn_select_kernel's rule (csrc/regress.hip) per query: the k-th smallest key found on
//                       the bit patterns, every key below it selected, the lowest positions among the keys equal
//                       to it until k are taken, positions written ascending, the targets added one by one in
//                       position order and divided by k.  Only the integer counts are reduced differently
//                       (a wave sum, then the four waves).
#include <cstdint>

#include "fold_math.hpp"
#include "kernels.hpp"

namespace edgedet {

constexpr int KP_STD_NT = 1024;
constexpr int KP_NT = 256;
constexpr int KP_LD = FOLD_MAXD + 2;  // LDS row stride of the query tile: a half wave's 8-byte reads hit 32 bank pairs
constexpr int KP_SEL_NT = 256;
constexpr int KP_SEL_KEYS = 16;  // keys a selection thread holds in registers: up to 4,096 stored rows
constexpr int KIND_SVR = 0, KIND_KNR = 1;

__host__ __device__ static inline int64_t kp_tiles(int64_t n) { return (n + 15) / 16; }

// ------------------------------------------------------------------------------------ standardise
__global__ void __launch_bounds__(KP_STD_NT) kp_prepare_kernel(const double* __restrict__ x, int64_t n, int D,
                                                               const double* __restrict__ mean,
                                                               const double* __restrict__ scale, double* z,
                                                               double* nrm) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    const int tid = threadIdx.x;
    stage_scaler(sm, si, mean, scale, 0, D);
    __syncthreads();
    const int sub = tid & 15;
    const int64_t r = (int64_t)blockIdx.x * 64 + (tid >> 4);
    const bool ok = r < n;
    double acc = 0.0;
    if (ok) {
        const double* src = x + r * D;
        double* dst = z + r * D;
        for (int k = sub; k < D; k += 16) {
            const double v = zscore(src[k], sm[k], si[k]);
            dst[k] = v;
            acc += v * v;
        }
    }
    acc = lane16_sum(acc);
    if (ok && sub == 0) nrm[r] = acc;
}

// ------------------------------------------------------------------------------------------ tiles
// Lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15] of a k-step of four; element i of the result is
// D[(l >> 4) + 4 i][l & 15].  out: KNR dist [B][n]; SVR partial [B][tiles].
template <int KIND>
__global__ void __launch_bounds__(KP_NT) kp_tile_kernel(const double* __restrict__ feat, int64_t B, int D,
                                                        const double* __restrict__ mean,
                                                        const double* __restrict__ scale,
                                                        const double* __restrict__ z,
                                                        const double* __restrict__ nrm,
                                                        const double* __restrict__ beta, int64_t n, double gamma,
                                                        double* __restrict__ out) {
    __shared__ double sm[FOLD_MAXD], si[FOLD_MAXD];
    __shared__ double zq[16 * KP_LD];
    __shared__ double qn[16];
    const int tid = threadIdx.x;
    stage_scaler_padded<KP_NT>(sm, si, mean, scale, 0, D);
    __syncthreads();
    const int64_t q0 = (int64_t)blockIdx.y * 16;
    for (int e = tid; e < 16 * FOLD_MAXD; e += KP_NT) {
        const int r = e >> 8, k = e & (FOLD_MAXD - 1);
        const int64_t q = q0 + r;
        zq[r * KP_LD + k] = q < B && k < D ? zscore(feat[q * D + k], sm[k], si[k]) : 0.0;
    }
    __syncthreads();
    {
        const int sub = tid & 15, r = tid >> 4;  // 256 threads: sixteen lanes for each of the sixteen queries
        double acc = 0.0;
        for (int k = sub; k < D; k += 16) {
            const double v = zq[r * KP_LD + k];
            acc += v * v;
        }
        acc = lane16_sum(acc);
        if (sub == 0) qn[r] = acc;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave, b0 = tile * 16;
    if (b0 >= n) return;  // uniform per wave, after the last barrier
    const int64_t bb = b0 + m;
    const bool okb = bb < n;
    const double* rowa = zq + m * KP_LD;
    const double* rowb = z + (okb ? bb : 0) * D;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + kk;
        const double a = rowa[k];  // zero past D and past B
        const double b = okb && k < D ? rowb[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const double nb = okb ? nrm[bb] : 0.0;
    if (KIND == KIND_KNR) {
        if (!okb) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t q = q0 + kk + 4 * i;
            if (q < B) out[q * n + bb] = sqdist(qn[kk + 4 * i], nb, acc[i]);
        }
    } else {
        const double wb = okb ? beta[bb] : 0.0;
        const int64_t tiles = kp_tiles(n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t q = q0 + kk + 4 * i;
            const double d = sqdist(qn[kk + 4 * i], nb, acc[i]);
            const double s = lane16_sum(okb ? wb * exp(-gamma * d) : 0.0);
            if (m == 0 && q < B) out[q * tiles + tile] = s;
        }
    }
}

__global__ void __launch_bounds__(64) kp_svr_sum_kernel(const double* __restrict__ part, int64_t tiles,
                                                        double intercept, double* __restrict__ est) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int64_t t = lane; t < tiles; t += 64) acc += part[q * tiles + t];
    acc += __shfl_xor(acc, 32);
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    if (lane == 0) est[q] = acc + intercept;
}

// ----------------------------------------------------------------------------------------- select
// An integer sum over the workgroup: exact in any order.
__device__ __forceinline__ int kp_block_count(int v, int* red) {
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    __syncthreads();  // the previous call's reads of red are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// One workgroup per query.  The k-th smallest key T is built bit by bit (keys are non-negative doubles, so
// their bit patterns order as unsigned integers): the largest T with count(key < T) <= k - 1.  Selected: every
// key < T and the first k - count(key < T) positions with key == T; written in position order, and the
// estimate is the mean of their targets summed in that order.  sel: [B][k], the caller's nbr or scratch.
__global__ void __launch_bounds__(KP_SEL_NT) kp_select_kernel(const double* __restrict__ dist, int n,
                                                              const double* __restrict__ y, int k, double* est,
                                                              int32_t* sel) {
    __shared__ int red[KP_SEL_NT / 64];
    __shared__ int base_lt[KP_SEL_NT], base_eq[KP_SEL_NT];
    __shared__ int total_lt;
    __shared__ double sy[KP_SEL_NT];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const unsigned long long* key = (const unsigned long long*)(dist + q * n);
    // up to KP_SEL_KEYS keys per thread stay in registers over the 63 passes; a key past n is all ones,
    // above every candidate
    const bool held = n <= KP_SEL_NT * KP_SEL_KEYS;  // uniform
    unsigned long long mine[KP_SEL_KEYS];
#pragma unroll
    for (int i = 0; i < KP_SEL_KEYS; ++i) {
        const int j = tid + i * KP_SEL_NT;
        mine[i] = held && j < n ? key[j] : ~0ull;
    }
    unsigned long long T = 0;
    for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long cand = T | (1ull << bit);
        int c = 0;
        if (held) {
#pragma unroll
            for (int i = 0; i < KP_SEL_KEYS; ++i) c += mine[i] < cand ? 1 : 0;
        } else {
            for (int j = tid; j < n; j += KP_SEL_NT) c += key[j] < cand ? 1 : 0;
        }
        if (kp_block_count(c, red) <= k - 1) T = cand;  // uniform
    }
    const int chunk = (n + KP_SEL_NT - 1) / KP_SEL_NT;
    const int j0 = (int64_t)tid * chunk < n ? tid * chunk : n, j1 = (int64_t)j0 + chunk < n ? j0 + chunk : n;
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
        for (int t = 0; t < KP_SEL_NT; ++t) {
            const int x0 = base_lt[t], x1 = base_eq[t];
            base_lt[t] = a;
            base_eq[t] = b;
            a += x0;
            b += x1;
        }
        total_lt = a;
    }
    __syncthreads();
    const int need = k - total_lt;  // ties taken at the k-th distance, >= 1
    int32_t* out = sel + q * k;
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
    for (int c0 = 0; c0 < k; c0 += KP_SEL_NT) {
        const int c = c0 + tid;
        if (c < k) sy[tid] = y[out[c]];
        __syncthreads();
        if (tid == 0) {
            const int cnt = k - c0 < KP_SEL_NT ? k - c0 : KP_SEL_NT;
            for (int i = 0; i < cnt; ++i) acc += sy[i];
        }
        __syncthreads();
    }
    if (tid == 0) est[q] = acc / (double)k;
}

// ------------------------------------------------------------------------------------- the C-ABI
constexpr int64_t KP_MAXN = (int64_t)1 << 30;   // stored rows (positions are int32)
constexpr int64_t KP_MAXB = 65535 * 16;         // queries of one call (the tile grid's second axis)

static int64_t kp_ws_bytes(int64_t n, int64_t B, int kind) {
    if (kind == KIND_SVR) {
        const int64_t parts = B * kp_tiles(n);
        return (parts > 0 ? parts : 1) * (int64_t)sizeof(double);
    }
    return B * n * (int64_t)sizeof(double) + (B * n * (int64_t)sizeof(int32_t) + 7) / 8 * 8;
}

}  // namespace edgedet

using namespace edgedet;

extern "C" int64_t edgedet_kmodel_workspace_size(int64_t n, int64_t D, int64_t B, int32_t kind) {
    if (!fold_dims_ok(D) || B < 1 || B > KP_MAXB || n > KP_MAXN) return -1;
    if (kind == KIND_SVR ? n < 0 : (kind != KIND_KNR || n < 1)) return -1;
    return kp_ws_bytes(n, B, kind);
}

extern "C" int edgedet_kmodel_prepare(const double* rows, int64_t n, int64_t D, const double* mean,
                                      const double* scale, double* z, double* norm, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && n >= 0 && n <= KP_MAXN, "kmodel_prepare: 1 <= features <= 255, 0 <= rows <= 2^30");
    EDGEDET_REQUIRE(mean && scale && (n == 0 || (rows && z && norm)), "kmodel_prepare: null pointer");
    if (n == 0) return 0;
    hipLaunchKernelGGL(kp_prepare_kernel, dim3((unsigned)cdiv(n, 64)), dim3(KP_STD_NT), 0, (hipStream_t)stream, rows, n,
                       (int)D, mean, scale, z, norm);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_svr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean,
                                         const double* scale, const double* z, const double* norm,
                                         const double* beta, int64_t n, double gamma, double intercept, void* ws,
                                         int64_t ws_bytes, double* est, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && B >= 1 && B <= KP_MAXB && n >= 0 && n <= KP_MAXN,
                    "svr_model_predict: 1 <= features <= 255, 1 <= rows <= 1,048,560, 0 <= support vectors <= 2^30");
    EDGEDET_REQUIRE(feat && mean && scale && ws && est && (n == 0 || (z && norm && beta)),
                    "svr_model_predict: null pointer");
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= kp_ws_bytes(n, B, KIND_SVR),
                    "svr_model_predict: workspace smaller than edgedet_kmodel_workspace_size, or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    if (n > 0) {
        hipLaunchKernelGGL(kp_tile_kernel<KIND_SVR>, dim3((unsigned)cdiv(n, 64), (unsigned)cdiv(B, 16)), dim3(KP_NT), 0,
                           st, feat, B, (int)D, mean, scale, z, norm, beta, n, gamma, part);
        EDGEDET_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(kp_svr_sum_kernel, dim3((unsigned)B), dim3(64), 0, st, part, kp_tiles(n), intercept, est);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_knn_model_predict(const double* feat, int64_t B, int64_t D, const double* mean,
                                         const double* scale, const double* z, const double* norm,
                                         const double* target, int64_t n, int32_t k, void* ws, int64_t ws_bytes,
                                         double* est, int32_t* nbr, void* stream) {
    EDGEDET_REQUIRE(fold_dims_ok(D) && B >= 1 && B <= KP_MAXB && n >= 1 && n <= KP_MAXN,
                    "knn_model_predict: 1 <= features <= 255, 1 <= rows <= 1,048,560, 1 <= training rows <= 2^30");
    EDGEDET_REQUIRE(k >= 1 && k <= n, "knn_model_predict: 1 <= n_neighbors <= training rows");
    EDGEDET_REQUIRE(feat && mean && scale && z && norm && target && ws && est, "knn_model_predict: null pointer");
    EDGEDET_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= kp_ws_bytes(n, B, KIND_KNR),
                    "knn_model_predict: workspace smaller than edgedet_kmodel_workspace_size, or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* dist = (double*)ws;
    int32_t* sel = nbr ? nbr : (int32_t*)(dist + B * n);
    hipLaunchKernelGGL(kp_tile_kernel<KIND_KNR>, dim3((unsigned)cdiv(n, 64), (unsigned)cdiv(B, 16)), dim3(KP_NT), 0, st,
                       feat, B, (int)D, mean, scale, z, norm, (const double*)nullptr, n, 0.0, dist);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(kp_select_kernel, dim3((unsigned)B), dim3(KP_SEL_NT), 0, st, (const double*)dist, (int)n, target,
                       (int)k, est, sel);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
