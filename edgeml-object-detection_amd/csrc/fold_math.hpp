// The float64 steps that the estimator kernels share (svr.hip, regress.hip, kpredict.hip, baseline.hip,
// gbr.hip), each stated once: two kernels that call the same function here round alike by construction, which
// is what lets a saved model's prediction equal the fit's bit for bit.  Every file is built with
// -ffp-contract=off, so an expression inlined from here rounds operation by operation, as written.
#pragma once
#include "common.hpp"

namespace edgedet {

constexpr int FOLD_MAXD = 256;  // LDS width of a standardised row: at most 255 features (+ a target or bias)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// fixed-order tree over the workgroup's NT values in red[NT]; every thread gets the result
template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

template <int NT>
__device__ __forceinline__ double block_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

// row r of a fold's training set: through the index list, or the r-th row of a contiguous run
__device__ __forceinline__ int64_t fold_row(const int32_t* idx, int64_t t0, int64_t r) {
    return idx ? (int64_t)idx[t0 + r] : t0 + r;
}

// sum over each group of sixteen lanes: the butterfly of 8, 4, 2, 1; every lane of the group gets it
__device__ __forceinline__ double lane16_sum(double v) {
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// StandardScaler's transform with the reciprocal of the scale taken once: two roundings after the reciprocal's
__device__ __forceinline__ double zscore(double x, double mean, double inv_scale) { return (x - mean) * inv_scale; }

// |a - b|^2 from the two norms and the dot product, clamped at zero
__device__ __forceinline__ double sqdist(double nq, double nb, double dot) {
    const double d = (nq + nb) - 2.0 * dot;
    return d > 0.0 ? d : 0.0;
}

// mean and 1 / scale of fold's D columns (mean and scale are [F][D]) into LDS, a column per thread (the workgroup
// has at least D threads); the caller's barrier follows
__device__ __forceinline__ void stage_scaler(double* sm, double* si, const double* __restrict__ mean,
                                             const double* __restrict__ scale, int fold, int D) {
    const int tid = threadIdx.x;
    if (tid < D) {
        sm[tid] = mean[(int64_t)fold * D + tid];
        si[tid] = 1.0 / scale[(int64_t)fold * D + tid];
    }
}

// the same into sm[FOLD_MAXD], si[FOLD_MAXD] by a workgroup of NT threads, zero past D: an operand loop that
// runs to a multiple of four past D reads zeros; the caller's barrier follows
template <int NT>
__device__ __forceinline__ void stage_scaler_padded(double* sm, double* si, const double* __restrict__ mean,
                                                    const double* __restrict__ scale, int fold, int D) {
    for (int k = threadIdx.x; k < FOLD_MAXD; k += NT) {
        sm[k] = k < D ? mean[(int64_t)fold * D + k] : 0.0;
        si[k] = k < D ? 1.0 / scale[(int64_t)fold * D + k] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------ host
static inline bool fold_dims_ok(int64_t D) { return D >= 1 && D <= FOLD_MAXD - 1; }

// The host copy of the fold offsets: 1..65535 folds from offset 0, every fold with 1..max_rows training rows.
// indexed: the folds pick their rows through an index list, so each holds at most N rows (N == 0: no bound);
// otherwise they are consecutive runs of the dataset, N rows in all.
static inline bool folds_ok(const int64_t* tr_off_host, int32_t folds, int64_t N, bool indexed,
                            int64_t max_rows = INT64_MAX) {
    if (!tr_off_host || folds < 1 || folds > 65535 || tr_off_host[0] != 0) return false;
    for (int f = 0; f < folds; ++f) {
        const int64_t n = tr_off_host[f + 1] - tr_off_host[f];
        if (n < 1 || n > max_rows || (indexed && N > 0 && n > N)) return false;
    }
    return indexed || tr_off_host[folds] <= N;
}

}  // namespace edgedet
