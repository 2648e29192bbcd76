// The offloading cascade's on-device decision chain (edgeml_amd/offload.py): from a weak detector
// plan's raw outputs to the bytes of the images that go on to the strong detector, without a host
// round trip.
//
//   offload_rows_kernel     detect.py:79-105 (fmt.format_batch) per image: the kept rows
//                           [cls, xc, yc, w, h, conf] as float64, compacted to the front in score order;
//   offload_feature_kernel  lib/data.py:127-160 (output_feature_kernel of csrc/orie.hip) on those padded
//                           rows: the stage-24 features [num_class + 5 k];
//   edgedet_offload_decide  the estimate of every image by the existing predict kernels
//                           (edgedet_reg_predict, or edgedet_mlp_predict on the float32 cast of the
//                           features), then flag = estimate > threshold (test.py:37);
//   edgedet_offload_flag    that flag alone, for estimates another call wrote (csrc/kpredict.hip's SVR and
//                           KNR predictions): the same kernel;
//   offload_dcsb_kernel     the DCSB baseline's rule (baseline.py:129-141) on the padded rows: counts above the
//                           model's confidence threshold and above 0.5, the minimum area, est = 0.0 / 1.0;
//   offload_svm_kernel      the Adaptive Feeding baseline's decision value on the stage-24 features, in the
//                           summation order of csrc/baseline.hip's svm_rows_dot, flag = value > 0;
//   offload_pack_kernel     the flagged images of a uint8 batch copied to the front of a destination
//                           batch in index order (flags read on the device), with their count and
//                           source indices;
//   offload_gather_kernel   up to OFFLOAD_MAXB images given as (source, index) pairs copied into one
//                           contiguous batch (the strong detector's input).
//
// Every float op of the formatter is individually rounded (the _rn intrinsics, and the build's
// -ffp-contract=off), so its rows are numpy's bytes.  The caller owns every buffer.
#include "fold_math.hpp"
#include "kernels.hpp"

namespace edgedet {

constexpr int OFFLOAD_NT = 256;
constexpr int OFFLOAD_MAXB = 64;     // images of one gather (the pair table is a kernel argument)
constexpr int OFFLOAD_CHUNKS = 64;   // workgroups per image of the copy kernels, at most
constexpr int COCO_IDS = 91;

// COCO-91 category id -> YOLOv5-80 class (edgeml_amd/labelmap.py: the 11 ids that are no COCO-2017
// detection category are dropped, the others numbered in increasing order).
// The dropped ids as bit sets: 0, 12, 26, 29, 30, 45 | 66, 68, 69, 71, 83 (bits id - 64).  An id
// outside 0..90 (numpy's table lookup would refuse it) is dropped.
__device__ __forceinline__ int64_t coco_to_yolo(int64_t id) {
    constexpr unsigned long long LO = (1ull << 0) | (1ull << 12) | (1ull << 26) | (1ull << 29) | (1ull << 30) |
                                      (1ull << 45);
    constexpr unsigned long long HI = (1ull << 2) | (1ull << 4) | (1ull << 5) | (1ull << 7) | (1ull << 19);
    if (id < 0 || id >= COCO_IDS) return -1;
    const int c = (int)id;
    const unsigned long long set = c < 64 ? LO : HI;
    const int bit = c & 63;
    if ((set >> bit) & 1ull) return -1;
    return c - (c < 64 ? 0 : __popcll(LO)) - __popcll(set & ((1ull << bit) - 1ull));
}

// One wave per image: 64 detections at a time, a ballot of the kept ones, each written at the count of
// kept detections before it.
__global__ void __launch_bounds__(64) offload_rows_kernel(const int32_t* __restrict__ count,
                                                          const float* __restrict__ boxes,
                                                          const float* __restrict__ scores,
                                                          const int64_t* __restrict__ labels, int K, float fh, float fw,
                                                          int voc, double* __restrict__ rows,
                                                          int32_t* __restrict__ nrow) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = count[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const int64_t at = (int64_t)b * K + k;
        int64_t cls = -1;
        if (k < n) cls = voc ? labels[at] - 1 : coco_to_yolo(labels[at]);  // detect.py:89-95
        const bool keep = cls != -1;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const float x1 = boxes[at * 4], y1 = boxes[at * 4 + 1], x2 = boxes[at * 4 + 2], y2 = boxes[at * 4 + 3];
            const float w = __fsub_rn(x2, x1), h = __fsub_rn(y2, y1);
            const float xc = __fadd_rn(x1, __fdiv_rn(w, 2.f)), yc = __fadd_rn(y1, __fdiv_rn(h, 2.f));
            double* r = rows + ((int64_t)b * K + base + __popcll(m & ((1ull << lane) - 1ull))) * 6;
            r[0] = (double)cls;
            r[1] = (double)__fdiv_rn(xc, fw);
            r[2] = (double)__fdiv_rn(yc, fh);
            r[3] = (double)__fdiv_rn(w, fw);
            r[4] = (double)__fdiv_rn(h, fh);
            r[5] = (double)scores[at];
        }
        base += __popcll(m);
    }
    if (lane == 0) nrow[b] = base;
}

// One workgroup per image, one thread per feature: the class counts of the first min(nrow, k) rows
// (int(row[0]) truncates, as output_feature_kernel does), then those rows' five other columns; zeros
// beyond them.  A count is a sum of ones, exact in any order.
__global__ void __launch_bounds__(OFFLOAD_NT) offload_feature_kernel(const double* __restrict__ rows,
                                                                     const int32_t* __restrict__ nrow, int K,
                                                                     int num_class, int k,
                                                                     double* __restrict__ out) {
    const int b = blockIdx.x;
    const int width = num_class + 5 * k;
    int nr = nrow[b];
    nr = nr < 0 ? 0 : (nr > K ? K : nr);
    nr = nr < k ? nr : k;
    const double* R = rows + (int64_t)b * K * 6;
    for (int j = threadIdx.x; j < width; j += OFFLOAD_NT) {
        double v = 0.0;
        if (j < num_class) {
            for (int r = 0; r < nr; ++r) v += (int)R[r * 6] == j ? 1.0 : 0.0;
        } else {
            const int r = (j - num_class) / 5, q = (j - num_class) % 5;
            if (r < nr) v = R[r * 6 + 1 + q];
        }
        out[(int64_t)b * width + j] = v;
    }
}

__global__ void offload_cast_kernel(const double* __restrict__ x, int64_t n, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];  // round to nearest even: numpy's astype(float32)
}

// est32 given: the MLP's float32 estimates, promoted into est; otherwise est holds the estimates.
__global__ void offload_flag_kernel(const float* __restrict__ est32, double* __restrict__ est, int64_t B,
                                    double threshold, uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const double e = est32 ? (double)est32[i] : est[i];
    if (est32) est[i] = e;
    flag[i] = e > threshold ? 1 : 0;
}

// The smaller of two float64 values, a NaN winning from either side (np.amin): whatever the order of the
// reduction, the result is the same value.
__device__ __forceinline__ double min_nan(double a, double b) { return (a < b || a != a) ? a : b; }

// DCSB's decision (baseline.py:129-141) for one fitted model.  One wave per image, 64 of its rows per pass:
// the two counts from ballots, the minimum area of the rows above conf_thresh per lane and then across the
// wave.  xywh2xyxy and get_area in the reference's operation order, each op rounded on its own.
__global__ void __launch_bounds__(64) offload_dcsb_kernel(const double* __restrict__ rows,
                                                          const int32_t* __restrict__ nrow, int K, double conf_thresh,
                                                          int num_thresh, double area_thresh,
                                                          int32_t* __restrict__ est_num, int32_t* __restrict__ det_num,
                                                          double* __restrict__ min_area, double* __restrict__ est,
                                                          uint8_t* __restrict__ flag) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = nrow[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    const double* R = rows + (int64_t)b * K * 6;
    int ne = 0, nd = 0;
    double amin = __builtin_inf();  // of this lane's rows above conf_thresh
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        bool over = false, det = false;
        if (k < n) {
            const double* r = R + (int64_t)k * 6;
            const double conf = r[5];
            over = conf > conf_thresh;
            det = conf > 0.5;
            if (over) {
                const double x1 = r[1] - r[3] / 2, y1 = r[2] - r[4] / 2;
                const double x2 = r[1] + r[3] / 2, y2 = r[2] + r[4] / 2;
                amin = min_nan((x2 - x1) * (y2 - y1), amin);
            }
        }
        ne += __popcll(__ballot(over));
        nd += __popcll(__ballot(det));
    }
    for (int s = 32; s > 0; s >>= 1) amin = min_nan(amin, __shfl_xor(amin, s, 64));
    if (lane != 0) return;
    if (ne == 0) amin = 0.0;  // filter_box: 0 for an image without a row above the threshold
    const bool cls = ne != nd && (ne > num_thresh || amin < area_thresh);
    if (est_num) est_num[b] = ne;
    if (det_num) det_num[b] = nd;
    if (min_area) min_area[b] = amin;
    est[b] = cls ? 1.0 : 0.0;
    flag[b] = cls ? 1 : 0;
}

// Adaptive Feeding's decision on unpadded features: svm_rows_dot (csrc/baseline.hip) on the row
// (feat[b], 1, 0, ...) of baseline.pad_features without that row in memory.  Sixteen lanes per image, lane
// `sub` adds its terms k = sub, sub + 16, ... < Dp in increasing k from 0.0, then lane16_sum: the same
// operations on the same values in the same order, so the sum is svm_decision_kernel's bit for bit.
__global__ void __launch_bounds__(OFFLOAD_NT) offload_svm_kernel(const double* __restrict__ feat, int B, int D,
                                                                 const double* __restrict__ v, int Dp,
                                                                 double* __restrict__ est,
                                                                 uint8_t* __restrict__ flag) {
    __shared__ double sv[FOLD_MAXD];
    if ((int)threadIdx.x < Dp) sv[threadIdx.x] = v[threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int64_t b = (int64_t)blockIdx.x * (OFFLOAD_NT / 16) + (threadIdx.x >> 4);
    const bool ok = b < B;
    const double* row = feat + (ok ? b : 0) * D;
    double acc = 0.0;
    if (ok)
        for (int k = sub; k < Dp; k += 16) acc += (k < D ? row[k] : (k == D ? 1.0 : 0.0)) * sv[k];
    acc = lane16_sum(acc);
    if (ok && sub == 0) {
        est[b] = acc;
        flag[b] = acc > 0.0 ? 1 : 0;  // fit_af_folds' (dec > 0)
    }
}

// n bytes by the calling workgroup's share of `parts` workgroups: 16-byte copies when both ends are
// 16-byte aligned, the bytes past the last whole 16 (or all of them) one by one.
__device__ __forceinline__ void copy_image(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t n,
                                           int part, int parts) {
    const int64_t tid = (int64_t)part * blockDim.x + threadIdx.x, step = (int64_t)parts * blockDim.x;
    const bool vec = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
    const int64_t nv = vec ? n / 16 : 0;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int64_t i = tid; i < nv; i += step) d4[i] = s4[i];
    for (int64_t i = nv * 16 + tid; i < n; i += step) dst[i] = src[i];
}

__global__ void __launch_bounds__(OFFLOAD_NT) offload_pack_kernel(const uint8_t* __restrict__ flag,
                                                                  const uint8_t* __restrict__ src, int B, int64_t n,
                                                                  uint8_t* __restrict__ dst,
                                                                  int32_t* __restrict__ count,
                                                                  int32_t* __restrict__ index) {
    const int b = blockIdx.y;
    int slot = 0;
    for (int j = 0; j < b; ++j) slot += flag[j] ? 1 : 0;  // uniform: the images kept before this one
    if (blockIdx.x == 0 && threadIdx.x == 0 && b == B - 1) *count = slot + (flag[b] ? 1 : 0);
    if (!flag[b]) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) index[slot] = b;
    copy_image(dst + (int64_t)slot * n, src + (int64_t)b * n, n, blockIdx.x, gridDim.x);
}

struct GatherTable {
    const uint8_t* src[OFFLOAD_MAXB];
    int32_t index[OFFLOAD_MAXB];
};

__global__ void __launch_bounds__(OFFLOAD_NT) offload_gather_kernel(GatherTable t, int64_t n,
                                                                    uint8_t* __restrict__ dst) {
    const int b = blockIdx.y;
    copy_image(dst + (int64_t)b * n, t.src[b] + (int64_t)t.index[b] * n, n, blockIdx.x, gridDim.x);
}

static unsigned copy_chunks(int64_t n) {
    const int64_t c = cdiv(n, (int64_t)OFFLOAD_NT * 16 * 4);  // four 16-byte copies per thread
    return (unsigned)(c < 1 ? 1 : (c > OFFLOAD_CHUNKS ? OFFLOAD_CHUNKS : c));
}

}  // namespace edgedet

using namespace edgedet;

extern "C" int edgedet_offload_rows(const int32_t* count, const float* boxes, const float* scores,
                                    const int64_t* labels, int64_t B, int64_t K, int32_t H, int32_t W, int32_t voc,
                                    double* rows, int32_t* nrow, void* stream) {
    EDGEDET_REQUIRE(count && boxes && scores && labels && rows && nrow, "offload_rows: null pointer");
    EDGEDET_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K < (1 << 24) && H >= 1 && W >= 1, "offload_rows: bad sizes");
    if (B == 0) return 0;
    hipLaunchKernelGGL(offload_rows_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, count, boxes, scores,
                       labels, (int)K, (float)H, (float)W, voc, rows, nrow);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_features(const double* rows, const int32_t* nrow, int64_t B, int64_t K,
                                        int32_t num_class, int32_t k, double* out, void* stream) {
    EDGEDET_REQUIRE(rows && nrow && out, "offload_features: null pointer");
    EDGEDET_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K < (1 << 24) && num_class > 0 && k >= 0 && k < (1 << 20),
                    "offload_features: bad sizes");
    if (B == 0) return 0;
    hipLaunchKernelGGL(offload_feature_kernel, dim3((unsigned)B), dim3(OFFLOAD_NT), 0, (hipStream_t)stream, rows, nrow,
                       (int)K, num_class, k, out);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_decide(const double* feat, int64_t B, int64_t D, const double* mean,
                                      const double* scale, const double* coef, const double* intercept, int32_t L,
                                      const int32_t* dims, const float* state, float* x32, float* est32,
                                      double threshold, double* est, uint8_t* flag, void* stream) {
    EDGEDET_REQUIRE(feat && est && flag && B >= 1 && D >= 1, "offload_decide: bad args");
    if (L == 0) {
        if (int rc = edgedet_reg_predict(feat, B, D, mean, scale, coef, intercept, 1, est, stream)) return rc;
    } else {
        EDGEDET_REQUIRE(x32 && est32, "offload_decide: the MLP needs its float32 scratch");
        hipLaunchKernelGGL(offload_cast_kernel, dim3((unsigned)cdiv(B * D, OFFLOAD_NT)), dim3(OFFLOAD_NT), 0,
                           (hipStream_t)stream, feat, B * D, x32);
        EDGEDET_LAUNCH_CHECK();
        if (int rc = edgedet_mlp_predict(x32, D, nullptr, B, L, dims, state, est32, stream)) return rc;
    }
    hipLaunchKernelGGL(offload_flag_kernel, dim3((unsigned)cdiv(B, OFFLOAD_NT)), dim3(OFFLOAD_NT), 0,
                       (hipStream_t)stream, L == 0 ? nullptr : est32, est, B, threshold, flag);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_flag(const double* est, int64_t B, double threshold, uint8_t* flag, void* stream) {
    EDGEDET_REQUIRE(est && flag, "offload_flag: null pointer");
    EDGEDET_REQUIRE(B >= 1 && B <= (int64_t)65535 * OFFLOAD_NT, "offload_flag: bad sizes");
    // est32 null: the kernel only reads est
    hipLaunchKernelGGL(offload_flag_kernel, dim3((unsigned)cdiv(B, OFFLOAD_NT)), dim3(OFFLOAD_NT), 0,
                       (hipStream_t)stream, (const float*)nullptr, const_cast<double*>(est), B, threshold, flag);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_dcsb(const double* rows, const int32_t* nrow, int64_t B, int64_t K, double conf_thresh,
                                    int32_t num_thresh, double area_thresh, int32_t* est_num, int32_t* det_num,
                                    double* min_area, double* est, uint8_t* flag, void* stream) {
    EDGEDET_REQUIRE(rows && nrow && est && flag, "offload_dcsb: null pointer");
    EDGEDET_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K < (1 << 24), "offload_dcsb: bad sizes");
    if (B == 0) return 0;
    hipLaunchKernelGGL(offload_dcsb_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, rows, nrow, (int)K,
                       conf_thresh, num_thresh, area_thresh, est_num, det_num, min_area, est, flag);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_svm(const double* feat, int64_t B, int64_t D, const double* v, int64_t Dp, double* est,
                                   uint8_t* flag, void* stream) {
    EDGEDET_REQUIRE(feat && v && est && flag, "offload_svm: null pointer");
    EDGEDET_REQUIRE(B >= 0 && B <= 65535 && fold_dims_ok(D) && Dp <= FOLD_MAXD && Dp == (D + 1 + 15) / 16 * 16,
                    "offload_svm: Dp = D + 1 padded to a multiple of 16, <= 256");
    if (B == 0) return 0;
    hipLaunchKernelGGL(offload_svm_kernel, dim3((unsigned)cdiv(B, (int64_t)(OFFLOAD_NT / 16))), dim3(OFFLOAD_NT), 0,
                       (hipStream_t)stream, feat, (int)B, (int)D, v, (int)Dp, est, flag);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_pack(const uint8_t* flag, const uint8_t* src, int64_t B, int64_t image_bytes,
                                    uint8_t* dst, int32_t* count, int32_t* index, void* stream) {
    EDGEDET_REQUIRE(flag && src && dst && count && index, "offload_pack: null pointer");
    EDGEDET_REQUIRE(B >= 1 && B <= 65535 && image_bytes >= 1, "offload_pack: bad sizes");
    hipLaunchKernelGGL(offload_pack_kernel, dim3(copy_chunks(image_bytes), (unsigned)B), dim3(OFFLOAD_NT), 0,
                       (hipStream_t)stream, flag, src, (int)B, image_bytes, dst, count, index);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_offload_gather(const void* const* src, const int32_t* index, int32_t n_images,
                                      int64_t image_bytes, uint8_t* dst, void* stream) {
    EDGEDET_REQUIRE(src && index && dst, "offload_gather: null pointer");
    EDGEDET_REQUIRE(n_images >= 1 && n_images <= OFFLOAD_MAXB && image_bytes >= 1, "offload_gather: 1..64 images");
    GatherTable t{};
    for (int j = 0; j < n_images; ++j) {
        EDGEDET_REQUIRE(src[j] && index[j] >= 0, "offload_gather: bad (source, index) pair");
        t.src[j] = static_cast<const uint8_t*>(src[j]);
        t.index[j] = index[j];
    }
    hipLaunchKernelGGL(offload_gather_kernel, dim3(copy_chunks(image_bytes), (unsigned)n_images), dim3(OFFLOAD_NT), 0,
                       (hipStream_t)stream, t, image_bytes, dst);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
