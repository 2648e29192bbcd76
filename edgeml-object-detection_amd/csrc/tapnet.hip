// The cascade's decision from a hidden-layer map: the eval-mode forward of edgeml_amd.convnet's EdgeDetectionNet
// (resize on: Conv2d 'same' + BatchNorm2d + ReLU (+ MaxPool 2x2) stacks, then Linear + BatchNorm1d + ReLU stacks,
// then Linear -> 1) as ONE launch, one workgroup per image.  The layered eval forward
// (convnet.Trainer.forward(train=False)) is about 21 tiny launches per batch on the weak chain's tail.
//
// The activations ping-pong between two LDS regions (kernels.hpp tapnet_regions): the pooled input map
// [S][S][Cin], then every conv output, pooled map and hidden vector.  A plane of C channels has the odd pitch
// C + 1, so the 16 pixels an MFMA A operand reads in one instruction fall into different banks.
//
// A conv layer is an implicit GEMM on v_mfma_f32_16x16x4_f32: M = the image's pixels, N = Cout, K = (kh, kw, ci)
// ascending, four K values per MFMA (Cin is a multiple of 4, so an MFMA stays inside one tap).  A tap outside the
// map contributes a zero A operand.  The weights [Cout][k][k][Cin] stream from global memory (every workgroup reads
// the same ones: they stay in L2).  A wave owns one 16 x 16 output tile at a time; the sixteen waves of the workgroup
// share out the tiles, eight weight operands in flight each.  Every output is one accumulator that runs through all of K in
// order, and an f32 MFMA is an fmaf chain: the result depends neither on the batch nor on the
// workgroup that computed it.  The epilogue is cnn_act_fwd_kernel's mode 2 in float32, then ReLU; the pool is
// cnn_maxpool_fwd_kernel's window walk.  A linear output is cnn_linear_fwd_kernel's sum: lane l over k = l, l + 64,
// ..., the 64 partial sums combined by the same butterfly.  No atomics anywhere.
#include <mutex>
#include <vector>

#include "kernels.hpp"

namespace edgedet {

typedef float tap_f32x4 __attribute__((ext_vector_type(4)));

constexpr int TAP_NT = 1024;  // sixteen waves: four per SIMD hide the weight loads' latency
constexpr int TAP_MJ = 1;     // M tiles per wave unit
constexpr int TAP_U = 8;      // weight operands in flight per wave: a 128-byte line of a weight row

struct TapLayer {
    int w, b, g, be, rm, rv;  // float offsets into the state vector (ConvSpec's layout)
};

struct TapnetParams {
    const float* x;      // [B][S][S][Cin]
    const float* P;      // the net's state vector
    double* est;         // [B]
    uint8_t* flag;       // [B]
    double threshold;
    TapnetShape t;
    TapLayer conv[TAPNET_MAXL], lin[TAPNET_MAXL];
    int region1;         // float offset of the second LDS region
};

__global__ void __launch_bounds__(TAP_NT) tapnet_kernel(TapnetParams p) {
    extern __shared__ float tap_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int img = blockIdx.x;
    float* cur = tap_lds;
    float* nxt = tap_lds + p.region1;
    int H = p.t.S, W = p.t.S, C = p.t.cin;
    {
        const float* xb = p.x + (int64_t)img * H * W * C;
        for (int e = tid; e < H * W * C; e += TAP_NT) {
            const int pix = e / C;
            cur[pix * (C + 1) + (e - pix * C)] = xb[e];
        }
    }
    __syncthreads();
    for (int li = 0; li < p.t.nconv; ++li) {
        const TapLayer L = p.conv[li];
        const int Co = p.t.cout[li], k = p.t.k[li], pad = k / 2, M = H * W, K = k * k * C;
        const int pin = C + 1, pout = Co + 1;
        const int MT = (M + 15) / 16, NT = (Co + 15) / 16, MG = (MT + TAP_MJ - 1) / TAP_MJ;
        for (int u = wid; u < NT * MG; u += TAP_NT / 64) {  // wave-uniform
            const int nt = u / MG, mt0 = (u - nt * MG) * TAP_MJ;
            const int n = nt * 16 + l16;
            const bool nok = n < Co;
            const float* wr = p.P + L.w + (int64_t)(nok ? n : 0) * K + q;
            int ph[TAP_MJ], pw[TAP_MJ];
            bool mok[TAP_MJ];
#pragma unroll
            for (int j = 0; j < TAP_MJ; ++j) {
                const int m = (mt0 + j) * 16 + l16;
                mok[j] = m < M;
                const int mm = mok[j] ? m : 0;
                ph[j] = mm / W;
                pw[j] = mm - ph[j] * W;
            }
            tap_f32x4 acc[TAP_MJ];
#pragma unroll
            for (int j = 0; j < TAP_MJ; ++j) acc[j] = tap_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kh = 0; kh < k; ++kh)
                for (int kw = 0; kw < k; ++kw) {
                    int base[TAP_MJ];
                    bool ok[TAP_MJ];
#pragma unroll
                    for (int j = 0; j < TAP_MJ; ++j) {
                        const int hh = ph[j] + kh - pad, ww = pw[j] + kw - pad;
                        ok[j] = mok[j] && hh >= 0 && hh < H && ww >= 0 && ww < W;
                        base[j] = ok[j] ? (hh * W + ww) * pin + q : q;  // q: inside the plane whatever the tap
                    }
                    const float* wt = wr + (kh * k + kw) * C;
                    for (int c0 = 0; c0 < C; c0 += 4 * TAP_U) {  // TAP_U weight loads issued, then their MFMAs in order
                        // every load is issued unconditionally at a clamped, valid address (row 0 for a channel past
                        // Cout, the tap's last four channels past Cin, the plane's start for a tap outside the map) and
                        // the value selected afterwards: straight-line code, the loads in flight together
                        float bv[TAP_U], av[TAP_U][TAP_MJ];
#pragma unroll
                        for (int u = 0; u < TAP_U; ++u) {
                            const int ci = c0 + 4 * u < C ? c0 + 4 * u : C - 4;
                            bv[u] = wt[ci];
#pragma unroll
                            for (int j = 0; j < TAP_MJ; ++j) av[u][j] = cur[base[j] + ci];
                        }
#pragma unroll
                        for (int u = 0; u < TAP_U; ++u)
                            if (c0 + 4 * u < C) {  // wave-uniform
#pragma unroll
                                for (int j = 0; j < TAP_MJ; ++j)
                                    if (mt0 + j < MT)  // wave-uniform
                                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok[j] ? av[u][j] : 0.f,
                                                                                      nok ? bv[u] : 0.f, acc[j], 0, 0, 0);
                            }
                    }
                }
            // C layout of 16x16x4: column (channel) = lane & 15, row (pixel) = 4 (lane >> 4) + reg
            if (nok) {
                const float bias = p.P[L.b + n], rm = p.P[L.rm + n], is = 1.f / sqrtf(p.P[L.rv + n] + 1e-5f);
                const float g = p.P[L.g + n], be = p.P[L.be + n];
#pragma unroll
                for (int j = 0; j < TAP_MJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = (mt0 + j) * 16 + 4 * q + r;
                        if (m < M) {
                            float h = ((acc[j][r] + bias) - rm) * is;
                            h = g * h + be;
                            nxt[m * pout + n] = fmaxf(h, 0.f);
                        }
                    }
            }
        }
        __syncthreads();
        {
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
        C = Co;
        if (p.t.pool[li]) {  // MaxPool2d(2, 2), floor mode: the first maximum in window order, NaN kept
            const int Ho = H / 2, Wo = W / 2;
            for (int e = tid; e < Ho * Wo * C; e += TAP_NT) {
                const int t = e / C, c = e - t * C, ho = t / Wo, wo = t - ho * Wo;
                float best = -__builtin_inff();
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j) {
                        const float v = cur[((2 * ho + i) * W + 2 * wo + j) * pout + c];
                        if (v > best || v != v) best = v;
                    }
                nxt[t * pout + c] = best;
            }
            __syncthreads();
            float* t = cur;
            cur = nxt;
            nxt = t;
            H = Ho;
            W = Wo;
        }
    }
    // the linear stacks; the first reads the last map in (h, w, c) order through its pitch
    int pc = C;
    for (int l = 0; l < p.t.nlin; ++l) {
        const TapLayer L = p.lin[l];
        const int din = p.t.dims[l], dout = p.t.dims[l + 1];
        const bool last = l == p.t.nlin - 1;
        for (int o = wid; o < dout; o += TAP_NT / 64) {  // wave-uniform
            const float* w = p.P + L.w + (int64_t)o * din;
            float acc = 0.f;
            for (int kk = lane; kk < din; kk += 64) acc = fmaf(cur[kk + kk / pc], w[kk], acc);
            for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
            if (lane == 0) {
                const float z = acc + p.P[L.b + o];
                if (last) {
                    const double e = (double)z;
                    p.est[img] = e;
                    p.flag[img] = e > p.threshold ? 1 : 0;
                } else {
                    float h = (z - p.P[L.rm + o]) * (1.f / sqrtf(p.P[L.rv + o] + 1e-5f));
                    h = p.P[L.g + o] * h + p.P[L.be + o];
                    nxt[o] = fmaxf(h, 0.f);
                }
            }
        }
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
        pc = 0x7fffffff;  // a hidden vector is dense
    }
}

// est = (double) est32, flag = est > threshold (strict, edgedet_offload_flag's test): the tail of the layered path.
__global__ void __launch_bounds__(TAP_NT) tapnet_finish_kernel(const float* __restrict__ est32, int64_t B,
                                                               double threshold, double* __restrict__ est,
                                                               uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * TAP_NT + threadIdx.x;
    if (i >= B) return;
    const double e = (double)est32[i];
    est[i] = e;
    flag[i] = e > threshold ? 1 : 0;
}

static int tap_set_lds(size_t bytes) {
    static std::mutex mu;
    static size_t done = 64 * 1024;  // what a kernel may take without the attribute
    std::lock_guard<std::mutex> lk(mu);
    if (bytes <= done) return 0;
    EDGEDET_CHECK_HIP(hipFuncSetAttribute((const void*)tapnet_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          TAPNET_LDS_MAX));
    done = TAPNET_LDS_MAX;
    return 0;
}

static bool tap_shape(int32_t S, int32_t cin, int32_t nconv, const int32_t* channels, const int32_t* kernels,
                      const int32_t* pools, int32_t nlin, const int32_t* dims, TapnetShape* t) {
    if (!channels || !kernels || !pools || !dims || nconv < 1 || nconv > TAPNET_MAXL || nlin < 1 || nlin > TAPNET_MAXL)
        return false;
    *t = TapnetShape{};
    t->S = S;
    t->cin = cin;
    t->nconv = nconv;
    t->nlin = nlin;
    for (int i = 0; i < nconv; ++i) {
        t->cout[i] = channels[i];
        t->k[i] = kernels[i];
        t->pool[i] = pools[i] != 0;
    }
    for (int l = 0; l <= nlin; ++l) t->dims[l] = dims[l];
    return true;
}

// ConvSpec's state layout (edgeml_amd/convnet.py): per layer w, b and (BatchNorm) gamma, beta; then the running
// mean and variance of every BatchNorm in the same order.  Returns the vector's length.
static int64_t tap_layout(const TapnetShape& t, TapLayer* conv, TapLayer* lin) {
    int64_t o = 0;
    int c = t.cin;
    for (int i = 0; i < t.nconv; ++i) {
        const int64_t nw = (int64_t)t.cout[i] * t.k[i] * t.k[i] * c;
        conv[i].w = (int)o;
        conv[i].b = (int)(o + nw);
        conv[i].g = (int)(o + nw + t.cout[i]);
        conv[i].be = (int)(o + nw + 2 * t.cout[i]);
        o += nw + 3 * (int64_t)t.cout[i];
        c = t.cout[i];
        if (o >= (1ll << 30)) return -1;
    }
    for (int l = 0; l < t.nlin; ++l) {
        const int64_t nw = (int64_t)t.dims[l] * t.dims[l + 1];
        const bool bn = l < t.nlin - 1;
        lin[l].w = (int)o;
        lin[l].b = (int)(o + nw);
        lin[l].g = (int)(o + nw + t.dims[l + 1]);
        lin[l].be = (int)(o + nw + 2 * t.dims[l + 1]);
        o += nw + (bn ? 3 : 1) * (int64_t)t.dims[l + 1];
        if (o >= (1ll << 30)) return -1;
    }
    for (int i = 0; i < t.nconv; ++i) {
        conv[i].rm = (int)o;
        conv[i].rv = (int)(o + t.cout[i]);
        o += 2 * (int64_t)t.cout[i];
    }
    for (int l = 0; l + 1 < t.nlin; ++l) {
        lin[l].rm = (int)o;
        lin[l].rv = (int)(o + t.dims[l + 1]);
        o += 2 * (int64_t)t.dims[l + 1];
    }
    return o;
}

}  // namespace edgedet

using namespace edgedet;

extern "C" int64_t edgedet_tapnet_lds(int32_t S, int32_t cin, int32_t nconv, const int32_t* channels,
                                      const int32_t* kernels, const int32_t* pools, int32_t nlin, const int32_t* dims) {
    TapnetShape t;
    if (!tap_shape(S, cin, nconv, channels, kernels, pools, nlin, dims, &t)) return -1;
    return tapnet_lds(t);
}

extern "C" int edgedet_tapnet_fits(int32_t S, int32_t cin, int32_t nconv, const int32_t* channels,
                                   const int32_t* kernels, const int32_t* pools, int32_t nlin, const int32_t* dims) {
    TapnetShape t;
    return tap_shape(S, cin, nconv, channels, kernels, pools, nlin, dims, &t) && tapnet_fits(t) ? 1 : 0;
}

extern "C" int edgedet_tapnet_infer(const float* x, int64_t B, int32_t S, int32_t cin, int32_t nconv,
                                    const int32_t* channels, const int32_t* kernels, const int32_t* pools, int32_t nlin,
                                    const int32_t* dims, const float* state, int64_t ns, double threshold, double* est,
                                    uint8_t* flag, void* stream) {
    TapnetParams p{};
    if (!tap_shape(S, cin, nconv, channels, kernels, pools, nlin, dims, &p.t) || !tapnet_fits(p.t)) {
        set_error(std::string("edgedet: ") + TAPNET_DOMAIN);
        return EDGEDET_TAPNET_NOFIT;
    }
    EDGEDET_REQUIRE(x && state && est && flag, "tapnet_infer: null pointer");
    EDGEDET_REQUIRE(B >= 1 && B < (1 << 20), "tapnet_infer: 1 <= B < 2^20");
    EDGEDET_REQUIRE(tap_layout(p.t, p.conv, p.lin) == ns, "tapnet_infer: the state vector is not this net's");
    int64_t size[2];
    tapnet_regions(p.t, size);
    p.x = x;
    p.P = state;
    p.est = est;
    p.flag = flag;
    p.threshold = threshold;
    p.region1 = (int)size[0];
    const size_t lds = 4 * (size_t)(size[0] + size[1]);
    if (tap_set_lds(lds)) return -2;
    hipLaunchKernelGGL(tapnet_kernel, dim3((unsigned)B), dim3(TAP_NT), lds, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_tapnet_finish(const float* est32, int64_t B, double threshold, double* est, uint8_t* flag,
                                     void* stream) {
    EDGEDET_REQUIRE(est32 && est && flag, "tapnet_finish: null pointer");
    EDGEDET_REQUIRE(B >= 1 && B < (1 << 20), "tapnet_finish: 1 <= B < 2^20");
    hipLaunchKernelGGL(tapnet_finish_kernel, dim3((unsigned)cdiv(B, TAP_NT)), dim3(TAP_NT), 0, (hipStream_t)stream,
                       est32, B, threshold, est, flag);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
