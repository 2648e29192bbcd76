// Device training of lib/nn_model.py EdgeDetectionNet WITH conv stacks (regression.py:242-355 fit_CNN on the
// hidden-layer feature maps of stages 0-23): the kernels of one training step, launched one by one from the
// host loop of edgeml_amd/convnet.py (one stream, plain launches, folds one after another).
//
// Layout: NHWC everywhere, so a conv map [B][H][W][C] and a linear batch [B][D] are both a row-major matrix
// [M][C] (M = B*H*W rows of C channels, or M = B rows of D units) and every per-channel kernel below serves
// BatchNorm2d and BatchNorm1d alike.  The conv forward and the data gradient run on the existing conv engine
// (edgedet_conv2d_ex, fp32 MFMA path): the data gradient is the same conv with the weight flipped and
// transposed, [Cin][k][k][Cout], which cnn_repack_kernel writes beside the forward pack after every Adam step.
//
// cnn_wgrad_kernel   dW[co][kh][kw][ci] = sum_{b,h,w} dy[b,h,w,co] x[b,h+kh-p,w+kw-p,ci] on v_mfma_f32_16x16x4_f32:
//                    a GEMM with M = Cout, N = k*k*Cin, K = B*H*W.  An f32 MFMA is a plain k-ordered fma chain, so
//                    K is cut into stages of 64 pixels, each summed from zero and added once into the running sum;
//                    the four waves of a workgroup take the stages round-robin and their sums meet in LDS in wave
//                    order.  No atomics: two runs are bit-identical.
// cnn_bn_stats_kernel / cnn_col_reduce_kernel   per-channel reductions over the M rows: 32 row groups per channel,
//                    each a sequential sum, combined in group order.
// cnn_act_fwd_kernel (BatchNorm apply) + ReLU + Dropout, cnn_act_bwd_kernel its backward
//                    (dy - mean(dy) - xhat mean(dy xhat)) gamma invstd, the formulas of estimator.hip.
// Dropout masks: mlp_hash(seed ^ fold << 48 ^ layer << 40, step << 32 | index), kept when u >= p, scaled by
//                    1 / (1 - p).  `index` is the element's NCHW flat index ((b C + c) H + h) W + w (for a linear
//                    layer, H = W = 1, that is b D + c), so a mask does not depend on the device layout.
#include "dropout_hash.hpp"
#include "kernels.hpp"

namespace edgedet {

typedef float cnn_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CNN_NT = 256;
constexpr int WG_STAGE = 64;  // pixels per stage sum: 16 MFMAs of 4

struct WgradParams {
    const float* x;   // [B][H][W][Cin]
    const float* dy;  // [B][H][W][Cout]
    float* dw;        // [Cout][k][k][Cin]
    int B, H, W, Cin, Cout, k, pad;
    int N, K;  // k*k*Cin, B*H*W
    FastDiv div_hw, div_w, div_cin, div_k;
};

// One workgroup: a 32 (co) x 32 (n) tile of dW as 2 x 2 MFMA tiles per wave, every wave over its own stages.
__global__ void __launch_bounds__(CNN_NT) cnn_wgrad_kernel(WgradParams p) {
    __shared__ float red[4][32 * 33];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    // this lane's two weight columns (kh, kw, ci) and two output channels
    int dh[2], dwv[2], ci[2], co[2];
    bool nok[2], cok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 16 * j + l16;
        nok[j] = n < p.N;
        const int nn = nok[j] ? n : 0;
        const int t = (int)fdiv((uint32_t)nn, p.div_cin);
        ci[j] = nn - t * p.Cin;
        const int kh = (int)fdiv((uint32_t)t, p.div_k);
        dh[j] = kh - p.pad;
        dwv[j] = t - kh * p.k - p.pad;
        co[j] = co0 + 16 * j + l16;
        cok[j] = co[j] < p.Cout;
    }
    cnn_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = cnn_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nstage = (p.K + WG_STAGE - 1) / WG_STAGE;
    for (int st = wid; st < nstage; st += 4) {  // wave-uniform
        cnn_f32x4 s[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) s[i][j] = cnn_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ks = 0; ks < WG_STAGE / 4; ++ks) {
            const int px = st * WG_STAGE + 4 * ks + q;  // this lane's pixel (b, h, w) of the K step
            const bool pok = px < p.K;
            const int pp = pok ? px : 0;
            const int b = (int)fdiv((uint32_t)pp, p.div_hw);
            const int hw = pp - b * p.H * p.W;
            const int h = (int)fdiv((uint32_t)hw, p.div_w);
            const int w = hw - h * p.W;
            float a[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = pok && cok[i] ? p.dy[(int64_t)pp * p.Cout + co[i]] : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int hh = h + dh[j], ww = w + dwv[j];
                const bool ok = pok && nok[j] && hh >= 0 && hh < p.H && ww >= 0 && ww < p.W;
                bv[j] = ok ? p.x[(((int64_t)b * p.H + hh) * p.W + ww) * p.Cin + ci[j]] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) s[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], s[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] += s[i][j];
    }
    // C layout of 16x16x4: column (n) = lane & 15, row (co) = 4 (lane >> 4) + reg
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wid][(16 * i + 4 * q + r) * 33 + 16 * j + l16] = acc[i][j][r];
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += CNN_NT) {
        const int r = e >> 5, c = e & 31;
        const float v = ((red[0][r * 33 + c] + red[1][r * 33 + c]) + red[2][r * 33 + c]) + red[3][r * 33 + c];
        if (co0 + r < p.Cout && n0 + c < p.N) p.dw[(int64_t)(co0 + r) * p.N + n0 + c] = v;
    }
}

// w [Cout][k][k][Cin] -> the conv engine's packs: wf [Cout][kpf] (the same order, rows padded) and, when wb is
// given, wb [Cin][kpb] holding w flipped and transposed, wb[ci][k-1-kh][k-1-kw][co].  The pads stay as they are.
__global__ void __launch_bounds__(CNN_NT) cnn_repack_kernel(const float* __restrict__ w, int Cout, int Cin, int k,
                                                            int kpf, int kpb, float* __restrict__ wf,
                                                            float* __restrict__ wb) {
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    const int N = k * k * Cin;
    if (e >= (int64_t)Cout * N) return;
    const int co = (int)(e / N), n = (int)(e - (int64_t)co * N);
    const int t = n / Cin, ci = n - t * Cin, kh = t / k, kw = t - kh * k;
    const float v = w[e];
    wf[(int64_t)co * kpf + n] = v;
    if (wb) wb[(int64_t)ci * kpb + ((k - 1 - kh) * k + (k - 1 - kw)) * Cout + co] = v;
}

// Train-mode batch statistics of z [M][C]: mean, invstd = 1 / sqrt(biased var + 1e-5), and the running
// estimates (momentum 0.1, the unbiased variance).  32 channels x 32 row groups per workgroup.
__global__ void __launch_bounds__(1024) cnn_bn_stats_kernel(const float* __restrict__ z, int M, int C,
                                                            float* __restrict__ rm, float* __restrict__ rv,
                                                            float* __restrict__ mean, float* __restrict__ invstd) {
    __shared__ float red[32][33];
    __shared__ float mu[32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const bool ok = c < C;
    float s = 0.f;
    if (ok)
        for (int r = g; r < M; r += 32) s += z[(int64_t)r * C + c];
    red[g][cl] = s;
    __syncthreads();
    if (g == 0) {
        float t = 0.f;
        for (int j = 0; j < 32; ++j) t += red[j][cl];
        mu[cl] = t / (float)M;
    }
    __syncthreads();
    const float m = mu[cl];
    float v = 0.f;
    if (ok)
        for (int r = g; r < M; r += 32) {
            const float d = z[(int64_t)r * C + c] - m;
            v = fmaf(d, d, v);
        }
    red[g][cl] = v;
    __syncthreads();
    if (g == 0 && ok) {
        float t = 0.f;
        for (int j = 0; j < 32; ++j) t += red[j][cl];
        const float var = t / (float)M;
        mean[c] = m;
        invstd[c] = 1.f / sqrtf(var + 1e-5f);
        rm[c] = 0.9f * rm[c] + 0.1f * m;
        rv[c] = 0.9f * rv[c] + 0.1f * (M > 1 ? t / (float)(M - 1) : var);
    }
}

// Column sums over the M rows.  a == null: out0[c] = sum_r v[r][c] (a bias gradient).  Otherwise v is the
// gradient da behind ReLU + Dropout, dy = a > 0 ? da * scale : 0, and out0 = sum dy (dbeta), out1 = sum dy xhat
// (dgamma).
__global__ void __launch_bounds__(1024) cnn_col_reduce_kernel(const float* __restrict__ v, const float* __restrict__ a,
                                                              const float* __restrict__ xhat, int M, int C, float scale,
                                                              float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ float red0[32][33];
    __shared__ float red1[32][33];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const bool ok = c < C;
    float s0 = 0.f, s1 = 0.f;
    if (ok)
        for (int r = g; r < M; r += 32) {
            const int64_t e = (int64_t)r * C + c;
            if (a) {
                const float dy = a[e] > 0.f ? v[e] * scale : 0.f;
                s0 += dy;
                s1 = fmaf(dy, xhat[e], s1);
            } else {
                s0 += v[e];
            }
        }
    red0[g][cl] = s0;
    red1[g][cl] = s1;
    __syncthreads();
    if (g == 0 && ok) {
        float t0 = 0.f, t1 = 0.f;
        for (int j = 0; j < 32; ++j) {
            t0 += red0[j][cl];
            t1 += red1[j][cl];
        }
        out0[c] = t0;
        if (a) out1[c] = t1;
    }
}

// mode 0: h = z.  mode 1: h = (z - mean) invstd (batch statistics).  mode 2: the same with mean = running mean
// and invstd = 1 / sqrt(running var + 1e-5) taken from `mean` and `invstd`.  a = dropout(relu(gamma h + beta)).
__global__ void __launch_bounds__(CNN_NT) cnn_act_fwd_kernel(const float* __restrict__ z, int64_t n, int C, int HW,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, int mode, float drop,
                                                             uint64_t key, uint64_t step, float* __restrict__ xhat,
                                                             float* __restrict__ a) {
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= n) return;
    const int64_t r = e / C;
    const int c = (int)(e - r * C);
    float h = z[e];
    if (mode != 0) {
        const float is = mode == 1 ? invstd[c] : 1.f / sqrtf(invstd[c] + 1e-5f);
        h = (h - mean[c]) * is;
        if (xhat) xhat[e] = h;
        h = gamma[c] * h + beta[c];
    }
    float v = fmaxf(h, 0.f);
    if (drop > 0.f) {
        const int64_t b = r / HW, pix = r - b * HW;
        const uint64_t idx = (uint64_t)((b * C + c) * HW + pix);
        v = hash_keep(mlp_hash(key, (step << 32) | idx), drop) ? v * (1.f / (1.f - drop)) : 0.f;
    }
    a[e] = v;
}

// dz from da: dy = a > 0 ? da * scale : 0, then (bn) (dy - sdy / M - xhat sdyx / M) invstd gamma.
__global__ void __launch_bounds__(CNN_NT) cnn_act_bwd_kernel(const float* __restrict__ da, const float* __restrict__ a,
                                                             const float* __restrict__ xhat, int64_t n, int C, int M,
                                                             float scale, const float* __restrict__ gamma,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ sdy,
                                                             const float* __restrict__ sdyx, int bn,
                                                             float* __restrict__ dz) {
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= n) return;
    const int c = (int)(e % C);
    const float dy = a[e] > 0.f ? da[e] * scale : 0.f;
    dz[e] = bn ? (dy - sdy[c] / (float)M - xhat[e] * (sdyx[c] / (float)M)) * invstd[c] * gamma[c] : dy;
}

// MaxPool2d(2, 2), floor mode: the first maximum in window order (kh, then kw), torch's test (v > best or NaN).
__global__ void __launch_bounds__(CNN_NT) cnn_maxpool_fwd_kernel(const float* __restrict__ x, int B, int H, int W, int C,
                                                                 float* __restrict__ y, int32_t* __restrict__ idx) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= (int64_t)B * Ho * Wo * C) return;
    const int c = (int)(e % C);
    int64_t t = e / C;
    const int wo = (int)(t % Wo);
    t /= Wo;
    const int ho = (int)(t % Ho), b = (int)(t / Ho);
    float best = -__builtin_inff();
    int bi = (2 * ho) * W + 2 * wo;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int h = 2 * ho + i, w = 2 * wo + j;
            const float v = x[(((int64_t)b * H + h) * W + w) * C + c];
            if (v > best || v != v) {
                best = v;
                bi = h * W + w;
            }
        }
    y[e] = best;
    idx[e] = bi;
}

// One thread per input element: it takes its window's gradient when it is that window's argmax.
__global__ void __launch_bounds__(CNN_NT) cnn_maxpool_bwd_kernel(const float* __restrict__ dy,
                                                                 const int32_t* __restrict__ idx, int B, int H, int W,
                                                                 int C, float* __restrict__ dx) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= (int64_t)B * H * W * C) return;
    const int c = (int)(e % C);
    int64_t t = e / C;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H), b = (int)(t / H);
    const int ho = h / 2, wo = w / 2;
    float g = 0.f;
    if (ho < Ho && wo < Wo) {
        const int64_t o = (((int64_t)b * Ho + ho) * Wo + wo) * C + c;
        if (idx[o] == h * W + w) g = dy[o];
    }
    dx[e] = g;
}

// torch.mean(x, dim=(2, 3)): y[b][c] = sum_p x[b][p][c] / HW, pixels in order.
__global__ void __launch_bounds__(CNN_NT) cnn_gmean_fwd_kernel(const float* __restrict__ x, int B, int HW, int C,
                                                               float* __restrict__ y) {
    const int e = blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= B * C) return;
    const int b = e / C, c = e - b * C;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += x[((int64_t)b * HW + p) * C + c];
    y[e] = s / (float)HW;
}

__global__ void __launch_bounds__(CNN_NT) cnn_gmean_bwd_kernel(const float* __restrict__ dy, int B, int HW, int C,
                                                               float* __restrict__ dx) {
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= (int64_t)B * HW * C) return;
    const int c = (int)(e % C);
    const int b = (int)(e / ((int64_t)HW * C));
    dx[e] = dy[b * C + c] / (float)HW;
}

// z[i][o] = b[o] + sum_k x[i][k] W[o][k]: one wave per output, lane l over k = l, l + 64, ..., the 64 partial
// sums combined by a fixed butterfly.
__global__ void __launch_bounds__(CNN_NT) cnn_linear_fwd_kernel(const float* __restrict__ x, int B, int din, int dout,
                                                                const float* __restrict__ W,
                                                                const float* __restrict__ bias, float* __restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int64_t o_ = (int64_t)blockIdx.x * (CNN_NT / 64) + (threadIdx.x >> 6);
    if (o_ >= (int64_t)B * dout) return;  // wave-uniform
    const int i = (int)(o_ / dout), o = (int)(o_ - (int64_t)i * dout);
    const float* r = x + (int64_t)i * din;
    const float* w = W + (int64_t)o * din;
    float acc = 0.f;
    for (int k = lane; k < din; k += 64) acc = fmaf(r[k], w[k], acc);
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) z[o_] = acc + bias[o];
}

// dx[i][k] = sum_o dz[i][o] W[o][k], o ascending
__global__ void __launch_bounds__(CNN_NT) cnn_linear_dx_kernel(const float* __restrict__ dz, int B, int din, int dout,
                                                               const float* __restrict__ W, float* __restrict__ dx) {
    const int64_t e = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (e >= (int64_t)B * din) return;
    const int i = (int)(e / din), k = (int)(e - (int64_t)i * din);
    float acc = 0.f;
    for (int o = 0; o < dout; ++o) acc = fmaf(dz[i * dout + o], W[(int64_t)o * din + k], acc);
    dx[e] = acc;
}

// loss[0] = mean (pred - y)^2 (times y when weighted), rows in order; dpred its gradient (nullable).
__global__ void __launch_bounds__(CNN_NT) cnn_loss_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                          int n, int weighted, float* __restrict__ loss,
                                                          float* __restrict__ dpred) {
    if (dpred)
        for (int i = threadIdx.x; i < n; i += CNN_NT) {
            const float d = pred[i] - y[i];
            dpred[i] = (weighted ? 2.f * d * y[i] : 2.f * d) / (float)n;
        }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) {
            const float d = pred[i] - y[i];
            s += weighted ? d * d * y[i] : d * d;
        }
        loss[0] = s / (float)n;
    }
}

// torch.optim.Adam, single-tensor path (the arithmetic of estimator.hip): g += wd p; m.lerp_(g, 0.1);
// v = 0.999 v + 0.001 g^2; p += (-step_size m) / (sqrt(v) / bc2s + 1e-8)
__global__ void __launch_bounds__(CNN_NT) cnn_adam_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                          float* __restrict__ am, float* __restrict__ av, int64_t n,
                                                          float step_size, float bc2s, float wd) {
    const int64_t t = (int64_t)blockIdx.x * CNN_NT + threadIdx.x;
    if (t >= n) return;
    const float g = G[t] + wd * P[t];
    const float mm = am[t] + 0.1f * (g - am[t]);
    const float vv = 0.999f * av[t] + 0.001f * g * g;
    am[t] = mm;
    av[t] = vv;
    const float denom = sqrtf(vv) / bc2s + 1e-8f;
    P[t] = P[t] + (-step_size * mm) / denom;
}

static unsigned cnn_grid(int64_t n) { return (unsigned)cdiv(n, CNN_NT); }

}  // namespace edgedet

using namespace edgedet;

extern "C" int edgedet_cnn_wgrad(const float* x, const float* dy, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                 int64_t Cout, int32_t k, float* dw, void* stream) {
    EDGEDET_REQUIRE(x && dy && dw, "cnn_wgrad: null pointer");
    EDGEDET_REQUIRE(k >= 1 && (k & 1) == 1, "cnn_wgrad: odd kernel sizes only ('same' padding is k / 2 on both sides)");
    EDGEDET_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "cnn_wgrad: empty problem");
    EDGEDET_REQUIRE(B * H * W < (1ll << 30) && (int64_t)k * k * Cin < (1ll << 30) && Cout < (1ll << 20),
                    "cnn_wgrad: sizes overflow int32");
    WgradParams p{};
    p.x = x;
    p.dy = dy;
    p.dw = dw;
    p.B = (int)B;
    p.H = (int)H;
    p.W = (int)W;
    p.Cin = (int)Cin;
    p.Cout = (int)Cout;
    p.k = k;
    p.pad = k / 2;
    p.N = (int)(k * k * Cin);
    p.K = (int)(B * H * W);
    p.div_hw = make_fastdiv((uint32_t)(H * W));
    p.div_w = make_fastdiv((uint32_t)W);
    p.div_cin = make_fastdiv((uint32_t)Cin);
    p.div_k = make_fastdiv((uint32_t)k);
    const dim3 grid((unsigned)cdiv(p.N, 32), (unsigned)cdiv(p.Cout, 32));
    EDGEDET_REQUIRE(grid.y < 65536, "cnn_wgrad: Cout too large");
    hipLaunchKernelGGL(cnn_wgrad_kernel, grid, dim3(CNN_NT), 0, (hipStream_t)stream, p);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_repack(const float* w, int64_t Cout, int64_t Cin, int32_t k, float* wf, float* wb,
                                  void* stream) {
    EDGEDET_REQUIRE(w && wf, "cnn_repack: null pointer");
    EDGEDET_REQUIRE(k >= 1 && (k & 1) == 1 && Cout >= 1 && Cin >= 1, "cnn_repack: odd kernel sizes only");
    const int64_t n = Cout * k * k * Cin;
    EDGEDET_REQUIRE(n < (1ll << 31), "cnn_repack: too large");
    hipLaunchKernelGGL(cnn_repack_kernel, dim3(cnn_grid(n)), dim3(CNN_NT), 0, (hipStream_t)stream, w, (int)Cout, (int)Cin,
                       (int)k, (int)edgedet_conv_weight_k(k, k, Cin), (int)edgedet_conv_weight_k(k, k, Cout), wf, wb);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_bn_stats(const float* z, int64_t M, int64_t C, float* running_mean, float* running_var,
                                    float* mean, float* invstd, void* stream) {
    EDGEDET_REQUIRE(z && running_mean && running_var && mean && invstd, "cnn_bn_stats: null pointer");
    EDGEDET_REQUIRE(M >= 1 && C >= 1 && M < (1ll << 31) && C < (1ll << 31), "cnn_bn_stats: sizes");
    hipLaunchKernelGGL(cnn_bn_stats_kernel, dim3((unsigned)cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, z, (int)M,
                       (int)C, running_mean, running_var, mean, invstd);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_col_reduce(const float* v, const float* a, const float* xhat, int64_t M, int64_t C,
                                      float scale, float* out0, float* out1, void* stream) {
    EDGEDET_REQUIRE(v && out0 && (!a || (xhat && out1)), "cnn_col_reduce: null pointer");
    EDGEDET_REQUIRE(M >= 1 && C >= 1 && M < (1ll << 31) && C < (1ll << 31), "cnn_col_reduce: sizes");
    hipLaunchKernelGGL(cnn_col_reduce_kernel, dim3((unsigned)cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, v, a, xhat,
                       (int)M, (int)C, scale, out0, out1);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_act_fwd(const float* z, int64_t M, int64_t C, int64_t HW, const float* gamma,
                                   const float* beta, const float* mean, const float* invstd, int32_t mode,
                                   float dropout, uint64_t key, uint64_t step, float* xhat, float* a, void* stream) {
    EDGEDET_REQUIRE(z && a && M >= 1 && C >= 1 && HW >= 1 && M % HW == 0, "cnn_act_fwd: null pointer or sizes");
    EDGEDET_REQUIRE(mode == 0 || (mode >= 1 && mode <= 2 && gamma && beta && mean && invstd),
                    "cnn_act_fwd: mode 1 | 2 needs gamma, beta, mean, invstd");
    EDGEDET_REQUIRE(dropout >= 0.f && dropout < 1.f && M * C < (1ll << 32) && C < (1ll << 31) && step < (1ull << 32),
                    "cnn_act_fwd: dropout in [0, 1), fewer than 2^32 elements and steps");
    hipLaunchKernelGGL(cnn_act_fwd_kernel, dim3(cnn_grid(M * C)), dim3(CNN_NT), 0, (hipStream_t)stream, z, M * C, (int)C,
                       (int)HW, gamma, beta, mean, invstd, (int)mode, dropout, key, step, xhat, a);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_act_bwd(const float* da, const float* a, const float* xhat, int64_t M, int64_t C,
                                   float scale, const float* gamma, const float* invstd, const float* sdy,
                                   const float* sdyx, int32_t bn, float* dz, void* stream) {
    EDGEDET_REQUIRE(da && a && dz && M >= 1 && C >= 1 && M < (1ll << 31) && C < (1ll << 31),
                    "cnn_act_bwd: null pointer or sizes");
    EDGEDET_REQUIRE(!bn || (xhat && gamma && invstd && sdy && sdyx), "cnn_act_bwd: bn needs xhat, gamma, invstd, sums");
    hipLaunchKernelGGL(cnn_act_bwd_kernel, dim3(cnn_grid(M * C)), dim3(CNN_NT), 0, (hipStream_t)stream, da, a, xhat, M * C,
                       (int)C, (int)M, scale, gamma, invstd, sdy, sdyx, (int)bn, dz);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_maxpool_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y,
                                       int32_t* idx, void* stream) {
    EDGEDET_REQUIRE(x && y && idx, "cnn_maxpool_fwd: null pointer");
    EDGEDET_REQUIRE(B >= 1 && H >= 2 && W >= 2 && C >= 1 && B * H * W * C < (1ll << 40) && H * W < (1ll << 31),
                    "cnn_maxpool_fwd: a 2 x 2 window needs H, W >= 2");
    hipLaunchKernelGGL(cnn_maxpool_fwd_kernel, dim3(cnn_grid(B * (H / 2) * (W / 2) * C)), dim3(CNN_NT), 0,
                       (hipStream_t)stream, x, (int)B, (int)H, (int)W, (int)C, y, idx);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_maxpool_bwd(const float* dy, const int32_t* idx, int64_t B, int64_t H, int64_t W, int64_t C,
                                       float* dx, void* stream) {
    EDGEDET_REQUIRE(dy && idx && dx, "cnn_maxpool_bwd: null pointer");
    EDGEDET_REQUIRE(B >= 1 && H >= 2 && W >= 2 && C >= 1 && B * H * W * C < (1ll << 40) && H * W < (1ll << 31),
                    "cnn_maxpool_bwd: a 2 x 2 window needs H, W >= 2");
    hipLaunchKernelGGL(cnn_maxpool_bwd_kernel, dim3(cnn_grid(B * H * W * C)), dim3(CNN_NT), 0, (hipStream_t)stream, dy,
                       idx, (int)B, (int)H, (int)W, (int)C, dx);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_gmean_fwd(const float* x, int64_t B, int64_t HW, int64_t C, float* y, void* stream) {
    EDGEDET_REQUIRE(x && y && B >= 1 && HW >= 1 && C >= 1 && B * C < (1ll << 31) && HW < (1ll << 31),
                    "cnn_gmean_fwd: null pointer or sizes");
    hipLaunchKernelGGL(cnn_gmean_fwd_kernel, dim3(cnn_grid(B * C)), dim3(CNN_NT), 0, (hipStream_t)stream, x, (int)B,
                       (int)HW, (int)C, y);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_gmean_bwd(const float* dy, int64_t B, int64_t HW, int64_t C, float* dx, void* stream) {
    EDGEDET_REQUIRE(dy && dx && B >= 1 && HW >= 1 && C >= 1 && B * C < (1ll << 31) && HW < (1ll << 31),
                    "cnn_gmean_bwd: null pointer or sizes");
    hipLaunchKernelGGL(cnn_gmean_bwd_kernel, dim3(cnn_grid(B * HW * C)), dim3(CNN_NT), 0, (hipStream_t)stream, dy, (int)B,
                       (int)HW, (int)C, dx);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_linear_fwd(const float* x, int64_t B, int64_t din, int64_t dout, const float* w,
                                      const float* bias, float* z, void* stream) {
    EDGEDET_REQUIRE(x && w && bias && z, "cnn_linear_fwd: null pointer");
    EDGEDET_REQUIRE(B >= 1 && din >= 1 && dout >= 1 && B * dout < (1ll << 31) && din < (1ll << 31), "cnn_linear_fwd: sizes");
    hipLaunchKernelGGL(cnn_linear_fwd_kernel, dim3((unsigned)cdiv(B * dout, CNN_NT / 64)), dim3(CNN_NT), 0,
                       (hipStream_t)stream, x, (int)B, (int)din, (int)dout, w, bias, z);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_linear_dx(const float* dz, int64_t B, int64_t din, int64_t dout, const float* w, float* dx,
                                     void* stream) {
    EDGEDET_REQUIRE(dz && w && dx, "cnn_linear_dx: null pointer");
    EDGEDET_REQUIRE(B >= 1 && din >= 1 && dout >= 1 && B * dout < (1ll << 31) && B * din < (1ll << 40) && din < (1ll << 31),
                    "cnn_linear_dx: sizes");
    hipLaunchKernelGGL(cnn_linear_dx_kernel, dim3(cnn_grid(B * din)), dim3(CNN_NT), 0, (hipStream_t)stream, dz, (int)B,
                       (int)din, (int)dout, w, dx);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_loss(const float* pred, const float* y, int64_t n, int32_t weighted, float* loss,
                                float* dpred, void* stream) {
    EDGEDET_REQUIRE(pred && y && loss && n >= 1 && n < (1ll << 31), "cnn_loss: null pointer or sizes");
    hipLaunchKernelGGL(cnn_loss_kernel, dim3(1), dim3(CNN_NT), 0, (hipStream_t)stream, pred, y, (int)n, (int)weighted, loss,
                       dpred);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

extern "C" int edgedet_cnn_adam(float* param, const float* grad, float* m, float* v, int64_t n, float step_size,
                                float bc2_sqrt, float weight_decay, void* stream) {
    EDGEDET_REQUIRE(param && grad && m && v && n >= 1, "cnn_adam: null pointer or empty");
    hipLaunchKernelGGL(cnn_adam_kernel, dim3(cnn_grid(n)), dim3(CNN_NT), 0, (hipStream_t)stream, param, grad, m, v, n,
                       step_size, bc2_sqrt, weight_decay);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}
