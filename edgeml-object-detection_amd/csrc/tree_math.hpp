// What the exact tree builders (gbr.hip, rfr.hip) share: sums of squares of fixed-point targets carried in
// 32-bit limbs, and sklearn's impurity rule evaluated on them in 128-bit integers.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace edgedet {

typedef unsigned long long gu64;
typedef unsigned __int128 gu128;

constexpr int TREE_QMIN = 26, TREE_QMAX = 1000;  // the fixed-point scale q the impurity rule is built for

__device__ __forceinline__ int tree_ceil_log2(int64_t n) { return n <= 1 ? 0 : 64 - __clzll((gu64)(n - 1)); }

// r^2 as four 32-bit limbs, least significant first: a sum of fewer than 2^31 of them (or of w r^2 with the
// weights w adding up to less than 2^31) fits four 64-bit accumulators.
__device__ __forceinline__ void tree_sq_limbs(int64_t r, gu64* limb) {
    const gu64 a = r < 0 ? 0ull - (gu64)r : (gu64)r;
    const gu64 lo = a * a, hi = __umul64hi(a, a);
    limb[0] = lo & 0xffffffffull;
    limb[1] = lo >> 32;
    limb[2] = hi & 0xffffffffull;
    limb[3] = hi >> 32;
}

// sklearn's impurity <= EPSILON (2^-52) on the integers: W Q - S^2 <= W^2 2^(2q - 52), W the (weighted) count,
// S the sum, Q4 the limbs of the sum of squares.  Q < 2^(124 - log2 W) and |S| < 2^62 while no target
// overflowed, so both sides fit 128 bits or the right one exceeds 2^124.
__device__ __forceinline__ bool tree_pure(int W, int64_t S, const gu64* Q4, int q) {
    const gu128 Q = ((gu128)Q4[3] << 96) + ((gu128)Q4[2] << 64) + ((gu128)Q4[1] << 32) + (gu128)Q4[0];
    const gu64 s = S < 0 ? 0ull - (gu64)S : (gu64)S;
    const gu128 lhs = Q * (gu128)(gu64)W - (gu128)s * (gu128)s;
    const gu64 n2 = (gu64)W * (gu64)W;
    int sh = 2 * q - 52;
    if (sh < 0) sh = 0;  // q >= 26 is checked on the host
    const int bits = 64 - __clzll(n2);
    if (sh + bits > 126) return true;
    return lhs <= ((gu128)n2 << sh);
}

}  // namespace edgedet
