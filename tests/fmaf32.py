"""fmaf in numpy, for the restatements of kernels that accumulate with a single-rounding fused
multiply-add (test_gpu_dwconv_exact.py, mbconv_cases.py).  test_gpu_dwconv_exact.py checks it against
libm's fmaf."""
import numpy as np

F32 = np.float32
_LOW29, _MID29 = np.int64((1 << 29) - 1), np.int64(1 << 28)
_TINY = 2.0 ** -125   # below it the float32 result may be subnormal, with midpoints of its own


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays with one rounding.  The product is exact in float64; the float64
    sum is rounded to odd with its TwoSum residual, so the final rounding to float32 cannot double-round
    across a float32 tie.  Rounding is monotone and every float32 midpoint is a float64 number, so the
    float64 sum can stand on the wrong side of a midpoint only by standing on it: the residual is
    worked out for those sums alone (and for the tiny ones, whose midpoints are the subnormals')."""
    a64, b64, c64 = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    p = a64 * b64
    s = np.asarray(p + c64)
    cand = ((s.view(np.int64) & _LOW29) == _MID29) | ((np.abs(s) < _TINY) & (s != 0))
    if cand.any():
        p, c64 = np.broadcast_to(p, s.shape)[cand], np.broadcast_to(c64, s.shape)[cand]
        sc = s[cand]
        bb = sc - p
        err = (p - (sc - bb)) + (c64 - bb)
        even = (sc.view(np.int64) & 1) == 0
        fix = np.isfinite(sc) & (err != 0) & even
        s = s.copy()
        s[cand] = np.where(fix, np.nextafter(sc, np.where(err > 0, np.inf, -np.inf)), sc)
    return s.astype(F32)
