"""Depthwise kernels, bit for bit: ops.dwconv2d_nhwc against a numpy restatement of the kernels' own
arithmetic (csrc/layers.hip dwconv_rb_kernel, dwconv_rb_se_kernel and the scalar fallbacks).

Per output the taps accumulate in (kh, kw) order with a single-rounding fmaf from +0, padded taps are
left out, then + bias and the activation in float32 (common.hpp apply_act).  The SE partial sums add
the outputs in the kernels' order: a lane takes the four-pixel groups g0 + gl, g0 + gl + 16, ... of
its split, o = 0..3 within a group, and the 16 lane sums are added in lane order.  Equality is on the
bit patterns, so the file passes unchanged on any library that keeps that arithmetic.
"""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

from tests.fmaf32 import fma32

DEV = "cuda"
F32 = np.float32


def test_fma32_matches_libm_fmaf():
    """The helper against libm's fmaf: random operands, and operands built to sit next to a float32
    tie of the float64 sum (product = half an ulp of c times (1 +- u^3), u = 2^-10 or 2^-11)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(7)
    n = 20000
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    c = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype(F32)
    # ties: c = m * 2^e with a 24-bit m, a * b = +-2^(e-24) * (1 +- u^3)
    m = rng.integers(1 << 23, 1 << 24, n).astype(np.float64)
    e = rng.integers(-20, 20, n)
    ct = (np.ldexp(m, e - 23) * rng.choice([-1.0, 1.0], n)).astype(F32)
    u = np.ldexp(1.0, -rng.integers(10, 12, n))
    sg = rng.choice([-1.0, 1.0], n)
    at = (1.0 + sg * u).astype(F32)
    bt = (np.ldexp(1.0 - sg * u + u * u, e - 24) * rng.choice([-1.0, 1.0], n)).astype(F32)
    # results in float32's subnormal range, whose midpoints are not the normal range's
    an = (rng.standard_normal(n) * 1e-19).astype(F32)
    bn = (rng.standard_normal(n) * 1e-20).astype(F32)
    cn = (rng.standard_normal(n) * 1e-39).astype(F32)
    a, b, c = np.concatenate([a, at, an]), np.concatenate([b, bt, bn]), np.concatenate([c, ct, cn])
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)
    got = fma32(a, b, c)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the constructed half really needs the residual: plain float64 rounding gets some of them wrong
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (plain[n:2 * n].view(np.int32) != want[n:2 * n].view(np.int32)).any()


def _act(v, act):
    if act == "RE":
        return np.where(v > 0, v, F32(0))
    if act == "HS":
        return v * np.minimum(np.maximum(v + F32(3), F32(0)), F32(6)) / F32(6)
    return v


def _inputs(B, H, W, C, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, C)).astype(F32)
    x[rng.random(x.shape) < 0.1] = 0.0
    w = (rng.standard_normal((k * k, C)) / k).astype(F32)  # [K*K][C] taps, about half of them negative
    b = (rng.standard_normal(C) * 0.1).astype(F32)
    return x, w, b


def _preact(x, w, b, k, s):
    """acc + bias for every output, [B, Ho, Wo, C] float32."""
    B, H, W, C = x.shape
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    xp = np.zeros((B, H + 2 * pad + s, W + 2 * pad + s, C), F32)
    xp[:, pad:pad + H, pad:pad + W] = x
    oh, ow = np.arange(Ho)[:, None] * s - pad, np.arange(Wo)[None, :] * s - pad
    acc = np.zeros((B, Ho, Wo, C), F32)
    for kh in range(k):
        for kw in range(k):
            valid = ((oh + kh >= 0) & (oh + kh < H) & (ow + kw >= 0) & (ow + kw < W))[None, :, :, None]
            xs = xp[:, kh:kh + s * Ho:s, kw:kw + s * Wo:s]
            acc = np.where(valid, fma32(xs, w[kh * k + kw], acc), acc)
    return acc + b


def _se_parts_rb(y, parts):
    """dwconv_rb_se_kernel's part[b][s][c]."""
    B, Ho, Wo, C = y.shape
    nwg = (Wo + 3) // 4
    G = Ho * nwg
    part = np.zeros((B, parts, C), F32)
    for sidx in range(parts):
        g0, g1 = sidx * G // parts, (sidx + 1) * G // parts
        lanes = []
        for gl in range(16):
            sm = np.zeros((B, C), F32)
            for g in range(g0 + gl, g1, 16):
                oh, ow0 = g // nwg, (g % nwg) * 4
                for o in range(4):
                    if ow0 + o < Wo:
                        sm = sm + y[:, oh, ow0 + o]
            lanes.append(sm)
        t = lanes[0]
        for q in range(1, 16):
            t = t + lanes[q]
        part[:, sidx] = t
    return part


def _se_parts_scalar(y, parts):
    """dwconv_se_kernel's (the fallback's) part[b][s][c]: pixels p0 + pl, p0 + pl + 16, ... per lane."""
    B, Ho, Wo, C = y.shape
    yf = y.reshape(B, Ho * Wo, C)
    part = np.zeros((B, parts, C), F32)
    for sidx in range(parts):
        p0, p1 = sidx * Ho * Wo // parts, (sidx + 1) * Ho * Wo // parts
        lanes = []
        for pl in range(16):
            sm = np.zeros((B, C), F32)
            for pix in range(p0 + pl, p1, 16):
                sm = sm + yf[:, pix]
            lanes.append(sm)
        t = lanes[0]
        for q in range(1, 16):
            t = t + lanes[q]
        part[:, sidx] = t
    return part


def _same_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = got.view(np.int32) != np.ascontiguousarray(want).view(np.int32)
    assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])


FLAT_SHAPES = [(2, 1, 1, 8),      # all taps but one padded
               (1, 2, 3, 24),     # map smaller than the kernel
               (2, 7, 10, 40),    # Wo not a multiple of 4, padded rows at both ends
               (1, 9, 13, 120)]   # the grid's last block partly empty


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("shape", FLAT_SHAPES)
def test_flat_bitwise(shape, s, k):
    from edgeml_amd import ops
    x, w, b = _inputs(*shape, k, seed=k * 10 + s)
    pre = _preact(x, w, b, k, s)
    xd, wd, bd = (torch.from_numpy(v).to(DEV) for v in (x, w, b))
    for act in (None, "RE", "HS"):
        _same_bits(ops.dwconv2d_nhwc(xd, wd, bd, k, s, (k - 1) // 2, act), _act(pre, act))


SE_CASES = [(2, 5, 5, 960, 5, 1, "HS"),     # parts = 1, Wo = 5
            (2, 10, 10, 72, 5, 1, "RE"),    # parts = 1, the second pass of the group loop partly masked
            (2, 40, 40, 24, 3, 1, "RE"),    # parts = 16
            (1, 40, 40, 72, 5, 2, "RE"),    # parts = 6
            (3, 13, 7, 40, 3, 2, "HS")]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C,k,s,act", SE_CASES)
def test_se_bitwise(B, H, W, C, k, s, act):
    from edgeml_amd import ops
    x, w, b = _inputs(B, H, W, C, k, seed=100 + C)
    want = _act(_preact(x, w, b, k, s), act)
    xd, wd, bd = (torch.from_numpy(v).to(DEV) for v in (x, w, b))
    y, part = ops.dwconv2d_nhwc(xd, wd, bd, k, s, (k - 1) // 2, act, se_part=True)
    assert part.shape[1] == ops.se_parts(want.shape[1], want.shape[2])
    _same_bits(y, want)
    _same_bits(part, _se_parts_rb(want, part.shape[1]))


@pytest.mark.gpu
def test_fallback_control_k7():
    """K = 7 runs the scalar kernels, which share none of the register-blocked code: the reference is
    checked against them too."""
    from edgeml_amd import ops
    x, w, b = _inputs(2, 9, 11, 24, 7, seed=77)
    want = _act(_preact(x, w, b, 7, 1), "HS")
    xd, wd, bd = (torch.from_numpy(v).to(DEV) for v in (x, w, b))
    _same_bits(ops.dwconv2d_nhwc(xd, wd, bd, 7, 1, 3, "HS"), want)
    y, part = ops.dwconv2d_nhwc(xd, wd, bd, 7, 1, 3, "HS", se_part=True)
    _same_bits(y, want)
    _same_bits(part, _se_parts_scalar(want, part.shape[1]))
