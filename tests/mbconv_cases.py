"""Cases, constructions and restatement of the fused InvertedResidual (MBCONV record, csrc/layers.hip
mbconv_kernel), shared by test_mbconv_cases.py (CPU), test_gpu_mbconv_exact.py and
test_gpu_mbconv_budget.py.  Host tensors and references; only run_record touches the device.

A case is (B, H, W, Cin, Cexp, Cout, K, S); its tensors are x [B, H, W, Cin], w1 [Cexp, Cin], b1,
wd [Cexp, K, K], bd, w2 [Cout, Cexp], b2 (float32), the residual taken when S == 1 and Cin == Cout.

Construction L (lattice, dense weights).  x integer in [-4, 4], weights integer in [-2, 2], biases
integer in [-8, 8]: |expand| <= 32*4*2 + 8 = 264, |depthwise| <= 25*264*2 + 8 = 13,208,
|y| <= 128*13,208*2 + 12 < 3.4e6, so every partial sum in any order is an integer below 2^24 and
the float32 result does not depend on the order.  Under R6 w1 is scaled by 2^-4 and wd by 2^-3 (the
clamp at 6 would otherwise flatten almost every value): the sums are then multiples of 2^-7 below
2^11.  The device must return the float64 torch chain bit for bit.

Construction S (selection, generic values).  w1 has one nonzero +-2^e per expanded channel, w2 one
per output channel; everything else is generic float32.  Both MFMA sums are then one exact product
plus zeros, and the rest is restated in numpy float32 in the kernel's order (restate): the depthwise
sum a single-rounding fmaf chain from +0 over (kh, kw) with padded taps as zeros, the expanded
tensor zero outside the image, y = f32(f32(sel2 + b2) + x_centre).  The selected columns rotate over
the rounds of a case (sel_rounds) until every input channel and every expanded channel has been
selected, in every full wave every w1 register slot.

Construction W (wave order).  S with one +-2^e of w2 in every wave's 16 columns: each wave's
partial projection is one exact product, and the device must add the partials in wave order,
((p0 + p1) + p2) + ..., then b2, then x.  L cannot see that order (exact) and S cannot (one nonzero
partial); W does wherever three or more waves are live.

restate serves all three: its 1x1 stages are float64 matrix products rounded to float32 (per wave
for the projection), exact for L (integers) and for S and W (one term) and for nothing else.  It can
also emulate the defects the constructions are meant to see (DEFECTS).
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.fmaf32 import fma32

F32 = np.float32

# name: (B, H, W, Cin, Cexp, Cout, K, S)
CASES = {
    "b02": (2, 19, 13, 16, 64, 24, 3, 2),        # block 0.2's form, ragged tiles on both edges
    "b03": (2, 19, 13, 24, 72, 24, 3, 1),        # block 0.3's form, residual, five waves, the last half empty
    "c20": (1, 9, 11, 20, 40, 12, 5, 1),         # Cin inside CINP 24, a dead fourth wave, Cout < 16
    "c28": (1, 9, 11, 28, 100, 28, 5, 1),        # Cin inside CINP 32, residual, seven waves
    "k5s2": (2, 7, 9, 32, 112, 32, 5, 2),        # the largest K5 / S2 geometry that fits the LDS
    "w8k5": (1, 10, 8, 32, 128, 32, 5, 1),       # eight full waves, K = 5, residual
    "m1x1": (3, 1, 1, 4, 17, 4, 3, 1),           # maps smaller than the window; a one-channel last wave
    "m2x3": (1, 2, 3, 8, 16, 8, 5, 2),
    "c28s2": (1, 9, 10, 28, 72, 20, 3, 2),       # Cin inside CINP 32 at stride 2
    "loop1": (52, 40, 36, 16, 64, 16, 3, 1),     # 1,300 tiles on 512 workgroups: 2 and 3 tiles each, residual
    "loop2": (130, 37, 29, 16, 64, 24, 3, 2),    # 1,300 tiles, stride 2, ragged on both edges
    "loop5": (175, 16, 16, 32, 128, 32, 5, 1),   # 700 tiles on 256 workgroups (per_cu = 1)
}
LOOP_CASES = ("loop1", "loop2", "loop5")
L_ACTS = ("RE", "R6")
S_ACTS = ("RE", "R6", "HS")
REFUSED = (1, 8, 8, 32, 128, 32, 5, 2)   # 169,728 bytes of LDS: the launcher and the lowering say no

LDS_MAX = 160 * 1024
CANARY_BYTES = 4096
CANARY = 12345.6787109375


def residual(case):
    return case[7] == 1 and case[3] == case[5]


def out_dims(case):
    B, H, W, Cin, Cexp, Cout, K, S = case
    pad = (K - 1) // 2
    return pad, (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1


def geom(case):
    """MbwGeom, mbw_cinp, mbw_waves (csrc/kernels.hpp) and mbconv_launch_t's grid rule (csrc/layers.hip)."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    TH, TW = (8 if S == 1 else 4), 8
    IHh, IWh = (TH - 1) * S + K, (TW - 1) * S + K
    NPX = IHh * IWh
    NPXP = -(-NPX // 16) * 16
    P = TH * TW
    cinp = 16 if Cin <= 16 else 24 if Cin <= 24 else 32
    nw = max(4, -(-Cexp // 16))
    EW = max(NPXP * 17, P * 33)
    lds = 4 * (NPXP * (cinp + 2) + nw * (EW + P * 17))
    pad, Ho, Wo = out_dims(case)
    tiles_w = -(-Wo // TW)
    tiles_img = -(-Ho // TH) * tiles_w
    ntiles = B * tiles_img
    per_cu = max(1, LDS_MAX // lds)
    return dict(TH=TH, TW=TW, IHh=IHh, IWh=IWh, NPX=NPX, NPXP=NPXP, cinp=cinp, nw=nw, lds=lds, tiles_w=tiles_w,
                tiles_img=tiles_img, ntiles=ntiles, per_cu=per_cu, grid=min(ntiles, 256 * per_cu))


def _rng(name, salt):
    return np.random.default_rng(1000 * sum(map(ord, name)) + salt)


# ------------------------------------------------------------------------------------- constructions
@functools.lru_cache(maxsize=None)
def lattice_case(name, act):
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    rng = _rng(name, 1)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(F32)  # noqa: E731
    s1, sd = (F32(2.0 ** -4), F32(2.0 ** -3)) if act == "R6" else (F32(1), F32(1))
    return dict(x=ints(-4, 4, (B, H, W, Cin)), w1=ints(-2, 2, (Cexp, Cin)) * s1, b1=ints(-8, 8, Cexp),
                wd=ints(-2, 2, (Cexp, K, K)) * sd, bd=ints(-8, 8, Cexp), w2=ints(-2, 2, (Cout, Cexp)),
                b2=ints(-8, 8, Cout))


POW2 = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)   # +-2^e, e in {-1, 0, 1}


def sel_rounds(name):
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    return max(-(-Cexp // Cout), -(-Cin // 16))


def sel_columns(name, r):
    """(ci selected by each expanded channel, ce selected by each output channel) in round r: a wave's
    16 channels select 16 consecutive input channels, the next 16 a round later."""
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    return (np.arange(Cexp) + 16 * r) % Cin, (np.arange(Cout) + r * Cout) % Cexp


@functools.lru_cache(maxsize=None)
def _sel_generic(name):
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    rng = _rng(name, 2)
    x = (2.0 * rng.standard_normal((B, H, W, Cin))).astype(F32)
    x[rng.random(x.shape) < 0.1] = 0.0
    return dict(x=x, b1=(0.5 * rng.standard_normal(Cexp)).astype(F32),
                wd=(rng.standard_normal((Cexp, K, K)) / K).astype(F32),
                bd=(0.5 * rng.standard_normal(Cexp)).astype(F32), b2=rng.standard_normal(Cout).astype(F32))


@functools.lru_cache(maxsize=None)
def selection_case(name, r):
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    ci, ce = sel_columns(name, r)
    w1, w2 = np.zeros((Cexp, Cin), F32), np.zeros((Cout, Cexp), F32)
    w1[np.arange(Cexp), ci] = np.array(POW2, F32)[(np.arange(Cexp) + r) % 6]
    w2[np.arange(Cout), ce] = np.array(POW2, F32)[(np.arange(Cout) + 2 * r) % 6]
    return dict(_sel_generic(name), w1=w1, w2=w2)


W_ROUNDS = 2


@functools.lru_cache(maxsize=None)
def wave_case(name, r):
    """Construction W: the selection case of round r with w2 holding one +-2^e in every wave's 16
    columns of each row.  A wave's partial is then one exact product, and the sum of the partials is a
    float32 chain whose order shows: ((p0 + p1) + p2) + ..."""
    B, H, W, Cin, Cexp, Cout, K, S = CASES[name]
    t = selection_case(name, r)
    w2 = np.zeros((Cout, Cexp), F32)
    co = np.arange(Cout)
    for w in range(-(-Cexp // 16)):
        live = min(16, Cexp - 16 * w)
        w2[co, 16 * w + (co + 5 * r + w) % live] = np.array(POW2, F32)[(co + w + r) % 6]
    return dict(t, w2=w2)


def budget_tensors(case, seed):
    """Probe-style inputs (conv_cases.budget_case): x = randn, weights randn * sqrt(2 / K), biases 0.1 randn."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rn(B, H, W, Cin), w1=rn(Cexp, Cin) * (2.0 / Cin) ** 0.5, b1=0.1 * rn(Cexp),
             wd=rn(Cexp, K, K) * (2.0 / (K * K)) ** 0.5, bd=0.1 * rn(Cexp), w2=rn(Cout, Cexp) * (2.0 / Cexp) ** 0.5,
             b2=0.1 * rn(Cout))
    return {k: v.numpy() for k, v in t.items()}


# ------------------------------------------------------------------------------------- torch chain
def _tact(v, act):
    return {"RE": F.relu, "R6": F.relu6, "HS": F.hardswish}[act](v)


def chain(t, case, act, dtype=torch.float64):
    """The block as three F.conv2d calls on contiguous NCHW tensors of `dtype` -> NHWC [B, Ho, Wo, Cout]."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    c = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in t.items()}
    xc = c["x"].permute(0, 3, 1, 2).contiguous()
    e = _tact(F.conv2d(xc, c["w1"].reshape(Cexp, Cin, 1, 1), c["b1"]), act)
    d = _tact(F.conv2d(e, c["wd"].reshape(Cexp, 1, K, K), c["bd"], S, (K - 1) // 2, 1, Cexp), act)
    y = F.conv2d(d, c["w2"].reshape(Cout, Cexp, 1, 1), c["b2"])
    if residual(case):
        y = y + xc
    return y.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------- restatement
def act32(v, act):
    """common.hpp apply_act on a float32 array."""
    if act == "RE":
        return np.where(v > 0, v, F32(0))
    if act == "R6":
        return np.minimum(np.maximum(v, F32(0)), F32(6))
    return v * np.minimum(np.maximum(v + F32(3), F32(0)), F32(6)) / F32(6)


DEFECTS = ("leak", "residual_off", "drop_wave", "tap_order", "wave_order")


def restate(t, case, act, defect=None, wave=0):
    """mbconv_kernel in numpy float32 -> [B, Ho, Wo, Cout]; valid for L and S tensors only (module doc).
    defect: "leak"          the expanded tensor not zeroed outside the image (act(b1) in the padding);
            "residual_off"  the residual taken one pixel to the right;
            "drop_wave"     the partial projection of wave `wave` left out of the sum;
            "tap_order"     the depthwise taps walked in (kw, kh) order;
            "wave_order"    the partials added from the last wave down."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    pad, Ho, Wo = out_dims(case)
    x, b1, bd, b2 = t["x"], t["b1"], t["bd"], t["b2"]
    sel = (x.astype(np.float64).reshape(-1, Cin) @ t["w1"].astype(np.float64).T).astype(F32).reshape(B, H, W, Cexp)
    e = act32(sel + b1, act)
    ep = np.zeros((B, H + 2 * pad + S, W + 2 * pad + S, Cexp), F32)
    if defect == "leak":
        ep[:] = act32(b1, act)
    ep[:, pad:pad + H, pad:pad + W] = e
    taps = [(kh, kw) for kh in range(K) for kw in range(K)]
    if defect == "tap_order":
        taps = [(kh, kw) for kw in range(K) for kh in range(K)]
    wd = t["wd"]
    acc = np.zeros((B, Ho, Wo, Cexp), F32)
    for b in range(B):   # an image at a time: fma32's float64 temporaries stay in the cache
        a = acc[b]
        for kh, kw in taps:
            a = fma32(ep[b, kh:kh + S * Ho:S, kw:kw + S * Wo:S], wd[:, kh, kw], a)
        acc[b] = a
    d = act32(acc + bd, act)
    # a wave's partial projection (one product or none per output in S and W, integers in L), then the
    # partials added in wave order; the launcher's waves past Cexp add +0
    d64, w264 = d.astype(np.float64).reshape(-1, Cexp), t["w2"].astype(np.float64)
    waves = list(range(-(-Cexp // 16)))
    if defect == "wave_order":
        waves.reverse()
    sel2 = np.zeros((B, Ho, Wo, Cout), F32)
    for w in waves:
        if defect == "drop_wave" and w == wave:
            continue
        k = slice(16 * w, 16 * w + 16)
        sel2 = sel2 + (d64[:, k] @ w264[:, k].T).astype(F32).reshape(B, Ho, Wo, Cout)
    y = sel2 + b2
    if residual(case):
        xr = x
        if defect == "residual_off":
            xr = np.zeros_like(x)
            xr[:, :, :-1] = x[:, :, 1:]
        y = y + xr
    return y


def stale_halo(t, case, act):
    """(y, y_bad, tile): the restatement, and the same with one halo pixel of `tile`, a tile that its
    workgroup runs second, still holding what the workgroup's first tile had in that halo slot (the
    value, or the zero of a pixel outside the image).  Returned are the tile's outputs only."""
    B, H, W, Cin, Cexp, Cout, K, S = case
    g = geom(case)
    pad, Ho, Wo = out_dims(case)
    assert g["ntiles"] > g["grid"]

    def origin(tile):
        b, r = divmod(tile, g["tiles_img"])
        th, tw = divmod(r, g["tiles_w"])
        return b, th * g["TH"], tw * g["TW"]

    for tile in range(g["grid"], g["ntiles"]):
        b, oh0, ow0 = origin(tile)
        pb, poh0, pow0 = origin(tile - g["grid"])
        ih, iw = oh0 * S - pad, ow0 * S - pad          # halo slot (0, 0), the border's corner
        pih, piw = poh0 * S - pad, pow0 * S - pad
        if ih < 0 or iw < 0:
            continue
        old = t["x"][pb, pih, piw] if pih >= 0 and piw >= 0 else np.zeros(Cin, F32)
        if (old != t["x"][b, ih, iw]).any():
            break
    else:
        raise AssertionError("no tile with a distinguishable stale slot")
    one = dict(t, x=t["x"][b:b + 1])
    sub = (1,) + tuple(case[1:])
    y1 = restate(one, sub, act)
    xb = one["x"].copy()
    xb[0, ih, iw] = old
    y1b = restate(dict(one, x=xb), sub, act)
    region = (slice(oh0, oh0 + g["TH"]), slice(ow0, ow0 + g["TW"]))   # only this tile saw the stale slot
    return y1[0][region], y1b[0][region], tile


def same_bits(got, want):
    """Mask of the elements whose bit patterns differ, -0 and +0 counted equal."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got.view(np.int32) != want.view(np.int32)) & ~((got == 0) & (want == 0))


def assert_same_bits(got, want, what=""):
    bad = same_bits(got, want)
    assert not bad.any(), (what, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ------------------------------------------------------------------------------------- device
def launch(t, case, act, fill=float("nan")):
    """One MBCONV record through edgedet_plan_run with y carved out of a buffer that has CANARY_BYTES of
    CANARY on each side and `fill` in between -> (return code, the whole buffer on the host, y's slice)."""
    from edgeml_amd import ops
    from edgeml_amd.plan import pack_conv_weight, pack_dw_weight
    B, H, W, Cin, Cexp, Cout, K, S = case
    pad, Ho, Wo = out_dims(case)
    p1, _, kp1, _ = pack_conv_weight(np.ascontiguousarray(t["w1"]).reshape(Cexp, Cin, 1, 1))
    p2, _, kp2, _ = pack_conv_weight(np.ascontiguousarray(t["w2"]).reshape(Cout, Cexp, 1, 1))
    host = (t["x"], p1, t["b1"], pack_dw_weight(np.ascontiguousarray(t["wd"]).reshape(Cexp, 1, K, K)), t["bd"], p2,
            t["b2"])
    dev = [torch.from_numpy(np.ascontiguousarray(a, F32)).cuda() for a in host]
    n, c = B * Ho * Wo * Cout, CANARY_BYTES // 4
    buf = torch.full((n + 2 * c,), CANARY, device="cuda")
    ys = slice(c, c + n)
    buf[ys] = fill
    rec = np.zeros(1, dtype=ops.OP_DTYPE)
    rec[0]["kind"] = ops.MBCONV
    for j, v in enumerate((B, H, W, Cin, Cexp, Cout, Ho, Wo, K, S, pad, ops.ACT[act], kp1, kp2, int(residual(case)))):
        rec[0]["i"][j] = v
    for j, d in enumerate(dev):
        rec[0]["p"][j] = d.data_ptr()
    rec[0]["p"][len(dev)] = buf.data_ptr() + CANARY_BYTES
    rc = ops.lib().edgedet_plan_run(rec.ctypes.data_as(ctypes.c_void_p), 1, ops.stream_handle())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), ys


def run_record(t, case, act):
    """The record run twice -> y [B, Ho, Wo, Cout] on the host: the canary intact, every element
    finite, the two runs bit-identical (the kernel has no atomics)."""
    from edgeml_amd import ops
    pad, Ho, Wo = out_dims(case)
    outs = []
    for _ in range(2):
        rc, buf, ys = launch(t, case, act)
        ops.check(rc)
        frame = np.concatenate([buf[:ys.start], buf[ys.stop:]])
        assert (frame == F32(CANARY)).all(), "canary overwritten"
        assert np.isfinite(buf[ys]).all(), "an output element was not written (or is not finite)"
        outs.append(buf[ys])
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "two runs differ"
    return outs[0].reshape(case[0], Ho, Wo, case[5])


# ------------------------------------------------------------------------------------- budget
# name: (case, act); N = B * Ho * Wo * Cout is 24,576 / 38,400 / 9,600 / 18,432.  The K5 / S2 shape is
# kept as it was specified although it ends 4 % short of the 10,000 outputs the others have: the
# sampling noise of its mean, 1 / sqrt(N) of rms(e), is 0.0102 rms(e) against 0.0100.
BUDGET_MIN_N = 9600
BUDGET_SHAPES = {
    "b02": ((1, 64, 64, 16, 64, 24, 3, 2), "RE"),
    "b03": ((1, 40, 40, 24, 72, 24, 3, 1), "RE"),    # residual
    "k5s2": ((1, 48, 40, 12, 40, 20, 5, 2), "HS"),
    "k5w8": ((1, 24, 24, 32, 128, 32, 5, 1), "R6"),  # residual
}
RMS_FACTOR = 4.0    # conv_cases.RMS_FACTOR: fp32 MFMA stage-sum kernels
BIAS_FACTOR = 0.1   # conv_cases.BIAS_FACTOR


@functools.lru_cache(maxsize=None)
def budget_case(name):
    """dict: t (tensors), ref (float64 torch chain), e_ref (torch's float32 CPU chain - ref), scale."""
    case, act = BUDGET_SHAPES[name]
    t = budget_tensors(case, 1000 * sum(map(ord, name)) + 3)
    ref = chain(t, case, act, torch.float64)
    cpu = chain(t, case, act, torch.float32).double()
    return dict(t=t, ref=ref, e_ref=cpu - ref, scale=ref.abs().max().item())


def rms(e):
    return e.double().pow(2).mean().sqrt().item()


def ratios(y, c):
    """(rms(e) / rms(e_ref), mean(e) / rms(e_ref)) of a result y [B, Ho, Wo, Cout]."""
    e = torch.as_tensor(y).double() - c["ref"]
    r = rms(c["e_ref"])
    return rms(e) / r, e.mean().item() / r
