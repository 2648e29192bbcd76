"""Conv test constructions shared by test_conv_cases.py (CPU), test_gpu_conv_exact.py and
test_gpu_conv_budget.py.  Host tensors and float64 references; only gpu_conv touches the device.

Selection convs.  Every output element is ONE product of a generic float32 value with +-2^e (all
other terms are exact zeros), so the float64 conv is representable in float32 and every kernel
family must return it bit for bit: the three bf16 planes of a value sum to it exactly in any order,
a bf16 x bf16 product has 16 bits, +-2^e times a value is exact, and adding zeros is exact.
  direction A  x generic, each w[co] zero but for one K index k0 = (co + r * Cout) mod K, over
               rounds r = 0 .. ceil(K / Cout) - 1 (every K index selected at least once);
  direction B  w generic, x zero but for a lattice of period k (offset per image) whose pixels
               light one channel each; the lit channel rotates over the rounds.

Budget convs.  The inputs of tools/accuracy_probe.py (post-ReLU activations, He-scaled zero-mean
weights, a bias), the float64 conv as reference and torch's float32 CPU conv on the same tensors as
the yardstick.

bf16x6 emulation.  The conv as the nine plane-by-plane float64 convs of the operands' three bf16
planes (plan.split_bf16x3), summed over any subset of the nine: the kernels keep six.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from edgeml_amd.plan import split_bf16x3

VALS = (1.0, -1.0, 2.0, -0.5)

# name: (B, H, W, Cin, Cout, k, stride)
SEL_SHAPES = {
    "Q": (3, 11, 9, 16, 136, 3, 1),     # K = 144: four full K blocks and a half; M = 297 spans two 256-row tiles
    "S": (2, 13, 10, 8, 24, 3, 2),      # stride 2
    "T": (2, 7, 6, 40, 72, 3, 1),       # taps straddle the 32-wide K blocks
    "STEM": (1, 23, 19, 4, 64, 7, 2),   # the 7x7 stem class
    "P": (3, 11, 9, 24, 40, 1, 1),      # 1x1 with ragged K
    "K520": (2, 5, 5, 520, 48, 1, 1),   # split-K tiles: K = 520 leaves ragged quarters and eighths
    "W72": (2, 9, 7, 72, 96, 1, 1),     # the streaming tiles' widest shape
    "W20": (2, 9, 7, 20, 36, 1, 1),     # the streaming tiles, Cin no multiple of 8
    "Q32": (3, 11, 9, 32, 136, 3, 1),   # Q with Cin = 32: the pre-split input path needs Cin % 32 == 0
}


def dims(shape):
    B, H, W, Cin, Cout, k, s = shape
    pad = (k - 1) // 2
    return pad, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def conv64(x_nhwc, w, shape, bias=None):
    """float64 conv of NHWC x and OIHW w -> NHWC float64."""
    s, pad = shape[6], dims(shape)[0]
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), s, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _seed(name, salt):
    return 1000 * sum(map(ord, name)) + salt


# ------------------------------------------------------------------------------------- selection
def sel_rounds(name, direction):
    B, H, W, Cin, Cout, k, s = SEL_SHAPES[name]
    if direction == "A":
        return -(-(k * k * Cin) // Cout)
    # B: a 1x1 lights every pixel, so one round lights B*H*W channels; a k x k lattice pixel walks
    # through every channel, one per round
    return -(-Cin // (B * H * W)) if k == 1 else Cin


def sel_scale(name):
    """SE input scale of the direction-A variant: powers of two per (b, ci)."""
    B, Cin = SEL_SHAPES[name][0], SEL_SHAPES[name][3]
    g = torch.Generator().manual_seed(_seed(name, 7))
    return torch.exp2(torch.randint(-3, 4, (B, Cin), generator=g).float())


@functools.lru_cache(maxsize=None)
def sel_case(name, direction, r, se=False):
    """(x [B, H, W, Cin] float32, w [Cout, Cin, k, k] float32, ref64 [B, Ho, Wo, Cout]) of round r.
    se (direction A): the reference scales x by sel_scale(name) first (exact: powers of two)."""
    shape = SEL_SHAPES[name]
    B, H, W, Cin, Cout, k, s = shape
    K = k * k * Cin
    g = torch.Generator().manual_seed(_seed(name, 1 if direction == "A" else 2))
    if direction == "A":
        x = torch.randn(B, H, W, Cin, generator=g)
        co = torch.arange(Cout)
        k0 = (co + r * Cout) % K                       # K is ordered (kh, kw, ci): pack_conv_weight
        w = torch.zeros(Cout, Cin, k, k)
        w[co, k0 % Cin, k0 // (k * Cin), (k0 // Cin) % k] = torch.tensor(VALS)[(co + r) % 4]
    else:
        assert not se
        w = torch.randn(Cout, Cin, k, k, generator=g)
        x = torch.zeros(B, H, W, Cin)
        j = 0                                          # lattice pixels, numbered across the batch
        step = B * H * W if k == 1 else 1
        for b in range(B):
            for h in range(b % k, H, k):
                for v in range((b // k) % k, W, k):
                    x[b, h, v, (j + r * step) % Cin] = VALS[(j + 3 * r) % 4]
                    j += 1
    xin = x * sel_scale(name)[:, None, None, :] if se else x
    return x, w, conv64(xin, w, shape)


def sel_terms(x, w, shape):
    """Nonzero terms per output element."""
    return conv64((x != 0).float(), (w != 0).float(), shape)


def sel_coverage(name, direction):
    """Fraction of the K indices (kh, kw, ci) that some output element selects, over all rounds."""
    shape = SEL_SHAPES[name]
    B, H, W, Cin, Cout, k, s = shape
    K = k * k * Cin
    hit = torch.zeros(K, dtype=torch.bool)
    if direction == "A":   # x is dense: a selected K index is read wherever its tap is inside the image
        for r in range(sel_rounds(name, "A")):
            hit[(torch.arange(Cout) + r * Cout) % K] = True
        return hit.float().mean().item()
    pad = dims(shape)[0]
    onehot = torch.eye(k * k).reshape(k * k, 1, k, k).repeat(Cin, 1, 1, 1)   # channel ci * k*k + tap
    for r in range(sel_rounds(name, "B")):
        x = sel_case(name, "B", r)[0]
        seen = F.conv2d((x != 0).float().permute(0, 3, 1, 2), onehot, None, s, pad, 1, Cin)
        seen = (seen.amax((0, 2, 3)) > 0).reshape(Cin, k * k)                # [ci, tap]
        hit |= seen.t().reshape(-1)                                         # (tap, ci) order
    return hit.float().mean().item()


# ------------------------------------------------------------------------------------- budget
# name: (B, H, W, Cin, Cout, k, stride); N = B * Ho * Wo * Cout >= 10,000 outputs, K <= 2,304
BUDGET_SHAPES = {
    "K2304": (1, 13, 11, 256, 256, 3, 1),
    "K1024": (2, 9, 9, 1024, 256, 1, 1),
    "K360": (1, 13, 11, 40, 72, 3, 1),     # eleven K blocks and a quarter
    "K72": (2, 20, 20, 72, 96, 1, 1),
    "K72n": (2, 20, 20, 72, 64, 1, 1),     # K72 for tile 33, whose launcher takes NB x KJ <= 18 (Cout <= 64 here)
}
RMS_FACTOR = 4.0         # stage-sum kernels (and the stream tiles): rms(e) <= 4 rms(e_ref)
RMS_FACTOR_CHAIN = 8.0   # the plain fmaf chain of tiles 3 and 4
BIAS_FACTOR = 0.1        # |mean(e)| <= 0.1 rms(e_ref), every tile but 3 and 4


@functools.lru_cache(maxsize=None)
def budget_case(name, se=False):
    """dict: x [B, H, W, Cin], w [Cout, Cin, k, k], b [Cout], sc [B, Cin] or None (float32), ref
    (float64 NHWC conv), scale = |ref|max, e_ref = float32 CPU conv - ref."""
    shape = BUDGET_SHAPES[name]
    B, H, W, Cin, Cout, k, s = shape
    g = torch.Generator().manual_seed(_seed(name, 3))
    x = torch.relu(torch.randn(B, H, W, Cin, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    sc = torch.rand(B, Cin, generator=g) if se else None
    xin = x * sc[:, None, None, :] if se else x      # the scale applied in float32 first
    ref = conv64(xin, w, shape, b)
    # the yardstick is torch's conv of a contiguous NCHW tensor, as the probe and every parity test
    # here run it: handed the NHWC view instead, torch takes its channels-last path, whose RMS error
    # at K = 2,304 is 3.6 times larger (1.3e-7 against 3.6e-8) and would loosen the budget by as much
    cpu = F.conv2d(xin.permute(0, 3, 1, 2).contiguous(), w, b, s, dims(shape)[0]).permute(0, 2, 3, 1).double()
    return dict(x=x, w=w, b=b, sc=sc, xin=xin, ref=ref, scale=ref.abs().max().item(), e_ref=cpu - ref)


def rms(e):
    return e.double().pow(2).mean().sqrt().item()


def ratios(y, case):
    """(rms(e) / rms(e_ref), mean(e) / rms(e_ref)) of a result y [B, Ho, Wo, Cout]; the common
    normalisation by |ref|max cancels."""
    e = y.double() - case["ref"]
    r = rms(case["e_ref"])
    return rms(e) / r, e.mean().item() / r


# ------------------------------------------------------------------------------------- emulation
def planes64(a):
    """The three bf16 planes of a float32 tensor as float64 [3, *a.shape] (plan.split_bf16x3; its
    negation of the odd 32-wide blocks undone: the RN split is odd, split(-v) = -split(v))."""
    flat = a.reshape(-1).numpy()
    n = flat.size
    buf = np.zeros((n + 31) // 32 * 32, dtype=np.float32)
    buf[:n] = flat
    bits = split_bf16x3(buf.reshape(1, -1)).astype(np.uint32) << 16
    sign = np.where((np.arange(buf.size) // 32) % 2 == 1, -1.0, 1.0)
    pl = bits.view(np.float32).reshape(3, -1).astype(np.float64) * sign
    return torch.from_numpy(pl[:, :n].copy()).reshape((3,) + tuple(a.shape))


HI, MID, LO = 0, 1, 2
KEPT = ((HI, HI), (HI, MID), (MID, HI), (HI, LO), (LO, HI), (MID, MID))   # (activation plane, weight plane)
SMALLEST_KEPT = {"hi.lo": (HI, LO), "lo.hi": (LO, HI), "mid.mid": (MID, MID)}


def emulate_x6(x, w, shape, bias=None, drop=None):
    """The bf16x6 conv in float64 with exact sums: the kept plane products, without `drop`."""
    xp, wp = planes64(x), planes64(w)
    y = 0
    for i in (HI, MID, LO):   # the conv is bilinear and plane sums are exact in float64: one conv per x plane
        js = [j for (a, j) in KEPT if a == i and (a, j) != drop]
        if js:
            y = y + conv64(xp[i], sum(wp[j] for j in js), shape)
    return y if bias is None else y + bias.double()


# ------------------------------------------------------------------------------------- tiles
LDS_TILES = [1, 2, 3, 4, 5, 6]                     # fp32 MFMA through LDS; 3 and 4 keep the plain fmaf chain
PW_TILES = [10, 11, 12, 13, 14, 15, 16, 17]        # direct pointwise fp32 MFMA; 13, 14, 16, 17 split K
X6_TILES = [21, 22, 23, 24, 27, 28]                # bf16x6, 16-deep stages
X6B_TILES = [25, 26, 29, 30, 31, 32, 38, 39]       # bf16x6, 32-deep stages; 26 splits K into a zeroed y
STREAM_TILES = [33, 34, 35]                        # streaming pointwise fp32 MFMA
AUTO = ["0", "0w"]                                 # the automatic choice without / with the split weight planes
CHAIN_TILES = (3, 4)

# budget shape -> tiles (tile 33 takes NB x KJ <= 18 column-block x K-chunk products: K72n, not K72)
BUDGET_TILES = {
    "K2304": LDS_TILES + X6_TILES + X6B_TILES + AUTO,
    "K1024": LDS_TILES + PW_TILES + X6_TILES + X6B_TILES + AUTO,
    "K360": LDS_TILES + X6_TILES + X6B_TILES,
    "K72": [34, 35] + PW_TILES + X6B_TILES,
    "K72n": [33],
}
# one SE in_scale variant per family on K1024, tile 25 with the input split up front (alone and under the scale)
BUDGET_SE_TILES = [3, 5, 10, 14, 16, 23, 25, 31, 39]
BUDGET_VARIANTS = ([("K1024", t, True, False) for t in BUDGET_SE_TILES] +
                   [("K1024", 25, False, True), ("K1024", 25, True, True)])
BUDGET_RUNS = [(n, t, False, False) for n, ts in BUDGET_TILES.items() for t in ts] + BUDGET_VARIANTS


def tile_of(t):
    """(tile number, with split weight planes) of a tile id or "0" / "0w"."""
    if isinstance(t, str):
        return 0, t.endswith("w")
    return t, t in X6_TILES or t in X6B_TILES


def budget_factors(tile):
    """(RMS factor, bias factor or None) of a tile."""
    if tile in CHAIN_TILES:
        return RMS_FACTOR_CHAIN, None
    return RMS_FACTOR, BIAS_FACTOR


@functools.lru_cache(maxsize=64)   # keyed by the (cached) host tensor's identity
def _device_weights(w):
    from edgeml_amd import ops
    from edgeml_amd.plan import pack_conv_weight
    wp = torch.from_numpy(pack_conv_weight(w.numpy())[0]).to("cuda")
    return wp, ops.split_bf16x3(wp)


def gpu_conv(x, w, shape, tile, bias=None, sc=None, presplit=False):
    """ops.conv2d_nhwc of host x [B, H, W, Cin] and w [Cout, Cin, k, k] on `tile` (no activation, no
    residual; bias zero when None) -> host [B, Ho, Wo, Cout]."""
    from edgeml_amd import ops
    B, H, W, Cin, Cout, k, s = shape
    tnum, x6 = tile_of(tile)
    wp, w3 = _device_weights(w)
    b = torch.zeros(Cout) if bias is None else bias
    y = ops.conv2d_nhwc(x.to("cuda"), wp, b.to("cuda"), Cout, k, s, dims(shape)[0], None, None, tile=tnum,
                        in_scale=None if sc is None else sc.to("cuda"), w3=w3 if x6 else None, presplit=presplit)
    return y.cpu()
