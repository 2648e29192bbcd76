"""One-record runs of the small kernels against a plain reference of the same operation.

MAXPOOL, CHANNEL_MEAN, SSD_SCORES, BOX_SCORES and ROI_ALIGN in mode 1 (multi-level: LevelMapper,
counts / RMAX padding) were only reached through whole-model runs.  Each test builds one plan record,
runs it on outputs filled with a canary bit pattern (with slack on both sides: nothing outside the
output may change) and compares with a float64 / ATen / torchvision-restatement reference.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0x7FC5A5A5  # a quiet NaN with a payload, compared as int32
SLACK = 64           # floats on either side of an output


class _Out:
    """An output of n floats inside a canary-filled parent with SLACK floats on both sides."""

    def __init__(self, n):
        self.n = n
        self.par = torch.full((n + 2 * SLACK,), CANARY, dtype=torch.int32, device=DEV)

    def ptr(self):
        return self.par.data_ptr() + 4 * SLACK

    def get(self, *shape):
        """The output's values on the host; the slack must still hold the canary."""
        h = self.par.cpu()
        assert bool((h[:SLACK] == CANARY).all()) and bool((h[SLACK + self.n:] == CANARY).all()), \
            "written outside the output"
        return h[SLACK:SLACK + self.n].reshape(shape)


def _run(kind, ints, ptrs, flts=()):
    from edgeml_amd import ops
    rec = np.zeros(1, dtype=ops.OP_DTYPE)
    rec[0]["kind"] = kind
    for j, v in ints.items() if isinstance(ints, dict) else enumerate(ints):
        rec[0]["i"][j] = v
    for j, t in enumerate(ptrs):
        rec[0]["p"][j] = 0 if t is None else (t.ptr() if isinstance(t, _Out) else t.data_ptr())
    for j, v in enumerate(flts):
        rec[0]["f"][j] = v
    ops.check(ops.lib().edgedet_plan_run(rec.ctypes.data_as(ctypes.c_void_p), 1, ops.stream_handle()))
    torch.cuda.synchronize()


def _f32(out_i32):
    return out_i32.contiguous().view(torch.float32)


# ------------------------------------------------------------------------------------- MAXPOOL
@pytest.mark.parametrize("B,H,W,C,K,s,p", [(2, 17, 13, 8, 3, 2, 1), (1, 40, 36, 64, 3, 2, 1), (1, 5, 5, 4, 2, 2, 0),
                                           (3, 1, 1, 4, 3, 2, 1)])
def test_maxpool_matches_torch(B, H, W, C, K, s, p):
    """MAXPOOL against F.max_pool2d: the NaN mask equal, the values bit-equal elsewhere.  Every input
    is negative (padding must not act as 0), with a few -inf and NaN inside windows and on the border."""
    from edgeml_amd import ops
    g = torch.Generator().manual_seed(H * W + C)
    x = -(torch.rand(B, H, W, C, generator=g) * 10 + 0.25)
    ninf, nan = float("-inf"), float("nan")
    x[0, 0, 0, 0] = nan                      # border (a corner)
    x[B - 1, H - 1, W - 1, C - 1] = ninf     # border (the opposite corner)
    if H > 4:
        x[0, H // 2, W // 2, 1] = nan        # inside
        x[0, 2, 3, 2] = ninf
        x[0, 1:4, 0:3, 3] = ninf             # a whole window of -inf at the left edge
        x[B - 1, H - 1, 1, 0] = nan          # last row
        x[B - 1, 3, W - 1, 2] = nan          # last column
    elif B > 1:
        x[1, 0, 0, 1] = ninf
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), K, s, p).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1], ref.shape[2]
    assert (Ho, Wo) == ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)
    y = _Out(B * Ho * Wo * C)
    _run(ops.MAXPOOL, [B, H, W, C, Ho, Wo, K, s, p], [x.to(DEV), y])
    got = _f32(y.get(B, Ho, Wo, C))
    assert torch.isnan(ref).any() and torch.isinf(ref).any() and bool((ref[~torch.isnan(ref)] < 0).all())
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert torch.equal(got[ok], ref[ok]), (got[ok] - ref[ok]).abs().max().item()


# ------------------------------------------------------------------------------------- CHANNEL_MEAN
@pytest.mark.parametrize("HW", [1, 3, 37, 400])
@pytest.mark.parametrize("C", [4, 72, 130])
def test_channel_mean_matches_float64(C, HW):
    """CHANNEL_MEAN (no lowering emits it any more; reachable through the record ABI) against a
    float64 mean.  The kernel adds four fixed-order fp32 partial sums of at most ceil(HW / 4) terms,
    three adds across them and one division: per channel at most (HW / 4 + 4) roundings of relative
    size 2^-24 on sums bounded by sum|x|, i.e. (HW / 4 + 4) * 2^-24 * mean|x|."""
    from edgeml_amd import ops
    B = 3
    g = torch.Generator().manual_seed(C * 1000 + HW)
    x = torch.randn(B, HW, C, generator=g) * 3 + 0.5
    ref = x.double().mean(1)
    bound = (HW / 4 + 4) * 2.0 ** -24 * x.double().abs().mean(1)
    out = _Out(B * C)
    _run(ops.CHANNEL_MEAN, [B, HW, C], [x.to(DEV), out])
    got = _f32(out.get(B, C)).double()
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (err / bound).max().item()


# ------------------------------------------------------------------------------------- softmax + decode
def _softmax_case(logits):
    """float64 softmax over the last axis, and e32: the error of torch's own fp32 CPU softmax."""
    ref = torch.softmax(logits.double(), -1)
    e32 = (torch.softmax(logits, -1).double() - ref).abs().max().item()
    return ref, e32


def _check_scores(got, ref, e32, what):
    """Allowance 4 * e32 + 2^-23: the device expf and the kernel's sum order differ from ATen's."""
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: engine error {err:.3e}, e32 {e32:.3e}, allowance {4 * e32 + 2.0 ** -23:.3e}")
    assert err <= 4 * e32 + 2.0 ** -23, (err, e32)


def _decode_ref(deltas, boxes, size):
    from oracle import tv_ops
    return tv_ops.clip_boxes(tv_ops.decode_boxes(deltas, boxes, (10.0, 10.0, 5.0, 5.0)), size)


def _boxes(rs, n, size):
    xy = rs.uniform(-10, size, (n, 2)).astype(np.float32)
    wh = rs.uniform(1, size / 2, (n, 2)).astype(np.float32)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


@pytest.mark.parametrize("NC", [91, 21, 92, 2])
@pytest.mark.parametrize("A", [1, 64, 101])
def test_ssd_scores_matches_reference(A, NC):
    """SSD_SCORES: softmax over the classes written class-major [B][NC][A] (odd LDS pitch NC = 91, 21;
    even NC = 92, 2, staged with a pitch of NC + 1), and BoxCoder decode (weights 10, 10, 5, 5) + clip.
    Scores against float64 softmax within 4 * e32 + 2^-23, e32 being torch's fp32 CPU softmax error on
    the same logits (4.4e-8 on a 2 x 91 x 37 sample).  Measured on MI355X over these twelve cases (the
    test prints both figures): the engine's error is largest at A = 64, NC = 91, 2.80e-7 beside an e32
    of 8.97e-8 (allowance 4.78e-7), and 2.33e-7 / 1.12e-7 at A = 101, NC = 91; at A = 1 and at NC = 2
    it equals e32 (at most 7.4e-8).
    One row has all logits equal and one is spread over +-80.  Boxes within rtol 3e-7 / atol 1e-4 of
    the oracle (the device expf may differ by an ulp), deltas beyond the log(1000 / 16) clamp included."""
    from edgeml_amd import ops
    B, img = 2, (320.0, 300.0)
    rs = np.random.RandomState(A * 131 + NC)
    logits = torch.from_numpy((rs.randn(B, A, NC) * 3).astype(np.float32))
    logits[0, 0, :] = 1.5
    logits[1, A - 1, :] = torch.linspace(-80, 80, NC)
    reg = (rs.randn(B, A, 4) * 2).astype(np.float32)
    reg[:, : max(1, A // 8), 2:] = 30.0  # beyond the clamp
    anchors = _boxes(rs, A, 320.0)
    ref_s, e32 = _softmax_case(logits)
    ref_b = _decode_ref(reg.reshape(B * A, 4), np.tile(anchors, (B, 1)), img)[:, 0].reshape(B, A, 4)
    scores, boxes = _Out(B * NC * A), _Out(B * A * 4)
    _run(ops.SSD_SCORES, [B, A, NC], [logits.to(DEV), torch.from_numpy(reg).to(DEV), torch.from_numpy(anchors).to(DEV),
                                      scores, boxes], img)
    got_s = _f32(scores.get(B, NC, A)).permute(0, 2, 1)
    got_b = _f32(boxes.get(B, A, 4))
    _check_scores(got_s, ref_s, e32, f"SSD_SCORES A={A} NC={NC}")
    torch.testing.assert_close(got_b, ref_b, rtol=3e-7, atol=1e-4)


@pytest.mark.parametrize("NC,LD,cls_off,delta_off", [(91, 456, 364, 0), (5, 28, 0, 8), (128, 640, 512, 0)],
                         ids=["product", "small", "nc128"])
def test_box_scores_matches_reference(NC, LD, cls_off, delta_off):
    """BOX_SCORES on predictor rows [B * R][LD] (class logits at cls_off, class deltas at delta_off):
    the product layout, a small one with the logits first, and NC = 128, the template bound.  Same
    references and bounds as SSD_SCORES; measured on MI355X (engine error beside e32): 9.84e-8 / 1.22e-7
    for the product layout, 4.53e-8 / 1.25e-7 for the small one, 6.46e-8 / 1.62e-7 for NC = 128.  Rows at or beyond counts[b] keep the canary: the
    kernel returns before it writes them."""
    from edgeml_amd import ops
    B, R, counts, img = 3, 9, [9, 3, 0], (800.0, 1088.0)
    rs = np.random.RandomState(NC)
    pred = np.full((B * R, LD), np.nan, np.float32)
    logits = torch.from_numpy((rs.randn(B * R, NC) * 3).astype(np.float32))
    logits[0, :] = -2.25
    logits[1, :] = torch.linspace(-80, 80, NC)
    logits[R + 2, :] = torch.linspace(80, -80, NC)
    deltas = (rs.randn(B * R, 4 * NC) * 2).astype(np.float32)
    deltas[:, 2:8] = 30.0  # beyond the clamp (dw, dh of class 0; dx, dy, dw, dh of class 1)
    pred[:, cls_off:cls_off + NC] = logits.numpy()
    pred[:, delta_off:delta_off + 4 * NC] = deltas
    props = _boxes(rs, B * R, 800.0)
    ref_s, e32 = _softmax_case(logits)
    ref_b = _decode_ref(deltas, props, img)
    scores, boxes = _Out(B * R * NC), _Out(B * R * NC * 4)
    _run(ops.BOX_SCORES, [LD, B, R, NC, cls_off, delta_off],
         [torch.from_numpy(pred).to(DEV), torch.from_numpy(props).to(DEV),
          torch.tensor(counts, dtype=torch.int32, device=DEV), scores, boxes], img)
    got_s, got_b = scores.get(B, R, NC), boxes.get(B, R, NC, 4)
    valid = torch.tensor([[r < counts[b] for r in range(R)] for b in range(B)])
    assert bool((got_s[~valid] == CANARY).all()) and bool((got_b[~valid] == CANARY).all())
    ref_s, ref_b = ref_s.reshape(B, R, NC), ref_b.reshape(B, R, NC, 4)
    _check_scores(_f32(got_s[valid]), ref_s[valid], e32, f"BOX_SCORES NC={NC}")
    torch.testing.assert_close(_f32(got_b[valid]), ref_b[valid], rtol=3e-7, atol=1e-4)


# ------------------------------------------------------------------------------------- ROI_ALIGN mode 1
@pytest.mark.parametrize("place", ["spread", "inside"])
@pytest.mark.parametrize("C", [4, 8])
def test_roi_align_multilevel_matches_oracle(C, place):
    """ROI_ALIGN in mode 1 (boxes [B][RMAX][4] with per-image counts, LevelMapper over four levels)
    against the oracle's multiscale_roi_align: bit-identical for valid slots, exactly zero for padded
    ones.  The 96 boxes spread over the levels as 50 / 24 / 14 / 8, and none sits within 1e-3 of a
    LevelMapper boundary (the nearest is 2.1e-3 away), where the device log2f could decide otherwise.
    "spread" draws the origins over [-20, 500] x [-20, 400], well past the 152 x 200 image of these
    levels, so most of its small boxes sample nothing but zeros (11 of the 65 valid RoIs are not all
    zero); "inside" keeps the same sides and moves the origins onto the image."""
    from edgeml_amd import ops
    from oracle import tv_ops
    B, RMAX, counts, k_min, k_max, sr = 2, 48, [48, 17], 2, 5, 2
    sizes, scales = [(50, 38), (25, 19), (13, 10), (7, 5)], [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    rs = np.random.RandomState(6)
    n = B * RMAX
    side = np.exp(rs.uniform(math.log(8), math.log(700), n))
    asp = np.exp(rs.uniform(-0.7, 0.7, n))
    x0, y0 = rs.uniform(-20, 500, n), rs.uniform(-20, 400, n)
    if place == "inside":
        x0, y0 = (x0 + 20) * (150 / 520) - 20, (y0 + 20) * (200 / 420) - 20
    bx = np.stack([x0, y0, x0 + side * np.sqrt(asp), y0 + side / np.sqrt(asp)], 1).astype(np.float32)
    t = 4 + np.log2(np.sqrt((bx[:, 2] - bx[:, 0]).astype(np.float64) * (bx[:, 3] - bx[:, 1])) / 224)
    assert np.abs(t - np.round(t)).min() >= 1e-3
    boxes = torch.from_numpy(bx)
    assert np.bincount(tv_ops.level_mapper(boxes, k_min, k_max).numpy(), minlength=4).tolist() == [50, 24, 14, 8]
    feats = [torch.from_numpy(rs.randn(B, C, h, w).astype(np.float32)) for h, w in sizes]
    per_image = [boxes[b * RMAX:b * RMAX + counts[b]] for b in range(B)]
    ref = tv_ops.multiscale_roi_align(feats, per_image, scales)  # [sum(counts), C, 7, 7]
    out = _Out(n * 7 * 7 * C)
    ints = {0: 1, 1: n, 2: RMAX, 3: B, 4: C, 5: 7, 6: 7, 7: sr, 8: 4, 9: k_min, 10: k_max}
    for l, (h, w) in enumerate(sizes):
        ints[11 + l], ints[15 + l] = h, w
    dev_feats = [f.permute(0, 2, 3, 1).contiguous().to(DEV) for f in feats]
    _run(ops.ROI_ALIGN, ints, dev_feats + [boxes.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), out],
         scales)
    got = out.get(B, RMAX, 7, 7, C)
    off = 0
    for b in range(B):
        g = _f32(got[b, :counts[b]]).permute(0, 3, 1, 2)
        want = ref[off:off + counts[b]]
        assert torch.equal(g, want), (b, (g - want).abs().max().item())
        assert bool((got[b, counts[b]:] == 0).all())
        off += counts[b]
    # the comparison is not over empty samples
    assert int((ref.abs().amax((1, 2, 3)) > 0).sum()) >= (60 if place == "inside" else 11)
