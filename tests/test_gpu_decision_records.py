"""Exact record-level parity of the RPN, RoI and RetinaNet decision kernels (csrc/detect.hip) with the
plain references of tests/decision_refs.py: MERGE_TOPK alone, BOX_CLASS_NMS + MERGE_TOPK,
RPN_LEVEL_NMS + MERGE_TOPK (single pass and chunked) and RETINA_SELECT + RETINA_CLASS_NMS + MERGE_TOPK.

Plans of one to three records run through edgedet_plan_run, built by slot number (csrc/records.hpp).
Every buffer a kernel writes sits in a canary-filled parent with slack on both sides, which must survive;
only rows below the written count are compared, and every comparison is assert_array_equal on count,
labels, boxes and scores.  The one exception: RPN / RetinaNet scores, where both sides evaluate a sigmoid,
use the recompute tolerance of tests/parity_models.py (rtol 2e-6); row identity and order stay exact.

Inputs that make exactness legitimate (asserted on the host where noted):

* Decode is exact in float32 under any evaluation order: dw = dh = 0 and dx, dy multiples of 1/8 in
  [-2, 2] on anchors with integer corners (asserted, with the float64 value of every decoded corner), so
  every product and sum is exact.  The over-clamp pattern has dw = dh = 10, above the log(1000 / 16)
  clamp: after the clip every such box is the image rectangle (asserted on the reference side), exact
  again, with IoU 1 everywhere.
* Logits come from two sets.  "Separated": multiples of 0.5 in [-6, 6]; neighbouring sigmoids differ by
  >= 1e-3 (asserted), so equal score means equal logit on both sides.  "Saturated": multiples of 0.5 in
  [20, 30], where exp(-x) < 3e-9, far below half an ulp of 1: both sides give exactly 1.0f.  No decision
  hangs on a last-bit sigmoid difference; -3.0 and -2.5 straddle RetinaNet's 0.05 threshold widely.
* The RoI tail gets class probabilities and boxes directly (no softmax / decode in the kernels under
  test): scores quantised to 1/64, box corners as stated per pattern.
* MERGE_TOPK's tiebreaks are unique per image (asserted), as every producer writes them.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import decision_refs as DR
from tests.test_gpu_small_ops import _Out, _f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCORE_RTOL = 2e-6  # recomputed sigmoid scores (tests/parity_models.py)


# ------------------------------------------------------------------------------------- plumbing
_KEEP = []  # device inputs of the running test: a record holds only their addresses


def _dev(a):
    _KEEP.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _KEEP.clear()


def _rec(kind, ints, ptrs, flts=(), dbls=()):
    from edgeml_amd import ops
    r = np.zeros(1, dtype=ops.OP_DTYPE)
    r[0]["kind"] = kind
    for j, v in ints.items() if isinstance(ints, dict) else enumerate(ints):
        r[0]["i"][j] = v
    for j, t in ptrs.items():
        r[0]["p"][j] = 0 if t is None else (t.ptr() if isinstance(t, _Out) else t.data_ptr())
    for j, v in enumerate(flts):
        r[0]["f"][j] = v
    for j, v in enumerate(dbls):
        r[0]["d"][j] = v
    return r


def _run(*recs):
    from edgeml_amd import ops
    arr = np.concatenate(recs)
    ops.check(ops.lib().edgedet_plan_run(arr.ctypes.data_as(ctypes.c_void_p), len(arr), ops.stream_handle()))
    torch.cuda.synchronize()


class _List:
    """A record list [B][S][kmax] (rec::seg order: box, score, tb, label, count), every array in a
    canary-filled parent."""

    def __init__(self, B, S, kmax):
        n = B * S * kmax
        self.shape = (B, S)
        self.bufs = [_Out(4 * n), _Out(n), _Out(n), _Out(n), _Out(B * S)]

    def ptrs(self, base):
        return {base + j: b for j, b in enumerate(self.bufs)}

    def check(self, kmax_le=None):
        """The slack of all five arrays holds the canary; returns the counts [B][S]."""
        for b in self.bufs:
            b.get(b.n)
        cnt = self.bufs[4].get(*self.shape).numpy()
        assert (cnt >= 0).all() and (kmax_le is None or (cnt <= kmax_le).all()), cnt
        return cnt


class _Dets:
    """MERGE_TOPK's outputs [B][N]: boxes, scores, optional int64 labels, counts."""

    def __init__(self, B, N, labels=True):
        self.B, self.N = B, N
        self.box, self.score, self.count = _Out(B * N * 4), _Out(B * N), _Out(B)
        self.label = _Out(2 * B * N) if labels else None

    def ptrs(self, base):
        return {base: self.box, base + 1: self.score, base + 2: self.label, base + 3: self.count}

    def read(self):
        B, N = self.B, self.N
        cnt = self.count.get(B).numpy()
        assert ((cnt >= 0) & (cnt <= N)).all(), cnt
        box = _f32(self.box.get(B, N, 4)).numpy()
        score = _f32(self.score.get(B, N)).numpy()
        lab = None
        if self.label is not None:
            lab = self.label.get(B, N, 2).contiguous().view(torch.int64).reshape(B, N).numpy()
        return [(box[b, :n], score[b, :n], None if lab is None else lab[b, :n]) for b, n in enumerate(cnt)]


def _compare(got, ref, what, score_rtol=None):
    assert len(got) == len(ref)
    for b, ((gb, gs, gl), r) in enumerate(zip(got, ref)):
        rb, rs = np.asarray(r[0]).reshape(-1, 4), np.asarray(r[1])
        print(f"{what} image {b}: count {gs.shape[0]}, reference {rs.shape[0]}")
        assert gs.shape[0] == rs.shape[0], (what, b, gs.shape[0], rs.shape[0])
        if gl is not None:
            np.testing.assert_array_equal(gl, np.asarray(r[2]), err_msg=f"{what} labels image {b}")
        np.testing.assert_array_equal(gb, rb, err_msg=f"{what} boxes image {b}")
        if score_rtol is None:
            np.testing.assert_array_equal(gs, rs, err_msg=f"{what} scores image {b}")
        else:
            np.testing.assert_allclose(gs, rs, rtol=score_rtol, atol=0, err_msg=f"{what} scores image {b}")


RATIO = np.asarray([[1.5, 0.75], [2.0, 3.25], [0.625, 1.0], [1.0, 1.125]], np.float32)


# ------------------------------------------------------------------------------------- MERGE_TOPK alone
def _tb(B, S, kmax, order):
    s, j = np.meshgrid(np.arange(S), np.arange(kmax), indexing="ij")
    if order == "segment":      # the order of the candidate index
        t = s * kmax + j
    elif order == "reversed":   # segment order reversed
        t = (S - 1 - s) * kmax + j
    elif order == "roi_class":  # BOX_CLASS_NMS: roi << 8 | class
        assert S < 255
        t = (j << 8) | (s + 1)
    else:                       # slot-major
        t = j * S + s
    return np.broadcast_to(t, (B, S, kmax)).astype(np.int64).copy()


def _merge(score, tb, count, N, ratio=None, labels=True):
    """One MERGE_TOPK record on hand-built lists, compared with ref_merge.  Slots at and beyond the valid
    prefix get a score above every valid one: they must be ignored.  The box of candidate f = (b, s, j)
    flattened is (f, f + 0.25, f + 1, f + 2.5), so a row's first coordinate names its candidate."""
    from edgeml_amd import ops
    score = np.asarray(score, np.float32).copy()
    count = np.asarray(count, np.int64)
    B, S, kmax = score.shape
    for b in range(B):
        assert np.unique(tb[b]).size == S * kmax, "tiebreaks must be unique per image"
        for s in range(S):
            score[b, s, min(int(count[b, s]), kmax):] = 2.0
    f = np.arange(B * S * kmax, dtype=np.float32).reshape(B, S, kmax)
    box = np.stack([f, f + 0.25, f + 1, f + 2.5], -1).astype(np.float32)
    label = (np.arange(B * S * kmax).reshape(B, S, kmax) * 7 % 1009).astype(np.int32)
    if ratio is not None:
        ratio = np.resize(ratio, (B, 2)).astype(np.float32)
    dets = _Dets(B, N, labels)
    ins = [_dev(box), _dev(score), _dev(tb.astype(np.uint32).view(np.int32)), _dev(label), _dev(count.astype(np.int32))]
    ptrs = dict(enumerate(ins))
    ptrs[5] = None if ratio is None else _dev(ratio)
    ptrs.update(dets.ptrs(6))
    _run(_rec(ops.MERGE_TOPK, [B, S, kmax, N], ptrs))
    got = dets.read()
    _compare(got, DR.ref_merge(box, score, tb, label, count, kmax, N, ratio), "merge")
    return got


def _quantised(rs, shape, levels):
    return (rs.randint(1, levels, shape) / levels).astype(np.float32)


def test_merge_counts_zero_and_clamped():
    """All counts 0 (nothing written but the counts); counts above kmax clamp to kmax."""
    rs = np.random.RandomState(0)
    got = _merge(_quantised(rs, (2, 3, 8), 16), _tb(2, 3, 8, "segment"), np.zeros((2, 3)), 5, RATIO)
    assert all(g[1].size == 0 for g in got)
    got = _merge(_quantised(rs, (2, 4, 16), 16), _tb(2, 4, 16, "reversed"), [[20, 16, 3, 0], [1000000, 0, 17, 5]], 40)
    assert [g[1].size for g in got] == [35, 37]


@pytest.mark.parametrize("S,kmax,N", [(1, 50, 10), (1023, 4, 300)])
def test_merge_one_and_1023_segments(S, kmax, N):
    rs = np.random.RandomState(S)
    count = rs.randint(0, kmax + 3, (2, S))
    count[0, 0] = kmax
    _merge(_quantised(rs, (2, S, kmax), 32), _tb(2, S, kmax, "slot"), count, N, RATIO, labels=S == 1)


def test_merge_8192_and_8193_candidates():
    """Image 0 has 8,192 candidates (the last size of the register path), image 1 has 8,193 (the first
    of the radix path); a few thousand distinct scores, so ties sit at the cut."""
    rs = np.random.RandomState(2)
    S, kmax = 8, 1025
    count = np.asarray([[1024] * 8, [1024] * 7 + [1025]])
    _merge(_quantised(rs, (2, S, kmax), 4096), _tb(2, S, kmax, "reversed"), count, 300)


@pytest.mark.parametrize("N,kmax", [(1, 400), (1024, 400), (1024, 100)])
def test_merge_shortest_and_longest_output(N, kmax):
    """N = 1 with the maximum held three times (the smallest tiebreak wins), N = 1024 out of about 1,750
    candidates, and N = 1024 with fewer candidates than N (all taken)."""
    rs = np.random.RandomState(N + kmax)
    S = 5
    score = _quantised(rs, (2, S, kmax), 4096) * 0.5
    score[:, 1, 7] = score[:, 3, 2] = score[:, 4, 250 % kmax] = 0.75
    count = rs.randint(kmax * 3 // 4, kmax + 1, (2, S))
    got = _merge(score, _tb(2, S, kmax, "reversed"), count, N, RATIO if N == 1 else None, labels=N != 1)
    assert all(g[1].size == min(N, int(c.sum())) for g, c in zip(got, count))


def test_merge_ties_under_capacity_against_segment_order():
    """600 candidates of two score values, tiebreaks in the opposite order to the segments."""
    rs = np.random.RandomState(5)
    score = np.where(rs.rand(2, 6, 100) < 0.1, 0.5, 0.25).astype(np.float32)
    _merge(score, _tb(2, 6, 100, "reversed"), np.full((2, 6), 100), 100, RATIO, labels=False)


def test_merge_ties_over_capacity_register_path():
    """S = 4, kmax = 340, every score 0.2, tiebreak = slot << 8 | (segment + 1), N = 100: 1,360 exact ties
    for a 1,024-entry list.  The 100 rows are slots 0..24 of segments 0..3, slot-major.  Image 1 adds 50
    distinct higher scores in the last segment, which come first.  (Before the merge chose over-capacity
    ties by tiebreak, 81 of image 0's 100 rows were wrong: segment 3 was cut off at slot 3.)"""
    S, kmax, N = 4, 340, 100
    score = np.full((2, S, kmax), 0.2, np.float32)
    score[1, 3, :50] = 0.9 - np.arange(50, dtype=np.float32) / 128
    got = _merge(score, _tb(2, S, kmax, "roi_class"), np.full((2, S), kmax), N)
    want = np.asarray([s * kmax + j for j in range(25) for s in range(S)], np.float32)
    np.testing.assert_array_equal(got[0][0][:, 0], want)
    np.testing.assert_array_equal(got[1][0][:50, 0], S * kmax + 3 * kmax + np.arange(50, dtype=np.float32))


def test_merge_ties_over_capacity_radix_path():
    """S = 20, kmax = 500 (10,000 candidates): segments 0..17 all 0.25, segment 18 lower, segment 19
    starts with 200 distinct higher scores, N = 300.  The higher keys must all come first, then the 100
    ties with the smallest tiebreaks.  Image 1: every score 0.25.  (Before the fix the ties of the first
    compaction batches filled the list and none of the 200 higher scores was returned: 299 of 300 rows
    wrong.)"""
    S, kmax, N = 20, 500, 300
    score = np.full((2, S, kmax), 0.25, np.float32)
    score[0, 18] = 0.125 - np.arange(kmax, dtype=np.float32) / 8192
    score[0, 19, :200] = 0.95 - np.arange(200, dtype=np.float32) / 512
    score[0, 19, 200:] = 0.0625
    got = _merge(score, _tb(2, S, kmax, "roi_class"), np.full((2, S), kmax), N, RATIO)
    np.testing.assert_array_equal(got[0][1][:200], score[0, 19, :200])
    assert (got[0][1][200:] == 0.25).all() and (got[1][1] == 0.25).all()


# ------------------------------------------------------------------------------------- BOX_CLASS_NMS + MERGE_TOPK
BOX_THR, BOX_MIN, BOX_IOU, BOX_N = 0.05, 1e-2, 0.5, 100  # as the lowering sets them (oracle/frcnn.py)


def _box_tail(scores, boxes, counts, what):
    from edgeml_amd import ops
    B, R, NC = scores.shape
    ratio = np.resize(RATIO, (B, 2)).astype(np.float32)
    lst, dets = _List(B, NC - 1, R), _Dets(B, BOX_N)
    _run(_rec(ops.BOX_CLASS_NMS, [B, R, NC, R],
              {0: _dev(scores), 1: _dev(boxes), 2: _dev(np.asarray(counts, np.int32)), **lst.ptrs(3)},
              flts=[BOX_THR, BOX_MIN], dbls=[BOX_IOU]),
         _rec(ops.MERGE_TOPK, [B, NC - 1, R, BOX_N], {**lst.ptrs(0), 5: _dev(ratio), **dets.ptrs(6)}))
    lst.check(kmax_le=R)
    got = dets.read()
    _compare(got, DR.ref_box_tail(scores, boxes, counts, BOX_THR, BOX_MIN, BOX_IOU, BOX_N, ratio), what)
    return got


@pytest.mark.parametrize("pattern", ["random", "clustered", "identical", "iou_boundary"])
@pytest.mark.parametrize("R,NC", [(1000, 91), (37, 21), (64, 2)])
def test_box_tail_matches_reference(R, NC, pattern):
    """Four images with 0, 1, R and about 2R/3 valid RoIs; rows at and beyond counts[b] hold score 1.0 and a
    valid box and must be ignored.  Scores are multiples of 1/64.  "random" adds scores of exactly
    float32(0.05) (rejected: the test is >), boxes whose width or height is exactly float32(0.01) (kept)
    or the next float below (dropped) and zero-area boxes with the top score (dropped before the NMS, so
    they suppress nothing).  "identical": one box per class survives.  "iou_boundary": small integer
    corners, so IoUs fall exactly on 1/2."""
    rs = np.random.RandomState(R + NC)
    B, counts = 4, [0, 1, R, max(2, 2 * R // 3)]
    scores = (np.floor(rs.rand(B, R, NC) ** 3 * 64) / 64).astype(np.float32)
    if pattern == "clustered":
        cen = rs.uniform(20, 180, (B, 6, 2))
        c = cen[np.arange(B)[:, None, None], rs.randint(0, 6, (B, R, NC))] + rs.normal(0, 3.0, (B, R, NC, 2))
        wh = rs.uniform(20, 60, (B, R, NC, 2))
        boxes = np.clip(np.concatenate([c - wh / 2, c + wh / 2], -1), 0, 256)
    elif pattern == "identical":
        boxes = np.tile(np.asarray([10, 20, 110, 90], np.float32), (B, R, NC, 1))
    elif pattern == "iou_boundary":
        xy = rs.randint(0, 12, (B, R, NC, 2))
        boxes = np.concatenate([xy, xy + rs.randint(1, 10, (B, R, NC, 2))], -1)
    else:
        xy = rs.uniform(0, 200, (B, R, NC, 2))
        boxes = np.clip(np.concatenate([xy, xy + rs.uniform(4, 80, (B, R, NC, 2))], -1), 0, 256)
    boxes = boxes.astype(np.float32)
    if pattern == "random":
        k = max(2, min(20, R // 10))
        lo = np.float32(0.01)
        below = np.nextafter(lo, np.float32(0))
        for b in (2, 3):
            cells = rs.permutation(counts[b] * (NC - 1))[:7 * k]
            rr, cc = cells // (NC - 1), cells % (NC - 1) + 1
            grp = [(rr[i * k:(i + 1) * k], cc[i * k:(i + 1) * k]) for i in range(7)]
            scores[b, grp[0][0], grp[0][1]] = np.float32(0.05)
            for g, (x2, y2) in zip(grp[1:5], [(lo, 30), (below, 30), (40, lo), (40, below)]):
                scores[b, g[0], g[1]] = 0.75
                boxes[b, g[0], g[1]] = np.asarray([0, 0, x2, y2], np.float32)
            scores[b, grp[5][0], grp[5][1]] = 63 / 64
            boxes[b, grp[5][0], grp[5][1], 2] = boxes[b, grp[5][0], grp[5][1], 0]  # zero width
            scores[b, grp[6][0], grp[6][1]] = 63 / 64
            boxes[b, grp[6][0], grp[6][1], 3] = boxes[b, grp[6][0], grp[6][1], 1]  # zero height
            v = boxes[b, :counts[b], 1:]
            w = v[..., 2] - v[..., 0]
            assert (scores[b, :counts[b], 1:] == np.float32(0.05)).sum() >= k
            assert (w == lo).sum() >= k and (w == below).sum() >= k and (w == 0).sum() >= k
    for b in range(B):  # padding rows: the top score on a valid box
        scores[b, counts[b]:] = 1.0
        boxes[b, counts[b]:] = np.asarray([1, 2, 50, 60], np.float32)
    got = _box_tail(scores, boxes, counts, f"box tail R={R} NC={NC} {pattern}")
    assert got[0][1].size == 0
    if pattern == "identical":
        for b in range(B):
            live = int(((scores[b, :counts[b], 1:] > np.float32(BOX_THR)).any(0)).sum())
            assert got[b][1].size == min(BOX_N, live), (b, got[b][1].size, live)


@pytest.mark.parametrize("R,NC", [(60, 5), (1000, 91)])
def test_box_tail_all_equal_scores_keep_roi_class_order(R, NC):
    """Every score equal on boxes that do not overlap within a class: nothing is suppressed and the 100
    rows are the first (roi, class) pairs in that order (R = 60, NC = 5: rois 0..24 x classes 1..4).
    R = 1000, NC = 91 is the same degenerate input at the product shape: 90,000 exact ties."""
    B = 2
    scores = np.full((B, R, NC), 0.5, np.float32)
    r, c = np.meshgrid(np.arange(R), np.arange(NC), indexing="ij")
    boxes = np.stack([3 * r, 2 * c, 3 * r + 2, 2 * c + 1.5], -1).astype(np.float32)
    boxes = np.broadcast_to(boxes, (B, R, NC, 4)).copy()
    got = _box_tail(scores, boxes, [R, R], f"box tail all-equal R={R} NC={NC}")
    pairs = [(i, k) for i in range(R) for k in range(1, NC)][:BOX_N]
    for b in range(B):
        np.testing.assert_array_equal(got[b][2], [k for _, k in pairs])
        np.testing.assert_array_equal(got[b][0][:, 0], np.asarray([3 * i for i, _ in pairs], np.float32) * RATIO[b, 0])


# ------------------------------------------------------------------------------------- head inputs (RPN, RetinaNet)
IMG_PAD, IMG = (128, 160), (120, 150)  # padded size (anchor grid) and image size (clip)


def _separated(rs, shape, lo=-12, hi=12):
    return (rs.randint(lo, hi + 1, shape) * 0.5).astype(np.float32)


def _saturated(rs, shape):
    return (20 + rs.randint(0, 21, shape) * 0.5).astype(np.float32)


def _exact_deltas(rs, anchors, overclamp=False, span=16, push_left=False):
    """[n, 4] deltas on anchors [n, 4]: dx, dy multiples of 1/8 in [-span / 8, span / 8] (at most [-2, 2]);
    dw = dh = 0, or 10 (beyond the clamp).  push_left: an anchor that reaches past the left border moves
    two widths further left, fully outside, so its clipped width is 0.  Asserts the float32 decode equal
    to its float64 value.  (tests/test_decision_refs.py asserts what the docstring says of the logit sets.)"""
    from oracle import tv_ops
    a = anchors.numpy()
    assert (a == np.round(a)).all(), "anchors must have integer corners"
    n = a.shape[0]
    d = np.zeros((n, 4), np.float32)
    d[:, :2] = rs.randint(-span, span + 1, (n, 2)) / 8
    if overclamp:
        d[:, 2:] = 10.0
        return d
    if push_left:
        d[a[:, 0] < 0, 0] = -2.0
    _assert_exact_decode(d, anchors)
    return d


def _assert_exact_decode(d, anchors):
    from oracle import tv_ops
    a = anchors.numpy()
    assert (d[:, 2:] == 0).all() and (d[:, :2] * 8 == np.round(d[:, :2] * 8)).all() and np.abs(d).max() <= 2
    a64, d64 = a.astype(np.float64), d.astype(np.float64)
    w, h = a64[:, 2] - a64[:, 0], a64[:, 3] - a64[:, 1]
    cx, cy = a64[:, 0] + 0.5 * w + d64[:, 0] * w, a64[:, 1] + 0.5 * h + d64[:, 1] * h
    exact = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], 1)
    got = tv_ops.decode_boxes(torch.from_numpy(d), anchors, (1.0, 1.0, 1.0, 1.0))[:, 0].numpy()
    assert (got.astype(np.float64) == exact).all(), "the decode must be exact in float32"
    return d


# ------------------------------------------------------------------------------------- RPN_LEVEL_NMS + MERGE_TOPK
RPN_GRIDS = [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)]  # x 3 anchors: 3840 / 960 / 240 / 60 / 18
RPN_TOPK, RPN_CHUNK = 1000, 1024


def _rpn_logits(rs, pattern, shape):
    if pattern == "separated":
        return _separated(rs, shape)
    if pattern == "all_equal":
        return np.full(shape, 0.5, np.float32)
    if pattern == "two_valued":  # a sparse high tie group that straddles the chunks
        return np.where(rs.rand(*shape) < 0.05, 1.0, -1.0).astype(np.float32)
    if pattern == "saturated":   # every score 1.0f: the merge order is (level, rank)
        return _saturated(rs, shape)
    return np.where(rs.rand(*shape) < 0.3, _saturated(rs, shape), _separated(rs, shape)).astype(np.float32)


@pytest.mark.parametrize("deltas", ["exact", "overclamp"])
@pytest.mark.parametrize("pattern", ["separated", "all_equal", "two_valued", "saturated", "mixed"])
def test_rpn_filter_matches_reference(pattern, deltas):
    """oracle.frcnn.rpn_filter on a 128 x 160 padded image (levels of 3840 / 960 / 240 / 60 / 18 anchors:
    P2 above the top-k of 1,000, the others below), B = 2, against the single-pass record and the chunked
    one (chunk = 1,024: P2 spans four chunks and its ties cross them)."""
    from edgeml_amd import ops
    from oracle import frcnn, tv_ops
    rs = np.random.RandomState(len(pattern) * 7 + len(deltas))
    B, L = 2, len(RPN_GRIDS)
    anchors = tv_ops.rpn_anchors(RPN_GRIDS, IMG_PAD)
    ns = [int(a.shape[0]) for a in anchors]
    assert ns == [3840, 960, 240, 60, 18]
    objs = [_rpn_logits(rs, pattern, (B, n)) for n in ns]
    dels = [np.stack([_exact_deltas(rs, a, deltas == "overclamp", push_left=True) for _ in range(B)]) for a in anchors]
    ref = DR.ref_rpn([torch.from_numpy(o) for o in objs], [torch.from_numpy(d) for d in dels], anchors, [IMG] * B)
    ref = [(bx.numpy(), sc.numpy()) for bx, sc in ref]
    if deltas == "overclamp":   # every box is the image rectangle: one proposal per level
        assert all(bx.shape[0] == L and (bx == np.asarray([0, 0, IMG[1], IMG[0]], np.float32)).all() for bx, _ in ref)
    else:                       # boxes of zero width after the clip exist (removed by min_size) and none is kept
        b0 = tv_ops.clip_boxes(tv_ops.decode_boxes(torch.from_numpy(dels[0][0]), anchors[0], (1.0,) * 4)[:, 0], IMG)
        assert int((b0[:, 2] - b0[:, 0] == 0).sum()) > 100
        assert all(((bx[:, 2] - bx[:, 0]) > 0).all() and 0 < bx.shape[0] < RPN_TOPK * L for bx, _ in ref)
    dev = {}
    for l in range(L):
        dev[l], dev[5 + l], dev[15 + l] = _dev(objs[l]), _dev(anchors[l].numpy()), _dev(dels[l])
    nch = (max(ns) + RPN_CHUNK - 1) // RPN_CHUNK
    assert nch == 4
    ints = {0: B, 1: L, 3: 3, 4: RPN_TOPK, 5: RPN_TOPK}
    ints.update({6 + l: n for l, n in enumerate(ns)})
    for chunked in (False, True):
        lst, dets = _List(B, L, RPN_TOPK), _Dets(B, frcnn.RPN_POST_NMS, labels=False)
        ptrs, ii, scratch = dict(dev), dict(ints), []
        ptrs.update(lst.ptrs(10))
        if chunked:
            scratch = [_Out(B * L * nch * 1024), _Out(B * L * nch * 1024), _Out(B * L * nch)]
            ptrs.update({20: scratch[0], 21: scratch[1], 22: scratch[2]})
            ii.update({16: RPN_CHUNK, 17: nch})
        _run(_rec(ops.RPN_LEVEL_NMS, ii, ptrs, flts=[IMG[0], IMG[1], frcnn.RPN_MIN_SIZE, frcnn.RPN_SCORE],
                  dbls=[frcnn.RPN_NMS]),
             _rec(ops.MERGE_TOPK, [B, L, RPN_TOPK, frcnn.RPN_POST_NMS], {**lst.ptrs(0), 5: None, **dets.ptrs(6)}))
        lst.check(kmax_le=RPN_TOPK)
        for s in scratch:
            s.get(s.n)
        _compare(dets.read(), ref, f"rpn {pattern} {deltas} chunked={chunked}", score_rtol=SCORE_RTOL)


# ------------------------------------------------------------------------------------- RetinaNet tail
RETINA_GRIDS = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]  # x 9 anchors: 2880 / 720 / 180 / 54 / 18
RET_TOPK, RET_DETS = 1000, 300


def _iou64(b, others):
    x1, y1 = np.maximum(b[0], others[:, 0]), np.maximum(b[1], others[:, 1])
    x2, y2 = np.minimum(b[2], others[:, 2]), np.minimum(b[3], others[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    area = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
    return inter / ((b[2] - b[0]) * (b[3] - b[1]) + area - inter)


def _retina_case(rs, case, anchors_all, K, B):
    """logits [B, Atot, K] and deltas [B, Atot, 4] of one case (see test_retina_tail_matches_reference)."""
    Atot = anchors_all.shape[0]
    # K = 2: shifts of at most a quarter of a side, so no box leaves the image (a zero-area box is never
    # suppressed) and the overlap of the anchors stays
    dels = np.stack([_exact_deltas(rs, anchors_all, span=16 if K == 91 else 2) for _ in range(B)])
    if case == "k91_separated":  # high logits rare: the top-k cut of the large levels falls inside a tie
        return (-6 + 0.5 * np.floor(25 * rs.rand(B, Atot, K) ** 64)).astype(np.float32), dels
    logits = np.full((B, Atot, K), -6.0, np.float32)
    logits[..., 1] = np.where(rs.rand(B, Atot) < 0.01, 2.0, -6.0)
    if case == "k2_clusters":    # every anchor a class-0 candidate, moved as near as dx, dy allow to one of 3 centres
        logits[..., 0] = _separated(rs, (B, Atot), -5, 12)
        a = anchors_all.numpy()
        w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        ctr = np.stack([a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h], 1)
        for b in range(B):
            cen = rs.uniform([30, 30], [IMG[1] - 30, IMG[0] - 30], (3, 2))
            to = cen[np.argmin(((ctr[:, None] - cen[None]) ** 2).sum(-1), 1)] - ctr
            dels[b, :, 0] = np.clip(np.round(to[:, 0] / w * 8) / 8, -2, 2)
            dels[b, :, 1] = np.clip(np.round(to[:, 1] / h * 8) / 8, -2, 2)
            _assert_exact_decode(dels[b], anchors_all)
    elif case == "k2_all_equal":
        logits[..., 0] = 1.0
    else:                        # k2_disjoint: class-0 candidates that do not suppress one another
        a = anchors_all.numpy().astype(np.float64)
        clipped = np.stack([a[:, 0].clip(0, IMG[1]), a[:, 1].clip(0, IMG[0]), a[:, 2].clip(0, IMG[1]),
                            a[:, 3].clip(0, IMG[0])], 1)
        for b in range(B):
            dels[b] = 0
            chosen = []
            for i in rs.permutation(Atot):  # greedy: pairwise IoU <= 0.45 (well below the 0.5 threshold)
                if not chosen or _iou64(clipped[i], clipped[chosen]).max() <= 0.45:
                    chosen.append(i)
            left = np.setdiff1d(np.nonzero(a[:, 0] < 0)[0], chosen)
            outside = rs.permutation(left)[:900]  # moved fully outside: zero width, IoU 0 / 0 never suppresses
            dels[b, outside, 0] = -2.0
            cand = np.concatenate([chosen, outside]).astype(np.int64)
            logits[b, cand, 0] = _separated(rs, cand.size, -5, 12)
            print(f"k2_disjoint image {b}: {len(chosen)} non-overlapping + {outside.size} outside candidates")
    return logits, dels


@pytest.mark.parametrize("case", ["k91_separated", "k2_disjoint", "k2_clusters", "k2_all_equal"])
def test_retina_tail_matches_reference(case):
    """oracle.retinanet.postprocess on the 128 x 160 image with retina_anchors (levels of 2880 / 720 / 180 /
    54 / 18 anchors), B = 2.  K = 91 with separated logits; K = 2 puts far more than 512 candidates into
    class 0, so retina_class_nms_kernel takes several rounds: candidates that do not suppress one another
    (it stops at 300 kept), the raw anchors (heavy overlap: many rounds, few kept, suppression by boxes kept
    in earlier rounds) and all-equal logits (the continuation walks through one long tie).  The chunk size
    gives the largest level three chunks; the smallest level has fewer flat entries than the top-k."""
    from edgeml_amd import ops
    from oracle import retinanet, tv_ops
    rs = np.random.RandomState(len(case))
    B, L = 2, len(RETINA_GRIDS)
    K = 91 if case.startswith("k91") else 2
    anchors = tv_ops.retina_anchors(RETINA_GRIDS, IMG_PAD)
    na = [int(a.shape[0]) for a in anchors]
    assert na == [2880, 720, 180, 54, 18]
    first = np.concatenate([[0], np.cumsum(na)[:-1]]).tolist()
    anchors_all = torch.cat(anchors)
    Atot = int(anchors_all.shape[0])
    logits, dels = _retina_case(rs, case, anchors_all, K, B)
    tl, td = torch.from_numpy(logits), torch.from_numpy(dels)
    ratio = np.resize(RATIO, (B, 2)).astype(np.float32)
    ref = DR.ref_retina([tl[:, f:f + n] for f, n in zip(first, na)], [td[:, f:f + n] for f, n in zip(first, na)],
                        anchors, [IMG] * B, ratio)
    if K == 2:  # class 0 holds more candidates than one round of the class kernel takes
        thr = np.float32(retinanet.SCORE_THRESH)
        for b in range(B):
            ncand = sum(min(RET_TOPK, int((torch.sigmoid(tl[b, f:f + n]).flatten() > thr).sum()))
                        for f, n in zip(first, na))
            kept0 = int((ref[b][2] == 0).sum())
            print(f"{case} image {b}: {ncand} candidates, class 0 keeps {kept0} of {ref[b][2].size}")
            assert ncand > 2 * 512
            if case == "k2_disjoint":  # the class reaches its capacity
                assert ref[b][2].size == RET_DETS and kept0 >= RET_DETS - 10
            else:                      # every round is walked: the class ends short of its capacity
                assert 0 < kept0 < (100 if case == "k2_clusters" else RET_DETS)
    chunk = (na[0] * K + 2) // 3
    nchunk = 3
    assert na[-1] * K < RET_TOPK or K == 91
    lvl, cls, dets = _List(B, L, RET_TOPK), _List(B, K, RET_DETS), _Dets(B, RET_DETS)
    scratch = [_Out(B * L * nchunk * 1024), _Out(B * L * nchunk * 1024), _Out(B * L * nchunk)]
    ints = {0: B, 1: L, 2: Atot, 3: K, 4: RET_TOPK, 5: RET_TOPK, 16: chunk, 17: nchunk}
    ints.update({6 + l: f for l, f in enumerate(first)})
    ints.update({11 + l: n for l, n in enumerate(na)})
    _run(_rec(ops.RETINA_SELECT, ints,
              {0: _dev(logits), 1: _dev(dels), 2: _dev(anchors_all.numpy()), **lvl.ptrs(3), 8: scratch[0],
               9: scratch[1], 10: scratch[2]}, flts=[IMG[0], IMG[1], retinanet.SCORE_THRESH]),
         _rec(ops.RETINA_CLASS_NMS, [B, L, RET_TOPK, K, RET_DETS], {**lvl.ptrs(0), **cls.ptrs(5)},
              dbls=[retinanet.NMS_THRESH]),
         _rec(ops.MERGE_TOPK, [B, K, RET_DETS, RET_DETS], {**cls.ptrs(0), 5: _dev(ratio), **dets.ptrs(6)}))
    lvl.check(kmax_le=RET_TOPK)
    cls.check(kmax_le=RET_DETS)
    for s in scratch:
        s.get(s.n)
    _compare(dets.read(), ref, f"retina {case}", score_rtol=SCORE_RTOL)
