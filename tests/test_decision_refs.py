"""The references of tests/decision_refs.py against the oracle they restate (CPU only): the reference
side of tests/test_gpu_decision_records.py must itself be right."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import frcnn, tv_ops
from tests import decision_refs as DR


def test_float32_scalar_comparison_rule():
    """The rule ref_box_tail and the kernels rely on: a float32 tensor compared with a Python scalar
    compares in float32, so a score of exactly float32(0.05) is not > 0.05 (in double it would be)."""
    s = torch.tensor([np.float32(0.05)])
    assert float(s[0]) > 0.05 and not bool((s > 0.05).any()) and bool((s >= 0.05).all())


def test_logit_sets_are_separated_and_saturated():
    """What tests/test_gpu_decision_records.py says of its logits: sigmoids of neighbouring multiples of
    0.5 in [-6, 6] differ by >= 1e-3, those of [20, 30] are exactly 1.0f, and -3.0 / -2.5 straddle 0.05."""
    s = torch.sigmoid(torch.arange(-12, 13, dtype=torch.float32) * 0.5)
    assert float((s[1:] - s[:-1]).min()) >= 1e-3
    assert bool((torch.sigmoid(20 + torch.arange(0, 21, dtype=torch.float32) * 0.5) == 1.0).all())
    assert float(np.exp(-20.0)) < 3e-9 < 2.0 ** -25
    assert float(torch.sigmoid(torch.tensor(-3.0))) < 0.048 and float(torch.sigmoid(torch.tensor(-2.5))) > 0.075


def test_ref_box_tail_reproduces_box_postprocess():
    rs = np.random.RandomState(7)
    NC, counts, shapes = 21, [37, 0, 1, 64], [(200, 300), (180, 240), (128, 160), (256, 256)]
    R = 64
    n = sum(counts)
    logits = torch.from_numpy((rs.randn(n, NC) * 3).astype(np.float32))
    deltas = torch.from_numpy((rs.randn(n, 4 * NC) * 1.5).astype(np.float32))
    xy = rs.uniform(-10, 200, (n, 2))
    wh = rs.uniform(1, 120, (n, 2))
    props = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).split(counts)
    want = frcnn.box_postprocess(logits, deltas, list(props), shapes)
    # the tail's inputs, as BOX_SCORES leaves them: probabilities and decoded, clipped boxes, padded to R
    sc_all = F.softmax(logits, -1).split(counts)
    bx_all = tv_ops.decode_boxes(deltas, torch.cat(props), (10.0, 10.0, 5.0, 5.0)).split(counts)
    scores = np.ones((len(counts), R, NC), np.float32)          # rows past counts[b]: score 1, a valid box
    boxes = np.tile(np.asarray([1, 2, 50, 60], np.float32), (len(counts), R, NC, 1))
    for b, c in enumerate(counts):
        scores[b, :c] = sc_all[b].numpy()
        boxes[b, :c] = tv_ops.clip_boxes(bx_all[b], shapes[b]).numpy()
    got = DR.ref_box_tail(scores, boxes, counts, frcnn.BOX_SCORE, frcnn.BOX_MIN_SIZE, frcnn.BOX_NMS, frcnn.BOX_DETS)
    sizes = []
    for (gb, gs, gl), w in zip(got, want):
        np.testing.assert_array_equal(gl, w["labels"].numpy())
        np.testing.assert_array_equal(gs, w["scores"].numpy())
        np.testing.assert_array_equal(gb, w["boxes"].numpy().reshape(-1, 4))
        sizes.append(gs.size)
    assert sizes[1] == 0 and sizes[0] == 100 and 0 < sizes[2] < 100, sizes  # full, empty and short lists


def test_ref_merge_orders_like_batched_nms():
    """Per-class kept lists (tv_ops.nms per class: score descending, lower index first; tiebreak = the
    candidate's index) merged by ref_merge equal batched_nms's own final order, under heavy score ties."""
    rs = np.random.RandomState(3)
    n, NCLS, N = 400, 5, 150
    xy = rs.randint(0, 40, (n, 2)).astype(np.float32)
    wh = rs.randint(2, 12, (n, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + wh], 1)
    scores = (rs.randint(1, 5, n) / 8).astype(np.float32)   # four distinct values
    labels = rs.randint(0, NCLS, n)
    keep = tv_ops.batched_nms(boxes, scores, labels, 0.5)[:N]
    assert keep.size == N and np.unique(scores[keep]).size >= 2
    rb, rsc = np.zeros((1, NCLS, n, 4), np.float32), np.zeros((1, NCLS, n), np.float32)
    rt, rl, rc = np.zeros((1, NCLS, n), np.int64), np.zeros((1, NCLS, n), np.int64), np.zeros((1, NCLS), np.int64)
    for c in range(NCLS):
        cur = np.nonzero(labels == c)[0]
        k = cur[tv_ops.nms(boxes[cur], scores[cur], 0.5)]
        rb[0, c, :k.size], rsc[0, c, :k.size], rt[0, c, :k.size], rl[0, c, :k.size] = boxes[k], scores[k], k, c
        rc[0, c] = k.size
    ratio = np.asarray([[1.5, 0.75]], np.float32)
    (gb, gs, gl), = DR.ref_merge(rb, rsc, rt, rl, rc, n, N, ratio)
    np.testing.assert_array_equal(gl, labels[keep])
    np.testing.assert_array_equal(gs, scores[keep])
    np.testing.assert_array_equal(gb, boxes[keep] * np.asarray([1.5, 0.75, 1.5, 0.75], np.float32))


def test_ref_merge_prefix_clamp_and_empty():
    box = np.arange(2 * 3 * 4 * 4, dtype=np.float32).reshape(2, 3, 4, 4)
    score = np.asarray([[[.5, .4, .9, .9], [.5, .5, .1, .9], [.9, .9, .9, .9]]] * 2, np.float32)
    tb = np.asarray([[[7, 6, 5, 4], [3, 2, 1, 0], [11, 10, 9, 8]]] * 2)
    count = np.asarray([[2, 9, 0], [0, 0, 0]])  # 9 > kmax clamps to 4; slots at and past count are ignored
    (b0, s0, l0), (b1, s1, l1) = DR.ref_merge(box, score, tb, tb, count, 4, 5)
    np.testing.assert_array_equal(l0, [0, 2, 3, 7, 6])
    np.testing.assert_array_equal(s0, np.asarray([.9, .5, .5, .5, .4], np.float32))
    np.testing.assert_array_equal(b0[0], box[0, 1, 3])
    assert s1.size == 0 and b1.shape == (0, 4)
