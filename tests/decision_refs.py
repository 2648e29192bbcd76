"""Plain references of the detectors' decision tails, built on oracle/tv_ops.py (no GPU).

* ref_merge      MERGE_TOPK: per image the valid prefix of every kept list, ordered by score descending
                 then tiebreak ascending, cut to N, boxes rescaled.
* ref_box_tail   RoIHeads.postprocess_detections after softmax, decode and clip (the part that
                 BOX_CLASS_NMS + MERGE_TOPK compute), a restatement of oracle.frcnn.box_postprocess.
* ref_rpn / ref_retina   oracle.frcnn.rpn_filter / oracle.retinanet.postprocess on head outputs.

tests/test_decision_refs.py checks these against the oracle on the CPU; tests/test_gpu_decision_records.py
compares the kernels with them.
"""
import numpy as np
import torch

from oracle import frcnn, retinanet, tv_ops


def _scale(ratio, b):
    if ratio is None:
        return np.ones(4, np.float32)
    rw, rh = np.float32(ratio[b][0]), np.float32(ratio[b][1])
    return np.asarray([rw, rh, rw, rh], np.float32)


def ref_merge(box, score, tb, label, count, kmax, N, ratio=None):
    """box [B,S,KM,4], score / tb / label [B,S,KM], count [B,S] (KM >= kmax: the list pitch is kmax in the
    kernel, so callers pass arrays of exactly that pitch).  Returns per image (boxes, scores, labels)."""
    box, score = np.asarray(box, np.float32), np.asarray(score, np.float32)
    tb, label, count = np.asarray(tb).astype(np.int64), np.asarray(label), np.asarray(count)
    B, S = count.shape
    assert box.shape[:3] == (B, S, kmax) and score.shape == (B, S, kmax)
    out = []
    for b in range(B):
        sel = [(s, j) for s in range(S) for j in range(min(int(count[b, s]), kmax))]
        si = np.asarray([p[0] for p in sel], np.int64)
        ji = np.asarray([p[1] for p in sel], np.int64)
        sc, t = score[b, si, ji], tb[b, si, ji]
        order = np.lexsort((t, -sc.astype(np.float64)))[:N]  # stable: score descending, then tb ascending
        si, ji = si[order], ji[order]
        out.append((box[b, si, ji].reshape(-1, 4) * _scale(ratio, b), score[b, si, ji], label[b, si, ji]))
    return out


def ref_box_tail(scores, boxes, counts, thr, min_size, iou, N, ratio=None):
    """scores [B,R,NC] (class probabilities), boxes [B,R,NC,4] (decoded, clipped), counts [B] valid RoIs.
    oracle.frcnn.box_postprocess after its clip_boxes: drop class 0, flatten in (roi, class) order,
    score > thr, remove_small, batched_nms, [:N].  thr and min_size compare as float32, as torch compares a
    float32 tensor with a Python scalar."""
    scores = torch.as_tensor(np.asarray(scores, np.float32))
    boxes = torch.as_tensor(np.asarray(boxes, np.float32))
    B, R, NC = scores.shape
    out = []
    for b in range(B):
        n = min(int(counts[b]), R)
        sc = scores[b, :n, 1:].reshape(-1)
        bx = boxes[b, :n, 1:].reshape(-1, 4)
        lab = torch.arange(NC).view(1, -1).expand(n, NC)[:, 1:].reshape(-1)
        inds = torch.where(sc > thr)[0]
        bx, sc, lab = bx[inds], sc[inds], lab[inds]
        keep = tv_ops.remove_small(bx, min_size)
        bx, sc, lab = bx[keep], sc[keep], lab[keep]
        keep = torch.from_numpy(tv_ops.batched_nms(bx.numpy(), sc.numpy(), lab.numpy(), iou))[:N]
        out.append((bx[keep].numpy().reshape(-1, 4) * _scale(ratio, b), sc[keep].numpy(), lab[keep].numpy()))
    return out


def ref_rpn(objs, dels, anchors, image_shapes):
    """oracle.frcnn.rpn_filter -> per image (proposals, scores)."""
    return frcnn.rpn_filter(objs, dels, anchors, image_shapes, with_scores=True)


def ref_retina(cls_all, reg_all, anchors, image_shapes, ratio=None):
    """oracle.retinanet.postprocess -> per image (boxes, scores, labels), boxes rescaled by ratio."""
    dets = retinanet.postprocess(cls_all, reg_all, anchors, image_shapes)
    return [(d["boxes"].numpy().reshape(-1, 4) * _scale(ratio, b), d["scores"].numpy(), d["labels"].numpy())
            for b, d in enumerate(dets)]
