"""The offloading cascade itself: the weak detector on every image, a reward estimate per image from the
weak detector's own output, and the strong detector only on the images whose estimate clears the
threshold (the policy test.py:30-42 simulates on saved files, run for real in one process).

    python -m edgeml_amd.offload img_dir save_dir --estimator WTS (--ratio R --estimates EST_DIR | --threshold T)
           [--fold 1] [--k 25] [--dataset coco|voc] [--weak ssd] [--strong faster_rcnn]
           [--weak-path P] [--strong-path P] [--weak-dir DIR] [--weak-batch N] [--strong-batch N]
           [--decode gpu|host] [--stage N --resize S [--pools P ...] [--fused]]
    python -m edgeml_amd.offload img_dir save_dir --estimator WTS --baseline af|dcsb   [the other options as above]

With --baseline, WTS is a saved comparison baseline, the wts<fold>.pickle of `edgeml_amd.baseline --model_dir`, and
the cascade runs that policy instead of ours.  Both are classifiers: an image is offloaded where its class is 1, the
threshold is 0.0, and --ratio, --estimates, --threshold, --stage, --resize, --pools and --fused are refused (a
classifier has no ratio).  af (Adaptive Feeding) is the linear SVM {coef, intercept, classes [0, 1]} on the
stage-24 features: rows -> features -> edgedet_offload_svm, whose decision value is edgedet_svm_decision's bit for
bit on the padded features (baseline.pad_features' layout, the padding implied), flag = value > 0 as the fit's
(dec > 0); `estimate` is the decision value.  dcsb is the tuple (conf_thresh, num_thresh, area_thresh):
rows -> edgedet_offload_dcsb (baseline.py:129-141 on the padded rows, one wave per image; no features are made);
`estimate` is 0.0 or 1.0.

With --stage N, WTS is a conv-stack estimator of `edgeml_amd.convnet --weak ssd --stage N --resize S --model-dir`
(conv_stacks.* tensors): the decision is taken from the weak detector's own stage-N map.  The hook pools each batch
chain's tapped buffer (edgeml_amd.tapnet.stage_table) to S x S with one edgedet_roi_align call -- convnet.pool_maps'
launcher and arguments, so the pooled values are the training route's bits -- and the layered eval forward
(convnet.Trainer.forward(train=False)) or, with --fused, one fused launch (csrc/tapnet.hip; a net outside its fit
rule is refused) writes the estimates and flags.  The layered forward is the default: in the weak stage the fused
kernel measured no faster.  A --resize 0 file runs the layered forward on the tapped map itself.

Otherwise WTS is a trained estimator on the stage-24 output features: wts<fold>.pickle as `edgeml_amd.estimator --model LR|EN|BR --model-dir` or
`edgeml_amd.svr --model LSVR --model-dir` writes it (plain numpy mean, scale, coef, intercept), wts<fold>.pth
as `--model CNN --model-dir` writes it (the MLP's tensors under EdgeDetectionNet's state-dict names; the
layer widths are read from the weight shapes), or the wts<fold>.pickle of `edgeml_amd.svr --model SVR` (the
support vectors and their dual coefficients) or of `edgeml_amd.estimator --model KNR` (the fold's training
rows and targets): those two predict from their stored rows through edgeml_amd.kpredict
(csrc/kpredict.hip), or the wts<fold>.pickle of `edgeml_amd.gbr --model GBR` (the boosted trees), which predicts
through edgeml_amd.gbr.GBRModel (csrc/gbr.hip), or the wts<fold>.pickle of `edgeml_amd.rfr --model RFR` (the
forest), which predicts through edgeml_amd.rfr.RFRModel (csrc/rfr.hip).  A KNR file written before the training rows were stored is
refused.  The threshold is
--threshold, or test.py:35 on EST_DIR/estimate<fold>.npz: train_est[argsort(-train_est)[int((len - 1) * R)]].

The weak model runs the detect CLI's batches (detect.image_sizes / distributed.size_batches /
detect._decoded_batches), so its results are that CLI's.  After each weak batch's replay a hook on the
batch's stream (models.run_batches post=) runs csrc/offload.hip: the detector's raw outputs -> the .npy
rows -> the stage-24 features -> the estimate -> flag = estimate > threshold -> the flagged images'
decoded bytes packed to the front of a device tensor; flags, estimates and the packed count come back
with the detections.  A generator feeds the strong model's run_batches from those packed tensors: per
image size it queues the survivors and, whenever --strong-batch of them wait (or the size group ends),
gathers them into one device batch.  The strong batches are therefore exactly
distributed.size_batches(selected images, strong_batch), the offloaded images are neither decoded nor
uploaded twice, and the device memory held for waiting images is a few batches.

Writes save_dir/<name>.npy for every image (the strong rows where offloaded, the weak rows otherwise;
fmt.save_npy), save_dir/offload.npz {names, estimate float64, offloaded bool, threshold, ratio_realized}
and, with --weak-dir, every weak file.  One process, one GPU: sharding the cascade is not built.
"""
import argparse
import ctypes
import os
import pickle
import sys
from pathlib import Path

import numpy as np
import torch

from . import fmt, ops


# ---------------------------------------------------------------------------------------- estimator file
MODEL_KINDS = ("svr", "knr", "gbr", "rfr")  # an Estimator.model (kpredict.KernelModel, gbr.GBRModel, rfr.RFRModel)
TREE_KINDS = ("gbr", "rfr")                 # ... of which these need no workspace
CLASSIFIER_KINDS = ("af", "dcsb")           # the comparison baselines: a class, not a reward; the threshold is 0.0


def _classifier_threshold(kind, threshold):
    if float(threshold) != 0.0:
        raise ValueError(f"the {kind} baseline is a classifier: it has no ratio and its threshold is 0.0, "
                         f"not {float(threshold)!r}")


class Estimator:
    """A trained reward estimator on `width` stage-24 features: kind "linear" (mean, scale, coef
    float64 [width], intercept), "mlp" (dims, state float32 in estimator.MlpSpec's layout), or "svr" /
    "knr" (model: the kpredict.KernelModel that predicts from the file's stored rows), or "gbr" (model: the
    gbr.GBRModel that walks the file's trees), or "rfr" (model: the rfr.RFRModel that walks the file's forest).
    Kind "convnet" reads no stage-24 features: net (a tapnet.TapNet) predicts from the weak detector's stage-`stage`
    map (map_shape = its C, H, W) pooled to resize x resize (0: the map itself, a --resize 0 net).
    The two comparison baselines of edgeml_amd.baseline are classifiers (CLASSIFIER_KINDS; the threshold is 0.0):
    kind "af" (v float64 [Dp]: the linear SVM's coef, its intercept at index width, zeros up to
    Dp = (width + 1 + 15) // 16 * 16) and kind "dcsb" (conf_thresh, num_thresh, area_thresh; width 0: it reads
    the detection rows, not the features)."""

    def __init__(self, kind, width, **data):
        self.kind, self.width = kind, int(width)
        self.__dict__.update(data)
        self._dev = None

    def device_data(self, device):
        """The model's arrays on the device (uploaded once)."""
        if self._dev is None or self._dev[0] != torch.device(device):
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            if self.kind in MODEL_KINDS:
                d = {"model": self.model.to(device)}  # uploads (and standardises the stored rows) once
            elif self.kind == "linear":
                d = {"mean": t(self.mean), "scale": t(self.scale), "coef": t(self.coef),
                     "intercept": t(np.array([self.intercept], np.float64))}
            elif self.kind == "af":
                d = {"v": t(self.v)}
            elif self.kind == "dcsb":
                d = {}  # three scalars, passed by value
            else:
                d = {"state": t(self.state)}
            self._dev = (torch.device(device), d)
        return self._dev[1]

    def workspace_bytes(self, B):
        """Bytes of the per-batch workspace an SVR or KNR model needs (edgedet_kmodel_workspace_size); 0 for
        the other kinds."""
        return self.model.workspace_bytes(B) if self.kind in MODEL_KINDS else 0

    def decide(self, feat, threshold, est, flag, scratch=(), stream=None, rows=None, nrow=None):
        """edgedet_offload_decide on feat [B, width] float64 (device): est [B] float64 and flag [B] uint8
        are written on `stream`; scratch = (x32 [B, width], est32 [B]) float32 for an MLP.  An SVR or KNR
        model takes a third entry, its uint8 workspace (workspace_bytes(B)): its estimates are
        kpredict.KernelModel's, then edgedet_offload_flag.  The classifiers take threshold 0.0 and no scratch:
        "af" is edgedet_offload_svm on feat (est: the decision value, flag: value > 0), "dcsb" is
        edgedet_offload_dcsb on rows [B, K, 6] and nrow [B] of format_rows (est: 0.0 / 1.0; feat is not read)."""
        if self.kind in CLASSIFIER_KINDS:
            _classifier_threshold(self.kind, threshold)
            if self.kind == "dcsb":
                ops._need_cuda(rows, nrow, est, flag)
                if rows is None or nrow is None:
                    raise ValueError("the dcsb baseline decides on the detection rows: give rows and nrow")
                ops.check(ops.lib().edgedet_offload_dcsb(ops._ptr(rows), ops._ptr(nrow), int(rows.shape[0]),
                                                         int(rows.shape[1]), float(self.conf_thresh), int(self.num_thresh),
                                                         float(self.area_thresh), None, None, None, ops._ptr(est),
                                                         ops._ptr(flag), ops.stream_handle(stream)))
                return
            ops._need_cuda(feat, est, flag)
            if feat.dim() != 2 or int(feat.shape[1]) != self.width:
                raise ValueError(f"the af baseline takes [B, {self.width}] features, got {tuple(feat.shape)}")
            v = self.device_data(feat.device)["v"]
            ops.check(ops.lib().edgedet_offload_svm(ops._ptr(feat), int(feat.shape[0]), self.width, ops._ptr(v),
                                                    int(v.numel()), ops._ptr(est), ops._ptr(flag),
                                                    ops.stream_handle(stream)))
            return
        B = int(feat.shape[0])
        d = self.device_data(feat.device)
        if self.kind in MODEL_KINDS:
            ws = scratch[2] if len(scratch) > 2 else None
            if ws is None and self.kind not in TREE_KINDS:  # the tree walks need no workspace
                raise ValueError(f"the {self.kind} estimator needs its workspace as scratch[2]")
            d["model"].predict_into(feat, est, ws, stream=stream)
            ops.check(ops.lib().edgedet_offload_flag(ops._ptr(est), B, float(threshold), ops._ptr(flag),
                                                     ops.stream_handle(stream)))
            return
        if self.kind == "linear":
            args = (ops._ptr(d["mean"]), ops._ptr(d["scale"]), ops._ptr(d["coef"]), ops._ptr(d["intercept"]), 0, None,
                    None, None, None)
        else:
            dims = (ctypes.c_int32 * len(self.dims))(*self.dims)
            args = (None, None, None, None, len(self.dims) - 1, dims, ops._ptr(d["state"]), ops._ptr(scratch[0]),
                    ops._ptr(scratch[1]))
        ops.check(ops.lib().edgedet_offload_decide(ops._ptr(feat), B, self.width, *args, float(threshold),
                                                   ops._ptr(est), ops._ptr(flag), ops.stream_handle(stream)))


def _check_width(path, what, have, width, consistent=True):
    if have != width or not consistent:
        raise ValueError(f"{path}: the {what} takes {have} features, the cascade makes {width} "
                         f"(num_class + 5 k: check --k and --dataset)")


def _is_af_file(m):
    return isinstance(m, dict) and "coef" in m and "intercept" in m and "classes" in m and "mean" not in m


def _is_dcsb_file(m):
    return isinstance(m, tuple) and len(m) == 3


def load_baseline(path, width, baseline):
    """The wts<fold>.pickle of `edgeml_amd.baseline --model_dir` as a classifier Estimator.  baseline "af": the
    dict {coef [width], intercept, classes [0, 1], ...} of the Adaptive Feeding SVM, as kind "af" with
    baseline.pad_features' layout of the weights; baseline "dcsb": the tuple (conf_thresh float, num_thresh int,
    area_thresh float), as kind "dcsb".  ValueError, naming what was expected, on any other file."""
    import numbers
    if baseline not in CLASSIFIER_KINDS:
        raise ValueError(f"baseline {baseline!r}: one of {', '.join(CLASSIFIER_KINDS)}")
    what = ("the Adaptive Feeding file of edgeml_amd.baseline --baseline af --model_dir "
            "({coef, intercept, classes: [0, 1]})" if baseline == "af" else
            "the DCSB file of edgeml_amd.baseline --baseline dcsb --model_dir "
            "((conf_thresh float, num_thresh int, area_thresh float))")
    m = None
    if not str(path).endswith(".pth"):
        with open(path, "rb") as f:
            try:
                m = pickle.load(f)
            except (pickle.UnpicklingError, EOFError):
                pass
    if baseline == "af":
        if not _is_af_file(m) or [int(c) for c in np.asarray(m["classes"]).reshape(-1)] != [0, 1]:
            raise ValueError(f"{path}: --baseline af expects {what}")
        coef = np.asarray(m["coef"], np.float64).reshape(-1)
        _check_width(path, "Adaptive Feeding SVM", len(coef), width)
        v = np.zeros((len(coef) + 1 + 15) // 16 * 16, np.float64)
        v[:len(coef)], v[len(coef)] = coef, float(m["intercept"])
        if len(v) > 256:
            raise ValueError(f"{path}: {len(coef)} features + bias exceed the decision kernel's 256 columns")
        return Estimator("af", width, v=v)
    real = lambda x: isinstance(x, numbers.Real) and not isinstance(x, (bool, numbers.Integral))  # noqa: E731
    if not _is_dcsb_file(m) or not real(m[0]) or not real(m[2]) or isinstance(m[1], bool) or \
            not isinstance(m[1], numbers.Integral):
        raise ValueError(f"{path}: --baseline dcsb expects {what}")
    return Estimator("dcsb", 0, conf_thresh=float(m[0]), num_thresh=int(m[1]), area_thresh=float(m[2]))


def load_estimator(path, width, support=False, stage=None, resize=None, pools=None, num_classes=91, reduced_tail=True,
                   fused=None, baseline=None):
    """With baseline="af" | "dcsb": load_baseline (the saved comparison baselines of edgeml_amd.baseline; stage,
    resize, pools and fused do not apply).  With stage=N: the conv-stack file of edgeml_amd.convnet as kind "convnet" (net: a tapnet.TapNet whose
    ConvSpec is rebuilt from the tensor shapes, for the SSDLite stage-N map of (num_classes, reduced_tail) pooled
    to resize x resize; pools: the net's pools when not the convnet CLI's default).  ValueError when the first conv
    layer's Cin is not the stage's channel count, when the first linear width is not the pooled geometry's, and
    for a stage the table does not have.  Without stage, as before:

    The estimator of a wts<fold>.pickle / wts<fold>.pth file (an LSVR file of edgeml_amd.svr is a linear
    model).  A KNR file that holds its training rows ('train', 'target') loads as kind "knr"; with
    support=True (what the cascade passes) an SVR file loads as kind "svr", otherwise it is refused as before;
    a GBR file of edgeml_amd.gbr loads as kind "gbr", an RFR file of edgeml_amd.rfr as kind "rfr".
    Raises ValueError on a KNR file without training rows, on a file that is none of these, on inconsistent
    shapes, and when the model's feature width is not `width`."""
    from . import gbr, kpredict, rfr
    from .estimator import MlpSpec
    if baseline is not None:
        return load_baseline(path, width, baseline)
    if str(path).endswith(".pth"):
        named = torch.load(path, map_location="cpu", weights_only=True)
        named = {k: v.numpy() for k, v in named.items() if torch.is_tensor(v)}
        if stage is not None:
            from . import tapnet
            if not any(k.startswith("conv_stacks.") for k in named):
                raise ValueError(f"{path}: --stage {stage} takes a conv-stack estimator of edgeml_amd.convnet "
                                 "(conv_stacks.* tensors); this file has none")
            token, C, H, W = tapnet.stage_info(stage, num_classes, reduced_tail)
            spec = tapnet.spec_from_named(path, named, C, resize, pools)
            if fused and not tapnet.TapNet(spec, spec.pack(named)).fits:
                raise ValueError(f"{path}: --fused: the net is outside the fused kernel's fit rule "
                                 "(edgedet_tapnet_fits); drop --fused for the layered forward")
            return Estimator("convnet", width, net=tapnet.TapNet(spec, spec.pack(named), fused=fused), stage=int(stage),
                             resize=int(resize or 0), map_shape=(C, H, W))
        if any(k.startswith("conv_stacks.") for k in named):
            raise ValueError(f"{path}: a conv-stack estimator of edgeml_amd.convnet (conv_stacks.* tensors): it reads the "
                             "weak detector's hidden-layer feature maps, which the cascade does not have; use an "
                             "estimator trained on the stage-24 output features")
        L = 0
        while f"linear_stacks.{L}.0.weight" in named:
            L += 1
        if L == 0:
            raise ValueError(f"{path}: no linear_stacks.<l>.0.weight tensors (not an estimator --model CNN file)")
        shapes = [tuple(named[f"linear_stacks.{l}.0.weight"].shape) for l in range(L)]
        dims = [int(shapes[0][1])] + [int(s[0]) for s in shapes]
        if any(len(s) != 2 for s in shapes) or any(shapes[l][1] != dims[l] for l in range(L)) or dims[-1] != 1:
            raise ValueError(f"{path}: the linear layers {shapes} do not chain to one output")
        _check_width(path, "MLP", dims[0], width)
        spec = MlpSpec(dims)
        missing = [k for k in spec.unpack(np.zeros(spec.ns, np.float32)) if k not in named]
        if missing:
            raise ValueError(f"{path}: missing tensors {missing[:4]}")
        return Estimator("mlp", width, dims=dims, state=spec.pack(named))
    with open(path, "rb") as f:
        m = pickle.load(f)
    if not isinstance(m, dict) or "mean" not in m or "scale" not in m:
        hint = " (an Adaptive Feeding file of edgeml_amd.baseline: give --baseline af)" if _is_af_file(m) else \
            " (a DCSB file of edgeml_amd.baseline: give --baseline dcsb)" if _is_dcsb_file(m) else ""
        raise ValueError(f"{path}: not a wts<fold>.pickle of edgeml_amd.estimator --model-dir{hint}")
    if stage is not None:
        raise ValueError(f"{path}: --stage {stage} takes a conv-stack wts<fold>.pth of edgeml_amd.convnet; this "
                         "estimator reads the stage-24 output features (drop --stage and --resize)")
    if m.get("model") == "SVR" and not support:
        raise ValueError(f"{path}: an SVR file holds support vectors, and the cascade does not predict from them "
                         f"yet; train --model LSVR, LR, EN, BR or CNN")
    if m.get("model") in ("GBR", "RFR", "SVR") or (m.get("model") == "KNR" and "train" in m and "target" in m):
        model = {"GBR": gbr, "RFR": rfr}.get(m["model"], kpredict).load(m)
        _check_width(path, "model", model.width, width)
        return Estimator(model.kind, width, model=model)
    if m.get("model") == "KNR" or "coef" not in m:
        raise ValueError(f"{path}: a KNR file holds no training rows, so the cascade cannot predict from it; "
                         f"train --model LR, EN, BR or CNN")
    mean, scale, coef = (np.ascontiguousarray(np.asarray(m[k], np.float64).reshape(-1)) for k in ("mean", "scale", "coef"))
    _check_width(path, "model", len(coef), width, len(mean) == len(scale) == len(coef))
    return Estimator("linear", width, mean=mean, scale=scale, coef=coef, intercept=float(m["intercept"]))


def _has_conv_stacks(path):
    named = torch.load(path, map_location="cpu", weights_only=True)
    return any(str(k).startswith("conv_stacks.") for k in named)


def _weak_tail(opts):
    """The tail of the weak SSDLite the detect CLI would load (detect.load_weak_models): the COCO-pretrained
    reduced tail without --weak-path, else what the file's tensors say."""
    if not opts.weak_path:
        return True
    sd = torch.load(opts.weak_path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "model" in sd and not torch.is_tensor(sd["model"]):
        sd = sd["model"]
    w = sd.get("backbone.features.1.3.0.weight")
    return True if w is None else tuple(w.shape)[1] == 80


def ratio_threshold(train_est, ratio):
    """test.py:35."""
    train_est = np.asarray(train_est)
    return train_est[np.argsort(-train_est)[int((len(train_est) - 1) * ratio)]]


def resolve_threshold(opts):
    if opts.threshold is not None:
        return float(opts.threshold)
    with np.load(os.path.join(opts.estimates, f"estimate{opts.fold}.npz"), allow_pickle=False) as z:
        return float(ratio_threshold(z["train_est"], opts.ratio))


# ---------------------------------------------------------------------------------------- strong queue
class BatchQueue:
    """The strong stage's batching as pure logic.  push(size, items) takes the survivors of one weak
    batch (all of one image size) and returns the batches that became ready; a change of size ends the
    previous size group and flushes its remainder first; finish() flushes what is left.  Fed the weak
    batches of distributed.size_batches (equal sizes arrive together), the batches that come out are
    size_batches(selected images, batch)."""

    def __init__(self, batch):
        self.batch, self.size, self.items = int(batch), None, []
        if self.batch < 1:
            raise ValueError("strong batch must be >= 1")

    def push(self, size, items):
        out = []
        if self.size is not None and size != self.size:
            out += self.finish()
        self.size = size
        self.items += list(items)
        while len(self.items) >= self.batch:
            out.append((self.size, self.items[:self.batch]))
            self.items = self.items[self.batch:]
        return out

    def finish(self):
        out = [(self.size, self.items)] if self.items else []
        self.items = []
        return out


# ---------------------------------------------------------------------------------------- device chain
def format_rows(count, boxes, scores, labels, H, W, dataset="coco", rows=None, nrow=None, stream=None):
    """edgedet_offload_rows: device tensors count [B] int32, boxes [B,K,4] f32, scores [B,K] f32, labels
    [B,K] int64 -> (rows [B,K,6] float64, nrow [B] int32); the first nrow[b] rows of image b are
    fmt.format_batch's."""
    ops._need_cuda(count, boxes, scores, labels, rows, nrow)
    B, K = (int(v) for v in scores.shape)
    if rows is None:
        rows = torch.zeros((B, K, 6), dtype=torch.float64, device=scores.device)
        nrow = torch.zeros((B,), dtype=torch.int32, device=scores.device)
    ops.check(ops.lib().edgedet_offload_rows(ops._ptr(count), ops._ptr(boxes), ops._ptr(scores), ops._ptr(labels), B, K,
                                             int(H), int(W), int(dataset != "coco"), ops._ptr(rows), ops._ptr(nrow),
                                             ops.stream_handle(stream)))
    return rows, nrow


def row_features(rows, nrow, num_class, k=25, out=None, stream=None):
    """edgedet_offload_features: padded rows [B,K,6] float64 + nrow [B] -> [B, num_class + 5 k] float64,
    features.output_features' bytes."""
    ops._need_cuda(rows, nrow, out)
    B, K = int(rows.shape[0]), int(rows.shape[1])
    if out is None:
        out = torch.empty((B, num_class + 5 * k), dtype=torch.float64, device=rows.device)
    ops.check(ops.lib().edgedet_offload_features(ops._ptr(rows), ops._ptr(nrow), B, K, int(num_class), int(k),
                                                 ops._ptr(out), ops.stream_handle(stream)))
    return out


def pack(flag, src, dst, count, index, stream=None):
    """edgedet_offload_pack: the images of src [B,...] uint8 whose flag [B] uint8 is set, copied to the
    front of dst in index order; count [1] and index [B] int32 (device)."""
    ops._need_cuda(flag, src, dst, count, index)
    B = int(src.shape[0])
    ops.check(ops.lib().edgedet_offload_pack(ops._ptr(flag), ops._ptr(src), B, src.numel() // B, ops._ptr(dst),
                                             ops._ptr(count), ops._ptr(index), ops.stream_handle(stream)))


def gather(pairs, out=None, stream=None):
    """edgedet_offload_gather: pairs [(device uint8 tensor [B,3,H,W], image index)] -> one contiguous
    [len(pairs),3,H,W] uint8 device tensor."""
    ops._need_cuda(*[t for t, _ in pairs])
    n, shape = len(pairs), tuple(pairs[0][0].shape[1:])
    if any(tuple(t.shape[1:]) != shape or t.dtype != torch.uint8 or not 0 <= int(j) < t.shape[0] for t, j in pairs):
        raise ValueError("gather: uint8 batches of one image shape, indices inside them")
    if out is None:
        out = torch.empty((n,) + shape, dtype=torch.uint8, device=pairs[0][0].device)
    src = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in pairs])
    idx = (ctypes.c_int32 * n)(*[int(j) for _, j in pairs])
    ops.check(ops.lib().edgedet_offload_gather(src, idx, n, out.numel() // n, ops._ptr(out), ops.stream_handle(stream)))
    return out


class Chain:
    """The run_batches post hook of the weak model: rows -> features -> estimate -> flags -> pack on the
    slot's stream.  Its device scratch and pinned result buffers live on the slot; the packed images are
    a fresh tensor per batch, handed on to the strong stage.  The "dcsb" baseline decides on the rows
    (rows -> edgedet_offload_dcsb -> pack: no features); "af" is rows -> features -> edgedet_offload_svm -> pack."""

    def __init__(self, estimator, threshold, num_class, k, dataset):
        self.est, self.threshold, self.num_class, self.k, self.dataset = estimator, float(threshold), num_class, k, dataset

    def map_buffers(self, plan, sl):
        """The convnet estimator's slot state: the plan's taps of its stage, the whole-image RoIs of every chain,
        the pooled maps and, for the layered path, one Trainer (its activation buffers belong to this slot's
        stream)."""
        from . import tapnet
        e, B = self.est, plan.B
        buf = sl.get("offload")
        fused = e.net.use_fused()
        if buf is None or buf["key"] != (B, e.stage, e.resize, fused, id(e.net)):
            dev = plan.device
            model = plan.model
            taps = tapnet.stage_table(model.num_classes, model.reduced_tail, B, plan.H, plan.W, plan.u8, e.stage)
            C, H, W = taps[0].C, taps[0].H, taps[0].W
            if (C, H, W) != tuple(e.map_shape):
                raise ValueError(f"stage {e.stage}: the plan's map is {(C, H, W)}, the estimator was loaded for "
                                 f"{tuple(e.map_shape)} (check --dataset and the weak model's tail)")
            d = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
            p = lambda shape, dt: torch.zeros(shape, dtype=dt, pin_memory=True)  # noqa: E731
            n = max(t.images for t in taps)
            rois = np.zeros((n, 5), np.float32)  # lib/data.py load_feature: box [0, 0, w, h] of image i
            rois[:, 0], rois[:, 3], rois[:, 4] = np.arange(n), W, H
            S = e.resize
            buf = sl["offload"] = {
                "key": (B, e.stage, e.resize, fused, id(e.net)), "taps": [(t, plan.buffer(t.buffer).tensor()) for t in taps],
                "rois": torch.from_numpy(rois).to(dev), "pooled": d((B, S, S, C), torch.float32) if S else None,
                "trainer": None if fused else e.net.trainer(dev, B if S else n, H * W),
                "est": d((B,), torch.float64), "flag": d((B,), torch.uint8), "count": d((1,), torch.int32),
                "index": d((B,), torch.int32),
                "h_est": p((B,), torch.float64), "h_flag": p((B,), torch.uint8), "h_count": p((1,), torch.int32),
                "h_index": p((B,), torch.int32)}
        return buf

    def decide_from_maps(self, plan, b, stream):
        """Pool each chain's tapped buffer (one edgedet_roi_align call per chain), then the estimates and flags
        of the batch."""
        e, S = self.est, self.est.resize
        for t, x in b["taps"]:
            if S:
                out = b["pooled"][t.image0:t.image0 + t.images]
                ops.check(ops.lib().edgedet_roi_align(ops._ptr(x), t.images, t.H, t.W, t.C, ops._ptr(b["rois"]),
                                                      t.images, 1.0, S, S, 0, ops._ptr(out), ops.stream_handle(stream)))
            else:  # a --resize 0 net reads the map itself: the layered forward, chain by chain
                sl = slice(t.image0, t.image0 + t.images)
                e.net.infer(x, self.threshold, b["est"][sl], b["flag"][sl], stream, b["trainer"])
        if S:
            e.net.infer(b["pooled"], self.threshold, b["est"], b["flag"], stream, b["trainer"])

    def buffers(self, plan, sl):
        B, K = (int(v) for v in plan.out_score.shape)
        D = self.num_class + 5 * self.k
        buf = sl.get("offload")
        wb = self.est.workspace_bytes(B)  # an SVR / KNR model's tiles; 0 otherwise
        if buf is None or buf["key"] != (B, K, D, wb):
            dev = plan.device
            d = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
            p = lambda shape, dt: torch.zeros(shape, dtype=dt, pin_memory=True)  # noqa: E731
            buf = sl["offload"] = {
                "key": (B, K, D, wb), "kws": d((wb,), torch.uint8) if wb else None,
                "rows": d((B, K, 6), torch.float64), "nrow": d((B,), torch.int32),
                "feat": None, "x32": None, "est32": None,
                "est": d((B,), torch.float64), "flag": d((B,), torch.uint8), "count": d((1,), torch.int32),
                "index": d((B,), torch.int32),
                "h_est": p((B,), torch.float64), "h_flag": p((B,), torch.uint8), "h_count": p((1,), torch.int32),
                "h_index": p((B,), torch.int32)}
        # what the rule reads, made when a rule first needs it (the slot may have served another estimator under
        # the same key): dcsb decides on the rows alone, af needs the features but not the MLP's float32 scratch
        kind = self.est.kind
        need = [] if kind == "dcsb" else [("feat", (B, D), torch.float64)]
        if kind not in CLASSIFIER_KINDS:
            need += [("x32", (B, D), torch.float32), ("est32", (B,), torch.float32)]
        for name, shape, dt in need:
            if buf[name] is None:
                buf[name] = torch.zeros(shape, dtype=dt, device=plan.device)
        return buf

    def __call__(self, plan, sl, stream, tag):
        if not plan.u8:
            raise ValueError("the cascade packs the decoded uint8 images: the weak batches must be uint8")
        if self.est.kind == "convnet":
            b = self.map_buffers(plan, sl)
            self.decide_from_maps(plan, b, stream)
        else:
            b = self.buffers(plan, sl)
            format_rows(plan.out_count.tensor(), plan.out_box.tensor(), plan.out_score.tensor(),
                        plan.out_label.tensor(), plan.H, plan.W, self.dataset, b["rows"], b["nrow"], stream)
            if self.est.kind == "dcsb":  # no features: the rule reads the rows
                self.est.decide(None, self.threshold, b["est"], b["flag"], stream=stream, rows=b["rows"], nrow=b["nrow"])
            else:
                row_features(b["rows"], b["nrow"], self.num_class, self.k, b["feat"], stream)
                self.est.decide(b["feat"], self.threshold, b["est"], b["flag"], (b["x32"], b["est32"], b["kws"]), stream)
        images = plan.input.tensor()
        packed = torch.empty_like(images)  # this batch's own: it outlives the slot's next use
        pack(b["flag"], images, packed, b["count"], b["index"], stream)
        for k in ("est", "flag", "count", "index"):
            b["h_" + k].copy_(b[k], non_blocking=True)
        sl["post"] = {"estimate": b["h_est"], "flag": b["h_flag"], "count": b["h_count"], "index": b["h_index"],
                      "packed": packed}


# ---------------------------------------------------------------------------------------- the cascade
def run(img_dir, estimator, threshold, k=25, dataset="coco", weak="ssd", strong="faster_rcnn", weak_path="",
        strong_path="", weak_batch=0, strong_batch=0, decode="gpu", on_rows=None, device="cuda:0", baseline=None):
    """Run the cascade on a directory of images.  estimator: an Estimator or a wts file (baseline "af" / "dcsb":
    a saved model of edgeml_amd.baseline; such a classifier takes threshold 0.0, anything else is a ValueError:
    estimate is then the SVM's decision value, or DCSB's 0.0 / 1.0); weak / strong:
    a detect CLI model name (loaded from weak_path / strong_path) or a detector of models.py.  Returns
    {names, estimate [n] float64, offloaded [n] bool, threshold, ratio_realized, rows {name: final
    rows}, weak_rows {name: weak rows}, strong_batches [[name, ...], ...], seconds {phase: host
    seconds}}.  on_rows(kind, name, rows)
    is called as rows become ready (kind "weak" for every image, "final" once per image)."""
    import time
    from . import detect, distributed as dist_mod
    clock = {"start": time.perf_counter(), "strong_model": 0.0}
    if isinstance(estimator, Estimator) and estimator.kind in CLASSIFIER_KINDS:
        _classifier_threshold(estimator.kind, threshold)
    if not torch.cuda.is_available():
        raise RuntimeError("edgeml_amd.offload needs an MI355X (HIP) device; there is no CPU path")
    num_class = 20 if dataset == "voc" else 80      # classes of the .npy rows (features.main)
    det_classes = 91 if dataset == "coco" else 21   # classes of the detectors (detect.main)
    if not isinstance(estimator, Estimator):
        estimator = load_estimator(estimator, num_class + 5 * k, support=True, baseline=baseline)
    if estimator.kind in CLASSIFIER_KINDS:
        _classifier_threshold(estimator.kind, threshold)
    if estimator.kind not in ("convnet", "dcsb") and estimator.width != num_class + 5 * k:
        raise ValueError(f"the estimator takes {estimator.width} features, the cascade makes {num_class + 5 * k}")
    torch.cuda.set_device(device)
    data = detect.ObjectDetectionDataset(img_dir)
    names = data.img_names
    load = lambda m, path: m if not isinstance(m, str) else \
        detect.load_weak_models(m, path, det_classes).to(device).eval()  # noqa: E731
    weak_model = load(weak, weak_path)
    clock["weak_model"] = time.perf_counter()
    sizes = detect.image_sizes(data)
    clock["sizes"] = time.perf_counter()
    chunks = dist_mod.size_batches(sizes, min(weak_batch or weak_model.max_batch, weak_model.max_batch))
    tagged = (((nm, hw), buf) for nm, hw, buf in
              detect._decoded_batches(data, chunks, sizes, device_decode=decode == "gpu"))
    chain = Chain(estimator, threshold, num_class, k, dataset)
    est, flags, weak_rows, rows, strong_batches = {}, {}, {}, {}, []
    tell = on_rows or (lambda kind, name, r: None)
    strong_model = [None]

    def strong_input():
        """Drives the weak model; yields the strong model's batches ((names, (H, W)), device tensor)."""
        queue = None

        def assemble(ready):
            for (h, w), items in ready:
                cur = torch.cuda.current_stream()
                batch = gather([(t, j) for _, t, j in items], stream=cur)
                for t in {id(t): t for _, t, _ in items}.values():
                    t.record_stream(cur)  # allocated on the weak slot's stream, read on this one
                strong_batches.append([n for n, _, _ in items])
                yield ([n for n, _, _ in items], (h, w)), batch

        for (nm, (h, w)), counts, boxes, scores, labels, ex in weak_model.run_batches(tagged, raw=True, post=chain):
            for name, r in zip(nm, fmt.format_batch(boxes, scores, labels, counts, h, w, dataset)):
                weak_rows[name] = r
                tell("weak", name, r)
            sel = np.nonzero(ex["flag"][:len(nm)])[0]
            if int(ex["count"][0]) != len(sel) or not np.array_equal(ex["index"][:len(sel)], sel):
                raise ops.EdgeDetError("offload: the packed images do not match the flags")
            for j, name in enumerate(nm):
                est[name], flags[name] = float(ex["estimate"][j]), bool(ex["flag"][j])
                if not flags[name]:
                    rows[name] = weak_rows[name]
                    tell("final", name, rows[name])
            if len(sel) == 0:
                continue
            if queue is None:
                if strong_model[0] is None:
                    t0 = time.perf_counter()
                    strong_model[0] = load(strong, strong_path)  # only once an image is offloaded
                    clock["strong_model"] = time.perf_counter() - t0
                queue = BatchQueue(min(strong_batch or strong_model[0].max_batch, strong_model[0].max_batch))
            yield from assemble(queue.push((h, w), [(nm[i], ex["packed"], j) for j, i in enumerate(sel)]))
        if queue is not None:
            yield from assemble(queue.finish())

    feed = strong_input()
    first = next(feed, None)  # runs the weak model up to the first strong batch (all of it when there is none)
    if first is not None:
        import itertools
        for (nm, (h, w)), counts, boxes, scores, labels in strong_model[0].run_batches(
                itertools.chain([first], feed), raw=True):
            for name, r in zip(nm, fmt.format_batch(boxes, scores, labels, counts, h, w, dataset)):
                rows[name] = r
                tell("final", name, r)
    offloaded = np.array([flags[n] for n in names], dtype=bool)
    end = time.perf_counter()
    # host seconds per phase (EDGEDET_DETECT_TIMING=1: the CLI prints them, as the detect CLI does)
    seconds = {"weak_model": clock["weak_model"] - clock["start"], "sizes": clock["sizes"] - clock["weak_model"],
               "strong_model": clock["strong_model"], "engine": end - clock["sizes"] - clock["strong_model"]}
    return {"seconds": seconds, "names": list(names), "estimate": np.array([est[n] for n in names], dtype=np.float64),
            "offloaded": offloaded, "threshold": float(threshold),
            "ratio_realized": float(offloaded.mean()) if len(names) else 0.0,
            "rows": rows, "weak_rows": weak_rows, "strong_batches": strong_batches}


def main(opts):
    import concurrent.futures as cf
    from .distributed import usable_cpus
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("edgeml_amd.offload runs in one process on one GPU: sharding the cascade over several "
                         "GPUs is not built (run it without torchrun)")
    num_class = 20 if opts.dataset == "voc" else 80
    if (opts.stage is None) != (opts.resize is None):
        raise SystemExit("edgeml_amd.offload: --stage N and --resize S go together (a conv-stack estimator of "
                         "edgeml_amd.convnet on the weak detector's stage-N map pooled to S x S; --resize 0 for a "
                         "net trained with --resize 0)")
    if opts.stage is not None and opts.weak != "ssd":
        raise SystemExit("edgeml_amd.offload: --stage reads SSDLite's stage table; --weak ssd is the only producer")
    try:
        if opts.baseline:
            estimator = load_baseline(opts.estimator, num_class + 5 * opts.k, opts.baseline)
        else:
            if opts.stage is None and str(opts.estimator).endswith(".pth") and _has_conv_stacks(opts.estimator):
                raise ValueError(f"{opts.estimator}: a conv-stack estimator of edgeml_amd.convnet: give --stage N (the "
                                 "SSDLite stage it was trained on) and --resize S (its --resize)")
            estimator = load_estimator(opts.estimator, num_class + 5 * opts.k, support=True, stage=opts.stage,
                                       resize=opts.resize, pools=opts.pools,
                                       num_classes=91 if opts.dataset == "coco" else 21,
                                       reduced_tail=_weak_tail(opts), fused=True if opts.fused else None)
    except ValueError as e:
        raise SystemExit(f"edgeml_amd.offload: {e}") from None
    threshold = 0.0 if opts.baseline else resolve_threshold(opts)  # a classifier: offload where the class is 1
    Path(opts.save_dir).mkdir(parents=True, exist_ok=True)
    if opts.weak_dir:
        Path(opts.weak_dir).mkdir(parents=True, exist_ok=True)
    with cf.ThreadPoolExecutor(usable_cpus()) as writers:
        pending = []

        def on_rows(kind, name, r):
            if kind == "final":
                pending.append(writers.submit(fmt.save_npy, opts.save_dir, name, r))
            elif opts.weak_dir:
                pending.append(writers.submit(fmt.save_npy, opts.weak_dir, name, r))

        res = run(opts.img_dir, estimator, threshold, opts.k, opts.dataset, opts.weak, opts.strong, opts.weak_path,
                  opts.strong_path, opts.weak_batch, opts.strong_batch, opts.decode, on_rows)
        for f in pending:
            f.result()  # re-raise a failed write
    np.savez(os.path.join(opts.save_dir, "offload.npz"), names=np.array(res["names"], dtype=str),
             estimate=res["estimate"], offloaded=res["offloaded"], threshold=np.float64(res["threshold"]),
             ratio_realized=np.float64(res["ratio_realized"]))
    if os.environ.get("EDGEDET_DETECT_TIMING") == "1":
        print("offload timing (s): " + ", ".join(f"{k} {v:.3f}" for k, v in res["seconds"].items()) +
              f", images {len(res['names'])}", file=sys.stderr, flush=True)
    print(f"offloaded {int(res['offloaded'].sum())} of {len(res['names'])} images "
          f"(threshold {res['threshold']!r}, realised ratio {res['ratio_realized']:.4f})")
    return res


def getargs(argv=None):
    a = argparse.ArgumentParser(prog="edgeml_amd.offload")
    a.add_argument("img_dir", help="Directory of the images to run the cascade on.")
    a.add_argument("save_dir", help="Directory for the detections (<name>.npy) and offload.npz.")
    a.add_argument("--estimator", required=True, help="wts<fold>.pickle (LR / EN / BR / LSVR / SVR / KNR / GBR / RFR) or wts<fold>.pth (CNN).")
    a.add_argument("--ratio", type=float, default=None, help="Offloading ratio: the threshold is test.py:35's on --estimates.")
    a.add_argument("--estimates", type=str, default=None, help="Directory holding estimate<fold>.npz (with --ratio).")
    a.add_argument("--threshold", type=float, default=None, help="Offload an image when its estimate exceeds this.")
    a.add_argument("--fold", type=int, default=1)
    a.add_argument("--k", type=int, default=25, help="Top-K bounding boxes of the stage-24 features.")
    a.add_argument("--dataset", choices=("coco", "voc"), default="coco")
    a.add_argument("--weak", type=str, default="ssd")
    a.add_argument("--strong", type=str, default="faster_rcnn")
    a.add_argument("--weak-path", type=str, default="")
    a.add_argument("--strong-path", type=str, default="")
    a.add_argument("--weak-dir", type=str, default="", help="Also write every weak detection file here.")
    a.add_argument("--weak-batch", type=int, default=0, help="Images per weak engine call (0 = model default).")
    a.add_argument("--strong-batch", type=int, default=0, help="Images per strong engine call (0 = model default).")
    a.add_argument("--decode", choices=("gpu", "host"), default="gpu")
    a.add_argument("--stage", type=int, default=None, help="Decide from the weak detector's stage-N map (SSDLite's "
                   "stage table) with a conv-stack estimator of edgeml_amd.convnet; needs --resize.")
    a.add_argument("--resize", type=int, default=None, help="The side S the maps are pooled to (the net's --resize).")
    a.add_argument("--pools", type=int, nargs="*", default=None, help="The net's --pools when not the default 1 1 0 ...")
    a.add_argument("--fused", action="store_true", help="Run the conv-stack estimator as one fused launch "
                   "(csrc/tapnet.hip) instead of the layered eval forward.")
    a.add_argument("--baseline", choices=CLASSIFIER_KINDS, default=None, help="--estimator is a saved comparison "
                   "baseline of edgeml_amd.baseline --model_dir (af: the Adaptive Feeding SVM, dcsb: the DCSB rule): a "
                   "classifier, offloading where its class is 1; replaces --threshold / --ratio.")
    opts = a.parse_args(argv)
    if opts.baseline:
        given = {"--ratio": opts.ratio is not None, "--estimates": opts.estimates is not None,
                 "--threshold": opts.threshold is not None, "--stage": opts.stage is not None,
                 "--resize": opts.resize is not None, "--pools": opts.pools is not None, "--fused": opts.fused}
        for flag, on in given.items():
            if on:
                raise SystemExit(f"edgeml_amd.offload: --baseline {opts.baseline}: a classifier has no ratio (it "
                                 f"offloads where its class is 1, on the weak detector's output): drop {flag}")
        return opts
    if (opts.threshold is None) == (opts.ratio is None):
        a.error("give either --threshold T or --ratio R with --estimates EST_DIR")
    if opts.ratio is not None and (opts.estimates is None or not 0.0 <= opts.ratio <= 1.0):
        a.error("--ratio R (0..1) needs --estimates EST_DIR")
    if opts.threshold is not None and opts.estimates is not None:
        a.error("--estimates goes with --ratio, not with --threshold")
    return opts


if __name__ == "__main__":
    main(getargs())
    sys.exit(0)
