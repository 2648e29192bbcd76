"""The producer of the weak detector's hidden-layer feature maps: SSDLite's backbone stages written in the layout
lib/data.py load_feature (and edgeml_amd.convnet --weak ssd) reads.

    python -m edgeml_amd.maps img_dir feature_dir --stages N [N ...] [--model ssd] [--model-path P]
           [--dataset coco|voc] [--batch N] [--decode gpu|host] [--save-dir DIR]

Writes feature_dir/<image>/stage{N}_{token}_features.npy, float32 [C, H, W], for every image and every stage N of
--stages.  The stages and their tokens are the library's stage table (edgeml_amd.tapnet.stage_table, csrc/lower.hip):
1-15 the InvertedResidual blocks of mobilenet_v3_large.features ("IR"), 16 its last 1x1 conv ("Conv"), 17-20
backbone.extra.0-3 ("Extra").  Stage 0, the stem conv, has no buffer under the default fused stem.

The detector runs the detect CLI's batches (detect.image_sizes / distributed.size_batches /
detect._decoded_batches).  SSDLite's plan writes every block's output into its own named NHWC buffer and never
reuses one, so after a batch's replay a run_batches post hook copies each chain's tapped buffers to pinned host
memory on the batch's stream; writer threads transpose and save them.  With --save-dir the weak detections are
written in the same pass, the detect CLI's bytes.
"""
import argparse
import concurrent.futures as cf
import os
import sys
from pathlib import Path

import numpy as np
import torch

from . import fmt, tapnet


def save_map(feature_dir, img_name, stage, token, hwc):
    """One [H, W, C] map as feature_dir/<image>/stage{N}_{token}_features.npy, float32 [C, H, W]."""
    d = os.path.join(feature_dir, fmt.output_name(img_name))
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"stage{stage}_{token}_features.npy")
    tmp = path + ".tmp.npy"
    np.save(tmp, np.ascontiguousarray(np.asarray(hwc, np.float32).transpose(2, 0, 1)))
    os.replace(tmp, path)  # never leave a partial file behind
    return path


class MapHook:
    """The run_batches post hook: the tapped buffers of `stages`, chain by chain, into pinned [B, H, W, C] host
    tensors owned by the slot."""

    def __init__(self, stages):
        self.stages = list(stages)

    def __call__(self, plan, sl, stream, tag):
        buf = sl.get("maps")
        if buf is None or buf["key"] != (plan.B, tuple(self.stages)):
            m = plan.model
            buf = sl["maps"] = {"key": (plan.B, tuple(self.stages)), "taps": {}, "host": {}, "token": {}}
            for s in self.stages:
                taps = tapnet.stage_table(m.num_classes, m.reduced_tail, plan.B, plan.H, plan.W, plan.u8, s)
                buf["taps"][s] = [(t, plan.buffer(t.buffer).tensor()) for t in taps]
                buf["token"][s] = taps[0].token
                buf["host"][s] = torch.empty((plan.B, taps[0].H, taps[0].W, taps[0].C), dtype=torch.float32,
                                             pin_memory=True)
        for s in self.stages:
            for t, x in buf["taps"][s]:
                buf["host"][s][t.image0:t.image0 + t.images].copy_(x, non_blocking=True)
        sl["post"] = {f"stage{s}": buf["host"][s] for s in self.stages}
        sl["post"]["tokens"] = dict(buf["token"])


def run(img_dir, stages, model="ssd", model_path="", dataset="coco", batch=0, decode="gpu", on_map=None, on_rows=None,
        device="cuda:0"):
    """Run the weak detector over img_dir; on_map(name, stage, token, [H, W, C] array) for every image and stage,
    on_rows(name, rows) for every image's detections.  model: the detect CLI's name, or an SSDLite320."""
    from . import detect, distributed as dist_mod
    if not torch.cuda.is_available():
        raise RuntimeError("edgeml_amd.maps needs an MI355X (HIP) device; there is no CPU path")
    torch.cuda.set_device(device)
    det_classes = 91 if dataset == "coco" else 21
    weak = model if not isinstance(model, str) else detect.load_weak_models(model, model_path, det_classes).to(device).eval()
    data = detect.ObjectDetectionDataset(img_dir)
    sizes = detect.image_sizes(data)
    chunks = dist_mod.size_batches(sizes, min(batch or weak.max_batch, weak.max_batch))
    tagged = (((nm, hw), buf) for nm, hw, buf in
              detect._decoded_batches(data, chunks, sizes, device_decode=decode == "gpu"))
    for (nm, (h, w)), counts, boxes, scores, labels, ex in weak.run_batches(tagged, raw=True, post=MapHook(stages)):
        if on_rows is not None:
            for name, r in zip(nm, fmt.format_batch(boxes, scores, labels, counts, h, w, dataset)):
                on_rows(name, r)
        for s in stages:
            arr = ex[f"stage{s}"]
            for j, name in enumerate(nm):
                on_map(name, s, ex["tokens"][s], arr[j])
    return list(data.img_names)


def check_args(opts):
    """Refuse what the table does not have, naming it."""
    if opts.model != "ssd":
        raise SystemExit(f"edgeml_amd.maps: --model {opts.model}: only SSDLite (--model ssd) has a stage table; the "
                         "YOLOv5 maps of the reference are out of scope")
    for s in opts.stages:
        try:
            tapnet.stage_info(s)
        except ValueError as e:
            raise SystemExit(f"edgeml_amd.maps: --stages {s}: not in SSDLite's stage table (edgeml_amd.tapnet."
                             f"stage_table: 1-16 mobilenet_v3_large.features, 17-20 backbone.extra): {e}") from None
    if len(set(opts.stages)) != len(opts.stages):
        raise SystemExit("edgeml_amd.maps: --stages: a stage is given twice")


def main(opts):
    from .distributed import usable_cpus
    check_args(opts)
    Path(opts.feature_dir).mkdir(parents=True, exist_ok=True)
    if opts.save_dir:
        Path(opts.save_dir).mkdir(parents=True, exist_ok=True)
    with cf.ThreadPoolExecutor(usable_cpus()) as writers:
        pending = []
        on_map = lambda name, s, token, a: pending.append(  # noqa: E731
            writers.submit(save_map, opts.feature_dir, name, s, token, a))
        on_rows = (lambda name, r: pending.append(writers.submit(fmt.save_npy, opts.save_dir, name, r))) \
            if opts.save_dir else None
        names = run(opts.img_dir, opts.stages, opts.model, opts.model_path, opts.dataset, opts.batch, opts.decode,
                    on_map, on_rows)
        for f in pending:
            f.result()  # re-raise a failed write
    print(f"wrote stages {opts.stages} of {len(names)} images to {opts.feature_dir}")
    return names


def getargs(argv=None):
    a = argparse.ArgumentParser(prog="edgeml_amd.maps")
    a.add_argument("img_dir", help="Directory of the images.")
    a.add_argument("feature_dir", help="Directory for <image>/stage{N}_{token}_features.npy.")
    a.add_argument("--stages", type=int, nargs="+", required=True, help="Stages of SSDLite's stage table (1-20).")
    a.add_argument("--dataset", type=str, default="coco")
    a.add_argument("--model", type=str, default="ssd")
    a.add_argument("--model-path", type=str, default="")
    a.add_argument("--batch", type=int, default=0, help="Images per engine call (0 = model default).")
    a.add_argument("--decode", choices=("gpu", "host"), default="gpu")
    a.add_argument("--save-dir", type=str, default="", help="Also write the weak detections (<name>.npy) here.")
    return a.parse_args(argv)


if __name__ == "__main__":
    main(getargs())
    sys.exit(0)
