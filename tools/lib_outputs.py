"""Detections of fixed synthetic batches under the library EDGEDET_LIB names, for bit-identity checks
between two builds of libedgedet.so (a change meant to keep the arithmetic, e.g. a new epilogue).

    EDGEDET_LIB=.../libedgedet_a.so python tools/lib_outputs.py -o a.npz
    EDGEDET_LIB=.../libedgedet_b.so python tools/lib_outputs.py -o b.npz --compare a.npz

SSDLite at the bench batch (32, two chains) and FRCNN at batch 8, seeded weights and images
(edgeml_amd.synthetic); --compare prints, per model and field, whether every value is bit-identical
and the largest difference, and exits 1 on any difference.

--convs adds the raw outputs of ops.conv2d_nhwc on every conv tile (a change to csrc/conv.hip meant to
keep the arithmetic): the small ragged shapes of tests/test_gpu_conv_views.py on seeded inputs, each
case plain and with an SE in_scale, compared the same way, one line per case."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgeml_amd import models, ops, synthetic  # noqa: E402
from edgeml_amd.plan import pack_conv_weight  # noqa: E402

# name: (B, H, W, Cin, Cout, k, stride, act), the shapes P, Q, S, Q32 of tests/test_gpu_conv_views.py
# (M = 297 and smaller: ragged against every tile, a batch boundary inside an MFMA block, two M tiles
# of the 256-row tiles)
CONV_SHAPES = {"P": (3, 11, 9, 24, 40, 1, 1, "HS"), "Q": (3, 11, 9, 16, 136, 3, 1, "RE"),
               "S": (2, 13, 10, 8, 24, 3, 2, None), "Q32": (3, 11, 9, 32, 136, 3, 1, "RE")}
W3_TILES = [21, 22, 23, 24, 25, 27, 28, 29, 30, 31, 32, 38, 39]  # bf16x6: take the split weight planes


def conv_cases():
    """(tile, shape, with split planes, presplit input, activation override)."""
    for shape in "PQS":
        yield 0, shape, False, False, ...
        yield 0, shape, True, False, ...
        for t in [1, 2, 3, 4, 5, 6] + W3_TILES:
            yield t, shape, t in W3_TILES, False, ...
    for t in [10, 11, 12, 13, 14, 15, 16, 17, 33, 34, 35]:  # the pointwise families: 1x1 dense inputs
        yield t, "P", False, False, ...
    yield 25, "Q32", True, True, ...
    yield 26, "Q", True, False, None  # split-K: no activation, into a zeroed output


def run_convs():
    out = {}
    dev = "cuda:0"
    data = {}
    for name, (B, H, W, Cin, Cout, k, s, act) in CONV_SHAPES.items():
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        wp = torch.from_numpy(pack_conv_weight(w.numpy())[0]).to(dev)
        data[name] = dict(x=torch.randn(B, H, W, Cin, generator=g).to(dev), wp=wp, w3=ops.split_bf16x3(wp),
                          b=(torch.randn(Cout, generator=g) * 0.1).to(dev), sc=torch.rand(B, Cin, generator=g).to(dev))
    for tile, name, w3, presplit, act in conv_cases():
        B, H, W, Cin, Cout, k, s, shape_act = CONV_SHAPES[name]
        d = data[name]
        for se in (False, True):
            key = f"conv/{tile}{'w' if w3 and tile == 0 else ''}/{name}{'/presplit' if presplit else ''}{'/se' if se else ''}"
            y = ops.conv2d_nhwc(d["x"], d["wp"], d["b"], Cout, k, s, (k - 1) // 2, shape_act if act is ... else act,
                                tile=tile, in_scale=d["sc"] if se else None, w3=d["w3"] if w3 else None,
                                presplit=presplit)
            torch.cuda.synchronize()
            out[key] = y.cpu().numpy()
    return out


def run():
    out = {}
    dev = "cuda:0"
    cases = [("ssd", lambda sd: models.SSDLite320(sd, 91, True), 32, 11),
             ("faster_rcnn", lambda sd: models.FasterRCNNFPNv2(sd, 91), 8, 23)]
    for kind, make, b, seed in cases:
        sd = synthetic.synthetic_state_dict(kind, 91, True, seed=0)
        model = make(sd).to(dev)
        imgs = synthetic.make_batch_u8(b, 640, 640, seed=seed).to(dev)
        got = model(imgs.float() / 255)
        torch.cuda.synchronize()
        for i, g in enumerate(got):
            for k in ("boxes", "scores", "labels"):
                out[f"{kind}/{i}/{k}"] = g[k].detach().cpu().numpy()
        del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--convs", action="store_true")
    a = ap.parse_args()
    out = run()
    if a.convs:
        out.update(run_convs())
    np.savez(a.out, **out)
    if not a.compare:
        return 0
    ref = np.load(a.compare)
    bad = 0
    for kind in ["ssd", "faster_rcnn"] + [k for k in out if k.startswith("conv/")]:
        keys = [kind] if kind in out else [k for k in out if k.startswith(kind + "/")]
        same = all(k in ref and out[k].shape == ref[k].shape and np.array_equal(out[k], ref[k]) for k in keys)
        dmax = max((float(np.abs(out[k].astype(np.float64) - ref[k].astype(np.float64)).max())
                    for k in keys if k in ref and out[k].shape == ref[k].shape and out[k].size), default=0.0)
        print(f"{kind}: {len(keys)} arrays, bit-identical={same}, max |diff| {dmax:.3g}")
        bad += not same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
