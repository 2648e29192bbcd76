"""Timing of the two baseline policies in the cascade's weak stage: edgeml_amd.offload with
--baseline dcsb (rows -> edgedet_offload_dcsb) and --baseline af (rows -> features -> edgedet_offload_svm) against
an LR estimator (rows -> features -> edgedet_offload_decide), nothing offloaded.  Nothing is asserted.

    python tools/cascade_rules_bench.py [--out FILE] [--images 1024] [--rounds 5] [--calls 200]

Decision steps alone: B = 32 images of K = 300 rows on the device; after a warm-up the three chains (everything
between the formatter and the pack) alternate, `--rounds` windows of `--calls` calls each, timed by device events
and by the host clock to the synchronise.  Weak stage: offload.run on `--images` seeded synthetic JPEGs in weak
batches of 32 with models that offload nothing (a DCSB rule with conf_thresh 0.5, whose two counts are always
equal; an SVM with a bias of -1e30; the LR estimator under a threshold of 1e30), the three alternating, the first
round of each as warm-up; the figure is run()'s "engine" host seconds (decode, weak model, hook, result copies).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 205


def estimators():
    from edgeml_amd import offload
    rng = np.random.default_rng(5)
    v = np.zeros(208)
    v[:D], v[D] = rng.normal(0, 1, D), -1e30
    return {"baseline dcsb": (offload.Estimator("dcsb", 0, conf_thresh=0.5, num_thresh=5, area_thresh=0.4), 0.0),
            "baseline af": (offload.Estimator("af", D, v=v), 0.0),
            "LR estimator": (offload.Estimator("linear", D, mean=rng.normal(0, 1, D), scale=rng.uniform(0.5, 2, D),
                                               coef=rng.normal(0, 1, D), intercept=0.5), 1e30)}


def summary(say, name, v, unit, extra=""):
    v = sorted(v)
    say(f"  {name:14s} median {v[len(v) // 2]:9.2f} {unit} (min {v[0]:.2f}, max {v[-1]:.2f}){extra}")


def steps_alone(rounds, calls, say):
    from edgeml_amd import offload
    B, K = 32, 300
    rng = np.random.default_rng(6)
    rows = np.column_stack([rng.integers(0, 80, B * K).astype(np.float64), rng.uniform(0.2, 0.8, (B * K, 2)),
                            rng.uniform(0.05, 1.0, (B * K, 2)), rng.uniform(0, 1, B * K)]).reshape(B, K, 6)
    dev = "cuda:0"
    g_rows = torch.from_numpy(rows).to(dev)
    g_nrow = torch.from_numpy(rng.integers(0, K + 1, B).astype(np.int32)).to(dev)
    feat = torch.zeros((B, D), dtype=torch.float64, device=dev)
    est, flag = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    ests = estimators()

    def chain(name):
        e, thr = ests[name]
        if e.kind == "dcsb":
            e.decide(None, thr, est, flag, rows=g_rows, nrow=g_nrow)
        else:
            offload.row_features(g_rows, g_nrow, 80, 25, feat)
            e.decide(feat, thr, est, flag)

    say(f"decision steps alone: B {B}, K {K}, {D} features; {calls} calls per window")
    for name in ests:  # warm-up: code objects, the models' uploads
        for _ in range(20):
            chain(name)
    torch.cuda.synchronize()
    res = {name: [] for name in ests}
    for r in range(rounds):
        for name in ests:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                chain(name)
            b.record()
            torch.cuda.synchronize()
            host = (time.perf_counter() - t0) / calls * 1e6
            d = a.elapsed_time(b) / calls * 1e3
            res[name].append(d)
            say(f"  round {r} {name:14s}: {d:8.2f} us/call device events, {host:8.2f} us/call host to the synchronise")
    for name, v in res.items():
        summary(say, name, v, "us/call")


def weak_stage(images, rounds, say):
    from PIL import Image
    from edgeml_amd import detect, offload, synthetic
    ests = estimators()
    with tempfile.TemporaryDirectory() as d:
        scenes = [Image.fromarray(synthetic.make_scene(9000 + i, 480, 640).transpose(1, 2, 0)) for i in range(16)]
        for i in range(images):
            scenes[i % 16].save(os.path.join(d, f"{i:012d}.jpg"))
        weak = detect.load_weak_models("ssd", "", 91).to("cuda:0")
        say(f"weak stage: {images} JPEGs of 480 x 640, weak batch 32, nothing offloaded; engine seconds of offload.run, "
            f"round 0 is the warm-up")
        res = {k: [] for k in ests}
        for r in range(rounds + 1):
            for k, (e, thr) in ests.items():
                out = offload.run(d, e, thr, weak=weak, weak_batch=32)
                assert not out["offloaded"].any()
                s = out["seconds"]["engine"]
                if r:
                    res[k].append(s * 1e3)
                say(f"  round {r} {k:14s}: {s * 1e3:9.2f} ms  ({images / s:9.1f} img/s)")
        for k, v in res.items():
            summary(say, k, v, "ms", f", {sorted(v)[len(v) // 2] / (images / 32):.3f} ms per weak batch")


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--out", default="")
    a.add_argument("--images", type=int, default=1024)
    a.add_argument("--rounds", type=int, default=5)
    a.add_argument("--calls", type=int, default=200)
    opts = a.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/cascade_rules_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}")
    steps_alone(opts.rounds, opts.calls, say)
    weak_stage(opts.images, opts.rounds, say)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
