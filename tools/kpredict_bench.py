"""Time prediction from a saved SVR / KNR model (csrc/kpredict.hip) on the decision chain's batch sizes, on
synthetic data at the flagship width D = 205 (80 classes + 5 x 25 box values):

  SVR  n = 1,350 support vectors (the count DESIGN 6d measured at 5,000 images), B = 32 and 64 rows, against
       edgedet_svr_predict on the same rows over a one-fold fit workspace holding the same model: the only way
       to those numbers before, two waves walking the support vectors one tile after another;
  KNR  n = 4,000 training rows, k = 500, B = 32 and 64 rows.

    python tools/kpredict_bench.py [--warmup 20] [--calls 200]

Each call is timed by a pair of device events on the current stream; the figure is the median.  One JSON line
per measurement, and the largest difference between the old and the new SVR estimates (a reordered sum: last
bits).  Needs the device: there is nothing to time without one.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 205


def synth(n, seed):
    rng = np.random.default_rng(seed)
    mean, scale = rng.normal(0, 1, D), rng.uniform(0.5, 2, D)
    return mean, scale, mean + scale * rng.normal(0, 1, (n, D)), rng


def timed(call, warmup, calls):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.sort(ms)
    return {"median_us": round(float(np.median(ms)) * 1e3, 2), "min_us": round(float(ms[0]) * 1e3, 2),
            "p90_us": round(float(ms[int(0.9 * (len(ms) - 1))]) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    from edgeml_amd import kpredict, ops
    if not torch.cuda.is_available():
        raise SystemExit("tools/kpredict_bench.py needs an MI355X (HIP) device")
    dev, L, p = "cuda:0", ops.lib(), ops._ptr
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731

    # ------------------------------------------------------------------------------------------ SVR
    n = 1350
    mean, scale, rows, rng = synth(n, 1)
    svr = kpredict.KernelModel("svr", mean, scale, rows, rng.uniform(-0.05, 0.05, n), gamma=1.0 / D,
                               intercept=0.5).to(dev)
    d = svr._dev
    # the fit's workspace of one fold holding this model: Z [n][D], then |z|^2 [n] (csrc/svr.hip)
    fit_ws = torch.cat([d["z"].reshape(-1), d["norm"]]).contiguous()
    off_host = (ctypes.c_int64 * 2)(0, n)
    off, icpt, gam = t(np.array([0, n], np.int64)), t(np.array([0.5])), t(np.array([1.0 / D]))
    for B in (32, 64):
        x = t(mean + scale * rng.normal(0, 1, (B, D)))
        est_new = torch.empty(B, dtype=torch.float64, device=dev)
        est_old = torch.empty(B, dtype=torch.float64, device=dev)
        ws = torch.empty(svr.workspace_bytes(B), dtype=torch.uint8, device=dev)

        def new():
            svr.predict_into(x, est_new, ws)

        def old():
            ops.check(L.edgedet_svr_predict(p(x), B, D, p(d["mean"]), p(d["scale"]), off_host, p(off), 1, p(fit_ws),
                                            fit_ws.numel() * 8, p(d["weight"]), p(icpt), p(gam), p(est_old),
                                            ops.stream_handle()))

        r_old, r_new = timed(old, a.warmup, a.calls), timed(new, a.warmup, a.calls)
        diff = float((est_new - est_old).abs().max())
        print(json.dumps({"what": "svr_model_predict", "n": n, "D": D, "B": B, **r_new}))
        print(json.dumps({"what": "svr_predict (fit workspace)", "n": n, "D": D, "B": B, **r_old,
                          "max_abs_diff_new_old": diff}))

    # ------------------------------------------------------------------------------------------ KNR
    n, k = 4000, 500
    mean, scale, rows, rng = synth(n, 2)
    knr = kpredict.KernelModel("knr", mean, scale, rows, rng.normal(0, 1, n), n_neighbors=k).to(dev)
    for B in (32, 64):
        x = t(mean + scale * rng.normal(0, 1, (B, D)))
        est = torch.empty(B, dtype=torch.float64, device=dev)
        ws = torch.empty(knr.workspace_bytes(B), dtype=torch.uint8, device=dev)
        r = timed(lambda: knr.predict_into(x, est, ws), a.warmup, a.calls)
        print(json.dumps({"what": "knn_model_predict", "n": n, "k": k, "D": D, "B": B, **r}))


if __name__ == "__main__":
    main()
