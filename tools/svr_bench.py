"""Time the device fits of SVR and LinearSVR (edgeml_amd.svr: every fold at once, each solved to its certified
optimum) at COCO-val scale on synthetic data: N images, 80 classes + 5 x 25 box values = 205 stage-24 features.

    python tools/svr_bench.py [--n 5000] [--folds 5] [--models SVR,LSVR] [--lsvr-tol-rel 1e-4] [--max-sweeps 10000]
    python tools/svr_bench.py --sklearn        # sklearn's SVR / LinearSVR on the same arrays, on the CPU

Without --sklearn: the wall time of each fit on the device (scaler, kernel matrix, solver and the predictions of
all rows, host packing and copies included), the best of three runs.  With --sklearn (no device): StandardScaler
+ SVR(kernel='rbf', C=0.05, epsilon=0.05) / LinearSVR(C=0.005, epsilon=0.005), regression.py's options, fitted
and predicting fold after fold as its main() runs them; these stop at sklearn's tol (1e-3 / 1e-4), the device
at its own (a KKT violation of 1e-9 / a duality gap of 1e-10 P(0)), so the two columns are not the same amount
of work.  Measured once, not gated.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.regress_bench import synth  # noqa: E402

MODELS = ("SVR", "LSVR")


def time_sklearn(feats, reward, split):
    import warnings
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVR, LinearSVR
    make = {"SVR": lambda: SVR(kernel="rbf", C=0.05, epsilon=0.05), "LSVR": lambda: LinearSVR(C=0.005, epsilon=0.005)}
    for name in MODELS:
        t0 = time.perf_counter()
        mse = []
        for m in split:
            scaler = StandardScaler().fit(feats[~m])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                reg = make[name]().fit(scaler.transform(feats[~m]), reward[~m])
            mse.append(float(np.mean((reward[~m] - reg.predict(scaler.transform(feats[~m]))) ** 2)))
            reg.predict(scaler.transform(feats[m]))
        print(f"{name}: sklearn on the CPU, {len(split)} folds, N={len(feats)}: {time.perf_counter() - t0:.4f} s; "
              f"train MSE {[float('%.4g' % v) for v in mse]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--max-sweeps", type=int, default=10000, help="LinearSVR sweeps before the run is given up")
    ap.add_argument("--max-iter", type=int, default=2000000, help="SVR iterations before the run is given up")
    ap.add_argument("--lsvr-tol-rel", type=float, default=None, help="LinearSVR gap tolerance / P(0) (default: the fit's)")
    ap.add_argument("--models", type=str, default=",".join(MODELS))
    a = ap.parse_args()
    models = [m for m in MODELS if m in a.models.split(",")]
    feats, reward, split = synth(a.n, a.folds)
    if a.sklearn:
        return time_sklearn(feats, reward, split)
    import torch
    from edgeml_amd import svr
    opts = {"SVR": svr.SVROpt(max_iter=a.max_iter), "LSVR": svr.LSVROpt(max_sweeps=a.max_sweeps)}
    if a.lsvr_tol_rel is not None:
        opts["LSVR"].tol_rel = a.lsvr_tol_rel
    for name in models:  # warm: library load, allocator
        svr.FITS[name](feats[:600], reward[:600], split[:, :600], opts[name])
    torch.cuda.synchronize()
    for name in models:
        times = []
        try:
            for _ in range(3):
                t0 = time.perf_counter()
                res, info = svr.FITS[name](feats, reward, split, opts[name])
                times.append(time.perf_counter() - t0)
                if sum(times) > 30.0:  # a long solve is timed once
                    break
        except RuntimeError as e:
            print(f"{name}: {a.folds} folds, N={a.n}: gave up after {time.perf_counter() - t0:.4f} s: {e}")
            continue
        mse = [float(np.mean((reward[~m] - r["train_est"]) ** 2)) for m, r in zip(split, res)]
        extra = {"SVR": lambda: f"iterations {info['iterations'].tolist()}, violation "
                                f"{[float('%.2g' % v) for v in info['violation']]}, support vectors "
                                f"{[int(np.count_nonzero(b)) for b in info['beta']]}",
                 "LSVR": lambda: f"sweeps {info['sweeps'].tolist()}, gap {[float('%.2g' % v) for v in info['gap']]}, "
                                 f"tol {[float('%.2g' % v) for v in info['tol']]}"}[name]()
        print(f"{name}: {a.folds} folds, N={a.n}: {min(times):.4f} s (runs {[round(t, 4) for t in times]}, host packing "
              f"and copies included); train MSE {[float('%.4g' % v) for v in mse]}; {extra}")


if __name__ == "__main__":
    main()
