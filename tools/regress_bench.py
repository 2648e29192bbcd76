"""Time the device fits of the four estimator regressors (edgeml_amd.regress: every fold at once) at COCO-val
scale on synthetic data: N images, 80 classes + 5 x 25 box values = 205 stage-24 features.

    python tools/regress_bench.py [--n 5000] [--folds 5]
    python tools/regress_bench.py --reference DIR      # the reference's fit_model on the same arrays, on the CPU

Without --reference: the wall time of each fit on the device (scaler, Gram, solver and the predictions of all
rows, host packing and copies included), the best of three runs.  With --reference DIR (a checkout of the
reference project; needs sklearn, no device): regression.py's fit_LR / fit_EN / fit_BR / fit_KNR over the same
folds, one after the other as its main() runs them.  Measured once, not gated.
"""
import argparse
import contextlib
import io
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NUM_CLASS, K = 80, 25
MODELS = ("LR", "EN", "BR", "KNR")


def synth(n, folds, seed=0):
    rng = np.random.default_rng(seed)
    feats = np.zeros((n, NUM_CLASS + 5 * K))
    for i in range(n):
        m = min(K, 1 + rng.poisson(17))
        conf = np.sort(rng.uniform(0.05, 0.95, m))[::-1]
        w, h = rng.uniform(0.1, 1.0, m), rng.uniform(0.1, 1.0, m)
        x, y = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
        np.add.at(feats[i], rng.integers(0, NUM_CLASS, m), 1)
        rows = np.stack([x, y, w, h, conf], 1)
        feats[i, NUM_CLASS:NUM_CLASS + rows.size] = rows.reshape(-1)
    reward = (0.15 * (feats[:, NUM_CLASS + 4] - 0.5) - 0.02 * feats[:, :8].sum(1) + 0.1 * feats[:, NUM_CLASS + 7]
              + 0.05 * rng.normal(0, 1, n))
    fold = rng.permutation(np.arange(n) % folds)
    return feats, reward, np.stack([fold == f for f in range(folds)])


def time_reference(ref_dir, feats, reward, split):
    for name in ("matplotlib", "matplotlib.pyplot", "torchvision", "torchvision.ops"):
        sys.modules.setdefault(name, types.ModuleType(name))  # imported by the reference, unused by these fits
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["torchvision.ops"].roi_align = sys.modules["torchvision.ops"].roi_pool = None
    sys.path.insert(0, ref_dir)
    import regression
    fits = {"LR": regression.fit_LR, "EN": regression.fit_EN, "BR": regression.fit_BR, "KNR": regression.fit_KNR}
    for name in MODELS:
        t0 = time.perf_counter()
        for m in split:
            data = ([f for f in feats[~m]], [f for f in feats[m]], reward[~m], reward[m])
            with contextlib.redirect_stdout(io.StringIO()):
                fits[name](data)
        print(f"{name}: reference fit_model on the CPU, {len(split)} folds, N={len(feats)}: "
              f"{time.perf_counter() - t0:.4f} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--reference", type=str, default="")
    a = ap.parse_args()
    feats, reward, split = synth(a.n, a.folds)
    if a.reference:
        return time_reference(a.reference, feats, reward, split)
    import torch
    from edgeml_amd import regress
    for name in MODELS:  # warm: library load, allocator
        regress.FITS[name](feats[:600], reward[:600], split[:, :600], regress.KNROpt(7) if name == "KNR" else None)
    torch.cuda.synchronize()
    for name in MODELS:
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            res, info = regress.FITS[name](feats, reward, split)
            times.append(time.perf_counter() - t0)
        mse = [float(np.mean((reward[~m] - r["train_est"]) ** 2)) for m, r in zip(split, res)]
        extra = {"LR": lambda: f"rank {info['rank'].tolist()}, Jacobi sweeps {info['eigh_sweeps'].tolist()}",
                 "BR": lambda: f"n_iter {info['n_iter'].tolist()}, Jacobi sweeps {info['eigh_sweeps'].tolist()}",
                 "EN": lambda: f"sweeps {info['sweeps'].tolist()}, |z| {[float('%.2g' % z) for z in info['znorm']]}",
                 "KNR": lambda: f"n_neighbors {info['n_neighbors']}"}[name]()
        print(f"{name}: {a.folds} folds, N={a.n}: {min(times):.4f} s (runs {[round(t, 4) for t in times]}, host packing "
              f"and copies included); train MSE {[float('%.4g' % v) for v in mse]}; {extra}")


if __name__ == "__main__":
    main()
