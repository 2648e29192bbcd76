"""Time the device fit of the gradient boosting regressor (edgeml_amd.gbr: every fold at once, exact to the tree)
at COCO-val scale on synthetic data: N images, 80 classes + 5 x 25 box values = 205 stage-24 features.

    python tools/gbr_bench.py [--n 5000] [--folds 5] [--n-estimators 1000] [--max-depth 3]
    python tools/gbr_bench.py --sklearn [--sklearn-stages 50]   # sklearn's GBR on one fold of the same arrays, CPU

Without --sklearn: the wall time of fit_gbr on the device (scaler, standardisation, the sorts, every stage and the
estimates of all rows, host packing and copies included), the best of three runs, and that time per launch;
then edgedet_gbr_model_predict at B = 32 and 64 on one fold's trees (the cascade's decision), each call timed
by a pair of device events, 20 warm-up calls, 200 timed.  With --sklearn (no device): StandardScaler +
GradientBoostingRegressor(learning_rate=0.1, subsample=1.0) at --sklearn-stages stages on the first fold, fit and
predictions as regression.py's fit_model runs them, and that time scaled linearly to --n-estimators stages and
--folds folds: a scaled figure, not a measured one.  Measured once, not gated.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.regress_bench import synth  # noqa: E402


def time_sklearn(feats, reward, split, stages, T):
    import sklearn
    from sklearn.ensemble import GradientBoostingRegressor
    from sklearn.preprocessing import StandardScaler
    m = split[0]
    t0 = time.perf_counter()
    scaler = StandardScaler().fit(feats[~m])
    reg = GradientBoostingRegressor(learning_rate=0.1, n_estimators=stages, subsample=1.0)
    reg.fit(scaler.transform(feats[~m]), reward[~m])
    mse = float(np.mean((reward[~m] - reg.predict(scaler.transform(feats[~m]))) ** 2))
    reg.predict(scaler.transform(feats[m]))
    dt = time.perf_counter() - t0
    print(f"GBR: sklearn {sklearn.__version__} on the CPU, one fold of {int((~m).sum())} x {feats.shape[1]}, {stages} "
          f"stages: {dt:.2f} s (train MSE {mse:.4g}); scaled linearly to {T} stages: {dt * T / stages:.0f} s per fold, "
          f"{dt * T / stages * len(split):.0f} s for {len(split)} folds (scaled, not measured)")


def events(call, warm=20, reps=200):
    import torch
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    us = np.sort(us)
    return float(np.median(us)), float(us[0]), float(us[int(0.9 * len(us))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--n-estimators", type=int, default=1000)
    ap.add_argument("--max-depth", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-stages", type=int, default=50)
    a = ap.parse_args()
    feats, reward, split = synth(a.n, a.folds)
    if a.sklearn:
        return time_sklearn(feats, reward, split, a.sklearn_stages, a.n_estimators)
    import torch
    from edgeml_amd import gbr
    opts = gbr.GBROpt(n_estimators=a.n_estimators, max_depth=a.max_depth)
    gbr.fit_gbr(feats[:600], reward[:600], split[:, :600], gbr.GBROpt(n_estimators=20))  # warm: library load, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        res, info = gbr.fit_gbr(feats, reward, split, opts)
        times.append(time.perf_counter() - t0)
    mse = [float(np.mean((reward[~m] - r["train_est"]) ** 2)) for m, r in zip(split, res)]
    launches = a.n_estimators * (2 * a.max_depth + 1) + 1
    print(f"GBR: {a.folds} folds, N={a.n}, D={feats.shape[1]}, {a.n_estimators} stages of depth {a.max_depth}: "
          f"{min(times):.4f} s (runs {[round(t, 4) for t in times]}, host packing, sorts and copies included); "
          f"{launches} launches, {min(times) / launches * 1e6:.2f} us of wall time per launch; train MSE "
          f"{[float('%.4g' % v) for v in mse]}; split nodes {info['nodes'].sum(1).tolist()}, tied "
          f"{info['tied_nodes'].tolist()}, q {info['q'].tolist()}")
    model = gbr.load(gbr.model_data(info, 0)).to("cuda")
    print("    call                                         B    median     min      p90   (us)")
    for B in (32, 64):
        x = torch.from_numpy(np.ascontiguousarray(feats[:B], dtype=np.float64)).cuda()
        est = torch.empty(B, dtype=torch.float64, device="cuda")
        med, lo, p90 = events(lambda: model.predict_into(x, est))
        print(f"    edgedet_gbr_model_predict, T = {a.n_estimators:<6d}          {B:3d}  {med:8.2f} {lo:8.2f} {p90:8.2f}")


if __name__ == "__main__":
    main()
