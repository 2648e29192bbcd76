"""Time the device fit of the random forest regressor (edgeml_amd.rfr: every tree of every fold at once, exact
tree by tree) at COCO-val scale on synthetic data: N images, 80 classes + 5 x 25 box values = 205 stage-24
features.

    python tools/rfr_bench.py [--n 5000] [--folds 5] [--n-estimators 100] [--max-depth 20] [--min-samples-split 100]
    python tools/rfr_bench.py --sklearn            # sklearn's RFR on one fold of the same arrays, CPU, one job

Without a flag: the wall time of fit_rfr on the device (the bootstraps drawn on the host, scaler, standardisation,
the sorts, every level and the estimates of all rows, host packing and copies included), the best of three runs;
then edgedet_rfr_model_predict at B = 32 and 64 on one fold's forest (the cascade's decision), each call timed by
a pair of device events, 20 warm-up calls, 200 timed.  The per-launch times of a level come from a kernel trace
of this script (rocprofv3 --kernel-trace --stats, a run of its own; profiles/rfr_ab.txt).  With --sklearn (no
device): StandardScaler + RandomForestRegressor(n_estimators, max_depth, min_samples_split) on the first fold,
fit and predictions as regression.py's fit_model runs them.  Measured once, not gated.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.gbr_bench import events  # noqa: E402
from tools.regress_bench import synth  # noqa: E402


def time_sklearn(feats, reward, split, a):
    import sklearn
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.preprocessing import StandardScaler
    m = split[0]
    np.random.seed(0)
    t0 = time.perf_counter()
    scaler = StandardScaler().fit(feats[~m])
    reg = RandomForestRegressor(n_estimators=a.n_estimators, max_depth=a.max_depth,
                                min_samples_split=a.min_samples_split)
    reg.fit(scaler.transform(feats[~m]), reward[~m])
    mse = float(np.mean((reward[~m] - reg.predict(scaler.transform(feats[~m]))) ** 2))
    reg.predict(scaler.transform(feats[m]))
    dt = time.perf_counter() - t0
    nodes = sum(e.tree_.node_count for e in reg.estimators_)
    print(f"RFR: sklearn {sklearn.__version__} on the CPU (one job), one fold of {int((~m).sum())} x {feats.shape[1]}, "
          f"{a.n_estimators} trees: {dt:.2f} s (train MSE {mse:.4g}, {nodes} nodes); {len(split)} folds one after "
          f"another: {dt * len(split):.1f} s (scaled, not measured)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--n-estimators", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=20)
    ap.add_argument("--min-samples-split", type=int, default=100)
    ap.add_argument("--sklearn", action="store_true")
    a = ap.parse_args()
    feats, reward, split = synth(a.n, a.folds)
    if a.sklearn:
        return time_sklearn(feats, reward, split, a)
    import torch
    from edgeml_amd import rfr
    opts = rfr.RFROpt(n_estimators=a.n_estimators, max_depth=a.max_depth, min_samples_split=a.min_samples_split)
    rfr.fit_rfr(feats[:600], reward[:600], split[:, :600], rfr.RFROpt(n_estimators=10))  # warm: library load, allocator
    torch.cuda.synchronize()
    times, device = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        res, info = rfr.fit_rfr(feats, reward, split, opts)
        times.append(time.perf_counter() - t0)
        device.append(info["fit_time"])
    mse = [float(np.mean((reward[~m] - r["train_est"]) ** 2)) for m, r in zip(split, res)]
    launches = 1 + 2 * a.max_depth + a.folds
    print(f"RFR: {a.folds} folds, N={a.n}, D={feats.shape[1]}, {a.n_estimators} trees per fold, max_depth {a.max_depth}, "
          f"min_samples_split {a.min_samples_split}: {min(times):.4f} s (runs {[round(t, 4) for t in times]}: the "
          f"bootstraps on the host, host packing, sorts and copies included; from the upload on "
          f"{[round(t, 4) for t in device]}); {launches} launches, {info['groups']} scan workgroups per tree; train MSE "
          f"{[float('%.4g' % v) for v in mse]}; nodes {info['node_count'].sum(1).tolist()}, deepest tree "
          f"{int(info['node_count'].max())} nodes, tied {info['tied_nodes'].tolist()}, q {info['q'].tolist()}")
    model = rfr.load(rfr.model_data(info, 0)).to("cuda")
    print("    call                                         B    median     min      p90   (us)")
    for B in (32, 64):
        x = torch.from_numpy(np.ascontiguousarray(feats[:B], dtype=np.float64)).cuda()
        est = torch.empty(B, dtype=torch.float64, device="cuda")
        med, lo, p90 = events(lambda: model.predict_into(x, est))
        print(f"    edgedet_rfr_model_predict, T = {a.n_estimators:<6d}          {B:3d}  {med:8.2f} {lo:8.2f} {p90:8.2f}")


if __name__ == "__main__":
    main()
