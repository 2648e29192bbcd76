"""Drop-in for baseline.py: the two comparison baselines of the paper's headline plot, fitted on the
GPU with every cross-validation fold in flight (csrc/baseline.hip).

    python -m edgeml_amd.baseline data_dir reward_path split_path save_dir
           [--baseline af|dcsb] [--positive_weight 3.0] [--label_dir D] [--model_dir D]

Same arguments, defaults and files as baseline.py:161-226.  The reward is binarised as reward > 0.

* ``af`` (Adaptive Feeding, baseline.py:29-64): a linear SVM on the stage-24 output features
  (<data_dir>/<image>/stage24_output_features.npy, edgeml_amd.features writes them).  The reference
  fits sklearn's LinearSVC(dual=False, class_weight={0: 1, 1: w}); here the same strongly convex
  objective, f(v) = 1/2 |v|^2 + sum_i C_i max(0, 1 - s_i v.(x_i, 1))^2 with the bias regularised
  (intercept_scaling = 1), is solved on the device by a damped Newton method in float64 down to
  |grad f| <= 1e-8, so the model is the unique optimum liblinear approaches.  Writes
  <save_dir>/<positive_weight>/estimate{k}.npz and, with --model_dir,
  <model_dir>/<positive_weight>/wts{k}.pickle = {"coef", "intercept", "classes": [0, 1],
  "positive_weight"}: plain numpy data, NOT a pickled sklearn object (the first deliberate deviation).
* ``dcsb`` (baseline.py:67-152): the confidence / object-count / minimum-area threshold rule on the
  weak detector's detection files, bit-exact.  Writes <save_dir>/estimate{k}.npz and, with
  --model_dir, wts{k}.pickle = (conf_thresh float, num_thresh int, area_thresh np.float64) as the
  reference does.  The reference's confidence bisection never ends when the detections cannot meet
  the label count; here it is bounded at 64 halvings and raises RuntimeError (the second deviation).

estimate{k}.npz holds train_est, val_est (int64), train_time, val_time, as test.py /
edgeml_amd.evaluate read them.  There is no CPU path.
"""
import argparse
import ctypes
import os
import pickle
import time
from pathlib import Path

import numpy as np
import torch

from . import ops
from .estimator import load_stage24, save_result
from .reward import load_data

MAX_NEWTON = 100
GRAD_TOL = 1e-8


def area_grid():
    """baseline.py:114: the area thresholds, exactly numpy's arange (not 0.2 + 0.01 i rounded otherwise)."""
    return np.arange(0.2, 0.9, 0.01)


def get_area(bbox_coord):
    """baseline.py:155-158: box areas from xyxy coordinates."""
    return (bbox_coord[:, 2] - bbox_coord[:, 0]) * (bbox_coord[:, 3] - bbox_coord[:, 1])


def dcsb_inputs(weak_data):
    """baseline.py:180: per image (conf, area), empty arrays for an image without detections."""
    return [(np.array([]), np.array([])) if len(wd) == 0 else (wd[2], get_area(wd[1])) for wd in weak_data]


def pack_dets(dets):
    """Flatten per-image (conf, area) into float64 conf [n], area [n] and offsets [N + 1] int64."""
    n = np.array([len(d[0]) for d in dets], np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    conf = np.concatenate([np.asarray(d[0], np.float64).reshape(-1) for d in dets] + [np.zeros(0)])
    area = np.concatenate([np.asarray(d[1], np.float64).reshape(-1) for d in dets] + [np.zeros(0)])
    assert len(conf) == len(area) == off[-1]
    return conf, area, off


def result_dir(save_dir, baseline, positive_weight):
    """baseline.py:198,203: af results live in a per-weight subdirectory ('3.0')."""
    return os.path.join(save_dir, f"{positive_weight}") if baseline == "af" else save_dir


def model_save_dir(directory, baseline, positive_weight):
    """baseline.py:174,183."""
    return os.path.join(directory, f"{positive_weight}") if baseline == "af" else directory


def model_path(directory, fold):
    return os.path.join(directory, f"wts{fold + 1}.pickle")


def _train_lists(split):
    tr = [np.nonzero(~m)[0].astype(np.int32) for m in split]
    off = np.concatenate([[0], np.cumsum([len(a) for a in tr])]).astype(np.int64)
    return tr, off


def _dev(a, device):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(device)


def fit_dcsb_folds(dets, label_num, reward01, split, device="cuda"):
    """fit_dcsb for every fold of `split` ((k, N) bool, True = validation) in one launch.

    dets[i] = (conf, area) of image i, label_num [N], reward01 [N] in {0, 1}.  Returns (results,
    models): per fold {train_est, val_est (int64), train_time, val_time} and the reference's model tuple
    (conf_thresh, num_thresh, area_thresh)."""
    ops.need_device("edgeml_amd.baseline")
    split = np.asarray(split, dtype=bool)
    k, N = split.shape
    assert len(dets) == N and len(label_num) == N and len(reward01) == N
    conf, area, off = pack_dets(dets)
    tr, tr_off = _train_lists(split)
    grid = area_grid()
    g_conf, g_area, g_off = _dev(conf, device), _dev(area, device), _dev(off, device)
    g_lab = _dev(np.asarray(label_num).astype(np.int64), device)
    g_rew = _dev(np.asarray(reward01).astype(np.int32), device)
    g_tr, g_tro, g_grid = _dev(np.concatenate(tr + [np.zeros(1, np.int32)]), device), _dev(tr_off, device), _dev(grid, device)
    ws_num = torch.empty((k, 2, N), dtype=torch.int32, device=device)
    ws_area = torch.empty((k, N), dtype=torch.float64, device=device)
    thresh = torch.zeros((k, 2), dtype=torch.float64, device=device)
    num = torch.zeros(k, dtype=torch.int32, device=device)
    est = torch.zeros((k, N), dtype=torch.int32, device=device)
    status = torch.zeros(k, dtype=torch.int32, device=device)
    steps = torch.zeros(k, dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.check(ops.lib().edgedet_dcsb_fit(ops._ptr(g_conf), ops._ptr(g_area), ops._ptr(g_off), N, ops._ptr(g_lab),
                                         ops._ptr(g_rew), ops._ptr(g_tr), ops._ptr(g_tro), k, ops._ptr(g_grid),
                                         len(grid), ops._ptr(ws_num), ops._ptr(ws_area), ops._ptr(thresh),
                                         ops._ptr(num), ops._ptr(est), ops._ptr(status), ops._ptr(steps),
                                         ops.stream_handle()))
    torch.cuda.synchronize()
    per_image = (time.perf_counter() - t0) / (k * N)  # fit and prediction are one launch
    status, thresh, num, est = status.cpu().numpy(), thresh.cpu().numpy(), num.cpu().numpy(), est.cpu().numpy()
    if np.any(status == 1):
        raise RuntimeError("DCSB confidence search did not converge")
    if np.any(status != 0):
        raise RuntimeError("DCSB grid search found no threshold pair with a positive training accuracy")
    results, models = [], []
    for f in range(k):
        e = est[f].astype(np.int64)
        results.append({"train_est": e[~split[f]], "val_est": e[split[f]], "train_time": per_image,
                        "val_time": per_image})
        models.append((float(thresh[f, 0]), int(num[f]), np.float64(thresh[f, 1])))
    return results, models


def pad_features(features):
    """[N, D] -> float64 [N, Dp]: the features, a column of ones (the bias), zero columns up to a
    multiple of 16 (the fp64 matrix instruction's tile)."""
    x = np.asarray(features, dtype=np.float64)
    x = x.reshape(len(x), -1)
    N, D = x.shape
    Dp = (D + 1 + 15) // 16 * 16
    xt = np.zeros((N, Dp))
    xt[:, :D] = x
    xt[:, D] = 1.0
    return xt, D


def fit_af_folds(features, reward01, split, positive_weight=3.0, device="cuda"):
    """fit_af for every fold of `split` at once.  Returns (results, models): per fold {train_est, val_est
    (int64), train_time, val_time} and {"coef" [D], "intercept", "classes", "positive_weight",
    "n_iter", "grad_norm"} (the last two: Newton steps taken and the final |grad f|)."""
    ops.need_device("edgeml_amd.baseline")
    split = np.asarray(split, dtype=bool)
    k, N = split.shape
    y = np.asarray(reward01).astype(np.int32)
    assert len(features) == N and len(y) == N
    for f in range(k):
        if len(np.unique(y[~split[f]])) < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but fold {f + 1}'s "
                             f"training set contains only one class")
    xt, D = pad_features(features)
    Dp = xt.shape[1]
    tr, tr_off = _train_lists(split)
    L = ops.lib()
    wb = int(L.edgedet_svm_workspace_size(k, Dp, int(tr_off[-1])))
    if wb < 0:
        raise ValueError(f"edgeml_amd.baseline: {D} features + bias exceed the solver's 256 columns")
    g_x, g_y = _dev(xt, device), _dev(y, device)
    g_tr, g_tro = _dev(np.concatenate(tr + [np.zeros(1, np.int32)]), device), _dev(tr_off, device)
    v = torch.zeros((k, Dp), dtype=torch.float64, device=device)
    ws = torch.empty(wb, dtype=torch.uint8, device=device)
    iters = torch.zeros(k, dtype=torch.int32, device=device)
    gnorm = torch.zeros(k, dtype=torch.float64, device=device)
    status = torch.zeros(k, dtype=torch.int32, device=device)
    tro_host = (ctypes.c_int64 * (k + 1))(*[int(o) for o in tr_off])
    ops.check(L.edgedet_svm_fit(ops._ptr(g_x), N, Dp, ops._ptr(g_y), float(positive_weight), ops._ptr(g_tr), tro_host,
                                ops._ptr(g_tro), k, ops._ptr(v), ops._ptr(ws), wb, MAX_NEWTON, GRAD_TOL,
                                ops._ptr(iters), ops._ptr(gnorm), ops._ptr(status), ops.stream_handle()))
    dec = torch.empty((k, N), dtype=torch.float64, device=device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.check(L.edgedet_svm_decision(ops._ptr(g_x), N, Dp, ops._ptr(v), k, ops._ptr(dec), ops.stream_handle()))
    torch.cuda.synchronize()
    per_image = (time.perf_counter() - t0) / (k * N)
    status, iters, gnorm = status.cpu().numpy(), iters.cpu().numpy(), gnorm.cpu().numpy()
    if np.any(status != 0):
        why = {1: "did not converge", 2: "line search failed", 3: "Hessian not positive definite"}
        bad = [f"fold {f + 1}: {why.get(int(s), s)} (|grad| {gnorm[f]:.3e} after {iters[f]} steps)"
               for f, s in enumerate(status) if s != 0]
        raise RuntimeError("Adaptive Feeding SVM solver: " + "; ".join(bad))
    v, dec = v.cpu().numpy(), dec.cpu().numpy()
    results, models = [], []
    for f in range(k):
        e = (dec[f] > 0).astype(np.int64)
        results.append({"train_est": e[~split[f]], "val_est": e[split[f]], "train_time": per_image,
                        "val_time": per_image})
        models.append({"coef": v[f, :D].copy(), "intercept": float(v[f, D]), "classes": [0, 1],
                       "positive_weight": float(positive_weight), "n_iter": int(iters[f]),
                       "grad_norm": float(gnorm[f])})
    return results, models


def _save_model(directory, fold, model):
    Path(directory).mkdir(parents=True, exist_ok=True)
    with open(model_path(directory, fold), "wb") as f:
        pickle.dump(model, f)


def main(opts):
    """baseline.py:161-204."""
    ops.need_device("edgeml_amd.baseline")
    with np.load(opts.reward_path, allow_pickle=False) as z:
        reward = np.where(z["reward"] > 0, 1, 0)
    split = np.load(opts.split_path, allow_pickle=False)
    assert len(reward) == split.shape[1], "Inconsistent number of data points from the dataset and the split."
    out_dir = result_dir(opts.save_dir, opts.baseline, opts.positive_weight)
    mdir = model_save_dir(opts.model_dir, opts.baseline, opts.positive_weight) if opts.model_dir != "" else ""
    if opts.baseline == "af":
        features = load_stage24(opts.data_dir)
        assert len(features) == len(reward), "Inconsistent number of feature maps and offloading rewards."
        results, models = fit_af_folds(features, reward, split, opts.positive_weight)
        models = [{k: m[k] for k in ("coef", "intercept", "classes", "positive_weight")} for m in models]
        name = "Adaptive Feeding SVM"
    else:
        img_names = [".".join(name.split(".")[:-1]) for name in sorted(os.listdir(opts.label_dir))]
        dets = dcsb_inputs(load_data(opts.data_dir, img_names, True))
        labels = load_data(opts.label_dir, img_names)
        label_num = np.array([0 if len(l) == 0 else len(l[0]) for l in labels], dtype=int)
        assert len(dets) == len(reward), "Inconsistent number of feature maps and offloading rewards."
        results, models = fit_dcsb_folds(dets, label_num, reward, split)
        name = "DCSB thresholds"
    for cv_idx, val_mask in enumerate(split):
        r = results[cv_idx]
        tr_acc = np.sum(reward[~val_mask] == r["train_est"]) / max(len(r["train_est"]), 1)
        va_acc = np.sum(reward[val_mask] == r["val_est"]) / max(len(r["val_est"]), 1)
        print(f"fold {cv_idx + 1}: {name} with training accuracy: {tr_acc:.3f}, validation accuracy: {va_acc:.3f}")
        save_result(out_dir, r, cv_idx)
        if mdir != "":
            _save_model(mdir, cv_idx, models[cv_idx])
    return results, models


def getargs(argv=None):
    """baseline.py:207-226."""
    args = argparse.ArgumentParser()
    args.add_argument('data_dir',
                      help="Directory that saves the data needed for predicting the offloading reward. "
                           "For Adaptive Feeding, the stage-24 features of the weak detector's outputs; "
                           "for DCSB, the weak detector's detection files.")
    args.add_argument('reward_path', help="Path to the (pre-computed) offloading reward.")
    args.add_argument('split_path', help="Path to the dataset split (for cross validation).")
    args.add_argument('save_dir', help="Directory to save the estimated offloading reward.")
    args.add_argument('--baseline', type=str, default="af", choices=['af', 'dcsb'],
                      help="'af' (Adaptive Feeding) or 'dcsb' (difficult-case based small-big model).")
    args.add_argument('--positive_weight', type=float, default=3.0,
                      help="The weight for the positive reward class. Only active when baseline is 'af'.")
    args.add_argument('--label_dir', type=str, default='',
                      help="Directory of the ground truth annotations. Only active when baseline is 'dcsb'.")
    args.add_argument('--model_dir', type=str, default='', help="Directory to save the model weights.")
    return args.parse_args(argv)


if __name__ == '__main__':
    main(getargs())
