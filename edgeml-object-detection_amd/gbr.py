"""regression.py's GradientBoostingRegressor on the GPU (csrc/gbr.hip), every cross-validation fold in flight,
exact to the tree.

It follows fit_model (regression.py:38-77) on the flattened stage-24 features: StandardScaler fitted on the
fold's training rows (edgeml_amd.regress's), rounded to float32 as sklearn's trees see it, then
GradientBoostingRegressor(learning_rate=0.1, n_estimators=1000, subsample=1.0) at sklearn's max_depth=3 and
criterion friedman_mse.  At those options sklearn's fit is deterministic except for the order in which its
splitter visits the features, which decides among equally good splits.  Here the residual sums are exact
integers (rq = rint(r 2^q)), so equally good splits have bit-equal gains on any hardware, and one rule decides
among them: the lowest feature index, then the lowest threshold.  That rule is the one documented deviation.

    results, info = fit_gbr(features, rewards, split)      # also GBROpt(learning_rate, n_estimators, subsample, max_depth)

features, rewards, split and results are edgeml_amd.regress's.  info: feature int16 [k, T, 2^depth - 1] (-1: a
leaf), threshold [k, T, 2^depth - 1], value [k, T, 2^(depth+1) - 1] (heap layout: the children of node i are
2 i + 1 and 2 i + 2, a row goes right when float64(z32) > threshold), init [k], q [k], mean, scale [k, D],
nodes [k, T] (split nodes per stage), tied_nodes [k] (split nodes at which a second feature attained the
maximal gain: how much of val_est the tie rule decided), fit_time.  There is no CPU path.

    python -m edgeml_amd.gbr data_dir reward_path split_path save_dir --model GBR [--normalize]
                             [--model-dir DIR] [--n-estimators 1000] [--learning-rate 0.1] [--max-depth 3]

takes regression.py's arguments, prints fit_model's MSE line per fold, writes estimate<k>.npz into save_dir and,
with --model-dir, wts<k>.pickle holding plain numpy data: {model: "GBR", mean, scale, init, learning_rate,
max_depth, feature, threshold, value, q}, which GBRModel predicts from (edgedet_gbr_model_predict) and the
offloading cascade loads as kind "gbr".
"""
import ctypes
import math
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import estimator, ops
from ._saved import DeviceModel, open_model, scaler
from .regress import _Folds

NAMES = {"GBR": "Gradient Boosting Regressor"}
MAX_DEPTH = 4
Q_MIN, Q_MAX = 26, 1000
KEYS = ("mean", "scale", "init", "learning_rate", "max_depth", "feature", "threshold", "value")


@dataclass
class GBROpt:
    """regression.py:188-192, and sklearn's default depth."""
    learning_rate: float = 0.1
    n_estimators: int = 1000
    subsample: float = 1.0
    max_depth: int = 3


_GBROPT = GBROpt()


def check_opts(opts):
    if opts.subsample != 1.0:
        raise ValueError(f"edgeml_amd.gbr: subsample = {opts.subsample} draws the rows of every stage at random, and "
                         f"that is not built; only subsample = 1.0 is")
    if not 1 <= int(opts.max_depth) <= MAX_DEPTH or int(opts.max_depth) != opts.max_depth:
        raise ValueError(f"edgeml_amd.gbr: max_depth = {opts.max_depth}; the tree builder takes 1 to {MAX_DEPTH}")
    if int(opts.n_estimators) < 1:
        raise ValueError(f"edgeml_amd.gbr: n_estimators = {opts.n_estimators}; at least 1")
    if not (math.isfinite(opts.learning_rate) and opts.learning_rate > 0.0):
        raise ValueError(f"edgeml_amd.gbr: learning_rate = {opts.learning_rate}; a positive number")


def init_and_q(y_tr):
    """F0 = the exactly rounded sum of the training targets / n, and the residual scale q = 62 - ceil(log2 n) - e
    with 2^e > 2 max|y - F0| (the least such e; 0 for constant targets)."""
    n = len(y_tr)
    init = math.fsum(y_tr.tolist()) / n
    e = math.frexp(2.0 * float(np.max(np.abs(y_tr - init))))[1]
    return init, 62 - max(0, (n - 1).bit_length()) - e


def fit_gbr(features, rewards, split, opts=None, device="cuda"):
    """GradientBoostingRegressor(learning_rate, n_estimators, subsample=1.0, max_depth): T stages enqueued at once,
    one scan and one select launch per tree level and one update launch per stage; the status words are read once
    at the end."""
    opts = opts or _GBROPT
    check_opts(opts)
    ops.need_device("edgeml_amd.gbr")
    fo = _Folds(features, rewards, split, device)
    k, N, D, T, depth = fo.k, fo.N, fo.D, int(opts.n_estimators), int(opts.max_depth)
    if not np.all(np.isfinite(fo.x)) or not np.all(np.isfinite(fo.y)):
        raise ValueError("edgeml_amd.gbr: features and targets must be finite")
    init, q = np.empty(k, np.float64), np.empty(k, np.int32)
    for f in range(k):
        init[f], q[f] = init_and_q(fo.y[f][fo.tr[f]])
        if not Q_MIN <= q[f] <= Q_MAX:
            raise ValueError(f"edgeml_amd.gbr: fold {f + 1}: the residual scale q = {q[f]} is outside {Q_MIN}..{Q_MAX} "
                             f"(targets of a magnitude the fixed-point residual sums cannot carry)")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fo.upload()
    L, p = ops.lib(), ops._ptr
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    z32 = torch.empty((k, N, D), dtype=torch.float32, device=device)
    ops.check(L.edgedet_gbr_prepare(p(fo.g_x), N, D, p(fo.mean), p(fo.scale), k, p(z32), ops.stream_handle()))
    # per (fold, feature) the training positions in value order, ties by position: a stable sort, once per fit
    pos = torch.full((k, N), -1, dtype=torch.int32, device=device)
    order, values = [], []
    for f in range(k):
        rows = fo.g_tr[int(fo.tr_off[f]):int(fo.tr_off[f + 1])].long()
        pos[f, rows] = torch.arange(len(rows), dtype=torch.int32, device=device)
        v, i = torch.sort(z32[f].index_select(0, rows), dim=0, stable=True)
        order.append(i.t().contiguous().to(torch.int32).reshape(-1))
        values.append(v.t().contiguous().reshape(-1))
    order, values = torch.cat(order), torch.cat(values)
    wb = int(L.edgedet_gbr_workspace_size(fo.tro_host, k, D))
    if wb < 0:
        raise ValueError("edgeml_amd.gbr: bad fold sizes")
    ws = torch.empty(wb // 8, dtype=torch.float64, device=device)
    ni, nv = (1 << depth) - 1, (2 << depth) - 1
    feature = torch.empty((k, T, ni), dtype=torch.int16, device=device)
    threshold = torch.empty((k, T, ni), dtype=torch.float64, device=device)
    value = torch.empty((k, T, nv), dtype=torch.float64, device=device)
    est = torch.empty((k, N), dtype=torch.float64, device=device)
    nodes = torch.empty((k, T), dtype=torch.int32, device=device)
    tied = torch.empty(k, dtype=torch.int32, device=device)
    status = torch.empty(k, dtype=torch.int32, device=device)
    g_init, g_q = t(init), t(q)
    q_host = (ctypes.c_int32 * k)(*[int(v) for v in q])
    ops.check(L.edgedet_gbr_fit(p(z32), N, D, p(fo.g_y), p(fo.g_tr), p(pos), p(order), p(values), fo.tro_host,
                                p(fo.g_tro), k, p(g_init), q_host, p(g_q), float(opts.learning_rate), T, depth, p(ws),
                                wb, p(feature), p(threshold), p(value), p(est), p(nodes), p(tied), p(status),
                                ops.stream_handle()))
    st = status.cpu().numpy()  # waits for the stream: the only read-back of the fit's state
    if np.any(st != 0):
        bad = [f"fold {f + 1}: stage {int(st[f])}" for f in np.nonzero(st)[0]]
        raise RuntimeError("edgeml_amd.gbr: a residual reached 2^(62 - ceil(log2 n)) quanta, the exact sums would "
                           "overflow: " + "; ".join(bad))
    est_host = est.cpu().numpy()
    t_fit = time.perf_counter() - t0
    info = {"feature": feature.cpu().numpy(), "threshold": threshold.cpu().numpy(), "value": value.cpu().numpy(),
            "init": init, "q": q, "mean": fo.mean.cpu().numpy(), "scale": fo.scale.cpu().numpy(),
            "nodes": nodes.cpu().numpy(), "tied_nodes": tied.cpu().numpy(), "fit_time": t_fit,
            "learning_rate": float(opts.learning_rate), "max_depth": depth}
    return fo.results(est_host, t_fit / (k * N)), info


FITS = {"GBR": fit_gbr}


# ------------------------------------------------------------------------------------------- saved model
class GBRModel(DeviceModel):
    """One fold's trees with its StandardScaler: mean, scale [width], feature int16 [T, 2^depth - 1], threshold
    [T, 2^depth - 1], value [T, 2^(depth+1) - 1], init, learning_rate, max_depth."""
    kind, module = "gbr", "edgeml_amd.gbr"

    def __init__(self, mean, scale, feature, threshold, value, init, learning_rate, max_depth):
        self.width, self.T, self.depth = len(mean), len(feature), int(max_depth)
        self.mean, self.scale, self.feature, self.threshold, self.value = mean, scale, feature, threshold, value
        self.init, self.learning_rate = float(init), float(learning_rate)

    def _upload(self, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return {"mean": t(self.mean), "scale": t(self.scale), "feature": t(self.feature),
                "threshold": t(self.threshold), "value": t(self.value)}

    def workspace_bytes(self, B):
        return 0  # edgedet_gbr_model_predict needs none

    def predict_into(self, feat, est, ws=None, nbr=None, stream=None):
        """One library call: feat [B, width] float64 and est [B] float64 on the model's device.  ws and nbr are
        KernelModel.predict_into's, unused here: the cascade calls the three model-backed kinds alike."""
        d = self._device_rows(feat, est)
        B, p = int(feat.shape[0]), ops._ptr
        ops.check(ops.lib().edgedet_gbr_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]),
                                                      p(d["feature"]), p(d["threshold"]), p(d["value"]), self.init,
                                                      self.learning_rate, self.T, self.depth, p(est),
                                                      ops.stream_handle(stream)))

    def predict(self, features):
        """Estimates float64 [N] of features [N, ...] (flattened to [N, width])."""
        dev, x = self._host_rows(features)
        if len(x) == 0:
            return np.empty(0, np.float64)
        with torch.cuda.device(dev):
            est = torch.empty(len(x), dtype=torch.float64, device=dev)
            self.predict_into(torch.from_numpy(x).to(dev), est)
            return est.cpu().numpy()


def load(path_or_dict):
    """The GBRModel of a GBR wts<fold>.pickle (a path, or the dict itself); ValueError on anything else, on
    missing keys, on tree arrays of inconsistent shape and on values that are not finite."""
    m, what = open_model(path_or_dict)
    if not isinstance(m, dict) or m.get("model") != "GBR":
        raise ValueError(f"{what}: not a wts<fold>.pickle of edgeml_amd.gbr --model-dir")
    missing = [key for key in KEYS if key not in m]
    if missing:
        raise ValueError(f"{what}: a GBR file without {', '.join(repr(key) for key in missing)}")
    mean, scale = scaler(what, m)
    D = len(mean)
    depth, lr, init = int(m["max_depth"]), float(m["learning_rate"]), float(m["init"])
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"{what}: max_depth = {depth}; 1 to {MAX_DEPTH}")
    feature = np.ascontiguousarray(np.asarray(m["feature"]))
    threshold = np.ascontiguousarray(np.asarray(m["threshold"], np.float64))
    value = np.ascontiguousarray(np.asarray(m["value"], np.float64))
    ni, nv = (1 << depth) - 1, (2 << depth) - 1
    T = len(feature) if feature.ndim == 2 else 0
    if T < 1 or feature.shape != (T, ni) or threshold.shape != (T, ni) or value.shape != (T, nv):
        raise ValueError(f"{what}: tree arrays of shapes {feature.shape}, {threshold.shape}, {value.shape}; expected "
                         f"[T][{ni}], [T][{ni}] and [T][{nv}] at max_depth {depth}")
    if not np.issubdtype(feature.dtype, np.integer) or feature.min() < -1 or feature.max() >= D:
        raise ValueError(f"{what}: 'feature' must hold integers from -1 to {D - 1}")
    if not (np.all(np.isfinite(threshold)) and np.all(np.isfinite(value)) and math.isfinite(init)
            and math.isfinite(lr)):
        raise ValueError(f"{what}: thresholds, values, init and learning_rate must be finite")
    return GBRModel(mean, scale, feature.astype(np.int16), threshold, value, init, lr, depth)


def model_data(info, fold):
    """What wts{k}.pickle holds for one fold: plain numpy data, not sklearn objects."""
    return {"model": "GBR", "mean": info["mean"][fold].copy(), "scale": info["scale"][fold].copy(),
            "init": float(info["init"][fold]), "learning_rate": float(info["learning_rate"]),
            "max_depth": int(info["max_depth"]), "feature": info["feature"][fold].copy(),
            "threshold": info["threshold"][fold].copy(), "value": info["value"][fold].copy(), "q": int(info["q"][fold])}


# --------------------------------------------------------------------------------------------------- CLI
def main(opts):
    if opts.model not in FITS:
        raise SystemExit(f"edgeml_amd.gbr builds --model GBR (Gradient Boosting Regressor); --model {opts.model} "
                         f"belongs to edgeml_amd.estimator, edgeml_amd.svr or edgeml_amd.rfr, and SGD is not built "
                         f"(DESIGN.md §7)")
    if opts.stage != 24:
        raise SystemExit("edgeml_amd.gbr runs on the stage-24 output features (--stage 24); the hidden-layer "
                         "feature maps of stages 0-23 train a conv net: python -m edgeml_amd.convnet")
    fit_opts = GBROpt(learning_rate=opts.learning_rate, n_estimators=opts.n_estimators, max_depth=opts.max_depth)
    try:
        check_opts(fit_opts)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    features, reward, split = estimator.load_inputs(opts)
    y = estimator.fold_targets(reward, split, opts.normalize, np.float64)
    results, info = fit_gbr(features, y, split, fit_opts)
    estimator.report_folds(opts, NAMES[opts.model], y, split, results, lambda fold: model_data(info, fold))
    return results, info


def getargs(argv=None):
    a = estimator.base_parser("GBR", prog="python -m edgeml_amd.gbr")
    a.add_argument("--n-estimators", type=int, default=_GBROPT.n_estimators)
    a.add_argument("--learning-rate", type=float, default=_GBROPT.learning_rate)
    a.add_argument("--max-depth", type=int, default=_GBROPT.max_depth)
    return a.parse_args(argv)


if __name__ == "__main__":
    main(getargs())
