"""regression.py's RandomForestRegressor on the GPU (csrc/rfr.hip), every tree of every cross-validation fold in
flight, exact tree by tree.

It follows fit_model (regression.py:38-77) on the flattened stage-24 features: StandardScaler fitted on the
fold's training rows (edgeml_amd.regress's), rounded to float32 as sklearn's trees see it, then
RandomForestRegressor(n_estimators=100, max_depth=20, min_samples_split=100) at sklearn's defaults: bootstrap
on, every feature tried at every node, criterion squared_error.  What sklearn draws at random is reproduced on
the host with numpy alone: one seed per tree from the global stream (randint(2^31 - 1, size=n_estimators), once
per fit, in fold order), and per tree the bootstrap RandomState(seed_t).randint(0, n, n), which reaches the tree
as the integer row weights bincount(indices).  --seed s therefore means the forests regression.py fits after
np.random.seed(s).  The tree's own generator only decides among equally good splits.  Here the targets are
carried as integers (yq = rint((y - F0) 2^q)), so equally good splits have bit-equal gains on any hardware, and
one rule decides among them: the lowest feature index, then the lowest threshold.  That rule is the one
documented deviation; tied_nodes counts the split nodes it decided.

    results, info = fit_rfr(features, rewards, split, seed=0)   # also RFROpt(n_estimators, max_depth, min_samples_split)

features, rewards, split and results are edgeml_amd.regress's.  info: per fold the padded tree arrays [T, cap],
cap = min(2^(max_depth+1) - 1, 2 n - 1): feature int16 (-1: a leaf), threshold float64, left int32 (the right
child is left + 1; nodes are numbered breadth first; a row goes right when float64(z32) > threshold), value
float64, n_node_samples int32 (in-bag rows), and node_count [T]; init [k], q [k], mean, scale [k, D], tied_nodes
[k], fit_time.  The estimate of a row is the sum of its leaf values in tree order in float64, divided by T.
There is no CPU path.

    python -m edgeml_amd.rfr data_dir reward_path split_path save_dir --model RFR [--normalize] [--model-dir DIR]
                             [--n-estimators 100] [--max-depth 20] [--min-samples-split 100] [--seed 0]

takes regression.py's arguments, prints fit_model's MSE line per fold, writes estimate<k>.npz into save_dir and,
with --model-dir, wts<k>.pickle holding plain numpy data: {model: "RFR", mean, scale, init, q, feature,
threshold, left, value, n_node_samples, node_count}, which RFRModel predicts from (edgedet_rfr_model_predict,
the fit's bits) and the offloading cascade loads as kind "rfr".
"""
import ctypes
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import estimator, ops
from ._saved import DeviceModel, open_model, scaler
from .gbr import Q_MAX, Q_MIN, init_and_q
from .regress import _Folds

NAMES = {"RFR": "Random Forest Regressor"}
MAX_DEPTH = 64
ARRAYS = ("feature", "threshold", "left", "value", "n_node_samples")
KEYS = ("mean", "scale", "init", *ARRAYS, "node_count")


@dataclass
class RFROpt:
    """regression.py:169-174."""
    n_estimators: int = 100
    max_depth: int = 20
    min_samples_split: int = 100


_RFROPT = RFROpt()


def check_opts(opts):
    if int(opts.max_depth) != opts.max_depth or not 1 <= int(opts.max_depth) <= MAX_DEPTH:
        raise ValueError(f"edgeml_amd.rfr: max_depth = {opts.max_depth}; the tree builder takes 1 to {MAX_DEPTH}")
    if int(opts.min_samples_split) != opts.min_samples_split or int(opts.min_samples_split) < 2:
        raise ValueError(f"edgeml_amd.rfr: min_samples_split = {opts.min_samples_split}; an integer, at least 2")
    if int(opts.n_estimators) < 1:
        raise ValueError(f"edgeml_amd.rfr: n_estimators = {opts.n_estimators}; at least 1")


def bootstrap_counts(seed, k, T, n_per_fold):
    """The bootstraps regression.py's forests draw after np.random.seed(seed): per fold, in fold order, one seed
    per tree from the global stream, then per tree the counts of n row indices drawn with replacement.  A list of
    k arrays uint8 [T, n_f].  numpy's RandomState stream is frozen by its compatibility policy."""
    rs = np.random.RandomState(seed)
    out = []
    for f in range(k):
        n = int(n_per_fold[f])
        seeds = rs.randint(np.iinfo(np.int32).max, size=int(T))
        c = np.stack([np.bincount(np.random.RandomState(s).randint(0, n, n), minlength=n) for s in seeds])
        if c.max() > 255:
            raise ValueError(f"edgeml_amd.rfr: a row was drawn {c.max()} times; the weights are stored in 8 bits")
        out.append(c.astype(np.uint8))
    return out


def node_cap(max_depth, n):
    return min((1 << (int(max_depth) + 1)) - 1, 2 * int(n) - 1)


def scan_groups(trees, D):
    """How many workgroups share the features of one tree in the scan: enough to fill the device when the trees
    alone do not.  The result of a fit does not depend on it."""
    return int(max(1, min(16, D, -(-2048 // trees))))


def fit_rfr(features, rewards, split, opts=None, seed=0, device="cuda", groups=None, counts=None):
    """RandomForestRegressor(n_estimators, max_depth, min_samples_split): the bootstraps drawn on the host, every
    level of every tree enqueued at once (one scan and one select launch per level); the status words are read once
    at the end.  counts (a list of k arrays [T, n_f]) replaces bootstrap_counts(seed, ...): the row weights of
    every tree, given."""
    opts = opts or _RFROPT
    check_opts(opts)
    ops.need_device("edgeml_amd.rfr")
    fo = _Folds(features, rewards, split, device)
    k, N, D = fo.k, fo.N, fo.D
    T, depth, mss = int(opts.n_estimators), int(opts.max_depth), int(opts.min_samples_split)
    if not np.all(np.isfinite(fo.x)) or not np.all(np.isfinite(fo.y)):
        raise ValueError("edgeml_amd.rfr: features and targets must be finite")
    n_fold = [len(a) for a in fo.tr]
    init, q, yq = np.empty(k, np.float64), np.empty(k, np.int32), []
    for f in range(k):
        y_tr = fo.y[f][fo.tr[f]]
        init[f], q[f] = init_and_q(y_tr)
        if not Q_MIN <= q[f] <= Q_MAX:
            raise ValueError(f"edgeml_amd.rfr: fold {f + 1}: the target scale q = {q[f]} is outside {Q_MIN}..{Q_MAX} "
                             f"(targets of a magnitude the fixed-point sums cannot carry)")
        # |yq| < 2^(61 - ceil(log2 n)) by the choice of q and the weights of a tree add up to n: every weighted
        # sum fits int64.  Checked once: there are no stages that could change it.
        v = np.rint(np.ldexp(y_tr - init[f], int(q[f])))
        if not np.all(np.abs(v) < float(1 << (62 - max(0, (n_fold[f] - 1).bit_length())))):
            raise ValueError(f"edgeml_amd.rfr: fold {f + 1}: a target reaches 2^(62 - ceil(log2 n)) quanta")
        yq.append(v.astype(np.int64))
    if counts is None:
        counts = bootstrap_counts(seed, k, T, n_fold)
    counts = [np.ascontiguousarray(c, dtype=np.uint8) for c in counts]
    if len(counts) != k or any(c.shape != (T, n) for c, n in zip(counts, n_fold)):
        raise ValueError("edgeml_amd.rfr: counts must hold one array [n_estimators, training rows] per fold")
    groups = scan_groups(k * T, D) if groups is None else int(groups)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fo.upload()
    L, p = ops.lib(), ops._ptr
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    z32 = torch.empty((k, N, D), dtype=torch.float32, device=device)
    ops.check(L.edgedet_gbr_prepare(p(fo.g_x), N, D, p(fo.mean), p(fo.scale), k, p(z32), ops.stream_handle()))
    # per (fold, feature) the training positions in value order, ties by position: a stable sort, once per fit,
    # shared by all trees of the fold
    order, values = [], []
    for f in range(k):
        rows = fo.g_tr[int(fo.tr_off[f]):int(fo.tr_off[f + 1])].long()
        v, i = torch.sort(z32[f].index_select(0, rows), dim=0, stable=True)
        order.append(i.t().contiguous().to(torch.int32).reshape(-1))
        values.append(v.t().contiguous().reshape(-1))
    order, values = torch.cat(order), torch.cat(values)
    g_w, g_yq = t(np.concatenate([c.reshape(-1) for c in counts])), t(np.concatenate(yq))
    cap = int(L.edgedet_rfr_node_cap(max(n_fold), depth))
    wb = int(L.edgedet_rfr_workspace_size(fo.tro_host, k, D, T, depth, mss, groups))
    if wb < 0 or cap < 0:
        raise ValueError("edgeml_amd.rfr: bad fold sizes")
    ws = torch.empty(wb // 8, dtype=torch.float64, device=device)
    dev = {"feature": torch.empty((k, T, cap), dtype=torch.int16, device=device),
           "threshold": torch.empty((k, T, cap), dtype=torch.float64, device=device),
           "left": torch.empty((k, T, cap), dtype=torch.int32, device=device),
           "value": torch.empty((k, T, cap), dtype=torch.float64, device=device),
           "n_node_samples": torch.empty((k, T, cap), dtype=torch.int32, device=device)}
    node_count = torch.empty((k, T), dtype=torch.int32, device=device)
    tied = torch.empty(k, dtype=torch.int32, device=device)
    status = torch.empty(k, dtype=torch.int32, device=device)
    est = torch.empty((k, N), dtype=torch.float64, device=device)
    g_init, g_q = t(init), t(q)
    q_host = (ctypes.c_int32 * k)(*[int(v) for v in q])
    ops.check(L.edgedet_rfr_fit(p(z32), N, D, p(fo.g_x), p(fo.mean), p(fo.scale), p(fo.g_tr), p(order), p(values),
                                fo.tro_host, p(fo.g_tro), k, p(g_init), q_host, p(g_q), p(g_w), p(g_yq), T, depth, mss,
                                groups, p(ws), wb, *[p(dev[key]) for key in ARRAYS], p(node_count), p(tied), p(status),
                                p(est), ops.stream_handle()))
    st = status.cpu().numpy()  # waits for the stream: the only read-back of the fit's state
    if np.any(st != 0):
        raise RuntimeError(f"edgeml_amd.rfr: a tree outgrew its arrays (status {st.tolist()}): an internal error")
    est_host = est.cpu().numpy()
    t_fit = time.perf_counter() - t0
    info = {key: [v[f, :, :node_cap(depth, n_fold[f])].cpu().numpy().copy() for f in range(k)] for key, v in dev.items()}
    info.update({"node_count": node_count.cpu().numpy(), "init": init, "q": q, "mean": fo.mean.cpu().numpy(),
                 "scale": fo.scale.cpu().numpy(), "tied_nodes": tied.cpu().numpy(), "fit_time": t_fit,
                 "max_depth": depth, "min_samples_split": mss, "seed": seed, "groups": groups})
    return fo.results(est_host, t_fit / (k * N)), info


FITS = {"RFR": fit_rfr}


# ------------------------------------------------------------------------------------------- saved model
class RFRModel(DeviceModel):
    """One fold's forest with its StandardScaler: mean, scale [width], feature int16, threshold, left int32,
    value, n_node_samples int32 [T, cap], node_count [T], init."""
    kind, module = "rfr", "edgeml_amd.rfr"

    def __init__(self, mean, scale, feature, threshold, left, value, n_node_samples, node_count, init):
        self.width, (self.T, self.cap) = len(mean), feature.shape
        self.mean, self.scale, self.feature, self.threshold, self.left = mean, scale, feature, threshold, left
        self.value, self.n_node_samples, self.node_count, self.init = value, n_node_samples, node_count, float(init)

    def _upload(self, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return {"mean": t(self.mean), "scale": t(self.scale), "feature": t(self.feature),
                "threshold": t(self.threshold), "left": t(self.left), "value": t(self.value)}

    def workspace_bytes(self, B):
        return 0  # edgedet_rfr_model_predict needs none

    def predict_into(self, feat, est, ws=None, nbr=None, stream=None):
        """One library call: feat [B, width] float64 and est [B] float64 on the model's device.  ws and nbr are
        KernelModel.predict_into's, unused here: the cascade calls the model-backed kinds alike."""
        d = self._device_rows(feat, est)
        B, p = int(feat.shape[0]), ops._ptr
        ops.check(ops.lib().edgedet_rfr_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]),
                                                      p(d["feature"]), p(d["threshold"]), p(d["left"]), p(d["value"]),
                                                      self.T, self.cap, p(est), ops.stream_handle(stream)))

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
    """The RFRModel of an RFR wts<fold>.pickle (a path, or the dict itself); ValueError on anything else, on
    missing keys, on tree arrays of inconsistent shape, on a child id out of range and on values that are not
    finite."""
    m, what = open_model(path_or_dict)
    if not isinstance(m, dict) or m.get("model") != "RFR":
        raise ValueError(f"{what}: not a wts<fold>.pickle of edgeml_amd.rfr --model-dir")
    missing = [key for key in KEYS if key not in m]
    if missing:
        raise ValueError(f"{what}: an RFR file without {', '.join(repr(key) for key in missing)}")
    mean, scale = scaler(what, m)
    D = len(mean)
    feature = np.ascontiguousarray(np.asarray(m["feature"]))
    threshold = np.ascontiguousarray(np.asarray(m["threshold"], np.float64))
    value = np.ascontiguousarray(np.asarray(m["value"], np.float64))
    left, nsamp, count = (np.ascontiguousarray(np.asarray(m[key])) for key in ("left", "n_node_samples", "node_count"))
    shape = feature.shape
    if feature.ndim != 2 or shape[0] < 1 or shape[1] < 1 or count.shape != shape[:1] or any(
            a.shape != shape for a in (threshold, left, value, nsamp)):
        raise ValueError(f"{what}: tree arrays of shapes {feature.shape}, {threshold.shape}, {left.shape}, "
                         f"{value.shape}, {nsamp.shape} and node_count {count.shape}; expected five of [T][cap] and [T]")
    if not all(np.issubdtype(a.dtype, np.integer) for a in (feature, left, nsamp, count)):
        raise ValueError(f"{what}: 'feature', 'left', 'n_node_samples' and 'node_count' must hold integers")
    if feature.min() < -1 or feature.max() >= D:
        raise ValueError(f"{what}: 'feature' must hold integers from -1 to {D - 1}")
    if count.min() < 1 or count.max() > shape[1]:
        raise ValueError(f"{what}: 'node_count' must hold integers from 1 to {shape[1]}")
    ids = np.arange(shape[1])[None, :]
    inner = feature >= 0
    if np.any(inner & (ids >= count[:, None])) or np.any(inner & ((left <= ids) | (left + 1 >= count[:, None]))):
        raise ValueError(f"{what}: 'left' out of range: a split node's children lie after it and inside node_count")
    if not (np.all(np.isfinite(threshold)) and np.all(np.isfinite(value)) and np.isfinite(float(m["init"]))):
        raise ValueError(f"{what}: thresholds, values and init must be finite")
    return RFRModel(mean, scale, feature.astype(np.int16), threshold, left.astype(np.int32), value,
                    nsamp.astype(np.int32), count.astype(np.int32), m["init"])


def model_data(info, fold):
    """What wts{k}.pickle holds for one fold: plain numpy data, not sklearn objects."""
    return {"model": "RFR", "mean": info["mean"][fold].copy(), "scale": info["scale"][fold].copy(),
            "init": float(info["init"][fold]), "q": int(info["q"][fold]),
            **{key: info[key][fold].copy() for key in ARRAYS}, "node_count": info["node_count"][fold].copy()}


# --------------------------------------------------------------------------------------------------- CLI
def main(opts):
    if opts.model not in FITS:
        raise SystemExit(f"edgeml_amd.rfr builds --model RFR (Random Forest Regressor); --model {opts.model} belongs "
                         f"to edgeml_amd.estimator, edgeml_amd.svr or edgeml_amd.gbr, and SGD is not built "
                         f"(DESIGN.md §7)")
    if opts.stage != 24:
        raise SystemExit("edgeml_amd.rfr runs on the stage-24 output features (--stage 24); the hidden-layer "
                         "feature maps of stages 0-23 train a conv net: python -m edgeml_amd.convnet")
    fit_opts = RFROpt(n_estimators=opts.n_estimators, max_depth=opts.max_depth,
                      min_samples_split=opts.min_samples_split)
    try:
        check_opts(fit_opts)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    features, reward, split = estimator.load_inputs(opts)
    y = estimator.fold_targets(reward, split, opts.normalize, np.float64)
    results, info = fit_rfr(features, y, split, fit_opts, seed=opts.seed)
    estimator.report_folds(opts, NAMES[opts.model], y, split, results, lambda fold: model_data(info, fold))
    return results, info


def getargs(argv=None):
    a = estimator.base_parser("RFR", prog="python -m edgeml_amd.rfr")
    a.add_argument("--n-estimators", type=int, default=_RFROPT.n_estimators)
    a.add_argument("--max-depth", type=int, default=_RFROPT.max_depth)
    a.add_argument("--min-samples-split", type=int, default=_RFROPT.min_samples_split)
    a.add_argument("--seed", type=int, default=0, help="the forests regression.py fits after np.random.seed(SEED)")
    return a.parse_args(argv)


if __name__ == "__main__":
    main(getargs())
